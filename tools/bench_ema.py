#!/usr/bin/env python3
"""The exponential moving average (mavg_ema_run) against the boxcar it sits beside.

One process, the hooks library, a warm-up of every path, alternating order, device-event timing
(the style of tools/bench_extrema.py).  Per dtype (fp32 / int16, mono / stereo) on 2^log2n samples:

  (a) mavg_ema_run by the rule at the alpha whose halo H * C * sample size is 256 B, 2 KiB, 8 KiB
      and 16 KiB (ema_tile), and at alpha = 1e-3, 1e-4 and 1e-6 (ema_chain);
  (b) the yardstick: mavg_run at k = 1024 on the same input -- for fp32 it moves the same
      algorithmic bytes as ema_tile.

--pairs: ema_tile and ema_chain forced (mavg_debug_force_ema) on the four halo shapes, and
ema_chain and ema_strip forced at alpha = 1e-3: the pairs the tile rule is read from.  The strip is
slow: use --log2n 27 there.

The chain's step B alone (the one-workgroup carry kernel): run the tool with --pairs --alphas 1e-3
under `rocprofv3 --kernel-trace --stats -- python tools/bench_ema.py ...` and read
ema_carry_kernel's share.

Times are means of one device-event pair per call, calls back to back.  Rates are fractions of the
8 TB/s HBM peak over the ALGORITHMIC bytes n (s + 4): x read once, fp32 y written once."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import digital_signal_processsing_amd as dsp  # noqa: E402
from digital_signal_processsing_amd import _lib  # noqa: E402

PEAK = 8.0e12
HALOS = (256, 2048, 8192, 16384)
CHAIN_ALPHAS = (1e-3, 1e-4, 1e-6)
KINDS = {"f32": (torch.float32, 1), "f32x2": (torch.float32, 2), "i16": (torch.int16, 1), "i16x2": (torch.int16, 2)}
PATHS = {"tile": _lib.EMA_TILE, "chain": _lib.EMA_CHAIN, "strip": _lib.EMA_STRIP}
H = _lib.HOOKS_LIB_PATH


def alpha_with_halo(frames):
    """d^frames = 2^-30 is the boundary to frames + 1: d a hair smaller."""
    a = 1.0 - 2.0 ** (-30.0 / frames) * (1.0 - 1e-12)
    assert dsp.ema_halo_frames(a, H) == frames
    return a


def timed_launches(fn, steps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def bench_shape(alpha, kind, a, bufs, forced=()):
    lib = _lib.load(H)
    C = KINDS[kind][1]
    code = dsp.F32 if kind.startswith("f32") else dsp.I16
    x, y, yrun, ws, state = bufs
    n, s = x.numel(), x.element_size()
    stream = torch.cuda.current_stream().cuda_stream

    def ema_fn():
        _lib.check(lib.mavg_ema_run(x.data_ptr(), y.data_ptr(), n, C, alpha, code, None, state.data_ptr(), ws.data_ptr(),
                                    ws.numel(), stream), "mavg_ema_run")

    def mavg():
        _lib.check(lib.mavg_run(x.data_ptr(), yrun.data_ptr(), n, C, 1024, code, 0, 0, None, ws.data_ptr(), ws.numel(), stream),
                   "mavg_run")

    fns = {"ema": ema_fn, "mavg": mavg}
    plans = {"ema": dsp.ema_plan(n, alpha, C, code, False, True, H), "mavg": dsp.plan(n, 1024, C, code, library=H)}
    for pname in forced:
        lib.mavg_debug_force_ema(PATHS[pname])
        try:
            plans[pname] = dsp.ema_plan(n, alpha, C, code, False, True, H)
            assert dsp.ema_workspace_bytes(n, alpha, C, code, H) <= ws.numel()

            def forced_fn(path=PATHS[pname]):
                lib.mavg_debug_force_ema(path)
                ema_fn()
                lib.mavg_debug_force_ema(_lib.EMA_AUTO)
            fns[pname] = forced_fn
        except dsp.MavgError:
            pass  # this path cannot take the shape
        finally:
            lib.mavg_debug_force_ema(_lib.EMA_AUTO)
    assert max(dsp.workspace_bytes(n, 1024, C, code, library=H), dsp.ema_workspace_bytes(n, alpha, C, code, H)) <= ws.numel()
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {f: [] for f in fns}
    names = list(fns)
    for r in range(a.rounds):
        for f in (names if r % 2 == 0 else names[::-1]):
            t[f] += timed_launches(fns[f], a.steps)
    ms = {f: statistics.mean(v) for f, v in t.items()}
    nbytes = n * (s + 4)
    halo = dsp.ema_halo_frames(alpha, H)
    res = {"dtype": kind, "channels": C, "alpha": alpha, "halo_frames": halo, "halo_bytes": halo * C * s, "samples": n,
           "plans": plans, "ms_mean": ms, "ms_min": {f: min(v) for f, v in t.items()}, "ema_over_mavg": ms["ema"] / ms["mavg"],
           "launches_timed": a.rounds * a.steps,
           "frac_of_peak": {f: nbytes / (ms[f] * 1e-3) / PEAK for f in ms if f != "mavg"}}
    res["frac_of_peak"]["mavg"] = 2 * n * s / (ms["mavg"] * 1e-3) / PEAK
    line = (f"{kind} alpha={alpha:.6g} halo={halo * C * s} B: (a) {plans['ema'].split('<')[0].split()[0]} {ms['ema']:.3f} ms = "
            f"{res['frac_of_peak']['ema']:.3f} of peak | (b) mavg_run k=1024 {ms['mavg']:.3f} ms = "
            f"{res['frac_of_peak']['mavg']:.3f}, (a)/(b) = {res['ema_over_mavg']:.2f}")
    for p in ("tile", "chain", "strip"):
        if p in ms:
            line += f" | forced {p} {ms[p]:.3f} ms"
    if "tile" in ms and "chain" in ms:
        res["chain_over_tile"] = ms["chain"] / ms["tile"]
        line += f", chain/tile = {res['chain_over_tile']:.2f}x"
    if "strip" in ms and "chain" in ms:
        res["strip_over_chain"] = ms["strip"] / ms["chain"]
        line += f", strip/chain = {res['strip_over_chain']:.2f}x"
    print(line, flush=True)
    print(f"    {plans['ema']}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10, help="timed launches per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=30, help="samples = 2^this")
    ap.add_argument("--alphas", type=float, nargs="+", help="coefficients instead of the default set")
    ap.add_argument("--pairs", action="store_true", help="ema_tile / ema_chain forced on the halo shapes, ema_chain / ema_strip at 1e-3")
    ap.add_argument("--dtypes", nargs="+", default=list(KINDS), choices=list(KINDS))
    ap.add_argument("--json", help="also write the results here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ema.py needs the GPU (no CPU fallback)")
    wake = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")  # wake the device: clocks up before timing
    for _ in range(20):
        wake.add_(1)
    torch.cuda.synchronize()
    del wake
    print(f"device {torch.cuda.get_device_name(0)}; libmavg_hooks build id {_lib.build_id(H)}; "
          f"rounds={a.rounds} steps={a.steps} samples=2^{a.log2n}", flush=True)
    res = []
    for kind in a.dtypes:
        tdt, C = KINDS[kind]
        n = 1 << a.log2n
        x = dsp.fill_synthetic(n, tdt, seed=0x5EED, dist=0, device="cuda")
        need = max(64 << 20, n // 64 * 8 + 16)   # the forced strip's records
        bufs = (x, torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty_like(x),
                torch.empty(need, dtype=torch.uint8, device="cuda"), torch.zeros(C, dtype=torch.float64, device="cuda"))
        if a.alphas:
            shapes = [(al, ("tile", "chain", "strip") if a.pairs else ()) for al in a.alphas]
        elif a.pairs:
            shapes = [(alpha_with_halo(h // (C * x.element_size())), ("tile", "chain")) for h in HALOS] + [(1e-3, ("chain", "strip"))]
        else:
            shapes = [(alpha_with_halo(h // (C * x.element_size())), ()) for h in HALOS] + [(al, ()) for al in CHAIN_ALPHAS]
        for alpha, forced in shapes:
            res.append(bench_shape(alpha, kind, a, bufs, forced=forced))
        del bufs, x
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_ema": [{k: v for k, v in r.items() if k != "plans"} for r in res]}))


if __name__ == "__main__":
    main()
