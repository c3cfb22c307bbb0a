#!/usr/bin/env python3
"""The FIR filter (mavg_fir_run) against the byte floor, the fp64 FMA peak and torch's conv1d.

One process, the hooks library, a warm-up of every path, alternating order, device-event timing
(the style of tools/bench_biquad.py).  Per dtype (fp32 / int16, mono / stereo) on 2^log2n samples
and per tap count (2 .. 1024 and the tile rule's boundary):

  (a) mavg_fir_run by the rule: time, Gsamples/s, useful fp64 FMA/s (samples * taps / time) and its
      fraction of the model peak of 39.3e12 FMA/s (256 CUs * 64 lanes * 2.4 GHz);
  (b) the byte floor: mavg_run at k = 1024 on the same buffer, and (a) / (b).

--pairs: fir_tile and fir_strip forced (mavg_debug_force_fir) on the same shapes: the table the tile
rule's boundary is read from.  The strip makes ntaps uncoalesced reads per output: use --log2n 24.
--conv: fp32 mono only, torch.nn.functional.conv1d in fp32 on the same signal (the alternative a
user has; fp32 accumulation, no history, no int16) beside (a); use --log2n 24.  Its default tap
counts stop at 1024: conv1d with a 4097-tap kernel did not return within four minutes on MI355X.

Times are means of one device-event pair per call, calls back to back.  --out DIR writes
DIR/<mode>.json and DIR/<mode>.txt (default profiles/fir)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import digital_signal_processsing_amd as dsp  # noqa: E402
from digital_signal_processsing_amd import _lib  # noqa: E402

FMA_PEAK = 256 * 64 * 2.4e9       # fp64 FMAs per second: a model, not a measurement
HBM_PEAK = 8.0e12                 # the nominal HBM peak every tool here quotes fractions of (mavg_run reaches 0.76-0.82 of it)
TAPS = (2, 4, 8, 16, 32, 64, 128, 256, 1024)
KINDS = {"f32": (torch.float32, 1), "f32x2": (torch.float32, 2), "i16": (torch.int16, 1), "i16x2": (torch.int16, 2)}
PATHS = {"tile": _lib.FIR_TILE, "strip": _lib.FIR_STRIP}
H = _lib.HOOKS_LIB_PATH


def boundary(kind):
    tdt, C = KINDS[kind]
    return 16384 // (C * (4 if tdt == torch.float32 else 2)) + 1


def make_taps(ntaps):
    """Asymmetric fp32-valued taps with an absolute sum near 1."""
    h = np.random.default_rng(ntaps).standard_normal(ntaps).astype(np.float32).astype(np.float64)
    return (h / np.abs(h).sum()).astype(np.float32).astype(np.float64)


def timed_launches(fn, steps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def time_all(fns, a):
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {f: [] for f in fns}
    names = list(fns)
    for r in range(a.rounds):
        for f in (names if r % 2 == 0 else names[::-1]):
            t[f] += timed_launches(fns[f], a.steps)
    return {f: statistics.mean(v) for f, v in t.items()}, {f: min(v) for f, v in t.items()}


def bench_shape(ntaps, kind, a, bufs, forced=(), conv=False):
    lib = _lib.load(H)
    C = KINDS[kind][1]
    code = dsp.F32 if kind.startswith("f32") else dsp.I16
    x, y, yrun, ws = bufs
    n, s = x.numel(), x.element_size()
    stream = torch.cuda.current_stream().cuda_stream
    h = make_taps(ntaps)
    hd = dsp.fir_taps(h, x.device)

    def fir_fn():
        _lib.check(lib.mavg_fir_run(x.data_ptr(), y.data_ptr(), n, C, hd.data_ptr(), ntaps, code, None, stream), "mavg_fir_run")

    def mavg():
        _lib.check(lib.mavg_run(x.data_ptr(), yrun.data_ptr(), n, C, 1024, code, 0, 0, None,
                                ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, stream), "mavg_run")

    plans = {"fir": dsp.fir_plan(n, ntaps, C, code, library=H)}
    fns = {"fir": fir_fn}
    if forced:
        fns = {}
        for pname in forced:
            lib.mavg_debug_force_fir(PATHS[pname])
            try:
                plans[pname] = dsp.fir_plan(n, ntaps, C, code, library=H)

                def forced_fn(path=PATHS[pname]):
                    lib.mavg_debug_force_fir(path)
                    fir_fn()
                    lib.mavg_debug_force_fir(_lib.FIR_AUTO)
                fns[pname] = forced_fn
            except dsp.MavgError:
                pass  # this path cannot take the shape
            finally:
                lib.mavg_debug_force_fir(_lib.FIR_AUTO)
    elif conv:
        w = hd.to(torch.float32).flip(0).reshape(1, 1, ntaps)       # conv1d correlates: the taps reversed
        xc = x.reshape(1, 1, n)

        def conv_fn():
            torch.nn.functional.conv1d(torch.nn.functional.pad(xc, (ntaps - 1, 0)), w)
        fns["conv1d"] = conv_fn
    else:
        fns["mavg"] = mavg
    ms, mn = time_all(fns, a)
    res = {"dtype": kind, "channels": C, "taps": ntaps, "samples": n, "plans": plans, "ms_mean": ms, "ms_min": mn,
           "launches_timed": a.rounds * a.steps,
           "gsamples_per_s": {f: n / (ms[f] * 1e-3) / 1e9 for f in ms},
           "fma_per_s": {f: n * ntaps / (ms[f] * 1e-3) for f in ms if f != "mavg"}}
    first = next(f for f in ms if f != "mavg" and f != "conv1d")
    res["frac_of_fma_peak"] = res["fma_per_s"][first] / FMA_PEAK
    res["frac_of_hbm_peak"] = n * (s + 4) / (ms[first] * 1e-3) / HBM_PEAK
    line = (f"{kind} taps={ntaps}: {first} {ms[first]:.3f} ms = {res['gsamples_per_s'][first]:.1f} Gsamples/s, "
            f"{res['fma_per_s'][first] / 1e12:.2f}e12 FMA/s = {res['frac_of_fma_peak']:.3f} of the FMA model peak, "
            f"{res['frac_of_hbm_peak']:.3f} of HBM peak over n(s+4) bytes")
    if "mavg" in ms:
        res["fir_over_mavg"] = ms["fir"] / ms["mavg"]
        line += f" | mavg_run k=1024 {ms['mavg']:.3f} ms, fir/mavg = {res['fir_over_mavg']:.2f}x"
    if "conv1d" in ms:
        res["conv1d_over_fir"] = ms["conv1d"] / ms["fir"]
        line += f" | conv1d fp32 {ms['conv1d']:.3f} ms = {res['conv1d_over_fir']:.1f}x the FIR's time"
    if "tile" in ms and "strip" in ms:
        res["strip_over_tile"] = ms["strip"] / ms["tile"]
        line += f" | forced strip {ms['strip']:.3f} ms, strip/tile = {res['strip_over_tile']:.2f}x"
    print(line, flush=True)
    print(f"    {plans[first]}", flush=True)
    return res, line


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5, help="timed launches per round")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--log2n", type=int, default=30, help="samples = 2^this")
    ap.add_argument("--pairs", action="store_true", help="fir_tile / fir_strip forced on the same shapes")
    ap.add_argument("--conv", action="store_true", help="fp32 mono against torch.nn.functional.conv1d")
    ap.add_argument("--taps", nargs="+", type=int, help="tap counts (default: 2 .. 1024 and the rule's boundary)")
    ap.add_argument("--dtypes", nargs="+", default=list(KINDS), choices=list(KINDS))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "fir"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fir.py needs the GPU (no CPU fallback)")
    mode = "pairs" if a.pairs else "conv1d" if a.conv else "sweep"
    wake = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")  # wake the device: clocks up before timing
    for _ in range(20):
        wake.add_(1)
    torch.cuda.synchronize()
    del wake
    head = (f"bench_fir {mode}: device {torch.cuda.get_device_name(0)}; libmavg_hooks build id {_lib.build_id(H)}; "
            f"rounds={a.rounds} steps={a.steps} samples=2^{a.log2n}")
    print(head, flush=True)
    res, lines = [], [head]
    os.makedirs(a.out, exist_ok=True)

    def save():
        with open(os.path.join(a.out, f"{mode}.json"), "w") as f:
            json.dump(res, f, indent=1)
        with open(os.path.join(a.out, f"{mode}.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")

    for kind in (["f32"] if a.conv else a.dtypes):
        tdt, C = KINDS[kind]
        n = 1 << a.log2n
        x = dsp.fill_synthetic(n, tdt, seed=0x5EED, dist=0, device="cuda")
        code = dsp.F32 if tdt == torch.float32 else dsp.I16
        ws_n = dsp.workspace_bytes(n, 1024, C, code, library=H)
        bufs = (x, torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty_like(x),
                torch.empty(ws_n, dtype=torch.uint8, device="cuda") if ws_n else None)
        taps = a.taps or (list(TAPS) + ([] if a.conv else [boundary(kind)]))
        for ntaps in taps:
            if a.pairs and ntaps > boundary(kind):
                continue
            r, line = bench_shape(ntaps, kind, a, bufs, forced=("tile", "strip") if a.pairs else (), conv=a.conv)
            res.append(r)
            lines.append(line)
            save()                                  # after every shape: a killed run keeps what it measured
        del bufs, x
        torch.cuda.empty_cache()
    print(json.dumps({f"bench_fir_{mode}": [{k: v for k, v in r.items() if k != "plans"} for r in res]}))


if __name__ == "__main__":
    main()
