#!/usr/bin/env python3
"""The cascade (mavg_sos_run) against the loop of biquads it replaces.

One process, the hooks library, a warm-up of every path, alternating order, device-event timing
(the style of tools/bench_biquad.py).  Per dtype (fp32 / int16, mono / stereo) on 2^log2n samples,
for S = 2, 4 and 8 equal RBJ low-pass sections (Q 0.7071) whose total halo sum H_j * C * 8 B is the
largest not above 256 B, 2 KiB, 8 KiB and 16 KiB (the fused kernel's limit):

  (a) mavg_sos_run by the rule;
  (b) the yardstick: S calls of mavg_biquad_run through two fp32 buffers, the last into the output
      -- what sos_filter does, and what sos_loop does from C;
  (c) one mavg_biquad_run of the first section.

--pairs: sos_tile and sos_loop forced (mavg_debug_force_sos) on the same shapes: the table the
rule's boundary is read from.

Times are means of one device-event pair per call, calls back to back.  Rates are fractions of the
8 TB/s HBM peak over the ALGORITHMIC bytes n (s + 4): x read once, fp32 y written once -- whatever
S; the loop moves (s + 4) + (S - 1) 8 bytes per sample."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import digital_signal_processsing_amd as dsp  # noqa: E402
from digital_signal_processsing_amd import _lib  # noqa: E402

PEAK = 8.0e12
HALOS = (256, 2048, 8192, 16384)
SECTIONS = (2, 4, 8)
KINDS = {"f32": (torch.float32, 1), "f32x2": (torch.float32, 2), "i16": (torch.int16, 1), "i16x2": (torch.int16, 2)}
PATHS = {"tile": _lib.SOS_TILE, "loop": _lib.SOS_LOOP}
H = _lib.HOOKS_LIB_PATH


def rbj_lp(f, Q=0.7071):
    w = 2.0 * math.pi * f
    cw, al = math.cos(w), math.sin(w) / (2.0 * Q)
    b = [(1 - cw) / 2, 1 - cw, (1 - cw) / 2]
    return tuple(v / (1 + al) for v in b) + (-2 * cw / (1 + al), (1 - al) / (1 + al))


def lp_with_halo(frames):
    """The RBJ low-pass, Q 0.7071, with the largest library H <= frames."""
    Hf = lambda f: dsp.biquad_halo_frames(rbj_lp(f), H)
    lo, hi = 1e-5, 0.25
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if Hf(mid) > frames else (lo, mid)
    return rbj_lp(hi)


def timed_launches(fn, steps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def bench_shape(label, coef, S, kind, a, bufs, forced=()):
    lib = _lib.load(H)
    C = KINDS[kind][1]
    code = dsp.F32 if kind.startswith("f32") else dsp.I16
    x, y, ping, pong, ws, state = bufs
    n, s = x.numel(), x.element_size()
    stream = torch.cuda.current_stream().cuda_stream
    rows = [[coef[0], coef[1], coef[2], 1.0, coef[3], coef[4]]] * S
    c5 = (ctypes.c_double * 5)(*coef)
    cS = (ctypes.c_double * (5 * S))(*(list(coef) * S))
    halo = dsp.sos_halo_frames(rows, H)

    def sos_fn():
        _lib.check(lib.mavg_sos_run(x.data_ptr(), y.data_ptr(), n, C, cS, S, code, 0, None, state.data_ptr(), ws.data_ptr(),
                                    ws.numel(), stream), "mavg_sos_run")

    def one(src, dst, dt):
        _lib.check(lib.mavg_biquad_run(src.data_ptr(), dst.data_ptr(), n, C, c5, dt, None, state.data_ptr(), ws.data_ptr(),
                                       ws.numel(), stream), "mavg_biquad_run")

    def biquads_fn():
        cur, dt = x, code
        for j in range(S):
            dst = y if j == S - 1 else (ping if j % 2 == 0 else pong)
            one(cur, dst, dt)
            cur, dt = dst, dsp.F32

    def biquad_fn():
        one(x, y, code)

    fns = {"sos": sos_fn} if forced else {"sos": sos_fn, "biquads": biquads_fn, "biquad": biquad_fn}
    plans = {"sos": dsp.sos_plan(n, rows, C, code, False, True, library=H)}
    for pname in forced:
        lib.mavg_debug_force_sos(PATHS[pname])
        try:
            plans[pname] = dsp.sos_plan(n, rows, C, code, False, True, library=H)
            assert dsp.sos_workspace_bytes(n, rows, C, code, library=H) <= ws.numel()

            def forced_fn(path=PATHS[pname]):
                lib.mavg_debug_force_sos(path)
                sos_fn()
                lib.mavg_debug_force_sos(_lib.SOS_AUTO)
            fns[pname] = forced_fn
        except dsp.MavgError:
            pass  # this path cannot take the shape
        finally:
            lib.mavg_debug_force_sos(_lib.SOS_AUTO)
    assert max(dsp.sos_workspace_bytes(n, rows, C, code, library=H), dsp.biquad_workspace_bytes(n, coef, C, code, H)) <= ws.numel()
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
    per_round = {f: [statistics.mean(v[i * a.steps:(i + 1) * a.steps]) for i in range(a.rounds)] for f, v in t.items()}
    nbytes = n * (s + 4)
    res = {"dtype": kind, "channels": C, "sections": S, "filter": label, "coef": list(coef), "halo_frames": halo,
           "halo_bytes": halo * C * 8, "samples": n, "plans": plans, "ms_mean": ms, "ms_round_means": per_round,
           "ms_min": {f: min(v) for f, v in t.items()}, "launches_timed": a.rounds * a.steps,
           "frac_of_peak": {f: nbytes / (ms[f] * 1e-3) / PEAK for f in ms}}
    line = (f"{kind} S={S} {label} halo={halo * C * 8} B: (a) {plans['sos'].split('<')[0].split()[0]} {ms['sos']:.3f} ms = "
            f"{res['frac_of_peak']['sos']:.3f} of peak")
    if "biquads" in ms:
        res["biquads_over_sos"] = ms["biquads"] / ms["sos"]
        line += (f" | (b) {S} x mavg_biquad_run {ms['biquads']:.3f} ms, (b)/(a) = {res['biquads_over_sos']:.2f}x | (c) one "
                 f"mavg_biquad_run {ms['biquad']:.3f} ms")
    for p in ("tile", "loop"):
        if p in ms:
            line += f" | forced {p} {ms[p]:.3f} ms"
    if "tile" in ms and "loop" in ms:
        res["loop_over_tile"] = ms["loop"] / ms["tile"]
        res["loop_over_tile_rounds"] = [lo / ti for lo, ti in zip(per_round["loop"], per_round["tile"])]
        line += f", loop/tile = {res['loop_over_tile']:.2f}x (rounds " + " ".join(f"{v:.2f}" for v in res["loop_over_tile_rounds"]) + ")"
    print(line, flush=True)
    print(f"    {plans['sos']}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10, help="timed launches per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=28, help="samples = 2^this")
    ap.add_argument("--pairs", action="store_true", help="sos_tile / sos_loop forced on every shape")
    ap.add_argument("--dtypes", nargs="+", default=list(KINDS), choices=list(KINDS))
    ap.add_argument("--sections", nargs="+", type=int, default=list(SECTIONS))
    ap.add_argument("--json", help="also write the results here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sos.py needs the GPU (no CPU fallback)")
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
        need = 2 * (n * 4 + 16) + (64 << 20)    # the forced loop's two buffers and a section's records
        bufs = (x, torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda"),
                torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(need, dtype=torch.uint8, device="cuda"),
                torch.zeros(2 * C * max(a.sections), dtype=torch.float64, device="cuda"))
        for S in a.sections:
            for h in HALOS:
                coef = lp_with_halo(h // (C * 8) // S)
                forced = ("tile", "loop") if a.pairs else ()
                res.append(bench_shape(f"LP total halo<={h}B", coef, S, kind, a, bufs, forced=forced))
        del bufs, x
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_sos": [{k: v for k, v in r.items() if k != "plans"} for r in res]}))


if __name__ == "__main__":
    main()
