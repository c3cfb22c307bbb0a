#!/usr/bin/env python3
"""Time the decimated moving average against what callers do today.

    python tools/bench_decim.py [--steps 10] [--rounds 3] [--log2n 30] [--shape K HOP ...] [--pairs] [--json out.json]

For every (grade k, hop), fp32 mono and int16 stereo, 2^30 samples, in ONE process on one device
(lib/libmavg_hooks.so: release flags plus the path hook), after a warm-up of every path, the
rounds alternating the order:

  (a) decim   mavg_decim_run, the path the dispatch rule picks (the plan is printed)
  (b) today   mavg_run at full rate, then y.view(-1, C)[phase::hop] copied into a preallocated
              packed buffer: the yardstick
  (c) full    mavg_run alone on the same input -- NOT a ceiling: (a) moves fewer bytes

With --pairs, every shape additionally runs with decim_scan and decim_window forced
(mavg_debug_force_decim) where each can take it: the pairs the window rule's two thresholds are
read from.

Times are means of one device-event pair per launch (per launch pair for (b)), launches back to
back.  Rates are fractions of the 8 TB/s HBM peak over the ALGORITHMIC bytes of the path that ran:
n s (1 + 1/hop) for the scan, M (k + 1) C s for the window sum (n samples of s bytes, M output
frames), 2 n s for the full-rate filter."""
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
DEFAULT_SHAPES = [(1024, 2), (1024, 4), (1024, 160), (1024, 512), (1024, 1024), (400, 160), (4, 4)]
PAIR_SHAPES = [(1024, 1024), (1024, 2048), (1024, 4096), (1024, 44100), (64, 256), (256, 1024)]
PATHS = {"scan": _lib.DECIM_SCAN, "window": _lib.DECIM_WINDOW}


def events(n):
    return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]


def timed_launches(fn, steps):
    ev = events(steps)
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def algo_bytes(plan, n, M, k, C, s, hop):
    if plan.startswith("decim_window<"):
        return M * (k + 1) * C * s
    if plan.startswith("decim_scan<"):
        return n * s * (1 + 1 / hop)
    return 2 * n * s + 2 * M * C * s  # decim_full: the full-rate filter, then the gather


def bench_shape(k, hop, kind, a, bufs, forced=()):
    lib = _lib.load(_lib.HOOKS_LIB_PATH)
    C = 1 if kind == "f32" else 2
    code = dsp.F32 if kind == "f32" else dsp.I16
    x, y, out, ws = bufs
    n, s, phase = x.numel(), x.element_size(), hop // 2
    M = len(range(phase, n // C, hop))
    stream = torch.cuda.current_stream().cuda_stream
    outv = out[:M * C]

    def decim():
        _lib.check(lib.mavg_decim_run(x.data_ptr(), outv.data_ptr(), n, C, k, hop, phase, code, None, ws.data_ptr(),
                                      ws.numel(), stream), "mavg_decim_run")

    def full():
        _lib.check(lib.mavg_run(x.data_ptr(), y.data_ptr(), n, C, k, code, 0, 0, None, ws.data_ptr(), ws.numel(),
                                stream), "mavg_run")

    def today():
        full()
        outv.view(M, C).copy_(y.view(-1, C)[phase::hop])

    fns = {"decim": decim, "today": today, "full": full}
    plans = {"decim": dsp.decim_plan(n, k, hop, phase, C, code, _lib.HOOKS_LIB_PATH)}
    for name in forced:
        lib.mavg_debug_force_decim(PATHS[name])
        try:
            plans[name] = dsp.decim_plan(n, k, hop, phase, C, code, _lib.HOOKS_LIB_PATH)

            def forced_fn(path=PATHS[name]):
                lib.mavg_debug_force_decim(path)
                decim()
                lib.mavg_debug_force_decim(_lib.DECIM_AUTO)
            fns[name] = forced_fn
        except dsp.MavgError:
            pass  # this path cannot take the shape
        finally:
            lib.mavg_debug_force_decim(_lib.DECIM_AUTO)
    need = dsp.decim_workspace_bytes(n, k, hop, phase, C, code, _lib.HOOKS_LIB_PATH)
    assert need <= ws.numel(), (need, ws.numel())
    for fn in fns.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in fns}
    names = list(fns)
    for r in range(a.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            t[name] += timed_launches(fns[name], a.steps)
    ms = {name: statistics.mean(v) for name, v in t.items()}
    res = {"dtype": kind, "channels": C, "k": k, "hop": hop, "phase": phase, "samples": n, "out_frames": M,
           "plans": plans, "ms_mean": ms, "ms_min": {name: min(v) for name, v in t.items()},
           "today_over_decim": ms["today"] / ms["decim"], "launches_timed": a.rounds * a.steps}
    res["frac_of_peak"] = {name: algo_bytes(plans[name], n, M, k, C, s, hop) / (ms[name] * 1e-3) / PEAK for name in plans}
    res["frac_of_peak"]["full"] = 2 * n * s / (ms["full"] * 1e-3) / PEAK
    line = (f"{kind} C={C} k={k} hop={hop}: (a) decim {ms['decim']:.3f} ms = {res['frac_of_peak']['decim']:.3f} of peak | "
            f"(b) today {ms['today']:.3f} ms, (b)/(a) = {res['today_over_decim']:.2f}x | "
            f"(c) full {ms['full']:.3f} ms = {res['frac_of_peak']['full']:.3f}")
    for name in forced:
        if name in ms:
            line += f" | forced {name} {ms[name]:.3f} ms = {res['frac_of_peak'][name]:.3f}"
    print(line, flush=True)
    print(f"    {plans['decim']}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10, help="timed launches per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=30, help="samples = 2^this")
    ap.add_argument("--shape", type=int, nargs=2, action="append", metavar=("K", "HOP"),
                    help="a shape instead of the defaults (repeatable)")
    ap.add_argument("--pairs", action="store_true", help="the window rule's shapes, scan and window forced")
    ap.add_argument("--dtypes", nargs="+", default=["f32", "i16"], choices=["f32", "i16"])
    ap.add_argument("--json", help="also write the results here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decim.py needs the GPU (no CPU fallback)")
    wake = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")  # wake the device: clocks up before timing
    for _ in range(20):
        wake.add_(1)
    torch.cuda.synchronize()
    del wake
    print(f"device {torch.cuda.get_device_name(0)}; libmavg_hooks build id {_lib.build_id(_lib.HOOKS_LIB_PATH)}; "
          f"rounds={a.rounds} steps={a.steps} samples=2^{a.log2n}", flush=True)
    shapes = a.shape or (PAIR_SHAPES if a.pairs else DEFAULT_SHAPES)
    res = []
    for kind in a.dtypes:
        tdt = torch.float32 if kind == "f32" else torch.int16
        n = 1 << a.log2n
        x = dsp.fill_synthetic(n, tdt, seed=0x5EED, dist=0, device="cuda")
        bufs = (x, torch.empty_like(x), torch.empty(n // 2 + 16, dtype=tdt, device="cuda"),
                torch.empty(n * x.element_size() + (64 << 20), dtype=torch.uint8, device="cuda"))
        for k, hop in shapes:
            res.append(bench_shape(k, hop, kind, a, bufs, forced=("scan", "window") if a.pairs else ()))
        del bufs, x
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_decim": [{k: v for k, v in r.items() if k != "plans"} for r in res]}))


if __name__ == "__main__":
    main()
