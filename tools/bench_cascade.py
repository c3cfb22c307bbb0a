#!/usr/bin/env python3
"""Time the cascaded moving average against what callers do today.

    python tools/bench_cascade.py [--steps 10] [--rounds 3] [--log2n 30] [--shape K PASSES ...] [--pairs] [--json out.json]

For every (grade k, passes), fp32 mono, int16 mono and int16 stereo, 2^30 samples, in ONE process
on one device (lib/libmavg_hooks.so: release flags plus the path hook), after a warm-up of every
path, the rounds alternating the order:

  (a) cascade  mavg_cascade_run, the path the dispatch rule picks (the plan is printed)
  (b) today    `passes` x mavg_run between the output and a preallocated ping-pong buffer, the last
               pass landing in the output: the yardstick

With --pairs, every shape additionally runs with cascade_tile and cascade_loop forced
(mavg_debug_force_cascade) where each can take it: the pairs the halo rule is read from.

The default shapes are the grades whose total halo passes * (k - 1) * C * sample size is about
256 B, 2 KiB, 8 KiB and 16 KiB, for passes 2, 3 and 4.

Times are means of one device-event pair per launch (per `passes` launches for (b) and the loop),
launches back to back.  Rates are fractions of the 8 TB/s HBM peak over the ALGORITHMIC bytes of
the path that ran: 2 n s for the fused kernel (n samples of s bytes), 2 passes n s for the loop
and for (b)."""
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
PASSES = (2, 3, 4)
KINDS = {"f32": (torch.float32, 1), "i16": (torch.int16, 1), "i16x2": (torch.int16, 2)}
PATHS = {"tile": _lib.CASCADE_TILE, "loop": _lib.CASCADE_LOOP}


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


def algo_bytes(plan, n, s, passes):
    return 2 * n * s if plan.startswith("cascade_tile<") else 2 * passes * n * s


def bench_shape(k, passes, kind, a, bufs, forced=()):
    lib = _lib.load(_lib.HOOKS_LIB_PATH)
    C = KINDS[kind][1]
    code = dsp.F32 if kind == "f32" else dsp.I16
    x, y, pong, ws = bufs
    n, s = x.numel(), x.element_size()
    stream = torch.cuda.current_stream().cuda_stream

    def cascade():
        _lib.check(lib.mavg_cascade_run(x.data_ptr(), y.data_ptr(), n, C, k, passes, code, None, ws.data_ptr(), ws.numel(),
                                        stream), "mavg_cascade_run")

    def today():
        src = x
        for j in range(1, passes + 1):
            dst = pong if (passes - j) & 1 else y
            _lib.check(lib.mavg_run(src.data_ptr(), dst.data_ptr(), n, C, k, code, 0, 0, None, ws.data_ptr(), ws.numel(),
                                    stream), "mavg_run")
            src = dst

    fns = {"cascade": cascade, "today": today}
    plans = {"cascade": dsp.cascade_plan(n, k, passes, C, code, False, _lib.HOOKS_LIB_PATH)}
    for name in forced:
        lib.mavg_debug_force_cascade(PATHS[name])
        try:
            plans[name] = dsp.cascade_plan(n, k, passes, C, code, False, _lib.HOOKS_LIB_PATH)
            assert dsp.cascade_workspace_bytes(n, k, passes, C, code, False, _lib.HOOKS_LIB_PATH) <= ws.numel()

            def forced_fn(path=PATHS[name]):
                lib.mavg_debug_force_cascade(path)
                cascade()
                lib.mavg_debug_force_cascade(_lib.CASCADE_AUTO)
            fns[name] = forced_fn
        except dsp.MavgError:
            pass  # this path cannot take the shape
        finally:
            lib.mavg_debug_force_cascade(_lib.CASCADE_AUTO)
    need = dsp.cascade_workspace_bytes(n, k, passes, C, code, False, _lib.HOOKS_LIB_PATH)
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
    halo = passes * (k - 1) * C * s
    res = {"dtype": kind, "channels": C, "k": k, "passes": passes, "halo_bytes": halo, "samples": n, "plans": plans,
           "ms_mean": ms, "ms_min": {name: min(v) for name, v in t.items()},
           "today_over_cascade": ms["today"] / ms["cascade"], "launches_timed": a.rounds * a.steps}
    if "tile" in ms:
        res["today_over_tile"] = ms["today"] / ms["tile"]
    res["frac_of_peak"] = {name: algo_bytes(plans[name], n, s, passes) / (ms[name] * 1e-3) / PEAK for name in plans}
    res["frac_of_peak"]["today"] = 2 * passes * n * s / (ms["today"] * 1e-3) / PEAK
    line = (f"{kind} C={C} k={k} passes={passes} halo={halo} B: (a) cascade {ms['cascade']:.3f} ms = "
            f"{res['frac_of_peak']['cascade']:.3f} of peak | (b) today {ms['today']:.3f} ms = "
            f"{res['frac_of_peak']['today']:.3f}, (b)/(a) = {res['today_over_cascade']:.2f}x")
    for name in forced:
        if name in ms:
            line += f" | forced {name} {ms[name]:.3f} ms, (b)/{name} = {ms['today'] / ms[name]:.2f}x"
    print(line, flush=True)
    print(f"    {plans['cascade']}", flush=True)
    return res


def default_shapes(kind):
    s = KINDS[kind][0].itemsize * KINDS[kind][1]
    return [(h // (p * s) + 1, p) for p in PASSES for h in HALOS]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10, help="timed launches per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=30, help="samples = 2^this")
    ap.add_argument("--shape", type=int, nargs=2, action="append", metavar=("K", "PASSES"),
                    help="a shape instead of the defaults (repeatable)")
    ap.add_argument("--pairs", action="store_true", help="cascade_tile and cascade_loop forced on every shape")
    ap.add_argument("--dtypes", nargs="+", default=list(KINDS), choices=list(KINDS))
    ap.add_argument("--json", help="also write the results here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_cascade.py needs the GPU (no CPU fallback)")
    wake = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")  # wake the device: clocks up before timing
    for _ in range(20):
        wake.add_(1)
    torch.cuda.synchronize()
    del wake
    print(f"device {torch.cuda.get_device_name(0)}; libmavg_hooks build id {_lib.build_id(_lib.HOOKS_LIB_PATH)}; "
          f"rounds={a.rounds} steps={a.steps} samples=2^{a.log2n}", flush=True)
    res = []
    for kind in a.dtypes:
        tdt = KINDS[kind][0]
        n = 1 << a.log2n
        x = dsp.fill_synthetic(n, tdt, seed=0x5EED, dist=0, device="cuda")
        bufs = (x, torch.empty_like(x), torch.empty_like(x),
                torch.empty(n * x.element_size() + (64 << 20), dtype=torch.uint8, device="cuda"))
        for k, passes in (a.shape or default_shapes(kind)):
            res.append(bench_shape(k, passes, kind, a, bufs, forced=("tile", "loop") if a.pairs else ()))
        del bufs, x
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_cascade": [{k: v for k, v in r.items() if k != "plans"} for r in res]}))


if __name__ == "__main__":
    main()
