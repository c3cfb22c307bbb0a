#!/usr/bin/env python3
"""Time the moving second moment against what callers compose today.

    python tools/bench_stat.py [--steps 10] [--rounds 3] [--log2n 30] [--k 1024 ...] [--pairs] [--ab LIB LIB ...]
                                [--json out.json]

For every grade k, fp32 and int16, mono and stereo, 2^30 samples, and the variants MEANSQ (one
scan), STD (two scans) and STD with d_mean, in ONE process on one device (lib/libmavg_hooks.so:
release flags plus the path hook), after a warm-up of every path, the rounds alternating the order:

  (a) stat   mavg_stat_run, the path the dispatch rule picks (the plan is printed)
  (b) today  the composition through preallocated buffers: int16 input converted to fp32, torch
             square, mavg_run on x (not for MEANSQ) and on x^2, torch combine (multiply, subtract,
             clamp, square root; the mean is mavg_run's output): the yardstick
  (c) mavg   mavg_run on the same input: the byte model's ceiling (2 s B/sample against the
             statistic's s + 4, s the sample size)

With --pairs, every shape additionally runs with stat_tile and stat_strip forced
(mavg_debug_force_stat) where each can take it, at the grades whose halo k * C * sample size is
256 B, 2 KiB, 8 KiB and 16 KiB: the pairs the tile rule is read from.  The strip is slow: use a
smaller --log2n there.

With --ab LIB [LIB ...], instead: mavg_stat_run alone (RMS, STD, STD with d_mean), by rule, through
each of the given builds (make variant) in turn, the first the yardstick; give one build under two
paths to read the spread.

Times are means of one device-event pair per call (per composition for (b)), calls back to back.
Rates are fractions of the 8 TB/s HBM peak over the ALGORITHMIC bytes of (a): n (s + 4), plus 4 n
with d_mean."""
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
KINDS = {"f32": (torch.float32, 1), "f32x2": (torch.float32, 2), "i16": (torch.int16, 1), "i16x2": (torch.int16, 2)}
VARIANTS = (("meansq", _lib.STAT_MEANSQ, False), ("std", _lib.STAT_STD, False), ("std+mean", _lib.STAT_STD, True))
PATHS = {"tile": _lib.STAT_TILE, "strip": _lib.STAT_STRIP}
H = _lib.HOOKS_LIB_PATH


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


def bench_shape(k, kind, variant, a, bufs, forced=()):
    lib = _lib.load(H)
    name, stat, with_mean = variant
    C = KINDS[kind][1]
    code = dsp.F32 if kind.startswith("f32") else dsp.I16
    x, y, mean, xf, sq, m1, yrun, ws = bufs
    n, s = x.numel(), x.element_size()
    stream = torch.cuda.current_stream().cuda_stream
    mp = mean.data_ptr() if with_mean else None

    def run_f32(src, dst):
        _lib.check(lib.mavg_run(src.data_ptr(), dst.data_ptr(), n, C, k, dsp.F32, 0, 0, None, ws.data_ptr(), ws.numel(),
                                stream), "mavg_run")

    def stat_fn():
        _lib.check(lib.mavg_stat_run(x.data_ptr(), y.data_ptr(), mp, n, C, k, stat, code, None, stream), "mavg_stat_run")

    def today():
        src = x
        if code == dsp.I16:
            xf.copy_(x)
            src = xf
        torch.mul(src, src, out=sq)
        if stat == _lib.STAT_MEANSQ and not with_mean:
            run_f32(sq, y)
            return
        run_f32(src, mean if with_mean else m1)
        run_f32(sq, y)
        mm = mean if with_mean else m1
        torch.mul(mm, mm, out=sq)
        y.sub_(sq).clamp_(min=0).sqrt_()

    def mavg():
        _lib.check(lib.mavg_run(x.data_ptr(), yrun.data_ptr(), n, C, k, code, 0, 0, None, ws.data_ptr(), ws.numel(), stream),
                   "mavg_run")

    fns = {"stat": stat_fn, "today": today, "mavg": mavg}
    plans = {"stat": dsp.stat_plan(n, k, stat, C, code, with_mean, H), "mavg": dsp.plan(n, k, C, code, library=H)}
    for pname in forced:
        lib.mavg_debug_force_stat(PATHS[pname])
        try:
            plans[pname] = dsp.stat_plan(n, k, stat, C, code, with_mean, H)

            def forced_fn(path=PATHS[pname]):
                lib.mavg_debug_force_stat(path)
                stat_fn()
                lib.mavg_debug_force_stat(_lib.STAT_AUTO)
            fns[pname] = forced_fn
        except dsp.MavgError:
            pass  # this path cannot take the shape
        finally:
            lib.mavg_debug_force_stat(_lib.STAT_AUTO)
    assert max(dsp.workspace_bytes(n, k, C, code, library=H), dsp.workspace_bytes(n, k, C, dsp.F32, library=H)) <= ws.numel()
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
    nbytes = n * (s + 4) + (4 * n if with_mean else 0)
    res = {"dtype": kind, "channels": C, "k": k, "variant": name, "halo_bytes": k * C * s, "samples": n, "plans": plans,
           "ms_mean": ms, "ms_min": {f: min(v) for f, v in t.items()}, "stat_over_mavg": ms["stat"] / ms["mavg"],
           "today_over_stat": ms["today"] / ms["stat"], "launches_timed": a.rounds * a.steps,
           "frac_of_peak": {f: nbytes / (ms[f] * 1e-3) / PEAK for f in ms if f not in ("today", "mavg")}}
    res["frac_of_peak"]["mavg"] = 2 * n * s / (ms["mavg"] * 1e-3) / PEAK
    line = (f"{kind} k={k} {name} halo={k * C * s} B: (a) stat {ms['stat']:.3f} ms = {res['frac_of_peak']['stat']:.3f} of peak"
            f" | (b) today {ms['today']:.3f} ms, (b)/(a) = {res['today_over_stat']:.2f}x | (c) mavg_run {ms['mavg']:.3f} ms = "
            f"{res['frac_of_peak']['mavg']:.3f}, (a)/(c) = {res['stat_over_mavg']:.2f}")
    if "tile" in ms and "strip" in ms:
        res["strip_over_tile"] = ms["strip"] / ms["tile"]
        line += f" | forced tile {ms['tile']:.3f} ms, strip {ms['strip']:.3f} ms, strip/tile = {res['strip_over_tile']:.2f}x"
    elif "strip" in ms:
        line += f" | forced strip {ms['strip']:.3f} ms"
    print(line, flush=True)
    print(f"    {plans['stat']}", flush=True)
    return res


AB_VARIANTS = (("rms", _lib.STAT_RMS, False), ("std", _lib.STAT_STD, False), ("std+mean", _lib.STAT_STD, True))


def bench_ab(a):
    """--ab: mavg_stat_run alone, by rule, through several builds of the library in one process
    (each path its own handle; the same build under two paths gives the spread), after a warm-up of
    every build, the rounds alternating the order.  Prints every build's mean and minimum and its
    mean over the first build's."""
    res = []
    libs = [(p, _lib.load(p)) for p in a.ab]
    stream = torch.cuda.current_stream().cuda_stream
    for kind in a.dtypes:
        tdt, C = KINDS[kind]
        code = dsp.F32 if kind.startswith("f32") else dsp.I16
        n = 1 << a.log2n
        x = dsp.fill_synthetic(n, tdt, seed=0x5EED, dist=0, device="cuda")
        y, mean = (torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(2))
        for k in a.k or [1024]:
            for name, stat, with_mean in AB_VARIANTS:
                mp = mean.data_ptr() if with_mean else None

                def run(lib):
                    _lib.check(lib.mavg_stat_run(x.data_ptr(), y.data_ptr(), mp, n, C, k, stat, code, None, stream), "mavg_stat_run")
                for _, lib in libs:
                    for _ in range(2):
                        run(lib)
                torch.cuda.synchronize()
                t = {p: [] for p, _ in libs}
                for r in range(a.rounds):
                    for p, lib in (libs if r % 2 == 0 else libs[::-1]):
                        t[p] += timed_launches(lambda: run(lib), a.steps)
                ms = {p: statistics.mean(v) for p, v in t.items()}
                first = ms[a.ab[0]]
                nbytes = n * (x.element_size() + 4) + (4 * n if with_mean else 0)
                print(f"{kind} k={k} {name}: {dsp.stat_plan(n, k, stat, C, code, with_mean, a.ab[0])}", flush=True)
                for p, _ in libs:
                    print(f"    {os.path.basename(p):28s} id {_lib.build_id(p)} mean {ms[p]:.4f} ms = {nbytes / (ms[p] * 1e-3) / PEAK:.4f} "
                          f"of peak, min {min(t[p]):.4f} ms, mean / first = {ms[p] / first:.4f}", flush=True)
                res.append({"dtype": kind, "channels": C, "k": k, "variant": name, "samples": n, "launches_timed": a.rounds * a.steps,
                            "ms_mean": {os.path.basename(p): ms[p] for p, _ in libs},
                            "ms_min": {os.path.basename(p): min(t[p]) for p, _ in libs},
                            "over_first": {os.path.basename(p): ms[p] / first for p, _ in libs}})
        del x, y, mean
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10, help="timed launches per round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--log2n", type=int, default=30, help="samples = 2^this")
    ap.add_argument("--k", type=int, nargs="+", help="grades instead of the default (1024; with --pairs the four halos)")
    ap.add_argument("--pairs", action="store_true", help="stat_tile and stat_strip forced on every shape")
    ap.add_argument("--dtypes", nargs="+", default=list(KINDS), choices=list(KINDS))
    ap.add_argument("--variants", nargs="+", default=[v[0] for v in VARIANTS], choices=[v[0] for v in VARIANTS])
    ap.add_argument("--json", help="also write the results here")
    ap.add_argument("--ab", nargs="+", metavar="LIB", help="time mavg_stat_run alone (RMS, STD, STD with d_mean) through these "
                    "builds of the library against each other, the first the yardstick (make variant)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_stat.py needs the GPU (no CPU fallback)")
    wake = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")  # wake the device: clocks up before timing
    for _ in range(20):
        wake.add_(1)
    torch.cuda.synchronize()
    del wake
    print(f"device {torch.cuda.get_device_name(0)}; libmavg_hooks build id {_lib.build_id(H)}; "
          f"rounds={a.rounds} steps={a.steps} samples=2^{a.log2n}", flush=True)
    res = bench_ab(a) if a.ab else []
    for kind in ([] if a.ab else a.dtypes):
        tdt, C = KINDS[kind]
        n = 1 << a.log2n
        x = dsp.fill_synthetic(n, tdt, seed=0x5EED, dist=0, device="cuda")
        f32 = lambda: torch.empty(n, dtype=torch.float32, device="cuda")  # noqa: E731
        bufs = (x, f32(), f32(), f32() if tdt == torch.int16 else None, f32(), f32(), torch.empty_like(x),
                torch.empty(64 << 20, dtype=torch.uint8, device="cuda"))
        ks = a.k or ([h // (C * x.element_size()) for h in HALOS] if a.pairs else [1024])
        for k in ks:
            for v in VARIANTS:
                if v[0] in a.variants:
                    res.append(bench_shape(k, kind, v, a, bufs, forced=("tile", "strip") if a.pairs else ()))
        del bufs, x
        torch.cuda.empty_cache()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps({"bench_stat": [{k: v for k, v in r.items() if k != "plans"} for r in res]}))


if __name__ == "__main__":
    main()
