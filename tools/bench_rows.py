#!/usr/bin/env python3
"""Time the batched rows API against its ceiling and against what callers did before it.

    python tools/bench_rows.py [--steps 20] [--rounds 3] [--loop-rows 2048] [--shape R L K ...] [--json out.json]

For every shape [R, L] (R rows of L frames) and window k, fp32 mono and int16 stereo, in ONE
process on one device, after a warm-up of every path:

  (a) rows   mavg_rows_run on the batch (one launch of the rows scan, or the library's per-row
             loop where the dispatch sends the shape there: the plan is printed)
  (b) flat   mavg_run on the same R*L frames as ONE signal with the same k: it moves the same
             bytes (8 B per fp32 sample, 4 B per int16 sample), so it is the ceiling of (a) --
             its RESULT is not the batch's (windows run across row starts)
  (c) loop   what callers had to do: moving_average_into once per row into a preallocated
             output.  Capped at --loop-rows rows per step; where R is larger the per-row cost
             of the capped step is multiplied out to R rows and the line says "extrapolated".

(a) and (b): the mean over rounds x steps launches of one device-event pair per launch, launches
back to back, the rounds alternating (a) and (b).  (c): device events around the whole loop
(host-bound: the time is the enqueue rate), the best of the rounds.  Rates are fractions of the
8 TB/s HBM peak over the algorithmic bytes (every sample read once and written once).  The
device is woken with a copy before anything is timed; the batch is 2^30 samples (4 GiB fp32 in,
4 GiB out), far past the 256-MiB MALL."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import digital_signal_processsing_amd as dsp  # noqa: E402
from digital_signal_processsing_amd import _lib  # noqa: E402

PEAK = 8.0e12
DEFAULT_SHAPES = [(1 << 22, 250, 64), (1 << 20, 1 << 10, 1024), (1 << 14, 1 << 16, 1024), (64, 1 << 24, 1024)]


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


def bench_shape(R, L, k, kind, a):
    C = 1 if kind == "f32" else 2
    R = max(1, R // C)  # the same 2^30 samples for stereo
    tdt, code = (torch.float32, dsp.F32) if kind == "f32" else (torch.int16, dsp.I16)
    n = R * L * C
    x = dsp.fill_synthetic(n, tdt, seed=0x5EED, dist=0, device="cuda")
    y = torch.empty_like(x)
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    rows_ws_n = dsp.rows_workspace_bytes(R, L, k, C, code)
    flat_ws_n = dsp.workspace_bytes(n, k, C, code)
    row_ws_n = dsp.workspace_bytes(L * C, k, C, code)
    ws = torch.empty(max(16, rows_ws_n, flat_ws_n, row_ws_n), dtype=torch.uint8, device="cuda")

    def rows():
        _lib.check(lib.mavg_rows_run(x.data_ptr(), y.data_ptr(), R, L, C, k, code, None, ws.data_ptr(), ws.numel(),
                                     stream), "mavg_rows_run")

    def flat():
        _lib.check(lib.mavg_run(x.data_ptr(), y.data_ptr(), n, C, k, code, 0, 0, None, ws.data_ptr(), ws.numel(),
                                stream), "mavg_run")

    nloop = min(R, a.loop_rows)
    xr, yr = x.view(R, L * C), y.view(R, L * C)

    def loop():
        for r in range(nloop):
            dsp.moving_average_into(xr[r], yr[r], k, channels=C, workspace=ws if row_ws_n else None)

    for fn in (rows, flat):
        for _ in range(3):
            fn()
    loop()
    torch.cuda.synchronize()
    t = {"rows": [], "flat": []}
    t_loop, t_loop_host = [], []
    for r in range(a.rounds):
        for name, fn in ((("rows", rows), ("flat", flat)) if r % 2 == 0 else (("flat", flat), ("rows", rows))):
            t[name] += timed_launches(fn, a.steps)
        e0, e1 = events(1)[0]
        h0 = time.perf_counter()
        e0.record()
        loop()
        e1.record()
        torch.cuda.synchronize()
        t_loop_host.append((time.perf_counter() - h0) * 1e3)
        t_loop.append(e0.elapsed_time(e1))
    byt = 2 * x.element_size() * n
    ms_rows, ms_flat = statistics.mean(t["rows"]), statistics.mean(t["flat"])
    ms_loop_step = min(t_loop)
    ms_loop = ms_loop_step * R / nloop
    res = {
        "dtype": kind, "channels": C, "rows": R, "row_frames": L, "k": k, "samples": n,
        "plan_rows": dsp.rows_plan(R, L, k, C, code), "plan_flat": dsp.plan(n, k, C, code),
        "ms_rows_mean": ms_rows, "ms_rows_median": statistics.median(t["rows"]), "ms_rows_min": min(t["rows"]),
        "ms_flat_mean": ms_flat, "ms_flat_median": statistics.median(t["flat"]), "ms_flat_min": min(t["flat"]),
        "rows_frac_of_peak": byt / (ms_rows * 1e-3) / PEAK, "flat_frac_of_peak": byt / (ms_flat * 1e-3) / PEAK,
        "rows_over_flat": ms_flat / ms_rows,
        "loop_rows_timed": nloop, "ms_loop_timed_step": ms_loop_step, "ms_loop_host_step": min(t_loop_host),
        "us_loop_per_row": ms_loop_step * 1e3 / nloop, "ms_loop_all_rows": ms_loop, "loop_extrapolated": nloop < R,
        "loop_over_rows": ms_loop / ms_rows, "launches_timed": len(t["rows"]),
    }
    print(f"{kind} C={C} [{R}, {L}] k={k}: (a) rows {ms_rows:.3f} ms = {res['rows_frac_of_peak']:.3f} of peak, "
          f"{res['rows_over_flat']:.3f} of (b) | (b) flat {ms_flat:.3f} ms = {res['flat_frac_of_peak']:.3f} | "
          f"(c) loop {ms_loop:.1f} ms{' (extrapolated from ' + str(nloop) + ' rows)' if nloop < R else ''}, "
          f"{res['us_loop_per_row']:.1f} us/row = {res['loop_over_rows']:.1f}x (a)", flush=True)
    print(f"    {res['plan_rows']}", flush=True)
    del x, y, ws
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20, help="timed launches per round (at least 20 in all)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-rows", type=int, default=2048, help="rows per timed step of (c)")
    ap.add_argument("--shape", type=int, nargs=3, action="append", metavar=("R", "L", "K"),
                    help="a shape instead of the default four (repeatable)")
    ap.add_argument("--dtypes", nargs="+", default=["f32", "i16"], choices=["f32", "i16"])
    ap.add_argument("--json", help="also write the results here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_rows.py needs the GPU (no CPU fallback)")
    wake = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")  # wake the device: clocks up before timing
    for _ in range(20):
        wake.add_(1)
    torch.cuda.synchronize()
    del wake
    print(f"device {torch.cuda.get_device_name(0)}; libmavg build id {_lib.build_id()}; "
          f"rounds={a.rounds} steps={a.steps} loop_rows={a.loop_rows}", flush=True)
    out = []
    for kind in a.dtypes:
        for R, L, k in (a.shape or DEFAULT_SHAPES):
            out.append(bench_shape(R, L, k, kind, a))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps({"bench_rows": [{k: v for k, v in r.items() if not k.startswith("plan")} for r in out]}))


if __name__ == "__main__":
    main()
