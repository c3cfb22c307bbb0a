#!/usr/bin/env python3
"""Time the ragged rows API against the rows scan on the same bytes and against what callers did before it.

    python tools/bench_ragged.py [--steps 20] [--rounds 3] [--loop-rows 2048] [--shapes NAME ...] [--json out.json]

For every batch shape and window k (64 and 1024), fp32 mono and int16 stereo, in ONE process on
one device, after a warm-up of every path:

  (a) ragged  mavg_ragged_run on the packed batch (one launch of the ragged scan: the plan is
              printed)
  (b) rows    mavg_rows_run on a UNIFORM batch of the same total (rows of the shape's mean
              length), dtype, channels and k: the same bytes through rows_scan_kernel, the
              kernel the ragged scan was derived from -- (a)'s yardstick.  Its result is not
              the ragged batch's.
  (c) loop    what callers had to do: moving_average_into once per row into a preallocated
              output, on a sample of --loop-rows rows spread evenly over the batch; the
              per-row cost of the sample is multiplied out to all rows (the spike row is
              kept out of the sample, so it counts as an ordinary row: (c) is understated).

Shapes: seeded log-uniform row lengths (a factor 64 between the shortest and the longest) with
mean 250, 2^10 and 2^16 frames, 2^30 samples per batch; and "spike": 2^20 rows of 250 frames
with a single 2^24-frame row in the middle (stereo: half as many rows).

(a) and (b): the mean over rounds x steps launches of one device-event pair per launch, launches
back to back, the rounds alternating (a) and (b).  (c): device events around the whole loop
(host-bound), the best of the rounds.  Rates are fractions of the 8 TB/s HBM peak over the
algorithmic bytes (every sample read once and written once); (a) / (b) compares rates, so a
uniform batch a few rows short of the ragged total does not bias it."""
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
from tools.bench_rows import events, timed_launches  # noqa: E402

PEAK = 8.0e12
TOTAL = 1 << 30
SHAPES = ("mean250", "mean1024", "mean65536", "spike")
WINDOWS = (64, 1024)


def log_uniform_lengths(mean, total_frames, seed):
    """Row lengths exp(U(ln a, ln 64a)) with the given mean, cumulating to exactly total_frames."""
    a = mean * np.log(64.0) / 63.0
    rng = np.random.RandomState(seed)
    n = int(total_frames / mean * 1.1) + 16
    v = np.maximum(1, np.exp(rng.uniform(np.log(a), np.log(64 * a), size=n)).astype(np.int64))
    cut = int(np.searchsorted(np.cumsum(v), total_frames, side="left"))
    v = v[:cut + 1]
    v[-1] -= int(v.sum()) - total_frames
    assert v.sum() == total_frames and (v > 0).all()
    return v


def shape_lengths(name, C):
    if name == "spike":
        half = (1 << 20) // C // 2
        return np.concatenate([np.full(half, 250), [1 << 24], np.full(half, 250)]).astype(np.int64), 250
    mean = int(name[4:])
    return log_uniform_lengths(mean, TOTAL // C, seed=mean), mean


def bench_shape(name, k, kind, a):
    C = 1 if kind == "f32" else 2
    tdt, code = (torch.float32, dsp.F32) if kind == "f32" else (torch.int16, dsp.I16)
    lengths, mean = shape_lengths(name, C)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64))
    R, frames = len(lengths), int(off[-1])
    n = frames * C
    x = dsp.fill_synthetic(n, tdt, seed=0x5EED, dist=0, device="cuda")
    y = torch.empty_like(x)
    d_off = off.cuda()
    lib = _lib.load()
    stream = torch.cuda.current_stream().cuda_stream
    h_off = dsp._offsets_ptr(off)
    Ru, Lu = frames // mean, mean  # the uniform yardstick: the same bytes, a few frames short at most
    nu = Ru * Lu * C
    plan_a, plan_b = dsp.ragged_plan(off, k, C, code), dsp.rows_plan(Ru, Lu, k, C, code)
    longest = int(lengths.max())
    ws_n = max(16, dsp.ragged_workspace_bytes(off, k, C, code), dsp.rows_workspace_bytes(Ru, Lu, k, C, code),
               dsp.workspace_bytes(longest * C, k, C, code))
    ws = torch.empty(ws_n, dtype=torch.uint8, device="cuda")

    def ragged():
        _lib.check(lib.mavg_ragged_run(x.data_ptr(), y.data_ptr(), h_off, d_off.data_ptr(), R, C, k, code, ws.data_ptr(),
                                       ws.numel(), stream), "mavg_ragged_run")

    def rows():
        _lib.check(lib.mavg_rows_run(x.data_ptr(), y.data_ptr(), Ru, Lu, C, k, code, None, ws.data_ptr(), ws.numel(),
                                     stream), "mavg_rows_run")

    pick = np.unique(np.linspace(0, R - 1, min(R, a.loop_rows)).astype(np.int64))
    pick = pick[lengths[pick] <= 100 * mean]  # not the spike: multiplied out, it would count 2^24 frames per row
    o = off.numpy()
    views = [(x[o[r] * C:o[r + 1] * C], y[o[r] * C:o[r + 1] * C]) for r in pick]

    def loop():
        for xr, yr in views:
            dsp.moving_average_into(xr, yr, k, channels=C, workspace=ws)

    for fn in (ragged, rows):
        for _ in range(3):
            fn()
    loop()
    torch.cuda.synchronize()
    t = {"ragged": [], "rows": []}
    t_loop = []
    for r in range(a.rounds):
        order = (("ragged", ragged), ("rows", rows))
        for key, fn in (order if r % 2 == 0 else order[::-1]):
            t[key] += timed_launches(fn, a.steps)
        e0, e1 = events(1)[0]
        e0.record()
        loop()
        e1.record()
        torch.cuda.synchronize()
        t_loop.append(e0.elapsed_time(e1))
    ms_a, ms_b = statistics.mean(t["ragged"]), statistics.mean(t["rows"])
    rate_a = 2 * x.element_size() * n / (ms_a * 1e-3)
    rate_b = 2 * x.element_size() * nu / (ms_b * 1e-3)
    us_row = min(t_loop) * 1e3 / len(views)
    ms_loop = us_row * 1e-3 * R
    res = {
        "shape": name, "dtype": kind, "channels": C, "k": k, "rows": R, "frames": frames, "samples": n,
        "mean_row_frames": frames / R, "max_row_frames": longest, "uniform_rows": Ru, "uniform_row_frames": Lu,
        "plan_ragged": plan_a, "plan_rows": plan_b,
        "ms_ragged_mean": ms_a, "ms_ragged_median": statistics.median(t["ragged"]), "ms_ragged_min": min(t["ragged"]),
        "ms_rows_mean": ms_b, "ms_rows_median": statistics.median(t["rows"]), "ms_rows_min": min(t["rows"]),
        "ragged_frac_of_peak": rate_a / PEAK, "rows_frac_of_peak": rate_b / PEAK, "ragged_over_rows": rate_a / rate_b,
        "loop_rows_timed": len(views), "us_loop_per_row": us_row, "ms_loop_all_rows": ms_loop,
        "loop_over_ragged": ms_loop / ms_a, "launches_timed": len(t["ragged"]),
    }
    print(f"{kind} C={C} {name} rows={R} k={k}: (a) ragged {ms_a:.3f} ms = {res['ragged_frac_of_peak']:.3f} of peak | "
          f"(b) rows [{Ru}, {Lu}] {ms_b:.3f} ms = {res['rows_frac_of_peak']:.3f} | (a)/(b) {res['ragged_over_rows']:.3f} | "
          f"(c) loop {ms_loop:.1f} ms (from {len(views)} rows, {us_row:.1f} us/row) = {res['loop_over_ragged']:.1f}x (a)",
          flush=True)
    print(f"    {plan_a}\n    {plan_b}", flush=True)
    del x, y, ws, d_off, views
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20, help="timed launches per round (at least 20 in all)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--loop-rows", type=int, default=2048, help="rows sampled per timed step of (c)")
    ap.add_argument("--shapes", nargs="+", default=list(SHAPES), choices=SHAPES)
    ap.add_argument("--windows", type=int, nargs="+", default=list(WINDOWS))
    ap.add_argument("--dtypes", nargs="+", default=["f32", "i16"], choices=["f32", "i16"])
    ap.add_argument("--json", help="also write the results here")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ragged.py needs the GPU (no CPU fallback)")
    wake = torch.empty(1 << 28, dtype=torch.uint8, device="cuda")  # wake the device: clocks up before timing
    for _ in range(20):
        wake.add_(1)
    torch.cuda.synchronize()
    del wake
    print(f"device {torch.cuda.get_device_name(0)}; libmavg build id {_lib.build_id()}; "
          f"rounds={a.rounds} steps={a.steps} loop_rows={a.loop_rows}", flush=True)
    out = []
    for kind in a.dtypes:
        for name in a.shapes:
            for k in a.windows:
                out.append(bench_shape(name, k, kind, a))
                if a.json:  # after every shape: a run cut short keeps what it measured
                    with open(a.json, "w") as f:
                        json.dump(out, f, indent=1)
    print(json.dumps({"bench_ragged": [{k: v for k, v in r.items() if not k.startswith("plan")} for r in out]}))


if __name__ == "__main__":
    main()
