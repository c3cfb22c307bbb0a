#!/usr/bin/env python3
"""plan_diff.py -- compare the dispatch of two builds of libmavg without a GPU.

    python3 tools/plan_diff.py <libA.so> <libB.so>

Plan mode needs no device.  For both libraries: mavg_plan and mavg_workspace_bytes over both
dtypes, 1..8 channels, every algo, every reference block size, n in {0, 1, 4099 C, 2^30} and the
windows around every dispatch threshold of csrc/mavg_launch.hpp; then a few rows and ragged
plans (rows_loop goes through the same launchers).  Every plan string, workspace size and error
status must be equal; the plan string's lds= field is the kernel's LDS layout, ws= the look-ahead
workspace layout.  Prints each difference and one summary line; exit status 1 if any differ.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import digital_signal_processsing_amd as dsp  # noqa: E402
from digital_signal_processsing_amd import _lib  # noqa: E402

ELEM = {dsp.I16: 2, dsp.F32: 4}
ACC = {dsp.I16: (4, 8), dsp.F32: (8,)}


def windows(dtype, C):
    """1, 7 and each dispatch threshold with the value below and above it."""
    e = ELEM[dtype]
    at = {1, 7, 65535, 65536, 131072, 1 << 21}
    at |= {2048, 2544, 2560, 3072, 3584, 512, 1024}  # the channel-per-lane rules (frames)
    for h in (256, 512, 2048, 4096, 8192, 16384, 32768, 40704, 49152, 65536, 1 << 21):  # halo bytes
        at.add(h // (C * e))
    for tf in (512, 1024, 2048, 4096, 8192, 16384):  # tile frames: self, past-L2, run-total, U8 bounds
        at |= {3 * tf, 8 * tf, 64 * tf, 384 * tf, 1024 * tf}
    # where a tile or a direct stage stops fitting its LDS budget
    for wg in (64, 128, 256, 512, 1024):
        budget = 80 * 1024 if wg >= 1024 else 64 * 1024
        for F in (1, 2, 4, 8):
            for U in (1, 2, 4, 8):
                for a in ACC[dtype]:
                    at.add(F * ((budget - (U + 1) * (wg // 64) * C * a) // (F * C * e) - U * wg - 1))
                at.add(F * (64 * 1024 // (F * C * e) - U * wg) + 1)
    ks = set()
    for k in at:
        ks |= {k - 1, k, k + 1}
    return sorted(k for k in ks if 1 <= k < (1 << 31))


def probe(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except _lib.MavgError as err:
        return f"status {err.status}"


def main(lib_a, lib_b):
    calls = differ = 0

    def both(what, fn, *a, **kw):
        nonlocal calls, differ
        ra, rb = probe(fn, *a, library=lib_a, **kw), probe(fn, *a, library=lib_b, **kw)
        calls += 1
        if ra != rb:
            differ += 1
            print(f"DIFF {what} {a} {kw}\n  A: {ra}\n  B: {rb}")

    for dtype in (dsp.I16, dsp.F32):
        for C in range(1, 9):
            ks = windows(dtype, C)
            for algo in sorted(dsp.ALGOS):
                for block in (0, 64, 128, 256, 512, 1024):
                    for n in (0, 1, 4099 * C, 1 << 30):
                        for k in ks:
                            both("plan", dsp.plan, n, k, C, dtype, algo, block)
                            both("workspace_bytes", dsp.workspace_bytes, n, k, C, dtype, algo, block)
    for dtype in (dsp.I16, dsp.F32):
        for C in (1, 2, 4):
            for rows, L in ((37, 1001), (3, 1 << 20), (1, 1 << 27), (100000, 64)):
                for k in (1, 64, 4096, 8191, 8192, 8193, 44100, 1 << 20):
                    for hist in (False, True):
                        both("rows_plan", dsp.rows_plan, rows, L, k, C, dtype, hist)
                        both("rows_workspace_bytes", dsp.rows_workspace_bytes, rows, L, k, C, dtype, hist)
            for lens in ([1001, 0, 5, 333, 0, 2048, 64], [1 << 22, 7, 1 << 20]):
                offs = [0]
                for ln in lens:
                    offs.append(offs[-1] + ln)
                for k in (1, 64, 4096, 8193, 44100):
                    both("ragged_plan", dsp.ragged_plan, offs, k, C, dtype)
                    both("ragged_workspace_bytes", dsp.ragged_workspace_bytes, offs, k, C, dtype)
    print(f"plan_diff: {calls} calls on each of {lib_a} and {lib_b}, {differ} differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])))
