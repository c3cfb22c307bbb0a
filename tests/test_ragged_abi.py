"""CPU tests of the ragged rows API (mavg_ragged_run, mavg_ragged_workspace_bytes,
mavg_ragged_plan, include/mavg.h): the symbols, the status table with dummy pointers, the
dispatch rule as the plan text shows it, the workspace sizes and the wrapper's argument checks.
No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import digital_signal_processsing_amd as dsp
from digital_signal_processsing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RAGGED_SYMBOLS = ("mavg_ragged_run", "mavg_ragged_workspace_bytes", "mavg_ragged_plan")
SCAN, LOOP = "ragged_scan<", "ragged_loop"


def test_ragged_symbols_are_exported_by_release_and_debug():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        lib = _lib.load(path)
        for name in RAGGED_SYMBOLS:
            assert hasattr(lib, name), (path, name)
        assert lib.mavg_abi_version() == _lib.ABI_VERSION == 4  # additive: the version stays


def test_ragged_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "mavg.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(mavg_\w+)\s*\(", text, re.M))
    assert set(RAGGED_SYMBOLS) <= declared
    assert set(RAGGED_SYMBOLS) <= set(_lib.EXPORTED_SYMBOLS)
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    assert len(lib.mavg_ragged_run.argtypes) == 11
    assert len(lib.mavg_ragged_workspace_bytes.argtypes) == 6
    assert len(lib.mavg_ragged_plan.argtypes) == 7


def _arr(off):
    return (ctypes.c_int64 * len(off))(*off) if off is not None else None


def _run(off, C=1, k=3, dtype=_lib.F32, din=16, dout=32, doff=64, rows=None):
    rows = (len(off) - 1) if rows is None else rows
    return _lib.load().mavg_ragged_run(din, dout, _arr(off), doff, rows, C, k, dtype, None, 0, None)


OFF = [0, 4, 4, 10]
HUGE = 1 << 62


@pytest.mark.parametrize("args,status", [
    (dict(off=OFF, k=0), _lib.ERR_INVALID_ARG),                    # grade < 1
    (dict(off=OFF, C=0), _lib.ERR_INVALID_ARG),                    # channels < 1
    (dict(off=OFF, dtype=7), _lib.ERR_INVALID_ARG),                # bad dtype
    (dict(off=None, rows=3), _lib.ERR_INVALID_ARG),                # null host offsets with rows > 0
    (dict(off=[1, 4, 10]), _lib.ERR_INVALID_ARG),                  # off[0] != 0
    (dict(off=[0, 5, 4, 10]), _lib.ERR_INVALID_ARG),               # a decreasing pair
    (dict(off=[0, 5, 10, 9]), _lib.ERR_INVALID_ARG),               # ... the last one
    (dict(off=OFF, doff=0), _lib.ERR_INVALID_ARG),                 # null device offsets with work to do
    (dict(off=OFF, din=0), _lib.ERR_INVALID_ARG),                  # null input with work to do
    (dict(off=OFF, dout=0), _lib.ERR_INVALID_ARG),
    (dict(off=OFF, din=18), _lib.ERR_MISALIGNED),                  # fp32 view not 4-B aligned
    (dict(off=OFF, dout=22), _lib.ERR_MISALIGNED),
    (dict(off=OFF, dtype=_lib.I16, din=21), _lib.ERR_MISALIGNED),  # int16 view not 2-B aligned
    (dict(off=OFF, doff=20), _lib.ERR_MISALIGNED),                 # device offsets at address 20: not 8-B aligned
    (dict(off=[0, HUGE]), _lib.ERR_UNSUPPORTED),                   # 2^62 frames
    (dict(off=[0, 1 << 50]), _lib.ERR_UNSUPPORTED),                # the scan's one launch past grid_too_large
    (dict(off=[0, 1 << 50], C=3), _lib.ERR_UNSUPPORTED),           # the loop's row past one launch
    (dict(off=[0], din=0, dout=0, doff=0), _lib.OK),               # rows == 0 is a no-op
    (dict(off=None, rows=0, din=0, dout=0, doff=0), _lib.OK),      # ... also without host offsets
    (dict(off=[0, 0, 0, 0], din=0, dout=0, doff=0), _lib.OK),      # all rows empty
    (dict(off=[0], k=0, din=0, dout=0, doff=0), _lib.ERR_INVALID_ARG),        # validated before the no-op
    (dict(off=[0, 0, 0], C=0, din=0, dout=0, doff=0), _lib.ERR_INVALID_ARG),
    (dict(off=[0, 0, -1], din=0, dout=0, doff=0), _lib.ERR_INVALID_ARG),      # decreasing, even with no frames
])
def test_ragged_run_validates_before_launch(args, status):
    assert _run(**args) == status


def test_ragged_plan_and_workspace_validate():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    out = ctypes.c_size_t(7)
    off = _arr(OFF)
    assert lib.mavg_ragged_plan(off, 3, 1, 3, _lib.F32, None, 0) == _lib.ERR_INVALID_ARG
    assert lib.mavg_ragged_plan(off, 0, 1, 3, _lib.F32, buf, len(buf)) == _lib.ERR_INVALID_ARG  # as mavg_plan
    assert lib.mavg_ragged_plan(_arr([0, 0, 0]), 2, 1, 3, _lib.F32, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_ragged_plan(off, 3, 1, 0, _lib.F32, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_ragged_plan(None, 3, 1, 3, _lib.F32, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_ragged_plan(_arr([0, 3, 2]), 2, 1, 3, _lib.F32, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_ragged_plan(_arr([0, HUGE]), 1, 1, 3, _lib.F32, buf, len(buf)) == _lib.ERR_UNSUPPORTED
    assert lib.mavg_ragged_workspace_bytes(off, 3, 1, 3, _lib.F32, None) == _lib.ERR_INVALID_ARG
    assert lib.mavg_ragged_workspace_bytes(off, 3, 0, 3, _lib.F32, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_ragged_workspace_bytes(_arr([1, 2]), 1, 1, 3, _lib.F32, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_ragged_workspace_bytes(None, 0, 1, 3, _lib.F32, ctypes.byref(out)) == _lib.OK and out.value == 0


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])


LENGTHS = [1000, 3, 0, 0, 517, 1, 999]  # 7 rows, 2520 frames, the longest 1000

FAST = [  # (lengths, channels, grade, dtype)
    (LENGTHS, 1, 64, _lib.F32),
    (LENGTHS, 2, 64, _lib.I16),
    (LENGTHS, 1, 100000, _lib.F32),   # effective halo min(grade, max_row_frames) = 1000 frames
    (LENGTHS, 1, 65535, _lib.I16),
]
SLOW = [
    (LENGTHS, 3, 64, _lib.F32),                  # three channels
    (LENGTHS, 1, 70000, _lib.I16),               # past int32 sums / the exact-division helpers' domain
    ([20000, 3, 0, 15000], 1, 20000, _lib.F32),  # window and longest row both past the LDS halo
]


@pytest.mark.parametrize("lengths,C,k,dt", FAST)
def test_scan_plan_and_workspace(lengths, C, k, dt):
    off = _offsets(lengths)
    R, N, M = len(lengths), int(off[-1]), max(lengths)
    p = dsp.ragged_plan(off, k, C, dt)
    assert p.startswith(SCAN + ("f32" if dt == _lib.F32 else "i16")), p
    m = re.search(r" tile_frames=(\d+) ", p)
    assert m and int(m.group(1)) > 0, p
    assert f" rows={R} " in p and f" frames={N} " in p and f" max_row_frames={M} " in p, p
    assert f" window={min(k, M)} " in p, p
    assert dsp.ragged_workspace_bytes(off, k, C, dt) == 0


@pytest.mark.parametrize("lengths,C,k,dt", SLOW)
def test_loop_plan_and_workspace(lengths, C, k, dt):
    off = _offsets(lengths)
    R, M = len(lengths), max(lengths)
    p = dsp.ragged_plan(off, k, C, dt)
    assert p == f"ragged_loop rows={R} max_row_frames={M} x " + dsp.plan(M * C, k, C, dt), p
    # all rows share one workspace: the longest row's
    assert dsp.ragged_workspace_bytes(off, k, C, dt) == dsp.workspace_bytes(M * C, k, C, dt)


def test_loop_workspace_is_positive_for_long_windows():
    off = _offsets([20000, 3, 0, 15000])
    assert dsp.ragged_workspace_bytes(off, 20000, 1, _lib.F32) > 0
    assert dsp.ragged_workspace_bytes(off, 5000, 1, _lib.F32) > 0
    assert dsp.ragged_plan(off, 5000, 1, _lib.F32).startswith("ragged_loop rows=4 max_row_frames=20000 x ahead_scan<")


def test_scan_boundary_is_the_lds_halo():
    """The scan takes effective halos min(grade, max_row_frames) up to 16 KiB, as rows_scan; one
    more frame in the longest row goes to the loop.  Bisection on max_row_frames with a grade
    past every row: the effective halo is the longest row."""
    for dt, C in ((_lib.F32, 1), (_lib.F32, 2), (_lib.I16, 1), (_lib.I16, 2)):
        k = 1 << 20 if dt == _lib.F32 else 65535
        plan = lambda M: dsp.ragged_plan(_offsets([5, M, 0, 77]), k, C, dt)
        lo, hi = 77, 1 << 15
        assert plan(lo).startswith(SCAN) and plan(hi).startswith(LOOP)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if plan(mid).startswith(SCAN):
                lo = mid
            else:
                hi = mid
        assert lo * C * (4 if dt == _lib.F32 else 2) == 16 * 1024, (dt, C, lo)
        assert 2 * 32768 * lo < 2 ** 31
        p = plan(lo)
        assert f" max_row_frames={lo} " in p and f" window={lo} " in p, p
        assert int(re.search(r" lds=(\d+) ", p).group(1)) <= 64 * 1024
        # the same boundary on the grade when a row is longer than the window
        big = _offsets([5, 1 << 20, 0, 77])
        assert dsp.ragged_plan(big, lo, C, dt).startswith(SCAN)
        assert dsp.ragged_plan(big, lo + 1, C, dt).startswith(LOOP)


def test_no_long_row_rule():
    """rows_scan's 64-MiB-row rule is not carried over: one huge row among small ones stays on the scan."""
    off = _offsets([250] * 8 + [1 << 26] + [250] * 8)
    assert dsp.rows_plan(8, 1 << 26, 1024, 1, _lib.F32).startswith("rows_loop")
    assert dsp.ragged_plan(off, 1024, 1, _lib.F32).startswith(SCAN)


def test_k1_is_the_flat_copy():
    off = _offsets(LENGTHS)
    p = dsp.ragged_plan(off, 1, 1, _lib.F32)
    assert p.startswith("ragged_scan<f32,C=1,k=1>") and "copy<f32,C=1>" in p and " window=1 " in p, p
    assert dsp.ragged_plan(off, 1, 2, _lib.I16).startswith("ragged_scan<i16,C=2,k=1>")
    assert dsp.ragged_workspace_bytes(off, 1, 1, _lib.F32) == 0


def test_plan_accepts_tensors_sequences_and_arrays():
    import torch
    off = _offsets(LENGTHS)
    want = dsp.ragged_plan(off, 64)
    assert dsp.ragged_plan([int(v) for v in off], 64) == want
    assert dsp.ragged_plan(tuple(int(v) for v in off), 64) == want
    assert dsp.ragged_plan(torch.from_numpy(off), 64) == want
    assert dsp.ragged_plan(off.astype(np.int32), 64) == want


def test_wrapper_argument_errors():
    import torch
    x = torch.zeros(10)
    with pytest.raises(ValueError, match="device tensor"):
        dsp.moving_average_ragged(x, 8, lengths=[4, 6])              # a CPU tensor
    with pytest.raises(ValueError, match="device tensor"):
        dsp.moving_average_ragged_into(x, torch.zeros(10), 8, lengths=[4, 6])
    with pytest.raises(ValueError, match=r"\[frames, 2\]"):
        dsp.moving_average_ragged(torch.zeros(10, 3), 8, lengths=[10], channels=2)  # last dimension != channels
    with pytest.raises(ValueError, match=r"\[frames\]"):
        dsp.moving_average_ragged(torch.zeros(2, 5), 8, lengths=[10])                # not the packed stream
    with pytest.raises(ValueError, match="channels must be"):
        dsp.moving_average_ragged(x, 8, lengths=[10], channels=0)
    # the offsets themselves (checked before any device work: _host_offsets)
    f = dsp._host_offsets
    with pytest.raises(ValueError, match="exactly one"):
        f(None, None)
    with pytest.raises(ValueError, match="exactly one"):
        f([0, 10], [10])
    with pytest.raises(ValueError, match="start at 0"):
        f([1, 10], None)
    with pytest.raises(ValueError, match="non-decreasing"):
        f([0, 6, 4, 10], None)
    with pytest.raises(ValueError, match="rows \\+ 1 entries"):
        f([], None)
    with pytest.raises(ValueError, match=">= 0"):
        f(None, [4, -1, 7])
    with pytest.raises(ValueError, match="integers"):
        f([0.0, 10.0], None)
    with pytest.raises(ValueError, match="one-dimensional"):
        f([[0, 10]], None)
    assert f(None, [4, 0, 6]).tolist() == [0, 4, 4, 10] and f(None, []).tolist() == [0]
    assert f(np.array([0, 4, 10]), None).dtype == torch.int64
    for name in ("moving_average_ragged", "moving_average_ragged_into", "ragged_plan", "ragged_workspace_bytes"):
        assert name in dsp.__all__ and callable(getattr(dsp, name))
