"""CPU tests of the batched rows API (mavg_rows_run, mavg_rows_workspace_bytes, mavg_rows_plan,
include/mavg.h): the symbols, the status table with dummy pointers, the dispatch rule as the
plan text shows it, the workspace sizes and the wrapper's argument checks.  No GPU."""
import ctypes
import os
import re

import pytest

import digital_signal_processsing_amd as dsp
from digital_signal_processsing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS_SYMBOLS = ("mavg_rows_run", "mavg_rows_workspace_bytes", "mavg_rows_plan")


def test_rows_symbols_are_exported_by_release_and_debug():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        lib = _lib.load(path)
        for name in ROWS_SYMBOLS:
            assert hasattr(lib, name), (path, name)
        assert lib.mavg_abi_version() == _lib.ABI_VERSION == 4  # additive: the version stays


def test_rows_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "mavg.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char\*)\s+(mavg_\w+)\s*\(", text, re.M))
    assert set(ROWS_SYMBOLS) <= declared
    assert set(ROWS_SYMBOLS) <= set(_lib.EXPORTED_SYMBOLS)
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    assert len(lib.mavg_rows_run.argtypes) == 11
    assert len(lib.mavg_rows_workspace_bytes.argtypes) == 7
    assert len(lib.mavg_rows_plan.argtypes) == 8


def _run(rows, L, C, k, dtype=_lib.F32, din=16, dout=32, hist=None):
    return _lib.load().mavg_rows_run(din, dout, rows, L, C, k, dtype, hist, None, 0, None)


@pytest.mark.parametrize("args,status", [
    (dict(rows=4, L=10, C=1, k=0), _lib.ERR_INVALID_ARG),            # grade < 1
    (dict(rows=4, L=10, C=0, k=3), _lib.ERR_INVALID_ARG),            # channels < 1
    (dict(rows=4, L=10, C=1, k=3, dtype=7), _lib.ERR_INVALID_ARG),   # bad dtype
    (dict(rows=4, L=10, C=1, k=3, din=0), _lib.ERR_INVALID_ARG),     # null input with work to do
    (dict(rows=4, L=10, C=1, k=3, dout=0), _lib.ERR_INVALID_ARG),
    (dict(rows=4, L=10, C=1, k=3, din=18), _lib.ERR_MISALIGNED),     # fp32 view not 4-B aligned
    (dict(rows=4, L=10, C=1, k=3, dout=22), _lib.ERR_MISALIGNED),
    (dict(rows=4, L=10, C=1, k=3, dtype=_lib.I16, din=21), _lib.ERR_MISALIGNED),  # int16 view not 2-B aligned
    (dict(rows=4, L=10, C=1, k=3, hist=19), _lib.ERR_MISALIGNED),    # history not sample-aligned
    (dict(rows=1 << 40, L=1 << 40, C=1, k=3), _lib.ERR_UNSUPPORTED),  # rows * row_frames overflows
    (dict(rows=1 << 31, L=1 << 31, C=1, k=3), _lib.ERR_UNSUPPORTED),  # 2^62 frames
    (dict(rows=1 << 40, L=1 << 10, C=1, k=3), _lib.ERR_UNSUPPORTED),  # the scan's one launch past grid_too_large
    (dict(rows=1 << 21, L=1 << 40, C=1, k=3), _lib.ERR_UNSUPPORTED),  # the loop's rows past one launch
    (dict(rows=0, L=10, C=1, k=3, din=0, dout=0), _lib.OK),           # empty input is a no-op
    (dict(rows=10, L=0, C=2, k=3, din=0, dout=0), _lib.OK),
    (dict(rows=0, L=10, C=1, k=0, din=0, dout=0), _lib.ERR_INVALID_ARG),  # validated before the no-op
])
def test_rows_run_validates_before_launch(args, status):
    assert _run(**args) == status


def test_rows_plan_and_workspace_validate():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    out = ctypes.c_size_t(7)
    assert lib.mavg_rows_plan(4, 10, 1, 3, _lib.F32, 0, None, 0) == _lib.ERR_INVALID_ARG
    assert lib.mavg_rows_plan(0, 10, 1, 3, _lib.F32, 0, buf, len(buf)) == _lib.ERR_INVALID_ARG  # as mavg_plan
    assert lib.mavg_rows_plan(4, 10, 1, 0, _lib.F32, 0, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_rows_plan(1 << 40, 1 << 40, 1, 3, _lib.F32, 0, buf, len(buf)) == _lib.ERR_UNSUPPORTED
    assert lib.mavg_rows_workspace_bytes(4, 10, 1, 3, _lib.F32, 0, None) == _lib.ERR_INVALID_ARG
    assert lib.mavg_rows_workspace_bytes(4, 10, 0, 3, _lib.F32, 0, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_rows_workspace_bytes(0, 10, 1, 3, _lib.F32, 0, ctypes.byref(out)) == _lib.OK and out.value == 0


FAST = [  # (rows, row_frames, channels, grade, dtype)
    (1024, 1000, 1, 64, _lib.F32),
    (1024, 1000, 1, 64, _lib.I16),
    (1024, 1000, 1, 100000, _lib.F32),   # effective halo min(grade, row_frames) = 1000 frames
]
LOOP = [  # (rows, row_frames, channels, grade, dtype, with_history)
    (1024, 1000, 1, 64, _lib.F32, True),
    (1024, 1000, 3, 64, _lib.F32, False),
    (3, 20000, 1, 20000, _lib.F32, False),  # window and row both past the LDS halo
    (1024, 1000, 1, 70000, _lib.I16, False),  # past int32 sums / the exact-division helpers' domain
]


@pytest.mark.parametrize("R,L,C,k,dt", FAST)
def test_fast_path_plan_and_workspace(R, L, C, k, dt):
    p = dsp.rows_plan(R, L, k, C, dt)
    assert p.startswith("rows_scan<" + ("f32" if dt == _lib.F32 else "i16")), p
    m = re.search(r" tile_frames=(\d+) ", p)
    assert m and int(m.group(1)) > 0 and f" rows={R} " in p and f" row_frames={L} " in p, p
    assert f" window={min(k, L)} " in p, p
    assert dsp.rows_workspace_bytes(R, L, k, C, dt) == 0


@pytest.mark.parametrize("R,L,C,k,dt,hist", LOOP)
def test_loop_plan_and_workspace(R, L, C, k, dt, hist):
    p = dsp.rows_plan(R, L, k, C, dt, with_history=hist)
    assert p == f"rows_loop rows={R} x " + dsp.plan(L * C, k, C, dt), p
    assert dsp.rows_workspace_bytes(R, L, k, C, dt, with_history=hist) == dsp.workspace_bytes(L * C, k, C, dt)


def test_loop_workspace_is_positive_for_long_windows():
    assert dsp.rows_workspace_bytes(3, 20000, 20000, 1, _lib.F32) > 0
    assert dsp.rows_workspace_bytes(3, 20000, 5000, 1, _lib.F32) > 0
    assert dsp.rows_plan(3, 20000, 5000, 1, _lib.F32).startswith("rows_loop rows=3 x ahead_scan<")


def test_fast_path_boundary_is_the_lds_halo():
    """The scan takes effective halos up to 16 KiB (where the single-signal dispatch leaves its
    LDS-staged tiles too); one more frame goes to the loop.  The stage fits the 64-KiB budget and
    int16 sums stay inside int32 there (2 * 32768 * window < 2^31)."""
    for dt, C in ((_lib.F32, 1), (_lib.F32, 2), (_lib.I16, 1), (_lib.I16, 2)):
        lo, hi = 1, 1 << 16
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if dsp.rows_plan(3, 1 << 20, mid, C, dt).startswith("rows_scan<"):
                lo = mid
            else:
                hi = mid
        assert dsp.rows_plan(3, 1 << 20, hi, C, dt).startswith("rows_loop"), (dt, C, hi)
        assert lo * C * (4 if dt == _lib.F32 else 2) == 16 * 1024, (dt, C, lo)
        assert 2 * 32768 * lo < 2 ** 31
        lds = int(re.search(r" lds=(\d+) ", dsp.rows_plan(3, 1 << 20, lo, C, dt)).group(1))
        assert lds <= 64 * 1024
        # the effective halo decides, not the grade: rows shorter than the window stay on the scan
        assert dsp.rows_plan(3, lo, 1 << 20 if dt == _lib.F32 else 65535, C, dt).startswith("rows_scan<")


def test_rows_of_64_mib_and_more_take_the_loop():
    """The measured boundary (DESIGN.md "Rows"): rows that fill the device by themselves run the
    single-signal kernels, one launch each."""
    for dt, C, eb in ((_lib.F32, 1, 4), (_lib.F32, 2, 4), (_lib.I16, 1, 2), (_lib.I16, 2, 2)):
        L = (64 << 20) // (eb * C)
        assert dsp.rows_plan(8, L - 1, 1024, C, dt).startswith("rows_scan<"), (dt, C)
        assert dsp.rows_plan(8, L, 1024, C, dt) == "rows_loop rows=8 x " + dsp.plan(L * C, 1024, C, dt), (dt, C)
        assert dsp.rows_workspace_bytes(8, L, 1024, C, dt) == 0  # the single-signal tiles need none either
        assert dsp.rows_plan(8, L, 1, C, dt).startswith("rows_scan<")  # grade 1 stays the one flat copy


def test_k1_is_the_flat_copy_on_the_fast_path():
    p = dsp.rows_plan(9, 1001, 1, 1, _lib.F32)
    assert p.startswith("rows_scan<f32,C=1,k=1>") and "copy<f32,C=1>" in p, p
    assert dsp.rows_workspace_bytes(9, 1001, 1, 1, _lib.F32) == 0


def test_wrapper_rejects_cpu_tensors_and_bad_shapes():
    import torch
    x = torch.zeros(4, 100)
    with pytest.raises(ValueError, match="device tensor"):
        dsp.moving_average_rows(x, 8)                      # a CPU tensor
    with pytest.raises(ValueError, match="device tensor"):
        dsp.moving_average_rows_into(x, torch.zeros(4, 100), 8)
    with pytest.raises(ValueError, match="time, 2"):
        dsp.moving_average_rows(torch.zeros(4, 100, 3), 8, channels=2)  # last dimension != channels
    with pytest.raises(ValueError, match="time, 2"):
        dsp.moving_average_rows(torch.zeros(100), 8, channels=2)        # no time dimension
    with pytest.raises(ValueError, match="time dimension"):
        dsp.moving_average_rows(torch.zeros(()), 8)
    with pytest.raises(ValueError, match="channels must be"):
        dsp.moving_average_rows(x, 8, channels=0)
    for name in ("moving_average_rows", "moving_average_rows_into", "rows_plan", "rows_workspace_bytes"):
        assert name in dsp.__all__ and callable(getattr(dsp, name))


def test_rows_shape_rule():
    import torch
    f = dsp._rows_shape
    assert f(torch.zeros(2, 500), 1) == (2, 500)            # planar [C, T] / batch [B, T]
    assert f(torch.zeros(2, 3, 500), 1) == (6, 500)         # [B, C, T]
    assert f(torch.zeros(4, 500, 2), 2) == (4, 500)         # [B, T, C]
    assert f(torch.zeros(500, 2), 2) == (1, 500)
    assert f(torch.zeros(500), 1) == (1, 500)
    assert f(torch.zeros(0, 500), 1) == (0, 500)
    assert f(torch.zeros(3, 0), 1) == (0, 0)
