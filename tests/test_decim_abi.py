"""CPU tests of the decimated moving average's ABI (mavg_decim_run, mavg_decim_out_frames,
mavg_decim_workspace_bytes, mavg_decim_plan, include/mavg.h; mavg_debug_force_decim,
include/mavg_debug.h): the symbols, the output-frame count, the status table with dummy pointers,
the dispatch rule as the plan text shows it, the workspace sizes and the wrappers' argument
checks.  No GPU."""
import ctypes
import os
import subprocess
import sys

import pytest

import digital_signal_processsing_amd as dsp
from digital_signal_processsing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECIM_SYMBOLS = ("mavg_decim_run", "mavg_decim_out_frames", "mavg_decim_workspace_bytes", "mavg_decim_plan")
HOOK = "mavg_debug_force_decim"
F32, I16 = _lib.F32, _lib.I16


def test_decim_symbols_are_exported_by_release_and_debug():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        lib = _lib.load(path)
        for name in DECIM_SYMBOLS:
            assert hasattr(lib, name), (path, name)
        assert lib.mavg_abi_version() == _lib.ABI_VERSION == 4  # additive: the version stays
    assert set(DECIM_SYMBOLS) <= set(_lib.EXPORTED_SYMBOLS)
    assert not hasattr(_lib.load(), HOOK)                       # the release build has no hook
    assert hasattr(_lib.load(_lib.DEBUG_LIB_PATH), HOOK) and HOOK in _lib.DEBUG_SYMBOLS
    lib = _lib.load()
    assert len(lib.mavg_decim_run.argtypes) == 12
    assert len(lib.mavg_decim_out_frames.argtypes) == 4
    assert len(lib.mavg_decim_workspace_bytes.argtypes) == 7
    assert len(lib.mavg_decim_plan.argtypes) == 8


def test_out_frames_is_len_of_range():
    lib = _lib.load()
    out = ctypes.c_size_t(99)
    for hop in (1, 2, 3, 7, 160, 1000):
        for phase in sorted({0, hop // 2, hop - 1}):
            # n <= phase, n == phase + 1, hop > n, hop == 1 and the general case
            for n in (0, 1, phase, phase + 1, phase + 2, hop - 1, hop, hop + 1, 999, 1000, 1001, 12345, (1 << 40) + 3):
                if n < 0:
                    continue
                assert lib.mavg_decim_out_frames(n, hop, phase, ctypes.byref(out)) == _lib.OK
                assert out.value == len(range(phase, n, hop)), (n, hop, phase)
                assert dsp.decim_out_frames(n, hop, phase) == out.value
    assert lib.mavg_decim_out_frames(10, 0, 0, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_decim_out_frames(10, 3, 3, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_decim_out_frames(10, 3, -1, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_decim_out_frames(10, 3, 0, None) == _lib.ERR_INVALID_ARG


def _run(n, C, k, hop, phase=0, dtype=F32, din=16, dout=32, hist=None, ws=None, ws_bytes=0):
    return _lib.load().mavg_decim_run(din, dout, n, C, k, hop, phase, dtype, hist, ws, ws_bytes, None)


@pytest.mark.parametrize("args,status", [
    (dict(n=100, C=1, k=3, hop=0), _lib.ERR_INVALID_ARG),             # hop < 1
    (dict(n=100, C=1, k=3, hop=-2), _lib.ERR_INVALID_ARG),
    (dict(n=100, C=1, k=3, hop=4, phase=4), _lib.ERR_INVALID_ARG),    # phase outside [0, hop)
    (dict(n=100, C=1, k=3, hop=4, phase=-1), _lib.ERR_INVALID_ARG),
    (dict(n=100, C=1, k=3, hop=1, phase=1), _lib.ERR_INVALID_ARG),
    (dict(n=100, C=1, k=0, hop=2), _lib.ERR_INVALID_ARG),             # mavg_run's: grade < 1
    (dict(n=100, C=0, k=3, hop=2), _lib.ERR_INVALID_ARG),             # channels < 1
    (dict(n=9, C=2, k=3, hop=2), _lib.ERR_INVALID_ARG),               # a partial frame
    (dict(n=100, C=1, k=3, hop=2, dtype=7), _lib.ERR_INVALID_ARG),    # bad dtype
    (dict(n=100, C=1, k=3, hop=2, din=0), _lib.ERR_INVALID_ARG),      # null input with work to do
    (dict(n=100, C=1, k=3, hop=2, dout=0), _lib.ERR_INVALID_ARG),
    (dict(n=100, C=1, k=3, hop=2, din=18), _lib.ERR_MISALIGNED),      # fp32 view not 4-B aligned
    (dict(n=100, C=1, k=3, hop=2, dout=22), _lib.ERR_MISALIGNED),
    (dict(n=100, C=1, k=3, hop=2, dtype=I16, din=21), _lib.ERR_MISALIGNED),
    (dict(n=100, C=1, k=3, hop=2, hist=19), _lib.ERR_MISALIGNED),     # history not sample-aligned
    (dict(n=0, C=1, k=3, hop=2, din=0, dout=0), _lib.OK),             # M == 0: nothing to do
    (dict(n=5, C=1, k=3, hop=9, phase=5, din=0, dout=0), _lib.OK),    # n_frames <= phase
    (dict(n=0, C=1, k=3, hop=0, din=0, dout=0), _lib.ERR_INVALID_ARG),  # validated before the no-op
    (dict(n=3 << 20, C=3, k=64, hop=16), _lib.ERR_WORKSPACE),         # decim_full without its workspace
    (dict(n=1 << 20, C=1, k=8192, hop=160, ws=1 << 22, ws_bytes=1 << 20), _lib.ERR_WORKSPACE),
    (dict(n=1 << 20, C=1, k=8192, hop=160, ws=(1 << 22) + 4, ws_bytes=1 << 30), _lib.ERR_MISALIGNED),
])
def test_decim_run_validates_before_launch(args, status):
    assert _run(**args) == status


def test_plan_and_workspace_validate():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    out = ctypes.c_size_t(7)
    assert lib.mavg_decim_plan(100, 1, 3, 2, 0, F32, None, 0) == _lib.ERR_INVALID_ARG
    assert lib.mavg_decim_plan(0, 1, 3, 2, 0, F32, buf, len(buf)) == _lib.ERR_INVALID_ARG   # as mavg_plan
    assert lib.mavg_decim_plan(5, 1, 3, 9, 5, F32, buf, len(buf)) == _lib.ERR_INVALID_ARG   # M == 0
    assert lib.mavg_decim_plan(100, 1, 3, 0, 0, F32, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_decim_plan(100, 1, 3, 2, 2, F32, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_decim_plan(100, 1, 0, 2, 0, F32, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_decim_workspace_bytes(100, 1, 3, 2, 0, F32, None) == _lib.ERR_INVALID_ARG
    assert lib.mavg_decim_workspace_bytes(100, 1, 3, 0, 0, F32, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_decim_workspace_bytes(100, 0, 3, 2, 0, F32, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_decim_workspace_bytes(0, 1, 3, 2, 0, F32, ctypes.byref(out)) == _lib.OK and out.value == 0


N = 1 << 22  # samples per channel count below: n = N * C

# (dtype, C, grade, hop) -> the plan's family token.  One row per dispatch branch and the
# neighbours of each threshold.
PLAN_TABLE = [
    # hop == 1: mavg_run itself
    (F32, 1, 1024, 1, "decim_none x tile_scan<"),
    (I16, 3, 7, 1, "decim_none x tile_scan<"),
    # fp32 mono grade=256, hop=512 sits on both window thresholds (1 KiB, 2 * grade) at once
    (F32, 1, 256, 512, "decim_window<f32,acc=f64,C=1,"),
    (F32, 1, 255, 512, "decim_scan<f32,"),      # below 1 KiB
    (F32, 1, 256, 511, "decim_scan<f32,"),      # below 2 * grade
    (F32, 1, 256, 513, "decim_window<"),
    (F32, 1, 257, 514, "decim_window<"),
    (I16, 2, 256, 512, "decim_window<i16,acc=i64,C=2,"),   # 256 * 2 * 2 B = 1 KiB
    (I16, 2, 255, 512, "decim_scan<i16,"),
    (I16, 1, 512, 1024, "decim_window<i16,acc=i64,C=1,"),
    (I16, 1, 511, 1024, "decim_scan<i16,"),
    # windows of 4 KiB and more are the window sum's from hop == grade on (measured)
    (F32, 1, 1024, 1024, "decim_window<f32,"),
    (F32, 1, 1023, 1023, "decim_scan<f32,"),    # 4092 B at hop == grade
    (F32, 1, 1024, 1023, "decim_scan<f32,"),    # overlapping windows
    (I16, 2, 1024, 1024, "decim_window<i16,"),
    (I16, 2, 1023, 2045, "decim_scan<i16,"),
    (I16, 2, 1023, 2046, "decim_window<i16,"),
    (F32, 1, 2048, 3000, "decim_window<f32,"),
    # dense reading: overlapping windows, block averaging with a small window, hop in [grade, 2 grade)
    (F32, 1, 1024, 2, "decim_scan<f32,acc=f64,C=1,F=4,U=2,"),
    (F32, 1, 400, 160, "decim_scan<f32,"),
    (I16, 2, 400, 160, "decim_scan<i16,acc=i32,C=2,F=4,U=4,"),
    (F32, 2, 256, 256, "decim_scan<f32,acc=f64,C=2,F=2,U=2,"),
    (F32, 1, 512, 512, "decim_scan<f32,"),
    (F32, 1, 4, 4, "decim_scan<f32,"),
    (F32, 1, 4, 9, "decim_scan<f32,"),          # hop > 2 * grade, window under 1 KiB
    (F32, 1, 200, 3000, "decim_scan<f32,"),     # hop > tile_frames: tiles that emit nothing
    (F32, 1, 2, 2, "decim_scan<f32,"),
    (F32, 1, 1, 2, "decim_full hop=2 phase=0 x copy<"),    # grade 1 is the copy, never a scan
    # 3+ channels: the window sum where it applies, else the fallback
    (F32, 3, 400, 400, "decim_window<f32,acc=f64,C=3,"),   # hop == grade, no scan for 3 channels
    (F32, 3, 400, 399, "decim_full hop=399 phase=0 x tile_scan<"),
    (F32, 3, 64, 16, "decim_full hop=16 phase=0 x tile_scan<"),
    (F32, 3, 64, 64, "decim_full hop=64 phase=0 x tile_scan<"),   # 768 B: a short window
    (F32, 8, 44100, 44100, "decim_window<f32,acc=f64,C=8,"),
    (I16, 8, 44100, 44100, "decim_window<i16,acc=i64,C=8,"),
    (F32, 9, 44100, 44100, "decim_full hop=44100 phase=0 x naive<"),   # more than 8 channels
    # int16 past int32 sums
    (I16, 1, 65535, 160, "decim_full hop=160 phase=0 x "),      # (a 128-KiB halo: past the scan's 16 KiB anyway)
    (I16, 1, 65536, 160, "decim_full hop=160 phase=0 x ahead_scan<i16,acc=i64"),
    (I16, 1, 65536, 65536, "decim_window<i16,acc=i64,C=1,"),
    (I16, 1, 70000, 70000, "decim_window<i16,"),
    # the scan's halo limit, narrowed by measurement from rows_scan's 16 KiB: 8 KiB against 8 KiB
    # plus one frame (16 KiB and one frame more are the fallback's as well)
    (F32, 1, 2048, 160, "decim_scan<f32,"),
    (F32, 1, 2049, 160, "decim_full hop=160 phase=0 x tile_scan<"),
    (F32, 1, 4096, 160, "decim_full hop=160 phase=0 x tile_scan<"),
    (F32, 1, 4097, 160, "decim_full hop=160 phase=0 x ahead_scan<"),
    (F32, 2, 1024, 160, "decim_scan<f32,"),
    (F32, 2, 1025, 160, "decim_full hop=160 phase=0 x "),
    (I16, 1, 4096, 160, "decim_scan<i16,"),
    (I16, 1, 4097, 160, "decim_full hop=160 phase=0 x "),
    (I16, 2, 2048, 160, "decim_scan<i16,"),
    (I16, 2, 2049, 160, "decim_full hop=160 phase=0 x "),
    (F32, 1, 2049, 2049, "decim_window<"),      # past the scan's halo with hop >= grade: sparse reading
    (F32, 1, 8192, 160, "decim_full hop=160 phase=0 x ahead_scan<f32"),   # the look-ahead plus its workspace
]


@pytest.mark.parametrize("dt,C,k,hop,token", PLAN_TABLE)
def test_plan_token_table(dt, C, k, hop, token):
    p = dsp.decim_plan(N * C, k, hop, 0, C, dt)
    assert p.startswith(token), p
    ws = dsp.decim_workspace_bytes(N * C, k, hop, 0, C, dt)
    if p.startswith(("decim_scan<", "decim_window<")):
        assert ws == 0, (p, ws)
        assert f" hop={hop} phase=0 out_frames={len(range(0, N, hop))} " in p, p
    elif p.startswith("decim_none"):
        assert p == "decim_none x " + dsp.plan(N * C, k, C, dt), p
        assert ws == dsp.workspace_bytes(N * C, k, C, dt)
    else:
        # the full-rate output, rounded up to 16 B, plus the full-rate run's own workspace
        assert p == f"decim_full hop={hop} phase=0 x " + dsp.plan(N * C, k, C, dt), p
        eb = 4 if dt == F32 else 2
        assert ws == (N * C * eb + 15) // 16 * 16 + dsp.workspace_bytes(N * C, k, C, dt), (p, ws)
    if "decim_scan<" in p:
        assert " tile_frames=" in p and " lds=" in p


def test_full_workspace_rounds_up_and_adds_the_look_ahead():
    n, k, hop = 1_000_003, 8192, 160
    inner = dsp.workspace_bytes(n, k)
    assert inner > 0
    assert dsp.decim_workspace_bytes(n, k, hop) == (n * 4 + 15) // 16 * 16 + inner
    assert dsp.decim_workspace_bytes(3 * 1001, 64, 16, 5, 3, I16) == (3 * 1001 * 2 + 15) // 16 * 16
    assert dsp.decim_plan(n, k, hop, 7).startswith("decim_full hop=160 phase=7 x ahead_scan<")


def test_phase_shows_in_the_plan_and_changes_no_path():
    for phase in (0, 80, 159):
        p = dsp.decim_plan(1 << 20, 400, 160, phase)
        assert p.startswith("decim_scan<") and f" phase={phase} out_frames={len(range(phase, 1 << 20, 160))} " in p, p


FORCE_CHILD = r'''
import sys
import digital_signal_processsing_amd as dsp
from digital_signal_processsing_amd import _lib
lib = _lib.load(_lib.DEBUG_LIB_PATH)
D = _lib.DEBUG_LIB_PATH
plan = lambda *a, **k: dsp.decim_plan(*a, library=D, **k)
assert lib.mavg_debug_force_decim(7) == _lib.ERR_INVALID_ARG and lib.mavg_debug_force_decim(-1) == _lib.ERR_INVALID_ARG
assert plan(1 << 20, 512, 512).startswith("decim_scan<")             # the rule
assert plan(1 << 20, 1024, 1024).startswith("decim_window<")
assert lib.mavg_debug_force_decim(_lib.DECIM_WINDOW) == _lib.OK
assert plan(1 << 20, 1024, 1024).startswith("decim_window<")
assert plan(1 << 20, 1024, 2).startswith("decim_window<")            # overlapping windows: it can, the rule never would
assert plan(1 << 20, 1024, 1).startswith("decim_none")               # hop == 1 stays mavg_run
try:
    plan(9 << 10, 64, 64, channels=9)
    raise SystemExit("forced window took 9 channels")
except dsp.MavgError as e:
    assert e.status == _lib.ERR_UNSUPPORTED
assert lib.mavg_debug_force_decim(_lib.DECIM_SCAN) == _lib.OK
assert plan(1 << 20, 1024, 4096).startswith("decim_scan<")
for kw in (dict(n=3 << 10, grade=64, hop=64, channels=3), dict(n=1 << 20, grade=4097, hop=4097)):
    try:
        plan(kw["n"], kw["grade"], kw["hop"], channels=kw.get("channels", 1))
        raise SystemExit("forced scan took a shape outside its range")
    except dsp.MavgError as e:
        assert e.status == _lib.ERR_UNSUPPORTED
    assert lib.mavg_decim_run(16, 32, kw["n"], kw.get("channels", 1), kw["grade"], kw["hop"], 0, _lib.F32, None, None, 0,
                              None) == _lib.ERR_UNSUPPORTED
assert lib.mavg_debug_force_decim(_lib.DECIM_FULL) == _lib.OK
assert plan(1 << 20, 1024, 4096).startswith("decim_full hop=4096 phase=0 x tile_scan<")
assert dsp.decim_workspace_bytes(1 << 20, 1024, 4096, library=D) == 4 << 20
assert lib.mavg_debug_force_decim(_lib.DECIM_AUTO) == _lib.OK
assert plan(1 << 20, 1024, 4096).startswith("decim_window<")
print("force hook ok")
'''


def test_force_hook_on_the_debug_build():
    """The hook is process-wide state: exercised in a child process of its own."""
    r = subprocess.run([sys.executable, "-c", FORCE_CHILD], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "force hook ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_wrappers_reject_host_tensors_bad_phase_and_wrong_out():
    import torch
    x = torch.zeros(1000)
    with pytest.raises(ValueError, match="device tensor"):
        dsp.moving_average_decimated(x, 8, 4)                       # a host tensor
    with pytest.raises(ValueError, match="device tensor"):
        dsp.moving_average_decimated_into(x, torch.zeros(250), 8, 4)
    for hop, phase in ((4, 4), (4, -1), (1, 1), (0, 0)):
        with pytest.raises(ValueError, match="phase must be|hop must be"):
            dsp.decim_plan(1000, 8, hop, phase)
        with pytest.raises(ValueError, match="phase must be|hop must be"):
            dsp.decim_workspace_bytes(1000, 8, hop, phase)
        with pytest.raises(ValueError, match="phase must be|hop must be|device tensor"):
            dsp.moving_average_decimated(x, 8, hop, phase)
    for m in (249, 251, 0):                                         # a wrong out size
        with pytest.raises(ValueError, match="out must hold"):
            dsp.moving_average_decimated_into(x, torch.zeros(m), 8, 4)
    with pytest.raises(ValueError, match="out must hold"):
        dsp.moving_average_decimated_into(torch.zeros(500, 2), torch.zeros(125, 3), 8, 4)
    with pytest.raises(ValueError, match="same dtype"):
        dsp.moving_average_decimated_into(x, torch.zeros(250, dtype=torch.int16), 8, 4)
    with pytest.raises(ValueError, match="multiple of channels"):
        dsp._decim_shape(torch.zeros(1001), 2)
    with pytest.raises(ValueError, match="frames, 2"):
        dsp._decim_shape(torch.zeros(100, 3), 2)
    assert dsp._decim_shape(torch.zeros(1000), 2) == (500, 2)
    assert dsp._decim_shape(torch.zeros(500, 2), 1) == (500, 2) and dsp._decim_shape(torch.zeros(500, 2), 2) == (500, 2)
    for name in ("moving_average_decimated", "moving_average_decimated_into", "decim_out_frames", "decim_plan",
                 "decim_workspace_bytes"):
        assert name in dsp.__all__ and callable(getattr(dsp, name))
