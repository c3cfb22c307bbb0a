"""CPU tests of the moving second moment's ABI (mavg_stat_run, mavg_stat_plan, include/mavg.h;
mavg_debug_force_stat, include/mavg_debug.h): the symbols, the status table with dummy pointers, the
dispatch rule as the plan text shows it -- each boundary on both sides -- and the wrappers'
argument checks.  No GPU.

The rule is a halo grade * channels * sample size of at most 16 KiB: the tile kernel measured faster
than the strip over that whole range (DESIGN.md "Moments"), so the boundaries are the starting ones."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

import digital_signal_processsing_amd as dsp
from digital_signal_processsing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAT_SYMBOLS = ("mavg_stat_run", "mavg_stat_plan")
HOOK = "mavg_debug_force_stat"
F32, I16 = _lib.F32, _lib.I16
TILE, STRIP = "stat_tile<", "stat_strip "


def test_stat_symbols_are_exported_by_release_and_debug():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        lib = _lib.load(path)
        for name in STAT_SYMBOLS:
            assert hasattr(lib, name), (path, name)
        assert lib.mavg_abi_version() == _lib.ABI_VERSION == 4  # additive: the version stays
    assert set(STAT_SYMBOLS) <= set(_lib.EXPORTED_SYMBOLS)
    assert not hasattr(_lib.load(), HOOK)                       # the release build has no hook
    assert hasattr(_lib.load(_lib.DEBUG_LIB_PATH), HOOK) and HOOK in _lib.DEBUG_SYMBOLS
    assert hasattr(_lib.load(_lib.HOOKS_LIB_PATH), HOOK)
    assert (_lib.STAT_AUTO, _lib.STAT_TILE, _lib.STAT_STRIP) == (0, 1, 2)
    assert (_lib.STAT_MEANSQ, _lib.STAT_RMS, _lib.STAT_VAR, _lib.STAT_STD) == (0, 1, 2, 3)
    assert dsp.STATS == {"meansq": 0, "rms": 1, "var": 2, "std": 3}
    lib = _lib.load()
    assert len(lib.mavg_stat_run.argtypes) == 10
    assert len(lib.mavg_stat_plan.argtypes) == 8


def test_header_declares_the_enum_and_strerror_is_unchanged():
    with open(os.path.join(ROOT, "include", "mavg.h")) as f:
        h = f.read()
    m = re.search(r"typedef enum \{([^}]*)\} mavg_stat;", h)
    assert m, "mavg_stat enum"
    vals = dict(re.findall(r"(MAVG_STAT_\w+)\s*=\s*(\d+)", m.group(1)))
    assert vals == {"MAVG_STAT_MEANSQ": "0", "MAVG_STAT_RMS": "1", "MAVG_STAT_VAR": "2", "MAVG_STAT_STD": "3"}
    block = h[h.index("Moving second moment"):h.index("} mavg_stat;")]
    assert "NOT tested past 2^31 samples" not in block and "tests/test_gpu_bigsignal.py" in block
    assert [_lib.strerror(s) for s in range(7)] == [
        "ok", "invalid argument", "unsupported configuration", "pointer not aligned to the sample size",
        "workspace too small", "HIP runtime error", "unknown status"]


def _run(n, C, k, stat=_lib.STAT_VAR, dtype=F32, din=16, dout=1 << 30, dmean=None, hist=None):
    return _lib.load().mavg_stat_run(din, dout, dmean, n, C, k, stat, dtype, hist, None)


@pytest.mark.parametrize("args,status", [
    (dict(n=100, C=1, k=3, stat=4), _lib.ERR_INVALID_ARG),               # bad stat
    (dict(n=100, C=1, k=3, stat=-1), _lib.ERR_INVALID_ARG),
    (dict(n=100, C=1, k=3, dtype=7), _lib.ERR_INVALID_ARG),              # bad dtype
    (dict(n=100, C=0, k=3), _lib.ERR_INVALID_ARG),                       # channels < 1
    (dict(n=100, C=1, k=0), _lib.ERR_INVALID_ARG),                       # grade < 1
    (dict(n=9, C=2, k=3), _lib.ERR_INVALID_ARG),                         # a partial frame
    (dict(n=100, C=1, k=3, din=0), _lib.ERR_INVALID_ARG),                # null input with work to do
    (dict(n=100, C=1, k=3, dout=0), _lib.ERR_INVALID_ARG),
    (dict(n=100, C=1, k=3, din=18), _lib.ERR_MISALIGNED),                # fp32 input off 4 B
    (dict(n=100, C=1, k=3, dtype=I16, din=21), _lib.ERR_MISALIGNED),     # int16 input off 2 B
    (dict(n=100, C=1, k=3, dtype=I16, dout=(1 << 30) + 2), _lib.ERR_MISALIGNED),   # the output is fp32: 4 B
    (dict(n=100, C=1, k=3, dout=(1 << 30) + 6), _lib.ERR_MISALIGNED),
    (dict(n=100, C=1, k=3, dmean=(1 << 29) + 2), _lib.ERR_MISALIGNED),   # d_mean off 4 B
    (dict(n=100, C=1, k=3, dtype=I16, dmean=(1 << 29) + 1), _lib.ERR_MISALIGNED),
    (dict(n=100, C=1, k=3, hist=19), _lib.ERR_MISALIGNED),               # history not sample-aligned
    (dict(n=0, C=1, k=3, din=0, dout=0), _lib.OK),                       # nothing to do
    (dict(n=0, C=1, k=3, stat=9, din=0, dout=0), _lib.ERR_INVALID_ARG),  # validated before the no-op
    # past the one-launch limit: the strip's one thread per (L = 16 frames, channel), 2^37 frames
    (dict(n=1 << 37, C=1, k=1), _lib.ERR_UNSUPPORTED),
    # the frame-unit tile form (4 frames per thread) from 2^34 frames; the 16-B-unit form still runs there
    (dict(n=1 << 34, C=1, k=64, din=20), _lib.ERR_UNSUPPORTED),
])
def test_stat_run_validates_before_launch(args, status):
    assert _run(**args) == status


def test_plan_validates():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    assert lib.mavg_stat_plan(100, 1, 3, 0, F32, 0, None, 0) == _lib.ERR_INVALID_ARG
    assert lib.mavg_stat_plan(0, 1, 3, 0, F32, 0, buf, len(buf)) == _lib.ERR_INVALID_ARG   # as mavg_plan
    assert lib.mavg_stat_plan(100, 1, 3, 4, F32, 0, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_stat_plan(100, 1, 0, 0, F32, 0, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_stat_plan(100, 0, 3, 0, F32, 0, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_stat_plan(1 << 37, 1, 1, 0, F32, 0, buf, len(buf)) == _lib.ERR_UNSUPPORTED
    assert lib.mavg_stat_plan(1 << 34, 1, 64, 0, F32, 0, buf, len(buf)) == _lib.OK and buf.value.startswith(b"stat_tile<")


N = 1 << 22  # frames below: n = N * C samples

# (dtype, C, grade) -> the plan's family token: each rule boundary on both sides
PLAN_TABLE = [
    (F32, 1, 4096, "stat_tile<f32,acc=f64/f64,C=1,F=4,U=2,"), (F32, 1, 4097, STRIP),     # 16 KiB of fp32 mono
    (F32, 2, 2048, "stat_tile<f32,acc=f64/f64,C=2,F=2,U=2,"), (F32, 2, 2049, STRIP),
    (I16, 1, 8192, "stat_tile<i16,acc=i32/i64,C=1,F=8,U=4,"), (I16, 1, 8193, STRIP),
    (I16, 2, 4096, "stat_tile<i16,acc=i32/i64,C=2,F=4,U=4,"), (I16, 2, 4097, STRIP),
    (F32, 3, 100, STRIP), (I16, 3, 100, STRIP), (F32, 8, 100, STRIP), (F32, 9, 7, STRIP),   # three or more channels
    (I16, 1, 65535, STRIP), (I16, 1, 65536, STRIP),                                         # past the halo; past int32 S1
    (F32, 1, 1, STRIP), (I16, 2, 1, STRIP),                                                 # grade == 1
    (F32, 1, 2, TILE), (I16, 1, 2, TILE), (F32, 2, 2, TILE), (I16, 2, 2, TILE),
    (F32, 1, 44100, STRIP), (I16, 1, 44100, STRIP),
]


@pytest.mark.parametrize("dt,C,k,token", PLAN_TABLE)
def test_plan_token_table(dt, C, k, token):
    for stat in range(4):
        for with_mean in (False, True):
            plan = dsp.stat_plan(N * C, k, stat, C, dt, with_mean)
            assert plan.startswith(token), plan
            assert f" stat={stat} mean={int(with_mean)} " in plan, plan
            if plan.startswith(TILE):
                # S2 alone for the mean square and the RMS without a mean; else both moments
                two = stat >= 2 or with_mean
                assert f",M={2 if two else 1}," in plan, plan
                assert f" halo_frames={k} " in plan and " tile_frames=" in plan, plan
                assert int(plan.split(" lds=")[1].split()[0]) <= 64 * 1024, plan
            else:
                L = min(max(k // 4, 16), 2048)
                assert f" grade={k} L={L} strips={(N + L - 1) // L} " in plan, plan
    assert dsp.stat_plan(N * C, k, "std", C, dt) == dsp.stat_plan(N * C, k, _lib.STAT_STD, C, dt)


FORCE_CHILD = r'''
import digital_signal_processsing_amd as dsp
from digital_signal_processsing_amd import _lib
lib = _lib.load(_lib.DEBUG_LIB_PATH)
D = _lib.DEBUG_LIB_PATH
plan = lambda *a, **k: dsp.stat_plan(*a, library=D, **k)
assert lib.mavg_debug_force_stat(3) == _lib.ERR_INVALID_ARG and lib.mavg_debug_force_stat(-1) == _lib.ERR_INVALID_ARG
assert plan(1 << 20, 100, "std").startswith("stat_tile<")            # the rule
assert plan(3 << 20, 100, "std", 3).startswith("stat_strip ")
assert lib.mavg_debug_force_stat(_lib.STAT_STRIP) == _lib.OK
assert plan(1 << 20, 100, "std").startswith("stat_strip ")
assert plan(1 << 20, 2, "rms", 2, _lib.I16).startswith("stat_strip ")
assert lib.mavg_debug_force_stat(_lib.STAT_TILE) == _lib.OK
assert plan(1 << 20, 100, "std").startswith("stat_tile<")
for kw in (dict(n=3 << 10, grade=33, channels=3), dict(n=1 << 20, grade=65536, dtype=_lib.I16), dict(n=1 << 20, grade=4097),
           dict(n=1 << 20, grade=1), dict(n=1 << 20, grade=8193, dtype=_lib.I16)):
    a = (kw["n"], kw["grade"], "var", kw.get("channels", 1), kw.get("dtype", _lib.F32))
    try:
        plan(*a)
        raise SystemExit("forced tile took a shape outside its range")
    except dsp.MavgError as e:
        assert e.status == _lib.ERR_UNSUPPORTED
    assert lib.mavg_stat_run(16, 1 << 30, None, a[0], a[3], a[1], 2, a[4], None, None) == _lib.ERR_UNSUPPORTED
assert lib.mavg_debug_force_stat(_lib.STAT_AUTO) == _lib.OK
assert plan(1 << 20, 4097, "var").startswith("stat_strip ") and plan(1 << 20, 4096, "var").startswith("stat_tile<")
print("force hook ok")
'''


def test_force_hook_on_the_debug_build():
    """The hook is process-wide state: exercised in a child process of its own."""
    r = subprocess.run([sys.executable, "-c", FORCE_CHILD], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "force hook ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_wrappers_check_their_arguments():
    import torch
    x = torch.zeros(1000)
    with pytest.raises(ValueError, match="device tensor"):
        dsp.moving_stat(x, 8, "rms")                                  # a host tensor
    with pytest.raises(ValueError, match="device tensor"):
        dsp.moving_stat_into(x, torch.zeros(1000), 8, "rms")
    for name in ("moving_rms", "moving_variance", "moving_std", "moving_mean_square"):
        with pytest.raises(ValueError, match="device tensor"):
            getattr(dsp, name)(x, 8)
    for stat in ("variance", 4, -1, None, True):
        with pytest.raises(ValueError, match="unknown stat"):
            dsp.stat_plan(1000, 8, stat)
        with pytest.raises(ValueError, match="unknown stat|device tensor"):
            dsp.moving_stat(x, 8, stat)
        with pytest.raises(ValueError, match="unknown stat"):
            dsp.moving_stat_into(x, torch.zeros(1000), 8, stat)
    for m in (999, 1001, 0):                                          # a wrong out size
        with pytest.raises(ValueError, match="out must hold"):
            dsp.moving_stat_into(x, torch.zeros(m), 8, "var")
    with pytest.raises(ValueError, match="mean_out must hold"):
        dsp.moving_stat_into(x, torch.zeros(1000), 8, "var", mean_out=torch.zeros(999))
    with pytest.raises(ValueError, match="out must be float32"):      # the output is fp32 for int16 input too
        dsp.moving_stat_into(torch.zeros(1000, dtype=torch.int16), torch.zeros(1000, dtype=torch.int16), 8, "var")
    with pytest.raises(ValueError, match="mean_out must be float32"):
        dsp.moving_stat_into(x, torch.zeros(1000), 8, "var", mean_out=torch.zeros(1000, dtype=torch.float64))
    with pytest.raises(ValueError, match="multiple of channels"):
        dsp.moving_stat_into(torch.zeros(1001), torch.zeros(1001), 8, "var", channels=2)
    with pytest.raises(TypeError, match="float32 and int16"):
        dsp.moving_stat_into(torch.zeros(1000, dtype=torch.float64), torch.zeros(1000), 8, "var")
    for name in ("moving_stat", "moving_stat_into", "moving_rms", "moving_variance", "moving_std", "moving_mean_square",
                 "stat_plan"):
        assert name in dsp.__all__ and callable(getattr(dsp, name))
