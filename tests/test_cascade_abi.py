"""CPU tests of the cascaded moving average's ABI (mavg_cascade_run, mavg_cascade_workspace_bytes,
mavg_cascade_plan, include/mavg.h; mavg_debug_force_cascade, include/mavg_debug.h): the symbols,
the status table with dummy pointers, the dispatch rule as the plan text shows it, the workspace
formula and the wrappers' argument checks.  No GPU."""
import ctypes
import os
import subprocess
import sys

import pytest

import digital_signal_processsing_amd as dsp
from digital_signal_processsing_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASCADE_SYMBOLS = ("mavg_cascade_run", "mavg_cascade_workspace_bytes", "mavg_cascade_plan")
HOOK = "mavg_debug_force_cascade"
F32, I16 = _lib.F32, _lib.I16
# The fused kernel's total-halo limits, passes * (grade - 1) * C * sample size (mavg_cascade.hip): the
# dispatch rule's measured range -- 2 KiB, 256 B for two int16 passes -- and what the kernel can take
# when it is forced (kCascadeMaxHaloBytes, 16 KiB: the force-hook test below).


def rule_limit(dt, p):
    return 256 if dt == I16 and p == 2 else 2048


def r16(b):
    return (b + 15) // 16 * 16


def test_cascade_symbols_are_exported_by_release_and_debug():
    for path in (_lib.LIB_PATH, _lib.DEBUG_LIB_PATH):
        lib = _lib.load(path)
        for name in CASCADE_SYMBOLS:
            assert hasattr(lib, name), (path, name)
        assert lib.mavg_abi_version() == _lib.ABI_VERSION == 4  # additive: the version stays
    assert set(CASCADE_SYMBOLS) <= set(_lib.EXPORTED_SYMBOLS)
    assert not hasattr(_lib.load(), HOOK)                       # the release build has no hook
    assert hasattr(_lib.load(_lib.DEBUG_LIB_PATH), HOOK) and HOOK in _lib.DEBUG_SYMBOLS
    assert hasattr(_lib.load(_lib.HOOKS_LIB_PATH), HOOK)
    assert (_lib.CASCADE_AUTO, _lib.CASCADE_TILE, _lib.CASCADE_LOOP) == (0, 1, 2)
    lib = _lib.load()
    assert len(lib.mavg_cascade_run.argtypes) == 11
    assert len(lib.mavg_cascade_workspace_bytes.argtypes) == 7
    assert len(lib.mavg_cascade_plan.argtypes) == 8


def _run(n, C, k, p, dtype=F32, din=16, dout=1 << 30, hist=None, ws=None, ws_bytes=0):
    return _lib.load().mavg_cascade_run(din, dout, n, C, k, p, dtype, hist, ws, ws_bytes, None)


@pytest.mark.parametrize("args,status", [
    (dict(n=100, C=1, k=3, p=0), _lib.ERR_INVALID_ARG),               # passes < 1
    (dict(n=100, C=1, k=3, p=-1), _lib.ERR_INVALID_ARG),
    (dict(n=100, C=1, k=0, p=2), _lib.ERR_INVALID_ARG),               # mavg_run's: grade < 1
    (dict(n=100, C=0, k=3, p=2), _lib.ERR_INVALID_ARG),               # channels < 1
    (dict(n=9, C=2, k=3, p=2), _lib.ERR_INVALID_ARG),                 # a partial frame
    (dict(n=100, C=1, k=3, p=2, dtype=7), _lib.ERR_INVALID_ARG),      # bad dtype
    (dict(n=100, C=1, k=3, p=2, din=0), _lib.ERR_INVALID_ARG),        # null input with work to do
    (dict(n=100, C=1, k=3, p=2, dout=0), _lib.ERR_INVALID_ARG),
    (dict(n=100, C=1, k=3, p=2, din=18), _lib.ERR_MISALIGNED),        # fp32 view not 4-B aligned
    (dict(n=100, C=1, k=3, p=2, dout=(1 << 30) + 6), _lib.ERR_MISALIGNED),
    (dict(n=100, C=1, k=3, p=2, dtype=I16, din=21), _lib.ERR_MISALIGNED),
    (dict(n=100, C=1, k=3, p=2, hist=19), _lib.ERR_MISALIGNED),       # history not sample-aligned
    (dict(n=0, C=1, k=3, p=2, din=0, dout=0), _lib.OK),               # nothing to do
    (dict(n=0, C=1, k=3, p=0, din=0, dout=0), _lib.ERR_INVALID_ARG),  # validated before the no-op
    (dict(n=100, C=1, k=1 << 30, p=3), _lib.ERR_UNSUPPORTED),         # passes * (grade-1) past int
    (dict(n=100, C=1, k=(1 << 30) + 1, p=2), _lib.ERR_UNSUPPORTED),
    (dict(n=3 << 20, C=3, k=33, p=3), _lib.ERR_WORKSPACE),            # cascade_loop without its workspace
    (dict(n=1 << 20, C=1, k=8192, p=2, ws=1 << 22, ws_bytes=1 << 20), _lib.ERR_WORKSPACE),
    (dict(n=1 << 20, C=1, k=8192, p=2, ws=(1 << 22) + 4, ws_bytes=1 << 30), _lib.ERR_MISALIGNED),
])
def test_cascade_run_validates_before_launch(args, status):
    assert _run(**args) == status


def test_a_workspace_one_byte_short_is_refused():
    for kw in (dict(n=3 * 1001, C=3, k=33, p=3, dtype=I16), dict(n=1 << 20, C=1, k=8192, p=2)):
        need = dsp.cascade_workspace_bytes(kw["n"], kw["k"], kw["p"], kw["C"], kw.get("dtype", F32))
        assert need > 0
        assert _run(ws=1 << 22, ws_bytes=need - 1, **kw) == _lib.ERR_WORKSPACE
        need_h = dsp.cascade_workspace_bytes(kw["n"], kw["k"], kw["p"], kw["C"], kw.get("dtype", F32), True)
        assert need_h > need
        assert _run(ws=1 << 22, ws_bytes=need_h - 1, hist=1 << 28, **kw) == _lib.ERR_WORKSPACE
        assert _run(ws=1 << 22, ws_bytes=need, hist=1 << 28, **kw) == _lib.ERR_WORKSPACE


def test_plan_and_workspace_validate():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(512)
    out = ctypes.c_size_t(7)
    assert lib.mavg_cascade_plan(100, 1, 3, 2, F32, 0, None, 0) == _lib.ERR_INVALID_ARG
    assert lib.mavg_cascade_plan(0, 1, 3, 2, F32, 0, buf, len(buf)) == _lib.ERR_INVALID_ARG   # as mavg_plan
    assert lib.mavg_cascade_plan(100, 1, 3, 0, F32, 0, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_cascade_plan(100, 1, 0, 2, F32, 0, buf, len(buf)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_cascade_plan(100, 1, 1 << 30, 4, F32, 0, buf, len(buf)) == _lib.ERR_UNSUPPORTED
    assert lib.mavg_cascade_workspace_bytes(100, 1, 3, 2, F32, 0, None) == _lib.ERR_INVALID_ARG
    assert lib.mavg_cascade_workspace_bytes(100, 1, 3, 0, F32, 0, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_cascade_workspace_bytes(100, 0, 3, 2, F32, 0, ctypes.byref(out)) == _lib.ERR_INVALID_ARG
    assert lib.mavg_cascade_workspace_bytes(0, 1, 3, 2, F32, 0, ctypes.byref(out)) == _lib.OK and out.value == 0


N = 1 << 22  # frames below: n = N * C samples


def _kmax(limit, p, C, eb):
    """The largest grade whose total halo p * (k - 1) * C * eb is within the limit."""
    return limit // (p * C * eb) + 1


# (dtype, C, grade, passes) -> the plan's family token.  One row per dispatch branch and the
# neighbours of each threshold.
PLAN_TABLE = [
    # passes == 1 or grade == 1: mavg_run itself
    (F32, 1, 1024, 1, "cascade_none x tile_scan<"),
    (I16, 3, 7, 1, "cascade_none x tile_scan<"),
    (F32, 1, 1, 3, "cascade_none x copy<"),
    (I16, 2, 1, 4, "cascade_none x copy<"),
    # the fused kernel
    (F32, 1, 100, 3, "cascade_tile<f32,acc=f64,C=1,F=4,U=2,"),
    (F32, 2, 60, 3, "cascade_tile<f32,acc=f64,C=2,F=2,U=2,"),
    (F32, 2, 100, 3, "cascade_loop passes=3 history=0 x wide_tile<f32,"),   # 2376 B: past the rule's 2 KiB
    (I16, 1, 100, 3, "cascade_tile<i16,acc=i32,C=1,F=8,U=4,"),
    (I16, 1, 100, 2, "cascade_loop passes=2 history=0 x tile_scan<"),   # two int16 passes: 256 B
    (I16, 2, 100, 3, "cascade_tile<i16,acc=i32,C=2,F=4,U=4,"),
    (F32, 1, 2, 2, "cascade_tile<f32,"),
    (I16, 1, 2, 4, "cascade_tile<i16,"),
    (F32, 1, 8, 64, "cascade_tile<f32,"),       # many passes of a short window
    (F32, 1, 1025, 2, "cascade_loop passes=2 history=0 x tile_scan<"),  # 8 KiB: measured slower than the loop
    # 3+ channels, int16 past int32 sums
    (F32, 3, 33, 3, "cascade_loop passes=3 history=0 x tile_scan<"),
    (I16, 3, 33, 3, "cascade_loop passes=3 history=0 x tile_scan<"),
    (F32, 9, 33, 2, "cascade_loop passes=2 history=0 x naive<"),
    (I16, 1, 70000, 2, "cascade_loop passes=2 history=0 x ahead_scan<i16,acc=i64"),
    (F32, 1, 8192, 2, "cascade_loop passes=2 history=0 x ahead_scan<f32"),   # the look-ahead plus its workspace
]
# the rule's halo limit: the largest grade inside it, and one frame more
for _dt, _eb in ((F32, 4), (I16, 2)):
    for _C in (1, 2):
        for _p in (2, 3, 4):
            _k = _kmax(rule_limit(_dt, _p), _p, _C, _eb)
            PLAN_TABLE.append((_dt, _C, _k, _p, "cascade_tile<"))
            PLAN_TABLE.append((_dt, _C, _k + 1, _p, f"cascade_loop passes={_p} history=0 x "))


@pytest.mark.parametrize("dt,C,k,p,token", PLAN_TABLE)
def test_plan_token_table(dt, C, k, p, token):
    eb = 4 if dt == F32 else 2
    plan = dsp.cascade_plan(N * C, k, p, C, dt)
    assert plan.startswith(token), plan
    ws = dsp.cascade_workspace_bytes(N * C, k, p, C, dt)
    ws_h = dsp.cascade_workspace_bytes(N * C, k, p, C, dt, True)
    inner = dsp.workspace_bytes(N * C, k, C, dt)
    if plan.startswith("cascade_tile<"):
        assert ws == 0 and ws_h == 0, (plan, ws, ws_h)
        assert f" passes={p} halo_frames={p * (k - 1)} " in plan and " tile_frames=" in plan and " lds=" in plan, plan
        lds = int(plan.split(" lds=")[1].split()[0])
        assert lds <= 64 * 1024, plan
        assert dsp.cascade_plan(N * C, k, p, C, dt, True) == plan
    elif plan.startswith("cascade_none"):
        assert plan == "cascade_none x " + dsp.plan(N * C, k, C, dt), plan
        assert ws == ws_h == inner
    else:
        assert plan == f"cascade_loop passes={p} history=0 x " + dsp.plan(N * C, k, C, dt), plan
        assert dsp.cascade_plan(N * C, k, p, C, dt, True) == plan.replace("history=0", "history=1")
        # the ping-pong buffer, rounded up to 16 B, plus one pass's own workspace
        assert ws == r16(N * C * eb) + inner, (plan, ws)
        # with a history: two block buffers, and the inner workspace covers the first block's run
        hs = p * (k - 1) * C
        assert ws_h == r16(N * C * eb) + 2 * r16(hs * eb) + max(inner, dsp.workspace_bytes(hs, k, C, dt)), (plan, ws_h)


def test_loop_workspace_rounds_up_and_adds_the_look_ahead():
    n, k, p = 1_000_003, 8192, 2
    inner = dsp.workspace_bytes(n, k)
    assert inner > 0
    assert dsp.cascade_workspace_bytes(n, k, p) == r16(n * 4) + inner
    hs = p * (k - 1)
    assert dsp.cascade_workspace_bytes(n, k, p, with_history=True) == \
        r16(n * 4) + 2 * r16(hs * 4) + max(inner, dsp.workspace_bytes(hs, k))
    assert dsp.cascade_workspace_bytes(3 * 1001, 33, 3, 3, I16) == r16(3 * 1001 * 2)
    assert dsp.cascade_workspace_bytes(3 * 1001, 33, 3, 3, I16, True) == r16(3 * 1001 * 2) + 2 * r16(3 * 32 * 3 * 2)
    # a signal shorter than its history block: the block's run sizes the inner workspace
    assert dsp.cascade_workspace_bytes(1000, 8192, 2, with_history=True) == \
        r16(1000 * 4) + 2 * r16(hs * 4) + max(dsp.workspace_bytes(1000, k), dsp.workspace_bytes(hs, k))


FORCE_CHILD = r'''
import sys
import digital_signal_processsing_amd as dsp
from digital_signal_processsing_amd import _lib
lib = _lib.load(_lib.DEBUG_LIB_PATH)
D = _lib.DEBUG_LIB_PATH
plan = lambda *a, **k: dsp.cascade_plan(*a, library=D, **k)
assert lib.mavg_debug_force_cascade(3) == _lib.ERR_INVALID_ARG and lib.mavg_debug_force_cascade(-1) == _lib.ERR_INVALID_ARG
assert plan(1 << 20, 100, 3).startswith("cascade_tile<")            # the rule
assert plan(3 << 20, 33, 3, 3).startswith("cascade_loop")
assert lib.mavg_debug_force_cascade(_lib.CASCADE_LOOP) == _lib.OK
assert plan(1 << 20, 100, 3).startswith("cascade_loop passes=3 history=0 x tile_scan<")
assert dsp.cascade_workspace_bytes(1 << 20, 100, 3, library=D) == 4 << 20
assert plan(1 << 20, 100, 1).startswith("cascade_none")             # passes == 1 stays mavg_run
assert lib.mavg_debug_force_cascade(_lib.CASCADE_TILE) == _lib.OK
assert plan(1 << 20, 100, 3).startswith("cascade_tile<")
# forced, the kernel takes what it can, past the rule's measured range: up to 16 KiB of total halo
assert plan(1 << 20, 2049, 2).startswith("cascade_tile<f32,") and plan(1 << 20, 4096, 2, 1, _lib.I16).startswith("cascade_tile<i16,")
assert plan(1 << 20, 1025, 4, 2, _lib.I16).startswith("cascade_tile<i16,acc=i32,C=2,")
assert dsp.cascade_workspace_bytes(1 << 20, 2049, 2, library=D) == 0
assert plan(1 << 20, 1, 3).startswith("cascade_none")
for kw in (dict(n=3 << 10, grade=33, channels=3), dict(n=1 << 20, grade=70000, dtype=_lib.I16), dict(n=1 << 20, grade=8192),
           dict(n=1 << 20, grade=2050), dict(n=1 << 20, grade=4098, dtype=_lib.I16)):
    a = (kw["n"], kw["grade"], 2, kw.get("channels", 1), kw.get("dtype", _lib.F32))
    try:
        plan(*a)
        raise SystemExit("forced tile took a shape outside its range")
    except dsp.MavgError as e:
        assert e.status == _lib.ERR_UNSUPPORTED
    try:
        dsp.cascade_workspace_bytes(*a, library=D)
        raise SystemExit("forced tile sized a shape outside its range")
    except dsp.MavgError as e:
        assert e.status == _lib.ERR_UNSUPPORTED
    assert lib.mavg_cascade_run(16, 1 << 30, a[0], a[3], a[1], 2, a[4], None, None, 0, None) == _lib.ERR_UNSUPPORTED
assert lib.mavg_debug_force_cascade(_lib.CASCADE_AUTO) == _lib.OK
assert plan(1 << 20, 8192, 2).startswith("cascade_loop") and plan(1 << 20, 2049, 2).startswith("cascade_loop")
print("force hook ok")
'''


def test_force_hook_on_the_debug_build():
    """The hook is process-wide state: exercised in a child process of its own."""
    r = subprocess.run([sys.executable, "-c", FORCE_CHILD], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "force hook ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


def test_wrappers_reject_host_tensors_bad_passes_and_wrong_out():
    import torch
    x = torch.zeros(1000)
    with pytest.raises(ValueError, match="device tensor"):
        dsp.moving_average_cascade(x, 8, 3)                         # a host tensor
    with pytest.raises(ValueError, match="device tensor"):
        dsp.moving_average_cascade_into(x, torch.zeros(1000), 8, 3)
    for passes in (0, -2):
        with pytest.raises(ValueError, match="passes must be"):
            dsp.cascade_plan(1000, 8, passes)
        with pytest.raises(ValueError, match="passes must be"):
            dsp.cascade_workspace_bytes(1000, 8, passes)
        with pytest.raises(ValueError, match="passes must be|device tensor"):
            dsp.moving_average_cascade(x, 8, passes)
        with pytest.raises(ValueError, match="passes must be"):
            dsp.moving_average_cascade_into(x, torch.zeros(1000), 8, passes)
    for m in (999, 1001, 0):                                        # a wrong out size
        with pytest.raises(ValueError, match="out must hold"):
            dsp.moving_average_cascade_into(x, torch.zeros(m), 8, 3)
    with pytest.raises(ValueError, match="same dtype"):
        dsp.moving_average_cascade_into(x, torch.zeros(1000, dtype=torch.int16), 8, 3)
    with pytest.raises(ValueError, match="multiple of channels"):
        dsp.moving_average_cascade_into(torch.zeros(1001), torch.zeros(1001), 8, 3, channels=2)
    for name in ("moving_average_cascade", "moving_average_cascade_into", "cascade_plan", "cascade_workspace_bytes"):
        assert name in dsp.__all__ and callable(getattr(dsp, name))
