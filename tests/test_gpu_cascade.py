"""GPU tests of the cascaded moving average (moving_average_cascade -> mavg_cascade_run): the fused
tile kernel (cascade_tile, csrc/mavg_cascade.hpp), the loop of mavg_run passes (cascade_loop) and
passes == 1 (cascade_none).

The reference everywhere is the CPU oracle applied `passes` times; with a history, applied to
concat(history, x) with the first passes * (k - 1) frames dropped.  Pass criteria: int16 bit-exact;
fp32 (dist 0 and dist 2) |y - ref| <= 1e-5 * max(|ref|, F) with F the passes-fold moving mean of |x|
in float64 (each pass adds at most one fp32 rounding, ~6e-8 F, and averaging does not amplify it).
Every case asserts the plan's family token, reads tile_frames from the plan and checks that nothing
outside the output view is written; signals are three tiles plus 17 frames unless stated.  A
reference is computed once per (kind, C, frames, k, passes, history) and shared.

The dispatch rule gives the fused kernel the range where it measured faster (a total halo of at
most 2 KiB, 256 B for two int16 passes); the kernel itself takes up to 16 KiB.  A tile-path case
past the rule's range runs the same kernel forced through the hooks build (run_tile_case)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "digital_signal_processsing_amd", "lib", "libmavg_debug.so")
HOOKS_LIB = os.path.join(ROOT, "digital_signal_processsing_amd", "lib", "libmavg_hooks.so")

TILE, LOOP, NONE = "cascade_tile<", "cascade_loop ", "cascade_none "
KINDS = [("i16", 1), ("i16", 2), ("f32d0", 1), ("f32d2", 1), ("f32d2", 2)]


def rule_limit(kind, p):
    """The rule's total-halo limit, passes * (k - 1) * C * sample size (mavg_cascade.hip)."""
    return 256 if kind == "i16" and p == 2 else 2048


def _dsp():
    import digital_signal_processsing_amd as dsp
    return dsp


def _dt(kind):
    dsp = _dsp()
    return dsp.I16 if kind == "i16" else dsp.F32


def _eb(kind):
    return 2 if kind == "i16" else 4


def cascade_ref(oracle, long, kind, C, k, p):
    """(the oracle applied p times, the p-fold moving mean of |x| in float64 or None)."""
    ref = long
    for _ in range(p):
        ref = oracle.mavg_i16(ref, k, C) if kind == "i16" else oracle.mavg_f32(ref, k, C)
    F = None
    if kind != "i16":
        F = np.abs(long.astype(np.float64)).reshape(-1, C)
        for _ in range(p):
            P = np.concatenate([np.zeros((k, C)), np.cumsum(F, axis=0)])
            F = (P[k:] - P[:-k]) / k
    return ref.reshape(-1, C), F


_refs = {}


def signal_and_ref(oracle, kind, C, frames, k, p, with_hist=False):
    """(x, hist or None, reference [frames, C], F [frames, C] or None), cached and never modified:
    x is `frames` frames; with a history, the p * (k - 1) frames before it."""
    key = (kind, C, frames, k, p, with_hist)
    if key not in _refs:
        pre = p * (k - 1) if with_hist else 0
        n = (frames + pre) * C
        seed = 7919 * frames + 31 * k + 7 * p + C + (5 if with_hist else 0)
        if kind == "i16":
            long = oracle.synth_i16(n, seed=seed)
        else:
            long = oracle.synth_f32(n, seed=seed, dist=0 if kind == "f32d0" else 2)
        ref, F = cascade_ref(oracle, long, kind, C, k, p)
        x = np.ascontiguousarray(long[pre * C:])
        hist = np.ascontiguousarray(long[:pre * C]) if with_hist else None
        ref = np.ascontiguousarray(ref[pre:])
        F = None if F is None else np.ascontiguousarray(F[pre:])
        for a in (x, hist, ref, F):
            if a is not None:
                a.setflags(write=False)
        _refs[key] = (x, hist, ref, F)
    return _refs[key]


def assert_cascade_equal(kind, y, ref, F, what):
    assert y.shape == ref.shape and y.dtype == ref.dtype, (what, y.shape, ref.shape)
    if kind == "i16":
        bad = y != ref
    else:
        r64 = ref.astype(np.float64)
        bad = ~(np.abs(y.astype(np.float64) - r64) <= 1e-5 * np.maximum(np.abs(r64), F))
    if bad.any():
        m, c = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} mismatches, first at frame {m} channel {c}: "
                             f"got {y[m, c]!r}, want {ref[m, c]!r}")


def plan_of(kind, C, frames, k, p, with_hist=False, library=None):
    return _dsp().cascade_plan(frames * C, k, p, C, _dt(kind), with_hist, library)


def tile_frames(plan):
    return int(re.search(r" tile_frames=(\d+) ", plan).group(1))


def run_signal(dev, kind, C, x, hist, ref, F, k, p, family, off_in=0, off_out=0, library=None, workspace=None):
    """Filter x on the device, through views `off_in` / `off_out` samples into larger buffers, and
    check every output against ref; nothing outside the output view may be written."""
    import torch
    dsp = _dsp()
    frames = x.size // C
    plan = plan_of(kind, C, frames, k, p, hist is not None, library)
    assert plan.startswith(family), (family, plan)
    tdt = torch.int16 if kind == "i16" else torch.float32
    xbuf = torch.zeros(frames * C + 8, dtype=tdt, device=dev)
    ybuf = torch.full((frames * C + 8,), 7, dtype=tdt, device=dev)
    xv = xbuf[off_in:off_in + frames * C]
    yv = ybuf[off_out:off_out + frames * C]
    xv.copy_(torch.tensor(x))
    assert xv.data_ptr() % 16 == (off_in * xbuf.element_size()) % 16
    ht = torch.tensor(hist).to(dev) if hist is not None else None
    dsp.moving_average_cascade_into(xv, yv, k, p, C, history=ht, library=library, workspace=workspace)
    yb = ybuf.cpu().numpy()
    y = yb[off_out:off_out + frames * C].reshape(frames, C)
    assert_cascade_equal(kind, y, ref, F, (kind, C, frames, k, p, hist is not None, off_in, off_out, plan))
    assert (yb[:off_out] == 7).all() and (yb[off_out + frames * C:] == 7).all(), "written outside the output view"
    return y


def run_case(dev, oracle, kind, C, frames, k, p, family, with_hist=False, **kw):
    x, hist, ref, F = signal_and_ref(oracle, kind, C, frames, k, p, with_hist)
    return run_signal(dev, kind, C, x, hist, ref, F, k, p, family, **kw)


FORCE_LIB = HOOKS_LIB   # the debug-build child below forces on the debug build instead


class forced_tile:
    """cascade_tile forced on the hooks build, the rule restored on the way out."""

    def __enter__(self):
        from digital_signal_processsing_amd import _lib
        self.lib = _lib.load(FORCE_LIB)
        assert self.lib.mavg_debug_force_cascade(_lib.CASCADE_TILE) == _lib.OK
        return FORCE_LIB

    def __exit__(self, *exc):
        self.lib.mavg_debug_force_cascade(0)


def by_rule(kind, C, k, p):
    return plan_of(kind, C, 1 << 16, k, p).startswith(TILE)


def tile_shape(kind, C, k, p, library=None):
    """(tile_frames, three tiles plus 17 frames) of the fused kernel at this cascade."""
    plan = plan_of(kind, C, 1 << 16, k, p, library=library)
    assert plan.startswith(TILE), plan
    return tile_frames(plan), 3 * tile_frames(plan) + 17


def run_tile_case(dev, oracle, kind, C, frames, k, p, **kw):
    """A case on the fused kernel: by the rule on the release build where the rule takes it, else
    forced on the hooks build.  frames: a number, or a function of tile_frames."""
    def go(library):
        TF, _ = tile_shape(kind, C, k, p, library)
        return run_case(dev, oracle, kind, C, frames(TF) if callable(frames) else frames, k, p, TILE, library=library, **kw)
    if by_rule(kind, C, k, p):
        return go(None)
    with forced_tile() as lib:
        return go(lib)


def three_tiles(TF):
    return 3 * TF + 17


# ---- cascade_tile ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", KINDS)
@pytest.mark.parametrize("p", (2, 3, 4))
def test_tile_passes_and_windows(gpu, oracle_mod, kind, C, p):
    for k in (2, 3, 100):
        run_tile_case(gpu, oracle_mod, kind, C, three_tiles, k, p)
    assert by_rule(kind, C, 3, p)     # short windows are the rule's in every kind


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", KINDS)
def test_tile_at_its_halo_limit(gpu, oracle_mod, kind, C):
    """The largest window with passes * (k - 1) * C * sample size inside the rule's limit runs the
    fused kernel; one frame more is the loop's.  Both are checked, by the rule on the release build."""
    for p in (2, 4):
        limit = rule_limit(kind, p)
        kmax = limit // (p * C * _eb(kind)) + 1
        assert p * (kmax - 1) * C * _eb(kind) <= limit < p * kmax * C * _eb(kind)
        TF, frames = tile_shape(kind, C, kmax, p)
        run_case(gpu, oracle_mod, kind, C, frames, kmax, p, TILE)
        run_case(gpu, oracle_mod, kind, C, frames, kmax + 1, p, LOOP)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", KINDS)
def test_forced_tile_at_the_kernels_halo_limit(gpu, oracle_mod, kind, C):
    """16 KiB of total halo, the most the kernel takes (forced: the rule stops at 2 KiB)."""
    for p in (2, 4):
        kmax = 16384 // (p * C * _eb(kind)) + 1
        assert not by_rule(kind, C, kmax, p)
        run_tile_case(gpu, oracle_mod, kind, C, three_tiles, kmax, p)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", KINDS)
def test_tile_signal_lengths(gpu, oracle_mod, kind, C):
    """Warm-up shorter than, equal to and longer than the signal, and the tile edge."""
    k, p = 64, 3
    for frames in (1, k - 1, k, p * (k - 1), p * (k - 1) + 1, lambda TF: TF - 1, lambda TF: TF, lambda TF: TF + 1):
        run_tile_case(gpu, oracle_mod, kind, C, frames, k, p)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", KINDS)
def test_tile_misaligned_views(gpu, oracle_mod, kind, C):
    """Views off 16-B alignment: the frame-unit form, element stores at the ends."""
    k, p = 100, 3
    for off_in, off_out in ((1, 0), (0, 1), (1, 1), (3, 2)):
        run_tile_case(gpu, oracle_mod, kind, C, three_tiles, k, p, off_in=off_in, off_out=off_out)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", KINDS)
def test_history_on_the_tile_and_forced_to_the_loop(gpu, oracle_mod, kind, C):
    from digital_signal_processsing_amd import _lib
    for k, p in ((300, 2), (50, 4)):
        run_tile_case(gpu, oracle_mod, kind, C, three_tiles, k, p, with_hist=True)
        run_tile_case(gpu, oracle_mod, kind, C, three_tiles, k, p, with_hist=True, off_in=1, off_out=1)
    lib = _lib.load(HOOKS_LIB)
    try:
        for k, p in ((300, 2), (50, 4)):
            assert lib.mavg_debug_force_cascade(_lib.CASCADE_TILE) == _lib.OK
            TF, frames = tile_shape(kind, C, k, p, library=HOOKS_LIB)
            assert lib.mavg_debug_force_cascade(_lib.CASCADE_LOOP) == _lib.OK
            run_case(gpu, oracle_mod, kind, C, frames, k, p, LOOP, with_hist=True, library=HOOKS_LIB)
    finally:
        lib.mavg_debug_force_cascade(_lib.CASCADE_AUTO)


@pytest.mark.gpu
def test_int16_full_scale(gpu, oracle_mod):
    """Constant 32767, constant -32768 and blocks alternating between them with period k, at
    k = 4096, two passes, mono: the largest int32 prefixes the tile sees.  Bit-exact."""
    k, p = 4096, 2
    with forced_tile() as lib:        # 16 KiB of halo: past the rule's range, forced
        TF, frames = tile_shape("i16", 1, k, p, library=lib)
        blocks = np.where((np.arange(frames) // k) % 2 == 0, 32767, -32768).astype(np.int16)
        for x in (np.full(frames, 32767, np.int16), np.full(frames, -32768, np.int16), blocks):
            ref, _ = cascade_ref(oracle_mod, x, "i16", 1, k, p)
            run_signal(gpu, "i16", 1, x, None, ref, None, k, p, TILE, library=lib)


# ---- cascade_loop, cascade_none ----
@pytest.mark.gpu
def test_loop_three_channels_and_the_look_ahead(gpu, oracle_mod):
    import torch
    dsp = _dsp()
    for kind in ("i16", "f32d2"):
        run_case(gpu, oracle_mod, kind, 3, 5017, 33, 3, LOOP)
        run_case(gpu, oracle_mod, kind, 3, 5017, 33, 3, LOOP, with_hist=True)
    frames, k, p = 3 * 8192 + 17, 8192, 2
    assert "ahead_scan<" in plan_of("f32d2", 1, frames, k, p)
    run_case(gpu, oracle_mod, "f32d2", 1, frames, k, p, LOOP)
    # a workspace one byte short is refused with the output untouched
    need = dsp.cascade_workspace_bytes(frames, k, p)
    assert need > dsp.workspace_bytes(frames, k) > 0
    x, _, ref, F = signal_and_ref(oracle_mod, "f32d2", 1, frames, k, p)
    xt = torch.tensor(x).to(gpu)
    y = torch.full((frames,), 7.0, device=gpu)
    with pytest.raises(dsp.MavgError) as e:
        dsp.moving_average_cascade_into(xt, y, k, p, workspace=torch.empty(need - 1, dtype=torch.uint8, device=gpu))
    assert e.value.status == 4   # MAVG_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((y == 7).all())
    dsp.moving_average_cascade_into(xt, y, k, p, workspace=torch.empty(need, dtype=torch.uint8, device=gpu))
    assert_cascade_equal("f32d2", y.cpu().numpy().reshape(-1, 1), ref, F, "caller's workspace")


@pytest.mark.gpu
def test_one_pass_is_moving_average(gpu, oracle_mod):
    import torch
    dsp = _dsp()
    for kind, C, k in (("f32d2", 1, 100), ("i16", 2, 41)):
        frames = 6161
        assert plan_of(kind, C, frames, k, 1).startswith(NONE + "x tile_scan<")
        x, _, _, _ = signal_and_ref(oracle_mod, kind, C, frames, k, 1)
        xt = torch.tensor(x).to(gpu)
        y1 = dsp.moving_average_cascade(xt, k, 1, channels=C)
        y0 = dsp.moving_average(xt, k, channels=C)
        assert np.array_equal(y1.cpu().numpy().view(np.uint8), y0.cpu().numpy().view(np.uint8))
        run_case(gpu, oracle_mod, kind, C, frames, k, 1, NONE)


# ---- two paths on one shape ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", KINDS)
def test_forced_tile_against_forced_loop(gpu, oracle_mod, kind, C):
    """Through the hooks build: int16 equal bit for bit and to the oracle; fp32 both within the bar."""
    from digital_signal_processsing_amd import _lib
    lib = _lib.load(HOOKS_LIB)
    k, p = 512, 3
    ys = {}
    try:
        assert lib.mavg_debug_force_cascade(_lib.CASCADE_TILE) == _lib.OK
        TF, frames = tile_shape(kind, C, k, p, library=HOOKS_LIB)
        for path, family in ((_lib.CASCADE_TILE, TILE), (_lib.CASCADE_LOOP, LOOP)):
            assert lib.mavg_debug_force_cascade(path) == _lib.OK
            ys[path] = run_case(gpu, oracle_mod, kind, C, frames, k, p, family, library=HOOKS_LIB)
    finally:
        lib.mavg_debug_force_cascade(_lib.CASCADE_AUTO)
    if kind == "i16":
        assert np.array_equal(ys[_lib.CASCADE_TILE], ys[_lib.CASCADE_LOOP])
    assert plan_of(kind, C, frames, k, p, library=HOOKS_LIB) == plan_of(kind, C, frames, k, p)  # the rule is back
    assert plan_of(kind, C, frames, 3, p, library=HOOKS_LIB).startswith(TILE)


# ---- the wrapper ----
@pytest.mark.gpu
def test_shapes_and_a_side_stream_through_the_wrapper(gpu, oracle_mod):
    import torch
    dsp = _dsp()
    k, p, frames = 100, 3, 6161
    x, _, ref, _ = signal_and_ref(oracle_mod, "i16", 2, frames, k, p)
    xt = torch.tensor(x).to(gpu)
    y1 = dsp.moving_average_cascade(xt, k, p, channels=2)
    y2 = dsp.moving_average_cascade(xt.view(frames, 2), k, p)
    assert tuple(y1.shape) == (frames * 2,) and tuple(y2.shape) == (frames, 2)
    assert np.array_equal(y2.cpu().numpy(), ref) and torch.equal(y1, y2.reshape(-1))
    s = torch.cuda.Stream()
    ys = dsp.moving_average_cascade(xt, k, p, channels=2, stream=s)
    s.synchronize()
    assert torch.equal(ys, y1)
    with pytest.raises(ValueError, match="contiguous"):
        dsp.moving_average_cascade(xt.view(frames, 2).t(), k, p)
    with pytest.raises(ValueError, match="history must hold"):
        dsp.moving_average_cascade(xt, k, p, channels=2, history=xt[:10].clone())
    with pytest.raises(ValueError, match="history must hold"):
        dsp.moving_average_cascade(xt, k, p, channels=2, history=xt[:(k - 1) * 2].clone())   # one pass's worth


@pytest.mark.gpu
def test_graph_capture_of_one_tile_launch(gpu, oracle_mod):
    """Capture and replay one cascade_tile launch (one stream, no parallel branches); the replay
    reads a new input in place."""
    import torch
    dsp = _dsp()
    kind, C, k, p = "f32d2", 1, 100, 3
    TF, frames = tile_shape(kind, C, k, p)
    x1, _, ref1, F1 = signal_and_ref(oracle_mod, kind, C, frames, k, p)
    x2 = np.ascontiguousarray(x1[::-1])  # a second input of the same length: the first, reversed
    ref2, F2 = cascade_ref(oracle_mod, x2, kind, C, k, p)
    x = torch.tensor(x1).to(gpu)
    y = torch.zeros(frames, device=gpu)
    dsp.moving_average_cascade_into(x, y, k, p)  # warm-up outside the capture
    torch.cuda.synchronize()
    y.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dsp.moving_average_cascade_into(x, y, k, p)
    g.replay()
    torch.cuda.synchronize()
    assert_cascade_equal(kind, y.cpu().numpy().reshape(-1, C), ref1, F1, "graph replay")
    x.copy_(torch.tensor(x2))
    g.replay()
    torch.cuda.synchronize()
    assert_cascade_equal(kind, y.cpu().numpy().reshape(-1, C), ref2, F2, "replay 2")


# ---- the debug build: device checks live ----
def run_debug_cases(dev, oracle):
    """A handful of the cases above (the child process below runs this on the debug build)."""
    n = 0
    for kind, C in KINDS:
        for k, p in ((100, 3), (2, 4)):
            for off_in, off_out in ((0, 0), (1, 0), (3, 2)):
                run_tile_case(dev, oracle, kind, C, three_tiles, k, p, off_in=off_in, off_out=off_out)
                n += 1
        run_tile_case(dev, oracle, kind, C, lambda TF: TF + 1, 300, 2, with_hist=True)
        run_tile_case(dev, oracle, kind, C, three_tiles, 300, 2, with_hist=True, off_in=1, off_out=1)
        kmax = 16384 // (4 * C * _eb(kind)) + 1
        run_tile_case(dev, oracle, kind, C, three_tiles, kmax, 4)    # the longest halo the kernel takes (forced)
        run_tile_case(dev, oracle, kind, C, 64, 64, 3)               # all warm-up
        n += 4
    run_case(dev, oracle, "i16", 3, 5017, 33, 3, LOOP, with_hist=True)
    return n + 1


CHILD = r'''
import sys
sys.path.insert(0, "tests")
import torch
import oracle
import test_gpu_cascade as t
from digital_signal_processsing_amd import _lib
oracle.build()
_lib.load()
maps = open("/proc/self/maps").read()
assert "libmavg_debug.so" in maps and "lib/libmavg.so" not in maps, "the debug build must be the one loaded"
t.FORCE_LIB = _lib.DEBUG_LIB_PATH
n = t.run_debug_cases(torch.device("cuda:0"), oracle)
torch.cuda.synchronize()
assert "libmavg_hooks.so" not in open("/proc/self/maps").read()
print("cascade debug build ok", n)
'''


@pytest.mark.gpu
@pytest.mark.timeout(200)
def test_debug_build_runs_cascade_cases_clean(gpu):
    """On lib/libmavg_debug.so no device check (stage indices, buffer extents, the output index)
    fires -- a firing check traps the kernel and the child fails -- and every output matches the
    oracle."""
    r = subprocess.run([sys.executable, "-u", "-c", CHILD], cwd=ROOT, env=dict(os.environ, MAVG_LIBRARY=DEBUG_LIB),
                       capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "cascade debug build ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "mavg debug check failed" not in r.stdout + r.stderr
