"""GPU tests of the decimated moving average (moving_average_decimated -> mavg_decim_run): the
compacting tile scan (decim_scan), the window sum (decim_window) and the full-rate fallback
(decim_full), csrc/mavg_decim.hpp.

The reference everywhere is the CPU oracle at full rate, sliced:
oracle.mavg_*(x, k, C).reshape(-1, C)[phase::hop]; with a history, oracle(concat(hist, x)) with
the first k-1 frames dropped, then sliced.  Pass criteria (tests/test_gpu_rows.py's): int16
bit-exact; fp32 on int16-valued data (dist 0) bit-equal; fp32 on dist-2 data |y - ref| <= 1e-5 *
max(|ref|, F) with F the window's mean absolute input.  Every case asserts the plan's family
token and reads tile_frames from the plan; signals are about three tiles plus 17 frames.  A
full-rate reference is computed once per (kind, C, frames, k, history) and shared."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "digital_signal_processsing_amd", "lib", "libmavg_debug.so")
HOOKS_LIB = os.path.join(ROOT, "digital_signal_processsing_amd", "lib", "libmavg_hooks.so")

SCAN, WINDOW, FULL, NONE = "decim_scan<", "decim_window<", "decim_full ", "decim_none "
SCAN_KINDS = [("i16", 1), ("i16", 2), ("f32d0", 1), ("f32d2", 1), ("f32d2", 2)]


def _dsp():
    import digital_signal_processsing_amd as dsp
    return dsp


def _dt(kind):
    dsp = _dsp()
    return dsp.I16 if kind == "i16" else dsp.F32


_refs = {}


def signal_and_ref(oracle, kind, C, frames, k, with_hist=False):
    """(x, hist or None, full-rate reference [frames, C], F [frames, C] or None), cached and
    never modified: x is `frames` frames; with a history, the k-1 frames before it."""
    key = (kind, C, frames, k, with_hist)
    if key not in _refs:
        pre = k - 1 if with_hist else 0
        n = (frames + pre) * C
        seed = 7919 * frames + 31 * k + C + (5 if with_hist else 0)
        if kind == "i16":
            long = oracle.synth_i16(n, seed=seed)
            ref = oracle.mavg_i16(long, k, C)
        else:
            long = oracle.synth_f32(n, seed=seed, dist=0 if kind == "f32d0" else 2)
            ref = oracle.mavg_f32(long, k, C)
        F = None
        if kind == "f32d2":
            a = np.abs(long.astype(np.float64)).reshape(-1, C)
            p = np.cumsum(a, axis=0)
            s = p.copy()
            if k < p.shape[0]:
                s[k:] = p[k:] - p[:-k]
            F = (s / k)[pre:]
        x = np.ascontiguousarray(long[pre * C:])
        hist = np.ascontiguousarray(long[:pre * C]) if with_hist else None
        ref = np.ascontiguousarray(ref.reshape(-1, C)[pre:])
        for a in (x, hist, ref, F):
            if a is not None:
                a.setflags(write=False)
        _refs[key] = (x, hist, ref, F)
    return _refs[key]


def assert_decim_equal(kind, y, ref, F, hop, phase, what):
    want = ref[phase::hop]
    assert y.shape == want.shape and y.dtype == want.dtype, (what, y.shape, want.shape)
    if kind == "i16":
        bad = y != want
    elif kind == "f32d0":
        bad = y.view(np.int32) != want.view(np.int32)
    else:
        r64 = want.astype(np.float64)
        bad = ~(np.abs(y.astype(np.float64) - r64) <= 1e-5 * np.maximum(np.abs(r64), F[phase::hop]))
    if bad.any():
        m, c = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} mismatches, first at output frame {m} channel {c}: "
                             f"got {y[m, c]!r}, want {want[m, c]!r}")


def plan_of(kind, C, frames, k, hop, phase=0, library=None):
    return _dsp().decim_plan(frames * C, k, hop, phase, C, _dt(kind), library)


def tile_frames(plan):
    return int(re.search(r" tile_frames=(\d+) ", plan).group(1))


def unit_frames(plan):
    return int(re.search(r",F=(\d+),", plan).group(1))


def run_case(dev, oracle, kind, C, frames, k, hop, phase, family, with_hist=False, off_in=0, off_out=0, library=None):
    """Filter a seeded signal on the device, through views `off_in` / `off_out` samples into
    larger buffers, and check every output against the sliced oracle; nothing outside the
    output view may be written."""
    import torch
    dsp = _dsp()
    plan = plan_of(kind, C, frames, k, hop, phase, library)
    assert plan.startswith(family), (family, plan)
    x, hist, ref, F = signal_and_ref(oracle, kind, C, frames, k, with_hist)
    M = len(range(phase, frames, hop))
    assert f" out_frames={M} " in plan or not plan.startswith((SCAN, WINDOW)), plan
    tdt = torch.int16 if kind == "i16" else torch.float32
    xbuf = torch.zeros(frames * C + 8, dtype=tdt, device=dev)
    ybuf = torch.full((M * C + 8,), 7, dtype=tdt, device=dev)
    xv = xbuf[off_in:off_in + frames * C]
    yv = ybuf[off_out:off_out + M * C]
    xv.copy_(torch.tensor(x))
    assert xv.data_ptr() % 16 == (off_in * xbuf.element_size()) % 16
    ht = torch.tensor(hist).to(dev) if hist is not None else None
    dsp.moving_average_decimated_into(xv, yv, k, hop, phase, C, history=ht, library=library)
    yb = ybuf.cpu().numpy()
    y = yb[off_out:off_out + M * C].reshape(M, C)
    assert_decim_equal(kind, y, ref, F, hop, phase, (kind, C, frames, k, hop, phase, with_hist, off_in, off_out, plan))
    assert (yb[:off_out] == 7).all() and (yb[off_out + M * C:] == 7).all(), "written outside the output view"
    return y


def scan_shape(kind, C, k, library=None):
    """(tile_frames, frames per unit, about three tiles plus 17 frames) of the scan at this window."""
    p = plan_of(kind, C, 1 << 16, k, 7, library=library)
    assert p.startswith(SCAN), p
    return tile_frames(p), unit_frames(p), 3 * tile_frames(p) + 17


# ---- decim_scan ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", SCAN_KINDS)
def test_scan_hops_and_phases(gpu, oracle_mod, kind, C):
    k = 100
    TF, F, frames = scan_shape(kind, C, k)
    for hop in sorted({2, 3, F - 1, F, F + 1, 7, 160} - {0, 1}):
        for phase in sorted({0, hop // 2, hop - 1}):
            run_case(gpu, oracle_mod, kind, C, frames, k, hop, phase, SCAN)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", SCAN_KINDS)
def test_scan_block_averaging_with_a_small_window(gpu, oracle_mod, kind, C):
    """hop == grade and hop > 2 * grade with a window under 1 KiB: dense reading, the scan's."""
    TF, F, frames = scan_shape(kind, C, 4)
    for hop in (4, 9):
        for phase in sorted({0, hop // 2, hop - 1}):
            run_case(gpu, oracle_mod, kind, C, frames, 4, hop, phase, SCAN)


@pytest.mark.gpu
def test_scan_hop_past_the_tile_some_tiles_emit_nothing(gpu, oracle_mod):
    """hop > tile_frames: tiles without a kept frame return before they load.  grade=200 is the
    scan's by the rule; fp32 mono grade=2048, hop=3000 (an 8-KiB window: the rule's decim_window
    since the thresholds were measured) runs the scan forced through the hooks build."""
    from digital_signal_processsing_amd import _lib
    hop = 3000
    TF, F, _ = scan_shape("f32d2", 1, 200)
    assert hop > TF
    frames = 5 * TF + 17
    for kind in ("f32d2", "f32d0"):
        for phase in (0, 1500, 2999):
            run_case(gpu, oracle_mod, kind, 1, frames, 200, hop, phase, SCAN)
    assert plan_of("f32d2", 1, frames, 2048, hop).startswith(WINDOW)
    lib = _lib.load(HOOKS_LIB)
    try:
        assert lib.mavg_debug_force_decim(_lib.DECIM_SCAN) == _lib.OK
        assert tile_frames(plan_of("f32d2", 1, frames, 2048, hop, library=HOOKS_LIB)) == TF
        for kind in ("f32d2", "f32d0"):
            for phase in (0, 1500, 2999):
                run_case(gpu, oracle_mod, kind, 1, frames, 2048, hop, phase, SCAN, library=HOOKS_LIB)
    finally:
        lib.mavg_debug_force_decim(_lib.DECIM_AUTO)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", SCAN_KINDS)
def test_scan_at_its_halo_limit(gpu, oracle_mod, kind, C):
    """The longest window the scan takes (8 KiB of halo); one frame more is the fallback's."""
    kmax = 8192 // (C * (2 if kind == "i16" else 4))
    TF, F, frames = scan_shape(kind, C, kmax)
    for hop, phase in ((3, 1), (160, 80)):
        run_case(gpu, oracle_mod, kind, C, frames, kmax, hop, phase, SCAN)
    run_case(gpu, oracle_mod, kind, C, frames, kmax + 1, 160, 80, FULL)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", SCAN_KINDS)
@pytest.mark.parametrize("k", (2, 1023, 1024))
def test_scan_windows_with_an_unaligned_xk(gpu, oracle_mod, kind, C, k):
    TF, F, frames = scan_shape(kind, C, k)
    for hop, phase in ((2, 1), (3, 0), (160, 80)):
        run_case(gpu, oracle_mod, kind, C, frames, k, hop, phase, SCAN)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", SCAN_KINDS)
def test_scan_signal_lengths_around_the_phase_and_the_tile(gpu, oracle_mod, kind, C):
    k = 64
    TF, F, _ = scan_shape(kind, C, k)
    for hop, phase in ((3, 2), (7, 3), (160, 159)):
        for frames in sorted({1, phase, phase + 1, TF - 1, TF, TF + 1} - {0}):
            M = len(range(phase, frames, hop))
            if M == 0:  # nothing to plan or launch: the call is a no-op
                import torch
                x = torch.zeros(frames * C, dtype=torch.int16 if kind == "i16" else torch.float32, device=gpu)
                assert _dsp().moving_average_decimated(x, k, hop, phase, C).numel() == 0
                continue
            run_case(gpu, oracle_mod, kind, C, frames, k, hop, phase, SCAN)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", SCAN_KINDS)
def test_scan_misaligned_views(gpu, oracle_mod, kind, C):
    """An input view one sample off 16-B alignment runs the frame-unit form; an output view one
    sample off takes element stores at the ends of every tile's range."""
    k = 100
    TF, F, frames = scan_shape(kind, C, k)
    for off_in, off_out in ((1, 0), (0, 1), (1, 1), (3, 2)):
        for hop, phase in ((2, 0), (3, 1), (7, 6)):
            run_case(gpu, oracle_mod, kind, C, frames, k, hop, phase, SCAN, off_in=off_in, off_out=off_out)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", SCAN_KINDS)
def test_scan_with_history(gpu, oracle_mod, kind, C):
    k = 300
    TF, F, frames = scan_shape(kind, C, k)
    for hop, phase in ((2, 1), (160, 0), (400, 399)):
        run_case(gpu, oracle_mod, kind, C, frames, k, hop, phase, SCAN, with_hist=True)
    run_case(gpu, oracle_mod, kind, C, frames, k, 3, 1, SCAN, with_hist=True, off_in=1, off_out=1)


# ---- decim_window ----
WINDOW_KINDS = [("i16", 1), ("i16", 2), ("f32d0", 1), ("f32d2", 1), ("f32d2", 2), ("f32d2", 3), ("i16", 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", WINDOW_KINDS)
def test_window_at_its_thresholds(gpu, oracle_mod, kind, C):
    """A window of exactly 1 KiB (where a frame divides it), hop in {2 grade, 2 grade + 1}: the
    first outputs' windows reach before frame 0, the last window ends short of the signal."""
    eb = 2 if kind == "i16" else 4
    k = -(-1024 // (C * eb))
    assert k * C * eb >= 1024 and (k - 1) * C * eb < 1024
    frames = 40 * k + 17
    for hop in (2 * k, 2 * k + 1):
        for phase in sorted({0, hop // 2, hop - 1, k - 1, k}):
            run_case(gpu, oracle_mod, kind, C, frames, k, hop, phase, WINDOW)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("i16", "f32d2"))
@pytest.mark.parametrize("C", (1, 2, 3, 8))
def test_window_one_second_blocks(gpu, oracle_mod, kind, C):
    k = hop = 44100
    frames = 3 * k + 17
    for phase in (0, k - 1, 22050):
        run_case(gpu, oracle_mod, kind, C, frames, k, hop, phase, WINDOW)


@pytest.mark.gpu
def test_window_int16_past_int32_sums(gpu, oracle_mod):
    k = 70000
    frames = 3 * k + 17
    for C in (1, 2):
        run_case(gpu, oracle_mod, "i16", C, frames, k, k, k - 1, WINDOW)
        run_case(gpu, oracle_mod, "i16", C, frames, k, 2 * k + 1, 5, WINDOW)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", WINDOW_KINDS)
def test_window_history_and_misaligned_views(gpu, oracle_mod, kind, C):
    eb = 2 if kind == "i16" else 4
    k = -(-1024 // (C * eb)) + 3
    frames = 20 * k + 17
    hop = 2 * k + 1
    for phase in (0, 5, k - 2):  # windows that reach before frame 0: into the history
        run_case(gpu, oracle_mod, kind, C, frames, k, hop, phase, WINDOW, with_hist=True)
    for off_in, off_out in ((1, 0), (0, 1), (1, 1)):
        run_case(gpu, oracle_mod, kind, C, frames, k, hop, 3, WINDOW, off_in=off_in, off_out=off_out)
        run_case(gpu, oracle_mod, kind, C, frames, k, hop, 3, WINDOW, with_hist=True, off_in=off_in, off_out=off_out)


# ---- decim_full ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("i16", "f32d0", "f32d2"))
def test_full_three_channels(gpu, oracle_mod, kind):
    for k, hop, phase in ((64, 16, 5), (400, 399, 0), (33, 2, 1)):
        run_case(gpu, oracle_mod, kind, 3, 5017, k, hop, phase, FULL)
    run_case(gpu, oracle_mod, kind, 3, 5017, 64, 16, 5, FULL, with_hist=True, off_in=1, off_out=1)


@pytest.mark.gpu
def test_full_long_window_and_its_workspace(gpu, oracle_mod):
    """fp32 mono grade=8192, hop=160: the look-ahead scan plus its workspace behind the gather; a
    workspace one byte short is refused with the output untouched."""
    import torch
    dsp = _dsp()
    from digital_signal_processsing_amd import _lib
    kind, k, hop, phase, frames = "f32d2", 8192, 160, 7, 3 * 4096 + 17
    plan = plan_of(kind, 1, frames, k, hop, phase)
    assert plan.startswith("decim_full hop=160 phase=7 x ahead_scan<"), plan
    run_case(gpu, oracle_mod, kind, 1, frames, k, hop, phase, FULL)
    need = dsp.decim_workspace_bytes(frames, k, hop, phase)
    assert need == (frames * 4 + 15) // 16 * 16 + dsp.workspace_bytes(frames, k) and dsp.workspace_bytes(frames, k) > 0
    x, _, ref, F = signal_and_ref(oracle_mod, kind, 1, frames, k)
    xt = torch.tensor(x).to(gpu)
    M = len(range(phase, frames, hop))
    out = torch.full((M,), -123.5, device=gpu)
    short = torch.empty(need - 1, dtype=torch.uint8, device=gpu)
    with pytest.raises(dsp.MavgError) as e:
        dsp.moving_average_decimated_into(xt, out, k, hop, phase, workspace=short)
    assert e.value.status == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == -123.5).all()), "a workspace error must leave the stream untouched"
    dsp.moving_average_decimated_into(xt, out, k, hop, phase, workspace=torch.empty(need, dtype=torch.uint8, device=gpu))
    assert_decim_equal(kind, out.cpu().numpy().reshape(M, 1), ref, F, hop, phase, "exact workspace")


@pytest.mark.gpu
def test_full_grade_one_is_the_sliced_copy(gpu, oracle_mod):
    import torch
    dsp = _dsp()
    x, _, _, _ = signal_and_ref(oracle_mod, "f32d2", 2, 5017, 1)
    assert plan_of("f32d2", 2, 5017, 1, 3, 2).startswith("decim_full hop=3 phase=2 x copy<")
    y = dsp.moving_average_decimated(torch.tensor(x).to(gpu).view(-1, 2), 1, 3, 2)
    assert tuple(y.shape) == (len(range(2, 5017, 3)), 2)
    assert np.array_equal(y.cpu().numpy().view(np.uint8), np.ascontiguousarray(x.reshape(-1, 2)[2::3]).view(np.uint8))


# ---- further cases ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind,C,k", [("f32d2", 1, 1024), ("i16", 2, 400), ("f32d2", 3, 33), ("f32d2", 1, 8192)])
def test_hop_one_equals_moving_average(gpu, oracle_mod, kind, C, k):
    import torch
    dsp = _dsp()
    frames = 3 * 4096 + 17
    assert plan_of(kind, C, frames, k, 1).startswith(NONE)
    x, _, _, _ = signal_and_ref(oracle_mod, kind, C, frames, k)
    xt = torch.tensor(x).to(gpu)
    a = dsp.moving_average(xt, k, channels=C)
    b = dsp.moving_average_decimated(xt, k, 1, 0, C)
    assert a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    b2 = dsp.moving_average_decimated(xt.view(-1, C), k, 1)
    assert tuple(b2.shape) == (frames, C) and torch.equal(a.view(torch.uint8), b2.reshape(-1).view(torch.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", [("i16", 1), ("i16", 2), ("f32d0", 1)])
def test_forced_scan_equals_forced_window(gpu, oracle_mod, kind, C):
    """One shape where both paths apply (hop == grade, windows of 1 and 2 KiB: the rule's
    decim_scan), each forced through the hooks build: equal to the oracle and to each other, bit
    for bit."""
    from digital_signal_processsing_amd import _lib
    lib = _lib.load(HOOKS_LIB)
    k = hop = 512
    TF, F, frames = scan_shape(kind, C, k, library=HOOKS_LIB)
    ys = {}
    try:
        for path, family in ((_lib.DECIM_SCAN, SCAN), (_lib.DECIM_WINDOW, WINDOW), (_lib.DECIM_FULL, FULL)):
            assert lib.mavg_debug_force_decim(path) == _lib.OK
            ys[path] = [run_case(gpu, oracle_mod, kind, C, frames, k, hop, phase, family, library=HOOKS_LIB)
                        for phase in (0, 255, 511)]
    finally:
        lib.mavg_debug_force_decim(_lib.DECIM_AUTO)
    for a, b, c in zip(ys[_lib.DECIM_SCAN], ys[_lib.DECIM_WINDOW], ys[_lib.DECIM_FULL]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)) and np.array_equal(a.view(np.uint8), c.view(np.uint8))
    assert plan_of(kind, C, frames, k, hop, library=HOOKS_LIB).startswith(SCAN)  # the rule is back


@pytest.mark.gpu
def test_forced_window_with_overlapping_windows(gpu, oracle_mod):
    from digital_signal_processsing_amd import _lib
    lib = _lib.load(HOOKS_LIB)
    try:
        assert lib.mavg_debug_force_decim(_lib.DECIM_WINDOW) == _lib.OK
        for kind, C in (("f32d2", 1), ("i16", 2), ("f32d2", 5)):
            run_case(gpu, oracle_mod, kind, C, 2065, 400, 160, 80, WINDOW, library=HOOKS_LIB)
    finally:
        lib.mavg_debug_force_decim(_lib.DECIM_AUTO)


@pytest.mark.gpu
def test_shapes_and_a_side_stream_through_the_wrapper(gpu, oracle_mod):
    import torch
    dsp = _dsp()
    k, hop, phase, frames = 400, 160, 3, 6161
    x, _, ref, _ = signal_and_ref(oracle_mod, "i16", 2, frames, k)
    M = len(range(phase, frames, hop))
    xt = torch.tensor(x).to(gpu)
    y1 = dsp.moving_average_decimated(xt, k, hop, phase, channels=2)
    y2 = dsp.moving_average_decimated(xt.view(frames, 2), k, hop, phase)
    assert tuple(y1.shape) == (M * 2,) and tuple(y2.shape) == (M, 2)
    assert np.array_equal(y2.cpu().numpy(), ref[phase::hop]) and torch.equal(y1, y2.reshape(-1))
    s = torch.cuda.Stream()
    ys = dsp.moving_average_decimated(xt, k, hop, phase, channels=2, stream=s)
    s.synchronize()
    assert torch.equal(ys, y1)
    with pytest.raises(ValueError, match="contiguous"):
        dsp.moving_average_decimated(xt.view(frames, 2).t(), k, hop, phase)
    with pytest.raises(ValueError, match="history must hold"):
        dsp.moving_average_decimated(xt, k, hop, phase, channels=2, history=xt[:10].clone())


@pytest.mark.gpu
def test_graph_capture_of_one_scan_launch(gpu, oracle_mod):
    """Capture and replay one decim_scan launch (one stream, no parallel branches); the replay
    reads a new input in place."""
    import torch
    dsp = _dsp()
    kind, C, k, hop, phase = "f32d2", 1, 400, 160, 80
    TF, F, frames = scan_shape(kind, C, k)
    assert plan_of(kind, C, frames, k, hop, phase).startswith(SCAN)
    M = len(range(phase, frames, hop))
    x1, _, ref1, F1 = signal_and_ref(oracle_mod, kind, C, frames, k)
    x2 = np.ascontiguousarray(x1[::-1])  # a second input of the same length: the first, reversed
    ref2 = oracle_mod.mavg_f32(x2, k, C).reshape(-1, C)
    p = np.cumsum(np.abs(x2.astype(np.float64)).reshape(-1, C), axis=0)
    s2 = p.copy()
    s2[k:] = p[k:] - p[:-k]
    x = torch.tensor(x1).to(gpu)
    y = torch.zeros(M, device=gpu)
    dsp.moving_average_decimated_into(x, y, k, hop, phase)  # warm-up outside the capture
    torch.cuda.synchronize()
    y.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dsp.moving_average_decimated_into(x, y, k, hop, phase)
    g.replay()
    torch.cuda.synchronize()
    assert_decim_equal(kind, y.cpu().numpy().reshape(M, C), ref1, F1, hop, phase, "graph replay")
    x.copy_(torch.tensor(x2))
    g.replay()
    torch.cuda.synchronize()
    assert_decim_equal(kind, y.cpu().numpy().reshape(M, C), ref2, s2 / k, hop, phase, "replay 2")


# ---- the debug build: device checks live ----
def run_debug_cases(dev, oracle):
    """A handful of the cases above (the child process below runs this on the debug build)."""
    n = 0
    for kind, C in SCAN_KINDS:
        TF, F, frames = scan_shape(kind, C, 100)
        for hop, phase, off_in, off_out in ((2, 1, 0, 0), (F + 1, 0, 0, 1), (7, 6, 1, 0), (160, 80, 1, 1)):
            run_case(dev, oracle, kind, C, frames, 100, hop, phase, SCAN, off_in=off_in, off_out=off_out)
            n += 1
        run_case(dev, oracle, kind, C, TF + 1, 1023, 3, 2, SCAN, with_hist=True)
        run_case(dev, oracle, kind, C, frames, 4, 9, 8, SCAN)
        n += 2
    TF, F, _ = scan_shape("f32d2", 1, 200)
    run_case(dev, oracle, "f32d2", 1, 5 * TF + 17, 200, 3000, 1500, SCAN)  # tiles that emit nothing
    run_case(dev, oracle, "i16", 2, 3 * 4096 + 17, 2048, 160, 80, SCAN)    # the longest halo
    for kind, C in (("f32d2", 1), ("i16", 2), ("f32d2", 3), ("i16", 8)):
        eb = 2 if kind == "i16" else 4
        k = -(-1024 // (C * eb)) + 3
        for with_hist, off_in in ((False, 0), (True, 0), (True, 1)):
            run_case(dev, oracle, kind, C, 20 * k + 17, k, 2 * k + 1, 5, WINDOW, with_hist=with_hist, off_in=off_in, off_out=1)
            n += 1
    run_case(dev, oracle, "i16", 3, 5017, 64, 16, 5, FULL)
    return n + 2


CHILD = r'''
import sys
sys.path.insert(0, "tests")
import torch
import oracle
import test_gpu_decim as t
from digital_signal_processsing_amd import _lib
oracle.build()
_lib.load()
maps = open("/proc/self/maps").read()
assert "libmavg_debug.so" in maps and "lib/libmavg.so" not in maps, "the debug build must be the one loaded"
n = t.run_debug_cases(torch.device("cuda:0"), oracle)
torch.cuda.synchronize()
print("decim debug build ok", n)
'''


@pytest.mark.gpu
@pytest.mark.timeout(200)
def test_debug_build_runs_decim_cases_clean(gpu):
    """On lib/libmavg_debug.so no device check (stage indices, slot < capacity, output index <
    M * C, window loads) fires -- a firing check traps the kernel and the child fails -- and
    every output matches the oracle."""
    r = subprocess.run([sys.executable, "-u", "-c", CHILD], cwd=ROOT, env=dict(os.environ, MAVG_LIBRARY=DEBUG_LIB),
                       capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "decim debug build ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "mavg debug check failed" not in r.stdout + r.stderr
