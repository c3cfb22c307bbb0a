"""GPU tests of the batched rows API (moving_average_rows -> mavg_rows_run): the one-launch
segmented rows scan (mavg_segscan.hpp) and the per-row loop fallback.

The reference everywhere is the CPU oracle applied PER ROW (oracle.mavg_i16 / mavg_f32 of
x[r]).  Pass criteria: int16 bit-exact; fp32 on int16-valued data (dist 0) bit-equal (the fp64
sums are exact); fp32 on dist-2 data |y - ref| <= 1e-5 * max(|ref|, F) with F the window's mean
absolute input sum|x| / k (numpy fp64 cumulative sums per row) -- the floor
oracle.check_synth_exact documents.  Every case asserts the plan's family token, so it cannot
silently test the other path, and reads tile_frames from the plan where a shape depends on it."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "digital_signal_processsing_amd", "lib", "libmavg_debug.so")

KINDS = ("i16", "f32d0", "f32d2")
SCAN, LOOP = "rows_scan<", "rows_loop"


def _dsp():
    import digital_signal_processsing_amd as dsp
    return dsp


def _dt(kind):
    dsp = _dsp()
    return dsp.I16 if kind == "i16" else dsp.F32


def make_batch(oracle, kind, R, L, C, seed):
    """[R, L*C] seeded batch: int16, int16-valued fp32 (dist 0) or mixed-scale fp32 (dist 2)."""
    n = R * L * C
    if kind == "i16":
        x = oracle.synth_i16(n, seed=seed)
    else:
        x = oracle.synth_f32(n, seed=seed, dist=0 if kind == "f32d0" else 2)
    return x.reshape(R, L * C)


def ref_rows(oracle, kind, x, k, C):
    f = oracle.mavg_i16 if kind == "i16" else oracle.mavg_f32
    return np.stack([f(x[r], k, C) for r in range(x.shape[0])])


def window_mean_abs(x, k, C):
    """F[r, n] = sum of |x| over the window of frame n inside row r, / k (fp64 cumulative sums)."""
    R = x.shape[0]
    a = np.abs(x.astype(np.float64)).reshape(R, -1, C)
    p = np.cumsum(a, axis=1)
    s = p.copy()
    if k < p.shape[1]:
        s[:, k:] = p[:, k:] - p[:, :-k]
    return (s / k).reshape(R, -1)


def assert_rows_equal(kind, y, x, ref, k, C, what):
    assert y.shape == ref.shape and y.dtype == ref.dtype, what
    if kind == "i16":
        bad = y != ref
    elif kind == "f32d0":
        bad = y.view(np.int32) != ref.view(np.int32)
    else:
        r64 = ref.astype(np.float64)
        bad = ~(np.abs(y.astype(np.float64) - r64) <= 1e-5 * np.maximum(np.abs(r64), window_mean_abs(x, k, C)))
    if bad.any():
        r, i = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: {int(bad.sum())} mismatches, first at row {r} sample {i}: "
                             f"got {y[r, i]!r}, want {ref[r, i]!r}")


def plan_of(kind, R, L, k, C, with_history=False, library=None):
    return _dsp().rows_plan(R, L, k, C, _dt(kind), with_history, library)


def tile_frames(plan):
    return int(re.search(r" tile_frames=(\d+) ", plan).group(1))


def run_case(dev, oracle, kind, C, R, L, k, family, seed=None, library=None):
    """Filter a seeded [R, L*C] batch on the device and check every row against the oracle."""
    import torch
    dsp = _dsp()
    plan = plan_of(kind, R, L, k, C, library=library)
    assert plan.startswith(family), (family, plan)
    seed = seed if seed is not None else 1000 * R + 10 * L + k + C
    x = make_batch(oracle, kind, R, L, C, seed)
    xt = torch.from_numpy(x).to(dev)
    if C > 1:
        xt = xt.view(R, L, C)
    yt = dsp.moving_average_rows(xt, k, channels=C, library=library)
    assert yt.shape == xt.shape and yt.dtype == xt.dtype
    y = yt.cpu().numpy().reshape(R, L * C)
    assert_rows_equal(kind, y, x, ref_rows(oracle, kind, x, k, C), k, C, (kind, C, R, L, k, plan))
    return y


CASE1 = [(37, 5, k) for k in (2, 3, 5, 8)] + [(1000, 1, 4)]
CASE2 = [(67, 1001, k) for k in (2, 64, 1000, 1001, 1002)]
CASE3 = [(129, L, 16) for L in (63, 64, 65)]
CASE4 = [("f32d0", 1), ("f32d2", 1), ("i16", 2)]


def case4_shapes(kind, C, library=None):
    """Row lengths around the tile: L in {T-1, T, T+1}, T read from the plan."""
    T = tile_frames(plan_of(kind, 5, 1 << 14, 1024, C, library=library))
    for L in (T - 1, T, T + 1):
        assert tile_frames(plan_of(kind, 5, L, 1024, C, library=library)) == T
        yield 5, L, 1024


def run_debug_cases(dev, oracle):
    """Cases 1, 2 and 4 (test 13 runs this in a child process on the debug build)."""
    n = 0
    for kind in KINDS:
        for C in (1, 2):
            for R, L, k in CASE1 + CASE2:
                run_case(dev, oracle, kind, C, R, L, k, SCAN)
                n += 1
    for kind, C in CASE4:
        for R, L, k in case4_shapes(kind, C):
            run_case(dev, oracle, kind, C, R, L, k, SCAN)
            n += 1
    return n


# ---- 1. many rows per tile; window longer than the row ----
@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,L,k", CASE1)
def test_many_rows_per_tile(gpu, oracle_mod, kind, C, R, L, k):
    run_case(gpu, oracle_mod, kind, C, R, L, k, SCAN)


# ---- 2. rows starting at every offset inside a 16-B unit; 9. determinism ----
_case2_outputs = {}


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,L,k", CASE2)
def test_row_starts_at_every_unit_offset(gpu, oracle_mod, kind, C, R, L, k):
    _case2_outputs[(kind, C, R, L, k)] = run_case(gpu, oracle_mod, kind, C, R, L, k, SCAN)


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_are_bit_identical(gpu, oracle_mod, kind, C):
    for R, L, k in CASE2:
        first = _case2_outputs.get((kind, C, R, L, k))
        if first is None:
            first = run_case(gpu, oracle_mod, kind, C, R, L, k, SCAN)
        again = run_case(gpu, oracle_mod, kind, C, R, L, k, SCAN)
        assert np.array_equal(first.view(np.uint8), again.view(np.uint8)), (kind, C, k)


# ---- 3. wave and segment edges ----
@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("R,L,k", CASE3)
def test_wave_and_segment_edges(gpu, oracle_mod, kind, C, R, L, k):
    run_case(gpu, oracle_mod, kind, C, R, L, k, SCAN)


# ---- 4. row start on a tile edge ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind,C", CASE4)
def test_row_start_on_a_tile_edge(gpu, oracle_mod, kind, C):
    for R, L, k in case4_shapes(kind, C):
        run_case(gpu, oracle_mod, kind, C, R, L, k, SCAN)


# ---- 5. long rows across many tiles, halo clipped at a row start ----
def largest_scan_window(kind, R, L, C):
    lo, hi = 1, L  # rows_scan at lo, not at hi (for these L the halo of L frames does not fit)
    assert plan_of(kind, R, L, lo, C).startswith(SCAN) and plan_of(kind, R, L, hi, C).startswith(LOOP)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan_of(kind, R, L, mid, C).startswith(SCAN):
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
def test_long_rows_across_many_tiles(gpu, oracle_mod, kind, C):
    R, L = 3, 100003
    # the scan takes halos up to 16 KiB: k = 4096 stereo fp32 (32 KiB) is the loop's
    for k in (1024, 4096):
        run_case(gpu, oracle_mod, kind, C, R, L, k, LOOP if (kind != "i16" and C == 2 and k == 4096) else SCAN)
    kmax = largest_scan_window(kind, R, L, C)
    assert kmax * C * (2 if kind == "i16" else 4) == 16384, kmax
    run_case(gpu, oracle_mod, kind, C, R, L, kmax, SCAN)
    run_case(gpu, oracle_mod, kind, C, R, L, kmax + 1, LOOP)


# ---- 6. k = 1, the copy ----
@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", ("i16", "f32d2"))
def test_grade_one_is_the_copy(gpu, oracle_mod, kind, C):
    y = run_case(gpu, oracle_mod, kind, C, 9, 1001, 1, SCAN)
    x = make_batch(oracle_mod, kind, 9, 1001, C, 1000 * 9 + 10 * 1001 + 1 + C)
    assert np.array_equal(y.view(np.uint8), x.view(np.uint8))


# ---- 7. misaligned views ----
@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
def test_misaligned_views(gpu, oracle_mod, kind, C):
    import torch
    dsp = _dsp()
    R, L, k = 9, 1001, 100
    assert plan_of(kind, R, L, k, C).startswith(SCAN)
    n = R * L * C
    x = make_batch(oracle_mod, kind, R, L, C, 77 + C)
    ref = ref_rows(oracle_mod, kind, x, k, C)
    shape = (R, L) if C == 1 else (R, L, C)
    for off_in, off_out in ((1, 0), (0, 1), (1, 1)):
        xbuf = torch.zeros(n + 8, dtype=torch.from_numpy(x).dtype, device=gpu)
        ybuf = torch.full((n + 8,), 7, dtype=xbuf.dtype, device=gpu)
        xv = xbuf[off_in:off_in + n].view(shape)
        yv = ybuf[off_out:off_out + n].view(shape)
        xv.copy_(torch.from_numpy(x).view(shape))
        assert xv.data_ptr() % 16 == (off_in * xbuf.element_size()) % 16 and xv.is_contiguous()
        dsp.moving_average_rows_into(xv, yv, k, channels=C)
        y = yv.cpu().numpy().reshape(R, L * C)
        assert_rows_equal(kind, y, x, ref, k, C, (kind, C, off_in, off_out))
        yb = ybuf.cpu().numpy()  # nothing written outside the view
        assert (yb[:off_out] == 7).all() and (yb[off_out + n:] == 7).all()


# ---- 8. row isolation ----
@pytest.mark.gpu
@pytest.mark.parametrize("k", (100, 1000))
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", ("i16", "f32d2"))
def test_row_isolation(gpu, oracle_mod, kind, C, k):
    """Row 16's output does not change by one bit when every other row becomes +-inf / nan
    (fp32) or +-32767 (int16): nothing of another row enters a row's sums."""
    import torch
    dsp = _dsp()
    R, L, keep = 33, 777, 16
    assert plan_of(kind, R, L, k, C).startswith(SCAN)
    x = make_batch(oracle_mod, kind, R, L, C, 4242 + C)
    poisoned = x.copy()
    if kind == "i16":
        fill = np.where(np.arange(L * C) % 2 == 0, 32767, -32767).astype(np.int16)
        for r in range(R):
            if r != keep:
                poisoned[r] = fill if r % 2 else -fill
    else:
        vals = (np.inf, -np.inf, np.nan)
        for r in range(R):
            if r != keep:
                poisoned[r] = np.array([vals[(r + i) % 3] for i in range(L * C)], dtype=np.float32)
    shape = (R, L) if C == 1 else (R, L, C)
    run = lambda a: dsp.moving_average_rows(torch.from_numpy(a).to(gpu).view(shape), k,
                                            channels=C).cpu().numpy().reshape(R, L * C)
    y_clean, y_poisoned = run(x), run(poisoned)
    assert np.array_equal(y_clean[keep].view(np.uint8), y_poisoned[keep].view(np.uint8))
    if kind != "i16":
        assert np.isfinite(y_poisoned[keep]).all()
    one = slice(keep, keep + 1)
    assert_rows_equal(kind, y_poisoned[one], x[one], ref_rows(oracle_mod, kind, x[one], k, C), k, C, (kind, C, k))


# ---- 10. loop fallback ----
@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", ("i16", "f32d2"))
def test_loop_with_per_row_history(gpu, oracle_mod, kind, C):
    """Each row's history is the true preceding samples, cut from longer rows."""
    import torch
    dsp = _dsp()
    R, L, k = 4, 5000, 300
    assert plan_of(kind, R, L, k, C, with_history=True).startswith(LOOP)
    long_rows = make_batch(oracle_mod, kind, R, L + k - 1, C, 555 + C)
    ref = ref_rows(oracle_mod, kind, long_rows, k, C)[:, (k - 1) * C:]
    hist = np.ascontiguousarray(long_rows[:, :(k - 1) * C])
    x = np.ascontiguousarray(long_rows[:, (k - 1) * C:])
    xt = torch.from_numpy(x).to(gpu)
    y = dsp.moving_average_rows(xt.view(R, L, C) if C > 1 else xt, k, channels=C,
                                history=torch.from_numpy(hist).to(gpu)).cpu().numpy().reshape(R, L * C)
    # the windows reach into the history: F over the long rows
    if kind == "i16":
        assert np.array_equal(y, ref)
    else:
        F = window_mean_abs(long_rows, k, C)[:, (k - 1) * C:]
        r64 = ref.astype(np.float64)
        assert (np.abs(y.astype(np.float64) - r64) <= 1e-5 * np.maximum(np.abs(r64), F)).all()
    with pytest.raises(ValueError, match="history must hold"):
        dsp.moving_average_rows(xt, k, history=torch.from_numpy(hist).to(gpu)[:, 1:].contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_loop_three_channels(gpu, oracle_mod, kind):
    run_case(gpu, oracle_mod, kind, 3, 5, 1000, 33, LOOP)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (20000, 5000))
def test_loop_long_window_and_its_workspace(gpu, oracle_mod, k):
    import torch
    dsp = _dsp()
    from digital_signal_processsing_amd import _lib
    R, L, kind = 3, 20000, "f32d2"
    run_case(gpu, oracle_mod, kind, 1, R, L, k, LOOP)
    need = dsp.rows_workspace_bytes(R, L, k, 1, dsp.F32)
    assert need > 0 and need == dsp.workspace_bytes(L, k, 1, dsp.F32)
    x = make_batch(oracle_mod, kind, R, L, 1, 31 + k)
    xt = torch.from_numpy(x).to(gpu)
    out = torch.full_like(xt, -123.5)
    short = torch.empty(need - 1, dtype=torch.uint8, device=gpu)
    with pytest.raises(dsp.MavgError) as e:
        dsp.moving_average_rows_into(xt, out, k, workspace=short)
    assert e.value.status == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == -123.5).all()), "a workspace error must leave the stream untouched"
    dsp.moving_average_rows_into(xt, out, k, workspace=torch.empty(need, dtype=torch.uint8, device=gpu))
    assert_rows_equal(kind, out.cpu().numpy(), x, ref_rows(oracle_mod, kind, x, k, 1), k, 1, ("exact workspace", k))


# ---- 11. shapes through the wrapper ----
@pytest.mark.gpu
def test_shapes_through_the_wrapper(gpu, oracle_mod):
    import torch
    dsp = _dsp()
    k = 50
    x = make_batch(oracle_mod, "f32d2", 6, 500, 1, 11)
    y = dsp.moving_average_rows(torch.from_numpy(x).to(gpu).view(2, 3, 500), k)
    assert tuple(y.shape) == (2, 3, 500)  # [B, C, T], planar: six independent rows
    assert_rows_equal("f32d2", y.cpu().numpy().reshape(6, 500), x, ref_rows(oracle_mod, "f32d2", x, k, 1), k, 1, "[2,3,500]")
    x = make_batch(oracle_mod, "i16", 4, 500, 2, 12)
    y = dsp.moving_average_rows(torch.from_numpy(x).to(gpu).view(4, 500, 2), k, channels=2)
    assert tuple(y.shape) == (4, 500, 2)  # [B, T, C]: four stereo rows
    assert np.array_equal(y.cpu().numpy().reshape(4, 1000), ref_rows(oracle_mod, "i16", x, k, 2))
    xt = torch.from_numpy(x).to(gpu).view(4, 500, 2)
    with pytest.raises(ValueError, match="contiguous"):
        dsp.moving_average_rows(xt.transpose(0, 1), k, channels=2)
    with pytest.raises(ValueError, match="same dtype and shape"):
        dsp.moving_average_rows_into(xt, torch.empty(4, 1000, dtype=xt.dtype, device=gpu), k, channels=2)
    # a side stream: the launch stream waits for x's, the result is ordered on it
    s = torch.cuda.Stream()
    ys = dsp.moving_average_rows(xt, k, channels=2, stream=s)
    s.synchronize()
    assert torch.equal(ys, y)
    # an empty batch is a no-op
    assert tuple(dsp.moving_average_rows(torch.empty(0, 500, device=gpu), k).shape) == (0, 500)


# ---- 12. past 2^31 samples ----
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_batch_past_2_31_samples(gpu, oracle_mod):
    """int16 mono, 2^15 + 1 rows of 2^16 + 3 frames (2.15e9 samples, 4.3 GB each way): every
    output against a torch int64 cumulative-sum reference along the rows, in row chunks, with
    the truncating division of tests/bigsignal_ref.py; oracle spot rows."""
    import torch
    dsp = _dsp()
    R, L, k = (1 << 15) + 1, (1 << 16) + 3, 1024
    assert R * L > 1 << 31
    assert plan_of("i16", R, L, k, 1).startswith(SCAN)
    x = dsp.fill_synthetic(R * L, dtype=torch.int16, seed=0xB16, device=gpu).view(R, L)
    y = dsp.moving_average_rows(x, k)
    bad, rc = 0, 512
    for r0 in range(0, R, rc):
        P = x[r0:r0 + rc].to(torch.int64).cumsum(1)
        S = P.clone()
        S[:, k:] -= P[:, :-k]
        del P
        bad += int((torch.div(S, k, rounding_mode="trunc").to(torch.int16) != y[r0:r0 + rc]).sum())
        del S
    assert bad == 0, f"{bad} mismatches"
    for r in (0, (1 << 31) // L, R - 1):  # the first row, the row holding flat sample 2^31, the last
        assert np.array_equal(y[r].cpu().numpy(), oracle_mod.mavg_i16(x[r].cpu().numpy(), k, 1)), r


# ---- 13. debug build ----
CHILD = r'''
import sys
sys.path.insert(0, "tests")
import torch
import oracle
import test_gpu_rows as t
from digital_signal_processsing_amd import _lib
oracle.build()
_lib.load()
maps = open("/proc/self/maps").read()
assert "libmavg_debug.so" in maps and "lib/libmavg.so" not in maps, "the debug build must be the one loaded"
n = t.run_debug_cases(torch.device("cuda:0"), oracle)
torch.cuda.synchronize()
print("rows debug build ok", n)
'''


@pytest.mark.gpu
@pytest.mark.timeout(200)
def test_debug_build_runs_the_rows_cases_clean(gpu):
    """Cases 1, 2 and 4 on lib/libmavg_debug.so: no device check (stage indices, x[n-k]
    extraction, row positions) fires -- a firing check traps the kernel and the child fails --
    and every output matches the oracle."""
    r = subprocess.run([sys.executable, "-u", "-c", CHILD], cwd=ROOT, env=dict(os.environ, MAVG_LIBRARY=DEBUG_LIB),
                       capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "rows debug build ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "mavg debug check failed" not in r.stdout + r.stderr
