"""GPU tests of the ragged rows API (moving_average_ragged -> mavg_ragged_run): the one-launch
ragged scan (mavg_segscan.hpp) and the per-row loop fallback.

The reference everywhere is the CPU oracle applied PER ROW (oracle.mavg_i16 / mavg_f32 of each
row's slice of the packed stream).  Pass criteria, those of tests/test_gpu_rows.py: int16
bit-exact; fp32 on int16-valued data (dist 0) bit-equal; fp32 on dist-2 data |y - ref| <= 1e-5 *
max(|ref|, F) with F the window's mean absolute input inside the row.  Every case asserts the
plan's family token, so it cannot silently test the other path, and reads tile_frames from the
plan where a shape depends on it."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_rows import KINDS, _dsp, _dt, assert_rows_equal, make_batch, ref_rows, tile_frames, window_mean_abs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "digital_signal_processsing_amd", "lib", "libmavg_debug.so")
SCAN, LOOP = "ragged_scan<", "ragged_loop"


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def make_packed(oracle, kind, lengths, C, seed):
    """The packed stream of sum(lengths) * C samples: int16, int16-valued fp32 or mixed-scale fp32."""
    n = int(sum(lengths)) * C
    if kind == "i16":
        return oracle.synth_i16(n, seed=seed)
    return oracle.synth_f32(n, seed=seed, dist=0 if kind == "f32d0" else 2)


def ref_packed(oracle, kind, x, lengths, k, C):
    """(per-row oracle output, per-row window mean |x|), both packed like x."""
    f = oracle.mavg_i16 if kind == "i16" else oracle.mavg_f32
    ref = np.empty_like(x)
    F = np.zeros(x.shape, dtype=np.float64) if kind == "f32d2" else None
    off = offsets_of(lengths) * C
    for r in range(len(lengths)):
        a, b = int(off[r]), int(off[r + 1])
        if b > a:
            ref[a:b] = f(x[a:b], k, C)
            if F is not None:
                F[a:b] = window_mean_abs(x[a:b].reshape(1, -1), k, C)[0]
    return ref, F


def assert_packed_equal(kind, y, ref, F, lengths, C, what):
    assert y.shape == ref.shape and y.dtype == ref.dtype, what
    if kind == "i16":
        bad = y != ref
    elif kind == "f32d0":
        bad = y.view(np.int32) != ref.view(np.int32)
    else:
        r64 = ref.astype(np.float64)
        bad = ~(np.abs(y.astype(np.float64) - r64) <= 1e-5 * np.maximum(np.abs(r64), F))
    if bad.any():
        i = int(np.argwhere(bad)[0][0])
        r = int(np.searchsorted(offsets_of(lengths) * C, i, side="right")) - 1
        raise AssertionError(f"{what}: {int(bad.sum())} mismatches, first at sample {i} (row {r}, length "
                             f"{lengths[r]}): got {y[i]!r}, want {ref[i]!r}")


def plan_of(kind, lengths, k, C, library=None):
    return _dsp().ragged_plan(offsets_of(lengths), k, C, _dt(kind), library)


_refs = {}  # (kind, C, lengths, k, seed) -> (x, ref, F): computed once, shared, never modified


def reference(oracle, kind, C, lengths, k, seed):
    key = (kind, C, tuple(lengths), k, seed)
    if key not in _refs:
        x = make_packed(oracle, kind, lengths, C, seed)
        _refs[key] = (x,) + ref_packed(oracle, kind, x, lengths, k, C)
    return _refs[key]


def run_case(dev, oracle, kind, C, lengths, k, family, seed=None, library=None):
    """Filter a seeded packed batch on the device and check every row against the oracle."""
    import torch
    dsp = _dsp()
    lengths = [int(v) for v in lengths]
    plan = plan_of(kind, lengths, k, C, library=library)
    assert plan.startswith(family), (family, plan)
    seed = seed if seed is not None else 7 * len(lengths) + 3 * sum(lengths) + k + C
    x, ref, F = reference(oracle, kind, C, lengths, k, seed)
    xt = torch.from_numpy(x).to(dev)
    if C > 1:
        xt = xt.view(-1, C)
    yt = dsp.moving_average_ragged(xt, k, lengths=lengths, channels=C, library=library)
    assert yt.shape == xt.shape and yt.dtype == xt.dtype
    y = yt.cpu().numpy().reshape(-1)
    assert_packed_equal(kind, y, ref, F, lengths, C, (kind, C, len(lengths), k, plan))
    return y


# ---- shapes (seeded and fixed) ----
def _tiny_lengths(force_ends_empty):
    rng = np.random.RandomState(20260)
    v = rng.choice([0, 0, 1, 1, 2, 3, 5, 8, 13], size=600)
    v[200:250] = 0  # 50 consecutive empty rows
    if force_ends_empty:
        v[0] = v[-1] = 0
    else:
        v[0], v[-1] = 5, 3
    return [int(a) for a in v]


CASE1 = [(_tiny_lengths(e), k) for e in (False, True) for k in (2, 3, 5, 8)]
CASE2 = ([([61 + i % 7 for i in range(129)], k) for k in (16, 64)] +
         [([999 + i % 5 for i in range(67)], k) for k in (2, 64, 1000, 1002)])
CASE3_K = (1024, 16)
CASE3 = [("f32d0", 1), ("f32d2", 1), ("f32d2", 2), ("i16", 1), ("i16", 2)]
MIXED = [100003, 1, 0, 0, 5, 30011, 7, 4097]


def _ids(cases):
    return [f"R{len(l)}-k{k}-{'e' if l[0] == 0 else 'n'}" for l, k in cases]


def case3_lengths(kind, C, k, library=None):
    """Row starts at t0 - 1, t0 and t0 + 1 of several tiles; T read from the plan."""
    T = tile_frames(plan_of(kind, [1 << 14] * 5, k, C, library=library))
    lengths = [T - 1, 1, T, T + 1, 2 * T - 1, 1, 0, T]
    assert tile_frames(plan_of(kind, lengths, k, C, library=library)) == T
    return lengths


def run_debug_cases(dev, oracle, library=None):
    """Cases 1 to 3 (test 14 runs this in a child process on the debug build)."""
    n = 0
    for kind in KINDS:
        for C in (1, 2):
            for lengths, k in CASE1 + CASE2:
                run_case(dev, oracle, kind, C, lengths, k, SCAN, library=library)
                n += 1
    for kind, C in CASE3:
        for k in CASE3_K:
            run_case(dev, oracle, kind, C, case3_lengths(kind, C, k, library), k, SCAN, library=library)
            n += 1
    return n


# ---- 1. tiny mixed rows, empty rows anywhere ----
@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lengths,k", CASE1, ids=_ids(CASE1))
def test_tiny_mixed_rows(gpu, oracle_mod, kind, C, lengths, k):
    assert lengths[200:250] == [0] * 50 and 13 in lengths
    run_case(gpu, oracle_mod, kind, C, lengths, k, SCAN)


# ---- 2. starts at every unit offset and around wave edges; 10. determinism ----
_case2_outputs = {}


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("lengths,k", CASE2, ids=_ids(CASE2))
def test_starts_at_every_unit_offset_and_wave_edge(gpu, oracle_mod, kind, C, lengths, k):
    _case2_outputs[(kind, C, len(lengths), k)] = run_case(gpu, oracle_mod, kind, C, lengths, k, SCAN)


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
def test_two_runs_are_bit_identical(gpu, oracle_mod, kind, C):
    for lengths, k in CASE2:
        first = _case2_outputs.get((kind, C, len(lengths), k))
        if first is None:
            first = run_case(gpu, oracle_mod, kind, C, lengths, k, SCAN)
        again = run_case(gpu, oracle_mod, kind, C, lengths, k, SCAN)
        assert np.array_equal(first.view(np.uint8), again.view(np.uint8)), (kind, C, k)


# ---- 3. row starts on tile edges ----
@pytest.mark.gpu
@pytest.mark.parametrize("k", CASE3_K)
@pytest.mark.parametrize("kind,C", CASE3)
def test_row_starts_on_tile_edges(gpu, oracle_mod, kind, C, k):
    run_case(gpu, oracle_mod, kind, C, case3_lengths(kind, C, k), k, SCAN)


# ---- 4. long and short rows mixed; the scan's largest window ----
def largest_scan_window(kind, lengths, C):
    lo, hi = 1, max(lengths)  # the scan at lo, not at hi (the halo of the longest row does not fit)
    assert plan_of(kind, lengths, lo, C).startswith(SCAN) and plan_of(kind, lengths, hi, C).startswith(LOOP)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan_of(kind, lengths, mid, C).startswith(SCAN):
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
def test_long_and_short_rows_mixed(gpu, oracle_mod, kind, C):
    run_case(gpu, oracle_mod, kind, C, MIXED, 1024, SCAN)
    kmax = largest_scan_window(kind, MIXED, C)
    assert kmax * C * (2 if kind == "i16" else 4) == 16384, kmax
    run_case(gpu, oracle_mod, kind, C, MIXED, kmax, SCAN)
    run_case(gpu, oracle_mod, kind, C, MIXED, kmax + 1, LOOP)


# ---- 5. window longer than some or all rows ----
def _spread_lengths(lo, hi, n, seed):
    rng = np.random.RandomState(seed)
    v = [int(a) for a in rng.randint(lo, hi + 1, size=n)]
    v[3], v[n // 2] = lo, hi
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
def test_window_longer_than_some_rows(gpu, oracle_mod, kind, C):
    lengths = _spread_lengths(10, 2000, 40, 5)
    assert min(lengths) == 10 and max(lengths) == 2000
    run_case(gpu, oracle_mod, kind, C, lengths, 1000, SCAN)


@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", ("f32d0", "f32d2"))
def test_window_longer_than_all_rows(gpu, oracle_mod, kind, C):
    lengths = _spread_lengths(10, 1000, 40, 6)
    plan = plan_of(kind, lengths, 100000, C)
    assert " max_row_frames=1000 " in plan and " window=1000 " in plan, plan
    run_case(gpu, oracle_mod, kind, C, lengths, 100000, SCAN)


# ---- 6. k = 1, the copy ----
@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", ("i16", "f32d2"))
def test_grade_one_is_the_copy(gpu, oracle_mod, kind, C):
    lengths = [999 + i % 5 for i in range(9)]
    y = run_case(gpu, oracle_mod, kind, C, lengths, 1, SCAN, seed=61)
    x = make_packed(oracle_mod, kind, lengths, C, 61)
    assert np.array_equal(y.view(np.uint8), x.view(np.uint8))


# ---- 7. equal lengths agree with moving_average_rows ----
@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
def test_equal_lengths_agree_with_the_rows_api(gpu, oracle_mod, kind, C):
    import torch
    dsp = _dsp()
    R, L, k = 37, 1001, 64
    assert plan_of(kind, [L] * R, k, C).startswith(SCAN) and dsp.rows_plan(R, L, k, C, _dt(kind)).startswith("rows_scan<")
    x = make_batch(oracle_mod, kind, R, L, C, 707 + C)
    xt = torch.from_numpy(x).to(gpu)
    y_rows = dsp.moving_average_rows(xt.view(R, L, C) if C > 1 else xt, k, channels=C).cpu().numpy().reshape(R, L * C)
    packed = xt.view(R * L, C) if C > 1 else xt.view(R * L)
    y = dsp.moving_average_ragged(packed, k, lengths=[L] * R, channels=C).cpu().numpy().reshape(R, L * C)
    if kind == "f32d2":
        assert_rows_equal(kind, y, x, ref_rows(oracle_mod, kind, x, k, C), k, C, (kind, C))
    else:
        assert np.array_equal(y.view(np.uint8), y_rows.view(np.uint8)), (kind, C)


# ---- 8. row isolation ----
@pytest.mark.gpu
@pytest.mark.parametrize("k", (100, 1000))
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", ("i16", "f32d2"))
def test_row_isolation(gpu, oracle_mod, kind, C, k):
    """The kept row's output does not change by one bit when every other row becomes +-inf / nan
    (fp32) or +-32767 (int16): nothing of another row enters a row's sums."""
    import torch
    dsp = _dsp()
    lengths = _spread_lengths(1, 1500, 33, 8)
    keep = 16
    lengths[keep] = 777
    lengths[keep - 1] = 2  # a short poisoned neighbour right before the kept row
    assert plan_of(kind, lengths, k, C).startswith(SCAN)
    off = offsets_of(lengths) * C
    x = make_packed(oracle_mod, kind, lengths, C, 4242 + C)
    a, b = int(off[keep]), int(off[keep + 1])
    poisoned = x.copy()
    if kind == "i16":
        fill = np.where(np.arange(x.size) % 2 == 0, 32767, -32767).astype(np.int16)
    else:
        fill = np.array([np.inf, -np.inf, np.nan], dtype=np.float32)[np.arange(x.size) % 3]
    poisoned[:a], poisoned[b:] = fill[:a], fill[b:]

    def run(v):
        t = torch.from_numpy(v).to(gpu)
        return dsp.moving_average_ragged(t.view(-1, C) if C > 1 else t, k, lengths=lengths,
                                         channels=C).cpu().numpy().reshape(-1)
    y_clean, y_poisoned = run(x), run(poisoned)
    assert np.array_equal(y_clean[a:b].view(np.uint8), y_poisoned[a:b].view(np.uint8))
    if kind != "i16":
        assert np.isfinite(y_poisoned[a:b]).all()
    xr = x[a:b].reshape(1, -1)
    assert_rows_equal(kind, y_poisoned[a:b].reshape(1, -1), xr, ref_rows(oracle_mod, kind, xr, k, C), k, C, (kind, C, k))


# ---- 9. misaligned views ----
@pytest.mark.gpu
@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("kind", KINDS)
def test_misaligned_views(gpu, oracle_mod, kind, C):
    import torch
    dsp = _dsp()
    lengths, k = [999 + i % 5 for i in range(9)], 100
    assert plan_of(kind, lengths, k, C).startswith(SCAN)
    x, ref, F = reference(oracle_mod, kind, C, lengths, k, 77 + C)
    n = x.size
    shape = (n,) if C == 1 else (n // C, C)
    for off_in, off_out in ((1, 0), (0, 1), (1, 1)):
        xbuf = torch.zeros(n + 8, dtype=torch.from_numpy(x).dtype, device=gpu)
        ybuf = torch.full((n + 8,), 7, dtype=xbuf.dtype, device=gpu)
        xv = xbuf[off_in:off_in + n].view(shape)
        yv = ybuf[off_out:off_out + n].view(shape)
        xv.copy_(torch.from_numpy(x).view(shape))
        assert xv.data_ptr() % 16 == (off_in * xbuf.element_size()) % 16 and xv.is_contiguous()
        dsp.moving_average_ragged_into(xv, yv, k, lengths=lengths, channels=C)
        assert_packed_equal(kind, yv.cpu().numpy().reshape(-1), ref, F, lengths, C, (kind, C, off_in, off_out))
        yb = ybuf.cpu().numpy()  # nothing written outside the view
        assert (yb[:off_out] == 7).all() and (yb[off_out + n:] == 7).all()


# ---- 11. loop fallback ----
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_loop_three_channels(gpu, oracle_mod, kind):
    run_case(gpu, oracle_mod, kind, 3, [1000, 3, 0, 0, 517, 1, 999], 33, LOOP)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (20000, 5000))
def test_loop_long_window_and_its_workspace(gpu, oracle_mod, k):
    import torch
    dsp = _dsp()
    from digital_signal_processsing_amd import _lib
    lengths, kind = [20000, 3, 0, 15000], "f32d2"
    run_case(gpu, oracle_mod, kind, 1, lengths, k, LOOP, seed=31 + k)
    need = dsp.ragged_workspace_bytes(offsets_of(lengths), k, 1, dsp.F32)
    assert need > 0 and need == dsp.workspace_bytes(20000, k, 1, dsp.F32)
    x, ref, F = reference(oracle_mod, kind, 1, lengths, k, 31 + k)
    xt = torch.from_numpy(x).to(gpu)
    out = torch.full_like(xt, -123.5)
    short = torch.empty(need - 1, dtype=torch.uint8, device=gpu)
    with pytest.raises(dsp.MavgError) as e:
        dsp.moving_average_ragged_into(xt, out, k, lengths=lengths, workspace=short)
    assert e.value.status == _lib.ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == -123.5).all()), "a workspace error must leave the stream untouched"
    dsp.moving_average_ragged_into(xt, out, k, lengths=lengths,
                                   workspace=torch.empty(need, dtype=torch.uint8, device=gpu))
    assert_packed_equal(kind, out.cpu().numpy(), ref, F, lengths, 1, ("exact workspace", k))


# ---- 12. the wrapper ----
@pytest.mark.gpu
def test_wrapper(gpu, oracle_mod):
    import torch
    dsp = _dsp()
    k, kind, C = 50, "i16", 2
    lengths = [500, 0, 123, 377]
    off = offsets_of(lengths)
    x, ref, F = reference(oracle_mod, kind, C, lengths, k, 12)
    xt = torch.from_numpy(x).to(gpu).view(-1, C)
    y = dsp.moving_average_ragged(xt, k, lengths=lengths, channels=C)
    assert tuple(y.shape) == (1000, 2)
    assert np.array_equal(y.cpu().numpy().reshape(-1), ref)
    for given in (off, [int(v) for v in off], torch.from_numpy(off)):  # offsets= in every accepted form
        assert torch.equal(dsp.moving_average_ragged(xt, k, offsets=given, channels=C), y)
    assert torch.equal(dsp.moving_average_ragged(xt, k, lengths=np.array(lengths), channels=C), y)
    # offsets_device= is what the kernel reads: the same offsets give the same result, and a device
    # copy with another interior boundary (same total, same longest row) gives THAT segmentation
    d_off = torch.from_numpy(off).to(gpu)
    assert torch.equal(dsp.moving_average_ragged(xt, k, lengths=lengths, channels=C, offsets_device=d_off), y)
    other = [500, 100, 23, 377]
    y_other = dsp.moving_average_ragged(xt, k, lengths=lengths, channels=C,
                                        offsets_device=torch.from_numpy(offsets_of(other)).to(gpu))
    assert np.array_equal(y_other.cpu().numpy().reshape(-1), ref_packed(oracle_mod, kind, x, other, k, C)[0])
    # a side stream: the launch stream waits for x's, the result is ordered on it
    s = torch.cuda.Stream()
    ys = dsp.moving_average_ragged(xt, k, lengths=lengths, channels=C, stream=s)
    s.synchronize()
    assert torch.equal(ys, y)
    # argument errors that need a device tensor
    with pytest.raises(ValueError, match="end at 999 frames"):
        dsp.moving_average_ragged(xt, k, lengths=[500, 0, 123, 376], channels=C)
    with pytest.raises(ValueError, match="exactly one"):
        dsp.moving_average_ragged(xt, k, channels=C)
    with pytest.raises(ValueError, match="rows \\+ 1 = 5 entries"):
        dsp.moving_average_ragged(xt, k, lengths=lengths, channels=C, offsets_device=d_off[:4])
    with pytest.raises(ValueError, match="int64 device tensor"):
        dsp.moving_average_ragged(xt, k, lengths=lengths, channels=C, offsets_device=torch.from_numpy(off))
    with pytest.raises(ValueError, match="same dtype and shape"):
        dsp.moving_average_ragged_into(xt, torch.empty(2000, dtype=xt.dtype, device=gpu), k, lengths=lengths, channels=C)
    with pytest.raises(ValueError, match="contiguous"):
        dsp.moving_average_ragged(torch.from_numpy(x).to(gpu).view(C, -1).t(), k, lengths=lengths, channels=C)
    # rows = 0 and all-empty rows are no-ops
    empty = torch.empty(0, device=gpu)
    assert tuple(dsp.moving_average_ragged(empty, k, lengths=[]).shape) == (0,)
    assert tuple(dsp.moving_average_ragged(empty, k, offsets=[0]).shape) == (0,)
    assert tuple(dsp.moving_average_ragged(empty, k, lengths=[0, 0, 0]).shape) == (0,)
    assert tuple(dsp.moving_average_ragged(torch.empty(0, 2, device=gpu), k, lengths=[0], channels=2).shape) == (0, 2)


# ---- 13. past 2^31 samples ----
@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_batch_past_2_31_samples(gpu, oracle_mod):
    """int16 mono, 2^15 + 2 rows of alternately L - 1 and L + 1 frames, L = 2^16 + 3 (2.15e9
    samples, 4.3 GB each way).  A pair of rows is 2L frames, so x and y viewed as [rows / 2, 2L]
    hold one short and one long row per line: every output against a torch int64 cumulative-sum
    reference along the two strided slices, in row chunks, with the truncating division of
    tests/bigsignal_ref.py; oracle spot rows."""
    import torch
    dsp = _dsp()
    R, L, k = (1 << 15) + 2, (1 << 16) + 3, 1024
    lengths = np.where(np.arange(R) % 2 == 0, L - 1, L + 1).astype(np.int64)
    off = offsets_of(lengths)
    N = int(off[-1])
    assert N == R * L and N > 1 << 31
    assert dsp.ragged_plan(off, k, 1, dsp.I16).startswith(SCAN)
    x = dsp.fill_synthetic(N, dtype=torch.int16, seed=0xB16, device=gpu)
    y = dsp.moving_average_ragged(x, k, offsets=off)
    x2, y2 = x.view(R // 2, 2 * L), y.view(R // 2, 2 * L)
    bad, rc = 0, 256
    for r0 in range(0, R // 2, rc):
        for sl in (slice(0, L - 1), slice(L - 1, 2 * L)):
            P = x2[r0:r0 + rc, sl].to(torch.int64).cumsum(1)
            S = P.clone()
            S[:, k:] -= P[:, :-k]
            del P
            bad += int((torch.div(S, k, rounding_mode="trunc").to(torch.int16) != y2[r0:r0 + rc, sl]).sum())
            del S
    assert bad == 0, f"{bad} mismatches"
    mid = int(np.searchsorted(off, 1 << 31, side="right")) - 1  # the row holding flat sample 2^31
    assert off[mid] <= 1 << 31 < off[mid + 1]
    for r in (0, mid, R - 1):
        a, b = int(off[r]), int(off[r + 1])
        assert np.array_equal(y[a:b].cpu().numpy(), oracle_mod.mavg_i16(x[a:b].cpu().numpy(), k, 1)), r


# ---- 14. debug build ----
CHILD = r'''
import sys
sys.path.insert(0, "tests")
import torch
import oracle
import test_gpu_ragged as t
from digital_signal_processsing_amd import _lib
oracle.build()
_lib.load()
maps = open("/proc/self/maps").read()
assert "libmavg_debug.so" in maps and "lib/libmavg.so" not in maps, "the debug build must be the one loaded"
n = t.run_debug_cases(torch.device("cuda:0"), oracle)
torch.cuda.synchronize()
print("ragged debug build ok", n)
'''


@pytest.mark.gpu
@pytest.mark.timeout(200)
def test_debug_build_runs_the_ragged_cases_clean(gpu):
    """Cases 1 to 3 on lib/libmavg_debug.so: no device check (mask indices, stage and x[n-k]
    indices, each lane's distance against a direct search of the offsets) fires -- a firing check
    traps the kernel and the child fails -- and every output matches the oracle."""
    r = subprocess.run([sys.executable, "-u", "-c", CHILD], cwd=ROOT, env=dict(os.environ, MAVG_LIBRARY=DEBUG_LIB),
                       capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "ragged debug build ok" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "mavg debug check failed" not in r.stdout + r.stderr
