"""A Python model of the moving extrema's kernels (csrc/mavg_extrema.hpp), checked exactly against
the definition.  No GPU.

The model restates extrema_tile_kernel's decomposition with the unit size F and the tile's unit
count as parameters, so that it runs with tiny tiles: with k - 1 = qq F + rr the window of frame fr
of stage unit s is (1) the suffix of its first unit from its first frame (the array S, read at a
shifted index), (2) for fr < rr the whole unit s - qq (S at that unit's first frame), (3) the
qq - 1 whole units between, from two overlapping entries of the doubling table R_p built in place
in radix-4 steps, and (4) the prefix of its own unit; k <= F windows that lie in one unit come
from the unit itself, and F == 1 is term 3 alone.  Missing frames are copies of the nearest frame
(ext_load_elem).  extrema_strip_kernel's park-and-combine is modelled too.

Windows straddle every level: every grade from 2 to past the signal is run for each (F, tile)
shape, which contains F - 1, F, F + 1, every power of two of units +- 1 (the table's levels), the
tile and the tile + 1; with and without a history, and without one on an all-negative signal."""
import numpy as np
import pytest

from extrema_ref import identity, moving_extrema_ref, moving_extremum_ref


def literal(x, k, hist, want_max):
    """The definition, frame by frame: the window truncated at frame 0 unless a history is given."""
    op = max if want_max else min
    pre = list(hist) if hist is not None else []
    out = []
    for f in range(len(x)):
        w = [x[j] if j >= 0 else pre[j + k - 1] for j in range(f - k + 1, f + 1) if j >= 0 or pre]
        out.append(op(w))
    return out


def load_elem(x, hist, f, k):
    """ext_load_elem: the history, else a copy of the nearest frame of the signal."""
    n = len(x)
    if f >= n:
        f = n - 1
    if f >= 0:
        return x[f]
    if hist is not None and k > 1:
        return hist[max(f + k - 1, 0)]
    return x[0]


def floor_log2(v):
    return v.bit_length() - 1          # -1 for 0


def tile_model(x, k, F, TU, hist, want_max):
    """extrema_tile_kernel for one channel: units of F frames, tiles of TU units."""
    assert k >= 2
    op = max if want_max else min
    n = len(x)
    Hu = (k + F - 1) // F
    qq, rr = divmod(k - 1, F)
    assert Hu == qq + 1
    span = k if F == 1 else max(qq - 1, 0)
    levels = floor_log2(span)
    TF, NU = TU * F, Hu + TU
    out = [None] * n
    for t0 in range(0, n, TF):
        h0 = t0 - Hu * F
        units = [[load_elem(x, hist, h0 + s * F + fr, k) for fr in range(F)] for s in range(NU)]
        S, R = {}, []
        for s, xu in enumerate(units):                    # emit()
            run = None
            for fr in range(F - 1, -1, -1):
                run = xu[fr] if run is None else op(run, xu[fr])
                if F > 1 and s <= TU:
                    S[s * F + fr] = run
            R.append(run)
        lvl = 0
        while lvl < levels:                                # the doubling table, in place
            rad = 3 if levels - lvl >= 2 else 1
            d = 1 << lvl
            R = [op(R[e - q * d] for q in range(rad + 1) if e - q * d >= 0) for e in range(NU)]
            lvl += 2 if rad == 3 else 1
        w = (1 << levels) if levels >= 0 else 0
        for j in range(TU):
            s = Hu + j
            hi = s if F == 1 else s - 1
            base = None
            if levels >= 0:
                lo2 = hi - span + w
                assert lo2 - w + 1 >= 0 and lo2 <= hi < NU      # the kernel's debug check
                base = op(R[hi], R[lo2])
            xu = units[s]
            for fr in range(F):
                f = t0 + j * F + fr
                if f >= n:
                    continue
                if F == 1:
                    v = base
                elif k - 1 < F and fr >= rr:
                    v = op(xu[fr - rr:fr + 1])
                else:
                    e = s * F - (k - 1)
                    assert 0 <= e and e + F <= (TU + 1) * F     # inside the S stage
                    v = op(op(xu[:fr + 1]), S[e + fr])
                    if levels >= 0:
                        v = op(v, base)
                    if k - 1 >= F and fr < rr:
                        v = op(v, S[(j + 1) * F])
                out[f] = v
    return out


def strip_frames(k):
    return min(max(k // 4, 16), 2048)


def strip_model(x, k, hist, want_max, L=None, direct_max=16):
    """extrema_strip_kernel for one channel."""
    op = max if want_max else min
    n = len(x)
    L = L or strip_frames(k)
    out = [None] * n
    for f0 in range(0, n, L):
        f1 = min(f0 + L, n)
        if k <= direct_max:
            for f in range(f0, f1):
                out[f] = op([x[f]] + [load_elem(x, hist, g, k) for g in range(f - k + 1, f)])
            continue
        assert L <= k - 1
        run = load_elem(x, hist, f0 - 1, k)
        for g in range(f0 - 1, f0 - k, -1):
            run = op(run, load_elem(x, hist, g, k))
            if g + k - 1 < f1:
                out[g + k - 1] = run                      # parked
        run = x[f0]
        for f in range(f0, f1):
            run = op(run, x[f])
            out[f] = op(out[f], run)
    return out


def signal(n, seed, negative=False):
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    if negative:
        x = (-1 - np.abs(x.astype(np.int32)) // 2).astype(np.int16)   # every sample < 0
    return x


SHAPES = [(1, 8), (2, 4), (2, 7), (4, 4), (8, 3), (4, 16)]     # (F, tile units)


@pytest.mark.parametrize("F,TU", SHAPES)
@pytest.mark.parametrize("mode", ["nohist", "hist", "negative"])
def test_tile_model_equals_the_definition(F, TU, mode):
    n = 3 * TU * F + 5
    x = [int(v) for v in signal(n, 100 * F + TU, negative=mode == "negative")]
    for k in list(range(2, n + 4)) + [2 * n + 1]:
        hist = [int(v) for v in signal(k - 1, 7 * k)] if mode == "hist" else None
        for want_max in (True, False):
            got = tile_model(x, k, F, TU, hist, want_max)
            assert got == literal(x, k, hist, want_max), (F, TU, k, mode, want_max)
    if mode == "negative":                                 # zero padding would show as a 0 here
        assert max(tile_model(x, n + 1, F, TU, None, True)) < 0


def test_tile_model_at_the_named_grades():
    """The grades the GPU tests run, on a tile of 64 units: F - 1, F, F + 1, 63, 64, 65 units of
    halo (the table's level 6), the tile and one past it, and a window longer than the signal."""
    F, TU = 4, 64
    n = 2 * TU * F + 17
    x = [int(v) for v in signal(n, 5)]
    grades = {2, 3, F - 1, F, F + 1, 63, 64, 65, 64 * F - 1, 64 * F, 64 * F + 1, TU * F - 1, TU * F, TU * F + 1, n + 9}
    for k in sorted(g for g in grades if g >= 2):
        for want_max in (True, False):
            assert tile_model(x, k, F, TU, None, want_max) == literal(x, k, None, want_max), (k, want_max)


@pytest.mark.parametrize("mode", ["nohist", "hist", "negative"])
def test_strip_model_equals_the_definition(mode):
    n = 150
    x = [int(v) for v in signal(n, 3, negative=mode == "negative")]
    for k in [1, 2, 3, 15, 16, 17, 18, 33, 64, 65, 100, 149, 150, 151, 400]:
        hist = [int(v) for v in signal(k - 1, k)] if mode == "hist" else None
        for want_max in (True, False):
            assert strip_model(x, k, hist, want_max) == literal(x, k, hist, want_max), (k, mode, want_max)
    for k in range(17, 80):                                # every strip length the parking allows
        for L in {16, k - 1, max(k // 2, 1)}:
            assert strip_model(x, k, None, True, L=L) == literal(x, k, None, True), (k, L)
    assert strip_frames(17) <= 16 and all(strip_frames(k) <= k - 1 for k in range(17, 20000))


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
@pytest.mark.parametrize("C", [1, 2, 3])
def test_reference_methods_agree_with_the_definition(dtype, C):
    """tests/extrema_ref.py: sliding windows, doubling and the literal loop; identity padding."""
    rng = np.random.default_rng(C)
    n = 97
    x = rng.integers(-3000, 3000, n * C).astype(dtype)
    for k in (1, 2, 3, 8, 9, 31, 32, 33, 96, 97, 98, 200):
        for hist in (None, rng.integers(-3000, 3000, (k - 1) * C).astype(dtype)):
            for want_max in (True, False):
                a = moving_extremum_ref(x, k, C, hist, want_max, "sliding")
                b = moving_extremum_ref(x, k, C, hist, want_max, "doubling")
                assert a.dtype == x.dtype and np.array_equal(a, b)
                for c in range(C):
                    h = None if hist is None else list(hist[c::C])
                    assert list(a[c::C]) == literal(list(x[c::C]), k, h, want_max), (k, c, want_max)
    hi, lo = moving_extrema_ref(x, 5, C)
    assert np.array_equal(hi, moving_extremum_ref(x, 5, C)) and (lo <= hi).all()
    assert identity(np.int16, True) == -32768 and identity(np.int16, False) == 32767
    assert identity(np.float32, True) == -np.inf and identity(np.float32, False) == np.inf
    neg = -1 - np.abs(x)
    assert (moving_extremum_ref(neg, 50, C) < 0).all()     # truncated, not zero-padded
