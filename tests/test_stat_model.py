"""CPU model of the moving second moment's arithmetic (csrc/mavg_stat.hpp) against the direct
definition: the tile kernel's halo reduction plus tile-local prefix of x^2 - x[n-k]^2 (wrapped
int64 / fp64) and of x - x[n-k] (wrapped int32 / fp64), N = k S2 - S1^2 in int64, the clamp, and the
strip kernel's direct sum and slide.  No GPU."""
import numpy as np
import pytest

import stat_ref


def load_elem(x, hist, f, k):
    """csrc/mavg_device.hpp load_elem, one channel: history in front of frame 0, zeros elsewhere."""
    if f >= 0:
        return x[f] if f < len(x) else 0
    if hist is not None and f >= -(k - 1):
        return hist[f + k - 1]
    return 0


def direct(x, k, hist=None):
    """(S1, S2) per frame as Python integers / float64 by the definition: a sum over the window."""
    exact = x.dtype == np.int16
    S1, S2 = [], []
    for f in range(len(x)):
        w = [load_elem(x, hist, j, k) for j in range(f - k + 1, f + 1)]
        w = [int(v) for v in w] if exact else np.array(w, dtype=np.float64)
        S1.append(sum(w) if exact else float(np.sum(w)))
        S2.append(sum(v * v for v in w) if exact else float(np.sum(w * w)))
    return S1, S2


def tile_model(x, k, TF, hist=None):
    """stat_tile_kernel's sums, one channel: per tile the halo's S1 and S2, then the prefix of the
    differences -- int16 in int32 (mod 2^32) and int64 (mod 2^64), fp32 in float64."""
    exact = x.dtype == np.int16
    A1, A2 = (np.int32, np.int64) if exact else (np.float64, np.float64)
    n = len(x)
    S1 = np.zeros(n, dtype=A1)
    S2 = np.zeros(n, dtype=A2)
    with np.errstate(over="ignore"):
        for t0 in range(0, n, TF):
            stage = np.array([load_elem(x, hist, f, k) for f in range(t0 - k, min(t0 + TF, n))], dtype=x.dtype)
            halo, tile, xk = stage[:k], stage[k:], stage[:-k]
            h1 = halo.astype(A1).sum(dtype=A1)
            h2 = (halo.astype(A2) * halo.astype(A2)).sum(dtype=A2)
            d1 = tile.astype(A1) - xk.astype(A1)
            if exact:   # x^2 - x[n-k]^2 formed in int32 (|d| <= 2^30), accumulated in int64
                d2 = (tile.astype(np.int32) * tile.astype(np.int32) - xk.astype(np.int32) * xk.astype(np.int32)).astype(A2)
            else:
                d2 = tile.astype(A2) * tile.astype(A2) - xk.astype(A2) * xk.astype(A2)
            S1[t0:t0 + TF] = h1 + np.cumsum(d1, dtype=A1)
            S2[t0:t0 + TF] = h2 + np.cumsum(d2, dtype=A2)
    return S1, S2


def strip_model(x, k, L, hist=None):
    """stat_strip_kernel's sums, one channel: a direct sum over the k frames before the strip, then
    the slide (int64 / float64)."""
    exact = x.dtype == np.int16
    conv = int if exact else float
    S1, S2 = [], []
    for f0 in range(0, len(x), L):
        s1 = s2 = conv(0)
        for f in range(f0 - k, f0):
            v = conv(load_elem(x, hist, f, k))
            s1 += v
            s2 += v * v
        for f in range(f0, min(f0 + L, len(x))):
            a, b = conv(x[f]), conv(load_elem(x, hist, f - k, k))
            s1 += a - b
            s2 += a * a - b * b
            S1.append(s1)
            S2.append(s2)
    return S1, S2


def rng_i16(n, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.int16)


@pytest.mark.parametrize("k,TF,with_hist", [(2, 16, False), (7, 16, True), (16, 16, False), (37, 16, True), (100, 64, False)])
def test_tile_model_matches_the_definition_int16(k, TF, with_hist):
    x = rng_i16(3 * TF + 17, k)
    x[:5] = -32768                                  # full scale, both signs
    x[5:9] = 32767
    hist = rng_i16(k - 1, k + 1) if with_hist else None
    S1, S2 = tile_model(x, k, TF, hist)
    D1, D2 = direct(x, k, hist)
    assert [int(v) for v in S1] == D1 and [int(v) for v in S2] == D2
    # the shared reference (prefix sums) says the same, and N is what Python integers give
    R1, R2 = stat_ref.window_sums(x, k, 1, hist)
    assert R1[:, 0].tolist() == D1 and R2[:, 0].tolist() == D2
    N = np.int64(k) * S2 - S1.astype(np.int64) * S1.astype(np.int64)
    assert N.tolist() == [k * b - a * a for a, b in zip(D1, D2)] and (N >= 0).all()


def test_tile_prefix_wraps_mod_2_32_and_still_gives_the_window_sum():
    """k = 65535 frames of -32768 then 32767: inside one (model) tile the prefix of x - x[n-k] passes
    2^31 in magnitude; the int32 sum wraps and halo + prefix is the window sum all the same."""
    k = 65535
    x = np.concatenate([np.full(k, -32768), np.full(k + 3, 32767)]).astype(np.int16)
    S1, S2 = tile_model(x, k, 1 << 18)
    R1, R2 = stat_ref.window_sums(x, k)
    assert np.array_equal(S1.astype(np.int64), R1[:, 0]) and np.array_equal(S2, R2[:, 0])
    assert R1.min() == -32768 * k and R1.max() == 32767 * k and abs(R1.max() - R1.min()) > 2 ** 31


def test_extremes_all_minus_full_scale_at_k_65535():
    k = 65535
    S1, S2 = -32768 * k, (1 << 30) * k            # the window of equal samples
    assert S2 < 1 << 46 and abs(S1) < 1 << 31
    a, b = k * S2, S1 * S1
    assert a < 1 << 62 and b < 1 << 62 and a - b == 0
    n = np.int64(k) * np.int64(S2) - np.int64(S1) * np.int64(S1)   # the kernel's int64 form: no overflow
    assert int(n) == 0
    x = np.full(2 * k + 17, -32768, dtype=np.int16)
    for stat in (stat_ref.VAR, stat_ref.STD):
        y, mean = stat_ref.stat_ref_i16(x, k, stat)
        assert (y[k - 1:] == 0).all() and y.dtype == np.float32
        assert (mean[k - 1:] == -32768).all()
    y, _ = stat_ref.stat_ref_i16(x, k, stat_ref.RMS)
    assert (y[k - 1:] == 32768).all()


def test_forming_n_in_fp64_first_would_be_wrong():
    """k S2 alone is past 2^53: rounding the two products to fp64 before the subtraction loses N.
    The exact N is small beside them -- a near-constant window -- and int64 keeps it."""
    k = 65535
    x = np.full(k, 32767, dtype=np.int16)
    x[0] = 32766
    S1, S2 = int(x.astype(np.int64).sum()), int((x.astype(np.int64) ** 2).sum())
    a, b = k * S2, S1 * S1
    N = a - b
    assert a > 1 << 53 and a < 1 << 62 and N == k - 1        # N = k sum (x - mean)^2 = k (1 - 1/k)
    assert int(np.int64(k) * np.int64(S2) - np.int64(S1) * np.int64(S1)) == N
    assert float(a) - float(b) != float(N)                    # what an fp64 N would have been
    y, _ = stat_ref.stat_ref_i16(np.concatenate([x, x]), k, stat_ref.VAR)
    assert y[k - 1] == np.float32(float(N) / (float(k) * float(k))) and y[k - 1] > 0


def test_past_65535_the_reference_keeps_python_integers():
    k = 65536
    x = rng_i16(k + 40, 3)
    S1, S2 = stat_ref.window_sums(x, k)
    N = stat_ref.exact_n(S1, S2, k)
    f = k + 7
    w = [int(v) for v in x[f - k + 1:f + 1]]
    assert int(N[f, 0]) == k * sum(v * v for v in w) - sum(w) ** 2
    assert all(isinstance(v, int) for v in N.ravel())         # Python integers: no width to overflow
    y, _ = stat_ref.stat_ref_i16(x, k, stat_ref.STD)
    assert np.isfinite(y).all() and y.dtype == np.float32


def test_the_clamp():
    """fp32: a constant window's S2/k - (S1/k)^2 is rounding noise of either sign; the clamp makes it a
    variance, and the root is finite."""
    x = np.full(4000, 1000.1, dtype=np.float32)
    S1, S2 = tile_model(x, 1000, 256)
    ms, m = S2 / 1000.0, S1 / 1000.0
    raw = ms - m * m
    assert (np.abs(raw[999:]) <= 1e-5 * ms[999:]).all()
    var = np.maximum(raw, 0.0)
    assert (var >= 0).all() and np.isfinite(np.sqrt(var)).all()
    # the rule itself: a negative difference clamps to +0, a positive one passes
    assert np.maximum(np.float64(-1e-9), 0.0) == 0.0 and np.maximum(np.float64(2.5), 0.0) == 2.5
    y, mean, M = stat_ref.stat_ref_f32(x, 1000, stat_ref.STD)
    assert (y >= 0).all() and np.isfinite(y).all() and (y[999:] <= np.sqrt(1e-5) * 1000.1).all()


@pytest.mark.parametrize("k,TF", [(3, 16), (16, 16), (50, 32)])
def test_tile_model_fp32_within_the_bars(k, TF):
    rng = np.random.default_rng(k)
    x = (rng.standard_normal(3 * TF + 17) * 10.0 ** rng.integers(-3, 4, 3 * TF + 17)).astype(np.float32)
    S1, S2 = tile_model(x, k, TF)
    D1, D2 = direct(x, k)
    M = np.array(D2) / k
    assert (np.abs(S2 / k - M) <= 1e-12 * np.maximum.accumulate(M)).all()
    var = np.maximum(S2 / k - (S1 / k) ** 2, 0.0)
    ref = np.maximum(M - (np.array(D1) / k) ** 2, 0.0)
    assert (np.abs(var - ref) <= 1e-5 * M + 1e-12 * np.maximum.accumulate(M)).all()


@pytest.mark.parametrize("k,L,with_hist", [(1, 16, False), (40, 16, False), (40, 16, True), (5, 16, True), (100, 25, False)])
def test_strip_model_with_a_boundary_inside_the_warm_up(k, L, with_hist):
    x = rng_i16(2 * k + 3 * L + 17, k + L)
    hist = rng_i16(k - 1, 9) if with_hist else None
    if k > L:
        assert L < k - 1                              # a strip starts inside the warm-up
    S1, S2 = strip_model(x, k, L, hist)
    D1, D2 = direct(x, k, hist)
    assert S1 == D1 and S2 == D2
    T1, T2 = tile_model(x, k, 32, hist)               # and the two kernels' sums agree exactly
    assert [int(v) for v in T1] == S1 and [int(v) for v in T2] == S2


# ---- a signal that falls silent: what include/mavg.h promises fp32 windows of more than 16 frames ----
def _meansq32(S2, k):
    """stat_value for MEANSQ: the clamp, then fp32."""
    return np.maximum(np.asarray(S2, dtype=np.float64) / k, 0.0).astype(np.float32)


@pytest.mark.parametrize("k", (17, 100, 256))
def test_models_on_a_signal_that_falls_silent(oracle_mod, k):
    """One and a half tiles near 1e15, then about 1e-3.  The exact reference first: its quiet
    windows equal a direct float64 sum (no residue of the loud prefix).  Then the tile model (running
    sums restarted per tile from the halo's direct sum) and the strip model (restarted per strip):
    (b) a tile whose halo is quiet -- it starts k frames or more after the last loud frame, so every
        tile that starts a full tile after it -- meets the ordinary bars against its own mean square;
        so does every strip that starts k frames or more after it;
    (c) everywhere else the implied window sum obeys the textbook bound over the terms that tile
        (strip) adds: the halo's k squares, then x^2 and x[n-k]^2 per frame."""
    TF = 256
    L = min(max(k // 4, 16), 2048)
    frames, loud = 4 * TF + 17, TF + TF // 2
    x = stat_ref.falls_silent(oracle_mod, 1, frames, loud)
    assert np.abs(x[:loud]).min() >= 0.4e15 and np.abs(x[loud:]).max() <= 2e-3
    ref, _, M = stat_ref.stat_ref_f32(x, k, stat_ref.MEANSQ)
    S2 = M[:, 0] * k
    x64 = x.astype(np.float64)
    for f in range(loud + k - 1, frames, 37):         # windows wholly in the quiet part, summed directly
        d = float(np.sum(x64[f - k + 1:f + 1] ** 2))
        assert abs(S2[f] - d) <= 1e-12 * d, (f, S2[f], d)
    sq = np.concatenate([np.zeros(k), x64 * x64])     # sq[k + f] = x[f]^2, zeros in front

    def terms(f0, f1):
        """(sum of |terms|, number of terms) the unit [f0, f1) adds: its halo, then x^2 and x[n-k]^2 per frame."""
        return sq[f0:f0 + k].sum() + sq[k + f0:k + f1].sum() + sq[f0:f1].sum(), k + 2 * (f1 - f0)

    for name, unit, (_, T2) in (("tile", TF, tile_model(x, k, TF)), ("strip", L, strip_model(x, k, L))):
        y = _meansq32(T2, k)
        assert np.isfinite(y).all() and (y >= 0).all()
        quiet_units = 0
        for f0 in range(0, frames, unit):
            f1 = min(f0 + unit, frames)
            if f0 - k >= loud:
                quiet_units += 1
                stat_ref.check_f32(stat_ref.MEANSQ, y[f0:f1, None], ref[f0:f1], M[f0:f1], (name, k, f0))
            sigma, n = terms(f0, f1)
            bad = stat_ref.summation_bound(y[f0:f1], k, S2[f0:f1], sigma, n)
            assert not bad.any(), (name, k, f0, int(bad.sum()))
        assert quiet_units >= 2, (name, quiet_units)
    # the bound is not vacuous: a float32 accumulator, or a halo sum that lost its loudest term, misses it
    f0 = TF
    sigma, n = terms(f0, 2 * TF)
    P32 = np.concatenate([np.zeros(k, np.float32), np.cumsum(x * x, dtype=np.float32)])
    assert stat_ref.summation_bound(_meansq32((P32[k:] - P32[:-k])[f0:2 * TF], k), k, S2[f0:2 * TF], sigma, n).any()
    lost = np.asarray(tile_model(x, k, TF)[1][f0:2 * TF]) - sq[f0:f0 + k].max()
    assert stat_ref.summation_bound(_meansq32(lost, k), k, S2[f0:2 * TF], sigma, n).any()
