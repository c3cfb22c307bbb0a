"""The reference of the moving second moment (mavg_stat_run, include/mavg.h): a numpy restatement
of the definitions, shared by tests/test_stat_model.py and tests/test_gpu_stat.py.

Per channel, S1 and S2 are the sums of x and x^2 over the k frames ending at frame f; frames before
frame 0 are zero, or the k - 1 history frames.  int16: exact integers (int64 prefix sums; N = k S2 -
S1^2 in Python integers), then fp64, then fp32.  fp32: prefix sums of x and of x^2 per channel, the
differences rounded to float64 -- in exact integer arithmetic (x 2^149 is an integer for every
float32), not in float64: a float64 prefix carries about 1e-16 of the WHOLE prefix, which on the
mixed-scale input is 1e-2 of a quiet window's mean square (measured: a window of two samples near
1e-5 after 6000 frames near 1), and the bars are 1e-5 of the window's own.  The exact reference
asks no less of the code than the float64 one would."""
import math

import numpy as np

MEANSQ, RMS, VAR, STD = 0, 1, 2, 3
STATS = {"meansq": MEANSQ, "rms": RMS, "var": VAR, "std": STD}


def _framed(x, C, hist, k):
    xf = np.asarray(x).reshape(-1, C)
    pre = np.zeros((k, C), dtype=xf.dtype)
    if hist is not None:
        h = np.asarray(hist).reshape(-1, C)
        assert h.shape[0] == k - 1, (h.shape, k)
        pre[1:] = h
    return np.concatenate([pre, xf])


def window_sums(x, k, C=1, hist=None):
    """(S1, S2) as [frames, C]: int64 (exact) for int16 input, float64 for float32 input."""
    long = _framed(x, C, hist, k)
    exact_f32 = long.dtype != np.int16
    if exact_f32:    # Python integers: x 2^149, exactly
        assert long.dtype == np.float32 and np.isfinite(long).all()
        a = np.array([int(v) for v in (long.astype(np.float64) * 2.0 ** 149).ravel()], dtype=object).reshape(long.shape)
    else:
        a = long.astype(np.int64)
    z = np.zeros((1, C), dtype=a.dtype)
    P1 = np.concatenate([z, np.cumsum(a, axis=0)])
    P2 = np.concatenate([z, np.cumsum(a * a, axis=0)])
    S1, S2 = P1[k + 1:] - P1[1:-k], P2[k + 1:] - P2[1:-k]
    if exact_f32:    # one rounding each
        S1 = np.array([math.ldexp(float(v), -149) for v in S1.ravel()], dtype=np.float64).reshape(S1.shape)
        S2 = np.array([math.ldexp(float(v), -298) for v in S2.ravel()], dtype=np.float64).reshape(S2.shape)
    return S1, S2


def exact_n(S1, S2, k):
    """N = k S2 - S1^2 as Python integers (an object array): exact for every k."""
    return S2.astype(object) * int(k) - S1.astype(object) * S1.astype(object)


def _f64(obj):
    return np.array([float(v) for v in obj.ravel()], dtype=np.float64).reshape(obj.shape)


def stat_ref_i16(x, k, stat, C=1, hist=None):
    """(y, mean) as float32 [frames, C]: the fp32 rounding of the fp64 evaluation."""
    S1, S2 = window_sums(np.asarray(x, dtype=np.int16), k, C, hist)
    if stat in (MEANSQ, RMS):
        v = S2.astype(np.float64) / float(k)            # S2 < 2^61: int64 -> float64 rounds correctly
    else:
        if k <= 65535:                                  # both products below 2^62: int64 is exact
            N = (np.int64(k) * S2 - S1 * S1).astype(np.float64)
        else:
            N = _f64(exact_n(S1, S2, k))
        assert (N >= 0).all()                           # Cauchy-Schwarz
        v = N / (float(k) * float(k))
    if stat in (RMS, STD):
        v = np.sqrt(v)
    return v.astype(np.float32), (S1.astype(np.float64) / float(k)).astype(np.float32)


def stat_ref_f32(x, k, stat, C=1, hist=None):
    """(y, mean, M) as float64 [frames, C]: the statistic, the window mean and the window's mean
    square M (what the fp32 tolerances scale with)."""
    S1, S2 = window_sums(np.asarray(x, dtype=np.float32), k, C, hist)
    M = np.maximum(S2 / k, 0.0)
    m = S1 / k
    v = M if stat in (MEANSQ, RMS) else np.maximum(M - m * m, 0.0)
    if stat in (RMS, STD):
        v = np.sqrt(v)
    return v, m, M


def check_i16(y, ref, what=""):
    """|y - ref| <= one fp32 ulp at ref, and exactly 0.0f where ref == 0: y and ref are fp32
    roundings of fp64 values that agree to a few 2^-52, so they differ only across a rounding
    boundary."""
    assert y.dtype == np.float32 and ref.dtype == np.float32 and y.shape == ref.shape, (what, y.dtype, y.shape, ref.shape)
    ulp = np.spacing(np.abs(ref))
    bad = ~(np.abs(y.astype(np.float64) - ref.astype(np.float64)) <= ulp.astype(np.float64))
    bad |= (ref == 0) & (y != 0)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} mismatches, first at {i}: got {y[i]!r}, want {ref[i]!r}")


def check_f32(stat, y, ref, M, what=""):
    """The fp32 bars of include/mavg.h: 1e-5 relative for MEANSQ and RMS; VAR within 1e-5 of the
    window's mean square M; STD: |y^2 - ref^2| <= 1e-5 M + 2^-22 ref^2 (VAR's bar on the square, plus
    the roundings of the root: the fp32 root of the variance rounded to fp32 at a rescaled exponent,
    1.5 * 2^-24 relative in all), finite and >= 0."""
    assert y.dtype == np.float32 and y.shape == ref.shape, (what, y.dtype, y.shape, ref.shape)
    y64 = y.astype(np.float64)
    if stat in (MEANSQ, RMS):
        bad = ~(np.abs(y64 - ref) <= 1e-5 * ref)
    elif stat == VAR:
        bad = ~(np.abs(y64 - ref) <= 1e-5 * M) | ~(y64 >= 0)
    else:
        bad = ~(np.abs(y64 * y64 - ref * ref) <= 1e-5 * M + 2.0 ** -22 * ref * ref) | ~np.isfinite(y64) | ~(y64 >= 0)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} mismatches, first at {i}: got {y[i]!r}, want {ref[i]!r} (M {M[i]!r})")


# ---- a signal that falls silent (the fp32 dynamic-range clauses of include/mavg.h) ----
LOUD, QUIET = 1e15, 1e-4      # loud amplitudes 0.5 .. 1.5 LOUD (squares near 1e30); quiet: dist 2 times QUIET (about 1e-3 and below)


def falls_silent(oracle, C, frames, loud_frames, seed=0):
    """fp32 [frames * C]: the first loud_frames frames near +-1e15, the rest the mixed-scale (dist 2)
    generator scaled to about 1e-3 -- a drop of 360 dB."""
    rng = np.random.default_rng(seed)
    x = oracle.synth_f32(frames * C, seed=77 + seed, dist=2).astype(np.float64) * QUIET
    n = loud_frames * C
    x[:n] = LOUD * rng.uniform(0.5, 1.5, n) * rng.choice((-1.0, 1.0), n)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def summation_bound(y, k, S2, sigma, nterms):
    """The textbook bound on a window sum of squares formed from `nterms` fp64 terms whose absolute
    values sum to `sigma`, read back from the MEANSQ output y = fl32(s2 / k):
    |y k - S2| <= nterms 2^-53 sigma + 2^-24 y k.  Returns the violations."""
    yk = y.astype(np.float64) * k
    return ~(np.abs(yk - S2) <= nterms * 2.0 ** -53 * sigma + 2.0 ** -24 * yk)
