"""Signals at the ends of the fp32 range, and what is asserted on them: shared by
tests/test_gpu_fp32_range.py (the kernels) and tests/test_fp32_range_refs.py (the references alone).

Every signal is a seeded base signal (oracle.synth_f32 dist 0: int16-valued, or dist 2: mixed-scale,
rounding) times a power of two, which is exact in fp32 while nothing overflows or becomes subnormal
with more bits than the format keeps:

    up         base * 2^e, max |x| in [2^99, 2^100): x^2 is near 2^200, past FLT_MAX
    mid-up     base * 2^e, max |x| in [2^59, 2^60): mean squares stay below 2^120
    down       dist 0 * 2^-110: nonzero magnitudes in [2^-110, 2^-95], all normal; x^2 is below 2^-149
    subnormal  dist 0 * 2^-140: multiples of 2^-140 of magnitude at most 2^-125, most subnormal
    top        constant FLT_MAX, and +-FLT_MAX alternating per frame

dist 2 is not scaled down: its small samples would become subnormal and the scaling itself round.

The scaling law.  A kernel that does all arithmetic in fp64 with constants that do not depend on the
data, and rounds every output once, multiplies every intermediate by exactly 2^e when its input is
multiplied by 2^e (fp64 has exponent range to spare: nothing here leaves [2^-300, 2^300]).  So
out(x 2^e) == out(x) 2^e as values, with no tolerance, for every output that is a normal fp32 number
on both sides -- 2^(2e) for a second moment -- and for every fp64 output."""
import math

import numpy as np

FLT_MAX = float(np.finfo(np.float32).max)
NORMAL_MIN = 2.0 ** -126        # the smallest normal fp32 magnitude
QUANTUM = 2.0 ** -149           # one fp32 subnormal quantum: the absolute term where an output can be subnormal

SCALED = (("up", 2), ("mid-up", 2), ("up", 0), ("down", 0), ("subnormal", 0))   # (name, base dist)
TOP = {"up": 100, "mid-up": 60}     # max |x| in [2^(top-1), 2^top)
FIXED = {"down": -110, "subnormal": -140}


def exponent_of(name, base):
    """The e of signal `name` on `base`."""
    if name in FIXED:
        return FIXED[name]
    _, ex = math.frexp(float(np.abs(base).max()))      # max |base| in [2^(ex-1), 2^ex)
    return TOP[name] - ex


def scale(x, e):
    """x * 2^e in fp32, checked exact in float64."""
    y = np.ldexp(x, e).astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x.astype(np.float64) * 2.0 ** e), "the scaling rounded"
    y.setflags(write=False)
    return y


class Signal:
    """One scaled signal: `x` = `base` * 2^`e`; `q` is the absolute term of its bars (QUANTUM where
    outputs can be subnormal, else 0)."""

    def __init__(self, name, dist, base, e):
        self.name, self.dist, self.base, self.e = name, dist, base, e
        self.x = scale(base, e)
        self.q = QUANTUM if name == "subnormal" else 0.0

    def __repr__(self):
        return f"{self.name}(dist {self.dist}, 2^{self.e})"


def bases(oracle, n, seed):
    """{dist: base signal of n samples}, read-only."""
    out = {}
    for dist in (0, 2):
        b = oracle.synth_f32(n, seed=seed, dist=dist)
        b.setflags(write=False)
        out[dist] = b
    return out


def signals(base_by_dist):
    """The five scaled signals on the given bases."""
    out = []
    for name, dist in SCALED:
        b = base_by_dist[dist]
        out.append(Signal(name, dist, b, exponent_of(name, b)))
    return out


def top_signals(frames, C=1):
    """{name: fp32 [frames * C]}: constant FLT_MAX, and +-FLT_MAX alternating per frame."""
    m = np.float32(FLT_MAX)
    const = np.full(frames * C, m, dtype=np.float32)
    alt = np.where(np.arange(frames) % 2 == 0, m, -m).astype(np.float32).repeat(C)
    for a in (const, alt):
        a.setflags(write=False)
    return {"constant": const, "alternating": alt}


def assert_scaling_law(y0, ys, e, what, power=1):
    """ys == y0 * 2^(power e) as values: for an fp32 output wherever both sides are normal fp32
    numbers, for an fp64 output everywhere."""
    assert y0.shape == ys.shape and y0.dtype == ys.dtype, (what, y0.shape, ys.shape)
    want = y0.astype(np.float64) * 2.0 ** (power * e)       # exact: a power of two, far inside fp64's range
    got = ys.astype(np.float64)
    if y0.dtype == np.float32:
        a0, aw = np.abs(y0.astype(np.float64)), np.abs(want)
        both = (a0 >= NORMAL_MIN) & np.isfinite(y0) & (aw >= NORMAL_MIN) & (aw <= FLT_MAX)
    else:
        assert y0.dtype == np.float64
        both = np.ones(y0.shape, dtype=bool)
    bad = both & (got != want)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: the scaling law fails at {int(bad.sum())} of {int(both.sum())} outputs, first at {i}: "
                             f"got {ys[i]!r}, want {y0[i]!r} * 2^{power * e} = {want[i]!r}")
    return int(both.sum())


def assert_finite_where_ref_is(y, ref64, what):
    """(c): finite wherever the fp64 reference rounds to a finite fp32 number, exactly +Inf where it
    rounds to +Inf."""
    with np.errstate(over="ignore"):
        r32 = np.asarray(ref64, dtype=np.float64).astype(np.float32)
    assert not np.isnan(r32).any() and not (r32 == -np.inf).any(), what
    fin = np.isfinite(r32)
    bad = (fin & ~np.isfinite(y)) | (~fin & ~(y == np.inf))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} outputs are not finite where the reference is (or not +Inf where it "
                             f"is), first at {i}: got {y[i]!r}, reference {np.asarray(ref64)[i]!r}")


def window_mean_abs(x, k, C):
    """The window mean of |x| per frame and channel, float64 [frames, C]: the floor of the moving
    average's relative bar."""
    a = np.abs(x.astype(np.float64)).reshape(-1, C)
    P = np.concatenate([np.zeros((k, C)), np.cumsum(a, axis=0)])
    return (P[k:] - P[:-k]) / k


def assert_mean_close(y, ref, F, q, what):
    """The moving average's bar: |y - ref| <= 1e-5 max(|ref|, F) (+ q)."""
    y64, r64 = y.astype(np.float64).reshape(F.shape), ref.astype(np.float64).reshape(F.shape)
    bad = ~(np.abs(y64 - r64) <= 1e-5 * np.maximum(np.abs(r64), F) + q)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} mismatches, first at {i}: got {y64[i]!r}, want {r64[i]!r}")


def assert_stat_close(stat, y, ref, M, q, what):
    """stat_ref.check_f32 when q == 0; with q > 0 the same bars plus what an error of q in y adds:
    q for MEANSQ, RMS and VAR, 2 ref q + q^2 for STD's bar on y^2."""
    import stat_ref
    if q == 0:
        stat_ref.check_f32(stat, y, ref, M, what)
        return
    y64 = y.astype(np.float64)
    if stat in (stat_ref.MEANSQ, stat_ref.RMS):
        bad = ~(np.abs(y64 - ref) <= 1e-5 * ref + q)
    elif stat == stat_ref.VAR:
        bad = ~(np.abs(y64 - ref) <= 1e-5 * M + q) | ~(y64 >= 0)
    else:
        bar = 1e-5 * M + 2.0 ** -22 * ref * ref + 2.0 * ref * q + q * q
        bad = ~(np.abs(y64 * y64 - ref * ref) <= bar) | ~np.isfinite(y64) | ~(y64 >= 0)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} mismatches, first at {i}: got {y[i]!r}, want {ref[i]!r} (M {M[i]!r})")


# ---- numpy models of stat_value's last step (csrc/mavg_stat.hpp), on stat_ref_f32's fp64 value ----
def root_after_rounding(v64):
    """Before this test existed: the mean square (or variance) rounded to fp32, then the fp32 root."""
    with np.errstate(over="ignore"):
        return np.sqrt(np.maximum(v64, 0.0).astype(np.float32))


def root_before_rounding(v64):
    """The fp64 root, rounded once (the int16 overload; measured too slow for fp32 input)."""
    return np.sqrt(np.maximum(v64, 0.0)).astype(np.float32)


def root_rescaled(v64):
    """What the kernel does: v = w 2^ex with w in [0.5, 1) split as (w 2^(ex - 2h)) 4^h, h = floor(ex / 2),
    the first factor in [0.5, 2) rounded to fp32, its correctly rounded fp32 root, times 2^h (frexp
    and ldexp are exact).  0 leaves as 0 (here through w = 0, in the kernel through 2^-511)."""
    w, ex = np.frexp(np.maximum(v64, 0.0))
    h = ex >> 1
    return np.ldexp(np.sqrt(np.ldexp(w, ex - 2 * h).astype(np.float32)), h).astype(np.float32)
