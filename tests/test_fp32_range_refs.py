"""CPU test of what tests/test_gpu_fp32_range.py relies on: its signals are exact scalings, and
every reference it compares a kernel with obeys the scaling law on exactly those signals (bitwise
for the fp32 references oracle.mavg_f32, fir_chain and the extrema; exactly in float64 for ema_ref,
biquad_ref and stat_ref_f32) -- so a failure on the GPU points at the kernel.  It also runs the two
numpy models of stat_value's last step: the fp32 root of an fp32 mean square (what the kernel did
before) is non-finite on `up` and zero on `down`; the fp64 root rounded once, and the fp32 root of
the value rescaled by an even power of two (what the kernel does), pass everywhere."""
import numpy as np
import pytest

import stat_ref
from biquad_ref import biquad_bar, biquad_gain, biquad_ref, biquad_scale, rbj
from ema_ref import ema_ref
from extrema_ref import moving_extrema_ref
from fir_ref import fir_chain
from fp32_range import (FLT_MAX, NORMAL_MIN, QUANTUM, assert_finite_where_ref_is, assert_scaling_law, assert_stat_close, bases,
                        root_after_rounding, root_before_rounding, root_rescaled, signals, top_signals)
from stat_ref import MEANSQ, RMS, STD, VAR

FRAMES, SEED = 6161, 3
LP = rbj("LP", 0.05, 0.7071)


@pytest.fixture(scope="module")
def family(oracle_mod):
    return signals(bases(oracle_mod, FRAMES, SEED))


def test_signals_are_exact_scalings_in_the_stated_ranges(family):
    assert [s.name for s in family] == ["up", "mid-up", "up", "down", "subnormal"]
    for s in family:
        assert np.array_equal(s.x.astype(np.float64), s.base.astype(np.float64) * 2.0 ** s.e), s
        top = float(np.abs(s.x).max())
        nz = np.abs(s.x[s.x != 0]).astype(np.float64)
        if s.name == "up":
            assert 2.0 ** 99 <= top <= 2.0 ** 100 and top * top > FLT_MAX, s
        elif s.name == "mid-up":
            assert 2.0 ** 59 <= top <= 2.0 ** 60, s
        elif s.name == "down":
            assert nz.min() >= 2.0 ** -110 and nz.max() <= 2.0 ** -95 and nz.min() >= NORMAL_MIN, s
        else:
            assert nz.max() <= 2.0 ** -125 and (nz < NORMAL_MIN).mean() > 0.5, s
            assert np.array_equal(nz / QUANTUM, np.round(nz / QUANTUM)), s
    t = top_signals(5, 2)
    assert (t["constant"] == np.float32(FLT_MAX)).all()
    assert t["alternating"].tolist() == [FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX] * 2 + [FLT_MAX, FLT_MAX]


@pytest.mark.parametrize("k", (7, 100, 1024))
def test_the_moving_average_oracle_scales_bitwise(oracle_mod, family, k):
    base = {d: oracle_mod.mavg_f32(s.base, k, 1) for d, s in ((s.dist, s) for s in family)}
    for s in family:
        n = assert_scaling_law(base[s.dist], oracle_mod.mavg_f32(s.x, k, 1), s.e, (s, k))
        assert s.name == "subnormal" or n > FRAMES // 2, (s, k, n)      # subnormal: few or no normal outputs


def test_fir_chain_and_the_extrema_scale_bitwise(family):
    h = np.random.default_rng(1065).standard_normal(65).astype(np.float32).astype(np.float64)
    base = {s.dist: (fir_chain(s.base, h), moving_extrema_ref(s.base, 100)) for s in family}
    for s in family:
        y0, (hi0, lo0) = base[s.dist]
        assert_scaling_law(y0, fir_chain(s.x, h), s.e, (s, "fir"))
        hi, lo = moving_extrema_ref(s.x, 100)
        assert np.array_equal(hi.astype(np.float64), hi0.astype(np.float64) * 2.0 ** s.e), s      # exact, subnormals too
        assert np.array_equal(lo.astype(np.float64), lo0.astype(np.float64) * 2.0 ** s.e), s


def test_ema_and_biquad_references_scale_exactly_in_float64(family):
    st = np.array([0.75])
    sq = np.array([[0.5, -0.25]])
    for s in family:
        amp = float(np.abs(s.base).max())
        for fast in (False, True):
            y0, so0 = biquad_ref(s.base, LP, 1, sq * amp, fast=fast)
            ys, sos = biquad_ref(s.x, LP, 1, sq * amp * 2.0 ** s.e, fast=fast)
            assert_scaling_law(y0, ys, s.e, (s, "biquad", fast))
            assert_scaling_law(so0, sos, s.e, (s, "biquad state", fast))
        for alpha in (0.05, 1e-3):
            assert_scaling_law(ema_ref(s.base, alpha, 1, st * amp), ema_ref(s.x, alpha, 1, st * amp * 2.0 ** s.e), s.e, (s, "ema"))
    # the bar's own scale follows the signal
    s = family[0]
    assert biquad_scale(s.x) == biquad_scale(s.base) * 2.0 ** s.e
    assert np.isfinite(biquad_bar(np.ones(1), biquad_gain(LP), biquad_scale(s.x))).all()


@pytest.mark.parametrize("k", (7, 100, 1024))
def test_the_moments_reference_scales_exactly_in_float64(family, k):
    base = {}
    for s in family:
        for stat in (MEANSQ, RMS, VAR, STD):
            if (s.dist, stat) not in base:
                base[(s.dist, stat)] = stat_ref.stat_ref_f32(s.base, k, stat)
            y0, m0, M0 = base[(s.dist, stat)]
            y, m, M = stat_ref.stat_ref_f32(s.x, k, stat)
            assert_scaling_law(y0, y, s.e, (s, k, stat), power=2 if stat in (MEANSQ, VAR) else 1)
            assert_scaling_law(m0, m, s.e, (s, k, stat, "mean"))
            assert_scaling_law(M0, M, s.e, (s, k, stat, "M"), power=2)


@pytest.mark.parametrize("k", (7, 100))
def test_the_fp32_root_of_an_fp32_moment_fails_and_the_fp64_root_passes(family, k):
    """The model of stat_value before the root moved in front of the rounding, on stat_ref_f32's own
    fp64 value: +Inf on `up` although the root is near 2^100, 0 on `down`; the fp64 root rounded once
    and the kernel's rescaled fp32 root meet the bar on every signal, and the rescaled root obeys the
    scaling law and gives the old order's bits wherever that order's fp32 moment was a normal number."""
    for s in family:
        for root_stat, moment in ((RMS, MEANSQ), (STD, VAR)):
            ref, _, M = stat_ref.stat_ref_f32(s.x, k, root_stat)
            v, _, _ = stat_ref.stat_ref_f32(s.x, k, moment)
            old = root_after_rounding(v)
            what = (s, k, root_stat)
            for new in (root_before_rounding(v), root_rescaled(v)):
                assert_stat_close(root_stat, new, ref, M, s.q, what)
                assert_finite_where_ref_is(new, ref, what)
            v0 = stat_ref.stat_ref_f32(s.base, k, moment)[0]
            assert_scaling_law(root_rescaled(v0), root_rescaled(v), s.e, what)
            assert np.array_equal(root_rescaled(v0), root_after_rounding(v0)), what      # the base: ordinary magnitudes
            if s.name == "up":
                assert np.isinf(old[k:]).mean() > 0.9 and np.isfinite(ref).all() and float(ref.max()) < 2.0 ** 101, what
                with pytest.raises(AssertionError):
                    assert_finite_where_ref_is(old, ref, what)
            elif s.name == "down":
                assert (old == 0).all() and (ref[k:] > 2.0 ** -115).mean() > 0.9, what
                with pytest.raises(AssertionError):
                    assert_stat_close(root_stat, old, ref, M, s.q, what)
            elif s.name == "mid-up":
                assert_stat_close(root_stat, old, ref, M, s.q, what)      # where the old order was tested: it passes
