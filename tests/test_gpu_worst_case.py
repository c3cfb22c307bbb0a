"""GPU tests of the truncating IIR tiles (ema_tile, biquad_tile) on the input that maximises what they
drop (tests/worst_case.py): x[j] = M sgn(h[t0 - j]) in front of the first tile that starts past the
halo H, so that the error at y[t0] is the whole dropped tail M sum_{n > H} |h[n]| and |y_ref[t0]| = G M.
On noise that tail mostly cancels; include/mavg.h bounds it by 2^-30 G M inside the bar

    |y - y_ref| <= 2^-23 |y_ref| + 2^-29 G M        (G = 1 for the EMA)

and says of the biquad's refined H that it rests on an allowance that is not derived.  This is the
direct test of the library's own H (mavg_ema_halo_frames, mavg_biquad_halo_frames) and of the kernels'
halo reduction.  tests/test_worst_case_model.py shows on the CPU that the numpy models hold the bars
at the smallest halo and that the input produces at least half the exact tail at t0.

fp32 with M = 1 and int16 with the pattern at 32767 / -32768, one and two channels (channel 1 the
negation), on 16-B-aligned views and one sample off alignment (the frame-unit form).  tile_frames and
halo_frames are read from the plan text; the signal is t0 plus one tile plus 17 frames.  The bars are
the header's, on every output and on d_state_out, through the guarded launches of test_gpu_ema.py and
test_gpu_biquad.py (plan token, guard regions, input unmodified).

An fp32 output carries its own rounding, up to 2^-24 |y_ref|, which at t0 is 2^6 times the dropped
tail.  So every case also runs the signal cut after frame t0: d_state_out is then the state after t0
in fp64 (for the EMA it is y[t0] itself) and shows the truncation alone.  It must hold the header's
bar for the state, and its error over G M is what DESIGN.md records as the measured headroom.

Controls: ema_chain, ema_strip, biquad_chain and biquad_strip forced on the same inputs.  They drop
nothing: their error at t0 is below 2^-40 G M beyond the output's fp32 rounding (half an ulp at
y_ref[t0]), and their d_state_out is within the header's 1e-12 M (EMA) and 2^-29 G M (biquad).  That
rounding is larger than the tail, so what shows that the controls drop nothing is again the fp64 state
of the signal cut after t0: within 1e-12 M for the EMA, and for the biquad within CONTROL_STATE = 2^-36
G M.  2^-40 cannot be asked of that comparison: at the low-pass with H at the 16-KiB limit (poles near
+1, rounding amplified by about 1 / theta^2) two fp64 evaluations of the reference recurrence itself,
the literal loop and scipy's lfilter, differ by 1.5e-12 G = 2^-39.3 G, and the numpy model of the chain
is 2.4e-12 G from the loop.  2^-36 is 16 times the former and is below every non-zero tail the tiles
drop here (the smallest, BP, is 2.3e-11 G M = 2^-35.3 G M); the observed value is printed."""
import numpy as np
import pytest

import test_gpu_biquad as B
import test_gpu_ema as E
from biquad_ref import biquad_gain, biquad_scale, impulse_loop, rbj
from ema_ref import ema_scale
from worst_case import as_f32, as_i16, ema_impulse, first_tile_past, worst_case_input

pytestmark = pytest.mark.gpu

KINDS = [("f32", 1), ("f32", 2), ("i16", 1), ("i16", 2)]
VIEWS = [(0, 0), (1, 1)]            # both views aligned; both one sample off: the frame-unit form
NEGATIVE_POLES = (1.0, 0.5, 0.25, 1.4, 0.45)
CONTROL_STATE = 2.0 ** -36          # x G M: the biquad controls' fp64 state after t0 (see above)
BIQUAD_FILTERS = [("LP", B.LP), ("HP", B.HP), ("BP", B.BP), ("PK", B.PK), ("FIR3", B.FIR3),
                  ("double", (1.0, 0.5, 0.25, -1.8, 0.81)), ("negative", NEGATIVE_POLES)]


def pattern(kind, C, x):
    return as_i16(x, C) if kind == "i16" else as_f32(x, C)


def control_bar(ref_t0, GM):
    """2^-40 G M, and the rounding of the fp32 output: half an fp32 ulp at the value being rounded."""
    v = np.abs(ref_t0) + 2.0 ** -40 * GM
    return 2.0 ** -40 * GM + 0.5 * np.spacing(v.astype(np.float32)).astype(np.float64)


# ---- EMA ----
def ema_alphas(kind, C, tf, F):
    """(label, alpha): the alphas of test_gpu_ema's test_tile_by_rule -- the last is the smallest the
    tile rule takes, a halo of exactly 16 KiB -- and alpha = 0.5."""
    hs = E.halos_of(kind, C, tf, F)
    assert hs[-1] == E.rule_boundary(kind, C)
    return [(f"H={h}", E.alpha_with_halo(h)) for h in hs] + [("0.5", 0.5)]


@pytest.mark.parametrize("kind,C", KINDS)
@pytest.mark.parametrize("off_in,off_out", VIEWS)
def test_ema_tile_on_its_worst_case(gpu, oracle_mod, kind, C, off_in, off_out):
    dsp = E._dsp()
    aligned = off_in == 0
    F = E.unit_frames(kind, C) if aligned else 1
    tf = E.tile_frames(kind, C, aligned)
    for label, a in ema_alphas(kind, C, tf, F):
        H = dsp.ema_halo_frames(a)
        plan = E.plan_of(kind, C, 1 << 20, a, aligned=aligned)
        assert plan.startswith(E.TILE) and E.plan_int(plan, "halo_frames") == H and E.plan_int(plan, "tile_frames") == tf, plan
        if label == "0.5":
            assert H == 30
        t0 = first_tile_past(H, tf)
        n = t0 + tf + 17
        x = pattern(kind, C, worst_case_input(ema_impulse(a, t0 + 1), t0, n))
        M = ema_scale(x)
        ref = E.reference(x, a, C).reshape(-1, C)
        kw = dict(off_in=off_in, off_out=off_out, form=F)
        y, _ = E.check(gpu, x, a, C, ref=ref.reshape(-1), family=E.TILE, **kw)         # the header's bars, every output and the state
        err = np.abs(y.reshape(-1, C)[t0].astype(np.float64) - ref[t0]).max() / M
        # the signal cut after t0: d_state_out is y[t0] in fp64
        cut = x[:(t0 + 1) * C]
        _, s = E.run(gpu, cut, a, C, family=E.TILE, **kw)
        serr = np.abs(s - ref[t0]).max() / M
        assert serr <= 2.0 ** -29, (kind, C, label, serr)
        print(f"worst case ema_tile {kind} C={C} F={F} alpha {label}: H={H} t0={t0} err[t0]/M={err:.3e} "
              f"state(t0) err/M={serr:.3e} tail d^(H+1)={(1.0 - a) ** (H + 1):.3e}")
        for path, fam in ((2, E.CHAIN), (3, E.STRIP)):
            with E.forced(path) as lib:
                yc, _ = E.check(gpu, x, a, C, ref=ref.reshape(-1), family=fam, library=lib, off_in=off_in, off_out=off_out)
                _, sc = E.run(gpu, cut, a, C, family=fam, library=lib, off_in=off_in, off_out=off_out)
            cerr = np.abs(yc.reshape(-1, C)[t0].astype(np.float64) - ref[t0])
            assert (cerr <= control_bar(ref[t0], M)).all(), (fam, kind, C, label, cerr.tolist())
            assert (np.abs(sc - ref[t0]) <= 1e-12 * M).all(), (fam, kind, C, label, "state at t0")


# ---- biquad ----
_impulses = {}


def impulse(coef, n):
    key = tuple(coef)
    if key not in _impulses or _impulses[key].size < n:
        _impulses[key] = impulse_loop(coef, n)
    return _impulses[key][:n]


def lp_near_the_limit(kind, C, F):
    """A low-pass whose library H lands within one unit of the 16-KiB tile limit."""
    lim = B.rule_boundary(kind, C)
    f_in, _ = B.lp_at_boundary(lim)
    coef = rbj("LP", f_in, 0.7071)
    H = B._dsp().biquad_halo_frames(coef)
    assert lim - max(F, 1) <= H <= lim, (H, lim)
    return coef


@pytest.mark.parametrize("kind,C", KINDS)
@pytest.mark.parametrize("off_in,off_out", VIEWS)
def test_biquad_tile_on_its_worst_case(gpu, oracle_mod, kind, C, off_in, off_out):
    dsp = B._dsp()
    aligned = off_in == 0
    F = B.unit_frames(kind, C) if aligned else 1
    tf = B.tile_frames(kind, C, aligned)
    for label, coef in BIQUAD_FILTERS + [("LP-limit", lp_near_the_limit(kind, C, B.unit_frames(kind, C)))]:
        H = dsp.biquad_halo_frames(coef)
        plan = B.plan_of(kind, C, 1 << 20, coef, aligned=aligned)
        assert plan.startswith(B.TILE) and B.plan_int(plan, "halo_frames") == H and B.plan_int(plan, "tile_frames") == tf, plan
        t0 = first_tile_past(H, tf)
        assert t0 > H
        n = t0 + tf + 17
        x = pattern(kind, C, worst_case_input(impulse(coef, t0 + 1), t0, n))
        G, M = biquad_gain(coef), biquad_scale(x)
        ref, rs = B.reference(x, coef, C)
        kw = dict(off_in=off_in, off_out=off_out, form=F)
        y, _ = B.check(gpu, x, coef, C, ref=(ref, rs), family=B.TILE, **kw)            # the header's bars, every output and the state
        r0 = ref.reshape(-1, C)[t0]
        assert (np.abs(r0) >= 0.99 * G * (M - 1.0 if kind == "i16" else M)).all()       # the largest output the filter gives
        err = np.abs(y.reshape(-1, C)[t0].astype(np.float64) - r0).max() / (G * M)
        cut = x[:(t0 + 1) * C]
        _, rcut = B.reference(cut, coef, C)
        _, s = B.run(gpu, cut, coef, C, family=B.TILE, **kw)
        serr = np.abs(s - rcut).max() / (G * M)
        assert serr <= 2.0 ** -29, (kind, C, label, serr)
        print(f"worst case biquad_tile {kind} C={C} F={F} {label}: H={H} t0={t0} err[t0]/(G M)={err:.3e} "
              f"state(t0) err/(G M)={serr:.3e}")
        for path, fam in ((2, B.CHAIN), (3, B.STRIP)):
            with B.forced(path) as lib:
                yc, _ = B.check(gpu, x, coef, C, ref=(ref, rs), family=fam, library=lib, off_in=off_in, off_out=off_out)
                _, sc = B.run(gpu, cut, coef, C, family=fam, library=lib, off_in=off_in, off_out=off_out)
            cerr = np.abs(yc.reshape(-1, C)[t0].astype(np.float64) - r0)
            assert (cerr <= control_bar(r0, G * M)).all(), (fam, kind, C, label, cerr.tolist())
            cserr = np.abs(sc - rcut).max() / (G * M)
            print(f"  control {fam.strip('< ')}: state(t0) err/(G M)={cserr:.3e}")
            assert cserr <= CONTROL_STATE, (fam, kind, C, label, "state at t0", cserr)
