"""The truncating IIR tiles on the input that maximises their truncation (tests/worst_case.py), on the
CPU: the numpy models of the kernels' decomposition (test_biquad_model.tile_path, test_ema_model.
model_tile) against the literal loops, at the smallest halo the contract allows.  They must hold the
bars of include/mavg.h, and the error at t0 must be at least half of what the halo drops -- which
shows that the input does what it is for (on noise the dropped tail mostly cancels).  No GPU, no library."""
import numpy as np
import pytest

import test_biquad_model as BM
import test_ema_model as EM
from biquad_ref import biquad_gain, biquad_loop, impulse_loop, min_halo, rbj, tail_after
from ema_ref import ema_loop
from worst_case import ema_impulse, first_tile_past, worst_case_input

FILTERS = {
    "LP": rbj("LP", 0.05, 0.7071), "HP": rbj("HP", 0.01, 0.7071), "BP": rbj("BP", 0.05, 4.0), "PK": rbj("PK", 0.25, 30.0),
    "FIR3": (0.25, 0.5, 0.25, 0.0, 0.0), "double": (1.0, 0.5, 0.25, -1.8, 0.81), "negative": (1.0, 0.5, 0.25, 1.4, 0.45),
}


def test_the_input_makes_every_term_positive():
    coef = FILTERS["BP"]
    t0, n = 700, 900
    h = impulse_loop(coef, t0 + 1)
    x = worst_case_input(h, t0, n, 3.0)
    assert set(np.abs(x).tolist()) == {3.0} and (x[t0 + 1:] == -x[t0:-1]).all()
    assert (x[:t0 + 1] * h[::-1] >= 0).all()
    y, _ = biquad_loop(x, coef)
    assert abs(y[t0] - 3.0 * np.abs(h).sum()) <= 1e-12 * 3.0 * biquad_gain(coef)
    assert abs(y[t0]) >= np.abs(y).max() * (1 - 1e-12)             # the largest output of all
    x0 = worst_case_input(np.zeros(5), 4, 8)                       # sgn(0) = +1
    assert x0.tolist() == [1, 1, 1, 1, 1, -1, 1, -1]
    assert (ema_impulse(0.25, 4) == 0.25 * 0.75 ** np.arange(4)).all()


@pytest.mark.parametrize("name", list(FILTERS))
def test_biquad_tile_model_on_its_worst_case(name):
    coef = FILTERS[name]
    F, NSEG = 2, 4
    TF = 64 * F * NSEG
    H = min_halo(coef)
    t0 = first_tile_past(H, TF)
    n = t0 + TF + 17
    x = worst_case_input(impulse_loop(coef, t0 + 1), t0, n)
    y, so = BM.tile_path(coef, x, None, F=F, NSEG=NSEG, H=H, state_frames=0)
    BM.check(coef, y, so, x, None, ("worst case", name, H))        # the header's bars, less the fp32 rounding
    ref, _ = biquad_loop(x, coef)
    G = biquad_gain(coef)
    Ha = -(-H // F) * F                                             # the model stages whole units
    dropped = tail_after(coef, Ha) - tail_after(coef, t0)           # sum over Ha < n <= t0 of |h[n]|
    err = abs(y[t0] - ref[t0])
    assert abs(ref[t0] - (G - tail_after(coef, t0))) <= 1e-12 * G   # |y_ref[t0]| = G M, less the part of h past the signal's start
    assert err >= 0.5 * dropped and err <= dropped + 2.0 ** -40 * G, (name, err / G, dropped / G)
    assert dropped <= 2.0 ** -30 * G
    if H > 8:
        assert dropped >= 2.0 ** -32 * G, (name, dropped / G)       # the truncation is really there
    print(f"{name}: H={H} t0={t0} err[t0]/(G M)={err / G:.2e} dropped/G={dropped / G:.2e} bar 2^-30={2.0 ** -30:.2e}")


@pytest.mark.parametrize("F,U,NW", [(2, 1, 4), (4, 2, 1), (1, 4, 1)])
@pytest.mark.parametrize("alpha", [0.5, 0.05, "halo=TF-1", "halo=TF+1"])
def test_ema_tile_model_on_its_worst_case(F, U, NW, alpha):
    TF = 64 * NW * F * U
    if isinstance(alpha, str):
        alpha = EM.alpha_for_halo(TF - 1 if alpha.endswith("-1") else TF + 1)
    d = 1.0 - alpha
    H = EM.halo_frames(alpha)                                        # the model's halo: the smallest with d^H <= 2^-30
    assert d ** H <= 2.0 ** -30 < d ** (H - 1)
    t0 = first_tile_past(H, TF)
    n = t0 + TF + 17
    x = worst_case_input(ema_impulse(alpha, t0 + 1), t0, n)
    assert (x[:t0 + 1] == 1.0).all()                                 # the EMA's worst case is a constant
    got, ref = EM.model_tile(x, alpha, F, U, NW), ema_loop(x, alpha)
    assert np.abs(got - ref).max() <= 2.0 ** -29, (alpha, np.abs(got - ref).max())
    Ha = -(-H // F) * F
    dropped = d ** (Ha + 1) - d ** (t0 + 1)                          # sum over Ha < n <= t0 of alpha d^n
    err = abs(got[t0] - ref[t0])
    assert err >= 0.5 * dropped and err <= dropped + 1e-12, (alpha, err, dropped)
    assert abs(ref[t0] - (1.0 - d ** (t0 + 1))) <= 1e-12
