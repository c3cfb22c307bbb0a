"""A numpy restatement of the fused cascade's tile decomposition (csrc/mavg_sos.hpp) with tiny tiles:
the staged halo of sum H_j frames, the shrinking ranges (section j starts H_(j-1) frames after
section j - 1 and its first H_j outputs are never read), each range scanned from a zero state in
runs of `run` frames per thread whose aggregates are combined with once-rounded powers of A (lanes,
then waves), the cut at frame 0 (state_in[j] exactly, or zeros), the state's entry into later tiles
as A^g state_in[j], and the state written by the tile that holds the last frame.  It must hold the
header's bar on random input, on the worst-case input and with a carried state.  No GPU; of the
library only mavg_sos_halo_frames, to tie the model's halos to the library's."""
import numpy as np
import pytest

import digital_signal_processsing_amd as dsp

from biquad_ref import FILTER_LIST, REAL_POLE_CASES, min_halo, rbj, state_horizon
from sos_ref import rows6, sos_bar, sos_min_halo, sos_ref, sos_state_bar, worst_case_input

LANES, WAVES = 4, 4          # a "workgroup" of 16 threads
TF = 256                     # frames of a tile


def mat_pow(coef, m):
    """A^m for A = [[-a1, 1], [-a2, 0]]: binary powers in long double, rounded once."""
    r = np.eye(2, dtype=np.longdouble)
    s = np.array([[-coef[3], 1.0], [-coef[4], 0.0]], dtype=np.longdouble)
    while m:
        if m & 1:
            r = r @ s
        m >>= 1
        if m:
            s = s @ s
    return r.astype(np.float64)


def run_pass(stage, a, nn, L, coef, s, write, last_i):
    """Every thread's recurrence over its run in lockstep; s: [threads, 2] in and out.  write: y over
    x.  Returns the state after stage frame last_i (None where no thread owns it)."""
    b0, b1, b2, a1, a2 = coef
    rec = None
    for i in range(L):
        act = i < nn
        idx = np.where(act, a + i, 0)
        x = stage[idx]
        y = b0 * x + s[:, 0]
        s1 = b1 * x - a1 * y + s[:, 1]
        s2 = b2 * x - a2 * y
        s[:, 0] = np.where(act, s1, s[:, 0])
        s[:, 1] = np.where(act, s2, s[:, 1])
        if write:
            stage[idx[act]] = y[act]
            hit = act & (a + i == last_i)
            if hit.any():
                rec = s[np.nonzero(hit)[0][0]].copy()
    return rec


def model(x, sos, state=None, halos=None):
    """(y as fp32, state_out [S, 2]) of a mono signal by the tile decomposition."""
    n, S = len(x), len(sos)
    halos = [min_halo(c) for c in sos] if halos is None else halos
    total = sum(halos)
    Hp = (total + 7) & ~7
    starts = [0]
    for j in range(S - 1):
        starts.append(starts[-1] + halos[j] + (Hp - total if j == 0 else 0))
    SF = Hp + TF
    WG = LANES * WAVES
    y = np.empty(n)
    so = np.zeros((S, 2))
    st = None if state is None else np.asarray(state, dtype=np.float64).reshape(S, 2)
    for t0 in range(0, n, TF):
        g0 = t0 - Hp
        stage = np.zeros(SF)
        lo, hi = max(0, g0), min(n, t0 + TF)
        stage[lo - g0:hi - g0] = x[lo:hi]
        z = max(0, Hp - t0)
        last_i = n - 1 - g0 if n - 1 - g0 < SF else -1
        for j, c in enumerate(sos):
            L = -(-(SF - starts[j]) // WG) | 1
            r = max(starts[j], z)
            g = g0 + r
            s0 = np.zeros(2)
            if st is not None and g < max(1, state_horizon(c)):
                s0 = st[j].copy() if g == 0 else mat_pow(c, g) @ st[j]
            a = r + np.arange(WG) * L
            nn = np.clip(SF - a, 0, L)
            agg = np.zeros((WG, 2))
            run_pass(stage, a, nn, L, c, agg, False, -1)
            lane_p = [mat_pow(c, L * e) for e in range(LANES)]           # A^(run lane)
            wave_p = [mat_pow(c, LANES * L * w) for w in range(WAVES)]   # A^(lanes run w)
            carry = np.zeros((WG, 2))
            tot = []
            for w in range(WAVES):
                b = agg[w * LANES:(w + 1) * LANES]
                tot.append(sum((lane_p[LANES - 1 - m] @ b[m] for m in range(LANES)), np.zeros(2)))
            for w in range(WAVES):
                cw = wave_p[w] @ s0 if w else s0.copy()
                for i in range(w):
                    cw = cw + (wave_p[w - 1 - i] @ tot[i] if w - 1 - i else tot[i])
                for l in range(LANES):
                    ex = sum((lane_p[l - 1 - m] @ agg[w * LANES + m] for m in range(l)), np.zeros(2))
                    carry[w * LANES + l] = lane_p[l] @ cw + ex
            rec = run_pass(stage, a, nn, L, c, carry, True, last_i)
            if rec is not None:
                so[j] = rec
        y[t0:hi] = stage[Hp:Hp + hi - t0]
    return y.astype(np.float32), so


def pick(seed, S):
    """S sections: RBJ filters of the list with f >= 0.05 (short halos for a quick model) and the
    real-pole cases."""
    rng = np.random.default_rng(seed)
    pool = [rbj(k, f, Q) for (k, f, Q) in FILTER_LIST if f >= 0.05 and Q <= 4.0] + list(REAL_POLE_CASES)
    return [pool[i] for i in rng.choice(len(pool), S, replace=False)]


def check(x, sos, state=None):
    # the model runs with the smallest valid halos; the library's are at least as long (the harsher truncation is modelled)
    assert dsp.sos_halo_frames(rows6(sos)) >= sos_min_halo(sos)
    ref, sref = sos_ref(x, sos, 1, state)
    y, so = model(x, sos, state)
    err = np.abs(y.astype(np.float64) - ref)
    bar = sos_bar(ref, sos, x, state)
    assert (err <= bar).all(), (float((err / bar).max()), int(np.argmax(err / bar)))
    serr = np.abs(so - sref.reshape(len(sos), 2)).max(axis=1)
    assert (serr <= sos_state_bar(sos, x, state)).all(), (serr, sos_state_bar(sos, x, state))
    return y, so, float((err / bar).max())


@pytest.mark.parametrize("S", [2, 3, 8])
def test_random_input_holds_the_bar(S):
    sos = pick(S, S)
    x = np.random.default_rng(S).standard_normal(3 * TF + 77).astype(np.float32).astype(np.float64)
    check(x, sos)


@pytest.mark.parametrize("S", [2, 3, 8])
def test_worst_case_input_holds_the_bar(S):
    """x = M sgn(h_total[t0 - j]) in front of the first tile that starts past sum H_j."""
    sos = pick(10 + S, S)
    H = sos_min_halo(sos)
    t0 = (H // TF + 1) * TF
    x = worst_case_input(sos, t0 + TF + 33, t0, M=1.0)
    check(x, sos)


@pytest.mark.parametrize("S", [2, 3, 8])
def test_carried_state_reproduces_the_one_shot(S):
    """Two unequal chunks, the second from the first's state: within the sum of the two bars of the
    one-shot reference; one cut inside the first tile, one past sum H_j."""
    sos = pick(20 + S, S)
    H = sos_min_halo(sos)
    n = (H // TF + 3) * TF + 41
    x = np.random.default_rng(30 + S).standard_normal(n).astype(np.float32).astype(np.float64)
    ref, sref = sos_ref(x, sos)
    for cut in (TF // 3, (H // TF + 1) * TF + 19):
        y1, s1, _ = check(x[:cut], sos)
        y2, s2, _ = check(x[cut:], sos, s1)
        y = np.concatenate([y1, y2]).astype(np.float64)
        bar = sos_bar(ref, sos, x) + sos_bar(ref, sos, x, s1)
        assert (np.abs(y - ref) <= bar).all()
        assert (np.abs(s2 - sref.reshape(S, 2)).max(axis=1) <= 2.0 * sos_state_bar(sos, x, s1)).all()


def test_cut_at_frame_zero_with_and_without_a_state():
    """Signals shorter than the halo: every range is cut at frame 0 and starts from state_in
    exactly (or from zeros) -- the model then is the serial recurrence, to one fp32 ulp."""
    sos = pick(5, 3)
    x = np.random.default_rng(5).standard_normal(50).astype(np.float32).astype(np.float64)
    assert len(x) < sos_min_halo(sos)
    _, so, _ = check(x, sos)
    ref, _ = sos_ref(x[:17], sos, 1, so)
    y, _ = model(x[:17], sos, so)
    assert (np.abs(y.astype(np.float64) - ref) <= np.spacing(np.abs(ref).astype(np.float32))).all()
    check(x[:17], sos, so)
    y1, _ = model(x[:1], sos)
    assert (np.abs(y1.astype(np.float64) - sos_ref(x[:1], sos)[0]) <= np.spacing(np.abs(x[:1]).astype(np.float32))).all()
