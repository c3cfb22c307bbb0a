"""The reference of the cascade's tests (mavg_sos_run, include/mavg.h): the fp64 cascade with
states -- biquad_ref's loop chained with no rounding between sections -- the two accuracy bars of
the header, the section sets the tests share and the worst-case input for a cascade.  numpy only."""
import math

import numpy as np

from biquad_ref import biquad_gain, biquad_ref, min_halo, rbj


def sos_ref(x, sos, channels=1, state=None):
    """(y, state_out): fp64 y in x's interleaved layout through every row of sos (5-coefficient rows
    b0 b1 b2 a1 a2), fp64 between the sections, and the [S, channels, 2] states after the last frame."""
    S = len(sos)
    st = None if state is None else np.asarray(state, dtype=np.float64).reshape(S, channels, 2)
    so = np.zeros((S, channels, 2))
    y = np.asarray(x, dtype=np.float64).reshape(-1)
    for j, c in enumerate(sos):
        y, so[j] = biquad_ref(y, c, channels, None if st is None else st[j], fast=True)
    return y, so


def sos_gains(sos):
    return [biquad_gain(c) for c in sos]


def sos_levels(sos, x, state=None):
    """m_1 = max(max |x|, |state_in[1]|), m_(j+1) = max(G_j m_j, |state_in[j+1]|)."""
    G = sos_gains(sos)
    st = None if state is None else np.abs(np.asarray(state, dtype=np.float64)).reshape(len(sos), -1)
    m = [max(float(np.abs(np.asarray(x, dtype=np.float64)).max()) if np.size(x) else 0.0,
             float(st[0].max()) if st is not None else 0.0)]
    for j in range(1, len(sos)):
        m.append(max(G[j - 1] * m[j - 1], float(st[j].max()) if st is not None else 0.0))
    return m


def _pushed(sos, x, state, upto, unit, last=None):
    """sum over sections j <= upto (j < last where given) of unit * G_j m_j prod_{j < i <= upto} G_i"""
    G, m = sos_gains(sos), sos_levels(sos, x, state)
    tot = 0.0
    for j in range(upto + 1 if last is None else min(last, upto + 1)):
        tot += unit * G[j] * m[j] * math.prod(G[j + 1:upto + 1])
    return tot


def sos_abs_bar(sos, x, state=None, loop=False):
    """The absolute term of the output's bar: 2^-29 sum_j G_j m_j prod_{i>j} G_i; on sos_loop plus
    2^-24 of the same sum over the sections before the last."""
    S = len(sos)
    return _pushed(sos, x, state, S - 1, 2.0 ** -29) + (_pushed(sos, x, state, S - 1, 2.0 ** -24, S - 1) if loop else 0.0)


def sos_bar(ref, sos, x, state=None, loop=False):
    """|y - y_ref| <= 2^-23 |y_ref| + the absolute term, element-wise."""
    return 2.0 ** -23 * np.abs(ref) + sos_abs_bar(sos, x, state, loop)


def sos_state_bar(sos, x, state=None, loop=False):
    """[S]: the bar of every component of state_out[j] -- the same sum over the sections <= j."""
    return np.array([_pushed(sos, x, state, j, 2.0 ** -29) + (_pushed(sos, x, state, j, 2.0 ** -24, j) if loop else 0.0)
                     for j in range(len(sos))])


def sos_abs_bar_at(sos, M, state=None, loop=False):
    """sos_abs_bar from the level M = max |x| (and the state) instead of the signal: for a signal
    that never comes to the host.  m_1 = max(M, |state_in[1]|), so a one-sample signal M gives it."""
    return sos_abs_bar(sos, np.array([float(M)]), state, loop)


def sos_state_bar_at(sos, M, state=None, loop=False):
    """sos_state_bar from the level M = max |x| (and the state) instead of the signal."""
    return sos_state_bar(sos, np.array([float(M)]), state, loop)


def sos_min_halo(sos):
    """sum of the sections' smallest halos"""
    return sum(min_halo(c) for c in sos)


def sos_impulse(sos, n):
    x = np.zeros(n)
    x[0] = 1.0
    return sos_ref(x, sos)[0]


def worst_case_input(sos, n, t0, M=1.0, tail=None):
    """x[j] = M sgn(h_total[t0 - j]) for j <= t0: the input that maximises |y[t0]|, and with it what a
    tile starting at t0 drops by reading only its halo.  Frames past t0 are `tail` (default: the
    same sign pattern continued periodically, so the level stays M)."""
    assert n > t0
    h = sos_impulse(sos, t0 + 1)
    x = np.empty(n)
    sg = np.where(h >= 0.0, 1.0, -1.0)
    x[:t0 + 1] = M * sg[::-1]
    if n > t0 + 1:
        x[t0 + 1:] = tail if tail is not None else M * np.resize(sg, n - t0 - 1)
    return x


def butter4_lp(f):
    """A fourth-order Butterworth low-pass at f cycles per sample as two sections: the bilinear
    transform of the two analog pole pairs, Q = 1 / (2 cos(pi/8)) and 1 / (2 cos(3 pi/8))."""
    return [rbj("LP", f, 1.0 / (2.0 * math.cos(math.pi / 8.0))), rbj("LP", f, 1.0 / (2.0 * math.cos(3.0 * math.pi / 8.0)))]


def rows6(sos):
    """5-coefficient rows as scipy's [S, 6] rows (a0 = 1)."""
    return [[c[0], c[1], c[2], 1.0, c[3], c[4]] for c in sos]


def flat5(sos):
    return [float(v) for c in sos for v in c]


def one_pole(p):
    """y = (1 - p) x + p y[-1]: unit DC gain, a halo that grows with p."""
    return (1.0 - p, 0.0, 0.0, -p, 0.0)


def sections_with_halo(total, halo_of, base):
    """`base` and one more section -- a one-pole low-pass whose pole is found by bisection -- whose
    halos (halo_of: the library's mavg_biquad_halo_frames) sum to exactly `total` frames."""
    want = total - sum(halo_of(c) for c in base)
    assert want >= 1, want
    lo, hi = 0.0, 1.0 - 2.0 ** -20
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        if halo_of(one_pole(mid)) >= want:
            hi = mid
        else:
            lo = mid
    assert halo_of(one_pole(hi)) == want, (halo_of(one_pole(hi)), want)
    return list(base) + [one_pole(hi)]


def rule_takes_tile(int16, channels, sections, halo_frames):
    """mavg_sos_run's default rule inside the range sos_tile fits: everywhere but int16 mono with
    two sections and more than 2 KiB of fp64 halo, where the loop measured faster (include/mavg.h)."""
    return not (int16 and channels == 1 and sections == 2 and halo_frames * 8 > 2048)


# the section sets of the GPU tests (5-coefficient rows); every fused one fits stereo (1024 frames of halo)
HP_PK = [rbj("HP", 0.02, 0.7071), rbj("PK", 0.1, 4.0, 6.0)]
THREE = [rbj("LP", 0.05, 0.7071), rbj("BP", 0.1, 2.0), rbj("HP", 0.05, 0.7071)]
SEVEN = [rbj("LP", 0.25, 0.7071), rbj("HP", 0.25, 0.7071), rbj("PK", 0.1, 1.0, -4.0), rbj("LP", 0.2, 1.0),
         rbj("LP", 0.05, 0.7071), rbj("HP", 0.05, 0.7071), rbj("BP", 0.1, 2.0)]   # with one more: the sets at the limit
THIRD = (1.0 / 3.0, 0.0, 0.0, 0.0, 0.0)
TIMES3 = (3.0, 0.0, 0.0, 0.0, 0.0)
COPY = (1.0, 0.0, 0.0, 0.0, 0.0)
DC_BLOCK = (1.0, -1.0, 0.0, -0.98, 0.0)
