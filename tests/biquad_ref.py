"""The reference of the biquad's tests: the literal fp64 transposed-direct-form-II loop

    y = b0 x + s1;  s1' = b1 x - a1 y + s2;  s2' = b2 x - a2 y

per channel with state in and out, the impulse response's absolute sum G, the accuracy bar of
include/mavg.h, the smallest halo, and the RBJ cookbook filters.  numpy only; scipy.signal.lfilter
(the same recurrence in C) replaces the loop on long signals when it is importable."""
import math

import numpy as np

try:  # optional: the tests do not rely on it
    from scipy.signal import lfilter as _lfilter
except Exception:  # pragma: no cover - depends on the image
    _lfilter = None

COPY = (1.0, 0.0, 0.0, 0.0, 0.0)
FIR3 = (0.25, 0.5, 0.25, 0.0, 0.0)


def biquad_loop(x, coef, channels=1, state=None):
    """(y, state_out): fp64 y in x's interleaved layout and the [channels, 2] state after the last
    frame, by the literal loop over Python floats (fp64)."""
    b0, b1, b2, a1, a2 = (float(v) for v in coef)
    x = np.asarray(x, dtype=np.float64).reshape(-1, channels)
    y = np.empty_like(x)
    so = np.zeros((channels, 2))
    st = None if state is None else np.asarray(state, dtype=np.float64).reshape(channels, 2)
    for c in range(channels):
        s1, s2 = (0.0, 0.0) if st is None else (float(st[c, 0]), float(st[c, 1]))
        col = []
        for v in x[:, c].tolist():
            o = b0 * v + s1
            s1 = b1 * v - a1 * o + s2
            s2 = b2 * v - a2 * o
            col.append(o)
        y[:, c] = col
        so[c] = (s1, s2)
    return y.reshape(-1), so


def biquad_ref(x, coef, channels=1, state=None, fast=False):
    """biquad_loop; with fast=True and scipy present, scipy.signal.lfilter per channel."""
    if not fast or _lfilter is None:
        return biquad_loop(x, coef, channels, state)
    b0, b1, b2, a1, a2 = (float(v) for v in coef)
    x = np.asarray(x, dtype=np.float64).reshape(-1, channels)
    st = np.zeros((channels, 2)) if state is None else np.asarray(state, dtype=np.float64).reshape(channels, 2)
    y = np.empty_like(x)
    so = np.zeros((channels, 2))
    for c in range(channels):
        y[:, c], so[c] = _lfilter([b0, b1, b2], [1.0, a1, a2], x[:, c], zi=st[c])
    return y.reshape(-1), so


def impulse_loop(coef, n):
    """h[0 .. n) by the loop."""
    x = np.zeros(n)
    if n:
        x[0] = 1.0
    return biquad_loop(x, coef)[0]


def pole_radius(coef):
    a1, a2 = float(coef[3]), float(coef[4])
    disc = a1 * a1 - 4.0 * a2
    return math.sqrt(a2) if disc < 0 else 0.5 * (abs(a1) + math.sqrt(disc))


_impulse = {}


def impulse_abs(coef):
    """|h[n]| for n = 0 .. N, N far past where the response is negligible (2^-110 of its start), in
    closed form: h[n] = c1 u_n + c2 u_(n-1), u_m = sum_j p1^j p2^(m-1-j) over the poles."""
    key = tuple(float(v) for v in coef)
    if key in _impulse:
        return _impulse[key]
    b0, b1, b2, a1, a2 = key
    c1, c2 = b1 - a1 * b0, b2 - a2 * b0
    rho = pole_radius(key)
    if rho == 0.0:
        h = np.abs(np.array([b0, c1, c2]))
    else:
        N = int(80.0 / -math.log(rho)) + 64 if rho < 1.0 else 0
        assert 0 < N <= 1 << 24, (key, N)
        n = np.arange(0, N + 1, dtype=np.float64)   # u_n for n = 0 .. N
        disc = a1 * a1 - 4.0 * a2
        if disc < 0:
            th = math.atan2(0.5 * math.sqrt(-disc), -0.5 * a1)
            u = np.exp((n - 1.0) * math.log(rho)) * np.sin(n * th) / math.sin(th)
        elif disc == 0:
            p = -0.5 * a1
            u = n * np.sign(p) ** (n - 1.0) * np.exp((n - 1.0) * math.log(abs(p)))
        else:
            p1, p2 = 0.5 * (-a1 + math.sqrt(disc)), 0.5 * (-a1 - math.sqrt(disc))
            pw = lambda p: np.zeros_like(n) if p == 0 else np.sign(p) ** n * np.exp(n * math.log(abs(p)))
            u = (pw(p1) - pw(p2)) / (p1 - p2)
        u[0] = 0.0
        h = np.empty(N + 1)
        h[0] = b0
        h[1:] = c1 * u[1:] + c2 * u[:-1]
        h = np.abs(h)
    h.setflags(write=False)
    _impulse[key] = h
    return h


def biquad_gain(coef):
    """G = sum |h[n]|, summed from the small end, until the tail is negligible."""
    return float(np.sum(impulse_abs(coef)[::-1]))


def tail_after(coef, H):
    """sum_{n > H} |h[n]|"""
    h = impulse_abs(coef)
    return float(np.sum(h[:H:-1])) if H + 1 < h.size else 0.0


def min_halo(coef):
    """The smallest H with sum_{n > H} |h[n]| <= 2^-30 G."""
    h = impulse_abs(coef)
    suffix = np.cumsum(h[::-1])[::-1]            # suffix[n] = sum_{m >= n} |h[m]|
    ok = np.nonzero(suffix <= 2.0 ** -30 * suffix[0])[0]
    return int(ok[0]) - 1 if ok.size else h.size - 1


def state_horizon(coef):
    """The frames an arbitrary state_in stays visible: the smallest N such that for every n >= N the
    first row of A^n, (u_(n+1), u_n), sums in magnitude to at most 2^-30 G -- past it a state of
    magnitude M moves an output by at most 2^-30 G M.  (|u_n| is |h[n]| of b = (0, 1, 0).)"""
    u = impulse_abs((0.0, 1.0, 0.0, float(coef[3]), float(coef[4])))
    s = u[1:] + u[:-1]
    over = np.nonzero(s > 2.0 ** -30 * biquad_gain(coef))[0]
    return int(over[-1]) + 2 if over.size else 0


def biquad_scale(x, state=None):
    """M: the largest of |x| over the signal and |state_in|."""
    m = float(np.abs(np.asarray(x, dtype=np.float64)).max()) if np.size(x) else 0.0
    if state is not None and np.size(state):
        m = max(m, float(np.abs(np.asarray(state, dtype=np.float64)).max()))
    return m


def biquad_bar(ref, G, M):
    """|y - y_ref| <= 2^-23 |y_ref| + 2^-29 G M, element-wise."""
    return 2.0 ** -23 * np.abs(ref) + 2.0 ** -29 * G * M


def domain_d(coef):
    """D = min(1 + a1 + a2, 1 - a1 + a2): the bar is promised for D >= 2^-22."""
    return min(1.0 + coef[3] + coef[4], 1.0 - coef[3] + coef[4])


def rbj(kind, f, Q, dB=6.0):
    """(b0, b1, b2, a1, a2) of the RBJ cookbook's LP / HP / BP (constant peak gain) / PK, normalised."""
    w = 2.0 * math.pi * f
    cw, al = math.cos(w), math.sin(w) / (2.0 * Q)
    a = [1.0 + al, -2.0 * cw, 1.0 - al]
    if kind == "LP":
        b = [(1.0 - cw) / 2.0, 1.0 - cw, (1.0 - cw) / 2.0]
    elif kind == "HP":
        b = [(1.0 + cw) / 2.0, -(1.0 + cw), (1.0 + cw) / 2.0]
    elif kind == "BP":
        b = [al, 0.0, -al]
    elif kind == "PK":
        A = 10.0 ** (dB / 40.0)
        b = [1.0 + al * A, -2.0 * cw, 1.0 - al * A]
        a = [1.0 + al / A, -2.0 * cw, 1.0 - al / A]
    else:
        raise ValueError(kind)
    return (b[0] / a[0], b[1] / a[0], b[2] / a[0], a[1] / a[0], a[2] / a[0])


def from_poles(p1, p2, b=(1.0, 0.0, 0.0)):
    """Real poles p1, p2: a1 = -(p1 + p2), a2 = p1 p2."""
    return (b[0], b[1], b[2], -(p1 + p2), p1 * p2)


REAL_POLE_CASES = [from_poles(0.9, 0.5, (1.0, 0.5, 0.25)), from_poles(0.9, 0.9, (1.0, 0.5, 0.25)),
                   from_poles(-0.9, -0.5, (1.0, 0.5, 0.25))]
FILTER_LIST = [(k, f, Q) for k in ("LP", "HP", "BP", "PK") for f in (0.25, 0.05, 0.01, 0.002, 0.0005)
               for Q in (0.5001, 0.7071, 4.0, 30.0)]      # the 80 filters of the halo bound's cap


def f_at_domain_edge(Q, kind="LP"):
    """The f at which an RBJ filter has D = 2^-22: D = 2 (1 - cos w) / (1 + alpha) for LP and HP."""
    lo, hi = 1e-6, 1e-3
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if domain_d(rbj(kind, mid, Q)) < 2.0 ** -22:
            lo = mid
        else:
            hi = mid
    return hi
