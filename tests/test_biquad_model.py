"""A numpy restatement of the biquad's decomposition (csrc/mavg_biquad.hpp) against the literal loop
of tests/biquad_ref.py and the accuracy bar of include/mavg.h.  No GPU, no library.

What is restated, with the kernels' structure and small parameters:
  * the powers of A = [[-a1, 1], [-a2, 0]] as the library forms them: binary powers and the products
    Q^1 .. Q^63 of a level's base in long double, rounded once; a lane's weight is one table entry
    (one fp64 product of two entries, Q^16 Q^j, measured 1e-8 G M at the domain's edge: not used);
  * the wave scan's real row structure: row shifts by 1, 2, 4, 8 inside 16-lane rows, then the
    broadcasts of lane 15 into rows 1 and 3 and of lane 31 into rows 2 and 3;
  * the tile: units of F frames, segments of 64 units, the segment totals scanned across one row;
  * the halo reduction (runs of R frames per thread, a wave scan, wave totals) and its truncation;
  * the chain: aggregates, the carry kernel's chunks of RUN records per lane, the tiles again;
  * the strip form: one serial run per strip at both ends of the same carry kernel.

With D = 2^-22 (the edge of the promised domain) the bar must hold for LP, HP and peaking filters
at Q 0.5001, 0.7071 and 4, on 3 tiles (the library's 2048-frame tile) and on 40 tiles."""
import numpy as np
import pytest

from biquad_ref import (biquad_bar, biquad_gain, biquad_loop, biquad_scale, domain_d, f_at_domain_edge, impulse_abs,
                        impulse_loop, min_halo, rbj, state_horizon, tail_after)

LD = np.longdouble


# ---- the powers, as csrc/mavg_biquad.hip forms them ----
def matl_pow(coef, m):
    r = np.array([[1, 0], [0, 1]], dtype=LD)
    s = np.array([[-LD(coef[3]), 1], [-LD(coef[4]), 0]], dtype=LD)
    while m:
        if m & 1:
            r = r @ s
        if m > 1:
            s = s @ s
        m >>= 1
    return r


def mat_pow(coef, m):
    return matl_pow(coef, m).astype(np.float64)


def fill_level(coef, m, N):
    """Q^1 .. Q^N of the base Q = A^m by successive long double products, each rounded once; and
    Q^N unrounded."""
    q = matl_pow(coef, m)
    p, t = q, []
    for j in range(N):
        t.append(p.astype(np.float64))
        if j < N - 1:
            p = p @ q
    return np.array(t), p


class Level:
    """One scan level: the uniform powers and the per-lane weights of the 64 lanes, every one a
    table entry (never a product of entries)."""

    def __init__(self, coef, m, N=63):
        t, self.top = fill_level(coef, m, N)
        self.q = {1: t[0], 2: t[1], 4: t[3], 8: t[7]}
        lane = np.arange(64)
        self.w15 = t[lane & 15]                                            # Q^((lane & 15) + 1)
        self.w31 = t[lane & 31] if N >= 32 else self.w15                   # Q^((lane & 31) + 1)
        eye = np.eye(2)
        e = np.minimum(lane, N)
        self.lane_pow = np.where((e == 0)[:, None, None], eye, t[np.maximum(e, 1) - 1])   # Q^lane (N < 63: lanes 0 .. N)

    def scan(self, v, steps=6):
        """wave_mat_scan on v[..., 64, 2]: the inclusive matrix-weighted scan across the lanes
        (steps=5: MatLane::scan_halves, lanes 31 and 63 end with the scans of their halves)."""
        lane = np.arange(64)
        v = v.copy()
        for k in (1, 2, 4, 8):
            src = np.zeros_like(v)
            ok = (lane & 15) >= k
            src[..., ok, :] = v[..., lane[ok] - k, :]
            v = v + np.einsum("ij,...j->...i", self.q[k], src)
        for w, at, rows in ((self.w15, 15, (1, 3)), (self.w31, 31, (2, 3)))[:steps - 4]:
            src = np.zeros_like(v)
            for r in rows:
                sel = (lane >> 4) == r
                frm = 16 * r - 1 if at == 15 else 31
                src[..., sel, :] = v[..., frm:frm + 1, :]
            v = v + np.einsum("lij,...lj->...li", w, src)
        return v


def excl(v):
    e = np.zeros_like(v)
    e[..., 1:, :] = v[..., :-1, :]
    return e


def run_frames(coef, x, s):
    """The recurrence over x[..., n] from states s[..., 2] (vectorised over the leading axes):
    (y[..., n], the states after)."""
    b0, b1, b2, a1, a2 = coef
    s1, s2 = s[..., 0].copy(), s[..., 1].copy()
    y = np.empty_like(x)
    for i in range(x.shape[-1]):
        v = x[..., i]
        o = b0 * v + s1
        s1, s2 = b1 * v - a1 * o + s2, b2 * v - a2 * o
        y[..., i] = o
    return y, np.stack([s1, s2], axis=-1)


class Tile:
    """biquad_tile_body for tiles of NSEG segments of 64 units of F frames (thread order ignored:
    the arithmetic does not depend on it)."""

    def __init__(self, coef, F, NSEG):
        assert NSEG <= 16
        self.coef, self.F, self.NSEG, self.TF = coef, F, NSEG, 64 * F * NSEG
        self.unit, self.seg = Level(coef, F), Level(coef, 64 * F, 16)

    def body(self, x, Y):
        """x[TF] (zero padded), carry-in Y[2] -> (y[TF], the state after every frame [TF, 2])."""
        F, NSEG = self.F, self.NSEG
        xu = x.reshape(NSEG, 64, F)
        _, agg = run_frames(self.coef, xu, np.zeros((NSEG, 64, 2)))          # lane step
        inc = self.unit.scan(agg)                                            # wave step
        cy = excl(inc)
        tot = np.zeros((64, 2))
        tot[:NSEG] = inc[:, 63, :]
        sc = self.seg.scan(tot)                                              # segment step (row 0 only)
        cs = np.einsum("lij,j->li", self.seg.lane_pow, Y) + excl(sc)
        cy = np.einsum("lij,sj->sli", self.unit.lane_pow, cs[:NSEG]) + cy
        y, after = run_frames(self.coef, xu, cy)                             # output step
        # the state after every frame, for the record and state_out
        states = np.empty((NSEG, 64, F, 2))
        s = cy
        for i in range(F):
            _, s = run_frames(self.coef, xu[..., i:i + 1], s)
            states[:, :, i, :] = s
        return y.reshape(-1), states.reshape(-1, 2)


def halo_carry(coef, halo, WG=256):
    """The tile kernel's halo reduction: `halo` staged frames (oldest first) -> the carry state."""
    Ha = halo.size
    if Ha == 0:
        return np.zeros(2)
    R = -(-Ha // WG)
    padded = np.concatenate([np.zeros(R * WG - Ha), halo]).reshape(WG // 64, 64, R)
    _, h = run_frames(coef, padded, np.zeros((WG // 64, 64, 2)))
    run = Level(coef, R, 16)
    q32 = run.top @ run.top
    hv = run.scan(h, steps=5)
    tot = np.einsum("ij,wj->wi", q32.astype(np.float64), hv[:, 31, :]) + hv[:, 63, :]
    wave = (q32 @ q32).astype(np.float64)
    y = np.zeros(2)
    for t in tot:
        y = wave @ y + t
    return y


def carry_kernel(coef, rec, state, span, last_frames, RUN, NW):
    """biquad_carry_kernel: aggregates rec[records, 2] -> (carry-ins, state_out)."""
    records = rec.shape[0]
    D, lanes = mat_pow(coef, span), Level(coef, span * RUN)
    wave, d_last = mat_pow(coef, span * RUN * 64), mat_pow(coef, last_frames)
    out = np.empty_like(rec)
    carry = np.zeros(2) if state is None else np.asarray(state, dtype=np.float64)
    chunk = RUN * 64 * NW
    for r0 in range(0, records, chunk):
        b = np.zeros((chunk, 2))
        m = min(chunk, records - r0)
        b[:m] = rec[r0:r0 + m]
        b = b.reshape(NW, 64, RUN, 2)
        a = np.zeros((NW, 64, 2))
        for i in range(RUN):
            a = np.einsum("ij,wlj->wli", D, a) + b[:, :, i]
        inc = lanes.scan(a)
        ex, tot = excl(inc), inc[:, 63, :]
        y = np.empty((NW, 64, 2))
        cw = carry
        for w in range(NW):
            y[w] = np.einsum("lij,j->li", lanes.lane_pow, cw) + ex[w]
            cw = wave @ cw + tot[w]
        ys = np.empty((NW, 64, RUN, 2))
        for i in range(RUN):
            ys[:, :, i] = y
            y = np.einsum("ij,wlj->wli", D, y) + b[:, :, i]
        out[r0:r0 + m] = ys.reshape(chunk, 2)[:m]
        carry = cw
    state_out = d_last @ out[-1] + rec[-1]
    return out, state_out


def chain(coef, x, state, F, NSEG, RUN=8, NW=4):
    t = Tile(coef, F, NSEG)
    n = x.size
    nt = -(-n // t.TF)
    xp = np.concatenate([x, np.zeros(nt * t.TF - n)]).reshape(nt, t.TF)
    last = n - (nt - 1) * t.TF
    rec = np.array([t.body(xp[i], np.zeros(2))[1][(t.TF if i < nt - 1 else last) - 1] for i in range(nt)])
    Y, so = carry_kernel(coef, rec, state, t.TF, last, RUN, NW)
    y = np.concatenate([t.body(xp[i], Y[i])[0] for i in range(nt)])[:n]
    return y, so


def strip(coef, x, state, L, RUN=8, NW=4):
    n = x.size
    ns = -(-n // L)
    xp = np.concatenate([x, np.zeros(ns * L - n)]).reshape(ns, L)
    last = n - (ns - 1) * L
    _, rec = run_frames(coef, xp[:-1], np.zeros((ns - 1, 2)))
    _, rl = run_frames(coef, xp[-1:, :last], np.zeros((1, 2)))
    rec = np.concatenate([rec, rl])
    Y, so = carry_kernel(coef, rec, state, L, last, RUN, NW)
    y, _ = run_frames(coef, xp, Y)
    return y.reshape(-1)[:n], so


def tile_path(coef, x, state, F, NSEG, H, state_frames):
    t = Tile(coef, F, NSEG)
    n = x.size
    nt = -(-n // t.TF)
    Ha = -(-H // F) * F
    xp = np.concatenate([np.zeros(Ha), x, np.zeros(nt * t.TF - n)])
    ys, so = [], None
    for i in range(nt):
        t0 = i * t.TF
        Y = halo_carry(coef, xp[t0:t0 + Ha])
        if state is not None and t0 < state_frames:
            Y = mat_pow(coef, t0) @ np.asarray(state, dtype=np.float64) + Y
        y, st = t.body(xp[Ha + t0:Ha + t0 + t.TF], Y)
        ys.append(y)
        if i == nt - 1:
            so = st[n - 1 - t0]
    return np.concatenate(ys)[:n], so


def warm_state(coef, scale=1.0, seed=9, n=4000):
    """A state the filter produces: what the loop reaches after n frames of noise of amplitude
    `scale` (a state that no input produces decays with the poles alone and is up to 1 / theta
    larger in its response than M: the bar is not stated for it)."""
    return biquad_loop(scale * signal(n, seed), coef)[1][0]


def signal(n, seed=1):
    return np.random.default_rng(seed).random(n)      # uniform [0, 1): the DC keeps the states large


def check(coef, y, so, x, state, tag):
    ref, rs = biquad_loop(x, coef, 1, state)
    G, M = biquad_gain(coef), biquad_scale(x, state)
    err = np.abs(y - ref)
    # the bar less the fp32 rounding, 2^-24 |y_ref|, which is not modelled
    bar = biquad_bar(ref, G, M) - 2.0 ** -24 * np.abs(ref)
    worst = int(np.argmax(err - bar))
    assert (err <= bar).all(), (tag, worst, float(err[worst]), float(bar[worst]), float(err.max() / (G * M)))
    assert np.abs(so - rs[0]).max() <= 2.0 ** -29 * G * M, (tag, so, rs)
    return float(err.max() / (G * M))


def test_the_closed_form_impulse_response_is_the_loop():
    for coef in (rbj("LP", 0.05, 0.7071), rbj("PK", 0.25, 30.0), rbj("HP", 0.01, 0.5001), (1.0, 0.5, 0.25, -1.8, 0.81),
                 (1.0, 0.5, 0.25, -1.4, 0.45), (1.0, 0.5, 0.25, 1.4, 0.45), (0.25, 0.5, 0.25, 0.0, 0.0)):
        h = impulse_abs(coef)
        n = min(h.size, 3000)
        ref = np.abs(impulse_loop(coef, n))
        assert np.abs(h[:n] - ref).max() <= 1e-12 * ref.max(), coef
        assert tail_after(coef, min_halo(coef)) <= 2.0 ** -30 * biquad_gain(coef)
        if min_halo(coef) > 0:
            assert tail_after(coef, min_halo(coef) - 1) > 2.0 ** -30 * biquad_gain(coef)


def test_the_wave_scan_is_the_serial_composition():
    coef = rbj("LP", 0.01, 0.7071)
    lv = Level(coef, 3)
    v = np.random.default_rng(0).standard_normal((64, 2))
    Q = mat_pow(coef, 3)
    want, acc = np.empty_like(v), np.zeros(2)
    for l in range(64):
        acc = Q @ acc + v[l]
        want[l] = acc
    assert np.abs(lv.scan(v) - want).max() <= 1e-12 * np.abs(want).max()
    for l in (0, 1, 15, 16, 17, 31, 32, 47, 48, 63):
        assert np.abs(lv.lane_pow[l] - mat_pow(coef, 3 * l)).max() <= 1e-13 * max(1.0, np.abs(mat_pow(coef, 3 * l)).max())


EDGE = [(k, Q) for k in ("LP", "HP", "PK") for Q in (0.5001, 0.7071, 4.0)]


@pytest.mark.parametrize("kind,Q", EDGE)
def test_chain_holds_the_bar_at_the_domain_edge(kind, Q):
    """D = 2^-22: 3 of the library's 2048-frame tiles plus 17 frames, and 40 tiles of 512."""
    coef = rbj(kind, f_at_domain_edge(Q, kind), Q)
    assert 2.0 ** -22 <= domain_d(coef) < 2.0 ** -22 * 1.001
    x = signal(3 * 2048 + 17)
    y, so = chain(coef, x, None, F=4, NSEG=8)
    e3 = check(coef, y, so, x, None, (kind, Q, 3))
    x = signal(40 * 512 + 17, seed=2)
    st = warm_state(coef)
    y, so = chain(coef, x, st, F=2, NSEG=4, RUN=2, NW=1)
    e40 = check(coef, y, so, x, st, (kind, Q, 40))
    print(f"{kind} Q={Q}: scan error / (G M) = {e3:.2e} (3 tiles), {e40:.2e} (40 tiles); bar {2.0 ** -29:.2e}")


def test_chain_crosses_a_carry_chunk_and_strip_form():
    for coef in (rbj("LP", 5e-4, 0.7071), rbj("HP", 1e-4, 0.7071)):
        x = signal(150 * 64 + 5, seed=3)
        st = warm_state(coef, 3.0)
        y, so = chain(coef, x, st, F=1, NSEG=1, RUN=2, NW=1)        # 151 records, chunks of 128
        check(coef, y, so, x, st, "chunk")
        y, so = strip(coef, x, st, L=7, RUN=2, NW=2)                 # 1372 strips, chunks of 256
        check(coef, y, so, x, st, "strip")
        y, so = strip(coef, x[:5], None, L=7)                         # less than one strip
        check(coef, y, so, x[:5], None, "strip1")


@pytest.mark.parametrize("coef", [rbj("LP", 0.05, 0.7071), rbj("HP", 0.01, 0.7071), rbj("BP", 0.05, 4.0),
                                  rbj("PK", 0.25, 30.0), (0.25, 0.5, 0.25, 0.0, 0.0), (1.0, 0.5, 0.25, -1.8, 0.81)])
def test_tile_path_with_the_halo_truncation(coef):
    """The halo is the smallest one (the library's is at least that): the truncation at its largest."""
    H = min_halo(coef)
    x = signal(3 * 512 + 17, seed=4)
    y, so = tile_path(coef, x, None, F=2, NSEG=4, H=H, state_frames=0)
    check(coef, y, so, x, None, ("tile", H))
    # a state the filter produced: streamed from a first chunk; it enters the tiles within H frames
    cut = 700
    _, mid = biquad_loop(x[:cut], coef)
    y2, so2 = tile_path(coef, x[cut:], mid[0], F=2, NSEG=4, H=H, state_frames=max(H, 1))
    ref, rs = biquad_loop(x, coef)
    G = biquad_gain(coef)
    assert np.abs(y2 - ref[cut:]).max() <= 2.0 ** -29 * G and np.abs(so2 - rs[0]).max() <= 2.0 ** -29 * G


def test_tile_path_with_a_state_no_input_produces():
    """A state_in of (100, 100) on a signal in [0, 1): it answers with the poles alone and outlives
    the halo.  The second tile starts between the halo and the state's horizon: with the state
    applied up to its horizon the outputs hold the bar, with the state dropped at the halo they do
    not (so the horizon is what this tests).  d_state_out is not promised for such a state."""
    coef = rbj("LP", 0.01, 0.7071)
    H, Hs = min_halo(coef), state_horizon(coef)
    assert H < 512 < Hs                                   # tile 1 starts at frame 512
    x = signal(5 * 512 + 17, seed=4)
    st = np.array([100.0, 100.0])
    ref, _ = biquad_loop(x, coef, 1, st)
    bar = biquad_bar(ref, biquad_gain(coef), 100.0) - 2.0 ** -24 * np.abs(ref)
    y, _ = tile_path(coef, x, st, F=2, NSEG=4, H=H, state_frames=Hs)
    assert (np.abs(y - ref) <= bar).all()
    y, _ = tile_path(coef, x, st, F=2, NSEG=4, H=H, state_frames=H)
    assert not (np.abs(y - ref) <= bar).all()
    # the chain applies every state: the same state at the domain's edge, outputs only
    edge = rbj("PK", f_at_domain_edge(4.0, "PK"), 4.0)
    x = signal(3 * 2048 + 17)
    ref, _ = biquad_loop(x, edge, 1, st)
    y, _ = chain(edge, x, st, F=4, NSEG=8)
    assert (np.abs(y - ref) <= biquad_bar(ref, biquad_gain(edge), 100.0) - 2.0 ** -24 * np.abs(ref)).all()
