"""A Python model of the exponential moving average's decomposition (csrc/mavg_ema.hpp) with tiny
parameters, against the literal loop.  No GPU.

The model keeps the kernels' structure: wave width 64 with the real row structure of
wave_decay_scan (four row shifts with the uniform weights q, q^2, q^4, q^8, the two row broadcasts
with their per-lane weights), thread tid owning units u * WG + tid, the segment totals scanned with
base d^(64 F), the tile's carry-in entering segment s as d^(64 F s) Y, the halo reduction in
contiguous runs with its truncation, the chain's A / B / C with the carry kernel's chunks, and the
strip form.  The carry kernel's chunk is RUN records per lane of its whole workgroup, so the
smallest chunk the model can take is one record per lane of one wave: 64 records.

Bars: the paths that do not truncate are within 1e-12 M of the loop, the tile path within 2^-29 M
(before the fp32 rounding) -- include/mavg.h."""
import numpy as np
import pytest

from ema_ref import ema_bar, ema_loop, ema_ref, ema_scale

W = 64


def wave_decay_scan(v, q):
    """wave_decay_scan of mavg_device.hpp on a [64] array: every step reads all lanes' old values."""
    v = np.array(v, dtype=np.float64)
    lane = np.arange(W)
    for s in (1, 2, 4, 8):                                   # row_shr:s, zero fill at the row's start
        src = np.where((lane & 15) >= s, np.roll(v, s), 0.0)
        v = q ** s * src + v
    src = np.where((lane >> 4) & 1, v[np.maximum((lane & ~15) - 1, 0)], 0.0)   # row_bcast:15, rows 1 and 3
    v = q ** ((lane & 15) + 1.0) * src + v
    src = np.where(lane >= 32, v[31], 0.0)                   # row_bcast:31, rows 2 and 3
    v = q ** ((lane & 31) + 1.0) * src + v
    return v


def excl(inc):
    return np.concatenate([[0.0], inc[:-1]])                 # the lane shift


def test_the_wave_scan_is_the_decayed_inclusive_scan():
    rng = np.random.default_rng(1)
    v = rng.standard_normal(W)
    for q in (0.0, 0.3, 0.999, 1e-200, 1.0 - 2.0 ** -40):
        got = wave_decay_scan(v, q)
        acc, want = 0.0, []
        for l in range(W):
            acc = q * acc + v[l]
            want.append(acc)
        assert np.abs(got - np.array(want)).max() <= 1e-13 * np.abs(want).max(), q


def tile_body(xt, alpha, F, U, NW, Y):
    """One tile of TF = 64 NW F U frames (zeros past the end) from the carry-in Y -> its outputs."""
    d = 1.0 - alpha
    WG = W * NW
    q = d ** F
    units = xt.reshape(U * WG, F)
    agg = np.zeros(U * WG)
    for fr in range(F):                                      # lane step: Horner from zero
        agg = d * agg + alpha * units[:, fr]
    ex = np.zeros(U * WG)
    tot = np.zeros(U * NW)
    for s in range(U * NW):                                  # wave step (segment s = units 64 s ..)
        inc = wave_decay_scan(agg[s * W:(s + 1) * W], q)
        ex[s * W:(s + 1) * W] = excl(inc)
        tot[s] = inc[63]
    tv = np.zeros(W)
    tv[:U * NW] = tot
    Q = d ** (W * F)
    cs = Q ** np.arange(W, dtype=np.float64) * Y + excl(wave_decay_scan(tv, Q))   # segment step
    y = np.empty((U * WG, F))
    for s in range(U * NW):
        carry = q ** np.arange(W, dtype=np.float64) * cs[s] + ex[s * W:(s + 1) * W]
        for fr in range(F):                                  # output step: Horner from the carry
            carry = d * carry + alpha * units[s * W:(s + 1) * W, fr]
            y[s * W:(s + 1) * W, fr] = carry
    return y.reshape(-1)


def halo_frames(alpha):
    d = 1.0 - alpha
    H = 0
    while d > 0 and d ** H > 2.0 ** -30:
        H += 1
    return H


def halo_carry(x, t0, alpha, F, WG, H):
    """The tile kernel's carry-in from the ceil(H / F) units staged before t0 (zeros before frame
    0): WG runs of R frames, zeros padded at the old end, combined per wave and across waves."""
    d = 1.0 - alpha
    Ha = -(-H // F) * F
    if Ha == 0:
        return 0.0
    halo = np.zeros(Ha)
    lo = max(t0 - Ha, 0)
    halo[Ha - (t0 - lo):] = x[lo:t0]
    R = -(-Ha // WG)
    padded = np.concatenate([np.zeros(R * WG - Ha), halo]).reshape(WG, R)
    h = np.zeros(WG)
    for i in range(R):
        h = d * h + alpha * padded[:, i]
    y = 0.0
    for w in range(WG // W):
        y = d ** (W * R) * y + wave_decay_scan(h[w * W:(w + 1) * W], d ** R)[63]
    return y


def model_tile(x, alpha, F, U, NW, state=None):
    d = 1.0 - alpha
    TF = W * NW * F * U
    H = halo_frames(alpha)
    n = x.size
    out = np.empty(n)
    for t0 in range(0, n, TF):
        xt = np.zeros(TF)
        m = min(TF, n - t0)
        xt[:m] = x[t0:t0 + m]
        Y = halo_carry(x, t0, alpha, F, W * NW, H)
        if state is not None and t0 < H:
            Y += (d ** TF) ** (t0 // TF) * state
        out[t0:t0 + m] = tile_body(xt, alpha, F, U, NW, Y)[:m]
    return out


def carry_kernel(rec, D, run, nw, y0, d_last):
    """ema_carry_kernel: aggregates -> carry-ins in place, chunks of run * 64 nw records; returns
    (carry-ins, state_out)."""
    WG = W * nw
    rec = rec.copy()
    R = rec.size
    carry = y0
    state_out = None
    for r0 in range(0, R, run * WG):
        b = np.zeros(run * WG)
        m = min(run * WG, R - r0)
        b[:m] = rec[r0:r0 + m]
        b = b.reshape(WG, run)
        a = np.zeros(WG)
        for i in range(run):
            a = D * a + b[:, i]
        ex, tot = np.zeros(WG), np.zeros(nw)
        for w in range(nw):
            inc = wave_decay_scan(a[w * W:(w + 1) * W], D ** run)
            ex[w * W:(w + 1) * W] = excl(inc)
            tot[w] = inc[63]
        cw = np.empty(nw)
        c = carry
        for w in range(nw):
            cw[w] = c
            c = D ** (run * W) * c + tot[w]
        y = (D ** run) ** np.tile(np.arange(W, dtype=np.float64), nw) * np.repeat(cw, W) + ex
        for i in range(run):
            idx = r0 + np.arange(WG) * run + i
            ok = idx < R
            rec[idx[ok]] = y[ok]
            last = idx == R - 1
            if last.any():
                state_out = d_last * y[last][0] + b[last, i][0]
            y = D * y + b[:, i]
        carry = c
    return rec, state_out


def model_chain(x, alpha, F, U, NW, state=None, run=1, nw=1):
    d = 1.0 - alpha
    TF = W * NW * F * U
    n = x.size
    nt = -(-n // TF)
    xp = np.zeros(nt * TF)
    xp[:n] = x
    rec = np.empty(nt)
    for t in range(nt):                                      # A: y at the tile's last frame from zero
        last = min(TF, n - t * TF) - 1
        rec[t] = tile_body(xp[t * TF:(t + 1) * TF], alpha, F, U, NW, 0.0)[last]
    Y, sout = carry_kernel(rec, d ** TF, run, nw, 0.0 if state is None else state, d ** (n - (nt - 1) * TF))
    out = np.concatenate([tile_body(xp[t * TF:(t + 1) * TF], alpha, F, U, NW, Y[t]) for t in range(nt)])[:n]
    return out, sout


def model_strip(x, alpha, L, state=None, run=1, nw=1):
    d = 1.0 - alpha
    n = x.size
    ns = -(-n // L)
    rec = np.array([ema_loop(x[s * L:(s + 1) * L], alpha)[-1] for s in range(ns)])
    Y, sout = carry_kernel(rec, d ** L, run, nw, 0.0 if state is None else state, d ** (n - (ns - 1) * L))
    out = np.concatenate([ema_loop(x[s * L:(s + 1) * L], alpha, state=[Y[s]]) for s in range(ns)])
    return out, sout


def alpha_for_halo(H):
    """An alpha whose halo is H frames: d^H = 2^-30 sits on the boundary, so nudge d down."""
    if H == 0:
        return 1.0
    a = 1.0 - 2.0 ** (-30.0 / H) * (1.0 - 1e-12)
    assert halo_frames(a) == H, (H, halo_frames(a))
    return a


SHAPES = [(F, U, NW) for F in (1, 2, 4, 8) for U in (1, 2, 4) for NW in (1, 4)]


def alphas_of(F, U, NW):
    TF = W * NW * F * U
    hs = {h for h in (F - 1, F, F + 1, W * F, TF, TF + 1) if h >= 1}
    return [1.0, 0.9, 0.5] + [alpha_for_halo(h) for h in sorted(hs)]


def signals_of(TF, F):
    rng = np.random.default_rng(TF + F)
    n = 3 * TF + 17
    yield "uniform", rng.random(n)
    yield "short", rng.random(max(F - 1, 1))
    yield "constant", np.full(n, 0.75)
    imp = np.zeros(n)
    imp[0] = 1.0
    yield "impulse", imp


@pytest.mark.parametrize("F,U,NW", SHAPES)
def test_tile_model_within_the_truncation_bar(F, U, NW):
    TF = W * NW * F * U
    for alpha in alphas_of(F, U, NW):
        for name, x in signals_of(TF, F):
            for state in (None, -1.5):
                ref = ema_loop(x, alpha, state=None if state is None else [state])
                M = ema_scale(x, None if state is None else [state])
                got = model_tile(x, alpha, F, U, NW, state)
                assert np.abs(got - ref).max() <= 2.0 ** -29 * M, (alpha, name, state)
                if name == "impulse" and state is None:      # alpha d^f, up to rounding and the truncation
                    f = np.arange(x.size, dtype=np.float64)
                    assert np.abs(got - alpha * (1.0 - alpha) ** f).max() <= 2.0 ** -29
                if name == "constant" and state is None and alpha >= 0.5:
                    assert abs(got[-1] - 0.75) <= 1e-9       # y -> x


@pytest.mark.parametrize("F,U,NW", SHAPES)
def test_chain_model_is_exact_to_fp64_rounding(F, U, NW):
    TF = W * NW * F * U
    for alpha in alphas_of(F, U, NW):
        for name, x in signals_of(TF, F):
            for state in (None, -1.5):
                ref = ema_loop(x, alpha, state=None if state is None else [state])
                M = ema_scale(x, None if state is None else [state])
                got, sout = model_chain(x, alpha, F, U, NW, state)
                assert np.abs(got - ref).max() <= 1e-12 * M, (alpha, name, state)
                assert abs(sout - ref[-1]) <= 1e-12 * M, (alpha, name, state)


@pytest.mark.parametrize("run,nw", [(1, 1), (2, 1), (1, 2), (3, 2)])
def test_carry_kernel_model_crosses_its_chunks(run, nw):
    """Tiles of 64 frames; the record counts straddle one, two and three chunks of run * 64 nw.
    The bar is 1e-12 M plus the literal loop's OWN rounding: three fp64 roundings per frame, each
    at most 2^-53 M, that decay like the signal -- at most 3 * 2^-53 * M * min(n, 1 / alpha), which
    matters only at alpha = 1e-6 (the loop drifts; the model's powers of d come straight from d)."""
    chunk = run * W * nw
    rng = np.random.default_rng(chunk)
    for records in (chunk - 1, chunk, chunk + 1, 2 * chunk + 3, 3 * chunk):
        x = rng.random(records * W - 5)
        for alpha in (0.3, 1e-3, 1e-6):
            for state in (None, 2.5):
                ref = ema_loop(x, alpha, state=None if state is None else [state])
                M = ema_scale(x, None if state is None else [state])
                tol = 1e-12 * M + 3 * 2.0 ** -53 * M * min(x.size, 1.0 / alpha)
                got, sout = model_chain(x, alpha, 1, 1, 1, state, run=run, nw=nw)
                assert np.abs(got - ref).max() <= tol, (records, alpha, state)
                assert abs(sout - ref[-1]) <= tol
                got, sout = model_strip(x, alpha, W, state, run=run, nw=nw)
                assert np.abs(got - ref).max() <= tol, (records, alpha, state)
                assert abs(sout - ref[-1]) <= tol


def test_ema_ref_equals_the_literal_loop():
    rng = np.random.default_rng(7)
    for C in (1, 2, 3):
        x = rng.random((3 * 4096 + 17) * C)
        for alpha in (1.0, 0.3, 1e-3, 1e-6):
            for state in (None, rng.standard_normal(C) * 10):
                a, b = ema_ref(x, alpha, C, state), ema_loop(x, alpha, C, state)
                assert np.abs(a - b).max() <= 1e-13 * max(ema_scale(x, state), 1.0), (C, alpha)
    assert ema_ref(np.zeros(0), 0.5).size == 0
    assert (ema_bar(np.array([1.0, -2.0]), 4.0) == 2.0 ** -23 * np.array([1.0, 2.0]) + 2.0 ** -27).all()
