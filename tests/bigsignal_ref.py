"""Full-coverage moving-average reference in plain torch (no project code).

``chunked_mismatches`` compares EVERY output of a signal of any length, on
whatever device the tensors live on, against the exact window sums: the
signal is walked in chunks of ``chunk_frames`` frames, each read with the
k-1 frames before it, so a signal past 2^32 samples is checked with a few GiB
of temporaries and without a host copy.  All indices are Python ints or int64.

    int16: y == trunc(S / k)                       (C++ truncating division)
    fp32:  bits(y) == bits(fl32(fl64(S) / k))      int16-VALUED inputs only
           (generator dist 0): |S| < 2^53, so fl64(S) is S and the quotient
           is the correctly rounded one the library promises for such data

A chunk is viewed as (frames, C) and summed along frames one column (channel)
at a time: a 1-D cumsum is the scan torch runs at memory speed, a 2-D one is
not.  tests/test_bigsignal_ref.py pins this to the C oracle bit for bit.

Siblings for the launchers built on the moving average, by the same walk:
  chunked_decim_mismatches    the kept frames phase + m * hop only, against the packed output
  chunked_cascade_mismatches  `passes` passes inside a chunk read with passes * (k-1) frames of lead
  chunked_stat_mismatches     S1 and S2 of int16(-valued) input, the bars of tests/stat_ref.py

And for the filters that are not built on it (second half of this file):
  chunked_extrema_mismatches  the moving maximum and minimum by log-step doubling, bit patterns
  chunked_fir_mismatches      exact fp64 sums of dyadic taps times int16-valued input, bit patterns
  chunked_ema_mismatches      fp64 decayed doubling over a chunk read with W frames of lead, d^W <= 2^-60,
  chunked_biquad_mismatches   the same on the state 2-vector, rho^W <= 2^-70; both against the bars
                              of include/mavg.h, and both report the largest err / bar seen
  chunked_sos_mismatches      the biquad's column section by section, fp64 between the sections, the
                              leads added up; the bar's absolute term comes from the caller"""
import math

import numpy as np
import torch


def chunked_mismatches(x, y, k, C, chunk_frames, first_frame=0):
    """(count, first_bad_sample_index_or_None) over frames >= first_frame of
    the interleaved signal ``x`` (frames x C, zero history before frame 0) and
    its claimed moving average ``y`` (same indexing as ``x``)."""
    if x.dtype != y.dtype or x.numel() != y.numel() or x.dim() != 1 or y.dim() != 1:
        raise ValueError("x and y must be 1-D tensors of one dtype and size")
    if x.dtype not in (torch.int16, torch.float32):
        raise TypeError(f"int16 or float32, got {x.dtype}")
    if k < 1 or C < 1 or chunk_frames < 1 or x.numel() % C != 0:
        raise ValueError("bad k, C, chunk_frames or a partial frame")
    F = x.numel() // C
    count, first = 0, None
    f0 = first_frame
    while f0 < F:
        f1 = min(F, f0 + chunk_frames)
        h0 = max(0, f0 - (k - 1))        # the (k-1)-frame overlap, cut at frame 0
        nf, lead = f1 - f0, f0 - h0
        j0 = lead + 1 - k                 # prefix index of the subtrahend for frame f0
        m = min(max(-j0, 0), nf)          # frames of this chunk still in the warm-up
        xv = x[h0 * C:f1 * C].view(-1, C)
        yv = y[f0 * C:f1 * C].view(-1, C)
        bad = torch.empty((nf, C), dtype=torch.bool, device=x.device)
        for c in range(C):
            # P[i] = sum of frames [h0, h0 + i) of channel c, exactly
            P = torch.zeros(1 + f1 - h0, dtype=torch.int64, device=x.device)
            P[1:].copy_(xv[:, c])
            if x.dtype == torch.float32 and not bool((P[1:] == xv[:, c]).all()):
                raise ValueError("fp32 reference: inputs must be integer-valued")
            P = P.cumsum(0)
            # S[f] = P[f + 1] - P[f + 1 - k], the second term only where f + 1 - k >= h0
            # (else the window starts at h0: either frame 0, or exactly k - 1 frames back)
            S = P[lead + 1:lead + 1 + nf].clone()
            if m < nf:
                S[m:] -= P[j0 + m:j0 + nf]
            del P
            if x.dtype == torch.int16:
                bad[:, c] = torch.div(S, k, rounding_mode="trunc").to(torch.int16) != yv[:, c]
            else:
                ref = (S.to(torch.float64) / k).to(torch.float32)
                bad[:, c] = ref.view(torch.int32) != yv[:, c].view(torch.int32)
                del ref
            del S
        n_bad = int(bad.sum())
        if n_bad:
            if first is None:
                first = f0 * C + int(bad.view(-1).nonzero()[0, 0])
            count += n_bad
        del bad
        f0 = f1
    return count, first


def _check_signal(x, k, C, chunk_frames, first_frame):
    if x.dim() != 1 or x.dtype not in (torch.int16, torch.float32):
        raise TypeError("x must be a 1-D int16 or float32 tensor")
    if k < 1 or C < 1 or chunk_frames < 1 or first_frame < 0 or x.numel() % C != 0:
        raise ValueError("bad k, C, chunk_frames, first_frame or a partial frame")
    return x.numel() // C


def _column_i64(col):
    """A channel of a chunk as int64 with a leading 0 (the prefix sums' P[0]); fp32 must hold integers."""
    P = torch.zeros(1 + col.numel(), dtype=torch.int64, device=col.device)
    P[1:].copy_(col)
    if col.dtype == torch.float32 and not bool((P[1:] == col).all()):
        raise ValueError("fp32 reference: inputs must be integer-valued")
    return P


def _window_sums(P, k, lead, i0, step, cnt):
    """From the prefix sums P of a chunk's frames [h0, f1) (P[i] = sum of the first i of them) the
    window sums of the frames lead + i0 + step * t, t in [0, cnt): k frames each, cut at the
    chunk's first frame (frame 0 of the signal, or at least k - 1 frames back)."""
    a = lead + 1 + i0                      # prefix index of the minuend of the first frame
    S = P[a:a + step * (cnt - 1) + 1:step].clone()
    t_w = min(cnt, max(0, -(-(k - a) // step)))    # frames whose window starts before the chunk
    if t_w < cnt:
        b = a - k + step * t_w
        S[t_w:] -= P[b:b + step * (cnt - t_w - 1) + 1:step]
    return S


def _count(bad, base, count, first):
    n_bad = int(bad.sum())
    if n_bad and first is None:
        first = base + int(bad.view(-1).nonzero()[0, 0])
    return count + n_bad, first


def chunked_decim_mismatches(x, y_dec, k, C, hop, phase, chunk_frames, first_frame=0):
    """(count, first bad sample of y_dec or None).  The signal proper starts at frame first_frame
    of ``x`` (what precedes it is its history); of its full-rate moving average y_dec claims the
    frames phase + m * hop, packed: M * C samples, M = len(range(phase, frames, hop))."""
    F = _check_signal(x, k, C, chunk_frames, first_frame)
    if hop < 1 or not 0 <= phase < hop:
        raise ValueError("bad hop or phase")
    if y_dec.dtype != x.dtype or y_dec.dim() != 1:
        raise ValueError("x and y_dec must be 1-D tensors of one dtype")
    M = len(range(phase, F - first_frame, hop))
    if y_dec.numel() != M * C:
        raise ValueError(f"y_dec must hold {M} * {C} samples")
    count, first = 0, None
    f0 = first_frame
    while f0 < F:
        f1 = min(F, f0 + chunk_frames)
        m_lo = max(0, -(-(f0 - first_frame - phase) // hop))     # first kept frame at or after f0
        g0 = first_frame + phase + m_lo * hop
        if g0 < f1:
            cnt = (f1 - 1 - g0) // hop + 1
            h0 = max(0, f0 - (k - 1))
            xv = x[h0 * C:f1 * C].view(-1, C)
            yv = y_dec[m_lo * C:(m_lo + cnt) * C].view(-1, C)
            bad = torch.empty((cnt, C), dtype=torch.bool, device=x.device)
            for c in range(C):
                P = _column_i64(xv[:, c]).cumsum(0)
                S = _window_sums(P, k, f0 - h0, g0 - f0, hop, cnt)
                del P
                if x.dtype == torch.int16:
                    bad[:, c] = torch.div(S, k, rounding_mode="trunc").to(torch.int16) != yv[:, c]
                else:
                    ref = (S.to(torch.float64) / k).to(torch.float32)
                    bad[:, c] = ref.view(torch.int32) != yv[:, c].view(torch.int32)
                del S
            count, first = _count(bad, m_lo * C, count, first)
            del bad
        f0 = f1
    return count, first


def chunked_cascade_mismatches(x, y, k, C, passes, chunk_frames, first_frame=0):
    """(count, first bad sample or None) of ``passes`` successive moving averages, each with zero
    history, the intermediate kept in x's dtype.  A chunk is read with passes * (k-1) frames of
    lead, cut at frame 0, and every pass runs inside it: pass j spoils the first j * (k-1) frames
    of a chunk that does not start at frame 0, all inside the lead.  int16: trunc(S / k) as int16
    per pass.  fp32: k = 2^s and int16-valued input only -- pass j's values are multiples of
    2^(-s j) below 2^15 in magnitude, kept as the int64 v * 2^(s j); their window sums stay below
    2^(15 + s passes) <= 2^45, so fl32(fl64(S) / k) is the correctly rounded value."""
    F = _check_signal(x, k, C, chunk_frames, first_frame)
    if passes < 1:
        raise ValueError("passes must be >= 1")
    if x.dtype != y.dtype or x.numel() != y.numel() or y.dim() != 1:
        raise ValueError("x and y must be 1-D tensors of one dtype and size")
    s = k.bit_length() - 1
    if x.dtype == torch.float32 and (k != 1 << s or s * passes > 30):
        raise ValueError("fp32 cascade reference: k must be a power of two, log2(k) * passes <= 30")
    count, first = 0, None
    f0 = first_frame
    while f0 < F:
        f1 = min(F, f0 + chunk_frames)
        h0 = max(0, f0 - passes * (k - 1))
        nf, lead, nb = f1 - f0, f0 - h0, f1 - h0
        xv = x[h0 * C:f1 * C].view(-1, C)
        yv = y[f0 * C:f1 * C].view(-1, C)
        bad = torch.empty((nf, C), dtype=torch.bool, device=x.device)
        for c in range(C):
            P = _column_i64(xv[:, c])
            for j in range(1, passes + 1):
                P = P.cumsum(0)
                S = _window_sums(P, k, 0, 0, 1, nb)     # every frame of the chunk, zeros in front
                last = j == passes
                if x.dtype == torch.int16:
                    v = torch.div(S, k, rounding_mode="trunc")
                    del S
                    if last:
                        bad[:, c] = v[lead:].to(torch.int16) != yv[:, c]
                else:
                    ref = S.to(torch.float64).mul_(2.0 ** (-s * j)).to(torch.float32)
                    del S
                    if last:
                        bad[:, c] = ref[lead:].view(torch.int32) != yv[:, c].view(torch.int32)
                        v = None
                    else:
                        v = ref.to(torch.float64).mul_(2.0 ** (s * j)).to(torch.int64)
                    del ref
                if not last:
                    P[0] = 0
                    P[1:].copy_(v)
                del v
            del P
        count, first = _count(bad, f0 * C, count, first)
        del bad
        f0 = f1
    return count, first


MEANSQ, RMS, VAR, STD = 0, 1, 2, 3     # mavg_stat's values


def _ulp32(ref):
    """numpy.spacing(|ref|) of a float32 tensor, as float64."""
    a = ref.abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))).to(torch.float64) - a.to(torch.float64))


def _bad_one_ulp(y, ref):
    """stat_ref.check_i16: |y - ref| <= one fp32 ulp at ref, exactly 0.0f where ref == 0."""
    bad = ~((y.to(torch.float64) - ref.to(torch.float64)).abs() <= _ulp32(ref))
    return bad | ((ref == 0) & (y != 0))


def chunked_stat_mismatches(x, y, mean, k, C, stat, chunk_frames, first_frame=0):
    """(count, first bad sample or None) of the moving second moment ``stat`` (0 MEANSQ, 1 RMS,
    2 VAR, 3 STD) of int16 or int16-valued fp32 input against exact integer window sums S1, S2
    (two int64 cumsums, one after the other) and N = k S2 - S1^2 in int64 (k <= 65535).  ``y`` and
    ``mean`` (or None) are float32, indexed like ``x``; a sample counts once if either is bad.
    The bars are tests/stat_ref.py's, restated in float64 on the tensors' device:
      int16   check_i16 for y and for the mean: one fp32 ulp at the fp32 rounding of the fp64
              value, exactly 0.0f where that is 0;
      fp32    check_f32 with M = S2 / k; the mean within 1e-5 max(|m|, window mean of |x|)."""
    F = _check_signal(x, k, C, chunk_frames, first_frame)
    if stat not in (MEANSQ, RMS, VAR, STD):
        raise ValueError("stat must be 0..3")
    if k > 65535:
        raise ValueError("k <= 65535: N = k S2 - S1^2 is formed in int64")
    for t in (y,) if mean is None else (y, mean):
        if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != x.numel():
            raise ValueError("y and mean must be 1-D float32 tensors of x's size")
    i16 = x.dtype == torch.int16
    count, first = 0, None
    f0 = first_frame
    while f0 < F:
        f1 = min(F, f0 + chunk_frames)
        h0 = max(0, f0 - (k - 1))
        nf, lead = f1 - f0, f0 - h0
        xv = x[h0 * C:f1 * C].view(-1, C)
        yv = y[f0 * C:f1 * C].view(-1, C)
        mv = mean[f0 * C:f1 * C].view(-1, C) if mean is not None else None
        bad = torch.empty((nf, C), dtype=torch.bool, device=x.device)
        for c in range(C):
            P = _column_i64(xv[:, c])
            need_s1 = stat in (VAR, STD) or mv is not None
            S1 = _window_sums(P.cumsum(0), k, lead, 0, 1, nf) if need_s1 else None
            if mv is not None and not i16:
                A = _window_sums(P.abs().cumsum(0), k, lead, 0, 1, nf).to(torch.float64) / k
            P.mul_(P)                                   # squares of int16 values: exact
            S2 = _window_sums(P.cumsum(0), k, lead, 0, 1, nf)
            del P
            yc = yv[:, c]
            M = S2.to(torch.float64) / k                # S2 < 2^46: exact in float64
            if stat in (MEANSQ, RMS):
                v = M
            else:
                N = k * S2 - S1 * S1
                if bool((N < 0).any()):
                    raise AssertionError("N = k S2 - S1^2 < 0: the reference itself is wrong")
                v = N.to(torch.float64) / (float(k) * float(k))
                del N
            del S2
            if stat in (RMS, STD):
                v = v.sqrt()
            if i16:
                b = _bad_one_ulp(yc, v.to(torch.float32))
            else:
                y64 = yc.to(torch.float64)
                if stat in (MEANSQ, RMS):
                    b = ~((y64 - v).abs() <= 1e-5 * v)
                elif stat == VAR:
                    b = ~((y64 - v).abs() <= 1e-5 * M) | ~(y64 >= 0)
                else:
                    b = ~((y64 * y64 - v * v).abs() <= 1e-5 * M + 2.0 ** -22 * v * v) | ~torch.isfinite(y64) | ~(y64 >= 0)
                del y64
            del v, M
            if mv is not None:
                m = S1.to(torch.float64) / k
                if i16:
                    b |= _bad_one_ulp(mv[:, c], m.to(torch.float32))
                else:
                    b |= ~((mv[:, c].to(torch.float64) - m).abs() <= 1e-5 * torch.maximum(m.abs(), A))
                    del A
                del m
            del S1
            bad[:, c] = b
            del b
        count, first = _count(bad, f0 * C, count, first)
        del bad
        f0 = f1
    return count, first


# ---- extrema, FIR, EMA, biquad: filters with kernels of their own ----
def _chunks(F, W, chunk_frames, first_frame):
    """(h0, f0, f1) of every chunk: frames [f0, f1) compared, read from frame h0 = max(0, f0 - W) on."""
    f0 = first_frame
    while f0 < F:
        f1 = min(F, f0 + chunk_frames)
        yield max(0, f0 - W), f0, f1
        f0 = f1


def _same_size(x, outs, dtype, what):
    for t in outs:
        if t is not None and (t.dtype != dtype or t.dim() != 1 or t.numel() != x.numel()):
            raise ValueError(f"{what} must be 1-D {dtype} tensors of x's size")


def _bits32(t):
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def chunked_extrema_mismatches(x, y_max, y_min, k, C, chunk_frames, first_frame=0):
    """(count, first bad sample or None) of the moving maximum and / or minimum (either output may be
    None, not both) of the causal k-frame window, truncated at frame 0 of ``x`` (frames before
    first_frame are the history).  Exact: every output is one of the samples, bit patterns must be
    equal; a sample counts once if either output is bad.  Per channel column, by log-step doubling:
    r_1 = the column, r_2w[i] = op(r_w[i], r_w[i - w]) for i >= w (a frame closer than w to the
    chunk's start already covers all of it), and a last step of k - w once 2 w > k."""
    F = _check_signal(x, k, C, chunk_frames, first_frame)
    if y_max is None and y_min is None:
        raise ValueError("y_max and y_min must not both be None")
    _same_size(x, (y_max, y_min), x.dtype, "y_max and y_min")
    count, first = 0, None
    for h0, f0, f1 in _chunks(F, k - 1, chunk_frames, first_frame):
        nf, lead = f1 - f0, f0 - h0
        xv = x[h0 * C:f1 * C].view(-1, C)
        bad = torch.zeros((nf, C), dtype=torch.bool, device=x.device)
        for y, op in ((y_max, torch.maximum), (y_min, torch.minimum)):
            if y is None:
                continue
            yv = y[f0 * C:f1 * C].view(-1, C)
            for c in range(C):
                r, w = xv[:, c].clone(), 1
                while 2 * w <= k:
                    if w < r.numel():
                        r[w:] = op(r[w:], r[:-w])     # (the right side is formed before it is stored)
                    w *= 2
                s = k - w
                if 0 < s < r.numel():
                    r[s:] = op(r[s:], r[:-s])
                bad[:, c] |= _bits32(r[lead:]) != _bits32(yv[:, c].contiguous())
                del r
        count, first = _count(bad, f0 * C, count, first)
        del bad
    return count, first


FIR_MAX_TAPS = 8193


def dyadic_taps(ntaps, seed, sparse=False):
    """ntaps host fp64 taps m / 1024, m a seeded integer in [-1024, 1024] that is never 0; with
    ``sparse`` only taps 0, 1, ntaps-2, ntaps-1 and 12 seeded positions between are kept."""
    rng = np.random.default_rng(seed)
    m = rng.integers(1, 1025, ntaps) * rng.choice((-1, 1), ntaps)
    if sparse:
        keep = np.zeros(ntaps, dtype=bool)
        keep[[0, 1, ntaps - 2, ntaps - 1]] = True
        keep[rng.choice(np.arange(2, ntaps - 2), 12, replace=False)] = True
        m = np.where(keep, m, 0)
    return m.astype(np.float64) / 1024.0


def chunked_fir_mismatches(x, y, taps, C, chunk_frames, first_frame=0):
    """(count, first bad sample or None) of y[f] = sum_j taps[j] x[f-j] (fp32 ``y``, frames before
    frame 0 of ``x`` read as zero, frames before first_frame are the history), bit for bit -- for
    exact data only: ``x`` integer-valued with |x| <= 32768 and host fp64 taps m / 1024, |m| <= 1024
    an integer, at most 8193 of them.  Every product and every partial sum is then a multiple of
    2^-10 below 2^28 in magnitude: 38 bits, exact in fp64 in any order, with or without fma, so the
    contract's chain is fl32(exact sum) and the reference adds h[j] * (the column shifted by j) in
    fp64 over the NON-ZERO taps only."""
    h = np.asarray(taps)
    if h.dtype != np.float64 or h.ndim != 1 or not 1 <= h.size <= FIR_MAX_TAPS:
        raise ValueError(f"taps: 1 to {FIR_MAX_TAPS} host float64 values")
    m = h * 1024.0
    if not (np.isfinite(m).all() and (m == np.rint(m)).all() and (np.abs(m) <= 1024).all()):
        raise ValueError("taps must be m / 1024 with an integer |m| <= 1024: the fp64 sums would not be exact")
    ntaps = h.size
    F = _check_signal(x, ntaps, C, chunk_frames, first_frame)
    _same_size(x, (y,), torch.float32, "y")
    nz = [(j, float(h[j])) for j in range(ntaps) if h[j] != 0.0]
    count, first = 0, None
    for h0, f0, f1 in _chunks(F, ntaps - 1, chunk_frames, first_frame):
        nf, lead = f1 - f0, f0 - h0
        xv = x[h0 * C:f1 * C].view(-1, C)
        yv = y[f0 * C:f1 * C].view(-1, C)
        bad = torch.empty((nf, C), dtype=torch.bool, device=x.device)
        for c in range(C):
            col = xv[:, c].to(torch.float64)
            if not bool(((col == col.round()) & (col.abs() <= 32768.0)).all()):
                raise ValueError("FIR reference: inputs must be integer-valued with |x| <= 32768")
            acc = torch.zeros(nf, dtype=torch.float64, device=x.device)
            for j, hj in nz:
                t0 = max(0, j - lead)            # frames of this chunk before it read x[f-j] = 0 (frame < 0)
                if t0 < nf:
                    acc[t0:].add_(col[lead + t0 - j:lead + nf - j], alpha=hj)
            del col
            bad[:, c] = acc.to(torch.float32).view(torch.int32) != yv[:, c].contiguous().view(torch.int32)
            del acc
        count, first = _count(bad, f0 * C, count, first)
        del bad
    return count, first


def ema_lead(alpha):
    """W: the smallest frame count with (1 - alpha)^W <= 2^-60."""
    d = 1.0 - alpha
    if d <= 0.0:
        return 0
    W = max(1, int(math.ceil(-60.0 * math.log(2.0) / math.log1p(-alpha))))
    while d ** W > 2.0 ** -60:
        W += 1
    while W > 1 and d ** (W - 1) <= 2.0 ** -60:
        W -= 1
    return W


def biquad_lead(coef):
    """W: the smallest frame count with rho^W <= 2^-70, rho the larger pole modulus; at least 2."""
    from biquad_ref import pole_radius
    rho = pole_radius(coef)
    if rho <= 0.0:
        return 2
    W = max(2, int(math.ceil(-70.0 * math.log(2.0) / math.log(rho))))
    while rho ** W > 2.0 ** -70:
        W += 1
    while W > 2 and rho ** (W - 1) <= 2.0 ** -70:
        W -= 1
    return W


def _ema_column(col, alpha, W):
    """fp64 EMA of a chunk's column from a zero state in front of it, by decayed doubling:
    e_0 = alpha x, e_(m+1)[f] = e_m[f] + d^(2^m) e_m[f - 2^m] until 2^m >= W."""
    e = col.to(torch.float64).mul_(alpha)
    d, s = np.longdouble(1.0) - np.longdouble(alpha), 1
    while s < W:
        if s < e.numel():
            t = e[:-s] * float(d ** s)
            e[s:] += t
            del t
        s *= 2
    return e


def _biquad_column(col, coef, W, nf):
    """fp64 biquad outputs of the last nf frames of a chunk's column from a zero state in front of
    it.  The state s = (s1, s2) after a frame obeys s' = A s + B x, A = [[-a1, 1], [-a2, 0]],
    B = (b1 - a1 b0, b2 - a2 b0); S_0 = B x and S_(m+1)[f] = S_m[f] + A^(2^m) S_m[f - 2^m] until
    2^m >= W, the matrices squared on the host in np.longdouble; then y[f] = b0 x[f] + s1[f-1]."""
    b0, b1, b2, a1, a2 = (float(v) for v in coef)
    x64 = col.to(torch.float64)
    s1 = x64 * (b1 - a1 * b0)
    s2 = x64 * (b2 - a2 * b0)
    P = np.array([[-a1, 1.0], [-a2, 0.0]], dtype=np.longdouble)
    s = 1
    while s < W:
        if s < x64.numel():
            t1 = s1[:-s] * float(P[0, 0])
            t1.add_(s2[:-s], alpha=float(P[0, 1]))
            t2 = s1[:-s] * float(P[1, 0])
            t2.add_(s2[:-s], alpha=float(P[1, 1]))
            s1[s:] += t1
            s2[s:] += t2
            del t1, t2
        P = P @ P
        s *= 2
    del s2
    lead = x64.numel() - nf
    ref = x64[lead:] * b0
    if lead:
        ref += s1[lead - 1:lead - 1 + nf]
    else:
        ref[1:] += s1[:nf - 1]
    return ref


def _chunked_recursive(x, y, C, M, chunk_frames, first_frame, W, column, abs_term, stats, keep):
    F = _check_signal(x, 1, C, chunk_frames, first_frame)
    if y is not None:
        _same_size(x, (y,), torch.float32, "y")
    if not (math.isfinite(M) and M >= 0.0):
        raise ValueError("M must be finite and >= 0")
    count, first, worst = 0, None, 0.0
    for h0, f0, f1 in _chunks(F, W, chunk_frames, first_frame):
        nf = f1 - f0
        xv = x[h0 * C:f1 * C].view(-1, C)
        bad = torch.empty((nf, C), dtype=torch.bool, device=x.device) if y is not None else None
        for c in range(C):
            ref = column(xv[:, c], nf)
            if keep is not None:
                keep[f0 * C + c:f1 * C:C] = ref.to(keep.device)
            if y is not None:
                err = (y[f0 * C:f1 * C].view(-1, C)[:, c].to(torch.float64) - ref).abs_()
                bar = ref.abs_().mul_(2.0 ** -23).add_(abs_term)
                bad[:, c] = ~(err <= bar)
                if abs_term > 0.0:
                    worst = max(worst, float(err.div_(bar).nan_to_num_(nan=math.inf).max()))
                del err, bar
            del ref
        if y is not None:
            count, first = _count(bad, f0 * C, count, first)
            del bad
    if stats is not None:
        stats["worst"] = worst
    return count, first


def chunked_ema_mismatches(x, y, alpha, C, M, chunk_frames, first_frame=0, stats=None, keep=None):
    """(count, first bad sample or None) of the outputs of frames >= first_frame outside the bar of
    include/mavg.h, |y - ref| <= 2^-23 |ref| + 2^-29 M, with ref the fp64 EMA of the stream ``x``
    from a zero state before its frame 0, formed per chunk by decayed doubling over ema_lead(alpha)
    frames of lead (cut at frame 0, where the state is zero; past the lead a sample weighs at most
    2^-60).  ``stats["worst"]`` receives the largest err / bar seen.  ``keep`` (a 1-D float64
    tensor of x's size, for the tests of this reference itself) receives ref; ``y`` may then be None."""
    if not 0.0 < alpha <= 1.0:
        raise ValueError("alpha must lie in (0, 1]")
    W = ema_lead(alpha)
    return _chunked_recursive(x, y, C, M, chunk_frames, first_frame, W,
                              lambda col, nf: _ema_column(col, alpha, W)[col.numel() - nf:],
                              2.0 ** -29 * M, stats, keep)


def chunked_biquad_mismatches(x, y, coef, C, G, M, chunk_frames, first_frame=0, stats=None, keep=None):
    """chunked_ema_mismatches for the biquad ``coef`` = (b0, b1, b2, a1, a2): the bar is
    |y - ref| <= 2^-23 |ref| + 2^-29 G M, the lead biquad_lead(coef) frames."""
    if len(coef) != 5 or not (math.isfinite(G) and G >= 0.0):
        raise ValueError("coef: five numbers; G finite and >= 0")
    W = biquad_lead(coef)
    return _chunked_recursive(x, y, C, M, chunk_frames, first_frame, W,
                              lambda col, nf: _biquad_column(col, coef, W, nf),
                              2.0 ** -29 * G * M, stats, keep)


def sos_lead(sos):
    """W: the sum of the sections' biquad_lead -- section j spoils the first W_j frames of what it reads."""
    return sum(biquad_lead(c) for c in sos)


def _sos_column(col, rows, leads, nf):
    """fp64 outputs of the last nf frames of a chunk's column through every row of ``rows``, each from
    a zero state in front of the chunk: _biquad_column section by section, its doubling run to the
    section's own lead; a section before the last returns every frame of its column, as fp64, and
    nothing is rounded between sections."""
    cur = col
    for j, (c, W) in enumerate(zip(rows, leads)):
        cur = _biquad_column(cur, c, W, nf if j == len(rows) - 1 else cur.numel())
    return cur


def chunked_sos_mismatches(x, y, sos, C, abs_term, chunk_frames, first_frame=0, stats=None, keep=None):
    """chunked_biquad_mismatches for the cascade ``sos`` (rows b0 b1 b2 a1 a2, fp64 between the
    sections): the bar is |y - ref| <= 2^-23 |ref| + abs_term, with abs_term the absolute term of
    the header's bar as the caller computes it (tests/sos_ref.py: sos_abs_bar_at); the lead is
    sos_lead(sos) frames -- in a chunk that does not start at frame 0, section j's first
    biquad_lead(sos[j]) outputs lack what precedes the chunk, and the sections' shares add up."""
    rows = [tuple(float(v) for v in c) if len(c) == 5 else None for c in sos]
    if not rows or None in rows or not all(math.isfinite(v) for c in rows for v in c):
        raise ValueError("sos: one or more rows of five finite numbers")
    if y is not None and y.dtype != torch.float32:
        raise ValueError("y must be float32")
    leads = [biquad_lead(c) for c in rows]
    return _chunked_recursive(x, y, C, abs_term, chunk_frames, first_frame, sum(leads),
                              lambda col, nf: _sos_column(col, rows, leads, nf), abs_term, stats, keep)


# The coefficients of the > 2^32-sample cases (tests/test_gpu_bigsignal_filters.py); the CPU tests of
# this reference (tests/test_bigsignal_ref.py) measure it against the literal loops at the same ones.
BIG_EMA_ALPHAS = (0.05, 0.01, 0.0051, 0.0026, 1e-4)
BIG_BIQUADS = (("LP", 0.1, 0.707), ("LP", 0.002, 0.707), ("BP", 0.01, 4.0), ("HP", 0.0005, 0.7071))   # biquad_ref.rbj's kind, f, Q
BIG_SOS = ("butter4", "three", "hp_pk", "limit8", "past9")     # big_sos's names


def big_sos(name, halo_of):
    """The rows (b0 b1 b2 a1 a2) of a named section set of the big cascade cases.  halo_of: the
    library's mavg_biquad_halo_frames -- limit8 is tests/sos_ref.py's SEVEN and a one-pole low-pass
    fitted so that the halos sum to stereo's limit of 1024 frames, past9 SEVEN, a one_pole(0.5) and
    a fitted one-pole whose halos sum to one frame more."""
    import sos_ref
    if name == "limit8":
        return sos_ref.sections_with_halo(1024, halo_of, sos_ref.SEVEN)
    if name == "past9":
        return sos_ref.sections_with_halo(1025, halo_of, sos_ref.SEVEN + [sos_ref.one_pole(0.5)])
    return list({"butter4": sos_ref.butter4_lp(0.05), "three": sos_ref.THREE, "hp_pk": sos_ref.HP_PK}[name])
