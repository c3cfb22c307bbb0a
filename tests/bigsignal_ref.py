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
  chunked_stat_mismatches     S1 and S2 of int16(-valued) input, the bars of tests/stat_ref.py"""
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
