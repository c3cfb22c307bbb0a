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
not.  tests/test_bigsignal_ref.py pins this to the C oracle bit for bit."""
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
