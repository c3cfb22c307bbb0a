"""The input that maximises what a truncating IIR tile drops (ema_tile, biquad_tile: the carry of a
tile that starts at frame t0 is rebuilt from H halo frames, everything older is dropped).

    x[j] = M sgn(h[t0 - j])   for j <= t0,   sgn(0) = +1

makes every term of y[t0] = sum_n h[n] x[t0 - n] positive: y_ref[t0] = M sum_{n <= t0} |h[n]|, G M up
to the response's own tail past t0, the largest output the filter can give, and the dropped part of
it is the whole tail M sum_{H < n <= t0} |h[n]|.  On noise that tail mostly cancels.  After t0 the
input alternates +-M (any bounded continuation does: the tile's error past t0 is the same dropped
history, decaying).  numpy only."""
import numpy as np


def sgn(h):
    return np.where(np.asarray(h) < 0, -1.0, 1.0)         # sgn(0) = +1


def worst_case_input(h, t0, n, M=1.0):
    """fp64 x[0 .. n): M sgn(h[t0 - j]) up to t0 (h: the signed impulse response, at least t0 + 1
    frames of it), then -+M alternating, starting opposite to x[t0]."""
    h = np.asarray(h, dtype=np.float64)
    assert 0 <= t0 < n and h.size > t0
    x = np.empty(n)
    x[:t0 + 1] = sgn(h[t0::-1][:t0 + 1])
    alt = np.where(np.arange(1, n - t0) & 1, -1.0, 1.0) * x[t0]
    x[t0 + 1:] = alt
    return M * x


def ema_impulse(alpha, n):
    """alpha (1 - alpha)^m, m = 0 .. n - 1: never negative, so the EMA's worst case is a constant."""
    return alpha * (1.0 - alpha) ** np.arange(n, dtype=np.float64)


def as_f32(x, C=1):
    """The pattern as fp32 (+-1 is exact), interleaved: channel 0 the pattern, channel 1 its negation."""
    assert C in (1, 2) and (np.abs(x) == 1.0).all()
    cols = [x, -x][:C]
    out = np.stack(cols, axis=1).reshape(-1).astype(np.float32)
    out.setflags(write=False)
    return out


def as_i16(x, C=1):
    """The pattern at full scale: +1 -> 32767, -1 -> -32768; channel 1 the negation, the two ends swapped."""
    assert C in (1, 2) and (np.abs(x) == 1.0).all()
    full = lambda s: np.where(s > 0, 32767, -32768).astype(np.int16)    # noqa: E731
    out = np.stack([full(x), full(-x)][:C], axis=1).reshape(-1)
    out.setflags(write=False)
    return out


def first_tile_past(H, tile_frames):
    """The start of the first tile that begins past H frames: its whole halo lies inside the signal
    and at least one frame in front of the halo is dropped."""
    return (H // tile_frames + 1) * tile_frames
