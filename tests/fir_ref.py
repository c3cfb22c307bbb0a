"""References for the FIR filter (mavg_fir_run, include/mavg.h).

fir_chain is the contract itself: per output one fp64 chain, the accumulator starting at +0.0, then
acc = acc + h[j] * x[f-j] for j = ntaps-1 down to 0 (oldest frame first), rounded to fp32.  numpy
has no fma, but the product h * x is exact in fp64 whenever the taps are fp32-representable (24-bit
by 24-bit or 24-bit by 16-bit mantissas), and then the add of the exact product is the fma: for
such taps this reference is bit for bit the contract.  Frames before frame 0 are zeros (or the
history); a zero frame adds +-0.0 to an accumulator that is never -0.0, which changes nothing.

fir_bar is the header's accuracy bar; fir_exact_i16 an int64 convolution for integer taps;
fir_longdouble a direct sum in np.longdouble for taps that are not fp32-valued."""
import numpy as np


def _padded(x, ntaps, C, history):
    """[ntaps - 1 + frames, C] fp64: the history (or zeros) in front of the signal."""
    xs = np.asarray(x).reshape(-1, C)
    H = ntaps - 1
    if history is None:
        head = np.zeros((H, C), dtype=xs.dtype)
    else:
        head = np.asarray(history).reshape(-1, C)
        assert head.shape[0] == H and head.dtype == xs.dtype
    return np.concatenate([head, xs]).astype(np.float64)


def fir_chain(x, taps, C=1, history=None):
    """The contract's chain in fp64, vectorised over frames; fp32 in x's interleaved layout."""
    h = np.asarray(taps, dtype=np.float64)
    ntaps = h.size
    assert h.ndim == 1 and ntaps >= 1
    p = _padded(x, ntaps, C, history)
    frames = p.shape[0] - (ntaps - 1)
    acc = np.zeros((frames, C), dtype=np.float64)
    for j in range(ntaps - 1, -1, -1):
        s = ntaps - 1 - j                      # x[f - j] of frame f sits at padded row f + (ntaps - 1) - j
        acc += h[j] * p[s:s + frames]
    return acc.astype(np.float32).reshape(-1)


def fir_bar(y_ref, taps, M):
    """|y - y_ref| <= 2^-23 |y_ref| + 2^-36 G M (scaled by ntaps / 8192 past 8192 taps)."""
    h = np.abs(np.asarray(taps, dtype=np.float64))
    G = float(h.sum())
    scale = max(1.0, h.size / 8192.0)
    return 2.0 ** -23 * np.abs(np.asarray(y_ref, dtype=np.float64)) + 2.0 ** -36 * G * float(M) * scale


def fir_exact_i16(x, taps, C=1):
    """The exact integer sums of an int16 signal with integer taps, int64, zero history."""
    h = np.asarray(taps)
    assert np.issubdtype(h.dtype, np.integer)
    xs = np.asarray(x).reshape(-1, C).astype(np.int64)
    assert float(np.abs(h.astype(np.float64)).sum()) * 32768.0 < 2.0 ** 62
    out = np.empty_like(xs)
    for c in range(C):
        out[:, c] = np.convolve(xs[:, c], h.astype(np.int64))[:xs.shape[0]]
    return out.reshape(-1)


def fir_longdouble(x, taps, C=1, history=None):
    """A direct sum in np.longdouble (newest frame first: not the contract's order), longdouble."""
    h = np.asarray(taps, dtype=np.longdouble)
    ntaps = h.size
    p = _padded(x, ntaps, C, history).astype(np.longdouble)
    frames = p.shape[0] - (ntaps - 1)
    acc = np.zeros((frames, C), dtype=np.longdouble)
    for j in range(ntaps):
        s = ntaps - 1 - j
        acc += h[j] * p[s:s + frames]
    return acc.reshape(-1)
