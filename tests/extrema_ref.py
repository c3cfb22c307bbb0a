"""Pure-numpy reference of the moving extrema (mavg_extrema_run, include/mavg.h): per channel the
maximum and the minimum of the causal ``grade``-frame window.  Frames before frame 0 come from the
history when one is given; without one the window is truncated at frame 0, which the reference
states by padding with the extremum's identity (the dtype's lowest value for a maximum, its highest
for a minimum), never with zeros.

Two evaluations of the same definition: ``sliding_window_view(...).max/min`` (k compares per
output: small shapes) and an O(n log k) doubling; ``moving_extrema_ref`` picks by size, and
tests/test_extrema_model.py checks them against each other and against a literal loop."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view


def identity(dtype, want_max: bool):
    """The value that never wins: the lowest of the dtype for a maximum, the highest for a minimum."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return dtype.type(-np.inf if want_max else np.inf)
    info = np.iinfo(dtype)
    return dtype.type(info.min if want_max else info.max)


def _padded(x, grade, channels, history, want_max):
    x2 = np.ascontiguousarray(x).reshape(-1, channels)
    if history is not None:
        pre = np.asarray(history, dtype=x2.dtype).reshape(-1, channels)
        assert pre.shape[0] == grade - 1, "history holds grade - 1 frames"
    else:
        pre = np.full((grade - 1, channels), identity(x2.dtype, want_max), dtype=x2.dtype)
    return np.concatenate([pre, x2], axis=0)


def _sliding(p, grade, want_max):
    w = sliding_window_view(p, grade, axis=0)          # [n, C, grade]
    return w.max(axis=2) if want_max else w.min(axis=2)


def _doubling(p, grade, want_max):
    op = np.maximum if want_max else np.minimum
    r, w = p, 1                                        # r[i] = extremum of p[i - w + 1 .. i]
    while 2 * w <= grade:
        nxt = r.copy()
        nxt[w:] = op(r[w:], r[:-w])
        r, w = nxt, 2 * w
    n = p.shape[0] - (grade - 1)
    hi = r[grade - 1:grade - 1 + n]                    # windows of w frames ending at the frame
    lo = r[w - 1:w - 1 + n]                            # ... and starting at the window's first frame
    return op(hi, lo)


def moving_extremum_ref(x, grade, channels=1, history=None, want_max=True, method=None):
    """The moving maximum (``want_max``) or minimum of ``x`` (interleaved, any shape holding whole
    frames), in ``x``'s dtype and shape."""
    x = np.asarray(x)
    assert grade >= 1 and x.size % channels == 0
    p = _padded(x, grade, channels, history, want_max)
    if method is None:
        method = "sliding" if p.shape[0] * grade <= (1 << 22) else "doubling"
    y = _sliding(p, grade, want_max) if method == "sliding" else _doubling(p, grade, want_max)
    return np.ascontiguousarray(y).astype(x.dtype, copy=False).reshape(x.shape)


def moving_extrema_ref(x, grade, channels=1, history=None, method=None):
    """``(max, min)`` of the causal ``grade``-frame window."""
    return (moving_extremum_ref(x, grade, channels, history, True, method),
            moving_extremum_ref(x, grade, channels, history, False, method))
