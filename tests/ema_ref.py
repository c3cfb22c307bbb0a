"""The reference of the exponential moving average's tests: the fp64 recurrence
y[f] = (1 - alpha) y[f-1] + alpha x[f] per channel, evaluated block-wise in numpy, and the accuracy
bar of include/mavg.h.  No scipy."""
import numpy as np

BLOCK = 4096


def ema_loop(x, alpha, channels=1, state=None):
    """The literal loop (slow: what ema_ref is checked against)."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, channels)
    d = 1.0 - alpha
    y = np.empty_like(x)
    for c in range(channels):
        prev = 0.0 if state is None else float(state[c])
        col = []
        for v in x[:, c].tolist():      # Python floats are fp64
            prev = d * prev + alpha * v
            col.append(prev)
        y[:, c] = col
    return y.reshape(-1)


def ema_ref(x, alpha, channels=1, state=None):
    """fp64 y, in x's interleaved layout.  Blocks of BLOCK frames run in lock-step from a zero
    state (a serial loop over the positions inside a block, vectorised over the blocks); a serial
    carry then runs over the blocks and enters position i of a block as d^(i+1) times itself."""
    C = channels
    x = np.asarray(x, dtype=np.float64).reshape(-1, C)
    n = x.shape[0]
    d = 1.0 - alpha
    nb = -(-n // BLOCK) if n else 0
    xp = np.zeros((nb * BLOCK, C))
    xp[:n] = x
    xb = xp.reshape(nb, BLOCK, C)
    yb = np.empty_like(xb)
    acc = np.zeros((nb, C))
    for i in range(BLOCK):
        acc = d * acc + alpha * xb[:, i, :]
        yb[:, i, :] = acc
    w = d ** np.arange(1, BLOCK + 1, dtype=np.float64)   # the carry's weight at position i: d^(i+1)
    carry = np.zeros(C) if state is None else np.asarray(state, dtype=np.float64).copy()
    for b in range(nb):
        yb[b] += w[:, None] * carry[None, :]
        carry = yb[b, BLOCK - 1].copy()
    return yb.reshape(nb * BLOCK, C)[:n].reshape(-1)


def ema_scale(x, state=None):
    """M: the largest of |x| over the signal and |state_in|."""
    m = float(np.abs(np.asarray(x, dtype=np.float64)).max()) if np.size(x) else 0.0
    if state is not None and np.size(state):
        m = max(m, float(np.abs(np.asarray(state, dtype=np.float64)).max()))
    return m


def ema_bar(ref, M):
    """|y - y_ref| <= 2^-23 |y_ref| + 2^-29 M, element-wise."""
    return 2.0 ** -23 * np.abs(ref) + 2.0 ** -29 * M
