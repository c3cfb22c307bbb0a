"""int16 test signals at the ends of the range, for the moving-average kernels (tests/test_i16_range_refs.py
on the CPU, tests/test_gpu_i16_range.py on the GPU).  A window sum of k int16 samples lies in
[-32768 k, 32767 k]; seeded zero-mean noise stays near sqrt(k) * 19000, far inside it.  These reach
the ends and every remainder of the output division:

  top, bottom            constant 32767 / -32768: S = 32767 k / -32768 k from frame k - 1 on
  top-band, bottom-band  32767 - (noise & 15) / -32768 + (noise & 15): the largest |S|, every remainder
  blocks(k)              32767 for k frames, -32768 for k frames, ...: S sweeps the whole interval and
                         crosses zero in both directions
  stairs(k)              unit steps L -> L + 1, each level held k + 3 frames, in three regions: from
                         -32768 up, across -1, 0, 1, and up to 32767.  Between two levels S takes every
                         value L k + r, r = 0 .. k, and the output (truncated toward zero) changes at
                         exactly one frame: the last for L >= 0, the first for L < 0.

Signals are interleaved and read-only.  Odd channels carry the negated signal with -32768 and 32767
swapped, so a frame holds both extremes and a slip from one channel into the next shows."""
import numpy as np

TOP, BOTTOM = 32767, -32768
NAMES = ("top", "bottom", "top-band", "bottom-band", "blocks", "stairs")
STAIR_LEVELS = (-32768, -32767, -32766, -1, 0, 1, 32765, 32766, 32767)
STRIP_FRAMES = 6161         # kernels without a tile: some hundred strips, a ragged last one


def negate_swap(x):
    """-x, with -32768 <-> 32767 (the negation of -32768 is not an int16)."""
    x = np.asarray(x, dtype=np.int16)
    return np.where(x == BOTTOM, TOP, np.where(x == TOP, BOTTOM, -x.astype(np.int32))).astype(np.int16)


def interleave(base, C):
    """[frames] -> interleaved [frames * C]: even channels the signal, odd channels negate_swap of it."""
    cols = [base if c % 2 == 0 else negate_swap(base) for c in range(C)]
    return np.ascontiguousarray(np.stack(cols, axis=1).reshape(-1))


def stairs_frames(k):
    return len(STAIR_LEVELS) * (k + 3) + k


def frames_needed(name, k):
    """The frames a signal needs to do what it is for: constants and bands a full window and a few
    frames more, blocks two periods, stairs every level and a window past the last."""
    return {"blocks": 4 * k, "stairs": stairs_frames(k)}.get(name, k + 17)


def stair_steps(k):
    """[(frame of the first sample at L + 1, L)] for the unit steps of stairs(k)."""
    hold = k + 3
    return [((i + 1) * hold, a) for i, (a, b) in enumerate(zip(STAIR_LEVELS, STAIR_LEVELS[1:])) if b == a + 1]


def mono(oracle, name, k, frames, seed=1):
    """One channel of `frames` frames (any length: periodic signals repeat, the last stair level is held)."""
    if name == "top":
        return np.full(frames, TOP, dtype=np.int16)
    if name == "bottom":
        return np.full(frames, BOTTOM, dtype=np.int16)
    if name == "top-band":
        return (TOP - (oracle.synth_i16(frames, seed=seed) & 15)).astype(np.int16)
    if name == "bottom-band":
        return (BOTTOM + (oracle.synth_i16(frames, seed=seed) & 15)).astype(np.int16)
    f = np.arange(frames, dtype=np.int64)
    if name == "blocks":
        return np.where((f // k) % 2 == 0, TOP, BOTTOM).astype(np.int16)
    if name == "stairs":
        level = np.minimum(f // (k + 3), len(STAIR_LEVELS) - 1)
        return np.array(STAIR_LEVELS, dtype=np.int16)[level]
    raise ValueError(name)


_signals = {}


def signal(oracle, name, k, frames, C=1, seed=1):
    """The interleaved signal, made once per shape and never modified."""
    key = (name, k if name in ("blocks", "stairs") else 0, frames, C, seed)
    if key not in _signals:
        x = interleave(mono(oracle, name, k, frames, seed), C)
        x.setflags(write=False)
        _signals[key] = x
    return _signals[key]


def frames_for(k, tile_frames=None, names=NAMES):
    """Three tiles plus 17 frames (6161 where there is no tile), or what the signals need if that is more."""
    base = 3 * tile_frames + 17 if tile_frames else STRIP_FRAMES
    return max([base] + [frames_needed(n, k) for n in names])


def assert_stairs_change_once(y0, k, what=""):
    """y0: channel 0 of the moving average of stairs(k), zero history.  Across each unit step L -> L + 1
    the output is L up to one frame and L + 1 from it on: the step's last window frame for L >= 0 (the
    quotient reaches L + 1 only at S = (L + 1) k), its first for L < 0 (truncation toward zero: S = L k + 1
    already gives L + 1)."""
    for s, L in stair_steps(k):
        if s < k:
            continue                                # the window still reaches before frame 0
        seg = y0[s - 1:s + k]                       # S = L k + r, r = 0 .. k
        change = k if L >= 0 else 1
        assert (seg[:change] == L).all() and (seg[change:] == L + 1).all(), (what, k, L, np.flatnonzero(np.diff(seg)) + s)
