"""tests/bigsignal_ref.py (the plain-torch reference of the > 2^32-sample GPU
tests) pinned to the C oracle on the CPU: bit-equal verdicts for every
(C, k, chunking), and single-sample tampering found at exactly its index."""
import functools

import numpy as np
import pytest
import torch

from bigsignal_ref import chunked_mismatches

FRAMES = 5 * 16384            # > 70001, so the longest window leaves its warm-up
CHUNKS = (16384, 10007)       # divides FRAMES / does not (and < k: boundaries inside the warm-up)
CS = (1, 2, 3, 8)
KS = (1, 2, 7, 1000, 5000, 70001)


@functools.lru_cache(maxsize=None)
def _signal(oracle_mod, C, dt):
    n = FRAMES * C
    return oracle_mod.synth_i16(n, seed=C) if dt == "i16" else oracle_mod.synth_f32(n, seed=C, dist=0)


@functools.lru_cache(maxsize=None)
def _pair(oracle_mod, C, k, dt):
    """(x, oracle output) as torch tensors; shared, never modified (tests clone)."""
    x = _signal(oracle_mod, C, dt)
    y = oracle_mod.mavg_i16(x, k, C) if dt == "i16" else oracle_mod.mavg_f32(x, k, C)
    return torch.from_numpy(x), torch.from_numpy(y)


@pytest.mark.parametrize("dt", ["i16", "f32"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("C", CS)
def test_reference_equals_oracle_bit_for_bit(oracle_mod, C, k, dt):
    x, y = _pair(oracle_mod, C, k, dt)
    for chunk in CHUNKS:
        assert chunked_mismatches(x, y, k, C, chunk) == (0, None), (C, k, dt, chunk)


def test_saturated_signal_longest_window(oracle_mod):
    """All -32768 at k = 70001: window sums past int32 (-2.29e9), truncation of a negative quotient."""
    k = 70001
    for C in (1, 2):
        xi = np.full(FRAMES * C, -32768, np.int16)
        for x, y in ((xi, oracle_mod.mavg_i16(xi, k, C)),
                     (xi.astype(np.float32), oracle_mod.mavg_f32(xi.astype(np.float32), k, C))):
            for chunk in CHUNKS:
                assert chunked_mismatches(torch.from_numpy(x), torch.from_numpy(y), k, C, chunk) == (0, None)


def _tamper(y, i):
    y = y.clone()
    bits = y.view(torch.int16 if y.dtype == torch.int16 else torch.int32)
    bits[i] ^= 1                      # one flipped output bit
    return y


@pytest.mark.parametrize("dt", ["i16", "f32"])
@pytest.mark.parametrize("C,k", [(1, 7), (2, 1000), (3, 70001), (8, 5000)])
def test_single_tampered_output_is_reported_at_its_index(oracle_mod, C, k, dt):
    x, y = _pair(oracle_mod, C, k, dt)
    n = x.numel()
    for chunk in CHUNKS:
        nchunks = -(-FRAMES // chunk)
        # first sample, one inside the first chunk's warm-up, the last sample of a
        # middle chunk, the first sample of the next one, and the last sample
        mid = (nchunks // 2) * chunk * C
        for i in (0, min(k, chunk) * C // 2, mid - 1, mid, n - 1):
            assert chunked_mismatches(x, _tamper(y, i), k, C, chunk) == (1, i), (chunk, i)
    # several: the count is the total, the index the lowest
    y3 = _tamper(_tamper(_tamper(y, n - 1), n // 2), 5 * C)
    assert chunked_mismatches(x, y3, k, C, CHUNKS[1]) == (3, 5 * C)


@pytest.mark.parametrize("C,k", [(1, 2), (2, 705), (8, 70001)])
def test_first_frame_skips_exactly_the_frames_before_it(oracle_mod, C, k):
    """The history form: outputs of frames < first_frame are not looked at,
    every later one is, against windows that reach back before first_frame."""
    x, y = _pair(oracle_mod, C, k, "i16")
    ff = k - 1
    junk = y.clone()
    junk[:ff * C] = 0x5A5A
    for chunk in CHUNKS:
        assert chunked_mismatches(x, junk, k, C, chunk, first_frame=ff) == (0, None)
        if ff:
            assert chunked_mismatches(x, _tamper(junk, ff * C - 1), k, C, chunk, first_frame=ff) == (0, None)
        assert chunked_mismatches(x, _tamper(junk, ff * C), k, C, chunk, first_frame=ff) == (1, ff * C)
        last = x.numel() - 1
        assert chunked_mismatches(x, _tamper(junk, last), k, C, chunk, first_frame=ff) == (1, last)


def test_warm_up_chunk_boundaries(oracle_mod):
    """Chunks far shorter than the window: every boundary of the first k frames
    falls inside the warm-up, and the overlap is cut at frame 0."""
    for C, k, chunk in ((1, 5000, 333), (3, 5000, 1000), (2, 70001, 4999)):
        x, y = _pair(oracle_mod, C, k, "i16")
        assert chunked_mismatches(x, y, k, C, chunk) == (0, None)
        i = (k - 1) * C - 1           # the last warm-up output
        assert chunked_mismatches(x, _tamper(y, i), k, C, chunk) == (1, i)


def test_rejects_what_it_cannot_check():
    x = torch.zeros(6, dtype=torch.float32)
    with pytest.raises(ValueError):
        chunked_mismatches(x, x, 2, 4, 8)                      # partial frame
    with pytest.raises(ValueError):
        chunked_mismatches(x + 0.5, x, 2, 1, 8)                # fp32 sums would not be exact
    with pytest.raises(TypeError):
        chunked_mismatches(x.double(), x.double(), 2, 1, 8)
