"""CPU checks of the references tests/test_gpu_i16_range.py relies on, on its own signals
(tests/i16_range.py): the C oracle and the independent numpy formulation agree bit for bit at full
scale, the exact window sums reach both ends of [-32768 k, 32767 k], and the stairs visit the
quotient boundaries q k - 1, q k, q k + 1 and change the output at exactly one frame per step."""
import numpy as np
import pytest

import i16_range as R

# every window the GPU file uses on mavg_run, the rows, ragged and decimated scans and the moments
WINDOWS = (2, 16, 17, 100, 255, 256, 257, 4096, 8192, 32767, 32768, 44100, 65535, 65536, 65537, 70000)


@pytest.mark.parametrize("k", WINDOWS)
def test_oracle_and_numpy_agree_bit_for_bit(oracle_mod, k):
    frames = R.frames_for(k)
    for C in (1, 2) if k > 257 else (1, 2, 4, 8):
        for name in R.NAMES:
            x = R.signal(oracle_mod, name, k, frames, C)
            y = oracle_mod.mavg_i16(x, k, C)
            assert y.dtype == np.int16 and np.array_equal(y, oracle_mod.numpy_mavg_i16(x, k, C)), (name, k, C)
            if name == "stairs":
                R.assert_stairs_change_once(y.reshape(-1, C)[:, 0], k, "oracle")
            if name in ("top", "bottom"):        # the average of a constant is the constant, on both channels
                assert np.array_equal(y[(k - 1) * C:], x[(k - 1) * C:]), (name, k, C)


@pytest.mark.parametrize("k", (2, 257, 8192, 65535, 65536, 70000))
def test_window_sums_reach_both_ends(oracle_mod, k):
    C = 2
    for name, want in (("top", {R.TOP * k}), ("bottom", {R.BOTTOM * k}), ("blocks", {R.TOP * k, R.BOTTOM * k})):
        frames = R.frames_needed(name, k)
        x = R.signal(oracle_mod, name, k, frames, C)
        S = oracle_mod.window_sum_i64(x, k, C, 0, frames).reshape(-1, C)
        assert np.array_equal(S.reshape(-1), oracle_mod.numpy_window_sum(x, k, C)), (name, k)
        assert S.min() >= R.BOTTOM * k and S.max() <= R.TOP * k
        assert want <= set(np.unique(S[:, 0]).tolist()), (name, k)
        assert {-s - k for s in want} <= set(np.unique(S[:, 1]).tolist()), (name, k, "odd channel")
        if name == "blocks":                     # crosses zero in both directions
            sg = np.sign(S[k:, 0])
            assert ((sg[:-1] > 0) & (sg[1:] <= 0)).any() and ((sg[:-1] < 0) & (sg[1:] >= 0)).any()
    if k <= 65535:
        assert R.BOTTOM * k >= -2 ** 31 and R.BOTTOM * 65535 == -2147450880     # 32768 short of wrapping an int32


@pytest.mark.parametrize("k", (2, 17, 256, 257, 8192, 65535, 65536))
def test_stairs_visit_the_quotient_boundaries(oracle_mod, k):
    frames = R.stairs_frames(k)
    x = R.signal(oracle_mod, "stairs", k, frames, 1)
    S = oracle_mod.window_sum_i64(x, k, 1, 0, frames)
    steps = R.stair_steps(k)
    assert len(steps) == 6 and [L for _, L in steps] == [-32768, -32767, -1, 0, 32765, 32766]
    for s, L in steps:
        assert np.array_equal(S[s - 1:s + k], L * k + np.arange(k + 1)), (k, L)     # every value L k + r
    have = set(S.tolist())
    for q in (-32767, 0, 32766):                 # a level entered and left by unit steps: all three
        assert {q * k - 1, q * k, q * k + 1} <= have, (k, q)
    assert {R.BOTTOM * k, R.BOTTOM * k + 1, R.TOP * k - 1, R.TOP * k} <= have
