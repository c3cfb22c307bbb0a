"""A numpy restatement of one tile of cascade_tile_kernel (csrc/mavg_cascade.hpp) against the oracle
applied `passes` times: a stage of the halo units plus the tile's frames, `passes` in-stage passes
with the dtype's rounding, each pass scanning from cascade_first_unit on and reading what lies
below the stage as zero, only the span frame >= -(passes - j)(k - 1) trusted after pass j.  It pins
that a halo of H = passes * (k - 1) frames suffices and that H - 1 does not.  No GPU."""
import numpy as np
import pytest

POISON = {np.int16: 12345, np.float32: 6.0e4}


def oracle_pass(oracle, x, k, C):
    return oracle.mavg_i16(x, k, C) if x.dtype == np.int16 else oracle.mavg_f32(x, k, C)


def oracle_cascade(oracle, x, k, C, p):
    """[p + 1, frames, C]: x and the result of each pass."""
    ys = [x]
    for _ in range(p):
        ys.append(oracle_pass(oracle, ys[-1], k, C))
    return [y.reshape(-1, C) for y in ys]


def first_unit(Hu, xk_units, p, j):
    """cascade_first_unit (mavg_cascade.hpp)."""
    return max(0, Hu - (p - j) * xk_units)


def one_pass(src, f0, k):
    """Window means of src [frames, C] for frames >= f0, frames below 0 read as zero; nothing below
    max(0, f0 - k + 1) is touched.  int16: exact sum, truncating division; fp32: fp64 sum, float(S / k)."""
    lo = max(0, f0 - k + 1)
    wide = np.int64 if src.dtype == np.int16 else np.float64
    P = np.concatenate([np.zeros((k, src.shape[1]), wide), np.cumsum(src[lo:].astype(wide), axis=0)])
    S = P[k + (f0 - lo):] - P[(f0 - lo):-k]
    if src.dtype == np.int16:
        return (np.sign(S) * (np.abs(S) // k)).astype(np.int16)
    return (S / k).astype(np.float32)


def tile_model(frame, t0, TF, k, p, C, F, Hs, dtype, trusted=None):
    """The tile's TF output frames.  frame(a, b) -> [b - a, C]: the signal's frames [a, b), with
    whatever stands before frame 0 (history or zeros).  Hs: the halo frames staged (H in the
    kernel); F: frames per unit.  trusted(j, first_frame, values) is called after every pass with
    the span the kernel relies on."""
    Hu = -(-Hs // F)
    Ha = Hu * F
    xk_units = -(-k // F)
    src = frame(t0 - Ha, t0 + TF).astype(dtype)
    for j in range(1, p + 1):
        f0 = first_unit(Hu, xk_units, p, j) * F
        assert f0 <= max(0, Ha - (p - j) * (k - 1))          # the trusted span is scanned
        # x[n-k] reads (whole units) stay inside what pass j-1 wrote, or fall below the stage (zero)
        assert j == 1 or prev_f0 == max(0, f0 - xk_units * F)
        dst = np.full_like(src, POISON[dtype])
        dst[f0:] = one_pass(src, f0, k)
        if trusted is not None:
            v = max(0, Ha - (p - j) * (k - 1))
            trusted(j, t0 - Ha + v, dst[v:])
        src, prev_f0 = dst, f0
    return src[Ha:]


def make_signal(oracle, kind, frames, C, seed):
    if kind == "i16":
        return oracle.synth_i16(frames * C, seed=seed)
    return oracle.synth_f32(frames * C, seed=seed, dist=2)


def close(kind, y, ref, F=None):
    if kind == "i16":
        return y == ref
    r = ref.astype(np.float64)
    return np.abs(y.astype(np.float64) - r) <= 1e-5 * np.maximum(np.abs(r), F)


def mean_abs(x, k, C, p):
    """The p-fold moving mean of |x| in float64 (the fp32 bar's floor)."""
    a = np.abs(x.astype(np.float64)).reshape(-1, C)
    for _ in range(p):
        P = np.concatenate([np.zeros((k, C)), np.cumsum(a, axis=0)])
        a = (P[k:] - P[:-k]) / k
    return a


@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("k", [2, 3, 100])
@pytest.mark.parametrize("p", [2, 3, 4])
def test_tile_model_matches_the_oracle_applied_p_times(oracle_mod, kind, C, k, p):
    dtype = np.int16 if kind == "i16" else np.float32
    TF, H = 256, p * (k - 1)
    frames = 3 * TF + 17
    Z = H + 16                       # zero frames in front: every staged frame exists in `ext`
    for with_hist in (False, True):
        pre = H if with_hist else 0
        long = make_signal(oracle_mod, kind, frames + pre, C, seed=1000 * p + 10 * k + C + pre)
        # the reference: the oracle applied p times to concat(history, x), the first H frames
        # dropped; zeros in front of that change nothing (the average of zeros is zero) and give
        # every intermediate at the frames before frame 0 as well
        ext = np.concatenate([np.zeros(Z * C, dtype), long])
        off = Z + pre                # ext frame of x's frame 0
        stages = oracle_cascade(oracle_mod, ext, k, C, p)
        direct = oracle_cascade(oracle_mod, long, k, C, p)[p][pre:]
        assert np.array_equal(stages[p][off:], direct)
        floors = [None] + [np.maximum(mean_abs(ext, k, C, j), 1e-30) for j in range(1, p + 1)] if kind == "f32" else None

        def frame(a, b):
            out = np.zeros((b - a, C), dtype)
            hi = min(b, frames)
            out[:hi - a] = stages[0][a + off:hi + off]
            return out

        def trusted(j, f_first, vals):
            n = min(vals.shape[0], frames - f_first)
            want = stages[j][f_first + off:f_first + off + n]
            Fj = floors[j][f_first + off:f_first + off + n] if floors else None
            ok = close(kind, vals[:n], want, Fj)
            assert ok.all(), (with_hist, j, f_first, np.argwhere(~ok)[:3])

        for F in (1, 16 // (C * np.dtype(dtype).itemsize)):
            for t0 in (0, TF, 2 * TF, 3 * TF):   # tile 0 (zeros or history in front), interior tiles, the partial tile
                y = tile_model(frame, t0, TF, k, p, C, F, H, dtype, trusted)
                n = min(TF, frames - t0)
                ok = close(kind, y[:n], direct[t0:t0 + n], floors[p][t0 + off:t0 + off + n] if floors else None)
                assert ok.all(), (with_hist, F, t0, np.argwhere(~ok)[:3])


@pytest.mark.parametrize("kind", ["i16", "f32"])
@pytest.mark.parametrize("k,p", [(2, 2), (3, 4), (100, 3)])
def test_a_stage_one_frame_short_is_wrong(oracle_mod, kind, k, p):
    """With H - 1 halo frames (frame units: no rounding up) at least one output of an interior tile
    differs: y[t0] depends on x[t0 - H]."""
    dtype = np.int16 if kind == "i16" else np.float32
    C, TF, H = 1, 256, p * (k - 1)
    frames, t0 = 3 * TF, 2 * TF
    assert t0 - H >= 0
    # a positive constant: every full window averages to it exactly, in both dtypes; a window that
    # misses x[t0 - H] comes out smaller (int16: by the truncation, c - 1), and so does every later
    # pass's window that holds that value
    x = np.full(frames, 1000, dtype)
    ref = oracle_cascade(oracle_mod, x, k, C, p)[p]

    def frame(a, b):
        out = np.zeros((b - a, C), dtype)
        lo, hi = max(a, 0), min(b, frames)
        out[lo - a:hi - a] = x.reshape(-1, C)[lo:hi]
        return out

    good = tile_model(frame, t0, TF, k, p, C, 1, H, dtype)
    short = tile_model(frame, t0, TF, k, p, C, 1, H - 1, dtype)
    assert np.array_equal(good, ref[t0:]) and (good == 1000).all()
    assert good[0, 0] != short[0, 0], (good[0, 0], short[0, 0])
    assert np.array_equal(good[1:], short[1:])      # only the frame that needs x[t0 - H]
