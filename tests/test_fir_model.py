"""A Python model of fir_tile_kernel's decomposition (csrc/mavg_fir.hpp) against the literal loop.
No GPU.

The model keeps what the kernel keeps: flat tiles of WG * R frames (R = U * F), the stage of
m = ceil((ntaps-1)/F) halo units and the tile's U * WG units laid out in U planes (stage unit s in
plane s % U at index s / U, FirLds::slot), the lane's walk over the m + U units that cover its R
output frames -- one unit per step, the sample of frame e of the unit of step t meeting output i
with the tap j = (m - t) * F + i - e, taps running from the largest j down inside a step, the
unguarded form of a step where every one of its taps is in range -- and the outputs' way back
through NO planes of 16-B units.  Tiny F, U and WG make every edge reachable with short signals.

The taps are fp32-valued, so acc + h * x in fp64 is the fma (tests/fir_ref.py): every comparison is
bitwise."""
import numpy as np
import pytest

from fir_ref import fir_chain


def literal(x, taps, C, history=None):
    """The contract, one output at a time: acc = +0.0, j = ntaps-1 .. 0, oldest frame first."""
    xs = np.asarray(x).reshape(-1, C)
    frames, ntaps = xs.shape[0], len(taps)
    hist = None if history is None else np.asarray(history).reshape(-1, C)
    y = np.empty((frames, C), dtype=np.float32)
    for f in range(frames):
        for c in range(C):
            acc = np.float64(0.0)
            for j in range(ntaps - 1, -1, -1):
                g = f - j
                if g >= 0:
                    v = xs[g, c]
                elif hist is not None:
                    v = hist[g + ntaps - 1, c]
                else:
                    v = 0
                acc = acc + np.float64(taps[j]) * np.float64(v)
            y[f, c] = np.float32(acc)
    return y.reshape(-1)


class Lds:
    """FirLds: the planes of the stage and of the outputs."""

    def __init__(self, m, F, C, U, WG):
        self.U, self.VE = U, F * C
        self.plane_units = (((m + U * WG + U - 1) // U + 7) & ~7) + (8 // U if U <= 8 else 0)
        self.out_units = U * F * C // 4 if F > 1 else 0
        self.out_plane = WG + 4

    def slot(self, s):
        return ((s % self.U) * self.plane_units + s // self.U) * self.VE


def load_elem(xs, hist, f, c, nframes, ntaps):
    if f >= 0:
        return xs[f, c] if f < nframes else xs.dtype.type(0)
    if hist is not None and f >= -(ntaps - 1):
        return hist[f + ntaps - 1, c]
    return xs.dtype.type(0)


def tile_model(x, taps, C, F, U, WG, history=None, counts=None):
    xs = np.asarray(x).reshape(-1, C)
    hist = None if history is None else np.asarray(history).reshape(-1, C)
    nframes, ntaps = xs.shape[0], len(taps)
    h = np.asarray(taps, dtype=np.float64)
    VE, R = F * C, U * F
    TF = WG * R
    m = (ntaps - 1 + F - 1) // F
    lds = Lds(m, F, C, U, WG)
    out = np.full(nframes * C, np.nan, dtype=np.float32)
    for tile in range((nframes + TF - 1) // TF):
        t0 = tile * TF
        h0 = t0 - m * F
        stage = np.full(lds.plane_units * U * VE, 7777, dtype=xs.dtype)   # what is never staged must not be read
        staged = np.zeros(stage.size, dtype=bool)
        for tid in range(WG):
            for u in range(U):
                s = m + u * WG + tid
                for fr in range(F):
                    for c in range(C):
                        stage[lds.slot(s) + fr * C + c] = load_elem(xs, hist, t0 + (u * WG + tid) * F + fr, c, nframes, ntaps)
                staged[lds.slot(s):lds.slot(s) + VE] = True
            for j in range(tid, m, WG):
                for fr in range(F):
                    for c in range(C):
                        stage[lds.slot(j) + fr * C + c] = load_elem(xs, hist, h0 + j * F + fr, c, nframes, ntaps)
                staged[lds.slot(j):lds.slot(j) + VE] = True
        ost = np.full(max(lds.out_units, 1) * lds.out_plane * 4, np.nan, dtype=np.float32)
        for tid in range(WG):
            acc = np.zeros((R, C), dtype=np.float64)
            for t in range(m + U):
                a = tid * VE + (t % U) * lds.plane_units * VE + (t // U) * VE     # the kernel's address form
                assert a == lds.slot(tid * U + t) and staged[a:a + VE].all()
                xe = stage[a:a + VE].astype(np.float64).reshape(F, C)
                jb = (m - t) * F
                guard = not (jb - (F - 1) >= 0 and jb + R - 1 < ntaps)
                if counts is not None:
                    counts["guarded" if guard else "steady"] += 1
                for d in range(R - 1, -F, -1):
                    j = jb + d
                    if guard and not (0 <= j < ntaps):
                        continue
                    assert 0 <= j < ntaps                                       # an unguarded step reads no tap outside
                    for e in range(F):
                        i = d + e
                        if 0 <= i < R:
                            acc[i] = acc[i] + h[j] * xe[e]
            y = acc.astype(np.float32).reshape(-1)                              # the lane's R * C floats
            if F > 1:
                for o in range(lds.out_units):
                    ost[(o * lds.out_plane + tid) * 4:(o * lds.out_plane + tid) * 4 + 4] = y[o * 4:o * 4 + 4]
            else:
                for i in range(R):
                    if t0 + tid * R + i < nframes:
                        out[(t0 + tid * R + i) * C:(t0 + tid * R + i + 1) * C] = y[i * C:(i + 1) * C]
        if F > 1:
            NO = lds.out_units
            for tid in range(WG):
                for i in range(NO):
                    v = i * WG + tid
                    unit = ost[((v % NO) * lds.out_plane + v // NO) * 4:((v % NO) * lds.out_plane + v // NO) * 4 + 4]
                    s = t0 * C + v * 4
                    for e in range(4):
                        if s + e < nframes * C:
                            out[s + e] = unit[e]
    assert not np.isnan(out).any()
    return out


def taps_f32(rng, n):
    return rng.standard_normal(n).astype(np.float32).astype(np.float64)


# (F, C, U): 16-B units of fp32 mono / stereo and int16 mono / stereo shapes, and the frame-unit form
SHAPES = [(4, 1, 4), (2, 2, 4), (8, 1, 2), (4, 2, 2), (1, 1, 8), (1, 2, 8), (2, 2, 2)]


@pytest.mark.parametrize("F,C,U", SHAPES)
@pytest.mark.parametrize("kind", ["f32", "i16"])
def test_tile_model_is_the_chain(F, C, U, kind):
    rng = np.random.default_rng(F * 100 + C * 10 + U)
    WG, R = 4, U * F
    TF = WG * R
    frames = 3 * TF + 5
    if kind == "f32":
        x = rng.standard_normal(frames * C).astype(np.float32)
    else:
        x = rng.integers(-32768, 32768, frames * C).astype(np.int16)
    counts = {"guarded": 0, "steady": 0}
    for ntaps in sorted({1, 2, F, F + 1, R * F - 1, R * F + 1, R - 1, R, R + 1, R + F, TF - 1, TF, TF + 1, 2 * TF + 3, frames + 2}):
        if ntaps < 1:
            continue
        h = taps_f32(rng, ntaps)
        ref = fir_chain(x, h, C)
        got = tile_model(x, h, C, F, U, WG, counts=counts)
        assert np.array_equal(got, ref), (ntaps, np.flatnonzero(got != ref)[:8])
        hist = (rng.standard_normal((ntaps - 1) * C).astype(np.float32) if kind == "f32"
                else rng.integers(-32768, 32768, (ntaps - 1) * C).astype(np.int16))
        assert np.array_equal(tile_model(x, h, C, F, U, WG, history=hist), fir_chain(x, h, C, hist)), ntaps
    assert counts["guarded"] > 0 and counts["steady"] > 0           # both forms of a step ran


def test_chain_reference_is_the_literal_loop():
    rng = np.random.default_rng(7)
    for C in (1, 2, 3):
        x = rng.standard_normal(50 * C).astype(np.float32)
        for ntaps in (1, 2, 5, 49, 50, 51, 80):
            h = taps_f32(rng, ntaps)
            hist = rng.standard_normal((ntaps - 1) * C).astype(np.float32)
            assert np.array_equal(fir_chain(x, h, C), literal(x, h, C))
            assert np.array_equal(fir_chain(x, h, C, hist), literal(x, h, C, hist))


def test_a_wrong_tap_order_shows():
    """Asymmetric taps on a unit impulse: the output is the taps, in order, from the impulse on."""
    F, C, U, WG = 2, 1, 2, 4
    TF = WG * U * F
    h = np.arange(1, 8, dtype=np.float64)                            # 1 .. 7: h[0] on the newest frame
    x = np.zeros(3 * TF, dtype=np.float32)
    at = TF - 3                                                      # the response crosses a tile boundary
    x[at] = 2.0
    y = tile_model(x, h, C, F, U, WG)
    want = np.zeros_like(x)
    want[at:at + 7] = 2.0 * h
    assert np.array_equal(y, want)
    assert not np.array_equal(tile_model(x, h[::-1].copy(), C, F, U, WG), want)


def test_the_planes_hold_every_unit_once():
    for F, C, U in SHAPES:
        for m in (0, 1, 7, 8, 9, 100):
            lds = Lds(m, F, C, U, 16)
            slots = [lds.slot(s) for s in range(m + U * 16)]
            assert len(set(slots)) == len(slots) and max(slots) + F * C <= lds.plane_units * U * F * C


def test_the_model_s_geometry_is_the_library_s():
    """What ties the model to the kernel it restates: for every instance the library's plan gives
    the model's F, U, R, tile frames, halo units and LDS bytes (FirLds), at tap counts on both sides
    of a unit and at the rule's boundary.  (The arithmetic itself is tied on the GPU:
    tests/test_gpu_fir.py compares the kernels with the same fir_chain bit for bit.)"""
    import digital_signal_processsing_amd as dsp
    WG = 256
    for dt, eb in ((dsp.F32, 4), (dsp.I16, 2)):
        for C in (1, 2):
            lim = 16384 // (C * eb) + 1
            for aligned, (F, U) in ((True, (16 // (C * eb), 4 if eb == 4 else 2)), (False, (1, 8))):
                for ntaps in (1, 2, F, F + 1, F + 2, 100, lim):
                    plan = dsp.fir_plan(C << 22, ntaps, C, dt, aligned=aligned)
                    m = (ntaps - 1 + F - 1) // F
                    lds = Lds(m, F, C, U, WG)
                    stage = (lds.plane_units * U * F * C * eb + 15) & ~15
                    assert plan.startswith(f"fir_tile<{'f32' if eb == 4 else 'i16'},C={C},F={F},U={U},R={U * F}> taps={ntaps} "), plan
                    assert f" halo_units={m} " in plan and f" tile_frames={WG * U * F} " in plan, plan
                    assert f" lds={max(stage, lds.out_units * lds.out_plane * 16)} " in plan, plan
