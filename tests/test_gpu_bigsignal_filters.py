"""Parity past 2^32 samples for the filters with kernels of their own: moving extrema, EMA,
biquad, the second-order-sections cascade and FIR.  One signal of 2^32 + ~10^6 samples (tests/test_gpu_bigsignal.py's sizes, views,
guard bands and checksum) per dispatch path and unit form.  Each case checks, in this order,
  1. the plan text (a dispatch change cannot pass under an old id);
  2. the input, the history and a state passed in: unchanged;
  3. guard bands around every output view (an extrema output that is not passed is still
     allocated and must still hold the sentinel);
  4. three host windows (head, around input sample 2^32, tail) through the small suites' own
     references and bars on input the oracle regenerates: extrema_ref, fir_ref.fir_chain, ema_ref +
     ema_bar, biquad_ref.biquad_loop + biquad_bar (the last two read with W frames of lead from a
     zero state, tests/bigsignal_ref.py's ema_lead / biquad_lead);
  5. every output through the chunked device references of tests/bigsignal_ref.py, pinned on the
     CPU by tests/test_bigsignal_ref.py: extrema and FIR bit for bit, EMA and biquad against the
     bars of include/mavg.h, the largest err / bar printed;
  6. d_state_out, where the case asks for it, against the tail window's reference state.
The cascade (mavg_sos_run) runs the same six through sos_ref.sos_ref, chunked_sos_mismatches and the
header's two bars formed from the level M (sos_abs_bar_at, sos_state_bar_at; a streamed case's from
the state actually passed in): sos_tile in both unit forms (element loads on the input side, the
frame-unit stores on the output side), with a carried state, behind the full 16-KiB stage with a
state_out, and sos_loop through one fp32 buffer of the signal's size and through two.
int16 and every FIR case use generator dist 0 (FIR: taps m / 1024, so that every fp64 sum is exact
and the contract's chain is bit for bit fl32 of it); fp32 extrema, EMA and biquad dist 2, the
rounding-stress data.  M is the device maximum of |x|.

The `_streamed` cases are the header's streaming promise: a prefix of 2^16 frames of the
stream is filtered with a state_out, the remainder with that state as state_in, and the reference
is the one-shot filter of the whole stream from a zero state, compared from frame 2^16 on.

Memory: the module docstring of tests/test_gpu_bigsignal.py."""
import pytest

from test_gpu_bigsignal import (CHUNK, GUARD, SENT, STAT_CHUNK, WIN, _bits, _check_plan, _checksum, _dt, _guarded,
                                _guards_intact, _host_slice, _need, _out_windows, _same_bits, _sizes, _stream)

pytestmark = pytest.mark.gpu

PREFIX = 1 << 16              # frames the streamed cases filter first
LOOP_WIN = 1 << 15            # frames per host window where the reference is a Python loop or has 4097 taps


def _absmax(x):
    """max |x| on the device, 2^28 samples at a time, without a temporary (int16: abs(-32768) does not fit)."""
    import torch
    m = 0.0
    for a in range(0, x.numel(), 1 << 28):
        lo, hi = torch.aminmax(x[a:a + (1 << 28)])
        m = max(m, -float(lo), float(hi))
    return m


def _history_split(xs, lead, want, C):
    """A host slice as (history, signal, frames to drop): the history when the slice holds all
    `want` frames of it, else the slice starts at frame 0 of the stream and has none."""
    if want and lead == want:
        return xs[:lead * C], xs[lead * C:], 0
    return None, xs, lead


def _index_in_y(got, hs):
    return (got[0], got[1] - hs) if got[1] is not None else got


# ---- extrema ----
def _run_extrema(oracle_mod, gpu, dt, C, k, want, with_max=True, with_min=True, out_off=0, history=False, tamper=None):
    import torch
    import digital_signal_processsing_amd as dsp
    import extrema_ref
    from bigsignal_ref import chunked_extrema_mismatches
    dtype, code, esz = _dt(dt)
    dist = 2 if dt == "f32" else 0
    F, n = _sizes(C)
    plan = dsp.extrema_plan(n, k, C, code, with_max, with_min, aligned=not out_off)
    tag = f"extrema {dt} C={C} k={k} max={with_max} min={with_min} n={n} out+{out_off} history={history}: {plan}"
    print(tag)
    _check_plan(plan, want, tag)
    hf = k - 1 if history else 0
    assert (hf * C * esz) % 16 == 0
    _need(gpu, 3 * (n + hf * C + 2 * GUARD + 8) * esz + (5 << 30))
    xall, x, hist = _stream(gpu, dtype, n, hf * C, 0, dist)
    hibuf, hiall = _guarded(gpu, dtype, n, hf * C, out_off)       # both allocated; one may not be passed
    lobuf, loall = _guarded(gpu, dtype, n, hf * C, out_off)
    hi, lo = (hiall[hf * C:] if with_max else None), (loall[hf * C:] if with_min else None)
    before = _checksum(xall)

    dsp.moving_extrema_into(x, hi, lo, k, C, history=hist)
    torch.cuda.synchronize()

    try:
        assert _checksum(xall) == before, tag
        for name, given, buf, yall in (("d_max", with_max, hibuf, hiall), ("d_min", with_min, lobuf, loall)):
            if given:
                _guards_intact(buf, yall, hf * C, name, tag)
            else:
                assert bool((_bits(buf) == SENT[esz]).all()), f"{name}'s buffer written though not passed: {tag}"
        for fa, fb in _out_windows(F, 2 ** 32 // C, WIN // C):
            xs, lead = _host_slice(oracle_mod, dt, C, hf + fa, hf + fb, k - 1, dist)
            hx, sx, drop = _history_split(xs, lead, k - 1, C)
            refs = extrema_ref.moving_extrema_ref(sx, k, C, hx)
            for name, y, ref in (("max", hi, refs[0]), ("min", lo, refs[1])):
                if y is not None:
                    ok = _same_bits(y[fa * C:fb * C].cpu().numpy(), ref[drop * C:])
                    print(f"  host frames [{fa}, {fb}) {name}: {'equal' if ok else 'DIFFERENT'}")
                    assert ok, f"[{fa}, {fb}) {name}: {tag}"
        expect = tamper(hi, lo, n) if tamper else (0, None)
        got = chunked_extrema_mismatches(xall, hiall if with_max else None, loall if with_min else None, k, C,
                                         CHUNK // C, first_frame=hf)
        got = _index_in_y(got, hf * C)
        assert got == expect, f"(mismatches, first bad sample) = {got}: {tag}"
    finally:
        del x, hist, xall, hi, lo, hiall, loall, hibuf, lobuf
        torch.cuda.empty_cache()


# ---- FIR ----
def _fir_taps(ntaps):
    from bigsignal_ref import dyadic_taps
    return dyadic_taps(ntaps, ntaps, sparse=ntaps > 64)


def _run_fir(oracle_mod, gpu, dt, C, ntaps, want, in_off=0, history=False, tamper=None):
    import numpy as np
    import torch
    import digital_signal_processsing_amd as dsp
    import fir_ref
    from bigsignal_ref import chunked_fir_mismatches
    dtype, code, esz = _dt(dt)
    F, n = _sizes(C)
    taps = _fir_taps(ntaps)
    assert taps[0] != 0 and taps[-1] != 0 and np.count_nonzero(taps) == (ntaps if ntaps <= 64 else 16)
    plan = dsp.fir_plan(n, ntaps, C, code, history=history, aligned=not in_off)
    tag = f"fir {dt} C={C} taps={ntaps} n={n} in+{in_off} history={history}: {plan}"
    print(tag)
    _check_plan(plan, want, tag)
    hf = ntaps - 1 if history else 0
    assert (hf * C * esz) % 16 == 0
    _need(gpu, (n + hf * C) * esz + (n + hf * C + 2 * GUARD + 4) * 4 + (5 << 30))
    h = dsp.fir_taps(taps, gpu)
    xall, x, hist = _stream(gpu, dtype, n, hf * C, in_off, 0)
    ybuf, yall = _guarded(gpu, torch.float32, n, hf * C, 0)
    y = yall[hf * C:]
    before, taps_before = _checksum(xall), h.clone()

    dsp.fir_filter_into(x, y, h, C, history=hist)
    torch.cuda.synchronize()

    try:
        assert _checksum(xall) == before and torch.equal(h, taps_before), tag
        _guards_intact(ybuf, yall, hf * C, "d_out", tag)
        for fa, fb in _out_windows(F, 2 ** 32 // C, (WIN if ntaps <= 64 else LOOP_WIN) // C):
            xs, lead = _host_slice(oracle_mod, dt, C, hf + fa, hf + fb, ntaps - 1, 0)
            hx, sx, drop = _history_split(xs, lead, ntaps - 1, C)
            ok = _same_bits(y[fa * C:fb * C].cpu().numpy(), fir_ref.fir_chain(sx, taps, C, hx)[drop * C:])
            print(f"  host frames [{fa}, {fb}): {'equal' if ok else 'DIFFERENT'}")
            assert ok, f"[{fa}, {fb}): {tag}"
        expect = tamper(y, n) if tamper else (0, None)
        got = _index_in_y(chunked_fir_mismatches(xall, yall, taps, C, CHUNK // C, first_frame=hf), hf * C)
        assert got == expect, f"(mismatches, first bad sample) = {got}: {tag}"
    finally:
        del x, hist, xall, y, yall, ybuf, h
        torch.cuda.empty_cache()


# ---- EMA and biquad: one runner, the filter as a small table of functions ----
class _Ema:
    name = "ema"

    def __init__(self, alpha):
        import ema_ref
        from bigsignal_ref import ema_lead
        self.alpha, self.ref, self.W, self.G = alpha, ema_ref, ema_lead(alpha), 1.0
        self.what = f"alpha={alpha}"

    def plan(self, dsp, n, C, code, state, ret, aligned):
        return dsp.ema_plan(n, self.alpha, C, code, state, ret, aligned=aligned)

    def workspace(self, dsp, n, C, code):
        return dsp.ema_workspace_bytes(n, self.alpha, C, code)

    def state(self, torch, C, gpu, fill):
        return torch.full((C,), fill, dtype=torch.float64, device=gpu)

    def run(self, dsp, x, y, C, **kw):
        dsp.exponential_moving_average_into(x, y, self.alpha, channels=C, **kw)

    def host(self, xs, C):
        """(fp64 outputs, the state after the last frame) from a zero state"""
        y = self.ref.ema_ref(xs, self.alpha, C)
        return y, y.reshape(-1, C)[-1].copy()

    def bar(self, ref, M):
        return self.ref.ema_bar(ref, M)

    def state_bar(self, plan, M):
        return 2.0 ** -29 * M if plan.startswith("ema_tile<") else 1e-12 * M

    def chunked(self, xall, yall, C, M, first_frame, stats):
        from bigsignal_ref import chunked_ema_mismatches
        return chunked_ema_mismatches(xall, yall, self.alpha, C, M, STAT_CHUNK // C, first_frame, stats)


class _Biquad:
    name = "biquad"

    def __init__(self, kind, f, Q):
        import biquad_ref
        from bigsignal_ref import biquad_lead
        self.coef, self.ref = biquad_ref.rbj(kind, f, Q), biquad_ref
        self.W, self.G = biquad_lead(self.coef), biquad_ref.biquad_gain(self.coef)
        self.what = f"RBJ {kind} f={f} Q={Q} G={self.G:.4f} D={biquad_ref.domain_d(self.coef):.2e}"
        assert biquad_ref.domain_d(self.coef) >= 2.0 ** -22          # inside the promised domain

    def plan(self, dsp, n, C, code, state, ret, aligned):
        return dsp.biquad_plan(n, self.coef, C, code, state, ret, aligned=aligned)

    def workspace(self, dsp, n, C, code):
        return dsp.biquad_workspace_bytes(n, self.coef, C, code)

    def state(self, torch, C, gpu, fill):
        return torch.full((C, 2), fill, dtype=torch.float64, device=gpu)

    def run(self, dsp, x, y, C, **kw):
        dsp.biquad_into(x, y, self.coef, channels=C, **kw)

    def host(self, xs, C):
        return self.ref.biquad_loop(xs, self.coef, C)

    def bar(self, ref, M):
        return self.ref.biquad_bar(ref, self.G, M)

    def state_bar(self, plan, M):
        return 2.0 ** -29 * self.G * M

    def chunked(self, xall, yall, C, M, first_frame, stats):
        from bigsignal_ref import chunked_biquad_mismatches
        return chunked_biquad_mismatches(xall, yall, self.coef, C, self.G, M, STAT_CHUNK // C, first_frame, stats)


class _Sos:
    """The cascade: a named section set of bigsignal_ref.big_sos.  intermediate="fp64" is the
    header's MAVG_SOS_FP64_ONLY (the tile or a refusal); loop: the case runs sos_loop and is held to
    its bar.  The state has shape [S, C, 2], its bar is per section, and a state passed in enters
    both bars through the levels m_j (state_in(), called with the host copy of a streamed case's)."""
    name = "sos"

    def __init__(self, set_name, intermediate="auto", loop=False):
        import biquad_ref
        import sos_ref
        import digital_signal_processsing_amd as dsp
        from bigsignal_ref import big_sos, sos_lead
        self.rows, self.ref = big_sos(set_name, dsp.biquad_halo_frames), sos_ref
        self.sos6, self.S = sos_ref.rows6(self.rows), len(self.rows)
        self.intermediate, self.loop, self.sin = intermediate, loop, None
        self.W = sos_lead(self.rows)
        D = min(biquad_ref.domain_d(c) for c in self.rows)
        self.what = (f"{set_name} sections={self.S} intermediate={intermediate} "
                     f"G={[round(g, 3) for g in sos_ref.sos_gains(self.rows)]} D>={D:.2e}")
        assert D >= 2.0 ** -22                                       # every row inside the promised domain

    def plan(self, dsp, n, C, code, state, ret, aligned):
        return dsp.sos_plan(n, self.sos6, C, code, state, ret, self.intermediate, aligned=aligned)

    def workspace(self, dsp, n, C, code):
        return dsp.sos_workspace_bytes(n, self.sos6, C, code, self.intermediate)

    def check_workspace(self, ws_n, plan, n, tag):
        """sos_tile: the sections' tables, exactly; sos_loop: one fp32 buffer of the signal's size (two
        with three or more sections), each padded to 16 B, and the sections' own workspace."""
        assert f" ws={ws_n} " in plan, tag
        if plan.startswith("sos_tile<"):
            assert not self.loop and ws_n == (self.S * 2712 + 15) // 16 * 16, tag
        else:
            nbuf = 2 if self.S > 2 else 1
            assert self.loop and f" buffers={nbuf} " in plan and ws_n >= nbuf * ((4 * n + 15) // 16 * 16), tag

    def state(self, torch, C, gpu, fill):
        return torch.full((self.S, C, 2), fill, dtype=torch.float64, device=gpu)

    def state_in(self, host_state):
        self.sin = host_state.copy()

    def run(self, dsp, x, y, C, **kw):
        dsp.sosfilt_into(x, y, self.sos6, channels=C, intermediate=self.intermediate, **kw)

    def host(self, xs, C):
        return self.ref.sos_ref(xs, self.rows, C)

    def bar(self, ref, M):
        import numpy as np
        return 2.0 ** -23 * np.abs(ref) + self.ref.sos_abs_bar_at(self.rows, M, self.sin, self.loop)

    def state_bar(self, plan, M):
        return self.ref.sos_state_bar_at(self.rows, M, self.sin, self.loop).reshape(self.S, 1, 1)

    def chunked(self, xall, yall, C, M, first_frame, stats):
        """(from frame 0 on -- a streamed case's prefix -- the state is zero and stays out of the bar)"""
        from bigsignal_ref import chunked_sos_mismatches
        abs_term = self.ref.sos_abs_bar_at(self.rows, M, self.sin if first_frame else None, self.loop)
        return chunked_sos_mismatches(xall, yall, self.rows, C, abs_term, STAT_CHUNK // C, first_frame, stats)


def _run_recursive(oracle_mod, gpu, filt, dt, C, want, in_off=0, out_off=0, streamed=False, state_out=False, tamper=None):
    import numpy as np
    import torch
    import digital_signal_processsing_amd as dsp
    dtype, code, esz = _dt(dt)
    dist = 2 if dt == "f32" else 0
    F, n = _sizes(C)
    ret = streamed or state_out
    plan = filt.plan(dsp, n, C, code, streamed, ret, not (in_off or out_off))
    tag = (f"{filt.name} {dt} C={C} {filt.what} W={filt.W} n={n} in+{in_off} out+{out_off} streamed={streamed} "
           f"state_out={ret}: {plan}")
    print(tag)
    _check_plan(plan, want, tag)
    hf = PREFIX if streamed else 0
    ws_n = filt.workspace(dsp, n, C, code)
    if hasattr(filt, "check_workspace"):      # a filter with a workspace on its tile too says what it expects
        filt.check_workspace(ws_n, plan, n, tag)
    else:
        assert (ws_n > 0) == (not plan.startswith(f"{filt.name}_tile<")), tag
    _need(gpu, (n + hf * C) * esz + (n + 2 * hf * C + 2 * GUARD + 4) * 4 + ws_n + (5 << 30))
    ws = torch.empty(ws_n, dtype=torch.uint8, device=gpu) if ws_n else None
    xall, x, pre = _stream(gpu, dtype, n, hf * C, in_off, dist)
    ybuf, yall = _guarded(gpu, torch.float32, n, hf * C, out_off)
    y = yall[hf * C:]
    before = _checksum(xall)
    M = _absmax(xall)
    assert M > 0.0
    sin = sin_before = ypre = None
    if streamed:              # the prefix first: its state_out is the remainder's state_in
        pplan = filt.plan(dsp, hf * C, C, code, False, True, True)
        print(f"  prefix of {hf} frames: {pplan}")
        assert pplan.startswith(f"{filt.name}_tile<"), pplan
        ypre = torch.empty(hf * C, dtype=torch.float32, device=gpu)
        sin = filt.state(torch, C, gpu, float("nan"))
        filt.run(dsp, pre, ypre, C, state_out=sin)
        torch.cuda.synchronize()
        sin_before = sin.clone()
        assert bool(torch.isfinite(sin).all()), tag
        if hasattr(filt, "state_in"):         # a bar that depends on the state: formed from the actual one
            filt.state_in(sin.cpu().numpy())
    sout = filt.state(torch, C, gpu, float("nan")) if ret else None

    filt.run(dsp, x, y, C, state=sin, state_out=sout, workspace=ws)
    torch.cuda.synchronize()

    try:
        assert _checksum(xall) == before, tag
        if streamed:
            assert torch.equal(sin, sin_before), f"state_in changed: {tag}"
        _guards_intact(ybuf, yall, hf * C, "d_out", tag)
        wf = (WIN if filt.name == "ema" else LOOP_WIN) // C
        tail_state = None
        for fa, fb in _out_windows(F, 2 ** 32 // C, wf):
            xs, lead = _host_slice(oracle_mod, dt, C, hf + fa, hf + fb, filt.W, dist)
            ref, tail_state = filt.host(xs, C)
            ref = ref[lead * C:]
            err = np.abs(y[fa * C:fb * C].cpu().numpy().astype(np.float64) - ref)
            ratio = err / filt.bar(ref, M)
            print(f"  host frames [{fa}, {fb}): err / bar <= {float(ratio.max()):.3f}")
            assert not (ratio > 1.0).any() and np.isfinite(ratio).all(), f"[{fa}, {fb}): {tag}"
        stats = {}
        if streamed:          # the prefix itself, from frame 0
            assert filt.chunked(xall[:hf * C], ypre, C, M, 0, stats) == (0, None), f"the prefix: {tag}"
        expect = tamper(y, n) if tamper else (0, None)
        got = _index_in_y(filt.chunked(xall, yall, C, M, hf, stats), hf * C)
        print(f"  every output: (mismatches, first bad sample) = {got}, largest err / bar {stats['worst']:.3f}")
        assert got == expect, f"(mismatches, first bad sample) = {got}: {tag}"
        if ret:
            dev = np.abs(sout.cpu().numpy().reshape(np.shape(tail_state)) - tail_state)
            sbar = filt.state_bar(plan, M)
            print(f"  d_state_out: off by {float(dev.max()):.3e}, the bar {float(np.max(sbar)):.3e}")
            assert (dev <= sbar).all(), f"d_state_out {sout.cpu().numpy()} against {tail_state}: {tag}"
    finally:
        del x, pre, xall, y, yall, ybuf, ws, ypre, sin, sout
        torch.cuda.empty_cache()


# id, dtype, C, k, plan, keyword arguments
EXTREMA_CASES = [
    # both outputs behind the full 16-KiB halo
    ("extrema_tile_i16_c1_k8193", "i16", 1, 8193, ("extrema_tile<i16,C=1,F=8,U=2,M=3", " halo_frames=8192 ", " tile_frames=4096 "), {}),
    # more than 2^21 tiles through the XCD remap; three fp32 buffers
    ("extrema_tile_f32_c2_k2049", "f32", 2, 2049, ("extrema_tile<f32,C=2,F=2,U=2,M=3", " grid=2098129 ", " tile_frames=1024 "), {}),
    ("extrema_tile_f32_c1_k64_max_only", "f32", 1, 64, ("extrema_tile<f32,C=1,F=4,U=4,M=1", " max=1 min=0 "), {"with_min": False}),
    # the output view one sample off 16-B alignment: the frame-unit form, four times the grid
    ("extrema_tile_i16_c2_k100_min_only_frame_unit", "i16", 2, 100, ("extrema_tile<i16,C=2,F=1,", " max=0 min=1 "),
     {"with_max": False, "out_off": 1}),
    ("extrema_tile_i16_c2_k705_history", "i16", 2, 705, ("extrema_tile<i16,C=2,F=4,U=2,M=3", " halo_frames=704 "), {"history": True}),
    ("extrema_strip_i16_c3_k100", "i16", 3, 100, ("extrema_strip dtype=i16 C=3", " L=25 "), {}),
    ("extrema_strip_f32_c1_k44100", "f32", 1, 44100, ("extrema_strip dtype=f32 C=1", " L=2048 "), {}),
]
# id, dtype, C, alpha, plan, keyword arguments
EMA_CASES = [
    ("ema_tile_f32_c1_a0.05_streamed", "f32", 1, 0.05, ("ema_tile<f32,C=1,F=4,U=2", " halo_frames=406 ", " state=3 "), {"streamed": True}),
    ("ema_tile_i16_c2_a0.01", "i16", 2, 0.01, ("ema_tile<i16,C=2,F=4,U=4", " halo_frames=2070 ", " tile_frames=4096 "), {}),
    # 16 268 B of halo: fp32 mono's last alpha on the tile
    ("ema_tile_f32_c1_a0.0051", "f32", 1, 0.0051, ("ema_tile<f32,C=1,F=4,U=2", " halo_frames=4067 "), {}),
    ("ema_tile_i16_c1_a0.05_frame_unit", "i16", 1, 0.05, ("ema_tile<i16,C=1,F=1,", " tile_frames=1024 "), {"out_off": 1}),
    # the carry kernel walks 2 097 641 records
    ("ema_chain_f32_c1_a1e-4", "f32", 1, 1e-4, ("ema_chain<f32,C=1,F=4,U=2", " state=2 ", " records=2097641 ", " launches=3"),
     {"state_out": True}),
    # the first alpha past the tile's range
    ("ema_chain_i16_c2_a0.0026", "i16", 2, 0.0026, ("ema_chain<i16,C=2,F=4,U=4", " records=524533 "), {}),
    ("ema_strip_f32_c3_a0.05", "f32", 3, 0.05, ("ema_strip dtype=f32 C=3 L=64 strips=22385247 ",), {}),
]
# id, dtype, C, (kind, f, Q), plan, keyword arguments
BIQUAD_CASES = [
    ("biquad_tile_f32_c1_LP0.1_streamed", "f32", 1, ("LP", 0.1, 0.707), ("biquad_tile<f32,C=1,F=4,U=2", " halo_frames=49 ", " state=3 "),
     {"streamed": True}),
    ("biquad_tile_i16_c2_LP0.002", "i16", 2, ("LP", 0.002, 0.707), ("biquad_tile<i16,C=2,F=4,U=4", " halo_frames=2378 "), {}),
    ("biquad_tile_f32_c1_BP0.01_Q4_frame_unit", "f32", 1, ("BP", 0.01, 4.0),
     ("biquad_tile<f32,C=1,F=1,", " halo_frames=3302 ", " tile_frames=1024 "), {"in_off": 1}),
    ("biquad_chain_f32_c1_HP0.0005", "f32", 1, ("HP", 0.0005, 0.7071),
     ("biquad_chain<f32,C=1,F=4,U=2", " state=2 ", " records=2097641 ", " carry_chunk=2048 "), {"state_out": True}),
    ("biquad_strip_f32_c3_LP0.1", "f32", 3, ("LP", 0.1, 0.707), ("biquad_strip dtype=f32 C=3 L=64 ",), {}),
]
# id, dtype, C, (section set, intermediate, held to the loop's bar), plan, keyword arguments
SOS_CASES = [
    # the header's streaming promise: the prefix's state_out carried in, a state_out again
    ("sos_tile_f32_c1_butter4_streamed", "f32", 1, ("butter4", "auto", False),
     ("sos_tile<f32,C=1,F=4>", " sections=2 ", " state=3 ", " launches=3"), {"streamed": True}),
    # the full 16-KiB stage, the largest lds, a state_out from the last of 2 097 641 tiles
    ("sos_tile_i16_c2_limit8", "i16", 2, ("limit8", "auto", False),
     ("sos_tile<i16,C=2,F=4>", " halo_frames=1024 ", " sections=8 ", " lds=49280 ", " state=2 "), {"state_out": True}),
    # an odd sample offset on stereo: the frame-unit form with element loads for the whole signal
    ("sos_tile_f32_c2_three_frame_unit_eio", "f32", 2, ("three", "auto", False), ("sos_tile<f32,C=2,F=1>", " sections=3 "), {"in_off": 1}),
    # the frame-unit output stores; the rule's exception run on the tile by MAVG_SOS_FP64_ONLY
    ("sos_tile_i16_c1_hp_pk_frame_unit_out", "i16", 1, ("hp_pk", "fp64", False),
     ("sos_tile<i16,C=1,F=1>", " sections=2 ", " halo_frames=661 "), {"out_off": 1}),
    # the measured exception by the rule: int16 into fp32 through one buffer of more than 2^34 B
    ("sos_loop_i16_c1_hp_pk_rule", "i16", 1, ("hp_pk", "auto", True),
     ("sos_loop dtype=i16 C=1 sections=2", " halo_frames=661 ", " buffers=1 "), {}),
    # both ping-pong buffers, the sections' own workspace behind 2 * buf
    ("sos_loop_i16_c2_past9", "i16", 2, ("past9", "auto", True),
     ("sos_loop dtype=i16 C=2 sections=9", " halo_frames=1025 ", " buffers=2 "), {"state_out": True}),
]
# id, dtype, C, taps, plan, keyword arguments
FIR_CASES = [
    ("fir_tile_f32_c1_t33", "f32", 1, 33, ("fir_tile<f32,C=1,F=4,U=4,R=16>", " tile_frames=4096 "), {}),
    # 16 taps kept of 4097, the oldest among them: 16 384 B of halo
    ("fir_tile_i16_c2_t4097_sparse", "i16", 2, 4097, ("fir_tile<i16,C=2,F=4,U=2,R=8>", " halo_frames=4096 "), {}),
    ("fir_tile_f32_c1_t4097_sparse", "f32", 1, 4097, ("fir_tile<f32,C=1,F=4,U=4,R=16>", " halo_frames=4096 ", " lds=32896 "), {}),
    ("fir_tile_f32_c1_t33_frame_unit", "f32", 1, 33, ("fir_tile<f32,C=1,F=1,U=8,R=8>",), {"in_off": 1}),
    ("fir_tile_i16_c2_t33_history", "i16", 2, 33, ("fir_tile<i16,C=2,F=4,U=2,R=8>", " history=1 "), {"history": True}),
    ("fir_strip_f32_c3_t33", "f32", 3, 33, ("fir_strip dtype=f32 C=3 taps=33 L=64 ",), {}),
]


@pytest.mark.parametrize("name,dt,C,k,want,kw", EXTREMA_CASES, ids=[c[0] for c in EXTREMA_CASES])
def test_every_extremum_past_2p32_samples(oracle_mod, gpu, name, dt, C, k, want, kw):
    _run_extrema(oracle_mod, gpu, dt, C, k, want, **kw)


@pytest.mark.parametrize("name,dt,C,alpha,want,kw", EMA_CASES, ids=[c[0] for c in EMA_CASES])
def test_every_ema_output_past_2p32_samples(oracle_mod, gpu, name, dt, C, alpha, want, kw):
    _run_recursive(oracle_mod, gpu, _Ema(alpha), dt, C, want, **kw)


@pytest.mark.parametrize("name,dt,C,rbj,want,kw", BIQUAD_CASES, ids=[c[0] for c in BIQUAD_CASES])
def test_every_biquad_output_past_2p32_samples(oracle_mod, gpu, name, dt, C, rbj, want, kw):
    _run_recursive(oracle_mod, gpu, _Biquad(*rbj), dt, C, want, **kw)


@pytest.mark.parametrize("name,dt,C,sos,want,kw", SOS_CASES, ids=[c[0] for c in SOS_CASES])
def test_every_sos_output_past_2p32_samples(oracle_mod, gpu, name, dt, C, sos, want, kw):
    _run_recursive(oracle_mod, gpu, _Sos(*sos), dt, C, want, **kw)


@pytest.mark.parametrize("name,dt,C,ntaps,want,kw", FIR_CASES, ids=[c[0] for c in FIR_CASES])
def test_every_fir_output_past_2p32_samples(oracle_mod, gpu, name, dt, C, ntaps, want, kw):
    _run_fir(oracle_mod, gpu, dt, C, ntaps, want, **kw)


def _flip_two(bit):
    def tamper(y, n):
        for i in (2 ** 32 + 5, n - 1):
            _bits(y)[i:i + 1] ^= 1 << bit
        return (2, 2 ** 32 + 5)
    return tamper


def test_extrema_reference_sees_past_2p32(oracle_mod, gpu):
    """Sensitivity: one flipped bit of the maximum at sample 2^32 + 5 and one of the minimum at
    n - 1 of a correct output are both counted, the first one located."""
    def tamper(hi, lo, n):
        _bits(hi)[2 ** 32 + 5:2 ** 32 + 6] ^= 1
        _bits(lo)[n - 1:n] ^= 1
        return (2, 2 ** 32 + 5)
    _run_extrema(oracle_mod, gpu, "i16", 1, 64, "extrema_tile<i16,C=1,F=8,", tamper=tamper)


def test_fir_reference_sees_past_2p32(oracle_mod, gpu):
    _run_fir(oracle_mod, gpu, "i16", 2, 33, "fir_tile<i16,C=2,F=4,U=2,R=8>", tamper=_flip_two(0))


def test_ema_reference_sees_past_2p32(oracle_mod, gpu):
    """Bit 20 of the fp32 pattern (an eighth of the value: one ulp is inside the bar)."""
    _run_recursive(oracle_mod, gpu, _Ema(0.05), "i16", 1, "ema_tile<i16,C=1,F=8,", tamper=_flip_two(20))


def test_biquad_reference_sees_past_2p32(oracle_mod, gpu):
    _run_recursive(oracle_mod, gpu, _Biquad("LP", 0.1, 0.707), "i16", 1, "biquad_tile<i16,C=1,F=8,", tamper=_flip_two(20))


def test_sos_reference_sees_past_2p32(oracle_mod, gpu):
    _run_recursive(oracle_mod, gpu, _Sos("butter4", "fp64"), "i16", 1, ("sos_tile<i16,C=1,F=8>", " sections=2 "), tamper=_flip_two(20))
