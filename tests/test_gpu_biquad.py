"""GPU tests of the biquad (mavg_biquad_run): the one-launch tile kernel (biquad_tile,
csrc/mavg_biquad.hpp), the three-launch chain (biquad_chain) and the strip form (biquad_strip), by
the rule and forced through the hooks build, in both unit forms, against the fp64 transposed-direct-
form-II recurrence of tests/biquad_ref.py and the accuracy bar of include/mavg.h:

    |y - y_ref| <= 2^-23 |y_ref| + 2^-29 G M,    G = sum |h[n]|,  M = max(|x|, |state_in|)

d_state_out: within 2^-29 G M of the reference state, per component, on every path.

Signals are three tiles plus 17 frames, tile_frames read from the plan text; inputs are uniform on
[0, 1) (oracle.synth_f32 dist 1: the DC component keeps the states large, so a wrong power of A
shows) or int16 (oracle.synth_i16).  A state_in is one the filter produces -- what the reference
reaches after a warm-up signal, of the signal's amplitude or 100 x it: include/mavg.h "Which states"
promises both bars for those.  A state no input produces answers with the poles alone, up to 1 /
theta above M; for it the header promises the outputs' bar only, and
test_tile_with_a_state_no_input_produces holds the tile kernel to that.  Outputs are written into
views inside guard regions, which must come back untouched."""
import math
import os

import numpy as np
import pytest

from biquad_ref import (COPY, FIR3, REAL_POLE_CASES, biquad_bar, biquad_gain, biquad_ref, biquad_scale, domain_d,
                        f_at_domain_edge, rbj, state_horizon)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "digital_signal_processsing_amd", "lib")
HOOKS_LIB = os.path.join(LIBDIR, "libmavg_hooks.so")
DEBUG_LIB = os.path.join(LIBDIR, "libmavg_debug.so")
TILE, CHAIN, STRIP = "biquad_tile<", "biquad_chain<", "biquad_strip "
KINDS = [("i16", 1), ("i16", 2), ("f32", 1), ("f32", 2)]
GUARD = 64          # floats before and after the output view
SENTINEL = 12345.5
STRIP_FRAMES = 64
CARRY_CHUNK = 2048

LP, HP, BP, PK = rbj("LP", 0.05, 0.7071), rbj("HP", 0.01, 0.7071), rbj("BP", 0.05, 4.0), rbj("PK", 0.25, 30.0)
TILE_FILTERS = [LP, HP, BP, PK, FIR3, COPY] + REAL_POLE_CASES
LP_SLOW, HP_SLOW = rbj("LP", 5e-4, 0.7071), rbj("HP", 1e-4, 0.7071)
HP_EDGE = rbj("HP", f_at_domain_edge(0.5001, "HP"), 0.5001)      # D = 2^-22, f about 7.8e-5: the domain's edge
CHAIN_FILTERS = [LP_SLOW, HP_SLOW, HP_EDGE]


def _dsp():
    import digital_signal_processsing_amd as dsp
    return dsp


def _dt(kind):
    return _dsp().I16 if kind == "i16" else _dsp().F32


def sample_size(kind):
    return 2 if kind == "i16" else 4


def rule_boundary(kind, C):
    """The longest halo the tile rule takes: H * C * sample size of 16 KiB."""
    return 16384 // (C * sample_size(kind))


def unit_frames(kind, C):
    return 16 // (C * sample_size(kind))


def plan_of(kind, C, frames, coef, aligned=True, library=None, **kw):
    return _dsp().biquad_plan(frames * C, coef, C, _dt(kind), library=library, aligned=aligned, **kw)


def plan_int(plan, key):
    return int(plan.split(f" {key}=")[1].split()[0])


def tile_frames(kind, C, aligned=True):
    return plan_int(plan_of(kind, C, 1 << 20, LP, aligned=aligned), "tile_frames")


_signals = {}


def signal(oracle, kind, C, frames, seed=1):
    """A synthetic signal, made once and never modified."""
    key = (kind, C, frames, seed)
    if key not in _signals:
        x = oracle.synth_i16(frames * C, seed=seed) if kind == "i16" else oracle.synth_f32(frames * C, seed=seed, dist=1)
        x.setflags(write=False)
        _signals[key] = x
    return _signals[key]


_refs = {}


def reference(x, coef, C, state=None, key=None):
    """(y_ref, state_ref) of biquad_ref, computed once per (signal, filter, state) and left unchanged."""
    k = (key, tuple(coef), C, None if state is None else tuple(np.asarray(state).reshape(-1)))
    if key is None or k not in _refs:
        r, s = biquad_ref(x, coef, C, state, fast=True)
        r.setflags(write=False)
        if key is None:
            return r, s
        _refs[k] = (r, s)
    return _refs[k]


_states = {}


def state_of(oracle, coef, x, C, big=False):
    """A state the filter produces: the reference's after 3000 warm-up frames of the signal's kind
    and amplitude (big: 100 x it), [C, 2]."""
    kind = "i16" if x.dtype == np.int16 else "f32"
    key = (tuple(coef), kind, C, big)
    if key not in _states:
        w = signal(oracle, kind, C, 3000, seed=77).astype(np.float64) * (100.0 if big else 1.0)
        _states[key] = biquad_ref(w, coef, C, None, fast=True)[1]
    return _states[key]


def run(dev, x, coef, C, state=None, want_state=True, off_in=0, off_out=0, library=None, family=None, form=None,
        workspace=None):
    """mavg_biquad_run on views `off_*` samples past a 16-B boundary, the output inside guard regions
    that must come back untouched; the plan must show `family` (and F=`form`).  Returns
    (y as fp32 numpy, state_out as fp64 [C, 2] numpy or None)."""
    import torch
    dsp = _dsp()
    n = x.size
    kind = "i16" if x.dtype == np.int16 else "f32"
    xin = torch.empty(n + 16, dtype=torch.int16 if kind == "i16" else torch.float32, device=dev)
    xv = xin[off_in:off_in + n]
    xv.copy_(torch.tensor(x))
    buf = torch.full((n + 2 * GUARD + 16,), SENTINEL, dtype=torch.float32, device=dev)
    assert xin.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    view = buf[GUARD + off_out:GUARD + off_out + n]
    sin = torch.tensor(np.asarray(state, dtype=np.float64).reshape(C, 2)).to(dev) if state is not None else None
    sbuf = torch.full((2 * C + 2,), SENTINEL, dtype=torch.float64, device=dev)
    sout = sbuf[1:1 + 2 * C] if want_state else None
    aligned = off_in * sample_size(kind) % 16 == 0 and off_out * 4 % 16 == 0
    if n:
        plan = dsp.biquad_plan(n, coef, C, _dt(kind), state is not None, want_state, library=library, aligned=aligned)
        if family is not None:
            assert plan.startswith(family), plan
        if form is not None:
            assert f",F={form}," in plan, plan
    dsp.biquad_into(xv, view, coef, channels=C, state=sin, state_out=sout, workspace=workspace, library=library)
    torch.cuda.synchronize()
    full = buf.cpu().numpy()
    lo, hi = GUARD + off_out, GUARD + off_out + n
    assert (full[:lo] == SENTINEL).all() and (full[hi:] == SENTINEL).all(), "guard region written"
    sfull = sbuf.cpu().numpy()
    assert sfull[0] == SENTINEL and sfull[-1] == SENTINEL, "state guard written"
    if not want_state or n == 0:
        assert (sfull == SENTINEL).all(), "state_out written though NULL or n == 0"
    assert np.array_equal(xv.cpu().numpy(), x), "the input was modified"
    return full[lo:hi].copy(), (sfull[1:1 + 2 * C].reshape(C, 2).copy() if want_state else None)


def check(dev, x, coef, C, state=None, ref=None, key=None, **kw):
    """run() against the reference and the bar; the state within 2^-29 G M per component."""
    r, rs = ref if ref is not None else reference(x, coef, C, state, key)
    G, M = biquad_gain(coef), biquad_scale(x, state)
    y, s = run(dev, x, coef, C, state=state, **kw)
    err = np.abs(y.astype(np.float64) - r)
    bar = biquad_bar(r, G, M)
    worst = int(np.argmax(err - bar)) if err.size else 0
    assert (err <= bar).all(), (coef, C, kw.get("family"), worst, float(err[worst]), float(bar[worst]))
    if s is not None and x.size:
        tol = 2.0 ** -29 * G * M
        serr = np.abs(s - rs)
        assert (serr <= tol).all(), (coef, C, kw.get("family"), serr.tolist(), tol)
    return y, s


class forced:
    """A path forced on the hooks build, the rule restored on the way out."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        from digital_signal_processsing_amd import _lib
        self.lib = _lib.load(HOOKS_LIB)
        assert self.lib.mavg_debug_force_biquad(self.path) == _lib.OK
        return HOOKS_LIB

    def __exit__(self, *exc):
        self.lib.mavg_debug_force_biquad(0)
        return False


# ---- the tile kernel by the rule: both unit forms, every filter class ----
@pytest.mark.parametrize("kind,C", KINDS)
@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 0), (0, 1), (3, 2), (2, 3)])
def test_tile_by_rule(gpu, oracle_mod, kind, C, off_in, off_out):
    aligned = off_in * sample_size(kind) % 16 == 0 and off_out * 4 % 16 == 0
    F = unit_frames(kind, C) if aligned else 1
    tf = tile_frames(kind, C, aligned)
    assert aligned or tf == 1024
    frames = 3 * tf + 17
    x = signal(oracle_mod, kind, C, frames)
    for i, coef in enumerate(TILE_FILTERS):
        kw = dict(off_in=off_in, off_out=off_out, family=TILE, form=F, key=(kind, C, frames))
        check(gpu, x, coef, C, **kw)
        check(gpu, x, coef, C, state=state_of(oracle_mod, coef, x, C), **kw)
        if i % 3 == 0:      # a state 100 x the signal: the closed-form state term is what is tested
            check(gpu, x, coef, C, state=state_of(oracle_mod, coef, x, C, big=True), **kw)
        if i % 3 == 1:      # no d_state_out
            check(gpu, x, coef, C, state=state_of(oracle_mod, coef, x, C), want_state=False, **kw)


def lp_with_halo_in(lo_frames, hi_frames):
    """An LP, Q 0.7071, whose library H lies in [lo_frames, hi_frames]."""
    lo, hi = 1e-5, 0.25
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        H = _dsp().biquad_halo_frames(rbj("LP", mid, 0.7071))
        if lo_frames <= H <= hi_frames:
            return rbj("LP", mid, 0.7071)
        lo, hi = (mid, hi) if H > hi_frames else (lo, mid)
    raise AssertionError((lo_frames, hi_frames))


# ---- a state no input produces: the tile kernel's state horizon (outputs only: mavg.h "Which states") ----
@pytest.mark.parametrize("kind,C", KINDS)
@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 3)])
def test_tile_with_a_state_no_input_produces(gpu, oracle_mod, kind, C, off_in, off_out):
    """A state_in 100 x the signal, both components of one sign, and a filter whose halo ends just
    before the second tile while the state's horizon (tests/biquad_ref.py state_horizon) ends after
    it starts: that tile is past H and must still see the state.  The test first shows from the
    reference alone that the state's share of the second tile's first output is above the bar."""
    aligned = off_in == 0 and off_out == 0
    F = unit_frames(kind, C) if aligned else 1
    tf = tile_frames(kind, C, aligned)
    frames = 3 * tf + 17
    x = signal(oracle_mod, kind, C, frames)
    coef = lp_with_halo_in(int(0.93 * tf), int(0.97 * tf))
    H = _dsp().biquad_halo_frames(coef)
    assert H < tf < state_horizon(coef), (H, tf, state_horizon(coef))
    amp = float(np.abs(x.astype(np.float64)).max())
    st = np.full((C, 2), 100.0 * amp)
    r, rs = reference(x, coef, C, st, key=(kind, C, frames))
    r0, _ = reference(x, coef, C, None, key=(kind, C, frames))
    G, M = biquad_gain(coef), biquad_scale(x, st)
    share = np.abs(r - r0).reshape(-1, C)[tf]            # what the state adds at the second tile's first frame
    assert (share > biquad_bar(r.reshape(-1, C)[tf], G, M)).all(), (share, G, M)
    y, _ = run(gpu, x, coef, C, state=st, off_in=off_in, off_out=off_out, family=TILE, form=F)
    err = np.abs(y.astype(np.float64) - r)
    bar = biquad_bar(r, G, M)
    worst = int(np.argmax(err - bar))
    assert (err <= bar).all(), (coef, worst, float(err[worst]), float(bar[worst]))


def lp_at_boundary(lim):
    """(f_in, f_out): LP filters, Q 0.7071, adjacent in f: the library's H <= lim, and H > lim."""
    H = lambda f: _dsp().biquad_halo_frames(rbj("LP", f, 0.7071))
    lo, hi = 1e-5, 0.25
    assert H(lo) > lim >= H(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if H(mid) > lim:
            lo = mid
        else:
            hi = mid
    return hi, lo


# ---- the rule's boundary: the longest halo the tile takes, the first the chain takes ----
@pytest.mark.parametrize("kind,C", KINDS)
@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 3)])
def test_boundary_by_rule(gpu, oracle_mod, kind, C, off_in, off_out):
    aligned = off_in == 0 and off_out == 0
    F = unit_frames(kind, C) if aligned else 1
    frames = 3 * tile_frames(kind, C, aligned) + 17
    x = signal(oracle_mod, kind, C, frames)
    f_in, f_out = lp_at_boundary(rule_boundary(kind, C))
    for f, fam in ((f_in, TILE), (f_out, CHAIN)):
        coef = rbj("LP", f, 0.7071)
        H = _dsp().biquad_halo_frames(coef)
        assert (H <= rule_boundary(kind, C)) == (fam == TILE)
        assert plan_int(plan_of(kind, C, frames, coef, aligned), "halo_frames") == H
        kw = dict(off_in=off_in, off_out=off_out, family=fam, form=F, key=(kind, C, frames))
        check(gpu, x, coef, C, **kw)
        check(gpu, x, coef, C, state=state_of(oracle_mod, coef, x, C), **kw)


# ---- the chain: by the rule, and forced on the tile's filters ----
@pytest.mark.parametrize("kind,C", KINDS)
@pytest.mark.parametrize("off_in,off_out", [(0, 0), (1, 3)])
def test_chain_by_rule_and_forced(gpu, oracle_mod, kind, C, off_in, off_out):
    aligned = off_in == 0 and off_out == 0
    F = unit_frames(kind, C) if aligned else 1
    tf = tile_frames(kind, C, aligned)
    frames = 3 * tf + 17
    x = signal(oracle_mod, kind, C, frames)
    kw = dict(off_in=off_in, off_out=off_out, family=CHAIN, form=F, key=(kind, C, frames))
    assert 2.0 ** -22 <= domain_d(HP_EDGE) < 2.0 ** -22 * 1.001
    for coef in CHAIN_FILTERS:
        check(gpu, x, coef, C, **kw)
        check(gpu, x, coef, C, state=state_of(oracle_mod, coef, x, C), **kw)
    with forced(2) as lib:
        for i, coef in enumerate(TILE_FILTERS):
            check(gpu, x, coef, C, library=lib, **kw)
            check(gpu, x, coef, C, state=state_of(oracle_mod, coef, x, C, big=(i == 0)), library=lib, **kw)


def test_chain_crosses_a_carry_chunk(gpu, oracle_mod):
    """(carry_chunk + 3) tiles plus 17 frames, fp32 mono, on the smallest tile the plan offers (the
    frame-unit form's): kernel B's running carry links two chunks."""
    plan = plan_of("f32", 1, 1 << 20, LP_SLOW, aligned=False)
    assert plan.startswith(CHAIN)
    tf, chunk = plan_int(plan, "tile_frames"), plan_int(plan, "carry_chunk")
    assert tf == 1024 and chunk == CARRY_CHUNK
    frames = (chunk + 3) * tf + 17
    assert plan_int(plan_of("f32", 1, frames, LP_SLOW, aligned=False), "records") == chunk + 4
    x = signal(oracle_mod, "f32", 1, frames, seed=2)
    check(gpu, x, LP_SLOW, 1, state=state_of(oracle_mod, LP_SLOW, x, 1), family=CHAIN, off_in=1, off_out=1, form=1)


# ---- the strip form: three or more channels by the rule, mono and stereo forced ----
@pytest.mark.parametrize("kind,C,frames,coef", [
    ("f32", 3, 6161, LP), ("i16", 3, 6161, LP_SLOW), ("f32", 5, 6161, HP_EDGE), ("i16", 8, 6161, COPY), ("f32", 8, 63, PK),
    ("f32", 3, CARRY_CHUNK * STRIP_FRAMES, HP_SLOW),          # carry_chunk strips exactly
    ("i16", 5, CARRY_CHUNK * STRIP_FRAMES + 1, LP),           # one strip of one frame past the chunk
    ("f32", 8, (CARRY_CHUNK + 1) * STRIP_FRAMES + 17, LP_SLOW),
])
def test_strip_by_rule(gpu, oracle_mod, kind, C, frames, coef):
    x = signal(oracle_mod, kind, C, frames, seed=3)
    assert plan_int(plan_of(kind, C, frames, coef), "strips") == -(-frames // STRIP_FRAMES)
    key = (kind, C, frames, 3)
    check(gpu, x, coef, C, family=STRIP, key=key)
    check(gpu, x, coef, C, state=state_of(oracle_mod, coef, x, C), off_in=1, off_out=3, family=STRIP, key=key)


@pytest.mark.parametrize("kind,C", KINDS)
def test_strip_forced(gpu, oracle_mod, kind, C):
    frames = (CARRY_CHUNK - 1) * STRIP_FRAMES + 130     # carry_chunk + 2 strips: past the carry kernel's chunk
    x = signal(oracle_mod, kind, C, frames, seed=4)
    with forced(3) as lib:
        for coef in (LP, LP_SLOW):
            check(gpu, x, coef, C, state=state_of(oracle_mod, coef, x, C), library=lib, family=STRIP,
                  key=(kind, C, frames, 4))


# ---- the three paths on one shape ----
@pytest.mark.parametrize("kind,C", KINDS)
def test_paths_agree_within_twice_the_bar(gpu, oracle_mod, kind, C):
    frames = 3 * tile_frames(kind, C) + 17
    x = signal(oracle_mod, kind, C, frames)
    for coef in (LP, rbj("LP", lp_at_boundary(rule_boundary(kind, C))[0], 0.7071)):
        s = state_of(oracle_mod, coef, x, C)
        ref = reference(x, coef, C, s, key=(kind, C, frames))
        ys = []
        for path, fam in ((1, TILE), (2, CHAIN), (3, STRIP)):
            with forced(path) as lib:
                ys.append(check(gpu, x, coef, C, state=s, ref=ref, library=lib, family=fam)[0].astype(np.float64))
        bar = 2.0 * biquad_bar(ref[0], biquad_gain(coef), biquad_scale(x, s))
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert (np.abs(ys[i] - ys[j]) <= bar).all(), (coef, i, j)


# ---- streaming: state_out -> state_in reproduces the one-shot output within the bar ----
@pytest.mark.parametrize("kind,C", KINDS)
@pytest.mark.parametrize("path", [1, 2, 3])
def test_streaming_through_the_state(gpu, oracle_mod, kind, C, path):
    tf = tile_frames(kind, C)
    cuts = [1, 7, tf - 1, tf + 1, 1000, 7, 1, tf + 1]
    frames = sum(cuts)
    x = signal(oracle_mod, kind, C, frames, seed=6)
    coef = rbj("LP", 0.004, 0.7071)           # a halo of about a thousand frames: inside every tile rule
    s0 = state_of(oracle_mod, coef, x, C)
    ref, rs = reference(x, coef, C, s0, key=(kind, C, frames, 6))
    ref = ref.reshape(-1, C)
    G, M = biquad_gain(coef), biquad_scale(x, s0)
    fam = {1: TILE, 2: CHAIN, 3: STRIP}[path]
    state, f0 = s0, 0
    with forced(path) as lib:
        for m in cuts:
            xc = x.reshape(-1, C)[f0:f0 + m].reshape(-1)
            # views that start wherever the chunk starts: the offset follows the cut
            y, after = run(gpu, xc, coef, C, state=state, off_in=f0 % 4, off_out=(f0 + 1) % 4, library=lib, family=fam)
            r = ref[f0:f0 + m].reshape(-1)
            err = np.abs(y.astype(np.float64) - r)
            assert (err <= biquad_bar(r, G, M)).all(), (path, f0, m, float(err.max()))
            # d_state_out as the header promises it: against the reference of this call, from this call's state_in
            want = biquad_ref(xc, coef, C, state)[1]
            assert (np.abs(after - want) <= 2.0 ** -29 * G * biquad_scale(xc, state)).all(), (path, f0, m)
            state, f0 = after, f0 + m


# ---- degenerate sizes ----
@pytest.mark.parametrize("kind,C", KINDS)
def test_degenerate_sizes(gpu, oracle_mod, kind, C):
    F = unit_frames(kind, C)
    for frames in sorted({1, F - 1, F + 1, 65} - {0}):
        x = signal(oracle_mod, kind, C, frames, seed=8)
        for coef, fam in ((LP, TILE), (COPY, TILE), (FIR3, TILE), (HP_SLOW, CHAIN)):
            check(gpu, x, coef, C, family=fam)
            check(gpu, x, coef, C, state=state_of(oracle_mod, coef, x, C, big=True), family=fam, off_in=1, off_out=1)
    empty = np.zeros(0, dtype=np.int16 if kind == "i16" else np.float32)
    y, s = run(gpu, empty, LP, C, state=np.ones((C, 2)))          # n = 0: state_out untouched (run() checks)
    assert y.size == 0


def test_three_channel_degenerate_and_wrapper(gpu, oracle_mod):
    import torch
    dsp = _dsp()
    x = signal(oracle_mod, "f32", 3, 1, seed=8)
    check(gpu, x, LP, 3, state=state_of(oracle_mod, LP, x, 3), family=STRIP)
    # the allocating wrapper: shapes, a scipy-style row of six, return_state
    xs = signal(oracle_mod, "i16", 2, 5003, seed=9)
    xt = torch.tensor(xs).to(gpu).reshape(-1, 2)
    row = (2.0 * LP[0], 2.0 * LP[1], 2.0 * LP[2], 2.0, 2.0 * LP[3], 2.0 * LP[4])
    y, st = dsp.biquad(xt, row, return_state=True)
    assert y.shape == xt.shape and y.dtype == torch.float32 and st.dtype == torch.float64 and st.shape == (2, 2)
    r, rs = biquad_ref(xs, LP, 2)
    G = biquad_gain(LP)
    assert (np.abs(y.cpu().numpy().reshape(-1).astype(np.float64) - r) <= biquad_bar(r, G, biquad_scale(xs))).all()
    assert (np.abs(st.cpu().numpy() - rs) <= 2.0 ** -29 * G * biquad_scale(xs)).all()
    y2 = dsp.biquad(xt, LP, state=st)
    r2, _ = biquad_ref(xs, LP, 2, rs)
    assert (np.abs(y2.cpu().numpy().reshape(-1).astype(np.float64) - r2) <= biquad_bar(r2, G, biquad_scale(xs, rs))).all()


# ---- graph capture: the chain's workspace needs no memset ----
def test_chain_graph_capture_and_replay(gpu, oracle_mod):
    import torch
    dsp = _dsp()
    frames = 3 * 2048 + 17
    x = signal(oracle_mod, "f32", 1, frames)
    coef = LP_SLOW
    assert plan_of("f32", 1, frames, coef).startswith(CHAIN)
    s0 = state_of(oracle_mod, coef, x, 1)
    xt = torch.tensor(x).to(gpu)
    out = torch.zeros(frames, dtype=torch.float32, device=gpu)
    sin = torch.tensor(s0, dtype=torch.float64, device=gpu)
    sout = torch.zeros((1, 2), dtype=torch.float64, device=gpu)
    ws = torch.full((dsp.biquad_workspace_bytes(frames, coef),), 0xAB, dtype=torch.uint8, device=gpu)   # garbage, never zeroed
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            dsp.biquad_into(xt, out, coef, state=sin, state_out=sout, workspace=ws, stream=side)
    r, rs = biquad_ref(x, coef, 1, s0)
    G, M = biquad_gain(coef), biquad_scale(x, s0)
    got = []
    for _ in range(2):
        out.zero_()
        sout.zero_()
        ws.fill_(0x5C)
        g.replay()
        torch.cuda.synchronize()
        got.append(out.cpu().numpy().copy())
        assert (np.abs(got[-1].astype(np.float64) - r) <= biquad_bar(r, G, M)).all()
        assert (np.abs(sout.cpu().numpy() - rs) <= 2.0 ** -29 * G * M).all()
    assert np.array_equal(got[0], got[1])


# ---- the debug build: the MAVG_DCHECK bounds run clean ----
@pytest.mark.parametrize("kind,C", [("f32", 1), ("i16", 2)])
def test_debug_build_bounds_run_clean(gpu, oracle_mod, kind, C):
    frames = 3 * tile_frames(kind, C) + 17
    x = signal(oracle_mod, kind, C, frames)
    key = (kind, C, frames)
    edge = rbj("LP", lp_at_boundary(rule_boundary(kind, C))[0], 0.7071)
    check(gpu, x, edge, C, state=state_of(oracle_mod, edge, x, C), library=DEBUG_LIB, family=TILE, key=key)
    check(gpu, x, LP, C, library=DEBUG_LIB, family=TILE, off_in=1, off_out=2, form=1)
    check(gpu, x, LP_SLOW, C, state=state_of(oracle_mod, LP_SLOW, x, C), library=DEBUG_LIB, family=CHAIN, key=key)


# ---- sos_filter: sections through fp32 ping-pong buffers ----
def butter4_lp(f):
    """A 4th-order Butterworth low-pass as two sections: RBJ low-passes with the Butterworth Qs."""
    return [rbj("LP", f, 1.0 / (2.0 * math.cos(math.pi / 8.0))), rbj("LP", f, 1.0 / (2.0 * math.cos(3.0 * math.pi / 8.0)))]


@pytest.mark.parametrize("kind,C,sections", [("f32", 1, "butter"), ("i16", 2, "hp_pk")])
def test_sos_filter(gpu, oracle_mod, kind, C, sections):
    import torch
    dsp = _dsp()
    secs = butter4_lp(0.05) if sections == "butter" else [HP, rbj("PK", 0.05, 4.0)]
    sos = np.array([[c[0], c[1], c[2], 1.0, c[3], c[4]] for c in secs])
    frames = 5003
    x = signal(oracle_mod, kind, C, frames, seed=10)
    xt = torch.tensor(x).to(gpu)

    def cascade(xin, states):
        """The fp64 cascade and the uniform tolerance sum_j e_j prod_{i > j} G_i, e_j = 2^-23 max |r_j| +
        2^-29 G_j M_j + 2^-24 max |r_j| (the last term: the fp32 intermediate)."""
        cur, outs, es = np.asarray(xin, dtype=np.float64), [], []
        for j, c in enumerate(secs):
            st = None if states is None else states[j]
            M = biquad_scale(cur, st)
            cur, so = biquad_ref(cur, c, C, st)
            outs.append(so)
            mr = float(np.abs(cur).max())
            es.append(2.0 ** -23 * mr + 2.0 ** -29 * biquad_gain(c) * M + 2.0 ** -24 * mr)
        Gs = [biquad_gain(c) for c in secs]
        tol = sum(e * float(np.prod(Gs[j + 1:])) for j, e in enumerate(es))
        return cur, np.array(outs), tol

    half = (frames // 2) * C
    r_all, _, tol = cascade(x, None)
    y = dsp.sos_filter(xt, sos, channels=C)
    assert y.dtype == torch.float32 and y.shape == xt.shape
    assert np.abs(y.cpu().numpy().astype(np.float64) - r_all).max() <= tol
    # the state round trip: two halves reproduce the whole
    ya, sa = dsp.sos_filter(xt[:half], sos, channels=C, return_state=True)
    assert sa.shape == (len(secs), C, 2) and sa.dtype == torch.float64
    ra, rsa, tola = cascade(x[:half], None)
    assert np.abs(ya.cpu().numpy().astype(np.float64) - ra).max() <= tola
    yb, sb = dsp.sos_filter(xt[half:], sos, channels=C, state=sa, return_state=True)
    rb, rsb, tolb = cascade(x[half:], sa.cpu().numpy())
    assert np.abs(yb.cpu().numpy().astype(np.float64) - rb).max() <= tolb
    assert np.abs(yb.cpu().numpy().astype(np.float64) - r_all[half:]).max() <= tol + tola
    assert np.abs(sb.cpu().numpy() - rsb).max() <= tolb
