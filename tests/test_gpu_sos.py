"""mavg_sos_run on the GPU against the fp64 cascade (tests/sos_ref.py) and the header's two bars:
sos_tile by rule and forced, sos_loop forced and past the halo limit, misaligned views, degenerate
sizes, the state round trip, the worst-case input, the proof that the fused intermediate is fp64,
graph capture, and an Inf that stays in its channel.  Shapes are about three tiles and a ragged tail;
9, 16 and 17 sections, signals that end on, one frame before and one frame past a tile boundary, and
a section without a halo between two with one have tests of their own."""
import os

import numpy as np
import pytest

from biquad_ref import rbj
from sos_ref import (COPY, DC_BLOCK, HP_PK, SEVEN, THIRD, THREE, TIMES3, butter4_lp, one_pole, rows6, rule_takes_tile,
                     sections_with_halo, sos_bar, sos_ref, sos_state_bar, worst_case_input)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "digital_signal_processsing_amd", "lib")
HOOKS_LIB = os.path.join(LIBDIR, "libmavg_hooks.so")
DEBUG_LIB = os.path.join(LIBDIR, "libmavg_debug.so")
TILE, LOOP = "sos_tile<", "sos_loop "
KINDS = [("i16", 1), ("i16", 2), ("f32", 1), ("f32", 2)]
GUARD = 64          # floats before and after the output view
SENTINEL = 12345.5
LIMIT = {1: 2048, 2: 1024}
B4 = butter4_lp(0.05)


def _dsp():
    import digital_signal_processsing_amd as dsp
    return dsp


def _dt(kind):
    return _dsp().I16 if kind == "i16" else _dsp().F32


def tile_frames(C):
    plan = _dsp().sos_plan(1 << 20, rows6(B4), C)
    return int(plan.split(" tile_frames=")[1].split()[0])


_sets = {}


def section_set(name, C):
    """The section sets of the issue; `limit` / `past`: eight sections whose halos sum to the fused
    kernel's limit for C channels, and to one frame more; `limit16`: the kernel's 16 sections at that
    limit (SEVEN, eight one-pole low-passes and the fitted one); `nine`: its first nine rows;
    `seventeen`: one section more than the kernel takes, far inside the halo limit."""
    if (name, C) not in _sets:
        halo = _dsp().biquad_halo_frames
        _sets[(name, C)] = {"butter4": lambda: B4, "hp_pk": lambda: HP_PK, "three": lambda: THREE,
                            "limit": lambda: sections_with_halo(LIMIT[C], halo, SEVEN),
                            "past": lambda: sections_with_halo(LIMIT[C] + 1, halo, SEVEN),
                            "limit16": lambda: sections_with_halo(LIMIT[C], halo, SEVEN + [one_pole(0.5)] * 8),
                            "nine": lambda: section_set("limit16", C)[:9],
                            "seventeen": lambda: SEVEN + [one_pole(0.5)] * 10,
                            "zero_halo_mid": lambda: [rbj("LP", 0.05, 0.7071), THIRD, rbj("HP", 0.05, 0.7071)]}[name]()
    return _sets[(name, C)]


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


def reference(x, sos, C, state=None, key=None):
    """(y_ref, state_ref) of sos_ref, computed once per key and left unchanged."""
    k = (key, tuple(map(tuple, sos)), C, None if state is None else tuple(np.asarray(state).reshape(-1)))
    if key is None or k not in _refs:
        r, s = sos_ref(x, sos, C, state)
        r.setflags(write=False)
        if key is None:
            return r, s
        _refs[k] = (r, s)
    return _refs[k]


def run(dev, x, sos, C, state=None, want_state=True, off_in=0, off_out=0, library=None, family=None, form=None,
        intermediate="auto"):
    """mavg_sos_run on views `off_*` samples past a 16-B boundary, the output and the state inside
    guard regions that must come back untouched; the plan must show `family` (and F=`form`).
    Returns (y as fp32 numpy, state_out as fp64 [S, C, 2] numpy or None)."""
    import torch
    dsp = _dsp()
    n, S = x.size, len(sos)
    kind = "i16" if x.dtype == np.int16 else "f32"
    xin = torch.empty(n + 16, dtype=torch.int16 if kind == "i16" else torch.float32, device=dev)
    xv = xin[off_in:off_in + n]
    xv.copy_(torch.tensor(x))
    buf = torch.full((n + 2 * GUARD + 16,), SENTINEL, dtype=torch.float32, device=dev)
    assert xin.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    view = buf[GUARD + off_out:GUARD + off_out + n]
    sin = torch.tensor(np.asarray(state, dtype=np.float64).reshape(S, C, 2)).to(dev) if state is not None else None
    sbuf = torch.full((2 * C * S + 2,), SENTINEL, dtype=torch.float64, device=dev)
    sout = sbuf[1:1 + 2 * C * S] if want_state else None
    aligned = off_in * (2 if kind == "i16" else 4) % 16 == 0 and off_out * 4 % 16 == 0
    if n:
        plan = dsp.sos_plan(n, rows6(sos), C, _dt(kind), state is not None, want_state, intermediate, library=library,
                            aligned=aligned)
        if family is not None:
            assert plan.startswith(family), plan
        if form is not None:
            assert f",F={form}>" in plan, plan
    dsp.sosfilt_into(xv, view, rows6(sos), channels=C, state=sin, state_out=sout, intermediate=intermediate, library=library)
    torch.cuda.synchronize()
    full = buf.cpu().numpy()
    lo, hi = GUARD + off_out, GUARD + off_out + n
    assert (full[:lo] == SENTINEL).all() and (full[hi:] == SENTINEL).all(), "guard region written"
    sfull = sbuf.cpu().numpy()
    assert sfull[0] == SENTINEL and sfull[-1] == SENTINEL, "state guard written"
    if not want_state or n == 0:
        assert (sfull == SENTINEL).all(), "state_out written though NULL or n == 0"
    assert np.array_equal(xv.cpu().numpy(), x), "the input was modified"
    return full[lo:hi].copy(), (sfull[1:1 + 2 * C * S].reshape(S, C, 2).copy() if want_state else None)


def check(dev, x, sos, C, state=None, ref=None, key=None, loop=False, **kw):
    """run() against the reference and the path's bar, the states against theirs; returns
    (y, state_out, the largest error over the bar)."""
    r, rs = ref if ref is not None else reference(x, sos, C, state, key)
    y, s = run(dev, x, sos, C, state=state, **kw)
    err = np.abs(y.astype(np.float64) - r)
    bar = sos_bar(r, sos, x, state, loop)
    worst = int(np.argmax(err - bar)) if err.size else 0
    ratio = float((err / bar).max()) if err.size else 0.0
    print(f"sos {kw.get('family')} S={len(sos)} C={C} {x.dtype} n={x.size}: max err / bar = {ratio:.4f}")
    assert (err <= bar).all(), (C, kw.get("family"), worst, float(err[worst]), float(bar[worst]))
    if s is not None and x.size:
        tol = sos_state_bar(sos, x, state, loop)
        serr = np.abs(s - rs.reshape(len(sos), C, 2)).reshape(len(sos), -1).max(axis=1)
        assert (serr <= tol).all(), (C, kw.get("family"), serr.tolist(), tol.tolist())
    return y, s, ratio


class forced:
    """A path forced on the hooks build, the rule restored on the way out."""

    def __init__(self, path):
        self.path = path

    def __enter__(self):
        from digital_signal_processsing_amd import _lib
        self.lib = _lib.load(HOOKS_LIB)
        assert self.lib.mavg_debug_force_sos(self.path) == _lib.OK
        return HOOKS_LIB

    def __exit__(self, *exc):
        self.lib.mavg_debug_force_sos(0)
        return False


def state_for(oracle, sos, kind, C):
    """A state the cascade produces: the reference's after 3000 warm-up frames of the signal's kind."""
    w = signal(oracle, kind, C, 3000, seed=77)
    return sos_ref(w, sos, C)[1]


# ---- parity: by rule, forced tile, forced loop, each with its own bar ----
@pytest.mark.parametrize("kind,C", KINDS)
@pytest.mark.parametrize("name", ["butter4", "hp_pk", "three", "limit", "past", "nine", "limit16"])
def test_parity_by_rule_and_forced(gpu, oracle_mod, kind, C, name):
    dsp = _dsp()
    sos = section_set(name, C)
    frames = 3 * tile_frames(C) + 1234
    x = signal(oracle_mod, kind, C, frames)
    key = (kind, C, frames)
    fits = name != "past"
    H = dsp.sos_halo_frames(rows6(sos))
    assert H <= LIMIT[C] if fits else H == LIMIT[C] + 1
    if name in ("nine", "limit16"):           # 9 and 16 distinct starts and run lengths, 10 and 17 launches
        assert len(sos) == (9 if name == "nine" else 16) and (name == "nine" or H == LIMIT[C])
        plan = dsp.sos_plan(x.size, rows6(sos), C, _dt(kind))
        assert f" sections={len(sos)} " in plan and plan.endswith(f" launches={len(sos) + 1}"), plan
    tile = fits and rule_takes_tile(kind == "i16", C, len(sos), H)      # (int16 mono pairs past 2 KiB: the loop)
    check(gpu, x, sos, C, key=key, family=TILE if tile else LOOP, loop=not tile)            # the rule
    s0 = state_for(oracle_mod, sos, kind, C)
    with forced(1) as lib:
        if fits:
            check(gpu, x, sos, C, state=s0, key=key, library=lib, family=TILE, intermediate="fp64")
        else:
            with pytest.raises(dsp.MavgError):
                run(gpu, x, sos, C, library=lib)
    with forced(2) as lib:
        check(gpu, x, sos, C, state=s0, key=key, library=lib, family=LOOP, loop=True)


# ---- views off 16-B alignment: the frame-unit form ----
@pytest.mark.parametrize("kind,C", KINDS)
@pytest.mark.parametrize("off_in,off_out", [(1, 0), (0, 1), (3, 2)])
def test_misaligned_views(gpu, oracle_mod, kind, C, off_in, off_out):
    frames = 3 * tile_frames(C) + 1234
    x = signal(oracle_mod, kind, C, frames)
    sos = section_set("hp_pk", C)
    check(gpu, x, sos, C, key=(kind, C, frames), family=TILE, form=1, off_in=off_in, off_out=off_out,
          state=state_for(oracle_mod, sos, kind, C), intermediate="fp64")


# ---- fewer frames than the halo; one frame ----
@pytest.mark.parametrize("kind,C", KINDS)
def test_degenerate_sizes(gpu, oracle_mod, kind, C):
    sos = section_set("three", C)
    H = _dsp().sos_halo_frames(rows6(sos))
    s0 = state_for(oracle_mod, sos, kind, C)
    for frames in (1, 2, 7, H - 1):
        x = signal(oracle_mod, kind, C, frames, seed=3)
        check(gpu, x, sos, C, family=TILE)
        check(gpu, x, sos, C, state=s0, family=TILE, off_in=1 if frames > 1 else 0)
    y, s = run(gpu, signal(oracle_mod, kind, C, 0), sos, C, state=s0)
    assert y.size == 0


# ---- streaming: chunk i's state_out is chunk i + 1's state_in ----
@pytest.mark.parametrize("kind,C", KINDS)
@pytest.mark.parametrize("path", [1, 2])
def test_state_round_trip_with_unequal_chunks(gpu, oracle_mod, kind, C, path):
    sos = section_set("butter4" if path == 1 else "three", C)
    TF = tile_frames(C)
    H = _dsp().sos_halo_frames(rows6(sos))
    frames = 3 * TF + 1234
    x = signal(oracle_mod, kind, C, frames)
    ref, sref = reference(x, sos, C, key=(kind, C, frames))
    loop = path == 2
    assert H // 2 < TF
    for cut in (H // 2, TF + H + 77):          # inside the first tile (and the halo); past sum H_j, in the second tile
        with forced(path) as lib:
            fam = TILE if path == 1 else LOOP
            y1, s1, _ = check(gpu, x[:cut * C], sos, C, library=lib, family=fam, loop=loop)
            y2, s2, _ = check(gpu, x[cut * C:], sos, C, state=s1, library=lib, family=fam, loop=loop)
        y = np.concatenate([y1, y2]).astype(np.float64)
        bar = sos_bar(ref, sos, x, None, loop) + sos_bar(ref, sos, x, s1, loop)
        assert (np.abs(y - ref) <= bar).all()
        sbar = sos_state_bar(sos, x, None, loop) + sos_state_bar(sos, x, s1, loop)
        assert (np.abs(s2 - sref).reshape(len(sos), -1).max(axis=1) <= sbar).all()


# ---- the input that maximises what a tile drops by reading only its halo ----
@pytest.mark.parametrize("kind,M", [("f32", 1.0), ("i16", 32767.0)])
@pytest.mark.parametrize("name", ["butter4", "limit"])
def test_worst_case_input_in_front_of_the_second_tile(gpu, kind, M, name):
    sos = section_set(name, 1)
    t0 = tile_frames(1)                       # the first tile past sum H_j (sum H_j < tile_frames)
    assert _dsp().sos_halo_frames(rows6(sos)) < t0
    x = worst_case_input(sos, t0 + t0 // 2 + 33, t0, M=M).astype(np.int16 if kind == "i16" else np.float32)
    with forced(1) as lib:
        _, _, ratio = check(gpu, x, sos, 1, library=lib, family=TILE)
    print(f"worst-case input, {name} {kind}: max err / bar = {ratio:.4f}")
    # The same in the frame-unit form, in front of the third tile, and in stereo: channel 0 carries
    # the pattern and channel 1 its negation one frame later, so a carry that slips from one channel
    # into the other adds up instead of cancelling; each channel against its own mono reference.
    dt = np.int16 if kind == "i16" else np.float32
    for C, off_in, tiles in [(1, 1, 1), (1, 0, 2), (1, 1, 2), (2, 0, 1), (2, 1, 1), (2, 0, 2), (2, 1, 2)]:
        sos = section_set(name, C)
        TF = tile_frames(C)
        t0 = tiles * TF
        assert _dsp().sos_halo_frames(rows6(sos)) < TF
        w = worst_case_input(sos, t0 + TF // 2 + 33, t0, M=M)
        if C == 1:
            x, ref = w.astype(dt), None
        else:
            x = np.stack([w, np.concatenate([[0.0], -w[:-1]])], axis=1).reshape(-1).astype(dt)
            mono = [sos_ref(x[c::2], sos, 1) for c in range(2)]
            ref = (np.stack([m[0] for m in mono], axis=1).reshape(-1), np.stack([m[1][:, 0, :] for m in mono], axis=1))
        with forced(1) as lib:
            _, _, ratio = check(gpu, x, sos, C, ref=ref, library=lib, family=TILE, off_in=off_in, form=1 if off_in else None)
        print(f"worst-case input, {name} {kind} C={C} in+{off_in} in front of tile {tiles}: max err / bar = {ratio:.4f}")


# ---- more sections than any other test runs: 9, 16 (parity above) and one past the kernel's count ----
@pytest.mark.parametrize("kind,C", KINDS)
def test_seventeen_sections_go_to_the_loop(gpu, oracle_mod, kind, C):
    dsp = _dsp()
    sos = section_set("seventeen", C)
    frames = 3 * tile_frames(C) + 1234
    x = signal(oracle_mod, kind, C, frames)
    assert len(sos) == 17 and dsp.sos_halo_frames(rows6(sos)) <= LIMIT[C]      # the count alone keeps it off the tile
    assert " sections=17 " in dsp.sos_plan(x.size, rows6(sos), C, _dt(kind))
    check(gpu, x, sos, C, key=(kind, C, frames), family=LOOP, loop=True)
    with pytest.raises(dsp.MavgError):
        run(gpu, x, sos, C, intermediate="fp64")
    with forced(1) as lib:
        with pytest.raises(dsp.MavgError):
            run(gpu, x, sos, C, library=lib)


# ---- signals that end on a tile boundary, one frame short of it and one frame past it ----
@pytest.mark.parametrize("kind,C", KINDS)
@pytest.mark.parametrize("off_in", [0, 1])
def test_tile_edge_lengths(gpu, oracle_mod, kind, C, off_in):
    """TF, 2 TF and 3 TF frames: the last tile is full (the 16-B-unit form stores it whole).  TF + 1:
    the last tile holds one frame, the last frame sits at stage index Hp and the state_out comes from
    there.  2 TF - 1: one frame short.  The guards of run() catch a store past the end."""
    sos = section_set("three", C)
    TF = tile_frames(C)
    s0 = state_for(oracle_mod, sos, kind, C)
    whole = signal(oracle_mod, kind, C, 3 * TF, seed=5)
    for frames in (TF, TF + 1, 2 * TF - 1, 2 * TF, 3 * TF):
        check(gpu, whole[:frames * C], sos, C, state=s0, family=TILE, form=1 if off_in else None, off_in=off_in,
              intermediate="fp64")


# ---- a section without a halo between two with one: `start` does not advance ----
@pytest.mark.parametrize("kind,C", [("f32", 1), ("i16", 2)])
def test_a_zero_halo_section_in_the_middle(gpu, oracle_mod, kind, C):
    dsp = _dsp()
    sos = section_set("zero_halo_mid", C)
    halos = [dsp.biquad_halo_frames(c) for c in sos]
    assert halos[1] == 0 and halos[0] > 0 and halos[2] > 0, halos
    frames = 3 * tile_frames(C) + 1234
    x = signal(oracle_mod, kind, C, frames)
    check(gpu, x, sos, C, key=(kind, C, frames), family=TILE, intermediate="fp64")
    check(gpu, x, sos, C, state=state_for(oracle_mod, sos, kind, C), key=(kind, C, frames), family=TILE, intermediate="fp64")


# ---- the intermediate is fp64 ----
def test_a_third_times_three_is_the_identity_only_in_fp64(gpu):
    """b = (1/3, 0, 0) then b = (3, 0, 0): an fp64 product pair is within 2^-51 relative of the fp32
    input and rounds back to it, so sos_tile returns x bit for bit; an fp32 intermediate does not."""
    rng = np.random.default_rng(33)
    frames = 3 * tile_frames(1) + 1234
    x = rng.uniform(-1.0, 1.0, frames).astype(np.float32)
    third = (x.astype(np.float64) * (1.0 / 3.0)).astype(np.float32)
    share = float(((third.astype(np.float64) * 3.0).astype(np.float32) != x).mean())
    assert share > 0.1, share                 # near a third of uniform floats do not survive fp32
    sos = [THIRD, TIMES3]
    with forced(1) as lib:
        y, _ = run(gpu, x, sos, 1, library=lib, family=TILE, intermediate="fp64")
    assert np.array_equal(y, x)
    y, _ = run(gpu, x, sos, 1, family=TILE)   # and by the rule
    assert np.array_equal(y, x)
    with forced(2) as lib:
        y, _ = run(gpu, x, sos, 1, library=lib, family=LOOP)
    assert (y != x).sum() >= 1 and abs(float((y != x).mean()) - share) < 0.05


@pytest.mark.parametrize("first", ["copy", "third"])
def test_a_dc_offset_through_a_dc_blocker_needs_the_fp64_stage(gpu, first):
    """1e4 of DC under a unit-scale signal, through a copy (or a gain of 1/3) and then a DC
    blocker: the fused path holds its bar.  With the gain, an fp32 stage cannot: the rounding of the
    intermediate, 2^-24 of 1e4 / 3, passes the blocker -- checked here in numpy."""
    rng = np.random.default_rng(44)
    frames = 3 * tile_frames(1) + 1234
    x = (1e4 + rng.standard_normal(frames)).astype(np.float32)
    sos = [COPY if first == "copy" else THIRD, DC_BLOCK]
    ref, _ = sos_ref(x, sos)
    if first == "third":
        mid = sos_ref(x, sos[:1])[0].astype(np.float32)
        y32 = sos_ref(mid, sos[1:])[0]
        assert (np.abs(y32 - ref) > sos_bar(ref, sos, x)).any()          # an fp32 intermediate misses the bar
    with forced(1) as lib:
        check(gpu, x, sos, 1, ref=(ref, sos_ref(x, sos)[1]), library=lib, family=TILE)


# ---- graph capture: the tables' workspace needs no memset ----
def test_tile_graph_capture_and_replay(gpu, oracle_mod):
    import torch
    dsp = _dsp()
    frames = 3 * tile_frames(1) + 1234
    x = signal(oracle_mod, "f32", 1, frames)
    sos = THREE
    s0 = state_for(oracle_mod, sos, "f32", 1)
    assert dsp.sos_plan(frames, rows6(sos)).startswith(TILE)
    xt = torch.tensor(x).to(gpu)
    out = torch.zeros(frames, dtype=torch.float32, device=gpu)
    sin = torch.tensor(s0, dtype=torch.float64, device=gpu)
    sout = torch.zeros((3, 1, 2), dtype=torch.float64, device=gpu)
    ws = torch.full((dsp.sos_workspace_bytes(frames, rows6(sos)),), 0xAB, dtype=torch.uint8, device=gpu)   # garbage, never zeroed
    dsp.sosfilt_into(xt, out, rows6(sos), state=sin, state_out=sout, workspace=ws)
    torch.cuda.synchronize()
    eager, eager_s = out.cpu().numpy().copy(), sout.cpu().numpy().copy()
    r, rs = sos_ref(x, sos, 1, s0)
    assert (np.abs(eager.astype(np.float64) - r) <= sos_bar(r, sos, x, s0)).all()
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            dsp.sosfilt_into(xt, out, rows6(sos), state=sin, state_out=sout, workspace=ws, stream=side)
    for _ in range(2):
        out.zero_()
        sout.zero_()
        ws.fill_(0x5C)
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), eager) and np.array_equal(sout.cpu().numpy(), eager_s)


# ---- channels are independent: an Inf stays in its channel ----
def test_an_inf_in_one_channel_leaves_the_other_finite(gpu, oracle_mod):
    frames = 3 * tile_frames(2) + 1234
    x = signal(oracle_mod, "f32", 2, frames).copy()
    x[2 * 2500] = np.inf                       # channel 0, inside the first tile
    sos = B4
    y, _ = run(gpu, x, sos, 2, family=TILE)
    clean = x.reshape(-1, 2)[:, 1].copy()
    r, _ = sos_ref(clean, sos, 1)
    y1 = y.reshape(-1, 2)[:, 1].astype(np.float64)
    assert np.isfinite(y1).all()
    assert (np.abs(y1 - r) <= sos_bar(r, sos, clean)).all()
    assert not np.isfinite(y.reshape(-1, 2)[2500:, 0]).all()


# ---- the debug build: the MAVG_DCHECK bounds run clean ----
@pytest.mark.parametrize("kind,C", [("f32", 1), ("i16", 2)])
def test_debug_build_bounds_run_clean(gpu, oracle_mod, kind, C):
    frames = 3 * tile_frames(C) + 1234
    x = signal(oracle_mod, kind, C, frames)
    sos = section_set("limit", C)
    check(gpu, x, sos, C, state=state_for(oracle_mod, sos, kind, C), key=(kind, C, frames), library=DEBUG_LIB, family=TILE)
    check(gpu, x, section_set("butter4", C), C, key=(kind, C, frames), library=DEBUG_LIB, family=TILE, off_in=1, off_out=2, form=1)


# ---- the wrapper ----
def test_sosfilt_wrapper(gpu, oracle_mod):
    import torch
    dsp = _dsp()
    frames = 5000
    x = signal(oracle_mod, "f32", 2, frames)
    xt = torch.tensor(x).to(gpu).reshape(frames, 2)
    y, s = dsp.sosfilt(xt, rows6(B4), return_state=True, intermediate="fp64")
    assert y.shape == (frames, 2) and y.dtype == torch.float32 and s.shape == (2, 2, 2)
    r, rs = sos_ref(x, B4, 2)
    assert (np.abs(y.cpu().numpy().reshape(-1).astype(np.float64) - r) <= sos_bar(r, B4, x)).all()
    x3 = torch.tensor(signal(oracle_mod, "f32", 3, frames)).to(gpu).reshape(frames, 3)
    with pytest.raises(dsp.MavgError):
        dsp.sosfilt(x3, rows6(B4), intermediate="fp64")
    y3 = dsp.sosfilt(x3, rows6(B4))
    r3, _ = sos_ref(signal(oracle_mod, "f32", 3, frames), B4, 3)
    assert (np.abs(y3.cpu().numpy().reshape(-1).astype(np.float64) - r3) <= sos_bar(r3, B4, x3.cpu().numpy(), None, True)).all()
