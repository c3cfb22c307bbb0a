"""GPU tests of the int16 moving-average kernels at the ends of the int16 range (tests/i16_range.py:
constant 32767 / -32768, the bands just inside them, blocks that sweep the window sum over the whole
of [-32768 k, 32767 k], and stairs that put it on every quotient boundary), on every path the int16
dispatch has.  Seeded noise keeps a window sum near sqrt(k) * 19000: the int32 prefix differences mod
2^32, the halo sums, segment totals and look-ahead records never come near a wrap on it, the high word
of an int64 record is a sign extension, and the output division sees small dividends only.

Every output is compared bit for bit with oracle.mavg_i16 (per channel, per row, or sliced for the
decimated forms); the moments with tests/stat_ref.py's exact-integer reference.  Signals are three
tiles plus 17 frames, tile_frames read from the plan text (6161 frames where there is no tile), or
what the signal needs if that is more (i16_range.frames_needed).  Every case asserts the plan token
of the path it names, launches into guard regions and checks that the input came back unmodified.

tests/test_i16_range_refs.py shows on the CPU that the oracle and an independent numpy formulation
agree on these signals and that the signals reach the sums they are for; tests/test_division.py
models both output divisions (dv=0: the fp64 product, dv=1: the magic multiply)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import i16_range as R
import stat_ref
import test_gpu_stat as S
from stat_ref import MEANSQ, RMS, STD, VAR
from test_gpu_fp32_range import by_rule, forced

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBUG_LIB = os.path.join(ROOT, "digital_signal_processsing_amd", "lib", "libmavg_debug.so")
GUARD = 12345               # no output here is 12345 next to a guard by chance: the guards are checked as regions
FGUARD = 7.0


def _dsp():
    import digital_signal_processsing_amd as dsp
    return dsp


def tile_of(plan):
    return int(plan.split(" tile_frames=")[1].split()[0]) if " tile_frames=" in plan else None


def guarded(dev, x, n_out, fn, off_in=0, off_out=0, in_shape=None, out_shape=None):
    """fn(x view, out view) on int16 views `off_*` samples into larger buffers; nothing outside the
    output view may be written and the input must come back as it went in.  Returns the output, flat."""
    import torch
    xbuf = torch.zeros(x.size + 16, dtype=torch.int16, device=dev)
    ybuf = torch.full((n_out + 16,), GUARD, dtype=torch.int16, device=dev)
    xv, yv = xbuf[off_in:off_in + x.size], ybuf[off_out:off_out + n_out]
    xv.copy_(torch.from_numpy(np.array(x)))
    assert xbuf.data_ptr() % 16 == 0 and ybuf.data_ptr() % 16 == 0
    fn(xv.view(in_shape) if in_shape else xv, yv.view(out_shape) if out_shape else yv)
    torch.cuda.synchronize()
    yb = ybuf.cpu().numpy()
    assert (yb[:off_out] == GUARD).all() and (yb[off_out + n_out:] == GUARD).all(), "written outside the output view"
    assert np.array_equal(xv.cpu().numpy(), x), "the input was modified"
    return yb[off_out:off_out + n_out].copy()


def assert_same(y, ref, what):
    bad = np.flatnonzero(y != ref)
    assert bad.size == 0, (what, int(bad.size), bad[:6].tolist(), y[bad[:6]].tolist(), ref[bad[:6]].tolist())


# ---- mavg_run ----
MAX = "max"     # the largest grade the path's dispatch takes, found from the plan text
RUN_CASES = [  # id, algo, C, offset of both views in samples, plan tokens, windows
    ("blelloch", "blelloch", 1, 0, ("tile_scan<", ",F=8,", ",blelloch,", "acc=i32"), (2, 255, 256, 257, MAX)),
    ("blelloch-C2", "blelloch", 2, 0, ("tile_scan<", ",F=4,", ",blelloch,", "acc=i32"), (2, 255, 256, 257, MAX)),
    ("blelloch_scalar", "blelloch_scalar", 1, 0, ("tile_scan<", ",F=1,", ",blelloch,", "acc=i32"), (2, 255, 256, 257, MAX)),
    ("hillis", "hillis", 1, 0, ("tile_scan<", ",F=8,", ",hillis,", "acc=i32"), (2, 255, 256, 257, MAX)),
    ("hillis-C2", "hillis", 2, 0, ("tile_scan<", ",F=4,", ",hillis,", "acc=i32"), (2, 257, MAX)),
    ("hillis_scalar", "hillis_scalar", 1, 0, ("tile_scan<", ",F=1,", ",hillis,", "acc=i32"), (2, 255, 256, 257, MAX)),
    # one sample off alignment, both views alike: the head peel, then the 16-B body.  mavg_plan is not told the
    # alignment, so these cases (and test_frame_unit_form_on_misaligned_views) can assert the kernel family only
    ("blelloch-peel", "blelloch", 1, 1, ("tile_scan<", ",blelloch,", "acc=i32"), (2, 255, 256, 257, MAX)),
    ("blelloch-peel-C2", "blelloch", 2, 1, ("tile_scan<", ",blelloch,", "acc=i32"), (2, 257, MAX)),
    ("direct", "direct", 1, 0, ("direct<", ",F=8,", "acc=i32"), (2, 255, 256, 257, MAX)),
    ("direct-C2", "direct", 2, 0, ("direct<", ",F=4,", "acc=i32"), (2, 257, MAX)),
    ("direct_vec2", "direct_vec2", 1, 0, ("direct<", ",F=4,", "acc=i32"), (2, 255, 256, 257, MAX)),
    ("direct_scalar", "direct_scalar", 1, 0, ("direct<", ",F=1,", "acc=i32"), (2, 255, 256, 257, MAX)),
    ("naive", "naive", 1, 0, ("naive<", "acc=i32"), (2, 255, 256, 257)),
    ("naive-C2", "naive", 2, 0, ("naive<", "acc=i32"), (2, 257)),
    ("ahead-i32", "auto", 1, 0, ("ahead_scan<", "acc=i32"), (32767, 32768, 65535)),
    ("ahead-i32-C2", "auto", 2, 0, ("ahead_scan<", "acc=i32"), (32767, 32768, 65535)),
    ("ahead-i64", "auto", 1, 0, ("ahead_scan<", "acc=i64"), (65536, 65537)),
    ("ahead-i64-C2", "auto", 2, 0, ("ahead_scan<", "acc=i64"), (65536, 65537)),
    ("hillis-records", "hillis", 1, 0, ("ahead_scan<", ",hillis,", "acc=i32"), (44100, 65535)),
    ("hillis-records-C2", "hillis", 2, 0, ("ahead_scan<", ",hillis,", "acc=i32"), (44100, 65535)),
    ("wide-C4", "auto", 4, 0, ("wide_tile<", "acc=i32"), (2, 257, MAX)),
    ("wide-C8", "auto", 8, 0, ("wide_tile<", "acc=i32"), (2, 257, MAX)),
    # past the wide tile.  Four channels: the wide look-ahead for 4096 < k <= 8192 (int32 records only: there is
    # no int16 C = 4 wide_ahead with int64 sums), the unit look-ahead scan past it.  Eight: the wide look-ahead.
    ("wide-ahead-C4", "auto", 4, 0, ("wide_ahead<", "acc=i32", "C=4,"), (4097, 8192)),
    ("long-C4-i32", "auto", 4, 0, ("ahead_scan<", "acc=i32"), (44100,)),
    ("long-C4-i64", "auto", 4, 0, ("ahead_scan<", "acc=i64"), (70000,)),
    ("wide-ahead-i32", "auto", 8, 0, ("wide_ahead<", "acc=i32"), (44100,)),
    ("wide-ahead-i64", "auto", 8, 0, ("wide_ahead<", "acc=i64"), (70000,)),
]
HISTORY_CASES = [  # one per kernel shape: id, algo, C, plan tokens, window
    ("tile_scan", "blelloch", 1, ("tile_scan<", ",blelloch,"), 257),
    ("tile_scan-hillis", "hillis", 2, ("tile_scan<", ",hillis,"), 257),
    ("direct", "direct", 1, ("direct<",), 257),
    ("naive", "naive", 2, ("naive<",), 255),
    ("ahead_scan", "auto", 2, ("ahead_scan<", "acc=i32"), 44100),
    ("ahead_scan-i64", "auto", 1, ("ahead_scan<", "acc=i64"), 65536),
    ("hillis-records", "hillis", 1, ("ahead_scan<", ",hillis,"), 44100),
    ("wide_tile", "auto", 4, ("wide_tile<",), 257),
    ("wide_ahead", "auto", 8, ("wide_ahead<",), 44100),
    ("wide_ahead-C4", "auto", 4, ("wide_ahead<", "C=4,"), 8192),
]


def run_plan(C, k, algo, tokens, frames=1 << 20):
    dsp = _dsp()
    plan = dsp.plan(frames * C, k, C, dsp.I16, algo)
    assert plan.startswith(tokens[0]) and all(t in plan for t in tokens), (k, tokens, plan)
    return plan


def takes(C, k, algo, tokens):
    dsp = _dsp()
    from digital_signal_processsing_amd import _lib
    try:
        plan = dsp.plan((1 << 20) * C, k, C, dsp.I16, algo)
    except _lib.MavgError as e:       # past the direct kernels' LDS halo the plan is refused; anything else is an error
        if e.status != _lib.ERR_UNSUPPORTED:
            raise
        return False
    return plan.startswith(tokens[0]) and all(t in plan for t in tokens)


def largest_window(C, algo, tokens):
    """The largest grade up to 65535 at which (algo, C) still runs the kernel `tokens` name, by
    bisection on the plan text (no launch), as test_gpu_parity's test_dispatch_boundaries finds its windows."""
    lo, hi = 257, 65536
    assert takes(C, lo, algo, tokens) and not takes(C, hi, algo, tokens), (algo, C, tokens)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if takes(C, mid, algo, tokens) else (lo, mid)
    return lo


def windows_of(case):
    name, algo, C, off, tokens, ks = case
    return [largest_window(C, algo, tokens) if k == MAX else k for k in ks]


def run_frames(C, k, algo, tokens):
    """The signal length of a case: settled when the plan at that length names the same tile."""
    frames = R.frames_for(k, tile_of(run_plan(C, k, algo, tokens)))
    again = R.frames_for(k, tile_of(run_plan(C, k, algo, tokens, frames)))
    return max(frames, again)


@pytest.mark.parametrize("case", RUN_CASES, ids=[c[0] for c in RUN_CASES])
def test_mavg_run(gpu, oracle_mod, case):
    name, algo, C, off, tokens, _ = case
    dsp = _dsp()
    for k in windows_of(case):
        frames = run_frames(C, k, algo, tokens)
        run_plan(C, k, algo, tokens, frames)
        for sname in R.NAMES:
            x = R.signal(oracle_mod, sname, k, frames, C)
            y = guarded(gpu, x, x.size, lambda xv, yv: dsp.moving_average_into(xv, yv, k, C, algo), off, off)
            assert_same(y, oracle_mod.mavg_i16(x, k, C), (name, k, sname))
            if sname == "stairs":
                R.assert_stairs_change_once(y.reshape(-1, C)[:, 0], k, name)


def test_frame_unit_form_on_misaligned_views(gpu, oracle_mod):
    """Input one sample off alignment into an aligned output: no common peel, the frame-unit form."""
    dsp = _dsp()
    for C in (1, 2):
        for k in (2, 257, largest_window(C, "blelloch", ("tile_scan<",))):
            frames = run_frames(C, k, "blelloch", ("tile_scan<",))
            for sname in R.NAMES:
                x = R.signal(oracle_mod, sname, k, frames, C)
                y = guarded(gpu, x, x.size, lambda xv, yv: dsp.moving_average_into(xv, yv, k, C, "blelloch"), 1, 0)
                assert_same(y, oracle_mod.mavg_i16(x, k, C), ("frame-unit", C, k, sname))


@pytest.mark.parametrize("case", HISTORY_CASES, ids=[c[0] for c in HISTORY_CASES])
def test_mavg_run_with_a_history(gpu, oracle_mod, case):
    """d_history = bottom-band: the window is at its extreme at frame 0.  Every signal follows it."""
    import torch
    name, algo, C, tokens, k = case
    dsp = _dsp()
    frames = run_frames(C, k, algo, tokens)
    hist = R.signal(oracle_mod, "bottom-band", k, k - 1, C, seed=5)
    ht = torch.from_numpy(np.array(hist)).to(gpu)
    for sname in R.NAMES:
        x = R.signal(oracle_mod, sname, k, frames, C)
        y = guarded(gpu, x, x.size, lambda xv, yv: dsp.moving_average_into(xv, yv, k, C, algo, history=ht))
        ref = oracle_mod.mavg_i16(np.concatenate([hist, x]), k, C)[(k - 1) * C:]
        assert_same(y, ref, (name, k, sname, "history"))
        assert np.array_equal(ht.cpu().numpy(), hist), "the history was modified"
        if sname == "bottom-band":      # bottom-band after bottom-band: the first output is already within 15 of -32768
            assert (y.reshape(-1, C)[0, 0::2] <= R.BOTTOM + 15).all() and (y.reshape(-1, C)[0, 1::2] >= R.TOP - 15).all()


def test_both_output_divisions_are_covered():
    """dv=0 (the fp64 product) and dv=1 (the magic multiply) both occur among the plans of the cases above."""
    seen = set()
    for case in RUN_CASES:
        name, algo, C, off, tokens, _ = case
        for k in windows_of(case):
            plan = run_plan(C, k, algo, tokens)
            if "dv=" in plan:
                seen.add((plan.split("<")[0], plan.split("dv=")[1][0]))
    assert {d for _, d in seen} == {"0", "1"}, seen
    assert ("tile_scan", "1") in seen and ("ahead_scan", "0") in seen and ("wide_tile", "0") in seen, seen


# ---- mavg_rows_run and mavg_ragged_run ----
ROWS = 5
SEG_CASES = [(1, 8192, True), (1, 257, False), (2, 4096, True)]        # C, window, at the 16-KiB halo limit


def rows_length(plan_at, k):
    """Row frames: every signal fits its needs into the batch, rows start inside tiles."""
    tile = tile_of(plan_at(1 << 14))
    L = max((3 * tile + 17) // ROWS + 1, -(-max(R.frames_needed(n, k) for n in R.NAMES) // ROWS))
    while L % tile == 0 or (ROWS * L) % tile == 0:
        L += 1
    return L


@pytest.mark.parametrize("C,k,limit", SEG_CASES)
def test_mavg_rows_run(gpu, oracle_mod, C, k, limit):
    dsp = _dsp()
    L = rows_length(lambda n: dsp.rows_plan(ROWS, n, k, C, dsp.I16), k)
    plan = dsp.rows_plan(ROWS, L, k, C, dsp.I16)
    assert plan.startswith("rows_scan<") and "acc=i32" in plan and f" window={k} " in plan, plan
    if limit:
        assert not dsp.rows_plan(ROWS, L, k + 1, C, dsp.I16).startswith("rows_scan<")
    shape = (ROWS, L) if C == 1 else (ROWS, L, C)
    for sname in R.NAMES:
        x = R.signal(oracle_mod, sname, k, ROWS * L, C)
        y = guarded(gpu, x, x.size, lambda xv, yv: dsp.moving_average_rows_into(xv, yv, k, channels=C),
                    in_shape=shape, out_shape=shape)
        ref = np.concatenate([oracle_mod.mavg_i16(r, k, C) for r in x.reshape(ROWS, L * C)])
        assert_same(y, ref, ("rows_scan", C, k, sname))


@pytest.mark.parametrize("C,k,limit", SEG_CASES)
def test_mavg_ragged_run(gpu, oracle_mod, C, k, limit):
    dsp = _dsp()
    frames = ROWS * rows_length(lambda n: dsp.ragged_plan([0, n], k, C, dsp.I16), k)
    lengths = [frames // 3 + 1, 0, 5, k - 1]         # an empty row, rows shorter than the window, two long ones
    lengths.append(frames - sum(lengths))
    assert lengths[0] > k and lengths[-1] > k
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    plan = dsp.ragged_plan(offs, k, C, dsp.I16)
    assert plan.startswith("ragged_scan<") and "acc=i32" in plan and f" window={k} " in plan, plan
    if limit:
        assert not dsp.ragged_plan(offs, k + 1, C, dsp.I16).startswith("ragged_scan<")
    shape = (frames,) if C == 1 else (frames, C)
    for sname in R.NAMES:
        x = R.signal(oracle_mod, sname, k, frames, C)
        y = guarded(gpu, x, x.size, lambda xv, yv: dsp.moving_average_ragged_into(xv, yv, k, lengths=lengths, channels=C),
                    in_shape=shape, out_shape=shape)
        ref = np.concatenate([oracle_mod.mavg_i16(x[a * C:b * C], k, C) for a, b in zip(offs[:-1], offs[1:]) if b > a])
        assert_same(y, ref, ("ragged_scan", C, k, sname))


# ---- mavg_decim_run: the three paths forced on one shape, and the scan at its 8-KiB limit ----
DECIM_CASES = [("DECIM_SCAN", "decim_scan<", 100), ("DECIM_WINDOW", "decim_window<", 100), ("DECIM_FULL", "decim_full ", 100),
               (None, "decim_scan<", 4096)]


@pytest.mark.parametrize("path,token,k", DECIM_CASES, ids=["scan", "window", "full", "scan-limit"])
def test_mavg_decim_run(gpu, oracle_mod, path, token, k):
    from digital_signal_processsing_amd import _lib
    dsp = _dsp()
    hop, phase, C = 7, 3, 1
    scan = dsp.decim_plan(1 << 20, k, hop, phase, C, dsp.I16)
    assert scan.startswith("decim_scan<") and "acc=i32" in scan, scan
    if path is None:
        assert not dsp.decim_plan(1 << 20, k + 1, hop, phase, C, dsp.I16).startswith("decim_scan<")
    frames = R.frames_for(k, tile_of(scan))
    M = len(range(phase, frames, hop))
    with (forced("decim", getattr(_lib, path)) if path else by_rule()) as lib:
        assert dsp.decim_plan(frames, k, hop, phase, C, dsp.I16, lib).startswith(token)
        for sname in R.NAMES:
            x = R.signal(oracle_mod, sname, k, frames, C)
            y = guarded(gpu, x, M, lambda xv, yv: dsp.moving_average_decimated_into(xv, yv, k, hop, phase, C, library=lib))
            assert_same(y, oracle_mod.mavg_i16(x, k, C)[phase::hop], (token, k, sname))


# ---- mavg_stat_run on int16: the tile by the rule, the strip forced on the same shapes ----
STAT_SIGNALS = ("top", "bottom", "blocks", "top-band")
STAT_NAMES = {MEANSQ: "meansq", RMS: "rms", VAR: "var", STD: "std"}


def stat_launch(dev, x, k, stat, C, family, library=None):
    """moving_stat_into with d_mean, both outputs inside guard regions; (y, mean) as [frames, C]."""
    import torch
    dsp = _dsp()
    n = x.size
    plan = dsp.stat_plan(n, k, stat, C, dsp.I16, True, library)
    assert plan.startswith(family), (family, plan)
    xt = torch.from_numpy(np.array(x)).to(dev)
    ybuf = torch.full((n + 8,), FGUARD, dtype=torch.float32, device=dev)
    mbuf = torch.full((n + 8,), FGUARD, dtype=torch.float32, device=dev)
    dsp.moving_stat_into(xt, ybuf[4:4 + n], k, stat, C, mean_out=mbuf[4:4 + n], library=library)
    torch.cuda.synchronize()
    yb, mb = ybuf.cpu().numpy(), mbuf.cpu().numpy()
    for b, what in ((yb, "d_out"), (mb, "d_mean")):
        assert (b[:4] == FGUARD).all() and (b[4 + n:] == FGUARD).all(), ("written outside " + what, plan)
    assert np.array_equal(xt.cpu().numpy(), x), "the input was modified"
    return yb[4:4 + n].reshape(-1, C).copy(), mb[4:4 + n].reshape(-1, C).copy()


@pytest.mark.parametrize("C", (1, 2))
@pytest.mark.parametrize("k", (2, 16, 17, "limit"))
def test_mavg_stat_run(gpu, oracle_mod, C, k):
    k = S.rule_boundary("i16", C) if k == "limit" else k
    dsp = _dsp()
    frames = max(S.three_tiles("i16", C, k), 4 * k + 17)
    assert not dsp.stat_plan(frames * C, S.rule_boundary("i16", C) + 1, VAR, C, dsp.I16, True).startswith(S.TILE)
    for sname in STAT_SIGNALS:
        x = R.signal(oracle_mod, sname, k, frames, C)
        for stat in (MEANSQ, RMS, VAR, STD):
            what = (sname, C, k, STAT_NAMES[stat])
            y, mean = stat_launch(gpu, x, k, stat, C, S.TILE)
            with S.forced_strip() as lib:
                ys, means = stat_launch(gpu, x, k, stat, C, S.STRIP, library=lib)
            assert y.tobytes() == ys.tobytes() and mean.tobytes() == means.tobytes(), (what, "tile and strip differ")
            ref, mref = stat_ref.stat_ref_i16(x, k, stat, C)
            stat_ref.check_i16(y, ref, what)
            stat_ref.check_i16(mean, mref, (what, "mean"))
            if sname in ("top", "bottom"):
                const = x.reshape(-1, C)[0].astype(np.float32)
                assert (mean[k - 1:] == const).all(), (what, "the mean of a constant")
                if stat in (VAR, STD):
                    assert (y[k - 1:] == 0.0).all(), (what, "a constant's variance")
                if stat == RMS:
                    assert (y[k - 1:] == np.abs(const)).all(), what


# ---- the debug build: three representative cases under its device bounds checks ----
def run_debug_cases(dev, oracle):
    """tile_scan, ahead_scan and rows_scan on blocks and bottom-band; MAVG_LIBRARY names the library."""
    dsp = _dsp()
    n = 0
    for C, k, algo, tokens in ((1, 257, "blelloch", ("tile_scan<",)), (2, 44100, "auto", ("ahead_scan<",))):
        frames = run_frames(C, k, algo, tokens)
        for sname in ("blocks", "bottom-band"):
            x = R.signal(oracle, sname, k, frames, C)
            y = guarded(dev, x, x.size, lambda xv, yv: dsp.moving_average_into(xv, yv, k, C, algo))
            assert_same(y, oracle.mavg_i16(x, k, C), ("debug", tokens, sname))
            n += 1
    C, k = 1, 8192
    L = rows_length(lambda m: dsp.rows_plan(ROWS, m, k, C, dsp.I16), k)
    assert dsp.rows_plan(ROWS, L, k, C, dsp.I16).startswith("rows_scan<")
    for sname in ("blocks", "bottom-band"):
        x = R.signal(oracle, sname, k, ROWS * L, C)
        y = guarded(dev, x, x.size, lambda xv, yv: dsp.moving_average_rows_into(xv, yv, k, channels=C),
                    in_shape=(ROWS, L), out_shape=(ROWS, L))
        assert_same(y, np.concatenate([oracle.mavg_i16(r, k, C) for r in x.reshape(ROWS, L)]), ("debug", "rows_scan", sname))
        n += 1
    return n


CHILD = r'''
import sys
sys.path.insert(0, "tests")
import torch
import oracle
import test_gpu_i16_range as t
from digital_signal_processsing_amd import _lib
oracle.build()
_lib.load()
maps = open("/proc/self/maps").read()
assert "libmavg_debug.so" in maps and "lib/libmavg.so" not in maps, "the debug build must be the one loaded"
n = t.run_debug_cases(torch.device("cuda:0"), oracle)
torch.cuda.synchronize()
print("i16 range debug build ok", n)
'''


@pytest.mark.timeout(200)
def test_debug_build_runs_full_scale_cases_clean(gpu):
    """A firing device check traps the kernel and the child fails; every output matches the oracle."""
    r = subprocess.run([sys.executable, "-u", "-c", CHILD], cwd=ROOT, env=dict(os.environ, MAVG_LIBRARY=DEBUG_LIB),
                       capture_output=True, text=True, timeout=170)
    assert r.returncode == 0 and "i16 range debug build ok 6" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert "mavg debug check failed" not in r.stdout + r.stderr
