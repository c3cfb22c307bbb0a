"""Parity past 2^31 and 2^32 samples: one signal of 2^32 + ~10^6 samples per
kernel family the dispatch can reach, every output checked.

F = 2^32 // C + 1_000_003 frames (a prime-length ragged tail), n = F * C
samples: the smallest shape at which an unsigned 32-bit sample index wraps; it
also crosses the signed 2^31 sample index and, for both dtypes, byte offsets of
2^32 and beyond (C = 1: frame and sample index cross together; C = 8: only the
sample index).  Each case checks
  1. every output on the device against the plain-torch exact window sums
     (tests/bigsignal_ref.py, pinned to the C oracle by test_bigsignal_ref.py);
  2. four 2^17-sample windows (first, around sample 2^31, around 2^32, the
     tail) against the C oracle, which regenerates the input from its counter:
     independent of torch and of the device generator;
  3. 4096-sample guard bands before and after the output view: unchanged;
  4. the input: unchanged (a device checksum before and after).
A whole signal is never copied to the host.  int16: bit-exact.  fp32: the
input is int16-valued (generator dist 0), every window sum exact, so the output
must be the correctly rounded quotient bit for bit (max_rel == 0.0).

The launchers built on mavg_run -- mavg_decim_run, mavg_cascade_run and
mavg_stat_run -- run the same signal through the same checks, one case per
dispatch path and unit form (second half of this file): every output through
chunked_decim / cascade / stat_mismatches, three host windows (head, around
input sample 2^32, tail) through the small suites' own references (the oracle
sliced, the oracle applied `passes` times, tests/stat_ref.py), guard bands
around every output view (d_out and d_mean), the input checksum, and for the
decimated output its exact length.

The filters with kernels of their own -- extrema, EMA, biquad, FIR -- run the
same signal through the same checks in tests/test_gpu_bigsignal_filters.py,
which imports this file's helpers.

A case holds 2 x 8.6 GB (int16) or 2 x 17.2 GB (fp32) plus < 5 GiB of chunk
temporaries (the second moment: the input and two fp32 views, up to 3 x 17.2
GB; the filters' cases: an fp32 output per int16 input, 8.6 + 17.2 GB, and at
most 3 x 17.2 GB for fp32 extrema with both outputs, plus up to 537 MB of
records; the cascade's loop cases: the int16 input, the fp32 output and one or two
fp32 buffers of the signal's size in the workspace, 8.6 + 2 x 17.2 GB and 8.6 +
3 x 17.2 GB = 60.2 GB), and skips only when the (shared) device has less than
that free."""
import pytest

from bigsignal_ref import chunked_mismatches

pytestmark = pytest.mark.gpu

SEED = 0x5EED
GUARD = 4096                 # sentinel samples on either side of the output view
CHUNK = 1 << 27              # samples per reference chunk (int64 temporaries: 1 GiB each)
WIN = 1 << 17                # samples per oracle window
SENT = {2: 0x5A5A, 4: 0x5A5A5A5A}   # sentinel bit pattern by sample size


def _sizes(C):
    F = 2 ** 32 // C + 1_000_003
    return F, F * C


def _bits(t):
    import torch
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _checksum(t):
    import torch
    return int(_bits(t).sum(dtype=torch.int64))


def _windows(n, C):
    """[a, b) of the four oracle windows: whole frames (a and b multiples of C;
    3 channels: 2^17 - 2 samples), the last one up to n."""
    w = WIN // C * C
    out = [(0, w)]
    for centre in (1 << 31, 1 << 32):
        a = (centre - WIN // 2) // C * C
        out.append((a, a + w))
    out.append(((n - WIN) // C * C, n))
    return out


def _check_plan(plan, want, tag):
    """want: the start of the plan, then tokens it must hold ("!token": must not)."""
    want = (want,) if isinstance(want, str) else want
    assert plan.startswith(want[0]), tag
    for tok in want[1:]:
        assert (tok[1:] not in plan) if tok.startswith("!") else (tok in plan), f"plan token {tok!r}: {tag}"


def _need(gpu, nbytes):
    import torch
    free = torch.cuda.mem_get_info(gpu)[0]
    if free < nbytes:
        pytest.skip(f"{free >> 30} GiB free on the device, this case needs {nbytes >> 30} GiB")


def _stream(gpu, dtype, n, hs=0, in_off=0, dist=0):
    """Samples [0, hs + n) of the synthetic stream on the device: (xall, x, hist) with x = xall[hs:]
    starting in_off samples past 16-B alignment and hist = xall[:hs] (None without one).  dist: the
    generator's distribution (fp32 only: 0 int16-valued, 2 the rounding-stress data)."""
    import torch
    import digital_signal_processsing_amd as dsp
    esz = torch.empty(0, dtype=dtype).element_size()
    pad = (in_off - hs) % (16 // esz)
    xall = torch.empty(pad + hs + n, dtype=dtype, device=gpu)[pad:]
    dsp.fill_synthetic(xall.numel(), seed=SEED, dist=dist, out=xall)
    x = xall[hs:]
    assert x.data_ptr() % 16 == (in_off * esz) % 16
    return xall, x, (xall[:hs] if hs else None)


def _guarded(gpu, dtype, n, lead=0, off=0):
    """A sentinel-filled buffer (stale results of an earlier case cannot pass) and its view yall of
    lead + n samples, GUARD samples and more from either end, with yall[lead:] starting off samples
    past 16-B alignment: (buffer, yall)."""
    import torch
    esz = torch.empty(0, dtype=dtype).element_size()
    assert (GUARD * esz) % 16 == 0
    pad = (off - lead) % (16 // esz)
    buf = torch.empty(GUARD + pad + lead + n + GUARD, dtype=dtype, device=gpu)
    _bits(buf).fill_(SENT[esz])
    yall = buf[GUARD + pad:GUARD + pad + lead + n]
    assert yall[lead:].data_ptr() % 16 == (off * esz) % 16
    return buf, yall


def _guards_intact(buf, yall, lead, name, tag):
    """Everything of buf outside yall[lead:] still holds the sentinel."""
    a = yall.storage_offset() + lead
    b = yall.storage_offset() + yall.numel()
    for side, band in (("before", buf[:a]), ("after", buf[b:])):
        assert band.numel() >= GUARD and bool((_bits(band) == SENT[buf.element_size()]).all()), \
            f"guard band {side} {name}: {tag}"


def _run(oracle_mod, gpu, dt, C, k, algo, want, in_off=0, out_off=0, history=False, tamper=None):
    """One launch at n = _sizes(C) and the four checks.  in_off / out_off:
    samples the views start past 16-B alignment.  history: the k-1 frames before
    x come from the same stream and are passed as history=.  tamper: called with
    the finished output before the device check (the sensitivity test); returns
    what chunked_mismatches must then report."""
    import torch
    import digital_signal_processsing_amd as dsp
    dtype, code = (torch.float32, dsp.F32) if dt == "f32" else (torch.int16, dsp.I16)
    esz = 4 if dt == "f32" else 2
    F, n = _sizes(C)
    plan = dsp.plan(n, k, C, code, algo)
    tag = f"{dt} C={C} k={k} {algo} n={n} in+{in_off} out+{out_off} history={history}: {plan}"
    print(tag)
    _check_plan(plan, want, tag)
    hs = (k - 1) * C if history else 0
    assert (hs * esz) % 16 == 0
    _need(gpu, 2 * (n + hs + 2 * GUARD) * esz + (5 << 30))
    ws_n = dsp.workspace_bytes(n, k, C, code, algo)
    if plan.startswith(("ahead_scan<", "wide_ahead<")):
        assert ws_n > 0 and " ws=" in plan, tag
    ws = torch.empty(ws_n, dtype=torch.uint8, device=gpu) if ws_n else None

    xall, x, hist = _stream(gpu, dtype, n, hs, in_off)
    ybuf, yall = _guarded(gpu, dtype, n, hs, out_off)     # yall is indexed like xall; the library writes yall[hs:]
    y = yall[hs:]
    before = _checksum(xall)

    dsp.moving_average_into(x, y, k, C, algo, history=hist, workspace=ws)
    torch.cuda.synchronize()

    try:
        # 4. the input (and the history) unchanged
        assert _checksum(xall) == before, tag
        # 3. guard bands (and, with history, the samples between band and view) unchanged
        _guards_intact(ybuf, yall, hs, "output", tag)
        # 2. oracle windows
        for a, b in _windows(n, C):
            r = oracle_mod.check_synth(y[a:b].cpu().numpy(), k, C, seed=SEED, offset=hs + a)
            print(f"  oracle [{a}, {b}): {r}")
            assert r["checked"] == b - a and r["mismatches"] == 0, f"[{a}, {b}) {r}: {tag}"
            if dt == "f32":
                assert r["max_rel"] == 0.0, f"[{a}, {b}) {r}: {tag}"
        # 1. every output
        expect = tamper(y, n) if tamper else (0, None)
        got = chunked_mismatches(xall, yall, k, C, CHUNK // C, first_frame=k - 1 if history else 0)
        if got[1] is not None:
            got = (got[0], got[1] - hs)   # as an index into y
        assert got == expect, f"(mismatches, first bad sample) = {got}: {tag}"
    finally:
        del x, hist, xall, y, yall, ybuf, ws
        torch.cuda.empty_cache()


# id, dtype, C, k, algo, plan at this n: (start of the plan: the kernel family and its unit shape,
# then the tokens of the sub-form the case is named for; "!token": must be absent).  A dispatch
# change that moves a case to another kernel or form fails here instead of passing under the old id.
FLAT_I16 = [
    ("i16_c1_k1024_blelloch", "i16", 1, 1024, "blelloch", ("tile_scan<i16,acc=i32,C=1,F=8,U=4,blelloch", "dma=0")),
    ("i16_c1_k1024_hillis", "i16", 1, 1024, "hillis", ("tile_scan<i16,acc=i32,C=1,F=8,U=4,hillis", "dma=0")),
    ("i16_c2_k1024_blelloch", "i16", 2, 1024, "blelloch", ("tile_scan<i16,acc=i32,C=2,F=4,U=4,blelloch", "dma=0")),
    ("i16_c3_k333_blelloch", "i16", 3, 333, "blelloch", ("tile_scan<i16,acc=i32,C=3,F=1,U=4,blelloch",)),
    ("i16_c8_k1024_blelloch", "i16", 8, 1024, "blelloch", ("wide_tile<i16,acc=i32,C=8,P=8,U=1",)),
    ("i16_c1_k64_hillis_scalar", "i16", 1, 64, "hillis_scalar", ("tile_scan<i16,acc=i32,C=1,F=1,U=4,hillis",)),
]
FLAT_F32 = [
    ("f32_c1_k1024_blelloch", "f32", 1, 1024, "blelloch", ("tile_scan<f32,acc=f64,C=1,F=4,U=2,blelloch", "dma=1")),
    ("f32_c1_k4096_blelloch", "f32", 1, 4096, "blelloch", ("tile_scan<f32,acc=f64,C=1,F=4,U=4,blelloch", "dma=1")),
    ("f32_c1_k64_blelloch_scalar", "f32", 1, 64, "blelloch_scalar", ("tile_scan<f32,acc=f64,C=1,F=1,U=2,blelloch",)),
    ("f32_c4_k1024_wide_tile", "f32", 4, 1024, "blelloch", ("wide_tile<f32,acc=f64,C=4,P=8,U=1",)),
    ("f32_c8_k1024_chan_tile", "f32", 8, 1024, "blelloch", ("chan_tile<f32,acc=f64,C=8,Q=32", ",xg=1>")),
    ("f32_c4_k2048_chan_tile_in_place", "f32", 4, 2048, "blelloch", ("chan_tile<f32,acc=f64,C=4,Q=32", ",xg=1,ip=1")),
]
AHEAD = [
    # per-wave records, self-published
    ("f32_c1_k8192_self_published", "f32", 1, 8192, "blelloch",
     ("ahead_scan<f32,acc=f64,C=1,F=4,U=4,blelloch", "wrec=1", " remap=1 ", " self=1 ", "!runs=1")),
    # per-wave records published ahead of the scan (not self-published)
    ("f32_c1_k44100", "f32", 1, 44100, "blelloch",
     ("ahead_scan<f32,acc=f64,C=1,F=4,U=4,blelloch", "wrec=1", " remap=1 ", "!self=1", "!runs=1")),
    # past the L2 reach: window-matched runs of 8192-frame tiles, one record per tile, no run totals
    ("f32_c1_k1000000_window_runs", "f32", 1, 1_000_000, "blelloch",
     ("ahead_scan<f32,acc=f64,C=1,F=4,U=8,blelloch", "wrec=0", "! remap=1 ", "!self=1", "!runs=1")),
    # a window of more than 1024 tiles: window-matched runs WITH run totals (the RUNS kernel, its
    # region of the workspace)
    ("f32_c1_k9000000_run_totals", "f32", 1, 9_000_000, "blelloch",
     ("ahead_scan<f32,acc=f64,C=1,F=4,U=4,blelloch", "wrec=0", "! remap=1 ", " runs=1 ")),
    ("f32_c1_k44100_hillis", "f32", 1, 44100, "hillis",
     ("ahead_scan<f32,acc=f64,C=1,F=4,U=4,hillis", "wrec=1", "!self=1")),
    ("i16_c2_k44100_aggregate_first", "i16", 2, 44100, "blelloch",
     ("ahead_scan<i16,acc=i32,C=2,F=4,U=8,blelloch", "wrec=0", " remap=1 ", " self=1 ")),
    ("i16_c1_k100000_int64_sums", "i16", 1, 100_000, "blelloch",
     ("ahead_scan<i16,acc=i64,C=1,F=8,U=8,blelloch", " self=1 ")),
    # channel-per-lane wide look-ahead, self-published, columns formed at once
    ("f32_c4_k44100_wide_ahead", "f32", 4, 44100, "blelloch",
     ("wide_ahead<f32,acc=f64,C=4,P=32,U=1", ",ch=1,xg=1,", ",xl=2>", " self=1 ")),
    # chunk form (no ch=1), int64 sums, a partial window (k mod tile_frames != 0)
    ("i16_c8_k70001_chunk_form", "i16", 8, 70_001, "blelloch",
     ("wide_ahead<i16,acc=i64,C=8,P=4,U=1", ",F=1,FU=4,mw=", "!ch=1", "!self=1", "tile_frames=1024 ")),
]
DIRECT = [
    ("f32_c1_k7_direct", "f32", 1, 7, "direct", ("direct<f32,acc=f64,C=1,F=4,U=2",)),
    ("i16_c2_k7_direct_vec2", "i16", 2, 7, "direct_vec2", ("direct<i16,acc=i32,C=2,F=2,U=2",)),
    ("i16_c1_k5_direct_scalar", "i16", 1, 5, "direct_scalar", ("direct<i16,acc=i32,C=1,F=1,U=2",)),
]
CASES = FLAT_I16 + FLAT_F32 + AHEAD + DIRECT


@pytest.mark.parametrize("name,dt,C,k,algo,want", CASES, ids=[c[0] for c in CASES])
def test_every_output_past_2p32_samples(oracle_mod, gpu, name, dt, C, k, algo, want):
    _run(oracle_mod, gpu, dt, C, k, algo, want)


def test_head_peel_and_body_one_sample_off_alignment(oracle_mod, gpu):
    """Both views 4 B past 16-B alignment: a 3-frame head in the frame-unit
    form, then the vector body with the head as the nearest part of its history."""
    _run(oracle_mod, gpu, "f32", 1, 1024, "blelloch", "tile_scan<f32,acc=f64,C=1,F=4,U=2,blelloch", in_off=1, out_off=1)


def test_frame_unit_form_on_views_with_different_offsets(oracle_mod, gpu):
    """Views 4 B and 8 B past alignment: blelloch runs its frame-unit form (the
    plan of blelloch_scalar at this n) over the whole signal."""
    import digital_signal_processsing_amd as dsp
    F, n = _sizes(1)
    scalar = dsp.plan(n, 1024, 1, dsp.F32, "blelloch_scalar")
    print("frame-unit form:", scalar)
    assert scalar.startswith("tile_scan<f32,acc=f64,C=1,F=1,U=2,blelloch"), scalar
    _run(oracle_mod, gpu, "f32", 1, 1024, "blelloch", "tile_scan<f32,acc=f64,C=1,F=4,U=2,blelloch", in_off=1, out_off=2)


def test_history_precedes_the_signal(oracle_mod, gpu):
    """int16 stereo k = 705 with history=: one stream of (k-1)*C + n samples,
    the first 2816 B the history (x stays 16-B aligned); every output compared
    from frame k-1 of the whole stream on."""
    _run(oracle_mod, gpu, "i16", 2, 705, "blelloch", "tile_scan<i16,acc=i32,C=2,F=4,U=4,blelloch", history=True)


def test_reference_sees_past_2p32(oracle_mod, gpu):
    """Sensitivity of check 1: one flipped bit at sample 2^32 + 5 and one at
    n - 1 of a correct output are both counted, the first one located."""
    def tamper(y, n):
        for i in (2 ** 32 + 5, n - 1):
            _bits(y)[i:i + 1] ^= 1
        return (2, 2 ** 32 + 5)
    _run(oracle_mod, gpu, "i16", 1, 1024, "blelloch", "tile_scan<i16,acc=i32,C=1,F=8,U=4,blelloch", tamper=tamper)


def test_naive_one_thread_per_sample(oracle_mod, gpu):
    """n work-items in all, more than one launch holds (2^32 - 1).  As a single
    launch the runtime took the grid with its work-item count wrapped to
    n mod 2^32 and returned success: outputs from sample 1_000_192 on were never
    written (and at exactly 2^32 samples the launch was refused)."""
    _run(oracle_mod, gpu, "i16", 1, 3, "naive", ("naive<i16,acc=i32>", " launches=3"))


def test_identity_flat_copy(oracle_mod, gpu):
    """k = 1 on 16-B-aligned views of a whole number of 16-B units (fp32, 4 channels)."""
    _run(oracle_mod, gpu, "f32", 4, 1, "blelloch", ("copy<f32,C=4>", "flat nt 16-B", "!launches="))


def test_identity_on_views_one_sample_off_alignment(oracle_mod, gpu):
    """k = 1 on views 4 B past alignment: hipMemcpyAsync."""
    _run(oracle_mod, gpu, "f32", 1, 1, "blelloch", ("copy<f32,C=1>", "hipMemcpyAsync"), in_off=1, out_off=1)


def test_flat_copy_past_one_launch(gpu):
    """The flat copy (mavg_stream_copy, and k = 1 on aligned views) over
    2^31 + 1_000_003 16-B units, 32 GiB and a ragged tail: more work-items than
    the 2^31 of one launch, so two launches, the second from its own offset.
    Every byte compared on the device; guard bands around the destination."""
    import torch
    import digital_signal_processsing_amd as dsp
    units = (1 << 31) + 1_000_003
    n = units * 4                                  # fp32 samples, 4 per unit (as 4-channel frames)
    plan = dsp.plan(n, 1, 4, dsp.F32)
    print(plan)
    assert plan.startswith("copy<f32,C=4>") and "flat nt 16-B launches=2" in plan, plan
    need = 2 * (n + 2 * GUARD) * 4 + (2 << 30)
    free = torch.cuda.mem_get_info(gpu)[0]
    if free < need:
        pytest.skip(f"{free >> 30} GiB free on the device, this case needs {need >> 30} GiB")
    x = dsp.fill_synthetic(n, torch.float32, seed=SEED, device=gpu)
    ybuf = torch.empty(GUARD + n + GUARD, dtype=torch.float32, device=gpu)
    y = ybuf[GUARD:GUARD + n]
    before = _checksum(x)
    try:
        for name, copy in (("mavg_stream_copy", lambda: dsp.stream_copy(x, y)),
                           ("k = 1", lambda: dsp.moving_average_into(x, y, 1, 4))):
            _bits(ybuf).fill_(SENT[4])
            copy()
            torch.cuda.synchronize()
            bad, first = 0, None
            for a in range(0, n, CHUNK):            # bit patterns, 2^27 samples at a time
                ne = _bits(x[a:a + CHUNK]) != _bits(y[a:a + CHUNK])
                c = int(ne.sum())
                if c and first is None:
                    first = a + int(ne.nonzero()[0, 0])
                bad += c
            assert (bad, first) == (0, None), f"{name}: (differing samples, first) = {(bad, first)}"
            for band in (ybuf[:GUARD], ybuf[GUARD + n:]):
                assert bool((_bits(band) == SENT[4]).all()), name
            assert _checksum(x) == before, name
    finally:
        del x, y, ybuf
        torch.cuda.empty_cache()


# ---- the launchers built on the moving average: decimated, cascaded, second moment ----
# The same signal, the same four checks; every output goes through the matching reference of
# tests/bigsignal_ref.py, and three windows of up to 2^17 outputs (head, around input sample 2^32,
# tail) through the small suites' own host references on input the oracle regenerates.
STAT_CHUNK = 1 << 26          # the second moment keeps more temporaries per chunk frame
HOST_IN = 1 << 24             # input samples a host window may need (decimated: hop per output)


def _dt(dt):
    import torch
    import digital_signal_processsing_amd as dsp
    return (torch.float32, dsp.F32, 4) if dt == "f32" else (torch.int16, dsp.I16, 2)


def _out_windows(frames, centre, wf):
    """[a, b) in output frames: the first wf, wf around `centre`, the last wf."""
    wf = min(wf, frames)
    mid = min(max(centre - wf // 2, 0), frames - wf)
    return [(0, wf), (mid, mid + wf), (frames - wf, frames)]


def _host_slice(oracle_mod, dt, C, f_lo, f_hi, lead, dist=0):
    """Stream frames [max(0, f_lo - lead), f_hi) regenerated on the host, and the frames in front of f_lo."""
    start = max(0, f_lo - lead)
    n = (f_hi - start) * C
    xs = oracle_mod.synth_i16(n, seed=SEED, offset=start * C) if dt == "i16" else \
        oracle_mod.synth_f32(n, seed=SEED, offset=start * C, dist=dist)
    return xs, f_lo - start


def _same_bits(a, b):
    import numpy as np
    return a.shape == b.shape and np.array_equal(a.view(np.int16 if a.dtype == np.int16 else np.int32),
                                                 b.view(np.int16 if b.dtype == np.int16 else np.int32))


def _run_decim(oracle_mod, gpu, dt, C, k, hop, phase, want, in_off=0, history=False, tamper=None):
    import torch
    import digital_signal_processsing_amd as dsp
    from bigsignal_ref import chunked_decim_mismatches
    dtype, code, esz = _dt(dt)
    F, n = _sizes(C)
    M = len(range(phase, F, hop))
    plan = dsp.decim_plan(n, k, hop, phase, C, code)
    tag = f"decim {dt} C={C} k={k} hop={hop} phase={phase} n={n} in+{in_off} history={history}: {plan}"
    print(tag)
    _check_plan(plan, want, tag)
    assert dsp.decim_out_frames(F, hop, phase) == M, tag
    assert plan.startswith("decim_full ") or f" out_frames={M} " in plan, tag
    hf = k - 1 if history else 0
    ws_n = dsp.decim_workspace_bytes(n, k, hop, phase, C, code)
    assert (ws_n >= n * esz) == plan.startswith("decim_full "), tag
    _need(gpu, (n + hf * C + M * C + 2 * GUARD) * esz + ws_n + (5 << 30))
    ws = torch.empty(ws_n, dtype=torch.uint8, device=gpu) if ws_n else None
    xall, x, hist = _stream(gpu, dtype, n, hf * C, in_off)
    ybuf, y = _guarded(gpu, dtype, M * C)
    before = _checksum(xall)

    dsp.moving_average_decimated_into(x, y, k, hop, phase, C, history=hist, workspace=ws)
    torch.cuda.synchronize()

    try:
        assert _checksum(xall) == before, tag
        assert y.numel() == M * C
        _guards_intact(ybuf, y, 0, "output", tag)         # exactly M frames: nothing behind the last one
        wf = min(WIN // C, max(1, HOST_IN // (hop * C)))
        for ma, mb in _out_windows(M, (2 ** 32 // C - phase) // hop, wf):
            g0 = hf + phase + ma * hop                    # stream frame of output frame ma
            xs, lead = _host_slice(oracle_mod, dt, C, g0, hf + phase + (mb - 1) * hop + 1, k - 1)
            full = (oracle_mod.mavg_i16 if dt == "i16" else oracle_mod.mavg_f32)(xs, k, C).reshape(-1, C)
            ref = full[lead::hop].reshape(-1)
            ok = _same_bits(y[ma * C:mb * C].cpu().numpy(), ref)
            print(f"  host frames [{ma}, {mb}) of {M}: {'equal' if ok else 'DIFFERENT'}")
            assert ok, f"[{ma}, {mb}): {tag}"
        expect = tamper(y, M * C) if tamper else (0, None)
        got = chunked_decim_mismatches(xall, y, k, C, hop, phase, CHUNK // C, first_frame=hf)
        assert got == expect, f"(mismatches, first bad sample) = {got}: {tag}"
    finally:
        del x, hist, xall, y, ybuf, ws
        torch.cuda.empty_cache()


def _run_cascade(oracle_mod, gpu, dt, C, k, passes, want, in_off=0, out_off=0, history=False, tamper=None):
    import torch
    import digital_signal_processsing_amd as dsp
    from bigsignal_ref import chunked_cascade_mismatches
    dtype, code, esz = _dt(dt)
    F, n = _sizes(C)
    plan = dsp.cascade_plan(n, k, passes, C, code, history)
    tag = f"cascade {dt} C={C} k={k} passes={passes} n={n} in+{in_off} out+{out_off} history={history}: {plan}"
    print(tag)
    _check_plan(plan, want, tag)
    hf = passes * (k - 1) if history else 0
    ws_n = dsp.cascade_workspace_bytes(n, k, passes, C, code, history)
    assert (ws_n >= n * esz) == plan.startswith("cascade_loop "), tag
    _need(gpu, 2 * (n + hf * C + 2 * GUARD) * esz + ws_n + (5 << 30))
    ws = torch.empty(ws_n, dtype=torch.uint8, device=gpu) if ws_n else None
    xall, x, hist = _stream(gpu, dtype, n, hf * C, in_off)
    ybuf, yall = _guarded(gpu, dtype, n, hf * C, out_off)
    y = yall[hf * C:]
    before = _checksum(xall)

    dsp.moving_average_cascade_into(x, y, k, passes, C, history=hist, workspace=ws)
    torch.cuda.synchronize()

    try:
        assert _checksum(xall) == before, tag
        _guards_intact(ybuf, yall, hf * C, "output", tag)
        mavg = oracle_mod.mavg_i16 if dt == "i16" else oracle_mod.mavg_f32
        for fa, fb in _out_windows(F, 2 ** 32 // C, WIN // C):
            xs, lead = _host_slice(oracle_mod, dt, C, hf + fa, hf + fb, passes * (k - 1))
            for _ in range(passes):
                xs = mavg(xs, k, C)
            ok = _same_bits(y[fa * C:fb * C].cpu().numpy(), xs[lead * C:])
            print(f"  host frames [{fa}, {fb}): {'equal' if ok else 'DIFFERENT'}")
            assert ok, f"[{fa}, {fb}): {tag}"
        expect = tamper(y, n) if tamper else (0, None)
        got = chunked_cascade_mismatches(xall, yall, k, C, passes, CHUNK // C, first_frame=hf)
        if got[1] is not None:
            got = (got[0], got[1] - hf * C)
        assert got == expect, f"(mismatches, first bad sample) = {got}: {tag}"
    finally:
        del x, hist, xall, y, yall, ybuf, ws
        torch.cuda.empty_cache()


def _run_stat(oracle_mod, gpu, dt, C, k, stat, with_mean, want, in_off=0, out_off=0, mean_off=0, history=False,
              tamper=None):
    import numpy as np
    import torch
    import digital_signal_processsing_amd as dsp
    import stat_ref
    from bigsignal_ref import chunked_stat_mismatches
    dtype, code, esz = _dt(dt)
    F, n = _sizes(C)
    plan = dsp.stat_plan(n, k, stat, C, code, with_mean)
    tag = (f"stat {dt} C={C} k={k} stat={stat} mean={with_mean} n={n} in+{in_off} out+{out_off} mean+{mean_off} "
           f"history={history}: {plan}")
    print(tag)
    _check_plan(plan, want, tag)
    hf = k - 1 if history else 0
    _need(gpu, (n + hf * C) * esz + 2 * (n + hf * C + 2 * GUARD + 4) * 4 + (5 << 30))
    xall, x, hist = _stream(gpu, dtype, n, hf * C, in_off)
    ybuf, yall = _guarded(gpu, torch.float32, n, hf * C, out_off)
    mbuf, mall = _guarded(gpu, torch.float32, n, hf * C, mean_off)     # allocated, not passed, without a mean
    y, mean = yall[hf * C:], (mall[hf * C:] if with_mean else None)
    before = _checksum(xall)

    dsp.moving_stat_into(x, y, k, stat, C, history=hist, mean_out=mean)
    torch.cuda.synchronize()

    try:
        assert _checksum(xall) == before, tag
        _guards_intact(ybuf, yall, hf * C, "d_out", tag)
        if with_mean:
            _guards_intact(mbuf, mall, hf * C, "d_mean", tag)
        else:
            assert bool((_bits(mbuf) == SENT[4]).all()), f"d_mean's buffer written without a mean: {tag}"
        for fa, fb in _out_windows(F, 2 ** 32 // C, WIN // C):
            xs, lead = _host_slice(oracle_mod, dt, C, hf + fa, hf + fb, k - 1)
            hx, sx, drop = (xs[:lead * C], xs[lead * C:], 0) if lead == k - 1 else (None, xs, lead)
            what = (f"[{fa}, {fb})", tag)
            yw = y[fa * C:fb * C].cpu().numpy().reshape(-1, C)
            mw = mean[fa * C:fb * C].cpu().numpy().reshape(-1, C) if with_mean else None
            if dt == "i16":
                ref, mref = stat_ref.stat_ref_i16(sx, k, stat, C, hx)
                stat_ref.check_i16(yw, ref[drop:], what)
                if with_mean:
                    stat_ref.check_i16(mw, mref[drop:], (what, "mean"))
            else:
                ref, mref, Msq = stat_ref.stat_ref_f32(sx, k, stat, C, hx)
                stat_ref.check_f32(stat, yw, ref[drop:], Msq[drop:], what)
                if with_mean:        # the small suite's bar for a moving mean: the window mean of |x| as the scale
                    S1a, _ = stat_ref.window_sums(np.abs(sx), k, C, None if hx is None else np.abs(hx))
                    bad = ~(np.abs(mw.astype(np.float64) - mref[drop:]) <= 1e-5 * np.maximum(np.abs(mref), S1a / k)[drop:])
                    assert not bad.any(), (what, "mean", int(bad.sum()), tuple(np.argwhere(bad)[0]))
            print(f"  host frames [{fa}, {fb}): within the bars")
        expect = tamper(y, mean, n) if tamper else (0, None)
        got = chunked_stat_mismatches(xall, yall, mall if with_mean else None, k, C, stat, STAT_CHUNK // C, first_frame=hf)
        if got[1] is not None:
            got = (got[0], got[1] - hf * C)
        assert got == expect, f"(mismatches, first bad sample) = {got}: {tag}"
    finally:
        del x, hist, xall, y, mean, yall, mall, ybuf, mbuf
        torch.cuda.empty_cache()


# id, dtype, C, k, hop, phase, plan, keyword arguments
DECIM_CASES = [
    # M * C itself crosses 2^31: the compacted output offset and its 16-B store phase
    ("decim_scan_i16_c1_k100_hop2", "i16", 1, 100, 2, 1, ("decim_scan<i16,acc=i32,C=1,F=8,U=4", "tile_frames=8192 "), {}),
    # stereo, sparse output; a grid of more than 2^20 tiles through the XCD remap
    ("decim_scan_f32_c2_k400_hop160", "f32", 2, 400, 160, 80, ("decim_scan<f32,acc=f64,C=2,F=2,U=2", "tile_frames=1024 ", " remap="), {}),
    # the frame-unit form (an input view one sample off 16-B alignment): F = 1 tiles, four times the grid
    ("decim_scan_i16_c2_k100_hop7_frame_unit", "i16", 2, 100, 7, 6, ("decim_scan<i16,acc=i32,C=2,F=4,U=4",), {"in_off": 1}),
    ("decim_scan_i16_c2_k705_hop3_history", "i16", 2, 705, 3, 1, ("decim_scan<i16,acc=i32,C=2,F=4,U=4",), {"history": True}),
    # one wave per output frame: f1 = phase + m * hop
    ("decim_window_f32_c1_k44100", "f32", 1, 44100, 44100, 22050, ("decim_window<f32,acc=f64,C=1,vec=1>",), {}),
    ("decim_window_i16_c3_k1024_hop2049", "i16", 3, 1024, 2049, 5, ("decim_window<i16,acc=i64,C=3,vec=0>",), {}),
    # the gather reads full[f * C + c] past 2^32; the workspace is the full-rate buffer
    ("decim_full_i16_c3_k64_hop16", "i16", 3, 64, 16, 5, ("decim_full hop=16 phase=5 x tile_scan<i16,acc=i32,C=3,F=1,U=4,blelloch",), {}),
]
# id, dtype, C, k, passes, plan, keyword arguments
CASCADE_CASES = [
    ("cascade_tile_i16_c1_k33_p2", "i16", 1, 33, 2, ("cascade_tile<i16,acc=i32,C=1,F=8,U=4", " passes=2 halo_frames=64 "), {}),
    ("cascade_tile_i16_c2_k100_p3", "i16", 2, 100, 3, ("cascade_tile<i16,acc=i32,C=2,F=4,U=4", " passes=3 halo_frames=297 "), {}),
    # 2016 B of halo; bit-exact by the power-of-two argument; more than 2^20 tiles
    ("cascade_tile_f32_c2_k64_p4", "f32", 2, 64, 4, ("cascade_tile<f32,acc=f64,C=2,F=2,U=2", " passes=4 halo_frames=252 ", "tile_frames=1024 "), {}),
    ("cascade_tile_i16_c1_k33_p2_frame_unit", "i16", 1, 33, 2, ("cascade_tile<i16,acc=i32,C=1,F=8,U=4",), {"in_off": 1, "out_off": 1}),
    ("cascade_tile_i16_c2_k100_p3_history", "i16", 2, 100, 3, ("cascade_tile<i16,acc=i32,C=2,F=4,U=4", " passes=3 "), {"history": True}),
    # the ping-pong buffer lies past 2^32 bytes inside the workspace
    ("cascade_loop_i16_c3_k64_p2", "i16", 3, 64, 2, ("cascade_loop passes=2 history=0 x tile_scan<i16,acc=i32,C=3,F=1,U=4,blelloch",), {}),
]
# id, dtype, C, k, stat, with_mean, plan, keyword arguments
STAT_CASES = [
    # fp32 out of int16 in: output bytes at twice the input's; two output views
    ("stat_tile_i16_c1_k1000_std_mean", "i16", 1, 1000, 3, True, ("stat_tile<i16,acc=i32/i64,C=1,F=8,U=4,M=2", " stat=3 mean=1 "), {}),
    ("stat_tile_i16_c2_k64_rms", "i16", 2, 64, 1, False, ("stat_tile<i16,acc=i32/i64,C=2,F=4,U=4,M=1", " stat=1 mean=0 "), {}),
    ("stat_tile_f32_c1_k1024_var_mean", "f32", 1, 1024, 2, True, ("stat_tile<f32,acc=f64/f64,C=1,F=4,U=2,M=2", " stat=2 mean=1 ", "! direct"), {}),
    ("stat_tile_f32_c2_k7_meansq_direct", "f32", 2, 7, 0, False, ("stat_tile<f32,acc=f64/f64,C=2,F=2,U=2,M=1", " stat=0 mean=0 ", " direct"), {}),
    ("stat_tile_i16_c1_k100_std_mean_frame_unit", "i16", 1, 100, 3, True, ("stat_tile<i16,acc=i32/i64,C=1,F=8,U=4,M=2",), {"mean_off": 3}),
    ("stat_tile_i16_c2_k300_var_mean_history", "i16", 2, 300, 2, True, ("stat_tile<i16,acc=i32/i64,C=2,F=4,U=4,M=2", " stat=2 mean=1 "), {"history": True}),
    # strip = t / C, f0 = strip * L
    ("stat_strip_f32_c8_k100_var_mean", "f32", 8, 100, 2, True, ("stat_strip dtype=f32 acc=f64 C=8 stat=2 mean=1 ", " L=25 "), {}),
    ("stat_strip_i16_c3_k100_std", "i16", 3, 100, 3, False, ("stat_strip dtype=i16 acc=i64 C=3 stat=3 mean=0 ", " L=25 "), {}),
]


@pytest.mark.parametrize("name,dt,C,k,hop,phase,want,kw", DECIM_CASES, ids=[c[0] for c in DECIM_CASES])
def test_every_decimated_output_past_2p32_samples(oracle_mod, gpu, name, dt, C, k, hop, phase, want, kw):
    _run_decim(oracle_mod, gpu, dt, C, k, hop, phase, want, **kw)


@pytest.mark.parametrize("name,dt,C,k,passes,want,kw", CASCADE_CASES, ids=[c[0] for c in CASCADE_CASES])
def test_every_cascaded_output_past_2p32_samples(oracle_mod, gpu, name, dt, C, k, passes, want, kw):
    _run_cascade(oracle_mod, gpu, dt, C, k, passes, want, **kw)


@pytest.mark.parametrize("name,dt,C,k,stat,with_mean,want,kw", STAT_CASES, ids=[c[0] for c in STAT_CASES])
def test_every_moment_output_past_2p32_samples(oracle_mod, gpu, name, dt, C, k, stat, with_mean, want, kw):
    _run_stat(oracle_mod, gpu, dt, C, k, stat, with_mean, want, **kw)


def test_decim_reference_sees_past_2p31_outputs(oracle_mod, gpu):
    """Sensitivity: the packed output holds 2^31 + ~5 * 10^5 samples; one flipped bit at output
    sample 2^31 + 5 and one at the last output are both counted, the first one located."""
    def tamper(y, n_out):
        for i in (2 ** 31 + 5, n_out - 1):
            _bits(y)[i:i + 1] ^= 1
        return (2, 2 ** 31 + 5)
    _run_decim(oracle_mod, gpu, "i16", 1, 100, 2, 1, "decim_scan<i16,acc=i32,C=1,F=8,U=4", tamper=tamper)


def test_cascade_reference_sees_past_2p32(oracle_mod, gpu):
    def tamper(y, n):
        for i in (2 ** 32 + 5, n - 1):
            _bits(y)[i:i + 1] ^= 1
        return (2, 2 ** 32 + 5)
    _run_cascade(oracle_mod, gpu, "i16", 1, 33, 2, "cascade_tile<i16,acc=i32,C=1,F=8,U=4", tamper=tamper)


def test_stat_reference_sees_past_2p32(oracle_mod, gpu):
    """Bit 20 of the fp32 pattern (an eighth of the value and more: one ulp is inside the bar): an
    output at sample 2^32 + 5, the mean of the last sample."""
    def tamper(y, mean, n):
        _bits(y)[2 ** 32 + 5:2 ** 32 + 6] ^= 1 << 20
        _bits(mean)[n - 1:n] ^= 1 << 20
        return (2, 2 ** 32 + 5)
    _run_stat(oracle_mod, gpu, "i16", 1, 1000, 3, True, "stat_tile<i16,acc=i32/i64,C=1,F=8,U=4,M=2", tamper=tamper)
