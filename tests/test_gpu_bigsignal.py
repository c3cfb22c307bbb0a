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

A case holds 2 x 8.6 GB (int16) or 2 x 17.2 GB (fp32) plus < 5 GiB of chunk
temporaries, and skips only when the (shared) device has less than that free."""
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
    want = (want,) if isinstance(want, str) else want
    assert plan.startswith(want[0]), tag
    for tok in want[1:]:
        assert (tok[1:] not in plan) if tok.startswith("!") else (tok in plan), f"plan token {tok!r}: {tag}"
    hs = (k - 1) * C if history else 0
    assert (GUARD * esz) % 16 == 0 and (hs * esz) % 16 == 0
    need = 2 * (n + hs + 2 * GUARD) * esz + (5 << 30)
    free = torch.cuda.mem_get_info(gpu)[0]
    if free < need:
        pytest.skip(f"{free >> 30} GiB free on the device, this case needs {need >> 30} GiB")
    ws_n = dsp.workspace_bytes(n, k, C, code, algo)
    if plan.startswith(("ahead_scan<", "wide_ahead<")):
        assert ws_n > 0 and " ws=" in plan, tag
    ws = torch.empty(ws_n, dtype=torch.uint8, device=gpu) if ws_n else None

    # input: samples [0, hs + n) of the synthetic stream; x is all of it but the history
    xbuf = torch.empty(in_off + hs + n, dtype=dtype, device=gpu)
    xall = xbuf[in_off:]
    dsp.fill_synthetic(xall.numel(), seed=SEED, out=xall)
    x, hist = xall[hs:], (xall[:hs] if history else None)
    # output: a view inside a sentinel-filled buffer (stale results of an earlier case cannot pass)
    ybuf = torch.empty(GUARD + out_off + hs + n + GUARD, dtype=dtype, device=gpu)
    _bits(ybuf).fill_(SENT[esz])
    lo = GUARD + out_off
    yall = ybuf[lo:lo + hs + n]          # indexed like xall; the library writes yall[hs:]
    y = yall[hs:]
    assert x.data_ptr() % 16 == (in_off * esz) % 16 and y.data_ptr() % 16 == (out_off * esz) % 16
    before = _checksum(xall)

    dsp.moving_average_into(x, y, k, C, algo, history=hist, workspace=ws)
    torch.cuda.synchronize()

    try:
        # 4. the input (and the history) unchanged
        assert _checksum(xall) == before, tag
        # 3. guard bands (and, with history, the samples between band and view) unchanged
        for name, band in (("before", ybuf[:lo + hs]), ("after", ybuf[lo + hs + n:])):
            assert band.numel() >= GUARD and bool((_bits(band) == SENT[esz]).all()), f"guard band {name}: {tag}"
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
        del x, hist, xall, xbuf, y, yall, ybuf, ws
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
