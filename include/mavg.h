/*
 * mavg.h -- C ABI of libmavg, the MI355X-native (gfx950) causal moving-average
 * filter.  Plain pointers and sizes only; no HIP, torch or C++ types.
 *
 * This is the in-process replacement for the reference's per-variant
 * "<Variant>GpuLoad" drivers and their kernels:
 *
 *   reference                                              replaced by
 *   ---------------------------------------------------    -------------------------
 *   blellochAveragerGpuLoad  basics/blelloch_scan_averager.cu:189-232        mavg_run(.., MAVG_ALGO_BLELLOCH_SCALAR ..)
 *     recursive_blelloch :134-167, blelloch_scan_inclusive :40-131,
 *     blelloch_uniform_add :17-36, averager_kernel :171-186
 *   blellochAveragerGpuLoad  basics/blelloch_scan_vloaded_averager.cu:183-228 mavg_run(.., MAVG_ALGO_BLELLOCH ..)
 *   hillisSteeleAveragerGpuLoad basics/hillis_steele_averager.cu:221-249     mavg_run(.., MAVG_ALGO_HILLIS_SCALAR ..)
 *   (vloaded)                basics/hillis_steele_vloaded_averager.cu         mavg_run(.., MAVG_ALGO_HILLIS ..)
 *   vload4AveragerGpuLoad    basics/profilable_sm_vload4.cu:91-145            mavg_run(.., MAVG_ALGO_DIRECT ..)
 *   vload2AveragerGpuLoad    basics/profilable_sm_vload2.cu:65-92             mavg_run(.., MAVG_ALGO_DIRECT_VEC2 ..)
 *   sharedMemoryAveragerGpuLoad basics/profilable_sm_averager.cu:48-74       mavg_run(.., MAVG_ALGO_DIRECT_SCALAR ..)
 *   parallelAveragerGpuLoad  basics/profilable_parallel_averager.cu:26-51    mavg_run(.., MAVG_ALGO_NAIVE ..)
 *   DspWorkspace<T,Mode>     gpu_utils.h:67-160 (halo zone, scratch)         caller-owned buffers + d_history
 *                                                                             + mavg_workspace_bytes
 *
 * Semantics (all algorithms, both dtypes) follow the serial reference
 * basics/profilable_moving_averager.cpp:14-37: interleaved frames x[f*C + c],
 * window k ("grade"), frames before the first one read as zero -- or, when
 * d_history is given, as the (k-1)*C samples immediately preceding d_in
 * (the multi-GPU halo; gpu_utils.h:112-123 is the reference's zero halo).
 *   MAVG_I16: y = (int16)(S / k), S the exact int64 window sum, C++ truncating
 *             division.  Bit-exact with the serial reference (the reference's
 *             GPU variants use a float reciprocal and are not).
 *   MAVG_F32: y = (float)(S / k), S accumulated in fp64; within 1e-5 relative
 *             of the fp64 serial restatement.
 *
 * Ownership: the caller owns d_in, d_out, d_history and d_ws (device memory);
 * mavg_run never allocates, never synchronises, never exits, and only
 * enqueues work on `stream` (a hipStream_t; NULL = the legacy default
 * stream), so it can be captured into a HIP graph.  d_in is const (the
 * reference scans in place; this library does not).  Thread-safe and
 * re-entrant; the only process state is per DEVICE (keyed on hipGetDevice):
 * the CU count and, per kernel, whether its dynamic-LDS limit has been raised
 * on that device -- so one process may drive several devices.  (The test
 * hook that forces the look-ahead scan's schedule is process-wide state; it
 * lives in the debug build only, include/mavg_debug.h.)
 */
#ifndef MAVG_H
#define MAVG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAVG_ABI_VERSION 4  /* 2: mavg_plan takes block_size; 3: the schedule test hook moved to mavg_debug.h;
                               4: mavg_build_id */

typedef enum {
    MAVG_I16 = 0, /* int16 PCM in/out (the reference's WAV data path) */
    MAVG_F32 = 1  /* fp32 in/out (BASELINE.json north_star) */
} mavg_dtype;

typedef enum {
    MAVG_ALGO_AUTO = 0,            /* pick by (dtype, k, C): see DESIGN.md */
    MAVG_ALGO_BLELLOCH = 1,        /* single-pass streaming work-efficient scan, 16-B units */
    MAVG_ALGO_BLELLOCH_SCALAR = 2, /* same scan, one frame per lane */
    MAVG_ALGO_HILLIS = 3,          /* streaming Hillis-Steele (log-step) scan, 16-B units */
    MAVG_ALGO_HILLIS_SCALAR = 4,   /* Hillis-Steele, one frame per lane */
    MAVG_ALGO_DIRECT = 5,          /* direct LDS-tiled window sum, 16-B loads (vload4) */
    MAVG_ALGO_DIRECT_VEC2 = 6,     /* direct LDS-tiled, 8-B loads (vload2) */
    MAVG_ALGO_DIRECT_SCALAR = 7,   /* direct LDS-tiled, element loads (shared) */
    MAVG_ALGO_NAIVE = 8            /* one thread per sample, window from global memory */
} mavg_algo;

typedef enum {
    MAVG_OK = 0,
    MAVG_ERR_INVALID_ARG = 1, /* null pointer, k < 1, C < 1, n not a multiple of C, bad enum */
    MAVG_ERR_UNSUPPORTED = 2, /* valid but not implemented (C > 8 outside AUTO/NAIVE, k too large for algo) */
    MAVG_ERR_MISALIGNED = 3,  /* a pointer not aligned to the sample size (2 B int16, 4 B fp32) */
    MAVG_ERR_WORKSPACE = 4,   /* ws_bytes smaller than mavg_workspace_bytes() */
    MAVG_ERR_HIP = 5          /* a HIP runtime call or kernel launch failed */
} mavg_status;

/* Device workspace (bytes) mavg_run needs for this problem, whatever the
 * alignment of the views later passed to mavg_run.  0 for every launch
 * except the look-ahead scan that AUTO/BLELLOCH pick for windows too long
 * for an LDS-staged halo (fp32 halos > 16 KiB, e.g. mono k > 4096; int16 past
 * ~47 KiB): 8-B tagged records, one per (tile, channel, 32-bit word of the
 * tile sum), or one per (tile, wave, ...) for mono windows short enough for
 * per-wave records, padded to 16, + 16, sized for the smaller tiles of the
 * frame-unit form a misaligned view may run (2^30 fp32 mono samples: 64 MiB
 * at k=8192..44100 with per-wave records, 16 MiB at k=10^6 with per-tile
 * records; int16 stereo k=44100: 8 MiB), + the run totals of windows past
 * 384 tiles (8 B per run of G tiles per channel word: < 1 % more).
 * 16-B alignment; contents need no initialisation (mavg_run zeroes them on
 * the stream); one workspace must not serve two launches that may run
 * concurrently. */
int mavg_workspace_bytes(size_t n_samples, int channels, int grade, int dtype,
                         int algo, int block_size, size_t* out_bytes);

/*
 * y[0..n) = moving average of x[0..n), n = frames * channels samples.
 *   d_in/d_out any sample-aligned views (2 B int16, 4 B fp32): a vector
 *              algorithm on views that are not 16-B aligned peels a head of
 *              < 16 B in its one-frame-per-lane form when both views share
 *              the offset, else runs that form over the whole signal.
 *   d_history  NULL (zero history) or (grade-1)*channels samples that
 *              precede d_in (sample-aligned).
 *   block_size the reference's argv block size (a multiple of 32 in
 *              [32, 1024]) or 0 for the tuned geometry.  Non-zero: the naive
 *              kernel runs exactly block_size threads per workgroup; the tile
 *              scans and the direct kernel run the next power of two of at
 *              least one wave64 (64, 128, 256, 512, 1024), while the window's
 *              halo fits that workgroup's LDS (longer windows keep the tuned
 *              look-ahead scan).  mavg_plan() shows the result.
 *   stream     hipStream_t or NULL.
 * Returns a mavg_status.  Nothing is enqueued unless MAVG_OK is returned
 * (MAVG_ERR_HIP excepted, when the launch itself failed).
 *
 * Supported maximum.  n_samples / channels < 2^62 frames, and one launch
 * holds at most 2^32 - 1 work-items (the HIP runtime's limit):
 *   - MAVG_ALGO_NAIVE (one thread per sample), the k = 1 copy and
 *     mavg_stream_copy (one thread per 16 B) cover a longer signal with
 *     several launches of 2^31 work-items: every size below 2^62 samples
 *     (mavg_plan shows "launches=" when there is more than one);
 *   - every other kernel makes one launch of `block` threads per
 *     `tile_frames` frames (both in mavg_plan's text; the direct kernels:
 *     U * F frames per thread), so it takes
 *         frames <= (2^32 - 1) / block * tile_frames:
 *     the tuned 16-B-unit forms 2^35 frames and more (fp32 mono k = 1024:
 *     8 frames per thread), the frame-unit forms (*_SCALAR, frames that do
 *     not divide 16 B, views off 16-B alignment by different amounts) 2 or 4
 *     frames per thread: 2^33 or 2^34 frames.  Past it mavg_run and mavg_plan
 *     return MAVG_ERR_UNSUPPORTED and nothing is enqueued.
 * Every kernel family is tested on 2^32 + 10^6-sample signals
 * (tests/test_gpu_bigsignal.py).  The int16 kernels are tested at full scale --
 * constant 32767 and -32768, window sums over the whole of [-32768 grade,
 * 32767 grade] and on every quotient boundary of the output division -- on
 * these paths (tests/test_gpu_i16_range.py): the eight explicit algorithms up
 * to the largest grade each takes, the head-peel and frame-unit forms, the
 * look-ahead scan with int32 and int64 sums up to grade 65537 (mono, stereo,
 * the Hillis record carry; 4 channels at 44100 and 70000), wide_tile with 4
 * and 8 channels, wide_ahead with 4 channels (4096 < grade <= 8192, int32 sums
 * only: past it 4 channels take the look-ahead scan) and with 8 (int32 and
 * int64), a d_history per kernel shape, and the rows, ragged, decimated and
 * moment calls at their halo limits.  int16 has no chan_tile path.  NOT run at
 * full scale: the window-matched and run-total forms of windows past the L2
 * reach, 3, 5, 6 and 7 channels, and the cascade beyond its own
 * test_int16_full_scale.  Both output divisions are modelled in
 * tests/test_division.py.
 */
int mavg_run(const void* d_in, void* d_out, size_t n_samples, int channels,
             int grade, int dtype, int algo, int block_size,
             const void* d_history, void* d_ws, size_t ws_bytes, void* stream);

/*
 * Batched rows: `rows` independent signals of `row_frames` frames each,
 * stored densely one after another (no row stride: row r starts at sample
 * r * row_frames * channels), every one filtered exactly as mavg_run would
 * filter it alone -- zero history before the row's frame 0 (or the row's own
 * history), divisor `grade` also in the warm-up and when grade > row_frames,
 * the same int16 / fp32 arithmetic.  A row's outputs depend on that row's
 * samples (and its history) only: nothing of another row enters them, not even
 * as a term that cancels (a neighbour's Inf or NaN stays in the neighbour).
 *   d_in/d_out any sample-aligned views of rows * row_frames * channels samples.
 *   d_history  NULL, or rows * (grade-1) * channels samples: row r's history
 *              at sample r * (grade-1) * channels.
 *   d_ws       mavg_rows_workspace_bytes() bytes, 16-B aligned (NULL when 0).
 * Ownership, stream and capture rules are mavg_run's: no allocation, no
 * synchronisation, nothing enqueued unless MAVG_OK is returned (MAVG_ERR_HIP
 * excepted).  rows == 0 or row_frames == 0: MAVG_OK, nothing enqueued.
 *
 * Dispatch (mavg_rows_plan shows which):
 *   rows_scan  ONE launch of the segmented rows scan over the whole batch, no
 *              workspace: d_history == NULL, channels 1 or 2, int16 grade <=
 *              65535, and the effective halo of min(grade, row_frames) frames
 *              is at most 16 KiB (min(grade, row_frames) * channels <= 4096
 *              fp32 or 8192 int16 samples: the LDS-staged halos, as far as
 *              mavg_run's own tiles go), and rows shorter than 64 MiB.  Tiles ignore row
 *              boundaries: rows of 5 frames and of 2^24 frames run the same
 *              code at the same rate.  Views that are not both 16-B aligned
 *              run its one-frame-per-lane form.  grade == 1 is the flat copy.
 *   rows_loop  everything else (a history, channels >= 3, windows and rows
 *              both past 16 KiB of halo, int16 grade > 65535, and rows of
 *              64 MiB or more, which fill the device one at a time and measured
 *              no slower that way, DESIGN.md "Rows"): mavg_run's
 *              dispatch (MAVG_ALGO_AUTO, block_size 0) once per row on
 *              `stream` -- it costs `rows` launches (twice that for rows whose
 *              views it peels), correct but not fast.  All rows share d_ws.
 *              Every row is planned before the first is launched: a workspace
 *              or support error leaves the stream untouched.
 *
 * Supported maximum.  rows * row_frames < 2^62 frames (and the byte count in
 * size_t), else MAVG_ERR_UNSUPPORTED.  rows_scan makes one launch of `block`
 * threads per `tile_frames` frames (both in mavg_rows_plan's text), so it takes
 *     rows * row_frames <= (2^32 - 1) / block * tile_frames
 * frames: 2^35 (fp32 mono) and more in the 16-B-unit form, 2^34 frames in the
 * one-frame-per-lane form of views off 16-B alignment; past it
 * MAVG_ERR_UNSUPPORTED, nothing enqueued.  rows_loop: each row is a mavg_run
 * signal (the "Supported maximum" above).  Tested on a 2^31 + 2^16-sample
 * int16 batch (tests/test_gpu_rows.py).
 */
int mavg_rows_run(const void* d_in, void* d_out, size_t rows, size_t row_frames,
                  int channels, int grade, int dtype, const void* d_history,
                  void* d_ws, size_t ws_bytes, void* stream);

/* Device workspace (bytes) mavg_rows_run needs: 0 for rows_scan; for
 * rows_loop what mavg_workspace_bytes gives for one row (the rows share it). */
int mavg_rows_workspace_bytes(size_t rows, size_t row_frames, int channels, int grade,
                              int dtype, int with_history, size_t* out_bytes);

/* Describe, without launching anything, what mavg_rows_run would do on
 * 16-B-aligned views: "rows_scan<...> ... tile_frames=N ..." or
 * "rows_loop rows=R x <mavg_plan's text for one row>" (up to ~300 characters). */
int mavg_rows_plan(size_t rows, size_t row_frames, int channels, int grade, int dtype,
                   int with_history, char* buf, size_t buflen);

/* Ragged rows: `rows` independent signals of DIFFERENT lengths, packed one
 * after another (CSR style).  Row r is frames [off[r], off[r+1]) of the packed
 * stream; the batch holds off[rows] frames = off[rows] * channels samples.
 * Every row is filtered exactly as mavg_run would filter it alone: zero
 * history before its frame 0, divisor `grade` (also in the warm-up and when
 * grade exceeds the row), the same int16 and fp32 arithmetic, and the rows
 * API's isolation guarantee -- nothing of another row enters a row's sums, not
 * even as a term that cancels.
 *   h_offsets  rows + 1 frame offsets in HOST memory: h_offsets[0] == 0,
 *              non-decreasing.  Empty rows are legal anywhere (several in a
 *              row, the first, the last).  This copy is what the library
 *              validates, what gives the longest row (max_row_frames) and what
 *              drives the per-row loop.
 *   d_offsets  the caller's DEVICE copy of the same rows + 1 values, 8-B
 *              aligned: what the kernel reads.  The library never copies
 *              between host and device.  Every index the kernel derives from
 *              it is clamped to the tile and halo it belongs to and every
 *              search is bounded by `rows`: a device copy that differs from the
 *              host's gives wrong values, not an access outside the views.
 *   d_in/d_out any sample-aligned views of off[rows] * channels samples.
 *   d_ws       mavg_ragged_workspace_bytes() bytes, 16-B aligned (NULL when 0).
 * Ownership, stream and capture rules are mavg_run's: no allocation, no
 * synchronisation, nothing enqueued unless MAVG_OK is returned (MAVG_ERR_HIP
 * excepted).  Arguments are validated first; then rows == 0 or off[rows] == 0:
 * MAVG_OK, nothing enqueued.
 *
 * Status: MAVG_ERR_INVALID_ARG for a bad dtype, channels or grade, a NULL
 * h_offsets with rows > 0, h_offsets[0] != 0, a decreasing pair, and a NULL
 * d_offsets, d_in or d_out with work to do; MAVG_ERR_MISALIGNED for views off
 * sample alignment or d_offsets off 8-B alignment; MAVG_ERR_UNSUPPORTED for
 * 2^62 frames or more, or past the one-launch limit below.
 *
 * Dispatch (mavg_ragged_plan shows which):
 *   ragged_scan  ONE launch of the ragged scan over the packed stream, no
 *                workspace: channels 1 or 2, int16 grade <= 65535, and the
 *                effective halo of min(grade, max_row_frames) frames at most
 *                16 KiB (rows_scan's limit).  Tiles ignore row boundaries; the
 *                row starts of a tile come from d_offsets (two bounded searches
 *                and a bitmask in LDS per tile).  Views that are not both 16-B
 *                aligned run its one-frame-per-lane form.  grade == 1 is the
 *                flat copy.  There is no long-row rule: rows_scan's 64-MiB rule
 *                was measured on uniform batches only.
 *   ragged_loop  everything else (channels >= 3, windows and longest row both
 *                past 16 KiB of halo, int16 grade > 65535): mavg_run's dispatch
 *                (MAVG_ALGO_AUTO, block_size 0) once per non-empty row on
 *                `stream`, from h_offsets -- correct, not fast.  All rows share
 *                d_ws, sized for the longest row.  Every row is planned before
 *                the first is launched: an error leaves the stream untouched.
 *
 * Supported maximum.  off[rows] < 2^62 frames (and the byte count in size_t).
 * ragged_scan makes one launch of `block` threads per `tile_frames` frames
 * (both in mavg_ragged_plan's text): off[rows] <= (2^32 - 1) / block *
 * tile_frames frames, as rows_scan.  Tested on a 2.15e9-sample int16 batch,
 * past 2^31 (tests/test_gpu_ragged.py).
 */
int mavg_ragged_run(const void* d_in, void* d_out, const int64_t* h_offsets,
                    const int64_t* d_offsets, size_t rows, int channels, int grade,
                    int dtype, void* d_ws, size_t ws_bytes, void* stream);

/* Device workspace (bytes) mavg_ragged_run needs: 0 for ragged_scan; for
 * ragged_loop what mavg_workspace_bytes gives for the longest row. */
int mavg_ragged_workspace_bytes(const int64_t* h_offsets, size_t rows, int channels,
                                int grade, int dtype, size_t* out_bytes);

/* Describe, without launching anything, what mavg_ragged_run would do on
 * 16-B-aligned views: "ragged_scan<...> rows=R frames=N max_row_frames=M
 * window=min(grade,M) ... tile_frames=T ..." or "ragged_loop rows=R
 * max_row_frames=M x <mavg_plan's text for the longest row>" (up to ~300
 * characters).  An empty batch has no plan: MAVG_ERR_INVALID_ARG. */
int mavg_ragged_plan(const int64_t* h_offsets, size_t rows, int channels, int grade,
                     int dtype, char* buf, size_t buflen);

/*
 * Decimated moving average: of mavg_run's full-rate output only the frames
 * phase + m * hop, m in [0, M), M = len(range(phase, n_frames, hop)), packed:
 * d_out holds M * channels samples.  hop >= 1, 0 <= phase < hop; phase counts
 * from d_in's frame 0, whatever the history.  Everything else is mavg_run's
 * contract: interleaved channels, zero history or d_history (the
 * (grade-1)*channels samples in front of d_in), divisor grade, int16 exact
 * truncating division, fp32 sums in fp64.  What a caller otherwise does with
 * mavg_run and y.view(-1, C)[phase::hop], without writing (or, for sparse
 * windows, reading) what is dropped.
 *   d_in   any sample-aligned view of n_samples samples; one that is not 16-B
 *          aligned runs the scan's one-frame-per-lane form (no head is peeled).
 *   d_out  any sample-aligned view of M * channels samples.
 *   d_ws   mavg_decim_workspace_bytes() bytes, 16-B aligned (NULL when 0).
 * Ownership, stream and capture rules are mavg_run's: no allocation, no
 * synchronisation, nothing enqueued unless MAVG_OK is returned (MAVG_ERR_HIP
 * excepted).  M == 0 (n_samples == 0, or n_frames <= phase): MAVG_OK, nothing
 * enqueued.
 *
 * Status: MAVG_ERR_INVALID_ARG for hop < 1, phase outside [0, hop) and
 * mavg_run's invalid cases; MAVG_ERR_MISALIGNED, MAVG_ERR_WORKSPACE and
 * MAVG_ERR_UNSUPPORTED as mavg_run.
 *
 * Dispatch, evaluated in this order (mavg_decim_plan shows which):
 *   decim_none    hop == 1: mavg_run (MAVG_ALGO_AUTO, block_size 0), unchanged.
 *   decim_window  sparse reading, ONE launch, no workspace: channels <= 8,
 *                 hop >= grade, a window of at least 1 KiB (grade * channels *
 *                 sample size >= 1024), and one of: hop >= 2 * grade, a window
 *                 of at least 4 KiB, decim_scan does not apply (the measured
 *                 crossovers, DESIGN.md "Decimated").  One wave per output frame sums
 *                 the grade frames that output needs, each read once, in fp64
 *                 (fp32) or int64 (int16): exact for every grade.
 *   decim_scan    dense reading, ONE launch, no workspace: hop >= 2, channels 1
 *                 or 2, 2 <= grade (int16: <= 65535), a halo of grade * channels
 *                 * sample size <= 8 KiB (half of rows_scan's range: at 16 KiB
 *                 it measured slower than mavg_run and a slice).  The flat tile
 *                 scan with a compacting end: every input frame is read, only
 *                 the kept frames are converted and stored.  Any hop, also
 *                 hop >= grade with a window under 1 KiB (block averaging).
 *   decim_full    everything else (3+ channels with a short or overlapping
 *                 window, longer halos with hop < grade, int16 grade > 65535
 *                 with hop < grade, grade == 1): mavg_run (AUTO) into the
 *                 workspace, then a strided gather -- correct, not fast.  Both
 *                 steps are planned before the first is launched: an error
 *                 leaves the stream untouched.
 *
 * Supported maximum.  mavg_run's: every kernel makes one launch
 * (decim_scan: `block` threads per `tile_frames` frames, decim_window: one wave
 * per output frame), past it MAVG_ERR_UNSUPPORTED and nothing is enqueued.
 * decim_scan (both unit forms, with and without a history), decim_window and
 * decim_full are tested on 2^32 + 10^6-sample signals, every output
 * (tests/test_gpu_bigsignal.py).
 */
int mavg_decim_run(const void* d_in, void* d_out, size_t n_samples, int channels, int grade,
                   int hop, int phase, int dtype, const void* d_history,
                   void* d_ws, size_t ws_bytes, void* stream);

/* M = len(range(phase, n_frames, hop)): the frames mavg_decim_run writes. */
int mavg_decim_out_frames(size_t n_frames, int hop, int phase, size_t* out_frames);

/* Device workspace (bytes) mavg_decim_run needs: 0 for decim_scan and
 * decim_window; mavg_workspace_bytes for decim_none; for decim_full the
 * full-rate output, n_samples * sample size rounded up to 16, plus
 * mavg_workspace_bytes for the full-rate run. */
int mavg_decim_workspace_bytes(size_t n_samples, int channels, int grade, int hop, int phase,
                               int dtype, size_t* out_bytes);

/* Describe, without launching anything, what mavg_decim_run would do on
 * 16-B-aligned views: "decim_none x <mavg_plan's text>", "decim_window<...> ...",
 * "decim_scan<...> ... tile_frames=N ..." or "decim_full hop=H phase=P x
 * <mavg_plan's text>" (up to ~300 characters).  M == 0 has no plan:
 * MAVG_ERR_INVALID_ARG. */
int mavg_decim_plan(size_t n_samples, int channels, int grade, int hop, int phase, int dtype,
                    char* buf, size_t buflen);

/*
 * Cascaded moving average: `passes` >= 1 boxcar passes of one window `grade`,
 * exactly what `passes` successive mavg_run calls with zero history produce,
 * the intermediate stored in the signal's own dtype between passes: int16
 * takes the exact sum, divides with truncation by grade and casts to int16 in
 * every pass (bit-exact with the CPU oracle applied `passes` times); fp32
 * accumulates in fp64, computes float(S / grade), and the intermediate is
 * rounded to fp32.  The divisor is grade in the warm-up of every pass.  Two
 * passes give a triangular window, three or four the usual Gaussian
 * approximation.
 *   d_history  NULL: frames before frame 0 read as zero in every pass (the same
 *              as passes * (grade-1) zero frames in front of the signal).  Else
 *              the passes * (grade-1) * channels samples that immediately
 *              precede d_in: the outputs are those of the cascade applied to
 *              concat(history, x) with the first passes * (grade-1) frames
 *              dropped -- exact for int16 too, every intermediate sample depends
 *              on a finite window: what a chunked streaming caller needs.
 *   d_in, d_out  any sample-aligned views of n_samples samples that do not
 *              overlap; views that are not both 16-B aligned run the fused
 *              kernel's one-frame-per-lane form (no head is peeled).
 *   d_ws       mavg_cascade_workspace_bytes() bytes, 16-B aligned (NULL when 0).
 * Ownership, stream and capture rules are mavg_run's: no allocation, no
 * synchronisation, every step planned before the first is launched, nothing
 * enqueued unless MAVG_OK is returned (MAVG_ERR_HIP excepted).  n_samples == 0:
 * MAVG_OK, nothing enqueued.  Nothing new is promised for non-finite fp32
 * inputs.
 *
 * Status: MAVG_ERR_INVALID_ARG for passes < 1 and mavg_run's invalid cases;
 * MAVG_ERR_UNSUPPORTED when passes * (grade-1) does not fit an int;
 * MAVG_ERR_MISALIGNED, MAVG_ERR_WORKSPACE and MAVG_ERR_UNSUPPORTED as mavg_run.
 *
 * Dispatch, evaluated in this order (mavg_cascade_plan shows which):
 *   cascade_none  passes == 1 or grade == 1 (every pass a copy): mavg_run
 *                 (MAVG_ALGO_AUTO, block_size 0), unchanged, with its workspace.
 *   cascade_tile  ONE launch, no workspace: channels 1 or 2, grade >= 2 (int16:
 *                 <= 65535), a total halo passes * (grade-1) * channels * sample
 *                 size of at most 2 KiB -- 256 B for two int16 passes -- (the
 *                 measured range, DESIGN.md "Cascade": at 8 KiB it measured
 *                 slower than the loop; the kernel itself takes up to 16 KiB
 *                 and an LDS layout inside the workgroup's budget in both unit
 *                 forms, which mavg_debug_force_cascade can force).  A tile
 *                 stages its frames and the total halo in LDS and runs every
 *                 pass there: the signal is read once (plus the halo, mostly
 *                 from L2) and written once, whatever `passes`.
 *   cascade_loop  everything else: mavg_run (AUTO, block_size 0) `passes` times
 *                 on `stream`, never in place, alternating between d_out and a
 *                 workspace buffer so that the last pass lands in d_out --
 *                 correct, not fast.  With a history, pass j also filters the
 *                 shrinking history block ((passes-j+1) * (grade-1) frames, zero
 *                 history, the first grade-1 outputs dropped) into the history
 *                 of pass j+1, and itself takes the block's last grade-1 frames.
 *                 Workspace, with s the sample size and r16 rounding up to 16:
 *                   r16(n_samples * s)
 *                   + (history ? 2 * r16(passes * (grade-1) * channels * s) : 0)
 *                   + max(mavg_workspace_bytes(n_samples),
 *                         history ? mavg_workspace_bytes(passes * (grade-1) * channels) : 0)
 *                 (both mavg_workspace_bytes at MAVG_ALGO_AUTO, block_size 0).
 *
 * Supported maximum.  mavg_run's: cascade_tile makes one launch of `block`
 * threads per `tile_frames` frames (both in mavg_cascade_plan's text), past it
 * MAVG_ERR_UNSUPPORTED and nothing is enqueued.  cascade_tile (both unit forms, with
 * and without a history) and cascade_loop are tested on 2^32 + 10^6-sample
 * signals, every output (tests/test_gpu_bigsignal.py).
 */
int mavg_cascade_run(const void* d_in, void* d_out, size_t n_samples, int channels, int grade,
                     int passes, int dtype, const void* d_history,
                     void* d_ws, size_t ws_bytes, void* stream);

/* Device workspace (bytes) mavg_cascade_run needs: mavg_workspace_bytes for
 * cascade_none, 0 for cascade_tile, the formula above for cascade_loop
 * (with_history != 0: a d_history will be passed). */
int mavg_cascade_workspace_bytes(size_t n_samples, int channels, int grade, int passes, int dtype,
                                 int with_history, size_t* out_bytes);

/* Describe, without launching anything, what mavg_cascade_run would do on
 * 16-B-aligned views: "cascade_none x <mavg_plan's text>", "cascade_tile<...>
 * ... passes=P halo_frames=H ... tile_frames=N ..." or "cascade_loop passes=P
 * history=0|1 x <mavg_plan's text>" (up to ~300 characters).  n_samples == 0
 * has no plan: MAVG_ERR_INVALID_ARG. */
int mavg_cascade_plan(size_t n_samples, int channels, int grade, int passes, int dtype,
                      int with_history, char* buf, size_t buflen);

/* Moving second moment: mean square, RMS, population variance or standard
 * deviation of the causal grade-frame window, per channel, in ONE launch.  With
 * k = grade, S1 = sum of x and S2 = sum of x^2 over the k frames ending at
 * frame f:
 *   MAVG_STAT_MEANSQ  S2 / k
 *   MAVG_STAT_RMS     sqrt(S2 / k)
 *   MAVG_STAT_VAR     max(0, (k S2 - S1^2) / k^2)      (population variance)
 *   MAVG_STAT_STD     sqrt(VAR)
 * Frames before frame 0 read as zero, or as d_history (the (grade-1) * channels
 * samples in front of d_in, exactly as in mavg_run); the divisor is `grade`
 * everywhere, so the warm-up outputs are the statistics of the zero-padded
 * window.  The output is ALWAYS fp32, for int16 input too (n_samples floats, in
 * d_in's layout).  d_mean (fp32, n_samples floats, or NULL) receives
 * (float)(S1 / k) from the same launch -- for z-scoring.
 *
 * int16 input: S1 and S2 are exact integers.  For grade <= 65535,
 * N = k S2 - S1^2 is formed exactly in int64 and the output is the fp32
 * rounding of an fp64 evaluation of N / k^2 (a reciprocal multiply) or its
 * square root: a window of equal samples gives VAR and STD of exactly 0.0f, and
 * outputs do not depend on how a signal is tiled or chunked.  For grade > 65535
 * the result is formed in fp64 from the exact S1 and S2 and carries the fp32
 * tolerance below.
 * fp32 input: S1 and S2 accumulate in fp64 (x^2 is exact there).  MEANSQ and
 * RMS are accurate to 1e-5 relative.  VAR is accurate to 1e-5 of the window's
 * mean SQUARE, not of itself: S2/k - (S1/k)^2 cancels.  Windows of at most 16
 * frames are summed directly, sample by sample, and hold these bars whatever
 * precedes them; longer windows are running sums (prefix differences in fp64,
 * as in mavg_run) with an absolute error near 1e-15 of the largest window sum
 * of squares nearby (the same tile, a few thousand frames), so the bars hold
 * while the window's mean square stays above about 1e-10 of that -- a signal
 * that falls silent by more than 100 dB keeps a residue of that size.  A signal with a large
 * DC offset loses that much of its variance; remove the offset first (subtract
 * a constant, or this library's moving mean) when the variance is small beside
 * the squared mean.  The clamp at 0 is part of the contract: STD is never NaN
 * for finite input.  RMS and STD take the root of the fp64 mean square or
 * variance rescaled by an even power of two (rounded to fp32 there, the root in
 * fp32, scaled back: all exact but the two roundings), so they are finite and
 * hold their bars over the whole fp32 range of the input (|x| near 2^100 or
 * 2^-110, subnormals); MEANSQ and VAR are +Inf when the true value exceeds
 * FLT_MAX.  Nothing new is promised for non-finite input.
 *
 *   d_in       n_samples samples of `dtype`, sample-aligned.
 *   d_out      n_samples floats, 4-B aligned; must not overlap d_in.
 *   d_mean     n_samples floats, 4-B aligned, or NULL.
 *   d_history  (grade-1) * channels samples or NULL, sample-aligned.
 * The 16-B-unit form of the tile kernel runs when d_in, d_out and d_mean are
 * all 16-B aligned; other views run its frame-unit form.  No workspace.
 * Ownership, stream and capture rules are mavg_run's: no allocation, no
 * synchronisation, nothing enqueued unless MAVG_OK is returned (MAVG_ERR_HIP
 * excepted).  n_samples == 0: MAVG_OK, nothing enqueued.
 *
 * Status: MAVG_ERR_INVALID_ARG for a bad stat or dtype, channels < 1,
 * grade < 1, n_samples not a multiple of channels, or a NULL d_in or d_out with
 * work to do; MAVG_ERR_MISALIGNED for d_in (or d_history) off sample alignment
 * or d_out or d_mean off 4 B; MAVG_ERR_UNSUPPORTED past the one-launch limit
 * below.
 *
 * Dispatch, evaluated in this order (mavg_stat_plan shows which):
 *   stat_tile   channels 1 or 2, grade >= 2 (int16: <= 65535), a halo grade *
 *               channels * sample size of at most 16 KiB (the tile scan's and
 *               the rows scan's limit; measured 4.7x and more faster than the
 *               strip over that whole range, DESIGN.md "Moments").  A tile stages its frames and the halo in
 *               LDS once and scans x[n]^2 - x[n-k]^2 from the stage; S1 is
 *               scanned beside it only for VAR, STD or a d_mean.  About
 *               8 B/sample of traffic for fp32, 6 for int16 (plus 4 per d_mean).
 *   stat_strip  everything else (grade == 1, three or more channels, longer
 *               halos, int16 grade > 65535): one thread per channel of a strip
 *               of L frames (L = clamp(grade / 4, 16, 2048), in the plan text)
 *               sums the window in front of its strip directly and slides it --
 *               correct, not fast (about grade / L + 2 reads per output).
 *
 * Supported maximum.  One launch of at most 2^32 - 1 work-items: stat_tile runs
 * `block` threads per `tile_frames` frames (both in the plan text; the frame-unit
 * form, 4 frames per thread, refuses from 2^34 frames), stat_strip one thread
 * per L frames and channel; past it MAVG_ERR_UNSUPPORTED and nothing is
 * enqueued.  stat_tile (both unit forms, the direct sums, with and without a
 * history or a d_mean) and stat_strip are tested on 2^32 + 10^6-sample signals,
 * every output (tests/test_gpu_bigsignal.py).
 */
typedef enum {
  MAVG_STAT_MEANSQ = 0,
  MAVG_STAT_RMS = 1,
  MAVG_STAT_VAR = 2,
  MAVG_STAT_STD = 3
} mavg_stat;
int mavg_stat_run(const void* d_in, float* d_out, float* d_mean /* or NULL */, size_t n_samples,
                  int channels, int grade, int stat, int dtype, const void* d_history,
                  void* stream);

/* Describe, without launching anything, what mavg_stat_run would do on
 * 16-B-aligned views: "stat_tile<...> stat=S mean=0|1 ... tile_frames=N ..." or
 * "stat_strip dtype=... L=... strips=...".  with_mean != 0: a d_mean will be
 * passed.  n_samples == 0 has no plan: MAVG_ERR_INVALID_ARG. */
int mavg_stat_plan(size_t n_samples, int channels, int grade, int stat, int dtype,
                   int with_mean, char* buf, size_t buflen);

/* Moving extrema (peak envelope): the maximum and / or the minimum of the causal
 * `grade`-frame window, per channel of an interleaved signal, in one launch:
 *
 *   max[f] = max(x[j]),  min[f] = min(x[j])   over  j in [f - grade + 1, f]
 *
 * Frames before frame 0.  With d_history (the (grade-1)*channels samples in
 * front of d_in, as for mavg_run) the window reads them.  With d_history == NULL
 * the window is TRUNCATED at frame 0: it covers only frames that exist.  This
 * departs on purpose from the averaging calls' "frames before frame 0 read as
 * zero": zero is neutral for a sum, not for a maximum, and an all-negative
 * signal must not report a maximum of 0 during its warm-up.  A caller who wants
 * zero padding passes a history of zeros.  A chunked streaming caller passes the
 * previous chunk's last grade - 1 frames as the history and gets exactly the
 * one-shot output.
 *
 * Outputs.  d_max and d_min have the input's dtype and size (int16 -> int16,
 * fp32 -> fp32); every output is the value of one sample of its window, so the
 * result is exact for both dtypes.  Either may be NULL, not both; both together
 * cost one launch and one read of the signal (peak-to-peak, or
 * peak = max(max, -min)).  The outputs must not overlap d_in or each other.
 * fp32: +-Inf are ordinary values (an Inf enters the maximum for exactly `grade`
 * frames, then leaves); -0.0 and +0.0 compare equal and either may be returned;
 * nothing is promised for NaN input.  grade == 1 is a copy; grade > n_frames is
 * legal.
 *
 * No workspace.  Ownership, stream and capture rules are mavg_run's: no
 * allocation, no synchronisation, nothing enqueued unless MAVG_OK is returned
 * (MAVG_ERR_HIP excepted).  n_samples == 0: MAVG_OK, nothing enqueued (the
 * arguments are validated first).  MAVG_ERR_INVALID_ARG for a bad dtype,
 * channels < 1, grade < 1, n_samples not a multiple of channels, both outputs
 * NULL, or a NULL d_in with work to do; MAVG_ERR_MISALIGNED for any view off
 * sample alignment; MAVG_ERR_UNSUPPORTED past the one-launch limit below.
 *
 * Dispatch, evaluated in this order (mavg_extrema_plan shows which):
 *   extrema_tile   channels 1 or 2, grade >= 2, a halo (grade - 1) * channels *
 *                  sample size of at most 16 KiB: fp32 grade <= 4097 (mono) /
 *                  2049 (stereo), int16 grade <= 8193 / 4097.  A tile and its
 *                  halo are read once; suffix extrema of each 16-B unit and a
 *                  doubling table over the units' extrema are kept in LDS, so a
 *                  frame costs a constant number of compares and a unit
 *                  O(log grade) (DESIGN.md "Extrema").  The 16-B-unit form runs
 *                  when d_in and every given output are 16-B aligned; other
 *                  views run the frame-unit form (F=1 in the plan text) over the
 *                  whole signal.  8 B/sample of traffic for fp32 and 4 for int16
 *                  with one output; a second output adds its own bytes.
 *   extrema_strip  everything else (grade == 1, three or more channels, longer
 *                  halos): one thread per channel of a strip of L frames
 *                  (L = clamp(grade / 4, 16, 2048), in the plan text) walks back
 *                  over the grade - 1 frames before its strip, then forward --
 *                  correct, not fast (about grade / L + 2 reads per output).
 *
 * Supported maximum.  One launch of at most 2^32 - 1 work-items: extrema_tile
 * runs `block` threads per `tile_frames` frames (both in the plan text; the
 * frame-unit form, 4 frames per thread, refuses from 2^34 frames), extrema_strip
 * one thread per L frames and channel; past it MAVG_ERR_UNSUPPORTED and nothing
 * is enqueued.  Frame and sample indices are 64-bit.  extrema_tile (both unit
 * forms, one output and both, the full 16-KiB halo, with and without a
 * history) and extrema_strip are tested on 2^32 + 10^6-sample signals, every
 * output (tests/test_gpu_bigsignal_filters.py).
 */
int mavg_extrema_run(const void* d_in, void* d_max /* or NULL */, void* d_min /* or NULL */,
                     size_t n_samples, int channels, int grade, int dtype,
                     const void* d_history, void* stream);

/* Describe, without launching anything, what mavg_extrema_run would do:
 * "extrema_tile<dtype,C=..,F=..,U=..,M=1|2|3,..> max=0|1 min=0|1 ... tile_frames=N ..."
 * or "extrema_strip dtype=... L=... strips=...".  with_max / with_min: 0 = that
 * output is NULL (not both), 1 = given; 2 added to either describes views off
 * 16-B alignment (the frame-unit form).  n_samples == 0 has no plan:
 * MAVG_ERR_INVALID_ARG. */
int mavg_extrema_plan(size_t n_samples, int channels, int grade, int dtype,
                      int with_max, int with_min, char* buf, size_t buflen);

/* Exponential moving average (EMA, one-pole low-pass, leaky integrator), per
 * channel of an interleaved signal x[f*C + c]:
 *
 *   y[f] = (1 - alpha) y[f-1] + alpha x[f],     0 < alpha <= 1
 *
 * -- ewm(adjust=False).mean(), the smoother behind envelope followers, the
 * running mean of an online normaliser.  The first filter here with infinite
 * memory: every output depends on every earlier frame.
 *
 * dtype is MAVG_F32 or MAVG_I16.  The output is ALWAYS fp32, for int16 input too
 * (n_samples floats, in d_in's layout); it must not overlap d_in.
 *
 * State.  y[-1] is 0 per channel when d_state_in is NULL (frames before the
 * first read as zero); otherwise y[-1] = d_state_in[c], `channels` doubles in
 * device memory, 8-B aligned.  A caller who wants the y[-1] = x[0] convention
 * passes x[0] as the state.  d_state_out (`channels` doubles, 8-B aligned, or
 * NULL) receives y[last frame] per channel in fp64 from the same call.  The two
 * state pointers must not be equal (MAVG_ERR_INVALID_ARG: the tile kernel's
 * first tiles read one while its last tile writes the other).  Passing chunk
 * i's state_out as chunk i+1's state_in reproduces the one-shot output within
 * the accuracy bar below -- NOT bitwise: the association of the fp64 sums
 * depends on the tiling.
 *
 * Accuracy.  Everything is evaluated in fp64 and rounded once to fp32.  With
 * y_ref the fp64 serial recurrence and M the largest of |x| over the signal and
 * |state_in|, every output satisfies
 *
 *   |y - y_ref| <= 2^-23 |y_ref| + 2^-29 M
 *
 * (the fp32 rounding, doubled; the truncation of ema_tile, at most 2^-30 M, and
 * fp64 re-association).  ema_chain and ema_strip do not truncate: their
 * d_state_out is within 1e-12 M of the reference; ema_tile's within 2^-29 M.
 * The truncation is tested on its worst-case input, a constant M in front of a
 * tile that starts past H, where nothing of the dropped tail cancels
 * (tests/test_gpu_worst_case.py, tests/test_worst_case_model.py).
 * Nothing is promised for non-finite fp32 input.
 *
 * Ownership, stream and capture rules are mavg_run's: no allocation, no
 * synchronisation, every step planned before the first is launched, nothing
 * enqueued unless MAVG_OK is returned (MAVG_ERR_HIP excepted).  The workspace
 * needs no initialisation -- every record read is written earlier in the same
 * call -- so a call may be captured into a graph with no memset node.
 * n_samples == 0: MAVG_OK, nothing enqueued, d_state_out untouched.
 *
 * Status: MAVG_ERR_INVALID_ARG for a bad dtype, channels < 1, n_samples not a
 * multiple of channels, alpha not finite, <= 0, > 1 or below 2^-52 (1 - alpha is
 * then 1 in fp64), equal state pointers, or a NULL view with work to do;
 * MAVG_ERR_MISALIGNED for d_in off sample alignment, d_out off 4 B, a state
 * pointer off 8 B or d_ws off 16 B; MAVG_ERR_WORKSPACE for ws_bytes too small;
 * MAVG_ERR_UNSUPPORTED past the one-launch limit below.
 *
 * Dispatch, evaluated in this order (mavg_ema_plan shows which).  With d = 1 -
 * alpha, the recurrence over m frames composes to y_out = d^m y_in + b, so only
 * b is scanned and every multiplier is a power of d computed on the host; and
 * the memory decays: H = mavg_ema_halo_frames(alpha) frames back a sample weighs
 * at most 2^-30 of its value.
 *   ema_tile   channels 1 or 2 and a halo H * channels * sample size of at most
 *              16 KiB (the stage limit of every tile kernel here; measured 1.1x
 *              to 2.3x faster than the forced chain over that whole range,
 *              DESIGN.md "EMA").  One launch, no workspace.  A tile
 *              stages its H halo frames in front of its own and rebuilds its
 *              carry-in from them; tiles within H frames of the start add the
 *              state in closed form.  alpha == 1 (H = 0) is the converting copy.
 *              The 16-B-unit form runs when d_in and d_out are 16-B aligned;
 *              other views run the frame-unit form (F=1 in the plan text) over
 *              the whole signal.  8 B/sample of traffic for fp32, 6 for int16.
 *   ema_chain  channels 1 or 2, any alpha: three launches through one fp64
 *              record per tile and channel -- the tiles' aggregates, one
 *              workgroup that turns them in place into the tiles' carry-ins
 *              (and writes d_state_out), the tiles again from their carry-ins.
 *              No truncation.  12 B/sample for fp32 (x is read twice), 8 for
 *              int16, plus 16 B per tile.
 *   ema_strip  three or more channels: the same three steps with one thread per
 *              strip of L frames and channel at both ends (L in the plan text)
 *              -- correct, not fast.
 *
 * Workspace (mavg_ema_workspace_bytes): 0 for ema_tile; for ema_chain the record
 * count of the smaller tile of the frame-unit form (1024 frames), so that a
 * misaligned view fits, times channels * 8, rounded up to 16; for ema_strip the
 * strip count times channels * 8, rounded up to 16.  d_ws 16-B aligned.
 *
 * Supported maximum.  Each launch takes at most 2^32 - 1 work-items: the tile
 * kernels run `block` threads per `tile_frames` frames (both in the plan text;
 * the frame-unit form, 4 frames per thread, refuses from 2^34 frames), the
 * strip kernels one thread per L frames and channel; past it
 * MAVG_ERR_UNSUPPORTED and nothing is enqueued.  Frame and sample indices are
 * 64-bit wherever they are not tile-local.  ema_tile (both unit forms, up to
 * the 16-KiB halo, a state carried from an earlier chunk in and out), ema_chain
 * (with a d_state_out) and ema_strip are tested on 2^32 + 10^6-sample signals,
 * every output (tests/test_gpu_bigsignal_filters.py).
 */
int mavg_ema_run(const void* d_in, float* d_out, size_t n_samples, int channels,
                 double alpha, int dtype,
                 const double* d_state_in /* or NULL */, double* d_state_out /* or NULL */,
                 void* d_ws, size_t ws_bytes, void* stream);

/* Device workspace mavg_ema_run needs for these arguments (see "Workspace"
 * above); the argument checks and the one-launch limit are mavg_ema_run's. */
int mavg_ema_workspace_bytes(size_t n_samples, int channels, double alpha, int dtype,
                             size_t* out_bytes);

/* H: the smallest H >= 0 with (1 - alpha)^H <= 2^-30 -- 0 for alpha == 1, 30 for
 * alpha == 0.5, about 20.8 / alpha for small alpha. */
int mavg_ema_halo_frames(double alpha, long long* out_frames);

/* Describe, without launching anything, what mavg_ema_run would do:
 * "ema_tile<dtype,C=..,F=..,U=..,nt=..> alpha=.. halo_frames=H state=0|1|2|3 ... tile_frames=N ...",
 * "ema_chain<...> ... tile_frames=N records=R carry_chunk=K launches=3" or
 * "ema_strip dtype=.. C=.. L=.. strips=.. carry_chunk=K launches=3 ...".
 * flags: 1 = a d_state_in, 2 = a d_state_out, 4 = views off 16-B alignment (the
 * frame-unit form).  n_samples == 0 has no plan: MAVG_ERR_INVALID_ARG. */
int mavg_ema_plan(size_t n_samples, int channels, double alpha, int dtype, int flags,
                  char* buf, size_t buflen);

/* Biquad (second-order IIR section), per channel of an interleaved signal
 * x[f*C + c]:
 *
 *   y[f] = b0 x[f] + b1 x[f-1] + b2 x[f-2] - a1 y[f-1] - a2 y[f-2]
 *
 * -- low-pass, high-pass, band-pass, peaking and shelving EQ, DC blockers,
 * Butterworth sections, one section of lfilter / sosfilt.
 *
 * Layout and dtypes.  dtype is MAVG_F32 or MAVG_I16.  The output is ALWAYS fp32,
 * for int16 input too (n_samples floats, in d_in's layout); it must not overlap
 * d_in.  Everything is evaluated in fp64 and rounded once to fp32.
 *
 * Coefficients.  coef is five host doubles b0 b1 b2 a1 a2, normalised (a0 == 1).
 * A non-finite value, or poles that are not strictly inside the unit circle --
 * the accepted region is |a2| < 1 && |a1| < 1 + a2 -- is MAVG_ERR_INVALID_ARG.
 * a1 = a2 = 0 is a 3-tap FIR; b = (1, 0, 0), a = (0, 0) is the converting copy.
 *
 * State.  Transposed direct form II, scipy.signal.lfilter's zi / zf for a
 * normalised section:
 *
 *   y = b0 x + s1;   s1' = b1 x - a1 y + s2;   s2' = b2 x - a2 y
 *
 * d_state_in holds channels * 2 doubles, [c][0] = s1 and [c][1] = s2, in device
 * memory, 8-B aligned; NULL means zeros (frames before the first read as zero).
 * d_state_out (same shape, or NULL) receives the state after the last frame
 * from the same call.  The two state pointers must not be equal
 * (MAVG_ERR_INVALID_ARG: the tile kernel's first tiles read one while its last
 * tile writes the other).  Passing chunk i's state_out as chunk i+1's state_in
 * reproduces the one-shot output within the accuracy bar below -- NOT bitwise:
 * the association of the fp64 sums depends on the tiling.
 *
 * Halo.  With h[n] the impulse response, G = sum |h[n]| and M the largest of
 * |x| over the signal and |state_in|, H = mavg_biquad_halo_frames(coef) is a
 * frame count for which the library bounds
 *
 *   sum_{n > H} |h[n]| <= 2^-30 G
 *
 * -- not necessarily the smallest.  The envelope's H is proved; the refined H
 * below rests on an fp64 iteration whose rounding is ALLOWED 2^-32 G, an
 * allowance that is not derived (the iteration's error grows like n eps max
 * |u_n|) and is checked against the exact tail on a list of 80 filters and on
 * real-pole cases (tests/test_biquad_abi.py), and the kernels are run with it on
 * the input that maximises what it drops, x[j] = M sgn(h[t0 - j]) in front of a
 * tile that starts at t0 > H (tests/test_gpu_worst_case.py; DESIGN.md "Biquad"
 * has the measured headroom).  How it is formed: G is bounded below by the
 * largest of |b0|, |h[1]| and the gains at DC and at Nyquist.  With u_m =
 * sum_j p1^j p2^(m-1-j) over the poles p1, p2 (|u_m| <= m rho^(m-1), rho the
 * larger modulus) the response is h[n] = c1 u_n + c2 u_(n-1), c1 = b1 - a1 b0,
 * c2 = b2 - a2 b0, which gives a pole envelope for every pole pair, |h[n]| <=
 * |c1| n rho^(n-1) + |c2| (n-1) rho^(n-2), and for complex poles r e^(+-i theta)
 * the tighter |h[n]| <= E r^n, E = (|c1| + |c2| / r) / |Im p|; the tail of the
 * smaller one is summed in closed form.  Where that envelope reaches 2^-30 G
 * within 16384 frames, it is taken on to 2^-32 G and the impulse response is
 * iterated in fp64 up to there: H is then the first frame count whose iterated
 * remainder is at most 2^-31 G (both: a pole envelope, and an iterated response
 * with a bounded tail).  Otherwise H is the envelope's.  Poles within 2^-48 of
 * the circle saturate H at 2^62.  The states satisfy s1 = y - b0 x and s2 = b2
 * x - a2 y with |a2| < 1, so the dependence of a state the filter produced on
 * frames more than H back is bounded by the same tail.  A d_state_in that no
 * input produces decays with the poles alone: biquad_tile carries it for as
 * many frames as the pole envelope needs to fall to 2^-30 G, in at most the
 * first 16 tiles (see "Which states" below).
 *
 * Accuracy, every path, every output.  With y_ref the serial fp64 recurrence
 * above,
 *
 *   |y - y_ref| <= 2^-23 |y_ref| + 2^-29 G M
 *
 * and d_state_out is within 2^-29 G M of the reference state of the same call
 * (its own d_state_in), per component.
 *
 * Which states.  Both promises are made for a d_state_in the filter can reach:
 * NULL (zeros), the d_state_out of an earlier call, or lfilter_zi scaled by the
 * signal's level.  Any other d_state_in is accepted, but it excites the poles
 * alone and answers up to 1 / theta above M: for it only the outputs' bar is
 * promised (the 2^-23 |y_ref| term carries the larger response), and on
 * biquad_tile only while that response falls to 2^-30 G M within the first 16
 * tiles (tile_frames in the plan text; 16384 frames in the frame-unit form) --
 * the state is not applied past them.  d_state_out is NOT promised for such a
 * state: the serial fp64 reference itself is off by more than 2^-29 G M there
 * (its rounding is amplified by about 1 / theta^2).  biquad_chain and
 * biquad_strip apply every state without a horizon.
 * Write D = min(1 + a1 + a2, 1 - a1 + a2): small when both poles sit near +1 or
 * near -1, as for a Butterworth corner far below the sample rate.  The bar is
 * promised for D >= 2^-22 (a corner of about 3.4 Hz at 44.1 kHz).  Below that the
 * call still runs, but the cancellation of the fp64 scan grows as the poles
 * approach +-1 (the entries of a power of the state matrix are 1 / theta larger
 * than what they sum to) and nothing is promised.  The powers of the state
 * matrix are formed on the host in long double and rounded once.  Nothing is
 * promised for non-finite fp32 input.
 *
 * Ownership, stream and capture rules are mavg_ema_run's: no allocation, no
 * synchronisation, every step planned before the first is launched, nothing
 * enqueued unless MAVG_OK is returned (MAVG_ERR_HIP excepted).  The workspace
 * needs no initialisation -- every record read is written earlier in the same
 * call -- so a call may be captured into a graph with no memset node.
 * n_samples == 0: MAVG_OK, nothing enqueued, d_state_out untouched.
 *
 * Status: MAVG_ERR_INVALID_ARG for a bad dtype, channels < 1, n_samples not a
 * multiple of channels, a NULL coef, coefficients as above, equal state
 * pointers, or a NULL view with work to do; MAVG_ERR_MISALIGNED for d_in off
 * sample alignment, d_out off 4 B, a state pointer off 8 B or d_ws off 16 B;
 * MAVG_ERR_WORKSPACE for ws_bytes too small; MAVG_ERR_UNSUPPORTED past the
 * one-launch limit below.
 *
 * Dispatch, evaluated in this order (mavg_biquad_plan shows which).  With the
 * state s = (s1, s2) the recurrence is s' = A s + B x, A = [[-a1, 1], [-a2, 0]];
 * over m frames it composes to s_out = A^m s_in + b, so only the 2-vector b is
 * scanned and every multiplier is a power of A.
 *   biquad_tile   channels 1 or 2 and a halo H * channels * sample size of at
 *                 most 16 KiB (the stage limit of every tile kernel here; measured
 *                 1.09x (int16 mono at 16 KiB) to 2.14x faster than the forced
 *                 chain at 256 B, 2, 8 and 16 KiB of halo, DESIGN.md "Biquad").
 *                 One launch, no workspace.  A tile stages its H
 *                 halo frames in front of its own and rebuilds its carry state
 *                 from them.  The 16-B-unit form runs when d_in and d_out are
 *                 16-B aligned; other views run the frame-unit form (F=1 in the
 *                 plan text) over the whole signal.
 *   biquad_chain  channels 1 or 2, any stable coefficients: three launches
 *                 through one record of two doubles per tile and channel -- the
 *                 tiles' aggregates, one workgroup that turns them in place
 *                 into the tiles' carry states (and writes d_state_out), the
 *                 tiles again from their carry states.  No truncation.
 *   biquad_strip  three or more channels: the same three steps with one thread
 *                 per strip of L frames and channel at both ends (L in the plan
 *                 text) -- correct, not fast.
 *
 * Workspace (mavg_biquad_workspace_bytes): 0 for biquad_tile; for biquad_chain
 * the record count of the smaller tile of the frame-unit form (1024 frames), so
 * that a misaligned view fits, times channels * 16; for biquad_strip the strip
 * count times channels * 16.  d_ws 16-B aligned.
 *
 * Supported maximum.  Each launch takes at most 2^32 - 1 work-items, as
 * mavg_ema_run's; past it MAVG_ERR_UNSUPPORTED and nothing is enqueued.  Frame
 * and sample indices are 64-bit wherever they are not tile-local.  biquad_tile
 * (both unit forms, a state carried from an earlier chunk in and out),
 * biquad_chain (with a d_state_out) and biquad_strip are tested on 2^32 +
 * 10^6-sample signals, every output (tests/test_gpu_bigsignal_filters.py).
 */
int mavg_biquad_run(const void* d_in, float* d_out, size_t n_samples, int channels,
                    const double coef[5] /* host: b0 b1 b2 a1 a2, a0 == 1 */, int dtype,
                    const double* d_state_in /* or NULL */, double* d_state_out /* or NULL */,
                    void* d_ws, size_t ws_bytes, void* stream);

/* Device workspace mavg_biquad_run needs for these arguments (see "Workspace"
 * above); the argument checks and the one-launch limit are mavg_biquad_run's. */
int mavg_biquad_workspace_bytes(size_t n_samples, int channels, const double coef[5], int dtype,
                                size_t* out_bytes);

/* H of "Halo" above: 0 for the copy, at most 2 for a1 = a2 = 0. */
int mavg_biquad_halo_frames(const double coef[5], long long* out_frames);

/* Describe, without launching anything, what mavg_biquad_run would do:
 * "biquad_tile<dtype,C=..,F=..,U=..,nt=..> halo_frames=H state=0|1|2|3 ... tile_frames=N ...",
 * "biquad_chain<...> halo_frames=H ... tile_frames=N records=R carry_chunk=K launches=3" or
 * "biquad_strip dtype=.. C=.. L=.. strips=.. carry_chunk=K launches=3 ...".
 * flags: 1 = a d_state_in, 2 = a d_state_out, 4 = views off 16-B alignment (the
 * frame-unit form).  n_samples == 0 has no plan: MAVG_ERR_INVALID_ARG. */
int mavg_biquad_plan(size_t n_samples, int channels, const double coef[5], int dtype, int flags,
                     char* buf, size_t buflen);

/* Second-order sections: `sections` biquads in series, per channel of an
 * interleaved signal -- scipy.signal.sosfilt with normalised rows.  coef holds
 * sections x 5 host doubles, row j = b0 b1 b2 a1 a2 of section j (a0 == 1).
 * Section j is mavg_biquad_run's recurrence (transposed direct form II, the
 * states are lfilter's zi / zf); section j + 1 reads section j's output.  The
 * input is MAVG_F32 or MAVG_I16, the output ALWAYS fp32, n_samples floats in
 * d_in's layout; it must not overlap d_in.
 *
 * The intermediate.  On sos_tile (below) section j + 1 reads section j's output
 * as fp64 and only the last section's output is rounded, once, to fp32: one
 * fp64 pipeline from x to y.  On sos_loop THE INTERMEDIATE IS fp32 -- it is
 * mavg_biquad_run once per section through fp32 buffers.  flags =
 * MAVG_SOS_FP64_ONLY refuses, with MAVG_ERR_UNSUPPORTED and nothing enqueued,
 * every shape that would not run with fp64 intermediates, so a caller who
 * needs the fp64 contract never gets fp32 silently.
 *
 * State.  d_state_in / d_state_out hold [sections][channels][2] doubles in
 * device memory, 8-B aligned, or are NULL (zeros / not wanted): row j is
 * section j's (s1, s2) as mavg_biquad_run's.  They must not be equal.  Chunk
 * i's state_out as chunk i + 1's state_in reproduces the one-shot output
 * within the bars below, not bitwise.  mavg_biquad_run's "Which states"
 * paragraph carries over section by section: a state the cascade can reach
 * (NULL, an earlier call's d_state_out) is promised; any other state is applied
 * on sos_tile only while its section's pole envelope falls to 2^-30 G within
 * the 16 tiles after the first.
 *
 * Accuracy.  G_j is section j's sum |h|; m_1 = max(max |x|, |state_in[1]|),
 * m_(j+1) = max(G_j m_j, |state_in[j+1]|); y_ref is the serial fp64 cascade
 * with fp64 intermediates.  On sos_tile (and sos_none) every output satisfies
 *
 *   |y - y_ref| <= 2^-23 |y_ref| + 2^-29 sum_j ( G_j m_j prod_{i>j} G_i )
 *
 * -- each section's 2^-29 G M pushed through the gains of the sections after
 * it -- while every section meets the biquad's D >= 2^-22; component c of
 * d_state_out[j] is within the same sum taken over the sections <= j (without
 * the later gains' product past j).  On sos_loop, a separate and weaker bar:
 * each section before the last also rounds its output to fp32, which adds
 *
 *   2^-24 sum_{j < S} ( G_j m_j prod_{i>j} G_i )
 *
 * to the right-hand side (and to the states of the sections after it).
 *
 * Dispatch, evaluated in this order (mavg_sos_plan shows which):
 *   sos_none  sections == 1: mavg_biquad_run unchanged, with its workspace.
 *   sos_tile  channels 1 or 2, 2 <= sections <= 16, and a total halo sum_j H_j
 *             (H_j = mavg_biquad_halo_frames of row j; mavg_sos_halo_frames) with
 *             sum H_j * channels * 8 B <= 16 KiB: the stage limit of every tile
 *             kernel here, taken in the intermediate's dtype.  ONE filtering
 *             launch: a tile stages its 4096 / channels frames and the sum H_j
 *             frames before them as fp64 in LDS (zeros before frame 0); section
 *             j runs in place over the range that starts sum_{i>=j} H_i frames
 *             before the tile, from a zero state (from d_state_in[j] exactly
 *             where the range is cut at frame 0), and its first H_j outputs are
 *             not used.  The sections' power tables (2712 B each, formed on the
 *             host in long double and rounded once) travel as the kernel
 *             arguments of one tiny set-up launch per section that writes them
 *             to the workspace: launches = 1 + sections in the plan text.  The
 *             16-B-unit form runs when d_in and d_out are 16-B aligned, the
 *             frame-unit form (F=1) otherwise.  The rule is "wherever it fits"
 *             but for one measured exception (tools/bench_sos.py --pairs, 2^28
 *             samples, DESIGN.md "SOS"): forced against sos_loop it is 1.03x to
 *             2.21x faster at 2, 4 and 8 sections and 256 B, 2, 8 and 16 KiB of
 *             total halo, except int16 mono with TWO sections, 1.09x at 2 KiB but
 *             0.90x at 8 KiB and 0.86x at 16 KiB.  There -- MAVG_I16, one channel,
 *             two sections, sum H_j * 8 B > 2 KiB -- the rule gives the cascade
 *             to sos_loop, and MAVG_SOS_FP64_ONLY (and the hook) still run it on
 *             sos_tile.  Three sections and 3 .. 7 between the measured counts
 *             were NOT MEASURED.
 *   sos_loop  everything else -- three or more channels, longer total halos,
 *             more sections: mavg_biquad_run's launches once per section on
 *             `stream`, every section planned before the first is launched, the
 *             last landing in d_out.  fp32 intermediate; refused by
 *             MAVG_SOS_FP64_ONLY.
 *
 * Workspace (mavg_sos_workspace_bytes): sos_none mavg_biquad_run's; sos_tile
 * sections * 2712 B rounded up to 16; sos_loop one fp32 buffer of the signal's
 * size (two with three or more sections), each padded to 16 B, and the largest
 * workspace a section's mavg_biquad_run needs.  d_ws 16-B aligned.  It needs no
 * initialisation, so a call captures into a graph with no memset node.
 *
 * Ownership, stream, capture, "planned before anything is launched", "nothing
 * enqueued unless MAVG_OK" and the n_samples == 0 rule are mavg_biquad_run's.
 * Status: mavg_biquad_run's table with every row of coef checked as its coef is,
 * and: sections < 1, or flags other than 0 / MAVG_SOS_FP64_ONLY, is
 * MAVG_ERR_INVALID_ARG; MAVG_ERR_UNSUPPORTED for MAVG_SOS_FP64_ONLY on a shape
 * sos_tile does not fit (more than 16 sections among them: the loop itself
 * takes any count) and past mavg_biquad_run's one-launch limit.
 *
 * Supported maximum.  Frame and sample indices are 64-bit wherever they are not
 * tile-local.  sos_tile (both unit forms, a state carried from an earlier chunk
 * in and out, the full 16-KiB stage) and sos_loop (with one fp32 buffer and
 * with two) are tested on 2^32 + 10^6-sample signals, every output
 * (tests/test_gpu_bigsignal_filters.py).
 */
#define MAVG_SOS_FP64_ONLY 1
int mavg_sos_run(const void* d_in, float* d_out, size_t n_samples, int channels,
                 const double* coef /* host: sections x 5, rows b0 b1 b2 a1 a2, a0 == 1 */, int sections,
                 int dtype, int flags,
                 const double* d_state_in /* device [sections][channels][2] or NULL */,
                 double* d_state_out /* same shape or NULL */,
                 void* d_ws, size_t ws_bytes, void* stream);

/* Device workspace mavg_sos_run needs for these arguments (see "Workspace"
 * above); the argument checks and refusals are mavg_sos_run's. */
int mavg_sos_workspace_bytes(size_t n_samples, int channels, const double* coef, int sections,
                             int dtype, int flags, size_t* out_bytes);

/* The sum of the rows' mavg_biquad_halo_frames (saturating at 2^62). */
int mavg_sos_halo_frames(const double* coef, int sections, long long* out_frames);

/* Describe, without launching anything, what mavg_sos_run would do:
 * "sos_none biquad_...", "sos_tile<dtype,C=..,F=..> sections=S intermediate=f64
 * halo_frames=H stage_halo=Hp state=0|1|2|3 frames=.. grid=.. block=.. lds=..
 * tile_frames=N remap=.. ws=B launches=1+S" or "sos_loop dtype=.. C=.. sections=S
 * intermediate=f32 halo_frames=H state=.. frames=.. buffers=1|2 ws=B launches=L".
 * flags packs two things, in separate bit ranges: bits 0 .. 3 are mavg_sos_run's
 * flags (MAVG_SOS_FP64_ONLY), bits 4 .. 6 describe the views as
 * mavg_biquad_plan's 1 / 2 / 4 do, shifted left by four:
 * MAVG_SOS_PLAN_STATE_IN, MAVG_SOS_PLAN_STATE_OUT and MAVG_SOS_PLAN_UNALIGNED
 * (views off 16-B alignment: the frame-unit form).  n_samples == 0 has no plan:
 * MAVG_ERR_INVALID_ARG. */
#define MAVG_SOS_PLAN_STATE_IN 16
#define MAVG_SOS_PLAN_STATE_OUT 32
#define MAVG_SOS_PLAN_UNALIGNED 64
int mavg_sos_plan(size_t n_samples, int channels, const double* coef, int sections, int dtype,
                  int flags, char* buf, size_t buflen);

/* FIR filter (finite impulse response), per channel of an interleaved signal
 * x[f*channels + c] with the caller's taps h[0 .. ntaps-1]:
 *
 *     y[f] = sum_{j = 0 .. ntaps-1} h[j] * x[f-j]
 *
 * h[0] multiplies the newest frame.  dtype is MAVG_F32 or MAVG_I16; the output is
 * always fp32, n_samples floats in d_in's layout, and must not overlap d_in.
 *
 * Taps.  d_taps holds ntaps doubles in DEVICE memory, 8-B aligned, caller-owned,
 * read by the kernel on the stream.  The library never copies between host and
 * device and never reads the taps on the host, so they are not validated: a
 * non-finite tap gives non-finite outputs, not an error.  ntaps >= 1;
 * (ntaps - 1) * channels must fit an int, else MAVG_ERR_UNSUPPORTED.
 *
 * History.  Frames before frame 0 read as zero; with d_history they read as the
 * (ntaps - 1) * channels samples of dtype in front of d_in, oldest first -- the
 * convention of mavg_run.  A signal cut into chunks, each passed the last
 * ntaps - 1 frames before it, gives the one-shot outputs bit for bit.
 *
 * Arithmetic.  Each output is the fp32 rounding of ONE fp64 fma chain: the
 * accumulator starts at +0.0, then acc = fma(h[j], (double)x[f-j], acc) for
 * j = ntaps-1 down to 0 -- oldest frame first.  Zero-padded frames enter as
 * fma(h[j], 0.0, acc) or are dropped, which gives the same bits.  No chain is
 * split or reordered, so -- unlike the EMA and the biquad -- every path and form
 * is bitwise equal: fir_tile, fir_strip, both unit forms, any tiling and any
 * chunking with a history give the same bits for the same signal.
 * The accuracy that follows: |y - y_ref| <= 2^-23 |y_ref| + 2^-36 G M with
 * G = sum |h[j]|, M = max |x| over signal and history and y_ref the exact sum (a
 * chain of T <= 8192 fmas errs by at most T 2^-53 G M <= 2^-40 G M; the bar
 * leaves 16x for a reference's own rounding).  Longer tap sets scale the second
 * term by ntaps / 8192.  Nothing is promised for non-finite input.
 *
 * Ownership, stream and capture rules are mavg_run's: no allocation, no
 * synchronisation, no workspace, one launch; nothing is enqueued unless MAVG_OK
 * is returned (MAVG_ERR_HIP excepted).  Arguments are validated first;
 * n_samples == 0: MAVG_OK, nothing enqueued.
 *
 * Status: MAVG_ERR_INVALID_ARG for a bad dtype, channels < 1, ntaps < 1,
 * n_samples not a multiple of channels, or a NULL d_in, d_out or d_taps with work
 * to do; MAVG_ERR_MISALIGNED for d_in or d_history off sample alignment, d_out
 * off 4 B or d_taps off 8 B; MAVG_ERR_UNSUPPORTED as above and past the
 * one-launch limit below.
 *
 * Dispatch (mavg_fir_plan shows which):
 *   fir_tile   channels 1 or 2 and a halo (ntaps - 1) * channels * sample size of
 *              at most 16 KiB (the stage limit of every tile kernel here): fp32
 *              up to 4097 taps mono and 2049 stereo, int16 up to 8193 and 4097.
 *              A tile stages itself and its halo in LDS in the input's dtype; a
 *              lane keeps the fp64 accumulators of R consecutive frames and feeds
 *              every 16-B unit it reads from LDS to all of them; the taps arrive
 *              as wave-uniform scalar loads.  The 16-B-unit form runs when d_in
 *              and d_out are 16-B aligned; other views run the frame-unit form
 *              (F=1 in the plan text) over the whole signal.
 *   fir_strip  everything else -- three or more channels, longer tap sets: one
 *              thread per channel of a strip of L frames (L in the plan text),
 *              ntaps global reads per output -- correct, not fast.
 *
 * Supported maximum.  The launch takes at most 2^32 - 1 work-items, as
 * mavg_run's; past it MAVG_ERR_UNSUPPORTED and nothing is enqueued.  Frame and
 * sample indices are 64-bit wherever they are not tile-local.  fir_tile (both
 * unit forms, 33 taps and the full 16-KiB halo, with and without a history) and
 * fir_strip (three channels, 33 taps; not its long tap sets) are tested on 2^32 +
 * 10^6-sample signals, every output (tests/test_gpu_bigsignal_filters.py).
 */
int mavg_fir_run(const void* d_in, float* d_out, size_t n_samples, int channels,
                 const double* d_taps /* device: ntaps doubles */, int ntaps, int dtype,
                 const void* d_history /* or NULL */, void* stream);

/* Describe, without launching anything, what mavg_fir_run would do:
 * "fir_tile<dtype,C=..,F=..,U=..,R=..> taps=T halo_frames=T-1 history=0|1 ... grid=.. block=.. lds=.. tile_frames=N ..."
 * or "fir_strip dtype=.. C=.. taps=T L=.. strips=.. ...".
 * flags: 1 = a d_history, 4 = views off 16-B alignment (the frame-unit form).
 * n_samples == 0 has no plan: MAVG_ERR_INVALID_ARG. */
int mavg_fir_plan(size_t n_samples, int channels, int ntaps, int dtype, int flags,
                  char* buf, size_t buflen);

/* Describe, without launching anything, the kernel and launch geometry
 * mavg_run would use for these arguments on 16-B-aligned views
 * (e.g. "tile_scan<f32,...> grid=... block=256 ..."). */
int mavg_plan(size_t n_samples, int channels, int grade, int dtype, int algo,
              int block_size, char* buf, size_t buflen);

/* The algorithm MAVG_ALGO_AUTO resolves to for these arguments. */
int mavg_resolve_algo(size_t n_samples, int channels, int grade, int dtype, int algo);

/* Counter-based synthetic signal on the device: x[i] for global index
 * offset+i, from splitmix64(seed + offset + i).  dist 0: int16-valued
 * (as int16 or as float); dist 1: uniform [0,1) floats; dist 2: zero-mean,
 * mixed-scale, non-dyadic floats whose fp64 window sums round (the fp32
 * rounding-stress input of the parity tests).  dist 1 and 2: MAVG_F32 only. */
int mavg_fill_synthetic(void* d_out, size_t n_samples, int dtype, uint64_t seed,
                        uint64_t offset, int dist, void* stream);

/* HBM calibration (not part of the filter): d_out = d_in with one flat,
 * non-temporal 16-B load + store per thread, the best copy measured on
 * MI355X.  bench.py times it beside the filter so a result can be
 * read against the same box's achievable streaming rate.  bytes a multiple
 * of 16, both pointers 16-B aligned. */
int mavg_stream_copy(const void* d_in, void* d_out, size_t bytes, void* stream);

const char* mavg_strerror(int status);
const char* mavg_algo_name(int algo);
int mavg_abi_version(void);
/* Source id the library was compiled from: 16 hex digits of a SHA-256 over
 * csrc/ and include/ (digital_signal_processsing_amd/build_id.py, linked in by
 * csrc/Makefile).  Lets a caller prove the loaded library is the tree's. */
const char* mavg_build_id(void);

#ifdef __cplusplus
}
#endif

#endif /* MAVG_H */
