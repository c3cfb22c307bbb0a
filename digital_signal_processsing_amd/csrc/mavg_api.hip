// mavg_api.hip -- C ABI of libmavg (declared in include/mavg.h).
//
// Host-side dispatch: validates arguments (the reference never validates
// grade or channels, SURVEY.md 8b "Errors"), resolves the algorithm, sizes the
// launch and enqueues exactly one kernel on the caller's stream.  No
// allocation, no synchronisation, no exit(): the reference's CUDA_CHECK
// (gpu_utils.h:10-18) becomes a returned status.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mavg_launch.hpp"

using namespace mavg;

namespace {

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

size_t elem_size(int dtype) { return dtype == MAVG_F32 ? 4 : 2; }

// frames per 16-B unit for (dtype, C), 0 if C*elem does not divide 16
int vec_frames(int dtype, int C) {
  const int eb = (int)elem_size(dtype);
  const int fb = eb * C;
  if (fb > 16 || 16 % fb != 0) return 0;
  return 16 / fb;
}

// Bytes of the vector unit an algorithm moves per lane access when it runs
// its vector form (16 or 8), or 0 for the frame-unit (F = 1) forms.
int vec_unit_bytes(int algo, int dtype, int C) {
  const int fb = (int)elem_size(dtype) * C;
  switch (algo) {
    case MAVG_ALGO_BLELLOCH:
    case MAVG_ALGO_HILLIS:
    case MAVG_ALGO_DIRECT: return vec_frames(dtype, C) > 0 ? 16 : 0;
    case MAVG_ALGO_DIRECT_VEC2: return (fb <= 8 && 8 % fb == 0) ? 8 : 0;
    default: return 0;
  }
}

// The frame-unit (one frame per lane) form of an algorithm family.
int scalar_form(int algo) {
  switch (algo) {
    case MAVG_ALGO_BLELLOCH: return MAVG_ALGO_BLELLOCH_SCALAR;
    case MAVG_ALGO_HILLIS: return MAVG_ALGO_HILLIS_SCALAR;
    case MAVG_ALGO_DIRECT:
    case MAVG_ALGO_DIRECT_VEC2: return MAVG_ALGO_DIRECT_SCALAR;
    default: return algo;
  }
}

int validate(size_t n, int C, int k, int dtype, int algo, int block) {
  if (dtype != MAVG_I16 && dtype != MAVG_F32) return MAVG_ERR_INVALID_ARG;
  if (algo < MAVG_ALGO_AUTO || algo > MAVG_ALGO_NAIVE) return MAVG_ERR_INVALID_ARG;
  if (C < 1 || k < 1) return MAVG_ERR_INVALID_ARG;
  if (n % (size_t)C != 0) return MAVG_ERR_INVALID_ARG;
  if (block != 0 && (block < 32 || block > 1024 || block % 32 != 0)) return MAVG_ERR_INVALID_ARG;
  if (C > kMaxChannels && algo != MAVG_ALGO_AUTO && algo != MAVG_ALGO_NAIVE) return MAVG_ERR_UNSUPPORTED;
  if (n / (size_t)C > (size_t)0x3fffffffffffffffULL) return MAVG_ERR_UNSUPPORTED;
  return MAVG_OK;
}

// The flat non-temporal copy (one thread per 16 B) of any size: launches of at
// most kMaxLaunchItems work-items each (the runtime's limit is on work-items,
// mavg_launch.hpp), every one over its own part of the views.
long long flat_copy_launches(size_t bytes) {
  return ((long long)(bytes / 16) + kMaxLaunchItems - 1) / kMaxLaunchItems;
}

int launch_flat_copy(const void* in, void* out, size_t bytes, hipStream_t s) {
  static_assert(kMaxLaunchItems % kWG == 0, "whole workgroups per launch");
  const long long n = (long long)(bytes / 16);
  for (long long b = 0; b < n; b += kMaxLaunchItems) {
    const long long m = std::min(kMaxLaunchItems, n - b);
    hipLaunchKernelGGL(stream_copy_kernel<u32x4>, dim3((unsigned)((m + kWG - 1) / kWG)), dim3(kWG), 0, s,
                       static_cast<const u32x4*>(in) + b, static_cast<u32x4*>(out) + b, m);
    if (hipGetLastError() != hipSuccess) return MAVG_ERR_HIP;
  }
  return MAVG_OK;
}

// k = 1: y = x / 1 = x exactly, for every algorithm and dtype (the window is
// the sample itself; no history).  A copy instead of a scan: a telescoped
// running sum loses up to ~1e-6 relative on mixed-scale fp32 data at k = 1
// (neighbours 2^30 times larger round the differences), a copy loses nothing.
// The flat non-temporal copy when both views are 16-B aligned, else hipMemcpyAsync.
int launch_identity(int dtype, int C, const Sig& sg, hipStream_t s) {
  if ((size_t)sg.nframes > (SIZE_MAX / 4) / (size_t)C) return MAVG_ERR_UNSUPPORTED;  // the byte count stays in size_t
  const size_t bytes = (size_t)sg.nframes * (size_t)C * elem_size(dtype);
  const bool flat = aligned(sg.in, 16) && aligned(sg.out, 16) && bytes % 16 == 0;
  if (g_plan) {
    const int len = snprintf(g_plan->text, sizeof(g_plan->text), "copy<%s,C=%d> (k=1: y = x) bytes=%zu %s",
                             dtype == MAVG_F32 ? "f32" : "i16", C, bytes, flat ? "flat nt 16-B" : "hipMemcpyAsync");
    if (flat && flat_copy_launches(bytes) > 1)
      snprintf(g_plan->text + len, sizeof(g_plan->text) - len, " launches=%lld", flat_copy_launches(bytes));
    return MAVG_OK;
  }
  if (bytes == 0) return MAVG_OK;
  if (flat) return launch_flat_copy(sg.in, sg.out, bytes, s);
  return hipMemcpyAsync(sg.out, sg.in, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess ? MAVG_OK : MAVG_ERR_HIP;
}

// One launch of a concrete algorithm over a view (no alignment policy here).
int launch_algo(int algo, int dtype, int C, const Sig& sg, int k, int block, hipStream_t s, Workspace ws) {
  if (k == 1) return launch_identity(dtype, C, sg, s);
  const bool f32 = dtype == MAVG_F32;
  const bool i64acc = !f32 && k > 65535;
  switch (algo) {
    case MAVG_ALGO_BLELLOCH:
    case MAVG_ALGO_BLELLOCH_SCALAR:
    case MAVG_ALGO_HILLIS:
    case MAVG_ALGO_HILLIS_SCALAR: {
      const bool vec = (algo == MAVG_ALGO_BLELLOCH || algo == MAVG_ALGO_HILLIS);
      const bool hs = (algo == MAVG_ALGO_HILLIS || algo == MAVG_ALGO_HILLIS_SCALAR);
      if (f32) return scan_f32(C, vec, hs, sg, k, block, s, ws);
      if (i64acc) return scan_i16_wide(C, vec, hs, sg, k, block, s, ws);
      return scan_i16(C, vec, hs, sg, k, block, s, ws);
    }
    case MAVG_ALGO_DIRECT:
    case MAVG_ALGO_DIRECT_VEC2:
    case MAVG_ALGO_DIRECT_SCALAR: {
      const int width = algo == MAVG_ALGO_DIRECT ? 16 : (algo == MAVG_ALGO_DIRECT_VEC2 ? 8 : 0);
      return direct_any(dtype, i64acc, C, width, sg, k, block, s);
    }
    case MAVG_ALGO_NAIVE: return naive_any(dtype, i64acc, sg, C, k, block, s);
    default: return MAVG_ERR_INVALID_ARG;
  }
}

// 16-B-aligned dummy device pointers for plan mode: nothing is launched or dereferenced
const void* const kPlanIn = reinterpret_cast<const void*>(uintptr_t(1) << 20);
void* const kPlanOut = reinterpret_cast<void*>(uintptr_t(1) << 21);
const void* const kPlanOff = reinterpret_cast<const void*>(uintptr_t(1) << 22);

// Plan mode for one scope: the launchers describe the launch into `plan` instead of making it.
struct PlanScope {
  LaunchPlan plan{};
  PlanScope() { g_plan = &plan; }
  ~PlanScope() { g_plan = nullptr; }
  PlanScope(const PlanScope&) = delete;
  PlanScope& operator=(const PlanScope&) = delete;
};

// The caller's workspace against the `need` bytes of a plan: present, large enough, 16-B aligned.
int check_workspace(size_t need, const void* d_ws, size_t ws_bytes) {
  if (need > 0 && (d_ws == nullptr || ws_bytes < need)) return MAVG_ERR_WORKSPACE;
  if (need > 0 && !aligned(d_ws, 16)) return MAVG_ERR_MISALIGNED;
  return MAVG_OK;
}

// Workspace the launch(es) for this problem need, whatever the pointers'
// alignment: a vector algorithm on a misaligned view may run its frame-unit
// form over the whole signal instead (more, smaller look-ahead tiles).
size_t plan_ws(size_t n, int C, int k, int dtype, int algo, int block) {
  size_t need = 0;
  const int forms[2] = {algo, scalar_form(algo)};
  for (int i = 0; i < (forms[1] == forms[0] ? 1 : 2); ++i) {
    PlanScope ps;
    const Sig sg{kPlanIn, kPlanOut, nullptr, (long long)(n / (size_t)C)};
    if (launch_algo(forms[i], dtype, C, sg, k, block, nullptr, Workspace{}) == MAVG_OK)
      need = std::max(need, ps.plan.ws_bytes);
  }
  return need;
}

// Alignment policy.  A vector algorithm (16-B or 8-B lane units) needs both
// views unit-aligned.  When they are not:
//   - same offset inside a unit, a whole number of frames: the first p < F
//     frames (the "head") run in the frame-unit form of the same family, the
//     rest (the "body") in the vector form; the body's history is the head
//     itself (Sig::pre) followed, further back, by the caller's history;
//   - otherwise the frame-unit form runs over the whole signal.
// A frame-unit launch whose frames are not aligned to their own (vector)
// size moves them as element accesses (Sig::eio).  Results are identical in
// every case; only element alignment is required.
//
// mavg_run for one signal.  dry: every check mavg_run makes -- arguments, support, workspace --
// with nothing enqueued (mavg_rows_run's loop plans every row before it launches any).
int run_signal(const void* d_in, void* d_out, size_t n_samples, int channels, int grade, int dtype, int algo,
               int block_size, const void* d_history, void* d_ws, size_t ws_bytes, void* stream, bool dry) {
  const Workspace ws{d_ws, ws_bytes};
  int st = validate(n_samples, channels, grade, dtype, algo, block_size);
  if (st != MAVG_OK) return st;
  if (n_samples == 0) return MAVG_OK;
  if (d_in == nullptr || d_out == nullptr) return MAVG_ERR_INVALID_ARG;
  const size_t eb = elem_size(dtype);
  if (!aligned(d_in, eb) || !aligned(d_out, eb) || (d_history != nullptr && !aligned(d_history, eb)))
    return MAVG_ERR_MISALIGNED;
  algo = mavg_resolve_algo(n_samples, channels, grade, dtype, algo);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int C = channels;
  const size_t fb = eb * (size_t)C;
  const long long nframes = (long long)(n_samples / (size_t)C);
  // frame-unit launches: element IO when a frame is not aligned to its own vector size
  auto frame_sig = [&](const void* in, void* out, const void* hist, long long nf, int pre) {
    Sig sg{in, out, hist, nf, pre, 0};
    const bool pow2 = (fb & (fb - 1)) == 0 && fb <= 32;
    if (pow2 && (!aligned(in, fb) || !aligned(out, fb))) sg.eio = 1;
    return sg;
  };
  // one launch in plan mode: its status and its workspace against the caller's
  auto check = [&](int a, const Sig& sg) -> int {
    PlanScope ps;
    const int c = launch_algo(a, dtype, C, sg, grade, block_size, nullptr, ws);
    return c != MAVG_OK ? c : check_workspace(ps.plan.ws_bytes, d_ws, ws_bytes);
  };
  auto single = [&](int a, const Sig& sg) -> int {
    return dry ? check(a, sg) : launch_algo(a, dtype, C, sg, grade, block_size, s, ws);
  };
  const int vu = vec_unit_bytes(algo, dtype, C);
  if (vu == 0) return single(algo, frame_sig(d_in, d_out, d_history, nframes, 0));
  if (aligned(d_in, vu) && aligned(d_out, vu)) return single(algo, Sig{d_in, d_out, d_history, nframes});
  const size_t ai = reinterpret_cast<uintptr_t>(d_in) % (size_t)vu;
  const size_t ao = reinterpret_cast<uintptr_t>(d_out) % (size_t)vu;
  const int sf = scalar_form(algo);
  if (ai != ao || ai % fb != 0) return single(sf, frame_sig(d_in, d_out, d_history, nframes, 0));
  const long long p = std::min<long long>(nframes, (long long)(((size_t)vu - ai) / fb));
  const Sig head = frame_sig(d_in, d_out, d_history, p, 0);
  const size_t off = (size_t)p * fb;
  const void* hist_body = d_history != nullptr ? static_cast<const char*>(d_history) + off : nullptr;
  const Sig body{static_cast<const char*>(d_in) + off, static_cast<char*>(d_out) + off, hist_body, nframes - p,
                 (int)p, 0};
  // both launches are first made in plan mode: an error of the second one
  // (e.g. a workspace that covers the head but not the body) must leave
  // nothing on the stream (mavg.h)
  for (int part = 0; part < (p == nframes ? 1 : 2); ++part) {
    st = part == 0 ? check(sf, head) : check(algo, body);
    if (st != MAVG_OK) return st;
  }
  if (dry) return MAVG_OK;
  st = launch_algo(sf, dtype, C, head, grade, block_size, s, ws);
  if (st != MAVG_OK || p == nframes) return st;
  return launch_algo(algo, dtype, C, body, grade, block_size, s, ws);
}

// The per-row loops of mavg_rows_run and mavg_ragged_run.  The workspace contract is the
// *_workspace_bytes call's -- what a signal of `ws_samples` samples needs, whatever the rows'
// alignment, not only what these rows' forms happen to need.  Then the first `ndry` rows are
// dry-run and every row is launched: row_run(r, dry).
template <typename RowRun>
int run_row_loop(size_t rows, size_t ndry, size_t ws_samples, int C, int k, int dtype, const void* d_ws,
                 size_t ws_bytes, RowRun row_run) {
  const size_t need = plan_ws(ws_samples, C, k, dtype, mavg_resolve_algo(ws_samples, C, k, dtype, MAVG_ALGO_AUTO), 0);
  int c = check_workspace(need, d_ws, ws_bytes);
  for (size_t r = 0; c == MAVG_OK && r < ndry; ++r) c = row_run(r, true);
  for (size_t r = 0; c == MAVG_OK && r < rows; ++r) c = row_run(r, false);
  return c;
}

// unit / eio of a batch launch (RowsSig, RaggedSig) from its views' alignment
template <typename S>
S with_alignment(S rs, int C, int dtype) {
  const size_t fb = elem_size(dtype) * (size_t)C;
  rs.unit = aligned(rs.in, 16) && aligned(rs.out, 16);
  rs.eio = !rs.unit && (!aligned(rs.in, fb) || !aligned(rs.out, fb)) ? 1 : 0;
  return rs;
}

// ---- rows (mavg_rows_run) -------------------------------------------------------------------
// Arguments of the three rows entry points, as validate() does for mavg_run; *total = the
// batch's frames.
int validate_rows(size_t rows, size_t row_frames, int C, int k, int dtype, size_t* total) {
  if (dtype != MAVG_I16 && dtype != MAVG_F32) return MAVG_ERR_INVALID_ARG;
  if (C < 1 || k < 1) return MAVG_ERR_INVALID_ARG;
  *total = 0;
  if (rows == 0 || row_frames == 0) return MAVG_OK;
  const size_t lim = (size_t)0x3fffffffffffffffULL;  // below 2^62 frames, as mavg_run
  if (row_frames > lim / rows) return MAVG_ERR_UNSUPPORTED;
  const size_t frames = rows * row_frames;
  if (frames > (SIZE_MAX / 4) / (size_t)C) return MAVG_ERR_UNSUPPORTED;  // the byte count stays in size_t
  *total = frames;
  return MAVG_OK;
}

// The dispatch rule: the one-launch segmented scan for zero-history batches of one or two
// channels whose effective halo fits its LDS stage (int16: sums in int32, grade <= 65535) and
// whose rows are shorter than kRowsLoopRowBytes; everything else runs the single-signal dispatch
// once per row ("rows_loop").
// kRowsLoopRowBytes is the measured boundary (DESIGN.md "Rows", tools/bench_rows.py, 2^30
// samples, k = 1024): a per-row loop of single-signal launches costs ~10 us a row on the host,
// so it loses by 82x .. 32000x at rows of 128 KiB .. 1 KB, by 1.2x / 1.1x (fp32 / int16 stereo)
// at rows of 32 MiB -- and ties (fp32, 0.99x) or wins (int16 stereo, 0.93x) at rows of 64 MiB,
// where every row fills the device by itself and runs the single-signal tiles (0.78 - 0.82 of
// peak against the rows scan's 0.59 - 0.67).
constexpr size_t kRowsLoopRowBytes = (size_t)64 << 20;
bool rows_fast_path(size_t row_frames, int C, int k, int dtype, bool with_history) {
  if (with_history || C > 2) return false;
  if (dtype == MAVG_I16 && k > 65535) return false;
  if (k == 1) return true;  // the flat copy over the whole batch
  if (row_frames >= kRowsLoopRowBytes / (elem_size(dtype) * (size_t)C)) return false;
  return rows_scan_fits(dtype, C, row_frames, k);
}

// The fast path's one launch (plan mode when g_plan is set); views of any sample alignment.
int rows_fast_launch(const void* in, void* out, size_t rows, size_t row_frames, size_t frames, int C, int k, int dtype,
                     hipStream_t s) {
  if (k == 1) return launch_identity(dtype, C, Sig{in, out, nullptr, (long long)frames}, s);
  return rows_scan_any(dtype, C, with_alignment(RowsSig{in, out, rows, row_frames}, C, dtype), k, s);
}

// Rows whose alignment classes cover the batch's: row r's views sit r * row_bytes further, and
// r * row_bytes mod 16 repeats after at most 16 rows.
size_t rows_alignment_period(size_t rows) { return std::min<size_t>(rows, 16); }

// ---- ragged rows (mavg_ragged_run) ----------------------------------------------------------
// Arguments of the three ragged entry points and the host offsets: *total = off[rows], *longest =
// the longest row, both in frames (0 for an empty batch).
int validate_ragged(const int64_t* off, size_t rows, int C, int k, int dtype, size_t* total, size_t* longest) {
  if (dtype != MAVG_I16 && dtype != MAVG_F32) return MAVG_ERR_INVALID_ARG;
  if (C < 1 || k < 1) return MAVG_ERR_INVALID_ARG;
  *total = 0;
  *longest = 0;
  if (rows == 0) return MAVG_OK;
  if (off == nullptr || off[0] != 0) return MAVG_ERR_INVALID_ARG;
  if (rows > (size_t)0x3fffffffffffffffULL) return MAVG_ERR_UNSUPPORTED;  // row indices stay in int64
  int64_t longest_row = 0;
  for (size_t r = 0; r < rows; ++r) {
    if (off[r + 1] < off[r]) return MAVG_ERR_INVALID_ARG;
    longest_row = std::max(longest_row, off[r + 1] - off[r]);
  }
  const size_t frames = (size_t)off[rows];
  if (frames > (size_t)0x3fffffffffffffffULL) return MAVG_ERR_UNSUPPORTED;  // below 2^62 frames, as mavg_run
  if (frames > (SIZE_MAX / 4) / (size_t)C) return MAVG_ERR_UNSUPPORTED;     // the byte count stays in size_t
  *total = frames;
  *longest = (size_t)longest_row;
  return MAVG_OK;
}

// The dispatch rule: the one-launch ragged scan for batches of one or two channels whose
// effective halo min(grade, longest row) fits its LDS (int16: sums in int32, grade <= 65535);
// everything else runs the single-signal dispatch once per non-empty row ("ragged_loop").  The
// rows scan's 64-MiB-row rule is NOT carried over: it was measured on uniform batches, and a
// batch with one huge row among small ones has not been measured (DESIGN.md "Ragged").
bool ragged_fast_path(size_t longest, int C, int k, int dtype) {
  if (C > 2) return false;
  if (dtype == MAVG_I16 && k > 65535) return false;
  if (k == 1) return true;  // the flat copy over the packed stream
  return ragged_scan_fits(dtype, C, longest, k);
}

// The fast path's one launch (plan mode when g_plan is set); views of any sample alignment.
int ragged_fast_launch(const void* in, void* out, const void* d_off, size_t rows, size_t frames, size_t longest, int C,
                       int k, int dtype, hipStream_t s) {
  if (k == 1) return launch_identity(dtype, C, Sig{in, out, nullptr, (long long)frames}, s);
  return ragged_scan_any(dtype, C, with_alignment(RaggedSig{in, out, d_off, rows, frames, longest}, C, dtype), k, s);
}

// ---- decimated (mavg_decim_run) -------------------------------------------------------------
// Arguments of the decimated entry points: validate()'s for the signal, then hop and phase;
// *out_frames = len(range(phase, frames, hop)).
int validate_decim(size_t n, int C, int k, int hop, int phase, int dtype, size_t* out_frames) {
  const int st = validate(n, C, k, dtype, MAVG_ALGO_AUTO, 0);
  if (st == MAVG_ERR_INVALID_ARG) return st;
  if (hop < 1 || phase < 0 || phase >= hop) return MAVG_ERR_INVALID_ARG;
  if (st != MAVG_OK) return st;
  const size_t frames = n / (size_t)C;
  *out_frames = frames > (size_t)phase ? (frames - (size_t)phase + (size_t)hop - 1) / (size_t)hop : 0;
  return MAVG_OK;
}

// The window sum reads k frames per output and each of them once when hop >= grade; its time goes
// with out_frames x (a per-wave cost + the window), the scan's with the signal.  Measured with both
// paths forced on one shape (tools/bench_decim.py --pairs, 2^30 samples, DESIGN.md "Decimated",
// window / scan in ms, fp32 mono | int16 stereo):
//   256-B window, hop = 4 grade: 1.29 / 1.03 | 0.93 / 0.49 (the scan's); 512 B: 0.67 / 0.96 | 0.48 / 0.47
//   1 KiB: hop = grade 1.36 / 0.99 | 0.97 / 0.48, 1.5 grade 0.97 / 0.97 | 0.68 / 0.49, 4 grade 0.37 / 0.98 | 0.26 / 0.46
//   2 KiB: hop = grade 0.96 / 0.97 | 0.63 / 0.47, 1.5 grade 0.69 / 0.99 | 0.43 / 0.46
//   4 KiB: hop = grade 0.76 / 1.04 | 0.51 / 0.53, 1.5 grade 0.53 / 0.99 | 0.34 / 0.53, 2 grade 0.40 / 1.01 | 0.26 / 0.53
//   8 KiB: hop = grade 0.69 / 1.22 | 0.35 / 0.65
// So: windows of 4 KiB and more from hop == grade on (a win or a tie at the boundary), windows of
// 1 KiB .. 4 KiB from hop == 2 grade on (the crossover lies between 1 and 1.5 grade at 2 KiB and
// between 1.5 and 2 grade at 1 KiB: a margin of up to a third in hop), shorter windows never (the
// crossover in window length lies between 256 B and 1 KiB at hop = 4 grade).
constexpr long long kDecimWindowMinBytes = 1024;
constexpr long long kDecimWindowHopRatio = 2;
constexpr long long kDecimWindowDenseBytes = 4096;  // from hop == grade on

// The dispatch rule for hop >= 2, in the order mavg.h gives; *path = kDecimWindow / Scan / Full.
// The test hook's forced path replaces the rule: MAVG_ERR_UNSUPPORTED where that path cannot
// take the shape.
int decim_path(int C, int k, int hop, int dtype, int* path) {
  const bool scan_ok = hop >= 2 && decim_scan_fits(dtype, C, k);
  const bool window_can = C <= kMaxChannels;
  int forced = kDecimAuto;
#ifdef MAVG_TEST_HOOKS
  forced = g_test_decim_path.load(std::memory_order_relaxed);
#endif
  if (forced != kDecimAuto) {
    if ((forced == kDecimScan && !scan_ok) || (forced == kDecimWindow && !window_can)) return MAVG_ERR_UNSUPPORTED;
    *path = forced;
    return MAVG_OK;
  }
  const long long window_bytes = (long long)k * C * (long long)elem_size(dtype);
  const bool window_ok = window_can && hop >= k && window_bytes >= kDecimWindowMinBytes;
  if (window_ok && ((long long)hop >= kDecimWindowHopRatio * k || window_bytes >= kDecimWindowDenseBytes || !scan_ok))
    *path = kDecimWindow;
  else *path = scan_ok ? kDecimScan : kDecimFull;
  return MAVG_OK;
}

struct DecimCall {
  const void* in;
  void* out;
  const void* hist;
  size_t n, out_frames;
  int C, k, hop, phase, dtype;
};

// The one launch of decim_scan / decim_window (plan mode when g_plan is set); views of any sample
// alignment.
int decim_fast_launch(int path, const DecimCall& a, hipStream_t s) {
  DecimSig ds{a.in, a.out, a.hist, a.n / (size_t)a.C, a.out_frames, a.hop, a.phase};
  ds.unit = aligned(a.in, 16);
  if (path == kDecimWindow) {
    ds.eio = ds.unit ? 0 : 1;
    return decim_window_any(a.dtype, a.C, ds, a.k, s);
  }
  ds.eio = !ds.unit && !aligned(a.in, elem_size(a.dtype) * (size_t)a.C) ? 1 : 0;
  return decim_scan_any(a.dtype, a.C, ds, a.k, s);
}

// decim_full's workspace: the full-rate output (16-B padded), then mavg_run's own workspace
int decim_full_layout(const DecimCall& a, size_t* full_bytes, size_t* inner) {
  if (a.n > (SIZE_MAX / 4 - 15)) return MAVG_ERR_UNSUPPORTED;  // the byte count stays in size_t
  *full_bytes = (a.n * elem_size(a.dtype) + 15) & ~(size_t)15;
  return mavg_workspace_bytes(a.n, a.C, a.k, a.dtype, MAVG_ALGO_AUTO, 0, inner);
}

// decim_full: mavg_run (AUTO, block 0) into the workspace, then the strided gather.  Both steps
// are planned before the first is launched: an error leaves the stream untouched.
int decim_full_run(const DecimCall& a, void* d_ws, size_t ws_bytes, void* stream) {
  size_t full_bytes = 0, inner = 0;
  int st = decim_full_layout(a, &full_bytes, &inner);
  if (st != MAVG_OK) return st;
  st = check_workspace(full_bytes + inner, d_ws, ws_bytes);
  if (st != MAVG_OK) return st;
  char* const full = static_cast<char*>(d_ws);
  void* const iws = inner > 0 ? full + full_bytes : nullptr;
  const DecimSig ds{full, a.out, nullptr, a.n / (size_t)a.C, a.out_frames, a.hop, a.phase};
  st = run_signal(a.in, full, a.n, a.C, a.k, a.dtype, MAVG_ALGO_AUTO, 0, a.hist, iws, inner, stream, true);
  if (st != MAVG_OK) return st;
  {
    PlanScope ps;
    st = decim_gather_any(a.dtype, a.C, full, ds, nullptr);
    if (st != MAVG_OK) return st;
  }
  st = run_signal(a.in, full, a.n, a.C, a.k, a.dtype, MAVG_ALGO_AUTO, 0, a.hist, iws, inner, stream, false);
  if (st != MAVG_OK) return st;
  return decim_gather_any(a.dtype, a.C, full, ds, static_cast<hipStream_t>(stream));
}

// ---- cascaded (mavg_cascade_run) ------------------------------------------------------------
// Arguments of the cascaded entry points: validate()'s for the signal, then passes; the total
// halo passes * (grade - 1) frames must stay in int.
int validate_cascade(size_t n, int C, int k, int passes, int dtype) {
  const int st = validate(n, C, k, dtype, MAVG_ALGO_AUTO, 0);
  if (st == MAVG_ERR_INVALID_ARG) return st;
  if (passes < 1) return MAVG_ERR_INVALID_ARG;
  if (st != MAVG_OK) return st;
  if ((long long)passes * (long long)(k - 1) > 0x7fffffffLL) return MAVG_ERR_UNSUPPORTED;
  return MAVG_OK;
}

// The dispatch rule past cascade_none, in the order mavg.h gives; *path = kCascadeTile / Loop: the
// fused kernel where it can take the cascade (cascade_tile_fits) and measured faster
// (cascade_tile_preferred).  The test hook's forced path replaces the rule: MAVG_ERR_UNSUPPORTED
// where the kernel cannot take the shape.
int cascade_path(int C, int k, int passes, int dtype, int* path) {
  const bool tile_ok = cascade_tile_fits(dtype, C, k, passes);
  int forced = kCascadeAuto;
#ifdef MAVG_TEST_HOOKS
  forced = g_test_cascade_path.load(std::memory_order_relaxed);
#endif
  if (forced == kCascadeTile && !tile_ok) return MAVG_ERR_UNSUPPORTED;
  const bool rule = tile_ok && cascade_tile_preferred(dtype, C, k, passes);
  *path = forced != kCascadeAuto ? forced : rule ? kCascadeTile : kCascadeLoop;
  return MAVG_OK;
}

struct CascadeCall {
  const void* in;
  void* out;
  const void* hist;
  size_t n;
  int C, k, passes, dtype;
};

// The one launch of cascade_tile (plan mode when g_plan is set); views of any sample alignment.
int cascade_tile_launch(const CascadeCall& a, hipStream_t s) {
  CascadeSig cs{a.in, a.out, a.hist, a.n / (size_t)a.C};
  cs.unit = aligned(a.in, 16) && aligned(a.out, 16);
  cs.eio = !cs.unit && !aligned(a.in, elem_size(a.dtype) * (size_t)a.C) ? 1 : 0;
  return cascade_tile_any(a.dtype, a.C, cs, a.k, a.passes, s);
}

// ---- moments (mavg_stat_run) -----------------------------------------------------------------
int validate_stat(size_t n, int C, int k, int stat, int dtype) {
  if (stat < MAVG_STAT_MEANSQ || stat > MAVG_STAT_STD) return MAVG_ERR_INVALID_ARG;
  return validate(n, C, k, dtype, MAVG_ALGO_AUTO, 0);
}

// The dispatch rule, in the order mavg.h gives; *path = kStatTile / kStatStrip: the tile kernel
// wherever it takes the window (stat_tile_fits; it measured faster than the strip over that whole range).  The test hook's
// forced path replaces the rule: MAVG_ERR_UNSUPPORTED where the tile kernel cannot take the shape.
int stat_path(int C, int k, int dtype, int* path) {
  const bool tile_ok = stat_tile_fits(dtype, C, k);
  int forced = kStatAuto;
#ifdef MAVG_TEST_HOOKS
  forced = g_test_stat_path.load(std::memory_order_relaxed);
#endif
  if (forced == kStatTile && !tile_ok) return MAVG_ERR_UNSUPPORTED;
  *path = forced != kStatAuto ? forced : tile_ok ? kStatTile : kStatStrip;
  return MAVG_OK;
}

struct StatCall {
  const void* in;
  float* out;
  float* mean;
  const void* hist;
  size_t n;
  int C, k, stat, dtype;
};

// The one launch of stat_tile / stat_strip (plan mode when g_plan is set); views of any sample
// alignment.
int stat_launch(int path, const StatCall& a, hipStream_t s) {
  StatSig ss{a.in, a.out, a.mean, a.hist, a.n / (size_t)a.C};
  if (path == kStatStrip) return stat_strip_any(a.dtype, a.C, ss, a.k, a.stat, s);
  ss.unit = aligned(a.in, 16) && aligned(a.out, 16) && (a.mean == nullptr || aligned(a.mean, 16));
  ss.eio = !ss.unit && !aligned(a.in, elem_size(a.dtype) * (size_t)a.C) ? 1 : 0;
  return stat_tile_any(a.dtype, a.C, ss, a.k, a.stat, s);
}

// ---- extrema (mavg_extrema_run) --------------------------------------------------------------
// The dispatch rule, in the order mavg.h gives; *path = kExtremaTile / kExtremaStrip: the tile
// kernel wherever it takes the window (extrema_tile_fits).  The test hook's forced path replaces
// the rule: MAVG_ERR_UNSUPPORTED where the tile kernel cannot take the shape.
int extrema_path(int C, int k, int dtype, int* path) {
  const bool tile_ok = extrema_tile_fits(dtype, C, k);
  int forced = kExtremaAuto;
#ifdef MAVG_TEST_HOOKS
  forced = g_test_extrema_path.load(std::memory_order_relaxed);
#endif
  if (forced == kExtremaTile && !tile_ok) return MAVG_ERR_UNSUPPORTED;
  *path = forced != kExtremaAuto ? forced : tile_ok ? kExtremaTile : kExtremaStrip;
  return MAVG_OK;
}

struct ExtremaCall {
  const void* in;
  void* omax;
  void* omin;
  const void* hist;
  size_t n;
  int C, k, dtype;
};

// The one launch of extrema_tile / extrema_strip (plan mode when g_plan is set); views of any
// sample alignment: the 16-B-unit form when the input and every given output are 16-B aligned,
// else the frame-unit form over the whole signal (no head is peeled).
int extrema_launch(int path, const ExtremaCall& a, hipStream_t s) {
  ExtremaSig es{a.in, a.omax, a.omin, a.hist, a.n / (size_t)a.C};
  if (path == kExtremaStrip) return extrema_strip_any(a.dtype, a.C, es, a.k, s);
  es.unit = aligned(a.in, 16) && (a.omax == nullptr || aligned(a.omax, 16)) && (a.omin == nullptr || aligned(a.omin, 16));
  es.eio = !es.unit && !aligned(a.in, elem_size(a.dtype) * (size_t)a.C) ? 1 : 0;
  return extrema_tile_any(a.dtype, a.C, es, a.k, s);
}

// ---- FIR filter (mavg_fir_run) -----------------------------------------------------------------
int validate_fir(size_t n, int C, int ntaps, int dtype) {
  const int st = validate(n, C, 1, dtype, MAVG_ALGO_AUTO, 0);
  if (st != MAVG_OK) return st;
  if (ntaps < 1) return MAVG_ERR_INVALID_ARG;
  if ((long long)(ntaps - 1) * (long long)C > 0x7fffffffLL) return MAVG_ERR_UNSUPPORTED;  // the history's samples
  return MAVG_OK;
}

// The dispatch rule: *path = kFirTile wherever the tile kernel takes the taps (fir_tile_fits), else
// kFirStrip.  The test hook's forced path replaces the rule: MAVG_ERR_UNSUPPORTED where the tile
// kernel cannot take the shape.
int fir_path(int C, int ntaps, int dtype, int* path) {
  const bool tile_ok = fir_tile_fits(dtype, C, ntaps);
  int forced = kFirAuto;
#ifdef MAVG_TEST_HOOKS
  forced = g_test_fir_path.load(std::memory_order_relaxed);
#endif
  if (forced == kFirTile && !tile_ok) return MAVG_ERR_UNSUPPORTED;
  *path = forced != kFirAuto ? forced : tile_ok ? kFirTile : kFirStrip;
  return MAVG_OK;
}

struct FirCall {
  const void* in;
  float* out;
  const void* hist;
  const double* taps;
  size_t n;
  int C, ntaps, dtype;
};

// The one launch of fir_tile / fir_strip (plan mode when g_plan is set); views of any sample
// alignment: the 16-B-unit form when the input and the output are 16-B aligned, else the frame-unit
// form over the whole signal (no head is peeled).
int fir_launch(int path, const FirCall& a, hipStream_t s) {
  FirSig fs{a.in, a.out, a.hist, a.taps, a.n / (size_t)a.C};
  if (path == kFirStrip) return fir_strip_any(a.dtype, a.C, fs, a.ntaps, s);
  fs.unit = aligned(a.in, 16) && aligned(a.out, 16);
  fs.eio = !fs.unit && !aligned(a.in, elem_size(a.dtype) * (size_t)a.C) ? 1 : 0;
  return fir_tile_any(a.dtype, a.C, fs, a.ntaps, s);
}

// ---- exponential moving average (mavg_ema_run) -----------------------------------------------
int validate_ema(size_t n, int C, double alpha, int dtype) {
  const int st = validate(n, C, 1, dtype, MAVG_ALGO_AUTO, 0);
  if (st != MAVG_OK) return st;
  // (below 2^-52, 1 - alpha is 1 in fp64: the filter would never forget)
  if (!std::isfinite(alpha) || !(alpha > 0.0) || alpha > 1.0 || alpha < 0x1p-52) return MAVG_ERR_INVALID_ARG;
  return MAVG_OK;
}

// The dispatch rule, in the order mavg.h gives; *path = kEmaTile / kEmaChain / kEmaStrip.  The test
// hook's forced path replaces the rule: MAVG_ERR_UNSUPPORTED where the forced kernel cannot take
// the shape (a tile past the stage limit, a tile or chain with three or more channels).
int ema_path(int C, double alpha, int dtype, int* path) {
  const bool tile_ok = ema_tile_fits(dtype, C, alpha);
  const bool chain_ok = C <= 2;
  int forced = kEmaAuto;
#ifdef MAVG_TEST_HOOKS
  forced = g_test_ema_path.load(std::memory_order_relaxed);
#endif
  if ((forced == kEmaTile && !tile_ok) || (forced == kEmaChain && !chain_ok)) return MAVG_ERR_UNSUPPORTED;
  *path = forced != kEmaAuto ? forced : tile_ok ? kEmaTile : chain_ok ? kEmaChain : kEmaStrip;
  return MAVG_OK;
}

struct EmaCall {
  const void* in;
  float* out;
  const double* state_in;
  double* state_out;
  size_t n;
  int C;
  double alpha;
  int dtype;
};

// what mavg_ema_workspace_bytes returns for a path
int ema_ws_bytes(int path, const EmaCall& a, size_t* bytes) {
  *bytes = 0;
  if (path == kEmaTile) return MAVG_OK;
  const size_t nframes = a.n / (size_t)a.C;
  return path == kEmaChain ? ema_chain_ws_bytes(nframes, a.C, bytes) : ema_strip_ws_bytes(nframes, a.C, bytes);
}

// The launches of one path (plan mode when g_plan is set); views of any sample alignment: the
// 16-B-unit form when d_in and d_out are 16-B aligned, else the frame-unit form over the whole
// signal (no head is peeled).
int ema_launch(int path, const EmaCall& a, Workspace ws, hipStream_t s) {
  EmaSig es{a.in, a.out, a.state_in, a.state_out, a.n / (size_t)a.C, a.alpha};
  if (path == kEmaStrip) return ema_strip_any(a.dtype, a.C, es, ws, s);
  es.unit = aligned(a.in, 16) && aligned(a.out, 16);
  es.eio = !es.unit && !aligned(a.in, elem_size(a.dtype) * (size_t)a.C) ? 1 : 0;
  return path == kEmaTile ? ema_tile_any(a.dtype, a.C, es, s) : ema_chain_any(a.dtype, a.C, es, ws, s);
}

// ---- biquad (mavg_biquad_run) -------------------------------------------------------------------
// b0 b1 b2 a1 a2 finite, the poles strictly inside the unit circle (the stability triangle)
int validate_biquad(size_t n, int C, const double* coef, int dtype) {
  const int st = validate(n, C, 1, dtype, MAVG_ALGO_AUTO, 0);
  if (st != MAVG_OK) return st;
  if (coef == nullptr) return MAVG_ERR_INVALID_ARG;
  for (int i = 0; i < 5; ++i)
    if (!std::isfinite(coef[i])) return MAVG_ERR_INVALID_ARG;
  const double a1 = coef[3], a2 = coef[4];
  if (!(std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2)) return MAVG_ERR_INVALID_ARG;
  return MAVG_OK;
}

// The dispatch rule, in the order mavg.h gives; *path = kBiquadTile / kBiquadChain / kBiquadStrip.
// The test hook's forced path replaces the rule: MAVG_ERR_UNSUPPORTED where the forced kernel cannot
// take the shape (a tile past the stage limit, a tile or chain with three or more channels).
int biquad_path(int C, long long halo, int dtype, int* path) {
  const bool tile_ok = biquad_tile_fits(dtype, C, halo);
  const bool chain_ok = C <= 2;
  int forced = kBiquadAuto;
#ifdef MAVG_TEST_HOOKS
  forced = g_test_biquad_path.load(std::memory_order_relaxed);
#endif
  if ((forced == kBiquadTile && !tile_ok) || (forced == kBiquadChain && !chain_ok)) return MAVG_ERR_UNSUPPORTED;
  *path = forced != kBiquadAuto ? forced : tile_ok ? kBiquadTile : chain_ok ? kBiquadChain : kBiquadStrip;
  return MAVG_OK;
}

struct BiquadCall {
  const void* in;
  float* out;
  const double* state_in;
  double* state_out;
  size_t n;
  int C;
  const double* coef;
  long long halo;
  int dtype;
};

// what mavg_biquad_workspace_bytes returns for a path
int biquad_ws_bytes(int path, const BiquadCall& a, size_t* bytes) {
  *bytes = 0;
  if (path == kBiquadTile) return MAVG_OK;
  const size_t nframes = a.n / (size_t)a.C;
  return path == kBiquadChain ? biquad_chain_ws_bytes(nframes, a.C, bytes) : biquad_strip_ws_bytes(nframes, a.C, bytes);
}

// The launches of one path (plan mode when g_plan is set); views of any sample alignment: the
// 16-B-unit form when d_in and d_out are 16-B aligned, else the frame-unit form over the whole
// signal (no head is peeled).
int biquad_launch(int path, const BiquadCall& a, Workspace ws, hipStream_t s) {
  BiquadSig bs{a.in, a.out, a.state_in, a.state_out, a.n / (size_t)a.C,
               {a.coef[0], a.coef[1], a.coef[2], a.coef[3], a.coef[4]}, a.halo};
  if (path == kBiquadStrip) return biquad_strip_any(a.dtype, a.C, bs, ws, s);
  bs.unit = aligned(a.in, 16) && aligned(a.out, 16);
  bs.eio = !bs.unit && !aligned(a.in, elem_size(a.dtype) * (size_t)a.C) ? 1 : 0;
  return path == kBiquadTile ? biquad_tile_any(a.dtype, a.C, bs, s) : biquad_chain_any(a.dtype, a.C, bs, ws, s);
}

// ---- second-order sections (mavg_sos_run) -------------------------------------------------------
constexpr long long kSosHaloSaturated = 1LL << 62;
constexpr int kSosPlanShift = 4;  // mavg_sos_plan's flags: the view bits sit above the run flags
constexpr int kSosMaxLoopSections = 1 << 20;
constexpr long long kSosI16MonoPairHaloBytes = 2048;  // (sos_path)

// the biquad's checks on every row
int validate_sos(size_t n, int C, const double* coef, int sections, int dtype) {
  const int st = validate(n, C, 1, dtype, MAVG_ALGO_AUTO, 0);
  if (st != MAVG_OK) return st;
  if (coef == nullptr || sections < 1) return MAVG_ERR_INVALID_ARG;
  for (int j = 0; j < sections; ++j) {
    const int sj = validate_biquad(n, C, coef + 5 * (size_t)j, dtype);
    if (sj != MAVG_OK) return sj;
  }
  return MAVG_OK;
}

struct SosCall {
  const void* in;
  float* out;
  const double* state_in;
  double* state_out;
  size_t n;
  int C;
  const double* coef;
  int sections;
  int dtype;
  int flags;
  std::vector<long long> halo;  // the rows' H
  long long sum_halo;           // saturates at kSosHaloSaturated

  void form_halos() {
    halo.resize((size_t)sections);
    sum_halo = 0;
    for (int j = 0; j < sections; ++j) {
      halo[(size_t)j] = biquad_halo_frames(coef + 5 * (size_t)j);
      sum_halo = std::min(kSosHaloSaturated, sum_halo + std::min(halo[(size_t)j], kSosHaloSaturated));
    }
  }
};

// The dispatch rule for two or more sections, in the order mavg.h gives; *path = kSosTile /
// kSosLoop.  The test hook's forced path replaces the rule; a forced sos_tile that cannot take the
// shape, and MAVG_SOS_FP64_ONLY on a shape the fused kernel does not fit, are MAVG_ERR_UNSUPPORTED.
int sos_path(const SosCall& a, int* path) {
  const bool tile_ok = sos_tile_fits(a.C, a.sections, a.sum_halo);
  // The one part of the fitted range where the fused kernel measured slower than the loop
  // (tools/bench_sos.py --pairs, DESIGN.md "SOS"): int16 mono, two sections, 0.90x at 8 KiB and
  // 0.86x at 16 KiB of total halo against 1.09x at 2 KiB.  The rule gives it to the loop past
  // 2 KiB; MAVG_SOS_FP64_ONLY and the hook still reach the tile there.
  const bool slower = a.dtype == MAVG_I16 && a.C == 1 && a.sections == 2 && a.sum_halo * 8 > kSosI16MonoPairHaloBytes;
  const bool want_tile = tile_ok && (!slower || (a.flags & MAVG_SOS_FP64_ONLY) != 0);
  int forced = kSosAuto;
#ifdef MAVG_TEST_HOOKS
  forced = g_test_sos_path.load(std::memory_order_relaxed);
#endif
  if (forced == kSosTile && !tile_ok) return MAVG_ERR_UNSUPPORTED;
  *path = forced != kSosAuto ? forced : want_tile ? kSosTile : kSosLoop;
  if (*path == kSosLoop && (a.flags & MAVG_SOS_FP64_ONLY) != 0) return MAVG_ERR_UNSUPPORTED;
  if (*path == kSosLoop && a.sections > kSosMaxLoopSections) return MAVG_ERR_UNSUPPORTED;
  return MAVG_OK;
}

int sos_tile_launch(const SosCall& a, Workspace ws, hipStream_t s) {
  SosSig ss{a.in, a.out, a.state_in, a.state_out, a.n / (size_t)a.C, a.coef, a.sections, a.halo.data()};
  ss.unit = aligned(a.in, 16) && aligned(a.out, 16);
  ss.eio = !ss.unit && !aligned(a.in, elem_size(a.dtype) * (size_t)a.C) ? 1 : 0;
  return sos_tile_any(a.dtype, a.C, ss, ws, s);
}

// sos_loop's workspace, in this order: one fp32 buffer of the signal's size (16-B padded), a second
// one with three or more sections, then the largest workspace a section's mavg_biquad_run needs.
struct SosLoopLayout {
  size_t buf = 0, inner = 0;
  int nbuf = 0;
  int launches = 0;
  size_t bytes() const { return (size_t)nbuf * buf + inner; }
};

// Section j of the loop as a biquad call: from d_in or the buffer section j - 1 wrote ((j - 1) & 1)
// to the buffer j & 1 or d_out.  launch == false: every section is planned (its limits, its
// workspace, its launches) with the buffers at `base`, nothing enqueued.
int sos_loop(const SosCall& a, char* base, SosLoopLayout* L, hipStream_t s, bool launch) {
  if (!launch) {
    if (a.n > (SIZE_MAX / 4 - 64) / 2) return MAVG_ERR_UNSUPPORTED;  // the byte counts stay in size_t
    L->buf = (a.n * 4 + 15) & ~(size_t)15;
    L->nbuf = a.sections > 2 ? 2 : 1;
    L->inner = 0;
    L->launches = 0;
  }
  for (int j = 0; j < a.sections; ++j) {
    const void* const in = j == 0 ? a.in : base + (size_t)((j - 1) & 1) * L->buf;
    float* const out = j == a.sections - 1 ? a.out : reinterpret_cast<float*>(base + (size_t)(j & 1) * L->buf);
    const int dtype = j == 0 ? a.dtype : MAVG_F32;
    const size_t so = (size_t)j * (size_t)a.C * 2;
    const BiquadCall c{in, out, a.state_in != nullptr ? a.state_in + so : nullptr,
                       a.state_out != nullptr ? a.state_out + so : nullptr, a.n, a.C, a.coef + 5 * (size_t)j,
                       a.halo[(size_t)j], dtype};
    int path = kBiquadStrip;
    int st = biquad_path(a.C, c.halo, dtype, &path);
    if (st != MAVG_OK) return st;
    if (launch) {
      st = biquad_launch(path, c, Workspace{base + (size_t)L->nbuf * L->buf, L->inner}, s);
      if (st != MAVG_OK) return st;
      continue;
    }
    {
      PlanScope ps;
      st = biquad_launch(path, c, Workspace{}, nullptr);
      if (st != MAVG_OK) return st;
    }
    size_t need = 0;
    st = biquad_ws_bytes(path, c, &need);
    if (st != MAVG_OK) return st;
    L->inner = std::max(L->inner, need);
    L->launches += path == kBiquadTile ? 1 : 3;
  }
  if (!launch && L->inner > SIZE_MAX - (size_t)L->nbuf * L->buf) return MAVG_ERR_UNSUPPORTED;
  return MAVG_OK;
}

// cascade_loop's workspace, in this order: the ping-pong buffer (the signal's bytes, 16-B padded);
// with a history two block buffers of passes * (grade - 1) * C samples each (16-B padded); then
// mavg_run's own workspace -- the signal's, and with a history at least the first block's.
struct CascadeLoopLayout {
  size_t pong, block, inner;
  size_t bytes() const { return pong + 2 * block + inner; }
};
int cascade_loop_layout(const CascadeCall& a, bool with_history, CascadeLoopLayout* l) {
  if (a.n > (SIZE_MAX / 4 - 15)) return MAVG_ERR_UNSUPPORTED;  // the byte count stays in size_t
  const size_t eb = elem_size(a.dtype);
  l->pong = (a.n * eb + 15) & ~(size_t)15;
  l->block = 0;
  int st = mavg_workspace_bytes(a.n, a.C, a.k, a.dtype, MAVG_ALGO_AUTO, 0, &l->inner);
  if (st != MAVG_OK || !with_history) return st;
  const size_t hs = (size_t)a.passes * (size_t)(a.k - 1) * (size_t)a.C;  // < 2^31 * 8 (validate_cascade, C <= 8 or naive)
  if (hs > (SIZE_MAX / 4 - 15)) return MAVG_ERR_UNSUPPORTED;
  l->block = (hs * eb + 15) & ~(size_t)15;
  size_t hin = 0;
  st = mavg_workspace_bytes(hs, a.C, a.k, a.dtype, MAVG_ALGO_AUTO, 0, &hin);
  l->inner = std::max(l->inner, hin);
  return st;
}

// cascade_loop: `passes` mavg_run calls (AUTO, block 0), never in place, between d_out and the
// ping-pong buffer so that the last lands in d_out.  With a history, pass j first filters block
// j - 1 (block 0 is the caller's history; zero history, the first grade - 1 outputs dropped) into
// block j, the history of pass j + 1; pass j itself takes the last grade - 1 frames of block j - 1.
// Every step is made dry first: an error leaves the stream untouched.
int cascade_loop_run(const CascadeCall& a, void* d_ws, size_t ws_bytes, void* stream) {
  CascadeLoopLayout l{};
  int st = cascade_loop_layout(a, a.hist != nullptr, &l);
  if (st != MAVG_OK) return st;
  st = check_workspace(l.bytes(), d_ws, ws_bytes);
  if (st != MAVG_OK) return st;
  char* const pong = static_cast<char*>(d_ws);
  char* const blocks[2] = {pong + l.pong, pong + l.pong + l.block};
  void* const iws = l.inner > 0 ? pong + l.pong + 2 * l.block : nullptr;
  const size_t fb = elem_size(a.dtype) * (size_t)a.C;
  const size_t km1 = (size_t)(a.k - 1);
  for (int dry = 1; dry >= 0; --dry) {
    const void* src = a.in;
    const char* blk = static_cast<const char*>(a.hist);  // block j - 1: (passes - j + 1)(k - 1) frames
    for (int j = 1; j <= a.passes; ++j) {
      void* const dst = ((a.passes - j) & 1) ? static_cast<void*>(pong) : a.out;
      const size_t bframes = (size_t)(a.passes - j + 1) * km1;
      const void* h = blk != nullptr ? blk + (bframes - km1) * fb : nullptr;
      st = run_signal(src, dst, a.n, a.C, a.k, a.dtype, MAVG_ALGO_AUTO, 0, h, iws, l.inner, stream, dry != 0);
      if (st != MAVG_OK) return st;
      if (blk != nullptr && j < a.passes) {
        char* const nb = blocks[(j - 1) & 1];
        st = run_signal(blk, nb, bframes * (size_t)a.C, a.C, a.k, a.dtype, MAVG_ALGO_AUTO, 0, nullptr, iws, l.inner,
                        stream, dry != 0);
        if (st != MAVG_OK) return st;
        blk = nb + km1 * fb;
      }
      src = dst;
    }
  }
  return MAVG_OK;
}

}  // namespace

extern "C" {

int mavg_abi_version(void) { return MAVG_ABI_VERSION; }

const char* mavg_strerror(int status) {
  switch (status) {
    case MAVG_OK: return "ok";
    case MAVG_ERR_INVALID_ARG: return "invalid argument";
    case MAVG_ERR_UNSUPPORTED: return "unsupported configuration";
    case MAVG_ERR_MISALIGNED: return "pointer not aligned to the sample size";
    case MAVG_ERR_WORKSPACE: return "workspace too small";
    case MAVG_ERR_HIP: return "HIP runtime error";
    default: return "unknown status";
  }
}

const char* mavg_algo_name(int algo) {
  switch (algo) {
    case MAVG_ALGO_AUTO: return "auto";
    case MAVG_ALGO_BLELLOCH: return "blelloch";
    case MAVG_ALGO_BLELLOCH_SCALAR: return "blelloch_scalar";
    case MAVG_ALGO_HILLIS: return "hillis";
    case MAVG_ALGO_HILLIS_SCALAR: return "hillis_scalar";
    case MAVG_ALGO_DIRECT: return "direct";
    case MAVG_ALGO_DIRECT_VEC2: return "direct_vec2";
    case MAVG_ALGO_DIRECT_SCALAR: return "direct_scalar";
    case MAVG_ALGO_NAIVE: return "naive";
    default: return "invalid";
  }
}

// AUTO: the Blelloch scan family at every window (flat tiles with the tile
// shape chosen by dispatch_scan_f; O(1) work per output for any k).  The
// direct kernel is kept for MAVG_ALGO_DIRECT*: since the tile scan's carry
// became a wave scan of the segment totals, tiles beat it even at k <= 9
// (k=7, 2^28 samples: fp32 0.821 vs 0.797 of HBM peak, int16 0.795 vs 0.761,
// tools/tune/tune_scan.hip).  Both move 1.00x the algorithmic bytes on HBM.
// More than kMaxChannels channels: only the naive kernel (runtime C) applies.
int mavg_resolve_algo(size_t n_samples, int channels, int grade, int dtype, int algo) {
  (void)n_samples;
  (void)dtype;
  (void)grade;
  if (algo != MAVG_ALGO_AUTO) return algo;
  if (channels > kMaxChannels) return MAVG_ALGO_NAIVE;
  return MAVG_ALGO_BLELLOCH;
}

int mavg_workspace_bytes(size_t n_samples, int channels, int grade, int dtype, int algo, int block_size,
                         size_t* out_bytes) {
  if (out_bytes == nullptr) return MAVG_ERR_INVALID_ARG;
  const int st = validate(n_samples, channels, grade, dtype, algo, block_size);
  if (st != MAVG_OK) return st;
  *out_bytes = 0;
  if (n_samples == 0) return MAVG_OK;
  // the dispatch decides; ask it in plan mode (nothing is launched)
  *out_bytes = plan_ws(n_samples, channels, grade, dtype,
                       mavg_resolve_algo(n_samples, channels, grade, dtype, algo), block_size);
  return MAVG_OK;
}

int mavg_run(const void* d_in, void* d_out, size_t n_samples, int channels, int grade, int dtype, int algo,
             int block_size, const void* d_history, void* d_ws, size_t ws_bytes, void* stream) {
  return run_signal(d_in, d_out, n_samples, channels, grade, dtype, algo, block_size, d_history, d_ws, ws_bytes, stream,
                    false);
}

int mavg_plan(size_t n_samples, int channels, int grade, int dtype, int algo, int block_size, char* buf,
              size_t buflen) {
  if (buf == nullptr || buflen == 0) return MAVG_ERR_INVALID_ARG;
  buf[0] = 0;
  if (n_samples == 0) return MAVG_ERR_INVALID_ARG;
  const int st0 = validate(n_samples, channels, grade, dtype, algo, block_size);
  if (st0 != MAVG_OK) return st0;
  PlanScope ps;
  const Sig sg{kPlanIn, kPlanOut, nullptr, (long long)(n_samples / (size_t)channels)};
  const int st = launch_algo(mavg_resolve_algo(n_samples, channels, grade, dtype, algo), dtype, channels, sg, grade,
                             block_size, nullptr, Workspace{});
  if (st != MAVG_OK) return st;
  snprintf(buf, buflen, "%s", ps.plan.text);
  return MAVG_OK;
}

int mavg_fill_synthetic(void* d_out, size_t n_samples, int dtype, uint64_t seed, uint64_t offset, int dist,
                        void* stream) {
  if (dtype != MAVG_I16 && dtype != MAVG_F32) return MAVG_ERR_INVALID_ARG;
  if (dist < 0 || dist > 2) return MAVG_ERR_INVALID_ARG;
  if (dist != 0 && dtype != MAVG_F32) return MAVG_ERR_INVALID_ARG;
  if (n_samples == 0) return MAVG_OK;
  if (d_out == nullptr) return MAVG_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long n = (long long)n_samples;
  const long long want = (n + kWG - 1) / kWG;
  const unsigned grid = (unsigned)std::min<long long>(want, (long long)device_cu_count() * 16);
  if (dtype == MAVG_F32)
    hipLaunchKernelGGL(synth_kernel<float>, dim3(grid), dim3(kWG), 0, s, static_cast<float*>(d_out), n,
                       seed + offset, dist);
  else
    hipLaunchKernelGGL(synth_kernel<int16_t>, dim3(grid), dim3(kWG), 0, s, static_cast<int16_t*>(d_out), n,
                       seed + offset, dist);
  return hipGetLastError() == hipSuccess ? MAVG_OK : MAVG_ERR_HIP;
}

int mavg_stream_copy(const void* d_in, void* d_out, size_t bytes, void* stream) {
  if (bytes == 0) return MAVG_OK;
  if (d_in == nullptr || d_out == nullptr || bytes % 16 != 0) return MAVG_ERR_INVALID_ARG;
  if (!aligned(d_in, 16) || !aligned(d_out, 16)) return MAVG_ERR_MISALIGNED;
  return launch_flat_copy(d_in, d_out, bytes, static_cast<hipStream_t>(stream));
}

int mavg_rows_workspace_bytes(size_t rows, size_t row_frames, int channels, int grade, int dtype, int with_history,
                              size_t* out_bytes) {
  if (out_bytes == nullptr) return MAVG_ERR_INVALID_ARG;
  size_t frames = 0;
  const int st = validate_rows(rows, row_frames, channels, grade, dtype, &frames);
  if (st != MAVG_OK) return st;
  *out_bytes = 0;
  if (frames == 0) return MAVG_OK;
  if (rows_fast_path(row_frames, channels, grade, dtype, with_history != 0)) {
    // no workspace; the launch's own limit (grid_too_large) shows here as it does in mavg_rows_run
    PlanScope ps;
    return rows_fast_launch(kPlanIn, kPlanOut, rows, row_frames, frames, channels, grade, dtype, nullptr);
  }
  return mavg_workspace_bytes(row_frames * (size_t)channels, channels, grade, dtype, MAVG_ALGO_AUTO, 0, out_bytes);
}

int mavg_rows_plan(size_t rows, size_t row_frames, int channels, int grade, int dtype, int with_history, char* buf,
                   size_t buflen) {
  if (buf == nullptr || buflen == 0) return MAVG_ERR_INVALID_ARG;
  buf[0] = 0;
  if (rows == 0 || row_frames == 0) return MAVG_ERR_INVALID_ARG;
  size_t frames = 0;
  const int st = validate_rows(rows, row_frames, channels, grade, dtype, &frames);
  if (st != MAVG_OK) return st;
  if (rows_fast_path(row_frames, channels, grade, dtype, with_history != 0)) {
    PlanScope ps;
    const int c = rows_fast_launch(kPlanIn, kPlanOut, rows, row_frames, frames, channels, grade, dtype, nullptr);
    if (c != MAVG_OK) return c;
    if (grade == 1)  // the flat copy over the whole batch
      snprintf(buf, buflen, "rows_scan<%s,C=%d,k=1> rows=%zu row_frames=%zu: %s", dtype == MAVG_F32 ? "f32" : "i16",
               channels, rows, row_frames, ps.plan.text);
    else
      snprintf(buf, buflen, "%s", ps.plan.text);
    return MAVG_OK;
  }
  char row[sizeof(LaunchPlan::text)];
  const int c = mavg_plan(row_frames * (size_t)channels, channels, grade, dtype, MAVG_ALGO_AUTO, 0, row, sizeof(row));
  if (c != MAVG_OK) return c;
  snprintf(buf, buflen, "rows_loop rows=%zu x %s", rows, row);
  return MAVG_OK;
}

// One launch of the segmented rows scan where it applies (rows_fast_path), else the single-signal
// dispatch once per row on the same stream, every row planned before the first is launched.
int mavg_rows_run(const void* d_in, void* d_out, size_t rows, size_t row_frames, int channels, int grade, int dtype,
                  const void* d_history, void* d_ws, size_t ws_bytes, void* stream) {
  size_t frames = 0;
  const int st = validate_rows(rows, row_frames, channels, grade, dtype, &frames);
  if (st != MAVG_OK) return st;
  if (frames == 0) return MAVG_OK;
  if (d_in == nullptr || d_out == nullptr) return MAVG_ERR_INVALID_ARG;
  const size_t eb = elem_size(dtype);
  if (!aligned(d_in, eb) || !aligned(d_out, eb) || (d_history != nullptr && !aligned(d_history, eb)))
    return MAVG_ERR_MISALIGNED;
  if (rows_fast_path(row_frames, channels, grade, dtype, d_history != nullptr))
    return rows_fast_launch(d_in, d_out, rows, row_frames, frames, channels, grade, dtype,
                            static_cast<hipStream_t>(stream));
  // rows_loop: `rows` launches (a misaligned row: two), all sharing the caller's workspace --
  // launches on one stream are serial and each zeroes its records
  const size_t row_samples = row_frames * (size_t)channels;
  const size_t row_bytes = row_samples * eb;
  const size_t hist_bytes = (size_t)(grade - 1) * (size_t)channels * eb;
  auto row_run = [&](size_t r, bool dry) -> int {
    const void* h = d_history != nullptr ? static_cast<const char*>(d_history) + r * hist_bytes : nullptr;
    return run_signal(static_cast<const char*>(d_in) + r * row_bytes, static_cast<char*>(d_out) + r * row_bytes,
                      row_samples, channels, grade, dtype, MAVG_ALGO_AUTO, 0, h, d_ws, ws_bytes, stream, dry);
  };
  return run_row_loop(rows, rows_alignment_period(rows), row_samples, channels, grade, dtype, d_ws, ws_bytes, row_run);
}

int mavg_decim_out_frames(size_t n_frames, int hop, int phase, size_t* out_frames) {
  if (out_frames == nullptr || hop < 1 || phase < 0 || phase >= hop) return MAVG_ERR_INVALID_ARG;
  *out_frames = n_frames > (size_t)phase ? (n_frames - (size_t)phase - 1) / (size_t)hop + 1 : 0;
  return MAVG_OK;
}

int mavg_decim_workspace_bytes(size_t n_samples, int channels, int grade, int hop, int phase, int dtype,
                               size_t* out_bytes) {
  if (out_bytes == nullptr) return MAVG_ERR_INVALID_ARG;
  size_t M = 0;
  int st = validate_decim(n_samples, channels, grade, hop, phase, dtype, &M);
  if (st != MAVG_OK) return st;
  *out_bytes = 0;
  if (M == 0) return MAVG_OK;
  if (hop == 1) return mavg_workspace_bytes(n_samples, channels, grade, dtype, MAVG_ALGO_AUTO, 0, out_bytes);
  int path = kDecimFull;
  st = decim_path(channels, grade, hop, dtype, &path);
  if (st != MAVG_OK) return st;
  const DecimCall a{kPlanIn, kPlanOut, nullptr, n_samples, M, channels, grade, hop, phase, dtype};
  if (path != kDecimFull) {
    // no workspace; the launch's own limit (grid_too_large) shows here as it does in mavg_decim_run
    PlanScope ps;
    return decim_fast_launch(path, a, nullptr);
  }
  size_t full_bytes = 0, inner = 0;
  st = decim_full_layout(a, &full_bytes, &inner);
  if (st != MAVG_OK) return st;
  *out_bytes = full_bytes + inner;
  return MAVG_OK;
}

int mavg_decim_plan(size_t n_samples, int channels, int grade, int hop, int phase, int dtype, char* buf,
                    size_t buflen) {
  if (buf == nullptr || buflen == 0) return MAVG_ERR_INVALID_ARG;
  buf[0] = 0;
  size_t M = 0;
  int st = validate_decim(n_samples, channels, grade, hop, phase, dtype, &M);
  if (st != MAVG_OK) return st;
  if (M == 0) return MAVG_ERR_INVALID_ARG;  // nothing to describe, as mavg_plan
  int path = kDecimFull;
  if (hop > 1) {
    st = decim_path(channels, grade, hop, dtype, &path);
    if (st != MAVG_OK) return st;
    if (path != kDecimFull) {
      PlanScope ps;
      st = decim_fast_launch(path, DecimCall{kPlanIn, kPlanOut, nullptr, n_samples, M, channels, grade, hop, phase, dtype},
                             nullptr);
      if (st == MAVG_OK) snprintf(buf, buflen, "%s", ps.plan.text);
      return st;
    }
  }
  char full[sizeof(LaunchPlan::text)];
  st = mavg_plan(n_samples, channels, grade, dtype, MAVG_ALGO_AUTO, 0, full, sizeof(full));
  if (st != MAVG_OK) return st;
  if (hop == 1) snprintf(buf, buflen, "decim_none x %s", full);
  else snprintf(buf, buflen, "decim_full hop=%d phase=%d x %s", hop, phase, full);
  return MAVG_OK;
}

// hop == 1: mavg_run itself.  Else one launch of the compacting scan or of the window sum where the
// rule (decim_path) takes them, else mavg_run into the workspace and a gather, both planned first.
int mavg_decim_run(const void* d_in, void* d_out, size_t n_samples, int channels, int grade, int hop, int phase,
                   int dtype, const void* d_history, void* d_ws, size_t ws_bytes, void* stream) {
  size_t M = 0;
  int st = validate_decim(n_samples, channels, grade, hop, phase, dtype, &M);
  if (st != MAVG_OK) return st;
  if (M == 0) return MAVG_OK;
  if (d_in == nullptr || d_out == nullptr) return MAVG_ERR_INVALID_ARG;
  const size_t eb = elem_size(dtype);
  if (!aligned(d_in, eb) || !aligned(d_out, eb) || (d_history != nullptr && !aligned(d_history, eb)))
    return MAVG_ERR_MISALIGNED;
  if (hop == 1)
    return run_signal(d_in, d_out, n_samples, channels, grade, dtype, MAVG_ALGO_AUTO, 0, d_history, d_ws, ws_bytes,
                      stream, false);
  int path = kDecimFull;
  st = decim_path(channels, grade, hop, dtype, &path);
  if (st != MAVG_OK) return st;
  const DecimCall a{d_in, d_out, d_history, n_samples, M, channels, grade, hop, phase, dtype};
  if (path != kDecimFull) return decim_fast_launch(path, a, static_cast<hipStream_t>(stream));
  return decim_full_run(a, d_ws, ws_bytes, stream);
}

int mavg_cascade_workspace_bytes(size_t n_samples, int channels, int grade, int passes, int dtype, int with_history,
                                 size_t* out_bytes) {
  if (out_bytes == nullptr) return MAVG_ERR_INVALID_ARG;
  int st = validate_cascade(n_samples, channels, grade, passes, dtype);
  if (st != MAVG_OK) return st;
  *out_bytes = 0;
  if (n_samples == 0) return MAVG_OK;
  if (passes == 1 || grade == 1)
    return mavg_workspace_bytes(n_samples, channels, grade, dtype, MAVG_ALGO_AUTO, 0, out_bytes);
  int path = kCascadeLoop;
  st = cascade_path(channels, grade, passes, dtype, &path);
  if (st != MAVG_OK) return st;
  const CascadeCall a{kPlanIn, kPlanOut, nullptr, n_samples, channels, grade, passes, dtype};
  if (path == kCascadeTile) {
    // no workspace; the launch's own limit (grid_too_large) shows here as it does in mavg_cascade_run
    PlanScope ps;
    return cascade_tile_launch(a, nullptr);
  }
  CascadeLoopLayout l{};
  st = cascade_loop_layout(a, with_history != 0, &l);
  if (st != MAVG_OK) return st;
  *out_bytes = l.bytes();
  return MAVG_OK;
}

int mavg_cascade_plan(size_t n_samples, int channels, int grade, int passes, int dtype, int with_history, char* buf,
                      size_t buflen) {
  if (buf == nullptr || buflen == 0) return MAVG_ERR_INVALID_ARG;
  buf[0] = 0;
  int st = validate_cascade(n_samples, channels, grade, passes, dtype);
  if (st != MAVG_OK) return st;
  if (n_samples == 0) return MAVG_ERR_INVALID_ARG;  // nothing to describe, as mavg_plan
  const bool none = passes == 1 || grade == 1;
  if (!none) {
    int path = kCascadeLoop;
    st = cascade_path(channels, grade, passes, dtype, &path);
    if (st != MAVG_OK) return st;
    if (path == kCascadeTile) {
      PlanScope ps;
      st = cascade_tile_launch(CascadeCall{kPlanIn, kPlanOut, nullptr, n_samples, channels, grade, passes, dtype}, nullptr);
      if (st == MAVG_OK) snprintf(buf, buflen, "%s", ps.plan.text);
      return st;
    }
  }
  char one[sizeof(LaunchPlan::text)];
  st = mavg_plan(n_samples, channels, grade, dtype, MAVG_ALGO_AUTO, 0, one, sizeof(one));
  if (st != MAVG_OK) return st;
  if (none) snprintf(buf, buflen, "cascade_none x %s", one);
  else snprintf(buf, buflen, "cascade_loop passes=%d history=%d x %s", passes, with_history != 0 ? 1 : 0, one);
  return MAVG_OK;
}

// passes == 1 or grade == 1: mavg_run itself.  Else one launch of the fused tile kernel where the
// rule (cascade_path) takes it, else `passes` mavg_run calls through the workspace, all planned
// first.
int mavg_cascade_run(const void* d_in, void* d_out, size_t n_samples, int channels, int grade, int passes, int dtype,
                     const void* d_history, void* d_ws, size_t ws_bytes, void* stream) {
  int st = validate_cascade(n_samples, channels, grade, passes, dtype);
  if (st != MAVG_OK) return st;
  if (n_samples == 0) return MAVG_OK;
  if (d_in == nullptr || d_out == nullptr) return MAVG_ERR_INVALID_ARG;
  const size_t eb = elem_size(dtype);
  if (!aligned(d_in, eb) || !aligned(d_out, eb) || (d_history != nullptr && !aligned(d_history, eb)))
    return MAVG_ERR_MISALIGNED;
  if (passes == 1 || grade == 1)
    return run_signal(d_in, d_out, n_samples, channels, grade, dtype, MAVG_ALGO_AUTO, 0, d_history, d_ws, ws_bytes,
                      stream, false);
  int path = kCascadeLoop;
  st = cascade_path(channels, grade, passes, dtype, &path);
  if (st != MAVG_OK) return st;
  const CascadeCall a{d_in, d_out, d_history, n_samples, channels, grade, passes, dtype};
  if (path == kCascadeTile) return cascade_tile_launch(a, static_cast<hipStream_t>(stream));
  return cascade_loop_run(a, d_ws, ws_bytes, stream);
}

int mavg_stat_plan(size_t n_samples, int channels, int grade, int stat, int dtype, int with_mean, char* buf,
                   size_t buflen) {
  if (buf == nullptr || buflen == 0) return MAVG_ERR_INVALID_ARG;
  buf[0] = 0;
  int st = validate_stat(n_samples, channels, grade, stat, dtype);
  if (st != MAVG_OK) return st;
  if (n_samples == 0) return MAVG_ERR_INVALID_ARG;  // nothing to describe, as mavg_plan
  int path = kStatStrip;
  st = stat_path(channels, grade, dtype, &path);
  if (st != MAVG_OK) return st;
  PlanScope ps;
  float* const mean = with_mean != 0 ? static_cast<float*>(const_cast<void*>(kPlanOff)) : nullptr;
  st = stat_launch(path, StatCall{kPlanIn, static_cast<float*>(kPlanOut), mean, nullptr, n_samples, channels, grade, stat, dtype},
                   nullptr);
  if (st == MAVG_OK) snprintf(buf, buflen, "%s", ps.plan.text);
  return st;
}

// One launch: the tile kernel where the rule (stat_path) takes the window, else the strip kernel.
int mavg_stat_run(const void* d_in, float* d_out, float* d_mean, size_t n_samples, int channels, int grade, int stat,
                  int dtype, const void* d_history, void* stream) {
  int st = validate_stat(n_samples, channels, grade, stat, dtype);
  if (st != MAVG_OK) return st;
  if (n_samples == 0) return MAVG_OK;
  if (d_in == nullptr || d_out == nullptr) return MAVG_ERR_INVALID_ARG;
  const size_t eb = elem_size(dtype);
  if (!aligned(d_in, eb) || !aligned(d_out, 4) || (d_mean != nullptr && !aligned(d_mean, 4)) ||
      (d_history != nullptr && !aligned(d_history, eb)))
    return MAVG_ERR_MISALIGNED;
  int path = kStatStrip;
  st = stat_path(channels, grade, dtype, &path);
  if (st != MAVG_OK) return st;
  return stat_launch(path, StatCall{d_in, d_out, d_mean, d_history, n_samples, channels, grade, stat, dtype},
                     static_cast<hipStream_t>(stream));
}

int mavg_extrema_plan(size_t n_samples, int channels, int grade, int dtype, int with_max, int with_min, char* buf,
                      size_t buflen) {
  if (buf == nullptr || buflen == 0) return MAVG_ERR_INVALID_ARG;
  buf[0] = 0;
  int st = validate(n_samples, channels, grade, dtype, MAVG_ALGO_AUTO, 0);
  if (st != MAVG_OK) return st;
  if (with_max == 0 && with_min == 0) return MAVG_ERR_INVALID_ARG;
  if (n_samples == 0) return MAVG_ERR_INVALID_ARG;  // nothing to describe, as mavg_plan
  int path = kExtremaStrip;
  st = extrema_path(channels, grade, dtype, &path);
  if (st != MAVG_OK) return st;
  PlanScope ps;
  void* const omax = with_max != 0 ? kPlanOut : nullptr;
  void* const omin = with_min != 0 ? const_cast<void*>(kPlanOff) : nullptr;
  // (bit 1 of either flag: views off 16-B alignment -- an input one sample past a 16-B boundary)
  const bool off = ((with_max | with_min) & 2) != 0;
  const void* const in = off ? static_cast<const char*>(kPlanIn) + elem_size(dtype) : kPlanIn;
  st = extrema_launch(path, ExtremaCall{in, omax, omin, nullptr, n_samples, channels, grade, dtype}, nullptr);
  if (st == MAVG_OK) snprintf(buf, buflen, "%s", ps.plan.text);
  return st;
}

// One launch: the tile kernel where the rule (extrema_path) takes the window, else the strip kernel.
int mavg_extrema_run(const void* d_in, void* d_max, void* d_min, size_t n_samples, int channels, int grade, int dtype,
                     const void* d_history, void* stream) {
  int st = validate(n_samples, channels, grade, dtype, MAVG_ALGO_AUTO, 0);
  if (st != MAVG_OK) return st;
  if (d_max == nullptr && d_min == nullptr) return MAVG_ERR_INVALID_ARG;
  if (n_samples == 0) return MAVG_OK;
  if (d_in == nullptr) return MAVG_ERR_INVALID_ARG;
  const size_t eb = elem_size(dtype);
  if (!aligned(d_in, eb) || !aligned(d_max, eb) || !aligned(d_min, eb) || (d_history != nullptr && !aligned(d_history, eb)))
    return MAVG_ERR_MISALIGNED;
  int path = kExtremaStrip;
  st = extrema_path(channels, grade, dtype, &path);
  if (st != MAVG_OK) return st;
  return extrema_launch(path, ExtremaCall{d_in, d_max, d_min, d_history, n_samples, channels, grade, dtype},
                        static_cast<hipStream_t>(stream));
}

int mavg_ema_halo_frames(double alpha, long long* out_frames) {
  if (out_frames == nullptr) return MAVG_ERR_INVALID_ARG;
  const int st = validate_ema(0, 1, alpha, MAVG_F32);
  if (st != MAVG_OK) return st;
  *out_frames = ema_halo_frames(alpha);
  return MAVG_OK;
}

int mavg_ema_workspace_bytes(size_t n_samples, int channels, double alpha, int dtype, size_t* out_bytes) {
  if (out_bytes == nullptr) return MAVG_ERR_INVALID_ARG;
  int st = validate_ema(n_samples, channels, alpha, dtype);
  if (st != MAVG_OK) return st;
  *out_bytes = 0;
  if (n_samples == 0) return MAVG_OK;
  int path = kEmaStrip;
  st = ema_path(channels, alpha, dtype, &path);
  if (st != MAVG_OK) return st;
  const EmaCall a{kPlanIn, static_cast<float*>(kPlanOut), nullptr, nullptr, n_samples, channels, alpha, dtype};
  {
    // the launches' own limit (grid_too_large) shows here as it does in mavg_ema_run
    PlanScope ps;
    st = ema_launch(path, a, Workspace{}, nullptr);
    if (st != MAVG_OK) return st;
  }
  return ema_ws_bytes(path, a, out_bytes);
}

int mavg_ema_plan(size_t n_samples, int channels, double alpha, int dtype, int flags, char* buf, size_t buflen) {
  if (buf == nullptr || buflen == 0) return MAVG_ERR_INVALID_ARG;
  buf[0] = 0;
  int st = validate_ema(n_samples, channels, alpha, dtype);
  if (st != MAVG_OK) return st;
  if (flags < 0 || flags > 7) return MAVG_ERR_INVALID_ARG;
  if (n_samples == 0) return MAVG_ERR_INVALID_ARG;  // nothing to describe, as mavg_plan
  int path = kEmaStrip;
  st = ema_path(channels, alpha, dtype, &path);
  if (st != MAVG_OK) return st;
  PlanScope ps;
  // (flag 4: views off 16-B alignment -- an input one sample past a 16-B boundary)
  const void* const in = (flags & 4) != 0 ? static_cast<const char*>(kPlanIn) + elem_size(dtype) : kPlanIn;
  const double* const sin = (flags & 1) != 0 ? static_cast<const double*>(kPlanOff) : nullptr;
  double* const sout = (flags & 2) != 0 ? static_cast<double*>(const_cast<void*>(kPlanOff)) + 64 : nullptr;
  st = ema_launch(path, EmaCall{in, static_cast<float*>(kPlanOut), sin, sout, n_samples, channels, alpha, dtype},
                  Workspace{}, nullptr);
  if (st == MAVG_OK) snprintf(buf, buflen, "%s", ps.plan.text);
  return st;
}

// One launch of the tile kernel where the rule (ema_path) takes the coefficient, else the three
// launches of the chain or the strip form, all planned before the first is made.
int mavg_ema_run(const void* d_in, float* d_out, size_t n_samples, int channels, double alpha, int dtype,
                 const double* d_state_in, double* d_state_out, void* d_ws, size_t ws_bytes, void* stream) {
  int st = validate_ema(n_samples, channels, alpha, dtype);
  if (st != MAVG_OK) return st;
  if (d_state_in != nullptr && d_state_in == d_state_out) return MAVG_ERR_INVALID_ARG;
  if (n_samples == 0) return MAVG_OK;
  if (d_in == nullptr || d_out == nullptr) return MAVG_ERR_INVALID_ARG;
  if (!aligned(d_in, elem_size(dtype)) || !aligned(d_out, 4) || !aligned(d_state_in, 8) || !aligned(d_state_out, 8))
    return MAVG_ERR_MISALIGNED;
  int path = kEmaStrip;
  st = ema_path(channels, alpha, dtype, &path);
  if (st != MAVG_OK) return st;
  const EmaCall a{d_in, d_out, d_state_in, d_state_out, n_samples, channels, alpha, dtype};
  {
    PlanScope ps;  // every launch's limits, with nothing enqueued
    st = ema_launch(path, a, Workspace{}, nullptr);
    if (st != MAVG_OK) return st;
  }
  size_t need = 0;
  st = ema_ws_bytes(path, a, &need);
  if (st != MAVG_OK) return st;
  st = check_workspace(need, d_ws, ws_bytes);
  if (st != MAVG_OK) return st;
  return ema_launch(path, a, Workspace{d_ws, ws_bytes}, static_cast<hipStream_t>(stream));
}

int mavg_biquad_halo_frames(const double coef[5], long long* out_frames) {
  if (out_frames == nullptr) return MAVG_ERR_INVALID_ARG;
  const int st = validate_biquad(0, 1, coef, MAVG_F32);
  if (st != MAVG_OK) return st;
  *out_frames = biquad_halo_frames(coef);
  return MAVG_OK;
}

int mavg_biquad_workspace_bytes(size_t n_samples, int channels, const double coef[5], int dtype, size_t* out_bytes) {
  if (out_bytes == nullptr) return MAVG_ERR_INVALID_ARG;
  int st = validate_biquad(n_samples, channels, coef, dtype);
  if (st != MAVG_OK) return st;
  *out_bytes = 0;
  if (n_samples == 0) return MAVG_OK;
  const long long halo = biquad_halo_frames(coef);
  int path = kBiquadStrip;
  st = biquad_path(channels, halo, dtype, &path);
  if (st != MAVG_OK) return st;
  const BiquadCall a{kPlanIn, static_cast<float*>(kPlanOut), nullptr, nullptr, n_samples, channels, coef, halo, dtype};
  {
    // the launches' own limit (grid_too_large) shows here as it does in mavg_biquad_run
    PlanScope ps;
    st = biquad_launch(path, a, Workspace{}, nullptr);
    if (st != MAVG_OK) return st;
  }
  return biquad_ws_bytes(path, a, out_bytes);
}

int mavg_biquad_plan(size_t n_samples, int channels, const double coef[5], int dtype, int flags, char* buf,
                     size_t buflen) {
  if (buf == nullptr || buflen == 0) return MAVG_ERR_INVALID_ARG;
  buf[0] = 0;
  int st = validate_biquad(n_samples, channels, coef, dtype);
  if (st != MAVG_OK) return st;
  if (flags < 0 || flags > 7) return MAVG_ERR_INVALID_ARG;
  if (n_samples == 0) return MAVG_ERR_INVALID_ARG;  // nothing to describe, as mavg_plan
  const long long halo = biquad_halo_frames(coef);
  int path = kBiquadStrip;
  st = biquad_path(channels, halo, dtype, &path);
  if (st != MAVG_OK) return st;
  PlanScope ps;
  // (flag 4: views off 16-B alignment -- an input one sample past a 16-B boundary)
  const void* const in = (flags & 4) != 0 ? static_cast<const char*>(kPlanIn) + elem_size(dtype) : kPlanIn;
  const double* const sin = (flags & 1) != 0 ? static_cast<const double*>(kPlanOff) : nullptr;
  double* const sout = (flags & 2) != 0 ? static_cast<double*>(const_cast<void*>(kPlanOff)) + 64 : nullptr;
  st = biquad_launch(path, BiquadCall{in, static_cast<float*>(kPlanOut), sin, sout, n_samples, channels, coef, halo, dtype},
                     Workspace{}, nullptr);
  if (st == MAVG_OK) snprintf(buf, buflen, "%s", ps.plan.text);
  return st;
}

// One launch of the tile kernel where the rule (biquad_path) takes the coefficients' halo, else the
// three launches of the chain or the strip form, all planned before the first is made.
int mavg_biquad_run(const void* d_in, float* d_out, size_t n_samples, int channels, const double coef[5], int dtype,
                    const double* d_state_in, double* d_state_out, void* d_ws, size_t ws_bytes, void* stream) {
  int st = validate_biquad(n_samples, channels, coef, dtype);
  if (st != MAVG_OK) return st;
  if (d_state_in != nullptr && d_state_in == d_state_out) return MAVG_ERR_INVALID_ARG;
  if (n_samples == 0) return MAVG_OK;
  if (d_in == nullptr || d_out == nullptr) return MAVG_ERR_INVALID_ARG;
  if (!aligned(d_in, elem_size(dtype)) || !aligned(d_out, 4) || !aligned(d_state_in, 8) || !aligned(d_state_out, 8))
    return MAVG_ERR_MISALIGNED;
  const long long halo = biquad_halo_frames(coef);
  int path = kBiquadStrip;
  st = biquad_path(channels, halo, dtype, &path);
  if (st != MAVG_OK) return st;
  const BiquadCall a{d_in, d_out, d_state_in, d_state_out, n_samples, channels, coef, halo, dtype};
  {
    PlanScope ps;  // every launch's limits, with nothing enqueued
    st = biquad_launch(path, a, Workspace{}, nullptr);
    if (st != MAVG_OK) return st;
  }
  size_t need = 0;
  st = biquad_ws_bytes(path, a, &need);
  if (st != MAVG_OK) return st;
  st = check_workspace(need, d_ws, ws_bytes);
  if (st != MAVG_OK) return st;
  return biquad_launch(path, a, Workspace{d_ws, ws_bytes}, static_cast<hipStream_t>(stream));
}

int mavg_sos_halo_frames(const double* coef, int sections, long long* out_frames) {
  if (out_frames == nullptr) return MAVG_ERR_INVALID_ARG;
  const int st = validate_sos(0, 1, coef, sections, MAVG_F32);
  if (st != MAVG_OK) return st;
  SosCall a{nullptr, nullptr, nullptr, nullptr, 0, 1, coef, sections, MAVG_F32, 0, {}, 0};
  a.form_halos();
  *out_frames = a.sum_halo;
  return MAVG_OK;
}

int mavg_sos_workspace_bytes(size_t n_samples, int channels, const double* coef, int sections, int dtype, int flags,
                             size_t* out_bytes) {
  if (out_bytes == nullptr) return MAVG_ERR_INVALID_ARG;
  int st = validate_sos(n_samples, channels, coef, sections, dtype);
  if (st != MAVG_OK) return st;
  if (flags < 0 || (flags & ~MAVG_SOS_FP64_ONLY) != 0) return MAVG_ERR_INVALID_ARG;
  if (sections == 1) return mavg_biquad_workspace_bytes(n_samples, channels, coef, dtype, out_bytes);
  *out_bytes = 0;
  if (n_samples == 0) return MAVG_OK;
  SosCall a{kPlanIn, static_cast<float*>(kPlanOut), nullptr, nullptr, n_samples, channels, coef, sections, dtype, flags, {}, 0};
  a.form_halos();
  int path = kSosLoop;
  st = sos_path(a, &path);
  if (st != MAVG_OK) return st;
  if (path == kSosTile) {
    PlanScope ps;  // the launch's own limit (grid_too_large) shows here as it does in mavg_sos_run
    st = sos_tile_launch(a, Workspace{}, nullptr);
    if (st == MAVG_OK) *out_bytes = sos_tile_ws_bytes(sections);
    return st;
  }
  SosLoopLayout L;
  st = sos_loop(a, static_cast<char*>(const_cast<void*>(kPlanOff)), &L, nullptr, false);
  if (st == MAVG_OK) *out_bytes = L.bytes();
  return st;
}

int mavg_sos_plan(size_t n_samples, int channels, const double* coef, int sections, int dtype, int flags, char* buf,
                  size_t buflen) {
  if (buf == nullptr || buflen == 0) return MAVG_ERR_INVALID_ARG;
  buf[0] = 0;
  int st = validate_sos(n_samples, channels, coef, sections, dtype);
  if (st != MAVG_OK) return st;
  const int views = flags >> kSosPlanShift;  // 1 / 2 / 4 as mavg_biquad_plan's
  if (flags < 0 || views > 7 || (flags & ((1 << kSosPlanShift) - 1) & ~MAVG_SOS_FP64_ONLY) != 0) return MAVG_ERR_INVALID_ARG;
  if (n_samples == 0) return MAVG_ERR_INVALID_ARG;  // nothing to describe, as mavg_plan
  if (sections == 1) {
    char inner[256];
    st = mavg_biquad_plan(n_samples, channels, coef, dtype, views, inner, sizeof(inner));
    if (st == MAVG_OK) snprintf(buf, buflen, "sos_none %s", inner);
    return st;
  }
  // (view bit 4: views off 16-B alignment -- an input one sample past a 16-B boundary)
  const void* const in = (views & 4) != 0 ? static_cast<const char*>(kPlanIn) + elem_size(dtype) : kPlanIn;
  const double* const sin = (views & 1) != 0 ? static_cast<const double*>(kPlanOff) : nullptr;
  double* const sout = (views & 2) != 0 ? static_cast<double*>(const_cast<void*>(kPlanOff)) + 64 : nullptr;
  SosCall a{in, static_cast<float*>(kPlanOut), sin, sout, n_samples, channels, coef, sections, dtype,
            flags & MAVG_SOS_FP64_ONLY, {}, 0};
  a.form_halos();
  int path = kSosLoop;
  st = sos_path(a, &path);
  if (st != MAVG_OK) return st;
  if (path == kSosTile) {
    PlanScope ps;
    st = sos_tile_launch(a, Workspace{}, nullptr);
    if (st == MAVG_OK) snprintf(buf, buflen, "%s", ps.plan.text);
    return st;
  }
  SosLoopLayout L;
  st = sos_loop(a, static_cast<char*>(const_cast<void*>(kPlanOff)) + 4096, &L, nullptr, false);
  if (st == MAVG_OK)
    snprintf(buf, buflen,
             "sos_loop dtype=%s C=%d sections=%d intermediate=f32 halo_frames=%lld state=%d frames=%zu buffers=%d ws=%zu "
             "launches=%d",
             dtype == MAVG_F32 ? "f32" : "i16", channels, sections, a.sum_halo, views & 3, n_samples / (size_t)channels,
             L.nbuf, L.bytes(), L.launches);
  return st;
}

// sections == 1 (sos_none): mavg_biquad_run.  Else the fused tile kernel where the rule (sos_path)
// takes the cascade, else one mavg_biquad_run per section through fp32 buffers in the workspace;
// every launch is planned before the first is made.
int mavg_sos_run(const void* d_in, float* d_out, size_t n_samples, int channels, const double* coef, int sections,
                 int dtype, int flags, const double* d_state_in, double* d_state_out, void* d_ws, size_t ws_bytes,
                 void* stream) {
  int st = validate_sos(n_samples, channels, coef, sections, dtype);
  if (st != MAVG_OK) return st;
  if (flags < 0 || (flags & ~MAVG_SOS_FP64_ONLY) != 0) return MAVG_ERR_INVALID_ARG;
  if (sections == 1)
    return mavg_biquad_run(d_in, d_out, n_samples, channels, coef, dtype, d_state_in, d_state_out, d_ws, ws_bytes, stream);
  if (d_state_in != nullptr && d_state_in == d_state_out) return MAVG_ERR_INVALID_ARG;
  if (n_samples == 0) return MAVG_OK;
  if (d_in == nullptr || d_out == nullptr) return MAVG_ERR_INVALID_ARG;
  if (!aligned(d_in, elem_size(dtype)) || !aligned(d_out, 4) || !aligned(d_state_in, 8) || !aligned(d_state_out, 8))
    return MAVG_ERR_MISALIGNED;
  SosCall a{d_in, d_out, d_state_in, d_state_out, n_samples, channels, coef, sections, dtype, flags, {}, 0};
  a.form_halos();
  int path = kSosLoop;
  st = sos_path(a, &path);
  if (st != MAVG_OK) return st;
  hipStream_t const s = static_cast<hipStream_t>(stream);
  if (path == kSosTile) {
    {
      PlanScope ps;  // the launch's limits, with nothing enqueued
      st = sos_tile_launch(a, Workspace{}, nullptr);
      if (st != MAVG_OK) return st;
    }
    st = check_workspace(sos_tile_ws_bytes(sections), d_ws, ws_bytes);
    if (st != MAVG_OK) return st;
    return sos_tile_launch(a, Workspace{d_ws, ws_bytes}, s);
  }
  SosLoopLayout L;
  // planned with the buffers at a 16-B aligned stand-in: the workspace's own alignment is checked below
  st = sos_loop(a, static_cast<char*>(const_cast<void*>(kPlanOff)) + 4096, &L, nullptr, false);
  if (st != MAVG_OK) return st;
  st = check_workspace(L.bytes(), d_ws, ws_bytes);
  if (st != MAVG_OK) return st;
  return sos_loop(a, static_cast<char*>(d_ws), &L, s, true);
}

int mavg_fir_plan(size_t n_samples, int channels, int ntaps, int dtype, int flags, char* buf, size_t buflen) {
  if (buf == nullptr || buflen == 0) return MAVG_ERR_INVALID_ARG;
  buf[0] = 0;
  int st = validate_fir(n_samples, channels, ntaps, dtype);
  if (st != MAVG_OK) return st;
  if (flags < 0 || (flags & ~5) != 0) return MAVG_ERR_INVALID_ARG;
  if (n_samples == 0) return MAVG_ERR_INVALID_ARG;  // nothing to describe, as mavg_plan
  int path = kFirStrip;
  st = fir_path(channels, ntaps, dtype, &path);
  if (st != MAVG_OK) return st;
  PlanScope ps;
  // (flag 4: views off 16-B alignment -- an input one sample past a 16-B boundary)
  const void* const in = (flags & 4) != 0 ? static_cast<const char*>(kPlanIn) + elem_size(dtype) : kPlanIn;
  const void* const hist = (flags & 1) != 0 ? kPlanOff : nullptr;
  st = fir_launch(path, FirCall{in, static_cast<float*>(kPlanOut), hist, static_cast<const double*>(kPlanOff), n_samples,
                                channels, ntaps, dtype},
                  nullptr);
  if (st == MAVG_OK) snprintf(buf, buflen, "%s", ps.plan.text);
  return st;
}

// One launch: the tile kernel where the rule (fir_path) takes the taps, else the strip kernel.
int mavg_fir_run(const void* d_in, float* d_out, size_t n_samples, int channels, const double* d_taps, int ntaps,
                 int dtype, const void* d_history, void* stream) {
  int st = validate_fir(n_samples, channels, ntaps, dtype);
  if (st != MAVG_OK) return st;
  if (n_samples == 0) return MAVG_OK;
  if (d_in == nullptr || d_out == nullptr || d_taps == nullptr) return MAVG_ERR_INVALID_ARG;
  const size_t eb = elem_size(dtype);
  if (!aligned(d_in, eb) || !aligned(d_out, 4) || !aligned(d_taps, 8) || (d_history != nullptr && !aligned(d_history, eb)))
    return MAVG_ERR_MISALIGNED;
  int path = kFirStrip;
  st = fir_path(channels, ntaps, dtype, &path);
  if (st != MAVG_OK) return st;
  return fir_launch(path, FirCall{d_in, d_out, d_history, d_taps, n_samples, channels, ntaps, dtype},
                    static_cast<hipStream_t>(stream));
}

int mavg_ragged_workspace_bytes(const int64_t* h_offsets, size_t rows, int channels, int grade, int dtype,
                                size_t* out_bytes) {
  if (out_bytes == nullptr) return MAVG_ERR_INVALID_ARG;
  size_t frames = 0, longest = 0;
  const int st = validate_ragged(h_offsets, rows, channels, grade, dtype, &frames, &longest);
  if (st != MAVG_OK) return st;
  *out_bytes = 0;
  if (frames == 0) return MAVG_OK;
  if (ragged_fast_path(longest, channels, grade, dtype)) {
    // no workspace; the launch's own limit (grid_too_large) shows here as it does in mavg_ragged_run
    PlanScope ps;
    return ragged_fast_launch(kPlanIn, kPlanOut, kPlanOff, rows, frames, longest, channels, grade, dtype, nullptr);
  }
  return mavg_workspace_bytes(longest * (size_t)channels, channels, grade, dtype, MAVG_ALGO_AUTO, 0, out_bytes);
}

int mavg_ragged_plan(const int64_t* h_offsets, size_t rows, int channels, int grade, int dtype, char* buf,
                     size_t buflen) {
  if (buf == nullptr || buflen == 0) return MAVG_ERR_INVALID_ARG;
  buf[0] = 0;
  size_t frames = 0, longest = 0;
  const int st = validate_ragged(h_offsets, rows, channels, grade, dtype, &frames, &longest);
  if (st != MAVG_OK) return st;
  if (frames == 0) return MAVG_ERR_INVALID_ARG;  // nothing to describe, as mavg_plan
  if (ragged_fast_path(longest, channels, grade, dtype)) {
    PlanScope ps;
    const int c = ragged_fast_launch(kPlanIn, kPlanOut, kPlanOff, rows, frames, longest, channels, grade, dtype, nullptr);
    if (c != MAVG_OK) return c;
    if (grade == 1)  // the flat copy over the packed stream
      snprintf(buf, buflen, "ragged_scan<%s,C=%d,k=1> rows=%zu frames=%zu max_row_frames=%zu window=1 : %s",
               dtype == MAVG_F32 ? "f32" : "i16", channels, rows, frames, longest, ps.plan.text);
    else
      snprintf(buf, buflen, "%s", ps.plan.text);
    return MAVG_OK;
  }
  char row[sizeof(LaunchPlan::text)];
  const int c = mavg_plan(longest * (size_t)channels, channels, grade, dtype, MAVG_ALGO_AUTO, 0, row, sizeof(row));
  if (c != MAVG_OK) return c;
  snprintf(buf, buflen, "ragged_loop rows=%zu max_row_frames=%zu x %s", rows, longest, row);
  return MAVG_OK;
}

// One launch of the ragged scan where it applies (ragged_fast_path), else the single-signal
// dispatch once per non-empty row on the same stream, every row planned before the first is
// launched.  The host offsets are validated and drive the dispatch and the loop; the kernel reads
// the device copy.
int mavg_ragged_run(const void* d_in, void* d_out, const int64_t* h_offsets, const int64_t* d_offsets, size_t rows,
                    int channels, int grade, int dtype, void* d_ws, size_t ws_bytes, void* stream) {
  size_t frames = 0, longest = 0;
  const int st = validate_ragged(h_offsets, rows, channels, grade, dtype, &frames, &longest);
  if (st != MAVG_OK) return st;
  if (frames == 0) return MAVG_OK;
  if (d_in == nullptr || d_out == nullptr || d_offsets == nullptr) return MAVG_ERR_INVALID_ARG;
  const size_t eb = elem_size(dtype);
  if (!aligned(d_in, eb) || !aligned(d_out, eb) || !aligned(d_offsets, 8)) return MAVG_ERR_MISALIGNED;
  if (ragged_fast_path(longest, channels, grade, dtype))
    return ragged_fast_launch(d_in, d_out, d_offsets, rows, frames, longest, channels, grade, dtype,
                              static_cast<hipStream_t>(stream));
  // ragged_loop: one mavg_run per non-empty row (a misaligned row: two), all sharing the caller's
  // workspace -- launches on one stream are serial and each zeroes its records
  const size_t fb = (size_t)channels * eb;
  auto row_run = [&](size_t r, bool dry) -> int {
    const size_t f0 = (size_t)h_offsets[r], nf = (size_t)(h_offsets[r + 1] - h_offsets[r]);
    if (nf == 0) return MAVG_OK;
    return run_signal(static_cast<const char*>(d_in) + f0 * fb, static_cast<char*>(d_out) + f0 * fb,
                      nf * (size_t)channels, channels, grade, dtype, MAVG_ALGO_AUTO, 0, nullptr, d_ws, ws_bytes, stream,
                      dry);
  };
  // (the workspace: the longest row's; every row is dry-run -- their lengths and alignments differ)
  return run_row_loop(rows, rows, longest * (size_t)channels, channels, grade, dtype, d_ws, ws_bytes, row_run);
}

}  // extern "C"
