// mavg_ema.hip -- the exponential moving average's instances (fp32 and int16, one and two channels,
// the 16-B-unit form and the frame-unit form, for the tile kernel and the chain's two ends; the
// strip kernels per dtype; the carry kernel), their launchers and the fit check.
#include "mavg_launch.hpp"
#include "mavg_ema.hpp"

namespace mavg {

namespace {

constexpr int kEmaNt = kNtSplit | kNtHalo | kNtStore;  // the tile kernel: the tile scan's split policy
constexpr int kEmaNtAgg = 0;                           // chain step A: plain loads (step C re-reads them)
constexpr int kEmaNtApply = kNtLoad | kNtStore;        // chain step C: streamed once from here on
// Tile shapes: the moments' -- 8-KiB tiles for fp32 (U = 2), 16-KiB tiles for int16 (U = 4); the
// frame-unit form takes 1024-frame tiles (F = 1, U = 4).
template <typename T>
constexpr int kEmaU = sizeof(T) == 2 ? 4 : 2;
constexpr int kEmaFrameU = 4;
constexpr int kEmaFrameTF = kWG * kEmaFrameU;  // the smaller tile: what the workspace is sized for
// The halos H * C * sample size the tile kernel takes, and the dispatch rule gives it: the stage
// limit of every tile kernel here.  Measured against the chain forced on the same shapes at halos of
// 256 B, 2, 8 and 16 KiB (tools/bench_ema.py --pairs, DESIGN.md "EMA"): 1.1x (fp32 mono at 16 KiB)
// to 2.3x faster everywhere.
constexpr long long kEmaMaxHaloBytes = 16384;
// The strip form's frames per thread.
constexpr int kEmaStripFrames = 64;

// d^(m 2^i), i = 0 .. 5, each straight from d (no repeated squaring: one rounding each)
DecayPow make_decay_pow(double d, double m) {
  DecayPow b{};
  for (int i = 0; i < 6; ++i) b.p[i] = std::pow(d, m * (double)(1 << i));
  return b;
}

int state_bits(const EmaSig& es) { return (es.state_in != nullptr ? 1 : 0) | (es.state_out != nullptr ? 2 : 0); }

template <typename T, int C, int F, int U, int WG = kWG>
EmaParams make_ema_params(const EmaSig& es, int halo_frames) {
  constexpr int TF = WG * F * U;
  EmaParams p{};
  p.in = es.in;
  p.out = es.out;
  p.state_in = es.state_in;
  p.state_out = es.state_out;
  p.nframes = (long long)es.nframes;
  p.ntiles = (p.nframes + TF - 1) / TF;
  p.alpha = es.alpha;
  p.d = 1.0 - es.alpha;
  p.unit = make_decay_pow(p.d, (double)F);
  p.seg = make_decay_pow(p.d, 64.0 * F);
  p.d_tile = std::pow(p.d, (double)TF);
  p.halo_frames = halo_frames;
  p.halo_units = (int)tile_halo_units<F>(halo_frames);
  p.halo_run = (p.halo_units * F + WG - 1) / WG;
  p.run = make_decay_pow(p.d, (double)std::max(p.halo_run, 1));
  p.run_wave = std::pow(p.d, 64.0 * std::max(p.halo_run, 1));
  p.xcd_remap = kRemapGroup;
  p.eio = es.eio;
  return p;
}

template <typename T, int C, int F, int U, int WG = kWG>
int launch_ema_tile(const EmaSig& es, hipStream_t st) {
  constexpr int TF = WG * F * U;
  const long long H = ema_halo_frames(es.alpha);
  if (H * C * (long long)sizeof(T) > kEmaMaxHaloBytes) return MAVG_ERR_UNSUPPORTED;
  const EmaParams p = make_ema_params<T, C, F, U, WG>(es, (int)H);  // (H == 0: no halo units, no runs)
  const size_t lds = EmaLds<T, C, F, U, WG>((size_t)p.halo_units).bytes;
  if (lds > lds_budget(WG) || grid_too_large(p.ntiles, WG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "ema_tile<%s,C=%d,F=%d,U=%d,nt=%d> alpha=%.17g halo_frames=%lld state=%d frames=%lld grid=%lld block=%d "
             "lds=%zu tile_frames=%d remap=%d",
             type_name<T>(), C, F, U, kEmaNt, es.alpha, H, state_bits(es), p.nframes, p.ntiles, WG, lds, TF, p.xcd_remap);
    return MAVG_OK;
  }
  return launch_kernel<&ema_tile_kernel<T, C, F, U, WG, kEmaNt>>(p.ntiles, WG, lds, lds_budget(WG), st, p);
}

// step B's parameters for `records` spans of `span` frames each, the last of `last_frames`
EmaCarryParams make_carry_params(const EmaSig& es, int C, double* rec, long long records, int span, long long last_frames) {
  EmaCarryParams q{};
  const double d = 1.0 - es.alpha;
  q.rec = rec;
  q.state_in = es.state_in;
  q.state_out = es.state_out;
  q.records = records;
  q.C = C;
  q.D = std::pow(d, (double)span);
  q.lanes = make_decay_pow(d, (double)span * kEmaCarryRun);
  q.wave = std::pow(d, (double)span * kEmaCarryRun * 64.0);
  q.d_last = std::pow(d, (double)last_frames);
  return q;
}

int launch_ema_carry(const EmaCarryParams& q, hipStream_t st) {
  hipLaunchKernelGGL(ema_carry_kernel<kWG>, dim3(1), dim3(kWG), 0, st, q);
  return hipGetLastError() == hipSuccess ? MAVG_OK : MAVG_ERR_HIP;
}

// the caller's workspace against `need` bytes of records
int check_records(size_t need, Workspace ws) {
  if (ws.ptr == nullptr || ws.bytes < need) return MAVG_ERR_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(ws.ptr) & 15u) != 0) return MAVG_ERR_MISALIGNED;
  return MAVG_OK;
}

template <typename T, int C, int F, int U, int WG = kWG>
int launch_ema_chain(const EmaSig& es, Workspace ws, hipStream_t st) {
  constexpr int TF = WG * F * U;
  EmaParams p = make_ema_params<T, C, F, U, WG>(es, 0);  // no halo
  p.state_out = nullptr;  // step B writes it
  const size_t lds = EmaLds<T, C, F, U, WG>(0).bytes;
  if (lds > lds_budget(WG) || grid_too_large(p.ntiles, WG)) return MAVG_ERR_UNSUPPORTED;
  const size_t need = (((size_t)p.ntiles * C * sizeof(double)) + 15) & ~(size_t)15;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "ema_chain<%s,C=%d,F=%d,U=%d,nt=%d> alpha=%.17g state=%d frames=%lld grid=%lld block=%d lds=%zu "
             "tile_frames=%d records=%lld carry_chunk=%d launches=3",
             type_name<T>(), C, F, U, kEmaNtApply, es.alpha, state_bits(es), p.nframes, p.ntiles, WG, lds, TF, p.ntiles,
             kEmaCarryChunk);
    g_plan->ws_bytes = need;
    return MAVG_OK;
  }
  int s = check_records(need, ws);
  if (s != MAVG_OK) return s;
  p.rec = static_cast<double*>(ws.ptr);
  const EmaCarryParams q =
      make_carry_params(es, C, p.rec, p.ntiles, TF, p.nframes - (p.ntiles - 1) * (long long)TF);
  s = launch_kernel<&ema_agg_kernel<T, C, F, U, WG, kEmaNtAgg>>(p.ntiles, WG, lds, lds_budget(WG), st, p);
  if (s != MAVG_OK) return s;
  s = launch_ema_carry(q, st);
  if (s != MAVG_OK) return s;
  return launch_kernel<&ema_apply_kernel<T, C, F, U, WG, kEmaNtApply>>(p.ntiles, WG, lds, lds_budget(WG), st, p);
}

template <typename T>
int launch_ema_strip(int C, const EmaSig& es, Workspace ws, hipStream_t st) {
  EmaStripParams p{};
  p.in = es.in;
  p.out = es.out;
  p.nframes = (long long)es.nframes;
  p.L = kEmaStripFrames;
  p.nstrips = (p.nframes + p.L - 1) / p.L;
  p.alpha = es.alpha;
  p.d = 1.0 - es.alpha;
  p.C = C;
  if (p.nstrips > 0x7fffffffffffffffLL / 16 / C) return MAVG_ERR_UNSUPPORTED;
  const long long groups = (p.nstrips * C + kWG - 1) / kWG;
  if (grid_too_large(groups, kWG)) return MAVG_ERR_UNSUPPORTED;
  const size_t need = (((size_t)p.nstrips * C * sizeof(double)) + 15) & ~(size_t)15;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "ema_strip dtype=%s C=%d L=%d strips=%lld carry_chunk=%d launches=3 alpha=%.17g state=%d frames=%lld "
             "grid=%lld block=%d",
             type_name<T>(), C, p.L, p.nstrips, kEmaCarryChunk, es.alpha, state_bits(es), p.nframes, groups, kWG);
    g_plan->ws_bytes = need;
    return MAVG_OK;
  }
  int s = check_records(need, ws);
  if (s != MAVG_OK) return s;
  p.rec = static_cast<double*>(ws.ptr);
  const EmaCarryParams q = make_carry_params(es, C, p.rec, p.nstrips, p.L, p.nframes - (p.nstrips - 1) * (long long)p.L);
  s = launch_kernel<&ema_strip_kernel<T, false, kWG>>(groups, kWG, 0, lds_budget(kWG), st, p);
  if (s != MAVG_OK) return s;
  s = launch_ema_carry(q, st);
  if (s != MAVG_OK) return s;
  return launch_kernel<&ema_strip_kernel<T, true, kWG>>(groups, kWG, 0, lds_budget(kWG), st, p);
}

template <typename T_, int C_>
struct EmaInst {
  using T = T_;
  static constexpr int C = C_;
  static constexpr int F = 16 / (C * (int)sizeof(T));  // frames per 16-B unit
};
template <typename R, typename Fn>
R ema_switch(int dtype, int C, R none, Fn fn) {
  if (dtype == MAVG_F32) return C == 1 ? fn(EmaInst<float, 1>{}) : C == 2 ? fn(EmaInst<float, 2>{}) : none;
  return C == 1 ? fn(EmaInst<int16_t, 1>{}) : C == 2 ? fn(EmaInst<int16_t, 2>{}) : none;
}

int records_bytes(size_t nframes, size_t span, int C, size_t* bytes) {
  const size_t records = nframes / span + (nframes % span != 0 ? 1 : 0);
  if (records > (SIZE_MAX / 8 - 2) / (size_t)C) return MAVG_ERR_UNSUPPORTED;
  *bytes = (records * (size_t)C * sizeof(double) + 15) & ~(size_t)15;
  return MAVG_OK;
}

}  // namespace

long long ema_halo_frames(double alpha) {
  const double d = 1.0 - alpha;
  if (!(d > 0.0)) return 0;  // alpha == 1: y = x
  const double bound = 0x1p-30;
  long long H = (long long)std::ceil(-30.0 / std::log2(d));
  if (H < 1) H = 1;
  while (H > 1 && std::pow(d, (double)(H - 1)) <= bound) --H;
  while (std::pow(d, (double)H) > bound) ++H;
  return H;
}

bool ema_tile_fits(int dtype, int C, double alpha) {
  const long long H = ema_halo_frames(alpha);
  return ema_switch(dtype, C, false, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    if (H * I::C * (long long)sizeof(T) > kEmaMaxHaloBytes) return false;
    return EmaLds<T, I::C, I::F, kEmaU<T>, kWG>(tile_halo_units<I::F>((int)H)).bytes <= lds_budget(kWG) &&
           EmaLds<T, I::C, 1, kEmaFrameU, kWG>(tile_halo_units<1>((int)H)).bytes <= lds_budget(kWG);
  });
}

int ema_tile_any(int dtype, int C, const EmaSig& es, hipStream_t st) {
  if (!ema_tile_fits(dtype, C, es.alpha)) return MAVG_ERR_UNSUPPORTED;
  return ema_switch(dtype, C, (int)MAVG_ERR_UNSUPPORTED, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    if (!es.unit) return launch_ema_tile<T, I::C, 1, kEmaFrameU>(es, st);
    return launch_ema_tile<T, I::C, I::F, kEmaU<T>>(es, st);
  });
}

int ema_chain_any(int dtype, int C, const EmaSig& es, Workspace ws, hipStream_t st) {
  return ema_switch(dtype, C, (int)MAVG_ERR_UNSUPPORTED, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    if (!es.unit) return launch_ema_chain<T, I::C, 1, kEmaFrameU>(es, ws, st);
    return launch_ema_chain<T, I::C, I::F, kEmaU<T>>(es, ws, st);
  });
}

int ema_strip_any(int dtype, int C, const EmaSig& es, Workspace ws, hipStream_t st) {
  return dtype == MAVG_F32 ? launch_ema_strip<float>(C, es, ws, st) : launch_ema_strip<int16_t>(C, es, ws, st);
}

int ema_chain_ws_bytes(size_t nframes, int C, size_t* bytes) { return records_bytes(nframes, kEmaFrameTF, C, bytes); }
int ema_strip_ws_bytes(size_t nframes, int C, size_t* bytes) { return records_bytes(nframes, kEmaStripFrames, C, bytes); }

}  // namespace mavg
