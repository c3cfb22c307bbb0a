// mavg_decim.hip -- the decimated moving average's instances (the compacting tile scan: fp32 and
// int16, one and two channels, the 16-B-unit form and the frame-unit form; the window sum: both
// dtypes, 1..8 channels; the gather) and their launch.
#include "mavg_launch.hpp"
#include "mavg_decim.hpp"

namespace mavg {

namespace {

constexpr int kDecimNt = kNtSplit | kNtHalo | kNtStore;  // the tile scan's split policy
// Tile shapes: the segmented scan's (mavg_segscan.hip) -- 8-KiB tiles for fp32 (U = 2), 16-KiB
// tiles for int16 (U = 4); the frame-unit form takes 1024-frame tiles (F = 1, U = 4).
template <typename T>
constexpr int kDecimU = sizeof(T) == 2 ? 4 : 2;
// The halos the compacting scan takes.  Narrower than rows_scan's 16 KiB (mavg_segscan.hip
// kSegMaxHaloBytes), by measurement: with these 8- and 16-KiB tiles a 16-KiB halo doubles or triples
// the bytes a tile loads, and at 2^30 samples the scan then lost to mavg_run plus a slice copy
// (fp32 mono k=4096 hop=4096: 2.05 ms against 1.39 ms; int16 stereo 0.86 against 0.74), while at
// 8 KiB it still won (fp32 mono k=2048: 1.21 against 1.35 ms; int16 stereo 0.64 against 0.70;
// tools/bench_decim.py, DESIGN.md "Decimated").  Nothing was measured between the two.
constexpr long long kDecimMaxHaloBytes = 8192;

DecimParams decim_params(const DecimSig& ds, int k) {
  DecimParams p{};
  p.in = ds.in;
  p.out = ds.out;
  p.hist = ds.hist;
  p.nframes = (long long)ds.nframes;
  p.out_frames = (long long)ds.out_frames;
  p.k = k;
  p.hop = ds.hop;
  p.phase = ds.phase;
  p.eio = ds.eio;
  p.o = make_out_params(k);
  return p;
}

// DV: the int16 output division, the magic multiply as in the tile scan (grade <= 65535 here)
template <typename T, typename A, int C, int F, int U, int WG = kWG, int DV = (sizeof(T) == 2 ? 1 : 0)>
int launch_decim_scan(const DecimSig& ds, int k, hipStream_t st, int xcd_remap = kRemapGroup) {
  constexpr int TF = WG * F * U;
  constexpr int VE = F * C;
  const size_t lds = DecimLds<T, A, C, F, U, WG>(tile_halo_units<F>(k)).bytes;
  if (lds > lds_budget(WG)) return MAVG_ERR_UNSUPPORTED;
  DecimParams p = decim_params(ds, k);
  p.ntiles = (p.nframes + TF - 1) / TF;
  p.halo_units = (int)tile_halo_units<F>(k);
  p.xk_off = (int)((VE - ((long long)k * C) % VE) % VE);
  p.xcd_remap = xcd_remap;
  if (grid_too_large(p.ntiles, WG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "decim_scan<%s,acc=%s,C=%d,F=%d,U=%d,nt=%d,dv=%d> frames=%lld hop=%d phase=%d out_frames=%lld grid=%lld "
             "block=%d lds=%zu tile_frames=%d remap=%d",
             type_name<T>(), type_name<A>(), C, F, U, kDecimNt, DV, p.nframes, p.hop, p.phase, p.out_frames, p.ntiles,
             WG, lds, TF, xcd_remap);
    return MAVG_OK;
  }
  return launch_kernel<&decim_scan_kernel<T, A, C, F, U, WG, kDecimNt, DV>>(p.ntiles, WG, lds, lds_budget(WG), st, p);
}

template <typename T_, typename A_, int C_>
struct DecimInst {
  using T = T_;
  using A = A_;
  static constexpr int C = C_;
  static constexpr int F = 16 / (C * (int)sizeof(T));  // frames per 16-B unit
};
template <typename R, typename Fn>
R decim_scan_switch(int dtype, int C, R none, Fn fn) {
  if (dtype == MAVG_F32) return C == 1 ? fn(DecimInst<float, double, 1>{}) : C == 2 ? fn(DecimInst<float, double, 2>{}) : none;
  return C == 1 ? fn(DecimInst<int16_t, int32_t, 1>{}) : C == 2 ? fn(DecimInst<int16_t, int32_t, 2>{}) : none;
}

template <typename T, typename A, int C>
int launch_decim_window(const DecimSig& ds, int k, hipStream_t st) {
  constexpr int WG = kWG;
  constexpr int FB = C * (int)sizeof(T);
  DecimParams p = decim_params(ds, k);
  const long long groups = (p.out_frames + WG / 64 - 1) / (WG / 64);
  if (grid_too_large(groups, WG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "decim_window<%s,acc=%s,C=%d,vec=%d> frames=%lld hop=%d phase=%d out_frames=%lld grid=%lld block=%d",
             type_name<T>(), type_name<A>(), C, (FB <= 16 && 16 % FB == 0 && ds.eio == 0) ? 1 : 0, p.nframes, p.hop, p.phase,
             p.out_frames, groups, WG);
    return MAVG_OK;
  }
  return launch_kernel<&decim_window_kernel<T, A, C, WG>>(groups, WG, 0, 0, st, p);
}

}  // namespace

bool decim_scan_fits(int dtype, int C, int grade) {
  if (grade < 2) return false;                           // grade 1 is a copy, never a scan (mavg_api.hip)
  if (dtype != MAVG_F32 && grade > 65535) return false;  // int32 sums and the exact-division helpers' domain
  return decim_scan_switch(dtype, C, false, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    using A = typename I::A;
    if ((long long)grade * I::C * (long long)sizeof(T) > kDecimMaxHaloBytes) return false;
    return DecimLds<T, A, I::C, I::F, kDecimU<T>, kWG>(tile_halo_units<I::F>(grade)).bytes <= lds_budget(kWG) &&
           DecimLds<T, A, I::C, 1, 4, kWG>(tile_halo_units<1>(grade)).bytes <= lds_budget(kWG);
  });
}

int decim_scan_any(int dtype, int C, const DecimSig& ds, int grade, hipStream_t st) {
  if (ds.hop < 2 || !decim_scan_fits(dtype, C, grade)) return MAVG_ERR_UNSUPPORTED;
  return decim_scan_switch(dtype, C, (int)MAVG_ERR_UNSUPPORTED, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    using A = typename I::A;
    if (!ds.unit) return launch_decim_scan<T, A, I::C, 1, 4>(ds, grade, st);
    return launch_decim_scan<T, A, I::C, I::F, kDecimU<T>>(ds, grade, st);
  });
}

int decim_window_any(int dtype, int C, const DecimSig& ds, int grade, hipStream_t st) {
  return dispatch_int<1, 2, 3, 4, 5, 6, 7, 8>(C, MAVG_ERR_UNSUPPORTED, [&](auto c) {
    constexpr int CC = decltype(c)::value;
    if (dtype == MAVG_F32) return launch_decim_window<float, double, CC>(ds, grade, st);
    return launch_decim_window<int16_t, int64_t, CC>(ds, grade, st);
  });
}

int decim_gather_any(int dtype, int C, const void* full, const DecimSig& ds, hipStream_t st) {
  const long long M = (long long)ds.out_frames;
  if (M > (1LL << 62) / C) return MAVG_ERR_UNSUPPORTED;  // the sample index stays in int64
  const long long n = M * C;
  const long long groups = std::min<long long>((n + kWG - 1) / kWG, 1LL << 16);  // a grid-stride loop past it
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text), "decim_gather<%s> out_frames=%lld grid=%lld block=%d",
             dtype == MAVG_F32 ? "f32" : "i16", M, groups, kWG);
    return MAVG_OK;
  }
  if (dtype == MAVG_F32)
    hipLaunchKernelGGL(decim_gather_kernel<float>, dim3((unsigned)groups), dim3(kWG), 0, st, static_cast<const float*>(full),
                       static_cast<float*>(ds.out), M, (long long)ds.nframes, C, ds.hop, ds.phase);
  else
    hipLaunchKernelGGL(decim_gather_kernel<int16_t>, dim3((unsigned)groups), dim3(kWG), 0, st,
                       static_cast<const int16_t*>(full), static_cast<int16_t*>(ds.out), M, (long long)ds.nframes, C, ds.hop,
                       ds.phase);
  return hipGetLastError() == hipSuccess ? MAVG_OK : MAVG_ERR_HIP;
}

}  // namespace mavg
