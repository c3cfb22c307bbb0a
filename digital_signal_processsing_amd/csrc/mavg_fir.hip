// mavg_fir.hip -- the FIR filter's instances (fp32 and int16, one and two channels, the 16-B-unit
// form and the frame-unit form; the strip kernel per dtype) and their launch.
#include "mavg_launch.hpp"
#include "mavg_fir.hpp"

namespace mavg {

namespace {

constexpr int kFirNt = kNtStore;  // outputs are written once; the inputs are re-read as halos
// Units per lane.  The 16-B-unit form keeps R * C = 16 accumulators: fp32 U = 4 (R = 16 mono, 8
// stereo; 16-KiB tiles), int16 U = 2 (R = 16 mono, 8 stereo; 8-KiB tiles of input, 16 KiB of
// output).  The frame-unit form: 8 frames per lane, 2048-frame tiles.
constexpr int kFirFrameU = 8;
constexpr long long kFirMaxHaloBytes = 16 * 1024;

template <typename T, int C, int F, int U, int WG = kWG>
int launch_fir_tile(const FirSig& fs, int ntaps, hipStream_t st, int xcd_remap = kRemapGroup) {
  constexpr int R = U * F;
  constexpr int TF = WG * R;
  const size_t m = fir_halo_units<F>(ntaps);
  const size_t lds = FirLds<T, C, F, U, WG>(m).bytes;
  if (lds > lds_budget(WG)) return MAVG_ERR_UNSUPPORTED;
  FirParams p{};
  p.in = fs.in;
  p.out = fs.out;
  p.hist = fs.hist;
  p.taps = fs.taps;
  p.nframes = (long long)fs.nframes;
  p.ntaps = ntaps;
  p.m = (int)m;
  p.xcd_remap = xcd_remap;
  p.eio = fs.eio;
  const long long ntiles = (p.nframes + TF - 1) / TF;
  if (grid_too_large(ntiles, WG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "fir_tile<%s,C=%d,F=%d,U=%d,R=%d> taps=%d halo_frames=%d history=%d frames=%lld halo_units=%zu "
             "fma_per_lds_dword=%d grid=%lld block=%d lds=%zu tile_frames=%d remap=%d nt=%d",
             type_name<T>(), C, F, U, R, ntaps, ntaps - 1, fs.hist != nullptr ? 1 : 0, p.nframes, m,
             R * F * C * 4 / (F * C * (int)sizeof(T)), ntiles, WG, lds, TF, xcd_remap, kFirNt);
    return MAVG_OK;
  }
  return launch_kernel<&fir_tile_kernel<T, C, F, U, WG, kFirNt>>(ntiles, WG, lds, lds_budget(WG), st, p);
}

template <typename T_, int C_>
struct FirInst {
  using T = T_;
  static constexpr int C = C_;
  static constexpr int F = 16 / (C * (int)sizeof(T));  // frames per 16-B unit
  static constexpr int U = sizeof(T) == 4 ? 4 : 2;
};
template <typename R, typename Fn>
R fir_switch(int dtype, int C, R none, Fn fn) {
  if (dtype == MAVG_F32) return C == 1 ? fn(FirInst<float, 1>{}) : C == 2 ? fn(FirInst<float, 2>{}) : none;
  return C == 1 ? fn(FirInst<int16_t, 1>{}) : C == 2 ? fn(FirInst<int16_t, 2>{}) : none;
}

template <typename T>
int launch_fir_strip(int C, const FirSig& fs, int ntaps, hipStream_t st) {
  FirStripParams p{};
  p.in = fs.in;
  p.out = fs.out;
  p.hist = fs.hist;
  p.taps = fs.taps;
  p.nframes = (long long)fs.nframes;
  p.C = C;
  p.ntaps = ntaps;
  p.L = kFirStripFrames;
  p.nstrips = (p.nframes + p.L - 1) / p.L;
  if (p.nstrips > 0x7fffffffffffffffLL / C) return MAVG_ERR_UNSUPPORTED;
  const long long groups = (p.nstrips * C + kWG - 1) / kWG;
  if (grid_too_large(groups, kWG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "fir_strip dtype=%s C=%d taps=%d L=%d strips=%lld history=%d frames=%lld grid=%lld block=%d",
             type_name<T>(), C, ntaps, p.L, p.nstrips, fs.hist != nullptr ? 1 : 0, p.nframes, groups, kWG);
    return MAVG_OK;
  }
  return launch_kernel<&fir_strip_kernel<T, kWG>>(groups, kWG, 0, lds_budget(kWG), st, p);
}

}  // namespace

bool fir_tile_fits(int dtype, int C, int ntaps) {
  if (ntaps < 1) return false;
  return fir_switch(dtype, C, false, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    if ((long long)(ntaps - 1) * I::C * (long long)sizeof(T) > kFirMaxHaloBytes) return false;
    return FirLds<T, I::C, I::F, I::U, kWG>(fir_halo_units<I::F>(ntaps)).bytes <= lds_budget(kWG) &&
           FirLds<T, I::C, 1, kFirFrameU, kWG>(fir_halo_units<1>(ntaps)).bytes <= lds_budget(kWG);
  });
}

int fir_tile_any(int dtype, int C, const FirSig& fs, int ntaps, hipStream_t st) {
  if (!fir_tile_fits(dtype, C, ntaps)) return MAVG_ERR_UNSUPPORTED;
  return fir_switch(dtype, C, (int)MAVG_ERR_UNSUPPORTED, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    if (!fs.unit) return launch_fir_tile<T, I::C, 1, kFirFrameU>(fs, ntaps, st);
    return launch_fir_tile<T, I::C, I::F, I::U>(fs, ntaps, st);
  });
}

int fir_strip_any(int dtype, int C, const FirSig& fs, int ntaps, hipStream_t st) {
  return dtype == MAVG_F32 ? launch_fir_strip<float>(C, fs, ntaps, st) : launch_fir_strip<int16_t>(C, fs, ntaps, st);
}

}  // namespace mavg
