// mavg_extrema.hip -- the moving extrema's instances (fp32 and int16, one and two channels, the
// 16-B-unit form and the frame-unit form, max, min and both; the strip kernel per dtype) and
// their launch.
#include "mavg_launch.hpp"
#include "mavg_extrema.hpp"

namespace mavg {

namespace {

constexpr int kExtNt = kNtSplit | kNtHalo | kNtStore;  // the tile scan's split policy
// Tile shapes of the 16-B-unit form (the lane keeps its units in registers across the table's
// barriers): 16-KiB tiles (U = 4) for one output, 8-KiB tiles (U = 2) for both.  Measured at 2^30
// samples, k = 1024 (tools/bench_extrema.py, DESIGN.md "Extrema"): one output 1.12 - 2.18x the
// time of mavg_run with U = 4 against 1.36 - 2.32x with U = 2 (a 16-KiB tile carries half the halo
// units per output); both outputs 3.2 - 8.7x with U = 4 against 2.2 - 6.5x with U = 2 (twice the
// LDS: fewer workgroups to hide the barriers behind).  The frame-unit form: 1024-frame tiles.
constexpr int kExtU = 4;
constexpr int kExtBothU = 2;
constexpr int kExtFrameU = 4;

int floor_log2(long long v) {
  int l = -1;
  while (v > 0) { v >>= 1; ++l; }
  return l;
}

template <typename T, int C, int F, int U, int M, int WG = kWG>
int launch_extrema_tile(const ExtremaSig& es, int k, hipStream_t st, int xcd_remap = kRemapGroup) {
  constexpr int TF = WG * F * U;
  constexpr int VE = F * C;
  constexpr int NO = M == kExtBoth ? 2 : 1;
  const size_t Hu = tile_halo_units<F>(k);
  const size_t lds = ExtremaLds<T, C, F, U, WG>(Hu, NO).bytes;
  if (lds > lds_budget(WG)) return MAVG_ERR_UNSUPPORTED;
  ExtremaParams p{};
  p.in = es.in;
  p.omax = es.omax;
  p.omin = es.omin;
  p.hist = es.hist;
  p.nframes = (long long)es.nframes;
  p.ntiles = (p.nframes + TF - 1) / TF;
  p.k = k;
  p.halo_units = (int)Hu;
  p.s_off = (int)((VE - ((long long)(k - 1) * C) % VE) % VE);
  p.span = F == 1 ? k : (k - 1) / F - 1;   // whole units between the window's first unit and the lane's
  if (p.span < 0) p.span = 0;
  p.levels = floor_log2(p.span);
  p.xcd_remap = xcd_remap;
  p.eio = es.eio;
  if (grid_too_large(p.ntiles, WG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "extrema_tile<%s,C=%d,F=%d,U=%d,M=%d,nt=%d> max=%d min=%d frames=%lld halo_frames=%d levels=%d grid=%lld "
             "block=%d lds=%zu tile_frames=%d remap=%d",
             type_name<T>(), C, F, U, M, kExtNt, es.omax != nullptr ? 1 : 0, es.omin != nullptr ? 1 : 0, p.nframes, k - 1,
             p.levels < 0 ? 0 : p.levels, p.ntiles, WG, lds, TF, xcd_remap);
    return MAVG_OK;
  }
  return launch_kernel<&extrema_tile_kernel<T, C, F, U, M, WG, kExtNt>>(p.ntiles, WG, lds, lds_budget(WG), st, p);
}

template <typename T_, int C_>
struct ExtInst {
  using T = T_;
  static constexpr int C = C_;
  static constexpr int F = 16 / (C * (int)sizeof(T));  // frames per 16-B unit
};
template <typename R, typename Fn>
R ext_switch(int dtype, int C, R none, Fn fn) {
  if (dtype == MAVG_F32) return C == 1 ? fn(ExtInst<float, 1>{}) : C == 2 ? fn(ExtInst<float, 2>{}) : none;
  return C == 1 ? fn(ExtInst<int16_t, 1>{}) : C == 2 ? fn(ExtInst<int16_t, 2>{}) : none;
}

// U: tile units per lane for one output, UB: for both
template <typename T, int C, int F, int U, int UB>
int launch_extrema_outputs(const ExtremaSig& es, int k, hipStream_t st) {
  if (es.omax != nullptr && es.omin != nullptr) return launch_extrema_tile<T, C, F, UB, kExtBoth>(es, k, st);
  if (es.omax != nullptr) return launch_extrema_tile<T, C, F, U, kExtMax>(es, k, st);
  return launch_extrema_tile<T, C, F, U, kExtMin>(es, k, st);
}

template <typename T>
int launch_extrema_strip(int C, const ExtremaSig& es, int k, hipStream_t st) {
  ExtStripParams p{};
  p.in = es.in;
  p.omax = es.omax;
  p.omin = es.omin;
  p.hist = es.hist;
  p.nframes = (long long)es.nframes;
  p.C = C;
  p.k = k;
  p.L = extrema_strip_frames(k);
  p.nstrips = (p.nframes + p.L - 1) / p.L;
  if (p.nstrips > 0x7fffffffffffffffLL / C) return MAVG_ERR_UNSUPPORTED;
  const long long groups = (p.nstrips * C + kWG - 1) / kWG;
  if (grid_too_large(groups, kWG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "extrema_strip dtype=%s C=%d max=%d min=%d frames=%lld grade=%d L=%d strips=%lld grid=%lld block=%d%s",
             type_name<T>(), C, es.omax != nullptr ? 1 : 0, es.omin != nullptr ? 1 : 0, p.nframes, k, p.L, p.nstrips,
             groups, kWG, k <= kExtDirectMax ? " direct" : "");
    return MAVG_OK;
  }
  return launch_kernel<&extrema_strip_kernel<T, kWG>>(groups, kWG, 0, lds_budget(kWG), st, p);
}

}  // namespace

// The strip length for a window: a quarter of it, so that the backward walk over the k - 1 frames
// before a strip costs about four reads per output; at least 16 frames, at most 2048 (a long
// signal still makes thousands of threads).  L <= grade - 1 from grade 17 on, which the kernel's
// parking needs; shorter windows are evaluated directly.
int extrema_strip_frames(int grade) { return std::min(std::max(grade / 4, 16), 2048); }

bool extrema_tile_fits(int dtype, int C, int grade) {
  if (grade < 2) return false;
  return ext_switch(dtype, C, false, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    if ((long long)(grade - 1) * I::C * (long long)sizeof(T) > kExtMaxHaloBytes) return false;
    return ExtremaLds<T, I::C, I::F, kExtU, kWG>(tile_halo_units<I::F>(grade), 1).bytes <= lds_budget(kWG) &&
           ExtremaLds<T, I::C, I::F, kExtBothU, kWG>(tile_halo_units<I::F>(grade), 2).bytes <= lds_budget(kWG) &&
           ExtremaLds<T, I::C, 1, kExtFrameU, kWG>(tile_halo_units<1>(grade), 2).bytes <= lds_budget(kWG);
  });
}

int extrema_tile_any(int dtype, int C, const ExtremaSig& es, int grade, hipStream_t st) {
  if (!extrema_tile_fits(dtype, C, grade)) return MAVG_ERR_UNSUPPORTED;
  return ext_switch(dtype, C, (int)MAVG_ERR_UNSUPPORTED, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    if (!es.unit) return launch_extrema_outputs<T, I::C, 1, kExtFrameU, kExtFrameU>(es, grade, st);
    return launch_extrema_outputs<T, I::C, I::F, kExtU, kExtBothU>(es, grade, st);
  });
}

int extrema_strip_any(int dtype, int C, const ExtremaSig& es, int grade, hipStream_t st) {
  return dtype == MAVG_F32 ? launch_extrema_strip<float>(C, es, grade, st)
                           : launch_extrema_strip<int16_t>(C, es, grade, st);
}

}  // namespace mavg
