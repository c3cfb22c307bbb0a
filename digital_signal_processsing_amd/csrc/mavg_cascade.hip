// mavg_cascade.hip -- the cascaded moving average's instances (fp32 and int16, one and two
// channels, the 16-B-unit form and the frame-unit form) and their launch.
#include "mavg_launch.hpp"
#include "mavg_cascade.hpp"

namespace mavg {

namespace {

constexpr int kCascadeNt = kNtSplit | kNtHalo | kNtStore;  // the tile scan's split policy
// Tile shapes: the decimated scan's (mavg_decim.hip) -- 8-KiB tiles for fp32 (U = 2), 16-KiB tiles
// for int16 (U = 4) while the two stages fit beside them, else 8-KiB tiles (U = 2); the frame-unit
// form takes 1024-frame tiles (F = 1, U = 4).
template <typename T>
constexpr int kCascadeU = sizeof(T) == 2 ? 4 : 2;
// The total halos passes * (grade - 1) * C * sample size the fused kernel CAN take (what its tests
// cover, and what mavg_debug_force_cascade may force): tile_scan's and rows_scan's 16 KiB.
constexpr long long kCascadeMaxHaloBytes = 16384;
// The total halos the dispatch RULE gives it, narrower by measurement (tools/bench_cascade.py
// --pairs, 2^30 samples, one MI355X, against `passes` x mavg_run through a ping-pong buffer in the
// same process; profiles/cascade/bench_cascade_pairs.txt, DESIGN.md "Cascade").  Yardstick time /
// fused time at total halos of 256 B | 2 KiB | 8 KiB | 16 KiB:
//   fp32 mono     2 passes 1.62 | 1.39 | 0.73 | 0.41   3 passes 1.77 | 1.60 | 0.89 | 0.52   4 passes 1.81 | 1.64 | 0.95 | 0.56
//   int16 mono    2 passes 1.10 | 1.02 | 0.61 | 0.28   3 passes 1.16 | 1.10 | 0.74 | 0.34   4 passes 1.21 | 1.17 | 0.77 | 0.36
//   int16 stereo  2 passes 1.11 | 1.06 | 0.71 | 0.38   3 passes 1.19 | 1.11 | 0.80 | 0.44   4 passes 1.21 | 1.17 | 0.83 | 0.44
// A class is kept where the fused kernel won by more than 5 % (the boxes' spread is 2 - 4 %): 2 KiB
// is the last measured point that won, and for two int16 passes (1.02 mono, 1.06 stereo: not a
// readable win) 256 B is.  Nothing was measured between 2 KiB and 8 KiB, nor below 256 B, nor on
// misaligned views (the frame-unit form), nor fp32 stereo (it takes fp32 mono's rule).
constexpr long long kCascadeRuleHaloBytes = 2048;
constexpr long long kCascadeRuleHaloBytesI16Two = 256;  // int16, passes == 2

// DV: the int16 output division, the magic multiply as in the tile scan (grade <= 65535 here)
template <typename T, typename A, int C, int F, int U, int WG = kWG, int DV = (sizeof(T) == 2 ? 1 : 0)>
int launch_cascade_tile(const CascadeSig& cs, int k, int passes, hipStream_t st, int xcd_remap = kRemapGroup) {
  constexpr int TF = WG * F * U;
  constexpr int VE = F * C;
  const int H = passes * (k - 1);  // no overflow: cascade_tile_fits bounds it
  const size_t Hu = tile_halo_units<F>(H);
  const size_t lds = CascadeLds<T, A, C, F, U, WG>(Hu).bytes;
  if (lds > lds_budget(WG)) return MAVG_ERR_UNSUPPORTED;
  CascadeParams p{};
  p.in = cs.in;
  p.out = cs.out;
  p.hist = cs.hist;
  p.nframes = (long long)cs.nframes;
  p.ntiles = (p.nframes + TF - 1) / TF;
  p.k = k;
  p.passes = passes;
  p.halo_frames = H;
  p.halo_units = (int)Hu;
  p.xk_units = (int)tile_halo_units<F>(k);
  p.xk_off = (int)((VE - ((long long)k * C) % VE) % VE);
  p.xcd_remap = xcd_remap;
  p.eio = cs.eio;
  p.o = make_out_params(k);
  if (grid_too_large(p.ntiles, WG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "cascade_tile<%s,acc=%s,C=%d,F=%d,U=%d,nt=%d,dv=%d> frames=%lld passes=%d halo_frames=%d grid=%lld "
             "block=%d lds=%zu tile_frames=%d remap=%d",
             type_name<T>(), type_name<A>(), C, F, U, kCascadeNt, DV, p.nframes, passes, H, p.ntiles, WG, lds, TF,
             xcd_remap);
    return MAVG_OK;
  }
  return launch_kernel<&cascade_tile_kernel<T, A, C, F, U, WG, kCascadeNt, DV>>(p.ntiles, WG, lds, lds_budget(WG), st, p);
}

template <typename T_, typename A_, int C_>
struct CascadeInst {
  using T = T_;
  using A = A_;
  static constexpr int C = C_;
  static constexpr int F = 16 / (C * (int)sizeof(T));  // frames per 16-B unit
};
template <typename R, typename Fn>
R cascade_switch(int dtype, int C, R none, Fn fn) {
  if (dtype == MAVG_F32)
    return C == 1 ? fn(CascadeInst<float, double, 1>{}) : C == 2 ? fn(CascadeInst<float, double, 2>{}) : none;
  return C == 1 ? fn(CascadeInst<int16_t, int32_t, 1>{}) : C == 2 ? fn(CascadeInst<int16_t, int32_t, 2>{}) : none;
}

}  // namespace

bool cascade_tile_preferred(int dtype, int C, int grade, int passes) {
  const long long halo = (long long)passes * (grade - 1) * C * (dtype == MAVG_F32 ? 4 : 2);
  return halo <= (dtype != MAVG_F32 && passes == 2 ? kCascadeRuleHaloBytesI16Two : kCascadeRuleHaloBytes);
}

bool cascade_tile_fits(int dtype, int C, int grade, int passes) {
  if (grade < 2 || passes < 2) return false;              // cascade_none (mavg_api.hip)
  if (dtype != MAVG_F32 && grade > 65535) return false;   // int32 sums and the exact-division helpers' domain
  return cascade_switch(dtype, C, false, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    using A = typename I::A;
    const long long H = (long long)passes * (grade - 1);
    if (H * I::C * (long long)sizeof(T) > kCascadeMaxHaloBytes) return false;
    // the narrowest tile of each form
    return CascadeLds<T, A, I::C, I::F, 2, kWG>(tile_halo_units<I::F>((int)H)).bytes <= lds_budget(kWG) &&
           CascadeLds<T, A, I::C, 1, 4, kWG>(tile_halo_units<1>((int)H)).bytes <= lds_budget(kWG);
  });
}

int cascade_tile_any(int dtype, int C, const CascadeSig& cs, int grade, int passes, hipStream_t st) {
  if (!cascade_tile_fits(dtype, C, grade, passes)) return MAVG_ERR_UNSUPPORTED;
  return cascade_switch(dtype, C, (int)MAVG_ERR_UNSUPPORTED, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    using A = typename I::A;
    if (!cs.unit) return launch_cascade_tile<T, A, I::C, 1, 4>(cs, grade, passes, st);
    if constexpr (kCascadeU<T> != 2) {
      const size_t Hu = tile_halo_units<I::F>(passes * (grade - 1));
      if (CascadeLds<T, A, I::C, I::F, kCascadeU<T>, kWG>(Hu).bytes <= lds_budget(kWG))
        return launch_cascade_tile<T, A, I::C, I::F, kCascadeU<T>>(cs, grade, passes, st);
    }
    return launch_cascade_tile<T, A, I::C, I::F, 2>(cs, grade, passes, st);
  });
}

}  // namespace mavg
