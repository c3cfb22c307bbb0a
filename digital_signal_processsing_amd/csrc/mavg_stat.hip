// mavg_stat.hip -- the moving second moment's instances (fp32 and int16, one and two channels,
// the 16-B-unit form and the frame-unit form, S2 alone and S1 + S2; the strip kernel per dtype)
// and their launch.
#include "mavg_launch.hpp"
#include "mavg_stat.hpp"

namespace mavg {

namespace {

constexpr int kStatNt = kNtSplit | kNtHalo | kNtStore;  // the tile scan's split policy
// Tile shapes: the decimated scan's and the cascade's -- 8-KiB tiles for fp32 (U = 2), 16-KiB tiles
// for int16 (U = 4); the frame-unit form takes 1024-frame tiles (F = 1, U = 4).
template <typename T>
constexpr int kStatU = sizeof(T) == 2 ? 4 : 2;
// The halos grade * C * sample size the tile kernel takes, and the dispatch rule gives it:
// tile_scan's and rows_scan's 16 KiB.  Measured against the strip forced on the same shapes at halos of
// 256 B, 2, 8 and 16 KiB (tools/bench_stat.py --pairs, DESIGN.md "Moments"): 4.7x and more faster everywhere.
constexpr long long kStatMaxHaloBytes = 16384;

StatOut make_stat_out(int k, int stat, bool i16) {
  StatOut o{};
  o.inv_k = 1.0 / (double)k;
  o.inv_k2 = 1.0 / ((double)k * (double)k);
  o.k = k;
  o.stat = stat;
  o.exact = i16 && k <= 65535 ? 1 : 0;
  o.direct = !i16 && k <= kStatDirectMax ? 1 : 0;
  return o;
}

// RC (rebuild the in-lane prefix from the stage after the barrier) for int16, whose 16-KiB tiles
// would keep 32 - 96 more VGPRs live (measured slower or no faster); fp32 keeps its 8 - 16 fp64
// prefixes per moment in registers (measured 6 - 11 % faster than RC; DESIGN.md "Moments").
template <typename T>
constexpr bool kStatRC = sizeof(T) == 2;

template <typename T, int C, int F, int U, int M, int WG = kWG>
int launch_stat_tile(const StatSig& ss, int k, int stat, hipStream_t st, int xcd_remap = kRemapGroup) {
  constexpr int TF = WG * F * U;
  constexpr int VE = F * C;
  const size_t Hu = tile_halo_units<F>(k);
  const size_t lds = StatLds<T, C, F, U, WG>(Hu).bytes;
  if (lds > lds_budget(WG)) return MAVG_ERR_UNSUPPORTED;
  StatParams p{};
  p.in = ss.in;
  p.out = ss.out;
  p.mean = ss.mean;
  p.hist = ss.hist;
  p.nframes = (long long)ss.nframes;
  p.ntiles = (p.nframes + TF - 1) / TF;
  p.k = k;
  p.halo_units = (int)Hu;
  p.xk_off = (int)((VE - ((long long)k * C) % VE) % VE);
  p.xcd_remap = xcd_remap;
  p.eio = ss.eio;
  p.o = make_stat_out(k, stat, sizeof(T) == 2);
  if (grid_too_large(p.ntiles, WG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "stat_tile<%s,acc=%s/%s,C=%d,F=%d,U=%d,M=%d,rc=%d,nt=%d> stat=%d mean=%d frames=%lld halo_frames=%d grid=%lld "
             "block=%d lds=%zu tile_frames=%d remap=%d%s",
             type_name<T>(), type_name<typename StatAcc<T>::A1>(), type_name<typename StatAcc<T>::A2>(), C, F, U, M,
             kStatRC<T> ? 1 : 0, kStatNt, stat, ss.mean != nullptr ? 1 : 0, p.nframes, k, p.ntiles, WG, lds, TF, xcd_remap,
             p.o.direct ? " direct" : "");
    return MAVG_OK;
  }
  return launch_kernel<&stat_tile_kernel<T, C, F, U, M, kStatRC<T>, WG, kStatNt>>(p.ntiles, WG, lds, lds_budget(WG), st, p);
}

template <typename T_, int C_>
struct StatInst {
  using T = T_;
  static constexpr int C = C_;
  static constexpr int F = 16 / (C * (int)sizeof(T));  // frames per 16-B unit
};
template <typename R, typename Fn>
R stat_switch(int dtype, int C, R none, Fn fn) {
  if (dtype == MAVG_F32) return C == 1 ? fn(StatInst<float, 1>{}) : C == 2 ? fn(StatInst<float, 2>{}) : none;
  return C == 1 ? fn(StatInst<int16_t, 1>{}) : C == 2 ? fn(StatInst<int16_t, 2>{}) : none;
}

template <typename T>
int launch_stat_strip(int C, const StatSig& ss, int k, int stat, hipStream_t st) {
  StripParams p{};
  p.in = ss.in;
  p.out = ss.out;
  p.mean = ss.mean;
  p.hist = ss.hist;
  p.nframes = (long long)ss.nframes;
  p.C = C;
  p.k = k;
  p.L = stat_strip_frames(k);
  p.nstrips = (p.nframes + p.L - 1) / p.L;
  p.o = make_stat_out(k, stat, sizeof(T) == 2);
  if (p.nstrips > 0x7fffffffffffffffLL / C) return MAVG_ERR_UNSUPPORTED;
  const long long groups = (p.nstrips * C + kWG - 1) / kWG;
  if (grid_too_large(groups, kWG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "stat_strip dtype=%s acc=%s C=%d stat=%d mean=%d frames=%lld grade=%d L=%d strips=%lld grid=%lld block=%d%s",
             type_name<T>(), sizeof(T) == 2 ? "i64" : "f64", C, stat, ss.mean != nullptr ? 1 : 0, p.nframes, k, p.L,
             p.nstrips, groups, kWG, p.o.direct ? " direct" : "");
    return MAVG_OK;
  }
  return launch_kernel<&stat_strip_kernel<T, kWG>>(groups, kWG, 0, lds_budget(kWG), st, p);
}

}  // namespace

// The strip length for a window: a quarter of it, so that the direct sum over the k frames before
// a strip costs about four reads per output; at least 16 frames (short windows: reads stay near
// three per output), at most 2048 (an fp32 slide adds at most 4096 fp64 terms, and a long signal
// still makes thousands of threads).
int stat_strip_frames(int grade) { return std::min(std::max(grade / 4, 16), 2048); }

bool stat_tile_fits(int dtype, int C, int grade) {
  if (grade < 2) return false;
  if (dtype != MAVG_F32 && grade > 65535) return false;  // int32 S1, and N = k S2 - S1^2 exact in int64
  return stat_switch(dtype, C, false, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    if ((long long)grade * I::C * (long long)sizeof(T) > kStatMaxHaloBytes) return false;
    return StatLds<T, I::C, I::F, kStatU<T>, kWG>(tile_halo_units<I::F>(grade)).bytes <= lds_budget(kWG) &&
           StatLds<T, I::C, 1, 4, kWG>(tile_halo_units<1>(grade)).bytes <= lds_budget(kWG);
  });
}

int stat_tile_any(int dtype, int C, const StatSig& ss, int grade, int stat, hipStream_t st) {
  if (!stat_tile_fits(dtype, C, grade)) return MAVG_ERR_UNSUPPORTED;
  const bool two = (stat & 2) != 0 || ss.mean != nullptr;  // S1 + S2
  return stat_switch(dtype, C, (int)MAVG_ERR_UNSUPPORTED, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    if (!ss.unit)
      return two ? launch_stat_tile<T, I::C, 1, 4, 2>(ss, grade, stat, st) : launch_stat_tile<T, I::C, 1, 4, 1>(ss, grade, stat, st);
    return two ? launch_stat_tile<T, I::C, I::F, kStatU<T>, 2>(ss, grade, stat, st)
               : launch_stat_tile<T, I::C, I::F, kStatU<T>, 1>(ss, grade, stat, st);
  });
}

int stat_strip_any(int dtype, int C, const StatSig& ss, int grade, int stat, hipStream_t st) {
  return dtype == MAVG_F32 ? launch_stat_strip<float>(C, ss, grade, stat, st)
                           : launch_stat_strip<int16_t>(C, ss, grade, stat, st);
}

}  // namespace mavg
