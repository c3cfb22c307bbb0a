// mavg_segscan.hip -- the segmented tile scan's instances (the rows scan and the ragged scan:
// fp32 and int16, one and two channels, the 16-B-unit form and the frame-unit form) and their
// launch.
#include "mavg_launch.hpp"
#include "mavg_segscan.hpp"

namespace mavg {

namespace {

constexpr int kSegNt = kNtSplit | kNtHalo | kNtStore;  // the tile scan's split policy

// What a row source adds to the launch: its parameter fields, the row length that bounds the
// effective window, and the head of its plan string.
struct RowsLaunch {
  using Src = DenseRows;
  using Sig = RowsSig;
  template <typename T, typename A, int C, int F, int U, int WG, int DV>
  static constexpr auto kernel = &rows_scan_kernel<T, A, C, F, U, WG, kSegNt, DV>;
  static constexpr const char* name = "rows_scan";
  static size_t nframes(const Sig& rs) { return rs.rows * rs.row_frames; }
  static size_t row_len(const Sig& rs) { return rs.row_frames; }
  static void fill(RowsParams& p, const Sig& rs) { p.row_frames = (long long)rs.row_frames; }
  static void shape(char* b, size_t n, const Sig& rs) {
    snprintf(b, n, "rows=%zu row_frames=%zu", rs.rows, rs.row_frames);
  }
};
struct RaggedLaunch {
  using Src = RaggedRows;
  using Sig = RaggedSig;
  template <typename T, typename A, int C, int F, int U, int WG, int DV>
  static constexpr auto kernel = &ragged_scan_kernel<T, A, C, F, U, WG, kSegNt, DV>;
  static constexpr const char* name = "ragged_scan";
  static size_t nframes(const Sig& rs) { return rs.nframes; }
  static size_t row_len(const Sig& rs) { return rs.max_row_frames; }
  static void fill(RaggedParams& p, const Sig& rs) {
    p.offsets = reinterpret_cast<const long long*>(rs.d_offsets);
    p.rows = (long long)rs.rows;
  }
  static void shape(char* b, size_t n, const Sig& rs) {
    snprintf(b, n, "rows=%zu frames=%zu max_row_frames=%zu", rs.rows, rs.nframes, rs.max_row_frames);
  }
};

// DV: the int16 output division, the magic multiply as in the tile scan (grade <= 65535 here)
template <typename L, typename T, typename A, int C, int F, int U, int WG = kWG, int DV = (sizeof(T) == 2 ? 1 : 0)>
int launch_seg_scan(const typename L::Sig& rs, int grade, hipStream_t st, int xcd_remap = kRemapGroup) {
  constexpr int TF = WG * F * U;
  constexpr int VE = F * C;
  const long long nframes = (long long)L::nframes(rs);
  const long long keff = std::min<long long>(grade, (long long)L::row_len(rs));
  const size_t lds = SegLds<typename L::Src, T, A, C, F, U, WG>((size_t)((keff + F - 1) / F)).bytes;
  if (lds > lds_budget(WG)) return MAVG_ERR_UNSUPPORTED;
  typename L::Src::Params p{};
  p.in = rs.in;
  p.out = rs.out;
  p.nframes = nframes;
  p.ntiles = (nframes + TF - 1) / TF;
  p.k = (int)keff;
  p.halo_units = (int)((keff + F - 1) / F);
  p.xk_off = (int)((VE - (keff * C) % VE) % VE);
  p.xcd_remap = xcd_remap;
  p.eio = rs.eio;
  p.o = make_out_params(grade);
  L::fill(p, rs);
  if (grid_too_large(p.ntiles, WG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    char shape[96];
    L::shape(shape, sizeof(shape), rs);
    snprintf(g_plan->text, sizeof(g_plan->text),
             "%s<%s,acc=%s,C=%d,F=%d,U=%d,nt=%d,dv=%d> %s window=%lld grid=%lld block=%d lds=%zu tile_frames=%d remap=%d",
             L::name, type_name<T>(), type_name<A>(), C, F, U, kSegNt, DV, shape, keff, p.ntiles, WG, lds, TF, xcd_remap);
    return MAVG_OK;
  }
  hipLaunchKernelGGL((L::template kernel<T, A, C, F, U, WG, DV>), dim3((unsigned)p.ntiles), dim3(WG), lds, st, p);
  return hipGetLastError() == hipSuccess ? MAVG_OK : MAVG_ERR_HIP;
}

// Tile shapes: 8-KiB tiles for fp32 (U = 2 units per lane), 16-KiB tiles for int16 (U = 4), as
// the tile scan's dispatch at these halos; the frame-unit form takes 1024-frame tiles (U = 4),
// whose stage is never larger than the unit form's.
template <typename T>
constexpr int kSegU = sizeof(T) == 2 ? 4 : 2;

// The halos the segmented scan takes: up to kSegMaxHaloBytes, where the single-signal dispatch
// itself leaves the LDS-staged tiles for the look-ahead scans (dispatch_scan_f: fp32 and int16
// mono / stereo halos past 16 KiB), and inside the LDS budget in both forms.
constexpr long long kSegMaxHaloBytes = 16384;
// The instances: one switch over dtype and channel count; fn takes the instance as a tag.
template <typename T_, typename A_, int C_>
struct SegInst {
  using T = T_;
  using A = A_;
  static constexpr int C = C_;
  static constexpr int F = 16 / (C * (int)sizeof(T));  // frames per 16-B unit
};
template <typename R, typename Fn>
R seg_switch(int dtype, int C, R none, Fn fn) {
  if (dtype == MAVG_F32) return C == 1 ? fn(SegInst<float, double, 1>{}) : C == 2 ? fn(SegInst<float, double, 2>{}) : none;
  return C == 1 ? fn(SegInst<int16_t, int32_t, 1>{}) : C == 2 ? fn(SegInst<int16_t, int32_t, 2>{}) : none;
}

template <typename Src>
bool seg_fits(int dtype, int C, size_t row_len, int grade) {
  const long long keff = (long long)std::min<size_t>((size_t)grade, row_len);
  return seg_switch(dtype, C, false, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    using A = typename I::A;
    if (keff * I::C * (long long)sizeof(T) > kSegMaxHaloBytes) return false;
    return SegLds<Src, T, A, I::C, I::F, kSegU<T>, kWG>((size_t)((keff + I::F - 1) / I::F)).bytes <= lds_budget(kWG) &&
           SegLds<Src, T, A, I::C, 1, 4, kWG>((size_t)keff).bytes <= lds_budget(kWG);
  });
}

template <typename L>
int seg_scan_any(int dtype, int C, const typename L::Sig& rs, int grade, hipStream_t st) {
  if (dtype != MAVG_F32 && grade > 65535) return MAVG_ERR_UNSUPPORTED;  // int32 sums and the exact-division helpers' domain
  return seg_switch(dtype, C, (int)MAVG_ERR_UNSUPPORTED, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    using A = typename I::A;
    if (!rs.unit) return launch_seg_scan<L, T, A, I::C, 1, 4>(rs, grade, st);
    return launch_seg_scan<L, T, A, I::C, I::F, kSegU<T>>(rs, grade, st);
  });
}

}  // namespace

bool rows_scan_fits(int dtype, int C, size_t row_frames, int grade) {
  return seg_fits<DenseRows>(dtype, C, row_frames, grade);
}
int rows_scan_any(int dtype, int C, const RowsSig& rs, int grade, hipStream_t st) {
  return seg_scan_any<RowsLaunch>(dtype, C, rs, grade, st);
}
bool ragged_scan_fits(int dtype, int C, size_t max_row_frames, int grade) {
  return seg_fits<RaggedRows>(dtype, C, max_row_frames, grade);
}
int ragged_scan_any(int dtype, int C, const RaggedSig& rs, int grade, hipStream_t st) {
  return seg_scan_any<RaggedLaunch>(dtype, C, rs, grade, st);
}

}  // namespace mavg
