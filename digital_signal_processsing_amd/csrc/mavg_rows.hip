// mavg_rows.hip -- the batched rows scan: its instances (fp32 and int16, one
// and two channels, the 16-B-unit form and the frame-unit form) and their launch.
#include "mavg_launch.hpp"
#include "mavg_rows.hpp"

namespace mavg {

namespace {

constexpr int kRowsNt = kNtSplit | kNtHalo | kNtStore;  // the tile scan's split policy

template <typename T, typename A, int C, int F, int U, int WG = kWG>
size_t rows_lds_bytes(long long keff) {
  constexpr int VE = F * C;
  constexpr int NSEG = U * (WG / 64);
  const size_t hu = (size_t)((keff + F - 1) / F);
  const size_t stage = (((hu + (size_t)U * WG + 1) * VE * sizeof(T)) + 15) & ~(size_t)15;
  return stage + (size_t)(NSEG + WG / 64) * C * sizeof(A) + (size_t)NSEG * sizeof(int32_t);
}

// DV: the int16 output division, the magic multiply as in the tile scan (grade <= 65535 here)
template <typename T, typename A, int C, int F, int U, int WG = kWG, int DV = (sizeof(T) == 2 ? 1 : 0)>
int launch_rows_scan(const RowsSig& rs, int grade, hipStream_t st, int xcd_remap = kRemapGroup) {
  constexpr int TF = WG * F * U;
  constexpr int VE = F * C;
  const long long L = (long long)rs.row_frames;
  const long long nframes = (long long)rs.rows * L;
  const long long keff = std::min<long long>(grade, L);
  const size_t lds = rows_lds_bytes<T, A, C, F, U, WG>(keff);
  if (lds > lds_budget(WG)) return MAVG_ERR_UNSUPPORTED;
  RowsParams p{};
  p.in = rs.in;
  p.out = rs.out;
  p.nframes = nframes;
  p.row_frames = L;
  p.ntiles = (nframes + TF - 1) / TF;
  p.k = (int)keff;
  p.halo_units = (int)((keff + F - 1) / F);
  p.xk_off = (int)((VE - (keff * C) % VE) % VE);
  p.xcd_remap = xcd_remap;
  p.eio = rs.eio;
  p.o = make_out_params(grade);
  if (grid_too_large(p.ntiles, WG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "rows_scan<%s,acc=%s,C=%d,F=%d,U=%d,nt=%d,dv=%d> rows=%zu row_frames=%zu window=%lld grid=%lld block=%d "
             "lds=%zu tile_frames=%d remap=%d",
             type_name<T>(), type_name<A>(), C, F, U, kRowsNt, DV, rs.rows, rs.row_frames, keff, p.ntiles, WG, lds, TF,
             xcd_remap);
    return MAVG_OK;
  }
  hipLaunchKernelGGL((rows_scan_kernel<T, A, C, F, U, WG, kRowsNt, DV>), dim3((unsigned)p.ntiles), dim3(WG), lds, st, p);
  return hipGetLastError() == hipSuccess ? MAVG_OK : MAVG_ERR_HIP;
}

// Tile shapes: 8-KiB tiles for fp32 (U = 2 units per lane), 16-KiB tiles for int16 (U = 4), as
// the tile scan's dispatch at these halos; the frame-unit form takes 1024-frame tiles (U = 4),
// whose stage is never larger than the unit form's.
template <typename T, typename A, int C>
int rows_scan_c(const RowsSig& rs, int grade, hipStream_t st) {
  constexpr int F = 16 / (C * (int)sizeof(T));
  constexpr int U = sizeof(T) == 2 ? 4 : 2;
  if (!rs.unit) return launch_rows_scan<T, A, C, 1, 4>(rs, grade, st);
  return launch_rows_scan<T, A, C, F, U>(rs, grade, st);
}

// The halos the rows scan takes: up to kRowsMaxHaloBytes, where the single-signal dispatch
// itself leaves the LDS-staged tiles for the look-ahead scans (dispatch_scan_f: fp32 and int16
// mono / stereo halos past 16 KiB), and inside the LDS budget in both forms (always, at that
// size: the check launch_tile_scan makes).
constexpr long long kRowsMaxHaloBytes = 16384;
template <typename T, typename A, int C>
bool rows_fits_c(long long keff) {
  constexpr int F = 16 / (C * (int)sizeof(T));
  constexpr int U = sizeof(T) == 2 ? 4 : 2;
  if (keff * C * (long long)sizeof(T) > kRowsMaxHaloBytes) return false;
  return rows_lds_bytes<T, A, C, F, U>(keff) <= lds_budget(kWG) && rows_lds_bytes<T, A, C, 1, 4>(keff) <= lds_budget(kWG);
}

}  // namespace

bool rows_scan_fits(int dtype, int C, size_t row_frames, int grade) {
  const long long keff = (long long)std::min<size_t>((size_t)grade, row_frames);
  if (dtype == MAVG_F32) return C == 1 ? rows_fits_c<float, double, 1>(keff) : C == 2 ? rows_fits_c<float, double, 2>(keff) : false;
  return C == 1 ? rows_fits_c<int16_t, int32_t, 1>(keff) : C == 2 ? rows_fits_c<int16_t, int32_t, 2>(keff) : false;
}

int rows_scan_any(int dtype, int C, const RowsSig& rs, int grade, hipStream_t st) {
  if (C != 1 && C != 2) return MAVG_ERR_UNSUPPORTED;
  if (dtype == MAVG_F32)
    return C == 1 ? rows_scan_c<float, double, 1>(rs, grade, st) : rows_scan_c<float, double, 2>(rs, grade, st);
  if (grade > 65535) return MAVG_ERR_UNSUPPORTED;  // int32 sums and the exact-division helpers' domain
  return C == 1 ? rows_scan_c<int16_t, int32_t, 1>(rs, grade, st) : rows_scan_c<int16_t, int32_t, 2>(rs, grade, st);
}

}  // namespace mavg
