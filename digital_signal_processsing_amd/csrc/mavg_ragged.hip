// mavg_ragged.hip -- the ragged rows scan: its instances (fp32 and int16, one
// and two channels, the 16-B-unit form and the frame-unit form) and their launch.
#include "mavg_launch.hpp"
#include "mavg_ragged.hpp"

namespace mavg {

namespace {

constexpr int kRaggedNt = kNtSplit | kNtHalo | kNtStore;  // the tile scan's split policy

// the rows scan's LDS (stage, segment totals, halo sums, segment flags) plus the row-start
// bitmask over the staged frames and its summary words
template <typename T, typename A, int C, int F, int U, int WG = kWG>
size_t ragged_lds_bytes(long long keff) {
  constexpr int VE = F * C;
  constexpr int NSEG = U * (WG / 64);
  const size_t hu = (size_t)((keff + F - 1) / F);
  const size_t stage = (((hu + (size_t)U * WG + 1) * VE * sizeof(T)) + 15) & ~(size_t)15;
  const size_t nwords = (hu * F + (size_t)WG * F * U + 31) / 32 + 1;
  const size_t nsumm = (nwords + 31) / 32;
  return stage + (size_t)(NSEG + WG / 64) * C * sizeof(A) + (size_t)NSEG * sizeof(int32_t) + (nwords + nsumm) * 4;
}

// DV: the int16 output division, the magic multiply as in the tile scan (grade <= 65535 here)
template <typename T, typename A, int C, int F, int U, int WG = kWG, int DV = (sizeof(T) == 2 ? 1 : 0)>
int launch_ragged_scan(const RaggedSig& rs, int grade, hipStream_t st, int xcd_remap = kRemapGroup) {
  constexpr int TF = WG * F * U;
  constexpr int VE = F * C;
  const long long nframes = (long long)rs.nframes;
  const long long keff = std::min<long long>(grade, (long long)rs.max_row_frames);
  const size_t lds = ragged_lds_bytes<T, A, C, F, U, WG>(keff);
  if (lds > lds_budget(WG)) return MAVG_ERR_UNSUPPORTED;
  RaggedParams p{};
  p.in = rs.in;
  p.out = rs.out;
  p.offsets = reinterpret_cast<const long long*>(rs.d_offsets);
  p.rows = (long long)rs.rows;
  p.nframes = nframes;
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
             "ragged_scan<%s,acc=%s,C=%d,F=%d,U=%d,nt=%d,dv=%d> rows=%zu frames=%zu max_row_frames=%zu window=%lld "
             "grid=%lld block=%d lds=%zu tile_frames=%d remap=%d",
             type_name<T>(), type_name<A>(), C, F, U, kRaggedNt, DV, rs.rows, rs.nframes, rs.max_row_frames, keff,
             p.ntiles, WG, lds, TF, xcd_remap);
    return MAVG_OK;
  }
  hipLaunchKernelGGL((ragged_scan_kernel<T, A, C, F, U, WG, kRaggedNt, DV>), dim3((unsigned)p.ntiles), dim3(WG), lds, st,
                     p);
  return hipGetLastError() == hipSuccess ? MAVG_OK : MAVG_ERR_HIP;
}

// Tile shapes: the rows scan's (8-KiB tiles for fp32, U = 2; 16-KiB tiles for int16, U = 4;
// 1024-frame tiles in the frame-unit form).
template <typename T, typename A, int C>
int ragged_scan_c(const RaggedSig& rs, int grade, hipStream_t st) {
  constexpr int F = 16 / (C * (int)sizeof(T));
  constexpr int U = sizeof(T) == 2 ? 4 : 2;
  if (!rs.unit) return launch_ragged_scan<T, A, C, 1, 4>(rs, grade, st);
  return launch_ragged_scan<T, A, C, F, U>(rs, grade, st);
}

// The halos the ragged scan takes: the rows scan's limit (mavg_rows.hip kRowsMaxHaloBytes), for
// the same reasons -- the LDS stage in both forms, and int16 sums inside int32.
constexpr long long kRaggedMaxHaloBytes = 16384;
template <typename T, typename A, int C>
bool ragged_fits_c(long long keff) {
  constexpr int F = 16 / (C * (int)sizeof(T));
  constexpr int U = sizeof(T) == 2 ? 4 : 2;
  if (keff * C * (long long)sizeof(T) > kRaggedMaxHaloBytes) return false;
  return ragged_lds_bytes<T, A, C, F, U>(keff) <= lds_budget(kWG) &&
         ragged_lds_bytes<T, A, C, 1, 4>(keff) <= lds_budget(kWG);
}

}  // namespace

bool ragged_scan_fits(int dtype, int C, size_t max_row_frames, int grade) {
  const long long keff = (long long)std::min<size_t>((size_t)grade, max_row_frames);
  if (dtype == MAVG_F32)
    return C == 1 ? ragged_fits_c<float, double, 1>(keff) : C == 2 ? ragged_fits_c<float, double, 2>(keff) : false;
  return C == 1 ? ragged_fits_c<int16_t, int32_t, 1>(keff) : C == 2 ? ragged_fits_c<int16_t, int32_t, 2>(keff) : false;
}

int ragged_scan_any(int dtype, int C, const RaggedSig& rs, int grade, hipStream_t st) {
  if (C != 1 && C != 2) return MAVG_ERR_UNSUPPORTED;
  if (dtype == MAVG_F32)
    return C == 1 ? ragged_scan_c<float, double, 1>(rs, grade, st) : ragged_scan_c<float, double, 2>(rs, grade, st);
  if (grade > 65535) return MAVG_ERR_UNSUPPORTED;  // int32 sums and the exact-division helpers' domain
  return C == 1 ? ragged_scan_c<int16_t, int32_t, 1>(rs, grade, st) : ragged_scan_c<int16_t, int32_t, 2>(rs, grade, st);
}

}  // namespace mavg
