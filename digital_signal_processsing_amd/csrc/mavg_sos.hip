// mavg_sos.hip -- the fused cascade's instances (fp32 and int16, one and two channels, the 16-B-unit
// form and the frame-unit form), the set-up launches that carry the sections' tables to the
// workspace, the launcher and the fit check.
#include "mavg_launch.hpp"
#include "mavg_sos.hpp"

#include <cstring>

namespace mavg {

namespace {

// the staged halo: the sections' halos together, rounded up to whole 16-B input units of every dtype
long long sos_stage_halo(long long sum_halo) { return (sum_halo + 7) & ~7LL; }

int sos_state_bits(const SosSig& ss) { return (ss.state_in != nullptr ? 1 : 0) | (ss.state_out != nullptr ? 2 : 0); }

// section j's tables for a tile of TF frames behind a staged halo of Hp frames
SosSection make_section(const double coef[5], int start, int Hp, int TF, bool with_state) {
  SosSection s{};
  s.k = BiquadCoef{coef[0], coef[1], coef[2], coef[3], coef[4]};
  s.start = start;
  s.run = ((Hp + TF - start + kWG - 1) / kWG) | 1;  // odd
  biquad_fill_pow63(coef, (unsigned long long)s.run, &s.lanes);
  for (int w = 1; w <= 4; ++w) s.wave[w - 1] = biquad_mat_pow(coef, 64ULL * (unsigned long long)s.run * w);
  if (with_state) {
    s.state_frames = (int)std::min<long long>(biquad_state_horizon(coef), (long long)kSosStateTiles * TF);
    for (int t = 1; t <= kSosStateTiles; ++t) {
      const long long g = (long long)t * TF - Hp + start;
      if (g < s.state_frames) s.tile_pow[t - 1] = biquad_mat_pow(coef, (unsigned long long)g);
    }
  }
  return s;
}

template <typename T, int C, int F, int WG = kWG>
int launch_sos_tile(const SosSig& ss, Workspace ws, hipStream_t st) {
  constexpr int TF = kSosTileSamples / C;
  long long sum = 0;
  for (int j = 0; j < ss.sections; ++j) sum += ss.halo[j];
  if (ss.sections < 2 || ss.sections > kSosMaxSections || sum * C * 8 > kSosMaxHaloBytes) return MAVG_ERR_UNSUPPORTED;
  const int Hp = (int)sos_stage_halo(sum);
  SosParams p{};
  p.in = ss.in;
  p.out = ss.out;
  p.state_in = ss.state_in;
  p.state_out = ss.state_out;
  p.nframes = (long long)ss.nframes;
  p.ntiles = (p.nframes + TF - 1) / TF;
  p.sections = ss.sections;
  p.halo = Hp;
  p.xcd_remap = kRemapGroup;
  p.eio = ss.eio;
  const size_t lds = SosLds<C, WG>((size_t)Hp).bytes;
  if (lds > lds_budget(WG) || grid_too_large(p.ntiles, WG)) return MAVG_ERR_UNSUPPORTED;
  const size_t need = sos_tile_ws_bytes(ss.sections);
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "sos_tile<%s,C=%d,F=%d> sections=%d intermediate=f64 halo_frames=%lld stage_halo=%d state=%d frames=%lld "
             "grid=%lld block=%d lds=%zu tile_frames=%d remap=%d ws=%zu launches=%d",
             type_name<T>(), C, F, ss.sections, sum, Hp, sos_state_bits(ss), p.nframes, p.ntiles, WG, lds, TF, p.xcd_remap,
             need, 1 + ss.sections);
    g_plan->ws_bytes = need;
    return MAVG_OK;
  }
  if (ws.ptr == nullptr || ws.bytes < need) return MAVG_ERR_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(ws.ptr) & 15u) != 0) return MAVG_ERR_MISALIGNED;
  SosSection* const sec = static_cast<SosSection*>(ws.ptr);
  p.sec = sec;
  int start = 0;
  for (int j = 0; j < ss.sections; ++j) {
    const SosSection s = make_section(ss.coef + 5 * j, start, Hp, TF, ss.state_in != nullptr);
    SosSetupParams q;
    std::memcpy(q.w, &s, sizeof(s));
    q.dst = reinterpret_cast<unsigned long long*>(sec + j);
    hipLaunchKernelGGL(sos_setup_kernel<kWG>, dim3(1), dim3(kWG), 0, st, q);
    if (hipGetLastError() != hipSuccess) return MAVG_ERR_HIP;
    start += (int)ss.halo[j] + (j == 0 ? Hp - (int)sum : 0);  // (section 0 takes the rounding)
  }
  return launch_kernel<&sos_tile_kernel<T, C, F, WG>>(p.ntiles, WG, lds, lds_budget(WG), st, p);
}

}  // namespace

size_t sos_tile_ws_bytes(int sections) { return ((size_t)sections * sizeof(SosSection) + 15) & ~(size_t)15; }

bool sos_tile_fits(int C, int sections, long long sum_halo) {
  if (C < 1 || C > 2 || sections < 2 || sections > kSosMaxSections) return false;
  if (sum_halo < 0 || sum_halo > kSosMaxHaloBytes || sum_halo * C * 8 > kSosMaxHaloBytes) return false;
  const size_t Hp = (size_t)sos_stage_halo(sum_halo);
  return (C == 1 ? SosLds<1>(Hp).bytes : SosLds<2>(Hp).bytes) <= lds_budget(kWG);
}

int sos_tile_any(int dtype, int C, const SosSig& ss, Workspace ws, hipStream_t st) {
  long long sum = 0;
  for (int j = 0; j < ss.sections; ++j) {
    if (ss.halo[j] > kSosMaxHaloBytes) return MAVG_ERR_UNSUPPORTED;
    sum += ss.halo[j];
  }
  if (!sos_tile_fits(C, ss.sections, sum)) return MAVG_ERR_UNSUPPORTED;
  if (dtype == MAVG_F32) {
    if (C == 1) return ss.unit ? launch_sos_tile<float, 1, 4>(ss, ws, st) : launch_sos_tile<float, 1, 1>(ss, ws, st);
    return ss.unit ? launch_sos_tile<float, 2, 2>(ss, ws, st) : launch_sos_tile<float, 2, 1>(ss, ws, st);
  }
  if (C == 1) return ss.unit ? launch_sos_tile<int16_t, 1, 8>(ss, ws, st) : launch_sos_tile<int16_t, 1, 1>(ss, ws, st);
  return ss.unit ? launch_sos_tile<int16_t, 2, 4>(ss, ws, st) : launch_sos_tile<int16_t, 2, 1>(ss, ws, st);
}

}  // namespace mavg
