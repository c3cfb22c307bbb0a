// mavg_biquad.hip -- the biquad's instances (fp32 and int16, one and two channels, the 16-B-unit
// form and the frame-unit form, for the tile kernel and the chain's two ends; the strip kernels per
// dtype; the carry kernel), their launchers, the powers of A, the halo length and the fit check.
#include "mavg_launch.hpp"
#include "mavg_biquad.hpp"

#include <cstring>

namespace mavg {

namespace {

constexpr int kBiquadNt = kNtSplit | kNtHalo | kNtStore;  // the tile kernel: the tile scan's split policy
constexpr int kBiquadNtAgg = 0;                           // chain step A: plain loads (step C re-reads them)
constexpr int kBiquadNtApply = kNtLoad | kNtStore;        // chain step C: streamed once from here on
// Tile shapes: the EMA's -- 8-KiB tiles for fp32 (U = 2), 16-KiB tiles for int16 (U = 4); the
// frame-unit form takes 1024-frame tiles (F = 1, U = 4).
template <typename T>
constexpr int kBiquadU = sizeof(T) == 2 ? 4 : 2;
constexpr int kBiquadFrameU = 4;
constexpr int kBiquadFrameTF = kWG * kBiquadFrameU;  // the smaller tile: what the workspace is sized for
// The halos H * C * sample size the tile kernel takes, and the dispatch rule gives it: the stage
// limit of every tile kernel here.  Measured against the chain forced on the same shapes at halos of
// 256 B, 2, 8 and 16 KiB (tools/bench_biquad.py --pairs, DESIGN.md "Biquad"): 1.09x (int16 mono at
// 16 KiB) to 2.14x faster everywhere, so the starting boundary ships.
constexpr long long kBiquadMaxHaloBytes = 16384;
// The strip form's frames per thread.
constexpr int kBiquadStripFrames = 64;

// ---- powers of A = [[-a1, 1], [-a2, 0]] ------------------------------------------------------
// Binary powers and products in the host's long double (a 64-bit significand on x86-64), rounded
// once to fp64 per entry.  The entries of A^m cancel like 1 / theta for poles at angle theta near
// +-1: squaring in fp64 loses that factor at every level (DESIGN.md "Biquad"), 11 extra bits keep
// every entry the kernels use at fp64 rounding over the promised domain.
struct MatL {
  long double a, b, c, d;
};
MatL matl_mul(const MatL& p, const MatL& q) {
  return MatL{p.a * q.a + p.b * q.c, p.a * q.b + p.b * q.d, p.c * q.a + p.d * q.c, p.c * q.b + p.d * q.d};
}
MatL matl_pow(const double coef[5], unsigned long long m) {
  MatL r{1.0L, 0.0L, 0.0L, 1.0L};
  MatL s{-(long double)coef[3], 1.0L, -(long double)coef[4], 0.0L};
  for (; m != 0; m >>= 1) {
    if (m & 1) r = matl_mul(r, s);
    if (m > 1) s = matl_mul(s, s);
  }
  return r;
}
Mat2 matl_round(const MatL& p) { return Mat2{(double)p.a, (double)p.b, (double)p.c, (double)p.d}; }
Mat2 mat_pow(const double coef[5], unsigned long long m) { return matl_round(matl_pow(coef, m)); }
// Q^1 .. Q^N of the base Q = A^m into *t; returns Q^N unrounded
template <int N>
MatL fill_level(const double coef[5], unsigned long long m, MatPow<N>* t) {
  const MatL q = matl_pow(coef, m);
  MatL p = q;
  for (int j = 0; j < N; ++j) {
    t->p[j] = matl_round(p);
    if (j < N - 1) p = matl_mul(p, q);
  }
  return p;  // Q^N in long double
}

long long biquad_state_frames(const double coef[5]);  // (below, beside the halo length)

BiquadCoef make_coef(const double coef[5]) { return BiquadCoef{coef[0], coef[1], coef[2], coef[3], coef[4]}; }
int state_bits(const BiquadSig& bs) { return (bs.state_in != nullptr ? 1 : 0) | (bs.state_out != nullptr ? 2 : 0); }

template <typename T, int C, int F, int U, int WG = kWG>
BiquadParams make_biquad_params(const BiquadSig& bs, int halo_frames, bool tile) {
  constexpr int TF = WG * F * U;
  BiquadParams p{};
  p.in = bs.in;
  p.out = bs.out;
  p.state_in = bs.state_in;
  p.state_out = bs.state_out;
  p.nframes = (long long)bs.nframes;
  p.ntiles = (p.nframes + TF - 1) / TF;
  p.k = make_coef(bs.coef);
  p.halo_frames = halo_frames;
  p.halo_units = (int)tile_halo_units<F>(halo_frames);
  p.halo_run = (p.halo_units * F + WG - 1) / WG;
  p.xcd_remap = kRemapGroup;
  p.eio = bs.eio;
  if (g_plan) return p;  // the powers are not part of a plan
  // (the chain takes the state through step B)
  if (tile && p.state_in != nullptr)
    p.state_frames = (int)std::min<long long>(biquad_state_frames(bs.coef), (long long)kBiquadStateTiles * TF);
  fill_level(bs.coef, (unsigned long long)F, &p.unit);
  fill_level(bs.coef, 64ULL * F, &p.seg);
  if (p.halo_run > 0) {
    const MatL q16 = fill_level(bs.coef, (unsigned long long)p.halo_run, &p.run);
    const MatL q32 = matl_mul(q16, q16);
    p.run_half = matl_round(q32);
    p.run_wave = matl_round(matl_mul(q32, q32));
  }
  if (p.state_in != nullptr && p.state_frames > 0)
    for (int j = 0; j < kBiquadStateTiles; ++j) p.tile_pow[j] = mat_pow(bs.coef, (unsigned long long)j * TF);
  return p;
}

template <typename T, int C, int F, int U, int WG = kWG>
int launch_biquad_tile(const BiquadSig& bs, hipStream_t st) {
  constexpr int TF = WG * F * U;
  const long long H = bs.halo;
  if (H * C * (long long)sizeof(T) > kBiquadMaxHaloBytes) return MAVG_ERR_UNSUPPORTED;
  const BiquadParams p = make_biquad_params<T, C, F, U, WG>(bs, (int)H, true);  // (H == 0: no halo units, no runs)
  const size_t lds = BiquadLds<T, C, F, U, WG>((size_t)p.halo_units).bytes;
  if (lds > lds_budget(WG) || grid_too_large(p.ntiles, WG)) return MAVG_ERR_UNSUPPORTED;
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "biquad_tile<%s,C=%d,F=%d,U=%d,nt=%d> halo_frames=%lld state=%d frames=%lld grid=%lld block=%d lds=%zu "
             "tile_frames=%d remap=%d b=%.6g,%.6g,%.6g a=%.9g,%.9g",
             type_name<T>(), C, F, U, kBiquadNt, H, state_bits(bs), p.nframes, p.ntiles, WG, lds, TF, p.xcd_remap,
             bs.coef[0], bs.coef[1], bs.coef[2], bs.coef[3], bs.coef[4]);
    return MAVG_OK;
  }
  return launch_kernel<&biquad_tile_kernel<T, C, F, U, WG, kBiquadNt>>(p.ntiles, WG, lds, lds_budget(WG), st, p);
}

// step B's parameters for `records` spans of `span` frames each, the last of `last_frames`
BiquadCarryParams make_carry_params(const BiquadSig& bs, int C, double* rec, long long records, int span,
                                    long long last_frames) {
  BiquadCarryParams q{};
  q.rec = rec;
  q.state_in = bs.state_in;
  q.state_out = bs.state_out;
  q.records = records;
  q.C = C;
  q.D = mat_pow(bs.coef, (unsigned long long)span);
  fill_level(bs.coef, (unsigned long long)span * kBiquadCarryRun, &q.lanes);
  q.wave = mat_pow(bs.coef, (unsigned long long)span * kBiquadCarryRun * 64ULL);
  q.d_last = mat_pow(bs.coef, (unsigned long long)last_frames);
  return q;
}

int launch_biquad_carry(const BiquadCarryParams& q, hipStream_t st) {
  hipLaunchKernelGGL(biquad_carry_kernel<kWG>, dim3(1), dim3(kWG), 0, st, q);
  return hipGetLastError() == hipSuccess ? MAVG_OK : MAVG_ERR_HIP;
}

// the caller's workspace against `need` bytes of records
int check_records(size_t need, Workspace ws) {
  if (ws.ptr == nullptr || ws.bytes < need) return MAVG_ERR_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(ws.ptr) & 15u) != 0) return MAVG_ERR_MISALIGNED;
  return MAVG_OK;
}

template <typename T, int C, int F, int U, int WG = kWG>
int launch_biquad_chain(const BiquadSig& bs, Workspace ws, hipStream_t st) {
  constexpr int TF = WG * F * U;
  BiquadParams p = make_biquad_params<T, C, F, U, WG>(bs, 0, false);  // no halo
  p.state_out = nullptr;  // step B writes it
  const size_t lds = BiquadLds<T, C, F, U, WG>(0).bytes;
  if (lds > lds_budget(WG) || grid_too_large(p.ntiles, WG)) return MAVG_ERR_UNSUPPORTED;
  const size_t need = (size_t)p.ntiles * C * 2 * sizeof(double);
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "biquad_chain<%s,C=%d,F=%d,U=%d,nt=%d> halo_frames=%lld state=%d frames=%lld grid=%lld block=%d lds=%zu "
             "tile_frames=%d records=%lld carry_chunk=%d launches=3 b=%.6g,%.6g,%.6g a=%.9g,%.9g",
             type_name<T>(), C, F, U, kBiquadNtApply, bs.halo, state_bits(bs), p.nframes, p.ntiles, WG, lds, TF, p.ntiles,
             kBiquadCarryChunk, bs.coef[0], bs.coef[1], bs.coef[2], bs.coef[3], bs.coef[4]);
    g_plan->ws_bytes = need;
    return MAVG_OK;
  }
  int s = check_records(need, ws);
  if (s != MAVG_OK) return s;
  p.rec = static_cast<double*>(ws.ptr);
  const BiquadCarryParams q =
      make_carry_params(bs, C, p.rec, p.ntiles, TF, p.nframes - (p.ntiles - 1) * (long long)TF);
  s = launch_kernel<&biquad_agg_kernel<T, C, F, U, WG, kBiquadNtAgg>>(p.ntiles, WG, lds, lds_budget(WG), st, p);
  if (s != MAVG_OK) return s;
  s = launch_biquad_carry(q, st);
  if (s != MAVG_OK) return s;
  return launch_kernel<&biquad_apply_kernel<T, C, F, U, WG, kBiquadNtApply>>(p.ntiles, WG, lds, lds_budget(WG), st, p);
}

template <typename T>
int launch_biquad_strip(int C, const BiquadSig& bs, Workspace ws, hipStream_t st) {
  BiquadStripParams p{};
  p.in = bs.in;
  p.out = bs.out;
  p.nframes = (long long)bs.nframes;
  p.L = kBiquadStripFrames;
  p.nstrips = (p.nframes + p.L - 1) / p.L;
  p.k = make_coef(bs.coef);
  p.C = C;
  if (p.nstrips > 0x7fffffffffffffffLL / 32 / C) return MAVG_ERR_UNSUPPORTED;
  const long long groups = (p.nstrips * C + kWG - 1) / kWG;
  if (grid_too_large(groups, kWG)) return MAVG_ERR_UNSUPPORTED;
  const size_t need = (size_t)p.nstrips * C * 2 * sizeof(double);
  if (g_plan) {
    snprintf(g_plan->text, sizeof(g_plan->text),
             "biquad_strip dtype=%s C=%d L=%d strips=%lld carry_chunk=%d launches=3 halo_frames=%lld state=%d frames=%lld "
             "grid=%lld block=%d b=%.6g,%.6g,%.6g a=%.9g,%.9g",
             type_name<T>(), C, p.L, p.nstrips, kBiquadCarryChunk, bs.halo, state_bits(bs), p.nframes, groups, kWG,
             bs.coef[0], bs.coef[1], bs.coef[2], bs.coef[3], bs.coef[4]);
    g_plan->ws_bytes = need;
    return MAVG_OK;
  }
  int s = check_records(need, ws);
  if (s != MAVG_OK) return s;
  p.rec = static_cast<double*>(ws.ptr);
  const BiquadCarryParams q =
      make_carry_params(bs, C, p.rec, p.nstrips, p.L, p.nframes - (p.nstrips - 1) * (long long)p.L);
  s = launch_kernel<&biquad_strip_kernel<T, false, kWG>>(groups, kWG, 0, lds_budget(kWG), st, p);
  if (s != MAVG_OK) return s;
  s = launch_biquad_carry(q, st);
  if (s != MAVG_OK) return s;
  return launch_kernel<&biquad_strip_kernel<T, true, kWG>>(groups, kWG, 0, lds_budget(kWG), st, p);
}

template <typename T_, int C_>
struct BiquadInst {
  using T = T_;
  static constexpr int C = C_;
  static constexpr int F = 16 / (C * (int)sizeof(T));  // frames per 16-B unit
};
template <typename R, typename Fn>
R biquad_switch(int dtype, int C, R none, Fn fn) {
  if (dtype == MAVG_F32) return C == 1 ? fn(BiquadInst<float, 1>{}) : C == 2 ? fn(BiquadInst<float, 2>{}) : none;
  return C == 1 ? fn(BiquadInst<int16_t, 1>{}) : C == 2 ? fn(BiquadInst<int16_t, 2>{}) : none;
}

int records_bytes(size_t nframes, size_t span, int C, size_t* bytes) {
  const size_t records = nframes / span + (nframes % span != 0 ? 1 : 0);
  if (records > (SIZE_MAX / 16 - 2) / (size_t)C) return MAVG_ERR_UNSUPPORTED;
  *bytes = records * (size_t)C * 2 * sizeof(double);
  return MAVG_OK;
}

// ---- the halo length -------------------------------------------------------------------------
constexpr long long kHaloSaturated = 1LL << 62;  // poles too close to the circle for a bound in fp64
constexpr long long kHaloRefine = 16384;         // envelopes up to here are refined by iteration
constexpr int kHaloBlock = 128;

// Upper bounds of sum_{n > N} |h[n]| from the poles.  With u_m = sum_j p1^j p2^(m-1-j) (|u_m| <= m
// rho^(m-1)) the impulse response is h[n] = c1 u_n + c2 u_(n-1) for n >= 1, c1 = b1 - a1 b0, c2 =
// b2 - a2 b0.  Every pole pair: |h[n]| <= |c1| n rho^(n-1) + |c2| (n-1) rho^(n-2).  Complex poles r
// e^(+-i theta): |u_m| <= r^m / |Im p|, so |h[n]| <= E r^n with E = (|c1| + |c2| / r) / |Im p|.
struct HaloEnvelope {
  double c1, c2, rho, E;  // rho rounded up; E = 0: real poles, the first bound only
  // sum_{m >= N} m rho^(m-1), N >= 1
  double S(double N) const {
    const double g = 1.0 - rho;
    return N * std::pow(rho, N - 1.0) / g + std::pow(rho, N) / (g * g);
  }
  double tail(double N) const {
    double t = c1 * S(N + 1.0) + c2 * S(N < 1.0 ? 1.0 : N);
    if (E > 0.0) t = std::min(t, E * std::pow(rho, N + 1.0) / (1.0 - rho));
    return t * (1.0 + 0x1p-30);
  }
  // the smallest N >= 0 with tail(N) <= thr (tail is a sum of non-negative terms past N: monotone)
  long long first_below(double thr) const {
    if (tail(0.0) <= thr) return 0;
    long long hi = 1;
    while (tail((double)hi) > thr) {
      if (hi >= kHaloSaturated) return kHaloSaturated;
      hi *= 2;
    }
    long long lo = hi / 2;  // tail(lo) > thr, or lo == 0
    while (hi - lo > 1) {
      const long long mid = lo + (hi - lo) / 2;
      if (tail((double)mid) <= thr) hi = mid; else lo = mid;
    }
    return hi;
  }
};

constexpr double kHaloEps = 0x1p-50;  // the rounding taken off or added to every bound below
// a lower bound of G = sum |h[n]|: |b0| = |h[0]|, |h[1]|, and the gains at DC and at Nyquist
double gain_lower_bound(const double coef[5]) {
  const double b0 = coef[0], b1 = coef[1], b2 = coef[2], a1 = coef[3], a2 = coef[4];
  const double eps = kHaloEps;
  const double bsum = std::fabs(b0) + std::fabs(b1) + std::fabs(b2);
  double glb = std::fabs(b0);
  glb = std::max(glb, (std::fabs(b0 + b1 + b2) - eps * bsum) / ((1.0 + a1 + a2) * (1.0 + eps)));
  glb = std::max(glb, (std::fabs(b0 - b1 + b2) - eps * bsum) / ((1.0 - a1 + a2) * (1.0 + eps)));
  return std::max(glb, std::fabs(b1 - a1 * b0) * (1.0 - eps));
}
// the envelope of c1 u_n + c2 u_(n-1) for these poles; false: rho is 1 to within the rounding
bool pole_envelope(const double coef[5], double c1, double c2, HaloEnvelope* env) {
  const double a1 = coef[3], a2 = coef[4];
  const double eps = kHaloEps;
  *env = HaloEnvelope{c1 * (1.0 + eps), c2 * (1.0 + eps), 0.0, 0.0};
  const double disc = a1 * a1 - 4.0 * a2;
  if (disc < 0.0) {
    env->rho = std::sqrt(a2);
    const double im = 0.5 * std::sqrt(-disc) * (1.0 - eps);
    if (im > 0.0 && env->rho > 0.0) env->E = (env->c1 + env->c2 / (env->rho * (1.0 - eps))) / im;
  } else {
    env->rho = 0.5 * (std::fabs(a1) + std::sqrt(disc));
  }
  env->rho *= 1.0 + eps;
  return env->rho < 1.0 - 0x1p-48;
}
// Frames after which a state_in of magnitude M moves an output by at most 2^-30 G M: the first row
// of A^n is (u_(n+1), u_n), so the envelope with c1 = c2 = 1 one frame on bounds it (its tail sum
// bounds every later term).  An arbitrary state decays with the poles, not with the zeros.
long long biquad_state_frames(const double coef[5]) {
  if (coef[3] == 0.0 && coef[4] == 0.0) return 2;  // A^2 = 0
  HaloEnvelope env{};
  if (!pole_envelope(coef, 1.0, 1.0, &env)) return kHaloSaturated;
  const long long n = env.first_below(0x1p-30 * gain_lower_bound(coef));
  return n >= kHaloSaturated ? n : n + 1;
}

}  // namespace

// How H is formed (include/mavg.h "Halo"): G is bounded below by max(|b0|, |H(1)|, |H(-1)|) (each
// is at most sum |h|; the two gains with their rounding taken off).  N30 is the first N at which the
// pole envelope's tail is at most 2^-30 of that: past kHaloRefine frames it is H.  Otherwise the
// envelope is taken down to 2^-32 at N32 and the impulse response is iterated in fp64 up to N32: H
// is the first frame count with sum_{H < n <= N32} |h[n]| <= 2^-31 of the bound, which leaves 2^-32
// for the rounding of the iteration (an allowance, not a derived bound: include/mavg.h says so).
static long long halo_frames_of(const double coef[5]) {
  const double b0 = coef[0], b1 = coef[1], b2 = coef[2], a1 = coef[3], a2 = coef[4];
  const double c1 = b1 - a1 * b0, c2 = b2 - a2 * b0;
  if (c1 == 0.0 && c2 == 0.0) return 0;  // h[n] = 0 for n >= 1
  const double glb = gain_lower_bound(coef);
  HaloEnvelope env{};
  if (!pole_envelope(coef, std::fabs(c1), std::fabs(c2), &env)) return kHaloSaturated;
  const long long n30 = env.first_below(0x1p-30 * glb);
  if (n30 > kHaloRefine) return n30;
  const long long n32 = env.first_below(0x1p-32 * glb);
  const double thr = 0x1p-31 * glb;
  // pass 1: |h| summed over blocks of kHaloBlock frames; frame n is in block (n - 1) / kHaloBlock
  constexpr int kMaxBlocks = (int)(4 * kHaloRefine / kHaloBlock);
  double blk[kMaxBlocks];
  if (n32 > (long long)kMaxBlocks * kHaloBlock) return n30;  // (the envelope decays slower than 4x its 2^-30 point)
  const int nblk = (int)((n32 + kHaloBlock - 1) / kHaloBlock);
  double s1 = c1, s2 = c2;
  for (int j = 0; j < nblk; ++j) {
    double acc = 0.0;
    for (long long n = (long long)j * kHaloBlock + 1; n <= std::min<long long>(n32, (long long)(j + 1) * kHaloBlock); ++n) {
      acc += std::fabs(s1);
      const double t = fma(-a1, s1, s2);
      s2 = -a2 * s1;
      s1 = t;
    }
    blk[j] = acc;
  }
  // the block in which the sum from the far end first passes thr
  double after = 0.0;
  int jc = nblk - 1;
  for (; jc >= 0 && after + blk[jc] <= thr; --jc) after += blk[jc];
  if (jc < 0) return 0;
  // pass 2: that block's frames
  double val[kHaloBlock];
  const long long first = (long long)jc * kHaloBlock + 1, last = std::min<long long>(n32, first + kHaloBlock - 1);
  s1 = c1, s2 = c2;
  for (long long n = 1; n <= last; ++n) {
    if (n >= first) val[n - first] = std::fabs(s1);
    const double t = fma(-a1, s1, s2);
    s2 = -a2 * s1;
    s1 = t;
  }
  for (long long n = last; n >= first; --n) {
    if (after + val[n - first] > thr) return n;
    after += val[n - first];
  }
  return first - 1;
}

// One call asks for H several times (the workspace query, the plan, the run) and the refinement
// costs up to about 2 N32 host steps: the last coefficients' H is kept per thread.
long long biquad_halo_frames(const double coef[5]) {
  struct Last {
    double coef[5];
    long long halo;
    bool valid;
  };
  static thread_local Last last{};
  if (last.valid && std::memcmp(last.coef, coef, sizeof(last.coef)) == 0) return last.halo;
  const long long halo = halo_frames_of(coef);
  std::memcpy(last.coef, coef, sizeof(last.coef));
  last.halo = halo;
  last.valid = true;
  return halo;
}

bool biquad_tile_fits(int dtype, int C, long long H) {
  return biquad_switch(dtype, C, false, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    if (H > kBiquadMaxHaloBytes || H * I::C * (long long)sizeof(T) > kBiquadMaxHaloBytes) return false;
    return BiquadLds<T, I::C, I::F, kBiquadU<T>, kWG>(tile_halo_units<I::F>((int)H)).bytes <= lds_budget(kWG) &&
           BiquadLds<T, I::C, 1, kBiquadFrameU, kWG>(tile_halo_units<1>((int)H)).bytes <= lds_budget(kWG);
  });
}

int biquad_tile_any(int dtype, int C, const BiquadSig& bs, hipStream_t st) {
  if (!biquad_tile_fits(dtype, C, bs.halo)) return MAVG_ERR_UNSUPPORTED;
  return biquad_switch(dtype, C, (int)MAVG_ERR_UNSUPPORTED, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    if (!bs.unit) return launch_biquad_tile<T, I::C, 1, kBiquadFrameU>(bs, st);
    return launch_biquad_tile<T, I::C, I::F, kBiquadU<T>>(bs, st);
  });
}

int biquad_chain_any(int dtype, int C, const BiquadSig& bs, Workspace ws, hipStream_t st) {
  return biquad_switch(dtype, C, (int)MAVG_ERR_UNSUPPORTED, [&](auto i) {
    using I = decltype(i);
    using T = typename I::T;
    if (!bs.unit) return launch_biquad_chain<T, I::C, 1, kBiquadFrameU>(bs, ws, st);
    return launch_biquad_chain<T, I::C, I::F, kBiquadU<T>>(bs, ws, st);
  });
}

int biquad_strip_any(int dtype, int C, const BiquadSig& bs, Workspace ws, hipStream_t st) {
  return dtype == MAVG_F32 ? launch_biquad_strip<float>(C, bs, ws, st) : launch_biquad_strip<int16_t>(C, bs, ws, st);
}

// the fused cascade's tables (mavg_sos.hip) take their powers and state horizon from here
Mat2 biquad_mat_pow(const double coef[5], unsigned long long m) { return mat_pow(coef, m); }
void biquad_fill_pow63(const double coef[5], unsigned long long m, MatPow<63>* t) { fill_level(coef, m, t); }
long long biquad_state_horizon(const double coef[5]) { return biquad_state_frames(coef); }

int biquad_chain_ws_bytes(size_t nframes, int C, size_t* bytes) { return records_bytes(nframes, kBiquadFrameTF, C, bytes); }
int biquad_strip_ws_bytes(size_t nframes, int C, size_t* bytes) { return records_bytes(nframes, kBiquadStripFrames, C, bytes); }

}  // namespace mavg
