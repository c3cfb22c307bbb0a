// mavg_sos.hpp -- the fused second-order-sections cascade (mavg_sos_run, path sos_tile): S biquads
// in series inside one LDS-staged tile, the signal read and written once, the intermediate between
// sections fp64 in LDS, one rounding to fp32 at the end.
//   stage       the tile's TF frames and the Hp frames before them (Hp = sum of the sections' halos
//               H_j, rounded up to 8 frames; zeros before frame 0 and past the end) as fp64
//   ranges      section j runs over stage frames [start_j, Hp + TF) from a zero state, start_0 = 0,
//               start_(j+1) = start_j + H_j (section 0 also takes the rounding): its first H_j outputs
//               lack the frames before start_j and are never read -- section j + 1 starts past them,
//               the outputs start at Hp.  In place: y_j[f] overwrites y_(j-1)[f].
//   one section thread tid owns the `run` consecutive frames from start + tid * run (run odd: the
//               8-B and 16-B LDS accesses of a wave are then conflict-free, DESIGN.md "SOS"): the
//               recurrence from a zero state gives the run's aggregate, wave_mat_scan (base A^run)
//               the lane's exclusive value, the wave totals go through LDS (weights A^(64 run w)),
//               and the recurrence runs again from the lane's carry, y written over x.
//   frame 0     a range that would start before frame 0 starts at frame 0 from state_in[j] exactly
//               (tile 0: every section).  In a later tile the state enters section j as A^g state_in[j],
//               g the range's first frame, while g < state_frames (tile_pow, as biquad_tile_kernel).
//   tables      every weight is one host-formed, once-rounded power of the section's A (SosSection,
//               2.7 KB a section): they live in the workspace, written by sos_setup_kernel from its
//               kernel arguments, one launch per section in front of the filtering launch.
#pragma once

#include "mavg_biquad.hpp"

namespace mavg {

constexpr int kSosMaxSections = 16;    // sections of one fused launch
constexpr int kSosStateTiles = 16;     // tiles after the first a state_in can enter (tile_pow)
constexpr int kSosTileSamples = 4096;  // samples of a tile: 4096 frames mono, 2048 stereo (32 KiB of fp64)
constexpr long long kSosMaxHaloBytes = 16384;  // sum H_j * C * 8 B: the stage limit of every tile kernel here

struct SosSection {
  BiquadCoef k;
  int start;         // first stage frame of the section's range
  int run;           // frames per thread (odd)
  int state_frames;  // the state enters ranges that start before this frame
  int pad_;
  MatPow<63> lanes;  // base A^run: the lanes of a wave
  Mat2 wave[4];      // A^(64 run w), w = 1 .. 4: the waves of the workgroup
  Mat2 tile_pow[kSosStateTiles];  // A^(t TF - Hp + start), t = 1 .. 16: the state enters tile t
};
static_assert(sizeof(SosSection) % 8 == 0 && sizeof(SosSection) + 8 <= 4096, "one section's tables are one launch's arguments");

struct SosSetupParams {
  unsigned long long w[sizeof(SosSection) / 8];
  unsigned long long* dst;
};

// one section's tables from the kernel arguments to the workspace (plain per-thread stores)
template <int WG = kWG>
__global__ __launch_bounds__(WG) void sos_setup_kernel(SosSetupParams p) {
  constexpr int N = (int)(sizeof(SosSection) / 8);
  for (int i = threadIdx.x; i < N; i += WG) p.dst[i] = p.w[i];
}

struct SosParams {
  const void* in;
  float* out;
  const double* state_in;  // [S][C][2] or NULL: zeros
  double* state_out;       // [S][C][2] or NULL
  const SosSection* sec;   // [S], in the workspace
  long long nframes;
  long long ntiles;
  int sections;
  int halo;                // Hp
  int xcd_remap;           // remap_tile mode
  int eio;                 // frame-unit launch on an element-aligned input (UnitIO::gload)
};

// The dynamic LDS of one workgroup, as byte offsets: the fp64 stage (halo, tile), the [NW][C][2]
// wave totals.  Read by the kernel, the launcher and the fit check; the same in both unit forms.
template <int C, int WG = kWG>
struct SosLds {
  static constexpr int NW = WG / 64;
  static constexpr int TF = kSosTileSamples / C;
  size_t stage_frames;  // halo + tile
  size_t tot, bytes;
  __host__ __device__ constexpr explicit SosLds(size_t halo)
      : stage_frames(halo + (size_t)TF),
        tot(stage_frames * C * sizeof(double)),
        bytes(tot + (size_t)NW * C * 2 * sizeof(double)) {}
};

template <int C>
struct alignas(8 * C) SosFrame {
  double e[C];
};

// halo and tile -> registers -> the fp64 stage: thread tid takes units tid, tid + WG, ...; units
// inside the signal move as one access (non-temporal where no later tile's halo re-reads them),
// the others as guarded elements (zeros outside).
template <typename T, int C, int F, int WG>
__device__ __forceinline__ void sos_stage(const SosParams& p, double* stage, long long t0) {
  constexpr int VE = F * C;
  constexpr int TF = kSosTileSamples / C;
  using IO = UnitIO<T, VE>;
  using U_t = Unit<T, VE>;
  const T* __restrict__ in = static_cast<const T*>(p.in);
  const int Hp = p.halo;
  const int units = (Hp + TF) / F;
  const long long h0 = t0 - Hp;  // first staged frame
  const long long nframes = p.nframes;
  const bool eio = F == 1 && p.eio != 0;
#pragma unroll 4
  for (int j = (int)threadIdx.x; j < units; j += WG) {
    const long long f = h0 + (long long)j * F;
    U_t x;
    if (f >= 0 && f + F <= nframes) {
      if (j * F >= Hp && j * F + F <= TF) x = IO::template gload<true>(in + f * C, eio);
      else x = IO::template gload<false>(in + f * C, eio);
    } else {
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
#pragma unroll
        for (int c = 0; c < C; ++c) x.e[fr * C + c] = load_elem<T>(in, nullptr, f + fr, c, C, nframes, 1, 0);
    }
#pragma unroll
    for (int fr = 0; fr < F; ++fr) {
      SosFrame<C> d;
#pragma unroll
      for (int c = 0; c < C; ++c) d.e[c] = (double)x.e[fr * C + c];
      *reinterpret_cast<SosFrame<C>*>(stage + (size_t)(j * F + fr) * C) = d;
    }
  }
}

// ----------------------------------------------------------------------------
// sos_tile_kernel.  Barriers: (0) after the stage is written; per section (1) after the wave
// totals are written and before any wave reads them, (2) after the section's outputs are written.
// Between (1) and (2) a thread reads and writes only its own run (x[f] is in a register before
// y[f] replaces it), and reads the totals; the next section's runs are cut differently and its
// totals are rewritten, both after (2).  The output step reads the stage after the last (2).
// Tile-local indices are int; frame and sample indices are 64-bit.
// ----------------------------------------------------------------------------
template <typename T, int C, int F, int WG = kWG>
__global__ __launch_bounds__(WG) void sos_tile_kernel(SosParams p) {
  constexpr int NW = WG / 64;
  constexpr int TF = kSosTileSamples / C;
  using Lds = SosLds<C, WG>;
  using Frame = SosFrame<C>;
  static_assert(NW <= 4, "SosSection::wave");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Hp = p.halo;
  const Lds lds((size_t)Hp);
  double* const stage = reinterpret_cast<double*>(smem);
  double* const tot = reinterpret_cast<double*>(smem + lds.tot);
  const int SF = Hp + TF;
  MAVG_DCHECK(lds.bytes <= lds_budget(WG) && Hp % 8 == 0 && Hp < TF, "sos LDS layout", lds.bytes, Hp);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wu = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long tile = remap_tile(blockIdx.x, gridDim.x, p.xcd_remap);
  const long long t0 = tile * TF;
  MAVG_DCHECK(tile >= 0 && tile < p.ntiles && t0 < p.nframes, "sos tile index", tile, p.ntiles);
  const bool tile_full = (t0 + TF <= p.nframes);
  sos_stage<T, C, F, WG>(p, stage, t0);
  __syncthreads();  // (0)

  const int z = t0 < (long long)Hp ? (int)((long long)Hp - t0) : 0;  // stage index of frame 0, where staged
  const long long last = p.nframes - 1 - (t0 - Hp);                  // stage index of the last frame
  const int last_i = last < (long long)SF ? (int)last : -1;          // (only its tile holds it)
  for (int j = 0; j < p.sections; ++j) {
    const SosSection* __restrict__ sc = p.sec + j;
    const BiquadCoef k = sc->k;
    const int L = sc->run;
    const int r = sc->start > z ? sc->start : z;
    const long long g = t0 - Hp + r;  // the range's first frame
    // ---- the state at the range's start (wave-uniform) ----
    Vec2 s0[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s0[c] = Vec2{0.0, 0.0};
    if (p.state_in != nullptr && g < (long long)sc->state_frames) {
      Mat2 ds{1.0, 0.0, 0.0, 1.0};
      if (g > 0) {
        MAVG_DCHECK(tile >= 1 && tile <= kSosStateTiles, "sos state tile", tile, sc->state_frames);
        ds = sc->tile_pow[tile - 1];
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const Vec2 si{p.state_in[((size_t)j * C + c) * 2], p.state_in[((size_t)j * C + c) * 2 + 1]};
        s0[c] = g > 0 ? mat_fma(ds, si, Vec2{0.0, 0.0}) : si;
      }
    }
    // ---- the run's aggregate from a zero state; the wave's scan ----
    const int a = r + tid * L;
    int n = SF - a;
    n = n < 0 ? 0 : (n > L ? L : n);
    MAVG_DCHECK(a >= 0 && r + WG * L >= SF, "sos run", a, L);
    Vec2 cy[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cy[c] = Vec2{0.0, 0.0};
    for (int i = 0; i < n; ++i) {
      const Frame x = *reinterpret_cast<const Frame*>(stage + (size_t)(a + i) * C);
#pragma unroll
      for (int c = 0; c < C; ++c) k.step(cy[c], x.e[c]);
    }
    {
      const MatLane ll(sc->lanes, lane);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const Vec2 inc = ll.scan(cy[c]);
        cy[c] = vec_excl(inc, lane);
        const Vec2 t = vec_readlane(inc, 63);
        if (lane == 0) {
          tot[(wu * C + c) * 2] = t.x;
          tot[(wu * C + c) * 2 + 1] = t.y;
        }
      }
    }
    __syncthreads();  // (1)
    // ---- the lane's carry: the waves before this one and the start state, then this wave's lanes ----
    {
      const Mat2 lane_pow = sc->lanes.at0(lane);  // A^(run lane)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        Vec2 cw = s0[c];
        if (wu > 0) {
          cw = mat_fma(sc->wave[wu - 1], s0[c], Vec2{0.0, 0.0});
          for (int i = 0; i < wu; ++i) {
            const Vec2 ti{tot[(i * C + c) * 2], tot[(i * C + c) * 2 + 1]};
            const int e = wu - 1 - i;
            if (e == 0) cw = Vec2{cw.x + ti.x, cw.y + ti.y};
            else cw = mat_fma(sc->wave[e - 1], ti, cw);
          }
        }
        cy[c] = mat_fma(lane_pow, cw, cy[c]);
      }
    }
    // ---- the run again from its carry, y over x; the state after the last frame ----
    double* const so = p.state_out;
    for (int i = 0; i < n; ++i) {
      Frame* const q = reinterpret_cast<Frame*>(stage + (size_t)(a + i) * C);
      const Frame x = *q;
      Frame y;
#pragma unroll
      for (int c = 0; c < C; ++c) y.e[c] = k.step(cy[c], x.e[c]);
      *q = y;
      if (a + i == last_i && so != nullptr) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          so[((size_t)j * C + c) * 2] = cy[c].x;
          so[((size_t)j * C + c) * 2 + 1] = cy[c].y;
        }
      }
    }
    __syncthreads();  // (2)
  }

  // ---- output: the last section's frames from Hp on, rounded once ----
  constexpr int FO = F == 1 ? 1 : 4 / C;  // frames per 16 B of output
  constexpr int VO = FO * C;
  using OIO = UnitIO<float, VO>;
  float* __restrict__ out = p.out;
#pragma unroll 2
  for (int u = tid; u < TF / FO; u += WG) {
    const long long f = t0 + (long long)u * FO;
    Unit<float, VO> yo;
#pragma unroll
    for (int fr = 0; fr < FO; ++fr) {
      const Frame y = *reinterpret_cast<const Frame*>(stage + (size_t)(Hp + u * FO + fr) * C);
#pragma unroll
      for (int c = 0; c < C; ++c) yo.e[fr * C + c] = (float)y.e[c];
    }
    if (F > 1 && tile_full) {
      MAVG_DCHECK(f >= 0 && f + FO <= p.nframes, "sos output index", f, p.nframes);
      OIO::template store<true>(out + f * C, yo);
    } else {
#pragma unroll
      for (int fr = 0; fr < FO; ++fr)
        if (f + fr < p.nframes) {
          MAVG_DCHECK(f + fr >= 0, "sos output index", f + fr, p.nframes);
#pragma unroll
          for (int c = 0; c < C; ++c) out[(f + fr) * C + c] = yo.e[fr * C + c];
        }
    }
  }
}

// The powers of a section's A for the tables, formed as the biquad's (mavg_biquad.hip: binary
// powers in the host's long double, rounded once per entry), and the frames a state_in is carried.
Mat2 biquad_mat_pow(const double coef[5], unsigned long long m);
void biquad_fill_pow63(const double coef[5], unsigned long long m, MatPow<63>* t);
long long biquad_state_horizon(const double coef[5]);

}  // namespace mavg
