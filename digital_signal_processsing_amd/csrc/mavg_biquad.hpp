// mavg_biquad.hpp -- the biquad (mavg_biquad_run): y[f] = b0 x[f] + b1 x[f-1] + b2 x[f-2] - a1 y[f-1]
// - a2 y[f-2] per channel of an interleaved signal, evaluated in fp64, fp32 out.  The EMA's design
// (mavg_ema.hpp) with a 2-vector state and 2 x 2 powers in place of the scalar d:
//   state       transposed direct form II: y = b0 x + s1; s1' = b1 x - a1 y + s2; s2' = b2 x - a2 y,
//               that is s' = A s + B x with A = [[-a1, 1], [-a2, 0]]
//   composition over m frames s_out = A^m s_in + b: only the 2-vector b is scanned, and every
//               multiplier is a power of A the host forms in extended precision (BiquadParams)
//   biquad_tile_body / biquad_tile_kernel / biquad_agg_kernel / biquad_carry_kernel /
//   biquad_apply_kernel / biquad_strip_kernel   as their ema_ namesakes
#pragma once

#include "mavg_ema.hpp"

namespace mavg {

struct Mat2 {  // [[a, b], [c, d]]
  double a, b, c, d;
};
struct Vec2 {
  double x, y;
};

// acc + M v
__host__ __device__ __forceinline__ Vec2 mat_fma(const Mat2& m, const Vec2& v, const Vec2& acc) {
  return Vec2{fma(m.a, v.x, fma(m.b, v.y, acc.x)), fma(m.c, v.x, fma(m.d, v.y, acc.y))};
}
__host__ __device__ __forceinline__ Mat2 mat_mul(const Mat2& p, const Mat2& q) {
  return Mat2{fma(p.a, q.a, p.b * q.c), fma(p.a, q.b, p.b * q.d), fma(p.c, q.a, p.d * q.c), fma(p.c, q.b, p.d * q.d)};
}
__device__ __forceinline__ Mat2 mat_sel(bool take, const Mat2& p, const Mat2& q) {
  return Mat2{take ? p.a : q.a, take ? p.b : q.b, take ? p.c : q.c, take ? p.d : q.d};
}
__device__ __forceinline__ Vec2 vec_readlane(const Vec2& v, int l) { return Vec2{readlane(v.x, l), readlane(v.y, l)}; }
// the inclusive value of the lane before (0 in lane 0): a lane's exclusive carry
__device__ __forceinline__ Vec2 vec_excl(const Vec2& incl, int lane) {
  return Vec2{decay_excl(incl.x, lane), decay_excl(incl.y, lane)};
}

// wave_decay_scan (mavg_device.hpp) on a 2-vector: each of the six steps applies the 2 x 2 power of
// the level's base Q that spans the step's distance -- four fmas per step.  Lanes a step does not
// write receive zeros, so their fmas leave v as it is.
template <int CTRL, int RM>
__device__ __forceinline__ Vec2 mat_scan_step(const Mat2& q, const Vec2& v) {
  return mat_fma(q, Vec2{dpp<CTRL, RM, 0xf>(v.x), dpp<CTRL, RM, 0xf>(v.y)}, v);
}
__device__ __forceinline__ Vec2 wave_mat_scan(Vec2 v, const Mat2& q1, const Mat2& q2, const Mat2& q4, const Mat2& q8,
                                              const Mat2& w15, const Mat2& w31) {
  v = mat_scan_step<0x111, 0xf>(q1, v);
  v = mat_scan_step<0x112, 0xf>(q2, v);
  v = mat_scan_step<0x114, 0xf>(q4, v);
  v = mat_scan_step<0x118, 0xf>(q8, v);
  v = mat_scan_step<0x142, 0xa>(w15, v);
  v = mat_scan_step<0x143, 0xc>(w31, v);
  return v;
}

// Q^1 .. Q^N of one scan level's base Q, each formed on the host in extended precision and rounded
// once.  A lane's weights are table entries, never products of entries: a product of two rounded
// powers is not a rounded power, and with poles near +-1 it is wrong by the entries' cancellation
// (DESIGN.md "Biquad": 1e-8 G M from one fp64 product at the domain's edge, in the numpy model).
template <int N>
struct MatPow {
  Mat2 p[N];  // p[j] = Q^(j + 1)
  // Q^e, 1 <= e <= N (a lane-indexed read of the kernel argument segment)
  __device__ __forceinline__ Mat2 at(int e) const { return p[e - 1]; }
  // Q^e, 0 <= e <= N
  __device__ __forceinline__ Mat2 at0(int e) const { return mat_sel(e == 0, Mat2{1.0, 0.0, 0.0, 1.0}, p[e > 0 ? e - 1 : 0]); }
};
// the scan of one level: the uniform powers and this lane's two broadcast weights, w15 = Q^((lane &
// 15) + 1) and w31 = Q^((lane & 31) + 1) (a 16-entry table: only rows a w15 step reaches hold values)
struct MatLane {
  Mat2 q1, q2, q4, q8, w15, w31;
  template <int N>
  __device__ __forceinline__ MatLane(const MatPow<N>& t, int lane)
      : q1(t.p[0]), q2(t.p[1]), q4(t.p[3]), q8(t.p[7]), w15(t.at((lane & 15) + 1)),
        w31(N >= 32 ? t.at((lane & (N >= 32 ? 31 : 15)) + 1) : w15) {}
  __device__ __forceinline__ Vec2 scan(const Vec2& v) const { return wave_mat_scan(v, q1, q2, q4, q8, w15, w31); }
  // the first five steps: lane 31 ends with the scan of lanes 0 .. 31, lane 63 with that of 32 .. 63
  __device__ __forceinline__ Vec2 scan_halves(Vec2 v) const {
    v = mat_scan_step<0x111, 0xf>(q1, v);
    v = mat_scan_step<0x112, 0xf>(q2, v);
    v = mat_scan_step<0x114, 0xf>(q4, v);
    v = mat_scan_step<0x118, 0xf>(q8, v);
    return mat_scan_step<0x142, 0xa>(w15, v);
  }
};

// one frame of the transposed direct form II
struct BiquadCoef {
  double b0, b1, b2, a1, a2;
  __host__ __device__ __forceinline__ double step(Vec2& s, double x) const {
    const double y = fma(b0, x, s.x);
    s.x = fma(b1, x, fma(-a1, y, s.y));
    s.y = fma(b2, x, -a2 * y);
    return y;
  }
};

constexpr int kBiquadStateTiles = 16;  // tiles a state_in can enter (tile_pow)

struct BiquadParams {
  const void* in;
  float* out;
  const double* state_in;  // [C][2] or NULL: zeros
  double* state_out;       // [C][2] or NULL (the tile kernel; the chain's is written by biquad_carry_kernel)
  double* rec;             // chain: one record of two doubles per tile and channel
  long long nframes;
  long long ntiles;
  BiquadCoef k;
  MatPow<63> unit;         // base A^F: the lanes of a segment
  MatPow<16> seg;          // base A^(64 F): the segments of a tile
  MatPow<16> run;          // base A^halo_run: the lanes of the halo reduction
  Mat2 run_half;           // A^(32 halo_run): the two halves of a wave
  Mat2 run_wave;           // A^(64 halo_run): the waves of the halo reduction
  Mat2 tile_pow[kBiquadStateTiles];  // A^(j tile_frames): the state enters tile j
  int halo_frames;         // H
  int state_frames;        // the state enters tiles with t0 < state_frames (at most kBiquadStateTiles tiles)
  int halo_units;          // ceil(H / F): units staged before the tile (0: chain)
  int halo_run;            // frames per thread of the halo reduction: ceil(halo_units F / WG)
  int xcd_remap;           // remap_tile mode
  int eio;                 // frame-unit launch on an element-aligned input (UnitIO::gload)
};

static_assert(sizeof(BiquadParams) <= 4096, "a kernel's arguments take at most 4 KiB");

// The dynamic LDS of one workgroup, as byte offsets: the stage of x (halo, tile), the [NSEG][C][2]
// segment totals, the [NW][C][2] halo partials.  Read by the kernels, the launcher and the fit check.
template <typename T, int C, int F, int U, int WG>
struct BiquadLds {
  static constexpr int NW = WG / 64;
  static constexpr int NSEG = U * NW;
  static constexpr int TF = WG * F * U;
  size_t stage_units;  // halo + tile
  size_t tot, hsum, bytes;
  __host__ __device__ constexpr explicit BiquadLds(size_t halo_units)
      : stage_units(halo_units + (size_t)U * WG),
        tot(((stage_units * F * C * sizeof(T)) + 15) & ~(size_t)15),
        hsum(tot + (size_t)NSEG * C * 2 * sizeof(double)),
        bytes(hsum + (size_t)NW * C * 2 * sizeof(double)) {}
};

// ----------------------------------------------------------------------------
// biquad_tile_body: ema_tile_body's four steps on a 2-vector per channel.
//   lane step     the recurrence over each of the lane's units from a zero state: the unit's aggregate
//   wave step     wave_mat_scan (base A^F) over the 64 aggregates of a segment; the lane's exclusive
//                 value by a lane shift; the segment's total to LDS
//   segment step  after the barrier every wave scans the NSEG totals (base A^(64 F)); the tile's
//                 carry-in Y (carry_in(), read after the barrier) enters segment s as A^(64 F s) Y
//   output step   the recurrence again from the lane's carry; OUT: (float)y stored, 16-B stores for
//                 whole tiles.  The thread that owns frame rec_frame writes the state after it to
//                 rec[c][0 .. 1] (fp64).
// ----------------------------------------------------------------------------
template <typename T, int C, int F, int U, int WG, bool OUT, int NT, typename CarryIn>
__device__ __forceinline__ void biquad_tile_body(const BiquadParams& p, const T* tile, double* tot, CarryIn&& carry_in,
                                                 long long t0, bool tile_full, double* rec, long long rec_frame) {
  constexpr int NW = WG / 64;
  constexpr int VE = F * C;
  constexpr int NSEG = U * NW;
  using IO = UnitIO<T, VE>;
  using OIO = UnitIO<float, VE>;
  using U_t = Unit<T, VE>;
  using O_t = Unit<float, VE>;
  static_assert(NSEG <= 16, "segment totals are scanned across one row of a wave");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const BiquadCoef k = p.k;

  // ---- lane step and wave step ----
  Vec2 cy[U][C];  // the lane's carry: first its exclusive value inside the segment
  {
    const MatLane ul(p.unit, lane);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const U_t xu = IO::load(tile + (u * WG + tid) * VE);
      Vec2 r[C];
#pragma unroll
      for (int c = 0; c < C; ++c) r[c] = Vec2{0.0, 0.0};
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
#pragma unroll
        for (int c = 0; c < C; ++c) k.step(r[c], (double)xu.e[fr * C + c]);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const Vec2 inc = ul.scan(r[c]);
        cy[u][c] = vec_excl(inc, lane);
        const Vec2 t = vec_readlane(inc, 63);
        if (lane == 0) {
          tot[((u * NW + w) * C + c) * 2] = t.x;
          tot[((u * NW + w) * C + c) * 2 + 1] = t.y;
        }
      }
    }
  }
  __syncthreads();

  // ---- segment step ----
  {
    Vec2 Y[C];
    carry_in(Y);
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const MatLane sl(p.seg, lane);
    const Mat2 seg_pow = p.seg.at0(lane & 15);  // A^(64 F lane), lanes 0 .. 15
    const Mat2 unit_pow = p.unit.at0(lane);     // A^(F lane)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      Vec2 tv{0.0, 0.0};
      if (lane < NSEG) tv = Vec2{tot[(lane * C + c) * 2], tot[(lane * C + c) * 2 + 1]};
      const Vec2 cs = mat_fma(seg_pow, Y[c], vec_excl(sl.scan(tv), lane));  // carry into segment `lane`
#pragma unroll
      for (int u = 0; u < U; ++u) cy[u][c] = mat_fma(unit_pow, vec_readlane(cs, u * NW + wu), cy[u][c]);
    }
  }

  // ---- output step ----
  float* __restrict__ out = p.out;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = u * WG + tid;
    const long long f = t0 + (long long)j * F;
    const bool mine = rec != nullptr && rec_frame >= f && rec_frame < f + F;
    if (!OUT && !mine) continue;
    const U_t xu = IO::load(tile + j * VE);
    O_t yo;
    Vec2 s[C];
#pragma unroll
    for (int c = 0; c < C; ++c) s[c] = cy[u][c];
#pragma unroll
    for (int fr = 0; fr < F; ++fr)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        yo.e[fr * C + c] = (float)k.step(s[c], (double)xu.e[fr * C + c]);
        if (mine && f + fr == rec_frame) {
          rec[c * 2] = s[c].x;
          rec[c * 2 + 1] = s[c].y;
        }
      }
    if constexpr (OUT) {
      if (F > 1 && tile_full) {
        MAVG_DCHECK(f >= 0 && f + F <= p.nframes, "biquad output index", f, p.nframes);
        OIO::template store<(NT & kNtStore) != 0>(out + f * C, yo);
      } else {
#pragma unroll
        for (int fr = 0; fr < F; ++fr)
          if (f + fr < p.nframes) {
            MAVG_DCHECK(f + fr >= 0, "biquad output index", f + fr, p.nframes);
#pragma unroll
            for (int c = 0; c < C; ++c) out[(f + fr) * C + c] = yo.e[fr * C + c];
          }
      }
    }
  }
}

// ----------------------------------------------------------------------------
// biquad_tile_kernel: one launch, no workspace.  A tile stages its halo_frames frames of halo (a
// re-read of the previous tile's tail; zeros before frame 0) in front of its own and reduces them to
// its carry-in: thread tid runs the recurrence over halo_run contiguous frames from a zero state
// (the runs padded with zeros at the old end), the waves' matrix scans (base A^halo_run, its two
// halves joined by A^(32 halo_run)) and the wave totals (weights A^(64 halo_run)) combine them.  What the halo leaves out -- earlier frames,
// and from t0 >= halo_frames on the state -- is bounded by the impulse response's tail past
// halo_frames (mavg.h).  Tiles with t0 < state_frames add A^t0 state_in (wave-uniform; A^t0 from
// tile_pow): an arbitrary state decays with the poles alone, so its horizon is its own.  Frame and sample indices are 64-bit wherever they are not tile-local.
// ----------------------------------------------------------------------------
template <typename T, int C, int F, int U, int WG = kWG, int NT = kNtSplit | kNtHalo | kNtStore>
__global__ __launch_bounds__(WG) void biquad_tile_kernel(BiquadParams p) {
  constexpr int NW = WG / 64;
  constexpr int VE = F * C;
  constexpr int TF = WG * F * U;
  using Lds = BiquadLds<T, C, F, U, WG>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Hu = p.halo_units;
  const int Ha = Hu * F;
  const Lds lds((size_t)Hu);
  T* const stage = reinterpret_cast<T*>(smem);
  double* const tot = reinterpret_cast<double*>(smem + lds.tot);
  double* const hsum = reinterpret_cast<double*>(smem + lds.hsum);
  MAVG_DCHECK(lds.bytes <= lds_budget(WG) && Ha >= p.halo_frames && p.halo_run * WG >= Ha, "biquad LDS layout", lds.bytes, Hu);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const long long tile = remap_tile(blockIdx.x, gridDim.x, p.xcd_remap);
  const long long t0 = tile * TF;
  MAVG_DCHECK(tile >= 0 && tile < p.ntiles && t0 < p.nframes, "biquad tile index", tile, p.ntiles);
  const bool tile_full = (t0 + TF <= p.nframes);
  ema_stage<T, C, F, U, WG, NT>(p, stage, t0, tile_full);
  __syncthreads();

  // ---- halo reduction (its partials are read after the body's barrier) ----
  const int R = p.halo_run;
  if (R > 0) {
    const int pad = R * WG - Ha;  // zeros in front of the oldest staged frame
    Vec2 h[C];
#pragma unroll
    for (int c = 0; c < C; ++c) h[c] = Vec2{0.0, 0.0};
    for (int i = 0; i < R; ++i) {
      const int g = tid * R + i - pad;
      if (g < 0) continue;
      MAVG_DCHECK(g < Ha, "biquad halo stage index", g, Ha);
#pragma unroll
      for (int c = 0; c < C; ++c) p.k.step(h[c], (double)stage[g * C + c]);
    }
    const MatLane rl(p.run, lane);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const Vec2 hv = rl.scan_halves(h[c]);
      const Vec2 t = mat_fma(p.run_half, vec_readlane(hv, 31), vec_readlane(hv, 63));
      if (lane == 0) {
        hsum[(w * C + c) * 2] = t.x;
        hsum[(w * C + c) * 2 + 1] = t.y;
      }
    }
  }
  auto carry_in = [&](Vec2(&Y)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      Vec2 y{0.0, 0.0};
      if (R > 0) {
#pragma unroll
        for (int i = 0; i < NW; ++i) y = mat_fma(p.run_wave, y, Vec2{hsum[(i * C + c) * 2], hsum[(i * C + c) * 2 + 1]});
      }
      Y[c] = y;
    }
    if (p.state_in != nullptr && t0 < (long long)p.state_frames) {
      MAVG_DCHECK(tile < kBiquadStateTiles, "biquad state tile", tile, p.state_frames);
      Mat2 ds = p.tile_pow[0];  // A^t0
#pragma unroll
      for (int j = 1; j < kBiquadStateTiles; ++j) ds = mat_sel(tile == j, p.tile_pow[j], ds);
#pragma unroll
      for (int c = 0; c < C; ++c) Y[c] = mat_fma(ds, Vec2{p.state_in[c * 2], p.state_in[c * 2 + 1]}, Y[c]);
    }
  };
  biquad_tile_body<T, C, F, U, WG, true, NT>(p, stage + (size_t)Hu * VE, tot, carry_in, t0, tile_full, p.state_out,
                                             p.nframes - 1);
}

// chain step A: the tile's aggregate -- its state after its last frame for a zero carry-in -- to
// rec[tile] (plain loads: step C reads the same frames again; its own are non-temporal)
template <typename T, int C, int F, int U, int WG = kWG, int NT = 0>
__global__ __launch_bounds__(WG) void biquad_agg_kernel(BiquadParams p) {
  constexpr int TF = WG * F * U;
  using Lds = BiquadLds<T, C, F, U, WG>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds lds(0);
  T* const stage = reinterpret_cast<T*>(smem);
  double* const tot = reinterpret_cast<double*>(smem + lds.tot);
  const long long tile = remap_tile(blockIdx.x, gridDim.x, p.xcd_remap);
  const long long t0 = tile * TF;
  MAVG_DCHECK(p.halo_units == 0 && tile >= 0 && tile < p.ntiles && t0 < p.nframes, "biquad tile index", tile, p.ntiles);
  const bool tile_full = (t0 + TF <= p.nframes);
  ema_stage<T, C, F, U, WG, NT>(p, stage, t0, tile_full);
  __syncthreads();
  auto carry_in = [&](Vec2(&Y)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) Y[c] = Vec2{0.0, 0.0};
  };
  const long long last = tile_full ? t0 + TF - 1 : p.nframes - 1;
  biquad_tile_body<T, C, F, U, WG, false, NT>(p, stage, tot, carry_in, t0, tile_full, p.rec + tile * C * 2, last);
}

// chain step C: the tile body from the carry-in rec[tile], outputs stored
template <typename T, int C, int F, int U, int WG = kWG, int NT = kNtLoad | kNtStore>
__global__ __launch_bounds__(WG) void biquad_apply_kernel(BiquadParams p) {
  constexpr int TF = WG * F * U;
  using Lds = BiquadLds<T, C, F, U, WG>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds lds(0);
  T* const stage = reinterpret_cast<T*>(smem);
  double* const tot = reinterpret_cast<double*>(smem + lds.tot);
  const long long tile = remap_tile(blockIdx.x, gridDim.x, p.xcd_remap);
  const long long t0 = tile * TF;
  MAVG_DCHECK(p.halo_units == 0 && tile >= 0 && tile < p.ntiles && t0 < p.nframes, "biquad tile index", tile, p.ntiles);
  const bool tile_full = (t0 + TF <= p.nframes);
  ema_stage<T, C, F, U, WG, NT>(p, stage, t0, tile_full);
  __syncthreads();
  auto carry_in = [&](Vec2(&Y)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) Y[c] = Vec2{p.rec[(tile * C + c) * 2], p.rec[(tile * C + c) * 2 + 1]};
  };
  biquad_tile_body<T, C, F, U, WG, true, NT>(p, stage, tot, carry_in, t0, tile_full, nullptr, 0);
}

// ----------------------------------------------------------------------------
// biquad_carry_kernel (chain step B): ONE workgroup turns the `records` aggregates b_t of spans of
// `span` frames (tiles or strips; the last may be shorter) in place into carry-ins: Y[0] = state_in,
// Y[t+1] = D Y[t] + b_t with D = A^span, per channel, and writes d_state_out = A^last_frames
// Y[records-1] + b_last.  ema_carry_kernel with a shorter per-lane run (a record is two doubles):
// chunks of kBiquadCarryChunk records, lane tid takes kBiquadCarryRun contiguous records of the
// chunk, the waves' matrix scans (base D^kBiquadCarryRun) and the wave totals combine the lanes, and
// a running carry links the chunks.  Records past the end read as 0 and are not written.
// ----------------------------------------------------------------------------
constexpr int kBiquadCarryRun = 8;
constexpr int kBiquadCarryChunk = kBiquadCarryRun * kWG;  // 2048 records
struct BiquadCarryParams {
  double* rec;             // [records][C][2]
  const double* state_in;  // or NULL
  double* state_out;       // or NULL
  long long records;
  int C;
  Mat2 D;                  // A^span
  MatPow<63> lanes;        // base D^kBiquadCarryRun
  Mat2 wave;               // D^(64 kBiquadCarryRun)
  Mat2 d_last;             // A^(frames of the last span)
};

template <int WG = kWG>
__global__ __launch_bounds__(WG) void biquad_carry_kernel(BiquadCarryParams p) {
  constexpr int NW = WG / 64;
  constexpr int RUN = kBiquadCarryRun;
  __shared__ double tot[NW][2];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int C = p.C;
  const MatLane ll(p.lanes, lane);
  const Mat2 lane_pow = p.lanes.at0(lane);  // D^(RUN lane)
  for (int c = 0; c < C; ++c) {
    Vec2 carry{0.0, 0.0};  // Y at the chunk's first record
    if (p.state_in != nullptr) carry = Vec2{p.state_in[c * 2], p.state_in[c * 2 + 1]};
    for (long long r0 = 0; r0 < p.records; r0 += (long long)RUN * WG) {
      const long long first = r0 + (long long)tid * RUN;
      Vec2 b[RUN];
      Vec2 a{0.0, 0.0};
#pragma unroll
      for (int i = 0; i < RUN; ++i) {
        b[i] = Vec2{0.0, 0.0};
        if (first + i < p.records) b[i] = Vec2{p.rec[((first + i) * C + c) * 2], p.rec[((first + i) * C + c) * 2 + 1]};
        a = mat_fma(p.D, a, b[i]);
      }
      const Vec2 inc = ll.scan(a);
      const Vec2 ex = vec_excl(inc, lane);
      const Vec2 t = vec_readlane(inc, 63);
      if (lane == 0) {
        tot[w][0] = t.x;
        tot[w][1] = t.y;
      }
      __syncthreads();
      Vec2 cw = carry;  // Y at this wave's first record
      Vec2 cn = carry;  // Y at the next chunk's first record
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        const Vec2 ti{tot[i][0], tot[i][1]};
        if (i < w) cw = mat_fma(p.wave, cw, ti);
        cn = mat_fma(p.wave, cn, ti);
      }
      Vec2 y = mat_fma(lane_pow, cw, ex);
#pragma unroll
      for (int i = 0; i < RUN; ++i) {
        if (first + i < p.records) {
          MAVG_DCHECK(first + i >= 0, "biquad record index", first + i, p.records);
          p.rec[((first + i) * C + c) * 2] = y.x;
          p.rec[((first + i) * C + c) * 2 + 1] = y.y;
          if (first + i == p.records - 1 && p.state_out != nullptr) {
            const Vec2 so = mat_fma(p.d_last, y, b[i]);
            p.state_out[c * 2] = so.x;
            p.state_out[c * 2 + 1] = so.y;
          }
        }
        y = mat_fma(p.D, y, b[i]);
      }
      carry = cn;
      __syncthreads();  // tot is rewritten by the next chunk
    }
  }
}

// ----------------------------------------------------------------------------
// The strip form's ends: thread t takes channel t % C of the strip of L consecutive frames t / C.
// (A') the strip's aggregate from a zero state to rec; (C') the strip again from its carry-in,
// outputs stored.  Any channel count, any sample-aligned views.
// ----------------------------------------------------------------------------
struct BiquadStripParams {
  const void* in;
  float* out;
  double* rec;  // [strips][C][2]
  long long nframes;
  long long nstrips;
  BiquadCoef k;
  int C;
  int L;
};

template <typename T, bool APPLY, int WG = kWG>
__global__ __launch_bounds__(WG) void biquad_strip_kernel(BiquadStripParams p) {
  const T* __restrict__ in = static_cast<const T*>(p.in);
  const int C = p.C;
  const long long t = (long long)blockIdx.x * WG + threadIdx.x;
  const long long strip = t / C;
  const int c = (int)(t - strip * C);
  if (strip >= p.nstrips) return;
  const long long f0 = strip * p.L;
  const long long f1 = f0 + p.L < p.nframes ? f0 + p.L : p.nframes;
  MAVG_DCHECK(f0 >= 0 && f0 < p.nframes, "biquad strip index", strip, p.nstrips);
  Vec2 s{0.0, 0.0};
  if constexpr (APPLY) s = Vec2{p.rec[(strip * C + c) * 2], p.rec[(strip * C + c) * 2 + 1]};
  for (long long f = f0; f < f1; ++f) {
    const double y = p.k.step(s, (double)in[f * C + c]);
    if constexpr (APPLY) p.out[f * C + c] = (float)y;
  }
  if constexpr (!APPLY) {
    p.rec[(strip * C + c) * 2] = s.x;
    p.rec[(strip * C + c) * 2 + 1] = s.y;
  }
}

}  // namespace mavg
