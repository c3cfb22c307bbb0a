// mavg_ema.hpp -- the exponential moving average (mavg_ema_run): y[f] = d y[f-1] + alpha x[f] with
// d = 1 - alpha, per channel of an interleaved signal, evaluated in fp64, fp32 out.
//   ema_tile_body     the shared in-tile decayed scan: the stat tile's units and segments, a lane
//                     step (Horner over a unit), a wave step (wave_decay_scan), a segment step
//   ema_tile_kernel   one launch: the carry-in rebuilt from the halo_frames frames before the tile
//                     (what lies further back weighs less than 2^-30), the state in closed form
//   ema_agg_kernel    chain step A: a tile's aggregate b_t (its last output for a zero carry-in)
//   ema_carry_kernel  chain step B, one workgroup: the aggregates turned in place into carry-ins
//                     Y[t+1] = d^T Y[t] + b_t, and d_state_out
//   ema_apply_kernel  chain step C: the tile body from Y[t], outputs stored
//   ema_strip_agg_kernel / ema_strip_apply_kernel   A and C for one thread per (strip of L
//                     frames, channel): every channel count -- correct, not fast
// The composition of the recurrence over m frames is y_out = d^m y_in + b: only b is scanned, and
// every multiplier is a power of d the host computes (EmaParams).
#pragma once

#include "mavg_device.hpp"

namespace mavg {

// b^(2^i), i = 0 .. 5, of one scan level's base b (computed on the host, each straight from d)
struct DecayPow {
  double p[6];
};
// b^e for 0 <= e < 64
__device__ __forceinline__ double decay_pow(const DecayPow& b, int e) {
  double r = 1.0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if ((e >> i) & 1) r *= b.p[i];
  return r;
}
// the decayed scan of one level: the uniform powers and this lane's two broadcast weights
struct DecayLane {
  double q1, q2, q4, q8, w15, w31;
  __device__ __forceinline__ DecayLane(const DecayPow& b, int lane)
      : q1(b.p[0]), q2(b.p[1]), q4(b.p[2]), q8(b.p[3]), w15(decay_pow(b, (lane & 15) + 1)),
        w31(decay_pow(b, (lane & 31) + 1)) {}
  __device__ __forceinline__ double scan(double v) const { return wave_decay_scan(v, q1, q2, q4, q8, w15, w31); }
};
// the inclusive value of the lane before (0 in lane 0): a lane's exclusive carry
__device__ __forceinline__ double decay_excl(double incl, int lane) {
  const double e = shfl_up(incl, 1);
  return lane == 0 ? 0.0 : e;
}

struct EmaParams {
  const void* in;
  float* out;
  const double* state_in;  // or NULL: y[-1] = 0
  double* state_out;       // or NULL (the tile kernel; the chain's is written by ema_carry_kernel)
  double* rec;             // chain: one fp64 record per tile and channel
  long long nframes;
  long long ntiles;
  double alpha;
  double d;                // 1 - alpha
  DecayPow unit;           // base d^F: the lanes of a segment
  DecayPow seg;            // base d^(64 F): the segments of a tile
  DecayPow run;            // base d^halo_run: the lanes of the halo reduction
  double run_wave;         // d^(64 halo_run): the waves of the halo reduction
  double d_tile;           // d^tile_frames
  int halo_frames;         // H: the state enters tiles with t0 < H
  int halo_units;          // ceil(H / F): units staged before the tile (0: chain)
  int halo_run;            // frames per thread of the halo reduction: ceil(halo_units F / WG)
  int xcd_remap;           // remap_tile mode
  int eio;                 // frame-unit launch on an element-aligned input (UnitIO::gload)
};

// The dynamic LDS of one workgroup, as byte offsets: the stage of x (halo, tile), the [NSEG][C]
// segment totals, the [NW][C] halo partials.  Read by the kernels, the launcher and the fit check.
template <typename T, int C, int F, int U, int WG>
struct EmaLds {
  static constexpr int NW = WG / 64;
  static constexpr int NSEG = U * NW;
  static constexpr int TF = WG * F * U;
  size_t stage_units;  // halo + tile
  size_t tot, hsum, bytes;
  __host__ __device__ constexpr explicit EmaLds(size_t halo_units)
      : stage_units(halo_units + (size_t)U * WG),
        tot(((stage_units * F * C * sizeof(T)) + 15) & ~(size_t)15),
        hsum(tot + (size_t)NSEG * C * sizeof(double)),
        bytes(hsum + (size_t)NW * C * sizeof(double)) {}
};

// tile (and halo) -> registers -> LDS, as stat_tile_kernel: thread tid takes units u * WG + tid;
// a whole tile moves as 16-B units, non-temporal except the frames the next tile's halo re-reads;
// a part tile and a halo that starts before frame 0 move as guarded elements (zeros outside).
// P: EmaParams, or another family's parameters with in, nframes, halo_units and eio (mavg_biquad.hpp).
template <typename T, int C, int F, int U, int WG, int NT, typename P>
__device__ __forceinline__ void ema_stage(const P& p, T* stage, long long t0, bool tile_full) {
  constexpr int VE = F * C;
  constexpr int TF = WG * F * U;
  using IO = UnitIO<T, VE>;
  using U_t = Unit<T, VE>;
  const T* __restrict__ in = static_cast<const T*>(p.in);
  const int tid = threadIdx.x;
  const int Hu = p.halo_units;
  const int Ha = Hu * F;
  const long long nframes = p.nframes;
  const bool eio = F == 1 && p.eio != 0;
  U_t x[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long long f = t0 + (long long)(u * WG + tid) * F;
    if (tile_full) {
      if constexpr ((NT & kNtSplit) != 0) {
        if ((u * WG + tid) * F + F > TF - Ha) x[u] = IO::template gload<false>(in + f * C, eio);
        else x[u] = IO::template gload<true>(in + f * C, eio);
      } else {
        x[u] = IO::template gload<(NT & kNtLoad) != 0>(in + f * C, eio);
      }
    } else {
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
#pragma unroll
        for (int c = 0; c < C; ++c) x[u].e[fr * C + c] = load_elem<T>(in, nullptr, f + fr, c, C, nframes, 1, 0);
    }
  }
  const long long h0 = t0 - Ha;  // first staged halo frame
  const bool halo_fast = h0 >= 0;
  for (int j = tid; j < Hu; j += WG) {
    const long long f = h0 + (long long)j * F;
    U_t h;
    if (halo_fast) {
      h = IO::template gload<(NT & kNtHalo) != 0>(in + f * C, eio);
    } else {
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
#pragma unroll
        for (int c = 0; c < C; ++c) h.e[fr * C + c] = load_elem<T>(in, nullptr, f + fr, c, C, nframes, 1, 0);
    }
    IO::store(stage + j * VE, h);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) IO::store(stage + (Hu + u * WG + tid) * VE, x[u]);
}

// ----------------------------------------------------------------------------
// ema_tile_body: the in-tile decayed scan over a staged tile (`tile`: its first unit in LDS).
//   lane step     Horner over each of the lane's units from zero: the unit's aggregate
//   wave step     wave_decay_scan (base d^F) over the 64 aggregates of a segment; the lane's
//                 exclusive value by a lane shift; the segment's total to LDS
//   segment step  after the barrier every wave scans the NSEG totals (base d^(64 F)); the tile's
//                 carry-in Y (carry_in(), read after the barrier) enters segment s as d^(64 F s) Y
//   output step   Horner again from the lane's carry; OUT: (float)y stored, 16-B stores for whole
//                 tiles.  The thread that owns frame rec_frame writes its y there to rec[c] (fp64).
// Thread tid owns units u * WG + tid: segment s = u * NW + wave holds units 64 s .. 64 s + 63.
// ----------------------------------------------------------------------------
template <typename T, int C, int F, int U, int WG, bool OUT, int NT, typename CarryIn>
__device__ __forceinline__ void ema_tile_body(const EmaParams& p, const T* tile, double* tot, CarryIn&& carry_in,
                                              long long t0, bool tile_full, double* rec, long long rec_frame) {
  constexpr int NW = WG / 64;
  constexpr int VE = F * C;
  constexpr int NSEG = U * NW;
  using IO = UnitIO<T, VE>;
  using OIO = UnitIO<float, VE>;
  using U_t = Unit<T, VE>;
  using O_t = Unit<float, VE>;
  static_assert(NSEG <= 64, "segment totals are scanned across one wave");
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const double d = p.d, alpha = p.alpha;

  // ---- lane step and wave step ----
  double cy[U][C];  // the lane's carry: first its exclusive value inside the segment
  {
    const DecayLane ul(p.unit, lane);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const U_t xu = IO::load(tile + (u * WG + tid) * VE);
      double r[C];
#pragma unroll
      for (int c = 0; c < C; ++c) r[c] = 0.0;
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
#pragma unroll
        for (int c = 0; c < C; ++c) r[c] = fma(d, r[c], alpha * (double)xu.e[fr * C + c]);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double inc = ul.scan(r[c]);
        cy[u][c] = decay_excl(inc, lane);
        const double t = readlane(inc, 63);
        if (lane == 0) tot[(u * NW + w) * C + c] = t;
      }
    }
  }
  __syncthreads();

  // ---- segment step ----
  {
    double Y[C];
    carry_in(Y);
    const int wu = __builtin_amdgcn_readfirstlane(w);
    const DecayLane sl(p.seg, lane);
    const double seg_pow = decay_pow(p.seg, lane);    // d^(64 F lane)
    const double unit_pow = decay_pow(p.unit, lane);  // d^(F lane)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double tv = lane < NSEG ? tot[lane * C + c] : 0.0;
      const double cs = fma(seg_pow, Y[c], decay_excl(sl.scan(tv), lane));  // carry into segment `lane`
#pragma unroll
      for (int u = 0; u < U; ++u) cy[u][c] = fma(unit_pow, readlane(cs, u * NW + wu), cy[u][c]);
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
    double y[C];
#pragma unroll
    for (int c = 0; c < C; ++c) y[c] = cy[u][c];
#pragma unroll
    for (int fr = 0; fr < F; ++fr)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        y[c] = fma(d, y[c], alpha * (double)xu.e[fr * C + c]);
        yo.e[fr * C + c] = (float)y[c];
        if (mine && f + fr == rec_frame) rec[c] = y[c];
      }
    if constexpr (OUT) {
      if (F > 1 && tile_full) {
        MAVG_DCHECK(f >= 0 && f + F <= p.nframes, "ema output index", f, p.nframes);
        OIO::template store<(NT & kNtStore) != 0>(out + f * C, yo);
      } else {
#pragma unroll
        for (int fr = 0; fr < F; ++fr)
          if (f + fr < p.nframes) {
            MAVG_DCHECK(f + fr >= 0, "ema output index", f + fr, p.nframes);
#pragma unroll
            for (int c = 0; c < C; ++c) out[(f + fr) * C + c] = yo.e[fr * C + c];
          }
      }
    }
  }
}

// ----------------------------------------------------------------------------
// ema_tile_kernel: one launch, no workspace.  A tile stages its halo_frames frames of halo (a
// re-read of the previous tile's tail; zeros before frame 0) in front of its own and reduces them
// to its carry-in: thread tid runs Horner over halo_run contiguous frames (the runs padded with
// zeros at the old end), the waves' decayed scans (base d^halo_run) and the four wave totals
// (weights d^(64 halo_run)) combine them.  What the halo leaves out -- earlier frames, and from
// t0 >= halo_frames on the state -- weighs at most d^halo_frames <= 2^-30.  Tiles with t0 <
// halo_frames add d^t0 y[-1] (wave-uniform; d^t0 as t0 / tile_frames products of d^tile_frames).
// Frame and sample indices are 64-bit wherever they are not tile-local.
// ----------------------------------------------------------------------------
template <typename T, int C, int F, int U, int WG = kWG, int NT = kNtSplit | kNtHalo | kNtStore>
__global__ __launch_bounds__(WG) void ema_tile_kernel(EmaParams p) {
  constexpr int NW = WG / 64;
  constexpr int VE = F * C;
  constexpr int TF = WG * F * U;
  using Lds = EmaLds<T, C, F, U, WG>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Hu = p.halo_units;
  const int Ha = Hu * F;
  const Lds lds((size_t)Hu);
  T* const stage = reinterpret_cast<T*>(smem);
  double* const tot = reinterpret_cast<double*>(smem + lds.tot);
  double* const hsum = reinterpret_cast<double*>(smem + lds.hsum);
  MAVG_DCHECK(lds.bytes <= lds_budget(WG) && Ha >= p.halo_frames && p.halo_run * WG >= Ha, "ema LDS layout", lds.bytes, Hu);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const long long tile = remap_tile(blockIdx.x, gridDim.x, p.xcd_remap);
  const long long t0 = tile * TF;
  MAVG_DCHECK(tile >= 0 && tile < p.ntiles && t0 < p.nframes, "ema tile index", tile, p.ntiles);
  const bool tile_full = (t0 + TF <= p.nframes);
  ema_stage<T, C, F, U, WG, NT>(p, stage, t0, tile_full);
  __syncthreads();

  // ---- halo reduction (its partials are read after the body's barrier) ----
  const int R = p.halo_run;
  if (R > 0) {
    const int pad = R * WG - Ha;  // zeros in front of the oldest staged frame
    double h[C];
#pragma unroll
    for (int c = 0; c < C; ++c) h[c] = 0.0;
    for (int i = 0; i < R; ++i) {
      const int g = tid * R + i - pad;
      if (g < 0) continue;
      MAVG_DCHECK(g < Ha, "ema halo stage index", g, Ha);
#pragma unroll
      for (int c = 0; c < C; ++c) h[c] = fma(p.d, h[c], p.alpha * (double)stage[g * C + c]);
    }
    const DecayLane rl(p.run, lane);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const double t = readlane(rl.scan(h[c]), 63);
      if (lane == 0) hsum[w * C + c] = t;
    }
  }
  auto carry_in = [&](double(&Y)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      double y = 0.0;
      if (R > 0) {
#pragma unroll
        for (int i = 0; i < NW; ++i) y = fma(p.run_wave, y, hsum[i * C + c]);
      }
      Y[c] = y;
    }
    if (p.state_in != nullptr && t0 < (long long)p.halo_frames) {
      double ds = 1.0;  // d^t0
      for (long long i = 0; i < tile; ++i) ds *= p.d_tile;
#pragma unroll
      for (int c = 0; c < C; ++c) Y[c] = fma(ds, p.state_in[c], Y[c]);
    }
  };
  ema_tile_body<T, C, F, U, WG, true, NT>(p, stage + (size_t)Hu * VE, tot, carry_in, t0, tile_full, p.state_out,
                                          p.nframes - 1);
}

// chain step A: the tile's aggregate -- its y at its last frame for a zero carry-in -- to rec[tile]
// (plain loads: step C reads the same frames again; its own are non-temporal)
template <typename T, int C, int F, int U, int WG = kWG, int NT = 0>
__global__ __launch_bounds__(WG) void ema_agg_kernel(EmaParams p) {
  constexpr int TF = WG * F * U;
  using Lds = EmaLds<T, C, F, U, WG>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds lds(0);
  T* const stage = reinterpret_cast<T*>(smem);
  double* const tot = reinterpret_cast<double*>(smem + lds.tot);
  const long long tile = remap_tile(blockIdx.x, gridDim.x, p.xcd_remap);
  const long long t0 = tile * TF;
  MAVG_DCHECK(p.halo_units == 0 && tile >= 0 && tile < p.ntiles && t0 < p.nframes, "ema tile index", tile, p.ntiles);
  const bool tile_full = (t0 + TF <= p.nframes);
  ema_stage<T, C, F, U, WG, NT>(p, stage, t0, tile_full);
  __syncthreads();
  auto carry_in = [&](double(&Y)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) Y[c] = 0.0;
  };
  const long long last = tile_full ? t0 + TF - 1 : p.nframes - 1;
  ema_tile_body<T, C, F, U, WG, false, NT>(p, stage, tot, carry_in, t0, tile_full, p.rec + tile * C, last);
}

// chain step C: the tile body from the carry-in rec[tile], outputs stored
template <typename T, int C, int F, int U, int WG = kWG, int NT = kNtLoad | kNtStore>
__global__ __launch_bounds__(WG) void ema_apply_kernel(EmaParams p) {
  constexpr int TF = WG * F * U;
  using Lds = EmaLds<T, C, F, U, WG>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds lds(0);
  T* const stage = reinterpret_cast<T*>(smem);
  double* const tot = reinterpret_cast<double*>(smem + lds.tot);
  const long long tile = remap_tile(blockIdx.x, gridDim.x, p.xcd_remap);
  const long long t0 = tile * TF;
  MAVG_DCHECK(p.halo_units == 0 && tile >= 0 && tile < p.ntiles && t0 < p.nframes, "ema tile index", tile, p.ntiles);
  const bool tile_full = (t0 + TF <= p.nframes);
  ema_stage<T, C, F, U, WG, NT>(p, stage, t0, tile_full);
  __syncthreads();
  auto carry_in = [&](double(&Y)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) Y[c] = p.rec[tile * C + c];
  };
  ema_tile_body<T, C, F, U, WG, true, NT>(p, stage, tot, carry_in, t0, tile_full, nullptr, 0);
}

// ----------------------------------------------------------------------------
// ema_carry_kernel (chain step B): ONE workgroup turns the `records` aggregates b_t of spans of
// `span` frames (tiles or strips; the last may be shorter) in place into carry-ins: Y[0] = y[-1],
// Y[t+1] = D Y[t] + b_t with D = d^span, per channel, and writes d_state_out = d^last_frames
// Y[records-1] + b_last.  It works in chunks of kEmaCarryChunk records: lane tid takes the
// kEmaCarryRun contiguous records tid * kEmaCarryRun .. of the chunk (Horner, base D), the waves'
// decayed scans (base D^kEmaCarryRun) and the wave totals combine the lanes, and a running carry
// links the chunks.  Records past the end read as 0 and are not written.
// ----------------------------------------------------------------------------
constexpr int kEmaCarryRun = 16;
constexpr int kEmaCarryChunk = kEmaCarryRun * kWG;  // 4096 records
struct EmaCarryParams {
  double* rec;             // [records][C]
  const double* state_in;  // or NULL
  double* state_out;       // or NULL
  long long records;
  int C;
  double D;                // d^span
  DecayPow lanes;          // base D^kEmaCarryRun
  double wave;             // D^(64 kEmaCarryRun)
  double d_last;           // d^(frames of the last span)
};

template <int WG = kWG>
__global__ __launch_bounds__(WG) void ema_carry_kernel(EmaCarryParams p) {
  constexpr int NW = WG / 64;
  constexpr int RUN = kEmaCarryRun;
  __shared__ double tot[NW];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int C = p.C;
  const DecayLane ll(p.lanes, lane);
  const double lane_pow = decay_pow(p.lanes, lane);  // D^(RUN lane)
  for (int c = 0; c < C; ++c) {
    double carry = p.state_in != nullptr ? p.state_in[c] : 0.0;  // Y at the chunk's first record
    for (long long r0 = 0; r0 < p.records; r0 += (long long)RUN * WG) {
      const long long first = r0 + (long long)tid * RUN;
      double b[RUN];
      double a = 0.0;
#pragma unroll
      for (int i = 0; i < RUN; ++i) {
        b[i] = first + i < p.records ? p.rec[(first + i) * C + c] : 0.0;
        a = fma(p.D, a, b[i]);
      }
      const double inc = ll.scan(a);
      const double ex = decay_excl(inc, lane);
      const double t = readlane(inc, 63);
      if (lane == 0) tot[w] = t;
      __syncthreads();
      double cw = carry;  // Y at this wave's first record
      double cn = carry;  // Y at the next chunk's first record
#pragma unroll
      for (int i = 0; i < NW; ++i) {
        if (i < w) cw = fma(p.wave, cw, tot[i]);
        cn = fma(p.wave, cn, tot[i]);
      }
      double y = fma(lane_pow, cw, ex);
#pragma unroll
      for (int i = 0; i < RUN; ++i) {
        if (first + i < p.records) {
          MAVG_DCHECK(first + i >= 0, "ema record index", first + i, p.records);
          p.rec[(first + i) * C + c] = y;
          if (first + i == p.records - 1 && p.state_out != nullptr) p.state_out[c] = fma(p.d_last, y, b[i]);
        }
        y = fma(p.D, y, b[i]);
      }
      carry = cn;
      __syncthreads();  // tot is rewritten by the next chunk
    }
  }
}

// ----------------------------------------------------------------------------
// The strip form's ends: thread t takes channel t % C of the strip of L consecutive frames t / C.
// (A') the strip's aggregate from zero to rec; (C') the strip again from its carry-in, outputs
// stored.  Any channel count, any sample-aligned views.
// ----------------------------------------------------------------------------
struct EmaStripParams {
  const void* in;
  float* out;
  double* rec;  // [strips][C]
  long long nframes;
  long long nstrips;
  double alpha;
  double d;
  int C;
  int L;
};

template <typename T, bool APPLY, int WG = kWG>
__global__ __launch_bounds__(WG) void ema_strip_kernel(EmaStripParams p) {
  const T* __restrict__ in = static_cast<const T*>(p.in);
  const int C = p.C;
  const long long t = (long long)blockIdx.x * WG + threadIdx.x;
  const long long strip = t / C;
  const int c = (int)(t - strip * C);
  if (strip >= p.nstrips) return;
  const long long f0 = strip * p.L;
  const long long f1 = f0 + p.L < p.nframes ? f0 + p.L : p.nframes;
  MAVG_DCHECK(f0 >= 0 && f0 < p.nframes, "ema strip index", strip, p.nstrips);
  double y = APPLY ? p.rec[strip * C + c] : 0.0;
  for (long long f = f0; f < f1; ++f) {
    y = fma(p.d, y, p.alpha * (double)in[f * C + c]);
    if constexpr (APPLY) p.out[f * C + c] = (float)y;
  }
  if constexpr (!APPLY) p.rec[strip * C + c] = y;
}

}  // namespace mavg
