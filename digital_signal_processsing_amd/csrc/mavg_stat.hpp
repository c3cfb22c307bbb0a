// mavg_stat.hpp -- the moving second moment (mavg_stat_run): mean square, RMS, population
// variance and standard deviation of the causal k-frame window, fp32 out, in one launch.
//   stat_tile_kernel   the flat tile scan's register-staged Blelloch body, scanning
//                      x[n]^2 - x[n-k]^2 (and x[n] - x[n-k]) from one LDS stage of x
//   stat_strip_kernel  one thread per (strip of L frames, channel): a direct window sum, then a
//                      slide -- every shape the tile kernel does not take
#pragma once

#include "mavg_device.hpp"

namespace mavg {

// Accumulators.  fp32 input: fp64 for both moments (x^2 is exact in fp64).  int16 input: S1 in
// int32 (|S1| <= 32768 k < 2^31 for k <= 65535; prefix differences mod 2^32) and S2 in int64
// (S2 <= k 2^30 < 2^46; prefix differences mod 2^64).
template <typename T> struct StatAcc;
template <> struct StatAcc<float> { using A1 = double; using A2 = double; };
template <> struct StatAcc<int16_t> { using A1 = int32_t; using A2 = int64_t; };

__device__ __forceinline__ double stat_sq(float x) { return (double)x * (double)x; }
__device__ __forceinline__ int64_t stat_sq(int16_t x) { return (int64_t)((int32_t)x * (int32_t)x); }
// x^2 - y^2: int16 in int32 (|d| <= 2^30), fp32 as a difference of two exact fp64 squares
__device__ __forceinline__ double stat_dsq(float x, float y) { return (double)x * (double)x - (double)y * (double)y; }
__device__ __forceinline__ int64_t stat_dsq(int16_t x, int16_t y) {
  return (int64_t)((int32_t)x * (int32_t)x - (int32_t)y * (int32_t)y);
}

// fp32 windows of at most this many frames are summed directly from the stage, frame by frame,
// instead of scanned: a prefix of differences carries an absolute error of about 2^-53 of the
// largest window sum near it in the tile, and the bars of include/mavg.h are relative to the
// window's OWN mean square -- squares span twice the exponent range of the samples, so a short
// window of quiet samples right after loud ones (the parity tests' mixed-scale input at k = 2, 3,
// 7: amplitudes over 2^38, a quarter of all windows of two quiet throughout) would keep the loud
// ones' rounding residue.  A direct sum has no cancellation.  From 17 frames on such a window is
// quiet throughout only in a signal that really falls silent; include/mavg.h says what then holds.
constexpr int kStatDirectMax = 16;

// What turns the window's S1 and S2 into an output.  stat is mavg_stat's value: bit 0 takes the
// square root (RMS, STD), bit 1 the variance instead of the mean square (VAR, STD).
struct StatOut {
  double inv_k;    // 1/k
  double inv_k2;   // 1/k^2
  int k;
  int stat;
  int exact;       // int16: N = k S2 - S1^2 formed in int64 (k <= 65535)
  int direct;      // fp32: k <= kStatDirectMax, every window summed directly
};

__device__ __forceinline__ double stat_i64_to_f64(int64_t s) {
  return (double)(int32_t)(s >> 32) * 4294967296.0 + (double)(uint32_t)s;  // one rounding past 2^53
}

// fp32 input: fp64 moments, the cancelling difference clamped at 0 (so is a mean square that
// prefix differences left a rounding below 0).  The root: an fp32 mean square overflows from |x|
// near 2^64 and underflows below 2^-75 although its root is an ordinary fp32 number, so the fp64
// value v = w 4^h is split first, w in [0.5, 2) (the exponent field moved by an even number:
// exact), w rounded to fp32, its correctly rounded fp32 root scaled by 2^h.  The same bits as
// sqrtf((float)v) wherever (float)v is a normal number, and 4^e v gives exactly 2^e times the root
// of v.  v == 0 (exponent field 0: h = -511) leaves as ldexpf(sqrt(0.5), -511) = 0.  (An fp64 root
// rounded once, and this with frexp, ldexp and sqrtf, measured slower: DESIGN.md, Moments.)
//
// The correctly rounded fp32 root of w in [0.5, 2]: the hardware root is within one ulp, and the sign
// of w - s * (neighbour of s), exact in one fma, says which neighbour is nearer -- sqrtf's own
// correction, without its rescaling of subnormal input and its pass-through of 0 and Inf.
__device__ __forceinline__ float stat_sqrt_half_2(float w) {
  float s = __builtin_amdgcn_sqrtf(w);
  const float down = __int_as_float(__float_as_int(s) - 1);
  const float up = __int_as_float(__float_as_int(s) + 1);
  const float rd = __builtin_fmaf(-down, s, w);
  const float ru = __builtin_fmaf(-up, s, w);
  s = rd <= 0.0f ? down : s;
  s = ru > 0.0f ? up : s;
  return s;
}
__device__ __forceinline__ float stat_value(double s1, double s2, const StatOut& o) {
  const double ms = s2 * o.inv_k;
  double v = ms;
  if (o.stat & 2) {
    const double m = s1 * o.inv_k;
    v = ms - m * m;
  }
  v = fmax(v, 0.0);
  const bool root = (o.stat & 1) != 0;
  // the high word of v (sign 0) less that of 0.5: its bits from 21 up count the factors of 4 in
  // v / 0.5, h (an arithmetic shift: floor), and the 21 below them, on 0.5's word, are v 4^-h
  const int hi = __double2hiint(v);
  const int t = hi - 0x3FE00000;
  const int half = t >> 21;
  // one conversion serves both: v, or v 4^-h for the root.  Selects, not a branch: the stat is
  // uniform, but a branch at every output costs more than the root it skips.
  const float f = (float)__hiloint2double(root ? ((t & 0x1FFFFF) | 0x3FE00000) : hi, __double2loint(v));
  const float r = ldexpf(stat_sqrt_half_2(f), half);
  return root ? r : f;
}
// int16 input: exact S1 and S2; N = k S2 - S1^2 exact in int64 while k <= 65535 (both products
// below 2^62), else the moments in fp64.  The fp32 rounding of an fp64 evaluation.
__device__ __forceinline__ float stat_value(int64_t s1, int64_t s2, const StatOut& o) {
  double v;
  if (!(o.stat & 2)) {
    v = stat_i64_to_f64(s2) * o.inv_k;
  } else if (o.exact) {
    const int64_t n = (int64_t)o.k * s2 - s1 * s1;
    v = stat_i64_to_f64(n > 0 ? n : 0) * o.inv_k2;
  } else {
    const double m = stat_i64_to_f64(s1) * o.inv_k;
    v = fmax(stat_i64_to_f64(s2) * o.inv_k - m * m, 0.0);
  }
  if (o.stat & 1) v = sqrt(v);
  return (float)v;
}
__device__ __forceinline__ float stat_value(int32_t s1, int64_t s2, const StatOut& o) {
  return stat_value((int64_t)s1, s2, o);
}
__device__ __forceinline__ float stat_mean(double s1, const StatOut& o) { return (float)(s1 * o.inv_k); }
__device__ __forceinline__ float stat_mean(int64_t s1, const StatOut& o) { return (float)(stat_i64_to_f64(s1) * o.inv_k); }
__device__ __forceinline__ float stat_mean(int32_t s1, const StatOut& o) { return (float)((double)s1 * o.inv_k); }

struct StatParams {
  const void* in;
  float* out;
  float* mean;       // or NULL
  const void* hist;  // k - 1 frames in front of `in`, or NULL
  long long nframes;
  long long ntiles;
  int k;
  int halo_units;    // ceil(k / F): units staged before the tile
  int xk_off;        // (-k*C) mod VE
  int xcd_remap;     // remap_tile mode
  int eio;           // frame-unit launch on an element-aligned input (UnitIO::gload)
  StatOut o;
};

// The dynamic LDS of one workgroup, as byte offsets: the stage of x (halo, tile, one pad unit),
// then per moment the [NSEG][C] segment totals and the [NW][C] halo partial sums -- S2's first
// (8-B accumulators), then S1's.  Read by the kernel, the launcher and the fit check.
template <typename T, int C, int F, int U, int WG>
struct StatLds {
  using A1 = typename StatAcc<T>::A1;
  using A2 = typename StatAcc<T>::A2;
  static constexpr int NW = WG / 64;
  static constexpr int NSEG = U * NW;
  static constexpr int TF = WG * F * U;
  size_t stage_units;  // halo + tile + pad
  size_t tot2, hsum2, tot1, hsum1, bytes;
  __host__ __device__ constexpr explicit StatLds(size_t halo_units)
      : stage_units(halo_units + (size_t)U * WG + 1),
        tot2(((stage_units * F * C * sizeof(T)) + 15) & ~(size_t)15),
        hsum2(tot2 + (size_t)NSEG * C * sizeof(A2)),
        tot1(hsum2 + (size_t)NW * C * sizeof(A2)),
        hsum1(tot1 + (size_t)NSEG * C * sizeof(A1)),
        bytes(hsum1 + (size_t)NW * C * sizeof(A1)) {}
};

// ----------------------------------------------------------------------------
// stat_tile_kernel: tile_scan_kernel's register-staged Blelloch body (RC: a lane keeps only its
// totals across the second barrier and rebuilds the in-lane prefix from the stage; !RC: it keeps
// the prefixes in registers and forms every difference once) -- the same tiles and remap_tile, the split non-temporal load policy, halo and tile staged in
// LDS as T, history through load_elem -- scanning the second moment's differences
// x[n]^2 - x[n-k]^2, formed from the staged x and x[n-k], and with M == 2 the first moment's
// x[n] - x[n-k] beside them: the halo reduction, the segment totals and the wave scans then run
// for both.  M == 1 (S2 alone: mean square and RMS without d_mean) is one scan, the tile scan's
// cost.  The stat is a wave-uniform choice at the output (StatOut).  The output, and the mean, are
// fp32: a 16-B unit of F frames leaves as VE floats (an int16 unit of 8 samples as two 16-B
// stores); the frame-unit form (F == 1, any sample-aligned views) stores elements.
// Frame and sample indices are 64-bit wherever they are not tile-local; tested on 2^32 +
// 10^6-sample signals (tests/test_gpu_bigsignal.py).
// ----------------------------------------------------------------------------
template <typename T, int C, int F, int U, int M, bool RC, int WG = kWG, int NT = kNtSplit | kNtHalo | kNtStore>
__global__ __launch_bounds__(WG) void stat_tile_kernel(StatParams p) {
  static_assert(M == 1 || M == 2, "S2 alone, or S1 and S2");
  constexpr bool kS1 = M == 2;
  constexpr int NW = WG / 64;
  constexpr int VE = F * C;
  constexpr int TF = WG * F * U;           // tile frames
  constexpr int NSEG = U * NW;
  using A1 = typename StatAcc<T>::A1;
  using A2 = typename StatAcc<T>::A2;
  using IO = UnitIO<T, VE>;
  using OIO = UnitIO<float, VE>;
  using U_t = Unit<T, VE>;
  using O_t = Unit<float, VE>;
  using Lds = StatLds<T, C, F, U, WG>;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Hu = p.halo_units;
  const int Ha = Hu * F;                     // staged halo frames (>= k)
  const Lds lds((size_t)Hu);
  [[maybe_unused]] const int SE = (int)lds.stage_units * VE;  // staged elements (the debug checks)
  T* const stage = reinterpret_cast<T*>(smem);
  A2* const tot2 = reinterpret_cast<A2*>(smem + lds.tot2);    // [NSEG][C]
  A2* const hsum2 = reinterpret_cast<A2*>(smem + lds.hsum2);  // [NW][C]
  A1* const tot1 = reinterpret_cast<A1*>(smem + lds.tot1);
  A1* const hsum1 = reinterpret_cast<A1*>(smem + lds.hsum1);
  MAVG_DCHECK(lds.bytes <= lds_budget(WG) && Ha >= p.k, "stat LDS layout", lds.bytes, Hu);

  const T* __restrict__ in = static_cast<const T*>(p.in);
  float* __restrict__ out = p.out;
  float* __restrict__ mean = p.mean;
  const T* __restrict__ hist = static_cast<const T*>(p.hist);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int k = p.k;
  const long long nframes = p.nframes;
  const bool eio = F == 1 && p.eio != 0;

  const long long tile = remap_tile(blockIdx.x, gridDim.x, p.xcd_remap);
  const long long t0 = tile * TF;
  const long long h0 = t0 - Ha;              // first staged halo frame
  MAVG_DCHECK(tile >= 0 && tile < p.ntiles && t0 < nframes, "stat tile index", tile, p.ntiles);
  const bool tile_full = (t0 + TF <= nframes);
  const bool direct = sizeof(T) == 4 && p.o.direct != 0;  // grid-uniform: no scan, windows summed from the stage

  // ---- tile -> registers -> LDS (thread tid takes units u * WG + tid: coalesced) ----
  {
    U_t x[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long f = t0 + (long long)(u * WG + tid) * F;
      if (tile_full) {
        if constexpr ((NT & kNtSplit) != 0) {
          // frames the next tile's halo re-reads keep the default policy (L2)
          if ((u * WG + tid) * F + F > TF - Ha) x[u] = IO::template gload<false>(in + f * C, eio);
          else x[u] = IO::template gload<true>(in + f * C, eio);
        } else {
          x[u] = IO::template gload<(NT & kNtLoad) != 0>(in + f * C, eio);
        }
      } else {
#pragma unroll
        for (int fr = 0; fr < F; ++fr)
#pragma unroll
          for (int c = 0; c < C; ++c) x[u].e[fr * C + c] = load_elem(in, hist, f + fr, c, C, nframes, k, 0);
      }
    }
    // ---- halo -> LDS (re-read of the previous tile's tail: L2) ----
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
          for (int c = 0; c < C; ++c) h.e[fr * C + c] = load_elem(in, hist, f + fr, c, C, nframes, k, 0);
      }
      IO::store(stage + j * VE, h);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) IO::store(stage + (Hu + u * WG + tid) * VE, x[u]);
    if (tid == 0) {
      U_t z;
#pragma unroll
      for (int i = 0; i < VE; ++i) z.e[i] = (T)0;
      IO::store(stage + (Hu + U * WG) * VE, z);   // pad unit (k < F reads one unit past the tile)
    }
  }
  __syncthreads();

  // ---- halo reduction: S1 and S2 of the k frames before t0 ----
  if (!direct) {
    A1 h1[C];
    A2 h2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { h1[c] = (A1)0; h2[c] = (A2)0; }
    for (int i = Ha - k + tid; i < Ha; i += WG) {
      MAVG_DCHECK(i >= 0 && i * C + C <= SE, "stat halo stage index", i, Ha);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const T xv = stage[i * C + c];
        if constexpr (kS1) h1[c] += to_acc<A1>(xv);
        h2[c] += stat_sq(xv);
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const A2 r2 = readlane(wave_incl_scan(h2[c]), 63);
      if (lane == 0) hsum2[w * C + c] = r2;
      if constexpr (kS1) {
        const A1 r1 = readlane(wave_incl_scan(h1[c]), 63);
        if (lane == 0) hsum1[w * C + c] = r1;
      }
    }
  }

  // x[n-k] for lane unit j, from the LDS stage (an unaligned x[n-k]: two aligned units and a
  // uniform shift)
  auto stage_xk = [&](int j) -> U_t {
    const int e = (Ha + j * F - k) * C;
    U_t xk;
    if constexpr (IO::kVec) {
      if (p.xk_off == 0) {
        MAVG_DCHECK(e >= 0 && e + VE <= SE, "stat x[n-k] stage index", e, j);
        xk = IO::load(stage + e);
      } else {
        const int e_lo = e - p.xk_off;
        MAVG_DCHECK(e_lo >= 0 && e_lo + 2 * VE <= SE, "stat x[n-k] extraction", e_lo, j);
        U_t a = IO::load_whole(stage + e_lo);
        U_t b = IO::load_whole(stage + e_lo + VE);
        xk = extract(a, b, p.xk_off);
      }
    } else {
      MAVG_DCHECK(e >= 0 && e + VE <= SE, "stat x[n-k] stage index", e, j);
#pragma unroll
      for (int i = 0; i < VE; ++i) xk.e[i] = stage[e + i];
    }
    return xk;
  };

  // ---- lane totals of the differences; wave scans; segment totals ----
  A1 lx1[U][C];  // exclusive prefix of the lane totals inside the wave
  A2 lx2[U][C];
  constexpr int VU = RC ? 1 : U;
  [[maybe_unused]] A1 v1[VU][F][C];  // !RC: the in-lane prefixes, kept across the barrier
  [[maybe_unused]] A2 v2[VU][F][C];
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int c = 0; c < C; ++c) { lx1[u][c] = (A1)0; lx2[u][c] = (A2)0; }
#pragma unroll
  for (int u = 0; u < U && !direct; ++u) {
    const int j = u * WG + tid;
    MAVG_DCHECK((Hu + j + 1) * VE <= SE, "stat stage index", j, Hu);
    const U_t xu = IO::load(stage + (Hu + j) * VE);
    const U_t xk = stage_xk(j);
    A1 r1[C];
    A2 r2[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { r1[c] = (A1)0; r2[c] = (A2)0; }
#pragma unroll
    for (int fr = 0; fr < F; ++fr)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        if constexpr (kS1) r1[c] += to_acc<A1>(xu.e[fr * C + c]) - to_acc<A1>(xk.e[fr * C + c]);
        r2[c] += stat_dsq(xu.e[fr * C + c], xk.e[fr * C + c]);
        if constexpr (!RC) {
          v1[u][fr][c] = r1[c];
          v2[u][fr][c] = r2[c];
        }
      }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const A2 i2 = wave_incl_scan(r2[c]);
      lx2[u][c] = i2 - r2[c];
      const A2 t2 = readlane(i2, 63);
      if (lane == 0) tot2[(u * NW + w) * C + c] = t2;
      if constexpr (kS1) {
        const A1 i1 = wave_incl_scan(r1[c]);
        lx1[u][c] = i1 - r1[c];
        const A1 t1 = readlane(i1, 63);
        if (lane == 0) tot1[(u * NW + w) * C + c] = t1;
      }
    }
  }
  __syncthreads();

  // ---- carry: halo sums + earlier segments (one exclusive wave scan of the totals) ----
  static_assert(NSEG <= 64, "segment totals are scanned across one wave");
  const int wu = __builtin_amdgcn_readfirstlane(w);
#pragma unroll
  for (int c = 0; c < C && !direct; ++c) {
    A2 w2 = (A2)0;
#pragma unroll
    for (int i = 0; i < NW; ++i) w2 += hsum2[i * C + c];
    const A2 tv2 = lane < NSEG ? tot2[lane * C + c] : (A2)0;
    const A2 ex2 = wave_incl_scan(tv2) - tv2;
#pragma unroll
    for (int u = 0; u < U; ++u) lx2[u][c] += w2 + readlane(ex2, u * NW + wu);
    if constexpr (kS1) {
      A1 w1 = (A1)0;
#pragma unroll
      for (int i = 0; i < NW; ++i) w1 += hsum1[i * C + c];
      const A1 tv1 = lane < NSEG ? tot1[lane * C + c] : (A1)0;
      const A1 ex1 = wave_incl_scan(tv1) - tv1;
#pragma unroll
      for (int u = 0; u < U; ++u) lx1[u][c] += w1 + readlane(ex1, u * NW + wu);
    }
  }

  // ---- outputs: the in-lane prefix again, in the same order ----
  const bool want_mean = kS1 && mean != nullptr;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = u * WG + tid;
    const long long f = t0 + (long long)j * F;
    O_t y, m;
    if (direct) {
      // short fp32 windows: each frame's k staged samples, oldest first (kStatDirectMax)
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
#pragma unroll
        for (int c = 0; c < C; ++c) {
          A1 s1 = (A1)0;
          A2 s2 = (A2)0;
          const int e1 = (Ha + j * F + fr) * C + c;   // the frame's own sample
          MAVG_DCHECK(e1 - (k - 1) * C >= 0 && e1 < SE, "stat direct stage index", e1, k);
          for (int i = k - 1; i >= 0; --i) {
            const T xv = stage[e1 - i * C];
            if constexpr (kS1) s1 += to_acc<A1>(xv);
            s2 += stat_sq(xv);
          }
          y.e[fr * C + c] = stat_value(s1, s2, p.o);
          m.e[fr * C + c] = stat_mean(s1, p.o);
        }
    } else if constexpr (!RC) {
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const A1 s1 = lx1[u][c] + v1[u][fr][c];
          y.e[fr * C + c] = stat_value(s1, lx2[u][c] + v2[u][fr][c], p.o);
          m.e[fr * C + c] = stat_mean(s1, p.o);
        }
    } else {
      const U_t xu = IO::load(stage + (Hu + j) * VE);
      const U_t xk = stage_xk(j);
      A1 r1[C];
      A2 r2[C];
#pragma unroll
      for (int c = 0; c < C; ++c) { r1[c] = lx1[u][c]; r2[c] = lx2[u][c]; }
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
#pragma unroll
        for (int c = 0; c < C; ++c) {
          if constexpr (kS1) r1[c] += to_acc<A1>(xu.e[fr * C + c]) - to_acc<A1>(xk.e[fr * C + c]);
          r2[c] += stat_dsq(xu.e[fr * C + c], xk.e[fr * C + c]);
          y.e[fr * C + c] = stat_value(r1[c], r2[c], p.o);
          m.e[fr * C + c] = stat_mean(r1[c], p.o);
        }
    }
    if (F > 1 && tile_full) {
      MAVG_DCHECK(f >= 0 && f + F <= nframes, "stat output index", f, nframes);
      OIO::template store<(NT & kNtStore) != 0>(out + f * C, y);
      if (want_mean) OIO::template store<(NT & kNtStore) != 0>(mean + f * C, m);
    } else {
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
        if (f + fr < nframes) {
          MAVG_DCHECK(f + fr >= 0, "stat output index", f + fr, nframes);
#pragma unroll
          for (int c = 0; c < C; ++c) {
            out[(f + fr) * C + c] = y.e[fr * C + c];
            if (want_mean) mean[(f + fr) * C + c] = m.e[fr * C + c];
          }
        }
    }
  }
}

// ----------------------------------------------------------------------------
// stat_strip_kernel: correct, not fast -- any channels, any grade, a history, any sample-aligned
// views.  Thread t takes channel t % C of the strip of L consecutive frames t / C: it sums S1 and
// S2 directly over the k frames before the strip (load_elem: history, zeros), then slides the
// window frame by frame, add x[f], subtract x[f-k].  int16 sums are exact in int64 (S2 <= k 2^30
// < 2^61 for every int k); fp32 sums are fp64, and L bounds the slide's length.
// ----------------------------------------------------------------------------
struct StripParams {
  const void* in;
  float* out;
  float* mean;
  const void* hist;
  long long nframes;
  long long nstrips;
  int C;
  int k;
  int L;
  StatOut o;
};

template <typename T, int WG = kWG>
__global__ __launch_bounds__(WG) void stat_strip_kernel(StripParams p) {
  using A = std::conditional_t<sizeof(T) == 2, int64_t, double>;
  const T* __restrict__ in = static_cast<const T*>(p.in);
  const T* __restrict__ hist = static_cast<const T*>(p.hist);
  const int C = p.C;
  const int k = p.k;
  const long long t = (long long)blockIdx.x * WG + threadIdx.x;
  const long long strip = t / C;
  const int c = (int)(t - strip * C);
  if (strip >= p.nstrips) return;
  const long long f0 = strip * p.L;
  const long long f1 = f0 + p.L < p.nframes ? f0 + p.L : p.nframes;
  MAVG_DCHECK(f0 >= 0 && f0 < p.nframes, "stat strip index", strip, p.nstrips);
  if (sizeof(T) == 4 && p.o.direct != 0) {
    // short fp32 windows: every window summed directly, oldest frame first (kStatDirectMax)
    for (long long f = f0; f < f1; ++f) {
      A s1 = (A)0, s2 = (A)0;
      for (long long g = f - k + 1; g <= f; ++g) {
        const T xv = load_elem(in, hist, g, c, C, p.nframes, k, 0);
        s1 += to_acc<A>(xv);
        s2 += stat_sq(xv);
      }
      p.out[f * C + c] = stat_value(s1, s2, p.o);
      if (p.mean != nullptr) p.mean[f * C + c] = stat_mean(s1, p.o);
    }
    return;
  }
  A s1 = (A)0, s2 = (A)0;
  for (long long f = f0 - k; f < f0; ++f) {
    const T xv = load_elem(in, hist, f, c, C, p.nframes, k, 0);
    s1 += to_acc<A>(xv);
    s2 += stat_sq(xv);
  }
  for (long long f = f0; f < f1; ++f) {
    const T xa = in[f * C + c];
    const T xs = load_elem(in, hist, f - k, c, C, p.nframes, k, 0);
    s1 += to_acc<A>(xa) - to_acc<A>(xs);
    s2 += stat_sq(xa) - stat_sq(xs);
    MAVG_DCHECK(f * C + c < p.nframes * C, "stat output index", f, p.nframes);
    p.out[f * C + c] = stat_value(s1, s2, p.o);
    if (p.mean != nullptr) p.mean[f * C + c] = stat_mean(s1, p.o);
  }
}

}  // namespace mavg
