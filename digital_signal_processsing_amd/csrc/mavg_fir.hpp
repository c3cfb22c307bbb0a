// mavg_fir.hpp -- the causal FIR filter y[f] = sum_j h[j] x[f-j] with the caller's taps
// (fir_tile_kernel, fir_strip_kernel).
#pragma once

#include "mavg_device.hpp"

namespace mavg {

// ----------------------------------------------------------------------------
// The contract both kernels keep (include/mavg.h): every output is the fp32 rounding of ONE fp64
// fma chain, acc = +0.0, then acc = fma(h[j], (double)x[f-j], acc) for j = ntaps-1 down to 0 --
// oldest frame first.  The chain of an output is never split or reordered, so every path, form,
// tiling and chunking gives the same bits; the parallelism is across outputs.
//
// fir_tile_kernel: the flat tile of direct_kernel, XCD-remapped, TF = WG * R frames with
// R = U * F: a lane owns U consecutive 16-B units = R consecutive output frames (all C channels)
// and keeps their R * C fp64 accumulators in registers.  The tile and its m = ceil((ntaps-1)/F)
// halo units are staged once in LDS in the input's dtype.  The lane then walks the m + U units
// that cover its windows, oldest first; step t brings ONE unit (F frames) from LDS and feeds it to
// every accumulator it belongs to: the sample of frame e of that unit meets output i with the tap
//     j = (m - t) * F + i - e,
// which is the same for every lane of the grid -- so the taps are wave-uniform scalar loads from
// the caller's device array and cost neither VGPRs nor LDS bandwidth -- and one 16-B LDS read
// feeds R * F * C fmas (fp32 mono 64, stereo 32, int16 mono 128, stereo 64: 8 to 32 per dword).
// Within a step the taps run from the largest j down, so each output still meets its samples oldest
// first.  Steps whose taps all lie in [0, ntaps) run unguarded; the first and last few test each
// tap (a scalar branch) and skip what lies outside.
//
// A lane's units are consecutive, so lanes l and l + 1 read units U apart.  The stage is therefore
// kept in U planes: stage unit s lives in plane s % U at index s / U.  At step t every lane reads
// plane t % U at index lane + t / U: consecutive lanes, consecutive 16-B units, no bank conflict.
// The outputs take the same way back: the lane's R * C floats go to LDS as 16-B units in planes
// (after a barrier, over the stage), and leave as coalesced 16-B stores.
// ----------------------------------------------------------------------------
struct FirParams {
  const void* in;
  float* out;
  const void* hist;
  const double* taps;
  long long nframes;
  int ntaps;
  int m;          // ceil((ntaps-1)/F): halo units in front of the tile
  int xcd_remap;
  int eio;        // frame-unit launch on element-aligned pointers (UnitIO::gload)
};

// FirParams::m of an ntaps-tap filter
template <int F>
constexpr size_t fir_halo_units(int ntaps) { return (size_t)(((long long)ntaps - 1 + F - 1) / F); }

// The dynamic LDS of one workgroup, read by the kernel, launch_fir_tile and fir_tile_fits: the
// stage of m + U * WG units in U planes, each padded so that the planes start 8 / U units apart
// in the 128-B row the stores bank on; the 16-B-unit form reuses it for the fp32 outputs, NO =
// R * C / 4 planes of WG units, 4 units apart in the 256-B row the 16-B reads bank on.
template <typename T, int C, int F, int U, int WG>
struct FirLds {
  static constexpr int kOutUnits = F > 1 ? U * F * C / 4 : 0;   // 16-B fp32 units a lane writes
  static constexpr int kOutPlane = WG + 4;
  size_t plane_units;
  size_t bytes;
  __host__ __device__ constexpr explicit FirLds(size_t m)
      : plane_units((((m + (size_t)U * WG + U - 1) / U + 7) & ~(size_t)7) + (U <= 8 ? 8 / U : 0)),
        bytes(0) {
    const size_t stage = (plane_units * U * F * C * sizeof(T) + 15) & ~(size_t)15;
    const size_t outs = (size_t)kOutUnits * kOutPlane * 16;
    bytes = stage > outs ? stage : outs;
  }
  // element offset of stage unit s
  __host__ __device__ constexpr size_t slot(size_t s) const { return ((s % U) * plane_units + s / U) * (size_t)(F * C); }
};

// One step: the F frames x[e][c] of the unit at distance jb = (m - t) * F meet the R outputs.
// GUARD: taps outside [0, ntaps) are skipped (the window's two ends), each by a uniform branch.
template <bool GUARD, int C, int F, int R>
__device__ __forceinline__ void fir_step(const double* __restrict__ taps, int jb, int ntaps, const double (&x)[F][C],
                                         double (&acc)[R][C]) {
#pragma unroll
  for (int d = R - 1; d >= -(F - 1); --d) {
    const int j = jb + d;  // wave-uniform
    if (!GUARD || (j >= 0 && j < ntaps)) {
      const double h = taps[j];
#pragma unroll
      for (int e = 0; e < F; ++e) {
        const int i = d + e;
        if (i >= 0 && i < R) {
#pragma unroll
          for (int c = 0; c < C; ++c) acc[i][c] = fma(h, x[e][c], acc[i][c]);
        }
      }
    }
    // Each accumulator the branch may have written is pinned to one register where the two ways
    // meet.  Without it the merges of the R + F - 1 branches turn into register copies and the
    // fp32 stereo instance takes 166 VGPRs; with it every instance stays within 128 (four waves
    // per SIMD; tests/test_fir_abi.py reads the compiler's report).  The asm is NOT volatile: a
    // volatile one counts as a possible write to memory, after which the compiler no longer proves
    // the taps unclobbered and loads them with vector loads into VGPRs instead of scalar loads.
    if (GUARD) {
#pragma unroll
      for (int e = 0; e < F; ++e) {
        const int i = d + e;
        if (i >= 0 && i < R) {
#pragma unroll
          for (int c = 0; c < C; ++c) asm("" : "+v"(acc[i][c]));
        }
      }
    }
  }
}

// NT: non-temporal policy bits (mavg_device.hpp): kNtLoad the tile's loads, kNtStore the stores
template <typename T, int C, int F, int U, int WG = kWG, int NT = 0>
__global__ __launch_bounds__(WG) void fir_tile_kernel(FirParams p) {
  static_assert((U & (U - 1)) == 0, "the plane index is a shift");
  constexpr int VE = F * C;
  constexpr int R = U * F;
  constexpr int TF = WG * R;
  using IO = UnitIO<T, VE>;
  using U_t = Unit<T, VE>;
  using Lds = FirLds<T, C, F, U, WG>;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  T* stage = reinterpret_cast<T*>(smem);

  const T* __restrict__ in = static_cast<const T*>(p.in);
  float* __restrict__ out = p.out;
  const T* __restrict__ hist = static_cast<const T*>(p.hist);
  const double* __restrict__ taps = p.taps;
  const int tid = threadIdx.x;
  const int ntaps = p.ntaps;
  const int m = p.m;
  const long long nframes = p.nframes;
  const bool eio = F == 1 && p.eio != 0;
  const Lds lds((size_t)m);

  const long long tile = remap_tile(blockIdx.x, gridDim.x, p.xcd_remap);
  const long long t0 = tile * TF;
  const long long h0 = t0 - (long long)m * F;
  MAVG_DCHECK(tile >= 0 && tile < (long long)gridDim.x && t0 < nframes, "fir tile index", tile, gridDim.x);
  MAVG_DCHECK(lds.bytes <= kLdsBudget, "fir LDS layout", m, U * WG);
  const bool tile_full = (t0 + TF <= nframes);

  // ---- stage: the tile's U * WG units and the m halo units in front of it --------------------
  U_t xr[U];  // every load issued before the first store waits
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long long f = t0 + (long long)(u * WG + tid) * F;
    if (tile_full) {
      xr[u] = IO::template gload<(NT & kNtLoad) != 0>(in + f * C, eio);
    } else {
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
#pragma unroll
        for (int c = 0; c < C; ++c) xr[u].e[fr * C + c] = load_elem(in, hist, f + fr, c, C, nframes, ntaps, 0);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) IO::store(stage + lds.slot((size_t)(m + u * WG + tid)), xr[u]);
  const bool halo_fast = h0 >= 0;
  for (int j = tid; j < m; j += WG) {
    const long long f = h0 + (long long)j * F;
    U_t h;
    if (halo_fast) {
      h = IO::gload(in + f * C, eio);
    } else {
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
#pragma unroll
        for (int c = 0; c < C; ++c) h.e[fr * C + c] = load_elem(in, hist, f + fr, c, C, nframes, ntaps, 0);
    }
    IO::store(stage + lds.slot((size_t)j), h);
  }
  __syncthreads();

  // ---- the chains: R * C accumulators, one unit from LDS per step, oldest first ---------------
  double acc[R][C];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int c = 0; c < C; ++c) acc[i][c] = 0.0;
  const int steps = m + U;  // stage units tid * U + t, t = 0 .. m + U - 1; the lane's own are the last U
  const T* lane0 = stage + (size_t)tid * VE;
  const size_t plane = lds.plane_units * VE;
  U_t nxt = IO::load(lane0);
#pragma unroll 1
  for (int t = 0; t < steps; ++t) {
    const U_t cur = nxt;
    if (t + 1 < steps) {
      const int tn = t + 1;
      MAVG_DCHECK((size_t)(tid + tn / U) < lds.plane_units && tid * U + tn < m + U * WG, "fir stage unit", tid * U + tn, m);
      nxt = IO::load(lane0 + (size_t)(tn % U) * plane + (size_t)(tn / U) * VE);
    }
    double x[F][C];
#pragma unroll
    for (int e = 0; e < F; ++e)
#pragma unroll
      for (int c = 0; c < C; ++c) x[e][c] = to_acc<double>(cur.e[e * C + c]);
    const int jb = (m - t) * F;
    if (jb - (F - 1) >= 0 && jb + R - 1 < ntaps) fir_step<false, C, F, R>(taps, jb, ntaps, x, acc);
    else fir_step<true, C, F, R>(taps, jb, ntaps, x, acc);
  }

  // ---- outputs ------------------------------------------------------------------------------
  if constexpr (F > 1) {
    constexpr int NO = Lds::kOutUnits;
    constexpr int OP = Lds::kOutPlane;
    static_assert((R * C) % 4 == 0 && (NO & (NO - 1)) == 0, "whole 16-B fp32 units per lane");
    using OIO = UnitIO<float, 4>;
    using O_t = Unit<float, 4>;
    float* ost = reinterpret_cast<float*>(smem);
    __syncthreads();  // every lane has read its last stage unit
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      O_t y;
#pragma unroll
      for (int e = 0; e < 4; ++e) y.e[e] = (float)acc[(o * 4 + e) / C][(o * 4 + e) % C];
      OIO::store(ost + (size_t)(o * OP + tid) * 4, y);
    }
    __syncthreads();
    const long long s0 = t0 * C;            // the tile's first sample
    const long long nsamp = nframes * C;
#pragma unroll
    for (int i = 0; i < NO; ++i) {
      const int v = i * WG + tid;            // 16-B unit of the tile's outputs
      const O_t y = OIO::load(ost + (size_t)((v % NO) * OP + v / NO) * 4);
      const long long s = s0 + (long long)v * 4;
      if (tile_full) {
        MAVG_DCHECK(s >= 0 && s + 4 <= nsamp, "fir output index", s, nsamp);
        OIO::template store<(NT & kNtStore) != 0>(out + s, y);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (s + e < nsamp) out[s + e] = y.e[e];
      }
    }
  } else {
    const long long f = t0 + (long long)tid * R;
#pragma unroll
    for (int i = 0; i < R; ++i)
      if (f + i < nframes) {
        MAVG_DCHECK(f + i >= 0, "fir output index", f + i, nframes);
#pragma unroll
        for (int c = 0; c < C; ++c) out[(f + i) * C + c] = (float)acc[i][c];
      }
  }
}

// ----------------------------------------------------------------------------
// fir_strip_kernel: correct, not fast -- any channels, any ntaps, a history, any sample-aligned
// views.  Thread t takes channel t % C of the strip of L consecutive frames t / C and runs the
// contract's chain for each of them from global memory: ntaps reads per output.
// ----------------------------------------------------------------------------
constexpr int kFirStripFrames = 64;

struct FirStripParams {
  const void* in;
  float* out;
  const void* hist;
  const double* taps;
  long long nframes;
  long long nstrips;
  int C;
  int ntaps;
  int L;
};

template <typename T, int WG = kWG>
__global__ __launch_bounds__(WG) void fir_strip_kernel(FirStripParams p) {
  const T* __restrict__ in = static_cast<const T*>(p.in);
  const T* __restrict__ hist = static_cast<const T*>(p.hist);
  const double* __restrict__ taps = p.taps;
  float* __restrict__ out = p.out;
  const int C = p.C;
  const int ntaps = p.ntaps;
  const long long t = (long long)blockIdx.x * WG + threadIdx.x;
  const long long strip = t / C;
  const int c = (int)(t - strip * C);
  if (strip >= p.nstrips) return;
  const long long f0 = strip * p.L;
  const long long f1 = f0 + p.L < p.nframes ? f0 + p.L : p.nframes;
  MAVG_DCHECK(f0 >= 0 && f0 < p.nframes && f1 <= p.nframes, "fir strip index", strip, p.nstrips);
  for (long long f = f0; f < f1; ++f) {
    double acc = 0.0;
    for (int j = ntaps - 1; j >= 0; --j)
      acc = fma(taps[j], to_acc<double>(load_elem(in, hist, f - j, c, C, p.nframes, ntaps, 0)), acc);
    out[f * C + c] = (float)acc;
  }
}

}  // namespace mavg
