// mavg_cascade.hpp -- the cascaded moving average (mavg_cascade_run): `passes` boxcar passes of
// one window inside one tile, the intermediates kept in LDS in the signal's own dtype.
//   cascade_tile_kernel  the flat tile scan's register-staged Blelloch body, run `passes` times
//                        over an LDS stage of passes * (k - 1) halo frames plus the tile
#pragma once

#include "mavg_device.hpp"

namespace mavg {

struct CascadeParams {
  const void* in;
  void* out;
  const void* hist;   // passes * (k - 1) frames in front of `in`, or NULL
  long long nframes;
  long long ntiles;
  int k;
  int passes;
  int halo_frames;    // H = passes * (k - 1)
  int halo_units;     // ceil(H / F): units staged before the tile
  int xk_units;       // ceil(k / F): a pass reads this many units below the first it writes
  int xk_off;         // (-k*C) mod VE
  int xcd_remap;      // remap_tile mode
  int eio;            // frame-unit launch on element-aligned views (UnitIO::gload)
  OutParams o;
};

// The dynamic LDS of one workgroup, as byte offsets: two stages of the same shape (a pass reads one
// and writes the other).  A stage is the halo units, the tile, one
// pad unit (k < F reads one unit past the tile) and one 16-B vector of slack: the frame-unit form
// lays the last pass's outputs down at the 16-B phase of their place in d_out.
template <typename T, typename A, int C, int F, int U, int WG>
struct CascadeLds {
  static constexpr int TF = WG * F * U;
  static constexpr int EPV = 16 / (int)sizeof(T);
  size_t stage_units;   // halo + tile + pad
  size_t stage_elems;   // stage_units * F * C + EPV, rounded up to a 16-B multiple
  size_t stage_b, bytes;
  __host__ __device__ constexpr explicit CascadeLds(size_t halo_units)
      : stage_units(halo_units + (size_t)U * WG + 1),
        stage_elems(((stage_units * F * C + EPV) + EPV - 1) / EPV * EPV),
        stage_b(stage_elems * sizeof(T)),
        bytes(2 * stage_b) {}
};

// The first unit pass j (1-based) of `passes` scans: the last pass scans the tile alone (unit
// halo_units); a pass reads xk_units units below the first unit it writes, so the pass before it
// starts that much lower, never below unit 0 (what lies before the stage reads as zero, and the
// frames that then come out wrong are frames no later pass trusts: frame -(passes - j)(k - 1) and
// later are right after pass j, tests/test_cascade_model.py).
__host__ __device__ inline int cascade_first_unit(int halo_units, int xk_units, int passes, int j) {
  const long long u = (long long)halo_units - (long long)(passes - j) * xk_units;
  return u > 0 ? (int)u : 0;
}

// ----------------------------------------------------------------------------
// cascade_tile_kernel: tile_scan_kernel's non-DMA Blelloch body -- the same tiles and remap_tile,
// the split non-temporal load policy, halo and tile staged in LDS, history through load_elem, the
// same in-lane prefix, DPP wave scan and to_out -- with two changes that let it run `passes` times
// on the stage.  (1) A wave owns a contiguous run of units and carries its running sum from one
// 64-unit round to the next in registers; the sum it starts from is the window sum just before its
// run, rebuilt from the k staged frames there as the tile scan rebuilds a tile's carry from its
// halo.  No wave waits for another inside a pass: one barrier per pass.  (2) Pass j reads stage
// (j - 1) & 1 and writes the window means, converted by to_out to T, to the other stage; the last
// pass writes the tile's frames to d_out instead.  Pass j scans units [cascade_first_unit(j),
// stage end): the span later passes still need, not the whole stage.
// int16 sums are int32 prefix differences mod 2^32 (a window sum is below 2^31 for k <= 65535);
// fp32 sums are fp64.  Frame and sample indices are 64-bit wherever they are not tile-local; tested
// on 2^32 + 10^6-sample signals (tests/test_gpu_bigsignal.py).
// ----------------------------------------------------------------------------
template <typename T, typename A, int C, int F, int U, int WG = kWG, int NT = kNtSplit | kNtHalo | kNtStore, int DV = 0>
__global__ __launch_bounds__(WG) void cascade_tile_kernel(CascadeParams p) {
  constexpr int VE = F * C;
  constexpr int TF = WG * F * U;           // tile frames
  using IO = UnitIO<T, VE>;
  using U_t = Unit<T, VE>;
  using Lds = CascadeLds<T, A, C, F, U, WG>;
  constexpr int EPV = Lds::EPV;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Hu = p.halo_units;
  const int Ha = Hu * F;                     // staged halo frames (>= H)
  const Lds lds((size_t)Hu);
  const int NU = Hu + U * WG;                // units a pass may write: halo + tile
  const int stage_elems = (int)lds.stage_elems;
  T* const stage0 = reinterpret_cast<T*>(smem);
  T* const stage1 = stage0 + stage_elems;

  const T* __restrict__ in = static_cast<const T*>(p.in);
  T* __restrict__ out = static_cast<T*>(p.out);
  const T* __restrict__ hist = static_cast<const T*>(p.hist);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int k = p.k;
  const int H1 = p.halo_frames + 1;          // load_elem's window: the history holds H1 - 1 frames
  const long long nframes = p.nframes;
  const bool eio = F == 1 && p.eio != 0;

  const long long tile = remap_tile(blockIdx.x, gridDim.x, p.xcd_remap);
  const long long t0 = tile * TF;
  const long long h0 = t0 - Ha;              // first staged halo frame
  MAVG_DCHECK(tile >= 0 && tile < p.ntiles && t0 < nframes, "cascade tile index", tile, p.ntiles);
  MAVG_DCHECK(lds.bytes <= lds_budget(WG) && Ha >= p.halo_frames, "cascade LDS layout", lds.bytes, Hu);
  const bool tile_full = (t0 + TF <= nframes);

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
          for (int c = 0; c < C; ++c) x[u].e[fr * C + c] = load_elem(in, hist, f + fr, c, C, nframes, H1, 0);
      }
    }
    // ---- halo -> LDS (re-read of the previous tiles' tail: L2) ----
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
          for (int c = 0; c < C; ++c) h.e[fr * C + c] = load_elem(in, hist, f + fr, c, C, nframes, H1, 0);
      }
      IO::store(stage0 + j * VE, h);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) IO::store(stage0 + (Hu + u * WG + tid) * VE, x[u]);
    if (tid == 0) {
      U_t z;
#pragma unroll
      for (int i = 0; i < VE; ++i) z.e[i] = (T)0;
      IO::store(stage0 + NU * VE, z);   // pad units (k < F reads one unit past the tile)
      IO::store(stage1 + NU * VE, z);
    }
  }
  __syncthreads();

  // the 16-B phase of the tile's first output sample, in samples (frame-unit form's output stage)
  const int sh = (int)(((reinterpret_cast<uintptr_t>(out) / sizeof(T)) + (unsigned long long)t0 * C) & (unsigned)(EPV - 1));

  for (int pass = 1; pass <= p.passes; ++pass) {
    const bool last = pass == p.passes;
    const T* const src = (pass & 1) ? stage0 : stage1;
    T* const dst = (pass & 1) ? stage1 : stage0;
    // units [u0, NU) in NW contiguous runs of `rounds` 64-unit rounds each
    const int u0 = cascade_first_unit(Hu, p.xk_units, p.passes, pass);
    const int rounds = (NU - u0 + WG - 1) / WG;
    const int ub = u0 + w * rounds * 64;     // this wave's first unit (uniform)

    // ---- the wave's base: the window sum at the frame before its run ----
    A run[C];
    {
      A hs[C];
#pragma unroll
      for (int c = 0; c < C; ++c) hs[c] = (A)0;
      const int fb = ub * F;                 // the run's first frame, stage-local
      if (ub < NU) {
        for (int i = fb - k + lane; i < fb; i += 64) {
          if (i >= 0) {
            MAVG_DCHECK(i * C + C <= NU * VE, "cascade base stage index", i, fb);
#pragma unroll
            for (int c = 0; c < C; ++c) hs[c] += to_acc<A>(src[i * C + c]);
          }
        }
      }
#pragma unroll
      for (int c = 0; c < C; ++c) run[c] = readlane(wave_incl_scan(hs[c]), 63);
    }

    // x[n-k] for unit j, from the source stage (an unaligned x[n-k]: two aligned units and a
    // uniform shift); below the stage it reads as zero
    auto stage_xk = [&](int j) -> U_t {
      const int e = (j * F - k) * C;
      U_t xk;
      if (e - p.xk_off < 0) {
#pragma unroll
        for (int i = 0; i < VE; ++i) xk.e[i] = e + i >= 0 ? src[e + i] : (T)0;
        return xk;
      }
      if constexpr (IO::kVec) {
        if (p.xk_off == 0) {
          MAVG_DCHECK(e + VE <= (int)lds.stage_units * VE, "cascade x[n-k] stage index", e, j);
          xk = IO::load(src + e);
        } else {
          const int e_lo = e - p.xk_off;
          MAVG_DCHECK(e_lo + 2 * VE <= (int)lds.stage_units * VE, "cascade x[n-k] extraction", e_lo, j);
          U_t a = IO::load_whole(src + e_lo);
          U_t b = IO::load_whole(src + e_lo + VE);
          xk = extract(a, b, p.xk_off);
        }
      } else {
        MAVG_DCHECK(e + VE <= (int)lds.stage_units * VE, "cascade x[n-k] stage index", e, j);
#pragma unroll
        for (int i = 0; i < VE; ++i) xk.e[i] = src[e + i];
      }
      return xk;
    };

    // ---- d = x - x[n-k]; in-lane prefix, wave scan, the carry from round to round ----
    for (int q = 0; q < rounds; ++q) {
      const int j = ub + q * 64 + lane;
      const bool live = j < NU;
      A v[F][C];
      U_t y;
      if (live) {
        MAVG_DCHECK(j >= 0 && (j + 1) * VE <= (int)lds.stage_units * VE, "cascade stage index", j, NU);
        const U_t xu = IO::load(src + j * VE);
        const U_t xk = stage_xk(j);
#pragma unroll
        for (int fr = 0; fr < F; ++fr)
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const A d = to_acc<A>(xu.e[fr * C + c]) - to_acc<A>(xk.e[fr * C + c]);
            v[fr][c] = fr == 0 ? d : v[fr - 1][c] + d;
          }
      } else {
#pragma unroll
        for (int fr = 0; fr < F; ++fr)
#pragma unroll
          for (int c = 0; c < C; ++c) v[fr][c] = (A)0;
      }
      A lx[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const A incl = wave_incl_scan(v[F - 1][c]);
        lx[c] = run[c] + (incl - v[F - 1][c]);
        run[c] += readlane(incl, 63);
      }
      if (!live) continue;
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
#pragma unroll
        for (int c = 0; c < C; ++c) y.e[fr * C + c] = to_out<T, A, DV>(lx[c] + v[fr][c], p.o);
      if (!last) {
        IO::store(dst + j * VE, y);
        continue;
      }
      // ---- the last pass: the tile's frames leave ----
      MAVG_DCHECK(j >= Hu, "cascade last pass unit", j, Hu);
      const int fl = (j - Hu) * F;             // tile-local frame
      const long long f = t0 + fl;
      if constexpr (F == 1) {
        // frame-unit form: through the free stage, at the output's 16-B phase
        MAVG_DCHECK(sh + (fl + 1) * C <= stage_elems, "cascade output stage index", sh + fl * C, stage_elems);
#pragma unroll
        for (int c = 0; c < C; ++c) dst[sh + fl * C + c] = y.e[c];
      } else if (tile_full) {
        MAVG_DCHECK(f >= 0 && f + F <= nframes, "cascade output index", f, nframes);
        IO::template gstore<(NT & kNtStore) != 0>(out + f * C, y, eio);
      } else {
#pragma unroll
        for (int fr = 0; fr < F; ++fr)
          if (f + fr < nframes)
#pragma unroll
            for (int c = 0; c < C; ++c) out[(f + fr) * C + c] = y.e[fr * C + c];
      }
    }
    __syncthreads();

    if constexpr (F == 1) {
      if (last) {
        // dst[sh .. sh + E) -> out[t0*C .. t0*C + E): 16-B stores on the aligned interior, element
        // stores at the two ends
        const int tl = tile_full ? TF : (int)(nframes - t0);
        const int E = tl * C;
        const int S = sh + E;
        const long long o0 = t0 * C;
        MAVG_DCHECK(S <= stage_elems, "cascade output stage", S, stage_elems);
        T* const gbase = out + (o0 - sh);      // 16-B aligned; only [sh, S) of it is touched
        for (int e0 = tid * EPV; e0 < S; e0 += WG * EPV) {
          if (e0 >= sh && e0 + EPV <= S) {
            MAVG_DCHECK(o0 - sh + e0 >= 0 && o0 - sh + e0 + EPV <= nframes * C, "cascade output index", o0 - sh + e0, E);
            const u32x4 r = *reinterpret_cast<const u32x4*>(dst + e0);
            if constexpr ((NT & kNtStore) != 0) __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(gbase + e0));
            else *reinterpret_cast<u32x4*>(gbase + e0) = r;
          } else {
            const int lo = e0 > sh ? e0 : sh;
            const int hi = e0 + EPV < S ? e0 + EPV : S;
            for (int e = lo; e < hi; ++e) {
              MAVG_DCHECK(o0 - sh + e >= 0 && o0 - sh + e < nframes * C, "cascade output index", o0 - sh + e, E);
              gbase[e] = dst[e];
            }
          }
        }
      }
    }
  }
}

}  // namespace mavg
