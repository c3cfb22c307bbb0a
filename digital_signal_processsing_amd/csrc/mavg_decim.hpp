// mavg_decim.hpp -- the decimated moving average (mavg_decim_run): only the full-rate output
// frames phase + m * hop are produced, packed.  Three kernels:
//   decim_scan_kernel    the flat tile scan (mavg_tile.hpp, the register-staged Blelloch flavour)
//                        with a compacting end: dense reading, 1/hop of the stores
//   decim_window_kernel  one wave per output frame sums that frame's window: sparse reading
//   decim_gather_kernel  the strided gather behind the full-rate fallback (decim_full)
#pragma once

#include "mavg_device.hpp"

namespace mavg {

struct DecimParams {
  const void* in;
  void* out;
  const void* hist;
  long long nframes;
  long long ntiles;
  long long out_frames;  // M = len(range(phase, nframes, hop))
  int k;
  int halo_units;        // ceil(k / F): units staged before the tile
  int xk_off;            // (-k*C) mod VE
  int xcd_remap;         // remap_tile mode
  int eio;               // frame-unit launch on an element-aligned input (UnitIO::gload)
  int hop;
  int phase;
  OutParams o;
};

// ----------------------------------------------------------------------------
// Which frames of a tile are kept, and where they go.  The tile holds frames
// [t0, t0 + tl), tl <= TF; kept frames are phase + m * hop.  Once per workgroup,
// uniform: the first kept index m_lo at or after t0 (one 64-bit divide), the
// tile-local index l0 of that frame (TF when it lies past the tile) and the
// number of kept frames cnt (a 32-bit divide).  The tile's outputs are
// out[m_lo .. m_lo + cnt); the next tile's m_lo is this one's m_lo + cnt.
// Then every lane, in 32-bit arithmetic: a unit's first frame i0 gives the first
// kept frame at or after it and that frame's slot (decim_first); walking the
// unit's F frames, a frame equal to `first` is kept at `slot`, and first += hop.
// tests/test_decim_model.py restates both steps.
// ----------------------------------------------------------------------------
struct DecimRange {
  long long m_lo;
  uint32_t l0, cnt;
};
__host__ __device__ inline DecimRange decim_tile_range(long long t0, uint32_t tl, uint32_t TF, uint32_t hop,
                                                       uint32_t phase) {
  DecimRange r;
  r.m_lo = t0 > (long long)phase ? (t0 - (long long)phase + (long long)hop - 1) / (long long)hop : 0;
  const long long d = (long long)phase + r.m_lo * (long long)hop - t0;  // >= 0
  r.l0 = d < (long long)TF ? (uint32_t)d : TF;
  r.cnt = r.l0 < tl ? (tl - r.l0 + hop - 1u) / hop : 0u;
  return r;
}
__host__ __device__ inline void decim_first(uint32_t i0, uint32_t l0, uint32_t hop, uint32_t& first, uint32_t& slot) {
  if (i0 <= l0) {
    slot = 0;
    first = l0;
  } else {
    slot = (i0 - l0 + hop - 1u) / hop;
    first = l0 + slot * hop;
  }
}

// The dynamic LDS of one workgroup, as byte offsets: the tile scan's stage (halo, tile, one pad
// unit), [NSEG][C] segment totals, [NW][C] halo partial sums, then the compaction buffer: at most
// TF/2 + 1 kept frames (hop >= 2) plus one 16-B vector of lead-in, so that a kept sample's place
// in the buffer has the 16-B phase of its place in the output.
template <typename T, typename A, int C, int F, int U, int WG>
struct DecimLds {
  static constexpr int NW = WG / 64;
  static constexpr int NSEG = U * NW;
  static constexpr int TF = WG * F * U;
  static constexpr int EPV = 16 / (int)sizeof(T);
  static constexpr int kCapFrames = TF / 2 + 1;
  static constexpr int kCbufElems = kCapFrames * C + EPV;
  size_t stage_units;
  size_t tot, hsum, cbuf, bytes;
  __host__ __device__ constexpr explicit DecimLds(size_t halo_units)
      : stage_units(halo_units + (size_t)U * WG + 1),
        tot(((stage_units * F * C * sizeof(T)) + 15) & ~(size_t)15),
        hsum(tot + (size_t)NSEG * C * sizeof(A)),
        cbuf((hsum + (size_t)NW * C * sizeof(A) + 15) & ~(size_t)15),
        bytes(cbuf + (((size_t)kCbufElems * sizeof(T) + 15) & ~(size_t)15)) {}
};

// ----------------------------------------------------------------------------
// decim_scan_kernel: tile_scan_kernel's non-DMA Blelloch body -- the same tiles and remap_tile,
// the split non-temporal load policy, halo and tile staged in LDS, history through load_elem, the
// same in-lane, wave and segment scan order and the same to_out -- up to the outputs.  There only
// the kept frames are converted, into the LDS compaction buffer; after a third barrier the
// workgroup stores out[m_lo*C .. (m_lo+cnt)*C) contiguously: 16-B stores on the aligned interior,
// element stores at the two ends.  A tile that keeps no frame (hop > TF) returns before it loads.
// Frame and sample indices are 64-bit wherever they are not tile-local; tested on 2^32 +
// 10^6-sample signals (tests/test_gpu_bigsignal.py).
// ----------------------------------------------------------------------------
template <typename T, typename A, int C, int F, int U, int WG = kWG, int NT = kNtSplit | kNtHalo | kNtStore, int DV = 0>
__global__ __launch_bounds__(WG) void decim_scan_kernel(DecimParams p) {
  constexpr int NW = WG / 64;
  constexpr int VE = F * C;
  constexpr int TF = WG * F * U;           // tile frames
  constexpr int NSEG = U * NW;
  static_assert(NSEG <= 64, "segment totals are scanned across one wave");
  using IO = UnitIO<T, VE>;
  using U_t = Unit<T, VE>;
  using Lds = DecimLds<T, A, C, F, U, WG>;
  constexpr int EPV = Lds::EPV;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Hu = p.halo_units;
  const int Ha = Hu * F;                     // staged halo frames (>= k)
  const Lds lds((size_t)Hu);
  T* stage = reinterpret_cast<T*>(smem);     // [Hu + U*WG + 1 pad] units
  A* tot = reinterpret_cast<A*>(smem + (int)lds.tot);    // [NSEG][C] segment totals
  A* hsum = reinterpret_cast<A*>(smem + (int)lds.hsum);  // [NW][C] halo partial sums
  T* cbuf = reinterpret_cast<T*>(smem + (int)lds.cbuf);  // [kCbufElems] kept samples, in output order

  const T* __restrict__ in = static_cast<const T*>(p.in);
  T* __restrict__ out = static_cast<T*>(p.out);
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
  MAVG_DCHECK(tile >= 0 && tile < p.ntiles && t0 < nframes, "decim tile index", tile, p.ntiles);
  MAVG_DCHECK(lds.bytes <= lds_budget(WG), "decim LDS layout", lds.bytes, Hu);
  const bool tile_full = (t0 + TF <= nframes);

  // ---- the tile's outputs (uniform) ----
  const uint32_t hop = (uint32_t)p.hop;
  const uint32_t tl = tile_full ? (uint32_t)TF : (uint32_t)(nframes - t0);
  const DecimRange rg = decim_tile_range(t0, tl, (uint32_t)TF, hop, (uint32_t)p.phase);
  const uint32_t l0 = rg.l0, cnt = rg.cnt;
  if (cnt == 0) return;                      // no kept frame in this tile (uniform: before any barrier)
  MAVG_DCHECK(cnt <= (uint32_t)Lds::kCapFrames && rg.m_lo + (long long)cnt <= p.out_frames, "decim tile outputs", cnt,
              rg.m_lo);
  const long long o0 = rg.m_lo * C;          // first output sample of the tile
  // the 16-B phase of out + o0, in samples: kept sample e lives at cbuf[sh + e]
  const int sh = (int)(((reinterpret_cast<uintptr_t>(out) / sizeof(T)) + (unsigned long long)o0) & (unsigned)(EPV - 1));

  // ---- tile -> registers -> LDS ----
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
  {
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
  }
#pragma unroll
  for (int u = 0; u < U; ++u) IO::store(stage + (Hu + u * WG + tid) * VE, x[u]);
  if (tid == 0) {
    U_t z;
#pragma unroll
    for (int i = 0; i < VE; ++i) z.e[i] = (T)0;
    IO::store(stage + (Hu + U * WG) * VE, z);   // pad unit (k < F reads one unit past the tile)
  }
  __syncthreads();

  // ---- halo reduction: W[t0-1] = sum of the k frames before t0 ----
  {
    A hs[C];
#pragma unroll
    for (int c = 0; c < C; ++c) hs[c] = (A)0;
    for (int i = Ha - k + tid; i < Ha; i += WG)
#pragma unroll
      for (int c = 0; c < C; ++c) hs[c] += to_acc<A>(stage[i * C + c]);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const A r = readlane(wave_incl_scan(hs[c]), 63);
      if (lane == 0) hsum[w * C + c] = r;
    }
  }

  // x[n-k] for lane unit j, from the LDS stage (an unaligned x[n-k]: two
  // aligned units and a uniform shift)
  auto stage_xk = [&](int j) -> U_t {
    const int e = (Ha + j * F - k) * C;
    U_t xk;
    if constexpr (IO::kVec) {
      if (p.xk_off == 0) {
        MAVG_DCHECK(e >= 0 && e + VE <= (int)lds.stage_units * VE, "decim x[n-k] stage index", e, j);
        xk = IO::load(stage + e);
      } else {
        const int e_lo = e - p.xk_off;
        MAVG_DCHECK(e_lo >= 0 && e_lo + 2 * VE <= (int)lds.stage_units * VE, "decim x[n-k] extraction", e_lo, j);
        U_t a = IO::load_whole(stage + e_lo);
        U_t b = IO::load_whole(stage + e_lo + VE);
        xk = extract(a, b, p.xk_off);
      }
    } else {
      MAVG_DCHECK(e >= 0 && e + VE <= (int)lds.stage_units * VE, "decim x[n-k] stage index", e, j);
#pragma unroll
      for (int i = 0; i < VE; ++i) xk.e[i] = stage[e + i];
    }
    return xk;
  };

  // ---- d = x - x[n-k]; in-lane, wave and segment scans ----
  A v[U][F][C];            // in-lane prefixes
  A lx[U][C];              // exclusive prefix of the lane totals inside the wave
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = u * WG + tid;
    const U_t xk = stage_xk(j);
#pragma unroll
    for (int fr = 0; fr < F; ++fr)
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const A d = to_acc<A>(x[u].e[fr * C + c]) - to_acc<A>(xk.e[fr * C + c]);
        v[u][fr][c] = fr == 0 ? d : v[u][fr - 1][c] + d;
      }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const A run = v[u][F - 1][c];
      const A incl = wave_incl_scan(run);
      lx[u][c] = incl - run;
      const A segtot = readlane(incl, 63);
      if (lane == 0) tot[(u * NW + w) * C + c] = segtot;
    }
  }
  __syncthreads();

  // ---- carry: halo sum + earlier segments ----
  const int wu = __builtin_amdgcn_readfirstlane(w);
  A base[U][C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    A w0 = (A)0;
#pragma unroll
    for (int i = 0; i < NW; ++i) w0 += hsum[i * C + c];
    const A tv = lane < NSEG ? tot[lane * C + c] : (A)0;
    const A ex = wave_incl_scan(tv) - tv;
#pragma unroll
    for (int u = 0; u < U; ++u) base[u][c] = w0 + readlane(ex, u * NW + wu);
  }

  // ---- kept frames -> the compaction buffer ----
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const uint32_t i0 = (uint32_t)((u * WG + tid) * F);
    uint32_t first, slot;
    decim_first(i0, l0, hop, first, slot);
#pragma unroll
    for (int fr = 0; fr < F; ++fr) {
      const uint32_t i = i0 + (uint32_t)fr;
      if (i == first && i < tl) {
        MAVG_DCHECK(slot < cnt && i >= l0 && (i - l0) % hop == 0, "decim slot", slot, cnt);
#pragma unroll
        for (int c = 0; c < C; ++c)
          cbuf[sh + (int)slot * C + c] = to_out<T, A, DV>(base[u][c] + lx[u][c] + v[u][fr][c], p.o);
        first += hop;
        ++slot;
      }
    }
  }
  __syncthreads();

  // ---- the tile's outputs, contiguous: cbuf[sh .. sh + E) -> out[o0 .. o0 + E) ----
  {
    const int E = (int)cnt * C;
    const int S = sh + E;
    MAVG_DCHECK(S <= Lds::kCbufElems, "decim compaction buffer", S, Lds::kCbufElems);
    T* const gbase = out + (o0 - sh);          // 16-B aligned; only [sh, S) of it is touched
    for (int e0 = tid * EPV; e0 < S; e0 += WG * EPV) {
      if (e0 >= sh && e0 + EPV <= S) {
        MAVG_DCHECK(o0 - sh + e0 >= 0 && o0 - sh + e0 + EPV <= p.out_frames * C, "decim output index", o0 - sh + e0, E);
        const u32x4 r = *reinterpret_cast<const u32x4*>(cbuf + e0);
        if constexpr ((NT & kNtStore) != 0) __builtin_nontemporal_store(r, reinterpret_cast<u32x4*>(gbase + e0));
        else *reinterpret_cast<u32x4*>(gbase + e0) = r;
      } else {
        const int lo = e0 > sh ? e0 : sh;
        const int hi = e0 + EPV < S ? e0 + EPV : S;
        for (int e = lo; e < hi; ++e) {
          MAVG_DCHECK(o0 - sh + e >= 0 && o0 - sh + e < p.out_frames * C, "decim output index", o0 - sh + e, E);
          gbase[e] = cbuf[e];
        }
      }
    }
  }
}

// ----------------------------------------------------------------------------
// decim_window_kernel: one wave per output frame m, four per 256-thread workgroup.  The wave sums
// the k frames [f - k + 1, f], f = phase + m * hop, each read once: lanes stride over the window,
// a lane takes all C channels of its frames.  Where a frame divides 16 B (VF = 16 / frame bytes)
// and the input is 16-B aligned (p.eio == 0), the window's aligned interior moves as 16-B loads of
// VF frames per lane; the frames before and after it -- and the frames before 0 (history or zero)
// and past the end -- go through load_elem, one frame per lane.  Sums in fp64 (fp32 data) or int64
// (int16 data): exact for every grade.  wave_incl_scan's last lane holds the total; lane 0 stores
// the C samples.
// ----------------------------------------------------------------------------
template <typename T, typename A, int C, int WG = kWG>
__global__ __launch_bounds__(WG) void decim_window_kernel(DecimParams p) {
  constexpr int FB = C * (int)sizeof(T);
  constexpr int VF = (FB <= 16 && 16 % FB == 0) ? 16 / FB : 0;   // frames per 16-B load (0: none)
  const T* __restrict__ in = static_cast<const T*>(p.in);
  T* __restrict__ out = static_cast<T*>(p.out);
  const T* __restrict__ hist = static_cast<const T*>(p.hist);
  const int lane = threadIdx.x & 63;
  const long long m = (long long)blockIdx.x * (WG / 64) + (threadIdx.x >> 6);   // wave-uniform
  if (m >= p.out_frames) return;
  const int k = p.k;
  const long long nframes = p.nframes;
  const long long f1 = (long long)p.phase + m * (long long)p.hop + 1;  // one past the window's last frame
  // its first frame: before 0 only with a history to read there (zero history adds nothing)
  const long long f0 = (hist == nullptr && f1 < k) ? 0 : f1 - k;
  MAVG_DCHECK(f1 >= 1 && f1 <= nframes, "decim window frame", f1, nframes);

  A acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = (A)0;
  auto frames_by_elem = [&](long long a, long long b) {  // frames [a, b), one per lane
    for (long long f = a + lane; f < b; f += 64)
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += to_acc<A>(load_elem(in, hist, f, c, C, nframes, k, 0));
  };
  long long a0 = f0, a1 = f0;  // the 16-B interior [a0, a1): empty unless the vector form applies
  if constexpr (VF > 0) {
    if (p.eio == 0) {
      const long long lo = f0 > 0 ? f0 : 0;
      a0 = (lo + VF - 1) / VF * VF;
      a1 = f1 / VF * VF;
      if (a1 < a0) a1 = a0;
    }
  }
  if (a1 > a0) {
    frames_by_elem(f0, a0);
    if constexpr (VF > 0) {
      using IO = UnitIO<T, VF * C>;
#pragma unroll 4
      for (long long f = a0 + (long long)lane * VF; f < a1; f += 64 * VF) {
        MAVG_DCHECK(f >= 0 && f + VF <= nframes, "decim window load", f, nframes);
        const Unit<T, VF * C> u = IO::load(in + f * C);
#pragma unroll
        for (int fr = 0; fr < VF; ++fr)
#pragma unroll
          for (int c = 0; c < C; ++c) acc[c] += to_acc<A>(u.e[fr * C + c]);
      }
    }
    frames_by_elem(a1, f1);
  } else {
    frames_by_elem(f0, f1);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const A s = readlane(wave_incl_scan(acc[c]), 63);
    if (lane == 0) {
      MAVG_DCHECK(m * C + c < p.out_frames * C, "decim window output index", m, c);
      out[m * C + c] = to_out<T, A, 0>(s, p.o);
    }
  }
}

// ----------------------------------------------------------------------------
// decim_gather_kernel: out[m*C + c] = full[(phase + m*hop)*C + c], a grid-stride loop over the
// M*C output samples.  The fallback's second step: plain code, not tuned.
// ----------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kWG) void decim_gather_kernel(const T* __restrict__ full, T* __restrict__ out,
                                                           long long out_frames, long long nframes, int C, int hop,
                                                           int phase) {
  const long long n = out_frames * C;
  const long long step = (long long)gridDim.x * kWG;
  for (long long i = (long long)blockIdx.x * kWG + threadIdx.x; i < n; i += step) {
    const long long m = i / C;
    const int c = (int)(i - m * C);
    const long long f = (long long)phase + m * (long long)hop;
    MAVG_DCHECK(f >= 0 && f < nframes, "decim gather frame", f, nframes);
    out[i] = full[f * C + c];
  }
}

}  // namespace mavg
