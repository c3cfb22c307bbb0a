// mavg_extrema.hpp -- the moving maximum and minimum (mavg_extrema_run): per channel the largest
// and the smallest sample of the causal k-frame window, in the input's dtype, in one launch.
//   extrema_tile_kernel   the tile scan's tiles and halo, combined in three levels: suffix and
//                         prefix extrema inside a lane's unit, a doubling table over the unit
//                         totals, one shifted read -- O(log k) steps per UNIT, O(1) per frame
//   extrema_strip_kernel  one thread per (strip of L frames, channel): a backward walk that parks
//                         the suffix extrema in the outputs, then a forward prefix -- every shape
//                         the tile kernel does not take
// A maximum has no inverse, so the x[n] - x[n-k] scan of the averaging kernels does not apply.
// Frames before frame 0 (no history) and frames past the signal enter as copies of the nearest
// frame of the signal (ext_load_elem): every window that reaches them holds that frame too, so
// they change neither extremum -- the window is, in effect, truncated at frame 0.
#pragma once

#include "mavg_device.hpp"

namespace mavg {

// M: the outputs of an instance
constexpr int kExtMax = 1, kExtMin = 2, kExtBoth = 3;

template <bool MAX>
__device__ __forceinline__ float ext_op(float a, float b) { return MAX ? __builtin_fmaxf(a, b) : __builtin_fminf(a, b); }
template <bool MAX>
__device__ __forceinline__ int16_t ext_op(int16_t a, int16_t b) { return MAX ? (a > b ? a : b) : (a < b ? a : b); }
// mx is a constant after unrolling over the outputs
template <typename T>
__device__ __forceinline__ T ext_sel(bool mx, T a, T b) { return mx ? ext_op<true>(a, b) : ext_op<false>(a, b); }

// Guarded element access for an extremum: frames < 0 come from the history; without one, and
// before it, they are copies of the first frame there is; frames >= nframes copy the last.
template <typename T>
__device__ __forceinline__ T ext_load_elem(const T* __restrict__ in, const T* __restrict__ hist, long long f, int c,
                                           int C, long long nframes, int k) {
  if (f >= nframes) f = nframes - 1;
  if (f >= 0) return in[f * C + c];
  if (hist != nullptr && k > 1) {
    long long g = f + (k - 1);
    if (g < 0) g = 0;
    return hist[g * C + c];
  }
  return in[c];
}

struct ExtremaParams {
  const void* in;
  void* omax;        // or NULL (M decides which are written)
  void* omin;
  const void* hist;  // k - 1 frames in front of `in`, or NULL
  long long nframes;
  long long ntiles;
  int k;
  int halo_units;    // ceil(k / F): units staged before the tile
  int s_off;         // (-(k-1)*C) mod VE: where the window's first frame lies in its unit
  int span;          // whole units between the window's first unit and the lane's own (F == 1: k)
  int levels;        // floor(log2 span): the doubling table's last level; -1: span == 0
  int xcd_remap;     // remap_tile mode
  int eio;           // frame-unit launch on an element-aligned input (UnitIO::gload)
};

// The dynamic LDS of one workgroup, as byte offsets, per output o < nout: the suffix extrema S of
// the units a window of this tile can start in (stage units 0 .. U * WG; none for F == 1, where a
// unit is a frame), then the table R of unit extrema, [halo + tile units][C].  Read by the kernel,
// the launcher and the fit check.
template <typename T, int C, int F, int U, int WG>
struct ExtremaLds {
  static constexpr int VE = F * C;
  size_t s_units, r_units, s_bytes, r_bytes, bytes;
  int nout;
  __host__ __device__ constexpr ExtremaLds(size_t halo_units, int nout_)
      : s_units(F > 1 ? (size_t)U * WG + 1 : 0),
        r_units(halo_units + (size_t)U * WG),
        s_bytes((s_units * VE * sizeof(T) + 15) & ~(size_t)15),
        r_bytes((r_units * C * sizeof(T) + 15) & ~(size_t)15),
        bytes((size_t)nout_ * (s_bytes + r_bytes)),
        nout(nout_) {}
  __host__ __device__ constexpr size_t s(int o) const { return (size_t)o * s_bytes; }
  __host__ __device__ constexpr size_t r(int o) const { return (size_t)nout * s_bytes + (size_t)o * r_bytes; }
};

// the longest halo the tile kernel takes, (k - 1) * C * sizeof(T) bytes (the dispatch rule's bound)
constexpr long long kExtMaxHaloBytes = 16384;
// table elements a thread owns at the longest halo: ceil((halo units + tile units) * C / WG)
template <typename T, int C, int F, int U, int WG>
constexpr int ext_table_slots() {
  const long long km = kExtMaxHaloBytes / (C * (long long)sizeof(T)) + 1;  // the longest window
  const long long hu = (km + F - 1) / F;
  return (int)(((hu + (long long)U * WG) * C + WG - 1) / WG);
}

// ----------------------------------------------------------------------------
// extrema_tile_kernel: stat_tile_kernel's tiles, remap_tile, split non-temporal load policy and
// two forms (16-B units of F frames; F == 1 for views off 16-B alignment).  Lane tid owns units
// u * WG + tid of the tile; the halo's ceil(k / F) units are spread over the workgroup.  With
// k - 1 = qq F + rr, the window of frame fr of stage unit s starts in unit s - qq (fr >= rr) or
// s - qq - 1 (fr < rr), so it is the extremum of
//   1. the suffix of its first unit from its first frame: S, one shifted 16-B read (extract);
//   2. for fr < rr the whole unit s - qq: S at that unit's first frame (the same read's upper half);
//   3. the span = qq - 1 whole units s - qq + 1 .. s - 1: two overlapping entries of the doubling
//      table R_p, R_p[i] = extremum of units i - 2^p + 1 .. i, p = floor(log2 span);
//   4. the prefix of its own unit up to fr: registers.
// R_p is built in place from the unit extrema in ceil(p / 2) steps of radix 4 (one of radix 2 when
// p is odd), each thread keeping its entries in registers: two barriers a step.  k <= F (qq == 0):
// frames fr >= rr take their window from the lane's own registers.  F == 1: the window is the
// span = k units s - k + 1 .. s, term 3 alone.  Every output is a copy of an input sample.
// Frame and sample indices are 64-bit wherever they are not tile-local.
// ----------------------------------------------------------------------------
template <typename T, int C, int F, int U, int M, int WG = kWG, int NT = kNtSplit | kNtHalo | kNtStore>
__global__ __launch_bounds__(WG) void extrema_tile_kernel(ExtremaParams p) {
  static_assert(M >= kExtMax && M <= kExtBoth, "max, min or both");
  constexpr int NO = M == kExtBoth ? 2 : 1;   // outputs; output 0 is the maximum when M has it
  constexpr int VE = F * C;
  constexpr int TF = WG * F * U;              // tile frames
  constexpr int NI = ext_table_slots<T, C, F, U, WG>();
  using IO = UnitIO<T, VE>;
  using U_t = Unit<T, VE>;
  using Lds = ExtremaLds<T, C, F, U, WG>;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Hu = p.halo_units;
  const int Ha = Hu * F;                      // staged halo frames (>= k)
  const Lds lds((size_t)Hu, NO);
  const int NU = Hu + U * WG;                 // stage units
  const int NE = NU * C;                      // table elements per output
  [[maybe_unused]] const int SE = (int)lds.s_units * VE;
  T* S[NO];
  T* R[NO];
#pragma unroll
  for (int o = 0; o < NO; ++o) {
    S[o] = reinterpret_cast<T*>(smem + lds.s(o));
    R[o] = reinterpret_cast<T*>(smem + lds.r(o));
  }
  MAVG_DCHECK(lds.bytes <= lds_budget(WG) && Ha >= p.k && (NE + WG - 1) / WG <= NI, "extrema LDS layout", lds.bytes, Hu);

  const T* __restrict__ in = static_cast<const T*>(p.in);
  const T* __restrict__ hist = static_cast<const T*>(p.hist);
  T* __restrict__ outp[NO];
  outp[0] = static_cast<T*>((M & kExtMax) ? p.omax : p.omin);
  if constexpr (NO == 2) outp[1] = static_cast<T*>(p.omin);
  const int tid = threadIdx.x;
  const int k = p.k;
  const long long nframes = p.nframes;
  const bool eio = F == 1 && p.eio != 0;

  const long long tile = remap_tile(blockIdx.x, gridDim.x, p.xcd_remap);
  const long long t0 = tile * TF;
  const long long h0 = t0 - Ha;               // first staged halo frame
  MAVG_DCHECK(tile >= 0 && tile < p.ntiles && t0 < nframes, "extrema tile index", tile, p.ntiles);
  const bool tile_full = (t0 + TF <= nframes);

  // a unit's suffix extrema -> S (where a window of this tile can start), its extrema -> R
  auto emit = [&](int s, const U_t& xu) {
    MAVG_DCHECK(s >= 0 && s < NU, "extrema stage unit", s, NU);
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const bool mx = (M & kExtMax) != 0 && o == 0;
      U_t sf;
      T run[C];
#pragma unroll
      for (int fr = F - 1; fr >= 0; --fr)
#pragma unroll
        for (int c = 0; c < C; ++c) {
          run[c] = fr == F - 1 ? xu.e[fr * C + c] : ext_sel(mx, run[c], xu.e[fr * C + c]);
          sf.e[fr * C + c] = run[c];
        }
      if constexpr (F > 1) {
        if (s <= U * WG) {
          MAVG_DCHECK((s + 1) * VE <= SE, "extrema suffix stage index", s, SE);
          IO::store(S[o] + s * VE, sf);
        }
      }
#pragma unroll
      for (int c = 0; c < C; ++c) R[o][s * C + c] = run[c];
    }
  };

  // ---- tile -> registers (thread tid takes units u * WG + tid: coalesced); halo; both -> LDS ----
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
        for (int c = 0; c < C; ++c) x[u].e[fr * C + c] = ext_load_elem(in, hist, f + fr, c, C, nframes, k);
    }
  }
  {
    const bool halo_fast = h0 >= 0;            // re-read of the previous tile's tail: L2
    for (int j = tid; j < Hu; j += WG) {
      const long long f = h0 + (long long)j * F;
      U_t h;
      if (halo_fast) {
        h = IO::template gload<(NT & kNtHalo) != 0>(in + f * C, eio);
      } else {
#pragma unroll
        for (int fr = 0; fr < F; ++fr)
#pragma unroll
          for (int c = 0; c < C; ++c) h.e[fr * C + c] = ext_load_elem(in, hist, f + fr, c, C, nframes, k);
      }
      emit(j, h);
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) emit(Hu + u * WG + tid, x[u]);
  __syncthreads();

  // ---- the doubling table, in place: thread tid owns elements tid + i * WG ----
  if (p.levels > 0) {
    T own[NO][NI];
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const int e = tid + i * WG;
        own[o][i] = e < NE ? R[o][e] : (T)0;
      }
    for (int lvl = 0; lvl < p.levels;) {
      const int rad = p.levels - lvl >= 2 ? 3 : 1;   // partners: radix 4 or 2
      const int dC = (1 << lvl) * C;
      if (lvl > 0) __syncthreads();                  // the previous step's writes
#pragma unroll
      for (int o = 0; o < NO; ++o) {
        const bool mx = (M & kExtMax) != 0 && o == 0;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int e = tid + i * WG;
          if (e < NE) {
#pragma unroll
            for (int q = 1; q <= 3; ++q) {
              const int pe = e - q * dC;
              if (q <= rad && pe >= 0) own[o][i] = ext_sel(mx, own[o][i], R[o][pe]);
            }
          }
        }
      }
      __syncthreads();                               // every read of this step
#pragma unroll
      for (int o = 0; o < NO; ++o)
#pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int e = tid + i * WG;
          if (e < NE) R[o][e] = own[o][i];
        }
      lvl += rad == 3 ? 2 : 1;
    }
    __syncthreads();
  }

  // ---- outputs ----
  const int wspan = p.levels >= 0 ? (1 << p.levels) : 0;
  const int rr = (k - 1) % F;
  const bool in_unit = F > 1 && k - 1 < F;           // qq == 0
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = u * WG + tid;
    const int s = Hu + j;
    const long long f = t0 + (long long)j * F;
    U_t y[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) {
      const bool mx = (M & kExtMax) != 0 && o == 0;
      // term 3: the whole units (F == 1: the window itself)
      T base[C];
#pragma unroll
      for (int c = 0; c < C; ++c) base[c] = x[u].e[c];
      const int hi = F == 1 ? s : s - 1;
      if (p.levels >= 0) {
        const int lo2 = hi - p.span + wspan;         // the entry whose range starts the span
        MAVG_DCHECK(lo2 - wspan + 1 >= 0 && lo2 <= hi && hi < NU, "extrema table index", lo2, hi);
#pragma unroll
        for (int c = 0; c < C; ++c) base[c] = ext_sel(mx, R[o][hi * C + c], R[o][lo2 * C + c]);
      }
      if constexpr (F == 1) {
#pragma unroll
        for (int c = 0; c < C; ++c) y[o].e[c] = base[c];
      } else {
        // terms 1 and 2: S at the window's first frame (two aligned units and a uniform shift)
        const int e = (s * F - (k - 1)) * C;
        U_t sv;
        T whole[C];                                  // term 2 (rr > 0 only)
        if (p.s_off == 0) {
          MAVG_DCHECK(e >= 0 && e + VE <= SE, "extrema suffix read", e, j);
          sv = IO::load(S[o] + e);
#pragma unroll
          for (int c = 0; c < C; ++c) whole[c] = sv.e[c];
        } else {
          const int e_lo = e - p.s_off;
          MAVG_DCHECK(e_lo >= 0 && e_lo + 2 * VE <= SE, "extrema suffix extraction", e_lo, j);
          const U_t a = IO::load_whole(S[o] + e_lo);
          const U_t b = IO::load_whole(S[o] + e_lo + VE);
          sv = extract(a, b, p.s_off);
#pragma unroll
          for (int c = 0; c < C; ++c) whole[c] = b.e[c];
        }
        T run[C];
#pragma unroll
        for (int fr = 0; fr < F; ++fr)
#pragma unroll
          for (int c = 0; c < C; ++c) {
            const T xv = x[u].e[fr * C + c];
            run[c] = fr == 0 ? xv : ext_sel(mx, run[c], xv);   // term 4
            T v;
            if (in_unit && fr >= rr) {
              v = xv;                                // the window lies in this unit
#pragma unroll
              for (int d = 1; d < F; ++d)
                if (d <= fr && d <= rr) v = ext_sel(mx, v, x[u].e[(fr - d) * C + c]);
            } else {
              v = ext_sel(mx, run[c], sv.e[fr * C + c]);
              if (p.levels >= 0) v = ext_sel(mx, v, base[c]);
              if (!in_unit && fr < rr) v = ext_sel(mx, v, whole[c]);
            }
            y[o].e[fr * C + c] = v;
          }
      }
    }
    if (F > 1 && tile_full) {
      MAVG_DCHECK(f >= 0 && f + F <= nframes, "extrema output index", f, nframes);
#pragma unroll
      for (int o = 0; o < NO; ++o) IO::template store<(NT & kNtStore) != 0>(outp[o] + f * C, y[o]);
    } else {
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
        if (f + fr < nframes) {
          MAVG_DCHECK(f + fr >= 0, "extrema output index", f + fr, nframes);
#pragma unroll
          for (int o = 0; o < NO; ++o)
#pragma unroll
            for (int c = 0; c < C; ++c) outp[o][(f + fr) * C + c] = y[o].e[fr * C + c];
        }
    }
  }
}

// ----------------------------------------------------------------------------
// extrema_strip_kernel: correct, not fast -- any channels, any grade, a history, any sample-aligned
// views.  Thread t takes channel t % C of the strip of L consecutive frames t / C.  Windows of at
// most kExtDirectMax frames are evaluated directly.  Longer ones (L <= k - 1 then): the window of
// frame n of the strip is the frames n - k + 1 .. f0 - 1 before the strip and the strip's f0 .. n.
// The thread walks backwards from f0 - 1 over k - 1 frames with a running extremum and parks the
// value reached at frame n - k + 1 in out[n] (it alone owns those outputs), then walks forward
// with a running prefix extremum and combines the two: about k / L + 2 reads per output.
// ----------------------------------------------------------------------------
constexpr int kExtDirectMax = 16;

struct ExtStripParams {
  const void* in;
  void* omax;
  void* omin;
  const void* hist;
  long long nframes;
  long long nstrips;
  int C;
  int k;
  int L;
};

template <typename T, int WG = kWG>
__global__ __launch_bounds__(WG) void extrema_strip_kernel(ExtStripParams p) {
  const T* __restrict__ in = static_cast<const T*>(p.in);
  const T* __restrict__ hist = static_cast<const T*>(p.hist);
  T* const omax = static_cast<T*>(p.omax);
  T* const omin = static_cast<T*>(p.omin);
  const int C = p.C;
  const int k = p.k;
  const long long t = (long long)blockIdx.x * WG + threadIdx.x;
  const long long strip = t / C;
  const int c = (int)(t - strip * C);
  if (strip >= p.nstrips) return;
  const long long f0 = strip * p.L;
  const long long f1 = f0 + p.L < p.nframes ? f0 + p.L : p.nframes;
  MAVG_DCHECK(f0 >= 0 && f0 < p.nframes && f1 <= p.nframes, "extrema strip index", strip, p.nstrips);
  if (k <= kExtDirectMax) {
    for (long long f = f0; f < f1; ++f) {
      T hi = in[f * C + c], lo = hi;
      for (long long g = f - k + 1; g < f; ++g) {
        const T xv = ext_load_elem(in, hist, g, c, C, p.nframes, k);
        hi = ext_op<true>(hi, xv);
        lo = ext_op<false>(lo, xv);
      }
      if (omax != nullptr) omax[f * C + c] = hi;
      if (omin != nullptr) omin[f * C + c] = lo;
    }
    return;
  }
  MAVG_DCHECK(p.L <= k - 1, "extrema strip length", p.L, k);
  {
    T hi = ext_load_elem(in, hist, f0 - 1, c, C, p.nframes, k), lo = hi;
    for (long long g = f0 - 1; g >= f0 - (k - 1); --g) {
      const T xv = ext_load_elem(in, hist, g, c, C, p.nframes, k);
      hi = ext_op<true>(hi, xv);
      lo = ext_op<false>(lo, xv);
      const long long n = g + (k - 1);            // the frame whose window starts at g
      if (n < f1) {
        MAVG_DCHECK(n >= f0, "extrema parked index", n, f0);
        if (omax != nullptr) omax[n * C + c] = hi;
        if (omin != nullptr) omin[n * C + c] = lo;
      }
    }
  }
  T hi = in[f0 * C + c], lo = hi;
  for (long long f = f0; f < f1; ++f) {
    const T xv = in[f * C + c];
    hi = ext_op<true>(hi, xv);
    lo = ext_op<false>(lo, xv);
    MAVG_DCHECK(f * C + c < p.nframes * C, "extrema output index", f, p.nframes);
    if (omax != nullptr) omax[f * C + c] = ext_op<true>(omax[f * C + c], hi);
    if (omin != nullptr) omin[f * C + c] = ext_op<false>(omin[f * C + c], lo);
  }
}

}  // namespace mavg
