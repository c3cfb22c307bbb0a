// mavg_segscan.hpp -- the segmented tile scan behind the two batch APIs: one
// scan body (seg_tile_scan) and the two row sources that tell it where rows
// start -- DenseRows (rows_scan_kernel: rows of one length, stored densely) and
// RaggedRows (ragged_scan_kernel: rows of different lengths, packed, with a CSR
// offsets array).
#pragma once

#include "mavg_device.hpp"

namespace mavg {

// ----------------------------------------------------------------------------
// The batch -- `rows` independent signals one after another -- is one flat
// stream of frames, cut into fixed tiles of T = WG*F*U frames exactly as
// tile_scan_kernel (mavg_tile.hpp) cuts a signal: 16-B lane units, the halo and
// the tile staged in LDS, the remap_tile XCD mapping, the split non-temporal
// policy, no inter-workgroup communication.  Tile boundaries ignore row
// boundaries, so every load and store of samples stays full-width whatever the
// row lengths are; a workgroup may hold hundreds of rows or a sliver of one.
//
// What the rows change: the scan is SEGMENTED.  With q = a frame's position
// inside its row,
//     d[n] = x[n] - (q >= k ? x[n-k] : 0)
//     W[n] = (q == 0 ? 0 : W[n-1]) + d[n]
// -- the in-lane scan, the wave scan (wave_seg_incl_scan) and the scan of the
// segment totals all reset at row starts, by selects on (flag, value) pairs;
// the halo sum covers only the min(k, q0) frames before the tile that belong
// to the row the tile continues (q0: the in-row position of the tile's first
// frame), and it and the earlier segments' totals are added only to frames
// with no row start at or before them in the tile.  No unsegmented prefix is
// ever formed, so nothing of another row enters a row's sums -- no rounding of
// a neighbour's magnitude, no Inf - Inf.
//
// The body needs two facts per frame, `start` (q == 0) and `has_xk` (q >= k),
// and one per tile, the halo frame count min(k, q0).  A row source supplies
// them, and nothing else:
//   lds_words   LDS words of its own behind the segment flags
//   prepare     once per workgroup, after the tile's global loads are issued and
//               before the halo is staged (it may hold a barrier of its own)
//   halo_frames min(k, q0), uniform, read after the stage barrier
//   walk        a lane unit's walker: frame() yields start and has_xk of the
//               unit's frames, one after another
//
// k is the EFFECTIVE window min(grade, longest row): with grade >= a row's
// length every position in it is < grade, x[n-k] is never used, and the stage
// only ever needs the row's own frames.  The divisor stays the grade (p.o).
// ----------------------------------------------------------------------------
struct SegParams {
  const void* in;
  void* out;
  long long nframes;     // the batch's frames
  long long ntiles;
  int k;                 // effective window: min(grade, longest row)
  int halo_units;        // ceil(k / F): units staged before the tile
  int xk_off;            // (-k*C) mod VE
  int xcd_remap;         // remap_tile mode
  int eio;               // frame-unit launch on element-aligned pointers (UnitIO::gload)
  OutParams o;           // of the grade (the divisor)
};
struct RowsParams : SegParams {
  long long row_frames;  // nframes = rows * row_frames
};
struct RaggedParams : SegParams {
  const long long* offsets;  // rows + 1 frame offsets, device memory; nframes = offsets[rows] (the host's copy)
  long long rows;
};

// The dynamic LDS of one workgroup, as byte offsets: the stage, [NSEG][C] segment totals,
// [NW][C] halo partial sums, [NSEG] segment flags, the row source's words.  The kernel, its
// layout check and the host's launch and dispatch all read it from here.
template <typename Src, typename T, typename A, int C, int F, int U, int WG>
struct SegLds {
  static constexpr int NW = WG / 64;
  static constexpr int NSEG = U * NW;
  size_t stage_units;  // halo + tile + 1 pad unit
  size_t tot, hsum, sflag, src, bytes;
  __host__ __device__ constexpr explicit SegLds(size_t halo_units)
      : stage_units(halo_units + (size_t)U * WG + 1),
        tot(((stage_units * F * C * sizeof(T)) + 15) & ~(size_t)15),
        hsum(tot + (size_t)NSEG * C * sizeof(A)),
        sflag(hsum + (size_t)NW * C * sizeof(A)),
        src(sflag + (size_t)NSEG * sizeof(int32_t)),
        bytes(src + Src::template lds_words<F, U, WG>(halo_units) * sizeof(uint32_t)) {}
};

// ----------------------------------------------------------------------------
// DenseRows: every row has row_frames frames, so a frame's position is its
// index modulo the row length -- without 64-bit divides: q0 = t0 mod row_frames
// once per workgroup (uniform), then every lane's position is 32-bit arithmetic
// (one 32-bit modulo per lane, increments with a conditional wrap after it).
// Rows longer than 2^30 frames are clamped: a tile then holds at most one row
// start and positions only matter while < k or == 0.
// ----------------------------------------------------------------------------
constexpr uint32_t kRowsPosClamp = 1u << 30;  // in-row positions are kept below this

struct DenseRows {
  using Params = RowsParams;
  template <int F, int U, int WG>
  static constexpr size_t lds_words(size_t) { return 0; }

  template <int F, int U, int WG>
  struct Tile {
    static_assert(F <= 16, "the per-lane row-start mask is 16 bits wide");
    uint32_t Lc, k;
    int hq;              // halo frames of the row the tile continues
    uint32_t pos[U];     // position of each unit's first frame

    __device__ __forceinline__ void prepare(const Params& p, uint32_t*, long long t0, int Ha, int tid) {
      constexpr int TF = WG * F * U;
      k = (uint32_t)p.k;
      const long long L = p.row_frames;
      MAVG_DCHECK((long long)p.k <= L, "rows effective window", p.k, L);
      const long long q0 = t0 % L;               // the one 64-bit divide, scalar
      uint32_t q0c;
      if (L <= (long long)kRowsPosClamp) {
        Lc = (uint32_t)L;
        q0c = (uint32_t)q0;
      } else {
        // at most one row start in the tile; positions matter only while < k or == 0
        const long long rem = L - q0;            // frames up to the next row start
        Lc = kRowsPosClamp;
        q0c = rem <= (long long)TF ? kRowsPosClamp - (uint32_t)rem
                                   : (uint32_t)(q0 < (long long)(kRowsPosClamp >> 1) ? q0 : (long long)(kRowsPosClamp >> 1));
      }
      hq = (int)(q0c < k ? q0c : k);
      const uint32_t pstep = (uint32_t)(WG * F) % Lc;
      pos[0] = (q0c + (uint32_t)(tid * F)) % Lc;
#pragma unroll
      for (int u = 1; u < U; ++u) {
        const uint32_t n = pos[u - 1] + pstep;
        pos[u] = n >= Lc ? n - Lc : n;
      }
#ifdef MAVG_DEBUG
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const long long q = (t0 + (long long)(u * WG + tid) * F) % L;
        MAVG_DCHECK((pos[u] == 0) == (q == 0) && (pos[u] < k) == (q < (long long)k), "rows position", pos[u], q);
      }
#endif
    }
    __device__ __forceinline__ int halo_frames() const { return hq; }

    struct Walker {
      uint32_t pp, Lc, k;
      __device__ __forceinline__ void frame(int, bool& start, bool& has_xk) {
        start = pp == 0;
        has_xk = pp >= k;
        pp = pp + 1 == Lc ? 0 : pp + 1;
      }
    };
    __device__ __forceinline__ Walker walk(int u, int) const { return Walker{pos[u], Lc, k}; }
  };
};

// ----------------------------------------------------------------------------
// RaggedRows: rows have no common length, so there is no modulo; instead, once
// per workgroup:
//   1. two bounded searches of the device offsets (uniform values, loads only)
//      find the boundaries that fall into the staged frames [t0 - Ha, t0 + T);
//   2. the workgroup's threads stride over those boundaries and set one bit per
//      row start in an LDS bitmask over the staged frames (halo + tile, at most
//      2 KiB + a pad word), and one bit per non-zero mask word in a summary
//      mask (at most 17 words).  Empty rows set the same bit again; boundaries
//      at or past the total are dropped.
// A lane then finds the last row start at or before its unit's first frame from
// its own mask word (31 - clz of the bits at or below the frame), else from the
// summary words behind it -- at most k / 1024 + 2 of them: a start k or more
// frames back is as good as none, and because the staged halo holds Ha >= k
// frames, a frame of the tile with no start bit at or before it in the mask IS
// at position >= k.  No row position before the staged frames is ever needed.
// The lane walks its F frames from there, resetting the distance on a set bit
// and saturating it at k: start = the bit, has_xk = distance >= k.  The halo
// frame count is the distance of the tile's first frame -- 0 when a row starts
// at t0.
//
// Distances never exceed k (no overflow whatever the row lengths); frame indices
// are 64-bit only in uniform values.  Every index derived from the device
// offsets is clamped to the mask it addresses and both searches are bounded by
// `rows`: an offsets array that does not match the host's gives wrong values,
// never an access outside the views.
// ----------------------------------------------------------------------------

// First index i in [lo, rows] with off[i] >= f, or rows + 1 if there is none; lo is clamped to
// [0, rows + 1].  A 64-ary search by one whole wave (every lane active; each wave of the
// workgroup runs it and gets the same uniform answer): the lanes probe 64 evenly spaced entries
// of the remaining range and a ballot keeps the gap that holds the answer, so the range shrinks
// 64-fold per round of loads -- 4 dependent rounds for 2^24 rows where a bisection takes 24, and
// it is the chain of dependent loads that a tile waits for.  The range shrinks strictly whatever
// the array holds, and every load is inside off[0 .. rows].
__device__ __forceinline__ long long ragged_lower_bound(const long long* __restrict__ off, long long rows, long long lo,
                                                        long long f, int lane) {
  lo = lo < 0 ? 0 : lo;
  long long hi = rows + 1;                   // the answer is in [lo, hi]
  lo = lo > hi ? hi : lo;
  while (hi > lo) {
    const long long step = (hi - lo + 63) >> 6;
    const long long idx = lo + (long long)lane * step;
    const bool ge = idx >= hi || off[idx] >= f;
    const unsigned long long b = __ballot(ge);
    const int first = __builtin_amdgcn_readfirstlane(b != 0 ? __builtin_ctzll(b) : 64);
    // probes of the lanes before `first` are < f; lane `first`'s is >= f (or past the range)
    if (first == 0) return lo;
    const long long nhi = lo + (long long)first * step;
    lo = lo + (long long)(first - 1) * step + 1;
    hi = nhi < hi ? nhi : hi;
  }
  return lo;
}

struct RaggedRows {
  using Params = RaggedParams;
  // mask words over `nbits` staged frames (+ a pad word); one summary bit per mask word
  __host__ __device__ static constexpr size_t mask_words(size_t nbits) { return (nbits + 31) / 32 + 1; }
  __host__ __device__ static constexpr size_t summ_words(size_t nwords) { return (nwords + 31) / 32; }
  template <int F, int U, int WG>
  __host__ __device__ static constexpr size_t lds_words(size_t halo_units) {
    const size_t nwords = mask_words(halo_units * F + (size_t)WG * F * U);
    return nwords + summ_words(nwords);
  }

  template <int F, int U, int WG>
  struct Tile {
    static_assert(F <= 16 && 32 % F == 0, "a unit's row-start bits lie in one mask word");
    const uint32_t* mask;  // [nwords] a row starts at the frame; bit i is frame t0 - Ha + i
    const uint32_t* summ;  // [nsumm] the mask word is non-zero
    int k, Ha, nbits;
#ifdef MAVG_DEBUG
    const long long* dbg_off;  // for the cross-check in walk()
    long long dbg_rows, dbg_t0, dbg_nframes;
#endif

    __device__ __forceinline__ void prepare(const Params& p, uint32_t* lds, long long t0, int halo, int tid) {
      constexpr int TF = WG * F * U;
      const int lane = tid & 63;
      const long long* __restrict__ off = p.offsets;
      const long long rows = p.rows, nframes = p.nframes;
      k = p.k;
      Ha = halo;                                 // staged halo frames
      const long long h0 = t0 - Ha;
      nbits = Ha + TF;
      const int nwords = (int)mask_words((size_t)nbits);
      const int nsumm = (int)summ_words((size_t)nwords);
      uint32_t* const m = lds;
      uint32_t* const sm = lds + nwords;
      mask = m;
      summ = sm;
#ifdef MAVG_DEBUG
      dbg_off = off, dbg_rows = rows, dbg_t0 = t0, dbg_nframes = nframes;
#endif
      for (int i = tid; i < nwords + nsumm; i += WG) m[i] = 0;  // (summ follows mask)
      // uniform: boundaries b_lo .. b_hi - 1 fall into [h0, t0 + TF)
      const long long b_lo = ragged_lower_bound(off, rows, 0, h0 > 0 ? h0 : 0, lane);
      // the 64 entries from b_lo on, one per lane: where the staged frames hold at most 64
      // boundaries (rows of 50 frames and more, on average) they give b_hi AND are the boundaries
      const long long pidx = b_lo + lane;
      const long long pv = pidx <= rows ? off[pidx] : nframes;
      long long b_hi;
      {
        const unsigned long long b = __ballot(pidx > rows || pv >= t0 + TF);
        b_hi = b != 0 ? b_lo + __builtin_amdgcn_readfirstlane(__builtin_ctzll(b))
                      : ragged_lower_bound(off, rows, b_lo + 64, t0 + TF, lane);
      }
      b_hi = b_hi < rows ? b_hi : rows;        // off[rows], the total, starts no row
      auto set_start = [&](long long f) {
        const long long pos = f - h0;
        if (pos >= 0 && pos < (long long)nbits && f < nframes) {  // clamped: the mask is all this can touch
          const int wd = (int)pos >> 5;
          MAVG_DCHECK(wd >= 0 && wd < nwords - 1 && (wd >> 5) < nsumm, "ragged mask index", wd, nwords);
          atomicOr(&m[wd], 1u << ((int)pos & 31));
          atomicOr(&sm[wd >> 5], 1u << (wd & 31));
        }
      };
      __syncthreads();
      if ((tid >> 6) == 0 && pidx < b_hi) set_start(pv);  // every wave holds the same 64; one sets them
      for (long long i = b_lo + 64 + tid; i < b_hi; i += WG) set_start(off[i]);
    }

    // frames from the last row start at or before staged frame s back to s, saturated at k
    // (k: no start within k frames, or none staged -- the staged halo holds Ha >= k frames)
    __device__ __forceinline__ int start_dist(int s) const {
      MAVG_DCHECK(s >= 0 && s < nbits, "ragged mask query", s, nbits);
      const int wd = s >> 5, b = s & 31;
      const uint32_t m = mask[wd] & (0xffffffffu >> (31 - b));
      if (m != 0) {
        const int d = b - (31 - __clz((int)m));
        return d < k ? d : k;
      }
      int sw = wd >> 5;
      uint32_t sm = summ[sw] & ((1u << (wd & 31)) - 1u);  // non-zero words before wd
      for (;;) {
        if (sm != 0) {
          const int pw = sw * 32 + 31 - __clz((int)sm);
          MAVG_DCHECK(pw >= 0 && pw < wd && mask[pw] != 0, "ragged summary word", pw, wd);
          const int d = s - (pw * 32 + 31 - __clz((int)mask[pw]));
          return d < k ? d : k;
        }
        if (sw == 0 || s - (sw * 1024 - 1) >= k) return k;  // every earlier start is k or more back
        --sw;
        sm = summ[sw];
      }
    }
    __device__ __forceinline__ int halo_frames() const { return start_dist(Ha); }  // 0: a row starts at t0

    struct Walker {
      uint32_t ub;       // the unit's row starts
      int dist, k;
      __device__ __forceinline__ void frame(int fr, bool& start, bool& has_xk) {
        start = ((ub >> fr) & 1u) != 0;
        dist = start ? 0 : dist;
        has_xk = dist >= k;
        dist = dist + 1 < k ? dist + 1 : k;     // saturates at k
      }
    };
    __device__ __forceinline__ Walker walk(int, int j) const {
      const int s = Ha + j * F;                 // the unit's first frame in the mask (a multiple of F)
      const uint32_t ub = (mask[s >> 5] >> (s & 31)) & ((1u << F) - 1u);
      const int dist = start_dist(s);
#ifdef MAVG_DEBUG
      {
        // the derived distance against a direct bounded search of the offsets
        const long long f = dbg_t0 + (long long)j * F;
        if (f < dbg_nframes) {
          long long a = -1, b = dbg_rows;            // the last i < rows with off[i] <= f
          while (b - a > 1) {
            const long long m = a + ((b - a) >> 1);
            if (dbg_off[m] <= f) a = m;
            else b = m;
          }
          const long long q = a >= 0 ? f - dbg_off[a] : (long long)k;
          MAVG_DCHECK((long long)dist == (q < (long long)k ? q : (long long)k), "ragged position", dist, q);
        }
      }
#endif
      return Walker{ub, dist, k};
    }
  };
};

// ----------------------------------------------------------------------------
// The scan body: two barriers of its own (after the stage, after the segment
// totals) plus what the row source's prepare holds.
// ----------------------------------------------------------------------------
template <typename Src, typename T, typename A, int C, int F, int U, int WG, int NT, int DV>
__device__ __forceinline__ void seg_tile_scan(const typename Src::Params& p) {
  constexpr int NW = WG / 64;
  constexpr int VE = F * C;
  constexpr int TF = WG * F * U;           // tile frames
  constexpr int NSEG = U * NW;
  static_assert(NSEG <= 64, "segment totals are scanned across one wave");
  using IO = UnitIO<T, VE>;
  using U_t = Unit<T, VE>;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Hu = p.halo_units;
  const int Ha = Hu * F;                     // staged halo frames (>= k)
  const SegLds<Src, T, A, C, F, U, WG> lds((size_t)Hu);
  T* stage = reinterpret_cast<T*>(smem);     // [Hu + U*WG + 1 pad] units
  A* tot = reinterpret_cast<A*>(smem + (int)lds.tot);              // [NSEG][C] segment totals (since the last row start)
  A* hsum = reinterpret_cast<A*>(smem + (int)lds.hsum);            // [NW][C] halo partial sums
  int32_t* sflag = reinterpret_cast<int32_t*>(smem + (int)lds.sflag);  // [NSEG] a row starts in the segment

  const T* __restrict__ in = static_cast<const T*>(p.in);
  T* __restrict__ out = static_cast<T*>(p.out);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = tid >> 6;
  const int k = p.k;
  const long long nframes = p.nframes;
  const bool eio = F == 1 && p.eio != 0;

  const long long tile = remap_tile(blockIdx.x, gridDim.x, p.xcd_remap);
  const long long t0 = tile * TF;
  const long long h0 = t0 - Ha;              // first staged halo frame
  MAVG_DCHECK(tile >= 0 && tile < p.ntiles && t0 < nframes, "segscan tile index", tile, p.ntiles);
  MAVG_DCHECK(lds.bytes <= (size_t)(WG >= 1024 ? 80 * 1024 : 64 * 1024), "segscan LDS layout", lds.bytes, Hu);
  MAVG_DCHECK(k >= 1 && k <= Ha, "segscan effective window", k, Ha);
  const bool tile_full = (t0 + TF <= nframes);

  auto guarded = [&](long long f, int c) -> T { return (f >= 0 && f < nframes) ? in[f * C + c] : (T)0; };

  // ---- tile -> registers (issued first: the loads' latency covers the row bookkeeping) ----
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
        for (int c = 0; c < C; ++c) x[u].e[fr * C + c] = guarded(f + fr, c);
    }
  }

  // ---- row bookkeeping: where the rows start in the staged frames ----
  typename Src::template Tile<F, U, WG> rows;
  rows.prepare(p, reinterpret_cast<uint32_t*>(smem + (int)lds.src), t0, Ha, tid);

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
          for (int c = 0; c < C; ++c) h.e[fr * C + c] = guarded(f + fr, c);
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

  // ---- halo reduction: the hq frames before t0 that belong to the row the tile continues ----
  const int hq = rows.halo_frames();          // uniform
  {
    A hs[C];
#pragma unroll
    for (int c = 0; c < C; ++c) hs[c] = (A)0;
    MAVG_DCHECK(hq >= 0 && hq <= Ha && hq <= k, "segscan halo frames", hq, Ha);
    for (int i = Ha - hq + tid; i < Ha; i += WG)
#pragma unroll
      for (int c = 0; c < C; ++c) hs[c] += to_acc<A>(stage[i * C + c]);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const A r = readlane(wave_incl_scan(hs[c]), 63);
      if (lane == 0) hsum[w * C + c] = r;
    }
  }

  // x[n-k] for lane unit j, from the LDS stage (an unaligned x[n-k]: two
  // aligned units and a uniform shift); frames at positions < k are masked by the caller
  auto stage_xk = [&](int j) -> U_t {
    const int e = (Ha + j * F - k) * C;
    U_t xk;
    if constexpr (IO::kVec) {
      if (p.xk_off == 0) {
        MAVG_DCHECK(e >= 0 && e + VE <= (int)lds.stage_units * VE, "segscan x[n-k] stage index", e, j);
        xk = IO::load(stage + e);
      } else {
        const int e_lo = e - p.xk_off;
        MAVG_DCHECK(e_lo >= 0 && e_lo + 2 * VE <= (int)lds.stage_units * VE, "segscan x[n-k] extraction", e_lo, j);
        U_t a = IO::load_whole(stage + e_lo);
        U_t b = IO::load_whole(stage + e_lo + VE);
        xk = extract(a, b, p.xk_off);
      }
    } else {
      MAVG_DCHECK(e >= 0 && e + VE <= (int)lds.stage_units * VE, "segscan x[n-k] stage index", e, j);
#pragma unroll
      for (int i = 0; i < VE; ++i) xk.e[i] = stage[e + i];
    }
    return xk;
  };

  // ---- d = x - x[n-k] (zero at positions < k); segmented in-lane and wave scans ----
  A v[U][F][C];        // in-lane prefixes since the last row start in the lane (or the lane's start)
  uint32_t seen[U];    // bit fr: a row start at or before frame fr in this lane's unit
  A lx[U][C];          // what the earlier lanes of the wave carry into this lane
  int32_t lxf[U];      // ... and whether a row starts in them
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = u * WG + tid;
    const U_t xk = stage_xk(j);
    auto walker = rows.walk(u, j);
    int32_t fl = 0;
    uint32_t sm = 0;
    A run[C];
#pragma unroll
    for (int c = 0; c < C; ++c) run[c] = (A)0;
#pragma unroll
    for (int fr = 0; fr < F; ++fr) {
      bool start, has_xk;
      walker.frame(fr, start, has_xk);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const T xkv = has_xk ? xk.e[fr * C + c] : (T)0;
        const A d = to_acc<A>(x[u].e[fr * C + c]) - to_acc<A>(xkv);
        run[c] = start ? d : run[c] + d;
        v[u][fr][c] = run[c];
      }
      fl |= start ? 1 : 0;
      sm |= (uint32_t)fl << fr;
    }
    seen[u] = sm;
    wave_seg_incl_scan(fl, run);             // inclusive over the wave's lanes
    const int32_t fe = shfl_up(fl, 1);
    lxf[u] = lane == 0 ? 0 : fe;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const A ve = shfl_up(run[c], 1);
      lx[u][c] = lane == 0 ? (A)0 : ve;
      const A segtot = readlane(run[c], 63);
      if (lane == 0) tot[(u * NW + w) * C + c] = segtot;
    }
    const int32_t segf = readlane(fl, 63);
    if (lane == 0) sflag[u * NW + w] = segf;
  }
  __syncthreads();

  // ---- carry: halo sum + earlier segments, both only up to the first row start; outputs ----
  // lane i loads segment i's (flag, total), one segmented wave scan gives every prefix, and
  // each unit reads its own with a uniform readlane (NSEG <= 64)
  const int wu = __builtin_amdgcn_readfirstlane(w);
  A base[U][C];
  {
    A w0[C];
    A tv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      w0[c] = (A)0;
#pragma unroll
      for (int i = 0; i < NW; ++i) w0[c] += hsum[i * C + c];
      tv[c] = lane < NSEG ? tot[lane * C + c] : (A)0;
    }
    int32_t tf = lane < NSEG ? sflag[lane] : 0;
    wave_seg_incl_scan(tf, tv);
    const int32_t ef0 = shfl_up(tf, 1);
    const int32_t ef = lane == 0 ? 0 : ef0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const A ev0 = shfl_up(tv[c], 1);
      const A ev = lane == 0 ? (A)0 : ev0;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t bf = readlane(ef, u * NW + wu);  // a row starts in an earlier segment of the tile
        const A bv = readlane(ev, u * NW + wu);
        base[u][c] = bf != 0 ? bv : w0[c] + bv;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const long long f = t0 + (long long)(u * WG + tid) * F;
    A lb[C];
#pragma unroll
    for (int c = 0; c < C; ++c) lb[c] = lxf[u] != 0 ? lx[u][c] : base[u][c] + lx[u][c];
    U_t y;
#pragma unroll
    for (int fr = 0; fr < F; ++fr) {
      const bool own = ((seen[u] >> fr) & 1u) != 0;  // the row started in this lane's unit
#pragma unroll
      for (int c = 0; c < C; ++c) y.e[fr * C + c] = to_out<T, A, DV>(own ? v[u][fr][c] : lb[c] + v[u][fr][c], p.o);
    }
    if (tile_full) {
      IO::template gstore<(NT & kNtStore) != 0>(out + f * C, y, eio);
    } else {
#pragma unroll
      for (int fr = 0; fr < F; ++fr)
        if (f + fr < nframes)
#pragma unroll
          for (int c = 0; c < C; ++c) out[(f + fr) * C + c] = y.e[fr * C + c];
    }
  }
}

template <typename T, typename A, int C, int F, int U, int WG = kWG, int NT = kNtSplit | kNtHalo | kNtStore,
          int DV = 0>
__global__ __launch_bounds__(WG) void rows_scan_kernel(RowsParams p) {
  seg_tile_scan<DenseRows, T, A, C, F, U, WG, NT, DV>(p);
}

template <typename T, typename A, int C, int F, int U, int WG = kWG, int NT = kNtSplit | kNtHalo | kNtStore,
          int DV = 0>
__global__ __launch_bounds__(WG) void ragged_scan_kernel(RaggedParams p) {
  seg_tile_scan<RaggedRows, T, A, C, F, U, WG, NT, DV>(p);
}

}  // namespace mavg
