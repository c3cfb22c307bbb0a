// mavg_rows.hpp -- the batched rows scan (rows_scan_kernel): many independent
// signals, stored densely one after another, filtered in one launch.
#pragma once

#include "mavg_device.hpp"

namespace mavg {

// ----------------------------------------------------------------------------
// rows scan kernel: the dense batch of `rows` signals of `row_frames` frames is
// one flat stream of rows * row_frames frames, cut into fixed tiles of
// T = WG*F*U frames exactly as tile_scan_kernel (mavg_tile.hpp) cuts a signal:
// 16-B lane units, the halo and the tile staged in LDS, the remap_tile XCD
// mapping, two barriers, no inter-workgroup communication.  Tile boundaries
// ignore row boundaries, so every load and store stays full-width whatever
// row_frames is; a workgroup may hold hundreds of rows or a sliver of one.
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
// Row positions without 64-bit divides: q0 = t0 mod row_frames once per
// workgroup (uniform), then every lane's position is 32-bit arithmetic (one
// 32-bit modulo per lane, increments with a conditional wrap after it).  Rows
// longer than 2^30 frames are clamped: a tile then holds at most one row start
// and positions only matter while < k or == 0.
//
// k here is the EFFECTIVE window min(grade, row_frames): with grade >=
// row_frames every position is < grade, x[n-k] is never used, and the stage
// only ever needs the row's own frames.  The divisor stays the grade (p.o).
// ----------------------------------------------------------------------------
struct RowsParams {
  const void* in;
  void* out;
  long long nframes;     // rows * row_frames
  long long row_frames;
  long long ntiles;
  int k;                 // effective window: min(grade, row_frames)
  int halo_units;        // ceil(k / F): units staged before the tile
  int xk_off;            // (-k*C) mod VE
  int xcd_remap;         // remap_tile mode
  int eio;               // frame-unit launch on element-aligned pointers (UnitIO::gload)
  OutParams o;           // of the grade (the divisor)
};

constexpr uint32_t kRowsPosClamp = 1u << 30;  // in-row positions are kept below this

template <typename T, typename A, int C, int F, int U, int WG = kWG, int NT = kNtSplit | kNtHalo | kNtStore,
          int DV = 0>
__global__ __launch_bounds__(WG) void rows_scan_kernel(RowsParams p) {
  constexpr int NW = WG / 64;
  constexpr int VE = F * C;
  constexpr int TF = WG * F * U;           // tile frames
  constexpr int NSEG = U * NW;
  static_assert(NSEG <= 64, "segment totals are scanned across one wave");
  static_assert(F <= 16, "the per-lane row-start mask is 16 bits wide");
  using IO = UnitIO<T, VE>;
  using U_t = Unit<T, VE>;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int Hu = p.halo_units;
  const int Ha = Hu * F;                     // staged halo frames (>= k)
  const int stage_bytes = (((Hu + U * WG + 1) * VE * (int)sizeof(T)) + 15) & ~15;
  T* stage = reinterpret_cast<T*>(smem);     // [Hu + U*WG + 1 pad] units
  A* tot = reinterpret_cast<A*>(smem + stage_bytes);  // [NSEG][C] segment totals (since the last row start)
  A* hsum = tot + NSEG * C;                            // [NW][C] halo partial sums
  int32_t* sflag = reinterpret_cast<int32_t*>(hsum + NW * C);  // [NSEG] a row starts in the segment

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
  MAVG_DCHECK(tile >= 0 && tile < p.ntiles && t0 < nframes, "rows tile index", tile, p.ntiles);
  MAVG_DCHECK(stage_bytes + (NSEG + NW) * C * (int)sizeof(A) + NSEG * 4 <= (int)(WG >= 1024 ? 80 * 1024 : 64 * 1024),
              "rows LDS layout", stage_bytes, Hu);
  MAVG_DCHECK(k >= 1 && (long long)k <= p.row_frames && k <= Ha, "rows effective window", k, Ha);
  const bool tile_full = (t0 + TF <= nframes);

  // ---- row bookkeeping (uniform): the tile's first frame sits at position q0 of its row ----
  const long long L = p.row_frames;
  const long long q0 = t0 % L;               // the one 64-bit divide, scalar
  uint32_t Lc, q0c;
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
  const int hq = (int)(q0c < (uint32_t)k ? q0c : (uint32_t)k);  // halo frames of the row the tile continues
  const uint32_t pstep = (uint32_t)(WG * F) % Lc;
  uint32_t pos[U];                           // position of each unit's first frame
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
    MAVG_DCHECK((pos[u] == 0) == (q == 0) && (pos[u] < (uint32_t)k) == (q < (long long)k), "rows position", pos[u], q);
  }
#endif

  auto guarded = [&](long long f, int c) -> T { return (f >= 0 && f < nframes) ? in[f * C + c] : (T)0; };

  // ---- tile -> registers ----
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

  // ---- halo reduction: the hq frames before t0 that belong to the tile's first row ----
  {
    A hs[C];
#pragma unroll
    for (int c = 0; c < C; ++c) hs[c] = (A)0;
    MAVG_DCHECK(hq >= 0 && hq <= Ha, "rows halo frames", hq, Ha);
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
        MAVG_DCHECK(e >= 0 && e + VE <= (Hu + U * WG + 1) * VE, "rows x[n-k] stage index", e, j);
        xk = IO::load(stage + e);
      } else {
        const int e_lo = e - p.xk_off;
        MAVG_DCHECK(e_lo >= 0 && e_lo + 2 * VE <= (Hu + U * WG + 1) * VE, "rows x[n-k] extraction", e_lo, j);
        U_t a = IO::load_whole(stage + e_lo);
        U_t b = IO::load_whole(stage + e_lo + VE);
        xk = extract(a, b, p.xk_off);
      }
    } else {
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
    uint32_t pp = pos[u];
    int32_t fl = 0;
    uint32_t sm = 0;
    A run[C];
#pragma unroll
    for (int c = 0; c < C; ++c) run[c] = (A)0;
#pragma unroll
    for (int fr = 0; fr < F; ++fr) {
      const bool start = pp == 0;
      const bool has_xk = pp >= (uint32_t)k;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const T xkv = has_xk ? xk.e[fr * C + c] : (T)0;
        const A d = to_acc<A>(x[u].e[fr * C + c]) - to_acc<A>(xkv);
        run[c] = start ? d : run[c] + d;
        v[u][fr][c] = run[c];
      }
      fl |= start ? 1 : 0;
      sm |= (uint32_t)fl << fr;
      pp = pp + 1 == Lc ? 0 : pp + 1;
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

}  // namespace mavg
