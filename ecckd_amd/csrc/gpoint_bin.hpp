// gpoint_bin.hpp - the binning of a tile of 256 wavenumbers into the g points ("columns") of a launch, written once for
// k_lbl_gpoint_fluxes_lw (lbl_gpoint_fluxes.hip) and k_lbl_gpoint_fluxes_sw (lbl_gpoint_fluxes_sw.hip).
//
// A g point is a scattered set of wavenumbers.  Walking the g-sorted permutation would make every load of the optical
// depths of a point a 4-byte gather (one cache line per lane), so the kernels walk the spectrum in NATURAL order - one thread
// per wavenumber, 256 consecutive wavenumbers per tile, every row load 1 KB contiguous per block - and bin inside the block:
//   * once per tile the 256 points are ranked by (column, lane), column = g point of this launch / "no g point" / none
//     (tile_key, tile_rank): a comparison count over the tile's keys in LDS, deterministic, the order inside a column is
//     the wavenumber order;
//   * every flux a thread produces goes to LDS at its RANK (s_f[row of the batch][pos]); after GB_LB rows the block turns
//     round (reduce_batch): thread (row slot, segment of GB_SEGLEN ranks) adds its segment left to right, one piece per
//     column.  A piece that starts its column is added to the block's accumulator row acc[column] (LDS) by that thread
//     alone; a piece that continues a column from the segment before is parked and, after a barrier, added by the thread that
//     owns the column's first piece, segment after segment.  Every accumulator entry has one writer per batch and a fixed
//     order: no atomics, bitwise reproducible;
//   * which accumulator row a slot of the batch feeds is the caller's business: that is where the kernels differ;
//   * a block walks `tpb` consecutive tiles (tile_grid: a function of nwav alone), then writes its accumulator as its
//     partial; k_gpoint_combine adds the blocks' partials in block order.
// The accumulator has to fit into LDS next to the 22 KB of static arrays below; a map with more columns than a launch holds
// is swept in several launches, each binning its own range of g points (bin_column_ranges).
#pragma once

#include "common.hpp"

#include <algorithm>

namespace {   // a kernel and LDS arrays: every translation unit that includes this gets its own (lbl_scenarios.hip, which
              // takes only the accumulator budgets from here, an unused copy of the small kernel)

constexpr int GB_THREADS = 256;
constexpr int GB_LB = 8;                          // rows per batch
constexpr int GB_SEG = GB_THREADS / GB_LB;        // 32 segments ...
constexpr int GB_SEGLEN = GB_THREADS / GB_SEG;    // ... of 8 ranks
constexpr int GB_ROW = GB_THREADS + GB_SEG;       // a row's 256 fluxes, one pad per segment: segment stride 9 doubles = 18 banks
constexpr int GB_NONE = 0x7fffff;                 // column of a point that is binned nowhere
constexpr size_t GB_FIXED_LDS = (size_t)GB_LB * GB_ROW * 8 + (size_t)GB_LB * GB_SEG * 8 + 2 * GB_THREADS * 4;
constexpr int GB_TARGET_BLOCKS = 2048;
// The accumulator budgets (dynamic LDS) of the two kernels.  Longwave: static + dynamic LDS of a block stay within 64 KB,
// which a launch may use without asking.  Shortwave: 80 KB per block, which has to be asked for with hipFuncSetAttribute; the
// header of lbl_gpoint_fluxes_sw.hip says why 80.
constexpr size_t GF_ACC_BYTES = 65536 - GB_FIXED_LDS;
constexpr size_t SF_BLOCK_LDS = 80 * 1024;
constexpr size_t SF_ACC_BYTES = SF_BLOCK_LDS - GB_FIXED_LDS;

__shared__ double s_f[GB_LB * GB_ROW];
__shared__ double s_cont[GB_LB * GB_SEG];
__shared__ __align__(16) int s_raw[GB_THREADS];
__shared__ int s_key[GB_THREADS];

// what thread (slot, seg) knows of its segment [base, base + GB_SEGLEN) of the ranked tile
struct TilePieces {
  unsigned brk;     // bit q: a break before rank base + q, where the column changes
  bool cont_in;     // the segment begins inside a column that the segment before began or continued
  int tail_key;     // the column of the segment's last rank
  bool collects;    // that column's first piece ends this segment and goes on in the next: this thread adds the parked pieces
};

// the column of point j: g points [g0, g0 + gcount) -> 0.., g_point < 0 -> col_unassigned (if any), everything else nowhere
__device__ __forceinline__ int tile_key(bool live, const int32_t* __restrict__ g_point /* NULL: every point in column 0 */, size_t j,
                                        int g0, int gcount, int col_unassigned /* column of g_point < 0, or -1 */) {
  int key = GB_NONE;
  if (live) {
    if (!g_point) key = 0;
    else {
      const int g = g_point[j];
      if (g >= g0 && g < g0 + gcount) key = g - g0;
      else if (g < 0 && col_unassigned >= 0) key = col_unassigned;
    }
  }
  return key;
}

// rank by (column, lane); leaves s_key[rank] = column for the whole tile and returns where this thread's fluxes go in a row of s_f
__device__ __forceinline__ int tile_rank(int tid, int key) {
  const int mine = (key << 8) | tid;
  s_raw[tid] = mine;
  __syncthreads();
  int rank = 0;
  for (int q = 0; q < GB_THREADS; q += 4) {
    const int4 c = *reinterpret_cast<const int4*>(&s_raw[q]);
    rank += (c.x < mine) + (c.y < mine) + (c.z < mine) + (c.w < mine);
  }
  s_key[rank] = key;
  const int pos = rank + rank / GB_SEGLEN;
  __syncthreads();
  return pos;
}

__device__ __forceinline__ TilePieces tile_pieces(int seg, int base) {
  TilePieces p;
  p.brk = 0;
  for (int q = 1; q < GB_SEGLEN; ++q) p.brk |= (s_key[base + q] != s_key[base + q - 1]) ? (1u << q) : 0u;
  p.cont_in = seg > 0 && s_key[base] == s_key[base - 1];
  p.tail_key = s_key[base + GB_SEGLEN - 1];
  p.collects = seg + 1 < GB_SEG && s_key[base + GB_SEGLEN] == p.tail_key && p.tail_key != GB_NONE && !(p.brk == 0 && p.cont_in);
  return p;
}

// Row `slot` of the batch in s_f, added per column into the accumulator row `acc` by the threads with `on` (every thread of
// the block calls this: two barriers).
__device__ __forceinline__ void reduce_batch(const TilePieces& p, bool on, int slot, int seg, int base, double* acc) {
  __syncthreads();
  if (on) {
    const double* f = s_f + slot * GB_ROW + base + seg;
    double sum = 0.0;
    int k = s_key[base];
    bool parked = p.cont_in;
    for (int q = 0; q < GB_SEGLEN; ++q) {
      if (q > 0 && ((p.brk >> q) & 1u)) {
        if (k != GB_NONE) { if (parked) s_cont[slot * GB_SEG + seg] = sum; else acc[k] += sum; }
        sum = 0.0; parked = false; k = s_key[base + q];
      }
      sum += f[q];
    }
    if (k != GB_NONE) { if (parked) s_cont[slot * GB_SEG + seg] = sum; else acc[k] += sum; }
  }
  __syncthreads();
  if (on && p.collects) {
    for (int s2 = seg + 1; s2 < GB_SEG && s_key[s2 * GB_SEGLEN] == p.tail_key; ++s2) {
      acc[p.tail_key] += s_cont[slot * GB_SEG + s2];
      if (s_key[s2 * GB_SEGLEN + GB_SEGLEN - 1] != p.tail_key) break;
    }
  }
}

// out[row0 + row][col_out(c)] = the blocks' partials added in block order; one thread per accumulator entry
__global__ void __launch_bounds__(256)
k_gpoint_combine(int nblk, int nacc, int ncols, int row0, int g0, int gcount, int out_cols, const double* __restrict__ partial,
                 double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nacc) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[(size_t)b * nacc + e];
  const int r = e / ncols, c = e % ncols;
  out[(size_t)(row0 + r) * out_cols + (c < gcount ? g0 + c : out_cols - 1)] = s;
}

// tiles per block and blocks of a spectrum: a function of nwav alone
struct TileGrid { int tpb, nblk; };
inline TileGrid tile_grid(size_t nwav) {
  const size_t ntiles = (nwav + GB_THREADS - 1) / GB_THREADS;
  const int tpb = (int)std::max<size_t>(1, (ntiles + GB_TARGET_BLOCKS - 1) / GB_TARGET_BLOCKS);
  return TileGrid{tpb, (int)((ntiles + tpb - 1) / tpb)};
}

// The launches that fill rows [row0, row0 + nrows) of d_out[..][ng + 1]: g points [g0, g0 + gcount) each, at most max_cols
// columns; the first one also bins the points without a g point (into column ng, if the spectrum has a map at all).
// launch(g0, gcount, col_unassigned, ncols) starts the flux kernel on ctx->stream, which leaves d_part[nblk][nrows][ncols].
template <typename Launch>
int bin_column_ranges(ecckd_ctx* ctx, int ng, bool mapped, int max_cols, int nblk, int nrows, int row0, const double* d_part,
                      double* d_out, Launch launch) {
  for (int g0 = 0, pass = 0; pass == 0 || g0 < ng; ++pass) {
    const bool with_none = pass == 0;
    const int gcount = std::min(ng - g0, max_cols - (with_none ? 1 : 0));
    const int ncols = gcount + (with_none ? 1 : 0);
    const int nacc = nrows * ncols;
    ECCKD_CHECK(launch(g0, gcount, (with_none && mapped) ? gcount : -1, ncols));
    ECCKD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_gpoint_combine, dim3((unsigned)((nacc + 255) / 256)), dim3(256), 0, ctx->stream, nblk, nacc, ncols, row0, g0,
                       gcount, ng + 1, d_part, d_out);
    ECCKD_HIP_CHECK(hipGetLastError());
    g0 += gcount;
  }
  return ECCKD_OK;
}

// The finished out[nsza][2][nhl][ng + 1] (direction 0 down, 1 up; longwave: nsza = 1) split into the caller's arrays: the g
// points into h_dn, h_up [nsza][nhl][ng], and every wavenumber - the g points in order, then the points of none
// (lw_spectra.cpp:231-232) - into the broadband rows h_bb_dn, h_bb_up [nsza][nhl], each of the two wanted or NULL.
inline void unpack_gpoint_out(const double* out, int nsza, int nhl, int ng, double* h_dn, double* h_up, double* h_bb_dn, double* h_bb_up) {
  for (int s = 0; s < nsza; ++s)
    for (int l = 0; l < nhl; ++l) {
      const double* dn = &out[((size_t)(s * 2) * nhl + l) * (ng + 1)];
      const double* up = &out[((size_t)(s * 2 + 1) * nhl + l) * (ng + 1)];
      double bdn = 0.0, bup = 0.0;
      for (int g = 0; g <= ng; ++g) { bdn += dn[g]; bup += up[g]; }
      const size_t o = (size_t)s * nhl + l;
      for (int g = 0; g < ng; ++g) { h_dn[o * ng + g] = dn[g]; h_up[o * ng + g] = up[g]; }
      if (h_bb_dn) h_bb_dn[o] = bdn;
      if (h_bb_up) h_bb_up[o] = bup;
    }
}

// The three-flux sibling (lbl_gpoint_fluxes_sw_rayleigh.hip): out[nsza][3][nhl][ng + 1], flux 0 the direct beam, 1 the total
// downwelling flux, 2 the upwelling one; h_flux[k] [nsza][nhl][ng] (all NULL when ng = 0) and h_bb[k] [nsza][nhl], each or NULL
inline void unpack_gpoint_out3(const double* out, int nsza, int nhl, int ng, double* const (&h_flux)[3], double* const (&h_bb)[3]) {
  for (int s = 0; s < nsza; ++s)
    for (int k = 0; k < 3; ++k)
      for (int l = 0; l < nhl; ++l) {
        const double* row = &out[((size_t)(s * 3 + k) * nhl + l) * (ng + 1)];
        double bb = 0.0;
        for (int g = 0; g <= ng; ++g) bb += row[g];
        const size_t o = (size_t)s * nhl + l;
        for (int g = 0; g < ng; ++g) h_flux[k][o * ng + g] = row[g];
        if (h_bb[k]) h_bb[k][o] = bb;
      }
}

}  // namespace
