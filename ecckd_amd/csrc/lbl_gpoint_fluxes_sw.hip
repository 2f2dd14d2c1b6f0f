// lbl_gpoint_fluxes_sw.hip - line-by-line shortwave fluxes of one column resolved per g point, for up to SF_MAX_SZA solar
// zenith angles at once: radiative_transfer_direct_sw and radiative_transfer_norayleigh_sw (radiative_transfer_sw.cpp:26-77),
// expression by expression what k_lbl_fluxes_sw (lbl_fluxes.hip) computes per wavenumber, and the sum of every flux row over
// the wavenumbers of every g point in one pass over the optical depths.  The other output mode of the same kernel writes the
// spectral fluxes themselves (FLOAT rows) with the broadband sums.
//
// Shape: that of k_lbl_gpoint_fluxes_lw (lbl_gpoint_fluxes.hip), whose binning scheme is repeated here (duplicated, not
// shared: the longwave file stays as it is, bit for bit).  One thread per wavenumber in NATURAL order, 256 consecutive
// wavenumbers per tile, every row load 1 KB contiguous per block; once per tile the points are ranked by (column, lane);
// every flux goes to LDS at its rank; after a batch of rows thread (row slot, segment of SF_SEG ranks) adds its segment left
// to right, one piece per column; a piece that starts its column is added to the block's accumulator by that thread alone, a
// piece that continues a column is parked and added by the owner of the column's first piece, segment after segment.  One
// writer per accumulator entry, fixed order, no atomics; a block walks `tiles_per_block` tiles (a function of nwav alone) and
// writes its accumulator as a partial; k_sf_combine adds the partials in block order.  Bitwise reproducible.
//
// Angles.  A launch carries A <= 8 angles.  A thread keeps the A fluxes of its wavenumber in registers and walks the layers
// ONCE down and once up: tau_l is loaded once per sweep for all angles, and exp(-2.0 * tau_l) of the upwelling sweep, which
// does not depend on the angle, is evaluated once per (point, layer) and multiplied into every angle's flux in the reference's
// order (no cumulative transmission: the rounding is that of A separate calls).  Per point and launch: nlay (A + 1)
// exponentials.  A batch of the binning is SF_LB / A levels x A angles (at most SF_LB = 8 rows).
//
// LDS budget: at most 80 KB per block (22 KB static + a dynamic accumulator of up to SF_ACC_BYTES = 58 KB, requested by its
// actual size).  The CU has 160 KB, so a launch never has fewer than two resident blocks per CU: one block per CU (up to
// 160 KB) would leave every barrier of the batch reduction uncovered by a second block.  The split below packs angles into a
// launch until the accumulator is nearly full, so where it packs, the launch runs at those two blocks (two waves per SIMD):
// ng = 32 at 54 layers takes 2 angles and 80.6 KB per block, where one angle per launch would take 51.5 KB and run three
// blocks per CU - the longwave kernel's residency at that shape - in 5 launches instead of 3.  Fewer launches against more
// resident waves: which wins is a measurement, and DESIGN.md (K11) says what has been taken.  The split into launches is a function of
// (nlay, nsza, ng) alone:
//   cap = SF_ACC_BYTES / (16 (nlay+1))   column-angles per launch (67 at 54 layers, 176 at 20)
//   cap >= ng + 1: every column in one launch, A = min(nsza, cap / (ng + 1)) angles per launch, spread evenly over
//                  ceil(nsza / A) launches (ng = 32, 54 layers: 2 + 2 + 1 angles; ng = 16: 3 + 2);
//   otherwise:     one angle per launch, and the columns in ceil((ng + 1) / cap) ranges per angle.
// Splitting angles only repeats the loads and the shared exponential; splitting columns repeats the whole transfer, which
// is why angles are split first.  The column ranges do not depend on nsza, so angle s of a multi-angle call has the bits of a
// single-angle call.
#include "common.hpp"
#include "gmap.hpp"

#include <algorithm>
#include <vector>

namespace {

constexpr int SF_THREADS = 256;
constexpr int SF_LB = 8;                          // rows per batch (at most)
constexpr int SF_SEG = SF_THREADS / SF_LB;        // 32 segments ...
constexpr int SF_SEGLEN = SF_THREADS / SF_SEG;    // ... of 8 ranks
constexpr int SF_ROW = SF_THREADS + SF_SEG;       // a row's 256 fluxes, one pad per segment
constexpr int SF_NONE = 0x7fffff;                 // column of a point that is binned nowhere
constexpr int SF_MAX_SZA = 8;
constexpr size_t SF_BLOCK_LDS = 80 * 1024;        // see the header
constexpr size_t SF_FIXED_LDS = (size_t)SF_LB * SF_ROW * 8 + (size_t)SF_LB * SF_SEG * 8 + 2 * SF_THREADS * 4;
constexpr size_t SF_ACC_BYTES = SF_BLOCK_LDS - SF_FIXED_LDS;
constexpr int SF_TARGET_BLOCKS = 2048;

// dynamic LDS: acc[A][2][nhl][ncols]
template <typename OdT, bool SPECTRAL>
__global__ void __launch_bounds__(SF_THREADS)
k_lbl_gpoint_fluxes_sw(int nlay, size_t nwav, size_t od_stride, int tiles_per_block, int nang,
                       const double* __restrict__ cos_sza, const double* __restrict__ minus_sec_sza /* [nang]: -1.0 / cos_sza */,
                       const double* __restrict__ ssi, const double* __restrict__ albedo /* per wavenumber or NULL */,
                       const OdT* __restrict__ od, const int32_t* __restrict__ g_point /* NULL: every point in column 0 */,
                       int g0, int gcount, int col_unassigned /* column of g_point < 0, or -1 */, int ncols,
                       double* __restrict__ partial, float* __restrict__ spec_dn, float* __restrict__ spec_up /* [nang][nhl][stride] */,
                       size_t spec_stride) {
  extern __shared__ double s_acc[];
  __shared__ double s_f[SF_LB * SF_ROW];
  __shared__ double s_cont[SF_LB * SF_SEG];
  __shared__ __align__(16) int s_raw[SF_THREADS];
  __shared__ int s_key[SF_THREADS];
  const int nhl = nlay + 1;
  const int tid = threadIdx.x;
  const int nacc = nang * 2 * nhl * ncols;
  for (int t = tid; t < nacc; t += SF_THREADS) s_acc[t] = 0.0;
  // this thread as an adder: row slot = (level of the batch, angle) and segment
  const int slot = tid / SF_SEG, seg = tid % SF_SEG, base = seg * SF_SEGLEN;
  const int lpb = SF_LB / nang;                   // levels per batch
  const int slot_lev = slot / nang, slot_ang = slot % nang;
  const int nsteps = albedo ? 2 * nhl : nhl;      // step k < nhl: down at level k; k >= nhl: up at level nlay - (k - nhl)

  const size_t tile0 = (size_t)blockIdx.x * tiles_per_block;
  for (int it = 0; it < tiles_per_block; ++it) {
    const size_t i = (tile0 + it) * SF_THREADS + tid;
    if ((tile0 + it) * SF_THREADS >= nwav) break;                           // (block-uniform)
    const bool live = i < nwav;
    const size_t j = live ? i : nwav - 1;
    int key = SF_NONE;
    if (live) {
      if (!g_point) key = 0;
      else {
        const int g = g_point[j];
        if (g >= g0 && g < g0 + gcount) key = g - g0;
        else if (g < 0 && col_unassigned >= 0) key = col_unassigned;
      }
    }
    // ---- rank by (column, lane)
    const int mine = (key << 8) | tid;
    s_raw[tid] = mine;
    __syncthreads();
    int rank = 0;
    for (int q = 0; q < SF_THREADS; q += 4) {
      const int4 c = *reinterpret_cast<const int4*>(&s_raw[q]);
      rank += (c.x < mine) + (c.y < mine) + (c.z < mine) + (c.w < mine);
    }
    s_key[rank] = key;
    const int pos = rank + rank / SF_SEGLEN;
    __syncthreads();
    // ---- the pieces of this thread's segment: a break before rank base + q where the column changes
    unsigned brk = 0;
    for (int q = 1; q < SF_SEGLEN; ++q) brk |= (s_key[base + q] != s_key[base + q - 1]) ? (1u << q) : 0u;
    const bool cont_in = seg > 0 && s_key[base] == s_key[base - 1];
    const int tail_key = s_key[base + SF_SEGLEN - 1];
    // the column's first piece ends this segment and goes on in the next one: this thread collects the parked pieces
    const bool collects = seg + 1 < SF_SEG && s_key[base + SF_SEGLEN] == tail_key && tail_key != SF_NONE && !(brk == 0 && cont_in);

    // the batch that ends with step `last` (nl levels of it): rows (angle, direction, level) of the accumulator
    auto reduce_batch = [&](int last, int nl) {
      __syncthreads();
      const bool on = slot_lev < nl && slot < lpb * nang;
      const int k = last - (nl - 1) + (on ? slot_lev : 0);
      const int r = (slot_ang * 2 + (k >= nhl ? 1 : 0)) * nhl + (k >= nhl ? nlay - (k - nhl) : k);
      double* acc = s_acc + (size_t)r * ncols;
      if (on) {
        const double* f = s_f + slot * SF_ROW + base + seg;
        double sum = 0.0;
        int kk = s_key[base];
        bool parked = cont_in;
        for (int q = 0; q < SF_SEGLEN; ++q) {
          if (q > 0 && ((brk >> q) & 1u)) {
            if (kk != SF_NONE) { if (parked) s_cont[slot * SF_SEG + seg] = sum; else acc[kk] += sum; }
            sum = 0.0; parked = false; kk = s_key[base + q];
          }
          sum += f[q];
        }
        if (kk != SF_NONE) { if (parked) s_cont[slot * SF_SEG + seg] = sum; else acc[kk] += sum; }
      }
      __syncthreads();
      if (on && collects) {
        for (int s2 = seg + 1; s2 < SF_SEG && s_key[s2 * SF_SEGLEN] == tail_key; ++s2) {
          acc[tail_key] += s_cont[slot * SF_SEG + s2];
          if (s_key[s2 * SF_SEGLEN + SF_SEGLEN - 1] != tail_key) break;
        }
      }
    };
    // the A fluxes of step k go to the rows of slot (k % lpb, angle); the batch is added when it is full or the steps end
    double flux[SF_MAX_SZA];
    auto put = [&](int k) {
      double* f = s_f + (size_t)((k % lpb) * nang) * SF_ROW + pos;
#pragma unroll
      for (int s = 0; s < SF_MAX_SZA; ++s)
        if (s < nang) f[s * SF_ROW] = flux[s];
      if ((k + 1) % lpb == 0) reduce_batch(k, lpb);
      else if (k + 1 == nsteps) reduce_batch(k, (k % lpb) + 1);
    };

    // ---- the column, as k_lbl_fluxes_sw computes it, every angle of the launch at once
    const double ssi_j = ssi[j];
#pragma unroll
    for (int s = 0; s < SF_MAX_SZA; ++s) {
      flux[s] = (live && s < nang) ? cos_sza[s] * ssi_j : 0.0;                 // radiative_transfer_sw.cpp:39
      if (SPECTRAL && live && s < nang) spec_dn[(size_t)s * nhl * spec_stride + i] = (float)flux[s];
    }
    put(0);
    for (int l = 0; l < nlay; ++l) {
      const double tau = (double)od[(size_t)l * od_stride + j];
#pragma unroll
      for (int s = 0; s < SF_MAX_SZA; ++s) {
        if (s < nang) {
          flux[s] = flux[s] * exp(minus_sec_sza[s] * tau);
          if (SPECTRAL && live) spec_dn[((size_t)s * nhl + l + 1) * spec_stride + i] = (float)flux[s];
        }
      }
      put(l + 1);
    }
    if (albedo) {                                                             // :70-76
      const double alb = albedo[j];
#pragma unroll
      for (int s = 0; s < SF_MAX_SZA; ++s) {
        flux[s] = flux[s] * alb;
        if (SPECTRAL && live && s < nang) spec_up[((size_t)s * nhl + nlay) * spec_stride + i] = (float)flux[s];
      }
      put(nhl);
      for (int l = nlay - 1; l >= 0; --l) {
        const double t2 = exp(-2.0 * (double)od[(size_t)l * od_stride + j]);  // the same for every angle
#pragma unroll
        for (int s = 0; s < SF_MAX_SZA; ++s) {
          flux[s] = flux[s] * t2;
          if (SPECTRAL && live && s < nang) spec_up[((size_t)s * nhl + l) * spec_stride + i] = (float)flux[s];
        }
        put(nhl + nlay - l);
      }
    } else if (SPECTRAL && live) {
      for (int r = 0; r < nang * nhl; ++r) spec_up[(size_t)r * spec_stride + i] = 0.0f;
    }
    __syncthreads();                                                          // s_raw / s_key / s_cont are rewritten by the next tile
  }
  __syncthreads();
  for (int t = tid; t < nacc; t += SF_THREADS) partial[(size_t)blockIdx.x * nacc + t] = s_acc[t];
}

// out[row0 + row][col_out(c)] = the blocks' partials added in block order; one thread per accumulator entry
__global__ void __launch_bounds__(256)
k_sf_combine(int nblk, int nacc, int ncols, int row0, int g0, int gcount, int out_cols, const double* __restrict__ partial,
             double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nacc) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[(size_t)b * nacc + e];
  const int r = e / ncols, c = e % ncols;
  out[(size_t)(row0 + r) * out_cols + (c < gcount ? g0 + c : out_cols - 1)] = s;
}

int check_angles(const char* who, int nsza, const double* h_cos_sza) {
  ECCKD_REQUIRE(nsza >= 1 && nsza <= SF_MAX_SZA, "%s: nsza (%d) must be between 1 and %d", who, nsza, SF_MAX_SZA);
  for (int s = 0; s < nsza; ++s)
    ECCKD_REQUIRE(h_cos_sza[s] > 0.0 && h_cos_sza[s] <= 1.0, "%s: cos_sza[%d] = %g is not in (0, 1]", who, s, h_cos_sza[s]);
  return ECCKD_OK;
}

// One column.  d_g_point == NULL: one column of the accumulator (the broadband sum); otherwise ng g points + "none".
// h_out[nsza][2][nhl][ng + 1]: direction 0 down, 1 up; column ng = the wavenumbers with no g point.
int run(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_cos_sza, const double* d_ssi, const double* d_albedo,
        const void* d_od, int od_type, size_t od_stride, const int32_t* d_g_point, int ng, float* d_spec_dn, float* d_spec_up,
        size_t spec_stride, std::vector<double>& h_out) {
  const int nhl = nlay + 1;
  const int out_cols = ng + 1;
  const int cap = (int)std::min<size_t>(SF_ACC_BYTES / ((size_t)2 * nhl * sizeof(double)), 1u << 20);   // column-angles per launch
  ECCKD_REQUIRE(cap >= 2, "line-by-line shortwave g-point fluxes: %d layers are more than the block's accumulator holds", nlay);
  // the split (see the header): a function of (nlay, nsza, ng) alone
  int ang_per_launch = 1, cols_per_launch = cap;
  if (cap >= out_cols) {
    const int amax = std::min(nsza, std::min(SF_MAX_SZA, cap / out_cols));
    const int nl = (nsza + amax - 1) / amax;
    ang_per_launch = (nsza + nl - 1) / nl;
    cols_per_launch = out_cols;
  }
  const size_t ntiles = (nwav + SF_THREADS - 1) / SF_THREADS;
  const int tpb = (int)std::max<size_t>(1, (ntiles + SF_TARGET_BLOCKS - 1) / SF_TARGET_BLOCKS);   // a function of nwav alone
  const int nblk = (int)((ntiles + tpb - 1) / tpb);
  const size_t nrows = (size_t)nsza * 2 * nhl;
  const size_t max_acc = (size_t)ang_per_launch * 2 * nhl * std::min(cols_per_launch, out_cols);
  const size_t b_out = ecckd_align_up(nrows * out_cols * sizeof(double), 256);
  const size_t b_part = ecckd_align_up((size_t)nblk * max_acc * sizeof(double), 256);
  const size_t b_ang = ecckd_align_up((size_t)2 * SF_MAX_SZA * sizeof(double), 256);
  ECCKD_CHECK(ecckd::ensure_scratch(ctx, b_ang + b_out + b_part));
  double* d_ang = (double*)ctx->scratch;
  double* d_out = (double*)((char*)ctx->scratch + b_ang);
  double* d_part = (double*)((char*)ctx->scratch + b_ang + b_out);
  double h_ang[2 * SF_MAX_SZA];                    // cos_sza, then -1.0 / cos_sza: divided on the host (IEEE, as on the device)
  for (int s = 0; s < SF_MAX_SZA; ++s) {
    h_ang[s] = s < nsza ? h_cos_sza[s] : 1.0;
    h_ang[SF_MAX_SZA + s] = -1.0 / h_ang[s];
  }
  ECCKD_CHECK(ecckd_h2d(ctx, d_ang, h_ang, sizeof(h_ang)));
  ECCKD_HIP_CHECK(hipMemsetAsync(d_out, 0, nrows * out_cols * sizeof(double), ctx->stream));
  const bool spectral = d_spec_dn != nullptr;
  for (int a0 = 0; a0 < nsza;) {
    const int na = std::min(ang_per_launch, nsza - a0);
    float* spec_dn = spectral ? d_spec_dn + (size_t)a0 * nhl * spec_stride : nullptr;
    float* spec_up = spectral ? d_spec_up + (size_t)a0 * nhl * spec_stride : nullptr;
    // the launches of these angles: g points [g0, g0 + gcount); the first one also bins the points without a g point
    for (int g0 = 0, pass = 0; pass == 0 || g0 < ng; ++pass) {
      const bool with_none = pass == 0;
      const int gcount = std::min(ng - g0, cols_per_launch - (with_none ? 1 : 0));
      const int ncols = gcount + (with_none ? 1 : 0);
      const int col_un = (with_none && d_g_point) ? gcount : -1;
      const int nacc = na * 2 * nhl * ncols;
      const size_t lds = (size_t)nacc * sizeof(double);
#define SF_LAUNCH(T, S)                                                                                                        \
  do {                                                                                                                         \
    ECCKD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_lbl_gpoint_fluxes_sw<T, S>),                           \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)SF_ACC_BYTES));                       \
    hipLaunchKernelGGL((k_lbl_gpoint_fluxes_sw<T, S>), dim3((unsigned)nblk), dim3(SF_THREADS), lds, ctx->stream, nlay, nwav,   \
                       od_stride, tpb, na, (const double*)d_ang + a0, (const double*)d_ang + SF_MAX_SZA + a0, d_ssi, d_albedo, (const T*)d_od, d_g_point, g0, gcount, col_un, ncols, d_part, \
                       spec_dn, spec_up, spec_stride);                                                                         \
  } while (0)
      if (od_type == ECCKD_F32) { if (spectral) SF_LAUNCH(float, true); else SF_LAUNCH(float, false); }
      else { if (spectral) SF_LAUNCH(double, true); else SF_LAUNCH(double, false); }
#undef SF_LAUNCH
      ECCKD_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(k_sf_combine, dim3((unsigned)((nacc + 255) / 256)), dim3(256), 0, ctx->stream, nblk, nacc, ncols,
                         a0 * 2 * nhl, g0, gcount, out_cols, (const double*)d_part, d_out);
      ECCKD_HIP_CHECK(hipGetLastError());
      g0 += gcount;
    }
    a0 += na;
  }
  h_out.resize(nrows * out_cols);
  return ecckd_d2h(ctx, h_out.data(), d_out, h_out.size() * sizeof(double));
}

}  // namespace

extern "C" {

int ecckd_lbl_gpoint_fluxes_sw(ecckd_gmap* gmap, int nlay, int nsza, const double* h_cos_sza, const double* d_ssi,
                               const double* d_albedo, const void* d_od, int od_type, size_t od_stride, double* h_flux_dn_direct,
                               double* h_flux_up, double* h_bb_dn, double* h_bb_up) {
  ECCKD_REQUIRE(gmap && nlay > 0 && h_cos_sza && d_ssi && d_od && h_flux_dn_direct && h_flux_up, "ecckd_lbl_gpoint_fluxes_sw: bad argument");
  ECCKD_CHECK(check_angles("ecckd_lbl_gpoint_fluxes_sw", nsza, h_cos_sza));
  ECCKD_REQUIRE(od_type == ECCKD_F32 || od_type == ECCKD_F64, "ecckd_lbl_gpoint_fluxes_sw: od_type must be 4 or 8");
  ECCKD_REQUIRE(od_stride >= gmap->n, "ecckd_lbl_gpoint_fluxes_sw: od_stride (%zu) < nwav (%zu)", od_stride, gmap->n);
  ecckd_ctx* ctx = gmap->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int32_t* d_g = nullptr; const double* d_wn = nullptr; const double* d_dwn = nullptr;
  ECCKD_CHECK(ecckd::gmap_natural(gmap, &d_g, &d_wn, &d_dwn));
  const int nhl = nlay + 1, ng = gmap->ng;
  std::vector<double> out;
  ECCKD_CHECK(run(ctx, nlay, gmap->n, nsza, h_cos_sza, d_ssi, d_albedo, d_od, od_type, od_stride, d_g, ng, nullptr, nullptr, 0, out));
  for (int s = 0; s < nsza; ++s)
    for (int l = 0; l < nhl; ++l) {
      const double* dn = &out[((size_t)(s * 2) * nhl + l) * (ng + 1)];
      const double* up = &out[((size_t)(s * 2 + 1) * nhl + l) * (ng + 1)];
      double bdn = 0.0, bup = 0.0;                 // every wavenumber: the g points in order, then the points of none
      for (int g = 0; g <= ng; ++g) { bdn += dn[g]; bup += up[g]; }
      const size_t o = (size_t)s * nhl + l;
      for (int g = 0; g < ng; ++g) { h_flux_dn_direct[o * ng + g] = dn[g]; h_flux_up[o * ng + g] = up[g]; }
      if (h_bb_dn) h_bb_dn[o] = bdn;
      if (h_bb_up) h_bb_up[o] = bup;
    }
  return ECCKD_OK;
}

int ecckd_lbl_spectral_fluxes_sw(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_cos_sza, const double* d_ssi,
                                 const double* d_albedo, const void* d_od, int od_type, size_t od_stride, float* d_flux_dn_direct,
                                 float* d_flux_up, size_t flux_stride, double* h_bb_dn, double* h_bb_up) {
  ECCKD_REQUIRE(ctx && nlay > 0 && nwav > 0 && h_cos_sza && d_ssi && d_od && d_flux_dn_direct && d_flux_up,
                "ecckd_lbl_spectral_fluxes_sw: bad argument");
  ECCKD_CHECK(check_angles("ecckd_lbl_spectral_fluxes_sw", nsza, h_cos_sza));
  ECCKD_REQUIRE(od_type == ECCKD_F32 || od_type == ECCKD_F64, "ecckd_lbl_spectral_fluxes_sw: od_type must be 4 or 8");
  ECCKD_REQUIRE(od_stride >= nwav, "ecckd_lbl_spectral_fluxes_sw: od_stride (%zu) < nwav (%zu)", od_stride, nwav);
  ECCKD_REQUIRE(flux_stride >= nwav, "ecckd_lbl_spectral_fluxes_sw: flux_stride (%zu) < nwav (%zu)", flux_stride, nwav);
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int nhl = nlay + 1;
  std::vector<double> out;
  ECCKD_CHECK(run(ctx, nlay, nwav, nsza, h_cos_sza, d_ssi, d_albedo, d_od, od_type, od_stride, nullptr, 0, d_flux_dn_direct,
                  d_flux_up, flux_stride, out));
  for (int s = 0; s < nsza; ++s)
    for (int l = 0; l < nhl; ++l) {
      if (h_bb_dn) h_bb_dn[(size_t)s * nhl + l] = out[(size_t)(s * 2) * nhl + l];
      if (h_bb_up) h_bb_up[(size_t)s * nhl + l] = out[(size_t)(s * 2 + 1) * nhl + l];
    }
  return ECCKD_OK;
}

}  // extern "C"
