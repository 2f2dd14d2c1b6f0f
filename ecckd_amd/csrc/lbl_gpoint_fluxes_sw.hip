// lbl_gpoint_fluxes_sw.hip - line-by-line shortwave fluxes of one column resolved per g point, for up to LBL_MAX_SZA solar
// zenith angles at once: radiative_transfer_direct_sw and radiative_transfer_norayleigh_sw (radiative_transfer_sw.cpp:26-77),
// the steps lbl_rt.hpp lists, which k_lbl_fluxes_sw (lbl_fluxes.hip) takes per wavenumber too, and the sum of every flux row over
// the wavenumbers of every g point in one pass over the optical depths.  The other output mode of the same kernel writes the
// spectral fluxes themselves (FLOAT rows) with the broadband sums.
//
// Shape: that of k_lbl_gpoint_fluxes_lw (lbl_gpoint_fluxes.hip): one thread per wavenumber in natural order, 256 per tile,
// binned into the g points inside the block - the scheme of gpoint_bin.hpp, which says how.  Bitwise reproducible.
//
// Angles.  A launch carries A <= 8 angles.  A thread keeps the A fluxes of its wavenumber in registers and walks the layers
// ONCE down and once up: tau_l is loaded once per sweep for all angles, and exp(-2.0 * tau_l) of the upwelling sweep, which
// does not depend on the angle, is evaluated once per (point, layer) and multiplied into every angle's flux in the reference's
// order (no cumulative transmission: the rounding is that of A separate calls).  Per point and launch: nlay (A + 1)
// exponentials.  A batch of the binning is GB_LB / A levels x A angles (at most GB_LB = 8 rows).
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
#include "gpoint_bin.hpp"
#include "lbl_rt.hpp"

#include <algorithm>
#include <vector>

namespace {

using namespace ecckd::lbl;

// dynamic LDS: acc[A][2][nhl][ncols]
template <typename OdT, bool SPECTRAL>
__global__ void __launch_bounds__(GB_THREADS)
k_lbl_gpoint_fluxes_sw(int nlay, size_t nwav, size_t od_stride, int tiles_per_block, int nang,
                       const double* __restrict__ cos_sza, const double* __restrict__ minus_sec_sza /* [nang]: -1.0 / cos_sza */,
                       const double* __restrict__ ssi, const double* __restrict__ albedo /* per wavenumber or NULL */,
                       const OdT* __restrict__ od, const int32_t* __restrict__ g_point /* NULL: every point in column 0 */,
                       int g0, int gcount, int col_unassigned /* column of g_point < 0, or -1 */, int ncols,
                       double* __restrict__ partial, float* __restrict__ spec_dn, float* __restrict__ spec_up /* [nang][nhl][stride] */,
                       size_t spec_stride) {
  extern __shared__ double s_acc[];
  const int nhl = nlay + 1;
  const int tid = threadIdx.x;
  const int nacc = nang * 2 * nhl * ncols;
  for (int t = tid; t < nacc; t += GB_THREADS) s_acc[t] = 0.0;
  // this thread as an adder: row slot = (level of the batch, angle) and segment
  const int slot = tid / GB_SEG, seg = tid % GB_SEG, base = seg * GB_SEGLEN;
  const int lpb = GB_LB / nang;                   // levels per batch
  const int slot_lev = slot / nang, slot_ang = slot % nang;
  const int nsteps = albedo ? 2 * nhl : nhl;      // step k < nhl: down at level k; k >= nhl: up at level nlay - (k - nhl)

  const size_t tile0 = (size_t)blockIdx.x * tiles_per_block;
  for (int it = 0; it < tiles_per_block; ++it) {
    const size_t i = (tile0 + it) * GB_THREADS + tid;
    if ((tile0 + it) * GB_THREADS >= nwav) break;                           // (block-uniform)
    const bool live = i < nwav;
    const size_t j = live ? i : nwav - 1;
    const int pos = tile_rank(tid, tile_key(live, g_point, j, g0, gcount, col_unassigned));
    const TilePieces pieces = tile_pieces(seg, base);

    // the batch that ends with step `last` (nl levels of it): rows (angle, direction, level) of the accumulator
    auto reduce = [&](int last, int nl) {
      const bool on = slot_lev < nl && slot < lpb * nang;
      const int k = last - (nl - 1) + (on ? slot_lev : 0);
      const int r = (slot_ang * 2 + (k >= nhl ? 1 : 0)) * nhl + (k >= nhl ? nlay - (k - nhl) : k);
      reduce_batch(pieces, on, slot, seg, base, s_acc + (size_t)r * ncols);
    };
    // the A fluxes of step k go to the rows of slot (k % lpb, angle); the batch is added when it is full or the steps end
    double flux[LBL_MAX_SZA];
    auto put = [&](int k) {
      double* f = s_f + (size_t)((k % lpb) * nang) * GB_ROW + pos;
#pragma unroll
      for (int s = 0; s < LBL_MAX_SZA; ++s)
        if (s < nang) f[s * GB_ROW] = flux[s];
      if ((k + 1) % lpb == 0) reduce(k, lpb);
      else if (k + 1 == nsteps) reduce(k, (k % lpb) + 1);
    };

    // ---- the column (the shortwave steps of lbl_rt.hpp), every angle of the launch at once
    const double ssi_j = ssi[j];
#pragma unroll
    for (int s = 0; s < LBL_MAX_SZA; ++s) {
      flux[s] = (live && s < nang) ? cos_sza[s] * ssi_j : 0.0;                 // radiative_transfer_sw.cpp:39
      if (SPECTRAL && live && s < nang) spec_dn[(size_t)s * nhl * spec_stride + i] = (float)flux[s];
    }
    put(0);
    for (int l = 0; l < nlay; ++l) {
      const double tau = (double)od[(size_t)l * od_stride + j];
#pragma unroll
      for (int s = 0; s < LBL_MAX_SZA; ++s) {
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
      for (int s = 0; s < LBL_MAX_SZA; ++s) {
        flux[s] = flux[s] * alb;
        if (SPECTRAL && live && s < nang) spec_up[((size_t)s * nhl + nlay) * spec_stride + i] = (float)flux[s];
      }
      put(nhl);
      for (int l = nlay - 1; l >= 0; --l) {
        const double t2 = exp(-2.0 * (double)od[(size_t)l * od_stride + j]);  // the same for every angle
#pragma unroll
        for (int s = 0; s < LBL_MAX_SZA; ++s) {
          flux[s] = flux[s] * t2;
          if (SPECTRAL && live && s < nang) spec_up[((size_t)s * nhl + l) * spec_stride + i] = (float)flux[s];
        }
        put(nhl + nlay - l);
      }
    } else if (SPECTRAL && live) {
      for (int r = 0; r < nang * nhl; ++r) spec_up[(size_t)r * spec_stride + i] = 0.0f;
    }
    __syncthreads();                                                          // the next tile rewrites the binner's arrays
  }
  __syncthreads();
  for (int t = tid; t < nacc; t += GB_THREADS) partial[(size_t)blockIdx.x * nacc + t] = s_acc[t];
}

// One column.  d_g_point == NULL: one column of the accumulator (the broadband sum); otherwise ng g points + "none".
// h_out[nsza][2][nhl][ng + 1]: direction 0 down, 1 up; column ng = the wavenumbers with no g point.
int run(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_ang /* sw_angle_table */, const double* d_ssi,
        const double* d_albedo, const void* d_od, int od_type, size_t od_stride, const int32_t* d_g_point, int ng, float* d_spec_dn, float* d_spec_up,
        size_t spec_stride, std::vector<double>& h_out) {
  const int nhl = nlay + 1;
  const int out_cols = ng + 1;
  const int cap = (int)std::min<size_t>(SF_ACC_BYTES / ((size_t)2 * nhl * sizeof(double)), 1u << 20);   // column-angles per launch
  ECCKD_REQUIRE(cap >= 2, "line-by-line shortwave g-point fluxes: %d layers are more than the block's accumulator holds", nlay);
  // the split (see the header): a function of (nlay, nsza, ng) alone
  int ang_per_launch = 1, cols_per_launch = cap;
  if (cap >= out_cols) {
    const int amax = std::min(nsza, std::min(LBL_MAX_SZA, cap / out_cols));
    const int nl = (nsza + amax - 1) / amax;
    ang_per_launch = (nsza + nl - 1) / nl;
    cols_per_launch = out_cols;
  }
  const TileGrid grid = tile_grid(nwav);
  const int tpb = grid.tpb, nblk = grid.nblk;
  const size_t nrows = (size_t)nsza * 2 * nhl;
  const size_t max_acc = (size_t)ang_per_launch * 2 * nhl * std::min(cols_per_launch, out_cols);
  void* d[3];
  ECCKD_CHECK(ecckd::carve_scratch(ctx, {(size_t)2 * LBL_MAX_SZA * sizeof(double), nrows * out_cols * sizeof(double),
                                         (size_t)nblk * max_acc * sizeof(double)}, d));
  double* d_ang = (double*)d[0];
  double* d_out = (double*)d[1];
  double* d_part = (double*)d[2];
  ECCKD_CHECK(ecckd_h2d(ctx, d_ang, h_ang, 2 * LBL_MAX_SZA * sizeof(double)));
  ECCKD_HIP_CHECK(hipMemsetAsync(d_out, 0, nrows * out_cols * sizeof(double), ctx->stream));
  const bool spectral = d_spec_dn != nullptr;
  for (int a0 = 0; a0 < nsza;) {
    const int na = std::min(ang_per_launch, nsza - a0);
    float* spec_dn = spectral ? d_spec_dn + (size_t)a0 * nhl * spec_stride : nullptr;
    float* spec_up = spectral ? d_spec_up + (size_t)a0 * nhl * spec_stride : nullptr;
    auto launch = [&](int g0, int gcount, int col_un, int ncols) {
      const size_t lds = (size_t)na * 2 * nhl * ncols * sizeof(double);
      return with_od_type(od_type, [&](auto t) {
        using OdT = decltype(t);
        const auto kernel = spectral ? k_lbl_gpoint_fluxes_sw<OdT, true> : k_lbl_gpoint_fluxes_sw<OdT, false>;
        ECCKD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)SF_ACC_BYTES));
        hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(GB_THREADS), lds, ctx->stream, nlay, nwav, od_stride, tpb, na,
                           (const double*)d_ang + a0, (const double*)d_ang + LBL_MAX_SZA + a0, d_ssi, d_albedo, (const OdT*)d_od,
                           d_g_point, g0, gcount, col_un, ncols, d_part, spec_dn, spec_up, spec_stride);
        return ECCKD_OK;
      });
    };
    ECCKD_CHECK(bin_column_ranges(ctx, ng, d_g_point != nullptr, cols_per_launch, nblk, na * 2 * nhl, a0 * 2 * nhl, d_part, d_out,
                                  launch));
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
  double h_ang[2 * LBL_MAX_SZA];
  ECCKD_CHECK(sw_angle_table("ecckd_lbl_gpoint_fluxes_sw", nsza, h_cos_sza, h_ang));
  ECCKD_CHECK(check_od("ecckd_lbl_gpoint_fluxes_sw", od_type, od_stride, gmap->n));
  ecckd_ctx* ctx = gmap->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int32_t* d_g = nullptr; const double* d_wn = nullptr; const double* d_dwn = nullptr;
  ECCKD_CHECK(ecckd::gmap_natural(gmap, &d_g, &d_wn, &d_dwn));
  const int nhl = nlay + 1, ng = gmap->ng;
  std::vector<double> out;
  ECCKD_CHECK(run(ctx, nlay, gmap->n, nsza, h_ang, d_ssi, d_albedo, d_od, od_type, od_stride, d_g, ng, nullptr, nullptr, 0, out));
  unpack_gpoint_out(out.data(), nsza, nhl, ng, h_flux_dn_direct, h_flux_up, h_bb_dn, h_bb_up);
  return ECCKD_OK;
}

int ecckd_lbl_spectral_fluxes_sw(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_cos_sza, const double* d_ssi,
                                 const double* d_albedo, const void* d_od, int od_type, size_t od_stride, float* d_flux_dn_direct,
                                 float* d_flux_up, size_t flux_stride, double* h_bb_dn, double* h_bb_up) {
  ECCKD_REQUIRE(ctx && nlay > 0 && nwav > 0 && h_cos_sza && d_ssi && d_od && d_flux_dn_direct && d_flux_up,
                "ecckd_lbl_spectral_fluxes_sw: bad argument");
  double h_ang[2 * LBL_MAX_SZA];
  ECCKD_CHECK(sw_angle_table("ecckd_lbl_spectral_fluxes_sw", nsza, h_cos_sza, h_ang));
  ECCKD_CHECK(check_od("ecckd_lbl_spectral_fluxes_sw", od_type, od_stride, nwav));
  ECCKD_REQUIRE(flux_stride >= nwav, "ecckd_lbl_spectral_fluxes_sw: flux_stride (%zu) < nwav (%zu)", flux_stride, nwav);
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int nhl = nlay + 1;
  std::vector<double> out;
  ECCKD_CHECK(run(ctx, nlay, nwav, nsza, h_ang, d_ssi, d_albedo, d_od, od_type, od_stride, nullptr, 0, d_flux_dn_direct,
                  d_flux_up, flux_stride, out));
  unpack_gpoint_out(out.data(), nsza, nhl, 0, nullptr, nullptr, h_bb_dn, h_bb_up);   // one column: the broadband sums
  return ECCKD_OK;
}

}  // extern "C"
