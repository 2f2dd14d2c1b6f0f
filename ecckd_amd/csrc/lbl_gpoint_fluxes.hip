// lbl_gpoint_fluxes.hip - line-by-line longwave fluxes of one column resolved per g point (lw_spectra.cpp:222-257): the
// Planck function (planck_function.cpp:22-54), both sweeps of radiative_transfer_lw (radiative_transfer_lw.cpp:27-60, unit
// surface emissivity, diffusivity 1.66 - what k_lbl_fluxes_lw does with nangle = 0, expression by expression) and the sum of
// the spectral flux over the wavenumbers of every g point in ONE pass over the optical depths.  No (nlay+1) x nwav flux
// matrix exists on this path; the other output mode of the same kernel writes exactly that matrix (FLOAT rows) for the
// caller that wants the spectrum, with the broadband sums.
//
// Shape: one thread per wavenumber in natural order, 256 per tile, binned into the g points inside the block - the scheme of
// gpoint_bin.hpp, which says how.  A thread produces nlay fluxes down and nlay + 1 up; they are batched GB_LB at a time in the
// order produced, and flux number idx feeds accumulator row row_of(idx).
// The accumulator has to fit into LDS: at most GF_ACC_BYTES / (16 (nlay+1)) columns per launch; a map with more g points is
// swept in several launches, each binning its own range of g points (ng = 32 ... 46 at 54 layers: one launch).
#include "common.hpp"
#include "gmap.hpp"
#include "gpoint_bin.hpp"
#include "lbl_rt.hpp"

#include <algorithm>
#include <vector>

namespace {

using namespace ecckd::lbl;

// dynamic LDS: acc[2 * nhl][ncols]
template <typename OdT, bool SPECTRAL>
__global__ void __launch_bounds__(GB_THREADS)
k_lbl_gpoint_fluxes_lw(int nlay, size_t nwav, size_t od_stride, int tiles_per_block, const double* __restrict__ hk,
                       const double* __restrict__ wn, const double* __restrict__ dwn, const OdT* __restrict__ od,
                       const int32_t* __restrict__ g_point /* NULL: every point in column 0 */, int g0, int gcount,
                       int col_unassigned /* column of g_point < 0, or -1 */, int ncols, double* __restrict__ partial,
                       float* __restrict__ spec_dn, float* __restrict__ spec_up, size_t spec_stride) {
  extern __shared__ double s_acc[];
  const int nhl = nlay + 1;
  const int tid = threadIdx.x;
  const int nacc = 2 * nhl * ncols;
  for (int t = tid; t < nacc; t += GB_THREADS) s_acc[t] = 0.0;
  // this thread as an adder: level slot and segment
  const int slot = tid / GB_SEG, seg = tid % GB_SEG, base = seg * GB_SEGLEN;
  const double sec = ECCKD_LW_DIFFUSIVITY;
  const double rsec = 1.0 / sec;
  const int nrows = 2 * nlay + 1;                 // fluxes a point produces: nlay down (levels 1..nlay), nlay + 1 up

  const size_t tile0 = (size_t)blockIdx.x * tiles_per_block;
  for (int it = 0; it < tiles_per_block; ++it) {
    const size_t i = (tile0 + it) * GB_THREADS + tid;
    if ((tile0 + it) * GB_THREADS >= nwav) break;                           // (block-uniform)
    const bool live = i < nwav;
    const size_t j = live ? i : nwav - 1;
    const int pos = tile_rank(tid, tile_key(live, g_point, j, g0, gcount, col_unassigned));
    const TilePieces pieces = tile_pieces(seg, base);

    // flux number `idx` of a point (in the order produced) -> accumulator row: down level l -> l, up level l -> nhl + l
    auto row_of = [&](int idx) { return idx < nlay ? idx + 1 : (idx == nlay ? nhl + nlay : nhl + 2 * nlay - idx); };
    auto reduce = [&](int first_idx, int nb) {
      const int r = row_of(first_idx + (slot < nb ? slot : 0));
      reduce_batch(pieces, slot < nb, slot, seg, base, s_acc + (size_t)r * ncols);
    };
    int produced = 0;
    auto emit = [&](double f) {
      s_f[(produced % GB_LB) * GB_ROW + pos] = f;
      ++produced;
      if (produced % GB_LB == 0) reduce(produced - GB_LB, GB_LB);
    };

    // ---- the column (lbl_rt.hpp), nangle = 0
    const double freq = wn_to_freq(wn[j]);
    const double pref = live ? planck_pref(dwn[j], freq) : 0.0;
    auto layer = [&](int l, double& eps, double& fac) { lw_layer(sec, rsec, (double)od[(size_t)l * od_stride + j], eps, fac); };
    double flux = 0.0;
    if (SPECTRAL && live) spec_dn[i] = 0.0f;                                  // nothing comes down at the top (:45)
    double b_prev = planck(pref, freq, hk[0]);
    for (int l = 0; l < nlay; ++l) {                                          // :45-50; dead lanes carry pref = 0
      double eps, fac;
      layer(l, eps, fac);
      const double b_next = planck(pref, freq, hk[l + 1]);
      flux = lw_step(flux, eps, fac, b_prev, b_next);
      if (SPECTRAL && live) spec_dn[(size_t)(l + 1) * spec_stride + i] = (float)flux;
      emit(flux);
      b_prev = b_next;
    }
    flux = lw_surface(flux, b_prev);                                            // :52-53
    if (SPECTRAL && live) spec_up[(size_t)nlay * spec_stride + i] = (float)flux;
    emit(flux);
    for (int l = nlay - 1; l >= 0; --l) {                                     // :55-59
      double eps, fac;
      layer(l, eps, fac);
      const double b_l = planck(pref, freq, hk[l]);
      flux = lw_step(flux, eps, fac, b_prev, b_l);
      if (SPECTRAL && live) spec_up[(size_t)l * spec_stride + i] = (float)flux;
      emit(flux);
      b_prev = b_l;
    }
    if (nrows % GB_LB) reduce(nrows - nrows % GB_LB, nrows % GB_LB);
    __syncthreads();                                                          // the next tile rewrites the binner's arrays
  }
  __syncthreads();
  for (int t = tid; t < nacc; t += GB_THREADS) partial[(size_t)blockIdx.x * nacc + t] = s_acc[t];
}

// The same with the zenith-angle quadrature (nangle > 0 of lw_angle_table): flux = sum_a wgt[a] I[a], every intensity I[a] the
// recurrence above along the slant path sec[a] * tau.  A thread keeps the nang <= LBL_MAX_ANGLES intensities of its wavenumber
// in registers (indexed by unrolled constants only) and walks the layers ONCE down and once up for all of them: per layer tau is
// loaded once and the Planck function of the level evaluated once, then angle after angle lw_layer and lw_step, and the
// level's flux is formed in angle order from 0.0 - the order in which k_lbl_fluxes_lw forms surf_acc / toa_acc.  ONE flux per
// level goes to the binner, so the accumulator, its budget and the launch split are those of the kernel above whatever nang.
// ang = [3][LBL_MAX_ANGLES]: secants, their reciprocals, weights (uniform, constant offsets: scalar loads).
template <typename OdT, bool SPECTRAL>
__global__ void __launch_bounds__(GB_THREADS)
k_lbl_gpoint_fluxes_lw_angles(int nang, const double* __restrict__ ang, int nlay, size_t nwav, size_t od_stride, int tiles_per_block,
                              const double* __restrict__ hk, const double* __restrict__ wn, const double* __restrict__ dwn,
                              const OdT* __restrict__ od, const int32_t* __restrict__ g_point /* NULL: every point in column 0 */,
                              int g0, int gcount, int col_unassigned /* column of g_point < 0, or -1 */, int ncols,
                              double* __restrict__ partial, float* __restrict__ spec_dn, float* __restrict__ spec_up,
                              size_t spec_stride) {
  extern __shared__ double s_acc[];
  const int nhl = nlay + 1;
  const int tid = threadIdx.x;
  const int nacc = 2 * nhl * ncols;
  for (int t = tid; t < nacc; t += GB_THREADS) s_acc[t] = 0.0;
  const int slot = tid / GB_SEG, seg = tid % GB_SEG, base = seg * GB_SEGLEN;
  const int nrows = 2 * nlay + 1;

  const size_t tile0 = (size_t)blockIdx.x * tiles_per_block;
  for (int it = 0; it < tiles_per_block; ++it) {
    const size_t i = (tile0 + it) * GB_THREADS + tid;
    if ((tile0 + it) * GB_THREADS >= nwav) break;                           // (block-uniform)
    const bool live = i < nwav;
    const size_t j = live ? i : nwav - 1;
    const int pos = tile_rank(tid, tile_key(live, g_point, j, g0, gcount, col_unassigned));
    const TilePieces pieces = tile_pieces(seg, base);

    auto row_of = [&](int idx) { return idx < nlay ? idx + 1 : (idx == nlay ? nhl + nlay : nhl + 2 * nlay - idx); };
    auto reduce = [&](int first_idx, int nb) {
      const int r = row_of(first_idx + (slot < nb ? slot : 0));
      reduce_batch(pieces, slot < nb, slot, seg, base, s_acc + (size_t)r * ncols);
    };
    int produced = 0;
    auto emit = [&](double f) {
      s_f[(produced % GB_LB) * GB_ROW + pos] = f;
      ++produced;
      if (produced % GB_LB == 0) reduce(produced - GB_LB, GB_LB);
    };

    // ---- the column (lbl_rt.hpp), every angle at once
    const double freq = wn_to_freq(wn[j]);
    const double pref = live ? planck_pref(dwn[j], freq) : 0.0;
    double inten[LBL_MAX_ANGLES];
#pragma unroll
    for (int a = 0; a < LBL_MAX_ANGLES; ++a) inten[a] = 0.0;
    // one layer for every angle: the intensities stepped from the level with b_prev to the one with b, and the level's flux
    auto step = [&](int l, double b_prev, double b) {
      const double tau = (double)od[(size_t)l * od_stride + j];
      double flux = 0.0;
#pragma unroll
      for (int a = 0; a < LBL_MAX_ANGLES; ++a) {
        if (a < nang) {
          double eps, fac;
          lw_layer(ang[a], ang[LBL_MAX_ANGLES + a], tau, eps, fac);
          inten[a] = lw_step(inten[a], eps, fac, b_prev, b);
          flux += ang[2 * LBL_MAX_ANGLES + a] * inten[a];
        }
      }
      return flux;
    };
    if (SPECTRAL && live) spec_dn[i] = 0.0f;                                  // nothing comes down at the top (:45)
    double b_prev = planck(pref, freq, hk[0]);
    for (int l = 0; l < nlay; ++l) {                                          // :45-50; dead lanes carry pref = 0
      const double b_next = planck(pref, freq, hk[l + 1]);
      const double flux = step(l, b_prev, b_next);
      if (SPECTRAL && live) spec_dn[(size_t)(l + 1) * spec_stride + i] = (float)flux;
      emit(flux);
      b_prev = b_next;
    }
    {                                                                         // :52-53
      double flux = 0.0;
#pragma unroll
      for (int a = 0; a < LBL_MAX_ANGLES; ++a) {
        if (a < nang) {
          inten[a] = lw_surface(inten[a], b_prev);
          flux += ang[2 * LBL_MAX_ANGLES + a] * inten[a];
        }
      }
      if (SPECTRAL && live) spec_up[(size_t)nlay * spec_stride + i] = (float)flux;
      emit(flux);
    }
    for (int l = nlay - 1; l >= 0; --l) {                                     // :55-59
      const double b_l = planck(pref, freq, hk[l]);
      const double flux = step(l, b_prev, b_l);
      if (SPECTRAL && live) spec_up[(size_t)l * spec_stride + i] = (float)flux;
      emit(flux);
      b_prev = b_l;
    }
    if (nrows % GB_LB) reduce(nrows - nrows % GB_LB, nrows % GB_LB);
    __syncthreads();                                                          // the next tile rewrites the binner's arrays
  }
  __syncthreads();
  for (int t = tid; t < nacc; t += GB_THREADS) partial[(size_t)blockIdx.x * nacc + t] = s_acc[t];
}

// One column.  d_g_point == NULL: one column of the accumulator (the broadband sum); otherwise ng g points + "none".
// h_out[2 * nhl][ng + 1]: rows 0..nhl-1 down, nhl.. up; column ng = the wavenumbers with no g point.
// nangle = 0: the two-stream kernel; nangle > 0: the quadrature kernel with sec_wgt of lw_angle_table.
int run(ecckd_ctx* ctx, int nangle, const std::vector<double>& sec_wgt, int nlay, size_t nwav, const double* h_temperature_hl,
        const double* d_wn, const double* d_dwn, const void* d_od, int od_type, size_t od_stride, const int32_t* d_g_point, int ng,
        float* d_spec_dn, float* d_spec_up, size_t spec_stride, std::vector<double>& h_out) {
  const int nhl = nlay + 1;
  const int out_cols = ng + 1;
  const int max_cols = (int)(GF_ACC_BYTES / ((size_t)2 * nhl * sizeof(double)));
  ECCKD_REQUIRE(max_cols >= 2, "line-by-line g-point fluxes: %d layers are more than the block's accumulator holds", nlay);
  std::vector<double> hk;
  ECCKD_CHECK(make_hk("line-by-line g-point fluxes", nhl, h_temperature_hl, hk));
  if (nangle > 0) {                                     // one upload: hk[nhl], then ang[3][LBL_MAX_ANGLES] (unused angles: weight 0)
    hk.resize((size_t)nhl + 3 * LBL_MAX_ANGLES, 0.0);
    for (int a = 0; a < LBL_MAX_ANGLES; ++a) {
      const double sec = a < nangle ? sec_wgt[a] : 1.0;
      hk[nhl + a] = sec;
      hk[nhl + LBL_MAX_ANGLES + a] = 1.0 / sec;         // (IEEE, as k_lbl_fluxes_lw divides on the device)
      hk[nhl + 2 * LBL_MAX_ANGLES + a] = a < nangle ? sec_wgt[nangle + a] : 0.0;
    }
  }
  const TileGrid grid = tile_grid(nwav);
  const int tpb = grid.tpb, nblk = grid.nblk;
  void* d[3];
  ECCKD_CHECK(ecckd::carve_scratch(ctx, {hk.size() * sizeof(double), (size_t)2 * nhl * out_cols * sizeof(double),
                                         (size_t)nblk * 2 * nhl * std::min(max_cols, out_cols) * sizeof(double)}, d));
  double* d_hk = (double*)d[0];
  double* d_out = (double*)d[1];
  double* d_part = (double*)d[2];
  ECCKD_CHECK(ecckd_h2d(ctx, d_hk, hk.data(), hk.size() * sizeof(double)));
  ECCKD_HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)2 * nhl * out_cols * sizeof(double), ctx->stream));
  const bool spectral = d_spec_dn != nullptr;
  auto launch = [&](int g0, int gcount, int col_un, int ncols) {
    const size_t lds = (size_t)2 * nhl * ncols * sizeof(double);
    with_od_type(od_type, [&](auto t) {
      using OdT = decltype(t);
      if (nangle > 0) {
        const auto kernel = spectral ? k_lbl_gpoint_fluxes_lw_angles<OdT, true> : k_lbl_gpoint_fluxes_lw_angles<OdT, false>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(GB_THREADS), lds, ctx->stream, nangle, (const double*)d_hk + nhl, nlay,
                           nwav, od_stride, tpb, (const double*)d_hk, d_wn, d_dwn, (const OdT*)d_od, d_g_point, g0, gcount, col_un,
                           ncols, d_part, d_spec_dn, d_spec_up, spec_stride);
        return;
      }
      const auto kernel = spectral ? k_lbl_gpoint_fluxes_lw<OdT, true> : k_lbl_gpoint_fluxes_lw<OdT, false>;
      hipLaunchKernelGGL(kernel, dim3((unsigned)nblk), dim3(GB_THREADS), lds, ctx->stream, nlay, nwav, od_stride, tpb,
                         (const double*)d_hk, d_wn, d_dwn, (const OdT*)d_od, d_g_point, g0, gcount, col_un, ncols, d_part,
                         d_spec_dn, d_spec_up, spec_stride);
    });
    return ECCKD_OK;
  };
  ECCKD_CHECK(bin_column_ranges(ctx, ng, d_g_point != nullptr, max_cols, nblk, 2 * nhl, 0, d_part, d_out, launch));
  h_out.resize((size_t)2 * nhl * out_cols);
  return ecckd_d2h(ctx, h_out.data(), d_out, h_out.size() * sizeof(double));
}

}  // namespace

extern "C" {

int ecckd_lbl_gpoint_fluxes_lw(ecckd_gmap* gmap, int nlay, const double* h_temperature_hl, const void* d_od, int od_type,
                               size_t od_stride, double* h_flux_dn, double* h_flux_up, double* h_bb_dn, double* h_bb_up) {
  return ecckd_lbl_gpoint_fluxes_lw_angles(gmap, 0, nlay, h_temperature_hl, d_od, od_type, od_stride, h_flux_dn, h_flux_up, h_bb_dn,
                                           h_bb_up);
}

int ecckd_lbl_gpoint_fluxes_lw_angles(ecckd_gmap* gmap, int nangle, int nlay, const double* h_temperature_hl, const void* d_od,
                                      int od_type, size_t od_stride, double* h_flux_dn, double* h_flux_up, double* h_bb_dn,
                                      double* h_bb_up) {
  int nang = 0;
  std::vector<double> sec_wgt;
  ECCKD_CHECK(lw_angle_table("ecckd_lbl_gpoint_fluxes_lw", nangle, &nang, sec_wgt));
  ECCKD_REQUIRE(gmap && nlay > 0 && h_temperature_hl && d_od && h_flux_dn && h_flux_up, "ecckd_lbl_gpoint_fluxes_lw: bad argument");
  ECCKD_CHECK(check_od("ecckd_lbl_gpoint_fluxes_lw", od_type, od_stride, gmap->n));
  ecckd_ctx* ctx = gmap->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int32_t* d_g = nullptr; const double* d_wn = nullptr; const double* d_dwn = nullptr;
  ECCKD_CHECK(ecckd::gmap_natural(gmap, &d_g, &d_wn, &d_dwn));
  const int nhl = nlay + 1, ng = gmap->ng;
  std::vector<double> out;
  ECCKD_CHECK(run(ctx, nangle, sec_wgt, nlay, gmap->n, h_temperature_hl, d_wn, d_dwn, d_od, od_type, od_stride, d_g, ng, nullptr,
                  nullptr, 0, out));
  unpack_gpoint_out(out.data(), 1, nhl, ng, h_flux_dn, h_flux_up, h_bb_dn, h_bb_up);
  return ECCKD_OK;
}

int ecckd_lbl_spectral_fluxes_lw(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_temperature_hl,
                                 const double* d_wavenumber, const double* d_d_wavenumber, const void* d_od, int od_type,
                                 size_t od_stride, float* d_flux_dn, float* d_flux_up, size_t flux_stride, double* h_bb_dn,
                                 double* h_bb_up) {
  return ecckd_lbl_spectral_fluxes_lw_angles(ctx, 0, nlay, nwav, h_temperature_hl, d_wavenumber, d_d_wavenumber, d_od, od_type,
                                             od_stride, d_flux_dn, d_flux_up, flux_stride, h_bb_dn, h_bb_up);
}

int ecckd_lbl_spectral_fluxes_lw_angles(ecckd_ctx* ctx, int nangle, int nlay, size_t nwav, const double* h_temperature_hl,
                                        const double* d_wavenumber, const double* d_d_wavenumber, const void* d_od, int od_type,
                                        size_t od_stride, float* d_flux_dn, float* d_flux_up, size_t flux_stride, double* h_bb_dn,
                                        double* h_bb_up) {
  int nang = 0;
  std::vector<double> sec_wgt;
  ECCKD_CHECK(lw_angle_table("ecckd_lbl_spectral_fluxes_lw", nangle, &nang, sec_wgt));
  ECCKD_REQUIRE(ctx && nlay > 0 && nwav > 0 && h_temperature_hl && d_wavenumber && d_d_wavenumber && d_od && d_flux_dn && d_flux_up,
                "ecckd_lbl_spectral_fluxes_lw: bad argument");
  ECCKD_CHECK(check_od("ecckd_lbl_spectral_fluxes_lw", od_type, od_stride, nwav));
  ECCKD_REQUIRE(flux_stride >= nwav, "ecckd_lbl_spectral_fluxes_lw: flux_stride (%zu) < nwav (%zu)", flux_stride, nwav);
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int nhl = nlay + 1;
  std::vector<double> out;
  ECCKD_CHECK(run(ctx, nangle, sec_wgt, nlay, nwav, h_temperature_hl, d_wavenumber, d_d_wavenumber, d_od, od_type, od_stride, nullptr,
                  0, d_flux_dn, d_flux_up, flux_stride, out));
  unpack_gpoint_out(out.data(), 1, nhl, 0, nullptr, nullptr, h_bb_dn, h_bb_up);   // one column: the broadband sums
  return ECCKD_OK;
}

}  // extern "C"
