// lbl_fluxes_sw_rayleigh.hip - line-by-line shortwave band fluxes of one column with Rayleigh scattering: the two-stream
// transfer of lbl_rt.hpp (rayleigh_layer, rayleigh_up, rayleigh_down) per wavenumber, which the reference does not contain
// (it masks the upwelling fluxes it cannot represent, LblFluxes::mask_rayleigh_up); the external CKDMIP shortwave tool scatters
// by the rayleigh_optical_depth that run_ckd writes apart for it (run_ckd.cpp:166-192).
//
// One thread per wavenumber of a BandChunk, nsza = 1..8 solar zenith angles per launch, angle after angle.  The adding method
// runs up the column and then down it, so a thread needs per level what the other sweep left: the direct flux D (written by
// the first sweep down, the chain of k_lbl_fluxes_sw), and the albedo A and source S below each level (written by the sweep
// up).  That is 3 (nlay + 1) doubles per thread for the angle in hand - 1.3 KB at 54 layers, too much for registers and, at
// 256 threads, for the LDS a block should take - so it lives in a device workspace [block][slot][level][thread]: a thread
// writes and later reads only its own element, every access coalesced, no barrier needed.  The layer terms are computed again
// in each sweep from the two optical depths rather than stored (two exp, a sqrt and three divisions against five more
// doubles per level written and read).  The grid is bounded (RAYLEIGH_BLOCKS_PER_CU blocks per compute unit, or
// ECCKD_RAYLEIGH_GRID blocks) and its blocks loop over the chunks, so the workspace is sized by the grid, not by nwav.
// Per level the fluxes of a block are reduced wave -> block in the fixed order of k_lbl_fluxes_sw and written as chunk
// partials per angle, which the host adds in chunk order (bitwise reproducible, and an angle's bits do not depend on the
// angles computed with it).
#include "common.hpp"
#include "lbl_rt.hpp"

#include <cstdlib>
#include <vector>

namespace {

using namespace ecckd::lbl;

// LDS: acc[4][3][nhl]; ws: [gridDim.x][3][nhl][LBL_THREADS]; partial: [nchunk][nsza][3][nhl]
template <typename AbsT, typename RayT>
__global__ void __launch_bounds__(LBL_THREADS)
k_lbl_fluxes_sw_rayleigh(int nlay, int nsza, int nchunk, size_t nwav, size_t abs_stride, size_t ray_stride,
                         const BandChunk* __restrict__ chunks, const double* __restrict__ ang /* sw_angle_table */,
                         const double* __restrict__ ssi, const double* __restrict__ albedo /* per wavenumber or NULL */,
                         const AbsT* __restrict__ od_abs, const RayT* __restrict__ od_ray, double* ws, double* __restrict__ partial,
                         double* __restrict__ surf_dn_direct /* [nsza][nwav] or NULL */, double* __restrict__ surf_dn /* same */,
                         double* __restrict__ toa_up /* same */) {
  extern __shared__ double s_acc[];
  const int nhl = nlay + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* acc_dir = s_acc + wave * RAYLEIGH_FLUXES * nhl;
  double* acc_dn = acc_dir + nhl;
  double* acc_up = acc_dn + nhl;
  double* my = ws + (size_t)blockIdx.x * RAYLEIGH_SLOTS * nhl * LBL_THREADS + tid;
  double* w_d = my;                                        // element (slot, level) of this thread: [(slot * nhl + level) * LBL_THREADS]
  double* w_a = my + (size_t)nhl * LBL_THREADS;
  double* w_s = my + (size_t)2 * nhl * LBL_THREADS;
  for (int ci = blockIdx.x; ci < nchunk; ci += gridDim.x) {
    const BandChunk c = chunks[ci];
    const long long i = c.i1 + tid;
    const bool live = i <= c.i2;
    const size_t j = live ? (size_t)i : (size_t)c.i2;
    const double inc = ssi[j];
    const double alb = albedo ? albedo[j] : 0.0;
    auto layer = [&](int l, double mu0, double minus_sec_sza) {
      return rayleigh_layer((double)od_abs[(size_t)l * abs_stride + j], (double)od_ray[(size_t)l * ray_stride + j], mu0, minus_sec_sza);
    };
    for (int s = 0; s < nsza; ++s) {
      const double cos_sza = ang[s], minus_sec_sza = ang[LBL_MAX_SZA + s];     // (uniform: scalar loads)
      for (int t = tid; t < 4 * RAYLEIGH_FLUXES * nhl; t += LBL_THREADS) s_acc[t] = 0.0;
      __syncthreads();
      // the direct beam, as k_lbl_fluxes_sw on tau_abs + tau_ray; dead lanes carry no flux at all
      double flux = live ? cos_sza * inc : 0.0;
      w_d[0] = flux;
      for (int l = 0; l < nlay; ++l) {
        const double tau = (double)od_abs[(size_t)l * abs_stride + j] + (double)od_ray[(size_t)l * ray_stride + j];
        flux = flux * exp(minus_sec_sza * tau);
        w_d[(size_t)(l + 1) * LBL_THREADS] = flux;
      }
      if (surf_dn_direct && live) surf_dn_direct[(size_t)s * nwav + j] = flux;
      const double d_surf = flux;
      // up: the albedo and the source below every level
      double a = alb, src = alb * flux;
      w_a[(size_t)nlay * LBL_THREADS] = a;
      w_s[(size_t)nlay * LBL_THREADS] = src;
      for (int l = nlay - 1; l >= 0; --l) {
        const RayleighLayer L = layer(l, cos_sza, minus_sec_sza);
        rayleigh_up(L, w_d[(size_t)l * LBL_THREADS], a, src, a, src);
        w_a[(size_t)l * LBL_THREADS] = a;
        w_s[(size_t)l * LBL_THREADS] = src;
      }
      // down: the diffuse and the upwelling flux at every level.  The direct flux is summed here, from the value the first sweep
      // stored, and not where it is computed: there the product flux * exp() would fuse into the first addition of the wave's sum,
      // and direct and total would differ in the last bit where nothing scatters.
      double dn = 0.0, up = src;
      double d_top = w_d[0];
      wave_add(&acc_dir[0], lane, d_top);
      wave_add(&acc_dn[0], lane, dn + d_top);
      wave_add(&acc_up[0], lane, up);
      if (toa_up && live) toa_up[(size_t)s * nwav + j] = up;
      for (int l = 0; l < nlay; ++l) {
        const RayleighLayer L = layer(l, cos_sza, minus_sec_sza);
        rayleigh_down(L, d_top, w_a[(size_t)(l + 1) * LBL_THREADS], w_s[(size_t)(l + 1) * LBL_THREADS], dn, dn, up);
        d_top = w_d[(size_t)(l + 1) * LBL_THREADS];
        wave_add(&acc_dir[l + 1], lane, d_top);
        wave_add(&acc_dn[l + 1], lane, dn + d_top);
        wave_add(&acc_up[l + 1], lane, up);
      }
      if (surf_dn && live) surf_dn[(size_t)s * nwav + j] = dn + d_surf;
      __syncthreads();
      for (int t = tid; t < RAYLEIGH_FLUXES * nhl; t += LBL_THREADS)
        partial[((size_t)ci * nsza + s) * RAYLEIGH_FLUXES * nhl + t] = add_waves(s_acc, RAYLEIGH_FLUXES * nhl, t);
      __syncthreads();
    }
  }
}

}  // namespace

extern "C" {

int ecckd_lbl_band_fluxes_sw_rayleigh(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_cos_sza, const double* d_ssi,
                                      const double* d_albedo, const void* d_od_abs, int abs_type, size_t abs_stride,
                                      const void* d_od_ray, int ray_type, size_t ray_stride, int nband, const int64_t* h_band_begin,
                                      const int64_t* h_band_end, double* h_flux_dn_direct, double* h_flux_dn, double* h_flux_up,
                                      double* d_surf_dn_direct, double* d_surf_dn, double* d_toa_up) {
  const char* who = "ecckd_lbl_band_fluxes_sw_rayleigh";
  ECCKD_REQUIRE(ctx && nlay > 0 && h_cos_sza && d_ssi && d_od_abs && d_od_ray && nband > 0 && h_band_begin && h_band_end &&
                h_flux_dn_direct && h_flux_dn && h_flux_up, "%s: bad argument", who);
  double h_ang[2 * LBL_MAX_SZA];
  ECCKD_CHECK(sw_angle_table(who, nsza, h_cos_sza, h_ang));
  ECCKD_CHECK(check_od(who, abs_type, abs_stride, nwav));
  ECCKD_CHECK(check_od(who, ray_type, ray_stride, nwav));
  const size_t nhl = (size_t)nlay + 1;
  const size_t lds = (size_t)4 * RAYLEIGH_FLUXES * nhl * sizeof(double);
  ECCKD_REQUIRE(lds <= 64 * 1024, "%s: nlay = %d needs %zu bytes of LDS for the level sums (64 KB at most)", who, nlay, lds);
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  BandRun r;
  const size_t rows = (size_t)nsza;
  ECCKD_CHECK(band_start(r, ctx, who, nwav, nband, h_band_begin, h_band_end, nhl, {{d_surf_dn_direct, rows}, {d_surf_dn, rows}, {d_toa_up, rows}},
                         {h_flux_dn_direct, h_flux_dn, h_flux_up}, rows));
  if (r.chunks.empty()) return ECCKD_OK;
  const size_t nchunk = r.chunks.size(), grid = rayleigh_grid(ctx, nchunk);
  ECCKD_CHECK(band_device(r, h_ang, 2 * LBL_MAX_SZA, nullptr, 0, nchunk * nsza * RAYLEIGH_FLUXES * nhl,
                          grid * RAYLEIGH_SLOTS * nhl * LBL_THREADS * sizeof(double)));
  with_od_type(abs_type, [&](auto ta) {
    with_od_type(ray_type, [&](auto tr) {
      using AbsT = decltype(ta);
      using RayT = decltype(tr);
      hipLaunchKernelGGL((k_lbl_fluxes_sw_rayleigh<AbsT, RayT>), dim3((unsigned)grid), dim3(LBL_THREADS), lds, ctx->stream, nlay, nsza,
                         (int)nchunk, nwav, abs_stride, ray_stride, r.d_chunks, r.d_tab0, d_ssi, d_albedo, (const AbsT*)d_od_abs,
                         (const RayT*)d_od_ray, (double*)r.d_work, r.d_part, d_surf_dn_direct, d_surf_dn, d_toa_up);
    });
  });
  ECCKD_HIP_CHECK(hipGetLastError());
  return band_collect(r, nsza, nullptr, {h_flux_dn_direct, h_flux_dn, h_flux_up});
}

}  // extern "C"
