// lbl_fluxes.hip - line-by-line band fluxes of one column (a stand-in for the external
// CKDMIP tool that test/run_lw_lbl_evaluation.sh uses to make the training fluxes, restricted to the
// no-scattering radiative transfer the reference itself contains):
//   longwave:  planck_function (planck_function.cpp:22-54) + radiative_transfer_lw (radiative_transfer_lw.cpp:27-60,
//              unit surface emissivity, surface Planck function at temperature_hl(end)), fluxes summed per band;
//   shortwave: radiative_transfer_direct_sw / _norayleigh_sw (radiative_transfer_sw.cpp:26-77).
// One thread per wavenumber, its transfer that of lbl_rt.hpp; per half level the fluxes of a block are reduced wave -> block
// in a fixed order and written as chunk partials, which the host adds in chunk order (bitwise reproducible).
#include "common.hpp"
#include "lbl_rt.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

using namespace ecckd::lbl;

// LDS: acc[4][2*nhl]
template <typename OdT>
__global__ void __launch_bounds__(LBL_THREADS)
k_lbl_fluxes_lw(int nang, const double* __restrict__ ang /*[nang] secants, [nang] weights*/, int nlay, size_t od_stride,
                const BandChunk* __restrict__ chunks, const double* __restrict__ hk, const double* __restrict__ wn, const double* __restrict__ dwn, const OdT* __restrict__ od,
                double* __restrict__ partial, double* __restrict__ surf_dn /* [nwav] or NULL */,
                double* __restrict__ toa_up /* [nwav] or NULL */) {
  extern __shared__ double s_acc[];
  const int nhl = nlay + 1;
  const BandChunk c = chunks[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int t = tid; t < 4 * 2 * nhl; t += LBL_THREADS) s_acc[t] = 0.0;
  __syncthreads();
  double* acc_dn = s_acc + wave * 2 * nhl;
  double* acc_up = acc_dn + nhl;
  const long long i = c.i1 + tid;
  const bool live = i <= c.i2;
  const size_t j = live ? (size_t)i : (size_t)c.i2;
  const double freq = wn_to_freq(wn[j]);
  const double pref = live ? planck_pref(dwn[j], freq) : 0.0;
  double surf_acc = 0.0, toa_acc = 0.0;
  for (int a = 0; a < nang; ++a) {
    const double sec = ang[a], wgt = ang[nang + a];          // (uniform: scalar loads)
    const double rsec = 1.0 / sec;
    auto layer = [&](int l, double& eps, double& fac) { lw_layer(sec, rsec, (double)od[(size_t)l * od_stride + j], eps, fac); };
    // down sweep from zero at the top of the atmosphere (:45-50); dead lanes carry pref = 0 -> all fluxes 0
    double flux = 0.0;
    double b_prev = planck(pref, freq, hk[0]);
    for (int l = 0; l < nlay; ++l) {
      double eps, fac;
      layer(l, eps, fac);
      const double b_next = planck(pref, freq, hk[l + 1]);
      flux = lw_step(flux, eps, fac, b_prev, b_next);
      wave_add(&acc_dn[l + 1], lane, wgt * flux);
      b_prev = b_next;
    }
    surf_acc += wgt * flux;                         // the spectral flux at the boundary (do_write_spectral_boundary_fluxes)
    // surface: emissivity 1, Planck function at temperature_hl(end) (:52-53)
    flux = lw_surface(flux, b_prev);
    wave_add(&acc_up[nlay], lane, wgt * flux);
    for (int l = nlay - 1; l >= 0; --l) {                                    // :55-59
      double eps, fac;
      layer(l, eps, fac);
      const double b_l = planck(pref, freq, hk[l]);
      flux = lw_step(flux, eps, fac, b_prev, b_l);
      wave_add(&acc_up[l], lane, wgt * flux);
      b_prev = b_l;
    }
    toa_acc += wgt * flux;
  }
  if (surf_dn && live) surf_dn[j] = surf_acc;
  if (toa_up && live) toa_up[j] = toa_acc;
  __syncthreads();
  for (int t = tid; t < 2 * nhl; t += LBL_THREADS)
    partial[(size_t)blockIdx.x * 2 * nhl + t] = add_waves(s_acc, 2 * nhl, t);
}

template <typename OdT>
__global__ void __launch_bounds__(LBL_THREADS)
k_lbl_fluxes_sw(int nlay, size_t od_stride, const BandChunk* __restrict__ chunks, double cos_sza,
                const double* __restrict__ ssi, const double* __restrict__ albedo /* per wavenumber or NULL */,
                const OdT* __restrict__ od, double* __restrict__ partial, double* __restrict__ surf_dn /* [nwav] or NULL */,
                double* __restrict__ toa_up /* [nwav] or NULL */) {
  extern __shared__ double s_acc[];
  const int nhl = nlay + 1;
  const BandChunk c = chunks[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int t = tid; t < 4 * 2 * nhl; t += LBL_THREADS) s_acc[t] = 0.0;
  __syncthreads();
  double* acc_dn = s_acc + wave * 2 * nhl;
  double* acc_up = acc_dn + nhl;
  const long long i = c.i1 + tid;
  const bool live = i <= c.i2;
  const size_t j = live ? (size_t)i : (size_t)c.i2;
  const double minus_sec_sza = -1.0 / cos_sza;
  double flux = live ? cos_sza * ssi[j] : 0.0;                              // radiative_transfer_sw.cpp:39
  wave_add(&acc_dn[0], lane, flux);
  for (int l = 0; l < nlay; ++l) {
    flux = flux * exp(minus_sec_sza * (double)od[(size_t)l * od_stride + j]);
    wave_add(&acc_dn[l + 1], lane, flux);
  }
  if (surf_dn && live) surf_dn[j] = flux;
  if (toa_up && live && !albedo) toa_up[j] = 0.0;
  if (albedo) {                                                             // :70-76
    flux = flux * albedo[j];
    wave_add(&acc_up[nlay], lane, flux);
    for (int l = nlay - 1; l >= 0; --l) {
      flux = flux * exp(-2.0 * (double)od[(size_t)l * od_stride + j]);
      wave_add(&acc_up[l], lane, flux);
    }
    if (toa_up && live) toa_up[j] = flux;
  }
  __syncthreads();
  for (int t = tid; t < 2 * nhl; t += LBL_THREADS)
    partial[(size_t)blockIdx.x * 2 * nhl + t] = add_waves(s_acc, 2 * nhl, t);
}

// Fluxes of (level, g point) matrices - what run_ckd leaves for a flux evaluation (test/run_ckd_lw.sh:133-137: optical depth and
// Planck function per g point) - one thread per (column, g point): radiative_transfer_lw.cpp:27-60 with unit emissivity along the
// slant path sec * tau, nangle = 0 the two-stream form (sec = 1.66), otherwise the sum over the Gauss-Legendre angles with the
// weights 2 w mu (as k_lbl_lw does per wavenumber).
__global__ void __launch_bounds__(256)
k_rt_lw_gpoints(int ncol, int nlay, int ng, int nsec, const double* __restrict__ sec_wgt /*[2][nsec]*/, const double* __restrict__ planck,
                const double* __restrict__ od, double* __restrict__ dn, double* __restrict__ up) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)ncol * ng) return;
  const size_t c = t / ng, g = t % ng;
  const double* pl = planck + c * (size_t)(nlay + 1) * ng + g;
  const double* tau = od + c * (size_t)nlay * ng + g;
  double* fd = dn + c * (size_t)(nlay + 1) * ng + g;
  double* fu = up + c * (size_t)(nlay + 1) * ng + g;
  for (int l = 0; l <= nlay; ++l) { fd[(size_t)l * ng] = 0.0; fu[(size_t)l * ng] = 0.0; }
  for (int a = 0; a < nsec; ++a) {
    const double sec = sec_wgt[a], w = sec_wgt[nsec + a];
    double f = 0.0;
    for (int l = 0; l < nlay; ++l) {
      const double x = tau[(size_t)l * ng];
      const double e = 1.0 - exp(-sec * x);
      const double fac = e > 1.0e-5 ? 1.0 - e * (1.0 / sec) / x : 0.5 * e;
      f = f * (1.0 - e) + pl[(size_t)l * ng] * (e - fac) + pl[(size_t)(l + 1) * ng] * fac;
      fd[(size_t)(l + 1) * ng] += w * f;
    }
    f = pl[(size_t)nlay * ng];
    fu[(size_t)nlay * ng] += w * f;
    for (int l = nlay - 1; l >= 0; --l) {
      const double x = tau[(size_t)l * ng];
      const double e = 1.0 - exp(-sec * x);
      const double fac = e > 1.0e-5 ? 1.0 - e * (1.0 / sec) / x : 0.5 * e;
      f = f * (1.0 - e) + pl[(size_t)(l + 1) * ng] * (e - fac) + pl[(size_t)l * ng] * fac;
      fu[(size_t)l * ng] += w * f;
    }
  }
}

// direct beam and surface-reflected upwelling flux per g point: radiative_transfer_sw.cpp:45-77 (norayleigh)
__global__ void __launch_bounds__(256)
k_rt_sw_gpoints(int ncol, int nlay, int ng, double mu0, double albedo, const double* __restrict__ incoming /*[ncol][ng]*/,
                const double* __restrict__ od, double* __restrict__ dn, double* __restrict__ up) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)ncol * ng) return;
  const size_t c = t / ng, g = t % ng;
  const double* tau = od + c * (size_t)nlay * ng + g;
  double* fd = dn + c * (size_t)(nlay + 1) * ng + g;
  double* fu = up + c * (size_t)(nlay + 1) * ng + g;
  double f = mu0 * incoming[c * ng + g];
  fd[0] = f;
  for (int l = 0; l < nlay; ++l) { f = f * exp(-tau[(size_t)l * ng] / mu0); fd[(size_t)(l + 1) * ng] = f; }
  f = f * albedo;
  fu[(size_t)nlay * ng] = f;
  for (int l = nlay - 1; l >= 0; --l) { f = f * exp(-2.0 * tau[(size_t)l * ng]); fu[(size_t)l * ng] = f; }
}

// k_rt_sw_gpoints with Rayleigh scattering: the two-stream transfer of lbl_rt.hpp per (column, g point).  The three output
// matrices hold the per-level state between the sweeps - D in `direct`, the albedo A below each level in `dn`, the source S in
// `up` - each element written and read by its own thread only, and leave holding the fluxes (dn: direct plus diffuse).
__global__ void __launch_bounds__(256)
k_rt_sw_gpoints_rayleigh(int ncol, int nlay, int ng, double mu0, double minus_sec_sza, double albedo, const double* __restrict__ incoming /*[ncol][ng]*/,
                         const double* __restrict__ od, const double* __restrict__ od_ray, double* direct, double* dn, double* up) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)ncol * ng) return;
  const size_t c = t / ng, g = t % ng;
  const double* tau_abs = od + c * (size_t)nlay * ng + g;
  const double* tau_ray = od_ray + c * (size_t)nlay * ng + g;
  double* fdir = direct + c * (size_t)(nlay + 1) * ng + g;
  double* fd = dn + c * (size_t)(nlay + 1) * ng + g;
  double* fu = up + c * (size_t)(nlay + 1) * ng + g;
  double f = mu0 * incoming[c * ng + g];
  fdir[0] = f;
  for (int l = 0; l < nlay; ++l) {
    f = f * exp(minus_sec_sza * (tau_abs[(size_t)l * ng] + tau_ray[(size_t)l * ng]));
    fdir[(size_t)(l + 1) * ng] = f;
  }
  double a = albedo, src = albedo * f;
  fd[(size_t)nlay * ng] = a;
  fu[(size_t)nlay * ng] = src;
  for (int l = nlay - 1; l >= 0; --l) {
    const RayleighLayer L = rayleigh_layer(tau_abs[(size_t)l * ng], tau_ray[(size_t)l * ng], mu0, minus_sec_sza);
    rayleigh_up(L, fdir[(size_t)l * ng], a, src, a, src);
    fd[(size_t)l * ng] = a;
    fu[(size_t)l * ng] = src;
  }
  double diffuse = 0.0, flux_up = src;
  fd[0] = diffuse + fdir[0];
  for (int l = 0; l < nlay; ++l) {
    const RayleighLayer L = rayleigh_layer(tau_abs[(size_t)l * ng], tau_ray[(size_t)l * ng], mu0, minus_sec_sza);
    rayleigh_down(L, fdir[(size_t)l * ng], fd[(size_t)(l + 1) * ng], fu[(size_t)(l + 1) * ng], diffuse, diffuse, flux_up);
    fd[(size_t)(l + 1) * ng] = diffuse + fdir[(size_t)(l + 1) * ng];
    fu[(size_t)(l + 1) * ng] = flux_up;
  }
}

struct HostArray { const double* in; double* out; size_t n; };   // n doubles that go to the device (in) or come back (out)

// The host arrays of a g-point transfer through the context's scratch, one piece per array in list order: the inputs copied
// in, launch(d) with d[i] the piece of array i, the outputs copied back, the stream synchronised.
template <size_t N, typename Launch>
int through_scratch(ecckd_ctx* ctx, const HostArray (&a)[N], Launch launch) {
  size_t bytes[N];
  void* d[N];
  for (size_t i = 0; i < N; ++i) bytes[i] = a[i].n * sizeof(double);
  ECCKD_CHECK(ecckd::carve_scratch(ctx, bytes, d));
  for (size_t i = 0; i < N; ++i)
    if (a[i].in) ECCKD_HIP_CHECK(hipMemcpyAsync(d[i], a[i].in, bytes[i], hipMemcpyHostToDevice, ctx->stream));
  launch((double* const*)d);
  ECCKD_HIP_CHECK(hipGetLastError());
  for (size_t i = 0; i < N; ++i)
    if (a[i].out) ECCKD_HIP_CHECK(hipMemcpyAsync(a[i].out, d[i], bytes[i], hipMemcpyDeviceToHost, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return ECCKD_OK;
}

}  // namespace

extern "C" {

int ecckd_lbl_band_fluxes_lw(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_temperature_hl,
                             const double* d_wavenumber, const double* d_d_wavenumber, const void* d_od, int od_type,
                             size_t od_stride, int nband, const int64_t* h_band_begin, const int64_t* h_band_end,
                             double* h_flux_dn, double* h_flux_up) {
  return ecckd_lbl_band_fluxes_lw_ex(ctx, nlay, nwav, h_temperature_hl, d_wavenumber, d_d_wavenumber, d_od, od_type, od_stride, nband,
                                     h_band_begin, h_band_end, h_flux_dn, h_flux_up, nullptr, nullptr);
}

int ecckd_lbl_band_fluxes_lw_ex(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_temperature_hl,
                                const double* d_wavenumber, const double* d_d_wavenumber, const void* d_od, int od_type,
                                size_t od_stride, int nband, const int64_t* h_band_begin, const int64_t* h_band_end,
                                double* h_flux_dn, double* h_flux_up, double* d_surf_dn, double* d_toa_up) {
  return ecckd_lbl_band_fluxes_lw_angles(ctx, 0, nlay, nwav, h_temperature_hl, d_wavenumber, d_d_wavenumber, d_od, od_type, od_stride,
                                         nband, h_band_begin, h_band_end, h_flux_dn, h_flux_up, d_surf_dn, d_toa_up);
}

int ecckd_gauss_legendre_01(int n, double* h_mu, double* h_weight) {
  ECCKD_REQUIRE(n >= 1 && n <= LBL_MAX_ANGLES && h_mu && h_weight, "ecckd_gauss_legendre_01: 1 <= n <= %d", LBL_MAX_ANGLES);
  // nodes of P_n on (-1, 1) by Newton's iteration from the Chebyshev guess, mapped to (0, 1); ascending mu
  for (int i = 0; i < n; ++i) {
    double t = std::cos(3.14159265358979323846 * (i + 0.75) / (n + 0.5));
    double dp = 1.0;
    for (int it = 0; it < 100; ++it) {
      double p0 = 1.0, p1 = t;
      for (int k = 2; k <= n; ++k) { const double pk = ((2.0 * k - 1.0) * t * p1 - (k - 1.0) * p0) / k; p0 = p1; p1 = pk; }
      if (n == 1) { p0 = 1.0; p1 = t; }
      dp = n * (t * p1 - p0) / (t * t - 1.0);
      const double dt = p1 / dp;
      t -= dt;
      if (std::fabs(dt) < 1e-16) break;
    }
    {
      double p0 = 1.0, p1 = t;
      for (int k = 2; k <= n; ++k) { const double pk = ((2.0 * k - 1.0) * t * p1 - (k - 1.0) * p0) / k; p0 = p1; p1 = pk; }
      dp = n * (t * p1 - p0) / (t * t - 1.0);
    }
    const double w = 2.0 / ((1.0 - t * t) * dp * dp);
    h_mu[n - 1 - i] = 0.5 * (1.0 + t);
    h_weight[n - 1 - i] = 0.5 * w;
  }
  return ECCKD_OK;
}

int ecckd_lbl_band_fluxes_lw_angles(ecckd_ctx* ctx, int nangle, int nlay, size_t nwav, const double* h_temperature_hl,
                                    const double* d_wavenumber, const double* d_d_wavenumber, const void* d_od, int od_type,
                                    size_t od_stride, int nband, const int64_t* h_band_begin, const int64_t* h_band_end,
                                    double* h_flux_dn, double* h_flux_up, double* d_surf_dn, double* d_toa_up) {
  const char* who = "ecckd_lbl_band_fluxes_lw";
  int nang = 0;
  std::vector<double> sec_wgt;
  ECCKD_CHECK(lw_angle_table(who, nangle, &nang, sec_wgt));
  ECCKD_REQUIRE(ctx && nlay > 0 && h_temperature_hl && d_wavenumber && d_d_wavenumber && d_od && nband > 0 && h_band_begin &&
                h_band_end && h_flux_dn && h_flux_up, "ecckd_lbl_band_fluxes_lw: bad argument");
  ECCKD_CHECK(check_od(who, od_type, od_stride, nwav));
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int nhl = nlay + 1;
  BandRun r;
  ECCKD_CHECK(band_start(r, ctx, nullptr, nwav, nband, h_band_begin, h_band_end, nhl, {{d_surf_dn, 1}, {d_toa_up, 1}},
                         {h_flux_dn, h_flux_up}, 1));
  std::vector<double> hk;
  ECCKD_CHECK(make_hk(who, nhl, h_temperature_hl, hk));
  hk.insert(hk.end(), sec_wgt.begin(), sec_wgt.end());   // one upload: hk[nhl], then the angles
  if (r.chunks.empty()) return ECCKD_OK;
  ECCKD_CHECK(band_device(r, hk.data(), hk.size(), nullptr, 0, r.chunks.size() * 2 * nhl, 0));
  const size_t lds = (size_t)4 * 2 * nhl * sizeof(double);
  with_od_type(od_type, [&](auto t) {
    using OdT = decltype(t);
    hipLaunchKernelGGL(k_lbl_fluxes_lw<OdT>, dim3((unsigned)r.chunks.size()), dim3(LBL_THREADS), lds, ctx->stream, nang,
                       r.d_tab0 + nhl, nlay, od_stride, r.d_chunks, r.d_tab0, d_wavenumber, d_d_wavenumber, (const OdT*)d_od,
                       r.d_part, d_surf_dn, d_toa_up);
  });
  ECCKD_HIP_CHECK(hipGetLastError());
  return band_collect(r, 1, nullptr, {h_flux_dn, h_flux_up});
}

int ecckd_lbl_band_fluxes_sw(ecckd_ctx* ctx, int nlay, size_t nwav, double cos_sza, const double* d_ssi,
                             const double* d_albedo, const void* d_od, int od_type, size_t od_stride, int nband,
                             const int64_t* h_band_begin, const int64_t* h_band_end, double* h_flux_dn_direct,
                             double* h_flux_up) {
  return ecckd_lbl_band_fluxes_sw_ex(ctx, nlay, nwav, cos_sza, d_ssi, d_albedo, d_od, od_type, od_stride, nband, h_band_begin,
                                     h_band_end, h_flux_dn_direct, h_flux_up, nullptr, nullptr);
}

int ecckd_lbl_band_fluxes_sw_ex(ecckd_ctx* ctx, int nlay, size_t nwav, double cos_sza, const double* d_ssi,
                                const double* d_albedo, const void* d_od, int od_type, size_t od_stride, int nband,
                                const int64_t* h_band_begin, const int64_t* h_band_end, double* h_flux_dn_direct,
                                double* h_flux_up, double* d_surf_dn_direct, double* d_toa_up) {
  double* const d_surf_dn = d_surf_dn_direct;
  ECCKD_REQUIRE(ctx && nlay > 0 && d_ssi && d_od && nband > 0 && h_band_begin && h_band_end && h_flux_dn_direct,
                "ecckd_lbl_band_fluxes_sw: bad argument");
  ECCKD_REQUIRE(cos_sza > 0.0, "ecckd_lbl_band_fluxes_sw: cos_sza must be positive");
  ECCKD_CHECK(check_od("ecckd_lbl_band_fluxes_sw", od_type, od_stride, nwav));
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int nhl = nlay + 1;
  BandRun r;
  ECCKD_CHECK(band_start(r, ctx, nullptr, nwav, nband, h_band_begin, h_band_end, nhl, {{d_surf_dn, 1}, {d_toa_up, 1}},
                         {h_flux_dn_direct, h_flux_up}, 1));
  if (r.chunks.empty()) return ECCKD_OK;
  ECCKD_CHECK(band_device(r, nullptr, 0, nullptr, 0, r.chunks.size() * 2 * nhl, 0));
  const size_t lds = (size_t)4 * 2 * nhl * sizeof(double);
  with_od_type(od_type, [&](auto t) {
    using OdT = decltype(t);
    hipLaunchKernelGGL(k_lbl_fluxes_sw<OdT>, dim3((unsigned)r.chunks.size()), dim3(LBL_THREADS), lds, ctx->stream, nlay, od_stride,
                       r.d_chunks, cos_sza, d_ssi, d_albedo, (const OdT*)d_od, r.d_part, d_surf_dn, d_toa_up);
  });
  ECCKD_HIP_CHECK(hipGetLastError());
  return band_collect(r, 1, nullptr, {h_flux_dn_direct, h_flux_up});   // h_flux_up may be NULL
}

// The fluxes of a CKD model's g points from the optical depths and Planck functions run_ckd wrote (the `--ckd` mode of the
// CKDMIP tools as the scripts use them, test/run_ckd_lw.sh:133-137, test/run_ckd_sw.sh:125-128).  Host arrays in and out (a few
// thousand values per column), the radiative transfer on the device.
int ecckd_rt_lw_gpoints(ecckd_ctx* ctx, int nangle, int ncol, int nlay, int ng, const double* h_planck_hl, const double* h_od,
                        double* h_flux_dn, double* h_flux_up) {
  ECCKD_REQUIRE(ctx && ncol > 0 && nlay > 0 && ng > 0 && h_planck_hl && h_od && h_flux_dn && h_flux_up, "ecckd_rt_lw_gpoints: bad argument");
  ECCKD_REQUIRE(nangle >= 0 && nangle <= LBL_MAX_ANGLES, "ecckd_rt_lw_gpoints: nangle %d outside 0..%d", nangle, LBL_MAX_ANGLES);
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  int nsec = 0;
  std::vector<double> sw;
  ECCKD_CHECK(lw_angle_table("ecckd_rt_lw_gpoints", nangle, &nsec, sw));
  const size_t nl = (size_t)ncol * nlay * ng, nh = (size_t)ncol * (nlay + 1) * ng;
  const HostArray a[] = {{sw.data(), nullptr, sw.size()}, {h_od, nullptr, nl}, {h_planck_hl, nullptr, nh}, {nullptr, h_flux_dn, nh},
                         {nullptr, h_flux_up, nh}};
  return through_scratch(ctx, a, [&](double* const* d) {
    hipLaunchKernelGGL(k_rt_lw_gpoints, dim3((unsigned)(((size_t)ncol * ng + 255) / 256)), dim3(256), 0, ctx->stream, ncol, nlay, ng, nsec,
                       d[0], d[2], d[1], d[3], d[4]);
  });
}

int ecckd_rt_sw_gpoints(ecckd_ctx* ctx, int ncol, int nlay, int ng, double cos_sza, double albedo, const double* h_incoming,
                        const double* h_od, double* h_flux_dn, double* h_flux_up) {
  ECCKD_REQUIRE(ctx && ncol > 0 && nlay > 0 && ng > 0 && h_incoming && h_od && h_flux_dn && h_flux_up, "ecckd_rt_sw_gpoints: bad argument");
  ECCKD_REQUIRE(cos_sza > 0.0, "ecckd_rt_sw_gpoints: cos_sza must be positive");
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const size_t nl = (size_t)ncol * nlay * ng, nh = (size_t)ncol * (nlay + 1) * ng, ni = (size_t)ncol * ng;
  const HostArray a[] = {{h_incoming, nullptr, ni}, {h_od, nullptr, nl}, {nullptr, h_flux_dn, nh}, {nullptr, h_flux_up, nh}};
  return through_scratch(ctx, a, [&](double* const* d) {
    hipLaunchKernelGGL(k_rt_sw_gpoints, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, ctx->stream, ncol, nlay, ng, cos_sza, albedo, d[0],
                       d[1], d[2], d[3]);
  });
}

int ecckd_rt_sw_gpoints_rayleigh(ecckd_ctx* ctx, int ncol, int nlay, int ng, double cos_sza, double albedo, const double* h_incoming,
                                 const double* h_od, const double* h_od_rayleigh, double* h_flux_dn_direct, double* h_flux_dn,
                                 double* h_flux_up) {
  const char* who = "ecckd_rt_sw_gpoints_rayleigh";
  ECCKD_REQUIRE(ctx && ncol > 0 && nlay > 0 && ng > 0 && h_incoming && h_od && h_od_rayleigh && h_flux_dn_direct && h_flux_dn && h_flux_up,
                "%s: bad argument", who);
  double h_ang[2 * LBL_MAX_SZA];
  ECCKD_CHECK(sw_angle_table(who, 1, &cos_sza, h_ang));
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const size_t nl = (size_t)ncol * nlay * ng, nh = (size_t)ncol * (nlay + 1) * ng, ni = (size_t)ncol * ng;
  const HostArray a[] = {{h_incoming, nullptr, ni}, {h_od, nullptr, nl}, {h_od_rayleigh, nullptr, nl}, {nullptr, h_flux_dn_direct, nh},
                         {nullptr, h_flux_dn, nh}, {nullptr, h_flux_up, nh}};
  return through_scratch(ctx, a, [&](double* const* d) {
    hipLaunchKernelGGL(k_rt_sw_gpoints_rayleigh, dim3((unsigned)((ni + 255) / 256)), dim3(256), 0, ctx->stream, ncol, nlay, ng, h_ang[0],
                       h_ang[LBL_MAX_SZA], albedo, d[0], d[1], d[2], d[3], d[4], d[5]);
  });
}

}  // extern "C"
