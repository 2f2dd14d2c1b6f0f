// lbl_rt.hpp - the transfer of ONE wavenumber, written once for the line-by-line kernels (lbl_fluxes.hip,
// lbl_gpoint_fluxes.hip, lbl_gpoint_fluxes_sw.hip, lbl_scenarios.hip: no scattering; lbl_fluxes_sw_rayleigh.hip,
// lbl_scenarios_sw_rayleigh.hip, lbl_gpoint_fluxes_sw_rayleigh.hip and k_rt_sw_gpoints_rayleigh of lbl_fluxes.hip: Rayleigh scattering; k_opt_forward_adjoint_rayleigh of optimize.hip takes the same
// Rayleigh functions and their derivative rayleigh_layer_d), and the host plumbing they share.  DESIGN.md and the
// tests compare these kernels with each other, bit for bit where they can: one source text keeps an edit from reaching only
// one of them.  The files are compiled with the default contraction, so an expression here and in rt_device.hpp keeps its form
// and operand order; a reordered one can fuse differently and change bits.
//
// Longwave: planck_function (planck_function.cpp:22-54) and radiative_transfer_lw (radiative_transfer_lw.cpp:27-60) with
// unit surface emissivity along the slant path sec * tau:
//   freq = wn_to_freq(wn);  pref = planck_pref(d_wn, freq);  B(level) = planck(pref, freq, hk[level]), hk = (h / k) / T
//   per layer   lw_layer(sec, 1 / sec, tau, eps, fac)                                          (:41-43)
//   down, up    flux = lw_step(flux, eps, fac, B(level left), B(level reached))                (:45-50, :55-59)
//   surface     flux = lw_surface(flux, B(surface))                                            (:52-53)
// Shortwave: radiative_transfer_direct_sw / _norayleigh_sw (radiative_transfer_sw.cpp:26-77).  Its steps are single
// products and stay written out where they are used, always in this form, with the IEEE exp and not exp_fast:
//   top         flux = cos_sza * ssi                                                           (:39)
//   down        flux = flux * exp(minus_sec_sza * tau),  minus_sec_sza = -1.0 / cos_sza        (:45-50)
//   surface     flux = flux * albedo                                                           (:70)
//   up          flux = flux * exp(-2.0 * tau)                                                  (:72-76)
// Shortwave with Rayleigh scattering (not in the reference: the external CKDMIP tool scatters by rayleigh_optical_depth, its
// arithmetic is unpinned): the two-stream equations at asymmetry 0 with ecRad's shortwave coefficients
// (Zdunkowski PIFM: g1 = 2 - 1.25 w, g2 = 0.75 w, g3 = g4 = 0.5), Meador & Weaver's (1980) closed form per layer and the
// adding method over the column; tests/rayleigh_ref.py restates it.  The direct beam is the chain above on tau_abs + tau_ray.
//   per layer   rayleigh_layer(tau_abs, tau_ray, mu0, minus_sec_sza) -> R, T, Tdir, Rdir, Tdd per unit direct flux at its top
//   surface     A = albedo, S = albedo * D(surface)
//   up          rayleigh_up(layer, D(top), A below, S below) -> A, S at the layer's top
//   top         up = S, diffuse down = 0
//   down        rayleigh_down(layer, D(top), A below, S below, diffuse down at the top) -> diffuse down, up at its base
// The constants, reductions, Planck function and longwave steps live in rt_device.hpp, which the tuned kernels of find_g.hip,
// optimize.hip, create_lut.hip and reorder.hip include too; of their own they keep only the SGPR-pinned and pairwise
// interleaved variants (k_rt_lw_bb, eps_fac_pair), whose arithmetic differs.
#pragma once

#include "rt_device.hpp"

#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <vector>

namespace ecckd {
namespace lbl {

constexpr int LBL_THREADS = 256;     // threads of a block = wavenumbers of a BandChunk
constexpr int LBL_MAX_ANGLES = 16;   // longwave zenith angles per hemisphere
constexpr int LBL_MAX_SZA = 8;       // solar zenith angles of one call

// ---------------------------------------------------------------------------------------------------------------- device
// constants, wave reductions, Planck function and longwave layer step: rt_device.hpp, shared with the tuned kernels
using ecckd::kPlanckH; using ecckd::kLightC; using ecckd::kPi;
using ecckd::wave_sum; using ecckd::wave_add; using ecckd::add_waves;
using ecckd::wn_to_freq; using ecckd::planck_pref; using ecckd::planck;
using ecckd::lw_layer; using ecckd::lw_step; using ecckd::lw_surface;

// The layer terms of the Rayleigh two-stream transfer per unit direct flux D at the layer's top: diffuse reflectance R and
// transmittance T, direct transmittance Tdir, and the parts of the direct beam that leave the layer upwards (Rdir) and
// downwards (Tdd) as diffuse light.
struct RayleighLayer { double R, T, Tdir, Rdir, Tdd; };

constexpr double RAYLEIGH_RESONANCE_H = 1.0e-4;

// Rdir and Tdd of the closed form before their clamps, with mu0 and tdir = exp(-tau / mu0) in every place they occur
__device__ __forceinline__ void rayleigh_direct(double w, double k, double e, double e2, double f, double a1, double a2, double mu0,
                                                double tdir, double& rdir, double& tdd) {
  const double g3 = 0.5, g4 = 0.5;
  const double km = k * mu0;
  const double f2 = w * f / (1.0 - km * km);
  rdir = f2 * ((1.0 - km) * (a2 + k * g3) - (1.0 + km) * (a2 - k * g3) * e2 - 2.0 * k * e * (g3 - a2 * mu0) * tdir);
  tdd = f2 * (2.0 * k * e * (g4 + a1 * mu0) - tdir * ((1.0 + km) * (a1 + k * g4) - (1.0 - km) * (a1 - k * g4) * e2));
}

// The closed form divides by 1 - (k mu0)^2, and k -> 2 as w -> 0: the resonance k mu0 = 1 sits on mu0 = 0.5 for every weakly
// scattering layer.  Within |1 - k mu0| < h the direct terms are therefore evaluated at mu0 = (1 -+ 2h) / k, each with its own
// Tdir, and interpolated linearly to mu0 (R, T and Tdir do not depend on the shift); w = 0 is a branch of its own, the
// no-scattering path with the diffuse transmittance exp(-2 tau).
__device__ __forceinline__ RayleighLayer rayleigh_layer(double tau_abs, double tau_ray, double mu0, double minus_sec_sza) {
  RayleighLayer L;
  const double tau = tau_abs + tau_ray;
  L.Tdir = exp(minus_sec_sza * tau);
  if (!(tau_ray > 0.0 && tau > 0.0)) {
    L.R = 0.0; L.T = exp(-2.0 * tau); L.Rdir = 0.0; L.Tdd = 0.0;
    return L;
  }
  const double g3 = 0.5, g4 = 0.5;
  const double w = tau_ray / tau;
  const double g1 = 2.0 - 1.25 * w, g2 = 0.75 * w;
  const double a1 = g1 * g4 + g2 * g3;
  const double a2 = g1 * g3 + g2 * g4;
  const double k = sqrt(fmax((g1 - g2) * (g1 + g2), 1e-12));
  const double e = exp(-k * tau);
  const double e2 = e * e;
  const double f = 1.0 / (k + g1 + (k - g1) * e2);
  L.R = g2 * (1.0 - e2) * f;
  L.T = 2.0 * k * e * f;
  double rdir, tdd;
  if (fabs(1.0 - k * mu0) < RAYLEIGH_RESONANCE_H) {
    const double mu_a = (1.0 - 2.0 * RAYLEIGH_RESONANCE_H) / k, mu_b = (1.0 + 2.0 * RAYLEIGH_RESONANCE_H) / k;
    double ra, ta, rb, tb;
    rayleigh_direct(w, k, e, e2, f, a1, a2, mu_a, exp((-1.0 / mu_a) * tau), ra, ta);
    rayleigh_direct(w, k, e, e2, f, a1, a2, mu_b, exp((-1.0 / mu_b) * tau), rb, tb);
    const double x = (mu0 - mu_a) / (mu_b - mu_a);
    rdir = ra + (rb - ra) * x;
    tdd = ta + (tb - ta) * x;
  } else {
    rayleigh_direct(w, k, e, e2, f, a1, a2, mu0, L.Tdir, rdir, tdd);
  }
  L.Rdir = fmin(fmax(rdir, 0.0), 1.0 - L.Tdir);
  L.Tdd = fmin(fmax(tdd, 0.0), 1.0 - L.Tdir - L.Rdir);
  return L;
}

// The layer of the resident fluxes under a cloud (gas_optics_fluxes.hip; tests/allsky_ref.py restates it): a particulate of
// optical depth t, single-scattering albedo ws and asymmetry a (delta-scaled by the caller where that is wanted) mixed into the
// gas, tau = tau_abs + tau_ray + t, sc = tau_ray + ws t, w = sc / tau, gg = ws t a / sc, under ecRad's shortwave coefficients
//   fac = 0.75 gg, g1 = 2 - w (1.25 + fac), g2 = w (0.75 - fac), g3 = 0.5 - mu0 fac, g4 = 1 - g3
// and otherwise rayleigh_layer's closed form, branches and clamps.  g3 and g4 depend on mu0, so cloud_direct forms them, a1 and
// a2 from the angle it is given: in the resonance treatment every place mu0 occurs takes the shifted angle.
__device__ __forceinline__ void cloud_direct(double w, double k, double e, double e2, double f, double g1, double g2, double fac, double mu0,
                                             double tdir, double& rdir, double& tdd) {
  const double g3 = 0.5 - mu0 * fac, g4 = 1.0 - g3;
  const double a1 = g1 * g4 + g2 * g3;
  const double a2 = g1 * g3 + g2 * g4;
  const double km = k * mu0;
  const double f2 = w * f / (1.0 - km * km);
  rdir = f2 * ((1.0 - km) * (a2 + k * g3) - (1.0 + km) * (a2 - k * g3) * e2 - 2.0 * k * e * (g3 - a2 * mu0) * tdir);
  tdd = f2 * (2.0 * k * e * (g4 + a1 * mu0) - tdir * ((1.0 + km) * (a1 + k * g4) - (1.0 - km) * (a1 - k * g4) * e2));
}

__device__ __forceinline__ RayleighLayer cloud_layer(double tau_abs, double tau_ray, double t, double ws, double a, double mu0,
                                                     double minus_sec_sza) {
  RayleighLayer L;
  const double tau = tau_abs + tau_ray + t;
  L.Tdir = exp(minus_sec_sza * tau);
  const double sc_cloud = ws * t;
  const double sc = tau_ray + sc_cloud;
  if (!(sc > 0.0 && tau > 0.0)) {
    L.R = 0.0; L.T = exp(-2.0 * tau); L.Rdir = 0.0; L.Tdd = 0.0;
    return L;
  }
  const double w = sc / tau;
  const double gg = sc_cloud * a / sc;
  const double fac = 0.75 * gg;
  const double g1 = 2.0 - w * (1.25 + fac), g2 = w * (0.75 - fac);
  const double k = sqrt(fmax((g1 - g2) * (g1 + g2), 1e-12));
  const double e = exp(-k * tau);
  const double e2 = e * e;
  const double f = 1.0 / (k + g1 + (k - g1) * e2);
  L.R = g2 * (1.0 - e2) * f;
  L.T = 2.0 * k * e * f;
  double rdir, tdd;
  if (fabs(1.0 - k * mu0) < RAYLEIGH_RESONANCE_H) {
    const double mu_a = (1.0 - 2.0 * RAYLEIGH_RESONANCE_H) / k, mu_b = (1.0 + 2.0 * RAYLEIGH_RESONANCE_H) / k;
    double ra, ta, rb, tb;
    cloud_direct(w, k, e, e2, f, g1, g2, fac, mu_a, exp((-1.0 / mu_a) * tau), ra, ta);
    cloud_direct(w, k, e, e2, f, g1, g2, fac, mu_b, exp((-1.0 / mu_b) * tau), rb, tb);
    const double x = (mu0 - mu_a) / (mu_b - mu_a);
    rdir = ra + (rb - ra) * x;
    tdd = ta + (tb - ta) * x;
  } else {
    cloud_direct(w, k, e, e2, f, g1, g2, fac, mu0, L.Tdir, rdir, tdd);
  }
  L.Rdir = fmin(fmax(rdir, 0.0), 1.0 - L.Tdir);
  L.Tdd = fmin(fmax(tdd, 0.0), 1.0 - L.Tdir - L.Rdir);
  return L;
}

// d / d tau_abs of rayleigh_direct at fixed tau_ray, forward mode: every d* argument is the derivative of the argument before
// it.  mu may itself depend on tau_abs (the shifted angles of the resonance treatment, dmu != 0).
__device__ __forceinline__ void rayleigh_direct_d(double w, double dw, double k, double dk, double e, double de, double e2, double de2,
                                                  double f, double df, double a1, double da1, double a2, double da2, double mu,
                                                  double dmu, double tdir, double dtdir, double& rdir, double& drdir, double& tdd,
                                                  double& dtdd) {
  const double g3 = 0.5, g4 = 0.5;
  const double km = k * mu, dkm = dk * mu + k * dmu;
  const double om = 1.0 / (1.0 - km * km);
  const double f2 = w * f * om;
  const double df2 = (dw * f + w * df) * om + f2 * (2.0 * km * dkm) * om;
  const double ke = k * e, dke = dk * e + k * de;
  const double p1 = a2 + k * g3, dp1 = da2 + dk * g3;
  const double p2 = a2 - k * g3, dp2 = da2 - dk * g3;
  const double p3 = g3 - a2 * mu, dp3 = -(da2 * mu + a2 * dmu);
  const double brd = (1.0 - km) * p1 - (1.0 + km) * p2 * e2 - 2.0 * ke * p3 * tdir;
  const double dbrd = -dkm * p1 + (1.0 - km) * dp1 - dkm * p2 * e2 - (1.0 + km) * (dp2 * e2 + p2 * de2) -
                      2.0 * (dke * p3 * tdir + ke * dp3 * tdir + ke * p3 * dtdir);
  const double q1 = a1 + k * g4, dq1 = da1 + dk * g4;
  const double q2 = a1 - k * g4, dq2 = da1 - dk * g4;
  const double q3 = g4 + a1 * mu, dq3 = da1 * mu + a1 * dmu;
  const double c = (1.0 + km) * q1 - (1.0 - km) * q2 * e2;
  const double dc = dkm * q1 + (1.0 + km) * dq1 + dkm * q2 * e2 - (1.0 - km) * (dq2 * e2 + q2 * de2);
  const double btd = 2.0 * ke * q3 - tdir * c;
  const double dbtd = 2.0 * (dke * q3 + ke * dq3) - dtdir * c - tdir * dc;
  rdir = f2 * brd; drdir = df2 * brd + f2 * dbrd;
  tdd = f2 * btd; dtdd = df2 * btd + f2 * dbtd;
}

// d / d tau_abs of the five terms of rayleigh_layer at fixed tau_ray, branch by branch as rayleigh_layer takes them (the
// optimiser's adjoint, optimize.hip): the w = 0 branch, the clamp of k (dk = 0 where it is active), the resonance interpolation
// (mu_a, mu_b and x move with k) and the two clamps of Rdir / Tdd - zero below 0, and the derivative of the bound 1 - Tdir
// (- Rdir) where that is the active one.  The values themselves are rayleigh_layer's: the caller takes them from there.
// WRT_RAY: d / d tau_ray at fixed tau_abs instead (the optimised Rayleigh coefficients, ECCKD_OPT_RAYLEIGH_ACTIVE).  With
// tau = tau_abs + tau_ray and w = tau_ray / tau both partial derivatives move tau with seed 1, so they differ in ONE seed only,
// dw = (1 - w) / tau in place of -w / tau; every other line is common.  The no-scattering branch tau_ray <= 0 belongs to a
// pinned element, whose gradient is 0 by definition: all five terms are 0 there.
template <bool WRT_RAY>
__device__ __forceinline__ RayleighLayer rayleigh_layer_dx(double tau_abs, double tau_ray, double mu0, double minus_sec_sza) {
  RayleighLayer d;
  const double tau = tau_abs + tau_ray;
  const double Tdir = exp(minus_sec_sza * tau);
  d.Tdir = minus_sec_sza * Tdir;
  if (!(tau_ray > 0.0 && tau > 0.0)) {
    if constexpr (WRT_RAY) { d.R = 0.0; d.T = 0.0; d.Tdir = 0.0; d.Rdir = 0.0; d.Tdd = 0.0; }
    else { d.R = 0.0; d.T = -2.0 * exp(-2.0 * tau); d.Rdir = 0.0; d.Tdd = 0.0; }
    return d;
  }
  const double g3 = 0.5, g4 = 0.5;
  const double w = tau_ray / tau, dw = WRT_RAY ? (1.0 - w) / tau : -w / tau;
  const double g1 = 2.0 - 1.25 * w, g2 = 0.75 * w, dg1 = -1.25 * dw, dg2 = 0.75 * dw;
  const double a1 = g1 * g4 + g2 * g3, da1 = dg1 * g4 + dg2 * g3;
  const double a2 = g1 * g3 + g2 * g4, da2 = dg1 * g3 + dg2 * g4;
  const double q = (g1 - g2) * (g1 + g2);
  const double k = sqrt(fmax(q, 1e-12));
  const double dk = q > 1e-12 ? ((dg1 - dg2) * (g1 + g2) + (g1 - g2) * (dg1 + dg2)) / (2.0 * k) : 0.0;
  const double e = exp(-k * tau), de = -e * (dk * tau + k);
  const double e2 = e * e, de2 = 2.0 * e * de;
  const double f = 1.0 / (k + g1 + (k - g1) * e2);
  const double df = -f * f * (dk + dg1 + (dk - dg1) * e2 + (k - g1) * de2);
  d.R = dg2 * (1.0 - e2) * f - g2 * de2 * f + g2 * (1.0 - e2) * df;
  d.T = 2.0 * (dk * e * f + k * de * f + k * e * df);
  double rdir, drdir, tdd, dtdd;
  if (fabs(1.0 - k * mu0) < RAYLEIGH_RESONANCE_H) {
    const double mu_a = (1.0 - 2.0 * RAYLEIGH_RESONANCE_H) / k, mu_b = (1.0 + 2.0 * RAYLEIGH_RESONANCE_H) / k;
    const double dmu_a = -mu_a * dk / k, dmu_b = -mu_b * dk / k;
    const double t_a = exp((-1.0 / mu_a) * tau), t_b = exp((-1.0 / mu_b) * tau);
    const double dt_a = t_a * (-1.0 / mu_a + tau * dmu_a / (mu_a * mu_a)), dt_b = t_b * (-1.0 / mu_b + tau * dmu_b / (mu_b * mu_b));
    double ra, dra, ta, dta, rb, drb, tb, dtb;
    rayleigh_direct_d(w, dw, k, dk, e, de, e2, de2, f, df, a1, da1, a2, da2, mu_a, dmu_a, t_a, dt_a, ra, dra, ta, dta);
    rayleigh_direct_d(w, dw, k, dk, e, de, e2, de2, f, df, a1, da1, a2, da2, mu_b, dmu_b, t_b, dt_b, rb, drb, tb, dtb);
    const double x = (mu0 - mu_a) / (mu_b - mu_a);
    const double dx = dk * mu0 / (4.0 * RAYLEIGH_RESONANCE_H);      // x = (k mu0 - (1 - 2h)) / (4h)
    rdir = ra + (rb - ra) * x; drdir = dra + (drb - dra) * x + (rb - ra) * dx;
    tdd = ta + (tb - ta) * x; dtdd = dta + (dtb - dta) * x + (tb - ta) * dx;
  } else {
    rayleigh_direct_d(w, dw, k, dk, e, de, e2, de2, f, df, a1, da1, a2, da2, mu0, 0.0, Tdir, d.Tdir, rdir, drdir, tdd, dtdd);
  }
  const double Rdir = fmin(fmax(rdir, 0.0), 1.0 - Tdir);
  d.Rdir = rdir < 0.0 ? 0.0 : (rdir > 1.0 - Tdir ? -d.Tdir : drdir);
  d.Tdd = tdd < 0.0 ? 0.0 : (tdd > 1.0 - Tdir - Rdir ? -d.Tdir - d.Rdir : dtdd);
  return d;
}

__device__ __forceinline__ RayleighLayer rayleigh_layer_d(double tau_abs, double tau_ray, double mu0, double minus_sec_sza) {
  return rayleigh_layer_dx<false>(tau_abs, tau_ray, mu0, minus_sec_sza);
}

__device__ __forceinline__ RayleighLayer rayleigh_layer_dray(double tau_abs, double tau_ray, double mu0, double minus_sec_sza) {
  return rayleigh_layer_dx<true>(tau_abs, tau_ray, mu0, minus_sec_sza);
}

// adding, upwards: the albedo A and the source S (the upwelling flux the direct beam alone causes) seen from the layer's top
__device__ __forceinline__ void rayleigh_up(const RayleighLayer& L, double d_top, double a_below, double s_below, double& a, double& s) {
  const double inv = 1.0 / (1.0 - a_below * L.R);
  a = L.R + L.T * L.T * a_below * inv;
  s = L.Rdir * d_top + L.T * (s_below + a_below * L.Tdd * d_top) * inv;
}

// adding, downwards: the diffuse downwelling and the upwelling flux at the layer's base from the diffuse one at its top
__device__ __forceinline__ void rayleigh_down(const RayleighLayer& L, double d_top, double a_below, double s_below, double dn_top,
                                              double& dn, double& up) {
  const double inv = 1.0 / (1.0 - a_below * L.R);
  dn = (L.T * dn_top + L.R * s_below + L.Tdd * d_top) * inv;
  up = a_below * dn + s_below;
}

// ------------------------------------------------------------------------------------------------------------------ host
using ecckd::kPlanckOverBoltzmann; using ecckd::make_hk;   // rt_device.hpp

struct BandChunk { long long i1, i2; int band; int pad; };

// one chunk per LBL_THREADS wavenumbers of a band, in wavenumber order; `who` (or NULL) prefixes the message
inline int make_chunks(const char* who, size_t nwav, int nband, const int64_t* b0, const int64_t* b1, std::vector<BandChunk>& chunks) {
  for (int b = 0; b < nband; ++b) {
    if (b1[b] < b0[b]) continue;                       // empty band
    ECCKD_REQUIRE(b0[b] >= 0 && (size_t)b1[b] < nwav, "%s%sband %d range [%lld,%lld] outside the spectrum", who ? who : "",
                  who ? ": " : "", b, (long long)b0[b], (long long)b1[b]);
    for (long long i = b0[b]; i <= b1[b]; i += LBL_THREADS)
      chunks.push_back(BandChunk{i, std::min<long long>(i + LBL_THREADS - 1, b1[b]), b, 0});
  }
  return ECCKD_OK;
}

// The host path of the band-flux entries (lbl_fluxes.hip, lbl_scenarios.hip, lbl_fluxes_sw_rayleigh.hip,
// lbl_scenarios_sw_rayleigh.hip): an entry checks its own arguments, then  band_start - band_device - per launch { its kernel,
// band_collect }.  Which launches there are, and the kernel, stay with the entry; the workspace is the context's scratch, kept
// for the next call.
struct BandRun {
  ecckd_ctx* ctx = nullptr;
  int nband = 0;
  size_t nhl = 0;
  std::vector<BandChunk> chunks;
  std::vector<double> part;                // a launch's partials on the host
  const BandChunk* d_chunks = nullptr;     // band_device: the chunk table, the entry's two small tables, the partials of
  const double* d_tab0 = nullptr;          // one launch and the workspace of its kernel
  const double* d_tab1 = nullptr;
  double* d_part = nullptr;
  void* d_work = nullptr;
};
struct DevRows { double* p; size_t rows; };   // a per-wavenumber device output [rows][nwav], or p = NULL

// The band ranges checked and cut into chunks; the device outputs zeroed (wavenumbers outside every band carry no flux) and the
// host outputs h_out, [h_rows][nband][nhl] each or NULL.  With every band empty that is the result: the stream is
// synchronised and r.chunks stays empty.
inline int band_start(BandRun& r, ecckd_ctx* ctx, const char* who, size_t nwav, int nband, const int64_t* b0, const int64_t* b1, size_t nhl,
                      std::initializer_list<DevRows> d_out, std::initializer_list<double*> h_out, size_t h_rows) {
  r.ctx = ctx; r.nband = nband; r.nhl = nhl;
  ECCKD_CHECK(make_chunks(who, nwav, nband, b0, b1, r.chunks));
  for (const DevRows& d : d_out)
    if (d.p) ECCKD_HIP_CHECK(hipMemsetAsync(d.p, 0, d.rows * nwav * sizeof(double), ctx->stream));
  for (double* h : h_out)
    if (h) std::fill(h, h + h_rows * nband * nhl, 0.0);
  if (r.chunks.empty()) ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return ECCKD_OK;
}

// The chunk table and the entry's small host tables (n0, n1 doubles; 0: none) on the device, with room for npart doubles of
// partials and work_bytes of workspace: one carve of the scratch
inline int band_device(BandRun& r, const double* h_tab0, size_t n0, const double* h_tab1, size_t n1, size_t npart, size_t work_bytes) {
  void* d[5];
  ECCKD_CHECK(ecckd::carve_scratch(r.ctx, {r.chunks.size() * sizeof(BandChunk), n0 * sizeof(double), n1 * sizeof(double),
                                           npart * sizeof(double), work_bytes}, d));
  r.d_chunks = (const BandChunk*)d[0]; r.d_tab0 = (const double*)d[1]; r.d_tab1 = (const double*)d[2];
  r.d_part = (double*)d[3]; r.d_work = d[4];
  ECCKD_CHECK(ecckd_h2d(r.ctx, d[0], r.chunks.data(), r.chunks.size() * sizeof(BandChunk)));
  ECCKD_CHECK(ecckd_h2d(r.ctx, d[1], h_tab0, n0 * sizeof(double)));
  return ecckd_h2d(r.ctx, d[2], h_tab1, n1 * sizeof(double));
}

// After a launch: its partials d_part[chunk][nslot][nflux][nhl] read back and added to the nflux host arrays h_flux (NULL: that
// flux is not wanted) at (slot_row[slot] * nband + band) * nhl; slot_row = NULL: slot k is row k.  The chunks are the outer
// loop, in order - wavenumber order within each band - so every output element is summed in one fixed order, bit for bit
// whatever the launch split.
inline int band_collect(BandRun& r, int nslot, const size_t* slot_row, std::initializer_list<double*> h_flux) {
  const size_t nflux = h_flux.size(), nhl = r.nhl;
  r.part.resize(r.chunks.size() * nslot * nflux * nhl);
  ECCKD_CHECK(ecckd_d2h(r.ctx, r.part.data(), r.d_part, r.part.size() * sizeof(double)));
  for (size_t c = 0; c < r.chunks.size(); ++c)
    for (int k = 0; k < nslot; ++k) {
      const double* p = &r.part[(c * nslot + k) * nflux * nhl];
      const size_t o = ((slot_row ? slot_row[k] : (size_t)k) * r.nband + r.chunks[c].band) * nhl;
      for (double* h : h_flux) {
        if (h) for (size_t i = 0; i < nhl; ++i) h[o + i] += p[i];
        p += nhl;
      }
    }
  return ECCKD_OK;
}

// The zenith angles of the longwave fluxes: sec_wgt = [nang] secants, then [nang] weights.  nangle = 0: one angle with
// sec = 1.66, weight = 1, the classic two-stream form the reference itself uses (radiative_transfer_lw.cpp:27-60,
// LW_DIFFUSIVITY).  nangle > 0: Gauss-Legendre quadrature in mu = cos(zenith angle) over one hemisphere, flux = sum_k 2 w_k
// mu_k L(mu_k), each L(mu_k) the same no-scattering recurrence with the slant path tau / mu_k in place of 1.66 tau (CKDMIP's
// `nangle`, Hogan & Matricardi 2020, GMD 13, 6501-6521, section 3.2: "N angles per hemisphere").  The CKDMIP tool is not
// among the reference's sources: its node set is unpinned, see DESIGN.md.
inline int lw_angle_table(const char* who, int nangle, int* nang, std::vector<double>& sec_wgt) {
  ECCKD_REQUIRE(nangle >= 0 && nangle <= LBL_MAX_ANGLES, "%s: nangle = %d outside 0..%d", who, nangle, LBL_MAX_ANGLES);
  *nang = nangle == 0 ? 1 : nangle;
  sec_wgt.assign(2 * (size_t)*nang, 0.0);
  if (nangle == 0) { sec_wgt[0] = ECCKD_LW_DIFFUSIVITY; sec_wgt[1] = 1.0; }
  else {
    double mu[LBL_MAX_ANGLES], w[LBL_MAX_ANGLES];
    ECCKD_CHECK(ecckd_gauss_legendre_01(nangle, mu, w));
    for (int a = 0; a < nangle; ++a) { sec_wgt[a] = 1.0 / mu[a]; sec_wgt[nangle + a] = 2.0 * w[a] * mu[a]; }
  }
  return ECCKD_OK;
}

// The solar zenith angles of a shortwave call, checked: h_ang = [LBL_MAX_SZA] cos_sza (1.0 beyond nsza), then
// [LBL_MAX_SZA] -1.0 / cos_sza, divided on the host (IEEE, as on the device).
inline int sw_angle_table(const char* who, int nsza, const double* h_cos_sza, double (&h_ang)[2 * LBL_MAX_SZA]) {
  ECCKD_REQUIRE(nsza >= 1 && nsza <= LBL_MAX_SZA, "%s: nsza (%d) must be between 1 and %d", who, nsza, LBL_MAX_SZA);
  for (int s = 0; s < nsza; ++s)
    ECCKD_REQUIRE(h_cos_sza[s] > 0.0 && h_cos_sza[s] <= 1.0, "%s: cos_sza[%d] = %g is not in (0, 1]", who, s, h_cos_sza[s]);
  for (int s = 0; s < LBL_MAX_SZA; ++s) {
    h_ang[s] = s < nsza ? h_cos_sza[s] : 1.0;
    h_ang[LBL_MAX_SZA + s] = -1.0 / h_ang[s];
  }
  return ECCKD_OK;
}

// The line-by-line Rayleigh kernels (lbl_fluxes_sw_rayleigh.hip, lbl_gpoint_fluxes_sw_rayleigh.hip) keep what one sweep leaves
// the next per level in a device workspace [block][slot][level][thread], so their grid is bounded and its blocks loop over
// the work: every unit (a chunk, a logical block of tiles) its own block up to blocks_per_cu per compute unit, or
// ECCKD_RAYLEIGH_GRID (>= 1) blocks in place of that bound.
constexpr int RAYLEIGH_BLOCKS_PER_CU = 3;     // the waves per SIMD the registers of k_lbl_fluxes_sw_rayleigh allow
constexpr int RAYLEIGH_SLOTS = 3;             // D, A, S per level
constexpr int RAYLEIGH_FLUXES = 3;            // direct, total down, up per level

inline size_t rayleigh_grid(const ecckd_ctx* ctx, size_t nwork, int blocks_per_cu = RAYLEIGH_BLOCKS_PER_CU) {
  size_t cap = (size_t)std::max(ctx->num_cu, 1) * blocks_per_cu;
  if (const char* e = std::getenv("ECCKD_RAYLEIGH_GRID")) {
    const long v = std::atol(e);
    if (v >= 1) cap = (size_t)v;
  }
  return std::min(nwork, cap);
}

inline int check_od(const char* who, int od_type, size_t od_stride, size_t nwav) {
  ECCKD_REQUIRE(od_type == ECCKD_F32 || od_type == ECCKD_F64, "%s: od_type must be 4 or 8", who);
  ECCKD_REQUIRE(od_stride >= nwav, "%s: od_stride (%zu) < nwav (%zu)", who, od_stride, nwav);
  return ECCKD_OK;
}

// f(OdT()) with OdT = float or double, as a checked od_type says
template <typename F>
auto with_od_type(int od_type, F&& f) {
  if (od_type == ECCKD_F32) return f(float());
  return f(double());
}

}  // namespace lbl
}  // namespace ecckd
