// optimize.hip - K8/K9: cost function and gradient of optimize_lut on gfx950, and the
// L-BFGS driver that replaces solve_adept.
//
// Replaces reference src/ecckd/solve_adept.cpp:
//   CkdOptimizable::calc_cost_function_gradient (:240-292)  -> ecckd_opt_cost_grad
//   calc_cost_function_and_gradient (:72-211)               -> K8a forward + hand-written adjoint
//   calc_total_optical_depth / CkdModel::calc_optical_depth
//       (:24-69, ckd_model.cpp:925-1102)                    -> sparse LUT interpolation, host-built
//   calc_cost_function_ckd_lw (calc_cost_function_lw.cpp:116-232)
//   CkdModel::calc_background_cost_function (ckd_model.cpp:840-877) -> K9 Kronecker stencil
//   solve_adept (:310-417, adept::Minimizer L-BFGS)         -> ecckd_opt_minimize
//
// Design.  The reference records ~1e6 (profile, layer, g) cells on an Adept tape and
// reverses it, serially, every iteration.  Here:
//  * The LUT interpolation weights depend only on (profile, layer, gas), not on g or on the
//    state, so they are computed ONCE on the host into a fixed-width sparse table
//    (cell -> up to 8 nodes per gas, coefficient = weight * interpolation weight).  The
//    optical depth of a cell is then a gather of contiguous ng-long rows of the state
//    (g is the fastest index of the LUT, ckd_model.cpp:153,216) - fully coalesced.
//  * K8a: one block per profile, one thread per g point: gather, negative-OD penalty, LW
//    two-stream forward sweep (fluxes kept in LDS), band sums, cost terms, then the
//    HAND-DERIVED adjoint of the two sweeps -> dJ/d(optical depth) per cell.
//  * K8b: the transpose of the gather as a second, host-built sparse table (node -> cells),
//    so the gradient is accumulated in a fixed order with NO atomics (bitwise reproducible),
//    fused with the chain rule x = ln k (:276-283).
//  * K9: the prior.  The reference forms B = rho_t^|dt| * rho_p^|dp| (* rho_c^|dc|), inverts it
//    densely with LAPACK and multiplies (ckd_model.cpp:706-713, :857).  B is a Kronecker
//    product of AR(1) matrices, so B^-1 is the Kronecker product of tridiagonals: a 9- or
//    27-point stencil per element.  Entries below 1e-6 are dropped as the reference does.
// The dominant costs are launch latency and ~50 MB of traffic per iteration;
// the metric is iterations per second.
#include "common.hpp"
#include <chrono>
#include "rt_device.hpp"
#include "lbl_rt.hpp"      // rayleigh_layer, rayleigh_layer_d, rayleigh_up, rayleigh_down: k_opt_forward_adjoint_rayleigh
#include "opt_lds.hpp"     // the LDS layouts of the three K8a kernels, shared with the host plan

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

namespace lds = ecckd::opt_lds;

constexpr double kD = ECCKD_LW_DIFFUSIVITY;
constexpr double MIN_X = -1.0e20;  // solve_adept.cpp:21

__device__ __forceinline__ double block_reduce_sum(double v, double* s_red) {
  // fixed-order reduction over a block of up to 1024 threads; result valid in every thread
  // wave_sum (rt_device.hpp) written out, here and in k_opt_gradient_finish and k_opt_sum_cost: with the call the compiler
  // orders the instructions of these kernels differently, and their code stays what was measured
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nwave = (blockDim.x + 63) >> 6;
  __syncthreads();
  if (lane == 0) s_red[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < nwave; ++w) t += s_red[w];
  return t;
}

// ---- what the three K8a kernels share --------------------------------------------------------------------------------
// Their common arguments, filled by k8a_args from the handle and the plan and passed by value.  Members are read by name only
// (no pointer to the struct, no index into it), so they stay in scalar registers.
struct K8aArgs {
  int nlay, ng, ngpad, nband, nent;
  int ray_ent;                 // entry of the Rayleigh term, kept apart from the absorbers (run_ckd mode: added AFTER the clamp), else -1
  int keep_negative;           // scale_lut mode: the optical depth is reported without the clamp at zero; 2: the sweeps see it too
  const double* mu0;           // [ncol], shortwave
  const double* rel_flux;      // [ncol][2][nhl][ng] CKD fluxes of the relative-to scene, or NULL (solve_adept.cpp:118-125)
  const double* k;             // [nk] coefficients of every gas
  const int* ent_idx;          // [ncell][nent] start of an ng-long row of k, or -1
  const double* ent_coef;      // [ncell][nent]
  const int* band_of_g;        // [ng]
  const double* planck_hl;     // [ncol][nhl][ng]; shortwave: row 0 of a column is the scaled solar irradiance
  const double* surf_emis;     // [ncol][nband]; shortwave: the band albedo
  const double* conv;          // [ncol][nlay] heating-rate conversion
  const double* layer_weight;  // [ncol][nlay] normalised
  const double* hr_true;       // [ncol][nlay][nband]
  const double* fdn_true;      // [ncol][nhl][nband]
  const double* fup_true;      // [ncol][nhl][nband]
  const double* sfds;          // [ncol][ng] or NULL
  const double* sfut;          // [ncol][ng] or NULL
  double flux_weight, flux_profile_weight, broadband_weight, spectral_boundary_weight, negative_od_penalty;
  double* dtau;                // [ncell][ng] dJ/d(optical depth)
  double* jcol;                // [ncol] cost of each profile (incl. penalty)
  double* od_out;              // optional [ncell][ng] total optical depth (after clamp)
  double* flux_out;            // optional [ncol][2][nhl][ng]
  const double* gp_truth;      // [ncol][2][nhl][ng] per-g flux truth of ecckd_opt_set_gpoint_truth (longwave), or NULL: no such term
  double gp_weight;            // its weight, > 0 where gp_truth is set
};

constexpr double HR_WEIGHT = 3600.0 * 24.0;

// the truth and weight rows of one column
struct ColumnTruth { const double *cv, *lw, *hrt, *fdt, *fut; };
__device__ __forceinline__ ColumnTruth column_truth(const K8aArgs& a, int col) {
  const int nhl = a.nlay + 1;
  return {a.conv + (size_t)col * a.nlay, a.layer_weight + (size_t)col * a.nlay, a.hr_true + (size_t)col * a.nlay * a.nband,
          a.fdn_true + (size_t)col * nhl * a.nband, a.fup_true + (size_t)col * nhl * a.nband};
}

// How a flux at (half level, g) of this block's column is read: rows of LDS (the general and the cell-parallel kernel) ...
struct LdsFlux {
  const double *D, *U;
  int ng;
  __device__ __forceinline__ double dn(int i, int g) const { return D[i * ng + g]; }
  __device__ __forceinline__ double up(int i, int g) const { return U[i * ng + g]; }
};

// Negative-OD penalty and clamp of one cell (solve_adept.cpp:107-116): penalty = negative_od_penalty * tau^2, then the optical
// depth is SET to 0, so the only derivative that survives for a clamped cell is the penalty's.  Returns the absorption optical
// depth as the sweeps see it (keep_negative == 2: as it comes out of the look-up tables, negative cells included: the
// "relative_to" fluxes, od = value(aod) -> LblFluxes::calc_ckd_fluxes (optimize_lut.cpp:231-234), which has no clamp).
// SCATTERING marks the two things k_opt_forward_adjoint_rayleigh does differently, both on purpose: it reports the TOTAL
// optical depth tau + tau_ray (the other kernels: molecular absorption only, run_ckd.cpp:318-326), and it writes dJ/dtau of
// every cell, 0 where nothing was clamped, because its phase E2 ADDS the transfer's share where the others store theirs.
// (tau_ray is read by <true> alone, for the reported optical depth; the other kernels add it to what this returns.)
template <bool SCATTERING>
__device__ __forceinline__ double clamp_cell(const K8aArgs& a, size_t at, double tau, double tau_ray, bool& clamped, double& penalty) {
  const double tau_raw = tau;
  clamped = tau < 0.0;
  if (clamped) {
    penalty += tau * tau;
    tau = 0.0;
  }
  if constexpr (SCATTERING) a.dtau[at] = clamped ? 2.0 * a.negative_od_penalty * tau_raw : 0.0;
  else if (clamped) a.dtau[at] = 2.0 * a.negative_od_penalty * tau_raw;
  if (a.od_out) {
    const double od = (a.keep_negative && clamped) ? tau_raw : tau;
    if constexpr (SCATTERING) a.od_out[at] = od + tau_ray; else a.od_out[at] = od;
  }
  return a.keep_negative == 2 ? tau_raw : tau;
}

// Longwave layer terms (radiative_transfer_lw.cpp:41-43): ex = exp(-D tau), eps = 1 - ex, fac
__device__ __forceinline__ void lw_eps_fac(double tau, double& ex, double& eps, double& fac) {
  ex = ecckd::exp_fast(-kD * tau);
  eps = 1.0 - ex;
  fac = (eps > 1.0e-5) ? 1.0 - ecckd::div_fast(eps * (1.0 / kD), tau) : 0.5 * eps;
}

// Adjoint of both longwave sweeps at layer l: dJ/dtau_l from the adjoints dn_bar of dn[l+1] and ubar_l of up[l], the forward
// dn[l] and up[l+1], the Planck levels b0 = B_l, b1 = B_l+1, and tau, ex = exp(-D tau) of the layer
//   dn_{l+1} = dn_l*(1-eps) + B_l*(eps-fac) + B_{l+1}*fac
//   up_l     = up_{l+1}*(1-eps) + B_{l+1}*(eps-fac) + B_l*fac
__device__ __forceinline__ double lw_tau_bar(double dn_bar, double ubar_l, double dn_l, double up_next, double b0, double b1, double tau, double ex) {
  const double eps = 1.0 - ex;
  const bool thick = eps > 1.0e-5;
  const double rtau = thick ? ecckd::div_fast(1.0 / kD, tau) : 0.0;      // 1 / (D tau)
  const double t_bar = dn_bar * dn_l + ubar_l * up_next;
  const double a_bar = dn_bar * b0 + ubar_l * b1;
  const double f_bar = dn_bar * b1 + ubar_l * b0;
  const double eps_bar = -t_bar + a_bar;
  const double fac_bar = f_bar - a_bar;
  // fac(eps, tau): thick: 1 - eps/(D tau); thin: eps/2   (radiative_transfer_lw.cpp:42-43)
  const double dfac_deps = thick ? -rtau : 0.5;
  const double dfac_dtau = thick ? eps * rtau * (kD * rtau) : 0.0;        // eps / (D tau^2)
  // (eps_bar + fac_bar dfac_deps) (D ex) + fac_bar dfac_dtau, with the fused multiply-add written out: of the two products the
  // compiler may fuse either one into the sum, and which it picks has changed with the code around this function
  return __builtin_fma(fac_bar, dfac_dtau, (eps_bar + fac_bar * dfac_deps) * (kD * ex));
}

// The same along a path of secant sec (k_opt_forward_adjoint_lw_angles, once per zenith angle): ex = exp(-sec tau), and
// rtau = 1 / (sec tau) comes from the caller - it is read only where the layer is thick - who forms it from one reciprocal of tau
// for all the angles of a cell.  A function of its own: with lw_tau_bar written as the sec = D case of this one the compiler
// orders the instructions of the two-stream longwave kernels differently, and their code stays what was measured.
__device__ __forceinline__ double lw_tau_bar_sec(double sec, double rtau, double dn_bar, double ubar_l, double dn_l, double up_next, double b0,
                                                 double b1, double ex) {
  const double eps = 1.0 - ex;
  const bool thick = eps > 1.0e-5;
  const double t_bar = dn_bar * dn_l + ubar_l * up_next;
  const double a_bar = dn_bar * b0 + ubar_l * b1;
  const double f_bar = dn_bar * b1 + ubar_l * b0;
  const double eps_bar = -t_bar + a_bar;
  const double fac_bar = f_bar - a_bar;
  const double dfac_deps = thick ? -rtau : 0.5;
  const double dfac_dtau = thick ? eps * rtau * (sec * rtau) : 0.0;       // eps / (sec tau^2)
  return __builtin_fma(fac_bar, dfac_dtau, (eps_bar + fac_bar * dfac_deps) * (sec * ex));
}

// Weights of the squared band residuals of dn / up at half level i: spectral (s) and broadband (b).  lw: the column's layer weights.
struct LevelWeights { double wd_s, wu_s, wd_b, wu_b; };
__device__ __forceinline__ LevelWeights level_weights(const K8aArgs& a, const double* lw, bool sw, bool all_pos, int i) {
  LevelWeights w = {0.0, 0.0, 0.0, 0.0};
  if (i == a.nlay) { w.wd_s = a.flux_weight; w.wd_b = a.flux_weight; }
  if (i == 0) {
    // SW: 20 x on the spectral TOA upwelling (calc_cost_function_sw.cpp:214); its broadband term only if all albedos > 0 (:252)
    w.wu_s = sw ? 20.0 * a.flux_weight : a.flux_weight;
    w.wu_b = (!sw || all_pos) ? a.flux_weight : 0.0;
  }
  if (i >= 1 && i <= a.nlay - 1 && a.flux_profile_weight > 0.0) {
    const double iw = a.flux_profile_weight * 0.5 * (lw[i - 1] + lw[i]);
    w.wd_s = iw; w.wu_s = iw; w.wd_b = iw;
    w.wu_b = (!sw || all_pos) ? iw : 0.0;                        // :264
  }
  return w;
}

// The per-g boundary term of the g point of this lane: longwave calc_cost_function_lw.cpp:223-229 on the un-banded fluxes at
// the surface and the TOA; shortwave calc_cost_function_sw.cpp:271-274 with per-g (erythemal) weights, carried in sfut, on the
// surface downwelling.  The relative-to fluxes are subtracted first.  Adds its cost to jpart and returns the seeds it adds to
// dJ/d(dn at the surface) and dJ/d(up at the TOA).  (SW is a template argument, not a flag: with a flag the compiler merges the
// stores of the two branches into one through a selected address, and the seeds leave the registers.)
template <bool SW, class Flux>
__device__ __forceinline__ void boundary_term(const K8aArgs& a, int col, int g, const Flux& flux, double& jpart,
                                              double& g_dn_surf_extra, double& g_up_toa_extra) {
  g_dn_surf_extra = 0.0; g_up_toa_extra = 0.0;
  if (a.sfds && a.sfut && (SW || a.spectral_boundary_weight > 0.0)) {
    const int nhl = a.nlay + 1;
    const double reld = a.rel_flux ? a.rel_flux[((size_t)col * 2 * nhl + a.nlay) * a.ng + g] : 0.0;
    const double d = (flux.dn(a.nlay, g) - reld) - a.sfds[(size_t)col * a.ng + g];
    if constexpr (SW) {
      const double wgt = a.sfut[(size_t)col * a.ng + g];
      jpart += wgt * d * d;
      g_dn_surf_extra = 2.0 * wgt * d;
    } else {
      const double relu = a.rel_flux ? a.rel_flux[((size_t)col * 2 * nhl + nhl) * a.ng + g] : 0.0;
      const double c = (flux.up(0, g) - relu) - a.sfut[(size_t)col * a.ng + g];
      jpart += a.spectral_boundary_weight * (d * d + c * c);
      g_dn_surf_extra = 2.0 * a.spectral_boundary_weight * d;
      g_up_toa_extra = 2.0 * a.spectral_boundary_weight * c;
    }
  }
}

// The per-g flux-profile term of ecckd_opt_set_gpoint_truth (longwave; the per-g twin of flux_profile_weight, not in the
// reference): J_gp = w sum_i hw_i sum_g [((dn - rel) - T_dn)^2 + ((up - rel) - T_up)^2] over ALL half levels, hw_i the mean of
// the normalised weights of the layers that touch level i (half of the one layer at the two ends, so sum_i hw_i = 1).
// Residual and seed are written once, here.  Called by every thread (layer group lgrp of nlgrp, g point g) of the cell-parallel
// and the angle kernel once nothing reads the forward flux rows s_D, s_U [nhl][ng] any more - the band sums are formed, the
// boundary term and the cell owners have taken what they need, a barrier has passed -: the thread turns the two fluxes of ITS
// half levels i = lgrp, lgrp + nlgrp, ... IN PLACE into the WHOLE seeds of the reversed recurrences at (i, g) - the band seed
// gdn / gup [nhl][nband] at the band b of g plus this term's 2 w hw_i residual on dJ/d(dn[i]) / dJ/d(up[i]) - and returns the
// cost of those levels, levels ascending.  The recurrences then find the seed of a level in the row where the forward flux
// was, in place of the band seed: they read row i before they overwrite it, still one LDS read per level, and the truth is
// read once, 512 contiguous bytes per wave, by all the waves of the block instead of the one that runs the recurrences.
// A barrier follows the call.
__device__ __forceinline__ double gpoint_seed_rows(const K8aArgs& a, const double* lw, int col, int g, int lgrp, int nlgrp, const double* gdn,
                                                   const double* gup, int b, double* s_D, double* s_U) {
  const int nlay = a.nlay, nhl = nlay + 1, ng = a.ng, nband = a.nband;
  const size_t at = (size_t)col * 2 * nhl * ng + g;
  const double* truth = a.gp_truth + at;
  const double* rel = a.rel_flux ? a.rel_flux + at : nullptr;
  double j = 0.0;
  // (one level at a time: the cell owners hold four values per cell in registers across this loop)
#pragma unroll 1
  for (int i = lgrp; i < nhl; i += nlgrp) {
    const double whw = a.gp_weight * (0.5 * ((i >= 1 ? lw[i - 1] : 0.0) + (i <= nlay - 1 ? lw[i] : 0.0)));
    const double rd = (s_D[i * ng + g] - (rel ? rel[(size_t)i * ng] : 0.0)) - truth[(size_t)i * ng];
    const double ru = (s_U[i * ng + g] - (rel ? rel[(size_t)(nhl + i) * ng] : 0.0)) - truth[(size_t)(nhl + i) * ng];
    j += whw * (rd * rd + ru * ru);
    s_D[i * ng + g] = gdn[i * nband + b] + 2.0 * whw * rd;
    s_U[i * ng + g] = gup[i * nband + b] + 2.0 * whw * ru;
  }
  return j;
}

// K8a, the general kernel.  grid = ncolumns (all scenes), block = ng rounded up to 64, LDS: lds::general.
__global__ void k_opt_forward_adjoint(const K8aArgs a, int do_sw) {
  extern __shared__ double smem[];
  const int nlay = a.nlay, ng = a.ng, ngpad = a.ngpad, nband = a.nband, nent = a.nent, ray_ent = a.ray_ent;
  const int nhl = nlay + 1;
  const auto L = lds::general(nlay, ng, nband);
  auto arr = [&](int which) { return (double*)((char*)smem + L.off[which]); };
  double* s_tau = arr(lds::GL_TAU);
  double* s_fdn = arr(lds::GL_FDN);
  double* s_fup = arr(lds::GL_FUP);
  double* s_bdn = arr(lds::GL_BDN);
  double* s_bup = arr(lds::GL_BUP);
  double* s_gdn = arr(lds::GL_GDN);
  double* s_gup = arr(lds::GL_GUP);
  double* s_red = arr(lds::GL_RED);
  unsigned char* s_clamp = (unsigned char*)arr(lds::GL_CLAMP);  // [nlay][ng] 1 where a negative optical depth was clamped
  const double* const k = a.k; const int* const ent_idx = a.ent_idx; const double* const ent_coef = a.ent_coef;
  const int* const band_of_g = a.band_of_g; const double* const surf_emis = a.surf_emis; const double* const rel_flux = a.rel_flux;
  double* const dtau = a.dtau;
  const double broadband_weight = a.broadband_weight;
  const int col = blockIdx.x;
  // blockDim = ngpad * (layer groups): the LUT gather is parallel over (layer group, g); the
  // sweeps and their adjoint are sequential in the layers and run on the first group only
  const int g = threadIdx.x % ngpad;
  const int lgrp = threadIdx.x / ngpad;
  const int nlgrp = blockDim.x / ngpad;
  const bool in_range = g < ng;
  const bool live = in_range && lgrp == 0;
  const double hr_weight = HR_WEIGHT;
  const double* pl = a.planck_hl + (size_t)col * nhl * ng;
  const size_t cell0 = (size_t)col * nlay;

  // ---- optical depth: sparse gather (calc_total_optical_depth, solve_adept.cpp:24-69) and
  //      the negative-OD penalty with clamp (clamp_cell)
  double penalty = 0.0;
  if (in_range) {
    for (int l = lgrp; l < nlay; l += nlgrp) {
      const int* ei = ent_idx + (cell0 + l) * nent;
      const double* ec = ent_coef + (cell0 + l) * nent;
      double tau = 0.0, tau_ray = 0.0;
      // eight (then four) entries at a time: the index -> coefficient loads of a batch are independent, so their (L2) latencies
      // overlap; the products are still added in entry order, absent entries (idx < 0) add an exact zero
      int e = 0;
      for (; e + 8 <= nent; e += 8) {
        int ix[8];
        double cv[8], kv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) { ix[q] = ei[e + q]; cv[q] = ec[e + q]; }
#pragma unroll
        for (int q = 0; q < 8; ++q) kv[q] = ix[q] >= 0 ? k[(size_t)ix[q] + g] : 0.0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          const double t = ix[q] >= 0 ? cv[q] * kv[q] : 0.0;
          if (e + q == ray_ent) tau_ray = t; else tau += t;
        }
      }
      for (; e + 4 <= nent; e += 4) {
        int ix[4];
        double cv[4], kv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { ix[q] = ei[e + q]; cv[q] = ec[e + q]; }
#pragma unroll
        for (int q = 0; q < 4; ++q) kv[q] = ix[q] >= 0 ? k[(size_t)ix[q] + g] : 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double t = ix[q] >= 0 ? cv[q] * kv[q] : 0.0;
          if (e + q == ray_ent) tau_ray = t; else tau += t;
        }
      }
      for (; e < nent; ++e) {
        const int idx = ei[e];
        if (idx >= 0) {
          if (e == ray_ent) tau_ray = ec[e] * k[(size_t)idx + g];
          else tau += ec[e] * k[(size_t)idx + g];
        }
      }
      bool clamped;
      tau = clamp_cell<false>(a, (cell0 + l) * ng + g, tau, tau_ray, clamped, penalty);
      s_clamp[l * ng + g] = clamped ? 1 : 0;
      tau += tau_ray;
      s_tau[l * ng + g] = tau;
    }
  }
  __syncthreads();
  // ---- forward sweeps ----
  // shortwave: are all band albedos > 0 (broadband/profile upwelling terms, calc_cost_function_sw.cpp:252,:264)?
  // all <= 0 selects the direct-only model with zero upwelling (:145-150)
  bool all_pos = true, all_nonpos = true;
  double cos_sza = 1.0;
  if (do_sw) {
    for (int b = 0; b < nband; ++b) {
      const bool pos = surf_emis[(size_t)col * nband + b] > 0.0;
      all_pos = all_pos && pos;
      all_nonpos = all_nonpos && !pos;
    }
    cos_sza = a.mu0[col];
  }
  if (live && !do_sw) {
    // radiative_transfer_lw.cpp:41-59
    double dn = 0.0;
    s_fdn[g] = 0.0;
    for (int l = 0; l < nlay; ++l) {
      double ex, eps, fac;
      lw_eps_fac(s_tau[l * ng + g], ex, eps, fac);
      dn = dn * (1.0 - eps) + pl[l * ng + g] * (eps - fac) + pl[(l + 1) * ng + g] * fac;
      s_fdn[(l + 1) * ng + g] = dn;
    }
    const double es = surf_emis[(size_t)col * nband + band_of_g[g]];
    double up = pl[nlay * ng + g] * es + (1.0 - es) * dn;  // surf_planck = planck_hl(end), optimize_lut.cpp:267
    s_fup[nlay * ng + g] = up;
    for (int l = nlay - 1; l >= 0; --l) {
      double ex, eps, fac;
      lw_eps_fac(s_tau[l * ng + g], ex, eps, fac);
      up = up * (1.0 - eps) + pl[(l + 1) * ng + g] * (eps - fac) + pl[l * ng + g] * fac;
      s_fup[l * ng + g] = up;
    }
  }
  if (live && do_sw) {
    // radiative_transfer_direct_sw / _norayleigh_sw (radiative_transfer_sw.cpp:26-77); row 0 of the
    // per-profile "planck" block carries the scaled solar irradiance per g (solve_adept.cpp:176-186),
    // surf_emis the effective band albedo.  Albedo 0 gives up = 0, which is the direct-only branch.
    const double minus_sec_sza = -1.0 / cos_sza;
    double dn = cos_sza * pl[g];
    s_fdn[g] = dn;
    for (int l = 0; l < nlay; ++l) {
      dn = dn * ecckd::exp_fast(minus_sec_sza * s_tau[l * ng + g]);
      s_fdn[(l + 1) * ng + g] = dn;
    }
    const double alb = all_nonpos ? 0.0 : surf_emis[(size_t)col * nband + band_of_g[g]];
    double up = dn * alb;
    s_fup[nlay * ng + g] = up;
    for (int l = nlay - 1; l >= 0; --l) {
      up = up * ecckd::exp_fast(-2.0 * s_tau[l * ng + g]);
      s_fup[l * ng + g] = up;
    }
  }
  if (live) {
    if (a.flux_out) {
      double* fo = a.flux_out + (size_t)col * 2 * nhl * ng;
      for (int i = 0; i < nhl; ++i) {
        fo[i * ng + g] = s_fdn[i * ng + g];
        fo[(nhl + i) * ng + g] = s_fup[i * ng + g];
      }
    }
  }
  __syncthreads();
  // The band sums and the cost below are this kernel's OWN, not band_sums / cost_residuals / cost_seed of the other two: it
  // scans band_of_g instead of the bands' CSR, adds the heating-rate seeds in two passes and splits jpart over the threads
  // differently (sharing would change jcol), and it is the independent form the tests cross-check the other two against.
  // ---- band sums (calc_cost_function_lw.cpp:171-184) ----
  for (int t = threadIdx.x; t < nhl * nband; t += blockDim.x) {
    const int i = t / nband, b = t % nband;
    double sd = 0.0, su = 0.0;
    const double* rel = rel_flux ? rel_flux + (size_t)col * 2 * nhl * ng : nullptr;
    for (int gg = 0; gg < ng; ++gg) {
      if (band_of_g[gg] == b) {
        // the relative-to fluxes are subtracted per g point before the band sums (calc_cost_function_lw.cpp:162-165)
        sd += rel ? s_fdn[i * ng + gg] - rel[i * ng + gg] : s_fdn[i * ng + gg];
        su += rel ? s_fup[i * ng + gg] - rel[(nhl + i) * ng + gg] : s_fup[i * ng + gg];
      }
    }
    s_bdn[t] = sd;
    s_bup[t] = su;
  }
  __syncthreads();
  // ---- cost (:186-229) and its derivative w.r.t. the band fluxes ----
  const ColumnTruth ct = column_truth(a, col);
  const double *cv = ct.cv, *lw = ct.lw, *hrt = ct.hrt, *fdt = ct.fdt, *fut = ct.fut;
  // LW always mixes spectral and broadband (calc_cost_function_lw.cpp:209); SW only if broadband_weight > 0
  // (calc_cost_function_sw.cpp:243)
  const double spec_scale = (!do_sw || broadband_weight > 0.0) ? (1.0 - broadband_weight) / nband : 1.0;
  const double up_in_hr = do_sw ? 0.0 : 1.0;  // SW heating rate from the direct beam only (:197)
  for (int t = threadIdx.x; t < nhl * nband; t += blockDim.x) { s_gdn[t] = 0.0; s_gup[t] = 0.0; }
  __syncthreads();
  double jpart = 0.0;
  // heating-rate terms: thread per layer (the broadband residual needs all bands of a layer).  A half level receives the
  // contributions of the layer above and of the layer below it: the even layers add theirs first, then the odd ones - each
  // slot has ONE writer per pass, a fixed order without atomics
  for (int pass = 0; pass < 2; ++pass) {
    for (int l = threadIdx.x; l < nlay; l += blockDim.x) {
      if ((l & 1) != pass) continue;
      double rsum = 0.0;
      for (int b = 0; b < nband; ++b) {
        const double hrf = cv[l] * (s_bdn[(l + 1) * nband + b] - s_bdn[l * nband + b] -
                                    up_in_hr * (s_bup[(l + 1) * nband + b] - s_bup[l * nband + b]));
        rsum += hrf - hrt[l * nband + b];
      }
      for (int b = 0; b < nband; ++b) {
        const double hrf = cv[l] * (s_bdn[(l + 1) * nband + b] - s_bdn[l * nband + b] -
                                    up_in_hr * (s_bup[(l + 1) * nband + b] - s_bup[l * nband + b]));
        const double r = hrf - hrt[l * nband + b];
        jpart += spec_scale * hr_weight * hr_weight * lw[l] * r * r;
        const double dhr = 2.0 * hr_weight * hr_weight * lw[l] * (spec_scale * r + broadband_weight * rsum);
        // hr_l = conv_l * (dn[l+1] - dn[l] - up[l+1] + up[l])
        s_gdn[(l + 1) * nband + b] += dhr * cv[l];
        s_gdn[l * nband + b] += -dhr * cv[l];
        if (!do_sw) {
          s_gup[(l + 1) * nband + b] += -dhr * cv[l];
          s_gup[l * nband + b] += dhr * cv[l];
        }
      }
      jpart += broadband_weight * hr_weight * hr_weight * lw[l] * rsum * rsum;
    }
    __syncthreads();
  }
  // boundary-flux and flux-profile terms: thread per half level
  for (int i = threadIdx.x; i < nhl; i += blockDim.x) {
    const LevelWeights w = level_weights(a, lw, do_sw != 0, all_pos, i);
    const double wd_s = w.wd_s, wu_s = w.wu_s, wd_b = w.wd_b, wu_b = w.wu_b;
    if (wd_s != 0.0 || wu_s != 0.0) {
      double sd = 0.0, su = 0.0;
      for (int b = 0; b < nband; ++b) {
        sd += s_bdn[i * nband + b] - fdt[i * nband + b];
        su += s_bup[i * nband + b] - fut[i * nband + b];
      }
      for (int b = 0; b < nband; ++b) {
        const double dd = s_bdn[i * nband + b] - fdt[i * nband + b];
        const double du = s_bup[i * nband + b] - fut[i * nband + b];
        jpart += spec_scale * (wd_s * dd * dd + wu_s * du * du);
        s_gdn[i * nband + b] += 2.0 * (spec_scale * wd_s * dd + broadband_weight * wd_b * sd);
        s_gup[i * nband + b] += 2.0 * (spec_scale * wu_s * du + broadband_weight * wu_b * su);
      }
      jpart += broadband_weight * (wd_b * sd * sd + wu_b * su * su);
    }
  }
  __syncthreads();
  // ---- adjoint of the two sweeps, per g ----
  const LdsFlux flux = {s_fdn, s_fup, ng};
  double g_dn_surf_extra = 0.0, g_up_toa_extra = 0.0;
  if (live && do_sw) {
    const int b = band_of_g[g];
    const double alb = all_nonpos ? 0.0 : surf_emis[(size_t)col * nband + b];
    boundary_term<true>(a, col, g, flux, jpart, g_dn_surf_extra, g_up_toa_extra);
    // up_l = up_{l+1} * exp(-2 tau_l): d up_l / d tau_l = -2 up_l
    double up_bar = s_gup[b];
    for (int l = 0; l < nlay; ++l) {
      const double tau = s_tau[l * ng + g];
      if (s_clamp[l * ng + g] == 0) dtau[(cell0 + l) * ng + g] = up_bar * s_fup[l * ng + g] * (-2.0);
      up_bar = up_bar * ecckd::exp_fast(-2.0 * tau) + s_gup[(l + 1) * nband + b];
    }
    // dn_{l+1} = dn_l * exp(-tau_l / mu0): d dn_{l+1} / d tau_l = -dn_{l+1} / mu0
    const double minus_sec_sza = -1.0 / cos_sza;
    double dn_bar = s_gdn[nlay * nband + b] + g_dn_surf_extra + up_bar * alb;
    for (int l = nlay - 1; l >= 0; --l) {
      const double tau = s_tau[l * ng + g];
      if (s_clamp[l * ng + g] == 0) dtau[(cell0 + l) * ng + g] += dn_bar * s_fdn[(l + 1) * ng + g] * minus_sec_sza;
      dn_bar = dn_bar * ecckd::exp_fast(minus_sec_sza * tau) + s_gdn[l * nband + b];
    }
  }
  if (live && !do_sw) {
    const int b = band_of_g[g];
    const double es = surf_emis[(size_t)col * nband + b];
    boundary_term<false>(a, col, g, flux, jpart, g_dn_surf_extra, g_up_toa_extra);
    // The per-g flux-profile term (ecckd_opt_set_gpoint_truth), in this kernel's own plain form (gpoint_seed_rows is the other two's):
    // its cost, half levels ascending, then gp_dn / gp_up give the seed of a level from the forward flux still in LDS
    const bool gp = a.gp_truth != nullptr;
    const double* gp_t = gp ? a.gp_truth + (size_t)col * 2 * nhl * ng + g : nullptr;
    const double* gp_r = (gp && rel_flux) ? rel_flux + (size_t)col * 2 * nhl * ng + g : nullptr;
    auto gp_hw = [&](int i) { return 0.5 * ((i > 0 ? lw[i - 1] : 0.0) + (i < nlay ? lw[i] : 0.0)); };
    auto gp_dn = [&](int i) { return (s_fdn[i * ng + g] - (gp_r ? gp_r[(size_t)i * ng] : 0.0)) - gp_t[(size_t)i * ng]; };
    auto gp_up = [&](int i) { return (s_fup[i * ng + g] - (gp_r ? gp_r[(size_t)(nhl + i) * ng] : 0.0)) - gp_t[(size_t)(nhl + i) * ng]; };
    if (gp) {
      double jg = 0.0;
      for (int i = 0; i < nhl; ++i) {
        const double rd = gp_dn(i), ru = gp_up(i);
        jg += gp_hw(i) * (rd * rd + ru * ru);
      }
      jpart += a.gp_weight * jg;
    }
    // Adjoint of the up sweep.  It ran l = nlay-1 .. 0 (up_l from up_{l+1}), so the adjoint of
    // up[l] is complete once levels 0..l-1 have been visited: u_bar[0] = seed[0],
    // u_bar[l+1] = seed[l+1] + u_bar[l]*(1-eps_l).  u_bar[l] overwrites the forward up[l] in LDS
    // (the forward values are re-generated from the surface in the combine loop below).
    double up_bar = s_gup[b] + g_up_toa_extra;  // level 0
    if (gp) up_bar += 2.0 * a.gp_weight * gp_hw(0) * gp_up(0);
    for (int l = 0; l < nlay; ++l) {
      const double eps = 1.0 - ecckd::exp_fast(-kD * s_tau[l * ng + g]);
      double seed = s_gup[(l + 1) * nband + b];
      if (gp) seed += 2.0 * a.gp_weight * gp_hw(l + 1) * gp_up(l + 1);   // (row l + 1 still holds the forward up)
      s_fup[l * ng + g] = up_bar;
      up_bar = up_bar * (1.0 - eps) + seed;
    }
    // up_bar is now the adjoint of up[nlay]; through the surface condition it feeds dn[nlay].
    double dn_bar = s_gdn[nlay * nband + b] + g_dn_surf_extra + up_bar * (1.0 - es);
    if (gp) dn_bar += 2.0 * a.gp_weight * gp_hw(nlay) * gp_dn(nlay);
    // forward up[l+1] values: rebuild from the surface
    double up_fwd_next = pl[nlay * ng + g] * es + (1.0 - es) * s_fdn[nlay * ng + g];  // up[nlay]
    for (int l = nlay - 1; l >= 0; --l) {
      const bool clamped = s_clamp[l * ng + g] != 0;
      const double tau = s_tau[l * ng + g];
      const double ex = ecckd::exp_fast(-kD * tau);
      const double eps = 1.0 - ex;
      const bool thick = eps > 1.0e-5;
      const double rtau = thick ? ecckd::div_fast(1.0 / kD, tau) : 0.0;      // 1 / (D tau)
      // fac as the adjoint writes it, eps * (1 / (D tau)), not lw_eps_fac's (eps / D) / tau, and the product rounded before the
      // subtraction: the rebuilt up[l] has always been this one (the product used to be shared with dfac_dtau, which kept the
      // compiler from fusing it; written out so that it no longer depends on that)
      double fac;
      {
#pragma clang fp contract(off)
        const double eps_rtau = eps * rtau;
        fac = thick ? 1.0 - eps_rtau : 0.5 * eps;
      }
      const double b0 = pl[l * ng + g], b1 = pl[(l + 1) * ng + g];
      const double ubar_l = s_fup[l * ng + g];  // adjoint of up[l]
      const double dn_l = s_fdn[l * ng + g];
      const double tau_bar = lw_tau_bar(dn_bar, ubar_l, dn_l, up_fwd_next, b0, b1, tau, ex);
      if (!clamped) dtau[(cell0 + l) * ng + g] = tau_bar;
      // propagate
      const double up_l = up_fwd_next * (1.0 - eps) + b1 * (eps - fac) + b0 * fac;
      up_fwd_next = up_l;
      double seed = s_gdn[l * nband + b];
      if (gp) seed += 2.0 * a.gp_weight * gp_hw(l) * gp_dn(l);
      dn_bar = dn_bar * (1.0 - eps) + seed;
    }
  }
  jpart += a.negative_od_penalty * penalty;
  const double jtot = block_reduce_sum(jpart, s_red);
  if (threadIdx.x == 0) a.jcol[col] = jtot;
}

// ---- K8a, the form that runs (the kernel above stays as the general fall-back and as the cross-check of this one) ----
// Same arithmetic per cell and the same sequential recurrences, but only what IS sequential runs on one wave:
//   A  every thread (layer group, g) owns the cells (l = lgrp + j * nlgrp, g), j < NC: LUT gather, clamp + penalty, then the
//      layer's transmittance and its two source terms (longwave: 1 - eps, B_l (eps - fac) + B_l+1 fac, B_l+1 (eps - fac) +
//      B_l fac; shortwave: the two transmittances) - the `exp` and the division of every cell, 16 layers side by side;
//   B  ONE wave runs the two recurrences dn_l+1 = dn_l t_l + s_l, up_l = up_l+1 t_l + s'_l: one FMA per layer from LDS;
//   C, D  band sums and cost terms: band_sums, cost_residuals and cost_seed below, shared with the scattering kernel (the
//      kernel above keeps a form of its own: it is the cross-check);
//   E  the adjoint recurrences (again one FMA per layer on one wave), then every thread forms dJ/dtau of ITS cells from the
//      adjoint and forward fluxes at its layer and what it kept in registers (tau, exp(-D tau)).
// The sequential part of a profile shrinks from 4 x nlay (exp + division + recurrence) to 4 x nlay FMAs.  LDS per profile:
// longwave t | dn | up, shortwave dn | up only (the transmittances sit in the rows the fluxes then overwrite, and come back
// from the owners' registers for the adjoint recurrences) -> lds::cells: 100 KiB / 73 KiB at nlay = 54, ng = 64, 13 bands: two
// shortwave blocks per CU (tools/check_opt_tables.cpp holds these figures).
__device__ __forceinline__ double readlane_f64(double v, int src_lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}

// Optical depth of one cell for the 64 g points of a wave (calc_total_optical_depth, solve_adept.cpp:24-69).  The cell is the
// same for the whole wave, so its table entries (node row, coefficient) are fetched ONCE, one entry per lane (two coalesced
// loads instead of 2 x nent same-address loads per lane; the caller fetches them for all its cells before the first is used),
// and handed round with v_readlane: the row offsets arrive in scalar registers and the loads of the coefficient rows are
// independent of each other - sixteen in flight per batch, the products still added in entry order; absent entries (idx < 0)
// add nothing.  `active` = this lane has a g point.
constexpr int K8A_GB = 8;      // coefficient rows per batch; two batches are in flight (the next one is issued before the
                               // current one is used)
struct GatherBatch { int ix[K8A_GB]; double cv[K8A_GB], kv[K8A_GB]; };

// (row_stride = 1: my_idx is the offset of the row in k; else the row's number, of row_stride doubles each)
__device__ __forceinline__ void gather_issue(GatherBatch& b, int my_idx, double my_c, int q0, int ne, const double* __restrict__ k, int gl,
                                             int row_stride = 1) {
#pragma unroll
  for (int q = 0; q < K8A_GB; ++q) {
    const int e = (q0 + q) & 63;                          // (lanes at and beyond `ne` hold idx = -1: no test needed; a batch
    b.ix[q] = __builtin_amdgcn_readlane(my_idx, e);       //  never wraps round because ne <= 64 and q0 is a multiple of 8)
    b.cv[q] = readlane_f64(my_c, e);
  }
  // the loads are UNCONDITIONAL (an absent entry reads row 0 and is dropped by the select in gather_use): a test round a
  // load makes the compiler wait for everything in flight where the paths join, one memory round trip per entry
#pragma unroll
  for (int q = 0; q < K8A_GB; ++q) b.kv[q] = k[(size_t)max(b.ix[q], 0) * row_stride + gl];
}

__device__ __forceinline__ void gather_use(const GatherBatch& b, int e_first, int ray_ent, double& tau, double& tau_ray) {
#pragma unroll
  for (int q = 0; q < K8A_GB; ++q) {
    const double t = b.ix[q] >= 0 ? b.cv[q] * b.kv[q] : 0.0;
    if (e_first + q == ray_ent) tau_ray = t; else tau += t;
  }
}

// NB > 0: the table has at most NB * 8 entries - all NB batches are issued before the first is used, in straight-line code
// (no loop, no test: the compiler counts the loads in flight exactly).  NB = 0: any length, two batches in flight.
template <int NB>
__device__ __forceinline__ void gather_batches(int my_idx, double my_c, int e0, int ne, const double* __restrict__ k, int gl,
                                               int ray_ent, double& tau, double& tau_ray) {
  if constexpr (NB > 0) {
    GatherBatch b[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) gather_issue(b[i], my_idx, my_c, i * K8A_GB, ne, k, gl);
#pragma unroll
    for (int i = 0; i < NB; ++i) gather_use(b[i], e0 + i * K8A_GB, ray_ent, tau, tau_ray);
  } else {
    GatherBatch A, B;
    gather_issue(A, my_idx, my_c, 0, ne, k, gl);
    for (int q0 = 0; q0 < ne; q0 += 2 * K8A_GB) {
      // (the issues are unconditional - past the end they fetch row 0 and drop it -: a conditional issue makes the compiler
      // assume the fewest loads in flight and wait for all of them)
      gather_issue(B, my_idx, my_c, (q0 + K8A_GB) & 63, ne, k, gl);
      gather_use(A, e0 + q0, ray_ent, tau, tau_ray);
      gather_issue(A, my_idx, my_c, (q0 + 2 * K8A_GB) & 63, ne, k, gl);
      if (q0 + K8A_GB < ne) gather_use(B, e0 + q0 + K8A_GB, ray_ent, tau, tau_ray);
    }
  }
}

constexpr int K8A_CH = 8;      // layers per prefetch chunk of the sequential recurrences
constexpr int K8A_MAXR = 4;    // (half level, band) slots per thread in the cost phase: (nlay + 1) * nband <= K8A_MAXR * blockDim

// ---- phases C and D of the cell-parallel and the scattering kernel ----
// C: band sums (calc_cost_function_lw.cpp:171-184, calc_cost_function_sw.cpp:160-163) of the column's fluxes, read through
// `flux`; the g points of a band (CSR s_bp, s_bg) in increasing order.
template <class Flux>
__device__ __forceinline__ void band_sums(const K8aArgs& a, int col, const Flux& flux, const int* s_bp, const int* s_bg, double* s_bdn, double* s_bup) {
  const int nhl = a.nlay + 1, ng = a.ng, nband = a.nband;
  const double* rel = a.rel_flux ? a.rel_flux + (size_t)col * 2 * nhl * ng : nullptr;
  for (int t = threadIdx.x; t < nhl * nband; t += blockDim.x) {
    const int i = t / nband, b = t % nband;
    double sd = 0.0, su = 0.0;
    for (int q = s_bp[b]; q < s_bp[b + 1]; ++q) {
      const int gg = s_bg[q];
      const double dn = flux.dn(i, gg), up = flux.up(i, gg);
      // the relative-to fluxes are subtracted per g point before the band sums (calc_cost_function_lw.cpp:162-165)
      sd += rel ? dn - rel[i * ng + gg] : dn;
      su += rel ? up - rel[(nhl + i) * ng + gg] : up;
    }
    s_bdn[t] = sd;
    s_bup[t] = su;
  }
}

// The arrays of phase D in LDS: band fluxes in, residuals and their broadband sums out
struct CostLds { double *bdn, *bup, *r, *rsum, *sd, *su; };

// SW: the shortwave weights and scaling; NET: the heating rate comes from dn - up (longwave, scattering), else from dn alone
// (shortwave without scattering: the direct beam, calc_cost_function_sw.cpp:197).  Instances: <false, true> longwave cells,
// <true, false> shortwave cells, <true, true> scattering.
template <bool SW>
__device__ __forceinline__ double spectral_scale(const K8aArgs& a) {   // calc_cost_function_lw.cpp:209, sw :243
  return (!SW || a.broadband_weight > 0.0) ? (1.0 - a.broadband_weight) / a.nband : 1.0;
}

// D1 one thread per (layer, band): heating-rate residual; D2 per layer / half level: the broadband sums, bands in order.
// (calc_cost_function_lw.cpp:186-229; sw :186-277).  A barrier follows each; the cost shares go to this thread's jpart.
template <bool SW, bool NET>
__device__ __forceinline__ void cost_residuals(const K8aArgs& a, const ColumnTruth& ct, bool all_pos, const CostLds& s, double& jpart) {
  const int nlay = a.nlay, nhl = nlay + 1, nband = a.nband;
  const double spec_scale = spectral_scale<SW>(a);
  const double up_in_hr = NET ? 1.0 : 0.0;
  const double hrw2 = HR_WEIGHT * HR_WEIGHT;
  for (int t = threadIdx.x; t < nlay * nband; t += blockDim.x) {
    const int l = t / nband, b = t % nband;
    const double hrf = ct.cv[l] * (s.bdn[(l + 1) * nband + b] - s.bdn[l * nband + b] -
                                   up_in_hr * (s.bup[(l + 1) * nband + b] - s.bup[l * nband + b]));
    const double r = hrf - ct.hrt[t];
    s.r[t] = r;
    jpart += spec_scale * hrw2 * ct.lw[l] * r * r;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < nlay + nhl; t += blockDim.x) {
    if (t < nlay) {
      double rsum = 0.0;
      for (int b = 0; b < nband; ++b) rsum += s.r[t * nband + b];
      s.rsum[t] = rsum;
      jpart += a.broadband_weight * hrw2 * ct.lw[t] * rsum * rsum;
    } else {
      const int i = t - nlay;
      double sd = 0.0, su = 0.0;
      const LevelWeights w = level_weights(a, ct.lw, SW, all_pos, i);
      if (w.wd_s != 0.0 || w.wu_s != 0.0) {
        for (int b = 0; b < nband; ++b) {
          sd += s.bdn[i * nband + b] - ct.fdt[i * nband + b];
          su += s.bup[i * nband + b] - ct.fut[i * nband + b];
        }
        jpart += a.broadband_weight * (w.wd_b * sd * sd + w.wu_b * su * su);
      }
      s.sd[i] = sd;
      s.su[i] = su;
    }
  }
  __syncthreads();
}

// D3, slot t = (half level, band): dJ/d(band flux dn), dJ/d(band flux up), gathered from the two layers that touch the level
// and the boundary / profile terms - every slot has one writer, no atomics.  The slot's cost share goes to jpart (added here,
// not returned, so that the sum keeps the shape it has always had: a returned share could not fuse into jpart the same way).
template <bool SW, bool NET>
__device__ __forceinline__ void cost_seed(const K8aArgs& a, const ColumnTruth& ct, bool all_pos, const CostLds& s, int t, double& gd, double& gu, double& jpart) {
  const int nlay = a.nlay, nband = a.nband;
  const double spec_scale = spectral_scale<SW>(a);
  const double hrw2 = HR_WEIGHT * HR_WEIGHT;
  const int i = t / nband, b = t % nband;
  gd = 0.0; gu = 0.0;
  if (i >= 1) {                                                 // layer i-1 ends at this level
    const int l = i - 1;
    const double dhr = 2.0 * hrw2 * ct.lw[l] * (spec_scale * s.r[l * nband + b] + a.broadband_weight * s.rsum[l]);
    gd = dhr * ct.cv[l];
    if (NET) gu = -dhr * ct.cv[l];
  }
  if (i <= nlay - 1) {                                          // layer i starts at it
    const double dhr = 2.0 * hrw2 * ct.lw[i] * (spec_scale * s.r[i * nband + b] + a.broadband_weight * s.rsum[i]);
    gd += -dhr * ct.cv[i];
    if (NET) gu += dhr * ct.cv[i];
  }
  const LevelWeights w = level_weights(a, ct.lw, SW, all_pos, i);
  if (w.wd_s != 0.0 || w.wu_s != 0.0) {
    const double dd = s.bdn[t] - ct.fdt[t];
    const double du = s.bup[t] - ct.fut[t];
    jpart += spec_scale * (w.wd_s * dd * dd + w.wu_s * du * du);
    gd += 2.0 * (spec_scale * w.wd_s * dd + a.broadband_weight * w.wd_b * s.sd[i]);
    gu += 2.0 * (spec_scale * w.wu_s * du + a.broadband_weight * w.wu_b * s.su[i]);
  }
}

// GP (longwave only): the handle carries the per-g flux-profile term (gpoint_seed_rows); its seeds join the band seeds where phase E
// loads them.  A template argument, so that the instances of the handles without the term are the code they have always been.
template <int NC, bool SW, int NB, bool GP = false>
__global__ void __launch_bounds__(1024)
k_opt_forward_adjoint_cells(const K8aArgs a, const int* __restrict__ band_ptr /*[nband+1]*/, const int* __restrict__ band_g /*[ng]: g points by band*/) {
  extern __shared__ double smem[];
  const int nlay = a.nlay, ng = a.ng, ngpad = a.ngpad, nband = a.nband, nent = a.nent, ray_ent = a.ray_ent;
  const int nhl = nlay + 1;
  const auto L = lds::cells(nlay, ng, nband, SW);
  auto arr = [&](int which) { return (double*)((char*)smem + L.off[which]); };
  double* s_T = arr(lds::CL_T);                                  // longwave only: [nlay][ng] 1 - eps
  double* s_D = arr(lds::CL_D);                                  // [nhl][ng] down: sources / transmittances, fluxes, adjoints
  double* s_U = arr(lds::CL_U);                                  // [nhl][ng] up
  double* s_bdn = arr(lds::CL_BDN);                              // [nhl][nband] band fluxes, then dJ/d(band flux)
  double* s_bup = arr(lds::CL_BUP);
  // [nlay][nband] heating-rate residuals, [nlay] their broadband sums, 2 x [nhl] broadband flux residuals
  const CostLds cost = {s_bdn, s_bup, arr(lds::CL_R), arr(lds::CL_RSUM), arr(lds::CL_SD), arr(lds::CL_SU)};
  double* s_red = arr(lds::CL_RED);                              // [16]
  int* s_bp = (int*)arr(lds::CL_BP);                             // [nband + 1]
  int* s_bg = (int*)arr(lds::CL_BG);                             // [ng]
  const double* const k = a.k; const int* const ent_idx = a.ent_idx; const double* const ent_coef = a.ent_coef;
  const int* const band_of_g = a.band_of_g; const double* const surf_emis = a.surf_emis; double* const dtau = a.dtau;
  const int col = blockIdx.x;
  const int g = threadIdx.x % ngpad;
  const int lgrp = __builtin_amdgcn_readfirstlane(threadIdx.x / ngpad);     // ngpad is a multiple of 64: uniform in a wave
  const int nlgrp = blockDim.x / ngpad;
  const bool in_range = g < ng;
  const bool live = in_range && lgrp == 0;
  const double* pl = a.planck_hl + (size_t)col * nhl * ng;
  const size_t cell0 = (size_t)col * nlay;
  bool all_pos = true, all_nonpos = true;
  double cos_sza = 1.0;
  if (SW) {
    for (int b = 0; b < nband; ++b) {
      const bool pos = surf_emis[(size_t)col * nband + b] > 0.0;
      all_pos = all_pos && pos;
      all_nonpos = all_nonpos && !pos;
    }
    cos_sza = a.mu0[col];
  }
  const double minus_sec_sza = -1.0 / cos_sza;
  for (int t = threadIdx.x; t <= nband; t += blockDim.x) s_bp[t] = band_ptr[t];
  for (int t = threadIdx.x; t < ng; t += blockDim.x) s_bg[t] = band_g[t];

  // ---- A: the cells of this thread ----
  double c_tau[NC], c_t[NC];       // optical depth as the sweeps see it; exp(-D tau) (longwave) / exp(-tau / mu0) (shortwave)
  double c_tu[SW ? NC : 1];        // shortwave: exp(-2 tau)
  unsigned clamp_mask = 0;
  double penalty = 0.0;
  // the table entries of all the cells of this thread first (entries 0..63; tables with more come in further rounds below)
  const int lane = threadIdx.x & 63;
  const int gl = in_range ? g : 0;        // lanes beyond the last g point read (and drop) the first one's values
  int t_idx[NC];
  double t_c[NC];
  const int ne0 = min(64, nent);
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int l = lgrp + j * nlgrp;
    const bool have = l < nlay && lane < ne0;
    t_idx[j] = have ? ent_idx[(cell0 + l) * nent + lane] : -1;
    t_c[j] = have ? ent_coef[(cell0 + l) * nent + lane] : 0.0;
  }
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int l = lgrp + j * nlgrp;
    c_tau[j] = 0.0; c_t[j] = 1.0;
    if constexpr (SW) c_tu[j] = 1.0;
    if (l < nlay) {
      double tau = 0.0, tau_ray = 0.0;
      gather_batches<NB>(t_idx[j], t_c[j], 0, ne0, k, gl, ray_ent, tau, tau_ray);
      for (int e0 = 64; e0 < nent; e0 += 64) {
        const int ne = min(64, nent - e0);
        const int my_idx = lane < ne ? ent_idx[(cell0 + l) * nent + e0 + lane] : -1;
        const double my_c = lane < ne ? ent_coef[(cell0 + l) * nent + e0 + lane] : 0.0;
        gather_batches<0>(my_idx, my_c, e0, ne, k, gl, ray_ent, tau, tau_ray);
      }
      if (in_range) {
        bool clamped;
        tau = clamp_cell<false>(a, (cell0 + l) * ng + g, tau, tau_ray, clamped, penalty);
        if (clamped) clamp_mask |= 1u << j;
        tau += tau_ray;
        c_tau[j] = tau;
        if constexpr (!SW) {
          double ex, eps, fac;
          lw_eps_fac(tau, ex, eps, fac);
          const double b0 = pl[l * ng + g], b1 = pl[(l + 1) * ng + g];
          c_t[j] = ex;
          s_T[l * ng + g] = 1.0 - eps;
          s_D[(l + 1) * ng + g] = b0 * (eps - fac) + b1 * fac;        // :47-49, the part of flux_dn(l+1) that is not flux_dn(l)
          s_U[l * ng + g] = b1 * (eps - fac) + b0 * fac;              // :56-58
        } else {
          const double td = ecckd::exp_fast(minus_sec_sza * tau), tu = ecckd::exp_fast(-2.0 * tau);
          c_t[j] = td;
          c_tu[j] = tu;
          s_D[(l + 1) * ng + g] = td;
          s_U[l * ng + g] = tu;
        }
      }
    }
  }
  __syncthreads();
  // ---- B: the two recurrences, one wave; the rows of a chunk of layers are fetched before its chain of FMAs starts ----
  if (live) {
    // full chunks without a test per layer (a scalar branch per step costs more than the step), then the remainder
    double dn = SW ? cos_sza * pl[g] : 0.0;
    double* pD = s_D + g;
    double* pU = s_U + g;
    const double* pT = s_T + g;
    pD[0] = dn;
    int l = 0;
    for (; l + K8A_CH <= nlay; l += K8A_CH) {
      double tt[K8A_CH], ss[K8A_CH];
#pragma unroll
      for (int q = 0; q < K8A_CH; ++q) {
        ss[q] = pD[(l + q + 1) * ng];
        if constexpr (!SW) tt[q] = pT[(l + q) * ng];
      }
#pragma unroll
      for (int q = 0; q < K8A_CH; ++q) {
        if constexpr (SW) dn = dn * ss[q]; else dn = dn * tt[q] + ss[q];
        pD[(l + q + 1) * ng] = dn;
      }
    }
    for (; l < nlay; ++l) {
      if constexpr (SW) dn = dn * pD[(l + 1) * ng]; else dn = dn * pT[l * ng] + pD[(l + 1) * ng];
      pD[(l + 1) * ng] = dn;
    }
    double up;
    if constexpr (SW) {
      const double alb = all_nonpos ? 0.0 : surf_emis[(size_t)col * nband + band_of_g[g]];
      up = dn * alb;
    } else {
      const double es = surf_emis[(size_t)col * nband + band_of_g[g]];
      up = pl[nlay * ng + g] * es + (1.0 - es) * dn;              // surf_planck = planck_hl(end), optimize_lut.cpp:267
    }
    pU[nlay * ng] = up;
    l = nlay - 1;
    for (; l - (K8A_CH - 1) >= 0; l -= K8A_CH) {
      double tt[K8A_CH], ss[K8A_CH];
#pragma unroll
      for (int q = 0; q < K8A_CH; ++q) {
        ss[q] = pU[(l - q) * ng];
        if constexpr (!SW) tt[q] = pT[(l - q) * ng];
      }
#pragma unroll
      for (int q = 0; q < K8A_CH; ++q) {
        if constexpr (SW) up = up * ss[q]; else up = up * tt[q] + ss[q];
        pU[(l - q) * ng] = up;
      }
    }
    for (; l >= 0; --l) {
      if constexpr (SW) up = up * pU[l * ng]; else up = up * pT[l * ng] + pU[l * ng];
      pU[l * ng] = up;
    }
  }
  __syncthreads();
  if (a.flux_out && in_range) {
    double* fo = a.flux_out + (size_t)col * 2 * nhl * ng;
    for (int i = lgrp; i < nhl; i += nlgrp) {
      fo[i * ng + g] = s_D[i * ng + g];
      fo[(nhl + i) * ng + g] = s_U[i * ng + g];
    }
  }
  // ---- C: band sums of the flux rows ----
  const LdsFlux flux = {s_D, s_U, ng};
  const ColumnTruth ct = column_truth(a, col);
  band_sums(a, col, flux, s_bp, s_bg, s_bdn, s_bup);
  __syncthreads();
  // ---- D: cost and its derivative with respect to the band fluxes; the heating rate takes the net flux in the longwave ----
  double jpart = 0.0;
  cost_residuals<SW, !SW>(a, ct, all_pos, cost, jpart);
  {
    // The seeds overwrite the band fluxes they are made from, so they wait in registers for the barrier: up to K8A_MAXR rounds
    // of the block over the (half level, band) slots (forward_plan refuses a shape that needs more)
    constexpr int MAXR = K8A_MAXR;
    double gd_r[MAXR], gu_r[MAXR];
    int nr = 0;
    for (int t = threadIdx.x; t < nhl * nband && nr < MAXR; t += blockDim.x, ++nr) {
      double gd, gu;
      cost_seed<SW, !SW>(a, ct, all_pos, cost, t, gd, gu, jpart);
      gd_r[nr] = gd;
      gu_r[nr] = gu;
    }
    __syncthreads();
    nr = 0;
    for (int t = threadIdx.x; t < nhl * nband && nr < MAXR; t += blockDim.x, ++nr) {
      s_bdn[t] = gd_r[nr];                                        // from here on: dJ/d(band flux dn), dJ/d(band flux up)
      s_bup[t] = gu_r[nr];
    }
  }
  double* s_gdn = s_bdn;
  double* s_gup = s_bup;
  // ---- E: adjoint.  The owners take the forward fluxes at their cells before the rows are reused ----
  double c_f0[NC], c_f1[NC];      // longwave: dn_l, up_l+1; shortwave: dn_l+1, up_l
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int l = lgrp + j * nlgrp;
    c_f0[j] = 0.0; c_f1[j] = 0.0;
    if (in_range && l < nlay) {
      c_f0[j] = SW ? s_D[(l + 1) * ng + g] : s_D[l * ng + g];
      c_f1[j] = SW ? s_U[l * ng + g] : s_U[(l + 1) * ng + g];
    }
  }
  double g_dn_surf_extra = 0.0, g_up_toa_extra = 0.0;
  if (live) boundary_term<SW>(a, col, g, flux, jpart, g_dn_surf_extra, g_up_toa_extra);
  static_assert(!(GP && SW), "the per-g flux-profile term is longwave only");
  __syncthreads();
  if constexpr (GP) {
    // the flux rows become the seeds of the per-g flux-profile term (the owners hold the forward fluxes they need in c_f0, c_f1)
    if (in_range) jpart += gpoint_seed_rows(a, ct.lw, col, g, lgrp, nlgrp, s_gdn, s_gup, band_of_g[g], s_D, s_U);
    __syncthreads();
  }
  if constexpr (SW) {
    // the transmittances back into the rows the fluxes occupied
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int l = lgrp + j * nlgrp;
      if (in_range && l < nlay) {
        s_D[(l + 1) * ng + g] = c_t[j];
        s_U[l * ng + g] = c_tu[j];
      }
    }
    __syncthreads();
  }
  if (live) {
    const int b = band_of_g[g];
    // u_bar[0] = seed[0], u_bar[l+1] = seed[l+1] + u_bar[l] t_l: row l of s_U becomes the adjoint of up[l]
    double up_bar = (GP ? s_U[g] : s_gup[b]) + g_up_toa_extra;
    double* pD = s_D + g;
    double* pU = s_U + g;
    const double* pT = s_T + g;
    const double* gU = s_gup + b;
    const double* gD = s_gdn + b;
    // (GP: the seed of a level comes from row l + 1 of s_U / row l of s_D, which still hold it when the recurrence adds it - each
    // row is overwritten one step later, and a chunk loads all its rows before it stores any)
    int l = 0;
    for (; l + K8A_CH <= nlay; l += K8A_CH) {
      double tt[K8A_CH], ss[K8A_CH];
#pragma unroll
      for (int q = 0; q < K8A_CH; ++q) {
        tt[q] = SW ? pU[(l + q) * ng] : pT[(l + q) * ng];
        ss[q] = GP ? pU[(l + q + 1) * ng] : gU[(l + q + 1) * nband];
      }
#pragma unroll
      for (int q = 0; q < K8A_CH; ++q) {
        pU[(l + q) * ng] = up_bar;
        up_bar = up_bar * tt[q] + ss[q];
      }
    }
    for (; l < nlay; ++l) {
      const double t = SW ? pU[l * ng] : pT[l * ng];
      double seed = 0.0;
      if constexpr (GP) seed = pU[(l + 1) * ng];
      pU[l * ng] = up_bar;
      if constexpr (GP) up_bar = up_bar * t + seed;
      else up_bar = up_bar * t + gU[(l + 1) * nband];
    }
    // through the surface condition into dn[nlay]; row l+1 of s_D becomes the adjoint of dn[l+1]
    const double refl = SW ? (all_nonpos ? 0.0 : surf_emis[(size_t)col * nband + b]) : 1.0 - surf_emis[(size_t)col * nband + b];
    double dn_bar = (GP ? pD[nlay * ng] : gD[nlay * nband]) + g_dn_surf_extra + up_bar * refl;
    l = nlay - 1;
    for (; l - (K8A_CH - 1) >= 0; l -= K8A_CH) {
      double tt[K8A_CH], ss[K8A_CH];
#pragma unroll
      for (int q = 0; q < K8A_CH; ++q) {
        tt[q] = SW ? pD[(l - q + 1) * ng] : pT[(l - q) * ng];
        ss[q] = GP ? pD[(l - q) * ng] : gD[(l - q) * nband];
      }
#pragma unroll
      for (int q = 0; q < K8A_CH; ++q) {
        pD[(l - q + 1) * ng] = dn_bar;
        dn_bar = dn_bar * tt[q] + ss[q];
      }
    }
    for (; l >= 0; --l) {
      const double t = SW ? pD[(l + 1) * ng] : pT[l * ng];
      double seed = 0.0;
      if constexpr (GP) seed = pD[l * ng];
      pD[(l + 1) * ng] = dn_bar;
      if constexpr (GP) dn_bar = dn_bar * t + seed;
      else dn_bar = dn_bar * t + gD[l * nband];
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int l = lgrp + j * nlgrp;
    if (in_range && l < nlay && !((clamp_mask >> j) & 1u)) {
      const double ubar_l = s_U[l * ng + g], dnbar = s_D[(l + 1) * ng + g];
      double tau_bar;
      if constexpr (SW) {
        // up_l = up_l+1 exp(-2 tau_l), dn_l+1 = dn_l exp(-tau_l / mu0)
        tau_bar = ubar_l * c_f1[j] * (-2.0) + dnbar * c_f0[j] * minus_sec_sza;
      } else {
        // (GP: exp(-D tau) comes back from the row of s_T, 1 - eps, which nothing overwrites - one rounding of 1 away from the
        // value the owner formed -, so that the instance keeps eight doubles fewer across phase E and stays out of scratch)
        const double ex = GP ? s_T[l * ng + g] : c_t[j];
        tau_bar = lw_tau_bar(dnbar, ubar_l, c_f0[j], c_f1[j], pl[l * ng + g], pl[(l + 1) * ng + g], c_tau[j], ex);
      }
      dtau[(cell0 + l) * ng + g] = tau_bar;
    }
  }
  jpart += a.negative_od_penalty * penalty;
  const double jtot = block_reduce_sum(jpart, s_red);
  if (threadIdx.x == 0) a.jcol[col] = jtot;
}

// ---- K8a with Rayleigh scattering (ECCKD_OPT_RAYLEIGH_SCATTERING): the two-stream transfer of lbl_rt.hpp and its adjoint ----
// Between optical depth and fluxes sits, per column and g point (levels 0 .. nlay from the top, D direct, V diffuse down, U up):
//   terms    R_l, T_l, Tdir_l, Rdir_l, Tdd_l = rayleigh_layer(tau_abs, tau_ray, mu0)            per cell
//   direct   D_0 = mu0 ssi,  D_l+1 = D_l Tdir_l
//   up       A_n = albedo, S_n = albedo D_n;  A_l, S_l = rayleigh_up(layer l, D_l, A_l+1, S_l+1)           l = n-1 .. 0
//   down     V_0 = 0, U_0 = S_0;  V_l+1, U_l+1 = rayleigh_down(layer l, D_l, A_l+1, S_l+1, V_l)            l = 0 .. n-1
//   model    dn_i = D_i + V_i, up_i = U_i -> band sums -> the shortwave cost (phase D, heating rate from dn - up)
// The adjoint (bars: dJ/d of the quantity; dnb_i, upb_i the seeds of phase D at the band of g, the per-g surface term added
// to dnb_n; i = 1 / (1 - A_l+1 R_l), a = A_l+1, s = S_l+1, everything at layer l unless indexed):
//   down sweep reversed, l = n-1 .. 0, c the carry into V_l (0 at the start):
//     vb = dnb_l+1 + c + upb_l+1 a;  nb = vb i;  q = vb V_l+1 i                  (q = -d/d(1 - a R))
//     Ab_l+1 = upb_l+1 V_l+1 + q R;  Sb_l+1 = upb_l+1 + nb R;  Db_l = dnb_l + nb Tdd
//     Rb = nb s + q a;  Tb = nb V_l;  Tddb = nb D_l;  c = nb T                   Ab_0 = 0, Sb_0 = upb_0, Db_n = dnb_n
//   up sweep reversed, l = 0 .. n-1, ca, cs the carries into A_l, S_l:
//     ab = Ab_l + ca;  sb = Sb_l + cs;  P = s + a Tdd D_l;  ib = ab T^2 a + sb T P
//     Rb += ab + ib i^2 a;  Tb += 2 ab T a i + sb P i;  Rdirb = sb D_l;  Tddb += sb T a D_l i
//     Db_l += sb (Rdir + T a Tdd i);  ca = ab T^2 i + sb T Tdd D_l i + ib i^2 R;  cs = sb T i
//   surface  Db_n += (Sb_n + cs) albedo
//   direct chain reversed, l = n-1 .. 0, t = Db_n:  Tdirb = t D_l;  t = Db_l + t Tdir
//   per cell  dJ/dtau_abs = Rb R' + Tb T' + Tdirb Tdir' + Rdirb Rdir' + Tddb Tdd',  ' = d/dtau_abs of rayleigh_layer_d
// Phases.  A (every lane owns the cells l = lgrp + j nlgrp of its g point): look-up, clamp and penalty, rayleigh_layer and
// rayleigh_layer_d - every exp, sqrt and division of the layer terms; B (one wave per 64 g points): the three forward
// recurrences over the stored terms; C, D: band_sums over D + V and U of the workspace, then cost_residuals and cost_seed
// <shortwave, net flux>, the functions the cell-parallel kernel calls; E1 (one wave per 64 g
// points): the three reversed recurrences - FMAs and one division per layer and sweep; E2 (cell owners): the sum above.
// The per-(level, g) state does not fit the LDS (23 arrays of (nlay + 1) ng doubles): it lives in a workspace of the handle,
// ws[column][slot][level][g], so a wave reads and writes 512 contiguous bytes; every element is written and read either by its
// own lane or by its owner with a block barrier in between.  The LDS holds the band and cost arrays only, so one kernel
// serves every shape.  All sums keep a fixed order.
enum RaySlot { RS_R, RS_T, RS_TDIR, RS_RDIR, RS_TDD,             // the layer terms, rows 0 .. nlay-1
               RS_DR, RS_DT, RS_DTDIR, RS_DRDIR, RS_DTDD,        // their d / d tau_abs (0 in clamped cells)
               RS_D, RS_A, RS_S, RS_V, RS_U,                     // levels 0 .. nlay
               RS_AB, RS_SB, RS_DB,                              // adjoints of A, S, D
               RS_RB, RS_TB, RS_TDIRB, RS_RDIRB, RS_TDDB,        // adjoints of the layer terms
               RS_COUNT };

// ... or (see LdsFlux) the column's slots of the workspace: total downwelling D + V, upwelling U
struct RayleighFlux {
  const double* wc;
  size_t slot;
  int ng;
  __device__ __forceinline__ double dn(int i, int g) const { return wc[RS_D * slot + i * ng + g] + wc[RS_V * slot + i * ng + g]; }
  __device__ __forceinline__ double up(int i, int g) const { return wc[RS_U * slot + i * ng + g]; }
};

// B: the forward recurrences of one g point; every pointer is its slot at this g, rows ng apart
__device__ __forceinline__ void rayleigh_forward_sweeps(int nlay, int ng, double d0, double alb, const double* __restrict__ pR,
                                                        const double* __restrict__ pT, const double* __restrict__ pTdir,
                                                        const double* __restrict__ pRdir, const double* __restrict__ pTdd,
                                                        double* __restrict__ pD, double* __restrict__ pA, double* __restrict__ pS,
                                                        double* __restrict__ pV, double* __restrict__ pU) {
  using ecckd::lbl::RayleighLayer;
  double d = d0;
  pD[0] = d;
#pragma unroll 4
  for (int l = 0; l < nlay; ++l) {
    d = d * pTdir[(size_t)l * ng];
    pD[(size_t)(l + 1) * ng] = d;
  }
  double a = alb, s = alb * d;
  pA[(size_t)nlay * ng] = a;
  pS[(size_t)nlay * ng] = s;
#pragma unroll 2
  for (int l = nlay - 1; l >= 0; --l) {
    const size_t r = (size_t)l * ng;
    const RayleighLayer L{pR[r], pT[r], pTdir[r], pRdir[r], pTdd[r]};
    double an, sn;
    ecckd::lbl::rayleigh_up(L, pD[r], a, s, an, sn);
    a = an; s = sn;
    pA[r] = a;
    pS[r] = s;
  }
  double v = 0.0;
  pV[0] = 0.0;
  pU[0] = s;
#pragma unroll 2
  for (int l = 0; l < nlay; ++l) {
    const size_t r = (size_t)l * ng, r1 = r + ng;
    const RayleighLayer L{pR[r], pT[r], pTdir[r], pRdir[r], pTdd[r]};
    double vn, un;
    ecckd::lbl::rayleigh_down(L, pD[r], pA[r1], pS[r1], v, vn, un);
    v = vn;
    pV[r1] = v;
    pU[r1] = un;
  }
}

// E1: the reversed recurrences of one g point (equations above).  gD, gU: dJ/d(band dn), dJ/d(band up) at the band of g, rows
// nband apart; dn_surf_extra: the per-g surface term's share of dnb_n.
__device__ __forceinline__ void rayleigh_adjoint_sweeps(int nlay, int ng, int nband, const double* gD, const double* gU, double dn_surf_extra,
                                                        double alb, const double* __restrict__ pR, const double* __restrict__ pT,
                                                        const double* __restrict__ pTdir, const double* __restrict__ pRdir,
                                                        const double* __restrict__ pTdd, const double* __restrict__ pD,
                                                        const double* __restrict__ pA, const double* __restrict__ pS,
                                                        const double* __restrict__ pV, double* __restrict__ pAb, double* __restrict__ pSb,
                                                        double* __restrict__ pDb, double* __restrict__ pRb, double* __restrict__ pTb,
                                                        double* __restrict__ pTdirb, double* __restrict__ pRdirb, double* __restrict__ pTddb) {
  double c = 0.0;
  pDb[(size_t)nlay * ng] = gD[nlay * nband] + dn_surf_extra;
#pragma unroll 2
  for (int l = nlay - 1; l >= 0; --l) {
    const size_t r = (size_t)l * ng, r1 = r + ng;
    const double a = pA[r1], s = pS[r1], R = pR[r], T = pT[r], Tdd = pTdd[r], Dl = pD[r], Vl = pV[r], Vn = pV[r1];
    const double inv = 1.0 / (1.0 - a * R);
    const double ub = gU[(l + 1) * nband];
    const double vb = gD[(l + 1) * nband] + (l + 1 == nlay ? dn_surf_extra : 0.0) + c + ub * a;
    const double nb = vb * inv;
    const double q = vb * Vn * inv;
    pAb[r1] = ub * Vn + q * R;
    pSb[r1] = ub + nb * R;
    pDb[r] = gD[l * nband] + nb * Tdd;
    pRb[r] = nb * s + q * a;
    pTb[r] = nb * Vl;
    pTddb[r] = nb * Dl;
    c = nb * T;
  }
  pAb[0] = 0.0;
  pSb[0] = gU[0];
  double ca = 0.0, cs = 0.0;
#pragma unroll 2
  for (int l = 0; l < nlay; ++l) {
    const size_t r = (size_t)l * ng, r1 = r + ng;
    const double a = pA[r1], s = pS[r1], R = pR[r], T = pT[r], Rdir = pRdir[r], Tdd = pTdd[r], Dl = pD[r];
    const double inv = 1.0 / (1.0 - a * R);
    const double ab = pAb[r] + ca, sb = pSb[r] + cs;
    const double P = s + a * Tdd * Dl;
    const double ib = ab * T * T * a + sb * T * P;
    pRb[r] += ab + ib * inv * inv * a;
    pTb[r] += 2.0 * ab * T * a * inv + sb * P * inv;
    pRdirb[r] = sb * Dl;
    pTddb[r] += sb * T * a * Dl * inv;
    pDb[r] += sb * (Rdir + T * a * Tdd * inv);
    ca = ab * T * T * inv + sb * T * Tdd * Dl * inv + ib * inv * inv * R;
    cs = sb * T * inv;
  }
  double t = pDb[(size_t)nlay * ng] + (pSb[(size_t)nlay * ng] + cs) * alb;
#pragma unroll 4
  for (int l = nlay - 1; l >= 0; --l) {
    const size_t r = (size_t)l * ng;
    pTdirb[r] = t * pD[r];
    t = pDb[r] + t * pTdir[r];
  }
}

// RAY_ACTIVE (ECCKD_OPT_RAYLEIGH_ACTIVE on a scattering handle): the kernel also leaves dJ/dk_ray per (column, g).  Phase A
// stores d/dtau_ray of the five layer terms (rayleigh_layer_dray) in five more slots of the workspace, RS_RAY_D ..., as the
// d/dtau_abs terms are stored - they are NOT zeroed in clamped cells: the clamp acts on the gases alone; phase E2 forms
//   dJ/dtau_ray = Rb R* + Tb T* + Tdirb Tdir* + Rdirb Rdir* + Tddb Tdd*          (* = d/dtau_ray at fixed tau_abs)
// of every cell, each thread adds moles_l dJ/dtau_ray over its own layers in ascending l, and the layer groups are added in
// group order through LDS (blockDim doubles behind the layout of lds::rayleigh) to ray_part[column][g], which sits behind the
// ncol columns of the workspace: no further kernel argument, and the <false> instance is the kernel it has always been.
constexpr int RS_RAY_D = RS_COUNT;                 // dR, dT, dTdir, dRdir, dTdd / dtau_ray
constexpr int RS_COUNT_ACTIVE = RS_COUNT + 5;
constexpr size_t ray_lds_offset(size_t layout_bytes) { return (layout_bytes + 7) / 8 * 8; }

template <bool RAY_ACTIVE>
__global__ void __launch_bounds__(512)
k_opt_forward_adjoint_rayleigh(const K8aArgs a, const int* __restrict__ band_ptr /*[nband+1]*/, const int* __restrict__ band_g /*[ng]: g points by band*/,
                               double* ws /*[ncol][NSLOT][nlay+1][ng], RAY_ACTIVE: then ray_part[ncol][ng]*/) {
  extern __shared__ double smem[];
  constexpr int NSLOT = RAY_ACTIVE ? RS_COUNT_ACTIVE : RS_COUNT;
  const int nlay = a.nlay, ng = a.ng, ngpad = a.ngpad, nband = a.nband, nent = a.nent, ray_ent = a.ray_ent;
  const int nhl = nlay + 1;
  const auto layout = lds::rayleigh(nlay, ng, nband);
  auto arr = [&](int which) { return (double*)((char*)smem + layout.off[which]); };
  double* s_bdn = arr(lds::RL_BDN);                              // [nhl][nband] band fluxes
  double* s_bup = arr(lds::RL_BUP);
  double* s_gdn = arr(lds::RL_GDN);                              // [nhl][nband] dJ/d(band flux)
  double* s_gup = arr(lds::RL_GUP);
  // [nlay][nband] heating-rate residuals, [nlay] their broadband sums, 2 x [nhl] broadband flux residuals
  const CostLds cost = {s_bdn, s_bup, arr(lds::RL_R), arr(lds::RL_RSUM), arr(lds::RL_SD), arr(lds::RL_SU)};
  double* s_red = arr(lds::RL_RED);                              // [16]
  int* s_bp = (int*)arr(lds::RL_BP);                             // [nband + 1]
  int* s_bg = (int*)arr(lds::RL_BG);                             // [ng]
  const double* const k = a.k; const int* const ent_idx = a.ent_idx; const double* const ent_coef = a.ent_coef;
  const int* const band_of_g = a.band_of_g; const double* const albedo = a.surf_emis; double* const dtau = a.dtau;
  const int col = blockIdx.x;
  const int g = threadIdx.x % ngpad;
  const int lgrp = __builtin_amdgcn_readfirstlane(threadIdx.x / ngpad);     // ngpad is a multiple of 64: uniform in a wave
  const int nlgrp = blockDim.x / ngpad;
  const bool in_range = g < ng;
  const bool live = in_range && lgrp == 0;
  const int lane = threadIdx.x & 63;
  const int gl = in_range ? g : 0;        // lanes beyond the last g point read (and drop) the first one's values
  const double* pl = a.planck_hl + (size_t)col * nhl * ng;      // row 0: the scaled solar irradiance
  const size_t cell0 = (size_t)col * nlay;
  const size_t slot = (size_t)nhl * ng;
  double* w = ws + (size_t)col * NSLOT * slot + gl;              // slot q of this g point: w + q * slot, rows ng apart
  bool all_pos = true;
  for (int b = 0; b < nband; ++b) all_pos = all_pos && albedo[(size_t)col * nband + b] > 0.0;
  const double cos_sza = a.mu0[col];
  const double minus_sec_sza = -1.0 / cos_sza;
  for (int t = threadIdx.x; t <= nband; t += blockDim.x) s_bp[t] = band_ptr[t];
  for (int t = threadIdx.x; t < ng; t += blockDim.x) s_bg[t] = band_g[t];

  // ---- A: the cells of this thread ----
  double penalty = 0.0;
  for (int l = lgrp; l < nlay; l += nlgrp) {
    double tau = 0.0, tau_ray = 0.0;
    for (int e0 = 0; e0 < nent; e0 += 64) {
      const int ne = min(64, nent - e0);
      const int my_idx = lane < ne ? ent_idx[(cell0 + l) * nent + e0 + lane] : -1;
      const double my_c = lane < ne ? ent_coef[(cell0 + l) * nent + e0 + lane] : 0.0;
      gather_batches<0>(my_idx, my_c, e0, ne, k, gl, ray_ent, tau, tau_ray);
    }
    if (in_range) {
      // <true>: dJ/dtau of every cell is written here - the penalty's derivative, all a clamped cell passes on (phase E2 adds
      // the transfer's share, 0 there: its d terms are 0) - and the reported optical depth includes tau_ray; both are meant
      bool clamped;
      tau = clamp_cell<true>(a, (cell0 + l) * ng + g, tau, tau_ray, clamped, penalty);
      const ecckd::lbl::RayleighLayer L = ecckd::lbl::rayleigh_layer(tau, tau_ray, cos_sza, minus_sec_sza);
      const ecckd::lbl::RayleighLayer dL = ecckd::lbl::rayleigh_layer_d(tau, tau_ray, cos_sza, minus_sec_sza);
      double* wl = w + (size_t)l * ng;
      wl[RS_R * slot] = L.R; wl[RS_T * slot] = L.T; wl[RS_TDIR * slot] = L.Tdir; wl[RS_RDIR * slot] = L.Rdir; wl[RS_TDD * slot] = L.Tdd;
      wl[RS_DR * slot] = clamped ? 0.0 : dL.R; wl[RS_DT * slot] = clamped ? 0.0 : dL.T; wl[RS_DTDIR * slot] = clamped ? 0.0 : dL.Tdir;
      wl[RS_DRDIR * slot] = clamped ? 0.0 : dL.Rdir; wl[RS_DTDD * slot] = clamped ? 0.0 : dL.Tdd;
      if constexpr (RAY_ACTIVE) {
        // (a clamped cell keeps these: tau is tau_ray there, w = 1 and the seed of w is 0)
        const ecckd::lbl::RayleighLayer rL = ecckd::lbl::rayleigh_layer_dray(tau, tau_ray, cos_sza, minus_sec_sza);
        wl[(RS_RAY_D + 0) * slot] = rL.R; wl[(RS_RAY_D + 1) * slot] = rL.T; wl[(RS_RAY_D + 2) * slot] = rL.Tdir;
        wl[(RS_RAY_D + 3) * slot] = rL.Rdir; wl[(RS_RAY_D + 4) * slot] = rL.Tdd;
      }
    }
  }
  __syncthreads();
  // ---- B: the forward recurrences, one wave per 64 g points ----
  const double alb = fmax(albedo[(size_t)col * nband + band_of_g[gl]], 0.0);      // a non-positive albedo counts as 0
  if (live)
    rayleigh_forward_sweeps(nlay, ng, cos_sza * pl[g], alb, w + RS_R * slot, w + RS_T * slot, w + RS_TDIR * slot, w + RS_RDIR * slot,
                            w + RS_TDD * slot, w + RS_D * slot, w + RS_A * slot, w + RS_S * slot, w + RS_V * slot, w + RS_U * slot);
  __syncthreads();
  const double* wc = ws + (size_t)col * NSLOT * slot;            // the column's slots, any g
  const RayleighFlux flux = {wc, slot, ng};
  if (a.flux_out && in_range) {
    double* fo = a.flux_out + (size_t)col * 2 * nhl * ng;
    for (int i = lgrp; i < nhl; i += nlgrp) {
      fo[i * ng + g] = flux.dn(i, g);                            // total downwelling
      fo[(nhl + i) * ng + g] = flux.up(i, g);
    }
  }
  // ---- C: band sums of the total downwelling and the upwelling flux ----
  const ColumnTruth ct = column_truth(a, col);
  band_sums(a, col, flux, s_bp, s_bg, s_bdn, s_bup);
  __syncthreads();
  // ---- D: the shortwave cost (calc_cost_function_sw.cpp:186-277) with the heating rate from the net flux, and its
  //      derivative with respect to the band fluxes; a second pair of arrays takes the seeds, so they are stored directly ----
  double jpart = 0.0;
  cost_residuals<true, true>(a, ct, all_pos, cost, jpart);
  for (int t = threadIdx.x; t < nhl * nband; t += blockDim.x) {
    double gd, gu;
    cost_seed<true, true>(a, ct, all_pos, cost, t, gd, gu, jpart);
    s_gdn[t] = gd;
    s_gup[t] = gu;
  }
  // the per-g (erythemal) weights act on the total downwelling flux at the surface; no term on the upwelling in the shortwave:
  // boundary_term<true> leaves up_toa_extra at 0 and nothing reads it
  double dn_surf_extra = 0.0, up_toa_extra = 0.0;
  if (live) boundary_term<true>(a, col, g, flux, jpart, dn_surf_extra, up_toa_extra);
  __syncthreads();
  // ---- E1: the reversed recurrences, one wave per 64 g points ----
  if (live) {
    const int b = band_of_g[g];
    rayleigh_adjoint_sweeps(nlay, ng, nband, s_gdn + b, s_gup + b, dn_surf_extra, alb, w + RS_R * slot, w + RS_T * slot, w + RS_TDIR * slot,
                            w + RS_RDIR * slot, w + RS_TDD * slot, w + RS_D * slot, w + RS_A * slot, w + RS_S * slot, w + RS_V * slot,
                            w + RS_AB * slot, w + RS_SB * slot, w + RS_DB * slot, w + RS_RB * slot, w + RS_TB * slot, w + RS_TDIRB * slot,
                            w + RS_RDIRB * slot, w + RS_TDDB * slot);
  }
  __syncthreads();
  // ---- E2: dJ/dtau_abs of the cells of this thread, the five terms in a fixed order ----
  double ray_bar = 0.0;                                          // RAY_ACTIVE: sum over this thread's layers of moles_l dJ/dtau_ray
  if (in_range) {
    for (int l = lgrp; l < nlay; l += nlgrp) {
      const double* wl = w + (size_t)l * ng;
      const double tau_bar = wl[RS_RB * slot] * wl[RS_DR * slot] + wl[RS_TB * slot] * wl[RS_DT * slot] +
                             wl[RS_TDIRB * slot] * wl[RS_DTDIR * slot] + wl[RS_RDIRB * slot] * wl[RS_DRDIR * slot] +
                             wl[RS_TDDB * slot] * wl[RS_DTDD * slot];
      dtau[(cell0 + l) * ng + g] += tau_bar;
      if constexpr (RAY_ACTIVE) {
        const double tau_ray_bar = wl[RS_RB * slot] * wl[(RS_RAY_D + 0) * slot] + wl[RS_TB * slot] * wl[(RS_RAY_D + 1) * slot] +
                                   wl[RS_TDIRB * slot] * wl[(RS_RAY_D + 2) * slot] + wl[RS_RDIRB * slot] * wl[(RS_RAY_D + 3) * slot] +
                                   wl[RS_TDDB * slot] * wl[(RS_RAY_D + 4) * slot];
        ray_bar += ent_coef[(cell0 + l) * nent + ray_ent] * tau_ray_bar;        // the entry's coefficient: moles of air in the layer
      }
    }
  }
  if constexpr (RAY_ACTIVE) {
    // the layer groups of a g point in group order: thread (lgrp, g) sits at lgrp * ngpad + g = threadIdx.x
    double* s_ray = (double*)((char*)smem + ray_lds_offset(layout.bytes()));      // [blockDim.x]
    s_ray[threadIdx.x] = ray_bar;
    __syncthreads();
    if (live) {
      double t = 0.0;
      for (int q = 0; q < nlgrp; ++q) t += s_ray[q * ngpad + g];
      ws[(size_t)gridDim.x * NSLOT * slot + (size_t)col * ng + g] = t;
    }
  }
  jpart += a.negative_od_penalty * penalty;
  const double jtot = block_reduce_sum(jpart, s_red);
  if (threadIdx.x == 0) a.jcol[col] = jtot;
}

// ---- K8a with the zenith-angle quadrature (ecckd_opt_create_angles, nangle > 0): the longwave transfer the line-by-line
// truth is made with (lw_angle_table of lbl_rt.hpp: sec_k = 1 / mu_k, wgt_k = 2 w_k mu_k) and its adjoint ----
// Per column, g point and angle k (levels 0 .. nlay from the top, B the Planck levels, tau after clamp and penalty):
//   t_k,l = 1 - eps_k,  eps_k = 1 - exp(-sec_k tau_l),  fac_k = eps_k > 1e-5 ? 1 - eps_k / (sec_k tau_l) : eps_k / 2
//   dn_k[0] = 0,  dn_k[l+1] = dn_k[l] t_k,l + B_l (eps_k - fac_k) + B_l+1 fac_k;   dn[i] = sum_k wgt_k dn_k[i]
//   up_k[nlay] = es B_nlay + (1 - es) dn[nlay]  (a Lambertian surface reflects the angle-summed flux: it couples the angles)
//   up_k[l] = up_k[l+1] t_k,l + B_l+1 (eps_k - fac_k) + B_l fac_k;                  up[i] = sum_k wgt_k up_k[i]
// and dn, up go the way of the two-stream kernels: band sums, the longwave cost, the seeds dnb_i, upb_i at the band of g.
// The adjoint (bars: dJ/d of the quantity):
//   ub_k[0] = wgt_k upb_0,  ub_k[l+1] = wgt_k upb_l+1 + ub_k[l] t_k,l
//   db_k[nlay] = wgt_k (dnb_nlay + (1 - es) sum_j ub_j[nlay]),  db_k[l] = wgt_k dnb_l + db_k[l+1] t_k,l
//   dJ/dtau_l = sum_k lw_tau_bar_sec(sec_k; db_k[l+1], ub_k[l], dn_k[l], up_k[l+1], B_l, B_l+1, t_k,l)   (0 in a clamped cell)
// Phases.  A (every lane owns the cells l = lgrp + j nlgrp of its g point): look-up, clamp and penalty as in the other
// longwave kernels, then per angle the one exp and, where the layer is thick, the one division of the cell and the layer's
// three terms; B1 .. B4: the dn chains, their angle sum, the up chains, their sum; C, D: band_sums, cost_residuals and
// cost_seed <longwave, net flux>; E1, E2: the reversed chains; E3 (cell owners): the sum above, one reciprocal of tau serving
// all the angles of a cell.  In the chains the layer
// groups take the ANGLES - wave group w the angles w, w + nlgrp, ... - so the nang dependent chains of FMAs run side by side;
// every sum over the angles is formed afterwards, by one thread, in angle order, so the grouping cannot change a bit of it.
// The per-angle state does not fit the LDS (5 nang + 1 arrays of (nlay + 1) ng doubles): it lives in a workspace of the
// handle, ws[column][slot][level][g], every element written and read by its own lane or with a block barrier in between.
// The LDS holds the angle-summed flux rows and the band and cost arrays (lds::lw_angles), so one kernel serves every shape.
// Slots: 0 the optical depth as the sweeps see it, the sign bit set where the cell was clamped; then per angle
enum LwaSlot { LA_T,        // rows 0 .. nlay-1: 1 - eps
               LA_DN,       // rows 1 .. nlay: the source of dn_k[l+1], then dn_k (row 0: 0)
               LA_UP,       // rows 0 .. nlay-1: the source of up_k[l], then up_k (row nlay: the surface)
               LA_UB,       // ub_k, rows 0 .. nlay
               LA_DB,       // db_k, rows 1 .. nlay
               LA_COUNT };
__host__ __device__ constexpr size_t lwa_slots(int nang) { return 1 + (size_t)LA_COUNT * nang; }

// One chain of nlay dependent FMAs x = x t[l] + src(l), l = l0, l0 + step, ...; dst(l, x) takes x BEFORE the step (the adjoint
// chains) or after it.  The rows of a chunk of layers are fetched before its FMAs start.
template <bool STORE_BEFORE, class Src, class Dst>
__device__ __forceinline__ double lwa_chain(double x, const double* __restrict__ pT, int ng, int nlay, int l0, int step, Src src, Dst dst) {
  int q0 = 0;
  for (; q0 + K8A_CH <= nlay; q0 += K8A_CH) {
    double tt[K8A_CH], ss[K8A_CH];
#pragma unroll
    for (int q = 0; q < K8A_CH; ++q) {
      const int l = l0 + (q0 + q) * step;
      tt[q] = pT[(size_t)l * ng];
      ss[q] = src(l);
    }
#pragma unroll
    for (int q = 0; q < K8A_CH; ++q) {
      const int l = l0 + (q0 + q) * step;
      if (STORE_BEFORE) dst(l, x);
      x = x * tt[q] + ss[q];
      if (!STORE_BEFORE) dst(l, x);
    }
  }
  for (; q0 < nlay; ++q0) {
    const int l = l0 + q0 * step;
    const double t = pT[(size_t)l * ng], s = src(l);
    if (STORE_BEFORE) dst(l, x);
    x = x * t + s;
    if (!STORE_BEFORE) dst(l, x);
  }
  return x;
}

__global__ void __launch_bounds__(1024)
k_opt_forward_adjoint_lw_angles(const K8aArgs a, const int* __restrict__ band_ptr /*[nband+1]*/, const int* __restrict__ band_g /*[ng]: g points by band*/,
                                int nang, const double* __restrict__ angles /*[3][nang]: sec, 1 / sec, wgt*/,
                                double* ws /*[ncol][lwa_slots(nang)][nlay+1][ng]*/) {
  extern __shared__ double smem[];
  const int nlay = a.nlay, ng = a.ng, ngpad = a.ngpad, nband = a.nband, nent = a.nent, ray_ent = a.ray_ent;
  const int nhl = nlay + 1;
  const auto layout = lds::lw_angles(nlay, ng, nband);
  auto arr = [&](int which) { return (double*)((char*)smem + layout.off[which]); };
  double* s_D = arr(lds::AL_D);                                  // [nhl][ng] dn, up summed over the angles
  double* s_U = arr(lds::AL_U);
  double* s_bdn = arr(lds::AL_BDN);                              // [nhl][nband] band fluxes
  double* s_bup = arr(lds::AL_BUP);
  double* s_gdn = arr(lds::AL_GDN);                              // [nhl][nband] dJ/d(band flux)
  double* s_gup = arr(lds::AL_GUP);
  const CostLds cost = {s_bdn, s_bup, arr(lds::AL_R), arr(lds::AL_RSUM), arr(lds::AL_SD), arr(lds::AL_SU)};
  double* s_red = arr(lds::AL_RED);                              // [16]
  int* s_bp = (int*)arr(lds::AL_BP);                             // [nband + 1]
  int* s_bg = (int*)arr(lds::AL_BG);                             // [ng]
  const double* const k = a.k; const int* const ent_idx = a.ent_idx; const double* const ent_coef = a.ent_coef;
  double* const dtau = a.dtau;
  const int col = blockIdx.x;
  const int g = threadIdx.x % ngpad;
  const int lgrp = __builtin_amdgcn_readfirstlane(threadIdx.x / ngpad);     // ngpad is a multiple of 64: uniform in a wave
  const int nlgrp = blockDim.x / ngpad;
  const bool in_range = g < ng;
  const int lane = threadIdx.x & 63;
  const int gl = in_range ? g : 0;        // lanes beyond the last g point read (and drop) the first one's values
  const double* pl = a.planck_hl + (size_t)col * nhl * ng;
  const size_t cell0 = (size_t)col * nlay;
  const size_t slot = (size_t)nhl * ng;
  double* w = ws + (size_t)col * lwa_slots(nang) * slot + gl;    // slot q of this g point: w + q * slot, rows ng apart
  auto wk = [&](int kk, int which) { return w + (1 + (size_t)LA_COUNT * kk + which) * slot; };
  const double* const sec = angles;
  const double* const rsec = angles + nang;
  const double* const wgt = angles + 2 * nang;
  for (int t = threadIdx.x; t <= nband; t += blockDim.x) s_bp[t] = band_ptr[t];
  for (int t = threadIdx.x; t < ng; t += blockDim.x) s_bg[t] = band_g[t];

  // ---- A: the cells of this thread ----
  double penalty = 0.0;
  for (int l = lgrp; l < nlay; l += nlgrp) {
    double tau = 0.0, tau_ray = 0.0;
    for (int e0 = 0; e0 < nent; e0 += 64) {
      const int ne = min(64, nent - e0);
      const int my_idx = lane < ne ? ent_idx[(cell0 + l) * nent + e0 + lane] : -1;
      const double my_c = lane < ne ? ent_coef[(cell0 + l) * nent + e0 + lane] : 0.0;
      gather_batches<0>(my_idx, my_c, e0, ne, k, gl, ray_ent, tau, tau_ray);
    }
    if (in_range) {
      bool clamped;
      tau = clamp_cell<false>(a, (cell0 + l) * ng + g, tau, tau_ray, clamped, penalty);
      tau += tau_ray;
      // (a clamped cell: -0.0, or the negative value itself where the sweeps see it, keep_negative == 2)
      w[(size_t)l * ng] = clamped ? -fabs(tau) : tau;
      const double b0 = pl[l * ng + g], b1 = pl[(l + 1) * ng + g];
      for (int kk = 0; kk < nang; ++kk) {
        // one exp and, where the layer is thick, one division per (cell, angle).  fac is a difference of two numbers near 1
        // at the thin edge (5e-6 there): a reciprocal of tau shared by the angles would cost it another rounding, 2e-11 each
        const double path = sec[kk] * tau;
        const double eps = 1.0 - ecckd::exp_fast(-path);
        const double fac = (eps > 1.0e-5) ? 1.0 - ecckd::div_fast(eps, path) : 0.5 * eps;
        wk(kk, LA_T)[(size_t)l * ng] = 1.0 - eps;
        wk(kk, LA_DN)[(size_t)(l + 1) * ng] = b0 * (eps - fac) + b1 * fac;
        wk(kk, LA_UP)[(size_t)l * ng] = b1 * (eps - fac) + b0 * fac;
      }
    }
  }
  __syncthreads();
  // ---- B1: the dn chains, one wave group per angle ----
  if (in_range)
    for (int kk = lgrp; kk < nang; kk += nlgrp) {
      double* pD = wk(kk, LA_DN);
      pD[0] = 0.0;
      lwa_chain<false>(0.0, wk(kk, LA_T), ng, nlay, 0, 1, [&](int l) { return pD[(size_t)(l + 1) * ng]; },
                       [&](int l, double x) { pD[(size_t)(l + 1) * ng] = x; });
    }
  __syncthreads();
  // ---- B2: dn summed over the angles, in angle order ----
  if (in_range)
    for (int i = lgrp; i < nhl; i += nlgrp) {
      double s = 0.0;
      for (int kk = 0; kk < nang; ++kk) s += wgt[kk] * wk(kk, LA_DN)[(size_t)i * ng];
      s_D[i * ng + g] = s;
    }
  __syncthreads();
  // ---- B3: the up chains from the Lambertian surface ----
  const double es = a.surf_emis[(size_t)col * nband + a.band_of_g[gl]];
  if (in_range)
    for (int kk = lgrp; kk < nang; kk += nlgrp) {
      double* pU = wk(kk, LA_UP);
      const double up = pl[nlay * ng + g] * es + (1.0 - es) * s_D[nlay * ng + g];
      pU[(size_t)nlay * ng] = up;
      lwa_chain<false>(up, wk(kk, LA_T), ng, nlay, nlay - 1, -1, [&](int l) { return pU[(size_t)l * ng]; },
                       [&](int l, double x) { pU[(size_t)l * ng] = x; });
    }
  __syncthreads();
  // ---- B4: up summed over the angles ----
  if (in_range)
    for (int i = lgrp; i < nhl; i += nlgrp) {
      double s = 0.0;
      for (int kk = 0; kk < nang; ++kk) s += wgt[kk] * wk(kk, LA_UP)[(size_t)i * ng];
      s_U[i * ng + g] = s;
      if (a.flux_out) {
        double* fo = a.flux_out + (size_t)col * 2 * nhl * ng;
        fo[i * ng + g] = s_D[i * ng + g];
        fo[(nhl + i) * ng + g] = s;
      }
    }
  __syncthreads();
  // ---- C: band sums of the flux rows ----
  const LdsFlux flux = {s_D, s_U, ng};
  const ColumnTruth ct = column_truth(a, col);
  band_sums(a, col, flux, s_bp, s_bg, s_bdn, s_bup);
  __syncthreads();
  // ---- D: the longwave cost (calc_cost_function_lw.cpp:186-229) and its derivative with respect to the band fluxes ----
  double jpart = 0.0;
  cost_residuals<false, true>(a, ct, true, cost, jpart);
  for (int t = threadIdx.x; t < nhl * nband; t += blockDim.x) {
    double gd, gu;
    cost_seed<false, true>(a, ct, true, cost, t, gd, gu, jpart);
    s_gdn[t] = gd;
    s_gup[t] = gu;
  }
  // the per-g boundary term: every angle owner needs its seeds, the first layer group adds its cost
  double dn_surf_extra = 0.0, up_toa_extra = 0.0;
  if (in_range) {
    double jb = 0.0;
    boundary_term<false>(a, col, g, flux, jb, dn_surf_extra, up_toa_extra);
    if (lgrp == 0) jpart += jb;
  }
  __syncthreads();
  // the per-g flux-profile term: nothing below reads the angle-summed rows s_D / s_U, so they become its seeds; every angle owner
  // adds the seed of a level where its chain loads the band seed, and scales the sum by wgt_k
  const bool gp = a.gp_truth != nullptr;
  if (gp) {
    if (in_range) jpart += gpoint_seed_rows(a, ct.lw, col, g, lgrp, nlgrp, s_gdn, s_gup, a.band_of_g[g], s_D, s_U);
    __syncthreads();
  }
  // ---- E1: the up chains reversed; row nlay of ub_k is the adjoint of up_k at the surface ----
  const int b = a.band_of_g[gl];
  if (in_range)
    for (int kk = lgrp; kk < nang; kk += nlgrp) {
      double* pB = wk(kk, LA_UB);
      const double wg = wgt[kk];
      const double ub0 = (gp ? s_U[g] : s_gup[b]) + up_toa_extra;
      const double ub = lwa_chain<true>(wg * ub0, wk(kk, LA_T), ng, nlay, 0, 1,
                                        [&](int l) {
                                          return wg * (gp ? s_U[(l + 1) * ng + g] : s_gup[(l + 1) * nband + b]);
                                        },
                                        [&](int l, double x) { pB[(size_t)l * ng] = x; });
      pB[(size_t)nlay * ng] = ub;
    }
  __syncthreads();
  // ---- E2: through the surface (the sum over ALL the angles' ub, in angle order) and the dn chains reversed ----
  if (in_range)
    for (int kk = lgrp; kk < nang; kk += nlgrp) {
      double ub_surf = 0.0;
      for (int j = 0; j < nang; ++j) ub_surf += wk(j, LA_UB)[(size_t)nlay * ng];
      double* pB = wk(kk, LA_DB);
      const double wg = wgt[kk];
      const double db0 = (gp ? s_D[nlay * ng + g] : s_gdn[nlay * nband + b]) + dn_surf_extra + (1.0 - es) * ub_surf;
      lwa_chain<true>(wg * db0, wk(kk, LA_T), ng, nlay, nlay - 1, -1,
                      [&](int l) {
                        return wg * (gp ? s_D[l * ng + g] : s_gdn[l * nband + b]);
                      },
                      [&](int l, double x) { pB[(size_t)(l + 1) * ng] = x; });
    }
  __syncthreads();
  // ---- E3: dJ/dtau of the cells of this thread, the angles in order; a clamped cell keeps the penalty's derivative ----
  if (in_range)
    for (int l = lgrp; l < nlay; l += nlgrp) {
      const double tau = w[(size_t)l * ng];
      if (__builtin_signbit(tau)) continue;
      const double b0 = pl[l * ng + g], b1 = pl[(l + 1) * ng + g];
      const double rt = ecckd::div_fast(1.0, tau);
      double tau_bar = 0.0;
      for (int kk = 0; kk < nang; ++kk)
        tau_bar += lw_tau_bar_sec(sec[kk], rsec[kk] * rt, wk(kk, LA_DB)[(size_t)(l + 1) * ng], wk(kk, LA_UB)[(size_t)l * ng],
                                  wk(kk, LA_DN)[(size_t)l * ng], wk(kk, LA_UP)[(size_t)(l + 1) * ng], b0, b1, wk(kk, LA_T)[(size_t)l * ng]);
      dtau[(cell0 + l) * ng + g] = tau_bar;
    }
  jpart += a.negative_od_penalty * penalty;
  const double jtot = block_reduce_sum(jpart, s_red);
  if (threadIdx.x == 0) a.jcol[col] = jtot;
}

// K8b + K9: gradient of the state, two launches of one WAVE per task, four waves per block, no LDS, no barrier.
//   grad_k = sum over the cells that reference this node of coef * dtau[cell][g]   (reference order)
//   grad_x = grad_k * k + B^-1 (x - x_prior) / sigma_g^2                            (:273-283)
// The nodes are referenced very unevenly (a few hundred references on average, thousands where the training profiles crowd
// one corner of the table): with a block or a wave per NODE the kernel lasted as long as its busiest node.  So the references
// of a node are cut into runs of at most K8B_RUN (host: ecckd_opt_create) and
//   k_opt_gradient_gather: a wave per (run, 64 g points) adds its run in reference order -> run_sum[run][g];
//   k_opt_gradient_finish: a wave per (node, 64 g points) adds the node's runs in order, then chain rule and prior.
// Every sum has a fixed order: bitwise reproducible.  The references come 64 at a time, one (cell, coefficient) pair per lane,
// v_readlane hands them round as scalars, and the dJ/dtau rows are loaded eight at a time, two batches in flight.
// Which wave takes which task is a pure speed choice (the order tables built by ecckd_opt_create): the blocks b, b + 8, ...
// share an XCD and walk ONE eighth of the pressure axis in order, so the dJ/dtau rows they gather (cells whose pressure lies
// between two neighbouring nodes) tend to stay in that XCD's L2.
constexpr int K8B_WAVES = 4;
constexpr int K8B_RUN = 64;
__global__ void __launch_bounds__(64 * K8B_WAVES)
k_opt_gradient_gather(int nslot, int ng, int nchunk, const int* __restrict__ run_order /*[nslot]: run * nchunk + chunk, -1 = none*/,
                      const int* __restrict__ run_r0 /*[nrun + 1]: first reference of each run*/, const int* __restrict__ run_last /*[nrun]: 1 + last reference*/,
                      const int* __restrict__ ref_cell, const double* __restrict__ ref_coef, const double* __restrict__ dtau,
                      double* __restrict__ run_sum /*[nrun][nchunk][64]*/) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int vb = blockIdx.x; vb * K8B_WAVES < nslot; vb += gridDim.x) {        // gridDim is a multiple of 8: vb stays on its XCD
    const int slot = vb * K8B_WAVES + wave;
    const int ordered = slot < nslot ? run_order[slot] : -1;
    if (ordered < 0) continue;
    const int run = ordered / nchunk;
    const int g = (ordered % nchunk) * 64 + lane;
    const int gl = g < ng ? g : 0;
    const int r0 = run_r0[run], r1 = run_last[run];
    const int myr = r0 + lane;
    const int my_cell = myr < r1 ? ref_cell[myr] : -1;
    const double my_w = myr < r1 ? ref_coef[myr] : 0.0;
    const int cnt = r1 - r0;                                   // <= K8B_RUN = 64
    double gk = 0.0;
    // the issues are unconditional (lanes past the end hold cell -1 and weight 0: row 0 is fetched and dropped), so that the
    // compiler counts the loads in flight exactly
    GatherBatch A, B;
    gather_issue(A, my_cell, my_w, 0, cnt, dtau, gl, ng);
    for (int q0 = 0; q0 < cnt; q0 += 2 * K8A_GB) {
      gather_issue(B, my_cell, my_w, (q0 + K8A_GB) & 63, cnt, dtau, gl, ng);
#pragma unroll
      for (int q = 0; q < K8A_GB; ++q) gk += A.ix[q] >= 0 ? A.cv[q] * A.kv[q] : 0.0;
      gather_issue(A, my_cell, my_w, (q0 + 2 * K8A_GB) & 63, cnt, dtau, gl, ng);
      const bool use_b = q0 + K8A_GB < cnt;                    // (at q0 + 8 = 64 the issue above wrapped round to batch 0)
#pragma unroll
      for (int q = 0; q < K8A_GB; ++q) gk += (use_b && B.ix[q] >= 0) ? B.cv[q] * B.kv[q] : 0.0;
    }
    run_sum[(size_t)ordered * 64 + lane] = gk;
  }
}

__global__ void __launch_bounds__(64 * K8B_WAVES)
k_opt_gradient_finish(int nslot /*entries of node_order*/, int ng, int nchunk /*64-g chunks per node*/, const double* __restrict__ x,
                      const double* __restrict__ x_prior, const double* __restrict__ k,
                      const int* __restrict__ node_run0 /*[nnode + 1]: first run of each node*/, const double* __restrict__ run_sum,
                      // prior: per node the (at most 27) neighbours of its Kronecker stencil and their weights, -1 = none
                      const int* __restrict__ node_gas, const int* __restrict__ st_nb /*[nnode][27]*/,
                      const double* __restrict__ st_w /*[nnode][27]*/, const double* __restrict__ inv_sigma2 /*[ngas][ng]*/,
                      int have_prior, double* __restrict__ grad, double* __restrict__ jb_part /*[nnode][nchunk]*/,
                      const int* __restrict__ node_order /*[nslot]: node * nchunk + chunk of each wave, -1 = none*/) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  for (int vb = blockIdx.x; vb * K8B_WAVES < nslot; vb += gridDim.x) {
    const int slot = vb * K8B_WAVES + wave;
    const int ordered = slot < nslot ? node_order[slot] : -1;
    if (ordered < 0) continue;
    const size_t node = (size_t)(ordered / nchunk);
    const int chunk = ordered % nchunk;
    const int g = chunk * 64 + lane;
    const bool active = g < ng;
    const int gl = active ? g : 0;
    // the node's runs, in order (eight loads in flight)
    double gk = 0.0;
    const int t1 = node_run0[node + 1];
    for (int t = node_run0[node]; t < t1; t += 8) {
      double v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = run_sum[((size_t)min(t + q, t1 - 1) * nchunk + chunk) * 64 + lane];
#pragma unroll
      for (int q = 0; q < 8; ++q) gk += (t + q < t1) ? v[q] : 0.0;
    }
    // B^-1 (x - x_prior) / sigma_g^2 at this node (calc_background_cost_function, ckd_model.cpp:852-865): the stencil's
    // neighbours come one per lane and go round as scalars, their 2 x 27 loads are in flight together, the terms are added in
    // the order of the host's loops (concentration, temperature, pressure offsets -1, 0, 1)
    double gb = 0.0;
    if (have_prior) {
      const int my_nb = lane < 27 ? st_nb[node * 27 + lane] : -1;
      const double my_w = lane < 27 ? st_w[node * 27 + lane] : 0.0;
      double acc = 0.0;
#pragma unroll
      for (int q0 = 0; q0 < 27; q0 += 9) {
        int nb[9];
        double w[9], xa[9], xb[9];
#pragma unroll
        for (int q = 0; q < 9; ++q) { nb[q] = __builtin_amdgcn_readlane(my_nb, q0 + q); w[q] = readlane_f64(my_w, q0 + q); }
#pragma unroll
        for (int q = 0; q < 9; ++q) {
          xa[q] = x[(size_t)max(nb[q], 0) * ng + gl];
          xb[q] = x_prior[(size_t)max(nb[q], 0) * ng + gl];
        }
#pragma unroll
        for (int q = 0; q < 9; ++q) acc += nb[q] >= 0 ? w[q] * (xa[q] - xb[q]) : 0.0;
      }
      if (active) gb = acc * inv_sigma2[(size_t)node_gas[node] * ng + g];
    }
    double jb = 0.0;
    if (active) {
      const size_t e = node * ng + g;
      const double xv = x[e];
      double gx = 0.0;
      if (xv > MIN_X) {
        gx = gk * k[e];
        if (have_prior) {
          gx += gb;
          jb = 0.5 * (xv - x_prior[e]) * gb;
        }
        if (fabs(gx) < 1.0e-80) gx = 0.0;  // :286
      }
      grad[e] = gx;
    }
    // the node's share of the background cost: lanes in shuffle order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) jb += __shfl_down(jb, off, 64);
    if (lane == 0) jb_part[ordered] = jb;
  }
}

// ---- the ng gradient elements of the optimised Rayleigh coefficients (ECCKD_OPT_RAYLEIGH_ACTIVE) ----
//   dJ/dk_ray[g] = sum over the rows r of wgt[r] * src[r][g]
// plain handle: rows = cells, src = dJ/dtau as the K8a kernels leave it (Rayleigh is one more absorber before the clamp, so a
// clamped cell's penalty derivative counts), wgt = moles of air of the cell; scattering handle: rows = columns, src = what
// k_opt_forward_adjoint_rayleigh<true> leaves per (column, g), no weights.  Two launches, every sum in a fixed order, no atomics:
//   k_opt_rayleigh_reduce: a wave per (RAY_CHUNK consecutive rows, 64 g points) adds its rows in row order - whole 512-byte
//     rows at ng = 64, RAY_BATCH loads in flight, the weights one per lane and handed round as scalars -> part[chunk][g];
//   k_opt_rayleigh_finish: a block of RAY_FIN_WAVES waves per 64 g points; wave w adds the partials [w per, (w + 1) per) in
//     order, per = ceil(npart / RAY_FIN_WAVES), RAY_BATCH loads in flight per round; wave 0 adds the waves' sums in wave order,
//     then per element: chain rule x = ln k, the prior d / sigma^2 (d = x - x_prior), 0 for a pinned element, the 1e-80 rule
//     (solve_adept.cpp:286), and the chunk's share 0.5 sum d^2 / sigma^2 of J_b into its slot behind the nodes' shares, where
//     k_opt_sum_cost finds it.
// About 1 000 partials at 64 000 cells: 63 per finishing wave, 8 rounds of 8 loads - not 1 000 in a row on one wave.
// Both levels add in double-double (two_sum: the rounding error of every addition is kept in a second word, which travels with
// the partials), so the sum of the rows is the correctly rounded one but for ties: a scene whose columns are repeated K = 2^n
// times gives K times the gradient of the scene itself, which a plain sum of 10^4 rows misses by several units in the last
// place (tests/test_optimize_rayleigh_active_gpu.py::test_many_rows).  The kernels are bound by their loads; the extra five
// additions per row do not show.
// two_sum is exact only in IEEE arithmetic as written: under -ffast-math (or any option that lets the compiler reassociate) the
// error word (hi - (s - b)) + (v - b) folds to 0 and the sums silently fall back to plain ones.  The build does not enable it
// (HIP_COMPILE_FLAGS of __graft_entry__.py, HIPFLAGS of the Makefile); a build that does is refused here.
#if defined(__FAST_MATH__) || defined(__ASSOCIATIVE_MATH__)
#error "optimize.hip: two_sum needs IEEE floating-point arithmetic without reassociation (no -ffast-math)"
#endif
__device__ __forceinline__ void two_sum(double& hi, double& lo, double v) {
  const double s = hi + v;
  const double b = s - hi;
  lo += (hi - (s - b)) + (v - b);
  hi = s;
}
constexpr int RAY_CHUNK = 64;        // rows per first-level wave
constexpr int RAY_FIN_WAVES = 16;    // waves of the finishing block
constexpr int RAY_BATCH = 8;         // loads in flight per wave
constexpr int RAY_RED_WAVES = 4;     // waves per block of the first level

__global__ void __launch_bounds__(64 * RAY_RED_WAVES)
k_opt_rayleigh_reduce(size_t nrows, int ng, int nchunk /*64-g chunks of a row*/, const double* __restrict__ src /*[nrows][ng]*/,
                      const double* __restrict__ wgt /*[nrows] or NULL = 1*/, double* __restrict__ part /*[2: sum, error word][ceil(nrows / RAY_CHUNK)][nchunk][64]*/) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const size_t ntask = (nrows + RAY_CHUNK - 1) / RAY_CHUNK * nchunk;
  const size_t task = (size_t)blockIdx.x * RAY_RED_WAVES + wave;
  if (task >= ntask) return;
  const size_t rc = task / nchunk;
  const int g = (int)(task % nchunk) * 64 + lane;
  const int gl = g < ng ? g : 0;                           // lanes beyond the last g point read (and their sums are never read) the first one's
  const size_t r0 = rc * RAY_CHUNK;
  const int cnt = (int)min((size_t)RAY_CHUNK, nrows - r0);   // >= 1
  const double my_w = lane < cnt ? (wgt ? wgt[r0 + lane] : 1.0) : 0.0;
  double acc = 0.0, err = 0.0;
  for (int q0 = 0; q0 < cnt; q0 += RAY_BATCH) {
    double v[RAY_BATCH], w[RAY_BATCH];
#pragma unroll
    for (int q = 0; q < RAY_BATCH; ++q) {
      v[q] = src[(r0 + min(q0 + q, cnt - 1)) * ng + gl];  // past the end: the last row again, dropped below
      w[q] = readlane_f64(my_w, (q0 + q) & 63);
    }
#pragma unroll
    for (int q = 0; q < RAY_BATCH; ++q) {
      double term;
      {
#pragma clang fp contract(off)       // the term is rounded once, before two_sum: fused into its first addition it would be two numbers
        term = w[q] * v[q];
      }
      two_sum(acc, err, q0 + q < cnt ? term : 0.0);
    }
  }
  part[task * 64 + lane] = acc;
  part[(ntask + task) * 64 + lane] = err;
}

__global__ void __launch_bounds__(64 * RAY_FIN_WAVES)
k_opt_rayleigh_finish(size_t npart, int ng, int nchunk, const double* __restrict__ part /*[2][npart][nchunk][64]*/, size_t e0 /*first Rayleigh element of x, k, grad*/,
                      const double* __restrict__ x, const double* __restrict__ x_prior, const double* __restrict__ k,
                      double inv_sigma2, int have_prior, double* __restrict__ grad, double* __restrict__ jb_part /*[nchunk]*/) {
  __shared__ double s_sum[2][RAY_FIN_WAVES][64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int chunk = blockIdx.x;
  const size_t per = (npart + RAY_FIN_WAVES - 1) / RAY_FIN_WAVES;
  const size_t p0 = min(npart, wave * per), p1 = min(npart, p0 + per);
  const double* part_err = part + npart * nchunk * 64;
  double acc = 0.0, err = 0.0;
  for (size_t t = p0; t < p1; t += RAY_BATCH) {
    double v[RAY_BATCH], ve[RAY_BATCH];
#pragma unroll
    for (int q = 0; q < RAY_BATCH; ++q) {
      const size_t at = (min(t + q, p1 - 1) * nchunk + chunk) * 64 + lane;
      v[q] = part[at];
      ve[q] = part_err[at];
    }
#pragma unroll
    for (int q = 0; q < RAY_BATCH; ++q) {
      two_sum(acc, err, t + q < p1 ? v[q] : 0.0);
      err += t + q < p1 ? ve[q] : 0.0;
    }
  }
  s_sum[0][wave][lane] = acc;
  s_sum[1][wave][lane] = err;
  __syncthreads();
  if (wave != 0) return;
  double gk_hi = 0.0, gk_lo = 0.0;
#pragma unroll
  for (int w = 0; w < RAY_FIN_WAVES; ++w) {
    two_sum(gk_hi, gk_lo, s_sum[0][w][lane]);
    gk_lo += s_sum[1][w][lane];
  }
  const double gk = gk_hi + gk_lo;
  const int g = chunk * 64 + lane;
  double jb = 0.0;
  if (g < ng) {
    const size_t e = e0 + g;
    const double xv = x[e];
    double gx = 0.0;
    if (xv > MIN_X) {
      gx = gk * k[e];                                            // dJ/dx = dJ/dk * k (:276-283)
      if (have_prior) {
        const double d = xv - x_prior[e];
        const double gb = d * inv_sigma2;
        gx += gb;
        jb = 0.5 * d * gb;
      }
      if (fabs(gx) < 1.0e-80) gx = 0.0;  // :286
    }
    grad[e] = gx;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) jb += __shfl_down(jb, off, 64);
  if (lane == 0) jb_part[chunk] = jb;
}

// k = exp(x) for the active part (:242-249)
__global__ void __launch_bounds__(256)
k_opt_exp(size_t nx, const double* __restrict__ x, double* __restrict__ k) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < nx) k[e] = (x[e] > MIN_X) ? exp(x[e]) : 0.0;
}


// ---------------------------------------------------------------------------------------
// Device-resident L-BFGS vector kernels.  All reductions are two-stage with a fixed order:
// stage 1 writes one partial per block (lanes by shuffle, then the block's waves in order), stage 2 (inside the consumer
// kernel, or k_lb_finish) sums the partials in index order.
constexpr int VEC_BLOCKS = 512;    // room for partials per reduction; the launches use min(512, ceil(n / 1024)) blocks
constexpr int VEC_THREADS = 1024;  // ONE element per thread at nx ~ 3e5: every load of a pass is in flight at once
constexpr int VEC_WAVES = VEC_THREADS / 64;
constexpr int FIN_THREADS = 256;   // k_lb_finish

using ecckd::wave_sum;   // rt_device.hpp

// the nblk (<= 512) partials of one reduction, summed by every caller in the same order (blockDim >= 256)
__device__ __forceinline__ double sum_partials(const double* __restrict__ part, int nblk, double* s_tmp /*[4]*/) {
  const int t = threadIdx.x;
  double v = 0.0;
  if (t < 256) {
    if (t < nblk) v = part[t];
    if (t + 256 < nblk) v += part[t + 256];
  }
  v = wave_sum(v);
  __syncthreads();
  if ((t & 63) == 0 && t < 256) s_tmp[t >> 6] = v;
  __syncthreads();
  return ((s_tmp[0] + s_tmp[1]) + s_tmp[2]) + s_tmp[3];
}

// NACC per-thread accumulators -> one partial per (accumulator, block).  Within a wave the NACC sums are taken TOGETHER
// (fold_wave, rt_device.hpp: the plain form, six exchanges per value, cost the update kernel more than its memory traffic);
// lane l ends up with the wave's sum of accumulator bitreverse6(l).
template <int NACC>
__device__ __forceinline__ void write_partials(double (&acc)[NACC], int nused, double* __restrict__ part, double* s_all /*[NACC][VEC_WAVES]*/) {
  static_assert(NACC <= 64, "one value per lane at the end");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the levels of fold_wave (rt_device.hpp) written out: through fold_wave itself the compiler orders k_lb_update and
  // k_lb_direction differently, and their code stays what was measured
  constexpr int U1 = (NACC + 1) / 2, U2 = (U1 + 1) / 2, U3 = (U2 + 1) / 2, U4 = (U3 + 1) / 2, U5 = (U4 + 1) / 2;
  auto add = [](double a, double b) { return a + b; };
  ecckd::fold_level<NACC, true>(acc, (lane & 32) != 0, 32, add);
  ecckd::fold_level<U1, true>(acc, (lane & 16) != 0, 16, add);
  ecckd::fold_level<U2, true>(acc, (lane & 8) != 0, 8, add);
  ecckd::fold_level<U3, true>(acc, (lane & 4) != 0, 4, add);
  ecckd::fold_level<U4, true>(acc, (lane & 2) != 0, 2, add);
  ecckd::fold_level<U5, true>(acc, (lane & 1) != 0, 1, add);
  const int kk = (int)(__brev((unsigned)lane) >> 26);           // the accumulator this lane now holds
  if (kk < NACC) s_all[kk * VEC_WAVES + wave] = acc[0];
  __syncthreads();
  if ((int)threadIdx.x < nused) {
    double t = 0.0;
    for (int w = 0; w < VEC_WAVES; ++w) t += s_all[threadIdx.x * VEC_WAVES + w];
    part[(size_t)threadIdx.x * VEC_BLOCKS + blockIdx.x] = t;
  }
}

// ---- L-BFGS on the device, compact representation (Byrd, Nocedal & Schnabel 1994) -----------------------------
// With S = [s_0 .. s_{m-1}], Y = [y_0 .. y_{m-1}] (oldest first), R = upper triangle of S^T Y, D = diag(s_i.y_i):
//   H g = gamma g + S top - gamma Y u,   u = R^-1 (S^T g),   top = R^-T ((D + gamma Y^T Y) u - gamma Y^T g)
// which is the two-loop recursion in matrix form.  Per iteration: ONE pass that stores the new curvature pair and takes
// every dot product the update needs (k_lb_update), the m x m solves on the host, the direction in one more pass
// (k_lb_direction), the trial point and its coefficients exp(x) (k_lb_step): three vector launches and two waits of the host
// on pinned result slots (the dots; the cost of the trial point).
constexpr int LB_M = 6;
struct LbSlots { int n; int slot[LB_M]; };                       // ring slots of the pairs, oldest first
struct LbCoef { double gamma; double cs[LB_M]; double cy[LB_M]; };
constexpr int LB_NPART = 3 + 5 * LB_M;

// The accepted step x -> xn, g -> gn (new_slot >= 0): curvature pair s = xn - x, y = gn - g into its ring slot, and its dots
// with the pairs that stay (keep): partials [1+2M] s.y, [2+2M] y.y, [3+2M+a] s.Y_a, [3+3M+a] S_a.y, [3+4M+a] y.Y_a.
// Then, at the new point: q = projected gradient (0 at active bounds and at pinned elements) and partials [0] |q|^2,
// [1+a] S_a.q, [1+M+a] Y_a.q for the pairs that stay and, as the newest (a = keep.n), the pair just stored.
// new_slot < 0 (first iteration): only q and |q|^2 at (xn, gn).
__global__ void __launch_bounds__(VEC_THREADS)
k_lb_update(size_t n, LbSlots keep, int new_slot, const double* __restrict__ x, const double* __restrict__ xn,
            const double* __restrict__ g, const double* __restrict__ gn, const double* __restrict__ xmin,
            const double* __restrict__ xmax, double* __restrict__ q, double* __restrict__ S, double* __restrict__ Y,
            double* __restrict__ part) {
  __shared__ double s_all[LB_NPART * VEC_WAVES];
  double acc[LB_NPART];
#pragma unroll
  for (int k = 0; k < LB_NPART; ++k) acc[k] = 0.0;
  const bool pair = new_slot >= 0;
  for (size_t i = (size_t)blockIdx.x * VEC_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * VEC_THREADS) {
    // every load of the element first, none behind a test of the number of pairs (a branch per pair put a full memory round
    // trip behind each): the slots of unused pairs hold zeros or the finite values of dropped pairs (S and Y are cleared when
    // they are allocated), their partials are never read
    double sa[LB_M], ya[LB_M];
#pragma unroll
    for (int a = 0; a < LB_M; ++a) {
      sa[a] = S[(size_t)keep.slot[a] * n + i];
      ya[a] = Y[(size_t)keep.slot[a] * n + i];
    }
    const double xi = xn[i];
    double gi = gn[i];
    const double xo = x[i], go = g[i];
    const double lo = xmin ? xmin[i] : 0.0, hi = xmin ? xmax[i] : 0.0;
    const double si = pair ? xi - xo : 0.0, yi = pair ? gi - go : 0.0;
    if (xmin && ((xi <= lo && gi > 0.0) || (xi >= hi && gi < 0.0))) gi = 0.0;
    if (!(xi > MIN_X)) gi = 0.0;
    q[i] = gi;
    acc[0] += gi * gi;
    acc[1 + 2 * LB_M] += si * yi;
    acc[2 + 2 * LB_M] += yi * yi;
#pragma unroll
    for (int a = 0; a < LB_M; ++a) {
      // position keep.n is the pair being stored: the newest of this iteration's direction
      const double sq = (a == keep.n && pair) ? si : sa[a];
      const double yq = (a == keep.n && pair) ? yi : ya[a];
      // (positions behind the pairs in use alias ring slot 0: dropped by a select, never multiplied)
      const bool used = a < keep.n || (a == keep.n && pair);
      acc[1 + a] += used ? sq * gi : 0.0;
      acc[1 + LB_M + a] += used ? yq * gi : 0.0;
      acc[3 + 2 * LB_M + a] += a < keep.n ? si * ya[a] : 0.0;
      acc[3 + 3 * LB_M + a] += a < keep.n ? sa[a] * yi : 0.0;
      acc[3 + 4 * LB_M + a] += a < keep.n ? yi * ya[a] : 0.0;
    }
    if (pair) {
      S[(size_t)new_slot * n + i] = si;     // the slot being written is never among the pairs that stay
      Y[(size_t)new_slot * n + i] = yi;
    }
  }
  write_partials<LB_NPART>(acc, LB_NPART, part, s_all);
}

// d = -gamma q - sum cs_a S_a + sum cy_a Y_a; partials of d.g and d.d
__global__ void __launch_bounds__(VEC_THREADS)
k_lb_direction(size_t n, LbSlots sl, LbCoef cf, const double* __restrict__ q, const double* __restrict__ S,
               const double* __restrict__ Y, const double* __restrict__ g, double* __restrict__ d,
               double* __restrict__ part_dg /* part_dd follows: [2][VEC_BLOCKS] */) {
  __shared__ double s_all[2 * VEC_WAVES];
  double acc[2] = {0.0, 0.0};
  for (size_t i = (size_t)blockIdx.x * VEC_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * VEC_THREADS) {
    // (no test of the number of pairs round the LOADS - a branch per pair put a memory round trip behind each -; an unused
    // position, which aliases ring slot 0, is dropped by a select: 0 x a stale non-finite value would be NaN)
    double sv[LB_M], yv[LB_M];
#pragma unroll
    for (int k = 0; k < LB_M; ++k) {
      sv[k] = S[(size_t)sl.slot[k] * n + i];
      yv[k] = Y[(size_t)sl.slot[k] * n + i];
    }
    double di = -cf.gamma * q[i];
#pragma unroll
    for (int k = 0; k < LB_M; ++k) di += (k < sl.n) ? cf.cy[k] * yv[k] - cf.cs[k] * sv[k] : 0.0;
    // a variable held by an active bound (or pinned) does not move: without this the slope d.g of the Armijo test would
    // count a decrease that the clamped trial point cannot deliver
    if (q[i] == 0.0 && g[i] != 0.0) di = 0.0;
    d[i] = di;
    acc[0] += di * g[i];
    acc[1] += di * di;
  }
  write_partials<2>(acc, 2, part_dg, s_all);
}

// xn = clamp(x + step*d), pinned elements stay; kn = exp(xn), the coefficients the cost function starts from (0 where pinned,
// solve_adept.cpp:242-249).  step < 0: chosen here from |d| (every block reduces the same partials in the same order):
// first iteration min(1, 1/|d|), later 1, never longer than max_step (solve_adept.cpp:331), times `hint`; out[0] = step, out[1] = d.d,
// out[2] = d.g (pinned host slots)
__global__ void __launch_bounds__(VEC_THREADS)
k_lb_step(size_t n, double step, int first, double max_step, double hint, const double* __restrict__ part_dg,
          const double* __restrict__ part_dd, const double* __restrict__ x, const double* __restrict__ d,
          const double* __restrict__ xmin, const double* __restrict__ xmax, double* __restrict__ xn,
          double* __restrict__ kn, double* __restrict__ out) {
  __shared__ double s_tmp[4];
  if (step < 0.0) {
    const double dd = sum_partials(part_dd, gridDim.x, s_tmp);
    const double dn = sqrt(dd);
    step = first ? fmin(1.0, 1.0 / fmax(dn, 1e-300)) : 1.0;
    if (step * dn > max_step) step = max_step / dn;
    step *= hint;             // the fraction of that step the line search starts from (ecckd_opt_minimize)
    if (blockIdx.x == 0) {
      const double dg = sum_partials(part_dg, gridDim.x, s_tmp);
      if (threadIdx.x == 0) { out[0] = step; out[1] = dd; out[2] = dg; }
    }
  }
  for (size_t i = (size_t)blockIdx.x * VEC_THREADS + threadIdx.x; i < n; i += (size_t)gridDim.x * VEC_THREADS) {
    double v = x[i] + step * d[i];
    if (xmin) v = fmin(fmax(v, xmin[i]), xmax[i]);
    const bool free_el = x[i] > MIN_X;
    if (!free_el) v = x[i];
    xn[i] = v;
    kn[i] = free_el ? exp(v) : 0.0;
  }
}

// out[k] = sum of partial array k: one block per array.  `out` is pinned, host-coherent memory: the host watches the slots
// (no copy, no stream synchronisation; see wait_slots)
__global__ void __launch_bounds__(FIN_THREADS)
k_lb_finish(const double* __restrict__ part, int nblk, double* __restrict__ out) {
  __shared__ double s_tmp[4];
  const int k = blockIdx.x;
  const double v = sum_partials(part + (size_t)k * VEC_BLOCKS, nblk, s_tmp);
  if (threadIdx.x == 0) out[k] = v;
}

// The cost of an evaluation: the profiles' costs, then the prior's node terms, each summed in a fixed order (thread t takes
// the elements t, t + 256, ...; the block combines in thread order), delivered to the host's slot and, for the profile-sharded
// all-reduce, into the slot behind the gradient.
__global__ void __launch_bounds__(256)
k_opt_sum_cost(const double* __restrict__ jcol, size_t ncol, const double* __restrict__ jb, size_t nnode, int prior,
               double* __restrict__ h_out /*pinned*/, double* __restrict__ d_out /*or NULL*/) {
  __shared__ double s_tmp[4];
  double a = 0.0, b = 0.0;
  // a thread's elements are loaded together (one memory round trip instead of one per element: the kernel is a single block
  // whose time is its chain of loads) and added in the order they always were
  constexpr int U = 8;
  for (size_t i0 = threadIdx.x; i0 < ncol; i0 += (size_t)256 * U) {
    double v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) { const size_t i = i0 + (size_t)256 * u; v[u] = jcol[i < ncol ? i : ncol - 1]; }
#pragma unroll
    for (int u = 0; u < U; ++u) if (i0 + (size_t)256 * u < ncol) a += v[u];
  }
  if (prior && nnode > 0)
    for (size_t i0 = threadIdx.x; i0 < nnode; i0 += (size_t)256 * U) {
      double v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) { const size_t i = i0 + (size_t)256 * u; v[u] = jb[i < nnode ? i : nnode - 1]; }
#pragma unroll
      for (int u = 0; u < U; ++u) if (i0 + (size_t)256 * u < nnode) b += v[u];
    }
  double r[2] = {a, b};
  double tot[2];
  for (int k = 0; k < 2; ++k) {
    double v = r[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
    __syncthreads();
    tot[k] = ((s_tmp[0] + s_tmp[1]) + s_tmp[2]) + s_tmp[3];
  }
  if (threadIdx.x == 0) {
    const double J = tot[0] + tot[1];
    if (d_out) *d_out = J;
    *h_out = J;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------
// The host side.  The tables a handle uploads are built by opt_tables.cpp, the L-BFGS history is lbfgs_history.hpp; here:
// the handle and its memory, the launches, and the entry points.
#include "lbfgs_history.hpp"
#include "opt_tables.hpp"

#include <memory>
#include <string>

namespace ot = ecckd::opt_tables;

static_assert(ot::MIN_X == MIN_X && ot::ACCEL_GRAVITY == ECCKD_ACCEL_GRAVITY && ot::SPECIFIC_HEAT_AIR == ECCKD_SPECIFIC_HEAT_AIR,
              "opt_tables.hpp repeats these constants");
static_assert(ecckd::LbfgsHistory::M == LB_M, "lbfgs_history.hpp repeats the number of pairs");

// Pinned, host-coherent result slots that the kernels write and the host watches (pageable read-backs cost ~30 us each through
// the runtime's staging path): the L-BFGS dot products (LB_NPART of them), then step / d.d / d.g of a trial point, the cost of
// an evaluation, and the all-reduced cost.
constexpr int PIN_LB_DOTS = 0, PIN_LB_STEP = 64, PIN_COST = 70, PIN_REDUCED_COST = 71, PIN_SLOTS = 80;
static_assert(PIN_LB_DOTS + LB_NPART <= PIN_LB_STEP, "the dot products overlap the step slots");

struct ecckd_opt : ot::Layout {
  ecckd_ctx* ctx = nullptr;
  ecckd_opt_config cfg{};
  // evaluation mode of the forward kernel, set for the length of a diagnostic pass only (opt_diagnostic_pass)
  int eval_ray_ent = -1;   // >= 0: entry of the Rayleigh term, added after the clamp (ecckd_run_ckd)
  int eval_keep_negative = 0;
  double* d_od_out = nullptr; double* d_flux_out = nullptr;   // non-NULL marks a diagnostic pass
  // Every other device block of the handle comes from alloc(), which records it; opt_free releases what is recorded.  The
  // named members below are views for the launch sites.
  std::vector<void*> blocks;
  template <typename T> hipError_t alloc(T** p, size_t count) {
    void* v = nullptr;
    const hipError_t e = hipMalloc(&v, std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) blocks.push_back(v);
    *p = (T*)v;
    return e;
  }
  // frees a block that alloc() recorded and forgets it
  template <typename T> void release(T** p) {
    if (!*p) return;
    blocks.erase(std::remove(blocks.begin(), blocks.end(), (void*)*p), blocks.end());
    (void)hipFree(*p);
    *p = nullptr;
  }
  double* d_rel = nullptr;   // relative-to CKD fluxes [ncol][2][nhl][ng]
  // ecckd_opt_set_gpoint_truth: the per-g flux truth [ncol][2][nhl][ng] (the layout of d_rel) and its weight; NULL / 0: no such term
  double* d_gp_truth = nullptr;
  double gp_weight = 0.0;
  double* d_ray_ws = nullptr;   // scattering handles: the per-(level, g) state of k_opt_forward_adjoint_rayleigh [ncol][RS_COUNT][nhl][ng]
  double* d_mu0 = nullptr;
  // ecckd_opt_create_angles with nangle > 0: the longwave forward model is the zenith-angle quadrature; [3][nangle] sec, 1 / sec,
  // wgt of lw_angle_table, and the per-angle state of k_opt_forward_adjoint_lw_angles [ncol][lwa_slots(nangle)][nhl][ng]
  int nangle = 0;
  double* d_lw_angles = nullptr;
  double* d_lwa_ws = nullptr;
  // ECCKD_OPT_RAYLEIGH_ACTIVE: the cells' moles of air (plain handle: the weights of dJ/dtau), the first-level partials of the
  // Rayleigh reduction, and the prior error of the ng tail elements (<= 0: no prior term on them)
  double* d_moles = nullptr;
  double* d_ray_part = nullptr;
  double* d_ray_exp = nullptr;          // [2][ng] ecckd_opt_rayleigh_coefficients: the state's tail and its exp
  double ray_prior_error = 0.0;
  double *d_k = nullptr, *d_x = nullptr, *d_xprior = nullptr, *d_grad = nullptr, *d_dtau = nullptr;
  double *d_jcol = nullptr, *d_jb = nullptr;
  int* d_ent_idx = nullptr; double* d_ent_coef = nullptr; int* d_band = nullptr;
  int *d_band_ptr = nullptr, *d_band_g = nullptr;   // the g points of each band in increasing order (CSR)
  int* d_node_order = nullptr;                      // K8b finish: wave slot -> node * nchunk + chunk (XCD-aware), -1 = idle
  int *d_run_order = nullptr, *d_run_r0 = nullptr, *d_run_last = nullptr, *d_node_run0 = nullptr;   // K8b gather: the runs
  double* d_run_sum = nullptr;                      // [nrun][nchunk][64]
  unsigned gradient_grid = 0, gather_grid = 0;
  int grad_nslot = 0, gather_nslot = 0;
  size_t grad_nrun = 0;
  double *d_planck = nullptr, *d_semis = nullptr, *d_conv = nullptr, *d_lw = nullptr;
  double *d_hr = nullptr, *d_fdn = nullptr, *d_fup = nullptr, *d_sfds = nullptr, *d_sfut = nullptr;
  int *d_ref_ptr = nullptr, *d_ref_cell = nullptr; double* d_ref_coef = nullptr;
  int *d_node_gas = nullptr, *d_st_nb = nullptr;    // K9: gas of each active node, its stencil's neighbours [nnode][27]
  double *d_st_w = nullptr, *d_inv_sigma2 = nullptr;
  unsigned grad_blocks = 0;
  double* h_pin = nullptr;    // the PIN_SLOTS pinned slots
  double* d_pin = nullptr;    // the same memory as the device sees it
  // device L-BFGS workspace (allocated by ecckd_opt_minimize)
  double *d_xmin = nullptr, *d_xmax = nullptr, *d_xn = nullptr, *d_gn = nullptr, *d_dir = nullptr, *d_q = nullptr;
  double *d_S = nullptr, *d_Y = nullptr, *d_part = nullptr;
  // profile-sharded optimisation: sum of [gradient, J] over the ranks (ecckd_opt_set_allreduce)
  ecckd_allreduce_fn reduce_fn = nullptr;
  void* reduce_user = nullptr;
  bool add_prior = true;     // exactly one rank contributes the prior term
  // timing
  long long n_eval = 0;
  // progress line and activity timers of solve_adept.cpp (:216-218 "minimizer", "a-priori", "radiative transfer"; :295-299)
  ecckd_evaluator_fn eval_fn = nullptr;    // cost / gradient supplied by the caller instead of the device kernels
  void* eval_user = nullptr;
  std::vector<double> eval_x, eval_g;
  ecckd_progress_fn progress_fn = nullptr;
  void* progress_user = nullptr;
  hipEvent_t tev[3] = {nullptr, nullptr, nullptr};
  double t_rt = 0.0, t_prior = 0.0, t_minimizer = 0.0;
};

namespace {

void opt_free(ecckd_opt* o) {
  if (!o) return;
  if (o->ctx) (void)hipStreamSynchronize(o->ctx->stream);
  for (void* p : o->blocks) (void)hipFree(p);
  if (o->d_od_out) (void)hipFree(o->d_od_out);
  if (o->d_flux_out) (void)hipFree(o->d_flux_out);
  if (o->h_pin) (void)hipHostFree(o->h_pin);
  for (hipEvent_t e : o->tev)
    if (e) (void)hipEventDestroy(e);
  delete o;
}

// a handle under construction: every early return frees it
struct OptDelete { void operator()(ecckd_opt* o) const { opt_free(o); } };
using OptPtr = std::unique_ptr<ecckd_opt, OptDelete>;

// (the sources are pageable vectors: the copy has left them when the stream has drained)
template <typename T>
int upload(ecckd_opt* o, T** d, const std::vector<T>& h) {
  ECCKD_HIP_CHECK(o->alloc(d, h.size()));
  if (!h.empty())
    ECCKD_HIP_CHECK(hipMemcpyAsync(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, o->ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(o->ctx->stream));
  return ECCKD_OK;
}

int opt_upload_tables(ecckd_opt* o, const ot::Tables& t) {
  int rc = ECCKD_OK;
  auto up = [&](auto** d, const auto& h) { if (rc == ECCKD_OK) rc = upload(o, d, h); };
  up(&o->d_k, o->k0);
  up(&o->d_ent_idx, t.ent_idx); up(&o->d_ent_coef, t.ent_coef); up(&o->d_band, t.band); up(&o->d_band_ptr, t.band_ptr); up(&o->d_band_g, t.band_g);
  up(&o->d_planck, t.planck); up(&o->d_semis, t.semis); up(&o->d_conv, t.conv); up(&o->d_lw, t.lw);
  up(&o->d_hr, t.hr); up(&o->d_fdn, t.fdn); up(&o->d_fup, t.fup);
  if (o->have_boundary) { up(&o->d_sfds, t.sfds); up(&o->d_sfut, t.sfut); }
  if (o->do_sw) up(&o->d_mu0, t.mu0);
  if (o->rayleigh_active && !o->scattering) up(&o->d_moles, t.moles);
  if (!t.rel.empty()) up(&o->d_rel, t.rel);
  up(&o->d_ref_ptr, t.ref_ptr); up(&o->d_ref_cell, t.ref_cell); up(&o->d_ref_coef, t.ref_coef); up(&o->d_node_order, t.node_order);
  up(&o->d_run_order, t.run_order); up(&o->d_run_r0, t.run_r0); up(&o->d_run_last, t.run_last); up(&o->d_node_run0, t.node_run0);
  up(&o->d_node_gas, t.node_gas); up(&o->d_st_nb, t.st_nb); up(&o->d_st_w, t.st_w); up(&o->d_inv_sigma2, t.inv_sigma2);
  return rc;
}

// The Rayleigh reduction of a handle with ECCKD_OPT_RAYLEIGH_ACTIVE: its rows (plain: cells, scattering: columns) and its
// first-level partials; and the shares of J_b that k_opt_sum_cost adds: the nodes' and, behind them, the Rayleigh chunks'.
size_t ray_nrows(const ecckd_opt* o) { return o->scattering ? o->ncol : o->ncell; }
size_t ray_npart(const ecckd_opt* o) { return (ray_nrows(o) + RAY_CHUNK - 1) / RAY_CHUNK; }
size_t opt_njb(const ecckd_opt* o) { return (o->nnode_active + (o->rayleigh_active ? 1 : 0)) * (size_t)o->grad_nchunk; }
// (slots per column of the scattering workspace, and the doubles of the per-(column, g) sums behind the columns)
size_t ray_ws_doubles(const ecckd_opt* o) {
  const size_t slot = (size_t)(o->nlay + 1) * o->ng;
  return o->ncol * (o->rayleigh_active ? RS_COUNT_ACTIVE : RS_COUNT) * slot + (o->rayleigh_active ? o->ncol * (size_t)o->ng : 0);
}
// doubles of the per-angle workspace of k_opt_forward_adjoint_lw_angles: (5 nangle + 1) (nlay + 1) ng per column
size_t lwa_ws_doubles(const ecckd_opt* o) { return o->ncol * lwa_slots(o->nangle) * (size_t)(o->nlay + 1) * o->ng; }
// dynamic LDS of the scattering kernel: the band and cost arrays; <true>: one double per thread behind them
size_t ray_lds_bytes(const ecckd_opt* o, int threads) {
  const size_t bytes = lds::rayleigh(o->nlay, o->ng, o->nband).bytes();
  return o->rayleigh_active ? ray_lds_offset(bytes) + (size_t)threads * sizeof(double) : bytes;
}

// the launch sizes of K8b and of the element-wise kernels, the work buffers and the pinned slots
int opt_alloc_work(ecckd_opt* o, const ot::Tables& t) {
  // every virtual block resident at once where that fits (8 blocks of 4 waves per CU), else a grid-stride loop
  auto grid_of = [&](size_t nslot) {
    unsigned gsz = (unsigned)std::min<size_t>((nslot + K8B_WAVES - 1) / K8B_WAVES, (size_t)std::max(o->ctx->num_cu, 1) * 8);
    return std::max(8u, (gsz + 7) / 8 * 8);
  };
  o->gradient_grid = grid_of(t.node_order.size());
  o->gather_grid = grid_of(t.run_order.size());
  o->grad_nslot = (int)t.node_order.size();
  o->gather_nslot = (int)t.run_order.size();
  o->grad_nrun = t.run_r0.size();
  o->grad_blocks = (unsigned)((o->nx + 255) / 256);
  if (o->alloc(&o->d_x, o->nx) != hipSuccess || o->alloc(&o->d_xprior, o->nx) != hipSuccess ||
      o->alloc(&o->d_grad, o->nx + 1) != hipSuccess || o->alloc(&o->d_dtau, o->ncell * o->ng) != hipSuccess ||
      o->alloc(&o->d_run_sum, std::max<size_t>(o->grad_nrun, 1) * o->grad_nchunk * 64) != hipSuccess ||
      o->alloc(&o->d_jcol, o->ncol) != hipSuccess || o->alloc(&o->d_jb, opt_njb(o)) != hipSuccess ||
      (o->rayleigh_active && (o->alloc(&o->d_ray_part, 2 * ray_npart(o) * o->grad_nchunk * 64) != hipSuccess ||
                              o->alloc(&o->d_ray_exp, 2 * (size_t)o->ng) != hipSuccess)))
    return ecckd::fail(ECCKD_OUT_OF_MEMORY, "ecckd_opt_create: device allocation failed");
  ECCKD_HIP_CHECK(hipHostMalloc((void**)&o->h_pin, PIN_SLOTS * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
  ECCKD_HIP_CHECK(hipHostGetDevicePointer((void**)&o->d_pin, o->h_pin, 0));
  return ECCKD_OK;
}

}  // namespace

extern "C" {

int ecckd_opt_create(ecckd_ctx* ctx, const ecckd_opt_model* m, int nscene, const ecckd_opt_scene* scenes,
                     const ecckd_opt_config* cfg, ecckd_opt** out) {
  return ecckd_opt_create_ex(ctx, m, nscene, scenes, cfg, 0u, out);
}

int ecckd_opt_create_ex(ecckd_ctx* ctx, const ecckd_opt_model* m, int nscene, const ecckd_opt_scene* scenes,
                        const ecckd_opt_config* cfg, unsigned flags, ecckd_opt** out) {
  return ecckd_opt_create_angles(ctx, m, nscene, scenes, cfg, flags, 0, out);
}

int ecckd_opt_create_angles(ecckd_ctx* ctx, const ecckd_opt_model* m, int nscene, const ecckd_opt_scene* scenes,
                            const ecckd_opt_config* cfg, unsigned flags, int nangle, ecckd_opt** out) {
  ECCKD_REQUIRE(ctx && m && scenes && cfg && out && nscene > 0, "ecckd_opt_create: NULL/empty argument");
  *out = nullptr;
  ECCKD_REQUIRE(nangle >= 0 && nangle <= ecckd::lbl::LBL_MAX_ANGLES, "ecckd_opt_create_angles: nangle = %d outside 0..%d", nangle,
                ecckd::lbl::LBL_MAX_ANGLES);
  std::vector<double> lw_angles;     // [3][nangle] sec, 1 / sec, wgt
  if (nangle > 0) {
    ECCKD_REQUIRE(!m->solar_irradiance, "ecckd_opt_create_angles: nangle = %d needs a longwave model (this one has solar_irradiance)", nangle);
    ECCKD_REQUIRE(flags == 0, "ecckd_opt_create_angles: nangle = %d cannot be combined with the ECCKD_OPT_RAYLEIGH flags (0x%x)", nangle, flags);
    // (one thread per g point of a column, at most 1 024 threads in a block)
    ECCKD_REQUIRE(m->ng <= 1024, "ecckd_opt_create_angles: nangle > 0 supports at most 1024 g points (ng = %d)", m->ng);
    int nang = 0;
    std::vector<double> sec_wgt;
    ECCKD_CHECK(ecckd::lbl::lw_angle_table("ecckd_opt_create_angles", nangle, &nang, sec_wgt));
    lw_angles.resize(3 * (size_t)nangle);
    for (int a = 0; a < nangle; ++a) {
      lw_angles[a] = sec_wgt[a];
      lw_angles[nangle + a] = 1.0 / sec_wgt[a];
      lw_angles[2 * nangle + a] = sec_wgt[nangle + a];
    }
  }
  ECCKD_REQUIRE((flags & ~(ECCKD_OPT_RAYLEIGH_SCATTERING | ECCKD_OPT_RAYLEIGH_ACTIVE)) == 0, "ecckd_opt_create_ex: unknown flags 0x%x", flags);
  const bool scattering = (flags & ECCKD_OPT_RAYLEIGH_SCATTERING) != 0;
  // (ECCKD_OPT_RAYLEIGH_ACTIVE on a model that is not shortwave with rayleigh_molar_scattering: refused by build_tables)
  if (scattering) {
    ECCKD_REQUIRE(m->solar_irradiance && m->rayleigh_molar_scattering,
                  "ecckd_opt_create_ex: ECCKD_OPT_RAYLEIGH_SCATTERING needs a shortwave model with rayleigh_molar_scattering");
    for (int s = 0; s < nscene; ++s)
      ECCKD_REQUIRE(scenes[s].mu0 && scenes[s].albedo, "ecckd_opt_create_ex: ECCKD_OPT_RAYLEIGH_SCATTERING: scene %d lacks mu0 or albedo", s);
    // (a block of k_opt_forward_adjoint_rayleigh has at most 512 threads - 256 VGPRs, nothing spilled - and one per g point)
    ECCKD_REQUIRE(m->ng <= 512, "ecckd_opt_create_ex: ECCKD_OPT_RAYLEIGH_SCATTERING supports at most 512 g points (ng = %d)", m->ng);
  }
  const char* plain = std::getenv("ECCKD_K8B_PLAIN_ORDER");
  const ot::Schedule schedule = {K8B_WAVES, K8B_RUN, plain && plain[0] == '1'};
  ot::Tables t;
  t.scattering = scattering;
  t.rayleigh_active = (flags & ECCKD_OPT_RAYLEIGH_ACTIVE) != 0;
  std::string refusal;
  const int rc = ot::build_tables(m, nscene, scenes, cfg, schedule, t, refusal);
  if (rc != ECCKD_OK) return ecckd::fail(rc, "%s", refusal.c_str());
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  OptPtr o(new ecckd_opt());
  o->ctx = ctx;
  o->cfg = *cfg;
  static_cast<ot::Layout&>(*o) = std::move(static_cast<ot::Layout&>(t));   // (k0 among it: from here on it is o->k0)
  if (o->scattering) {
    // the LDS of k_opt_forward_adjoint_rayleigh depends on the shapes alone: refused here, where the handle is made, and the
    // kernel's limit raised once, not at every launch of the minimiser's loop
    const size_t bytes = ray_lds_bytes(o.get(), 512);
    ECCKD_REQUIRE(bytes <= 160 * 1024, "ecckd_opt_create_ex: nlay * nband too large for the LDS of the scattering kernel (%zu B)", bytes);
    ECCKD_HIP_CHECK(hipFuncSetAttribute(o->rayleigh_active ? reinterpret_cast<const void*>(k_opt_forward_adjoint_rayleigh<true>)
                                                           : reinterpret_cast<const void*>(k_opt_forward_adjoint_rayleigh<false>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  }
  if (nangle > 0) {
    // as for the scattering kernel: the LDS depends on the shapes alone, so a shape is refused here and the limit raised once
    const size_t bytes = lds::lw_angles(o->nlay, o->ng, o->nband).bytes();
    ECCKD_REQUIRE(bytes <= 160 * 1024, "ecckd_opt_create_angles: nangle > 0: (nlay + 1) * (2 ng + 4 nband) too large for the LDS of the kernel (%zu B)", bytes);
    ECCKD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_opt_forward_adjoint_lw_angles),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    o->nangle = nangle;
  }
  ECCKD_CHECK(opt_upload_tables(o.get(), t));
  ECCKD_CHECK(opt_alloc_work(o.get(), t));
  if (nangle > 0) {
    ECCKD_CHECK(upload(o.get(), &o->d_lw_angles, lw_angles));
    if (o->alloc(&o->d_lwa_ws, lwa_ws_doubles(o.get())) != hipSuccess)
      return ecckd::fail(ECCKD_OUT_OF_MEMORY, "ecckd_opt_create_angles: device allocation of the per-angle workspace failed (%zu B)",
                         lwa_ws_doubles(o.get()) * sizeof(double));
  }
  if (o->scattering && o->alloc(&o->d_ray_ws, ray_ws_doubles(o.get())) != hipSuccess)
    return ecckd::fail(ECCKD_OUT_OF_MEMORY, "ecckd_opt_create_ex: device allocation of the scattering workspace failed");
  std::vector<double> xp(o->nx);
  ot::initial_state(*o, xp.data(), nullptr, nullptr);
  ECCKD_HIP_CHECK(hipMemcpyAsync(o->d_xprior, xp.data(), o->nx * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  *out = o.release();
  return ECCKD_OK;
}

int ecckd_opt_destroy(ecckd_opt* o) {
  opt_free(o);
  return ECCKD_OK;
}

size_t ecckd_opt_nx(ecckd_opt* o) { return o ? o->nx : 0; }

int ecckd_opt_nangle(ecckd_opt* o) { return o ? o->nangle : 0; }

int ecckd_opt_set_evaluator(ecckd_opt* o, ecckd_evaluator_fn fn, void* user) {
  ECCKD_REQUIRE(o, "ecckd_opt_set_evaluator: NULL handle");
  o->eval_fn = fn;
  o->eval_user = user;
  return ECCKD_OK;
}

int ecckd_opt_set_progress(ecckd_opt* o, ecckd_progress_fn fn, void* user) {
  ECCKD_REQUIRE(o, "ecckd_opt_set_progress: NULL handle");
  o->progress_fn = fn;
  o->progress_user = user;
  if (!o->tev[0]) {
    ECCKD_HIP_CHECK(hipSetDevice(o->ctx->device));
    for (int k = 0; k < 3; ++k) ECCKD_HIP_CHECK(hipEventCreate(&o->tev[k]));
  }
  return ECCKD_OK;
}

int ecckd_opt_timings(ecckd_opt* o, double* minimizer_s, double* a_priori_s, double* radiative_transfer_s) {
  ECCKD_REQUIRE(o, "ecckd_opt_timings: NULL handle");
  if (minimizer_s) *minimizer_s = o->t_minimizer;
  if (a_priori_s) *a_priori_s = o->t_prior;
  if (radiative_transfer_s) *radiative_transfer_s = o->t_rt;
  return ECCKD_OK;
}

// The prior of the optimised Rayleigh coefficients: J_b += 0.5 sum_g d_g^2 / sigma^2, d = x - x_prior on the unpinned tail
// elements, WITH its gradient d_g / sigma^2 (the reference adds the cost and drops the gradient, ckd_model.cpp:869-874).
int ecckd_opt_set_rayleigh_prior(ecckd_opt* o, double prior_error) {
  ECCKD_REQUIRE(o, "ecckd_opt_set_rayleigh_prior: NULL handle");
  ECCKD_REQUIRE(o->rayleigh_active, "ecckd_opt_set_rayleigh_prior: the handle was made without ECCKD_OPT_RAYLEIGH_ACTIVE");
  o->ray_prior_error = prior_error > 0.0 ? prior_error : 0.0;
  return ECCKD_OK;
}

// The Rayleigh molar scattering coefficients at state h_x: exp of the tail of an ECCKD_OPT_RAYLEIGH_ACTIVE handle's state (0 where
// pinned), formed by k_opt_exp on the device - the very numbers the forward kernels read at that state, which the host's exp
// matches only to a unit in the last place; any other handle, or h_x = NULL: the model's own.
int ecckd_opt_rayleigh_coefficients(ecckd_opt* o, const double* h_x, double* h_coeff) {
  ECCKD_REQUIRE(o && h_coeff, "ecckd_opt_rayleigh_coefficients: NULL argument");
  ECCKD_REQUIRE(o->ray_ent >= 0, "ecckd_opt_rayleigh_coefficients: the model has no rayleigh_molar_scattering");
  const size_t ng = (size_t)o->ng;
  if (!(o->rayleigh_active && h_x)) {
    std::memcpy(h_coeff, &o->k0[o->rayleigh_ix], ng * sizeof(double));
    return ECCKD_OK;
  }
  ecckd_ctx* ctx = o->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  double* d_in = o->d_ray_exp;                // [2][ng]: the tail of the state, its exp
  ECCKD_HIP_CHECK(hipMemcpyAsync(d_in, h_x + o->rayleigh_ix, ng * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_opt_exp, dim3((unsigned)((ng + 255) / 256)), dim3(256), 0, ctx->stream, ng, d_in, d_in + ng);
  ECCKD_HIP_CHECK(hipGetLastError());
  ECCKD_HIP_CHECK(hipMemcpyAsync(h_coeff, d_in + ng, ng * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return ECCKD_OK;
}

// The shape of the Rayleigh reduction of this handle (k_opt_rayleigh_reduce / _finish).
int ecckd_opt_rayleigh_plan(ecckd_opt* o, ecckd_rayleigh_plan* out) {
  ECCKD_REQUIRE(o && out, "ecckd_opt_rayleigh_plan: NULL argument");
  ecckd_rayleigh_plan p{};
  p.active = o->rayleigh_active ? 1 : 0;
  p.chunk_rows = RAY_CHUNK; p.finish_waves = RAY_FIN_WAVES; p.batch = RAY_BATCH;
  p.nrows = o->rayleigh_active ? ray_nrows(o) : 0;
  p.npart = o->rayleigh_active ? ray_npart(o) : 0;
  *out = p;
  return ECCKD_OK;
}

// The per-g flux-profile term (gpoint_seed_rows of the K8a kernels): weight and truth [ncol][2][nhl][ng], columns in scene order.
// weight <= 0 or h_truth == NULL removes the term and frees its block: the handle is then the handle it was.
int ecckd_opt_set_gpoint_truth(ecckd_opt* o, double weight, const double* h_truth) {
  ECCKD_REQUIRE(o, "ecckd_opt_set_gpoint_truth: NULL handle");
  ecckd_ctx* ctx = o->ctx;
  const size_t count = o->ncol * 2 * (size_t)(o->nlay + 1) * o->ng;
  std::string refusal;
  const int rc = ot::check_gpoint_truth(o->do_sw, o->scattering, o->rayleigh_active, weight, h_truth, count, refusal);
  if (rc != ECCKD_OK) return ecckd::fail(rc, "%s", refusal.c_str());
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (!ot::gpoint_truth_active(weight, h_truth)) {
    o->release(&o->d_gp_truth);
    o->gp_weight = 0.0;
    return ECCKD_OK;
  }
  if (!o->d_gp_truth && o->alloc(&o->d_gp_truth, count) != hipSuccess)
    return ecckd::fail(ECCKD_OUT_OF_MEMORY, "ecckd_opt_set_gpoint_truth: device allocation failed (%zu B)", count * sizeof(double));
  ECCKD_HIP_CHECK(hipMemcpyAsync(o->d_gp_truth, h_truth, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  o->gp_weight = weight;
  return ECCKD_OK;
}

int ecckd_opt_set_allreduce(ecckd_opt* o, ecckd_allreduce_fn fn, void* user, int add_prior) {
  ECCKD_REQUIRE(o, "ecckd_opt_set_allreduce: NULL argument");
  o->reduce_fn = fn;
  o->reduce_user = user;
  o->add_prior = fn == nullptr || add_prior != 0;
  return ECCKD_OK;
}

// Initial state and log-space bounds, solve_adept.cpp:335-353.  h_x_min/h_x_max may be NULL;
// unbounded elements get -/+ infinity.  Returns the gas order of the state in h_gas_order
// (user gas indices of the active gases, in state order) if not NULL.
int ecckd_opt_initial_state(ecckd_opt* o, double* h_x, double* h_x_min, double* h_x_max) {
  ECCKD_REQUIRE(o && h_x, "ecckd_opt_initial_state: NULL argument");
  ot::initial_state(*o, h_x, h_x_min, h_x_max);
  return ECCKD_OK;
}

}  // extern "C"

namespace {

// The arguments the three K8a kernels share, from the handle and the plan.  A scattering handle always keeps the Rayleigh entry
// apart from the absorbers; the others only in a run_ckd pass.  A diagnostic pass changes keep_negative and the two outputs.
K8aArgs k8a_args(const ecckd_opt* o, const ecckd_forward_plan& p) {
  K8aArgs a{};
  a.nlay = o->nlay; a.ng = o->ng; a.ngpad = p.ngpad; a.nband = o->nband; a.nent = o->nent;
  a.ray_ent = o->scattering ? o->ray_ent : o->eval_ray_ent;
  a.keep_negative = o->eval_keep_negative;
  a.mu0 = o->d_mu0; a.rel_flux = o->d_rel; a.k = o->d_k; a.ent_idx = o->d_ent_idx; a.ent_coef = o->d_ent_coef; a.band_of_g = o->d_band;
  a.planck_hl = o->d_planck; a.surf_emis = o->d_semis; a.conv = o->d_conv; a.layer_weight = o->d_lw;
  a.hr_true = o->d_hr; a.fdn_true = o->d_fdn; a.fup_true = o->d_fup; a.sfds = o->d_sfds; a.sfut = o->d_sfut;
  a.flux_weight = o->cfg.flux_weight; a.flux_profile_weight = o->cfg.flux_profile_weight; a.broadband_weight = o->cfg.broadband_weight;
  a.spectral_boundary_weight = o->cfg.spectral_boundary_weight; a.negative_od_penalty = o->cfg.negative_od_penalty;
  a.dtau = o->d_dtau; a.jcol = o->d_jcol; a.od_out = o->d_od_out; a.flux_out = o->d_flux_out;
  a.gp_truth = o->d_gp_truth; a.gp_weight = o->d_gp_truth ? o->gp_weight : 0.0;
  return a;
}

// The cell-parallel K8a kernel, one instance per (cells per thread, shortwave, 8-entry batches of a cell's table, and in the
// longwave the per-g flux-profile term).
template <int NC, bool SW, int NB, bool GP = false>
int launch_cells(ecckd_opt* o, const ecckd_forward_plan& p) {
  const auto kernel = k_opt_forward_adjoint_cells<NC, SW, NB, GP>;
  ECCKD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  hipLaunchKernelGGL(kernel, dim3((unsigned)o->ncol), dim3(p.threads), p.lds_bytes, o->ctx->stream, k8a_args(o, p), o->d_band_ptr, o->d_band_g);
  return ECCKD_OK;
}

template <int NC, bool SW, bool GP = false>
int launch_cells_nb(ecckd_opt* o, const ecckd_forward_plan& p) {
  switch (p.nb) {
    case 1: return launch_cells<NC, SW, 1, GP>(o, p);
    case 2: return launch_cells<NC, SW, 2, GP>(o, p);
    case 3: return launch_cells<NC, SW, 3, GP>(o, p);
    case 4: return launch_cells<NC, SW, 4, GP>(o, p);
    default: return launch_cells<NC, SW, 0, GP>(o, p);
  }
}

int launch_cells_for(ecckd_opt* o, const ecckd_forward_plan& p) {   // p.nc_template: 4 or 8, the instance
  if (o->do_sw) return p.nc_template <= 4 ? launch_cells_nb<4, true>(o, p) : launch_cells_nb<8, true>(o, p);
  if (o->d_gp_truth) return p.nc_template <= 4 ? launch_cells_nb<4, false, true>(o, p) : launch_cells_nb<8, false, true>(o, p);
  return p.nc_template <= 4 ? launch_cells_nb<4, false>(o, p) : launch_cells_nb<8, false>(o, p);
}

// Which K8a kernel a forward pass runs and how it is launched: a function of the shapes and the two environment knobs alone
// (ecckd_opt_forward_plan reports it, opt_launch_forward launches from it and from nothing else).
//   cell-parallel kernel: longwave 1 024 threads (16 layer groups at ng = 64, one block per CU), shortwave 512 (8 groups, 73 KiB
//   of LDS: two blocks per CU), `env_threads` (64 ... 1024, else 0) in place of either; up to 8 cells per thread (the <4> and
//   <8> instances), nb = 8-entry batches of a cell's table among its first 64 entries (1 ... 4 in straight-line code, 0 = the loop);
//   else the general kernel, whose LDS tile the caller has to check against 160 KB.
ecckd_forward_plan forward_plan(bool do_sw, int nlay, int ng, int nband, int nent, int env_threads, bool force_generic) {
  ecckd_forward_plan p{};
  const int nhl = nlay + 1;
  p.ngpad = (ng + 63) / 64 * 64;
  {
    const int threads_c = env_threads ? env_threads : (do_sw ? 512 : 1024);
    const int lgroups = std::max(1, threads_c / p.ngpad);
    const int nc = (nlay + lgroups - 1) / lgroups;
    const size_t bytes = lds::cells(nlay, ng, nband, do_sw).bytes();
    if (!force_generic && nc <= 8 && bytes <= 160 * 1024 && p.ngpad * lgroups <= 1024 && nhl * nband <= K8A_MAXR * p.ngpad * lgroups) {
      p.cells = 1;
      p.nc_template = nc <= 4 ? 4 : 8;
      const int nb = (std::min(nent, 64) + K8A_GB - 1) / K8A_GB;       // 8-entry batches of a cell's table (first 64 entries)
      p.nb = nb <= 4 ? nb : 0;
      p.threads = p.ngpad * lgroups;
      p.lgroups = lgroups;
      p.lds_bytes = bytes;
      return p;
    }
  }
  const int k8a_threads = env_threads ? env_threads : 1024;
  p.lgroups = std::max(1, k8a_threads / p.ngpad);
  p.threads = p.ngpad * p.lgroups;
  p.lds_bytes = lds::general(nlay, ng, nband).bytes();
  return p;
}

// the plan of this handle at the environment as it is now (both knobs are read at every call: the tests switch between the
// kernels and the block sizes within one process)
ecckd_forward_plan opt_forward_plan(const ecckd_opt* o) {
  const char* e = std::getenv("ECCKD_K8A_THREADS");
  const int v = e ? std::atoi(e) : 0;
  if (o->scattering) {
    // k_opt_forward_adjoint_rayleigh, the one kernel of a scattering handle: 512 threads (8 layer groups at ng = 64), the LDS
    // holds the band and cost arrays only
    ecckd_forward_plan p{};
    p.cells = 2;
    p.ngpad = (o->ng + 63) / 64 * 64;
    p.lgroups = std::max(1, (v >= 64 && v <= 512 ? v : 512) / p.ngpad);   // (ecckd_opt_create_ex has refused ng > 512)
    p.threads = p.ngpad * p.lgroups;
    p.lds_bytes = ray_lds_bytes(o, p.threads);
    return p;
  }
  if (o->nangle > 0) {
    // k_opt_forward_adjoint_lw_angles, the one kernel of a handle with the angle quadrature: 1 024 threads (16 layer groups at
    // ng = 64), the LDS holds the angle-summed flux rows and the band and cost arrays
    ecckd_forward_plan p{};
    p.cells = 3;
    p.ngpad = (o->ng + 63) / 64 * 64;
    p.lgroups = std::max(1, (v >= 64 && v <= 1024 ? v : 1024) / p.ngpad);   // (ecckd_opt_create_angles has refused ng > 1024)
    p.threads = p.ngpad * p.lgroups;
    p.lds_bytes = lds::lw_angles(o->nlay, o->ng, o->nband).bytes();
    return p;
  }
  const char* env_generic = std::getenv("ECCKD_K8A_GENERIC");
  return forward_plan(o->do_sw, o->nlay, o->ng, o->nband, o->nent, v >= 64 && v <= 1024 ? v : 0, env_generic && env_generic[0] == '1');
}

// K8a at the coefficients in d_k: the cell-parallel kernel where the profile fits it, else the general one.
int opt_launch_forward(ecckd_opt* o) {
  ecckd_ctx* ctx = o->ctx;
  const ecckd_forward_plan p = opt_forward_plan(o);
  if (o->scattering) {
    // (ecckd_opt_create_ex has checked the LDS and raised the kernel's limit; the Rayleigh entry is always kept apart from the absorbers; a diagnostic pass changes only keep_negative)
    if (o->rayleigh_active)
      hipLaunchKernelGGL(k_opt_forward_adjoint_rayleigh<true>, dim3((unsigned)o->ncol), dim3(p.threads), p.lds_bytes, ctx->stream, k8a_args(o, p),
                         o->d_band_ptr, o->d_band_g, o->d_ray_ws);
    else
      hipLaunchKernelGGL(k_opt_forward_adjoint_rayleigh<false>, dim3((unsigned)o->ncol), dim3(p.threads), p.lds_bytes, ctx->stream, k8a_args(o, p),
                         o->d_band_ptr, o->d_band_g, o->d_ray_ws);
    ECCKD_HIP_CHECK(hipGetLastError());
    return ECCKD_OK;
  }
  if (o->nangle > 0) {
    // (ecckd_opt_create_angles has checked the LDS and raised the kernel's limit)
    hipLaunchKernelGGL(k_opt_forward_adjoint_lw_angles, dim3((unsigned)o->ncol), dim3(p.threads), p.lds_bytes, ctx->stream, k8a_args(o, p),
                       o->d_band_ptr, o->d_band_g, o->nangle, o->d_lw_angles, o->d_lwa_ws);
    ECCKD_HIP_CHECK(hipGetLastError());
    return ECCKD_OK;
  }
  if (p.cells) {
    ECCKD_CHECK(launch_cells_for(o, p));
    ECCKD_HIP_CHECK(hipGetLastError());
    return ECCKD_OK;
  }
  ECCKD_REQUIRE(p.lds_bytes <= 160 * 1024, "ecckd_opt_cost_grad: nlay*ng too large for the per-profile LDS tile (%zu B)", p.lds_bytes);
  ECCKD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_opt_forward_adjoint),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  hipLaunchKernelGGL(k_opt_forward_adjoint, dim3((unsigned)o->ncol), dim3(p.threads), p.lds_bytes, ctx->stream, k8a_args(o, p), o->do_sw ? 1 : 0);
  ECCKD_HIP_CHECK(hipGetLastError());
  return ECCKD_OK;
}

// CkdOptimizable::calc_cost_function_gradient (solve_adept.cpp:240-292).
// cost and gradient at the DEVICE state d_x -> d_grad; J on the host (one stream sync).
// Results the host needs at once (the cost of a trial point, the dot products of the L-BFGS update) arrive in pinned slots
// that the host watches (slots_mark_pending / slots_wait, common.hpp): two waits per iteration, each a PCIe write away from
// the kernel's end.
int opt_cost_grad_dev(ecckd_opt* o, const double* d_x, double* d_grad, double* J, bool k_ready = false) {
  ecckd_ctx* ctx = o->ctx;
  if (o->eval_fn && o->d_od_out == nullptr) {
    // the caller's cost function and gradient in place of the device's: the minimizer itself is unchanged
    o->eval_x.resize(o->nx);
    o->eval_g.assign(o->nx, 0.0);
    ECCKD_HIP_CHECK(hipMemcpyAsync(o->eval_x.data(), d_x, o->nx * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const int rc = o->eval_fn(o->nx, o->eval_x.data(), J, o->eval_g.data(), o->eval_user);
    if (rc != 0) return ecckd::fail(ECCKD_PROCESSING_ERROR, "ecckd_opt: the cost-function callback failed (%d)", rc);
    ECCKD_HIP_CHECK(hipMemcpyAsync(d_grad, o->eval_g.data(), o->nx * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    o->n_eval++;
    return ECCKD_OK;
  }
  const bool reduce = o->reduce_fn != nullptr && o->d_od_out == nullptr;   // not for the diagnostic forward pass
  const bool prior = !reduce || o->add_prior;   // (the reference always adds calc_background_cost_function, :273)
  if (!k_ready)     // (the minimizer's step kernel leaves exp(x) of its trial point in d_k)
    hipLaunchKernelGGL(k_opt_exp, dim3(o->grad_blocks), dim3(256), 0, ctx->stream, o->nx, d_x, o->d_k);
  const int ng = o->ng;
  const bool timed = o->tev[0] != nullptr;
  if (timed) ECCKD_HIP_CHECK(hipEventRecord(o->tev[0], ctx->stream));
  ECCKD_CHECK(opt_launch_forward(o));
  if (timed) ECCKD_HIP_CHECK(hipEventRecord(o->tev[1], ctx->stream));
  hipLaunchKernelGGL(k_opt_gradient_gather, dim3(o->gather_grid), dim3(64 * K8B_WAVES), 0, ctx->stream, o->gather_nslot, ng, o->grad_nchunk,
                     o->d_run_order, o->d_run_r0, o->d_run_last, o->d_ref_cell, o->d_ref_coef, o->d_dtau, o->d_run_sum);
  hipLaunchKernelGGL(k_opt_gradient_finish, dim3(o->gradient_grid), dim3(64 * K8B_WAVES), 0, ctx->stream, o->grad_nslot, ng, o->grad_nchunk,
                     d_x, o->d_xprior, o->d_k, o->d_node_run0, o->d_run_sum, o->d_node_gas, o->d_st_nb, o->d_st_w, o->d_inv_sigma2,
                     prior ? 1 : 0, d_grad, o->d_jb, o->d_node_order);
  if (o->rayleigh_active) {
    // the ng tail elements: rows -> first-level partials -> gradient and the tail's share of J_b (two launches, no host wait)
    const size_t nrows = ray_nrows(o), npart = ray_npart(o);
    const double* src = o->scattering ? o->d_ray_ws + (ray_ws_doubles(o) - o->ncol * (size_t)ng) : o->d_dtau;
    const bool ray_prior = prior && o->ray_prior_error > 0.0;
    hipLaunchKernelGGL(k_opt_rayleigh_reduce, dim3((unsigned)((npart * o->grad_nchunk + RAY_RED_WAVES - 1) / RAY_RED_WAVES)), dim3(64 * RAY_RED_WAVES),
                       0, ctx->stream, nrows, ng, o->grad_nchunk, src, o->scattering ? nullptr : o->d_moles, o->d_ray_part);
    hipLaunchKernelGGL(k_opt_rayleigh_finish, dim3((unsigned)o->grad_nchunk), dim3(64 * RAY_FIN_WAVES), 0, ctx->stream, npart, ng, o->grad_nchunk,
                       o->d_ray_part, o->rayleigh_ix, d_x, o->d_xprior, o->d_k,
                       ray_prior ? 1.0 / (o->ray_prior_error * o->ray_prior_error) : 0.0, ray_prior ? 1 : 0, d_grad,
                       o->d_jb + o->nnode_active * (size_t)o->grad_nchunk);
  }
  ECCKD_HIP_CHECK(hipGetLastError());
  if (timed) ECCKD_HIP_CHECK(hipEventRecord(o->tev[2], ctx->stream));
  // the cost: profiles, then the prior's node terms, summed on the device in a fixed order and delivered to the host's slot
  // (and, for the profile-sharded all-reduce, into the slot behind the gradient: ONE collective of nx + 1 doubles)
  double* h_cost = o->h_pin + PIN_COST;
  ecckd::slots_mark_pending(h_cost, 1);
  hipLaunchKernelGGL(k_opt_sum_cost, dim3(1), dim3(256), 0, ctx->stream, o->d_jcol, o->ncol, o->d_jb, opt_njb(o), prior ? 1 : 0,
                     o->d_pin + PIN_COST, reduce ? d_grad + o->nx : nullptr);
  ECCKD_HIP_CHECK(hipGetLastError());
  ECCKD_CHECK(ecckd::slots_wait(ctx->stream, h_cost, 1, "ecckd_opt: results"));
  if (timed) {
    // "radiative transfer": look-up, penalty, two sweeps, cost and their adjoint; "a-priori": the gradient kernel, which
    // gathers the adjoint back onto the coefficients and adds the prior term (the reference times the prior alone there)
    float ms = 0.f;
    ECCKD_HIP_CHECK(hipEventSynchronize(o->tev[2]));
    ECCKD_HIP_CHECK(hipEventElapsedTime(&ms, o->tev[0], o->tev[1]));
    o->t_rt += 1e-3 * ms;
    ECCKD_HIP_CHECK(hipEventElapsedTime(&ms, o->tev[1], o->tev[2]));
    o->t_prior += 1e-3 * ms;
  }
  *J = *h_cost;
  if (reduce) {
    double* slot = o->h_pin + PIN_REDUCED_COST;
    ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const int rc = o->reduce_fn(d_grad, o->nx + 1, (void*)ctx->stream, o->reduce_user);
    if (rc != 0) return ecckd::fail(ECCKD_PROCESSING_ERROR, "ecckd_opt: the all-reduce callback failed (%d)", rc);
    ECCKD_HIP_CHECK(hipMemcpyAsync(slot, d_grad + o->nx, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *J = *slot;
  }
  o->n_eval++;
  return ECCKD_OK;
}

// A diagnostic forward pass: `body` runs K8a with the two output buffers in place and the evaluation mode set (ray_ent: the
// entry added after the clamp, or -1; keep_negative: 0 clamp, 1 / 2 report the optical depth / also the fluxes unclamped),
// then total optical depth [ncol][nlay][ng] and CKD fluxes [ncol][2][nlay+1][ng] are copied out where asked for.  The buffers
// and the mode are the handle's for the length of this call only, whichever way it ends: while they are set the evaluator
// and the all-reduce are bypassed (opt_cost_grad_dev).
template <typename Body>
int opt_diagnostic_pass(ecckd_opt* o, int ray_ent, int keep_negative, double* h_od, double* h_flux, Body body) {
  ecckd_ctx* ctx = o->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const size_t od_bytes = o->ncell * o->ng * sizeof(double), flux_bytes = o->ncol * 2 * (o->nlay + 1) * o->ng * sizeof(double);
  void* od = nullptr;
  void* flux = nullptr;
  ECCKD_HIP_CHECK(hipMalloc(&od, od_bytes));
  const hipError_t e = hipMalloc(&flux, flux_bytes);
  if (e != hipSuccess) (void)hipFree(od);
  ECCKD_HIP_CHECK(e);
  o->d_od_out = (double*)od;
  o->d_flux_out = (double*)flux;
  o->eval_ray_ent = ray_ent;
  o->eval_keep_negative = keep_negative;
  int rc = body();
  o->eval_ray_ent = -1;
  o->eval_keep_negative = 0;
  if (rc == ECCKD_OK && h_od) rc = ecckd_d2h(ctx, h_od, o->d_od_out, od_bytes);
  if (rc == ECCKD_OK && h_flux) rc = ecckd_d2h(ctx, h_flux, o->d_flux_out, flux_bytes);
  (void)hipFree(o->d_od_out); (void)hipFree(o->d_flux_out);
  o->d_od_out = nullptr; o->d_flux_out = nullptr;
  return rc;
}

}  // namespace

extern "C" {

// The K8a kernel the next forward pass of this handle runs (forward_plan above), at the environment as it is now.
int ecckd_opt_forward_plan(ecckd_opt* o, ecckd_forward_plan* out) {
  ECCKD_REQUIRE(o && out, "ecckd_opt_forward_plan: NULL argument");
  *out = opt_forward_plan(o);
  return ECCKD_OK;
}

int ecckd_opt_cost_grad(ecckd_opt* o, const double* h_x, double* J, double* h_grad) {
  ECCKD_REQUIRE(o && h_x && J, "ecckd_opt_cost_grad: NULL argument");
  ecckd_ctx* ctx = o->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  ECCKD_HIP_CHECK(hipMemcpyAsync(o->d_x, h_x, o->nx * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ECCKD_CHECK(opt_cost_grad_dev(o, o->d_x, o->d_grad, J));
  if (h_grad) {
    ECCKD_HIP_CHECK(hipMemcpyAsync(h_grad, o->d_grad, o->nx * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  }
  return ECCKD_OK;
}

// Forward products for checking/diagnostics: total optical depth [ncol][nlay][ng] (after the
// negative clamp) and the CKD fluxes [ncol][2][nlay+1][ng] (LblFluxes::calc_ckd_fluxes,
// lbl_fluxes.cpp:443-471) at state h_x.
int ecckd_opt_forward(ecckd_opt* o, const double* h_x, double* h_od, double* h_flux) {
  return ecckd_opt_forward_ex(o, h_x, 0, h_od, h_flux);
}

// unclamped != 0: optical depths and fluxes WITHOUT the clamp of negative total optical depths at zero, as the reference
// evaluates the "relative_to" scene (optimize_lut.cpp:229-234: calc_total_optical_depth -> value() -> calc_ckd_fluxes;
// the clamp lives in calc_cost_function_and_gradient only, solve_adept.cpp:107-116).
int ecckd_opt_forward_ex(ecckd_opt* o, const double* h_x, int unclamped, double* h_od, double* h_flux) {
  ECCKD_REQUIRE(o && h_x, "ecckd_opt_forward: NULL argument");
  return opt_diagnostic_pass(o, -1, unclamped ? 2 : 0, h_od, h_flux, [&] {
    double J;
    return ecckd_opt_cost_grad(o, h_x, &J, nullptr);
  });
}

// The optimised molar absorption coefficients of one (user-indexed) gas at state h_x:
// k = exp(x), 0 where x is pinned at MIN_X (solve_adept.cpp:242-249).
int ecckd_opt_coefficients(ecckd_opt* o, const double* h_x, int gas, double* h_molar_abs) {
  ECCKD_REQUIRE(o && h_molar_abs && gas >= 0 && gas < o->ngas, "ecckd_opt_coefficients: bad argument");
  const ot::GasInfo& gi = o->gases[o->user_to_k[gas]];
  for (size_t e = 0; e < gi.nnode * o->ng; ++e) {
    const size_t ge = gi.ix + e;
    if (gi.active && h_x) h_molar_abs[e] = h_x[ge] > MIN_X ? std::exp(h_x[ge]) : 0.0;
    else h_molar_abs[e] = o->k0[ge];
  }
  return ECCKD_OK;
}

}  // extern "C"

namespace {

// the minimizer's device workspace (kept by the handle for the next call), the start point and the bounds
int opt_minimize_workspace(ecckd_opt* o, const std::vector<double>& x0, const std::vector<double>& xmin, const std::vector<double>& xmax) {
  hipStream_t stream = o->ctx->stream;
  const size_t n = o->nx;
  auto ensure = [&](double** p, size_t cnt) -> int {
    if (!*p) ECCKD_HIP_CHECK(o->alloc(p, cnt));
    return ECCKD_OK;
  };
  ECCKD_CHECK(ensure(&o->d_xn, n)); ECCKD_CHECK(ensure(&o->d_gn, n + 1)); ECCKD_CHECK(ensure(&o->d_dir, n));
  ECCKD_CHECK(ensure(&o->d_q, n)); ECCKD_CHECK(ensure(&o->d_S, (size_t)LB_M * n)); ECCKD_CHECK(ensure(&o->d_Y, (size_t)LB_M * n));
  ECCKD_HIP_CHECK(hipMemsetAsync(o->d_S, 0, (size_t)LB_M * n * sizeof(double), stream));     // unused pairs are read (with zero weight)
  ECCKD_HIP_CHECK(hipMemsetAsync(o->d_Y, 0, (size_t)LB_M * n * sizeof(double), stream));
  ECCKD_CHECK(ensure(&o->d_part, (size_t)(LB_NPART + 2) * VEC_BLOCKS));
  if (!xmin.empty()) {
    ECCKD_CHECK(ensure(&o->d_xmin, n)); ECCKD_CHECK(ensure(&o->d_xmax, n));
    ECCKD_HIP_CHECK(hipMemcpyAsync(o->d_xmin, xmin.data(), n * sizeof(double), hipMemcpyHostToDevice, stream));
    ECCKD_HIP_CHECK(hipMemcpyAsync(o->d_xmax, xmax.data(), n * sizeof(double), hipMemcpyHostToDevice, stream));
  }
  ECCKD_HIP_CHECK(hipMemcpyAsync(o->d_x, x0.data(), n * sizeof(double), hipMemcpyHostToDevice, stream));
  return ECCKD_OK;
}

LbSlots lb_slots(const ecckd::LbfgsHistory& h) {
  LbSlots s;
  s.n = h.n;
  h.slots(s.slot);
  return s;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------
// solve_adept (solve_adept.cpp:310-417).  adept::Minimizer is a third-party L-BFGS that is not
// available here (trajectory parity unpinned); this is a standard L-BFGS (m = 6, compact
// representation, see the k_lb_* kernels and lbfgs_history.hpp) with Armijo backtracking + curvature-guarded updates, the step
// capped at max_step_size = 2 in the 2-norm (:331) and simple projection onto [x_min, x_max] when
// bounded (:344-353).  Status values follow adept::MinimizerStatus (0 success, 2 max
// iterations, 3 failed to converge, 6 invalid cost function, 7 invalid gradient).
int ecckd_opt_minimize(ecckd_opt* o, int max_iterations, double convergence_criterion, int is_bounded,
                       double* h_x, int* status, int* n_iterations, double* J_final, double* gnorm_final) {
  ECCKD_REQUIRE(o && h_x && status, "ecckd_opt_minimize: NULL argument");
  ecckd_ctx* ctx = o->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const size_t n = o->nx;
  constexpr int NPART = LB_NPART;   // update: |q|^2, S.q, Y.q (1 + 2M) | pair dots (2 + 3M)
  // state, bounds and history live on the device; the host only sees scalars
  const bool bounded = is_bounded && !o->kmin.empty();
  std::vector<double> x0(n), xmin(bounded ? n : 0), xmax(bounded ? n : 0);
  ot::initial_state(*o, x0.data(), bounded ? xmin.data() : nullptr, bounded ? xmax.data() : nullptr);
  ECCKD_CHECK(opt_minimize_workspace(o, x0, xmin, xmax));
  const double* bmin = bounded ? o->d_xmin : nullptr;
  const double* bmax = bounded ? o->d_xmax : nullptr;
  double* x = o->d_x; double* g = o->d_grad; double* xn = o->d_xn; double* gn = o->d_gn;
  double* part_a = o->d_part;                                  // the update's NPART partial arrays
  double* part_dg = o->d_part + (size_t)NPART * VEC_BLOCKS;    // direction: d.g, then d.d
  double* part_dd = part_dg + VEC_BLOCKS;
  double* h_dots = o->h_pin + PIN_LB_DOTS;
  double* h_step = o->h_pin + PIN_LB_STEP;
  // one block of 16 waves per CU is what the update kernel's registers allow: no more blocks than CUs (a second, nearly empty
  // round would cost a whole pass again)
  const int nblk = (int)std::min<size_t>(std::min<size_t>(VEC_BLOCKS, (size_t)std::max(ctx->num_cu, 1)), std::max<size_t>(1, (n + VEC_THREADS - 1) / VEC_THREADS));
  const dim3 vb(nblk), vt(VEC_THREADS);
  const double max_step = 2.0;  // minimizer.set_max_step_size(2.0), solve_adept.cpp:331
  ecckd::LbfgsHistory lb;
  // the pair (x1 - x0, g1 - g0) into ring slot `slot` (-1: none), its dots with the pairs `keep`, and the projected gradient
  // at x1 with every pair's dots, in ONE pass; awaited at the top of the loop
  auto launch_update = [&](const LbSlots& keep, int slot, const double* x0d, const double* x1d, const double* g0d, const double* g1d) {
    ecckd::slots_mark_pending(h_dots, NPART);
    hipLaunchKernelGGL(k_lb_update, vb, vt, 0, ctx->stream, n, keep, slot, x0d, x1d, g0d, g1d, bmin, bmax, o->d_q, o->d_S, o->d_Y, part_a);
    hipLaunchKernelGGL(k_lb_finish, dim3(NPART), dim3(FIN_THREADS), 0, ctx->stream, part_a, nblk, o->d_pin + PIN_LB_DOTS);
    return hipGetLastError();
  };
  // the trial point (and its coefficients) at `step` along the direction (-1: the first trial, its length chosen on the
  // device), then the cost there
  auto trial = [&](double step, bool steepest, double* Jn) {
    hipLaunchKernelGGL(k_lb_step, vb, vt, 0, ctx->stream, n, step, steepest ? 1 : 0, max_step, 1.0, part_dg, part_dd,
                       x, o->d_dir, bmin, bmax, xn, o->d_k, o->d_pin + PIN_LB_STEP);
    ECCKD_HIP_CHECK(hipGetLastError());
    return opt_cost_grad_dev(o, xn, gn, Jn, true);
  };

  const auto wall0 = std::chrono::steady_clock::now();
  const double dev0 = o->t_rt + o->t_prior;
  double J = 0.0;
  ECCKD_CHECK(opt_cost_grad_dev(o, x, g, &J));
  int st = 2, it = 0;
  double gnorm = 0.0;
  if (!(J == J)) { *status = 6; if (J_final) *J_final = J; return ECCKD_OK; }
  ECCKD_HIP_CHECK(launch_update(lb_slots(lb), -1, x, x, g, g));   // projected gradient and its norm at the starting point (no pair yet)
  for (it = 0; it <= max_iterations; ++it) {
    // |q|^2, S^T q, Y^T q at the current point (the pending pair included, as the newest) and the pending pair's own dots
    ECCKD_CHECK(ecckd::slots_wait(ctx->stream, h_dots, NPART, "ecckd_opt: results"));
    lb.absorb_pending(h_dots);
    gnorm = std::sqrt(h_dots[0]);
    if (o->progress_fn) o->progress_fn(it, J, gnorm, o->progress_user);   // report_progress, solve_adept.cpp:295-299
    if (!(gnorm == gnorm)) { st = 7; break; }
    if (gnorm <= convergence_criterion) { st = 0; break; }
    if (it == max_iterations) { st = 2; break; }

    bool restarted = false;
    double Jn = J, step = 0.0, dg = 0.0;
    bool ok = false;
    for (;;) {
      LbCoef cf;
      cf.gamma = lb.coefficients(h_dots, cf.cs, cf.cy);
      hipLaunchKernelGGL(k_lb_direction, vb, vt, 0, ctx->stream, n, lb_slots(lb), cf, o->d_q, o->d_S, o->d_Y, g, o->d_dir, part_dg);
      // one wait for the step and the cost of the first trial
      ecckd::slots_mark_pending(h_step, 3);
      ECCKD_CHECK(trial(-1.0, lb.n == 0, &Jn));
      ECCKD_CHECK(ecckd::slots_wait(ctx->stream, h_step, 3, "ecckd_opt: results"));
      step = h_step[0];
      dg = h_step[2];
      if (!(dg < 0.0)) {
        // not a descent direction: drop the history, steepest descent on the projected gradient
        // steepest descent on a non-zero projected gradient that is not a descent direction either: the gradient is not
        // a number (MINIMIZER_STATUS_INVALID_GRADIENT) or no direction can be found (..._DIRECTION_FAILURE) - not "converged"
        if (restarted || lb.n == 0) { ok = false; st = (dg != dg) ? 7 : 4; break; }
        restarted = true;
        lb.restart();
        continue;
      }
      ok = (Jn == Jn && Jn <= J + 1.0e-4 * step * dg);
      // (Tried in round 4 and dropped: a line search that remembers - the next iteration starting from the fraction of the capped
      // step that was accepted last, doubled after a first-trial acceptance.  Over 300 iterations at nx = 3.05e5: 5 800 against
      // 6 000 iterations/s longwave, 3 830 against 3 730 shortwave, final costs 66.62 against 66.39 and 53.62 against 53.56 -
      // fewer evaluations per iteration, smaller steps, nothing gained.)
      for (int ls = 1; !ok && ls < 30; ++ls) {
        step *= 0.5;
        ECCKD_CHECK(trial(step, false, &Jn));
        ok = (Jn == Jn && Jn <= J + 1.0e-4 * step * dg);
      }
      if (!ok && lb.n > 0 && !restarted) {
        // the quasi-Newton direction did not give a sufficient decrease (typically many variables at their bounds):
        // forget the history and try the projected steepest descent before giving up
        restarted = true;
        lb.restart();
        continue;
      }
      if (!ok) st = 3;
      break;
    }
    if (!ok) break;
    // curvature pair into the next ring slot (replacing the oldest when the ring is full)
    const int slot = lb.next_slot();
    ECCKD_HIP_CHECK(launch_update(lb_slots(lb), slot, x, xn, g, gn));
    std::swap(x, xn);
    std::swap(g, gn);
    J = Jn;
  }
  // (a break may leave the slots of an update in flight: they belong to this handle's pinned block, nobody else reads them)
  ECCKD_HIP_CHECK(hipMemcpyAsync(h_x, x, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  o->t_minimizer += std::chrono::duration<double>(std::chrono::steady_clock::now() - wall0).count() - (o->t_rt + o->t_prior - dev0);
  *status = st;
  if (n_iterations) *n_iterations = it;
  if (J_final) *J_final = J;
  if (gnorm_final) *gnorm_final = gnorm;
  return ECCKD_OK;
}

// ---------------------------------------------------------------------------------------
// run_ckd (run_ckd.cpp:27-373): evaluate a CKD model on a set of profiles.  The gas optical depths
// are summed and clamped at zero (:318), Rayleigh scattering is added after the clamp (:361), the
// longwave fluxes come from radiative_transfer_lw with unit emissivity and the surface Planck
// function at temperature_hl(end) (:343-347), the shortwave direct beam from
// radiative_transfer_direct_sw at the scene's mu0 with tsi / sum(ssi) scaling (:358-363).
// The coefficients are used as they are (no exp(log k) round trip): d_k still holds what ecckd_opt_create uploaded.
static int run_ckd_impl(ecckd_ctx* ctx, const ecckd_opt_model* m, const ecckd_opt_scene* scene, double* h_od,
                        double* h_rayleigh_od, double* h_planck_hl, double* h_flux, int keep_negative) {
  ECCKD_REQUIRE(ctx && m && scene && m->gases && m->iband_per_g, "ecckd_run_ckd: NULL argument");
  ECCKD_REQUIRE(scene->ncol > 0 && scene->nlay > 0 && scene->pressure_hl && scene->temperature_hl,
                "ecckd_run_ckd: scene needs pressure_hl and temperature_hl");
  const bool do_sw = m->solar_irradiance != nullptr;
  std::vector<ecckd_opt_gas> gases(m->gases, m->gases + m->ngas);
  // gases outside the scene's list are skipped whatever their concentration dependence (run_ckd.cpp:270-276;
  // the optimiser keeps concentration-independent gases, solve_adept.cpp:55-67): give them zero coefficients
  size_t zsize = 0;
  for (int i = 0; i < m->ngas; ++i)
    zsize = std::max(zsize, (size_t)(m->gases[i].conc_dependence == 2 ? m->gases[i].nconc : 1) * m->nt * m->np * m->ng);
  std::vector<double> zero_k(zsize, 0.0);
  for (int i = 0; i < m->ngas; ++i) {
    ecckd_opt_gas& g = gases[i];
    g.is_active = 1;
    g.min_molar_abs = nullptr;
    g.max_molar_abs = nullptr;
    if (scene->gas_present && !scene->gas_present[i]) g.molar_abs = zero_k.data();
  }
  ecckd_opt_model mm = *m;
  mm.gases = gases.data();
  int nband = 0;
  for (int g = 0; g < m->ng; ++g) nband = std::max(nband, m->iband_per_g[g] + 1);
  const size_t ncol = (size_t)scene->ncol, nhl = (size_t)scene->nlay + 1, nlay = (size_t)scene->nlay, ng = (size_t)m->ng;
  std::vector<double> zeros(ncol * nhl * (size_t)nband, 0.0), albedo0((size_t)nband, 0.0);
  ecckd_opt_scene sc = *scene;
  sc.nband = nband;
  sc.flux_dn = zeros.data();
  sc.flux_up = zeros.data();
  sc.surf_emissivity = nullptr;          // unit emissivity (:339-340)
  sc.spectral_flux_dn_surf = nullptr;
  sc.spectral_flux_up_toa = nullptr;
  sc.spectral_boundary_weights = nullptr;
  sc.relative_flux_dn = nullptr;
  sc.relative_flux_up = nullptr;
  if (do_sw) sc.albedo = albedo0.data();  // direct beam only
  ecckd_opt_config cfg;
  std::memset(&cfg, 0, sizeof(cfg));
  cfg.pressure_weight_power = 0.5;
  cfg.prior_error = 1.0;
  cfg.pressure_corr = cfg.temperature_corr = cfg.conc_corr = 0.5;
  ecckd_opt* created = nullptr;
  ECCKD_CHECK(ecckd_opt_create(ctx, &mm, 1, &sc, &cfg, &created));
  const OptPtr o(created);
  ECCKD_CHECK(opt_diagnostic_pass(o.get(), o->ray_ent, keep_negative, h_od, h_flux, [&] {
    ECCKD_CHECK(opt_launch_forward(o.get()));
    return h_planck_hl ? ecckd_d2h(ctx, h_planck_hl, o->d_planck, ncol * nhl * ng * sizeof(double)) : ECCKD_OK;
  }));
  if (h_rayleigh_od) {
    // CkdModel::calc_rayleigh_optical_depth (ckd_model.h:242-252)
    for (size_t c = 0; c < ncol; ++c)
      for (size_t l = 0; l < nlay; ++l) {
        const double* p = scene->pressure_hl + c * nhl;
        const double moles = (p[l + 1] - p[l]) * ot::MOLES_PER_PA;
        for (size_t g = 0; g < ng; ++g)
          h_rayleigh_od[(c * nlay + l) * ng + g] = m->rayleigh_molar_scattering ? moles * m->rayleigh_molar_scattering[g] : 0.0;
      }
  }
  return ECCKD_OK;
}

int ecckd_run_ckd(ecckd_ctx* ctx, const ecckd_opt_model* m, const ecckd_opt_scene* scene, double* h_od,
                  double* h_rayleigh_od, double* h_planck_hl, double* h_flux) {
  return run_ckd_impl(ctx, m, scene, h_od, h_rayleigh_od, h_planck_hl, h_flux, 0);
}

// ---------------------------------------------------------------------------------------
// scale_lut (scale_lut.cpp:117-189) + CkdModel::scale_optical_depth (ckd_model.cpp:1151-1176)
int ecckd_scale_lut(ecckd_ctx* ctx, const ecckd_opt_model* m, int nz, const double* h_pressure_hl,
                    const double* h_temperature_hl, const double* h_vmr_fl, const int* gas_present, double mu0,
                    const double* h_flux_sums, double* h_scaling, double* const* h_molar_abs_out) {
  ECCKD_REQUIRE(ctx && m && nz > 0 && h_pressure_hl && h_temperature_hl && h_flux_sums && h_molar_abs_out,
                "ecckd_scale_lut: NULL argument");
  const int ng = m->ng, np = m->np, nt = m->nt;
  // od_best (:117-133)
  std::vector<double> od_best((size_t)nz * ng), od_total((size_t)nz * ng), scaling((size_t)nz * ng);
  for (int g = 0; g < ng; ++g) {
    double flux_top = h_flux_sums[g];
    for (int iz = 0; iz < nz; ++iz) {
      const double flux_base = h_flux_sums[(size_t)(iz + 1) * ng + g];
      od_best[(size_t)iz * ng + g] = (flux_base <= 0.0) ? -1.0 : -mu0 * std::log(flux_base / flux_top);
      flux_top = flux_base;
    }
  }
  // od_total (:137-182): the CKD model on the reference profile, plain-mean temperature (:108), no clamp
  std::vector<double> t_fl(nz);
  for (int l = 0; l < nz; ++l) t_fl[l] = 0.5 * (h_temperature_hl[l] + h_temperature_hl[l + 1]);
  ecckd_opt_scene sc;
  std::memset(&sc, 0, sizeof(sc));
  sc.ncol = 1;
  sc.nlay = nz;
  sc.pressure_hl = h_pressure_hl;
  sc.temperature_hl = h_temperature_hl;
  sc.temperature_fl = t_fl.data();
  sc.vmr_fl = h_vmr_fl;
  sc.gas_present = gas_present;
  const double mu0v[1] = {mu0};
  sc.mu0 = mu0v;
  sc.tsi = 1.0;
  ECCKD_CHECK(run_ckd_impl(ctx, m, &sc, od_total.data(), nullptr, nullptr, nullptr, 1));
  for (size_t i = 0; i < scaling.size(); ++i) scaling[i] = (od_best[i] <= 0.0) ? 1.0 : od_best[i] / od_total[i];  // :186-187
  if (h_scaling) std::memcpy(h_scaling, scaling.data(), scaling.size() * sizeof(double));
  // interp(log(pressure_fl), scaling, log_pressure_) (ckd_model.cpp:1152): per g point, linear in log p with
  // linear extrapolation outside the profile
  std::vector<double> x(nz);
  for (int l = 0; l < nz; ++l) x[l] = std::log(0.5 * (h_pressure_hl[l] + h_pressure_hl[l + 1]));
  std::vector<double> local((size_t)np * ng);
  for (int ip = 0; ip < np; ++ip) {
    const double xi = m->log_pressure[ip];
    int j = 0;
    if (nz >= 2) {
      while (j < nz - 2 && xi > x[j + 1]) ++j;
    }
    for (int g = 0; g < ng; ++g) {
      if (nz == 1) { local[(size_t)ip * ng + g] = scaling[g]; continue; }
      const double w = (xi - x[j]) / (x[j + 1] - x[j]);
      local[(size_t)ip * ng + g] = (1.0 - w) * scaling[(size_t)j * ng + g] + w * scaling[(size_t)(j + 1) * ng + g];
    }
  }
  // every gas scaled equally (:1157-1175), then held inside [min, max]
  for (int i = 0; i < m->ngas; ++i) {
    const ecckd_opt_gas& ug = m->gases[i];
    const int nconc = ug.conc_dependence == 2 ? ug.nconc : 1;
    double* out = h_molar_abs_out[i];
    ECCKD_REQUIRE(out && ug.molar_abs, "ecckd_scale_lut: gas %d has no coefficient buffer", i);
    for (int ic = 0; ic < nconc; ++ic)
      for (int it = 0; it < nt; ++it)
        for (int ip = 0; ip < np; ++ip)
          for (int g = 0; g < ng; ++g) {
            const size_t e = (((size_t)ic * nt + it) * np + ip) * ng + g;
            double v = ug.molar_abs[e] * local[(size_t)ip * ng + g];
            if (ug.min_molar_abs && ug.max_molar_abs) v = std::fmax(ug.min_molar_abs[e], std::fmin(v, ug.max_molar_abs[e]));
            out[e] = v;
          }
  }
  return ECCKD_OK;
}

}  // extern "C"

