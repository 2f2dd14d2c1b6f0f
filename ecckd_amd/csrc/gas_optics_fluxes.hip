// gas_optics_fluxes.hip - the fused call of the resident gas-optics handle: from (pressure_hl, temperature_hl, vmr_fl) in device
// memory to broadband, band and per-g fluxes and heating rates in device memory, one launch, no [ncol][nlay][ng] array and no
// host round trip.  The host step (the plan, the refusals) is gas_optics_tables.cpp; the device code shared with gas_optics.hip
// (cell_entries, chain4, planck_value) is gas_optics_device.hpp.
//
// k_gas_optics_fluxes: the work item is a (column, g point) pair and its thread walks the column's layers.  A block of 256
// threads owns max(1, 256 / ng) whole columns (with ng > 256 one column, and it loops over g in passes of 256); a bounded grid
// (3 blocks per compute unit, or ECCKD_GAS_OPTICS_FLUXES_GRID) loops over the column groups.  Per group and pass:
//   A  layers in tiles: one lane per (column, layer) cell of the tile forms the cell's entries in LDS as k_gas_optics does;
//      after a barrier every thread forms the optical depth of its (column, g) for the tile's layers - the same chains, gas
//      order and clamp - and keeps it in its own row of the context's scratch, [block][row][level][thread]: coalesced, read
//      and written by that thread only.  Shortwave: moles * rayleigh[g] beside it.
//   B  longwave: the Planck function of the half levels, k_gas_optics_planck's expression, in a second row.
//   C  the transfer, expression for expression that of k_rt_lw_gpoints, k_rt_sw_gpoints or k_rt_sw_gpoints_rayleigh
//      (lbl_fluxes.hip, lbl_rt.hpp), the flux rows in the scratch in place of those kernels' output arrays.
//   D  the sums over g: a few levels at a time every thread puts its own values into LDS (and stores the per-g outputs);
//      after a barrier one thread per (column, level[, band]) adds them over g in ascending order.  The broadband doubles go
//      to a small per-block array, from which the heating rates are formed after one more barrier.
// Nothing a column computes depends on the batch, the grid or the column's place in it, and there are no atomics.
// A, B and the heating rate are compiled without contraction (the bits of the stand-alone calls); C with the default, as
// lbl_fluxes.hip is.
// The sky instances (ecckd_gas_optics_fluxes_{lw,sw}_sky_dev with an ecckd_flux_sky that gives something) differ in A and C
// only: longwave adds the band's cloud optical depth to tau after the clamp and runs every angle down before every angle up
// from the Lambertian surface (transfer_lw_sky); two-stream takes cloud_layer of lbl_rt.hpp in the layers that have a cloud
// (transfer_sw_twostream_sky).  Rows, LDS and plan are those of the clear instance of the mode.
#include "gas_optics_device.hpp"
#include "lbl_rt.hpp"

#include <cstdlib>
#include <string>

namespace go = ecckd::gas_optics;
using ecckd::lbl::RayleighLayer; using ecckd::lbl::rayleigh_layer; using ecckd::lbl::cloud_layer; using ecckd::lbl::rayleigh_up; using ecckd::lbl::rayleigh_down;

namespace {

using go::GoModel; using go::GoCall; using go::cell_entries; using go::chain4; using go::put; using go::planck_value;

constexpr int THREADS = go::THREADS;
constexpr int LW = go::FLUX_LW, SW_DIRECT = go::FLUX_SW_DIRECT, SW_TWOSTREAM = go::FLUX_SW_TWOSTREAM;

// what the fused kernel reads of the model beyond GoModel, and of the call beyond GoCall
struct FxCall {
  const double *tpl, *planck;       // longwave: the Planck look-up table [ntp], [ntp][ng]
  const double* solar;              // shortwave: solar_irradiance [ng]
  const int* iband;                 // [ng] or NULL
  const double *cos_sza, *albedo;   // shortwave: [ncol]; albedo NULL = 0
  double* scratch;
  ecckd_flux_outputs out;
  double tsi_scaling;               // tsi / sum(ssi)
  double sec_wgt[2 * go::FLUX_MAX_ANGLES];   // longwave: [nsec] secants, then [nsec] weights (lw_angle_table)
  size_t ngroup, block_doubles;
  int ntp, nband, nsec, ncol;
  int cpb, layer_tile, passes, reduce_levels, width;
};

// what the sky instances read beside it (ecckd_flux_sky); an argument of its own, and an empty one for the clear instances,
// whose arguments so stay what they were
template <bool SKY> struct FxSky {};
template <> struct FxSky<true> {
  const double *cloud_od, *cloud_ssa, *cloud_asymmetry;   // [ncol][nlay][nband] or NULL
  const double *surface_emissivity, *skin_temperature;    // [ncol][nband], [ncol] or NULL
  int delta_eddington, nband;
};

// The optical depth of one (cell, g) from the cell's entries, as k_gas_optics forms and clamps its total, and the Rayleigh
// optical depth beside it.  MODE LW: *tau = od; SW_DIRECT: *tau = od + rayleigh_od (the Rayleigh part joins after the clamp);
// SW_TWOSTREAM: *tau = od, *ray = rayleigh_od.
template <int MODE>
__device__ inline void cell_optical_depth(const GoModel& m, uint32_t present, const double* coef, const uint32_t* idx, double moles,
                                          unsigned g, double* tau, double* ray) {
#pragma clang fp contract(off)
  const double* kg = m.k + g;
  double total = 0.0;
  for (int i = 0; i < m.ngas; ++i) {
    double part = 0.0;
    if ((present >> i) & 1u) {
      const int e0 = m.gases[i].ent0;
      part = chain4(kg, coef + e0, idx + e0, part);
      if (m.gases[i].nent == 8) part = chain4(kg, coef + e0 + 4, idx + e0 + 4, part);
      total += part;
    }
  }
  total = total < 0.0 ? 0.0 : total;
  if (MODE == LW) { *tau = total; return; }
  const double r = m.rayleigh ? moles * m.rayleigh[g] : 0.0;
  if (MODE == SW_DIRECT) *tau = total + r;
  else { *tau = total; *ray = r; }
}

__device__ inline double incoming_value(double tsi_scaling, double ssi) {
#pragma clang fp contract(off)
  return tsi_scaling * ssi;
}

// heating_rate_single (heating_rate.h:55-72): conv * (dn[l+1] - dn[l] - up[l+1] + up[l]), left to right
__device__ inline double heating_rate_value(double p0, double p1, double dn0, double dn1, double up0, double up1) {
#pragma clang fp contract(off)
  const double conv = -(ECCKD_ACCEL_GRAVITY / ECCKD_SPECIFIC_HEAT_AIR) / (p1 - p0);
  return conv * (dn1 - dn0 - up1 + up0);
}

// k_rt_lw_gpoints per thread: tau, pl, fd, fu are the thread's rows (stride THREADS doubles per level)
__device__ inline void transfer_lw(int nlay, int nsec, const double* sec_wgt, const double* tau, const double* pl, double* fd, double* fu) {
  constexpr size_t ng = THREADS;   // the stride of a row, where k_rt_lw_gpoints has ng
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

// k_rt_sw_gpoints per thread
__device__ inline void transfer_sw_direct(int nlay, double mu0, double albedo, double incoming, const double* tau, double* fd, double* fu) {
  constexpr size_t ng = THREADS;
  double f = mu0 * incoming;
  fd[0] = f;
  for (int l = 0; l < nlay; ++l) { f = f * exp(-tau[(size_t)l * ng] / mu0); fd[(size_t)(l + 1) * ng] = f; }
  f = f * albedo;
  fu[(size_t)nlay * ng] = f;
  for (int l = nlay - 1; l >= 0; --l) { f = f * exp(-2.0 * tau[(size_t)l * ng]); fu[(size_t)l * ng] = f; }
}

// k_rt_sw_gpoints_rayleigh per thread: the three flux rows hold the per-level state between the sweeps, as there
__device__ inline void transfer_sw_twostream(int nlay, double mu0, double minus_sec_sza, double albedo, double incoming, const double* tau_abs,
                                             const double* tau_ray, double* fdir, double* fd, double* fu) {
  constexpr size_t ng = THREADS;
  double f = mu0 * incoming;
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

// transfer_lw over a Lambertian surface of emissivity eps and Planck function b_skin: every angle's down sweep first, then
// every angle's up sweep from eps * b_skin + (1 - eps) * dn[nlay] with dn[nlay] the angle-summed flux (optimize.hip's coupling
// of its angle form; with one angle the reference's own surface line).  The sweeps' expressions and the order in which the
// angles are added are transfer_lw's.
__device__ inline void transfer_lw_sky(int nlay, int nsec, const double* sec_wgt, double eps, double b_skin, const double* tau, const double* pl,
                                       double* fd, double* fu) {
  constexpr size_t ng = THREADS;
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
  }
  const double surface = eps * b_skin + (1.0 - eps) * fd[(size_t)nlay * ng];
  for (int a = 0; a < nsec; ++a) {
    const double sec = sec_wgt[a], w = sec_wgt[nsec + a];
    double f = surface;
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

// The cloud of one (cell, band) as the layer takes it: false where cloud_od is not > 0 (the clear layer), else the triple,
// delta-Eddington scaled here where the call asks for it.  Read from the small arrays in each sweep, not kept per thread.
__device__ inline bool cloud_values(const FxSky<true>& x, size_t i, double& t, double& w, double& a) {
  t = x.cloud_od[i];
  if (!(t > 0.0)) return false;
  w = x.cloud_ssa[i];
  a = x.cloud_asymmetry[i];
  if (x.delta_eddington) {
    const double f = a * a;
    t = t * (1.0 - w * f);
    a = a / (1.0 + a);
    w = w * (1.0 - f) / (1.0 - w * f);
  }
  return true;
}

__device__ inline RayleighLayer sky_layer(const FxSky<true>& x, size_t i, double tau_abs, double tau_ray, double mu0, double minus_sec_sza) {
  double t, w, a;
  if (!cloud_values(x, i, t, w, a)) return rayleigh_layer(tau_abs, tau_ray, mu0, minus_sec_sza);
  return cloud_layer(tau_abs, tau_ray, t, w, a, mu0, minus_sec_sza);
}

// transfer_sw_twostream with the cloud of the thread's band in the layers that have one; cloud0 = (col * nlay) * nband + band
// is the thread's first cloud value, the next layer's nband further on
__device__ inline void transfer_sw_twostream_sky(const FxSky<true>& x, size_t cloud0, int nlay, double mu0, double minus_sec_sza, double albedo,
                                                 double incoming, const double* tau_abs, const double* tau_ray, double* fdir, double* fd,
                                                 double* fu) {
  constexpr size_t ng = THREADS;
  const size_t nband = (size_t)x.nband;
  double f = mu0 * incoming;
  fdir[0] = f;
  for (int l = 0; l < nlay; ++l) {
    double t, w, a;
    if (cloud_values(x, cloud0 + (size_t)l * nband, t, w, a))
      f = f * exp(minus_sec_sza * (tau_abs[(size_t)l * ng] + tau_ray[(size_t)l * ng] + t));
    else
      f = f * exp(minus_sec_sza * (tau_abs[(size_t)l * ng] + tau_ray[(size_t)l * ng]));
    fdir[(size_t)(l + 1) * ng] = f;
  }
  double a = albedo, src = albedo * f;
  fd[(size_t)nlay * ng] = a;
  fu[(size_t)nlay * ng] = src;
  for (int l = nlay - 1; l >= 0; --l) {
    const RayleighLayer L = sky_layer(x, cloud0 + (size_t)l * nband, tau_abs[(size_t)l * ng], tau_ray[(size_t)l * ng], mu0, minus_sec_sza);
    rayleigh_up(L, fdir[(size_t)l * ng], a, src, a, src);
    fd[(size_t)l * ng] = a;
    fu[(size_t)l * ng] = src;
  }
  double diffuse = 0.0, flux_up = src;
  fd[0] = diffuse + fdir[0];
  for (int l = 0; l < nlay; ++l) {
    const RayleighLayer L = sky_layer(x, cloud0 + (size_t)l * nband, tau_abs[(size_t)l * ng], tau_ray[(size_t)l * ng], mu0, minus_sec_sza);
    rayleigh_down(L, fdir[(size_t)l * ng], fd[(size_t)(l + 1) * ng], fu[(size_t)(l + 1) * ng], diffuse, diffuse, flux_up);
    fd[(size_t)(l + 1) * ng] = diffuse + fdir[(size_t)(l + 1) * ng];
    fu[(size_t)(l + 1) * ng] = flux_up;
  }
}

// the state rows of a mode (gas_optics_tables.hpp flux_state_rows): which row holds what
template <int MODE> struct Rows;
template <> struct Rows<LW> { static constexpr int N = 4, TAU = 0, PL = 1, DN = 2, UP = 3, RAY = -1, DIR = -1; };
template <> struct Rows<SW_DIRECT> { static constexpr int N = 3, TAU = 0, DN = 1, UP = 2, PL = -1, RAY = -1, DIR = -1; };
template <> struct Rows<SW_TWOSTREAM> { static constexpr int N = 5, TAU = 0, RAY = 1, DIR = 2, DN = 3, UP = 4, PL = -1; };

// SKY: the instances of ecckd_gas_optics_fluxes_{lw,sw}_sky_dev (longwave and two-stream; the state rows are the clear ones)
template <int MODE, bool F32, bool SKY>
__global__ __launch_bounds__(THREADS) void k_gas_optics_fluxes(const GoModel m, const GoCall c, const FxCall x, const FxSky<SKY> sky) {
  using R = Rows<MODE>;
  static_assert(R::N == go::flux_state_rows(MODE), "state rows");
  static_assert(!SKY || MODE != SW_DIRECT, "the direct-beam mode has no sky instance");
  extern __shared__ double s_mem[];
  const int nent = m.nent, ng = m.ng, nlay = c.nlay, nhl = nlay + 1;
  const int cpb = x.cpb, LT = x.layer_tile, width = x.width;
  const size_t cells = (size_t)cpb * LT;
  double* s_coef = s_mem;                                         // [cells][nent]
  double* s_moles = s_coef + cells * nent;                        // [cells]
  double* s_red = s_moles + cells;                                // [reduce_levels][width]
  uint32_t* s_idx = (uint32_t*)(s_red + (size_t)x.reduce_levels * width);   // [cells][nent]
  const unsigned t = threadIdx.x;
  double* const rows = x.scratch + (size_t)blockIdx.x * x.block_doubles;    // [pass][row][level][thread]
  const size_t pass_doubles = (size_t)R::N * nhl * THREADS;
  double* const bb = rows + (size_t)x.passes * pass_doubles;      // [2][cpb][nhl] broadband dn, up
  const bool one_pass = ng <= THREADS;
  const unsigned ci = one_pass ? t / (unsigned)ng : 0u;           // the thread's column of the group

  for (size_t grp = blockIdx.x; grp < x.ngroup; grp += gridDim.x) {
    const size_t col0 = grp * (size_t)cpb;
    const unsigned ncg = (unsigned)((size_t)x.ncol - col0 < (size_t)cpb ? (size_t)x.ncol - col0 : (size_t)cpb);
    const size_t col = col0 + ci;
    for (int pass = 0; pass < x.passes; ++pass) {
      const unsigned g = one_pass ? t % (unsigned)ng : (unsigned)pass * THREADS + t;
      const bool live = ci < ncg && g < (unsigned)ng && (one_pass ? t < (unsigned)cpb * (unsigned)ng : true);
      double* const my = rows + (size_t)pass * pass_doubles + t;  // row r, level l: my[((size_t)r * nhl + l) * THREADS]
      auto row = [&](int r) { return my + (size_t)r * nhl * THREADS; };
      // (sky) the thread's first cloud value, [col][layer 0][band of g]; the next layer's is nband further on
      size_t band = 0, cloud0 = 0;
      if constexpr (SKY) {
        band = live && x.iband ? (size_t)x.iband[g] : 0;
        cloud0 = col * (size_t)nlay * (size_t)sky.nband + band;
      }
      // ---- A: optical depths, a tile of layers at a time
      for (int l0 = 0; l0 < nlay; l0 += LT) {
        const unsigned ln = (unsigned)(nlay - l0 < LT ? nlay - l0 : LT);
        __syncthreads();                                          // the LDS of the tile (or of the reduction) before is done with
        if (t < ncg * ln) {
          const unsigned cc = t / ln, li = t % ln;
          cell_entries(m, c, (col0 + cc) * (size_t)nlay + (size_t)(l0 + li), s_coef + (size_t)t * nent, s_idx + (size_t)t * nent, s_moles + t);
        }
        __syncthreads();
        if (live)
          for (unsigned li = 0; li < ln; ++li) {
            const size_t cl = (size_t)ci * ln + li;
            double* tau = row(R::TAU) + (size_t)(l0 + li) * THREADS;
            double* ray = MODE == SW_TWOSTREAM ? row(R::RAY) + (size_t)(l0 + li) * THREADS : nullptr;
            cell_optical_depth<MODE>(m, c.present, s_coef + cl * nent, s_idx + cl * nent, s_moles[cl], g, tau, ray);
            if constexpr (SKY && MODE == LW)
              if (sky.cloud_od) {                                 // the absorption optical depth of the band's cloud joins after the clamp
                const double cloud = sky.cloud_od[cloud0 + (size_t)(l0 + li) * (size_t)sky.nband];
                if (cloud > 0.0) *tau = *tau + cloud;
              }
          }
      }
      if (live) {
        if (MODE == LW) {
          // ---- B: the Planck function at the half levels
          const double* T = c.t_hl + col * (size_t)nhl;
          double* pl = row(R::PL);
          for (int l = 0; l < nhl; ++l) pl[(size_t)l * THREADS] = planck_value(x.ntp, x.tpl, x.planck, ng, g, T[l]);
          // ---- C
          if constexpr (SKY) {
            const double eps = sky.surface_emissivity ? sky.surface_emissivity[col * (size_t)sky.nband + band] : 1.0;
            const double b_skin = sky.skin_temperature ? planck_value(x.ntp, x.tpl, x.planck, ng, g, sky.skin_temperature[col]) : pl[(size_t)nlay * THREADS];
            transfer_lw_sky(nlay, x.nsec, x.sec_wgt, eps, b_skin, row(R::TAU), pl, row(R::DN), row(R::UP));
          } else {
            transfer_lw(nlay, x.nsec, x.sec_wgt, row(R::TAU), pl, row(R::DN), row(R::UP));
          }
        } else {
          const double mu0 = x.cos_sza[col], albedo = x.albedo ? x.albedo[col] : 0.0;
          if (!(mu0 > 0.0)) {                                     // no sun: zeros in every output
            for (int l = 0; l < nhl; ++l) {
              row(R::DN)[(size_t)l * THREADS] = 0.0;
              row(R::UP)[(size_t)l * THREADS] = 0.0;
              if (MODE == SW_TWOSTREAM) row(R::DIR)[(size_t)l * THREADS] = 0.0;
            }
          } else {
            const double incoming = incoming_value(x.tsi_scaling, x.solar[g]);
            if (MODE == SW_DIRECT) transfer_sw_direct(nlay, mu0, albedo, incoming, row(R::TAU), row(R::DN), row(R::UP));
            else if constexpr (SKY) transfer_sw_twostream_sky(sky, cloud0, nlay, mu0, -1.0 / mu0, albedo, incoming, row(R::TAU), row(R::RAY), row(R::DIR), row(R::DN), row(R::UP));
            else transfer_sw_twostream(nlay, mu0, -1.0 / mu0, albedo, incoming, row(R::TAU), row(R::RAY), row(R::DIR), row(R::DN), row(R::UP));
          }
        }
      }
    }
    // ---- D: per-g outputs and the sums over g, reduce_levels levels at a time
    const int nq = MODE == SW_TWOSTREAM ? 3 : 2;
    for (int q = 0; q < nq; ++q) {
      const int r = q == 0 ? R::DN : (q == 1 ? R::UP : R::DIR);
      void* const o_bb = q == 0 ? x.out.flux_dn : (q == 1 ? x.out.flux_up : x.out.flux_dn_direct);
      void* const o_band = q == 0 ? x.out.band_flux_dn : (q == 1 ? x.out.band_flux_up : x.out.band_flux_dn_direct);
      void* const o_spec = q == 0 ? x.out.spectral_flux_dn : (q == 1 ? x.out.spectral_flux_up : x.out.spectral_flux_dn_direct);
      if (q == 2 && !o_bb && !o_band && !o_spec) continue;       // (uniform over the block)
      const bool sums = q < 2 || o_bb || o_band;
      for (int L0 = 0; L0 < nhl; L0 += x.reduce_levels) {
        const int rn = nhl - L0 < x.reduce_levels ? nhl - L0 : x.reduce_levels;
        __syncthreads();
        for (int pass = 0; pass < x.passes; ++pass) {
          const unsigned g = one_pass ? t % (unsigned)ng : (unsigned)pass * THREADS + t;
          const bool live = ci < ncg && g < (unsigned)ng && (one_pass ? t < (unsigned)cpb * (unsigned)ng : true);
          if (!live) continue;
          const double* v = rows + (size_t)pass * pass_doubles + t + ((size_t)r * nhl + L0) * THREADS;
          const unsigned slot = one_pass ? t : g;
          for (int k = 0; k < rn; ++k) {
            const double f = v[(size_t)k * THREADS];
            s_red[(size_t)k * width + slot] = f;
            if (o_spec) put<F32>(o_spec, (col * (size_t)nhl + (size_t)(L0 + k)) * (size_t)ng + g, f);
          }
        }
        __syncthreads();
        if (!sums) continue;
        const unsigned per_level = 1u + (o_band ? (unsigned)x.nband : 0u);
        const unsigned ntask = ncg * (unsigned)rn * per_level;
        for (unsigned task = t; task < ntask; task += THREADS) {
          const unsigned b = task % per_level, k = (task / per_level) % (unsigned)rn, cc = task / (per_level * (unsigned)rn);
          const double* v = s_red + (size_t)k * width + (one_pass ? (size_t)cc * ng : 0);
          const size_t lev = (col0 + cc) * (size_t)nhl + (size_t)(L0 + k);
          double sum = 0.0;
          if (b == 0) {
            for (int g = 0; g < ng; ++g) sum += v[g];
            if (o_bb) put<F32>(o_bb, lev, sum);
            if (q < 2) bb[((size_t)q * cpb + cc) * nhl + (size_t)(L0 + k)] = sum;
          } else {
            const int band = (int)b - 1;
            for (int g = 0; g < ng; ++g)
              if (x.iband[g] == band) sum += v[g];
            put<F32>(o_band, lev * (size_t)x.nband + (size_t)band, sum);
          }
        }
      }
    }
    if (x.out.heating_rate) {
      __syncthreads();                                            // the broadband doubles of the group are in place
      const unsigned ntask = ncg * (unsigned)nlay;
      for (unsigned task = t; task < ntask; task += THREADS) {
        const unsigned cc = task / (unsigned)nlay, l = task % (unsigned)nlay;
        const double* p = c.p_hl + (col0 + cc) * (size_t)nhl;
        const double* dn = bb + (size_t)cc * nhl;
        const double* up = bb + ((size_t)cpb + cc) * nhl;
        put<F32>(x.out.heating_rate, (col0 + cc) * (size_t)nlay + l, heating_rate_value(p[l], p[l + 1], dn[l], dn[l + 1], up[l], up[l + 1]));
      }
    }
    __syncthreads();                                              // bb and the LDS are free for the next group
  }
}

template <int MODE, bool F32, bool SKY = false>
int launch(ecckd_gas_optics* h, const ecckd_flux_plan& plan, const GoModel& m, const GoCall& c, const FxCall& x, const FxSky<SKY>& sky = {}) {
  const auto kernel = k_gas_optics_fluxes<MODE, F32, SKY>;
  if (plan.lds_bytes > 48 * 1024)
    ECCKD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes));
  hipLaunchKernelGGL(kernel, dim3(plan.grid), dim3(plan.threads), plan.lds_bytes, h->ctx->stream, m, c, x, sky);
  ECCKD_HIP_CHECK(hipGetLastError());
  return ECCKD_OK;
}

long long grid_override() {
  if (const char* e = std::getenv("ECCKD_GAS_OPTICS_FLUXES_GRID")) {
    const long long v = std::atoll(e);
    if (v >= 1) return v;
  }
  return 0;
}

int fluxes(ecckd_gas_optics* h, const go::FluxCallArgs& a, const double* d_pressure_hl, const double* d_temperature_hl,
           const double* d_temperature_fl, const double* d_vmr_fl, const double* h_gas_scaling, const double* d_cos_sza, const double* d_albedo,
           double tsi) {
  const go::Flat& f = h->f;
  std::string err;
  uint32_t present = 0;
  int mode = 0;
  unsigned wants = 0;
  ecckd_flux_plan plan{};
  bool sky = false;
  int rc = go::check_fluxes_call(f, a, present, mode, wants, err);
  if (rc == ECCKD_OK) rc = go::check_fluxes_sky(f, a, sky, err);
  if (rc == ECCKD_OK)
    rc = go::fluxes_plan(a.ncol, a.nlay, f.ng, f.nent, f.nband, mode, a.nangle, wants, std::max(h->ctx->num_cu, 1), grid_override(), plan, err);
  if (rc != ECCKD_OK) return ecckd::fail(rc, "%s", err.c_str());
  const GoModel m = {h->d_k, h->d_temperature, h->d_rayleigh, h->d_gases, f.log_p_0, f.d_log_p, f.d_t, f.ng, f.nt, f.np, f.ngas, f.nent};
  GoCall c{};
  c.p_hl = d_pressure_hl; c.t_hl = d_temperature_hl; c.t_fl = d_temperature_fl; c.vmr = d_vmr_fl;
  for (int i = 0; i < f.ngas; ++i) c.scaling[i] = h_gas_scaling ? h_gas_scaling[i] : 1.0;
  c.ncell = (size_t)a.ncol * (size_t)a.nlay; c.present = present; c.nlay = a.nlay; c.keep_negative = 0;
  FxCall x{};
  x.tpl = h->d_tpl; x.planck = h->d_planck; x.solar = h->d_solar; x.iband = h->d_iband;
  x.cos_sza = d_cos_sza; x.albedo = d_albedo;
  x.out = *a.out;
  x.ntp = f.ntp; x.nband = f.nband; x.ncol = a.ncol;
  if (mode == LW) {
    std::vector<double> sec_wgt;
    ECCKD_CHECK(ecckd::lbl::lw_angle_table(a.sky_call ? "ecckd_gas_optics_fluxes_lw_sky_dev" : "ecckd_gas_optics_fluxes_lw_dev", a.nangle, &x.nsec, sec_wgt));
    std::copy(sec_wgt.begin(), sec_wgt.end(), x.sec_wgt);
  } else {
    x.tsi_scaling = go::incoming_scaling(f, tsi);
  }
  x.ngroup = plan.ngroup;
  x.block_doubles = plan.scratch_bytes / plan.grid / sizeof(double);
  x.cpb = plan.columns_per_block; x.layer_tile = plan.layer_tile; x.passes = plan.g_passes; x.reduce_levels = plan.reduce_levels;
  x.width = f.ng <= THREADS ? THREADS : f.ng;
  ECCKD_HIP_CHECK(hipSetDevice(h->ctx->device));
  void* d[1];
  ECCKD_CHECK(ecckd::carve_scratch(h->ctx, {plan.scratch_bytes}, d));
  x.scratch = (double*)d[0];
  const bool f32 = a.out_type == ECCKD_F32;
  if (sky) {                                                      // (without a sky pointer the call is the clear call: the clear instance)
    const FxSky<true> s = {a.sky->cloud_od, a.sky->cloud_ssa, a.sky->cloud_asymmetry, a.sky->surface_emissivity, a.sky->skin_temperature,
                           a.sky->delta_eddington, f.nband};
    if (mode == LW) return f32 ? launch<LW, true, true>(h, plan, m, c, x, s) : launch<LW, false, true>(h, plan, m, c, x, s);
    return f32 ? launch<SW_TWOSTREAM, true, true>(h, plan, m, c, x, s) : launch<SW_TWOSTREAM, false, true>(h, plan, m, c, x, s);
  }
  if (mode == LW) return f32 ? launch<LW, true>(h, plan, m, c, x) : launch<LW, false>(h, plan, m, c, x);
  if (mode == SW_DIRECT) return f32 ? launch<SW_DIRECT, true>(h, plan, m, c, x) : launch<SW_DIRECT, false>(h, plan, m, c, x);
  return f32 ? launch<SW_TWOSTREAM, true>(h, plan, m, c, x) : launch<SW_TWOSTREAM, false>(h, plan, m, c, x);
}

}  // namespace

extern "C" {

int ecckd_gas_optics_fluxes_lw_dev(ecckd_gas_optics* h, int nangle, int ncol, int nlay, const double* d_pressure_hl,
                                   const double* d_temperature_hl, const double* d_temperature_fl, const double* d_vmr_fl,
                                   const int* h_gas_present, const double* h_gas_scaling, int out_type, const ecckd_flux_outputs* out) {
  ECCKD_REQUIRE(h, "ecckd_gas_optics_fluxes_lw_dev: handle is NULL");
  const go::FluxCallArgs a = {false, nangle, 0, ncol, nlay, d_pressure_hl != nullptr, d_temperature_hl != nullptr, d_vmr_fl != nullptr, false,
                              h_gas_present, out_type, out};
  return fluxes(h, a, d_pressure_hl, d_temperature_hl, d_temperature_fl, d_vmr_fl, h_gas_scaling, nullptr, nullptr, 0.0);
}

int ecckd_gas_optics_fluxes_sw_dev(ecckd_gas_optics* h, int scattering, int ncol, int nlay, const double* d_pressure_hl,
                                   const double* d_temperature_hl, const double* d_temperature_fl, const double* d_vmr_fl,
                                   const int* h_gas_present, const double* h_gas_scaling, const double* d_cos_sza, const double* d_albedo,
                                   double tsi, int out_type, const ecckd_flux_outputs* out) {
  ECCKD_REQUIRE(h, "ecckd_gas_optics_fluxes_sw_dev: handle is NULL");
  const go::FluxCallArgs a = {true, 0, scattering, ncol, nlay, d_pressure_hl != nullptr, d_temperature_hl != nullptr, d_vmr_fl != nullptr,
                              d_cos_sza != nullptr, h_gas_present, out_type, out};
  return fluxes(h, a, d_pressure_hl, d_temperature_hl, d_temperature_fl, d_vmr_fl, h_gas_scaling, d_cos_sza, d_albedo, tsi);
}

int ecckd_gas_optics_fluxes_lw_sky_dev(ecckd_gas_optics* h, int nangle, int ncol, int nlay, const double* d_pressure_hl,
                                       const double* d_temperature_hl, const double* d_temperature_fl, const double* d_vmr_fl,
                                       const int* h_gas_present, const double* h_gas_scaling, int out_type, const ecckd_flux_outputs* out,
                                       const ecckd_flux_sky* sky) {
  ECCKD_REQUIRE(h, "ecckd_gas_optics_fluxes_lw_sky_dev: handle is NULL");
  const go::FluxCallArgs a = {false, nangle, 0, ncol, nlay, d_pressure_hl != nullptr, d_temperature_hl != nullptr, d_vmr_fl != nullptr, false,
                              h_gas_present, out_type, out, true, sky};
  return fluxes(h, a, d_pressure_hl, d_temperature_hl, d_temperature_fl, d_vmr_fl, h_gas_scaling, nullptr, nullptr, 0.0);
}

int ecckd_gas_optics_fluxes_sw_sky_dev(ecckd_gas_optics* h, int ncol, int nlay, const double* d_pressure_hl, const double* d_temperature_hl,
                                       const double* d_temperature_fl, const double* d_vmr_fl, const int* h_gas_present,
                                       const double* h_gas_scaling, const double* d_cos_sza, const double* d_albedo, double tsi, int out_type,
                                       const ecckd_flux_outputs* out, const ecckd_flux_sky* sky) {
  ECCKD_REQUIRE(h, "ecckd_gas_optics_fluxes_sw_sky_dev: handle is NULL");
  // (always the two-stream transfer)
  const go::FluxCallArgs a = {true, 0, 1, ncol, nlay, d_pressure_hl != nullptr, d_temperature_hl != nullptr, d_vmr_fl != nullptr,
                              d_cos_sza != nullptr, h_gas_present, out_type, out, true, sky};
  return fluxes(h, a, d_pressure_hl, d_temperature_hl, d_temperature_fl, d_vmr_fl, h_gas_scaling, d_cos_sza, d_albedo, tsi);
}

int ecckd_gas_optics_fluxes_geometry(ecckd_gas_optics* h, int nlay, int mode, int* columns_per_block, int* threads, int* layer_tile,
                                     size_t* scratch_bytes) {
  ECCKD_REQUIRE(h, "ecckd_gas_optics_fluxes_geometry: handle is NULL");
  std::string err;
  ecckd_flux_plan plan{};
  // (a saturated grid: the scratch no call of this shape exceeds)
  const int rc = go::fluxes_plan(0x7fffffffLL, nlay, h->f.ng, h->f.nent, h->f.nband, mode, 0, go::WANT_BROADBAND, std::max(h->ctx->num_cu, 1),
                                 grid_override(), plan, err);
  if (rc != ECCKD_OK) return ecckd::fail(rc, "%s", err.c_str());
  if (columns_per_block) *columns_per_block = plan.columns_per_block;
  if (threads) *threads = plan.threads;
  if (layer_tile) *layer_tile = plan.layer_tile;
  if (scratch_bytes) *scratch_bytes = plan.scratch_bytes;
  return ECCKD_OK;
}

}  // extern "C"
