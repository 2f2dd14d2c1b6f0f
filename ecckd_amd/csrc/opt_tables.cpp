// opt_tables.cpp - see opt_tables.hpp.  Every floating-point expression keeps the operand order it had inside ecckd_opt_create,
// so the tables are the same bits.
#include "opt_tables.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>

namespace ecckd {
namespace opt_tables {

namespace {

int refuse(std::string& err, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  err = buf;
  return ECCKD_PARAMETER_ERROR;
}

int count_bands(const ecckd_opt_model* m) {
  int nband = 0;
  for (int g = 0; g < m->ng; ++g) nband = std::max(nband, m->iband_per_g[g] + 1);
  return nband;
}

// user gas indices in k order: active gases first (they are the state x), then fixed gases
std::vector<int> gas_order(const ecckd_opt_model* m) {
  std::vector<int> order;
  for (int a = 1; a >= 0; --a)
    for (int i = 0; i < m->ngas; ++i)
      if ((m->gases[i].is_active != 0) == (a == 1)) order.push_back(i);
  return order;
}

int nconc_of(const ecckd_opt_gas& ug) { return ug.conc_dependence == 2 ? ug.nconc : 1; }

bool has_rayleigh(const ecckd_opt_model* m) { return m->solar_irradiance && m->rayleigh_molar_scattering; }

// the scene brings spectral boundary fluxes (SW: with their per-g weights)
bool has_boundary(const ecckd_opt_scene& sc, bool do_sw) {
  return sc.spectral_flux_dn_surf && (do_sw ? sc.spectral_boundary_weights != nullptr : sc.spectral_flux_up_toa != nullptr);
}

bool has_relative(const ecckd_opt_scene& sc) { return sc.relative_flux_dn && sc.relative_flux_up; }

// per-dimension tridiagonal of an AR(1) inverse
struct Tri { std::vector<double> lo, di, up; };

Tri ar1_inverse(int n, double rho) {
  Tri t;
  t.lo.assign(n, 0.0); t.di.assign(n, 1.0); t.up.assign(n, 0.0);
  if (n == 1) return t;
  const double den = 1.0 - rho * rho;
  for (int i = 0; i < n; ++i) {
    t.di[i] = ((i == 0 || i == n - 1) ? 1.0 : 1.0 + rho * rho) / den;
    if (i > 0) t.lo[i] = -rho / den;
    if (i < n - 1) t.up[i] = -rho / den;
  }
  return t;
}

// CkdModel::calc_planck_function, ckd_model.cpp:1121-1145
void planck_lut(int ntp, const double* tpl, const double* pf, int ng, double t, double* out) {
  const double d_t = tpl[1] - tpl[0], t0 = tpl[0];
  const double tindex0 = (t - t0) / d_t;
  if (tindex0 >= 0) {
    int it0 = std::min((int)tindex0, ntp - 2);
    const double w1 = tindex0 - it0, w0 = 1.0 - w1;
    for (int g = 0; g < ng; ++g) out[g] = w0 * pf[(size_t)it0 * ng + g] + w1 * pf[(size_t)(it0 + 1) * ng + g];
  } else {
    for (int g = 0; g < ng; ++g) out[g] = (t / t0) * pf[g];
  }
}

// background_error per g estimated from min/max (ckd_model.cpp:679-745)
void estimate_sigma(const ecckd_opt_config& cfg, const Tables& t, GasInfo& gi) {
  for (int g = 0; g < t.ng; ++g) {
    double local_sum = 0.0;
    int local_count = 0;
    for (size_t nd = 0; nd < gi.nnode; ++nd) {
      const size_t e = gi.ix + nd * t.ng + g;
      if (t.k0[e] > 0.0) {
        if (t.kmin[e] > 0.0) local_sum += 0.25 * std::log(t.kmax[e] / t.kmin[e]);
        else local_sum += 0.5 * std::log(t.kmax[e] / t.k0[e]);
        ++local_count;
      }
    }
    if (local_count > 0) gi.sigma[g] = cfg.prior_error_scaling * local_sum / local_count;
  }
  if (cfg.min_prior_error > 0.0) for (double& sg : gi.sigma) sg = std::max(cfg.min_prior_error, sg);
  if (cfg.max_prior_error > 0.0) for (double& sg : gi.sigma) sg = std::min(sg, cfg.max_prior_error);
}

// position on one evenly spaced LUT axis of n nodes, held inside it: lower node and the weight of the upper one
struct AxisPos { int i0; double w0, w1; };
AxisPos axis_pos(double index0, int n) {
  index0 = std::fmax(0.0, std::fmin(index0, n - 1.0001));
  const int i0 = (int)index0;
  const double w1 = index0 - i0;
  return {i0, 1.0 - w1, w1};
}

}  // namespace

int check_model_shape(const ecckd_opt_model* m, const char* who, std::string& err) {
  if (!(m->ng > 0 && m->ng <= 1024 && m->nt >= 2 && m->np >= 2 && m->ngas > 0 && m->gases && m->log_pressure && m->temperature &&
        m->iband_per_g))
    return refuse(err, "%s: bad model dimensions (ng=%d nt=%d np=%d ngas=%d)", who, m->ng, m->nt, m->np, m->ngas);
  const bool do_sw = m->solar_irradiance != nullptr;
  if (!(do_sw || (m->ntp >= 2 && m->temperature_planck && m->planck_function)))
    return refuse(err, "%s: Planck look-up table missing", who);
  if (m->logarithmic_interpolation)
    return refuse(err, "%s: logarithmic LUT interpolation is not supported (ckd_model.h:359 default is linear)", who);
  return ECCKD_OK;
}

int check_model_gases(const ecckd_opt_model* m, const char* who, std::string& err, size_t& ncoef) {
  ncoef = 0;
  for (int i : gas_order(m)) {
    const ecckd_opt_gas& ug = m->gases[i];
    if (!(ug.conc_dependence >= 0 && ug.conc_dependence <= 3) || !ug.molar_abs ||
        (ug.conc_dependence == 2 && (ug.nconc < 2 || !ug.vmr)))
      return refuse(err, "%s: gas %d is ill-defined", who, i);
    ncoef += (size_t)nconc_of(ug) * m->nt * m->np * m->ng;
  }
  return ECCKD_OK;
}

int check_arguments(const ecckd_opt_model* m, int nscene, const ecckd_opt_scene* scenes, const ecckd_opt_config* cfg, std::string& err,
                    bool rayleigh_active) {
  const char* who = "ecckd_opt_create";
  if (!(m && scenes && cfg && nscene > 0)) return refuse(err, "%s: NULL/empty argument", who);
  int rc = check_model_shape(m, who, err);
  if (rc != ECCKD_OK) return rc;
  const bool do_sw = m->solar_irradiance != nullptr;
  if (rayleigh_active && !has_rayleigh(m))
    return refuse(err, "ecckd_opt_create_ex: ECCKD_OPT_RAYLEIGH_ACTIVE needs a shortwave model with rayleigh_molar_scattering");
  size_t ncoef = 0;
  rc = check_model_gases(m, who, err, ncoef);
  if (rc != ECCKD_OK) return rc;
  size_t nx = rayleigh_active ? m->ng : 0;
  const size_t nk = ncoef + (has_rayleigh(m) ? m->ng : 0);
  for (int i = 0; i < m->ngas; ++i)
    if (m->gases[i].is_active) nx += (size_t)nconc_of(m->gases[i]) * m->nt * m->np * m->ng;
  if (!(nx > 0)) return refuse(err, "%s: no active gas to optimise", who);
  if (!(nk < (size_t)0x7fffffff)) return refuse(err, "%s: coefficient vector too long for int32 indexing", who);
  const int nlay = scenes[0].nlay, nband = count_bands(m);
  if (nlay < 1 || nlay > 128) return refuse(err, "ecckd_opt_create: nlay = %d outside the supported range 1..128", nlay);
  for (int s = 0; s < nscene; ++s)
    if (scenes[s].nlay != nlay || scenes[s].ncol <= 0 || !scenes[s].pressure_hl || !scenes[s].temperature_hl ||
        !scenes[s].flux_dn || !scenes[s].flux_up || scenes[s].nband != nband ||
        (do_sw && (!scenes[s].mu0 || !scenes[s].albedo || !(scenes[s].tsi > 0.0))))
      return refuse(err, "ecckd_opt_create: scene %d is inconsistent (nlay/nband/arrays)", s);
  return ECCKD_OK;
}

void order_gases(const ecckd_opt_model* m, Tables& t) {
  const int ng = t.ng = m->ng;
  t.nt = m->nt; t.np = m->np; t.ngas = m->ngas;
  t.do_sw = m->solar_irradiance != nullptr;
  t.nband = count_bands(m);
  t.grad_nchunk = (ng + 63) / 64;
  t.order = gas_order(m);
  t.user_to_k.assign(m->ngas, -1);
  size_t off = 0;
  bool rayleigh_placed = false;
  // rayleigh_active: the Rayleigh row directly behind the last active gas, so that x[e] <-> k[e] holds for the whole state
  auto place_rayleigh = [&] {
    t.rayleigh_ix = off;
    off += ng;
    t.nx = off;
    rayleigh_placed = true;
  };
  for (size_t pos = 0; pos < t.order.size(); ++pos) {
    const ecckd_opt_gas& ug = m->gases[t.order[pos]];
    if (t.rayleigh_active && !rayleigh_placed && !ug.is_active) place_rayleigh();
    GasInfo gi;
    gi.conc = ug.conc_dependence;
    gi.active = ug.is_active != 0;
    gi.nconc = nconc_of(ug);
    gi.nnode = (size_t)gi.nconc * t.nt * t.np;
    gi.ix = off;
    gi.reference_vmr = ug.reference_vmr;
    if (ug.conc_dependence == 2) gi.vmr.assign(ug.vmr, ug.vmr + ug.nconc);
    off += gi.nnode * ng;
    if (gi.active) { t.nx = off; t.nnode_active += gi.nnode; }
    t.user_to_k[t.order[pos]] = (int)pos;
    t.gases.push_back(gi);
  }
  // Rayleigh scattering (calc_total_optical_depth, solve_adept.cpp:33-36; ckd_model.h:242-252): a fixed
  // one-node pseudo gas at the end of the coefficient vector (rayleigh_active: part of the state, placed above or here)
  if (t.rayleigh_active) {
    if (!rayleigh_placed) place_rayleigh();
  } else {
    t.rayleigh_ix = off;
    if (has_rayleigh(m)) off += ng;
  }
  t.nk = off;
  t.k0.assign(t.nk, 0.0);
  t.kmin.assign(t.nx, 0.0);
  t.kmax.assign(t.nx, 0.0);
  bool have_minmax = true;
  for (size_t pos = 0; pos < t.order.size(); ++pos) {
    const ecckd_opt_gas& ug = m->gases[t.order[pos]];
    const GasInfo& gi = t.gases[pos];
    std::memcpy(&t.k0[gi.ix], ug.molar_abs, gi.nnode * ng * sizeof(double));
    if (!gi.active) continue;
    if (ug.min_molar_abs && ug.max_molar_abs) {
      std::memcpy(&t.kmin[gi.ix], ug.min_molar_abs, gi.nnode * ng * sizeof(double));
      std::memcpy(&t.kmax[gi.ix], ug.max_molar_abs, gi.nnode * ng * sizeof(double));
    } else {
      have_minmax = false;
    }
  }
  if (!have_minmax) { t.kmin.clear(); t.kmax.clear(); }
  if (has_rayleigh(m)) std::memcpy(&t.k0[t.rayleigh_ix], m->rayleigh_molar_scattering, ng * sizeof(double));
}

// cap_relative_linear_coeffts(0.8), optimize_lut.cpp:185, ckd_model.cpp:883-917
void cap_relative_linear(double cap_fraction, Tables& t) {
  int ibg = -1;
  for (size_t pos = 0; pos < t.gases.size(); ++pos)
    if (t.gases[pos].conc == 0) ibg = (int)pos;  // the LAST gas with NONE, as the reference loop leaves it
  if (ibg < 0 || !(cap_fraction > 0.0)) return;
  const GasInfo& bg = t.gases[ibg];
  for (const GasInfo& gi : t.gases) {
    if (!(gi.active && gi.conc == 3 && gi.nnode == bg.nnode)) continue;
    for (size_t e = 0; e < gi.nnode * t.ng; ++e) {
      const double cap = t.k0[bg.ix + e] / (gi.reference_vmr * cap_fraction);
      if (t.k0[gi.ix + e] * (gi.reference_vmr * cap_fraction) > t.k0[bg.ix + e]) t.k0[gi.ix + e] = std::min(t.k0[gi.ix + e], cap);
    }
  }
}

// create_error_covariances, ckd_model.cpp:646-832 (the reference always adds calc_background_cost_function, :273)
void build_prior(const ecckd_opt_config& cfg, Tables& t) {
  const int ng = t.ng, nt = t.nt, np = t.np;
  t.tri_off.assign(t.gases.size(), 0);
  t.gas_dims.assign(t.gases.size() * 4, 0);
  t.inv_sigma2.assign(t.gases.size() * ng, 0.0);
  size_t node0 = 0;
  for (size_t pos = 0; pos < t.gases.size(); ++pos) {
    GasInfo& gi = t.gases[pos];
    t.gas_dims[pos * 4 + 0] = gi.nconc; t.gas_dims[pos * 4 + 1] = nt; t.gas_dims[pos * 4 + 2] = np;
    t.gas_dims[pos * 4 + 3] = (int)node0;
    if (!gi.active) continue;
    t.tri_off[pos] = (int)t.tri.size();
    const Tri tc = ar1_inverse(gi.nconc, cfg.conc_corr), tt = ar1_inverse(nt, cfg.temperature_corr), tp = ar1_inverse(np, cfg.pressure_corr);
    for (const Tri* a : {&tc, &tt, &tp}) {
      t.tri.insert(t.tri.end(), a->lo.begin(), a->lo.end());
      t.tri.insert(t.tri.end(), a->di.begin(), a->di.end());
      t.tri.insert(t.tri.end(), a->up.begin(), a->up.end());
    }
    gi.sigma.assign(ng, cfg.prior_error > 0.0 ? cfg.prior_error : 1.0);
    if (cfg.prior_error <= 0.0 && !t.kmin.empty()) estimate_sigma(cfg, t, gi);
    for (int g = 0; g < ng; ++g) t.inv_sigma2[pos * ng + g] = 1.0 / (gi.sigma[g] * gi.sigma[g]);
    for (int ic = 0; ic < gi.nconc; ++ic)
      for (int it = 0; it < nt; ++it)
        for (int ip = 0; ip < np; ++ip) {
          t.node_gas.push_back((int)pos); t.node_ic.push_back(ic); t.node_it.push_back(it); t.node_ip.push_back(ip);
        }
    node0 += gi.nnode;
  }
}

// training scenes -> flat per-profile arrays
void flatten_scenes(const ecckd_opt_model* m, int nscene, const ecckd_opt_scene* scenes, const ecckd_opt_config& cfg, Tables& t) {
  const int ng = t.ng, nband = t.nband, nlay = t.nlay = scenes[0].nlay, nhl = nlay + 1;
  const bool do_sw = t.do_sw;
  size_t ncol = 0;
  for (int s = 0; s < nscene; ++s) {
    ncol += scenes[s].ncol;
    t.have_boundary = t.have_boundary || has_boundary(scenes[s], do_sw);
  }
  t.ncol = ncol;
  t.ncell = ncol * nlay;
  t.planck.assign(ncol * nhl * ng, 0.0); t.semis.assign(ncol * nband, 1.0); t.conv.assign(ncol * nlay, 0.0); t.lw.assign(ncol * nlay, 0.0);
  t.hr.assign(ncol * nlay * nband, 0.0); t.fdn.assign(ncol * nhl * nband, 0.0); t.fup.assign(ncol * nhl * nband, 0.0);
  if (t.have_boundary) { t.sfds.assign(ncol * ng, 0.0); t.sfut.assign(ncol * ng, 0.0); }
  t.mu0.assign(do_sw ? ncol : 0, 0.0);
  double solar_sum = 0.0;
  if (do_sw)
    for (int g = 0; g < ng; ++g) solar_sum += m->solar_irradiance[g];
  size_t col = 0;
  for (int s = 0; s < nscene; ++s) {
    const ecckd_opt_scene& sc = scenes[s];
    for (int c = 0; c < sc.ncol; ++c, ++col) {
      const double* p = sc.pressure_hl + (size_t)c * nhl;
      const double* T = sc.temperature_hl + (size_t)c * nhl;
      if (!do_sw) {
        for (int i = 0; i < nhl; ++i) planck_lut(m->ntp, m->temperature_planck, m->planck_function, ng, T[i], &t.planck[(col * nhl + i) * ng]);
        if (sc.surf_emissivity) std::memcpy(&t.semis[col * nband], sc.surf_emissivity + (size_t)c * nband, nband * sizeof(double));
      } else {
        // tsi_scaling * ckd_model.solar_irradiance() (solve_adept.cpp:176,186) in row 0; band albedo
        const double tsi_scaling = sc.tsi / solar_sum;
        for (int g = 0; g < ng; ++g) t.planck[(col * nhl) * ng + g] = tsi_scaling * m->solar_irradiance[g];
        std::memcpy(&t.semis[col * nband], sc.albedo, nband * sizeof(double));
        t.mu0[col] = sc.mu0[c];
      }
      // layer weights, solve_adept.cpp:131-143
      double* lw = &t.lw[col * nlay];
      double* conv = &t.conv[col * nlay];
      double wsum = 0.0;
      for (int l = 0; l < nlay; ++l) {
        double w;
        if (cfg.pressure_weight_power == 0.5) w = std::sqrt(p[l + 1]) - std::sqrt(p[l]);
        else if (cfg.pressure_weight_power == 1.0) w = p[l + 1] - p[l];
        else w = std::pow(p[l + 1], cfg.pressure_weight_power) - std::pow(p[l], cfg.pressure_weight_power);
        lw[l] = w;
        wsum += w;
        conv[l] = -(ACCEL_GRAVITY / SPECIFIC_HEAT_AIR) / (p[l + 1] - p[l]);
      }
      for (int l = 0; l < nlay; ++l) lw[l] /= wsum;
      // truth: band fluxes and their heating rate (lbl_fluxes.cpp:380-388, heating_rate.h:30-50)
      double* d = &t.fdn[col * nhl * nband];
      double* u = &t.fup[col * nhl * nband];
      std::memcpy(d, sc.flux_dn + (size_t)c * nhl * nband, (size_t)nhl * nband * sizeof(double));
      std::memcpy(u, sc.flux_up + (size_t)c * nhl * nband, (size_t)nhl * nband * sizeof(double));
      for (int l = 0; l < nlay; ++l)
        for (int b = 0; b < nband; ++b)
          // LW: net flux divergence; SW: direct beam only (lbl_fluxes.cpp:365-369 passes an empty flux_up), unless the
          // handle scatters: then flux_dn is the total downwelling and the heating rate is the net one, as the model's
          t.hr[(col * nlay + l) * nband + b] =
              do_sw && !t.scattering
                    ? conv[l] * (d[(l + 1) * nband + b] - d[l * nband + b])
                    : conv[l] * (d[(l + 1) * nband + b] - d[l * nband + b] - u[(l + 1) * nband + b] + u[l * nband + b]);
      if (has_boundary(sc, do_sw)) {
        std::memcpy(&t.sfds[col * ng], sc.spectral_flux_dn_surf + (size_t)c * ng, ng * sizeof(double));
        // SW: the second array carries the per-g weights (calc_cost_function_sw.cpp:271-274)
        if (do_sw) std::memcpy(&t.sfut[col * ng], sc.spectral_boundary_weights, ng * sizeof(double));
        else std::memcpy(&t.sfut[col * ng], sc.spectral_flux_up_toa + (size_t)c * ng, ng * sizeof(double));
      }
    }
  }
}

// the sparse interpolation table, ckd_model.cpp:960-1086: per cell and gas the 2 x 2 (x 2) LUT nodes around the layer's
// (concentration,) temperature and pressure, each with weight * interpolation weight; a gas without a concentration axis sits
// at concentration node 0 with weight 1
void build_entries(const ecckd_opt_model* m, int nscene, const ecckd_opt_scene* scenes, Tables& t) {
  const int ng = t.ng, nt = t.nt, np = t.np, nlay = t.nlay, nhl = nlay + 1;
  const bool have_rayleigh = has_rayleigh(m);
  int nent = have_rayleigh ? 1 : 0;
  for (const GasInfo& gi : t.gases) nent += (gi.conc == 2) ? 8 : 4;
  t.ray_ent = have_rayleigh ? nent - 1 : -1;
  t.nent = nent;
  t.ent_idx.assign(t.ncell * nent, -1);
  t.ent_coef.assign(t.ncell * nent, 0.0);
  if (t.rayleigh_active) t.moles.assign(t.ncell, 0.0);
  const double log_p_0 = m->log_pressure[0];
  const double d_log_p = m->log_pressure[1] - m->log_pressure[0];
  const double d_t = m->temperature[1 * np + 0] - m->temperature[0];
  size_t col = 0;
  for (int s = 0; s < nscene; ++s) {
    const ecckd_opt_scene& sc = scenes[s];
    for (int c = 0; c < sc.ncol; ++c, ++col) {
      const double* p = sc.pressure_hl + (size_t)c * nhl;
      const double* T = sc.temperature_hl + (size_t)c * nhl;
      for (int l = 0; l < nlay; ++l) {
        int* idx = &t.ent_idx[(col * nlay + l) * nent];
        double* coef = &t.ent_coef[(col * nlay + l) * nent];
        // full-level temperature, solve_adept.cpp:38-41
        const double t_fl = sc.temperature_fl ? sc.temperature_fl[(size_t)c * nlay + l]
                                              : (T[l] * p[l] + T[l + 1] * p[l + 1]) / (p[l] + p[l + 1]);
        const double log_pressure_fl = std::log(0.5 * (p[l + 1] + p[l]));
        const AxisPos ap = axis_pos((log_pressure_fl - log_p_0) / d_log_p, np);
        const double t_0 = ap.w0 * m->temperature[ap.i0] + ap.w1 * m->temperature[ap.i0 + 1];
        const AxisPos at = axis_pos((t_fl - t_0) / d_t, nt);
        const double simple_weight = MOLES_PER_PA * (p[l + 1] - p[l]);
        int e = 0;
        for (size_t pos = 0; pos < t.gases.size(); ++pos) {
          const GasInfo& gi = t.gases[pos];
          const int ugas = t.order[pos];
          const int nc = (gi.conc == 2) ? 2 : 1;
          const bool present = sc.gas_present ? sc.gas_present[ugas] != 0 : true;
          // ckd_model.cpp:995-1004, :1066-1073 and solve_adept.cpp:47-67: a gas without a
          // concentration dependence always contributes with the dry-air weight; the others need
          // their mole fraction from the training file and are skipped when it is absent
          double weight = 0.0, vm = 0.0;
          bool use = true;
          if (gi.conc == 0) {
            weight = simple_weight;
          } else if (present && sc.vmr_fl) {
            vm = sc.vmr_fl[((size_t)c * m->ngas + ugas) * nlay + l];
            weight = (gi.conc == 3) ? simple_weight * (vm - gi.reference_vmr) : simple_weight * vm;
          } else {
            use = false;
          }
          if (use) {
            AxisPos ac = {0, 1.0, 1.0};
            if (gi.conc == 2) {
              const double log_conc = std::log(vm);
              const double d_log_c = std::log(gi.vmr[1] / gi.vmr[0]);
              ac = axis_pos((log_conc - std::log(gi.vmr[0])) / d_log_c, gi.nconc);
            }
            int q = 0;
            for (int dc = 0; dc < nc; ++dc)
              for (int dt = 0; dt < 2; ++dt)
                for (int dp = 0; dp < 2; ++dp) {
                  const size_t node = ((size_t)(ac.i0 + dc) * nt + (at.i0 + dt)) * np + (ap.i0 + dp);
                  idx[e + q] = (int)(gi.ix + node * ng);
                  coef[e + q] = weight * (dc ? ac.w1 : ac.w0) * (dt ? at.w1 : at.w0) * (dp ? ap.w1 : ap.w0);
                  ++q;
                }
          }
          e += 4 * nc;
        }
        if (have_rayleigh) {
          // moles of air per unit area in the layer (ckd_model.h:246-247) times the molar scattering
          idx[e] = (int)t.rayleigh_ix;
          coef[e] = (p[l + 1] - p[l]) * MOLES_PER_PA;
          if (t.rayleigh_active) t.moles[col * nlay + l] = coef[e];
        }
      }
    }
  }
}

// transpose of the gather for the active nodes: node -> (cell, coef), in cell order
void transpose_entries(Tables& t) {
  const int nent = t.nent, ng = t.ng;
  // (the active gases' part of the state: all of it unless rayleigh_active, whose tail is no node)
  const size_t nx_gas = t.nnode_active * ng;
  auto kept = [&](size_t i) { return t.ent_idx[i] >= 0 && (size_t)t.ent_idx[i] < nx_gas && t.ent_coef[i] != 0.0; };
  t.ref_ptr.assign(t.nnode_active + 1, 0);
  for (size_t i = 0; i < t.ncell * nent; ++i)
    if (kept(i)) ++t.ref_ptr[(size_t)t.ent_idx[i] / ng + 1];
  for (size_t i = 0; i < t.nnode_active; ++i) t.ref_ptr[i + 1] += t.ref_ptr[i];
  t.ref_cell.assign(t.ref_ptr.back(), 0);
  t.ref_coef.assign(t.ref_ptr.back(), 0.0);
  std::vector<int> fill(t.ref_ptr.begin(), t.ref_ptr.end() - 1);
  for (size_t i = 0; i < t.ncell * nent; ++i)
    if (kept(i)) {
      const int slot = fill[(size_t)t.ent_idx[i] / ng]++;
      t.ref_cell[slot] = (int)(i / nent);
      t.ref_coef[slot] = t.ent_coef[i];
    }
}

// K8b: which block takes which node.  The pressure axis is cut into 8 contiguous pieces of about equal numbers of
// references; piece x is walked, pressure index ascending, by the blocks x, x + 8, x + 16, ... (one XCD, in dispatch order)
void build_k8b_schedule(const Schedule& s, Tables& t) {
  constexpr int NX = 8;
  const int np = t.np, nchunk = t.grad_nchunk;
  std::vector<long long> refs_of_ip(np, 0);
  for (size_t nd = 0; nd < t.nnode_active; ++nd) refs_of_ip[t.node_ip[nd]] += t.ref_ptr[nd + 1] - t.ref_ptr[nd] + 1;
  long long total = 0;
  for (long long v : refs_of_ip) total += v;
  std::vector<int> piece_of_ip(np, 0);
  long long run = 0;
  for (int ip = 0; ip < np; ++ip) {
    piece_of_ip[ip] = (int)std::min<long long>(NX - 1, run * NX / std::max<long long>(total, 1));
    run += refs_of_ip[ip];
  }
  std::vector<std::vector<int>> list(NX);
  for (int ip = 0; ip < np; ++ip)
    for (size_t nd = 0; nd < t.nnode_active; ++nd)
      if (t.node_ip[nd] == ip) list[piece_of_ip[ip]].push_back((int)nd);
  // a wave per task, s.waves waves per block: virtual block j of piece x (= j * NX + x) takes the next s.waves entries of
  // the piece's list.  Tasks of the first launch: the runs (at most s.run references of one node) x 64-g chunks; of the
  // second: the nodes x 64-g chunks.
  t.node_run0.assign(t.nnode_active + 1, 0);
  for (size_t nd = 0; nd < t.nnode_active; ++nd) {
    t.node_run0[nd] = (int)t.run_r0.size();
    for (int r = t.ref_ptr[nd]; r < t.ref_ptr[nd + 1]; r += s.run) {
      t.run_r0.push_back(r);
      t.run_last.push_back(std::min(r + s.run, t.ref_ptr[nd + 1]));
    }
  }
  t.node_run0[t.nnode_active] = (int)t.run_r0.size();
  auto lay_out = [&](const std::vector<std::vector<int>>& entries) {
    size_t longest = 0;
    for (const auto& l : entries) longest = std::max(longest, (l.size() + s.waves - 1) / s.waves);
    std::vector<int> order(longest * NX * s.waves, -1);
    for (int x = 0; x < NX; ++x)
      for (size_t q = 0; q < entries[x].size(); ++q) order[((q / s.waves) * NX + x) * s.waves + q % s.waves] = entries[x][q];
    return order;
  };
  std::vector<std::vector<int>> node_entries(NX), run_entries(NX);
  if (s.plain_order) {
    for (size_t q = 0; q < t.nnode_active * nchunk; ++q) node_entries[(q / s.waves) % NX].push_back((int)q);
    for (size_t q = 0; q < t.run_r0.size() * nchunk; ++q) run_entries[(q / s.waves) % NX].push_back((int)q);
  } else {
    for (int x = 0; x < NX; ++x)
      for (int nd : list[x]) {
        for (int c = 0; c < nchunk; ++c) node_entries[x].push_back(nd * nchunk + c);
        for (int r = t.node_run0[nd]; r < t.node_run0[nd + 1]; ++r)
          for (int c = 0; c < nchunk; ++c) run_entries[x].push_back(r * nchunk + c);
      }
  }
  t.node_order = lay_out(node_entries);
  t.run_order = lay_out(run_entries);
}

// K9: the prior's stencil per node.  B^-1 is the Kronecker product of the three AR(1) inverses (tridiagonal each):
// up to 27 neighbours, weight = wc * wt * wp, entries below MIN_ERROR_COVARIANCE dropped as the reference zeroes them in its
// dense inverse (ckd_model.cpp:650, :709-713, :776-780); neighbours in the order (dc, dt, dp) = (-1,-1,-1) ... (1,1,1)
void build_k9_stencil(Tables& t) {
  const int nt = t.nt, np = t.np;
  t.st_nb.assign(t.nnode_active * 27, -1);
  t.st_w.assign(t.nnode_active * 27, 0.0);
  for (size_t nd = 0; nd < t.nnode_active; ++nd) {
    const int gas = t.node_gas[nd];
    const int nconc = t.gas_dims[gas * 4 + 0];
    const size_t node0 = (size_t)t.gas_dims[gas * 4 + 3];
    const double* tc = t.tri.data() + t.tri_off[gas];
    const double* tt = tc + 3 * nconc;
    const double* tp = tt + 3 * nt;
    const int ic = t.node_ic[nd], it = t.node_it[nd], ip = t.node_ip[nd];
    int slot = 0;
    for (int dc = -1; dc <= 1; ++dc) {
      const int jc = ic + dc;
      if (jc < 0 || jc >= nconc) continue;
      const double wc = tc[(dc + 1) * nconc + ic];
      if (wc == 0.0) continue;
      for (int dt = -1; dt <= 1; ++dt) {
        const int jt = it + dt;
        if (jt < 0 || jt >= nt) continue;
        const double wt = tt[(dt + 1) * nt + it];
        if (wt == 0.0) continue;
        for (int dp = -1; dp <= 1; ++dp) {
          const int jp = ip + dp;
          if (jp < 0 || jp >= np) continue;
          const double w = wc * wt * tp[(dp + 1) * np + ip];
          if (std::fabs(w) < 1.0e-6) continue;             // MIN_ERROR_COVARIANCE
          t.st_nb[nd * 27 + slot] = (int)(node0 + ((size_t)jc * nt + jt) * np + jp);
          t.st_w[nd * 27 + slot] = w;
          ++slot;
        }
      }
    }
  }
}

// the g points of each band in increasing order (CSR); a g point with a negative band number belongs to no band
void build_band_csr(const ecckd_opt_model* m, Tables& t) {
  t.band.assign(m->iband_per_g, m->iband_per_g + t.ng);
  t.band_ptr.assign(t.nband + 1, 0);
  for (int b = 0; b < t.nband; ++b) {
    for (int g = 0; g < t.ng; ++g) if (t.band[g] == b) t.band_g.push_back(g);
    t.band_ptr[b + 1] = (int)t.band_g.size();
  }
  t.band_g.resize(t.ng, 0);
}

// relative-to CKD fluxes [ncol][2][nhl][ng]; empty when no scene brings them
void gather_relative_fluxes(int nscene, const ecckd_opt_scene* scenes, Tables& t) {
  bool any_rel = false;
  for (int s = 0; s < nscene; ++s) any_rel = any_rel || has_relative(scenes[s]);
  if (!any_rel) return;
  const size_t row = (size_t)(t.nlay + 1) * t.ng;
  t.rel.assign(t.ncol * 2 * row, 0.0);
  size_t c0 = 0;
  for (int s = 0; s < nscene; ++s) {
    const ecckd_opt_scene& sc = scenes[s];
    if (has_relative(sc))
      for (size_t c = 0; c < (size_t)sc.ncol; ++c) {
        std::memcpy(&t.rel[((c0 + c) * 2) * row], sc.relative_flux_dn + c * row, row * sizeof(double));
        std::memcpy(&t.rel[((c0 + c) * 2 + 1) * row], sc.relative_flux_up + c * row, row * sizeof(double));
      }
    c0 += sc.ncol;
  }
}

int build_tables(const ecckd_opt_model* m, int nscene, const ecckd_opt_scene* scenes, const ecckd_opt_config* cfg,
                 const Schedule& s, Tables& t, std::string& err) {
  const int rc = check_arguments(m, nscene, scenes, cfg, err, t.rayleigh_active);
  if (rc != ECCKD_OK) return rc;
  order_gases(m, t);
  cap_relative_linear(cfg->cap_relative_linear, t);
  build_prior(*cfg, t);
  flatten_scenes(m, nscene, scenes, *cfg, t);
  build_entries(m, nscene, scenes, t);
  transpose_entries(t);
  build_k8b_schedule(s, t);
  build_k9_stencil(t);
  build_band_csr(m, t);
  gather_relative_fluxes(nscene, scenes, t);
  return ECCKD_OK;
}

int check_gpoint_truth(bool do_sw, bool scattering, bool rayleigh_active, double weight, const double* truth, size_t count, std::string& err) {
  if (do_sw) {
    err = "ecckd_opt_set_gpoint_truth: the per-g flux-profile term needs a longwave handle (this one is shortwave)";
    return ECCKD_PARAMETER_ERROR;
  }
  if (scattering || rayleigh_active) {
    err = "ecckd_opt_set_gpoint_truth: the per-g flux-profile term cannot be combined with the ECCKD_OPT_RAYLEIGH flags";
    return ECCKD_PARAMETER_ERROR;
  }
  if (!std::isfinite(weight)) {
    err = "ecckd_opt_set_gpoint_truth: the weight is not finite";
    return ECCKD_PARAMETER_ERROR;
  }
  if (!gpoint_truth_active(weight, truth)) return ECCKD_OK;
  for (size_t e = 0; e < count; ++e)
    if (!std::isfinite(truth[e])) {
      err = "ecckd_opt_set_gpoint_truth: truth value " + std::to_string(e) + " of " + std::to_string(count) + " is not finite";
      return ECCKD_PARAMETER_ERROR;
    }
  return ECCKD_OK;
}

void initial_state(const Layout& l, double* x, double* x_min, double* x_max) {
  for (size_t e = 0; e < l.nx; ++e) x[e] = ln_k0(l.k0[e]);
  if (!(x_min && x_max)) return;
  for (size_t e = 0; e < l.nx; ++e) {
    x_min[e] = -INFINITY;
    x_max[e] = INFINITY;
    if (l.kmin.empty()) continue;
    if (l.kmin[e] > 0.0) x_min[e] = std::log(l.kmin[e]);
    if (l.kmax[e] > 0.0) x_max[e] = std::log(l.kmax[e]);
    if (l.kmin[e] == 0.0 && l.k0[e] > 0.0 && l.kmax[e] > 0.0) x_min[e] = std::min(3.0 * x[e] - 2.0 * x_max[e], x_max[e] - 1.0);
  }
}

}  // namespace opt_tables
}  // namespace ecckd
