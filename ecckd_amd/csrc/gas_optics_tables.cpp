// gas_optics_tables.cpp - see gas_optics_tables.hpp.
#include "gas_optics_tables.hpp"

#include "opt_tables.hpp"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>

namespace ecckd {
namespace gas_optics {

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

}  // namespace

int flatten_model(const ecckd_opt_model* m, Flat& f, std::string& err) {
  const char* who = "ecckd_gas_optics_create";
  if (!m) return refuse(err, "%s: NULL argument", who);
  // (a model without iband_per_g is served, less the band sums: the shared check sees a stand-in for the missing map)
  const int no_band = 0;
  ecckd_opt_model checked = *m;
  if (!m->iband_per_g) checked.iband_per_g = &no_band;
  int rc = opt_tables::check_model_shape(&checked, who, err);
  if (rc != ECCKD_OK) return rc;
  size_t ncoef = 0;
  rc = opt_tables::check_model_gases(m, who, err, ncoef);
  if (rc != ECCKD_OK) return rc;
  if (!(ncoef < (size_t)0x7fffffff)) return refuse(err, "%s: coefficient vector too long for int32 indexing", who);
  if (m->ngas > MAX_GASES) return refuse(err, "%s: %d gases, at most %d are supported", who, m->ngas, MAX_GASES);
  const size_t ng = f.ng = m->ng;
  f.nt = m->nt; f.np = m->np; f.ngas = m->ngas;
  f.is_sw = m->solar_irradiance != nullptr;
  f.has_rayleigh = f.is_sw && m->rayleigh_molar_scattering != nullptr;
  f.log_p_0 = m->log_pressure[0];
  f.d_log_p = m->log_pressure[1] - m->log_pressure[0];
  f.d_t = m->temperature[1 * f.np + 0] - m->temperature[0];
  f.temperature.assign(m->temperature, m->temperature + (size_t)f.nt * f.np);
  f.k.reserve(ncoef);
  f.nent = 0;
  for (int i = 0; i < m->ngas; ++i) {
    const ecckd_opt_gas& ug = m->gases[i];
    GasDesc d{};
    d.conc = ug.conc_dependence;
    d.nconc = ug.conc_dependence == 2 ? ug.nconc : 1;
    d.ent0 = f.nent;
    d.nent = ug.conc_dependence == 2 ? 8 : 4;
    d.ix = (uint32_t)f.k.size();
    d.reference_vmr = ug.reference_vmr;
    if (ug.conc_dependence == 2) {
      d.log_vmr0 = std::log(ug.vmr[0]);
      d.d_log_c = std::log(ug.vmr[1] / ug.vmr[0]);
    }
    f.nent += d.nent;
    f.k.insert(f.k.end(), ug.molar_abs, ug.molar_abs + (size_t)d.nconc * f.nt * f.np * ng);
    f.gases.push_back(d);
  }
  if (f.is_sw) {
    f.solar_irradiance.assign(m->solar_irradiance, m->solar_irradiance + ng);
    if (f.has_rayleigh) f.rayleigh.assign(m->rayleigh_molar_scattering, m->rayleigh_molar_scattering + ng);
  } else {
    f.ntp = m->ntp;
    f.temperature_planck.assign(m->temperature_planck, m->temperature_planck + f.ntp);
    f.planck_function.assign(m->planck_function, m->planck_function + (size_t)f.ntp * ng);
  }
  f.nband = 0;
  if (m->iband_per_g) {
    f.iband.assign(m->iband_per_g, m->iband_per_g + ng);
    for (int b : f.iband) f.nband = std::max(f.nband, b + 1);
  }
  if (tile_lds_bytes(f.nent) > MAX_LDS_BYTES)
    return refuse(err, "%s: %d table entries per cell need %zu bytes of LDS per tile, more than %zu", who, f.nent, tile_lds_bytes(f.nent),
                  MAX_LDS_BYTES);
  return ECCKD_OK;
}

int launch_plan(long long ncol, int nlay, int ng, int nent, Plan& p, std::string& err) {
  const char* who = "ecckd_gas_optics_dev";
  if (!(ncol > 0 && nlay > 0 && ng > 0 && nent > 0)) return refuse(err, "%s: ncol, nlay must be positive (ncol=%lld nlay=%d)", who, ncol, nlay);
  p.lds_bytes = tile_lds_bytes(nent);
  if (p.lds_bytes > MAX_LDS_BYTES)
    return refuse(err, "%s: %d table entries per cell need %zu bytes of LDS per tile, more than %zu", who, nent, p.lds_bytes, MAX_LDS_BYTES);
  p.ncell = (size_t)ncol * (size_t)nlay;
  const size_t blocks = (p.ncell + CELLS_PER_BLOCK - 1) / CELLS_PER_BLOCK;
  if (blocks > (size_t)0x7fffffff) return refuse(err, "%s: %zu cells are more than one launch holds", who, p.ncell);
  p.nvalue = p.ncell * (size_t)ng;
  p.blocks = (unsigned)blocks;
  p.threads = THREADS;
  return ECCKD_OK;
}

int check_call(const Flat& f, const CallArgs& a, uint32_t& present_mask, bool& any_gas_od, std::string& err) {
  const char* who = "ecckd_gas_optics_dev";
  if (!(a.ncol > 0 && a.nlay > 0)) return refuse(err, "%s: ncol, nlay must be positive (ncol=%d nlay=%d)", who, a.ncol, a.nlay);
  if (!(a.have_pressure && a.have_temperature_hl)) return refuse(err, "%s: d_pressure_hl and d_temperature_hl are needed", who);
  if (a.out_type != ECCKD_F64 && a.out_type != ECCKD_F32)
    return refuse(err, "%s: out_type %d is neither ECCKD_F32 nor ECCKD_F64", who, a.out_type);
  if (a.keep_negative != 0 && a.keep_negative != 1) return refuse(err, "%s: keep_negative must be 0 or 1, not %d", who, a.keep_negative);
  if (a.have_rayleigh_od && !f.is_sw) return refuse(err, "%s: d_rayleigh_od asked of a longwave handle", who);
  present_mask = 0;
  any_gas_od = false;
  for (int i = 0; i < f.ngas; ++i) {
    const bool present = !a.gas_present || a.gas_present[i] != 0;
    if (present) present_mask |= 1u << i;
    if (present && f.gases[i].conc != 0 && !a.have_vmr)
      return refuse(err, "%s: d_vmr_fl is NULL but gas %d depends on its mole fraction", who, i);
    if (a.gas_od && a.gas_od[i]) any_gas_od = true;
  }
  if (!(a.have_od || a.have_rayleigh_od || any_gas_od)) return refuse(err, "%s: no output asked for", who);
  return ECCKD_OK;
}

double incoming_scaling(const Flat& f, double tsi) {
  double solar_sum = 0.0;
  for (int g = 0; g < f.ng; ++g) solar_sum += f.solar_irradiance[g];
  return tsi / solar_sum;
}

void incoming(const Flat& f, double tsi, double* out) {
  const double tsi_scaling = incoming_scaling(f, tsi);
  for (int g = 0; g < f.ng; ++g) out[g] = tsi_scaling * f.solar_irradiance[g];
}

int fluxes_plan(long long ncol, int nlay, int ng, int nent, int nband, int mode, int nangle, unsigned wants, int cu_count,
                long long grid_override, ecckd_flux_plan& p, std::string& err) {
  const char* who = "ecckd_gas_optics_fluxes";
  p = ecckd_flux_plan{};
  if (!(ncol > 0 && nlay > 0)) return refuse(err, "%s: ncol, nlay must be positive (ncol=%lld nlay=%d)", who, ncol, nlay);
  if (ncol > 0x7fffffffLL) return refuse(err, "%s: %lld columns are more than one call holds", who, ncol);
  if (!(ng > 0 && nent > 0 && nband >= 0 && cu_count > 0))
    return refuse(err, "%s: bad plan dimensions (ng=%d entries=%d nband=%d compute units=%d)", who, ng, nent, nband, cu_count);
  if (mode != FLUX_LW && mode != FLUX_SW_DIRECT && mode != FLUX_SW_TWOSTREAM) return refuse(err, "%s: mode %d is not 0, 1 or 2", who, mode);
  if (nangle < 0 || nangle > FLUX_MAX_ANGLES) return refuse(err, "%s: nangle = %d outside 0..%d", who, nangle, FLUX_MAX_ANGLES);
  if (wants == 0 || wants > 31u) return refuse(err, "%s: no output asked for (wants=%u)", who, wants);
  if ((wants & WANT_BANDS) && nband == 0) return refuse(err, "%s: band outputs asked of a model without iband_per_g", who);
  if ((wants & WANT_DIRECT) && mode != FLUX_SW_TWOSTREAM)
    return refuse(err, "%s: the direct outputs belong to the two-stream shortwave mode, not to mode %d", who, mode);
  p.threads = THREADS;
  p.columns_per_block = std::max(1, THREADS / ng);
  p.g_passes = ng > THREADS ? (ng + THREADS - 1) / THREADS : 1;
  p.layer_tile = std::max(1, FLUX_TILE_CELLS / p.columns_per_block);
  p.state_rows = flux_state_rows(mode);
  const size_t cells = (size_t)p.columns_per_block * p.layer_tile;      // <= THREADS: one lane forms one cell's entries
  const size_t width = ng <= THREADS ? (size_t)THREADS : (size_t)ng;      // values of one level in a reduction
  p.reduce_levels = (int)std::max<size_t>(1, FLUX_REDUCE_DOUBLES / width);
  p.lds_bytes = cells * ((size_t)nent * 12 + 8) + (size_t)p.reduce_levels * width * 8;
  if (p.lds_bytes > MAX_LDS_BYTES)
    return refuse(err, "%s: ng=%d with %d table entries per cell needs %zu bytes of LDS per block, more than %zu", who, ng, nent, p.lds_bytes,
                  MAX_LDS_BYTES);
  const size_t nhl = (size_t)nlay + 1;
  // per block: [g pass][state row][level][thread], then the broadband doubles [2][column][level]; whole 256-byte lines
  size_t block_doubles = (size_t)p.g_passes * p.state_rows * nhl * THREADS + 2 * (size_t)p.columns_per_block * nhl;
  block_doubles = (block_doubles + 31) / 32 * 32;
  p.ngroup = ((size_t)ncol + p.columns_per_block - 1) / p.columns_per_block;
  const size_t cap = grid_override >= 1 ? (size_t)std::min<long long>(grid_override, 0x7fffffffLL) : (size_t)cu_count * FLUX_BLOCKS_PER_CU;
  p.grid = (unsigned)std::min(p.ngroup, cap);
  p.scratch_bytes = (size_t)p.grid * block_doubles * 8;
  return ECCKD_OK;
}

static const char* fluxes_entry(const FluxCallArgs& a) {
  if (a.sky_call) return a.sw_call ? "ecckd_gas_optics_fluxes_sw_sky_dev" : "ecckd_gas_optics_fluxes_lw_sky_dev";
  return a.sw_call ? "ecckd_gas_optics_fluxes_sw_dev" : "ecckd_gas_optics_fluxes_lw_dev";
}

int check_fluxes_call(const Flat& f, const FluxCallArgs& a, uint32_t& present_mask, int& mode, unsigned& wants, std::string& err) {
  const char* who = fluxes_entry(a);
  if (a.sw_call != f.is_sw)
    return refuse(err, "%s: the handle holds a %s model", who, f.is_sw ? "shortwave" : "longwave");
  if (!a.sw_call && (a.nangle < 0 || a.nangle > FLUX_MAX_ANGLES)) return refuse(err, "%s: nangle = %d outside 0..%d", who, a.nangle, FLUX_MAX_ANGLES);
  if (a.sw_call && a.scattering != 0 && a.scattering != 1) return refuse(err, "%s: scattering must be 0 or 1, not %d", who, a.scattering);
  if (a.sw_call && a.scattering == 1 && !f.has_rayleigh)
    return refuse(err, "%s: scattering = 1 needs a model with Rayleigh coefficients (rayleigh_molar_scattering)", who);
  mode = !a.sw_call ? FLUX_LW : (a.scattering ? FLUX_SW_TWOSTREAM : FLUX_SW_DIRECT);
  if (!a.out) return refuse(err, "%s: the output structure is NULL", who);
  const ecckd_flux_outputs& o = *a.out;
  wants = 0;
  if (o.flux_dn || o.flux_up) wants |= WANT_BROADBAND;
  if (o.band_flux_dn || o.band_flux_up) wants |= WANT_BANDS;
  if (o.spectral_flux_dn || o.spectral_flux_up) wants |= WANT_SPECTRAL;
  if (o.heating_rate) wants |= WANT_HEATING;
  if (o.flux_dn_direct || o.band_flux_dn_direct || o.spectral_flux_dn_direct) wants |= WANT_DIRECT;
  if ((wants & WANT_DIRECT) && mode != FLUX_SW_TWOSTREAM)
    return refuse(err, "%s: the *_direct outputs need scattering = 1%s", who,
                  a.sw_call ? " (with scattering = 0 flux_dn is the direct beam)" : ", a longwave call has no direct beam");
  if (wants == 0) return refuse(err, "%s: no output asked for", who);
  if (((wants & WANT_BANDS) || o.band_flux_dn_direct) && f.nband == 0)
    return refuse(err, "%s: band outputs asked of a model created without iband_per_g", who);
  if (!a.have_pressure) return refuse(err, "%s: d_pressure_hl is NULL", who);
  if (!a.have_temperature_hl) return refuse(err, "%s: d_temperature_hl is NULL", who);
  if (a.sw_call && !a.have_cos_sza) return refuse(err, "%s: d_cos_sza is NULL", who);
  present_mask = 0;
  for (int i = 0; i < f.ngas; ++i) {
    const bool present = !a.gas_present || a.gas_present[i] != 0;
    if (present) present_mask |= 1u << i;
    if (present && f.gases[i].conc != 0 && !a.have_vmr)
      return refuse(err, "%s: d_vmr_fl is NULL but gas %d depends on its mole fraction", who, i);
  }
  if (a.out_type != ECCKD_F64 && a.out_type != ECCKD_F32)
    return refuse(err, "%s: out_type %d is neither ECCKD_F32 nor ECCKD_F64", who, a.out_type);
  return ECCKD_OK;
}

int check_fluxes_sky(const Flat& f, const FluxCallArgs& a, bool& sky_given, std::string& err) {
  const char* who = fluxes_entry(a);
  sky_given = false;
  if (!a.sky) return ECCKD_OK;
  const ecckd_flux_sky& s = *a.sky;
  if (s.delta_eddington != 0 && s.delta_eddington != 1)
    return refuse(err, "%s: sky.delta_eddington must be 0 or 1, not %d", who, s.delta_eddington);
  if (a.sw_call) {
    if (s.surface_emissivity) return refuse(err, "%s: sky.surface_emissivity belongs to the longwave call (the shortwave surface is d_albedo)", who);
    if (s.skin_temperature) return refuse(err, "%s: sky.skin_temperature belongs to the longwave call", who);
    if (s.cloud_od && !s.cloud_ssa) return refuse(err, "%s: sky.cloud_od is given without sky.cloud_ssa", who);
    if (s.cloud_od && !s.cloud_asymmetry) return refuse(err, "%s: sky.cloud_od is given without sky.cloud_asymmetry", who);
    if (s.cloud_ssa && !s.cloud_od) return refuse(err, "%s: sky.cloud_ssa is given without sky.cloud_od", who);
    if (s.cloud_asymmetry && !s.cloud_od) return refuse(err, "%s: sky.cloud_asymmetry is given without sky.cloud_od", who);
  } else {
    if (s.cloud_ssa) return refuse(err, "%s: sky.cloud_ssa belongs to the shortwave call (longwave scattering is not treated)", who);
    if (s.cloud_asymmetry) return refuse(err, "%s: sky.cloud_asymmetry belongs to the shortwave call (longwave scattering is not treated)", who);
    if (s.delta_eddington != 0) return refuse(err, "%s: sky.delta_eddington = 1 belongs to the shortwave call", who);
  }
  if (f.nband == 0) {
    const char* band_input = s.cloud_od ? "cloud_od" : (s.surface_emissivity ? "surface_emissivity" : nullptr);
    if (band_input) return refuse(err, "%s: sky.%s is indexed by band, and the model was created without iband_per_g", who, band_input);
  }
  sky_given = s.cloud_od || s.surface_emissivity || s.skin_temperature;
  return ECCKD_OK;
}

}  // namespace gas_optics
}  // namespace ecckd

extern "C" int ecckd_gas_optics_fluxes_plan(long long ncol, int nlay, int ng, int nent, int nband, int mode, int nangle, unsigned wants,
                                            int cu_count, long long grid_override, ecckd_flux_plan* plan, char* message,
                                            size_t message_bytes) {
  std::string err;
  ecckd_flux_plan p{};
  const int rc = ecckd::gas_optics::fluxes_plan(ncol, nlay, ng, nent, nband, mode, nangle, wants, cu_count, grid_override, p, err);
  if (plan) *plan = p;
  if (message && message_bytes > 0) std::snprintf(message, message_bytes, "%s", err.c_str());
  return rc;
}
