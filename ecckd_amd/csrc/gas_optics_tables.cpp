// gas_optics_tables.cpp - see gas_optics_tables.hpp.
#include "gas_optics_tables.hpp"

#include "opt_tables.hpp"

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
  int rc = opt_tables::check_model_shape(m, who, err);
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

void incoming(const Flat& f, double tsi, double* out) {
  double solar_sum = 0.0;
  for (int g = 0; g < f.ng; ++g) solar_sum += f.solar_irradiance[g];
  const double tsi_scaling = tsi / solar_sum;
  for (int g = 0; g < f.ng; ++g) out[g] = tsi_scaling * f.solar_irradiance[g];
}

}  // namespace gas_optics
}  // namespace ecckd
