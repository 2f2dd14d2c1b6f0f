// gas_optics_device.hpp - the device code and the handle that gas_optics.hip (optical depths, Planck function) and
// gas_optics_fluxes.hip (the fused fluxes) share: the model and the call as the kernels read them, a cell's table entries
// (build_entries of opt_tables.cpp line for line), the FMA chain over four entries and the Planck look-up.  One source text,
// compiled without contraction, so that both files form the same bits: the fused kernel feeds its transfer the very optical
// depth and Planck value the stand-alone calls store.
#pragma once

#include "common.hpp"
#include "gas_optics_tables.hpp"
#include "opt_tables.hpp"

#include <vector>

namespace ecckd {
namespace gas_optics {

constexpr double MOLES_PER_PA = ecckd::opt_tables::MOLES_PER_PA;

struct GoModel {
  const double* k;
  const double* temperature;    // [nt][np]; the temperature axis hangs on row 0
  const double* rayleigh;       // [ng] or NULL
  const GasDesc* gases;
  double log_p_0, d_log_p, d_t;
  int ng, nt, np, ngas, nent;
};

struct GoCall {
  const double *p_hl, *t_hl, *t_fl, *vmr;
  void* od;
  void* ray_od;
  void* gas_od[MAX_GASES];
  double scaling[MAX_GASES];
  size_t ncell;
  uint32_t present;
  int nlay, keep_negative;
};

struct AxisPos { int i0; double w0, w1; };

// opt_tables.cpp axis_pos: the position on an evenly spaced axis of n nodes, held inside it
__device__ inline AxisPos axis_pos(double index0, int n) {
#pragma clang fp contract(off)
  index0 = fmax(0.0, fmin(index0, n - 1.0001));
  const int i0 = (int)index0;
  const double w1 = index0 - i0;
  return {i0, 1.0 - w1, w1};
}

// One cell's entries: opt_tables.cpp build_entries, with run_ckd's rule for absent gases (the caller skips them: their slots
// are never read).  No contraction, so that every product and sum rounds as the host's.
__device__ inline void cell_entries(const GoModel& m, const GoCall& c, size_t cell, double* coef, uint32_t* idx, double* moles) {
#pragma clang fp contract(off)
  const size_t col = cell / (size_t)c.nlay;
  const int l = (int)(cell - col * (size_t)c.nlay);
  const double* p = c.p_hl + col * (size_t)(c.nlay + 1);
  const double* T = c.t_hl + col * (size_t)(c.nlay + 1);
  const double p0 = p[l], p1 = p[l + 1];
  const double t_fl = c.t_fl ? c.t_fl[cell] : (T[l] * p0 + T[l + 1] * p1) / (p0 + p1);
  const double log_pressure_fl = log(0.5 * (p1 + p0));
  const AxisPos ap = axis_pos((log_pressure_fl - m.log_p_0) / m.d_log_p, m.np);
  const double t_0 = ap.w0 * m.temperature[ap.i0] + ap.w1 * m.temperature[ap.i0 + 1];
  const AxisPos at = axis_pos((t_fl - t_0) / m.d_t, m.nt);
  const double simple_weight = MOLES_PER_PA * (p1 - p0);
  *moles = simple_weight;
  for (int i = 0; i < m.ngas; ++i) {
    if (!((c.present >> i) & 1u)) continue;
    const GasDesc gd = m.gases[i];
    double weight = simple_weight, vm = 0.0;
    if (gd.conc != 0) {
      vm = c.vmr[(col * (size_t)m.ngas + (size_t)i) * (size_t)c.nlay + (size_t)l] * c.scaling[i];
      weight = (gd.conc == 3) ? simple_weight * (vm - gd.reference_vmr) : simple_weight * vm;
    }
    AxisPos ac = {0, 1.0, 1.0};
    if (gd.conc == 2) ac = axis_pos((log(vm) - gd.log_vmr0) / gd.d_log_c, gd.nconc);
    const int nc = gd.conc == 2 ? 2 : 1;
    int q = gd.ent0;
    for (int dc = 0; dc < nc; ++dc)
      for (int dt = 0; dt < 2; ++dt)
        for (int dp = 0; dp < 2; ++dp) {
          const uint32_t node = ((uint32_t)(ac.i0 + dc) * (uint32_t)m.nt + (uint32_t)(at.i0 + dt)) * (uint32_t)m.np + (uint32_t)(ap.i0 + dp);
          idx[q] = gd.ix + node * (uint32_t)m.ng;
          coef[q] = weight * (dc ? ac.w1 : ac.w0) * (dt ? at.w1 : at.w0) * (dp ? ap.w1 : ap.w0);
          ++q;
        }
  }
}

template <bool F32>
__device__ inline void put(void* out, size_t i, double v) {
  if (F32) ((float*)out)[i] = (float)v;
  else ((double*)out)[i] = v;
}

// four entries of a chain: the loads go out together, the FMAs follow in entry order
__device__ inline double chain4(const double* kg, const double* coef, const uint32_t* idx, double acc) {
  const double k0 = kg[idx[0]], k1 = kg[idx[1]], k2 = kg[idx[2]], k3 = kg[idx[3]];
  acc = fma(coef[0], k0, acc);
  acc = fma(coef[1], k1, acc);
  acc = fma(coef[2], k2, acc);
  return fma(coef[3], k3, acc);
}

// planck_lut of opt_tables.cpp (CkdModel::calc_planck_function, ckd_model.cpp:1121-1145) at one (temperature, g)
__device__ inline double planck_value(int ntp, const double* tpl, const double* pf, int ng, size_t g, double t) {
#pragma clang fp contract(off)
  const double d_t = tpl[1] - tpl[0], t0 = tpl[0];
  const double tindex0 = (t - t0) / d_t;
  double v;
  if (tindex0 >= 0) {
    const int it0 = min((int)tindex0, ntp - 2);
    const double w1 = tindex0 - it0, w0 = 1.0 - w1;
    v = w0 * pf[(size_t)it0 * ng + g] + w1 * pf[(size_t)(it0 + 1) * ng + g];
  } else {
    v = (t / t0) * pf[g];
  }
  return v;
}

}  // namespace gas_optics
}  // namespace ecckd

struct ecckd_gas_optics {
  ecckd_ctx* ctx = nullptr;
  ecckd::gas_optics::Flat f;        // the model's small arrays; the tables themselves live on the device only
  std::vector<void*> blocks;        // every device block of the handle, from the context's allocator
  double *d_k = nullptr, *d_temperature = nullptr, *d_tpl = nullptr, *d_planck = nullptr, *d_rayleigh = nullptr;
  double* d_solar = nullptr;        // shortwave: solar_irradiance[ng], for the fused fluxes
  int* d_iband = nullptr;           // iband_per_g[ng] where the model has it
  ecckd::gas_optics::GasDesc* d_gases = nullptr;
  template <typename T> int upload(T** d, const std::vector<T>& h) {
    void* v = nullptr;
    ECCKD_HIP_CHECK(ecckd::dev_malloc(ctx, &v, std::max<size_t>(h.size(), 1) * sizeof(T)));
    blocks.push_back(v);
    *d = (T*)v;
    if (!h.empty()) ECCKD_HIP_CHECK(hipMemcpyAsync(v, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return ECCKD_OK;
  }
};
