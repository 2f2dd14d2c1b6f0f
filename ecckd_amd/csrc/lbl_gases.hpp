// lbl_gases.hpp - the gas table of the many-scenario entries (lbl_scenarios.hip, lbl_scenarios_sw_rayleigh.hip): the gases'
// rows as a kernel argument, the merged optical depth of a wavenumber and layer formed from them, and the check of the
// arguments that describe them.  One source text, so that both files merge the gases as k_merge does (merge.hip:36-38).
#pragma once

#include "common.hpp"
#include "lbl_rt.hpp"

namespace ecckd {
namespace lbl {

constexpr int LS_MAX_GAS = 16;

// the gases' rows, by value in the kernel arguments: indexed with the (uniform) gas counter, so scalar loads
struct GasRows {
  const void* od[LS_MAX_GAS];
  unsigned long long stride[LS_MAX_GAS];
  int type[LS_MAX_GAS];
};

// tau[s] = sum over the gases, in gas order, of od_g * scale[s][g][l] (k_merge, merge.hip:36-38), s < ns
template <int S>
__device__ __forceinline__ void merged_tau(const GasRows& gr, int ngas, int nlay, int l, size_t j, int ns,
                                           const double* __restrict__ scale, double (&tau)[S]) {
  for (int g = 0; g < ngas; ++g) {
    const size_t at = (size_t)l * gr.stride[g] + j;
    const double x = gr.type[g] == ECCKD_F64 ? static_cast<const double*>(gr.od[g])[at]
                                             : (double)static_cast<const float*>(gr.od[g])[at];
    const double* sc = scale + (size_t)g * nlay + l;
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (s < ns) {
        const double v = __dmul_rn(x, sc[(size_t)s * ngas * nlay]);
        tau[s] = g == 0 ? v : __dadd_rn(tau[s], v);
      }
  }
}

inline int check_gases(const char* who, int ngas, const void* const* d_od, const int* od_type, const size_t* od_stride, size_t nwav,
                       int nscen, const double* h_scale, GasRows& gr) {
  ECCKD_REQUIRE(ngas >= 1 && ngas <= LS_MAX_GAS, "%s: ngas (%d) must be between 1 and %d", who, ngas, LS_MAX_GAS);
  ECCKD_REQUIRE(nscen >= 1, "%s: nscen (%d) must be at least 1", who, nscen);
  ECCKD_REQUIRE(d_od && od_type && od_stride && h_scale, "%s: NULL argument", who);
  for (int g = 0; g < LS_MAX_GAS; ++g) { gr.od[g] = nullptr; gr.stride[g] = 0; gr.type[g] = ECCKD_F64; }
  for (int g = 0; g < ngas; ++g) {
    ECCKD_REQUIRE(d_od[g], "%s: d_od[%d] is NULL", who, g);
    ECCKD_REQUIRE(od_type[g] == ECCKD_F32 || od_type[g] == ECCKD_F64, "%s: od_type[%d] must be 4 or 8", who, g);
    ECCKD_REQUIRE(od_stride[g] >= nwav, "%s: od_stride[%d] (%zu) < nwav (%zu)", who, g, od_stride[g], nwav);
    gr.od[g] = d_od[g]; gr.stride[g] = od_stride[g]; gr.type[g] = od_type[g];
  }
  return ECCKD_OK;
}

}  // namespace lbl
}  // namespace ecckd
