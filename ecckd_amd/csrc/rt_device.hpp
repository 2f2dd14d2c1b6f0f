// rt_device.hpp - the device and host primitives that every kernel file takes from ONE place: the physical constants, the wave
// and block reductions, the Planck function and the longwave layer step.  The line-by-line kernels reach them through lbl_rt.hpp,
// the tuned kernels of find_g.hip, reorder.hip, create_lut.hip and optimize.hip include this file (the block sums are those of
// find_g.hip's interval kernels and of create_lut.hip's partial kernels).  DESIGN.md and the tests compare
// kernels of different files with each other bit for bit (k_planck_sorted rebuilds the matrix k_gas_prep_lw writes): one
// source text keeps an edit from reaching only one of them.  The files are compiled with the default contraction, so an
// expression here keeps its form and operand order; a reordered one can fuse differently and change bits - in every caller.
#pragma once

#include "common.hpp"
#include "fastmath.hpp"

#include <vector>

namespace ecckd {

// ---------------------------------------------------------------------------------------------------------------- device
__device__ constexpr double kPlanckH = 6.62606896e-34;
__device__ constexpr double kLightC = 2.99792458e8;
__device__ constexpr double kPi = 3.14159265358979323846;
constexpr double kPlanckOverBoltzmann = 6.62606896e-34 / 1.3806504e-23;   // h / k, planck_function.cpp:29-31 (host and device)

// the lanes of a wave in shuffle order: a fixed tree, bitwise reproducible; the result is valid in lane 0
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_down(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}

// the sum of v over the wave, added to *acc by lane 0: one writer per wave's accumulator
__device__ __forceinline__ void wave_add(double* acc, int lane, double v) {
  const double s = wave_sum(v);
  if (lane == 0) *acc += s;
}

// the four waves' accumulators s[w * n + t], added in a fixed order
__device__ __forceinline__ double add_waves(const double* s, int n, int t) {
  return ((s[t] + s[n + t]) + s[2 * n + t]) + s[3 * n + t];
}

// sum over a 256-thread block; result valid in thread 0.  s4 = 4 doubles of LDS.
__device__ __forceinline__ double block_sum_256(double v, double* s4) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) s4[wave] = v;
  __syncthreads();
  return ((s4[0] + s4[1]) + s4[2]) + s4[3];
}

// two (or three) block sums behind ONE pair of barriers; every sum is formed exactly as block_sum_256 forms it
__device__ __forceinline__ void block_sum_256_x3(double& a, double& b, double& c, double (*s4)[4]) {
  a = wave_sum(a);
  b = wave_sum(b);
  c = wave_sum(c);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) { s4[0][wave] = a; s4[1][wave] = b; s4[2][wave] = c; }
  __syncthreads();
  a = ((s4[0][0] + s4[0][1]) + s4[0][2]) + s4[0][3];
  b = ((s4[1][0] + s4[1][1]) + s4[1][2]) + s4[1][3];
  c = ((s4[2][0] + s4[2][1]) + s4[2][2]) + s4[2][3];
}

// Several per-lane values reduced over the wave TOGETHER: at lane distance 32 a lane hands over one half of its values and
// combines what it receives with the half it keeps, at distance 16 a half of those, ... - NV + NV/2 + ... exchanges instead of
// six per value (every exchange is an LDS crossbar operation that all the waves of a CU queue for).  Lane l ends up with the
// wave's result of value bitreverse6(l) in v[0], for bitreverse6(l) < NV.  A fixed tree, the same for every value: bitwise
// reproducible.  Where a level has an odd number of values left, the last one is paired with 0.0 (PAD_ZERO, for sums: the
// optimiser's form, one lane of the exchange keeps its result) or with itself (the look-up table's form, right for any op:
// both lanes keep it).  Both forms stay because each is the measured code of its kernels.
template <int USED, bool PAD_ZERO, typename Op>
__device__ __forceinline__ void fold_level(double* v, bool upper, int mask, Op op) {
  constexpr int NEXT = (USED + 1) / 2;
#pragma unroll
  for (int i = 0; i < NEXT; ++i) {
    const double a = v[2 * i];
    const double b = (2 * i + 1 < USED) ? v[2 * i + 1] : (PAD_ZERO ? 0.0 : a);
    const double send = upper ? a : b;
    const double keep = upper ? b : a;
    v[i] = op(keep, __shfl_xor(send, mask, 64));
  }
}
template <int NV, bool PAD_ZERO, typename Op>
__device__ __forceinline__ void fold_wave(double (&v)[NV], int lane, Op op) {
  static_assert(NV <= 64, "one value per lane at the end");
  constexpr int U1 = (NV + 1) / 2, U2 = (U1 + 1) / 2, U3 = (U2 + 1) / 2, U4 = (U3 + 1) / 2, U5 = (U4 + 1) / 2;
  fold_level<NV, PAD_ZERO>(v, (lane & 32) != 0, 32, op);
  fold_level<U1, PAD_ZERO>(v, (lane & 16) != 0, 16, op);
  fold_level<U2, PAD_ZERO>(v, (lane & 8) != 0, 8, op);
  fold_level<U3, PAD_ZERO>(v, (lane & 4) != 0, 4, op);
  fold_level<U4, PAD_ZERO>(v, (lane & 2) != 0, 2, op);
  fold_level<U5, PAD_ZERO>(v, (lane & 1) != 0, 1, op);
}

// planck_function (planck_function.cpp:22-54): freq = wn_to_freq(wn); pref = planck_pref(d_wn, freq);
// B(level) = planck(pref, freq, hk[level]) with hk = (h / k) / T
__device__ __forceinline__ double wn_to_freq(double wn) {
  const double inv_cm_2_Hz = 100.0 * kLightC;
  return wn * inv_cm_2_Hz;
}

__device__ __forceinline__ double planck_pref(double dwn, double freq) {
  const double inv_cm_2_Hz = 100.0 * kLightC;
  return (dwn * 2.0 * kPlanckH * inv_cm_2_Hz * kPi / (kLightC * kLightC)) * (freq * freq * freq);
}

__device__ __forceinline__ double planck(double pref, double freq, double hk_level) {
  return div_fast(pref, exp_fast(freq * hk_level) - 1.0);
}

// radiative_transfer_lw (radiative_transfer_lw.cpp:27-60) along the slant path sec * tau, rsec = 1 / sec
__device__ __forceinline__ void lw_layer(double sec, double rsec, double tau, double& eps, double& fac) {
  eps = 1.0 - exp_fast(-sec * tau);
  fac = (eps > 1.0e-5) ? 1.0 - div_fast(eps * rsec, tau) : 0.5 * eps;
}

__device__ __forceinline__ double lw_step(double flux, double eps, double fac, double b_prev, double b) {
  return flux * (1.0 - eps) + b_prev * (eps - fac) + b * fac;
}

// emissivity 1: the reference's emissivity * B + (1 - emissivity) * flux, kept as it stands
__device__ __forceinline__ double lw_surface(double flux, double b_surf) {
  return b_surf * 1.0 + (1.0 - 1.0) * flux;
}

// ------------------------------------------------------------------------------------------------------------------ host
// hk[level] = (h / k) / temperature[level]
inline int make_hk(const char* who, int nhl, const double* h_temperature_hl, std::vector<double>& hk) {
  hk.resize(nhl);
  for (int i = 0; i < nhl; ++i) {
    ECCKD_REQUIRE(h_temperature_hl[i] > 0.0, "%s: temperature_hl must be positive", who);
    hk[i] = kPlanckOverBoltzmann / h_temperature_hl[i];
  }
  return ECCKD_OK;
}

}  // namespace ecckd
