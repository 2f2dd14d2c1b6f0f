// lbl_scenarios.hip - line-by-line band fluxes of one column for MANY scenarios from one read of the gases' spectra: the loop
// of test/run_lw_lbl_evaluation.sh:286-323 and test/run_sw_lbl_evaluation.sh:70-260 (one call of the CKDMIP tool per scenario,
// the scenarios differing in one scaling per gas file) as one call.  The arithmetic per scenario is that of the single-scenario
// path: the merged optical depth of k_merge (merge.hip:36-38: product and sum rounded separately, in gas order - bit for bit the
// DOUBLE matrix ecckd_merge_spectrum_dev would leave in HBM, which is never written here) under the recurrences of
// k_lbl_fluxes_lw / k_lbl_fluxes_sw (lbl_fluxes.hip): the same functions and steps of lbl_rt.hpp.
//
// Shape.  One thread per wavenumber, 256-thread blocks over the BandChunk list of lbl_fluxes.hip.  A SLOT is what owns one row
// of fluxes: a scenario in the longwave kernel, a (scenario, solar zenith angle) pair in the shortwave one.  A launch carries up
// to T slots.  Per layer a thread loads the ngas optical depths of its wavenumber once (FLOAT or DOUBLE per gas), forms the
// merged optical depth of every scenario of the launch in registers (one multiply-add pair per gas and scenario, scales read
// with uniform loads from the [nscen][ngas][nlay] table), and feeds every slot's flux.  The upward sweep loads the gas rows
// again and forms tau again: nlay transmissions per scenario do not fit the register file at 54 layers.  What does not depend
// on the scaling is computed once per launch and level: the Planck terms (longwave); exp(-2 tau) is computed once per scenario
// and shared by its angles (shortwave).
//
// Reduction, as in lbl_fluxes.hip: per half level and slot wave_sum -> lane 0's per-wave accumulator in LDS; the four waves
// added in the fixed order ((w0 + w1) + w2) + w3 into partial[chunk][slot][2 nhl]; the host adds the chunks in chunk order.
// Nothing depends on the launch geometry or on which slots share a launch: slot s of a call with many scenarios has the bits
// of the same scenario run alone.
//
// Tiling.  LDS per block: 4 waves x T slots x 2 nhl doubles = 64 T (nlay + 1) bytes, held within the budgets the g-point
// kernels use for their accumulators (LS_LW_LDS = 42 KB longwave, LS_SW_LDS = 58 KB shortwave), and T is capped by what the
// kernels keep in registers without scratch (LS_LW_SLOTS = 8 scenarios; LS_SW_SLOTS = 16 scenario-angles):
//   longwave:  T = min(8, GF_ACC_BYTES / (64 (nlay+1)))    8 up to 83 layers;  nlay <= 671, above that PARAMETER_ERROR
//   shortwave: T = min(16, SF_ACC_BYTES / (64 (nlay+1)))  16 up to 57 layers;  nlay <= 927, above that PARAMETER_ERROR
// More slots than T: ceil(slots / T) launches, each reading the gas rows again.  Scenarios are split first: the longwave
// scenarios go evenly over ceil(nscen / T) launches; the shortwave launch takes all nsza angles and S = min(T / nsza,
// 16 / nsza) scenarios (nsza = 5: 3 scenarios, 15 slots), the scenarios evenly over ceil(nscen / S) launches.  Only where one
// scenario's angles exceed T (nsza > T: more than 114 layers) the angles are split too, evenly over ceil(nsza / T) launches of
// one scenario.  The shortwave kernel is instantiated per number of angles of a launch (1..8), so that fluxes stay in registers.
#include "common.hpp"
#include "gpoint_bin.hpp"
#include "lbl_gases.hpp"
#include "lbl_rt.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

using namespace ecckd::lbl;

constexpr int LS_LW_SLOTS = 8;
constexpr int LS_SW_SLOTS = 16;
constexpr size_t LS_LW_LDS = GF_ACC_BYTES;         // 43008: the accumulator budgets of the g-point kernels (gpoint_bin.hpp)
constexpr size_t LS_SW_LDS = SF_ACC_BYTES;         // 59392
static_assert(LS_LW_LDS == 43008 && LS_SW_LDS == 59392, "the slot counts of ecckd_lbl_scenarios_slots follow from these");

// LDS: acc[4][ns][2*nhl]
__global__ void __launch_bounds__(LBL_THREADS)
k_lbl_scenarios_lw(int nang, const double* __restrict__ ang /*[nang] secants, [nang] weights*/, int nlay, int ngas, GasRows gr, int ns,
                   const double* __restrict__ scale /* [ns][ngas][nlay]: the scenarios of this launch */,
                   const BandChunk* __restrict__ chunks, const double* __restrict__ hk, const double* __restrict__ wn,
                   const double* __restrict__ dwn, double* __restrict__ partial /* [chunk][ns][2*nhl] */,
                   double* __restrict__ surf_dn /* [ns][nwav] or NULL */, double* __restrict__ toa_up /* [ns][nwav] or NULL */,
                   size_t nwav) {
  extern __shared__ double s_acc[];
  constexpr int S = LS_LW_SLOTS;
  const int nhl = nlay + 1;
  const BandChunk c = chunks[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nrow = ns * 2 * nhl;
  for (int t = tid; t < 4 * nrow; t += LBL_THREADS) s_acc[t] = 0.0;
  __syncthreads();
  double* acc = s_acc + wave * nrow;               // slot s: down at acc[s * 2 * nhl + level], up nhl further on
  const long long i = c.i1 + tid;
  const bool live = i <= c.i2;
  const size_t j = live ? (size_t)i : (size_t)c.i2;
  const double freq = wn_to_freq(wn[j]);
  const double pref = live ? planck_pref(dwn[j], freq) : 0.0;
  double surf_acc[S], toa_acc[S];
#pragma unroll
  for (int s = 0; s < S; ++s) { surf_acc[s] = 0.0; toa_acc[s] = 0.0; }
  for (int a = 0; a < nang; ++a) {
    const double sec = ang[a], wgt = ang[nang + a];          // (uniform: scalar loads)
    const double rsec = 1.0 / sec;
    double flux[S], tau[S];
#pragma unroll
    for (int s = 0; s < S; ++s) { flux[s] = 0.0; tau[s] = 0.0; }
    // down sweep from zero at the top of the atmosphere (:45-50); dead lanes carry pref = 0 -> all fluxes 0
    double b_prev = planck(pref, freq, hk[0]);
    for (int l = 0; l < nlay; ++l) {
      merged_tau<S>(gr, ngas, nlay, l, j, ns, scale, tau);
      const double b_next = planck(pref, freq, hk[l + 1]);                   // once per level for every scenario of the launch
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (s < ns) {
          double eps, fac;
          lw_layer(sec, rsec, tau[s], eps, fac);
          flux[s] = lw_step(flux[s], eps, fac, b_prev, b_next);
          wave_add(&acc[s * 2 * nhl + l + 1], lane, wgt * flux[s]);
        }
      b_prev = b_next;
    }
    // surface: emissivity 1, Planck function at temperature_hl(end) (:52-53)
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (s < ns) {
        surf_acc[s] += wgt * flux[s];
        flux[s] = lw_surface(flux[s], b_prev);
        wave_add(&acc[s * 2 * nhl + nhl + nlay], lane, wgt * flux[s]);
      }
    for (int l = nlay - 1; l >= 0; --l) {                                    // :55-59
      merged_tau<S>(gr, ngas, nlay, l, j, ns, scale, tau);
      const double b_l = planck(pref, freq, hk[l]);
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (s < ns) {
          double eps, fac;
          lw_layer(sec, rsec, tau[s], eps, fac);
          flux[s] = lw_step(flux[s], eps, fac, b_prev, b_l);
          wave_add(&acc[s * 2 * nhl + nhl + l], lane, wgt * flux[s]);
        }
      b_prev = b_l;
    }
#pragma unroll
    for (int s = 0; s < S; ++s) toa_acc[s] += wgt * flux[s];
  }
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (s < ns && live) {
      if (surf_dn) surf_dn[(size_t)s * nwav + j] = surf_acc[s];
      if (toa_up) toa_up[(size_t)s * nwav + j] = toa_acc[s];
    }
  __syncthreads();
  for (int t = tid; t < nrow; t += LBL_THREADS)
    partial[(size_t)blockIdx.x * nrow + t] = add_waves(s_acc, nrow, t);
}

// A angles per launch (compile time), up to LS_SW_SLOTS / A scenarios.  LDS: acc[4][ns][A][2*nhl]
template <int A>
__global__ void __launch_bounds__(LBL_THREADS)
k_lbl_scenarios_sw(int nlay, int ngas, GasRows gr, int ns, const double* __restrict__ scale /* [ns][ngas][nlay] */,
                   const BandChunk* __restrict__ chunks, const double* __restrict__ cos_sza /* [A] */,
                   const double* __restrict__ minus_sec_sza /* [A]: -1.0 / cos_sza */, const double* __restrict__ ssi,
                   const double* __restrict__ albedo /* per wavenumber or NULL */, double* __restrict__ partial /* [chunk][ns][A][2*nhl] */,
                   double* __restrict__ surf_dn /* NULL or the first angle of the first scenario of this launch */,
                   double* __restrict__ toa_up, size_t scen_stride /* nsza * nwav */, size_t nwav) {
  extern __shared__ double s_acc[];
  constexpr int S = LS_SW_SLOTS / A;
  const int nhl = nlay + 1;
  const BandChunk c = chunks[blockIdx.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nrow = ns * A * 2 * nhl;
  for (int t = tid; t < 4 * nrow; t += LBL_THREADS) s_acc[t] = 0.0;
  __syncthreads();
  double* acc = s_acc + wave * nrow;               // slot (s, a): down at acc[(s * A + a) * 2 * nhl + level], up nhl further on
  const long long i = c.i1 + tid;
  const bool live = i <= c.i2;
  const size_t j = live ? (size_t)i : (size_t)c.i2;
  double mu[A], msec[A];
#pragma unroll
  for (int a = 0; a < A; ++a) { mu[a] = cos_sza[a]; msec[a] = minus_sec_sza[a]; }
  const double ssi_j = ssi[j];
  double flux[S][A], tau[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    tau[s] = 0.0;
#pragma unroll
    for (int a = 0; a < A; ++a) {
      flux[s][a] = live ? mu[a] * ssi_j : 0.0;                               // radiative_transfer_sw.cpp:39
      if (s < ns) wave_add(&acc[(s * A + a) * 2 * nhl], lane, flux[s][a]);
    }
  }
  for (int l = 0; l < nlay; ++l) {
    merged_tau<S>(gr, ngas, nlay, l, j, ns, scale, tau);
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (s < ns) {
#pragma unroll
        for (int a = 0; a < A; ++a) {
          flux[s][a] = flux[s][a] * exp(msec[a] * tau[s]);
          wave_add(&acc[(s * A + a) * 2 * nhl + l + 1], lane, flux[s][a]);
        }
      }
  }
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (s < ns && live) {
#pragma unroll
      for (int a = 0; a < A; ++a) {
        if (surf_dn) surf_dn[(size_t)s * scen_stride + (size_t)a * nwav + j] = flux[s][a];
        if (toa_up && !albedo) toa_up[(size_t)s * scen_stride + (size_t)a * nwav + j] = 0.0;
      }
    }
  if (albedo) {                                                             // :70-76
    const double alb = albedo[j];
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (s < ns) {
#pragma unroll
        for (int a = 0; a < A; ++a) {
          flux[s][a] = flux[s][a] * alb;
          wave_add(&acc[(s * A + a) * 2 * nhl + nhl + nlay], lane, flux[s][a]);
        }
      }
    for (int l = nlay - 1; l >= 0; --l) {
      merged_tau<S>(gr, ngas, nlay, l, j, ns, scale, tau);
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (s < ns) {
          const double t2 = exp(-2.0 * tau[s]);                             // the same for every angle of the scenario
#pragma unroll
          for (int a = 0; a < A; ++a) {
            flux[s][a] = flux[s][a] * t2;
            wave_add(&acc[(s * A + a) * 2 * nhl + nhl + l], lane, flux[s][a]);
          }
        }
    }
    if (toa_up && live) {
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (s < ns) {
#pragma unroll
          for (int a = 0; a < A; ++a) toa_up[(size_t)s * scen_stride + (size_t)a * nwav + j] = flux[s][a];
        }
    }
  }
  __syncthreads();
  for (int t = tid; t < nrow; t += LBL_THREADS)
    partial[(size_t)blockIdx.x * nrow + t] = add_waves(s_acc, nrow, t);
}

// slots per launch: what the LDS budget holds, capped by what the kernel keeps in registers (see the header); 0: nlay too large
int slots_per_launch(bool sw, int nlay) {
  const size_t per_slot = (size_t)4 * 2 * ((size_t)nlay + 1) * sizeof(double);
  return (int)std::min<size_t>(sw ? LS_SW_SLOTS : LS_LW_SLOTS, (sw ? LS_SW_LDS : LS_LW_LDS) / per_slot);
}

template <int A>
void launch_sw(ecckd_ctx* ctx, unsigned nblk, size_t lds, int nlay, int ngas, const GasRows& gr, int ns, const double* d_scale,
               const BandChunk* d_chunks, const double* d_mu, const double* d_msec, const double* d_ssi, const double* d_albedo,
               double* d_part, double* surf, double* toa, size_t scen_stride, size_t nwav) {
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_lbl_scenarios_sw<A>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LS_SW_LDS);
  hipLaunchKernelGGL(k_lbl_scenarios_sw<A>, dim3(nblk), dim3(LBL_THREADS), lds, ctx->stream, nlay, ngas, gr, ns, d_scale, d_chunks, d_mu,
                     d_msec, d_ssi, d_albedo, d_part, surf, toa, scen_stride, nwav);
}

}  // namespace

extern "C" {

int ecckd_lbl_scenarios_slots(int shortwave, int nlay) {
  return nlay > 0 ? slots_per_launch(shortwave != 0, nlay) : 0;
}

int ecckd_lbl_band_fluxes_lw_scenarios(ecckd_ctx* ctx, int nangle, int nlay, size_t nwav, const double* h_temperature_hl,
                                       const double* d_wavenumber, const double* d_d_wavenumber, int ngas, const void* const* d_od,
                                       const int* od_type, const size_t* od_stride, int nscen, const double* h_scale, int nband,
                                       const int64_t* h_band_begin, const int64_t* h_band_end, double* h_flux_dn, double* h_flux_up,
                                       double* d_surf_dn, double* d_toa_up) {
  const char* who = "ecckd_lbl_band_fluxes_lw_scenarios";
  int nang = 0;
  std::vector<double> sec_wgt;
  ECCKD_CHECK(lw_angle_table(who, nangle, &nang, sec_wgt));
  ECCKD_REQUIRE(ctx && nlay > 0 && h_temperature_hl && d_wavenumber && d_d_wavenumber && nband > 0 && h_band_begin && h_band_end &&
                h_flux_dn && h_flux_up, "%s: bad argument", who);
  GasRows gr;
  ECCKD_CHECK(check_gases(who, ngas, d_od, od_type, od_stride, nwav, nscen, h_scale, gr));
  const int T = slots_per_launch(false, nlay);
  ECCKD_REQUIRE(T >= 1, "%s: %d layers are more than the block's accumulator holds (at most %d)", who, nlay,
                (int)(LS_LW_LDS / 64) - 1);
  const int nhl = nlay + 1;
  std::vector<double> hk;
  ECCKD_CHECK(make_hk(who, nhl, h_temperature_hl, hk));
  hk.insert(hk.end(), sec_wgt.begin(), sec_wgt.end());   // one upload: hk[nhl], then the angles
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  BandRun r;
  ECCKD_CHECK(band_start(r, ctx, who, nwav, nband, h_band_begin, h_band_end, nhl, {{d_surf_dn, (size_t)nscen}, {d_toa_up, (size_t)nscen}},
                         {h_flux_dn, h_flux_up}, nscen));
  if (r.chunks.empty()) return ECCKD_OK;
  // the scenarios evenly over ceil(nscen / T) launches
  const int nlaunch = (nscen + T - 1) / T, per = (nscen + nlaunch - 1) / nlaunch;
  ECCKD_CHECK(band_device(r, hk.data(), hk.size(), h_scale, (size_t)nscen * ngas * nlay, r.chunks.size() * per * 2 * nhl, 0));
  std::vector<size_t> slot_row;
  for (int s0 = 0; s0 < nscen; s0 += per) {
    const int ns = std::min(per, nscen - s0);
    const size_t lds = (size_t)4 * ns * 2 * nhl * sizeof(double);
    hipLaunchKernelGGL(k_lbl_scenarios_lw, dim3((unsigned)r.chunks.size()), dim3(LBL_THREADS), lds, ctx->stream, nang, r.d_tab0 + nhl,
                       nlay, ngas, gr, ns, r.d_tab1 + (size_t)s0 * ngas * nlay, r.d_chunks, r.d_tab0, d_wavenumber, d_d_wavenumber,
                       r.d_part, d_surf_dn ? d_surf_dn + (size_t)s0 * nwav : nullptr, d_toa_up ? d_toa_up + (size_t)s0 * nwav : nullptr,
                       nwav);
    ECCKD_HIP_CHECK(hipGetLastError());
    slot_row.resize(ns);
    for (int k = 0; k < ns; ++k) slot_row[k] = (size_t)(s0 + k);
    ECCKD_CHECK(band_collect(r, ns, slot_row.data(), {h_flux_dn, h_flux_up}));
  }
  return ECCKD_OK;
}

int ecckd_lbl_band_fluxes_sw_scenarios(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_cos_sza, const double* d_ssi,
                                       const double* d_albedo, int ngas, const void* const* d_od, const int* od_type,
                                       const size_t* od_stride, int nscen, const double* h_scale, int nband,
                                       const int64_t* h_band_begin, const int64_t* h_band_end, double* h_flux_dn_direct,
                                       double* h_flux_up, double* d_surf_dn_direct, double* d_toa_up) {
  const char* who = "ecckd_lbl_band_fluxes_sw_scenarios";
  ECCKD_REQUIRE(ctx && nlay > 0 && h_cos_sza && d_ssi && nband > 0 && h_band_begin && h_band_end && h_flux_dn_direct && h_flux_up,
                "%s: bad argument", who);
  double h_ang[2 * LBL_MAX_SZA];
  ECCKD_CHECK(sw_angle_table(who, nsza, h_cos_sza, h_ang));
  GasRows gr;
  ECCKD_CHECK(check_gases(who, ngas, d_od, od_type, od_stride, nwav, nscen, h_scale, gr));
  const int T = slots_per_launch(true, nlay);
  ECCKD_REQUIRE(T >= 1, "%s: %d layers are more than the block's accumulator holds (at most %d)", who, nlay,
                (int)(LS_SW_LDS / 64) - 1);
  const int nhl = nlay + 1;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const size_t nslots = (size_t)nscen * nsza;
  BandRun r;
  ECCKD_CHECK(band_start(r, ctx, who, nwav, nband, h_band_begin, h_band_end, nhl, {{d_surf_dn_direct, nslots}, {d_toa_up, nslots}},
                         {h_flux_dn_direct, h_flux_up}, nslots));
  if (r.chunks.empty()) return ECCKD_OK;
  // the split (see the header): scenarios first, angles only where one scenario's angles do not fit
  int ang_per = nsza, scen_per = 1;
  if (nsza <= T) {
    const int smax = std::min(T / nsza, LS_SW_SLOTS / nsza);
    const int nl = (nscen + smax - 1) / smax;
    scen_per = (nscen + nl - 1) / nl;
  } else {
    const int nl = (nsza + T - 1) / T;
    ang_per = (nsza + nl - 1) / nl;
  }
  ECCKD_CHECK(band_device(r, h_ang, 2 * LBL_MAX_SZA, h_scale, (size_t)nscen * ngas * nlay,
                          r.chunks.size() * scen_per * ang_per * 2 * nhl, 0));
  std::vector<size_t> slot_row;
  const size_t scen_stride = (size_t)nsza * nwav;
  for (int s0 = 0; s0 < nscen; s0 += scen_per) {
    const int ns = std::min(scen_per, nscen - s0);
    for (int a0 = 0; a0 < nsza; a0 += ang_per) {
      const int na = std::min(ang_per, nsza - a0);
      const size_t lds = (size_t)4 * ns * na * 2 * nhl * sizeof(double);
      const size_t first = ((size_t)s0 * nsza + a0) * nwav;
      double* surf = d_surf_dn_direct ? d_surf_dn_direct + first : nullptr;
      double* toa = d_toa_up ? d_toa_up + first : nullptr;
      const double* d_mu = r.d_tab0 + a0;
      const double* d_msec = r.d_tab0 + LBL_MAX_SZA + a0;
      const double* d_sc = r.d_tab1 + (size_t)s0 * ngas * nlay;
#define LS_SW(A)                                                                                                           \
  case A:                                                                                                                  \
    launch_sw<A>(ctx, (unsigned)r.chunks.size(), lds, nlay, ngas, gr, ns, d_sc, r.d_chunks, d_mu, d_msec, d_ssi, d_albedo, \
                 r.d_part, surf, toa, scen_stride, nwav);                                                                  \
    break
      switch (na) { LS_SW(1); LS_SW(2); LS_SW(3); LS_SW(4); LS_SW(5); LS_SW(6); LS_SW(7); LS_SW(8); }
#undef LS_SW
      ECCKD_HIP_CHECK(hipGetLastError());
      slot_row.resize((size_t)ns * na);
      for (int k = 0; k < ns; ++k)
        for (int a = 0; a < na; ++a) slot_row[(size_t)k * na + a] = (size_t)(s0 + k) * nsza + a0 + a;
      ECCKD_CHECK(band_collect(r, ns * na, slot_row.data(), {h_flux_dn_direct, h_flux_up}));
    }
  }
  return ECCKD_OK;
}

}  // extern "C"
