// lbl_scenarios_sw_rayleigh.hip - line-by-line shortwave band fluxes of one column WITH Rayleigh scattering for MANY scenarios
// from one read of the gases' spectra: what lbl_scenarios.hip is to k_lbl_fluxes_sw, this file is to k_lbl_fluxes_sw_rayleigh
// (lbl_fluxes_sw_rayleigh.hip).  Scenario s at angle a is the sequence "ngas calls of ecckd_merge_spectrum_dev with
// h_scale[s], then ecckd_lbl_band_fluxes_sw_rayleigh on that DOUBLE matrix and the Rayleigh spectrum": the absorption optical
// depth is merged_tau of lbl_gases.hpp (the arithmetic of k_merge in gas order; the matrix is never written), the scattering one
// is the same row in every scenario, and the transfer is rayleigh_layer / rayleigh_up / rayleigh_down of lbl_rt.hpp, called as
// k_lbl_fluxes_sw_rayleigh calls them.  With one gas the results are the parent sequence's bit for bit; with more the compiler
// may fuse merged_tau's product and sum of a gas into one FMA where k_merge rounds twice, as in lbl_scenarios.hip (DESIGN.md,
// "Rayleigh scattering with many scenarios": 4e-14 of the incoming flux at most in the tests).
//
// Shape: that kernel's.  One thread per wavenumber of a BandChunk, a bounded grid (rayleigh_grid) whose blocks loop over the
// chunks, the per-level state in a device workspace [block][slot][level][thread] that a thread writes and later reads alone.
// Inside a chunk the block loops over the scenarios of the launch and, within a scenario, over the angles.  The workspace has a
// fourth slot beside D, A and S: the merged absorption optical depth of the scenario in hand, formed from the ngas rows in the
// direct-beam sweep of the first angle and read back by the other 3 nsza - 1 sweeps of the scenario - 4 (nlay + 1) doubles per
// thread.  Per level the fluxes are reduced wave -> block in the fixed order of wave_add / add_waves into chunk partials
// [chunk][scenario][angle][3][nhl], which the host adds in chunk order (band_collect): no bit depends on the grid, on which
// block walks a chunk, on the scenarios that share a launch or on the angles computed together.
//
// Launch split.  The partials of a launch are nchunk x ns x nsza x 3 x (nlay + 1) doubles, so a launch takes whole scenarios,
// with all their angles, up to RAYLEIGH_SCENARIO_BYTES of partials (ECCKD_RAYLEIGH_SCENARIO_BYTES = N bytes instead), one
// scenario at least: ecckd_lbl_rayleigh_scenarios_per_launch.
#include "common.hpp"
#include "lbl_gases.hpp"
#include "lbl_rt.hpp"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <vector>

namespace {

using namespace ecckd::lbl;

constexpr int RS_SLOTS = RAYLEIGH_SLOTS + 1;                              // D, A, S and the merged tau_abs per level
constexpr size_t RAYLEIGH_SCENARIO_BYTES = (size_t)512 << 20;             // partial bytes of one launch
constexpr int RS_BLOCKS_PER_CU = 4;                                       // the waves per SIMD this kernel's registers allow

// LDS: acc[4][3][nhl]; ws: [gridDim.x][4][nhl][LBL_THREADS]; partial: [nchunk][ns][nsza][3][nhl]
template <typename RayT>
__global__ void __launch_bounds__(LBL_THREADS)
k_lbl_scenarios_sw_rayleigh(int nlay, int nsza, int nchunk, int ngas, GasRows gr, int ns,
                            const double* __restrict__ scale /* [ns][ngas][nlay]: the scenarios of this launch */, size_t nwav,
                            size_t ray_stride, const BandChunk* __restrict__ chunks, const double* __restrict__ ang /* sw_angle_table */,
                            const double* __restrict__ ssi, const double* __restrict__ albedo /* per wavenumber or NULL */,
                            const RayT* __restrict__ od_ray, double* ws, double* __restrict__ partial,
                            double* __restrict__ surf_dn_direct /* NULL or the first scenario of this launch: [ns][nsza][nwav] */,
                            double* __restrict__ surf_dn /* same */, double* __restrict__ toa_up /* same */) {
  extern __shared__ double s_acc[];
  const int nhl = nlay + 1;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double* acc_dir = s_acc + wave * RAYLEIGH_FLUXES * nhl;
  double* acc_dn = acc_dir + nhl;
  double* acc_up = acc_dn + nhl;
  double* my = ws + (size_t)blockIdx.x * RS_SLOTS * nhl * LBL_THREADS + tid;
  double* w_d = my;                                        // element (slot, level) of this thread: [(slot * nhl + level) * LBL_THREADS]
  double* w_a = my + (size_t)nhl * LBL_THREADS;
  double* w_s = my + (size_t)2 * nhl * LBL_THREADS;
  double* w_t = my + (size_t)3 * nhl * LBL_THREADS;        // tau_abs of layer l at level l
  for (int ci = blockIdx.x; ci < nchunk; ci += gridDim.x) {
    const BandChunk c = chunks[ci];
    const long long i = c.i1 + tid;
    const bool live = i <= c.i2;
    const size_t j = live ? (size_t)i : (size_t)c.i2;
    const double inc = ssi[j];
    const double alb = albedo ? albedo[j] : 0.0;
    auto layer = [&](int l, double mu0, double minus_sec_sza) {
      return rayleigh_layer(w_t[(size_t)l * LBL_THREADS], (double)od_ray[(size_t)l * ray_stride + j], mu0, minus_sec_sza);
    };
    for (int k = 0; k < ns; ++k) {
      const double* sc = scale + (size_t)k * ngas * nlay;
      for (int s = 0; s < nsza; ++s) {
        const double cos_sza = ang[s], minus_sec_sza = ang[LBL_MAX_SZA + s];   // (uniform: scalar loads)
        const size_t row = (size_t)k * nsza + s;
        for (int t = tid; t < 4 * RAYLEIGH_FLUXES * nhl; t += LBL_THREADS) s_acc[t] = 0.0;
        __syncthreads();
        // the direct beam on tau_abs + tau_ray; the scenario's first angle merges the gases and leaves tau_abs for every later sweep
        double flux = live ? cos_sza * inc : 0.0;
        w_d[0] = flux;
        for (int l = 0; l < nlay; ++l) {
          double tau_abs;
          if (s == 0) {
            double m[1] = {0.0};
            merged_tau<1>(gr, ngas, nlay, l, j, 1, sc, m);
            tau_abs = m[0];
            w_t[(size_t)l * LBL_THREADS] = tau_abs;
          } else {
            tau_abs = w_t[(size_t)l * LBL_THREADS];
          }
          const double tau = tau_abs + (double)od_ray[(size_t)l * ray_stride + j];
          flux = flux * exp(minus_sec_sza * tau);
          w_d[(size_t)(l + 1) * LBL_THREADS] = flux;
        }
        if (surf_dn_direct && live) surf_dn_direct[row * nwav + j] = flux;
        const double d_surf = flux;
        // up: the albedo and the source below every level
        double a = alb, src = alb * flux;
        w_a[(size_t)nlay * LBL_THREADS] = a;
        w_s[(size_t)nlay * LBL_THREADS] = src;
        for (int l = nlay - 1; l >= 0; --l) {
          const RayleighLayer L = layer(l, cos_sza, minus_sec_sza);
          rayleigh_up(L, w_d[(size_t)l * LBL_THREADS], a, src, a, src);
          w_a[(size_t)l * LBL_THREADS] = a;
          w_s[(size_t)l * LBL_THREADS] = src;
        }
        // down: the diffuse and the upwelling flux at every level; the direct flux is summed here from the stored value, as in
        // k_lbl_fluxes_sw_rayleigh and for its reason (no fused first addition: direct == total where nothing scatters)
        double dn = 0.0, up = src;
        double d_top = w_d[0];
        wave_add(&acc_dir[0], lane, d_top);
        wave_add(&acc_dn[0], lane, dn + d_top);
        wave_add(&acc_up[0], lane, up);
        if (toa_up && live) toa_up[row * nwav + j] = up;
        for (int l = 0; l < nlay; ++l) {
          const RayleighLayer L = layer(l, cos_sza, minus_sec_sza);
          rayleigh_down(L, d_top, w_a[(size_t)(l + 1) * LBL_THREADS], w_s[(size_t)(l + 1) * LBL_THREADS], dn, dn, up);
          d_top = w_d[(size_t)(l + 1) * LBL_THREADS];
          wave_add(&acc_dir[l + 1], lane, d_top);
          wave_add(&acc_dn[l + 1], lane, dn + d_top);
          wave_add(&acc_up[l + 1], lane, up);
        }
        if (surf_dn && live) surf_dn[row * nwav + j] = dn + d_surf;
        __syncthreads();
        for (int t = tid; t < RAYLEIGH_FLUXES * nhl; t += LBL_THREADS)
          partial[((size_t)ci * ns * nsza + row) * RAYLEIGH_FLUXES * nhl + t] = add_waves(s_acc, RAYLEIGH_FLUXES * nhl, t);
        __syncthreads();
      }
    }
  }
}

size_t scenario_budget() {
  if (const char* e = std::getenv("ECCKD_RAYLEIGH_SCENARIO_BYTES")) {
    const long long v = std::atoll(e);
    if (v >= 1) return (size_t)v;
  }
  return RAYLEIGH_SCENARIO_BYTES;
}

// whole scenarios whose partials fit the budget, one at least
int scenarios_per_launch(int nlay, int nsza, size_t nchunk) {
  const size_t per_scen = std::max<size_t>(nchunk, 1) * (size_t)nsza * RAYLEIGH_FLUXES * ((size_t)nlay + 1) * sizeof(double);
  return (int)std::min<size_t>(std::max<size_t>(scenario_budget() / per_scen, 1), INT_MAX);
}

}  // namespace

extern "C" {

int ecckd_lbl_rayleigh_scenarios_per_launch(int nlay, int nsza, size_t nchunk) {
  return nlay > 0 && nsza > 0 ? scenarios_per_launch(nlay, nsza, nchunk) : 0;
}

int ecckd_lbl_band_fluxes_sw_rayleigh_scenarios(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_cos_sza,
                                                const double* d_ssi, const double* d_albedo, int ngas, const void* const* d_od,
                                                const int* od_type, const size_t* od_stride, const void* d_od_ray, int ray_type,
                                                size_t ray_stride, int nscen, const double* h_scale, int nband,
                                                const int64_t* h_band_begin, const int64_t* h_band_end, double* h_flux_dn_direct,
                                                double* h_flux_dn, double* h_flux_up, double* d_surf_dn_direct, double* d_surf_dn,
                                                double* d_toa_up) {
  const char* who = "ecckd_lbl_band_fluxes_sw_rayleigh_scenarios";
  ECCKD_REQUIRE(ctx && nlay > 0 && h_cos_sza && d_ssi && d_od_ray && nband > 0 && h_band_begin && h_band_end && h_flux_dn_direct &&
                h_flux_dn && h_flux_up, "%s: bad argument", who);
  double h_ang[2 * LBL_MAX_SZA];
  ECCKD_CHECK(sw_angle_table(who, nsza, h_cos_sza, h_ang));
  GasRows gr;
  ECCKD_CHECK(check_gases(who, ngas, d_od, od_type, od_stride, nwav, nscen, h_scale, gr));
  ECCKD_CHECK(check_od(who, ray_type, ray_stride, nwav));
  const size_t nhl = (size_t)nlay + 1;
  const size_t lds = (size_t)4 * RAYLEIGH_FLUXES * nhl * sizeof(double);
  ECCKD_REQUIRE(lds <= 64 * 1024, "%s: nlay = %d needs %zu bytes of LDS for the level sums (64 KB at most)", who, nlay, lds);
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  BandRun r;
  const size_t rows = (size_t)nscen * nsza;
  ECCKD_CHECK(band_start(r, ctx, who, nwav, nband, h_band_begin, h_band_end, nhl, {{d_surf_dn_direct, rows}, {d_surf_dn, rows}, {d_toa_up, rows}},
                         {h_flux_dn_direct, h_flux_dn, h_flux_up}, rows));
  if (r.chunks.empty()) return ECCKD_OK;
  const size_t nchunk = r.chunks.size(), grid = rayleigh_grid(ctx, nchunk, RS_BLOCKS_PER_CU);
  const int per = std::min(scenarios_per_launch(nlay, nsza, nchunk), nscen);
  // one carve for every launch of the call: the partials of the largest launch, the workspace of the grid that is launched
  ECCKD_CHECK(band_device(r, h_ang, 2 * LBL_MAX_SZA, h_scale, (size_t)nscen * ngas * nlay, nchunk * per * nsza * RAYLEIGH_FLUXES * nhl,
                          grid * RS_SLOTS * nhl * LBL_THREADS * sizeof(double)));
  std::vector<size_t> slot_row;
  for (int s0 = 0; s0 < nscen; s0 += per) {
    const int ns = std::min(per, nscen - s0);
    const size_t first = (size_t)s0 * nsza * nwav;
    double* sdd = d_surf_dn_direct ? d_surf_dn_direct + first : nullptr;
    double* sdn = d_surf_dn ? d_surf_dn + first : nullptr;
    double* tup = d_toa_up ? d_toa_up + first : nullptr;
    with_od_type(ray_type, [&](auto tr) {
      using RayT = decltype(tr);
      hipLaunchKernelGGL((k_lbl_scenarios_sw_rayleigh<RayT>), dim3((unsigned)grid), dim3(LBL_THREADS), lds, ctx->stream, nlay, nsza,
                         (int)nchunk, ngas, gr, ns, r.d_tab1 + (size_t)s0 * ngas * nlay, nwav, ray_stride, r.d_chunks, r.d_tab0, d_ssi,
                         d_albedo, (const RayT*)d_od_ray, (double*)r.d_work, r.d_part, sdd, sdn, tup);
    });
    ECCKD_HIP_CHECK(hipGetLastError());
    slot_row.resize((size_t)ns * nsza);
    for (size_t k = 0; k < slot_row.size(); ++k) slot_row[k] = (size_t)s0 * nsza + k;
    ECCKD_CHECK(band_collect(r, ns * nsza, slot_row.data(), {h_flux_dn_direct, h_flux_dn, h_flux_up}));
  }
  return ECCKD_OK;
}

}  // extern "C"
