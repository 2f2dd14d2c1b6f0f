// opt_tables.hpp - the host tables of the optimiser (optimize.hip), built once per handle from the model, the training
// scenes and the configuration.  Plain C++: nothing here touches the device, so the steps can be built and run on their own
// (tools/check_opt_tables.cpp).  ecckd_opt_create uploads what build_tables leaves.
#pragma once

#include "../../include/ecckd_hip.h"

#include <cmath>
#include <cstddef>
#include <string>
#include <vector>

namespace ecckd {
namespace opt_tables {

constexpr double MIN_X = -1.0e20;  // solve_adept.cpp:21
// reference src/ecckd/constants.h:22-26 (the same values as common.hpp, which needs the HIP headers)
constexpr double ACCEL_GRAVITY = 9.80665;
constexpr double SPECIFIC_HEAT_AIR = 1004.0;
// moles of dry air per unit area and Pa of layer thickness (ckd_model.h:246-247, ckd_model.cpp:952)
constexpr double MOLES_PER_PA = 1.0 / (ACCEL_GRAVITY * 0.001 * 28.970);

// x = ln k0, pinned at MIN_X where k0 <= 0 (solve_adept.cpp:335-341)
inline double ln_k0(double k0) { return k0 > 0.0 ? std::log(k0) : MIN_X; }

struct GasInfo {
  int conc = 0;       // 0 none, 1 linear, 2 lut, 3 relative-linear (ckd_model.cpp:1020-1086)
  int active = 0;
  int nconc = 1;
  size_t nnode = 0;   // nconc*nt*np
  size_t ix = 0;      // offset of this gas in the coefficient vector k
  double reference_vmr = 0.0;
  std::vector<double> vmr;
  std::vector<double> sigma;  // background_error per g (ckd_model.cpp:672-683)
};

// What the handle keeps on the host for its lifetime: the sizes, the gases in k order and the first-guess coefficients.
struct Layout {
  int ng = 0, nt = 0, np = 0, nband = 0, ngas = 0, nlay = 0, nent = 0;
  size_t nx = 0, nk = 0, ncol = 0, ncell = 0, nnode_active = 0;
  bool do_sw = false;
  bool have_boundary = false;
  bool scattering = false;          // ECCKD_OPT_RAYLEIGH_SCATTERING, set by the caller of build_tables: the two-stream transfer with
                                    // Rayleigh scattering between optical depth and fluxes; the heating rates come from the net flux
  int ray_ent = -1;                 // entry index of the Rayleigh pseudo gas
  bool rayleigh_active = false;     // ECCKD_OPT_RAYLEIGH_ACTIVE, set by the caller of build_tables: the Rayleigh row sits directly behind
                                    // the active gases in k and its ng elements x = ln k_ray are the tail of the state (nx grows by ng);
                                    // no bounds (kmin = kmax = 0 there), not a node of the prior's stencil or of K8b
  size_t rayleigh_ix = 0;           // offset of the Rayleigh pseudo gas in k (ray_ent >= 0)
  int grad_nchunk = 1;              // 64-g chunks of a row
  std::vector<GasInfo> gases;       // in k order: active gases first
  std::vector<int> order;           // position in `gases` -> user gas index
  std::vector<int> user_to_k;       // user gas index -> position in `gases`
  std::vector<double> k0, kmin, kmax;   // [nk], [nx], [nx]; kmin and kmax empty unless every active gas has both
};

// Everything ecckd_opt_create uploads, in the layouts the kernels read.
struct Tables : Layout {
  // prior
  std::vector<double> tri;          // per active gas: lo | di | up of the concentration, temperature and pressure AR(1) inverses
  std::vector<int> tri_off, gas_dims;   // [ngas] offset into tri; [ngas][4] nconc, nt, np, first node
  std::vector<double> inv_sigma2;   // [ngas][ng]
  std::vector<int> node_gas, node_ic, node_it, node_ip;   // [nnode_active]
  // scenes, one row per profile
  std::vector<double> planck, semis, conv, lw, hr, fdn, fup, sfds, sfut, mu0, rel;
  // interpolation: cell -> nent (coefficient row, weight) entries, and its transpose for the active nodes
  std::vector<int> ent_idx;
  std::vector<double> ent_coef;
  std::vector<int> ref_ptr, ref_cell;
  std::vector<double> ref_coef;
  // K8b schedule
  std::vector<int> node_order, run_order, run_r0, run_last, node_run0;
  // K9 stencil [nnode_active][27]
  std::vector<int> st_nb;
  std::vector<double> st_w;
  // g points by band
  std::vector<int> band, band_ptr, band_g;
  // rayleigh_active: moles of air per unit area of every cell [ncell], the weight of dJ/dtau in dJ/dk_ray
  std::vector<double> moles;
};

// K8b's constants (optimize.hip) and the ECCKD_K8B_PLAIN_ORDER knob
struct Schedule { int waves = 4, run = 64; bool plain_order = false; };

// The steps, in the order they run; each reads what the ones before left in `t`.  check_arguments returns ECCKD_OK, or
// ECCKD_PARAMETER_ERROR with the refusal in `err`; the others assume arguments that passed it.
int check_arguments(const ecckd_opt_model* m, int nscene, const ecckd_opt_scene* scenes, const ecckd_opt_config* cfg, std::string& err,
                    bool rayleigh_active = false);
// The model part of check_arguments, shared with the gas-optics handle (gas_optics_tables.cpp); `who` opens the refusal.
// check_model_shape: dimensions, the Planck look-up table of a longwave model, linear interpolation.  check_model_gases: every
// gas well-defined; ncoef = the number of coefficients of all gases.  Both take a non-NULL model.
int check_model_shape(const ecckd_opt_model* m, const char* who, std::string& err);
int check_model_gases(const ecckd_opt_model* m, const char* who, std::string& err, size_t& ncoef);
void order_gases(const ecckd_opt_model* m, Tables& t);              // gas order, sizes and the coefficient vector
void cap_relative_linear(double cap_fraction, Tables& t);
void build_prior(const ecckd_opt_config& cfg, Tables& t);           // AR(1) inverses, sigma, the active nodes
void flatten_scenes(const ecckd_opt_model* m, int nscene, const ecckd_opt_scene* scenes, const ecckd_opt_config& cfg, Tables& t);
void build_entries(const ecckd_opt_model* m, int nscene, const ecckd_opt_scene* scenes, Tables& t);
void transpose_entries(Tables& t);
void build_k8b_schedule(const Schedule& s, Tables& t);
void build_k9_stencil(Tables& t);
void build_band_csr(const ecckd_opt_model* m, Tables& t);
void gather_relative_fluxes(int nscene, const ecckd_opt_scene* scenes, Tables& t);

// all of the above
int build_tables(const ecckd_opt_model* m, int nscene, const ecckd_opt_scene* scenes, const ecckd_opt_config* cfg,
                 const Schedule& s, Tables& t, std::string& err);

// Initial state and log-space bounds, solve_adept.cpp:335-353.  x_min / x_max may both be NULL; unbounded elements get
// -/+ infinity.
void initial_state(const Layout& l, double* x, double* x_min, double* x_max);

// ecckd_opt_set_gpoint_truth.  Does the call set the term (a weight > 0 with a truth) or remove it?
inline bool gpoint_truth_active(double weight, const double* truth) { return weight > 0.0 && truth != nullptr; }
// Its refusals, ECCKD_PARAMETER_ERROR with the reason in `err`: a shortwave handle, either ECCKD_OPT_RAYLEIGH flag, a weight
// that is not finite, and - where the call sets the term - a truth value, of `count`, that is not finite.
int check_gpoint_truth(bool do_sw, bool scattering, bool rayleigh_active, double weight, const double* truth, size_t count, std::string& err);
// hw_i of the term, the mean of the normalised weights lw[nlay] of the layers that touch half level i: they add up to sum(lw)
inline double gpoint_level_weight(const double* lw, int nlay, int i) {
  return 0.5 * ((i >= 1 ? lw[i - 1] : 0.0) + (i <= nlay - 1 ? lw[i] : 0.0));
}

}  // namespace opt_tables
}  // namespace ecckd
