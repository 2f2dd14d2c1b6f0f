// ASan/UBSan harness for the optimiser's host tables (csrc/opt_tables.cpp) and its L-BFGS history (csrc/lbfgs_history.hpp): builds
// the tables at the edge shapes - two-node temperature and pressure axes, two mole fractions, 1 and 128 layers, 1, 64 and 65 g
// points, a g point of no band, a gas absent from a scene, a profile outside the look-up table on both sides, longwave and shortwave
// with Rayleigh scattering, both K8b orders - and checks that every index the kernels follow is -1 or in range, that the two K8b
// orders hold every task once, and that the transpose holds exactly the non-zero entries of the gather.  Then the history: more
// pairs than the ring holds, one rejected, one restart; the triangular solves are checked by their residuals.  First of all the
// LDS layouts of the K8a kernels (csrc/opt_lds.hpp): nlay 1 / 17 / 54 / 128 x ng 1 / 64 / 70 x nband 1 / 13, longwave and shortwave.
// Last the tables of a handle that optimises the Rayleigh coefficients (Tables::rayleigh_active): with active gases against the
// tables without the flag, Rayleigh alone, a zero coefficient, and the flag on a longwave model, refused.  And the host step of
// ecckd_opt_set_gpoint_truth (check_gpoint_truth, gpoint_level_weight) at 1 / 7 / 8 / 9 / 17 layers x 1 / 3 / 64 / 65 g points.
// build: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iecckd_amd/csrc tools/check_opt_tables.cpp \
//        ecckd_amd/csrc/opt_tables.cpp -o /tmp/check_opt_tables && /tmp/check_opt_tables
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <tuple>
#include <vector>
#include "lbfgs_history.hpp"
#include "opt_lds.hpp"
#include "opt_tables.hpp"
namespace ot = ecckd::opt_tables;

#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    if (!(cond)) { std::printf("%s:%d: %s does not hold (%s)\n", __FILE__, __LINE__, #cond, what); std::exit(1); } \
  } while (0)

static const char* what = "";

struct Case { int ng, nt, np, nconc, nlay; bool sw, plain; };

// the model and two scenes of one case; the vectors own what the C structs point to
struct Problem {
  std::vector<double> log_p, temperature, tpl, planck, ssi, rayleigh, vmr_lut;
  std::vector<int> iband, present0, present1;
  std::vector<std::vector<double>> k, kmin, kmax;
  std::vector<ecckd_opt_gas> gases;
  ecckd_opt_model m{};
  std::vector<double> p_hl, t_hl, vmr_fl, flux, mu0, albedo, weights;
  ecckd_opt_scene scenes[2] = {};
  ecckd_opt_config cfg{};

  explicit Problem(const Case& c, std::mt19937_64& rng) {
    std::uniform_real_distribution<double> u(0.5, 1.5);
    const int ng = c.ng, nt = c.nt, np = c.np, nband = 3;
    for (int i = 0; i < np; ++i) log_p.push_back(std::log(2.0) + i * (std::log(110000.0) - std::log(2.0)) / (np - 1));
    for (int it = 0; it < nt; ++it)
      for (int ip = 0; ip < np; ++ip) temperature.push_back(200.0 + 12.0 * (log_p[ip] - log_p[0]) + 20.0 * it);
    for (int i = 0; i < 4; ++i) tpl.push_back(150.0 + 60.0 * i);
    for (size_t i = 0; i < tpl.size() * ng; ++i) planck.push_back(u(rng));
    for (int g = 0; g < ng; ++g) { iband.push_back(g * nband / ng); ssi.push_back(u(rng)); rayleigh.push_back(1e-6 * u(rng)); }
    iband[ng - 1] = nband - 1;
    if (ng > 2) iband[1] = -1;                                // a g point of no band
    for (int i = 0; i < c.nconc; ++i) vmr_lut.push_back(1e-6 * std::pow(4e4, (double)i / (c.nconc - 1)));
    const int conc[5] = {0, 2, 1, 3, 1};
    for (int i = 0; i < 5; ++i) {
      const size_t n = (size_t)(conc[i] == 2 ? c.nconc : 1) * nt * np * ng;
      k.emplace_back(n); kmin.emplace_back(n); kmax.emplace_back(n);
      for (size_t e = 0; e < n; ++e) { k[i][e] = e % 7 == 3 ? 0.0 : u(rng); kmin[i][e] = e % 5 ? 0.5 * k[i][e] : 0.0; kmax[i][e] = 2.0 * k[i][e]; }
    }
    for (int i = 0; i < 5; ++i) {
      ecckd_opt_gas g{};
      g.conc_dependence = conc[i];
      g.is_active = i != 4;
      g.nconc = conc[i] == 2 ? c.nconc : 1;
      g.vmr = conc[i] == 2 ? vmr_lut.data() : nullptr;
      g.reference_vmr = 1.8e-6;
      g.molar_abs = k[i].data(); g.min_molar_abs = kmin[i].data(); g.max_molar_abs = kmax[i].data();
      gases.push_back(g);
    }
    m.ng = ng; m.nt = nt; m.np = np; m.ngas = 5;
    m.log_pressure = log_p.data(); m.temperature = temperature.data(); m.iband_per_g = iband.data(); m.gases = gases.data();
    if (c.sw) { m.solar_irradiance = ssi.data(); m.rayleigh_molar_scattering = rayleigh.data(); }
    else { m.ntp = (int)tpl.size(); m.temperature_planck = tpl.data(); m.planck_function = planck.data(); }
    // three profiles: inside the table; above its top and colder than its coldest node; below its bottom and hotter
    const int ncol = 3, nlay = c.nlay, nhl = nlay + 1;
    const double top[3] = {5.0, 1e-4, 2.0e5}, bottom[3] = {101325.0, 1.0, 9.0e5}, t0[3] = {250.0, 20.0, 900.0};
    for (int col = 0; col < ncol; ++col)
      for (int i = 0; i < nhl; ++i) {
        p_hl.push_back(std::exp(std::log(top[col]) + i * (std::log(bottom[col]) - std::log(top[col])) / nlay));
        t_hl.push_back(t0[col] + i);
      }
    const double vm[5] = {1.0, 3e-3, 4e-4, 0.9e-6, 5e-6};
    for (int col = 0; col < ncol; ++col)
      for (int gas = 0; gas < 5; ++gas)
        for (int l = 0; l < nlay; ++l) vmr_fl.push_back(vm[gas] * (col == 1 ? 1e-4 : col == 2 ? 50.0 : 1.0) * u(rng));   // also outside the mole-fraction axis
    for (size_t i = 0; i < (size_t)ncol * nhl * std::max(nband, ng); ++i) flux.push_back(100.0 * u(rng));
    mu0.assign(ncol, 0.6); albedo.assign(nband, 0.2); weights.assign(ng, 0.01);
    present0.assign(5, 1); present1.assign(5, 1);
    present1[2] = 0; present1[4] = 0;                          // an active and a fixed gas absent from the second scene
    for (int s = 0; s < 2; ++s) {
      ecckd_opt_scene& sc = scenes[s];
      sc.ncol = ncol; sc.nlay = nlay; sc.nband = nband;
      sc.pressure_hl = p_hl.data(); sc.temperature_hl = t_hl.data(); sc.vmr_fl = vmr_fl.data();
      sc.gas_present = s ? present1.data() : present0.data();
      sc.flux_dn = sc.flux_up = flux.data();
      sc.mu0 = mu0.data(); sc.tsi = 1361.0; sc.albedo = albedo.data();
      if (s == 0) {                                            // boundary terms and relative-to fluxes in the first scene only
        sc.spectral_flux_dn_surf = flux.data();
        sc.spectral_flux_up_toa = flux.data();
        sc.spectral_boundary_weights = weights.data();
        sc.relative_flux_dn = sc.relative_flux_up = flux.data();
      }
    }
    cfg.pressure_weight_power = 0.7; cfg.prior_error = -1.0; cfg.prior_error_scaling = 1.0; cfg.min_prior_error = 0.1; cfg.max_prior_error = 3.0;
    cfg.pressure_corr = cfg.temperature_corr = 0.95; cfg.conc_corr = 0.9; cfg.cap_relative_linear = 0.8;
  }
};

// every value of `order` is -1 or a task in [0, ntask), and every task is there once
static void check_order(const std::vector<int>& order, size_t ntask, int waves) {
  std::vector<int> seen(ntask, 0);
  REQUIRE(order.size() % (8 * waves) == 0);
  for (int v : order) {
    REQUIRE(v >= -1 && v < (int)ntask);
    if (v >= 0) ++seen[v];
  }
  for (int n : seen) REQUIRE(n == 1);
}

static void check_tables(const Case& c, std::mt19937_64& rng) {
  static char label[160];
  std::snprintf(label, sizeof(label), "ng=%d nt=%d np=%d nconc=%d nlay=%d sw=%d plain=%d", c.ng, c.nt, c.np, c.nconc, c.nlay, c.sw, c.plain);
  what = label;
  Problem pr(c, rng);
  ot::Tables t;
  std::string err;
  const ot::Schedule sched = {4, 64, c.plain};
  const int rc = ot::build_tables(&pr.m, 2, pr.scenes, &pr.cfg, sched, t, err);
  if (rc != ECCKD_OK) { std::printf("%s: refused: %s\n", what, err.c_str()); std::exit(1); }
  const size_t ng = c.ng, nchunk = (ng + 63) / 64;
  REQUIRE(t.ncol == 6 && t.ncell == 6 * (size_t)c.nlay && t.nx > 0 && t.nx <= t.nk && t.nx % ng == 0 && t.nnode_active == t.nx / ng);
  REQUIRE(t.k0.size() == t.nk && t.kmin.size() == t.nx && t.kmax.size() == t.nx && (t.ray_ent >= 0) == c.sw);
  REQUIRE(t.ent_idx.size() == t.ncell * t.nent && t.ent_coef.size() == t.ent_idx.size());
  std::vector<std::tuple<int, int, double>> gathered, transposed;   // (node, cell, coefficient)
  size_t absent = 0;
  for (size_t i = 0; i < t.ent_idx.size(); ++i) {
    const int idx = t.ent_idx[i];
    REQUIRE(idx == -1 || (idx >= 0 && idx % c.ng == 0 && (size_t)idx + ng <= t.nk));
    REQUIRE(std::isfinite(t.ent_coef[i]) && (idx >= 0 || t.ent_coef[i] == 0.0));
    absent += idx < 0;
    if (idx >= 0 && (size_t)idx < t.nx && t.ent_coef[i] != 0.0) gathered.emplace_back(idx / c.ng, (int)(i / t.nent), t.ent_coef[i]);
  }
  REQUIRE(absent == 3 * (size_t)c.nlay * 8);                  // the two absent gases' four entries each, in the second scene's cells
  REQUIRE(t.ref_ptr.size() == t.nnode_active + 1 && t.ref_ptr[0] == 0 && (size_t)t.ref_ptr.back() == t.ref_cell.size() &&
          t.ref_coef.size() == t.ref_cell.size());
  for (size_t nd = 0; nd < t.nnode_active; ++nd) {
    REQUIRE(t.ref_ptr[nd] <= t.ref_ptr[nd + 1]);
    for (int r = t.ref_ptr[nd]; r < t.ref_ptr[nd + 1]; ++r) {
      REQUIRE(t.ref_cell[r] >= 0 && (size_t)t.ref_cell[r] < t.ncell);
      REQUIRE(r == t.ref_ptr[nd] || t.ref_cell[r - 1] <= t.ref_cell[r]);   // in cell order: the gradient's fixed summation order
      transposed.emplace_back((int)nd, t.ref_cell[r], t.ref_coef[r]);
    }
  }
  std::sort(gathered.begin(), gathered.end());
  std::sort(transposed.begin(), transposed.end());
  REQUIRE(!gathered.empty() && gathered == transposed);
  // K8b: the runs cut every node's references into pieces of at most 64, and both orders hold every task once
  REQUIRE(t.node_run0.size() == t.nnode_active + 1 && t.run_r0.size() == t.run_last.size() && (size_t)t.node_run0.back() == t.run_r0.size());
  for (size_t nd = 0; nd < t.nnode_active; ++nd) {
    int at = t.ref_ptr[nd];
    for (int r = t.node_run0[nd]; r < t.node_run0[nd + 1]; ++r) {
      REQUIRE(t.run_r0[r] == at && t.run_last[r] > at && t.run_last[r] - at <= 64);
      at = t.run_last[r];
    }
    REQUIRE(at == t.ref_ptr[nd + 1]);
  }
  check_order(t.node_order, t.nnode_active * nchunk, sched.waves);
  check_order(t.run_order, t.run_r0.size() * nchunk, sched.waves);
  // K9
  REQUIRE(t.st_nb.size() == t.nnode_active * 27 && t.st_w.size() == t.st_nb.size() && t.node_gas.size() == t.nnode_active);
  for (size_t i = 0; i < t.st_nb.size(); ++i) {
    REQUIRE(t.st_nb[i] >= -1 && t.st_nb[i] < (int)t.nnode_active && std::isfinite(t.st_w[i]));
    REQUIRE((t.st_nb[i] < 0) == (t.st_w[i] == 0.0));
    REQUIRE(t.st_nb[i] < 0 || t.node_gas[t.st_nb[i]] == t.node_gas[i / 27]);
  }
  for (int gas : t.node_gas) REQUIRE(gas >= 0 && gas < 4);
  REQUIRE(t.inv_sigma2.size() == 5 * ng);
  for (size_t i = 0; i < 4 * ng; ++i) REQUIRE(t.inv_sigma2[i] >= 1.0 / 9.0 - 1e-12 && t.inv_sigma2[i] <= 100.0 + 1e-9);   // sigma held in [0.1, 3]
  // bands
  REQUIRE(t.band_ptr.size() == (size_t)t.nband + 1 && t.band_g.size() == ng && t.band_ptr[0] == 0);
  for (int b = 0; b < t.nband; ++b)
    for (int q = t.band_ptr[b]; q < t.band_ptr[b + 1]; ++q) REQUIRE(t.band_g[q] >= 0 && t.band_g[q] < c.ng && t.band[t.band_g[q]] == b);
  REQUIRE(t.band_ptr.back() == c.ng - (c.ng > 2));
  // per-profile arrays
  const size_t nhl = c.nlay + 1;
  REQUIRE(t.planck.size() == t.ncol * nhl * ng && t.semis.size() == t.ncol * t.nband && t.conv.size() == t.ncell && t.lw.size() == t.ncell);
  REQUIRE(t.hr.size() == t.ncell * t.nband && t.fdn.size() == t.ncol * nhl * t.nband && t.fup.size() == t.fdn.size());
  REQUIRE(t.have_boundary && t.sfds.size() == t.ncol * ng && t.sfut.size() == t.sfds.size() && t.mu0.size() == (c.sw ? t.ncol : 0));
  REQUIRE(t.rel.size() == t.ncol * 2 * nhl * ng && t.rel[3 * 2 * nhl * ng] == 0.0);   // the second scene brings none
  for (double v : t.lw) REQUIRE(std::isfinite(v));
  for (double v : t.planck) REQUIRE(std::isfinite(v));
  // initial state and bounds
  std::vector<double> x(t.nx), lo(t.nx), hi(t.nx);
  ot::initial_state(t, x.data(), lo.data(), hi.data());
  for (size_t e = 0; e < t.nx; ++e) REQUIRE(t.k0[e] > 0.0 ? (lo[e] <= x[e] && x[e] <= hi[e]) : x[e] == ot::MIN_X);
}

static void check_refusals() {
  what = "refusals";
  std::mt19937_64 rng(1);
  const Case c = {12, 5, 16, 4, 18, false, false};
  std::string err;
  { Problem p(c, rng); REQUIRE(ot::check_arguments(&p.m, 2, p.scenes, &p.cfg, err) == ECCKD_OK); }
  { Problem p(c, rng); REQUIRE(ot::check_arguments(nullptr, 2, p.scenes, &p.cfg, err) == ECCKD_PARAMETER_ERROR); }
  { Problem p(c, rng); p.m.nt = 1; REQUIRE(ot::check_arguments(&p.m, 2, p.scenes, &p.cfg, err) == ECCKD_PARAMETER_ERROR); }
  { Problem p(c, rng); p.m.ntp = 1; REQUIRE(ot::check_arguments(&p.m, 2, p.scenes, &p.cfg, err) == ECCKD_PARAMETER_ERROR); }
  { Problem p(c, rng); p.m.logarithmic_interpolation = 1; REQUIRE(ot::check_arguments(&p.m, 2, p.scenes, &p.cfg, err) == ECCKD_PARAMETER_ERROR); }
  { Problem p(c, rng); p.gases[1].nconc = 1; REQUIRE(ot::check_arguments(&p.m, 2, p.scenes, &p.cfg, err) == ECCKD_PARAMETER_ERROR && err == "ecckd_opt_create: gas 1 is ill-defined"); }
  { Problem p(c, rng); for (auto& g : p.gases) g.is_active = 0; REQUIRE(ot::check_arguments(&p.m, 2, p.scenes, &p.cfg, err) == ECCKD_PARAMETER_ERROR); }
  { Problem p(c, rng); p.scenes[0].nlay = p.scenes[1].nlay = 129; REQUIRE(ot::check_arguments(&p.m, 2, p.scenes, &p.cfg, err) == ECCKD_PARAMETER_ERROR); }
  { Problem p(c, rng); p.scenes[1].nband = 2; REQUIRE(ot::check_arguments(&p.m, 2, p.scenes, &p.cfg, err) == ECCKD_PARAMETER_ERROR && err == "ecckd_opt_create: scene 1 is inconsistent (nlay/nband/arrays)"); }
}

// Tables::rayleigh_active.  With active gases: against the tables of the same problem without the flag - the Rayleigh row sits
// directly behind the active gases (its ng elements are the tail of the state: no bounds, no node), the fixed gas moves up by
// ng, and everything that is not an offset into k is the same bytes.  Rayleigh alone: every gas inactive, the state is the ng
// elements and K8b / K9 have no node.  A zero coefficient is pinned at MIN_X.  The flag on a longwave model is refused.
static int check_rayleigh_active() {
  int ncase = 0;
  for (int ng : {1, 64, 65})
    for (int nlay : {1, 128}) {
      static char label[96];
      std::snprintf(label, sizeof(label), "rayleigh_active ng=%d nlay=%d", ng, nlay);
      what = label;
      const Case c = {ng, 5, 16, 4, nlay, true, false};
      const ot::Schedule sched = {4, 64, false};
      std::string err;
      std::mt19937_64 rng0(99), rng1(99), rng2(99);
      Problem p0(c, rng0), p1(c, rng1), p2(c, rng2);
      if (ng > 2) p1.rayleigh[2] = p0.rayleigh[2] = 0.0;          // a zero coefficient
      ot::Tables t0, t1, t2;
      t1.rayleigh_active = true;
      t2.rayleigh_active = true;
      REQUIRE(ot::build_tables(&p0.m, 2, p0.scenes, &p0.cfg, sched, t0, err) == ECCKD_OK);
      REQUIRE(ot::build_tables(&p1.m, 2, p1.scenes, &p1.cfg, sched, t1, err) == ECCKD_OK);
      const size_t n = ng;
      // flag with active gases
      REQUIRE(t1.nx == t0.nx + n && t1.nk == t0.nk && t1.nnode_active == t0.nnode_active && t1.rayleigh_ix == t0.nx && t0.rayleigh_ix == t0.nk - n);
      REQUIRE(t1.kmin.size() == t1.nx && t1.kmax.size() == t1.nx && t1.k0.size() == t1.nk && t1.moles.size() == t1.ncell && t0.moles.empty());
      for (size_t e = 0; e < t0.nx; ++e) REQUIRE(t1.k0[e] == t0.k0[e] && t1.kmin[e] == t0.kmin[e] && t1.kmax[e] == t0.kmax[e]);
      for (size_t g = 0; g < n; ++g) REQUIRE(t1.k0[t1.rayleigh_ix + g] == p1.rayleigh[g] && t1.kmin[t0.nx + g] == 0.0 && t1.kmax[t0.nx + g] == 0.0);
      for (size_t e = t0.nx; e < t0.nk - n; ++e) REQUIRE(t1.k0[e + n] == t0.k0[e]);      // the fixed gas, moved up by ng
      REQUIRE(t1.nent == t0.nent && t1.ray_ent == t0.ray_ent && t1.ent_coef == t0.ent_coef && t1.ent_idx.size() == t0.ent_idx.size());
      for (size_t i = 0; i < t0.ent_idx.size(); ++i) {
        const int a = t0.ent_idx[i], b = t1.ent_idx[i];
        const bool ray = (int)(i % t0.nent) == t0.ray_ent;
        REQUIRE(ray ? (a == (int)t0.rayleigh_ix && b == (int)t1.rayleigh_ix) : (a < 0 || (size_t)a < t0.nx) ? b == a : b == a + ng);
        if (ray) REQUIRE(t1.moles[i / t0.nent] == t1.ent_coef[i] && t1.moles[i / t0.nent] > 0.0);
      }
      REQUIRE(t1.ref_ptr == t0.ref_ptr && t1.ref_cell == t0.ref_cell && t1.ref_coef == t0.ref_coef && t1.node_order == t0.node_order &&
              t1.run_order == t0.run_order && t1.run_r0 == t0.run_r0 && t1.run_last == t0.run_last && t1.node_run0 == t0.node_run0);
      REQUIRE(t1.st_nb == t0.st_nb && t1.st_w == t0.st_w && t1.inv_sigma2 == t0.inv_sigma2 && t1.node_gas == t0.node_gas);
      REQUIRE(t1.planck == t0.planck && t1.hr == t0.hr && t1.lw == t0.lw && t1.rel == t0.rel && t1.band_g == t0.band_g);
      {
        std::vector<double> x0(t0.nx), lo0(t0.nx), hi0(t0.nx), x(t1.nx), lo(t1.nx), hi(t1.nx);
        ot::initial_state(t0, x0.data(), lo0.data(), hi0.data());
        ot::initial_state(t1, x.data(), lo.data(), hi.data());
        for (size_t e = 0; e < t0.nx; ++e) REQUIRE(x[e] == x0[e] && lo[e] == lo0[e] && hi[e] == hi0[e]);
        for (size_t g = 0; g < n; ++g) {
          const size_t e = t0.nx + g;
          REQUIRE(lo[e] == -INFINITY && hi[e] == INFINITY);                               // no bounds, with min / max tables present
          REQUIRE(p1.rayleigh[g] > 0.0 ? x[e] == std::log(p1.rayleigh[g]) : x[e] == ot::MIN_X);
        }
        if (ng > 2) REQUIRE(x[t0.nx + 2] == ot::MIN_X);
      }
      // Rayleigh alone
      for (auto& g : p2.gases) g.is_active = 0;
      REQUIRE(ot::check_arguments(&p2.m, 2, p2.scenes, &p2.cfg, err) == ECCKD_PARAMETER_ERROR && err == "ecckd_opt_create: no active gas to optimise");
      REQUIRE(ot::build_tables(&p2.m, 2, p2.scenes, &p2.cfg, sched, t2, err) == ECCKD_OK);
      REQUIRE(t2.nx == n && t2.nk == t0.nk && t2.rayleigh_ix == 0 && t2.nnode_active == 0 && t2.kmin == std::vector<double>(n, 0.0) && t2.kmax == t2.kmin);
      REQUIRE(t2.ref_ptr.size() == 1 && t2.ref_cell.empty() && t2.run_r0.empty() && t2.node_run0.size() == 1 && t2.st_nb.empty() && t2.node_gas.empty());
      for (int v : t2.node_order) REQUIRE(v == -1);
      for (int v : t2.run_order) REQUIRE(v == -1);
      for (size_t i = 0; i < t2.ent_idx.size(); ++i) {
        const int idx = t2.ent_idx[i];
        REQUIRE(idx == -1 || ((int)(i % t2.nent) == t2.ray_ent ? idx == 0 : (idx >= ng && idx % ng == 0 && (size_t)idx + n <= t2.nk)));
      }
      {
        std::vector<double> x(t2.nx), lo(t2.nx), hi(t2.nx);
        ot::initial_state(t2, x.data(), lo.data(), hi.data());
        for (size_t g = 0; g < n; ++g) REQUIRE(x[g] == std::log(p2.rayleigh[g]) && lo[g] == -INFINITY && hi[g] == INFINITY);
      }
      ncase += 2;
    }
  // the flag on a longwave model, and on a shortwave model without the coefficient
  what = "rayleigh_active refusals";
  std::mt19937_64 rng(5);
  std::string err;
  const ot::Schedule sched = {4, 64, false};
  {
    Problem p(Case{12, 5, 16, 4, 18, false, false}, rng);
    ot::Tables t;
    t.rayleigh_active = true;
    REQUIRE(ot::build_tables(&p.m, 2, p.scenes, &p.cfg, sched, t, err) == ECCKD_PARAMETER_ERROR && err.find("ECCKD_OPT_RAYLEIGH_ACTIVE") != std::string::npos);
  }
  {
    Problem p(Case{12, 5, 16, 4, 18, true, false}, rng);
    p.m.rayleigh_molar_scattering = nullptr;
    ot::Tables t;
    t.rayleigh_active = true;
    REQUIRE(ot::build_tables(&p.m, 2, p.scenes, &p.cfg, sched, t, err) == ECCKD_PARAMETER_ERROR && err.find("ECCKD_OPT_RAYLEIGH_ACTIVE") != std::string::npos);
  }
  return ncase + 2;
}

// The history over 20 accepted pairs, one rejected and one restart.  The dots are those of vectors that exist (S, Y, q random),
// so S^T Y is what a run would see; the direction's coefficients are checked through R u = p.
static void check_history() {
  what = "history";
  constexpr int M = ecckd::LbfgsHistory::M, N = 40;
  std::mt19937_64 rng(7);
  std::normal_distribution<double> nrm;
  auto dot = [](const std::vector<double>& a, const std::vector<double>& b) { double s = 0.0; for (int i = 0; i < N; ++i) s += a[i] * b[i]; return s; };
  std::vector<std::vector<double>> S(M, std::vector<double>(N)), Y(M, std::vector<double>(N));
  ecckd::LbfgsHistory lb;
  double dots[3 + 5 * M];
  int accepted = 0;
  for (int round = 0; round < 24; ++round) {
    const int slot = lb.next_slot();
    REQUIRE(slot >= 0 && slot < M && lb.pending && lb.n < M);
    for (int a = 0; a < lb.n; ++a) REQUIRE(lb.ord[a] != slot);
    const bool reject = round == 9;
    for (int i = 0; i < N; ++i) { S[slot][i] = nrm(rng); Y[slot][i] = (reject ? -1.0 : 1.0) * S[slot][i] + 0.1 * nrm(rng); }
    std::vector<double> q(N);
    for (double& v : q) v = nrm(rng);
    int slots[M];
    lb.slots(slots);
    for (double& v : dots) v = 0.0;
    dots[0] = dot(q, q);
    for (int a = 0; a <= lb.n; ++a) {                          // the stored pairs, then the pending one as the newest
      const int s = a < lb.n ? slots[a] : slot;
      dots[1 + a] = dot(S[s], q);
      dots[1 + M + a] = dot(Y[s], q);
    }
    double* rp = dots + 1 + 2 * M;
    rp[0] = dot(S[slot], Y[slot]); rp[1] = dot(Y[slot], Y[slot]);
    for (int a = 0; a < lb.n; ++a) { rp[2 + a] = dot(S[slot], Y[slots[a]]); rp[2 + M + a] = dot(S[slots[a]], Y[slot]); rp[2 + 2 * M + a] = dot(Y[slot], Y[slots[a]]); }
    const int before = lb.n;
    lb.absorb_pending(dots);
    REQUIRE(!lb.pending && lb.n == before + (reject ? 0 : 1) && lb.n <= M);
    accepted += !reject;
    if (!reject) REQUIRE(lb.ord[lb.n - 1] == slot && lb.gamma == rp[0] / rp[1]);
    lb.slots(slots);
    for (int a = 0; a < M; ++a)
      for (int b = 0; b < a; ++b) REQUIRE(a >= lb.n || slots[a] != slots[b]);
    double cs[M], cy[M];
    const double gamma = lb.coefficients(dots, cs, cy);
    REQUIRE(gamma == (lb.n > 0 ? lb.gamma : 1.0));
    for (int a = 0; a < M; ++a) REQUIRE(std::isfinite(cs[a]) && std::isfinite(cy[a]) && (a < lb.n || (cs[a] == 0.0 && cy[a] == 0.0)));
    if (!reject)
      for (int a = 0; a < lb.n; ++a) {                         // R u = p with u = cy / gamma, R the upper triangle of S^T Y in age order
        double r = -dots[1 + a];
        for (int b = a; b < lb.n; ++b) r += dot(S[slots[a]], Y[slots[b]]) * cy[b] / gamma;
        REQUIRE(std::fabs(r) < 1e-8 * (1.0 + std::fabs(dots[1 + a])));
      }
    if (round == 15) { lb.restart(); REQUIRE(lb.n == 0 && lb.coefficients(dots, cs, cy) == 1.0 && cs[0] == 0.0); }
  }
  REQUIRE(accepted == 23 && lb.n == M);
}

// The LDS layouts of the three K8a kernels (csrc/opt_lds.hpp) against the byte formulas the host plan used before the kernels
// and the plan shared one header, written out here as literals.  Every array has the size its kernel indexes it with, so the
// arrays neither overlap nor leave a gap; the doubles start on 8 bytes and the int (or byte) arrays follow them.
template <int N>
static void check_layout(const ecckd::opt_lds::Layout<N>& l, const size_t (&size)[N], int ndouble_arrays, size_t total) {
  REQUIRE(l.off[0] == 0 && l.bytes() == total);
  size_t doubles_end = 0;
  for (int i = 0; i < N; ++i) {
    REQUIRE(l.off[i + 1] - l.off[i] == size[i] && l.off[i + 1] >= l.off[i]);
    if (i < ndouble_arrays) { REQUIRE(l.off[i] % 8 == 0 && size[i] % 8 == 0); doubles_end = l.off[i + 1]; }
    else REQUIRE(l.off[i] >= doubles_end && l.off[i] % 4 == 0);
  }
}

static int check_lds() {
  namespace lds = ecckd::opt_lds;
  static char label[96];
  int ncase = 0;
  for (size_t nlay : {1, 17, 54, 128})
    for (size_t ng : {1, 64, 70})
      for (size_t nband : {1, 13}) {
        const size_t nhl = nlay + 1, d = sizeof(double), flux = nhl * ng * d, band = nhl * nband * d;
        for (int sw = 0; sw < 2; ++sw) {
          std::snprintf(label, sizeof(label), "LDS nlay=%zu ng=%zu nband=%zu sw=%d", nlay, ng, nband, sw);
          what = label;
          const size_t cells_total = ((sw ? (size_t)0 : nlay * ng) + 2 * nhl * ng + 2 * nhl * nband + nlay * nband + nlay + 2 * nhl + 16) * sizeof(double) +
                                     (nband + 1 + ng) * sizeof(int);
          const size_t cells_size[lds::CL_COUNT] = {sw ? 0 : nlay * ng * d, flux, flux, band, band, nlay * nband * d, nlay * d, nhl * d, nhl * d,
                                                    16 * d, (nband + 1) * 4, ng * 4};
          check_layout(lds::cells((int)nlay, (int)ng, (int)nband, sw != 0), cells_size, lds::CL_BP, cells_total);
          ++ncase;
        }
        std::snprintf(label, sizeof(label), "LDS nlay=%zu ng=%zu nband=%zu", nlay, ng, nband);
        const size_t rayleigh_total = (4 * nhl * nband + nlay * nband + nlay + 2 * nhl + 16) * sizeof(double) + (nband + 1 + ng) * sizeof(int);
        const size_t rayleigh_size[lds::RL_COUNT] = {band, band, band, band, nlay * nband * d, nlay * d, nhl * d, nhl * d, 16 * d, (nband + 1) * 4, ng * 4};
        check_layout(lds::rayleigh((int)nlay, (int)ng, (int)nband), rayleigh_size, lds::RL_BP, rayleigh_total);
        const size_t general_total = (nlay * ng + 2 * nhl * ng + 4 * nhl * nband + 16) * sizeof(double) + (nlay * ng + 15) / 16 * 16;
        const size_t general_size[lds::GL_COUNT] = {nlay * ng * d, flux, flux, band, band, band, band, 16 * d, (nlay * ng + 15) / 16 * 16};
        check_layout(lds::general((int)nlay, (int)ng, (int)nband), general_size, lds::GL_CLAMP, general_total);
        ncase += 2;
      }
  // the figures in the comment of k_opt_forward_adjoint_cells, at the benchmark's shapes (13 bands): 100 KiB longwave - one block
  // per CU -, 73 KiB shortwave - two
  what = "LDS of the cell-parallel kernel at nlay = 54, ng = 64, nband = 13";
  const size_t lw = lds::cells(54, 64, 13, false).bytes(), sw = lds::cells(54, 64, 13, true).bytes();
  REQUIRE(lw == 102776 && lw / 1024 == 100 && sw == 75128 && sw / 1024 == 73 && 2 * sw <= 160 * 1024 && 2 * lw > 160 * 1024);
  return ncase;
}

// The host step of ecckd_opt_set_gpoint_truth (check_gpoint_truth) at the edge shapes - one layer, 1 / 64 / 65 g points, one and two
// columns -: a finite truth passes and every element of it is read (the last one made NaN or infinite is found), a removal
// passes with no truth at all, the refusals refuse; and the level weights of the term add up to the layer weights' sum.
static int check_gpoint() {
  static char label[96];
  std::string err;
  int ncase = 0;
  for (size_t ncol : {1, 2})
    for (size_t nlay : {1, 7, 8, 9, 17})
      for (size_t ng : {1, 3, 64, 65}) {
        std::snprintf(label, sizeof(label), "gpoint truth ncol=%zu nlay=%zu ng=%zu", ncol, nlay, ng);
        what = label;
        const size_t count = ncol * 2 * (nlay + 1) * ng;
        std::vector<double> truth(count, 1.5);
        REQUIRE(ot::check_gpoint_truth(false, false, false, 0.1, truth.data(), count, err) == ECCKD_OK);
        for (const double bad : {(double)NAN, (double)INFINITY}) {
          for (const size_t at : {(size_t)0, count - 1}) {
            truth[at] = bad;
            REQUIRE(ot::check_gpoint_truth(false, false, false, 0.1, truth.data(), count, err) == ECCKD_PARAMETER_ERROR && !err.empty());
            // (a removal reads no truth)
            REQUIRE(ot::check_gpoint_truth(false, false, false, 0.0, truth.data(), count, err) == ECCKD_OK);
            truth[at] = 1.5;
          }
        }
        REQUIRE(ot::check_gpoint_truth(false, false, false, 0.0, nullptr, count, err) == ECCKD_OK);
        REQUIRE(ot::check_gpoint_truth(false, false, false, 0.1, nullptr, count, err) == ECCKD_OK);
        REQUIRE(ot::check_gpoint_truth(false, false, false, -1.0, truth.data(), count, err) == ECCKD_OK);
        REQUIRE(ot::check_gpoint_truth(true, false, false, 0.1, truth.data(), count, err) == ECCKD_PARAMETER_ERROR);
        REQUIRE(ot::check_gpoint_truth(true, false, false, 0.0, nullptr, count, err) == ECCKD_PARAMETER_ERROR);
        REQUIRE(ot::check_gpoint_truth(false, true, false, 0.1, truth.data(), count, err) == ECCKD_PARAMETER_ERROR);
        REQUIRE(ot::check_gpoint_truth(false, false, true, 0.1, truth.data(), count, err) == ECCKD_PARAMETER_ERROR);
        REQUIRE(ot::check_gpoint_truth(false, false, false, (double)NAN, truth.data(), count, err) == ECCKD_PARAMETER_ERROR);
        REQUIRE(ot::check_gpoint_truth(false, false, false, (double)INFINITY, truth.data(), count, err) == ECCKD_PARAMETER_ERROR);
        REQUIRE(ot::gpoint_truth_active(0.1, truth.data()) && !ot::gpoint_truth_active(0.0, truth.data()) && !ot::gpoint_truth_active(0.1, nullptr));
        std::vector<double> lw(nlay);
        for (size_t l = 0; l < nlay; ++l) lw[l] = (1.0 + (double)l) / (0.5 * (double)nlay * ((double)nlay + 1.0));
        double sum = 0.0;
        for (size_t i = 0; i <= nlay; ++i) sum += ot::gpoint_level_weight(lw.data(), (int)nlay, (int)i);
        REQUIRE(std::fabs(sum - 1.0) < 1e-14);
        if (nlay == 1) REQUIRE(ot::gpoint_level_weight(lw.data(), 1, 0) == 0.5 && ot::gpoint_level_weight(lw.data(), 1, 1) == 0.5);
        ++ncase;
      }
  return ncase;
}

int main() {
  const int ngp = check_gpoint();
  const int nlds = check_lds();
  std::mt19937_64 rng(2024);
  int ncase = 0;
  for (int ng : {1, 64, 65})
    for (int nlay : {1, 128})
      for (int small : {0, 1})
        for (int sw : {0, 1}) {
          const Case c = {ng, small ? 2 : 5, small ? 2 : 16, small ? 2 : 4, nlay, sw != 0, (ncase % 3) == 1};
          check_tables(c, rng);
          ++ncase;
        }
  check_refusals();
  check_history();
  const int nray = check_rayleigh_active();
  std::printf("check_opt_tables: %d LDS layouts, %d table cases, %d cases of the optimised Rayleigh row, %d shapes of the per-g truth, "
              "the refusals and the history: no complaint\n",
              nlds, ncase, nray, ngp);
  return 0;
}
