// ASan/UBSan harness for the host step of the gas-optics handle (csrc/gas_optics_tables.cpp): flattens models of 1 / 33 / 64 / 65
// g points with every concentration dependence, longwave and shortwave with and without Rayleigh coefficients, and checks the
// flattened tables against the model element by element; the refusals of the model check, of a call and of the launch plan; the
// plan at the tile's edges and for ncol * nlay * ng > 2^32; the incoming flux.  No device, no Python.
// build: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iecckd_amd/csrc tools/check_gas_optics_tables.cpp \
//        ecckd_amd/csrc/gas_optics_tables.cpp ecckd_amd/csrc/opt_tables.cpp -o /tmp/check_gas_optics_tables && /tmp/check_gas_optics_tables
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "gas_optics_tables.hpp"
namespace go = ecckd::gas_optics;

#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    if (!(cond)) { std::printf("%s:%d: %s does not hold (%s)\n", __FILE__, __LINE__, #cond, what.c_str()); std::exit(1); } \
  } while (0)

static std::string what;

// a model whose vectors own what the C structs point to; gas i has concentration dependence conc[i]
struct Problem {
  std::vector<double> log_p, temperature, tpl, planck, ssi, rayleigh, vmr_lut;
  std::vector<int> iband;
  std::vector<std::vector<double>> k;
  std::vector<ecckd_opt_gas> gases;
  ecckd_opt_model m{};

  Problem(int ng, int nt, int np, int nconc, const std::vector<int>& conc, bool sw, bool with_rayleigh, std::mt19937_64& rng) {
    std::uniform_real_distribution<double> u(-0.5, 1.5);     // negative coefficients too
    for (int i = 0; i < np; ++i) log_p.push_back(std::log(2.0) + i * (std::log(110000.0) - std::log(2.0)) / (np - 1));
    for (int it = 0; it < nt; ++it)
      for (int ip = 0; ip < np; ++ip) temperature.push_back(200.0 + 12.0 * (log_p[ip] - log_p[0]) + 20.0 * it);
    for (int i = 0; i < 4; ++i) tpl.push_back(150.0 + 60.0 * i);
    for (size_t i = 0; i < tpl.size() * ng; ++i) planck.push_back(u(rng));
    for (int g = 0; g < ng; ++g) { iband.push_back(0); ssi.push_back(1.0 + u(rng)); rayleigh.push_back(1e-6 * (1.0 + u(rng))); }
    for (int i = 0; i < nconc; ++i) vmr_lut.push_back(1e-6 * std::pow(4e4, (double)i / (nconc - 1)));
    for (int c : conc) {
      k.emplace_back((size_t)(c == 2 ? nconc : 1) * nt * np * ng);
      for (double& v : k.back()) v = u(rng);
    }
    for (size_t i = 0; i < conc.size(); ++i) {
      ecckd_opt_gas g{};
      g.conc_dependence = conc[i];
      g.is_active = 0;                                        // ignored by the handle
      g.nconc = conc[i] == 2 ? nconc : 1;
      g.vmr = conc[i] == 2 ? vmr_lut.data() : nullptr;
      g.reference_vmr = 1.8e-6;
      g.molar_abs = k[i].data();
      gases.push_back(g);
    }
    m.ng = ng; m.nt = nt; m.np = np; m.ngas = (int)conc.size();
    m.log_pressure = log_p.data(); m.temperature = temperature.data(); m.iband_per_g = iband.data(); m.gases = gases.data();
    if (sw) { m.solar_irradiance = ssi.data(); m.rayleigh_molar_scattering = with_rayleigh ? rayleigh.data() : nullptr; }
    else { m.ntp = (int)tpl.size(); m.temperature_planck = tpl.data(); m.planck_function = planck.data(); }
  }
};

static int flatten_cases(std::mt19937_64& rng) {
  int n = 0;
  const std::vector<std::vector<int>> mixes = {{0}, {1}, {2}, {3}, {0, 2, 1, 3, 1}, {2, 2, 0}};
  for (int ng : {1, 33, 64, 65})
    for (const auto& conc : mixes)
      for (int mode = 0; mode < 3; ++mode) {                   // longwave, shortwave with Rayleigh, shortwave without
        const int nt = 2 + n % 4, np = 2 + n % 15, nconc = 2 + n % 3;
        what = "ng " + std::to_string(ng) + " mix " + std::to_string(conc.size()) + " mode " + std::to_string(mode);
        Problem pr(ng, nt, np, nconc, conc, mode > 0, mode == 1, rng);
        go::Flat f;
        std::string err;
        REQUIRE(go::flatten_model(&pr.m, f, err) == ECCKD_OK);
        REQUIRE(f.ng == ng && f.nt == nt && f.np == np && f.ngas == (int)conc.size());
        REQUIRE(f.is_sw == (mode > 0) && f.has_rayleigh == (mode == 1));
        REQUIRE(f.log_p_0 == pr.log_p[0] && f.d_log_p == pr.log_p[1] - pr.log_p[0] && f.d_t == pr.temperature[np] - pr.temperature[0]);
        REQUIRE(f.temperature == pr.temperature);
        int nent = 0;
        size_t off = 0;
        for (size_t i = 0; i < conc.size(); ++i) {
          const go::GasDesc& d = f.gases[i];
          REQUIRE(d.conc == conc[i] && d.nconc == (conc[i] == 2 ? nconc : 1) && d.ent0 == nent && d.nent == (conc[i] == 2 ? 8 : 4));
          REQUIRE(d.ix == off && d.reference_vmr == 1.8e-6);
          if (conc[i] == 2) REQUIRE(d.log_vmr0 == std::log(pr.vmr_lut[0]) && d.d_log_c == std::log(pr.vmr_lut[1] / pr.vmr_lut[0]));
          REQUIRE(off + pr.k[i].size() <= f.k.size());
          REQUIRE(std::memcmp(&f.k[off], pr.k[i].data(), pr.k[i].size() * sizeof(double)) == 0);
          // the last node a cell can reach: concentration nconc - 1, temperature nt - 1, pressure np - 1, g point ng - 1
          const size_t last = off + (((size_t)(d.nconc - 1) * nt + (nt - 1)) * np + (np - 1)) * ng + (ng - 1);
          REQUIRE(last == off + pr.k[i].size() - 1);
          nent += d.nent;
          off += pr.k[i].size();
        }
        REQUIRE(f.nent == nent && off == f.k.size());
        if (mode == 0) REQUIRE(f.ntp == 4 && f.temperature_planck == pr.tpl && f.planck_function == pr.planck && f.solar_irradiance.empty());
        else REQUIRE(f.solar_irradiance == pr.ssi && f.planck_function.empty() && (mode == 1 ? f.rayleigh == pr.rayleigh : f.rayleigh.empty()));
        if (mode > 0) {
          std::vector<double> inc(ng);
          go::incoming(f, 1361.0, inc.data());
          double sum = 0.0;
          for (double v : pr.ssi) sum += v;
          for (int g = 0; g < ng; ++g) REQUIRE(inc[g] == 1361.0 / sum * pr.ssi[g]);
        }
        ++n;
      }
  return n;
}

static int model_refusals(std::mt19937_64& rng) {
  int n = 0;
  auto refused = [&](const ecckd_opt_model* m, const char* word) {
    go::Flat f;
    std::string err;
    what = word;
    REQUIRE(go::flatten_model(m, f, err) == ECCKD_PARAMETER_ERROR);
    REQUIRE(err.find("ecckd_gas_optics_create") == 0 && err.find(word) != std::string::npos);
    ++n;
  };
  refused(nullptr, "NULL");
  { Problem p(8, 3, 4, 2, {0, 2}, false, false, rng); p.m.logarithmic_interpolation = 1; refused(&p.m, "logarithmic"); }
  { Problem p(8, 3, 4, 2, {0, 2}, false, false, rng); p.m.np = 1; refused(&p.m, "bad model dimensions"); }
  { Problem p(8, 3, 4, 2, {0, 2}, false, false, rng); p.m.planck_function = nullptr; refused(&p.m, "Planck"); }
  { Problem p(8, 3, 4, 2, {0, 2}, false, false, rng); p.gases[1].vmr = nullptr; refused(&p.m, "gas 1 is ill-defined"); }
  { Problem p(8, 3, 4, 2, {0, 4}, false, false, rng); refused(&p.m, "gas 1 is ill-defined"); }
  { Problem p(2, 2, 2, 2, std::vector<int>(go::MAX_GASES + 1, 1), false, false, rng); refused(&p.m, "gases"); }
  { Problem p(2, 2, 2, 2, std::vector<int>(go::MAX_GASES, 2), false, false, rng); refused(&p.m, "LDS"); }   // 256 entries per cell
  return n;
}

static int call_refusals(std::mt19937_64& rng) {
  int n = 0;
  Problem lw(8, 3, 4, 2, {0, 2, 1, 3}, false, false, rng), sw(8, 3, 4, 2, {0, 2}, true, true, rng);
  go::Flat fl, fs;
  std::string err;
  REQUIRE(go::flatten_model(&lw.m, fl, err) == ECCKD_OK && go::flatten_model(&sw.m, fs, err) == ECCKD_OK);
  const int all[4] = {1, 1, 1, 1}, none_only[4] = {1, 0, 0, 0};
  int dummy = 0;
  const void* ptrs[4] = {nullptr, &dummy, nullptr, nullptr};
  const go::CallArgs good = {3, 5, true, true, true, true, false, all, nullptr, nullptr, 0, ECCKD_F64};
  uint32_t mask = 0;
  bool any = true;
  what = "a sound call";
  REQUIRE(go::check_call(fl, good, mask, any, err) == ECCKD_OK && mask == 0xfu && !any);
  auto refused = [&](const go::Flat& f, go::CallArgs a, const char* word) {
    what = word;
    REQUIRE(go::check_call(f, a, mask, any, err) == ECCKD_PARAMETER_ERROR);
    REQUIRE(err.find("ecckd_gas_optics_dev") == 0 && err.find(word) != std::string::npos);
    ++n;
  };
  { go::CallArgs a = good; a.ncol = 0; refused(fl, a, "positive"); }
  { go::CallArgs a = good; a.nlay = -3; refused(fl, a, "positive"); }
  { go::CallArgs a = good; a.have_pressure = false; refused(fl, a, "d_pressure_hl"); }
  { go::CallArgs a = good; a.have_temperature_hl = false; refused(fl, a, "d_temperature_hl"); }
  { go::CallArgs a = good; a.out_type = 2; refused(fl, a, "out_type"); }
  { go::CallArgs a = good; a.keep_negative = 2; refused(fl, a, "keep_negative"); }
  { go::CallArgs a = good; a.keep_negative = -1; refused(fl, a, "keep_negative"); }
  { go::CallArgs a = good; a.have_rayleigh_od = true; refused(fl, a, "longwave"); }
  { go::CallArgs a = good; a.have_vmr = false; refused(fl, a, "gas 1"); }
  { go::CallArgs a = good; a.have_od = false; refused(fl, a, "no output"); }
  what = "calls that are sound";
  { go::CallArgs a = good; a.have_vmr = false; a.gas_present = none_only; REQUIRE(go::check_call(fl, a, mask, any, err) == ECCKD_OK && mask == 1u); }
  { go::CallArgs a = good; a.have_od = false; a.gas_od = ptrs; REQUIRE(go::check_call(fl, a, mask, any, err) == ECCKD_OK && any); }
  { go::CallArgs a = good; a.gas_present = nullptr; a.keep_negative = 1; a.out_type = ECCKD_F32; REQUIRE(go::check_call(fl, a, mask, any, err) == ECCKD_OK && mask == 0xfu); }
  { go::CallArgs a = good; a.have_od = false; a.have_rayleigh_od = true; REQUIRE(go::check_call(fs, a, mask, any, err) == ECCKD_OK && mask == 3u); }
  return n;
}

static int plans() {
  int n = 0;
  const int cpb = go::CELLS_PER_BLOCK;
  auto plan = [&](long long ncol, int nlay, int ng, int nent) {
    go::Plan p;
    std::string err;
    what = "plan " + std::to_string(ncol) + " x " + std::to_string(nlay) + " x " + std::to_string(ng);
    REQUIRE(go::launch_plan(ncol, nlay, ng, nent, p, err) == ECCKD_OK);
    REQUIRE(p.ncell == (size_t)ncol * nlay && p.nvalue == p.ncell * ng && p.threads == go::THREADS && p.threads % 64 == 0);
    REQUIRE((size_t)p.blocks * cpb >= p.ncell && ((size_t)p.blocks - 1) * cpb < p.ncell);
    REQUIRE(p.lds_bytes == (size_t)cpb * (12 * (size_t)nent + 8) && p.lds_bytes <= go::MAX_LDS_BYTES);
    ++n;
    return p;
  };
  for (int ng : {1, 33, 64, 65})
    for (long long ncell : {1LL, (long long)cpb - 1, (long long)cpb, (long long)cpb + 1, 2LL * cpb + 1}) REQUIRE(plan(ncell, 1, ng, 24).ncell == (size_t)ncell);
  REQUIRE(plan(9, 7, 33, 24).blocks == 1 && plan(13, 5, 33, 24).blocks == 2);
  // the sizes this is for: every index past 2^32
  const go::Plan big = plan(1000000, 137, 64, 24);
  REQUIRE(big.nvalue == 8768000000ull && big.nvalue > (1ull << 32) && big.blocks == 2140625u);
  REQUIRE(plan(2000000000LL, 60, 1, 4).ncell == 120000000000ull);
  go::Plan p;
  std::string err;
  what = "plans refused";
  REQUIRE(go::launch_plan(0, 5, 8, 24, p, err) == ECCKD_PARAMETER_ERROR && err.find("positive") != std::string::npos);
  REQUIRE(go::launch_plan(5, 0, 8, 24, p, err) == ECCKD_PARAMETER_ERROR);
  REQUIRE(go::launch_plan(2147483647LL, 128, 8, 24, p, err) == ECCKD_PARAMETER_ERROR && err.find("one launch") != std::string::npos);
  REQUIRE(go::launch_plan(5, 5, 8, 213, p, err) == ECCKD_PARAMETER_ERROR && err.find("LDS") != std::string::npos);
  REQUIRE(go::launch_plan(5, 5, 8, 212, p, err) == ECCKD_OK);
  return n + 5;
}

int main() {
  std::mt19937_64 rng(20240611);
  const int nflat = flatten_cases(rng), nmodel = model_refusals(rng), ncall = call_refusals(rng), nplan = plans();
  std::printf("check_gas_optics_tables: %d models flattened, %d model refusals, %d call refusals, %d plans: all hold\n", nflat, nmodel, ncall,
              nplan);
  return 0;
}
