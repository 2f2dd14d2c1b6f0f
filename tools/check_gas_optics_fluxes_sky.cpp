// Harness for the host step of the sky argument of the fused fluxes (check_fluxes_sky of csrc/gas_optics_tables.cpp): every
// refusal by its message, under the name of the entry that was called, and what a sound argument reports (sky_given).
// No device, no Python.
// build: g++ -O1 -g -std=c++17 -Iecckd_amd/csrc tools/check_gas_optics_fluxes_sky.cpp ecckd_amd/csrc/gas_optics_tables.cpp \
//        ecckd_amd/csrc/opt_tables.cpp -o /tmp/check_gas_optics_fluxes_sky && /tmp/check_gas_optics_fluxes_sky
#include <cstdio>
#include <cstdlib>
#include <string>
#include "gas_optics_tables.hpp"
namespace go = ecckd::gas_optics;

static std::string what;
static int checks = 0;

#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    ++checks;                                                                          \
    if (!(cond)) { std::printf("%s:%d: %s does not hold (%s)\n", __FILE__, __LINE__, #cond, what.c_str()); std::exit(1); } \
  } while (0)

int main() {
  go::Flat lw, sw;
  for (go::Flat* f : {&lw, &sw}) {
    f->ng = 4; f->ngas = 1; f->nent = 4; f->nband = 2; f->iband = {1, 0, 1, 0};
    f->gases.assign(1, go::GasDesc{});
  }
  sw.is_sw = true; sw.has_rayleigh = true; sw.solar_irradiance = {1.0, 2.0, 3.0, 4.0};
  go::Flat bare_lw = lw, bare_sw = sw;
  for (go::Flat* f : {&bare_lw, &bare_sw}) { f->nband = 0; f->iband.clear(); }
  int dummy = 0;
  const double d = 0.0;
  ecckd_flux_outputs o{};
  o.flux_dn = &dummy;
  std::string err;
  bool given = false;
  auto args = [&](bool sw_call, const ecckd_flux_sky* s) {
    return go::FluxCallArgs{sw_call, 0, sw_call ? 1 : 0, 3, 7, true, true, true, true, nullptr, ECCKD_F64, &o, true, s};
  };
  auto sky = [&](bool od, bool ssa, bool asym, bool emis, bool skin, int de) {
    return ecckd_flux_sky{od ? &d : nullptr, ssa ? &d : nullptr, asym ? &d : nullptr, emis ? &d : nullptr, skin ? &d : nullptr, de};
  };
  auto refused = [&](const go::Flat& f, bool sw_call, const ecckd_flux_sky& s, const char* word) {
    err.clear();
    given = true;
    const int rc = go::check_fluxes_sky(f, args(sw_call, &s), given, err);
    what = std::string("refusal: ") + word + " in \"" + err + "\"";
    REQUIRE(rc == ECCKD_PARAMETER_ERROR);
    REQUIRE(err.find(word) != std::string::npos);
    REQUIRE(err.find(sw_call ? "ecckd_gas_optics_fluxes_sw_sky_dev: " : "ecckd_gas_optics_fluxes_lw_sky_dev: ") == 0);
    REQUIRE(!given);
  };
  auto sound = [&](const go::Flat& f, bool sw_call, const ecckd_flux_sky* s, bool want_given) {
    given = !want_given;
    what = "a sound argument";
    REQUIRE(go::check_fluxes_sky(f, args(sw_call, s), given, err) == ECCKD_OK);
    REQUIRE(given == want_given);
  };
  // sound: NULL, all NULL (with and without the flag), each longwave input alone, the shortwave triple
  sound(lw, false, nullptr, false);
  sound(sw, true, nullptr, false);
  { const ecckd_flux_sky s = sky(0, 0, 0, 0, 0, 0); sound(lw, false, &s, false); sound(sw, true, &s, false); }
  { const ecckd_flux_sky s = sky(0, 0, 0, 0, 0, 1); sound(sw, true, &s, false); }
  { const ecckd_flux_sky s = sky(1, 0, 0, 0, 0, 0); sound(lw, false, &s, true); }
  { const ecckd_flux_sky s = sky(0, 0, 0, 1, 0, 0); sound(lw, false, &s, true); }
  { const ecckd_flux_sky s = sky(0, 0, 0, 0, 1, 0); sound(lw, false, &s, true); sound(bare_lw, false, &s, true); }
  { const ecckd_flux_sky s = sky(1, 0, 0, 1, 1, 0); sound(lw, false, &s, true); }
  { const ecckd_flux_sky s = sky(1, 1, 1, 0, 0, 0); sound(sw, true, &s, true); }
  { const ecckd_flux_sky s = sky(1, 1, 1, 0, 0, 1); sound(sw, true, &s, true); }
  // delta_eddington outside {0, 1}
  refused(sw, true, sky(1, 1, 1, 0, 0, 2), "must be 0 or 1, not 2");
  refused(sw, true, sky(0, 0, 0, 0, 0, -1), "must be 0 or 1, not -1");
  refused(lw, false, sky(1, 0, 0, 0, 0, 7), "must be 0 or 1, not 7");
  // shortwave: the triple whole or absent, no longwave surface
  refused(sw, true, sky(1, 0, 1, 0, 0, 1), "cloud_od is given without sky.cloud_ssa");
  refused(sw, true, sky(1, 1, 0, 0, 0, 1), "cloud_od is given without sky.cloud_asymmetry");
  refused(sw, true, sky(0, 1, 0, 0, 0, 1), "cloud_ssa is given without sky.cloud_od");
  refused(sw, true, sky(0, 0, 1, 0, 0, 1), "cloud_asymmetry is given without sky.cloud_od");
  refused(sw, true, sky(1, 1, 1, 1, 0, 1), "surface_emissivity belongs to the longwave call");
  refused(sw, true, sky(0, 0, 0, 0, 1, 0), "skin_temperature belongs to the longwave call");
  // longwave: no scattering inputs
  refused(lw, false, sky(1, 1, 0, 0, 0, 0), "cloud_ssa belongs to the shortwave call");
  refused(lw, false, sky(1, 0, 1, 0, 0, 0), "cloud_asymmetry belongs to the shortwave call");
  refused(lw, false, sky(1, 0, 0, 0, 0, 1), "delta_eddington = 1 belongs to the shortwave call");
  // band-indexed inputs on a model without iband_per_g
  refused(bare_lw, false, sky(1, 0, 0, 0, 0, 0), "sky.cloud_od is indexed by band");
  refused(bare_lw, false, sky(0, 0, 0, 1, 0, 0), "sky.surface_emissivity is indexed by band");
  refused(bare_sw, true, sky(1, 1, 1, 0, 0, 1), "sky.cloud_od is indexed by band");
  // the clear refusals carry the sky entries' names: the wrong kind of handle
  {
    uint32_t present = 0; int mode = -1; unsigned wants = 0;
    what = "wrong kind of handle";
    REQUIRE(go::check_fluxes_call(sw, args(false, nullptr), present, mode, wants, err) == ECCKD_PARAMETER_ERROR);
    REQUIRE(err.find("ecckd_gas_optics_fluxes_lw_sky_dev: the handle holds a shortwave model") == 0);
    REQUIRE(go::check_fluxes_call(lw, args(true, nullptr), present, mode, wants, err) == ECCKD_PARAMETER_ERROR);
    REQUIRE(err.find("ecckd_gas_optics_fluxes_sw_sky_dev: the handle holds a longwave model") == 0);
    REQUIRE(go::check_fluxes_call(sw, args(true, nullptr), present, mode, wants, err) == ECCKD_OK && mode == go::FLUX_SW_TWOSTREAM);
    REQUIRE(go::check_fluxes_call(lw, args(false, nullptr), present, mode, wants, err) == ECCKD_OK && mode == go::FLUX_LW);
  }
  std::printf("%d checks of the sky argument: all hold\n", checks);
  return 0;
}
