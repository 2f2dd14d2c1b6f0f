// ASan/UBSan harness for the host step of the fused fluxes (fluxes_plan and check_fluxes_call of csrc/gas_optics_tables.cpp):
// walks the plan over ng 1..1024, nlay 1..200, ncol up to 2^31 - 1 and ncol * nlay * ng > 2^32, and holds every index the kernel
// of gas_optics_fluxes.hip forms against the sizes the plan gives it - the cells of a layer tile, the reduction's LDS, a
// block's scratch, the last block's last byte; the scratch stops growing with ncol once the grid is saturated; the forced grid;
// each refusal of the plan and of a call by its message.  No device, no Python.
// build: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iecckd_amd/csrc \
//        tools/check_gas_optics_fluxes_plan.cpp ecckd_amd/csrc/gas_optics_tables.cpp ecckd_amd/csrc/opt_tables.cpp \
//        -o /tmp/check_gas_optics_fluxes_plan && /tmp/check_gas_optics_fluxes_plan
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "gas_optics_tables.hpp"
namespace go = ecckd::gas_optics;

static std::string what;

#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    if (!(cond)) { std::printf("%s:%d: %s does not hold (%s)\n", __FILE__, __LINE__, #cond, what.c_str()); std::exit(1); } \
  } while (0)

static void refused(int rc, const std::string& err, const char* word) {
  what = std::string("refusal: ") + word + " in \"" + err + "\"";
  REQUIRE(rc == ECCKD_PARAMETER_ERROR);
  REQUIRE(err.find(word) != std::string::npos);
}

// every index of k_gas_optics_fluxes against the plan's sizes
static void hold_plan(long long ncol, int nlay, int ng, int nent, int mode, int cu, long long grid, const ecckd_flux_plan& p) {
  const size_t T = go::THREADS, nhl = (size_t)nlay + 1;
  REQUIRE(p.threads == go::THREADS && p.columns_per_block == std::max(1, go::THREADS / ng));
  REQUIRE((size_t)p.columns_per_block * ng <= T || p.columns_per_block == 1);
  REQUIRE(p.g_passes >= 1 && (size_t)p.g_passes * T >= (size_t)ng && (ng <= (int)T ? p.g_passes == 1 : (size_t)(p.g_passes - 1) * T < (size_t)ng));
  const size_t cells = (size_t)p.columns_per_block * p.layer_tile;
  REQUIRE(p.layer_tile >= 1 && cells <= T);                                   // one lane per cell of a tile
  const size_t width = ng <= (int)T ? T : (size_t)ng;
  REQUIRE(p.reduce_levels >= 1);
  // LDS: [cells][nent] doubles, [cells] doubles, [reduce_levels][width] doubles, [cells][nent] uint32
  REQUIRE(p.lds_bytes == cells * nent * 8 + cells * 8 + (size_t)p.reduce_levels * width * 8 + cells * nent * 4);
  REQUIRE(p.lds_bytes <= go::MAX_LDS_BYTES);
  REQUIRE((size_t)(p.columns_per_block - 1) * ng + (ng <= (int)T ? ng : 0) <= width);   // a column's g points within a reduction row
  REQUIRE(p.state_rows == go::flux_state_rows(mode));
  REQUIRE(p.ngroup == ((size_t)ncol + p.columns_per_block - 1) / p.columns_per_block);
  REQUIRE((p.ngroup - 1) * p.columns_per_block < (size_t)ncol);                // the last group holds a column
  const size_t cap = grid >= 1 ? (size_t)grid : (size_t)cu * go::FLUX_BLOCKS_PER_CU;
  REQUIRE(p.grid >= 1 && p.grid == std::min(p.ngroup, cap));
  REQUIRE(p.scratch_bytes % p.grid == 0 && (p.scratch_bytes / p.grid) % 256 == 0);
  const size_t block_doubles = p.scratch_bytes / p.grid / 8;
  // the last element of the last pass's last row, and of the broadband doubles behind the rows
  const size_t last_row = ((size_t)(p.g_passes - 1) * p.state_rows * nhl + ((size_t)(p.state_rows - 1) * nhl + (nhl - 1))) * T + (T - 1);
  const size_t bb0 = (size_t)p.g_passes * p.state_rows * nhl * T;
  REQUIRE(last_row < bb0);
  REQUIRE(bb0 + ((size_t)1 * p.columns_per_block + (p.columns_per_block - 1)) * nhl + (nhl - 1) < block_doubles);
  REQUIRE(((size_t)p.grid - 1) * block_doubles + block_doubles <= p.scratch_bytes / 8);
}

int main() {
  std::string err;
  ecckd_flux_plan p{};
  long long plans = 0;
  // ---- the walk: every ng, a spread of nlay, ncol at 1, the group edges, a saturating count and the largest
  for (int ng = 1; ng <= 1024; ++ng) {
    const int cpb = std::max(1, go::THREADS / ng);
    for (int nlay : {1, 2, 7, 53, 54, 63, 64, 65, 137, 200})
      for (long long ncol : {1LL, (long long)cpb - 1, (long long)cpb, (long long)cpb + 1, 2LL * cpb + 1, 100000LL, 1000000LL, 0x7fffffffLL}) {
        if (ncol < 1) continue;
        for (int mode = 0; mode < 3; ++mode) {
          what = "ng " + std::to_string(ng) + " nlay " + std::to_string(nlay) + " ncol " + std::to_string(ncol) + " mode " + std::to_string(mode);
          const int rc = go::fluxes_plan(ncol, nlay, ng, 24, 3, mode, mode == 0 ? 4 : 0, go::WANT_BROADBAND | go::WANT_HEATING, 256, 0, p, err);
          REQUIRE(rc == ECCKD_OK);
          hold_plan(ncol, nlay, ng, 24, mode, 256, 0, p);
          ++plans;
        }
      }
  }
  for (int nlay = 1; nlay <= 200; ++nlay)
    for (int ng : {1, 16, 33, 64, 65, 257}) {
      what = "nlay walk " + std::to_string(nlay) + " ng " + std::to_string(ng);
      REQUIRE(go::fluxes_plan(12345, nlay, ng, 24, 1, 2, 0, 31, 256, 0, p, err) == ECCKD_OK);
      hold_plan(12345, nlay, ng, 24, 2, 256, 0, p);
      ++plans;
    }
  // ---- ncol * nlay * ng > 2^32, and the scratch of a saturated grid does not depend on ncol
  what = "beyond 2^32";
  REQUIRE(go::fluxes_plan(0x7fffffffLL, 200, 1024, 24, 3, 0, 16, 31u & ~go::WANT_DIRECT, 256, 0, p, err) == ECCKD_OK);
  hold_plan(0x7fffffffLL, 200, 1024, 24, 0, 256, 0, p);
  REQUIRE(p.ngroup == 0x7fffffffULL && p.grid == 768u);
  for (int ng : {1, 16, 64, 257}) {
    ecckd_flux_plan a{}, b{};
    what = "saturated scratch ng " + std::to_string(ng);
    REQUIRE(go::fluxes_plan(100000, 54, ng, 24, 3, 0, 0, 1, 256, 0, a, err) == ECCKD_OK);
    REQUIRE(go::fluxes_plan(1000000, 54, ng, 24, 3, 0, 0, 1, 256, 0, b, err) == ECCKD_OK);
    if (a.grid == b.grid) REQUIRE(a.scratch_bytes == b.scratch_bytes);
    REQUIRE(b.grid == 768u && b.scratch_bytes >= a.scratch_bytes);
  }
  // ---- the forced grid
  what = "forced grid";
  REQUIRE(go::fluxes_plan(29, 7, 33, 24, 3, 0, 0, 1, 256, 2, p, err) == ECCKD_OK && p.grid == 2u && p.ngroup == 5u);
  hold_plan(29, 7, 33, 24, 0, 256, 2, p);
  REQUIRE(go::fluxes_plan(29, 7, 33, 24, 3, 0, 0, 1, 256, 100, p, err) == ECCKD_OK && p.grid == 5u);
  REQUIRE(go::fluxes_plan(29, 7, 33, 24, 3, 0, 0, 1, 256, 0x100000000LL, p, err) == ECCKD_OK && p.grid == 5u);
  // ---- the plan's refusals
  refused(go::fluxes_plan(0, 7, 16, 24, 3, 0, 0, 1, 256, 0, p, err), err, "positive");
  refused(go::fluxes_plan(4, 0, 16, 24, 3, 0, 0, 1, 256, 0, p, err), err, "positive");
  refused(go::fluxes_plan(0x80000000LL, 7, 16, 24, 3, 0, 0, 1, 256, 0, p, err), err, "more than one call");
  refused(go::fluxes_plan(4, 7, 0, 24, 3, 0, 0, 1, 256, 0, p, err), err, "bad plan dimensions");
  refused(go::fluxes_plan(4, 7, 16, 24, 3, 0, 0, 1, 0, 0, p, err), err, "compute units=0");
  refused(go::fluxes_plan(4, 7, 16, 24, 3, 3, 0, 1, 256, 0, p, err), err, "mode 3");
  refused(go::fluxes_plan(4, 7, 16, 24, 3, 0, 17, 1, 256, 0, p, err), err, "nangle = 17");
  refused(go::fluxes_plan(4, 7, 16, 24, 3, 0, 0, 0, 256, 0, p, err), err, "no output");
  refused(go::fluxes_plan(4, 7, 16, 24, 0, 0, 0, go::WANT_BANDS, 256, 0, p, err), err, "iband_per_g");
  refused(go::fluxes_plan(4, 7, 16, 24, 3, 1, 0, go::WANT_DIRECT, 256, 0, p, err), err, "direct outputs");
  refused(go::fluxes_plan(4, 7, 1, 64, 3, 0, 0, 1, 256, 0, p, err), err, "bytes of LDS");
  // the longest entry list a handle accepts (212) leaves no room for the reduction beside a tile of 64 cells; 190 entries do
  refused(go::fluxes_plan(4, 7, 64, 212, 3, 0, 0, 1, 256, 0, p, err), err, "212 table entries");
  what = "190 entries";
  REQUIRE(go::fluxes_plan(4, 7, 64, 190, 3, 0, 0, 1, 256, 0, p, err) == ECCKD_OK);
  hold_plan(4, 7, 64, 190, 0, 256, 0, p);
  // ---- a call's refusals
  go::Flat lw, sw;
  for (go::Flat* f : {&lw, &sw}) {
    f->ng = 4; f->ngas = 2; f->nent = 8; f->nband = 2; f->iband = {0, 0, 1, 1};
    f->gases.assign(2, go::GasDesc{});
    f->gases[1].conc = 1;
  }
  sw.is_sw = true; sw.has_rayleigh = true; sw.solar_irradiance = {1.0, 2.0, 3.0, 4.0};
  int dummy = 0, mode = -1;
  uint32_t present = 0;
  unsigned wants = 0;
  ecckd_flux_outputs o{};
  o.flux_dn = &dummy;
  auto args = [&](bool sw_call) { return go::FluxCallArgs{sw_call, 0, 0, 3, 7, true, true, true, true, nullptr, ECCKD_F64, &o}; };
  what = "sound calls";
  REQUIRE(go::check_fluxes_call(lw, args(false), present, mode, wants, err) == ECCKD_OK && mode == go::FLUX_LW && present == 3u && wants == go::WANT_BROADBAND);
  REQUIRE(go::check_fluxes_call(sw, args(true), present, mode, wants, err) == ECCKD_OK && mode == go::FLUX_SW_DIRECT);
  { go::FluxCallArgs a = args(true); a.scattering = 1; o.spectral_flux_dn_direct = &dummy; o.heating_rate = &dummy;
    REQUIRE(go::check_fluxes_call(sw, a, present, mode, wants, err) == ECCKD_OK && mode == go::FLUX_SW_TWOSTREAM);
    REQUIRE(wants == (go::WANT_BROADBAND | go::WANT_HEATING | go::WANT_DIRECT));
    refused(go::check_fluxes_call(lw, args(false), present, mode, wants, err), err, "longwave call has no direct beam");
    refused(go::check_fluxes_call(sw, args(true), present, mode, wants, err), err, "scattering = 0");
    o.spectral_flux_dn_direct = nullptr; o.heating_rate = nullptr; }
  refused(go::check_fluxes_call(sw, args(false), present, mode, wants, err), err, "shortwave model");
  refused(go::check_fluxes_call(lw, args(true), present, mode, wants, err), err, "longwave model");
  { go::FluxCallArgs a = args(false); a.nangle = 17; refused(go::check_fluxes_call(lw, a, present, mode, wants, err), err, "nangle = 17"); }
  { go::FluxCallArgs a = args(true); a.scattering = 2; refused(go::check_fluxes_call(sw, a, present, mode, wants, err), err, "scattering must be"); }
  { go::FluxCallArgs a = args(true); a.scattering = 1; sw.has_rayleigh = false;
    refused(go::check_fluxes_call(sw, a, present, mode, wants, err), err, "Rayleigh coefficients"); sw.has_rayleigh = true; }
  { go::FluxCallArgs a = args(false); a.out = nullptr; refused(go::check_fluxes_call(lw, a, present, mode, wants, err), err, "output structure"); }
  { ecckd_flux_outputs none{}; go::FluxCallArgs a = args(false); a.out = &none;
    refused(go::check_fluxes_call(lw, a, present, mode, wants, err), err, "no output"); }
  { go::Flat bare = lw; bare.nband = 0; bare.iband.clear(); o.band_flux_up = &dummy;
    refused(go::check_fluxes_call(bare, args(false), present, mode, wants, err), err, "iband_per_g");
    REQUIRE(go::check_fluxes_call(lw, args(false), present, mode, wants, err) == ECCKD_OK && (wants & go::WANT_BANDS)); o.band_flux_up = nullptr; }
  { go::FluxCallArgs a = args(false); a.have_pressure = false; refused(go::check_fluxes_call(lw, a, present, mode, wants, err), err, "d_pressure_hl"); }
  { go::FluxCallArgs a = args(false); a.have_temperature_hl = false; refused(go::check_fluxes_call(lw, a, present, mode, wants, err), err, "d_temperature_hl"); }
  { go::FluxCallArgs a = args(true); a.have_cos_sza = false; refused(go::check_fluxes_call(sw, a, present, mode, wants, err), err, "d_cos_sza"); }
  { go::FluxCallArgs a = args(false); a.have_vmr = false; refused(go::check_fluxes_call(lw, a, present, mode, wants, err), err, "gas 1");
    const int only0[2] = {1, 0}; a.gas_present = only0;
    what = "absent gas needs no mole fraction";
    REQUIRE(go::check_fluxes_call(lw, a, present, mode, wants, err) == ECCKD_OK && present == 1u); }
  { go::FluxCallArgs a = args(false); a.out_type = 2; refused(go::check_fluxes_call(lw, a, present, mode, wants, err), err, "out_type 2"); }
  what = "incoming scaling";
  REQUIRE(go::incoming_scaling(sw, 20.0) == 2.0);
  std::printf("%lld plans and the refusals: all hold\n", plans);
  return 0;
}
