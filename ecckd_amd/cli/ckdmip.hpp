// ckdmip.hpp - bin/ckdmip_lw and bin/ckdmip_sw: stand-ins for the EXTERNAL CKDMIP tools that the reference's scripts call (they are
// not part of ecCKD; test/config.h:32-35), restricted to what those scripts use and, unless ckdmip_sw is asked to scatter
// (--rayleigh, --rayleigh-scattering), to the no-scattering radiative transfer the reference itself contains.
//
// ckdmip_{lw,sw} [--config file.nam] [--scenario name] [--merge-only] [--column-range a b] [--ssi file]
//                {[--scale s | --conc c | --const c] spectrum-file}... [--ckd optical-depth-file] --output file
// ckdmip_sw      ... [--rayleigh rayleigh-spectrum-file] spectrum-file... --output file
// ckdmip_sw      ... --ckd optical-depth-file --rayleigh-scattering --output file
// ckdmip_{lw,sw} [--config file.nam] [--column-range a b] [--ssi file] --scenarios table spectrum-file...
// ckdmip_sw      ... --scenarios table --scenarios-rayleigh rayleigh-spectrum-file spectrum-file...
//
//   --merge-only   test/merge_well_mixed_lw.sh:28-31, :46-49, :60-63 (merge_well_mixed_sw.sh:35-81): the optical depths of
//                  several gas files added up, each scaled as requested, written as one spectrum file that read_spectrum /
//                  read_merged_spectrum read (what src/ecckd/merge_spectra.cpp:20-156 does too);
//   (default)      test/run_lw_lbl_evaluation.sh:286-323, test/run_sw_lbl_evaluation.sh:70-260: the line-by-line training
//                  fluxes of every column - the gases' optical depths added up with their scalings, radiative transfer per
//                  wavenumber, fluxes summed over the bands of the namelist - in the variables LblFluxes::read expects
//                  (lbl_fluxes.cpp:60-133).  Longwave: Planck function + two-stream.  Shortwave: direct beam and the
//                  upwelling flux reflected by the surface (radiative_transfer_norayleigh_sw, radiative_transfer_sw.cpp:45-77)
//                  for every cos_solar_zenith_angle of the namelist; a Rayleigh spectrum file among the inputs is one more
//                  absorber, as the reference's own forward model treats Rayleigh scattering (solve_adept.cpp:34) - the real
//                  tool scatters, which is why the reference masks the upwelling fluxes it cannot represent
//                  (LblFluxes::mask_rayleigh_up);
//   --rayleigh FILE   (ckdmip_sw, default mode) the spectrum whose optical depth SCATTERS: read and streamed like a gas file,
//                  unscaled, and not one of the gases of the output; the other files remain the absorbers.  The fluxes are
//                  those of the two-stream transfer with Rayleigh scattering (ecckd_lbl_band_fluxes_sw_rayleigh: ecRad's
//                  shortwave two-stream coefficients at asymmetry 0, Meador & Weaver's layer solution, the adding method,
//                  a Lambertian surface of albedo surf_albedo).  The output keeps its variables - flux_dn_sw now the true
//                  total, flux_up_sw and band_flux_up_sw with the scattered light - and gains band_flux_dn_sw, with
//                  do_write_spectral_boundary_fluxes spectral_flux_dn_surf_sw (direct plus diffuse), and the global
//                  attribute rayleigh_scattering = "two-stream".  The real tool's arithmetic is not among the reference's
//                  sources: agreement with it node for node is unpinned;
//   --rayleigh-scattering   (ckdmip_sw --ckd) rayleigh_optical_depth of the file scatters (ecckd_rt_sw_gpoints_rayleigh)
//                  instead of absorbing; the file must hold it.  flux_dn_sw is the true total, spectral_flux_dn_sw is added,
//                  and the same global attribute.  Neither switch goes with --merge-only or --scenarios, or with ckdmip_lw;//   --ckd file     test/run_ckd_lw.sh:133-137, test/run_ckd_sw.sh:125-128: radiative transfer on the g-point optical depths
//                  that run_ckd wrote, fluxes per column.
//   --scenarios FILE   the loop of test/run_lw_lbl_evaluation.sh:286-323 / test/run_sw_lbl_evaluation.sh:70-260 - one call per
//                  scenario, the scenarios differing in one scaling per gas file - as ONE call: FILE is a text table (`#` starts a
//                  comment, blank lines are skipped), one line per scenario,  NAME OUTPUT SPEC_1 ... SPEC_n,  exactly one SPEC per
//                  spectrum file of the command line in command-line order, a SPEC one of  asis  scale=S  conc=C  const=C  with
//                  the meanings of --scale / --conc / --const below.  Every gas file is read once per column and stays on the
//                  device; all scenarios (shortwave: and all zenith angles) are computed from that one read
//                  (ecckd_lbl_band_fluxes_lw_scenarios / _sw_scenarios), and every OUTPUT is the file the default mode would
//                  have written with `--scenario NAME --output OUTPUT` and the line's scalings.  Not with --merge-only, --ckd,
//                  --output, --scenario or a per-file --scale / --conc / --const.
//   --scenarios-rayleigh FILE   (ckdmip_sw --scenarios) the spectrum whose optical depth SCATTERS in every scenario of the
//                  table: checked against the grid as --rayleigh FILE is, read once per column, never scaled, and not one of
//                  the gases of the outputs.  All scenarios and angles come from one read of the gas files
//                  (ecckd_lbl_band_fluxes_sw_rayleigh_scenarios), and every OUTPUT is the file
//                  `--rayleigh FILE --scenario NAME --output OUTPUT` with the line's scalings would have written.  The spelling
//                  `--rayleigh FILE --scenarios TABLE` stays refused, as it always was - which is why the combination has a
//                  switch of its own.  Only with --scenarios, and not with --rayleigh, --rayleigh-scattering, --ckd,
//                  --merge-only or ckdmip_lw.
// A file may be preceded by  --scale s  (optical depth times s),  --conc c  (scaled so that the file's reference surface
// mole fraction becomes c)  or  --const c  (a mole fraction c at every level: each level scaled by c / its own).
// Namelist (&longwave_config / &shortwave_config): band_wavenumber1 / band_wavenumber2, nspectralstride (1 only), nangle (0:
// classic two-stream, diffusivity 1.66; N = 1..16: N Gauss-Legendre zenith angles per hemisphere, as test/run_ckd_lw.sh:28
// and test/copy_to_ckdmip_lw.sh:32 ask for with NANGLE=4), surf_albedo, cos_solar_zenith_angle, do_write_spectral_boundary_fluxes (the
// spectral fluxes at the surface and the top of the atmosphere per wavenumber, with the wavenumber grid); the
// *_name keys must keep their CKDMIP defaults.  Spectra are streamed from the files into HBM (ecckd_nc_read_dev) and merged
// there; the per-wavenumber radiative transfer is ecckd_lbl_band_fluxes_lw / _sw.  Output is a classic NetCDF file whatever
// its name.
#pragma once
#include <algorithm>
#include <cctype>
#include <fstream>
#include <memory>
#include <sstream>

#include "scenario_table.hpp"
#include "tool.hpp"

using namespace tool;

namespace {

struct Namelist {
  std::vector<double> band1, band2;
  int nspectralstride = 1, nangle = 0;
  bool boundary_fluxes = false;
  double surf_albedo = 0.15;                       // test/run_sw_lbl_evaluation.sh sets it
  std::vector<double> mu0;                         // cos_solar_zenith_angle
};

std::string lower(std::string s) { std::transform(s.begin(), s.end(), s.begin(), ::tolower); return s; }

// Fortran namelist, as far as the scripts' files go: `key = v, v, ...` items, `!` comments, `key(a:b)` index ranges ignored
Namelist read_namelist(const std::string& path) {
  Namelist nl;
  std::ifstream in(path);
  if (!in) fail(ECCKD_PARAMETER_ERROR, "Cannot open namelist %s", path.c_str());
  std::string text, line;
  while (std::getline(in, line)) {
    const size_t c = line.find('!');
    if (c != std::string::npos) line.erase(c);
    text += line + "\n";
  }
  // split into key = value chunks
  std::vector<std::pair<std::string, std::string>> items;
  size_t pos = 0;
  std::string key;
  while (true) {
    const size_t eq = text.find('=', pos);
    if (eq == std::string::npos) break;
    // key = the token before '=' (back to the previous separator)
    size_t k0 = text.find_last_of(",\n&", eq);
    k0 = k0 == std::string::npos ? 0 : k0 + 1;
    std::string k = text.substr(k0, eq - k0);
    k.erase(std::remove_if(k.begin(), k.end(), ::isspace), k.end());
    const size_t paren = k.find('(');
    if (paren != std::string::npos) k.erase(paren);
    // value = up to the next "key =" or the closing '/'
    size_t next_eq = text.find('=', eq + 1);
    size_t end = text.size();
    if (next_eq != std::string::npos) {
      size_t nk = text.find_last_of(",\n", next_eq);
      if (nk != std::string::npos && nk > eq) end = nk;
    }
    std::string v = text.substr(eq + 1, end - eq - 1);
    const size_t slash = v.find('/');
    if (slash != std::string::npos && v.find('"') == std::string::npos) v.erase(slash);
    items.push_back({lower(k), v});
    pos = eq + 1;
  }
  auto numbers = [](const std::string& v) {
    std::vector<double> out;
    std::string t = v;
    std::replace(t.begin(), t.end(), ',', ' ');
    std::istringstream ss(t);
    double x;
    while (ss >> x) out.push_back(x);
    return out;
  };
  auto truth = [](const std::string& v) { const std::string t = lower(v); return t.find("true") != std::string::npos || t.find(".t") != std::string::npos; };
  for (auto& kv : items) {
    if (kv.first == "band_wavenumber1") nl.band1 = numbers(kv.second);
    else if (kv.first == "band_wavenumber2") nl.band2 = numbers(kv.second);
    else if (kv.first == "nspectralstride") nl.nspectralstride = (int)numbers(kv.second).at(0);
    else if (kv.first == "nangle") nl.nangle = (int)numbers(kv.second).at(0);
    else if (kv.first == "do_write_spectral_boundary_fluxes") nl.boundary_fluxes = truth(kv.second);
    else if (kv.first == "surf_albedo") nl.surf_albedo = numbers(kv.second).at(0);
    else if (kv.first == "cos_solar_zenith_angle") nl.mu0 = numbers(kv.second);
  }
  return nl;
}

// The scaling profile of one gas file in one column and the mole fractions the output reports for it
void gas_scaling(const GasArg& g, const std::string& path, int nlay, const std::vector<double>& pressure_hl, double ref,
                 const std::vector<double>& vmr, std::vector<double>& profile, std::vector<double>& vmr_out) {
  profile.assign(nlay, 1.0); vmr_out.assign(nlay, -1.0);
  if (g.mode == GasArg::SCALE) {
    for (int l = 0; l < nlay; ++l) { profile[l] = g.value; vmr_out[l] = vmr[l] >= 0.0 ? vmr[l] * g.value : -1.0; }
  } else if (g.mode == GasArg::CONC) {
    ck(ecckd_merge_scaling(nlay, pressure_hl.data(), -1.0, g.value, ref, vmr.data(), 0, nullptr, nullptr, profile.data(), vmr_out.data()));
  } else if (g.mode == GasArg::CONST) {
    for (int l = 0; l < nlay; ++l) {
      if (!(vmr[l] > 0.0)) fail(ECCKD_PARAMETER_ERROR, "--const needs mole_fraction_fl in %s", path.c_str());
      profile[l] = g.value / vmr[l];
      vmr_out[l] = g.value;
    }
  } else {
    vmr_out = vmr;
  }
}

// The dimensions and variables of a flux file after pressure_hl / temperature_hl (what LblFluxes::read expects, lbl_fluxes.cpp:60-133)
void define_flux_variables(NcOut& out, bool sw, size_t ngas, int nmu, int nband, size_t nwav, const std::string& ids, bool boundary,
                           bool rayleigh = false) {
  if (sw) {
    out.dim("gas", ngas); out.dim("mu0", nmu); out.dim("band_sw", nband);
    out.var("mole_fraction_fl", NC_FLOAT_T, {"column", "gas", "level"}, "Mole fraction at full levels", "1");
    out.var("mu0", NC_FLOAT_T, {"mu0"}, "Cosine of solar zenith angle", "1");
    out.var("flux_up_sw", NC_FLOAT_T, {"column", "mu0", "half_level"}, "Upwelling shortwave flux", "W m-2");
    out.var("flux_dn_sw", NC_FLOAT_T, {"column", "mu0", "half_level"}, "Downwelling shortwave flux", "W m-2");
    out.var("flux_dn_direct_sw", NC_FLOAT_T, {"column", "mu0", "half_level"}, "Downwelling direct shortwave flux", "W m-2");
    out.var("band_wavenumber1_sw", NC_FLOAT_T, {"band_sw"}, "Lower bound wavenumber for shortwave band", "cm-1");
    out.var("band_wavenumber2_sw", NC_FLOAT_T, {"band_sw"}, "Upper bound wavenumber for shortwave band", "cm-1");
    out.var("band_flux_up_sw", NC_FLOAT_T, {"column", "mu0", "half_level", "band_sw"}, "Upwelling shortwave flux in bands", "W m-2");
    out.var("band_flux_dn_direct_sw", NC_FLOAT_T, {"column", "mu0", "half_level", "band_sw"}, "Downwelling direct shortwave flux in bands", "W m-2");
    if (rayleigh) out.var("band_flux_dn_sw", NC_FLOAT_T, {"column", "mu0", "half_level", "band_sw"}, "Downwelling shortwave flux in bands", "W m-2");
    out.att(ids, "constituent_id");
    if (rayleigh) out.att("two-stream", "rayleigh_scattering");
    if (boundary) {     // what LblFluxes::read maps to g points (lbl_fluxes.cpp:183-246)
      out.dim("wavenumber", nwav);
      out.var("wavenumber", NC_DOUBLE_T, {"wavenumber"}, "Wavenumber", "cm-1");
      out.var("spectral_flux_dn_direct_surf_sw", NC_FLOAT_T, {"column", "mu0", "wavenumber"}, "Spectral direct shortwave flux at the surface", "W m-2");
      out.var("spectral_flux_up_toa_sw", NC_FLOAT_T, {"column", "mu0", "wavenumber"}, "Spectral upwelling shortwave flux at top of atmosphere", "W m-2");
      if (rayleigh) out.var("spectral_flux_dn_surf_sw", NC_FLOAT_T, {"column", "mu0", "wavenumber"}, "Spectral shortwave flux at the surface", "W m-2");
    }
  } else {
    out.dim("gas", ngas); out.dim("band_lw", nband);
    out.var("mole_fraction_fl", NC_FLOAT_T, {"column", "gas", "level"}, "Mole fraction at full levels", "1");
    out.var("flux_up_lw", NC_FLOAT_T, {"column", "half_level"}, "Upwelling longwave flux", "W m-2");
    out.var("flux_dn_lw", NC_FLOAT_T, {"column", "half_level"}, "Downwelling longwave flux", "W m-2");
    out.var("band_wavenumber1_lw", NC_FLOAT_T, {"band_lw"}, "Lower bound wavenumber for longwave band", "cm-1");
    out.var("band_wavenumber2_lw", NC_FLOAT_T, {"band_lw"}, "Upper bound wavenumber for longwave band", "cm-1");
    out.var("band_flux_up_lw", NC_FLOAT_T, {"column", "half_level", "band_lw"}, "Upwelling longwave flux in bands", "W m-2");
    out.var("band_flux_dn_lw", NC_FLOAT_T, {"column", "half_level", "band_lw"}, "Downwelling longwave flux in bands", "W m-2");
    out.att(ids, "constituent_id");
    if (boundary) {     // lbl_fluxes.cpp:301-325
      out.dim("wavenumber", nwav);
      out.var("wavenumber", NC_DOUBLE_T, {"wavenumber"}, "Wavenumber", "cm-1");
      out.var("spectral_flux_dn_surf_lw", NC_FLOAT_T, {"column", "wavenumber"}, "Spectral downwelling longwave flux at the surface", "W m-2");
      out.var("spectral_flux_up_toa_lw", NC_FLOAT_T, {"column", "wavenumber"}, "Spectral upwelling longwave flux at top of atmosphere", "W m-2");
    }
  }
}

// [band][level] fluxes -> (half_level, band) and the sums over the bands
void bands_to_file_order(int nband, size_t nhl, const double* b, double* t /* [nhl][nband] */, double* sum /* [nhl] */) {
  for (size_t i = 0; i < nhl; ++i) sum[i] = 0.0;
  for (int k = 0; k < nband; ++k)
    for (size_t i = 0; i < nhl; ++i) {
      t[i * nband + k] = b[(size_t)k * nhl + i];
      sum[i] += b[(size_t)k * nhl + i];
    }
}

// [nrow][ng] fluxes -> the sum over the g points of every row, g ascending
std::vector<double> sum_over_g_points(const std::vector<double>& f, size_t nrow, int ng) {
  std::vector<double> sum(nrow, 0.0);
  for (size_t r = 0; r < nrow; ++r)
    for (int g = 0; g < ng; ++g) sum[r] += f[r * ng + g];
  return sum;
}

// The command line, checked as far as it can be without a file of spectra or a device
struct Args {
  bool sw = false;
  std::vector<GasArg> gases;
  std::string config_file, scenario, output, ckd_file, ssi_file, scenarios_file, rayleigh_file, scenarios_rayleigh_file, history;
  bool merge_only = false, per_file_scaling = false, rayleigh_scattering = false;
  long col_a = -1, col_b = -1;
  std::vector<ScenarioRow> table;              // --scenarios
  Namelist nl;
};

Args parse_args(int argc, char** argv, bool sw) {
  Args p;
  p.sw = sw;
  GasArg pending;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto need = [&](int n) { if (i + n >= argc) fail(ECCKD_PARAMETER_ERROR, "%s needs %d argument(s)", a.c_str(), n); };
    auto scaling = [&](int mode) { need(1); pending.mode = (decltype(pending.mode))mode; pending.value = std::atof(argv[++i]); p.per_file_scaling = true; };
    if (a == "--config") { need(1); p.config_file = argv[++i]; }
    else if (a == "--scenario") { need(1); p.scenario = argv[++i]; }
    else if (a == "--output") { need(1); p.output = argv[++i]; }
    else if (a == "--ckd") { need(1); p.ckd_file = argv[++i]; }
    else if (a == "--ssi") { need(1); p.ssi_file = argv[++i]; }
    else if (a == "--merge-only") p.merge_only = true;
    else if (a == "--scenarios") { need(1); p.scenarios_file = argv[++i]; }
    else if (a == "--rayleigh") { need(1); p.rayleigh_file = argv[++i]; }
    else if (a == "--scenarios-rayleigh") { need(1); p.scenarios_rayleigh_file = argv[++i]; }
    else if (a == "--rayleigh-scattering") p.rayleigh_scattering = true;
    else if (a == "--column-range") { need(2); p.col_a = std::atol(argv[++i]); p.col_b = std::atol(argv[++i]); }
    else if (a == "--scale") scaling(GasArg::SCALE);
    else if (a == "--conc") scaling(GasArg::CONC);
    else if (a == "--const") scaling(GasArg::CONST);
    else if (a.rfind("--", 0) == 0) fail(ECCKD_PARAMETER_ERROR, "Argument \"%s\" not understood", a.c_str());
    else { pending.path = a; p.gases.push_back(pending); pending = GasArg(); }
  }
  if (!p.scenarios_rayleigh_file.empty()) {     // the scattering spectrum of a table: shortwave, and only beside --scenarios
    const char* with = !sw ? "the longwave tool" : !p.rayleigh_file.empty() ? "--rayleigh" : p.rayleigh_scattering ? "--rayleigh-scattering"
                       : !p.ckd_file.empty() ? "--ckd" : p.merge_only ? "--merge-only" : nullptr;
    if (with) fail(ECCKD_PARAMETER_ERROR, "\"--scenarios-rayleigh\" cannot be combined with %s", with);
    if (p.scenarios_file.empty())
      fail(ECCKD_PARAMETER_ERROR, "\"--scenarios-rayleigh\" needs --scenarios; for one scenario name the spectrum with --rayleigh");
  }
  if (!p.rayleigh_file.empty() || p.rayleigh_scattering) {     // scattering is opt-in, shortwave only, one column set per call
    const char* sw_switch = !p.rayleigh_file.empty() ? "--rayleigh" : "--rayleigh-scattering";
    const char* with = !sw ? "the longwave tool" : p.merge_only ? "--merge-only" : !p.scenarios_file.empty() ? "--scenarios" : nullptr;
    if (with) fail(ECCKD_PARAMETER_ERROR, "\"%s\" cannot be combined with %s", sw_switch, with);
    if (!p.rayleigh_file.empty() && !p.ckd_file.empty())
      fail(ECCKD_PARAMETER_ERROR, "\"--rayleigh\" names a spectrum file of the default mode; with --ckd use --rayleigh-scattering");
    if (p.rayleigh_scattering && p.ckd_file.empty())
      fail(ECCKD_PARAMETER_ERROR, "\"--rayleigh-scattering\" needs --ckd; in the default mode name the spectrum with --rayleigh");
  }
  if (!p.scenarios_file.empty()) {             // every check of the table before a device is opened
    const char* with = p.merge_only ? "--merge-only" : !p.ckd_file.empty() ? "--ckd" : !p.output.empty() ? "--output" : !p.scenario.empty() ? "--scenario"
                       : p.per_file_scaling ? "a per-file --scale, --conc or --const" : nullptr;
    if (with) fail(ECCKD_PARAMETER_ERROR, "\"--scenarios\" cannot be combined with %s (names, outputs and scalings come from the table)", with);
    if (p.gases.empty()) fail(ECCKD_PARAMETER_ERROR, "No spectrum files given");
    p.table = read_scenarios(p.scenarios_file, p.gases.size());
  } else if (p.output.empty()) fail(ECCKD_PARAMETER_ERROR, "\"--output\" file not specified");
  if (!p.config_file.empty()) p.nl = read_namelist(p.config_file);
  if (p.nl.nspectralstride != 1) fail(ECCKD_PARAMETER_ERROR, "nspectralstride = %d is not supported (1 only)", p.nl.nspectralstride);
  if (p.nl.nangle < 0 || p.nl.nangle > 16) fail(ECCKD_PARAMETER_ERROR, "nangle = %d outside 0..16", p.nl.nangle);
  if (sw && p.nl.nangle != 0) WARN("nangle = %d has no meaning for the direct solar beam: ignored", p.nl.nangle);
  p.history = history_line(argc, argv);
  return p;
}

// ---- --ckd: radiative transfer on a CKD model's optical depths (test/run_ckd_lw.sh:133-137, test/run_ckd_sw.sh:125-128) ----
// The output's header: per column (shortwave: and angle) and half level the fluxes, broadband and per g point
void define_ckd_output(NcOut& out, const Args& a, int ncol, int nmu, int nlay, int ng) {
  const bool sw = a.sw, scattering = a.rayleigh_scattering;
  const std::string x = sw ? "_sw" : "_lw", X = sw ? " shortwave flux" : " longwave flux";
  out.dim("column", ncol);
  if (sw) out.dim("mu0", nmu);
  out.dim("half_level", nlay + 1); out.dim("g_point", ng);
  std::vector<std::string> hl = {"column", "half_level"};
  if (sw) hl.insert(hl.begin() + 1, "mu0");
  std::vector<std::string> hl_g = hl;
  hl_g.push_back("g_point");
  auto flux = [&](const std::string& name, const std::vector<std::string>& dims, const std::string& long_name) {
    out.var(name + x, NC_FLOAT_T, dims, long_name.c_str(), "W m-2");
  };
  out.var("pressure_hl", NC_FLOAT_T, {"column", "half_level"}, "Pressure at half levels", "Pa");
  if (sw) out.var("mu0", NC_FLOAT_T, {"mu0"}, "Cosine of solar zenith angle", "1");
  flux("flux_up", hl, "Upwelling" + X);
  flux("flux_dn", hl, "Downwelling" + X);
  if (sw) flux("flux_dn_direct", hl, "Downwelling direct" + X);
  flux("spectral_flux_up", hl_g, "Upwelling" + X + " per g point");
  if (sw) flux("spectral_flux_dn_direct", hl_g, "Downwelling direct" + X + " per g point");
  if (!sw || scattering) flux("spectral_flux_dn", hl_g, "Downwelling" + X + " per g point");
  if (!a.scenario.empty()) out.att(a.scenario, "scenario");
  out.att(a.history, "history");
  if (scattering) out.att("two-stream", "rayleigh_scattering");
  out.end_define();
}

// Fluxes [row][half_level][g_point], a row per angle (longwave: one row).  Shortwave: flux 0 is the direct beam, which is the
// whole downwelling flux too unless the Rayleigh optical depth scatters; the last flux is the upwelling one.
int mode_ckd(const Args& a) {
  const bool sw = a.sw, scattering = a.rayleigh_scattering;
  const Namelist& nl = a.nl;
  Device dev;
  NcIn f(a.ckd_file);
  const std::vector<size_t> sh = f.shape("optical_depth");
  if (sh.size() != 3) fail(ECCKD_PARAMETER_ERROR, "optical_depth in %s is not (column, level, g_point)", a.ckd_file.c_str());
  const int ncol = (int)sh[0], nlay = (int)sh[1], ng = (int)sh[2];
  std::vector<double> mu0 = nl.mu0;
  bool have_ray = false;
  if (sw) {
    if (!f.exist("incoming_sw")) fail(ECCKD_PARAMETER_ERROR, "%s holds no incoming_sw: not a shortwave optical-depth file", a.ckd_file.c_str());
    if (mu0.empty()) mu0 = {0.5};
    have_ray = f.exist("rayleigh_optical_depth");
    if (scattering && !have_ray)
      fail(ECCKD_PARAMETER_ERROR, "\"--rayleigh-scattering\": %s holds no rayleigh_optical_depth", a.ckd_file.c_str());
  } else if (!f.exist("planck_hl")) {
    fail(ECCKD_PARAMETER_ERROR, "%s holds no planck_hl: not a longwave optical-depth file", a.ckd_file.c_str());
  }
  const int nrow = sw ? (int)mu0.size() : 1, nflux = scattering ? 3 : 2, dn = scattering ? 1 : 0, up = nflux - 1;
  NcOut out(a.output);
  define_ckd_output(out, a, ncol, nrow, nlay, ng);
  if (sw) out.write("mu0", mu0);
  const size_t nhg = (size_t)(nlay + 1) * ng;
  const std::string x = sw ? "_sw" : "_lw";
  for (int c = 0; c < ncol; ++c) {
    std::vector<double> od = f.read("optical_depth", c), ray, flux[3];
    for (int k = 0; k < nflux; ++k) flux[k].resize(nrow * nhg);
    if (have_ray) ray = f.read("rayleigh_optical_depth", c);
    if (have_ray && !scattering)                // one more absorber, as in the reference's forward model (solve_adept.cpp:34)
      for (size_t i = 0; i < od.size(); ++i) od[i] += ray[i];
    const std::vector<double> source = f.read(sw ? "incoming_sw" : "planck_hl", c);
    for (int m = 0; m < nrow; ++m) {            // per g point, on the device
      if (scattering)                           // two-stream
        ck(ecckd_rt_sw_gpoints_rayleigh(dev.ctx(), 1, nlay, ng, mu0[m], nl.surf_albedo, source.data(), od.data(), ray.data(), &flux[0][m * nhg],
                                        &flux[1][m * nhg], &flux[2][m * nhg]));
      else if (sw)                              // radiative_transfer_sw.cpp:45-77
        ck(ecckd_rt_sw_gpoints(dev.ctx(), 1, nlay, ng, mu0[m], nl.surf_albedo, source.data(), od.data(), &flux[0][m * nhg], &flux[1][m * nhg]));
      else                                      // radiative_transfer_lw.cpp:27-60 (two-stream or nangle Gauss-Legendre angles)
        ck(ecckd_rt_lw_gpoints(dev.ctx(), nl.nangle, 1, nlay, ng, source.data(), od.data(), flux[0].data(), flux[1].data()));
    }
    const size_t nsum = (size_t)nrow * (nlay + 1);
    out.write_slice("pressure_hl", c, f.read("pressure_hl", c));
    if (sw) out.write_slice("flux_dn_direct_sw", c, sum_over_g_points(flux[0], nsum, ng));
    out.write_slice("flux_dn" + x, c, sum_over_g_points(flux[dn], nsum, ng));
    out.write_slice("flux_up" + x, c, sum_over_g_points(flux[up], nsum, ng));
    if (sw) out.write_slice("spectral_flux_dn_direct_sw", c, flux[0]);
    if (!sw || scattering) out.write_slice("spectral_flux_dn" + x, c, flux[dn]);
    out.write_slice("spectral_flux_up" + x, c, flux[up]);
  }
  out.close();
  return done(0);
}

// ---- the modes that read files of spectra ----
// Grids and profiles from the first file (every other file must share them) and the columns asked for: no device needed
struct Grid {
  Spectrum first;
  int nlay = 0, c0 = 0, c1 = 0, ncol = 0;
  size_t nwav = 0;
};

Grid read_grid(const Args& a) {
  Grid g;
  g.first = read_spectrum(a.gases[0].path, 0, false);
  g.nlay = g.first.nlay; g.nwav = g.first.nwav;
  g.c1 = g.first.ncol - 1;
  if (a.col_a >= 1) { g.c0 = (int)a.col_a - 1; g.c1 = std::min<long>(a.col_b, g.first.ncol) - 1; }   // 1-based, inclusive, like the Fortran tool
  g.ncol = g.c1 - g.c0 + 1;
  if (g.ncol <= 0) fail(ECCKD_PARAMETER_ERROR, "Empty column range");
  LOG("%d gas file(s), %d column(s), %d layers, %zu spectral points\n", (int)a.gases.size(), g.ncol, g.nlay, g.nwav);
  return g;
}

// ... and what they keep on the device or take from the namelist
struct Spectra {
  const Grid g;
  Device dev;
  DevBuf d_wn, d_dwn, d_ssi, d_albedo;
  std::vector<double> mu0;
  int nmu = 0, nband = 0;
  std::string ids;
  std::vector<int64_t> bbegin, bend;           // bands of the namelist -> wavenumber index ranges

  explicit Spectra(const Args& a) : g(read_grid(a)) {
    const Namelist& nl = a.nl;
    d_wn.upload(dev, g.first.wavenumber_cm_1);
    d_dwn.upload(dev, g.first.d_wavenumber_cm_1);
    mu0 = nl.mu0;
    if (a.sw && !a.merge_only) {
      if (a.ssi_file.empty()) fail(ECCKD_PARAMETER_ERROR, "\"--ssi\" file not specified");
      NcIn fs(a.ssi_file);
      const std::vector<double> ssi = fs.read("solar_spectral_irradiance");
      if (ssi.size() != g.nwav) fail(ECCKD_PARAMETER_ERROR, "solar_spectral_irradiance has %zu points, the spectra %zu", ssi.size(), g.nwav);
      d_ssi.upload(dev, ssi);
      d_albedo.upload(dev, std::vector<double>(g.nwav, nl.surf_albedo));
      if (mu0.empty()) fail(ECCKD_PARAMETER_ERROR, "cos_solar_zenith_angle missing from the namelist");
    }
    nmu = (int)mu0.size();
    for (const GasArg& gas : a.gases) {
      NcIn f(gas.path);
      std::string m;
      if (!f.att_text("constituent_id", m)) f.att_text("molecules", m);
      ids += (ids.empty() ? "" : " ") + m.substr(0, m.find(' '));
    }
    if (!a.merge_only) {
      if (nl.band1.empty() || nl.band1.size() != nl.band2.size())
        fail(ECCKD_PARAMETER_ERROR, "band_wavenumber1 / band_wavenumber2 missing from the namelist");
      nband = (int)nl.band1.size();
      bbegin.resize(nband); bend.resize(nband);
      ck(ecckd_band_ranges(g.nwav, g.first.wavenumber_cm_1.data(), nband, nl.band1.data(), nl.band2.data(), nullptr, bbegin.data(), bend.data()));
    }
  }
};

// A flux file as far as the column dimension, the profiles and define_flux_variables go, and its coordinate variables
void define_flux_file(NcOut& o, const Args& a, const Spectra& s, const std::string& scenario, bool rayleigh) {
  o.dim("column", s.g.ncol); o.dim("half_level", s.g.nlay + 1); o.dim("level", s.g.nlay);
  o.var("pressure_hl", NC_FLOAT_T, {"column", "half_level"}, "Pressure at half levels", "Pa");
  o.var("temperature_hl", NC_FLOAT_T, {"column", "half_level"}, "Temperature at half levels", "K");
  if (a.merge_only) {
    o.dim("wavenumber", s.g.nwav);
    o.var("wavenumber", NC_DOUBLE_T, {"wavenumber"}, "Wavenumber", "cm-1");
    o.var("optical_depth", NC_FLOAT_T, {"column", "level", "wavenumber"}, "Layer optical depth");
    o.att(s.ids, "molecules");
    o.att("composite", "constituent_id");
  } else {
    define_flux_variables(o, a.sw, a.gases.size(), s.nmu, s.nband, s.g.nwav, s.ids, a.nl.boundary_fluxes, rayleigh);
  }
  if (!scenario.empty()) o.att(scenario, "scenario");
  o.att(a.history, "history");
  o.end_define();
  if (!a.merge_only) {
    const std::string x = a.sw ? "_sw" : "_lw";
    o.write("band_wavenumber1" + x, a.nl.band1); o.write("band_wavenumber2" + x, a.nl.band2);
    if (a.sw) o.write("mu0", s.mu0);
  }
  if (a.merge_only || a.nl.boundary_fluxes) o.write("wavenumber", s.g.first.wavenumber_cm_1);
}

// ---- --scenarios: every scenario of the table from one read of the gas files per column ----
int mode_scenarios(const Args& a, Spectra& s) {
  const Namelist& nl = a.nl;
  const bool sw = a.sw, rayleigh = !a.scenarios_rayleigh_file.empty();
  const Device& dev = s.dev;
  const int nlay = s.g.nlay, nband = s.nband, nmu = s.nmu;
  const size_t nwav = s.g.nwav, nscen = a.table.size(), ngas = a.gases.size(), nhl = (size_t)nlay + 1;
  std::vector<std::unique_ptr<NcOut>> outs;
  for (const ScenarioRow& row : a.table) {
    outs.emplace_back(new NcOut(row.output));
    define_flux_file(*outs.back(), a, s, row.name, rayleigh);
  }
  const size_t nslot = sw ? nscen * nmu : nscen;            // rows of fluxes: (scenario[, angle])
  const int ngroup = sw ? std::min(8, nmu) : 1;              // angles per call: the entry takes up to 8
  DevBuf d_sdn, d_tup, d_tot;                                // d_tot: direct plus diffuse at the surface (--scenarios-rayleigh)
  if (nl.boundary_fluxes) { d_sdn.alloc(dev, nscen * ngroup * nwav * sizeof(double)); d_tup.alloc(dev, nscen * ngroup * nwav * sizeof(double)); }
  if (nl.boundary_fluxes && rayleigh) d_tot.alloc(dev, nscen * ngroup * nwav * sizeof(double));
  double* const p_sdn = nl.boundary_fluxes ? d_sdn.as<double>() : nullptr;
  double* const p_tup = nl.boundary_fluxes ? d_tup.as<double>() : nullptr;
  double* const p_tot = nl.boundary_fluxes && rayleigh ? d_tot.as<double>() : nullptr;
  for (int c = s.g.c0; c <= s.g.c1; ++c) {
    const Spectrum col = c == 0 ? s.g.first : read_spectrum(a.gases[0].path, c, false);
    std::vector<DevOd> ods;                                  // the gases side by side on the device, read once
    std::vector<const void*> od_ptr;
    std::vector<int> od_type;
    std::vector<size_t> od_stride(ngas, nwav);
    std::vector<double> scale(nscen * ngas * nlay), vmr_all(nscen * ngas * nlay);   // [scenario][gas][level]
    for (size_t ig = 0; ig < ngas; ++ig) {
      NcIn f(a.gases[ig].path);
      double ref = -1.0;
      std::vector<double> vmr, profile, vmr_out;
      std::string mol;
      read_od_meta(f, c, nlay, ref, vmr, mol);
      for (size_t k = 0; k < nscen; ++k) {
        gas_scaling(a.table[k].specs[ig], a.gases[ig].path, nlay, col.pressure_hl, ref, vmr, profile, vmr_out);
        std::copy(profile.begin(), profile.end(), scale.begin() + (k * ngas + ig) * nlay);
        std::copy(vmr_out.begin(), vmr_out.end(), vmr_all.begin() + (k * ngas + ig) * nlay);
      }
      ods.push_back(read_od_dev(dev, f, c, nlay, nwav));
      od_ptr.push_back(ods.back().buf.ptr());
      od_type.push_back(ods.back().type);
    }
    DevOd ray;                                               // --scenarios-rayleigh: what scatters, read once, never scaled
    if (rayleigh) {
      NcIn fr(a.scenarios_rayleigh_file);
      ray = read_od_dev(dev, fr, c, nlay, nwav);
    }
    ck(ecckd_synchronize(dev.ctx()));
    std::vector<double> bdn(nslot * nband * nhl), bup(nslot * nband * nhl), btot;   // bdn: the direct beam where light scatters
    std::vector<double> all_dn, all_up, all_tot;             // [slot][wavenumber] boundary fluxes of this column
    if (rayleigh) btot.resize(nslot * nband * nhl);
    if (nl.boundary_fluxes) { all_dn.resize(nslot * nwav); all_up.resize(nslot * nwav); }
    if (nl.boundary_fluxes && rayleigh) all_tot.resize(nslot * nwav);
    if (sw) {
      for (int m0 = 0; m0 < nmu; m0 += ngroup) {             // [scenario][angle] rows per group of angles
        const size_t nm = (size_t)std::min(ngroup, nmu - m0);
        std::vector<double> gdn(nscen * nm * nband * nhl), gup(gdn.size()), gtot(rayleigh ? gdn.size() : 0);
        if (rayleigh)
          ck(ecckd_lbl_band_fluxes_sw_rayleigh_scenarios(dev.ctx(), nlay, nwav, (int)nm, s.mu0.data() + m0, s.d_ssi.as<double>(),
                                                         s.d_albedo.as<double>(), (int)ngas, od_ptr.data(), od_type.data(), od_stride.data(),
                                                         ray.buf.ptr(), ray.type, nwav, (int)nscen, scale.data(), nband, s.bbegin.data(),
                                                         s.bend.data(), gdn.data(), gtot.data(), gup.data(), p_sdn, p_tot, p_tup));
        else
          ck(ecckd_lbl_band_fluxes_sw_scenarios(dev.ctx(), nlay, nwav, (int)nm, s.mu0.data() + m0, s.d_ssi.as<double>(), s.d_albedo.as<double>(),
                                                (int)ngas, od_ptr.data(), od_type.data(), od_stride.data(), (int)nscen, scale.data(), nband,
                                                s.bbegin.data(), s.bend.data(), gdn.data(), gup.data(), p_sdn, p_tup));
        std::vector<double> sd, tu, tt;
        if (nl.boundary_fluxes) { sd = d_sdn.download<double>(); tu = d_tup.download<double>(); }
        if (nl.boundary_fluxes && rayleigh) tt = d_tot.download<double>();
        for (size_t k = 0; k < nscen; ++k) {
          const size_t n = nm * nband * nhl, to = (k * nmu + m0) * nband * nhl;
          std::copy(gdn.begin() + k * n, gdn.begin() + (k + 1) * n, bdn.begin() + to);
          std::copy(gup.begin() + k * n, gup.begin() + (k + 1) * n, bup.begin() + to);
          if (rayleigh) std::copy(gtot.begin() + k * n, gtot.begin() + (k + 1) * n, btot.begin() + to);
          if (nl.boundary_fluxes) {
            std::copy(sd.begin() + k * nm * nwav, sd.begin() + (k + 1) * nm * nwav, all_dn.begin() + (k * nmu + m0) * nwav);
            std::copy(tu.begin() + k * nm * nwav, tu.begin() + (k + 1) * nm * nwav, all_up.begin() + (k * nmu + m0) * nwav);
            if (rayleigh) std::copy(tt.begin() + k * nm * nwav, tt.begin() + (k + 1) * nm * nwav, all_tot.begin() + (k * nmu + m0) * nwav);
          }
        }
      }
    } else {
      if (col.temperature_hl.empty()) fail(ECCKD_PARAMETER_ERROR, "temperature_hl missing from %s", a.gases[0].path.c_str());
      ck(ecckd_lbl_band_fluxes_lw_scenarios(dev.ctx(), nl.nangle, nlay, nwav, col.temperature_hl.data(), s.d_wn.as<double>(), s.d_dwn.as<double>(),
                                            (int)ngas, od_ptr.data(), od_type.data(), od_stride.data(), (int)nscen, scale.data(), nband,
                                            s.bbegin.data(), s.bend.data(), bdn.data(), bup.data(), p_sdn, p_tup));
      if (nl.boundary_fluxes) { all_dn = d_sdn.download<double>(); all_up = d_tup.download<double>(); }
    }
    const size_t oc = (size_t)(c - s.g.c0), per = sw ? (size_t)nmu : 1;   // rows per scenario
    std::vector<double> tdn(per * nhl * nband), tup(per * nhl * nband), sdn(per * nhl), sup(per * nhl), ttot, stot;
    if (rayleigh) { ttot.resize(per * nhl * nband); stot.resize(per * nhl); }
    const std::string x = sw ? "_sw" : "_lw";
    for (size_t k = 0; k < nscen; ++k) {
      NcOut& o = *outs[k];
      o.write_slice("pressure_hl", oc, col.pressure_hl);
      if (!col.temperature_hl.empty()) o.write_slice("temperature_hl", oc, col.temperature_hl);
      for (size_t m = 0; m < per; ++m) {
        bands_to_file_order(nband, nhl, &bdn[(k * per + m) * nband * nhl], &tdn[m * nhl * nband], &sdn[m * nhl]);
        bands_to_file_order(nband, nhl, &bup[(k * per + m) * nband * nhl], &tup[m * nhl * nband], &sup[m * nhl]);
        if (rayleigh) bands_to_file_order(nband, nhl, &btot[(k * per + m) * nband * nhl], &ttot[m * nhl * nband], &stot[m * nhl]);
      }
      o.write_slice("mole_fraction_fl", oc, std::vector<double>(vmr_all.begin() + k * ngas * nlay, vmr_all.begin() + (k + 1) * ngas * nlay));
      o.write_slice(sw ? "band_flux_dn_direct_sw" : "band_flux_dn_lw", oc, tdn);
      if (rayleigh) o.write_slice("band_flux_dn_sw", oc, ttot);
      o.write_slice("band_flux_up" + x, oc, tup);
      if (sw) o.write_slice("flux_dn_direct_sw", oc, sdn);
      o.write_slice("flux_dn" + x, oc, rayleigh ? stot : sdn); o.write_slice("flux_up" + x, oc, sup);
      if (nl.boundary_fluxes) {
        const std::vector<double> sd(all_dn.begin() + k * per * nwav, all_dn.begin() + (k + 1) * per * nwav);
        const std::vector<double> tu(all_up.begin() + k * per * nwav, all_up.begin() + (k + 1) * per * nwav);
        o.write_slice(sw ? "spectral_flux_dn_direct_surf_sw" : "spectral_flux_dn_surf_lw", oc, sd);
        if (rayleigh)
          o.write_slice("spectral_flux_dn_surf_sw", oc, std::vector<double>(all_tot.begin() + k * per * nwav, all_tot.begin() + (k + 1) * per * nwav));
        o.write_slice("spectral_flux_up_toa" + x, oc, tu);
      }
    }
    LOG("  column %d done (%zu scenarios)\n", c + 1, nscen);
  }
  for (auto& o : outs) o->close();
  return done(0);
}

// ---- default, and --merge-only: the gases of every column merged with their scalings, then written or carried through the
// radiative transfer.  Fluxes [row][band][half_level], a row per angle (longwave: one row): flux 0 is the downwelling one
// (shortwave: the direct beam, the whole downwelling flux too unless --rayleigh scatters), the last the upwelling one. ----
int mode_default(const Args& a, Spectra& s) {
  const Namelist& nl = a.nl;
  const bool sw = a.sw, rayleigh = !a.rayleigh_file.empty(), bnd = nl.boundary_fluxes && !a.merge_only;
  const Device& dev = s.dev;
  const int nlay = s.g.nlay, nband = s.nband, nrow = sw ? s.nmu : 1;
  const size_t nwav = s.g.nwav, nhl = (size_t)nlay + 1;
  DevBuf d_merged(dev, (size_t)nlay * nwav * sizeof(double));
  NcOut out(a.output);
  define_flux_file(out, a, s, a.scenario, rayleigh);
  const int nflux = rayleigh ? 3 : 2, dn = rayleigh ? 1 : 0, up = nflux - 1;
  const int ngroup = rayleigh ? std::min(8, std::max(nrow, 1)) : 1;   // angles per call: the Rayleigh entry takes up to 8
  DevBuf d_bnd[3];                                                    // the boundary fluxes of a call, [angle][wavenumber]
  double* p_bnd[3] = {nullptr, nullptr, nullptr};
  if (bnd)
    for (int k = 0; k < nflux; ++k) { d_bnd[k].alloc(dev, (size_t)ngroup * nwav * sizeof(double)); p_bnd[k] = d_bnd[k].as<double>(); }
  const std::string x = sw ? "_sw" : "_lw";

  for (int c = s.g.c0; c <= s.g.c1; ++c) {
    const Spectrum col = c == 0 ? s.g.first : read_spectrum(a.gases[0].path, c, false);
    std::vector<double> vmr_all;   // [gas][level]
    for (size_t ig = 0; ig < a.gases.size(); ++ig) {
      const GasArg& gas = a.gases[ig];
      NcIn f(gas.path);
      double ref = -1.0;
      std::vector<double> vmr, profile, vmr_out;
      std::string mol;
      read_od_meta(f, c, nlay, ref, vmr, mol);
      gas_scaling(gas, gas.path, nlay, col.pressure_hl, ref, vmr, profile, vmr_out);
      vmr_all.insert(vmr_all.end(), vmr_out.begin(), vmr_out.end());
      DevOd od = read_od_dev(dev, f, c, nlay, nwav);
      ck(ecckd_merge_spectrum_dev(dev.ctx(), nlay, nwav, od.buf.ptr(), od.type, nwav, profile.data(), ig == 0 ? 1 : 0,
                                  d_merged.as<double>(), nwav));
      ck(ecckd_synchronize(dev.ctx()));
    }
    const size_t oc = (size_t)(c - s.g.c0);
    out.write_slice("pressure_hl", oc, col.pressure_hl);
    if (!col.temperature_hl.empty()) out.write_slice("temperature_hl", oc, col.temperature_hl);
    if (a.merge_only) {
      out.write_slice("optical_depth", oc, d_merged.download<double>());
      LOG("  column %d done\n", c + 1);
      continue;
    }
    DevOd ray;                                   // --rayleigh: the spectrum that scatters, beside the merged absorbers
    if (rayleigh) {
      NcIn fr(a.rayleigh_file);
      ray = read_od_dev(dev, fr, c, nlay, nwav);
      ck(ecckd_synchronize(dev.ctx()));
    } else if (!sw && col.temperature_hl.empty()) {
      fail(ECCKD_PARAMETER_ERROR, "temperature_hl missing from %s", a.gases[0].path.c_str());
    }
    std::vector<double> t[3], sum[3], all[3], g[3];   // (row, half_level, band), (row, half_level), (row, wavenumber), one call's
    for (int k = 0; k < nflux; ++k) { t[k].resize((size_t)nrow * nhl * nband); sum[k].resize((size_t)nrow * nhl); }
    for (int m0 = 0; m0 < nrow; m0 += ngroup) {
      const int nm = std::min(ngroup, nrow - m0);
      for (int k = 0; k < nflux; ++k) g[k].assign((size_t)nm * nband * nhl, 0.0);
      if (rayleigh)
        ck(ecckd_lbl_band_fluxes_sw_rayleigh(dev.ctx(), nlay, nwav, nm, s.mu0.data() + m0, s.d_ssi.as<double>(), s.d_albedo.as<double>(), d_merged.ptr(),
                                             ECCKD_F64, nwav, ray.buf.ptr(), ray.type, nwav, nband, s.bbegin.data(), s.bend.data(), g[0].data(),
                                             g[1].data(), g[2].data(), p_bnd[0], p_bnd[1], p_bnd[2]));
      else if (sw)
        ck(ecckd_lbl_band_fluxes_sw_ex(dev.ctx(), nlay, nwav, s.mu0[m0], s.d_ssi.as<double>(), s.d_albedo.as<double>(), d_merged.ptr(), ECCKD_F64, nwav,
                                       nband, s.bbegin.data(), s.bend.data(), g[0].data(), g[1].data(), p_bnd[0], p_bnd[1]));
      else
        ck(ecckd_lbl_band_fluxes_lw_angles(dev.ctx(), nl.nangle, nlay, nwav, col.temperature_hl.data(), s.d_wn.as<double>(), s.d_dwn.as<double>(),
                                           d_merged.ptr(), ECCKD_F64, nwav, nband, s.bbegin.data(), s.bend.data(), g[0].data(), g[1].data(),
                                           p_bnd[0], p_bnd[1]));
      for (int k = 0; k < nflux; ++k) {
        if (bnd) {
          const std::vector<double> b = d_bnd[k].download<double>();
          all[k].insert(all[k].end(), b.begin(), b.begin() + (size_t)nm * nwav);
        }
        for (int m = 0; m < nm; ++m)
          bands_to_file_order(nband, nhl, &g[k][(size_t)m * nband * nhl], &t[k][(size_t)(m0 + m) * nhl * nband], &sum[k][(size_t)(m0 + m) * nhl]);
      }
    }
    out.write_slice("mole_fraction_fl", oc, vmr_all);
    out.write_slice(sw ? "band_flux_dn_direct_sw" : "band_flux_dn_lw", oc, t[0]);
    if (rayleigh) out.write_slice("band_flux_dn_sw", oc, t[1]);
    out.write_slice("band_flux_up" + x, oc, t[up]);
    if (sw) out.write_slice("flux_dn_direct_sw", oc, sum[0]);
    out.write_slice("flux_dn" + x, oc, sum[dn]); out.write_slice("flux_up" + x, oc, sum[up]);
    if (bnd) {
      out.write_slice(sw ? "spectral_flux_dn_direct_surf_sw" : "spectral_flux_dn_surf_lw", oc, all[0]);
      if (rayleigh) out.write_slice("spectral_flux_dn_surf_sw", oc, all[1]);
      out.write_slice("spectral_flux_up_toa" + x, oc, all[up]);
    }
    LOG("  column %d done\n", c + 1);
  }
  out.close();
  return done(0);
}

}  // namespace

inline int ckdmip_main(int argc, char** argv, bool sw) {
  try {
    const Args a = parse_args(argc, argv, sw);
    if (!a.ckd_file.empty()) return mode_ckd(a);
    if (a.gases.empty()) fail(ECCKD_PARAMETER_ERROR, "No spectrum files given");
    Spectra s(a);
    return a.table.empty() ? mode_default(a, s) : mode_scenarios(a, s);
  } catch (const Fatal& f) {
    std::fprintf(stderr, "*** Error: %s\n", f.msg.c_str());
    return f.code ? f.code : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "*** Error: %s\n", e.what());
    return ECCKD_UNEXPECTED_EXCEPTION;
  }
}
