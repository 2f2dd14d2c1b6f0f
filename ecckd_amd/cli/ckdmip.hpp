// ckdmip.hpp - bin/ckdmip_lw and bin/ckdmip_sw: stand-ins for the EXTERNAL CKDMIP tools that the reference's scripts call (they are
// not part of ecCKD; test/config.h:32-35), restricted to what those scripts use and, unless ckdmip_sw is asked to scatter
// (--rayleigh, --rayleigh-scattering), to the no-scattering radiative transfer the reference itself contains.
//
// ckdmip_{lw,sw} [--config file.nam] [--scenario name] [--merge-only] [--column-range a b] [--ssi file]
//                {[--scale s | --conc c | --const c] spectrum-file}... [--ckd optical-depth-file] --output file
// ckdmip_sw      ... [--rayleigh rayleigh-spectrum-file] spectrum-file... --output file
// ckdmip_sw      ... --ckd optical-depth-file --rayleigh-scattering --output file
// ckdmip_{lw,sw} [--config file.nam] [--column-range a b] [--ssi file] --scenarios table spectrum-file...
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

#include "tool.hpp"

using namespace tool;

namespace {

struct GasArg {
  std::string path;
  enum { NONE, SCALE, CONC, CONST } mode = NONE;
  double value = 1.0;
};

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

// One line of a --scenarios table: the scenario's name, its output file and one GasArg (path empty) per spectrum file
struct ScenarioRow {
  std::string name, output;
  std::vector<GasArg> specs;
};

std::vector<ScenarioRow> read_scenarios(const std::string& path, size_t ngas) {
  std::ifstream in(path);
  if (!in) fail(ECCKD_PARAMETER_ERROR, "Cannot open scenario table %s", path.c_str());
  std::vector<ScenarioRow> rows;
  std::string line;
  int lineno = 0;
  while (std::getline(in, line)) {
    ++lineno;
    const size_t c = line.find('#');
    if (c != std::string::npos) line.erase(c);
    std::istringstream ss(line);
    std::vector<std::string> tok;
    for (std::string t; ss >> t;) tok.push_back(t);
    if (tok.empty()) continue;
    if (tok.size() != 2 + ngas)
      fail(ECCKD_PARAMETER_ERROR, "%s:%d: %zu scaling spec(s) for %zu spectrum file(s) (NAME OUTPUT and one spec per file)", path.c_str(),
           lineno, tok.size() >= 2 ? tok.size() - 2 : (size_t)0, ngas);
    ScenarioRow row;
    row.name = tok[0]; row.output = tok[1];
    for (size_t g = 0; g < ngas; ++g) {
      const std::string& t = tok[2 + g];
      GasArg a;
      const size_t eq = t.find('=');
      const std::string key = t.substr(0, eq);
      if (t == "asis") a.mode = GasArg::NONE;
      else if (eq != std::string::npos && key == "scale") a.mode = GasArg::SCALE;
      else if (eq != std::string::npos && key == "conc") a.mode = GasArg::CONC;
      else if (eq != std::string::npos && key == "const") a.mode = GasArg::CONST;
      else fail(ECCKD_PARAMETER_ERROR, "%s:%d: unknown scaling spec \"%s\" (asis, scale=S, conc=C or const=C)", path.c_str(), lineno, t.c_str());
      if (a.mode != GasArg::NONE) {
        const std::string v = t.substr(eq + 1);
        char* end = nullptr;
        a.value = std::strtod(v.c_str(), &end);
        if (v.empty() || *end) fail(ECCKD_PARAMETER_ERROR, "%s:%d: unknown scaling spec \"%s\" (no number after '=')", path.c_str(), lineno, t.c_str());
      }
      row.specs.push_back(a);
    }
    for (const ScenarioRow& r : rows)
      if (r.output == row.output) fail(ECCKD_PARAMETER_ERROR, "%s:%d: duplicate output file \"%s\"", path.c_str(), lineno, row.output.c_str());
    rows.push_back(row);
  }
  if (rows.empty()) fail(ECCKD_PARAMETER_ERROR, "Scenario table %s is empty", path.c_str());
  return rows;
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

}  // namespace

inline int ckdmip_main(int argc, char** argv, bool sw) {
  try {
    std::vector<GasArg> gases;
    std::string config_file, scenario, output, ckd_file, ssi_file, scenarios_file, rayleigh_file;
    bool merge_only = false, per_file_scaling = false, rayleigh_scattering = false;
    long col_a = -1, col_b = -1;
    GasArg pending;
    for (int i = 1; i < argc; ++i) {
      const std::string a = argv[i];
      auto need = [&](int n) { if (i + n >= argc) fail(ECCKD_PARAMETER_ERROR, "%s needs %d argument(s)", a.c_str(), n); };
      if (a == "--config") { need(1); config_file = argv[++i]; }
      else if (a == "--scenario") { need(1); scenario = argv[++i]; }
      else if (a == "--output") { need(1); output = argv[++i]; }
      else if (a == "--ckd") { need(1); ckd_file = argv[++i]; }
      else if (a == "--ssi") { need(1); ssi_file = argv[++i]; }
      else if (a == "--merge-only") merge_only = true;
      else if (a == "--scenarios") { need(1); scenarios_file = argv[++i]; }
      else if (a == "--rayleigh") { need(1); rayleigh_file = argv[++i]; }
      else if (a == "--rayleigh-scattering") rayleigh_scattering = true;
      else if (a == "--column-range") { need(2); col_a = std::atol(argv[++i]); col_b = std::atol(argv[++i]); }
      else if (a == "--scale") { need(1); pending.mode = GasArg::SCALE; pending.value = std::atof(argv[++i]); per_file_scaling = true; }
      else if (a == "--conc") { need(1); pending.mode = GasArg::CONC; pending.value = std::atof(argv[++i]); per_file_scaling = true; }
      else if (a == "--const") { need(1); pending.mode = GasArg::CONST; pending.value = std::atof(argv[++i]); per_file_scaling = true; }
      else if (a.rfind("--", 0) == 0) fail(ECCKD_PARAMETER_ERROR, "Argument \"%s\" not understood", a.c_str());
      else { pending.path = a; gases.push_back(pending); pending = GasArg(); }
    }
    if (!rayleigh_file.empty() || rayleigh_scattering) {     // scattering is opt-in, shortwave only, one column set per call
      const char* sw_switch = !rayleigh_file.empty() ? "--rayleigh" : "--rayleigh-scattering";
      const char* with = !sw ? "the longwave tool" : merge_only ? "--merge-only" : !scenarios_file.empty() ? "--scenarios" : nullptr;
      if (with) fail(ECCKD_PARAMETER_ERROR, "\"%s\" cannot be combined with %s", sw_switch, with);
      if (!rayleigh_file.empty() && !ckd_file.empty())
        fail(ECCKD_PARAMETER_ERROR, "\"--rayleigh\" names a spectrum file of the default mode; with --ckd use --rayleigh-scattering");
      if (rayleigh_scattering && ckd_file.empty())
        fail(ECCKD_PARAMETER_ERROR, "\"--rayleigh-scattering\" needs --ckd; in the default mode name the spectrum with --rayleigh");
    }
    std::vector<ScenarioRow> table;              // --scenarios: every check of the table before a device is opened
    if (!scenarios_file.empty()) {
      const char* with = merge_only ? "--merge-only" : !ckd_file.empty() ? "--ckd" : !output.empty() ? "--output" : !scenario.empty() ? "--scenario"
                         : per_file_scaling ? "a per-file --scale, --conc or --const" : nullptr;
      if (with) fail(ECCKD_PARAMETER_ERROR, "\"--scenarios\" cannot be combined with %s (names, outputs and scalings come from the table)", with);
      if (gases.empty()) fail(ECCKD_PARAMETER_ERROR, "No spectrum files given");
      table = read_scenarios(scenarios_file, gases.size());
    } else if (output.empty()) fail(ECCKD_PARAMETER_ERROR, "\"--output\" file not specified");
    Namelist nl;
    if (!config_file.empty()) nl = read_namelist(config_file);
    if (nl.nspectralstride != 1) fail(ECCKD_PARAMETER_ERROR, "nspectralstride = %d is not supported (1 only)", nl.nspectralstride);
    if (nl.nangle < 0 || nl.nangle > 16) fail(ECCKD_PARAMETER_ERROR, "nangle = %d outside 0..16", nl.nangle);
    if (sw && nl.nangle != 0) WARN("nangle = %d has no meaning for the direct solar beam: ignored", nl.nangle);
    const std::string history = history_line(argc, argv);

    // ---------------------------------------------------------------------------------------------------------------
    if (!ckd_file.empty()) {   // radiative transfer on a CKD model's optical depths (test/run_ckd_lw.sh:133-137)
      Device dev;
      NcIn f(ckd_file);
      const std::vector<size_t> sh = f.shape("optical_depth");
      if (sh.size() != 3) fail(ECCKD_PARAMETER_ERROR, "optical_depth in %s is not (column, level, g_point)", ckd_file.c_str());
      const int ncol = (int)sh[0], nlay = (int)sh[1], ng = (int)sh[2];
      if (sw) {
        if (!f.exist("incoming_sw")) fail(ECCKD_PARAMETER_ERROR, "%s holds no incoming_sw: not a shortwave optical-depth file", ckd_file.c_str());
        std::vector<double> mu0 = nl.mu0;
        if (mu0.empty()) mu0 = {0.5};
        const int nmu = (int)mu0.size();
        const bool have_ray = f.exist("rayleigh_optical_depth");
        if (rayleigh_scattering && !have_ray)
          fail(ECCKD_PARAMETER_ERROR, "\"--rayleigh-scattering\": %s holds no rayleigh_optical_depth", ckd_file.c_str());
        NcOut out(output);
        out.dim("column", ncol); out.dim("mu0", nmu); out.dim("half_level", nlay + 1); out.dim("g_point", ng);
        out.var("pressure_hl", NC_FLOAT_T, {"column", "half_level"}, "Pressure at half levels", "Pa");
        out.var("mu0", NC_FLOAT_T, {"mu0"}, "Cosine of solar zenith angle", "1");
        out.var("flux_up_sw", NC_FLOAT_T, {"column", "mu0", "half_level"}, "Upwelling shortwave flux", "W m-2");
        out.var("flux_dn_sw", NC_FLOAT_T, {"column", "mu0", "half_level"}, "Downwelling shortwave flux", "W m-2");
        out.var("flux_dn_direct_sw", NC_FLOAT_T, {"column", "mu0", "half_level"}, "Downwelling direct shortwave flux", "W m-2");
        out.var("spectral_flux_up_sw", NC_FLOAT_T, {"column", "mu0", "half_level", "g_point"}, "Upwelling shortwave flux per g point", "W m-2");
        out.var("spectral_flux_dn_direct_sw", NC_FLOAT_T, {"column", "mu0", "half_level", "g_point"}, "Downwelling direct shortwave flux per g point", "W m-2");
        if (rayleigh_scattering)
          out.var("spectral_flux_dn_sw", NC_FLOAT_T, {"column", "mu0", "half_level", "g_point"}, "Downwelling shortwave flux per g point", "W m-2");
        if (!scenario.empty()) out.att(scenario, "scenario");
        out.att(history, "history");
        if (rayleigh_scattering) out.att("two-stream", "rayleigh_scattering");
        out.end_define();
        out.write("mu0", mu0);
        const size_t nhg = (size_t)(nlay + 1) * ng;
        if (rayleigh_scattering) for (int c = 0; c < ncol; ++c) {  // two-stream per g point, on the device (ecckd_rt_sw_gpoints_rayleigh)
          const std::vector<double> od = f.read("optical_depth", c), ray = f.read("rayleigh_optical_depth", c), incoming = f.read("incoming_sw", c);
          std::vector<double> dir_all(nmu * nhg), dn_all(nmu * nhg), up_all(nmu * nhg);
          std::vector<double> bdir((size_t)nmu * (nlay + 1), 0.0), bdn(bdir), bup(bdir);
          for (int m = 0; m < nmu; ++m) {
            ck(ecckd_rt_sw_gpoints_rayleigh(dev.ctx(), 1, nlay, ng, mu0[m], nl.surf_albedo, incoming.data(), od.data(), ray.data(), &dir_all[m * nhg],
                                            &dn_all[m * nhg], &up_all[m * nhg]));
            for (int i = 0; i <= nlay; ++i)
              for (int g = 0; g < ng; ++g) {
                bdir[(size_t)m * (nlay + 1) + i] += dir_all[m * nhg + (size_t)i * ng + g];
                bdn[(size_t)m * (nlay + 1) + i] += dn_all[m * nhg + (size_t)i * ng + g];
                bup[(size_t)m * (nlay + 1) + i] += up_all[m * nhg + (size_t)i * ng + g];
              }
          }
          out.write_slice("pressure_hl", c, f.read("pressure_hl", c));
          out.write_slice("flux_dn_direct_sw", c, bdir); out.write_slice("flux_dn_sw", c, bdn); out.write_slice("flux_up_sw", c, bup);
          out.write_slice("spectral_flux_dn_direct_sw", c, dir_all); out.write_slice("spectral_flux_dn_sw", c, dn_all);
          out.write_slice("spectral_flux_up_sw", c, up_all);
        }
        else for (int c = 0; c < ncol; ++c) {
          std::vector<double> od = f.read("optical_depth", c);
          if (have_ray) {                       // one more absorber, as in the reference's forward model (solve_adept.cpp:34)
            const std::vector<double> ray = f.read("rayleigh_optical_depth", c);
            for (size_t i = 0; i < od.size(); ++i) od[i] += ray[i];
          }
          const std::vector<double> incoming = f.read("incoming_sw", c);
          std::vector<double> dn_all(nmu * nhg), up_all(nmu * nhg), bdn((size_t)nmu * (nlay + 1), 0.0), bup((size_t)nmu * (nlay + 1), 0.0);
          for (int m = 0; m < nmu; ++m) {
            // radiative_transfer_sw.cpp:45-77 per g point, on the device (ecckd_rt_sw_gpoints)
            ck(ecckd_rt_sw_gpoints(dev.ctx(), 1, nlay, ng, mu0[m], nl.surf_albedo, incoming.data(), od.data(), &dn_all[m * nhg], &up_all[m * nhg]));
            for (int i = 0; i <= nlay; ++i)
              for (int g = 0; g < ng; ++g) {
                bdn[(size_t)m * (nlay + 1) + i] += dn_all[m * nhg + (size_t)i * ng + g];
                bup[(size_t)m * (nlay + 1) + i] += up_all[m * nhg + (size_t)i * ng + g];
              }
          }
          out.write_slice("pressure_hl", c, f.read("pressure_hl", c));
          out.write_slice("flux_dn_direct_sw", c, bdn); out.write_slice("flux_dn_sw", c, bdn); out.write_slice("flux_up_sw", c, bup);
          out.write_slice("spectral_flux_dn_direct_sw", c, dn_all); out.write_slice("spectral_flux_up_sw", c, up_all);
        }
        out.close();
        return done(0);
      }
      if (!f.exist("planck_hl")) fail(ECCKD_PARAMETER_ERROR, "%s holds no planck_hl: not a longwave optical-depth file", ckd_file.c_str());
      NcOut out(output);
      out.dim("column", ncol); out.dim("half_level", nlay + 1); out.dim("g_point", ng);
      out.var("pressure_hl", NC_FLOAT_T, {"column", "half_level"}, "Pressure at half levels", "Pa");
      out.var("flux_up_lw", NC_FLOAT_T, {"column", "half_level"}, "Upwelling longwave flux", "W m-2");
      out.var("flux_dn_lw", NC_FLOAT_T, {"column", "half_level"}, "Downwelling longwave flux", "W m-2");
      out.var("spectral_flux_up_lw", NC_FLOAT_T, {"column", "half_level", "g_point"}, "Upwelling longwave flux per g point", "W m-2");
      out.var("spectral_flux_dn_lw", NC_FLOAT_T, {"column", "half_level", "g_point"}, "Downwelling longwave flux per g point", "W m-2");
      if (!scenario.empty()) out.att(scenario, "scenario");
      out.att(history, "history");
      out.end_define();
      const size_t nhg = (size_t)(nlay + 1) * ng;
      for (int c = 0; c < ncol; ++c) {
        const std::vector<double> od = f.read("optical_depth", c), planck = f.read("planck_hl", c);
        std::vector<double> dn(nhg), up(nhg), bdn(nlay + 1, 0.0), bup(nlay + 1, 0.0);
        // radiative_transfer_lw.cpp:27-60 per g point (two-stream or nangle Gauss-Legendre angles), on the device
        ck(ecckd_rt_lw_gpoints(dev.ctx(), nl.nangle, 1, nlay, ng, planck.data(), od.data(), dn.data(), up.data()));
        for (int i = 0; i <= nlay; ++i)
          for (int g = 0; g < ng; ++g) { bdn[i] += dn[(size_t)i * ng + g]; bup[i] += up[(size_t)i * ng + g]; }
        out.write_slice("pressure_hl", c, f.read("pressure_hl", c));
        out.write_slice("flux_dn_lw", c, bdn); out.write_slice("flux_up_lw", c, bup);
        out.write_slice("spectral_flux_dn_lw", c, dn); out.write_slice("spectral_flux_up_lw", c, up);
      }
      out.close();
      return done(0);
    }

    if (gases.empty()) fail(ECCKD_PARAMETER_ERROR, "No spectrum files given");
    // ---- grids and profiles from the first file; every other file must share them ----
    Spectrum first = read_spectrum(gases[0].path, 0, false);
    const int nlay = first.nlay, ncol_file = first.ncol;
    const size_t nwav = first.nwav;
    int c0 = 0, c1 = ncol_file - 1;
    if (col_a >= 1) { c0 = (int)col_a - 1; c1 = std::min<long>(col_b, ncol_file) - 1; }   // 1-based, inclusive, like the Fortran tool
    const int ncol = c1 - c0 + 1;
    if (ncol <= 0) fail(ECCKD_PARAMETER_ERROR, "Empty column range");
    LOG("%d gas file(s), %d column(s), %d layers, %zu spectral points\n", (int)gases.size(), ncol, nlay, nwav);

    Device dev;
    DevBuf d_merged;
    if (table.empty()) d_merged.alloc(dev, (size_t)nlay * nwav * sizeof(double));
    DevBuf d_wn, d_dwn;
    d_wn.upload(dev, first.wavenumber_cm_1);
    d_dwn.upload(dev, first.d_wavenumber_cm_1);
    DevBuf d_ssi, d_albedo;
    std::vector<double> mu0 = nl.mu0;
    if (sw && !merge_only) {
      if (ssi_file.empty()) fail(ECCKD_PARAMETER_ERROR, "\"--ssi\" file not specified");
      NcIn fs(ssi_file);
      const std::vector<double> ssi = fs.read("solar_spectral_irradiance");
      if (ssi.size() != nwav) fail(ECCKD_PARAMETER_ERROR, "solar_spectral_irradiance has %zu points, the spectra %zu", ssi.size(), nwav);
      d_ssi.upload(dev, ssi);
      d_albedo.upload(dev, std::vector<double>(nwav, nl.surf_albedo));
      if (mu0.empty()) fail(ECCKD_PARAMETER_ERROR, "cos_solar_zenith_angle missing from the namelist");
    }
    const int nmu = (int)mu0.size();
    std::string ids;
    std::vector<std::string> molecules;
    for (const GasArg& g : gases) {
      NcIn f(g.path);
      std::string m;
      if (!f.att_text("constituent_id", m)) f.att_text("molecules", m);
      molecules.push_back(m.substr(0, m.find(' ')));
      ids += (ids.empty() ? "" : " ") + molecules.back();
    }

    // bands of the namelist -> wavenumber index ranges
    std::vector<int64_t> bbegin, bend;
    int nband = 0;
    if (!merge_only) {
      if (nl.band1.empty() || nl.band1.size() != nl.band2.size())
        fail(ECCKD_PARAMETER_ERROR, "band_wavenumber1 / band_wavenumber2 missing from the namelist");
      nband = (int)nl.band1.size();
      bbegin.resize(nband); bend.resize(nband);
      ck(ecckd_band_ranges(nwav, first.wavenumber_cm_1.data(), nband, nl.band1.data(), nl.band2.data(), nullptr, bbegin.data(), bend.data()));
    }

    // ---------------------------------------------------------------------------------------------------------------
    if (!table.empty()) {   // every scenario of the table from one read of the gas files per column
      const size_t nscen = table.size(), ngas = gases.size(), nhl = (size_t)nlay + 1;
      std::vector<std::unique_ptr<NcOut>> outs;
      for (const ScenarioRow& row : table) {
        outs.emplace_back(new NcOut(row.output));
        NcOut& o = *outs.back();
        o.dim("column", ncol); o.dim("half_level", nlay + 1); o.dim("level", nlay);
        o.var("pressure_hl", NC_FLOAT_T, {"column", "half_level"}, "Pressure at half levels", "Pa");
        o.var("temperature_hl", NC_FLOAT_T, {"column", "half_level"}, "Temperature at half levels", "K");
        define_flux_variables(o, sw, ngas, nmu, nband, nwav, ids, nl.boundary_fluxes);
        o.att(row.name, "scenario");
        o.att(history, "history");
        o.end_define();
        if (sw) { o.write("band_wavenumber1_sw", nl.band1); o.write("band_wavenumber2_sw", nl.band2); o.write("mu0", mu0); }
        else { o.write("band_wavenumber1_lw", nl.band1); o.write("band_wavenumber2_lw", nl.band2); }
        if (nl.boundary_fluxes) o.write("wavenumber", first.wavenumber_cm_1);
      }
      const size_t nslot = sw ? nscen * nmu : nscen;            // rows of fluxes: (scenario[, angle])
      const int ngroup = sw ? std::min(8, nmu) : 1;              // angles per call: the entry takes up to 8
      DevBuf d_sdn, d_tup;
      if (nl.boundary_fluxes) { d_sdn.alloc(dev, nscen * ngroup * nwav * sizeof(double)); d_tup.alloc(dev, nscen * ngroup * nwav * sizeof(double)); }
      double* const p_sdn = nl.boundary_fluxes ? d_sdn.as<double>() : nullptr;
      double* const p_tup = nl.boundary_fluxes ? d_tup.as<double>() : nullptr;
      for (int c = c0; c <= c1; ++c) {
        const Spectrum col = c == 0 ? first : read_spectrum(gases[0].path, c, false);
        std::vector<DevOd> ods;                                  // the gases side by side on the device, read once
        std::vector<const void*> od_ptr;
        std::vector<int> od_type;
        std::vector<size_t> od_stride(ngas, nwav);
        std::vector<double> scale(nscen * ngas * nlay), vmr_all(nscen * ngas * nlay);   // [scenario][gas][level]
        for (size_t ig = 0; ig < ngas; ++ig) {
          NcIn f(gases[ig].path);
          double ref = -1.0;
          std::vector<double> vmr, profile, vmr_out;
          std::string mol;
          read_od_meta(f, c, nlay, ref, vmr, mol);
          for (size_t s = 0; s < nscen; ++s) {
            gas_scaling(table[s].specs[ig], gases[ig].path, nlay, col.pressure_hl, ref, vmr, profile, vmr_out);
            std::copy(profile.begin(), profile.end(), scale.begin() + (s * ngas + ig) * nlay);
            std::copy(vmr_out.begin(), vmr_out.end(), vmr_all.begin() + (s * ngas + ig) * nlay);
          }
          ods.push_back(read_od_dev(dev, f, c, nlay, nwav));
          od_ptr.push_back(ods.back().buf.ptr());
          od_type.push_back(ods.back().type);
        }
        ck(ecckd_synchronize(dev.ctx()));
        std::vector<double> bdn(nslot * nband * nhl), bup(nslot * nband * nhl);
        std::vector<double> all_dn, all_up;                      // [slot][wavenumber] boundary fluxes of this column
        if (nl.boundary_fluxes) { all_dn.resize(nslot * nwav); all_up.resize(nslot * nwav); }
        if (sw) {
          for (int m0 = 0; m0 < nmu; m0 += ngroup) {             // [scenario][angle] rows per group of angles
            const size_t nm = (size_t)std::min(ngroup, nmu - m0);
            std::vector<double> gdn(nscen * nm * nband * nhl), gup(gdn.size());
            ck(ecckd_lbl_band_fluxes_sw_scenarios(dev.ctx(), nlay, nwav, (int)nm, mu0.data() + m0, d_ssi.as<double>(), d_albedo.as<double>(), (int)ngas,
                                                  od_ptr.data(), od_type.data(), od_stride.data(), (int)nscen, scale.data(), nband, bbegin.data(),
                                                  bend.data(), gdn.data(), gup.data(), p_sdn, p_tup));
            std::vector<double> a, b;
            if (nl.boundary_fluxes) { a = d_sdn.download<double>(); b = d_tup.download<double>(); }
            for (size_t s = 0; s < nscen; ++s) {
              const size_t n = nm * nband * nhl, to = (s * nmu + m0) * nband * nhl;
              std::copy(gdn.begin() + s * n, gdn.begin() + (s + 1) * n, bdn.begin() + to);
              std::copy(gup.begin() + s * n, gup.begin() + (s + 1) * n, bup.begin() + to);
              if (nl.boundary_fluxes) {
                std::copy(a.begin() + s * nm * nwav, a.begin() + (s + 1) * nm * nwav, all_dn.begin() + (s * nmu + m0) * nwav);
                std::copy(b.begin() + s * nm * nwav, b.begin() + (s + 1) * nm * nwav, all_up.begin() + (s * nmu + m0) * nwav);
              }
            }
          }
        } else {
          if (col.temperature_hl.empty()) fail(ECCKD_PARAMETER_ERROR, "temperature_hl missing from %s", gases[0].path.c_str());
          ck(ecckd_lbl_band_fluxes_lw_scenarios(dev.ctx(), nl.nangle, nlay, nwav, col.temperature_hl.data(), d_wn.as<double>(), d_dwn.as<double>(),
                                                (int)ngas, od_ptr.data(), od_type.data(), od_stride.data(), (int)nscen, scale.data(), nband,
                                                bbegin.data(), bend.data(), bdn.data(), bup.data(), p_sdn, p_tup));
          if (nl.boundary_fluxes) { all_dn = d_sdn.download<double>(); all_up = d_tup.download<double>(); }
        }
        const size_t oc = (size_t)(c - c0), per = sw ? (size_t)nmu : 1;   // rows per scenario
        std::vector<double> tdn(per * nhl * nband), tup(per * nhl * nband), sdn(per * nhl), sup(per * nhl);
        for (size_t s = 0; s < nscen; ++s) {
          NcOut& o = *outs[s];
          o.write_slice("pressure_hl", oc, col.pressure_hl);
          if (!col.temperature_hl.empty()) o.write_slice("temperature_hl", oc, col.temperature_hl);
          for (size_t m = 0; m < per; ++m) {
            bands_to_file_order(nband, nhl, &bdn[(s * per + m) * nband * nhl], &tdn[m * nhl * nband], &sdn[m * nhl]);
            bands_to_file_order(nband, nhl, &bup[(s * per + m) * nband * nhl], &tup[m * nhl * nband], &sup[m * nhl]);
          }
          o.write_slice("mole_fraction_fl", oc, std::vector<double>(vmr_all.begin() + s * ngas * nlay, vmr_all.begin() + (s + 1) * ngas * nlay));
          if (sw) {
            o.write_slice("band_flux_dn_direct_sw", oc, tdn); o.write_slice("band_flux_up_sw", oc, tup);
            o.write_slice("flux_dn_direct_sw", oc, sdn); o.write_slice("flux_dn_sw", oc, sdn); o.write_slice("flux_up_sw", oc, sup);
          } else {
            o.write_slice("band_flux_dn_lw", oc, tdn); o.write_slice("band_flux_up_lw", oc, tup);
            o.write_slice("flux_dn_lw", oc, sdn); o.write_slice("flux_up_lw", oc, sup);
          }
          if (nl.boundary_fluxes) {
            const std::vector<double> a(all_dn.begin() + s * per * nwav, all_dn.begin() + (s + 1) * per * nwav);
            const std::vector<double> b(all_up.begin() + s * per * nwav, all_up.begin() + (s + 1) * per * nwav);
            o.write_slice(sw ? "spectral_flux_dn_direct_surf_sw" : "spectral_flux_dn_surf_lw", oc, a);
            o.write_slice(sw ? "spectral_flux_up_toa_sw" : "spectral_flux_up_toa_lw", oc, b);
          }
        }
        LOG("  column %d done (%zu scenarios)\n", c + 1, nscen);
      }
      for (auto& o : outs) o->close();
      return done(0);
    }

    NcOut out(output);
    out.dim("column", ncol); out.dim("half_level", nlay + 1); out.dim("level", nlay);
    out.var("pressure_hl", NC_FLOAT_T, {"column", "half_level"}, "Pressure at half levels", "Pa");
    out.var("temperature_hl", NC_FLOAT_T, {"column", "half_level"}, "Temperature at half levels", "K");
    if (merge_only) {
      out.dim("wavenumber", nwav);
      out.var("wavenumber", NC_DOUBLE_T, {"wavenumber"}, "Wavenumber", "cm-1");
      out.var("optical_depth", NC_FLOAT_T, {"column", "level", "wavenumber"}, "Layer optical depth");
      out.att(ids, "molecules");
      out.att("composite", "constituent_id");
    } else {
      define_flux_variables(out, sw, gases.size(), nmu, nband, nwav, ids, nl.boundary_fluxes, !rayleigh_file.empty());
    }
    if (!scenario.empty()) out.att(scenario, "scenario");
    out.att(history, "history");
    out.end_define();
    if (merge_only) out.write("wavenumber", first.wavenumber_cm_1);
    else if (sw) { out.write("band_wavenumber1_sw", nl.band1); out.write("band_wavenumber2_sw", nl.band2); out.write("mu0", mu0); }
    else { out.write("band_wavenumber1_lw", nl.band1); out.write("band_wavenumber2_lw", nl.band2); }
    DevBuf d_bnd_dn, d_bnd_up;
    if (!merge_only && nl.boundary_fluxes) {
      out.write("wavenumber", first.wavenumber_cm_1);
      d_bnd_dn.alloc(dev, nwav * sizeof(double));
      d_bnd_up.alloc(dev, nwav * sizeof(double));
    }
    double* const p_bnd_dn = nl.boundary_fluxes && !merge_only ? d_bnd_dn.as<double>() : nullptr;
    double* const p_bnd_up = nl.boundary_fluxes && !merge_only ? d_bnd_up.as<double>() : nullptr;
    const int ngroup = std::min(8, std::max(nmu, 1));          // --rayleigh: angles per call, the entry takes up to 8
    DevBuf d_ray_dir, d_ray_dn, d_ray_up;                      // their boundary fluxes, [angle][wavenumber]
    if (!rayleigh_file.empty() && nl.boundary_fluxes)
      for (DevBuf* b : {&d_ray_dir, &d_ray_dn, &d_ray_up}) b->alloc(dev, (size_t)ngroup * nwav * sizeof(double));

    for (int c = c0; c <= c1; ++c) {
      const Spectrum col = c == 0 ? first : read_spectrum(gases[0].path, c, false);
      std::vector<double> vmr_all;   // [gas][level]
      for (size_t ig = 0; ig < gases.size(); ++ig) {
        const GasArg& g = gases[ig];
        NcIn f(g.path);
        double ref = -1.0;
        std::vector<double> vmr;
        std::string mol;
        read_od_meta(f, c, nlay, ref, vmr, mol);
        std::vector<double> profile, vmr_out;
        gas_scaling(g, g.path, nlay, col.pressure_hl, ref, vmr, profile, vmr_out);
        vmr_all.insert(vmr_all.end(), vmr_out.begin(), vmr_out.end());
        DevOd od = read_od_dev(dev, f, c, nlay, nwav);
        ck(ecckd_merge_spectrum_dev(dev.ctx(), nlay, nwav, od.buf.ptr(), od.type, nwav, profile.data(), ig == 0 ? 1 : 0,
                                    d_merged.as<double>(), nwav));
        ck(ecckd_synchronize(dev.ctx()));
      }
      const size_t oc = (size_t)(c - c0);
      out.write_slice("pressure_hl", oc, col.pressure_hl);
      if (!col.temperature_hl.empty()) out.write_slice("temperature_hl", oc, col.temperature_hl);
      if (merge_only) {
        out.write_slice("optical_depth", oc, d_merged.download<double>());
      } else if (sw && !rayleigh_file.empty()) {   // the absorbers merged above, the Rayleigh spectrum beside them: two-stream
        const size_t nhl = (size_t)nlay + 1;
        NcIn fr(rayleigh_file);
        const DevOd ray = read_od_dev(dev, fr, c, nlay, nwav);
        ck(ecckd_synchronize(dev.ctx()));
        std::vector<double> tdir((size_t)nmu * nhl * nband), tdn(tdir.size()), tup(tdir.size()), sdir((size_t)nmu * nhl), sdn(sdir.size()), sup(sdir.size());
        std::vector<double> all_dir, all_dn, all_up;     // (mu0, wavenumber) boundary fluxes of this column
        const bool bnd = nl.boundary_fluxes;
        for (int m0 = 0; m0 < nmu; m0 += ngroup) {
          const int nm = std::min(ngroup, nmu - m0);
          std::vector<double> gdir((size_t)nm * nband * nhl), gdn(gdir.size()), gup(gdir.size());
          ck(ecckd_lbl_band_fluxes_sw_rayleigh(dev.ctx(), nlay, nwav, nm, mu0.data() + m0, d_ssi.as<double>(), d_albedo.as<double>(), d_merged.ptr(),
                                               ECCKD_F64, nwav, ray.buf.ptr(), ray.type, nwav, nband, bbegin.data(), bend.data(), gdir.data(),
                                               gdn.data(), gup.data(), bnd ? d_ray_dir.as<double>() : nullptr, bnd ? d_ray_dn.as<double>() : nullptr,
                                               bnd ? d_ray_up.as<double>() : nullptr));
          if (bnd) {
            const std::vector<double> a = d_ray_dir.download<double>(), b = d_ray_dn.download<double>(), u = d_ray_up.download<double>();
            all_dir.insert(all_dir.end(), a.begin(), a.begin() + (size_t)nm * nwav);
            all_dn.insert(all_dn.end(), b.begin(), b.begin() + (size_t)nm * nwav);
            all_up.insert(all_up.end(), u.begin(), u.begin() + (size_t)nm * nwav);
          }
          for (int m = 0; m < nm; ++m) {
            const size_t from = (size_t)m * nband * nhl, to = (size_t)(m0 + m);
            bands_to_file_order(nband, nhl, &gdir[from], &tdir[to * nhl * nband], &sdir[to * nhl]);
            bands_to_file_order(nband, nhl, &gdn[from], &tdn[to * nhl * nband], &sdn[to * nhl]);
            bands_to_file_order(nband, nhl, &gup[from], &tup[to * nhl * nband], &sup[to * nhl]);
          }
        }
        out.write_slice("mole_fraction_fl", oc, vmr_all);
        out.write_slice("band_flux_dn_direct_sw", oc, tdir); out.write_slice("band_flux_dn_sw", oc, tdn); out.write_slice("band_flux_up_sw", oc, tup);
        out.write_slice("flux_dn_direct_sw", oc, sdir); out.write_slice("flux_dn_sw", oc, sdn); out.write_slice("flux_up_sw", oc, sup);
        if (bnd) {
          out.write_slice("spectral_flux_dn_direct_surf_sw", oc, all_dir); out.write_slice("spectral_flux_dn_surf_sw", oc, all_dn);
          out.write_slice("spectral_flux_up_toa_sw", oc, all_up);
        }
      } else if (sw) {
        const size_t nhl = (size_t)nlay + 1;
        std::vector<double> tdn((size_t)nmu * nhl * nband), tup((size_t)nmu * nhl * nband), sdn((size_t)nmu * nhl, 0.0), sup((size_t)nmu * nhl, 0.0);
        std::vector<double> bdn((size_t)nband * nhl), bup((size_t)nband * nhl);
        std::vector<double> all_dn, all_up;     // (mu0, wavenumber) boundary fluxes of this column
        for (int m = 0; m < nmu; ++m) {
          ck(ecckd_lbl_band_fluxes_sw_ex(dev.ctx(), nlay, nwav, mu0[m], d_ssi.as<double>(), d_albedo.as<double>(), d_merged.ptr(), ECCKD_F64, nwav,
                                         nband, bbegin.data(), bend.data(), bdn.data(), bup.data(), p_bnd_dn, p_bnd_up));
          if (p_bnd_dn) {
            const std::vector<double> a = d_bnd_dn.download<double>(), b = d_bnd_up.download<double>();
            all_dn.insert(all_dn.end(), a.begin(), a.end());
            all_up.insert(all_up.end(), b.begin(), b.end());
          }
          for (int b = 0; b < nband; ++b)
            for (size_t i = 0; i < nhl; ++i) {
              tdn[((size_t)m * nhl + i) * nband + b] = bdn[(size_t)b * nhl + i];
              tup[((size_t)m * nhl + i) * nband + b] = bup[(size_t)b * nhl + i];
              sdn[(size_t)m * nhl + i] += bdn[(size_t)b * nhl + i];
              sup[(size_t)m * nhl + i] += bup[(size_t)b * nhl + i];
            }
        }
        out.write_slice("mole_fraction_fl", oc, vmr_all);
        out.write_slice("band_flux_dn_direct_sw", oc, tdn); out.write_slice("band_flux_up_sw", oc, tup);
        out.write_slice("flux_dn_direct_sw", oc, sdn); out.write_slice("flux_dn_sw", oc, sdn); out.write_slice("flux_up_sw", oc, sup);
        if (p_bnd_dn) { out.write_slice("spectral_flux_dn_direct_surf_sw", oc, all_dn); out.write_slice("spectral_flux_up_toa_sw", oc, all_up); }
      } else {
        if (col.temperature_hl.empty()) fail(ECCKD_PARAMETER_ERROR, "temperature_hl missing from %s", gases[0].path.c_str());
        std::vector<double> bdn((size_t)nband * (nlay + 1)), bup((size_t)nband * (nlay + 1));
        ck(ecckd_lbl_band_fluxes_lw_angles(dev.ctx(), nl.nangle, nlay, nwav, col.temperature_hl.data(), d_wn.as<double>(), d_dwn.as<double>(),
                                       d_merged.ptr(), ECCKD_F64, nwav, nband, bbegin.data(), bend.data(), bdn.data(), bup.data(),
                                       p_bnd_dn, p_bnd_up));
        // [band][level] -> (half_level, band) and the broadband sums
        std::vector<double> tdn((size_t)(nlay + 1) * nband), tup((size_t)(nlay + 1) * nband), sdn(nlay + 1, 0.0), sup(nlay + 1, 0.0);
        for (int b = 0; b < nband; ++b)
          for (int i = 0; i <= nlay; ++i) {
            tdn[(size_t)i * nband + b] = bdn[(size_t)b * (nlay + 1) + i];
            tup[(size_t)i * nband + b] = bup[(size_t)b * (nlay + 1) + i];
            sdn[i] += bdn[(size_t)b * (nlay + 1) + i];
            sup[i] += bup[(size_t)b * (nlay + 1) + i];
          }
        out.write_slice("mole_fraction_fl", oc, vmr_all);
        out.write_slice("band_flux_dn_lw", oc, tdn); out.write_slice("band_flux_up_lw", oc, tup);
        out.write_slice("flux_dn_lw", oc, sdn); out.write_slice("flux_up_lw", oc, sup);
        if (p_bnd_dn) {
          out.write_slice("spectral_flux_dn_surf_lw", oc, d_bnd_dn.download<double>());
          out.write_slice("spectral_flux_up_toa_lw", oc, d_bnd_up.download<double>());
        }
      }
      LOG("  column %d done\n", c + 1);
    }
    out.close();
    return done(0);
  } catch (const Fatal& f) {
    std::fprintf(stderr, "*** Error: %s\n", f.msg.c_str());
    return f.code ? f.code : 1;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "*** Error: %s\n", e.what());
    return ECCKD_UNEXPECTED_EXCEPTION;
  }
}
