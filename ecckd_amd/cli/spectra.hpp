// spectra.hpp - bin/lw_spectra and bin/sw_spectra (their header comments say what each one is): line-by-line fluxes of every
// column (or of column `iprofile`) of a merged spectrum, written per wavenumber or, with `gpoints`, summed over the wavenumbers
// of each g point, together with the optical depth.  One program: the shortwave tool has an angle dimension, the `ssi` input
// and its own names; the longwave tool keeps the reference's quirks (src/ecckd/lw_spectra.cpp:31-275).
//
// scenarios=TABLE (both tools): the scenarios of a training set - they differ in one scaling per gas file - from ONE read of the
// spectra.  TABLE has the grammar of `ckdmip_lw --scenarios` (scenario_table.hpp): one line per scenario,
// NAME OUTPUT SPEC_1 ... SPEC_n, one SPEC per file of `input` in `input` order;  asis,  scale=S  and  conc=C  are what element i
// of `scaling` / `conc` is to ecckd_merge_scaling;  const=C  is refused.  Per column every gas file is read once and stays on
// the device as stored; scenario after scenario the gases are merged in one pass into one DOUBLE matrix
// (ecckd_merge_scenario_dev: the bits read_merged_spectrum leaves) and the record is written into the scenario's own OUTPUT,
// which is the file `output=OUTPUT scaling=... conc=...` writes, plus the global attribute `scenario`.  `output`, `scaling`,
// `conc` and `conc_input` are refused beside the key; every other key means to every line what it means to a single run.
#pragma once
#include <algorithm>
#include <memory>

#include "scenario_table.hpp"
#include "tool.hpp"

using namespace tool;

namespace {

// optical depths on the device as doubles on the host, from FLOAT or DOUBLE as they are
std::vector<double> download_od(const Device& dev, const void* d_od, int od_type, size_t n) {
  std::vector<double> od(n);
  if (od_type == ECCKD_F32) {
    std::vector<float> f(n);
    if (n) ck(ecckd_d2h(dev.ctx(), f.data(), d_od, n * sizeof(float)));
    std::copy(f.begin(), f.end(), od.begin());
  } else {
    ck(ecckd_d2h(dev.ctx(), od.data(), d_od, od.size() * sizeof(double)));
  }
  return od;
}

std::vector<double> download_as_double(const DevBuf& b) {
  const std::vector<float> f = b.download<float>();
  return std::vector<double>(f.begin(), f.end());
}

// the same file?  By name, or by what both names resolve to where both exist
bool same_file(const std::string& a, const std::string& b) {
  if (a == b) return true;
  char ra[PATH_MAX], rb[PATH_MAX];
  return realpath(a.c_str(), ra) && realpath(b.c_str(), rb) && std::string(ra) == rb;
}

// One column of the gas files of a table run: every file's optical depths on the device as stored, and what the scalings need
struct ColumnGases {
  Spectrum first;                               // grid, pressures, temperatures of the first file
  std::string molecules;
  std::vector<DevOd> od;
  std::vector<double> reference_surface_vmr;
  std::vector<std::vector<double>> vmr_fl;      // as the files hold them
};

ColumnGases read_column_gases(const Device& dev, const std::vector<std::string>& paths, int iprofile) {
  ColumnGases c;
  for (size_t ibg = 0; ibg < paths.size(); ++ibg) {      // file by file as read_merged_spectrum reads them (tool.hpp)
    LOG("  Reading %s\n", paths[ibg].c_str());
    NcIn f(paths[ibg]);
    double ref = -1.0;
    std::vector<double> vmr;
    std::string molecule;
    if (ibg == 0) {
      c.first = read_spectrum(paths[ibg], iprofile, false);
      ref = c.first.reference_surface_vmr; vmr = c.first.vmr_fl; molecule = c.first.molecule;
      c.molecules = molecule;
    } else {
      read_od_meta(f, iprofile, c.first.nlay, ref, vmr, molecule);
      if (molecule.empty()) fail(ECCKD_PARAMETER_ERROR, "Found neither \"constituent_id\" nor \"molecules\" amongst the global attributes");
      c.molecules += " " + molecule;
    }
    c.od.push_back(read_od_dev(dev, f, iprofile, c.first.nlay, c.first.nwav));
    c.reference_surface_vmr.push_back(ref);
    c.vmr_fl.push_back(vmr);
  }
  return c;
}

}  // namespace

inline int spectra_main(int argc, char** argv, bool sw) {
  return run(argc, argv, [&](Config& config) -> int {
    std::string output, ssi_file_name, rayleigh_file_name, scenarios_file;
    const bool have_scenarios = config.read(scenarios_file, "scenarios");
    if (have_scenarios) {                       // names, outputs and scalings come from the table
      for (const char* key : {"output", "scaling", "conc", "conc_input"})
        if (config.exist(key))
          fail(ECCKD_PARAMETER_ERROR, "\"%s\" cannot be combined with \"scenarios\" (outputs and scalings come from the table)", key);
    } else if (!config.read(output, "output")) fail(ECCKD_PARAMETER_ERROR, "\"output\" file not specified");
    std::vector<double> mu0;
    double surface_albedo = 0.15;
    if (sw) {                                   // every check of the shortwave parameters before a device is opened
      if (!config.read(ssi_file_name, "ssi")) fail(ECCKD_PARAMETER_ERROR, "\"ssi\" file not specified");
      if (!config.read(mu0, "cos_solar_zenith_angle")) mu0 = {0.5};
      if (mu0.empty() || mu0.size() > 8) fail(ECCKD_PARAMETER_ERROR, "cos_solar_zenith_angle must list 1 to 8 numbers");
      for (double m : mu0)
        if (!(m > 0.0 && m <= 1.0)) fail(ECCKD_PARAMETER_ERROR, "cos_solar_zenith_angle %g is not in (0, 1]", m);
      config.read(surface_albedo, "surface_albedo");
    }
    // rayleigh=FILE (shortwave): a spectrum file whose optical_depth scatters, beside the merged absorbers (two-stream transfer)
    const bool rayleigh = config.read(rayleigh_file_name, "rayleigh");
    if (rayleigh && !sw) fail(ECCKD_PARAMETER_ERROR, "\"rayleigh\" is a key of sw_spectra: the longwave fluxes do not scatter");
    // nangle=N (longwave): N Gauss-Legendre zenith angles per hemisphere in place of the two-stream form (0), the CKDMIP tool's key
    int nangle = 0;
    const bool have_nangle = config.read(nangle, "nangle");
    if (have_nangle && sw) fail(ECCKD_PARAMETER_ERROR, "\"nangle\" is a key of lw_spectra: the shortwave angles are cos_solar_zenith_angle");
    if (nangle < 0 || nangle > 16) fail(ECCKD_PARAMETER_ERROR, "nangle = %d outside 0..16", nangle);
    const int nmu = sw ? (int)mu0.size() : 1;   // rows of fluxes per column
    SearchPath paths;
    paths.configure(config);
    // scenarios=TABLE: every check of the table before a device is opened or a file created
    std::vector<ScenarioRow> table;
    std::vector<std::string> inputs;
    if (have_scenarios) {
      inputs = config.read_list("input");
      if (inputs.empty()) fail(ECCKD_PARAMETER_ERROR, "Unable to read input file names in input");
      if (inputs.size() > 16) fail(ECCKD_PARAMETER_ERROR, "\"scenarios\": %zu input files, 16 at most", inputs.size());
      table = read_scenarios(scenarios_file, inputs.size());
      std::vector<std::pair<std::string, std::string>> read_files;      // (key, file) of everything this run reads
      for (const std::string& f : inputs) read_files.push_back({"input", f});
      std::string gpoint_file;
      if (config.read(gpoint_file, "gpoints")) read_files.push_back({"gpoints", gpoint_file});
      if (sw) read_files.push_back({"ssi", ssi_file_name});
      if (rayleigh) read_files.push_back({"rayleigh", rayleigh_file_name});
      for (const ScenarioRow& row : table) {
        for (const GasArg& a : row.specs)
          if (a.mode == GasArg::CONST)
            fail(ECCKD_PARAMETER_ERROR, "%s: scenario \"%s\": const=C is not a scaling of %s (asis, scale=S or conc=C)", scenarios_file.c_str(),
                 row.name.c_str(), sw ? "sw_spectra" : "lw_spectra");
        for (const auto& kf : read_files) {
          std::string found = kf.second;
          try { found = paths.find(kf.second); } catch (const Fatal&) {}     // a file that is missing fails where it is read
          if (same_file(row.output, kf.second) || same_file(row.output, found))
            fail(ECCKD_PARAMETER_ERROR, "%s: scenario \"%s\": the output \"%s\" is the %s file of this run", scenarios_file.c_str(),
                 row.name.c_str(), row.output.c_str(), kf.first.c_str());
        }
      }
    }
    Device dev;

    // ---- g points (:63-74) ----
    std::vector<int32_t> g_point;
    int ng = -1;
    const bool have_gpoints = config.exist("gpoints");
    if (have_gpoints) {
      std::string gpoint_file;
      config.read(gpoint_file, "gpoints");
      const std::vector<double> g = NcIn(paths.find(gpoint_file)).read("g_point");
      g_point.assign(g.begin(), g.end());
      for (int32_t v : g_point) ng = std::max(ng, (int)v + 1);
      if (ng < 1) fail(ECCKD_PARAMETER_ERROR, "%s assigns no wavenumber to a g point", gpoint_file.c_str());
    }
    std::vector<double> ssi;
    if (sw) {
      LOG("Reading %s\n", ssi_file_name.c_str());
      ssi = NcIn(paths.find(ssi_file_name)).read("solar_spectral_irradiance");
    }
    int iprofile = -1;
    const bool do_one_profile = config.read(iprofile, "iprofile");
    int icol = do_one_profile ? iprofile : 0;
    int ncol = 10000;
    size_t irec = 0;

    std::vector<std::unique_ptr<NcOut>> files;  // one, or one per line of the table: all open at once
    if (have_scenarios) for (const ScenarioRow& row : table) files.emplace_back(new NcOut(row.output));
    else files.emplace_back(new NcOut(output));
    ecckd_gmap* gmap = nullptr;
    DevBuf d_wn, d_dwn, d_g, d_ssi, d_albedo, d_spec_dn, d_spec_up, d_spec_tot;
    std::string rayleigh_path;
    std::vector<double> solar;                  // solar irradiance across each g point
    const std::string spec_name = have_gpoints ? "g_point" : "wavenumber";
    const std::string bb_dn_name = sw ? "flux_dn_direct_sw" : "flux_dn_lw", bb_up_name = sw ? "flux_up_sw" : "flux_up_lw";
    const std::string spec_dn_name = "spectral_" + bb_dn_name, spec_up_name = "spectral_" + bb_up_name;
    bool is_first_profile = true, have_temperature = true;

    // The first column read: the inputs checked against its grid
    auto check_first_column = [&](const Spectrum& first) {
      const int nlay = first.nlay;
      const size_t nwav = first.nwav;
      if (have_gpoints && g_point.size() != nwav)
        fail(ECCKD_PARAMETER_ERROR, "g_point has %zu elements, the spectrum %zu wavenumbers", g_point.size(), nwav);
      if (sw && ssi.size() != nwav)
        fail(ECCKD_PARAMETER_ERROR, "solar_spectral_irradiance has %zu points, the spectrum %zu", ssi.size(), nwav);
      if (sw) have_temperature = !first.temperature_hl.empty();
      if (rayleigh) {                         // the grid of the spectrum that scatters is the merged one's
        rayleigh_path = paths.find(rayleigh_file_name);
        LOG("  Reading %s\n", rayleigh_path.c_str());
        const Spectrum r = read_spectrum(rayleigh_path, icol, false);
        if (r.nwav != nwav || r.wavenumber_cm_1 != first.wavenumber_cm_1)
          fail(ECCKD_PARAMETER_ERROR, "%s: %zu wavenumbers that are not the %zu of the merged spectrum", rayleigh_path.c_str(), r.nwav, nwav);
        if (r.nlay != nlay) fail(ECCKD_PARAMETER_ERROR, "%s has %d levels, the merged spectrum %d", rayleigh_path.c_str(), r.nlay, nlay);
        if (r.ncol != ncol) fail(ECCKD_PARAMETER_ERROR, "%s has %d columns, the input %d", rayleigh_path.c_str(), r.ncol, ncol);
      }
    };
    // The header of an output and its coordinate variables; `scenario`: the line of the table the file belongs to
    auto define_file = [&](NcOut& file, const Spectrum& first, size_t ngas, std::string molecules, const std::string* scenario) {
      const int nlay = first.nlay, nhl = nlay + 1;
      const size_t nwav = first.nwav;
      std::vector<std::string> hl = {"column", "half_level"};
      if (sw) hl.insert(hl.begin() + 1, "mu0");
      std::vector<std::string> hl_spec = hl;
      hl_spec.push_back(spec_name);
      file.dim("column", 0);                                                                // unlimited (:132)
      if (sw) file.dim("mu0", (size_t)nmu);
      file.dim("level", (size_t)nlay);
      file.dim("half_level", (size_t)nhl);
      file.dim(spec_name, have_gpoints ? (size_t)ng : nwav);
      file.dim("gas", ngas);
      if (sw) file.var("mu0", NC_FLOAT_T, {"mu0"}, "Cosine of solar zenith angle", "1");
      file.var("pressure_hl", NC_FLOAT_T, {"column", "half_level"}, "Pressure at half levels", "Pa");
      if (have_temperature) file.var("temperature_hl", NC_FLOAT_T, {"column", "half_level"}, "Temperature at half levels", "K");
      if (!have_gpoints) {
        file.var("wavenumber", NC_DOUBLE_T, {"wavenumber"});
        file.deflate("wavenumber");
        file.att("Wavenumber", "long_name", "wavenumber");
        file.att("cm-1", "units", "wavenumber");
      } else if (sw) {
        file.var("solar_irradiance", NC_FLOAT_T, {"g_point"}, "Solar irradiance across each g point", "W m-2");
      }
      file.var("vmr_fl", NC_FLOAT_T, {"column", "gas", "level"}, "Volume mixing ratio", "mol mol-1");
      file.att("The gases are listed in the global attribute \"molecules\".", "comment", "vmr_fl");
      if (sw) {
        file.var(bb_dn_name, NC_FLOAT_T, hl, "Downwelling direct shortwave flux", "W m-2");
        file.var(bb_up_name, NC_FLOAT_T, hl, "Upwelling shortwave flux", "W m-2");
        if (rayleigh) file.var("flux_dn_sw", NC_FLOAT_T, hl, "Downwelling shortwave flux", "W m-2");
      } else {
        file.var(bb_dn_name, NC_FLOAT_T, hl, "Upwelling longwave flux", "W m-2");   // (sic, :169)
        file.var(bb_up_name, NC_FLOAT_T, hl, "Upwelling longwave flux", "W m-2");
      }
      file.var("optical_depth", NC_FLOAT_T, {"column", "level", spec_name});
      if (!have_gpoints) file.deflate("optical_depth");
      file.att("Layer optical depth", "long_name", "optical_depth");
      if (rayleigh && have_gpoints)
        file.var("rayleigh_optical_depth", NC_FLOAT_T, {"column", "level", spec_name}, "Layer optical depth due to Rayleigh scattering");
      if (sw) {
        file.var(spec_dn_name, NC_FLOAT_T, hl_spec,
                 have_gpoints ? "Downwelling direct shortwave flux per g point" : "Downwelling direct shortwave spectral flux", "W m-2");
        file.var(spec_up_name, NC_FLOAT_T, hl_spec, have_gpoints ? "Upwelling shortwave flux per g point" : "Upwelling shortwave spectral flux",
                 "W m-2");
        if (rayleigh)
          file.var("spectral_flux_dn_sw", NC_FLOAT_T, hl_spec,
                   have_gpoints ? "Downwelling shortwave flux per g point" : "Downwelling shortwave spectral flux", "W m-2");
      } else {
        file.var(spec_dn_name, NC_FLOAT_T, hl_spec, "Downwelling longwave spectral flux", "W m-2");
        file.var(spec_up_name, NC_FLOAT_T, hl_spec, "Upwelling longwave spectral flux", "W m-2");
      }
      if (scenario) file.att(*scenario, "scenario");
      file.att(history_line(argc, argv), "history");
      std::replace(molecules.begin(), molecules.end(), ',', ' ');                           // :193
      file.att(molecules, "molecules");
      file.att(config.str(), "config");
      if (rayleigh) file.att("two-stream", "rayleigh_scattering");
      if (nangle > 0) file.att_int(nangle, "nangle");
      file.end_define();
      if (sw) file.write("mu0", mu0);
      if (!have_gpoints) file.write("wavenumber", first.wavenumber_cm_1);
    };
    // What every column and scenario shares on the device
    auto share_on_device = [&](const Spectrum& first) {
      const int nhl = first.nlay + 1;
      const size_t nwav = first.nwav;
      if (sw) {
        d_ssi.upload(dev, ssi);
        d_albedo.upload(dev, std::vector<double>(nwav, surface_albedo));
      }
      if (!sw || have_gpoints) {
        d_wn.upload(dev, first.wavenumber_cm_1);
        d_dwn.upload(dev, first.d_wavenumber_cm_1);
      }
      if (have_gpoints) {
        d_g.upload(dev, g_point);
        ck(ecckd_gmap_create(dev.ctx(), nwav, d_g.as<int32_t>(), ng, d_wn.as<double>(), d_dwn.as<double>(), &gmap));
        if (sw) {
          solar.resize((size_t)ng);
          ck(ecckd_gmap_sum_rows(gmap, 1, d_ssi.ptr(), ECCKD_F64, nwav, solar.data()));
        }
      } else {
        d_spec_dn.alloc(dev, (size_t)nhl * nwav * sizeof(float));
        d_spec_up.alloc(dev, (size_t)nhl * nwav * sizeof(float));
        if (rayleigh) d_spec_tot.alloc(dev, (size_t)nhl * nwav * sizeof(float));
      }
    };
    // This column of the spectrum that scatters, unscaled, as it is stored
    auto read_rayleigh = [&](int nlay, size_t nwav) {
      DevOd ray;
      if (rayleigh) {
        ray = read_od_dev(dev, NcIn(rayleigh_path), icol, nlay, nwav);
        ck(ecckd_synchronize(dev.ctx()));
      }
      return ray;
    };
    // Record `irec` of a file: the profiles, and the fluxes and optical depths of the merged matrix d_od
    auto write_record = [&](NcOut& file, const Spectrum& first, const std::vector<std::vector<double>>& vmr_fl, const void* d_od, int od_type,
                            const DevOd& ray) {
      const int nlay = first.nlay, nhl = nlay + 1;
      const size_t nwav = first.nwav;
      file.write_slice("pressure_hl", irec, first.pressure_hl);
      if (have_temperature) file.write_slice("temperature_hl", irec, first.temperature_hl);
      std::vector<double> vmr;
      for (const std::vector<double>& row : vmr_fl) vmr.insert(vmr.end(), row.begin(), row.end());
      file.write_slice("vmr_fl", irec, vmr);

      if (sw) LOG("  Performing shortwave radiative transfer for %d solar zenith angles\n", nmu);
      else LOG("  Computing Planck function and performing longwave radiative transfer\n");
      std::vector<double> bb_dn((size_t)nmu * nhl), bb_up((size_t)nmu * nhl), bb_tot(rayleigh ? (size_t)nmu * nhl : 0);
      const std::vector<double>& p = first.pressure_hl;
      const std::vector<double>& t = first.temperature_hl;
      if (!have_gpoints && rayleigh) {
        for (int s = 0; s < nmu; ++s) {                           // one angle at a time, as without scattering
          ck(ecckd_lbl_spectral_fluxes_sw_rayleigh(dev.ctx(), nlay, nwav, 1, &mu0[s], d_ssi.as<double>(), d_albedo.as<double>(), d_od,
                                                   od_type, nwav, ray.buf.ptr(), ray.type, nwav, d_spec_dn.as<float>(),
                                                   d_spec_tot.as<float>(), d_spec_up.as<float>(), nwav, &bb_dn[(size_t)s * nhl],
                                                   &bb_tot[(size_t)s * nhl], &bb_up[(size_t)s * nhl]));
          file.write_subslice(spec_dn_name, irec, (size_t)s, download_as_double(d_spec_dn));
          file.write_subslice(spec_up_name, irec, (size_t)s, download_as_double(d_spec_up));
          file.write_subslice("spectral_flux_dn_sw", irec, (size_t)s, download_as_double(d_spec_tot));
        }
        file.write_slice(bb_dn_name, irec, bb_dn);
        file.write_slice(bb_up_name, irec, bb_up);
        file.write_slice("flux_dn_sw", irec, bb_tot);
        file.write_slice("optical_depth", irec, download_od(dev, d_od, od_type, (size_t)nlay * nwav));
      } else if (!have_gpoints && sw) {
        for (int s = 0; s < nmu; ++s) {                           // one angle at a time, on the device and on the host
          ck(ecckd_lbl_spectral_fluxes_sw(dev.ctx(), nlay, nwav, 1, &mu0[s], d_ssi.as<double>(), d_albedo.as<double>(), d_od,
                                          od_type, nwav, d_spec_dn.as<float>(), d_spec_up.as<float>(), nwav, &bb_dn[(size_t)s * nhl],
                                          &bb_up[(size_t)s * nhl]));
          file.write_subslice(spec_dn_name, irec, (size_t)s, download_as_double(d_spec_dn));
          file.write_subslice(spec_up_name, irec, (size_t)s, download_as_double(d_spec_up));
        }
        file.write_slice(bb_dn_name, irec, bb_dn);
        file.write_slice(bb_up_name, irec, bb_up);
        file.write_slice("optical_depth", irec, download_od(dev, d_od, od_type, (size_t)nlay * nwav));
      } else if (!have_gpoints) {
        ck(ecckd_lbl_spectral_fluxes_lw_angles(dev.ctx(), nangle, nlay, nwav, t.data(), d_wn.as<double>(), d_dwn.as<double>(), d_od,
                                               od_type, nwav, d_spec_dn.as<float>(), d_spec_up.as<float>(), nwav, bb_dn.data(),
                                               bb_up.data()));
        file.write_slice(bb_dn_name, irec, bb_dn);                                            // :231-232
        file.write_slice(bb_up_name, irec, bb_up);
        file.write_slice("optical_depth", irec, download_od(dev, d_od, od_type, (size_t)nlay * nwav));
        file.write_slice(spec_dn_name, irec, download_as_double(d_spec_dn));
        file.write_slice(spec_up_name, irec, download_as_double(d_spec_up));
      } else {
        std::vector<double> dn((size_t)nmu * nhl * ng), up((size_t)nmu * nhl * ng), od_g((size_t)nlay * ng), t_fl;
        std::vector<double> tot(rayleigh ? dn.size() : 0);
        if (rayleigh) {
          ck(ecckd_lbl_gpoint_fluxes_sw_rayleigh(gmap, nlay, nmu, mu0.data(), d_ssi.as<double>(), d_albedo.as<double>(), d_od, od_type,
                                                 nwav, ray.buf.ptr(), ray.type, nwav, dn.data(), tot.data(), up.data(), bb_dn.data(),
                                                 bb_tot.data(), bb_up.data()));
        } else if (sw) {
          ck(ecckd_lbl_gpoint_fluxes_sw(gmap, nlay, nmu, mu0.data(), d_ssi.as<double>(), d_albedo.as<double>(), d_od, od_type,
                                        nwav, dn.data(), up.data(), bb_dn.data(), bb_up.data()));
        } else {
          ck(ecckd_lbl_gpoint_fluxes_lw_angles(gmap, nangle, nlay, t.data(), d_od, od_type, nwav, dn.data(), up.data(),
                                               bb_dn.data(), bb_up.data()));
          t_fl.resize(nlay);          // the Planck weight at the pressure-weighted full-level temperature (:242-251)
          for (int l = 0; l < nlay; ++l) {
            const double p_fl = 0.5 * (p[l] + p[l + 1]);
            t_fl[l] = 0.5 * (t[l] * p[l] + t[l + 1] * p[l + 1]) / p_fl;
          }
        }
        file.write_slice(bb_dn_name, irec, bb_dn);
        file.write_slice(bb_up_name, irec, bb_up);
        // averaged by transmission: the weight the Planck function at t_fl, or the solar spectral irradiance
        ck(ecckd_average_to_gpoints(gmap, nlay, p.data(), sw ? nullptr : t_fl.data(), sw ? d_ssi.as<double>() : nullptr, d_od, od_type,
                                    nwav, ECCKD_AVG_TRANSMISSION, 0.0, od_g.data(), nullptr, nullptr));
        file.write_slice("optical_depth", irec, od_g);
        file.write_slice(spec_dn_name, irec, dn);
        file.write_slice(spec_up_name, irec, up);
        if (rayleigh) {                       // the Rayleigh spectrum averaged like optical_depth, which stays the absorbers'
          ck(ecckd_average_to_gpoints(gmap, nlay, p.data(), nullptr, d_ssi.as<double>(), ray.buf.ptr(), ray.type, nwav, ECCKD_AVG_TRANSMISSION,
                                      0.0, od_g.data(), nullptr, nullptr));
          file.write_slice("flux_dn_sw", irec, bb_tot);
          file.write_slice("rayleigh_optical_depth", irec, od_g);
          file.write_slice("spectral_flux_dn_sw", irec, tot);
        }
      }
    };

    std::vector<std::string> input_paths;       // of a table run
    DevBuf d_merged;                            // ... and its one DOUBLE matrix, which every scenario of every column fills again
    if (have_scenarios) for (const std::string& f : inputs) input_paths.push_back(paths.find(f));
    while (icol < ncol) {
      LOG("Profile %d\n", icol);
      if (!have_scenarios) {
        NcOut& file = *files[0];
        Merged m = read_merged_spectrum(dev, config, paths, icol, "");
        ncol = m.first.ncol;
        if (is_first_profile) {
          is_first_profile = false;
          check_first_column(m.first);
          define_file(file, m.first, m.vmr_fl.size(), m.molecules, nullptr);
          share_on_device(m.first);
          if (have_gpoints && sw) file.write("solar_irradiance", solar);
        }
        const DevOd ray = read_rayleigh(m.first.nlay, m.first.nwav);
        write_record(file, m.first, m.vmr_fl, m.od_ptr(), m.od_type(), ray);
      } else {
        const ColumnGases c = read_column_gases(dev, input_paths, icol);      // the one read of this column
        ncol = c.first.ncol;
        const int nlay = c.first.nlay, ngas = (int)c.od.size();
        const size_t nwav = c.first.nwav;
        if (is_first_profile) {
          is_first_profile = false;
          check_first_column(c.first);
          for (size_t k = 0; k < table.size(); ++k) define_file(*files[k], c.first, (size_t)ngas, c.molecules, &table[k].name);
          share_on_device(c.first);
          if (have_gpoints && sw) for (auto& file : files) file->write("solar_irradiance", solar);
        }
        const DevOd ray = read_rayleigh(nlay, nwav);
        std::vector<const void*> od_ptr;
        std::vector<int> od_type;
        std::vector<size_t> od_stride((size_t)ngas, nwav);
        for (const DevOd& od : c.od) { od_ptr.push_back(od.buf.ptr()); od_type.push_back(od.type); }
        for (size_t k = 0; k < table.size(); ++k) {
          LOG("  Scenario %s\n", table[k].name.c_str());
          std::vector<double> scale((size_t)ngas * nlay);
          std::vector<std::vector<double>> vmr_fl((size_t)ngas, std::vector<double>(nlay));
          bool unscaled = true;
          for (int g = 0; g < ngas; ++g) {
            const GasArg& a = table[k].specs[g];
            ck(ecckd_merge_scaling(nlay, c.first.pressure_hl.data(), a.mode == GasArg::SCALE ? a.value : -1.0,
                                   a.mode == GasArg::CONC ? a.value : -1.0, c.reference_surface_vmr[g], c.vmr_fl[g].data(), 0, nullptr, nullptr,
                                   &scale[(size_t)g * nlay], vmr_fl[g].data()));
            bool one = true;
            for (int l = 0; l < nlay; ++l) one = one && scale[(size_t)g * nlay + l] == 1.0;
            if (!one) LOG("    Scaling %s by %g\n", inputs[g].c_str(), scale[(size_t)g * nlay]);
            unscaled = unscaled && one;
          }
          if (ngas == 1 && unscaled) {          // a single unscaled input is taken as stored (Merged::is_single)
            write_record(*files[k], c.first, vmr_fl, od_ptr[0], od_type[0], ray);
            continue;
          }
          if (d_merged.empty()) d_merged.alloc(dev, (size_t)nlay * nwav * sizeof(double));
          ck(ecckd_merge_scenario_dev(dev.ctx(), nlay, nwav, ngas, od_ptr.data(), od_type.data(), od_stride.data(), scale.data(),
                                      d_merged.as<double>(), nwav));
          write_record(*files[k], c.first, vmr_fl, d_merged.ptr(), ECCKD_F64, ray);
        }
      }
      if (do_one_profile) break;
      ++icol;
      ++irec;
    }
    if (gmap) ecckd_gmap_destroy(gmap);
    for (auto& file : files) file->close();
    return 0;
  });
}
