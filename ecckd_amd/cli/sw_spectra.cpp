// sw_spectra [key=value ...] [file.cfg]
//
// The shortwave counterpart of lw_spectra (the reference has none): line-by-line shortwave fluxes of every column (or of
// column `iprofile`) of a merged spectrum - the direct beam and its reflection at a Lambertian surface without scattering in
// the atmosphere (radiative_transfer_sw.cpp:26-77) - for every cos_solar_zenith_angle, written per wavenumber or, with
// `gpoints`, summed over the wavenumbers of each g point, together with the optical depth (per wavenumber, or averaged to the
// g points by transmission with the solar spectral irradiance as the weight).
// Keys: output (mandatory), ssi (mandatory: a file with solar_spectral_irradiance(wavenumber), as reorder_spectrum and
// find_g_points read it), input / scaling / conc / conc_input as read_merged_spectrum reads them, gpoints, iprofile,
// cos_solar_zenith_angle (1..8 numbers, default 0.5: calc_cost_function_sw.h:20), surface_albedo (default 0.15, the value
// find_g_points uses below max_no_rayleigh_wavenumber), log_level, prepend_path, append_path.
// `column` is the unlimited dimension, in classic and in NetCDF-4 (*.h5) files; names and attributes of the flux variables are
// those of the ckdmip_sw stand-in's --ckd output (ckdmip.hpp:165-172).  The fluxes come from ecckd_lbl_gpoint_fluxes_sw (all
// angles in one call) / ecckd_lbl_spectral_fluxes_sw (one angle per call, written to the file angle by angle: device memory
// stays at 2 (nlay+1) nwav floats, host memory at one angle's rows), the g-point optical depths from
// ecckd_average_to_gpoints (include/ecckd_hip.h).
#include <algorithm>
#include <memory>

#include "tool.hpp"

using namespace tool;

int main(int argc, char** argv) {
  return run(argc, argv, [&](Config& config) -> int {
    std::string output, ssi_file_name;
    if (!config.read(output, "output")) fail(ECCKD_PARAMETER_ERROR, "\"output\" file not specified");
    if (!config.read(ssi_file_name, "ssi")) fail(ECCKD_PARAMETER_ERROR, "\"ssi\" file not specified");
    std::vector<double> mu0;
    if (!config.read(mu0, "cos_solar_zenith_angle")) mu0 = {0.5};
    if (mu0.empty() || mu0.size() > 8) fail(ECCKD_PARAMETER_ERROR, "cos_solar_zenith_angle must list 1 to 8 numbers");
    for (double m : mu0)
      if (!(m > 0.0 && m <= 1.0)) fail(ECCKD_PARAMETER_ERROR, "cos_solar_zenith_angle %g is not in (0, 1]", m);
    double surface_albedo = 0.15;
    config.read(surface_albedo, "surface_albedo");
    const int nmu = (int)mu0.size();
    SearchPath paths;
    paths.configure(config);
    Device dev;

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
    LOG("Reading %s\n", ssi_file_name.c_str());
    const std::vector<double> ssi = NcIn(paths.find(ssi_file_name)).read("solar_spectral_irradiance");
    int iprofile = -1;
    const bool do_one_profile = config.read(iprofile, "iprofile");
    int icol = do_one_profile ? iprofile : 0;
    int ncol = 10000;
    size_t irec = 0;

    NcOut file(output);
    ecckd_gmap* gmap = nullptr;
    DevBuf d_wn, d_dwn, d_g, d_ssi, d_albedo, d_spec_dn, d_spec_up;
    const std::string spec_name = have_gpoints ? "g_point" : "wavenumber";
    bool is_first_profile = true, have_temperature = false;
    while (icol < ncol) {
      LOG("Profile %d\n", icol);
      Merged m = read_merged_spectrum(dev, config, paths, icol, "");
      ncol = m.first.ncol;
      const int nlay = m.first.nlay;
      const int nhl = nlay + 1;
      const size_t nwav = m.first.nwav;
      if (is_first_profile) {
        is_first_profile = false;
        if (have_gpoints && g_point.size() != nwav)
          fail(ECCKD_PARAMETER_ERROR, "g_point has %zu elements, the spectrum %zu wavenumbers", g_point.size(), nwav);
        if (ssi.size() != nwav)
          fail(ECCKD_PARAMETER_ERROR, "solar_spectral_irradiance has %zu points, the spectrum %zu", ssi.size(), nwav);
        have_temperature = !m.first.temperature_hl.empty();
        file.dim("column", 0);                                                                // unlimited
        file.dim("mu0", (size_t)nmu);
        file.dim("level", (size_t)nlay);
        file.dim("half_level", (size_t)nhl);
        file.dim(spec_name, have_gpoints ? (size_t)ng : nwav);
        file.dim("gas", m.vmr_fl.size());
        file.var("mu0", NC_FLOAT_T, {"mu0"}, "Cosine of solar zenith angle", "1");
        file.var("pressure_hl", NC_FLOAT_T, {"column", "half_level"}, "Pressure at half levels", "Pa");
        if (have_temperature) file.var("temperature_hl", NC_FLOAT_T, {"column", "half_level"}, "Temperature at half levels", "K");
        if (!have_gpoints) {
          file.var("wavenumber", NC_DOUBLE_T, {"wavenumber"});
          file.deflate("wavenumber");
          file.att("Wavenumber", "long_name", "wavenumber");
          file.att("cm-1", "units", "wavenumber");
        } else {
          file.var("solar_irradiance", NC_FLOAT_T, {"g_point"}, "Solar irradiance across each g point", "W m-2");
        }
        file.var("vmr_fl", NC_FLOAT_T, {"column", "gas", "level"}, "Volume mixing ratio", "mol mol-1");
        file.att("The gases are listed in the global attribute \"molecules\".", "comment", "vmr_fl");
        file.var("flux_dn_direct_sw", NC_FLOAT_T, {"column", "mu0", "half_level"}, "Downwelling direct shortwave flux", "W m-2");
        file.var("flux_up_sw", NC_FLOAT_T, {"column", "mu0", "half_level"}, "Upwelling shortwave flux", "W m-2");
        file.var("optical_depth", NC_FLOAT_T, {"column", "level", spec_name});
        if (!have_gpoints) file.deflate("optical_depth");
        file.att("Layer optical depth", "long_name", "optical_depth");
        file.var("spectral_flux_dn_direct_sw", NC_FLOAT_T, {"column", "mu0", "half_level", spec_name},
                 have_gpoints ? "Downwelling direct shortwave flux per g point" : "Downwelling direct shortwave spectral flux", "W m-2");
        file.var("spectral_flux_up_sw", NC_FLOAT_T, {"column", "mu0", "half_level", spec_name},
                 have_gpoints ? "Upwelling shortwave flux per g point" : "Upwelling shortwave spectral flux", "W m-2");
        file.att(history_line(argc, argv), "history");
        std::string molecules = m.molecules;
        std::replace(molecules.begin(), molecules.end(), ',', ' ');
        file.att(molecules, "molecules");
        file.att(config.str(), "config");
        file.end_define();
        file.write("mu0", mu0);
        if (!have_gpoints) file.write("wavenumber", m.first.wavenumber_cm_1);
        d_ssi.upload(dev, ssi);
        d_albedo.upload(dev, std::vector<double>(nwav, surface_albedo));
        if (have_gpoints) {
          d_wn.upload(dev, m.first.wavenumber_cm_1);
          d_dwn.upload(dev, m.first.d_wavenumber_cm_1);
          d_g.upload(dev, g_point);
          ck(ecckd_gmap_create(dev.ctx(), nwav, d_g.as<int32_t>(), ng, d_wn.as<double>(), d_dwn.as<double>(), &gmap));
          std::vector<double> solar((size_t)ng);
          ck(ecckd_gmap_sum_rows(gmap, 1, d_ssi.ptr(), ECCKD_F64, nwav, solar.data()));
          file.write("solar_irradiance", solar);
        } else {
          d_spec_dn.alloc(dev, (size_t)nhl * nwav * sizeof(float));
          d_spec_up.alloc(dev, (size_t)nhl * nwav * sizeof(float));
        }
      }
      file.write_slice("pressure_hl", irec, m.first.pressure_hl);
      if (have_temperature) file.write_slice("temperature_hl", irec, m.first.temperature_hl);
      std::vector<double> vmr;
      for (const std::vector<double>& row : m.vmr_fl) vmr.insert(vmr.end(), row.begin(), row.end());
      file.write_slice("vmr_fl", irec, vmr);

      LOG("  Performing shortwave radiative transfer for %d solar zenith angles\n", nmu);
      std::vector<double> bb_dn((size_t)nmu * nhl), bb_up((size_t)nmu * nhl);
      if (!have_gpoints) {
        for (int s = 0; s < nmu; ++s) {                           // one angle at a time, on the device and on the host
          ck(ecckd_lbl_spectral_fluxes_sw(dev.ctx(), nlay, nwav, 1, &mu0[s], d_ssi.as<double>(), d_albedo.as<double>(), m.od_ptr(),
                                          m.od_type(), nwav, d_spec_dn.as<float>(), d_spec_up.as<float>(), nwav, &bb_dn[(size_t)s * nhl],
                                          &bb_up[(size_t)s * nhl]));
          for (int up = 0; up < 2; ++up) {
            const std::vector<float> f = (up ? d_spec_up : d_spec_dn).download<float>();
            file.write_subslice(up ? "spectral_flux_up_sw" : "spectral_flux_dn_direct_sw", irec, (size_t)s,
                                std::vector<double>(f.begin(), f.end()));
          }
        }
        file.write_slice("flux_dn_direct_sw", irec, bb_dn);
        file.write_slice("flux_up_sw", irec, bb_up);
        std::vector<double> od((size_t)nlay * nwav);
        if (m.od_type() == ECCKD_F32) {
          const std::vector<float> f = m.single.buf.download<float>();
          std::copy(f.begin(), f.end(), od.begin());
        } else {
          ck(ecckd_d2h(dev.ctx(), od.data(), m.od_ptr(), od.size() * sizeof(double)));
        }
        file.write_slice("optical_depth", irec, od);
      } else {
        std::vector<double> dn((size_t)nmu * nhl * ng), up((size_t)nmu * nhl * ng), od_g((size_t)nlay * ng);
        ck(ecckd_lbl_gpoint_fluxes_sw(gmap, nlay, nmu, mu0.data(), d_ssi.as<double>(), d_albedo.as<double>(), m.od_ptr(), m.od_type(),
                                      nwav, dn.data(), up.data(), bb_dn.data(), bb_up.data()));
        file.write_slice("flux_dn_direct_sw", irec, bb_dn);
        file.write_slice("flux_up_sw", irec, bb_up);
        ck(ecckd_average_to_gpoints(gmap, nlay, m.first.pressure_hl.data(), nullptr, d_ssi.as<double>(), m.od_ptr(), m.od_type(), nwav,
                                    ECCKD_AVG_TRANSMISSION, 0.0, od_g.data(), nullptr, nullptr));
        file.write_slice("optical_depth", irec, od_g);
        file.write_slice("spectral_flux_dn_direct_sw", irec, dn);
        file.write_slice("spectral_flux_up_sw", irec, up);
      }
      if (do_one_profile) break;
      ++icol;
      ++irec;
    }
    if (gmap) ecckd_gmap_destroy(gmap);
    file.close();
    return 0;
  });
}
