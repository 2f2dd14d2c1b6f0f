// lw_spectra [key=value ...] [file.cfg]
//
// Drop-in for the reference executable of the same name (src/ecckd/lw_spectra.cpp:31-275): line-by-line longwave fluxes of
// every column (or of column `iprofile`) of a merged spectrum - the Planck function and the no-scattering radiative transfer
// with unit surface emissivity - written per wavenumber or, with `gpoints`, summed over the wavenumbers of each g point,
// together with the optical depth (per wavenumber, or averaged to the g points by transmission).
// Keys: output (mandatory), input / scaling / conc / conc_input as read_merged_spectrum reads them, gpoints, iprofile,
// log_level, prepend_path, append_path.  `column` is the unlimited dimension (:132), in classic and in NetCDF-4 (*.h5) files.
// The fluxes come from ecckd_lbl_gpoint_fluxes_lw / ecckd_lbl_spectral_fluxes_lw, the g-point optical depths from
// ecckd_average_to_gpoints (include/ecckd_hip.h).
#include <algorithm>
#include <memory>

#include "tool.hpp"

using namespace tool;

int main(int argc, char** argv) {
  return run(argc, argv, [&](Config& config) -> int {
    std::string output;
    if (!config.read(output, "output")) fail(ECCKD_PARAMETER_ERROR, "\"output\" file not specified");
    SearchPath paths;
    paths.configure(config);
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
    int iprofile = -1;
    const bool do_one_profile = config.read(iprofile, "iprofile");
    int icol = do_one_profile ? iprofile : 0;
    int ncol = 10000;
    size_t irec = 0;

    NcOut file(output);
    ecckd_gmap* gmap = nullptr;
    DevBuf d_wn, d_dwn, d_g, d_spec_dn, d_spec_up;
    const std::string spec_name = have_gpoints ? "g_point" : "wavenumber";
    bool is_first_profile = true;
    while (icol < ncol) {
      LOG("Profile %d\n", icol);
      Merged m = read_merged_spectrum(dev, config, paths, icol, "");
      ncol = m.first.ncol;
      const int nlay = m.first.nlay;
      const size_t nwav = m.first.nwav;
      if (is_first_profile) {
        is_first_profile = false;
        if (have_gpoints && g_point.size() != nwav)
          fail(ECCKD_PARAMETER_ERROR, "g_point has %zu elements, the spectrum %zu wavenumbers", g_point.size(), nwav);
        file.dim("column", 0);                                                                // unlimited (:132)
        file.dim("level", (size_t)nlay);
        file.dim("half_level", (size_t)nlay + 1);
        file.dim(spec_name, have_gpoints ? (size_t)ng : nwav);
        file.dim("gas", m.vmr_fl.size());
        file.var("pressure_hl", NC_FLOAT_T, {"column", "half_level"}, "Pressure at half levels", "Pa");
        file.var("temperature_hl", NC_FLOAT_T, {"column", "half_level"}, "Temperature at half levels", "K");
        if (!have_gpoints) {
          file.var("wavenumber", NC_DOUBLE_T, {"wavenumber"});
          file.deflate("wavenumber");
          file.att("Wavenumber", "long_name", "wavenumber");
          file.att("cm-1", "units", "wavenumber");
        }
        file.var("vmr_fl", NC_FLOAT_T, {"column", "gas", "level"}, "Volume mixing ratio", "mol mol-1");
        file.att("The gases are listed in the global attribute \"molecules\".", "comment", "vmr_fl");
        file.var("flux_dn_lw", NC_FLOAT_T, {"column", "half_level"}, "Upwelling longwave flux", "W m-2");   // (sic, :169)
        file.var("flux_up_lw", NC_FLOAT_T, {"column", "half_level"}, "Upwelling longwave flux", "W m-2");
        file.var("optical_depth", NC_FLOAT_T, {"column", "level", spec_name});
        if (!have_gpoints) file.deflate("optical_depth");
        file.att("Layer optical depth", "long_name", "optical_depth");
        file.var("spectral_flux_dn_lw", NC_FLOAT_T, {"column", "half_level", spec_name}, "Downwelling longwave spectral flux", "W m-2");
        file.var("spectral_flux_up_lw", NC_FLOAT_T, {"column", "half_level", spec_name}, "Upwelling longwave spectral flux", "W m-2");
        file.att(history_line(argc, argv), "history");
        std::string molecules = m.molecules;
        std::replace(molecules.begin(), molecules.end(), ',', ' ');                           // :193
        file.att(molecules, "molecules");
        file.att(config.str(), "config");
        file.end_define();
        if (!have_gpoints) file.write("wavenumber", m.first.wavenumber_cm_1);
        d_wn.upload(dev, m.first.wavenumber_cm_1);
        d_dwn.upload(dev, m.first.d_wavenumber_cm_1);
        if (have_gpoints) {
          d_g.upload(dev, g_point);
          ck(ecckd_gmap_create(dev.ctx(), nwav, d_g.as<int32_t>(), ng, d_wn.as<double>(), d_dwn.as<double>(), &gmap));
        } else {
          d_spec_dn.alloc(dev, (size_t)(nlay + 1) * nwav * sizeof(float));
          d_spec_up.alloc(dev, (size_t)(nlay + 1) * nwav * sizeof(float));
        }
      }
      file.write_slice("pressure_hl", irec, m.first.pressure_hl);
      file.write_slice("temperature_hl", irec, m.first.temperature_hl);
      std::vector<double> vmr;
      for (const std::vector<double>& row : m.vmr_fl) vmr.insert(vmr.end(), row.begin(), row.end());
      file.write_slice("vmr_fl", irec, vmr);

      LOG("  Computing Planck function and performing longwave radiative transfer\n");
      std::vector<double> bb_dn(nlay + 1), bb_up(nlay + 1);
      if (!have_gpoints) {
        ck(ecckd_lbl_spectral_fluxes_lw(dev.ctx(), nlay, nwav, m.first.temperature_hl.data(), d_wn.as<double>(), d_dwn.as<double>(),
                                        m.od_ptr(), m.od_type(), nwav, d_spec_dn.as<float>(), d_spec_up.as<float>(), nwav,
                                        bb_dn.data(), bb_up.data()));
        file.write_slice("flux_dn_lw", irec, bb_dn);                                          // :231-232
        file.write_slice("flux_up_lw", irec, bb_up);
        std::vector<double> od((size_t)nlay * nwav);
        if (m.od_type() == ECCKD_F32) {
          const std::vector<float> f = m.single.buf.download<float>();
          std::copy(f.begin(), f.end(), od.begin());
        } else {
          ck(ecckd_d2h(dev.ctx(), od.data(), m.od_ptr(), od.size() * sizeof(double)));
        }
        file.write_slice("optical_depth", irec, od);
        for (int up = 0; up < 2; ++up) {
          const std::vector<float> f = (up ? d_spec_up : d_spec_dn).download<float>();
          const std::vector<double> d(f.begin(), f.end());
          file.write_slice(up ? "spectral_flux_up_lw" : "spectral_flux_dn_lw", irec, d);
        }
      } else {
        std::vector<double> dn((size_t)(nlay + 1) * ng), up((size_t)(nlay + 1) * ng), od_g((size_t)nlay * ng);
        ck(ecckd_lbl_gpoint_fluxes_lw(gmap, nlay, m.first.temperature_hl.data(), m.od_ptr(), m.od_type(), nwav, dn.data(), up.data(),
                                      bb_dn.data(), bb_up.data()));
        file.write_slice("flux_dn_lw", irec, bb_dn);
        file.write_slice("flux_up_lw", irec, bb_up);
        // the Planck weight at the pressure-weighted full-level temperature (:242-251)
        const std::vector<double>& p = m.first.pressure_hl;
        const std::vector<double>& t = m.first.temperature_hl;
        std::vector<double> t_fl(nlay);
        for (int l = 0; l < nlay; ++l) {
          const double p_fl = 0.5 * (p[l] + p[l + 1]);
          t_fl[l] = 0.5 * (t[l] * p[l] + t[l + 1] * p[l + 1]) / p_fl;
        }
        ck(ecckd_average_to_gpoints(gmap, nlay, p.data(), t_fl.data(), nullptr, m.od_ptr(), m.od_type(), nwav, ECCKD_AVG_TRANSMISSION,
                                    0.0, od_g.data(), nullptr, nullptr));
        file.write_slice("optical_depth", irec, od_g);
        file.write_slice("spectral_flux_dn_lw", irec, dn);
        file.write_slice("spectral_flux_up_lw", irec, up);
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
