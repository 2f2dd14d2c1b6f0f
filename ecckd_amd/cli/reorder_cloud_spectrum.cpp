// reorder_cloud_spectrum [key=value ...] [file.cfg]
//
// Drop-in for the reference executable of the same name (src/ecckd/reorder_cloud_spectrum.cpp:31-201): ranks the wavenumbers
// of every band by the absorptance of an optically thick cloud of one droplet size and writes the reordering file that
// find_g_points reads for its `cloud` pseudo-gas (test/reorder_spectrum_sw.sh writes sw_order_<bands>_cloud.h5 with it).
// Keys: input (Mie scattering file), isize (0-based index of its effective_radius), wavenumber_input (a file with the spectral
// grid, e.g. the CKDMIP solar spectrum), output, wavenumber1, wavenumber2, log_level, prepend_path, append_path.
// The absorptance, its interpolation onto the grid and the per-band stable sort run on the GPU
// (ecckd_cloud_sorting_variable_dev, ecckd_stable_argsort_bands_dev in include/ecckd_hip.h).
#include <algorithm>

#include "tool.hpp"

using namespace tool;

int main(int argc, char** argv) {
  return run(argc, argv, [&](Config& config) -> int {
    std::string input, wavenumber_input, output;
    int isize = 0;
    if (!config.read(input, "input")) fail(ECCKD_PARAMETER_ERROR, "\"input\" file not specified");
    if (!config.read(isize, "isize")) fail(ECCKD_PARAMETER_ERROR, "\"isize\" not specified");
    if (!config.read(wavenumber_input, "wavenumber_input")) fail(ECCKD_PARAMETER_ERROR, "\"wavenumber_input\" file not specified");
    if (!config.read(output, "output")) fail(ECCKD_PARAMETER_ERROR, "\"output\" file not specified");
    SearchPath paths;
    paths.configure(config);

    // ---- the spectral grid (:77-92) ----
    LOG("Reading %s\n", wavenumber_input.c_str());
    std::vector<double> wn;
    {
      NcIn f(paths.find(wavenumber_input));
      wn = f.read("wavenumber");
    }
    const size_t nwav = wn.size();
    if (nwav < 3) fail(ECCKD_PARAMETER_ERROR, "%s holds %zu wavenumbers: at least 3 needed", wavenumber_input.c_str(), nwav);

    // ---- one size bin of the cloud's optical properties (:95-109) ----
    LOG("Reading %s\n", input.c_str());
    std::vector<double> cloud_wn, ssa, asymmetry;
    {
      NcIn f(paths.find(input));
      cloud_wn = f.read("wavenumber");
      const std::vector<size_t> shape = f.shape("single_scattering_albedo");
      if (shape.size() != 2 || shape[1] != cloud_wn.size() || f.shape("asymmetry_factor") != shape)
        fail(ECCKD_PARAMETER_ERROR, "single_scattering_albedo and asymmetry_factor of %s must be [effective_radius][wavenumber]", input.c_str());
      // the reference indexes the matrices without a check (:107-108)
      if (isize < 0 || (size_t)isize >= shape[0])
        fail(ECCKD_PARAMETER_ERROR, "isize = %d is outside the %zu size bins of %s", isize, shape[0], input.c_str());
      ssa = f.read("single_scattering_albedo", isize);
      asymmetry = f.read("asymmetry_factor", isize);
    }

    std::vector<double> band_bound1, band_bound2;
    Device dev;
    DevBuf d_wn, d_dwn(dev, nwav * sizeof(double)), d_key(dev, nwav * sizeof(double)), d_rank(dev, nwav * sizeof(int32_t));
    d_wn.upload(dev, wn);
    ck(ecckd_derive_d_wavenumber_dev(dev.ctx(), nwav, d_wn.as<double>(), d_dwn.as<double>()));   // :86-92
    const std::vector<double> dwn = d_dwn.download<double>();
    if (config.exist("wavenumber1")) {
      config.read(band_bound1, "wavenumber1");
      config.read(band_bound2, "wavenumber2");
    } else {   // :132-137
      band_bound1 = {std::max(0.0, wn.front() - dwn.front())};
      band_bound2 = {wn.back() + dwn.back()};
    }
    const int nband = (int)band_bound1.size();
    if (nband <= 0 || band_bound2.size() != band_bound1.size())
      fail(ECCKD_PARAMETER_ERROR, "Failure to interpret wavenumber1 and wavenumber2 as a list of band boundaries");
    if (nband == 1) LOG("Treating the entire spectrum as one band\n");
    else LOG("Splitting the spectrum into %d bands\n", nband);

    // ---- absorptance in the optically thick limit on the grid (:111-123), per-band stable sort (:150-188) ----
    ck(ecckd_cloud_sorting_variable_dev(dev.ctx(), (int)cloud_wn.size(), cloud_wn.data(), ssa.data(), asymmetry.data(), nwav,
                                        d_wn.as<double>(), d_key.as<double>()));
    std::vector<int16_t> iband(nwav);
    std::vector<int64_t> bb(nband), be(nband);
    ck(ecckd_band_ranges(nwav, wn.data(), nband, band_bound1.data(), band_bound2.data(), iband.data(), bb.data(), be.data()));
    // the file stores the bounds clamped to the range of the data (:156-161), membership used the unclamped ones
    std::vector<double> clamp1 = band_bound1, clamp2 = band_bound2;
    clamp1.front() = std::max(wn.front(), band_bound1.front());
    clamp2.back() = std::min(wn.back(), band_bound2.back());
    for (int b = 0; b < nband; ++b) {
      LOG("  Band %d: %g-%g cm-1\n", b, clamp1[b], clamp2[b]);
      // the reference takes index(0) of an empty set here (:178)
      if (bb[b] > be[b]) fail(ECCKD_PARAMETER_ERROR, "Band %d (%g-%g cm-1) contains no wavenumbers", b, band_bound1[b], band_bound2[b]);
    }
    ck(ecckd_stable_argsort_bands_dev(dev.ctx(), nwav, d_key.as<double>(), nband, bb.data(), be.data(), d_rank.as<int32_t>(), nullptr));
    const std::vector<double> key = d_key.download<double>();
    const std::vector<int32_t> rank = d_rank.download<int32_t>();

    LOG("Writing %s\n", output.c_str());
    const std::string history = history_line(argc, argv);
    ck(ecckd_write_order_file(output.c_str(), "cloud", config.str().c_str(), history.c_str(), nband, clamp1.data(), clamp2.data(),
                              nwav, wn.data(), dwn.data(), iband.data(), rank.data(), nullptr, key.data()));
    return done(0);
  });
}
