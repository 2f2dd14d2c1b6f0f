// merge_spectra [key=value ...] [file.cfg]
//
// Drop-in for the reference executable of the same name (src/ecckd/merge_spectra.cpp:27-170): merges the optical-depth spectra
// of several gases (keys input, scaling, conc, conc_input / iprofile as read_merged_spectrum reads them) column by column and
// writes pressure_hl, temperature_hl, wavenumber and the merged optical_depth (FLOAT, deflated where the file is NetCDF-4).
// Keys: input, output (both mandatory), log_level, prepend_path, append_path.  The merge runs on the GPU
// (ecckd_merge_spectrum_dev in include/ecckd_hip.h).
#include <algorithm>
#include <cctype>
#include <memory>

#include "tool.hpp"

using namespace tool;

int main(int argc, char** argv) {
  return run(argc, argv, [&](Config& config) -> int {
    std::string input, output;
    if (!config.read(input, "input")) fail(ECCKD_PARAMETER_ERROR, "\"input\" file not specified");
    if (!config.read(output, "output")) fail(ECCKD_PARAMETER_ERROR, "\"output\" file not specified");
    SearchPath paths;
    paths.configure(config);
    Device dev;
    std::unique_ptr<NcOut> file;
    int ncol = 1;
    for (int icol = 0; icol < ncol; ++icol) {
      LOG("Merging profile %d\n", icol);
      Merged m = read_merged_spectrum(dev, config, paths, icol, "");
      const int nlay = m.first.nlay;
      const size_t nwav = m.first.nwav;
      if (icol == 0) {
        ncol = m.first.ncol;
        LOG("Writing %s\n", output.c_str());
        file.reset(new NcOut(output));
        file->dim("column", (size_t)ncol);                                                    // :88-91
        file->dim("level", (size_t)nlay);
        file->dim("half_level", (size_t)nlay + 1);
        file->dim("wavenumber", nwav);
        file->var("pressure_hl", NC_FLOAT_T, {"column", "half_level"}, "Pressure at half levels", "Pa");
        file->var("temperature_hl", NC_FLOAT_T, {"column", "half_level"}, "Temperature at half levels", "K");
        file->var("wavenumber", NC_DOUBLE_T, {"wavenumber"});
        file->deflate("wavenumber");
        file->att("Wavenumber", "long_name", "wavenumber");
        file->att("cm-1", "units", "wavenumber");
        file->var("optical_depth", NC_FLOAT_T, {"column", "level", "wavenumber"});
        file->deflate("optical_depth");
        file->att("Layer optical depth", "long_name", "optical_depth");
        std::string title = "Merged spectral optical depth profiles of ";                    // :115-125
        for (char c : m.molecules) {
          if (c == ',') title += ", ";
          else title += (char)std::toupper((unsigned char)c);
        }
        file->att(title, "title");
        file->att("hybrid:" + m.molecules, "molecule");
        file->att(history_line(argc, argv), "history");
        file->att(config.str(), "config");
        file->end_define();
        file->write("wavenumber", m.first.wavenumber_cm_1);
      }
      file->write_slice("pressure_hl", (size_t)icol, m.first.pressure_hl);
      file->write_slice("temperature_hl", (size_t)icol, m.first.temperature_hl);
      std::vector<double> od((size_t)nlay * nwav);
      if (m.od_type() == ECCKD_F32) {
        const std::vector<float> f = m.single.buf.download<float>();
        std::copy(f.begin(), f.end(), od.begin());
      } else {
        ck(ecckd_d2h(dev.ctx(), od.data(), m.od_ptr(), od.size() * sizeof(double)));
      }
      file->write_slice("optical_depth", (size_t)icol, od);
    }
    file->close();
    return 0;
  });
}
