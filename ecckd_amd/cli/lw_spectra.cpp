// lw_spectra [key=value ...] [file.cfg]
//
// Drop-in for the reference executable of the same name (src/ecckd/lw_spectra.cpp:31-275): line-by-line longwave fluxes of
// every column (or of column `iprofile`) of a merged spectrum - the Planck function and the no-scattering radiative transfer
// with unit surface emissivity - written per wavenumber or, with `gpoints`, summed over the wavenumbers of each g point,
// together with the optical depth (per wavenumber, or averaged to the g points by transmission).
// Keys: output (mandatory), input / scaling / conc / conc_input as read_merged_spectrum reads them, gpoints, iprofile,
// log_level, prepend_path, append_path.  `column` is the unlimited dimension (:132), in classic and in NetCDF-4 (*.h5) files.
// Not in the reference: nangle=N (0..16, default 0), the CKDMIP tool's key (test/run_ckd_lw.sh:28).  0 is the reference's
// two-stream form (diffusivity 1.66); N > 0 integrates N Gauss-Legendre zenith angles per hemisphere, in both output modes, and
// the file then carries the global attribute `nangle`; the other variables do not depend on the key.
// Also not in the reference: scenarios=TABLE in place of output / scaling / conc / conc_input - many scenarios from one read of the
// spectra, one output file per line of TABLE (spectra.hpp says how).
// The fluxes come from ecckd_lbl_gpoint_fluxes_lw_angles / ecckd_lbl_spectral_fluxes_lw_angles, the g-point optical depths
// from ecckd_average_to_gpoints (include/ecckd_hip.h).
#include "spectra.hpp"

int main(int argc, char** argv) { return spectra_main(argc, argv, false); }
