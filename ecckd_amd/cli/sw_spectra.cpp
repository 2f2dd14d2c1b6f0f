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
// rayleigh=FILE: a spectrum file like any gas file whose optical_depth SCATTERS, read column by column beside the merged
// absorbers, unscaled (as ckdmip_sw --rayleigh reads it); its wavenumbers and levels must be the merged spectrum's and it must
// have as many columns as `input`, otherwise the tool fails with a parameter error.  The fluxes are then those of the
// two-stream transfer (ecckd_lbl_gpoint_fluxes_sw_rayleigh / ecckd_lbl_spectral_fluxes_sw_rayleigh): the file holds in
// addition flux_dn_sw and spectral_flux_dn_sw (direct plus diffuse), its upwelling fluxes hold the backscatter, the global
// attribute rayleigh_scattering = "two-stream" is set and, with `gpoints`, rayleigh_optical_depth(column, level, g_point) is
// that spectrum averaged like optical_depth, which stays the absorbers' average: the file then holds the flux variables of a
// ckdmip_sw --ckd --rayleigh-scattering output (ckdmip.hpp: define_ckd_output) and the two optical depths run_ckd writes, so a
// CKD model is compared with it variable by variable.  Without `gpoints` device memory is 3 (nlay+1) nwav floats.  Without
// the key the file is byte for byte what it was.
// scenarios=TABLE in place of output / scaling / conc / conc_input: many scenarios from one read of the spectra, one output file
// per line of TABLE (spectra.hpp says how); the spectrum of rayleigh= is read once per column and never scaled.
#include "spectra.hpp"

int main(int argc, char** argv) { return spectra_main(argc, argv, true); }
