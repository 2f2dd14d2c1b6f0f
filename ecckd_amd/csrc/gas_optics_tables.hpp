// gas_optics_tables.hpp - the host step of the resident gas-optics handle (gas_optics.hip): the model flattened into what the
// handle uploads once, the refusals of a call, and the launch plan.  Plain C++: nothing here touches the device, so the step can
// be built and run on its own (tools/check_gas_optics_tables.cpp).
#pragma once

#include "../../include/ecckd_hip.h"

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace ecckd {
namespace gas_optics {

constexpr int MAX_GASES = 32;          // per-call gas arguments travel in the kernel arguments
constexpr int CELLS_PER_BLOCK = 64;    // one lane of the first wave per cell of a tile
constexpr int THREADS = 256;
constexpr size_t MAX_LDS_BYTES = 160 * 1024;
// a tile's LDS: per cell nent (coefficient, table row) entries of 8 + 4 bytes and the moles of air
constexpr size_t tile_lds_bytes(int nent) { return (size_t)CELLS_PER_BLOCK * ((size_t)nent * 12 + 8); }

// One gas as the kernel reads it (device array, gases in model order).
struct GasDesc {
  int conc;             // 0 none, 1 linear, 2 look-up table, 3 relative-linear
  int nconc;            // concentration nodes (1 unless conc == 2)
  int ent0;             // first entry of the gas in a cell's entry list
  int nent;             // 4, or 8 for conc == 2
  uint32_t ix;          // offset of the gas's table in the coefficient vector
  uint32_t pad;
  double reference_vmr;
  double log_vmr0;      // conc == 2: log(vmr[0]) and log(vmr[1] / vmr[0]), formed on the host as build_entries forms them
  double d_log_c;
};

// Everything ecckd_gas_optics_create uploads or keeps.
struct Flat {
  int ng = 0, nt = 0, np = 0, ngas = 0, ntp = 0, nent = 0;
  bool is_sw = false, has_rayleigh = false;
  double log_p_0 = 0.0, d_log_p = 0.0, d_t = 0.0;      // ckd_model.cpp:946-950: all the kernel needs of log_pressure
  std::vector<GasDesc> gases;
  std::vector<double> k;                 // all gases' tables, model order
  std::vector<double> temperature;       // [nt][np]
  std::vector<double> temperature_planck, planck_function;   // longwave: [ntp], [ntp][ng]
  std::vector<double> solar_irradiance;  // shortwave: [ng]; stays on the host, only `incoming` reads it
  std::vector<double> rayleigh;          // [ng] or empty
  std::vector<int> iband;                // [ng] g point -> band, or empty: a model without iband_per_g has no band sums
  int nband = 0;                         // 1 + max(iband), 0 without iband_per_g
};

// Validates the model (the model part of the optimiser's check, opt_tables.hpp) and flattens it.  ECCKD_OK, or
// ECCKD_PARAMETER_ERROR with the refusal in `err`.
int flatten_model(const ecckd_opt_model* m, Flat& f, std::string& err);

struct Plan {
  size_t ncell = 0;        // ncol * nlay
  size_t nvalue = 0;       // ncol * nlay * ng: elements of one output array
  unsigned blocks = 0;     // tiles of CELLS_PER_BLOCK consecutive cells
  int threads = THREADS;
  size_t lds_bytes = 0;    // per block: tile_lds_bytes(nent)
};

// The launch as a function of the shape alone.  Refused: non-positive sizes, more tiles than a grid holds, a tile's entry list
// beyond the LDS of a compute unit.
int launch_plan(long long ncol, int nlay, int ng, int nent, Plan& p, std::string& err);

// What a call asks for, as far as the host can judge it.
struct CallArgs {
  int ncol, nlay;
  bool have_pressure, have_temperature_hl, have_vmr, have_od, have_rayleigh_od;
  const int* gas_present;          // [ngas] or NULL
  const double* gas_scaling;       // [ngas] or NULL
  const void* const* gas_od;       // [ngas] device pointers or NULL
  int keep_negative, out_type;
};
// The refusals of ecckd_gas_optics_dev, each with its own message; on ECCKD_OK `present_mask` has bit i set for every gas that
// contributes and `any_gas_od` says whether a per-gas output was asked for.
int check_call(const Flat& f, const CallArgs& a, uint32_t& present_mask, bool& any_gas_od, std::string& err);

// tsi / sum(ssi) * ssi, flatten_scenes' expression; out[ng]
void incoming(const Flat& f, double tsi, double* out);
// the factor of that expression, tsi / sum(ssi): the fused fluxes multiply it with ssi[g] on the device
double incoming_scaling(const Flat& f, double tsi);

// ---- the fused fluxes (gas_optics_fluxes.hip) ----
constexpr int FLUX_LW = 0, FLUX_SW_DIRECT = 1, FLUX_SW_TWOSTREAM = 2;
constexpr unsigned WANT_BROADBAND = 1, WANT_BANDS = 2, WANT_SPECTRAL = 4, WANT_HEATING = 8, WANT_DIRECT = 16;
constexpr int FLUX_BLOCKS_PER_CU = 3;
constexpr int FLUX_TILE_CELLS = 64;        // cells of a layer tile where the columns of a block allow it
constexpr int FLUX_REDUCE_DOUBLES = 2048;  // LDS doubles of one reduction over g
constexpr int FLUX_MAX_ANGLES = 16;
// per-thread state rows of nlay + 1 doubles: longwave tau, Planck, dn, up; direct beam tau, dn, up; two-stream tau_abs,
// tau_ray, direct, dn, up
constexpr int flux_state_rows(int mode) { return mode == FLUX_LW ? 4 : (mode == FLUX_SW_DIRECT ? 3 : 5); }

// The launch of a fused-flux call as a function of the shape alone (ecckd_flux_plan, ecckd_hip.h): a block of THREADS threads
// owns max(1, THREADS / ng) whole columns, with ng > THREADS it loops over g; layers go through LDS in tiles of layer_tile;
// the grid is bounded (FLUX_BLOCKS_PER_CU per compute unit, or grid_override >= 1 blocks) and its blocks loop over the column
// groups, so scratch_bytes depends on the grid, not on ncol.  Refused: non-positive sizes, a mode, nangle or wants outside
// their values, more LDS than a compute unit has.
int fluxes_plan(long long ncol, int nlay, int ng, int nent, int nband, int mode, int nangle, unsigned wants, int cu_count,
                long long grid_override, ecckd_flux_plan& p, std::string& err);

struct FluxCallArgs {
  bool sw_call;                    // ecckd_gas_optics_fluxes_sw_dev
  int nangle, scattering, ncol, nlay;
  bool have_pressure, have_temperature_hl, have_vmr, have_cos_sza;
  const int* gas_present;          // [ngas] or NULL
  int out_type;
  const ecckd_flux_outputs* out;
  bool sky_call = false;           // ecckd_gas_optics_fluxes_{lw,sw}_sky_dev: the refusals carry that entry's name
  const ecckd_flux_sky* sky = nullptr;
};
// The refusals of the two fused-flux calls, each with its own message; on ECCKD_OK the gases that contribute, the mode and
// what the outputs ask for (WANT_*).
int check_fluxes_call(const Flat& f, const FluxCallArgs& a, uint32_t& present_mask, int& mode, unsigned& wants, std::string& err);
// The refusals the sky argument of the *_sky_dev calls adds (after check_fluxes_call); on ECCKD_OK `sky_given` says whether any
// of its pointers is set: without one the call is the clear call and runs the clear kernel.
int check_fluxes_sky(const Flat& f, const FluxCallArgs& a, bool& sky_given, std::string& err);

}  // namespace gas_optics
}  // namespace ecckd
