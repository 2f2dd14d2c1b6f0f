/* ecckd_hip.h - C ABI of libecckd_hip.so, the MI355X (gfx950) implementation of
 * ecCKD's spectral-integration hot path.
 *
 * The reference (ecmwf-ifs/ecckd 1.6) has no plugin/FFI layer: its hot path is a
 * set of C++ free functions and one virtual callback called from the four
 * executables' main().  Each entry point below replaces one of those in-process
 * seams (cited as reference file:line); INTEGRATION.md shows the call a
 * maintainer would substitute at each site.
 *
 * Conventions
 *  - Plain C types only.  All 2-D arrays are row-major (level, wavenumber) with
 *    wavenumber fastest, exactly as the reference's adept::Matrix holds them.
 *  - Pointers named d_* are DEVICE pointers (from ecckd_dev_alloc, hipMalloc or
 *    any allocator on the same device); h_* are host pointers.  Entry points
 *    without a _dev suffix take host pointers and stage through the context's
 *    stream.
 *  - Every function returns 0 on success or one of the reference's exit codes
 *    (src/include/EsaExitCodes.h:16-51): ECCKD_PARAMETER_ERROR (147),
 *    ECCKD_PROCESSING_ERROR (148), ECCKD_OUT_OF_MEMORY (130); HIP failures map
 *    to ECCKD_UNEXPECTED_EXCEPTION (131).  Nothing throws across the boundary.
 *    ecckd_last_error() returns a message for the calling thread.
 *  - A context owns one HIP stream; calls on one context are single-caller
 *    (the reference calls calc_error from OpenMP threads, equipartition.h:100;
 *    here the batch IS the parallelism).  Work is asynchronous on the stream
 *    unless the function returns host-visible results.
 *  - There is no CPU fallback: if no gfx950 device is usable the call fails.
 */
#ifndef ECCKD_HIP_H
#define ECCKD_HIP_H 1

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ECCKD_OK 0
#define ECCKD_OUT_OF_MEMORY 130
#define ECCKD_UNEXPECTED_EXCEPTION 131
#define ECCKD_PARAMETER_ERROR 147
#define ECCKD_PROCESSING_ERROR 148

/* element type of an optical-depth matrix on the device */
#define ECCKD_F32 4 /* FLOAT as stored in the CKDMIP files */
#define ECCKD_F64 8 /* the reference's in-memory Real */

/* averaging methods, find_g_points.cpp:1119-1150 / :54-204 */
#define ECCKD_AVG_LINEAR 0
#define ECCKD_AVG_TRANSMISSION 1
#define ECCKD_AVG_TRANSMISSION_2 2
#define ECCKD_AVG_SQUARE_ROOT 3
#define ECCKD_AVG_LOGARITHMIC 4
#define ECCKD_AVG_TOTAL_TRANSMISSION 5
/* create_look_up_table only, average_optical_depth.cpp:60-126 */
#define ECCKD_AVG_TRANSMISSION_3 6
#define ECCKD_AVG_TRANSMISSION_10 7
#define ECCKD_AVG_HYBRID_LOG_TRANSMISSION_3 8

typedef struct ecckd_ctx ecckd_ctx;

/* ---- context, memory, stream ------------------------------------------------ */
int ecckd_version(void);
const char* ecckd_last_error(void);
int ecckd_init(int device, ecckd_ctx** ctx);
int ecckd_destroy(ecckd_ctx* ctx);
int ecckd_synchronize(ecckd_ctx* ctx);
/* Device buffers released by gas / g-point-map handles are parked in the context and reused for later
 * handles of the same shapes (up to ECCKD_CACHE_GB, default 96); this returns them to the driver. */
int ecckd_trim_cache(ecckd_ctx* ctx);
/* the context's hipStream_t, for callers that record their own events */
void* ecckd_stream(ecckd_ctx* ctx);
int ecckd_dev_alloc(ecckd_ctx* ctx, size_t bytes, void** d_ptr);
int ecckd_dev_free(ecckd_ctx* ctx, void* d_ptr);
/* free and total device memory in bytes as the driver reports them (what another process on the same GPU holds counts as used) */
int ecckd_mem_info(ecckd_ctx* ctx, size_t* free_bytes, size_t* total_bytes);
int ecckd_h2d(ecckd_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int ecckd_d2h(ecckd_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
/* per-kernel timing of the dominant kernels with HIP events on the context's stream:
 * kernel = "k_rt_lw_bb" | "k_reorder_key_lw"; units = wavenumber points processed.
 * Enabling resets the counters.  on = 1: every launch is timed; on = N > 1: every N-th launch of the sweep kernel (the
 * two event records and the event query cost several microseconds per batch of a search: a sample keeps them out of the
 * way); "k_rt_lw_bb.all" then gives the number of launches and points of ALL launches (ms = 0). */
int ecckd_profile_enable(ecckd_ctx* ctx, int on);
int ecckd_profile_get(ecckd_ctx* ctx, const char* kernel, long long* calls, double* ms, double* units);
/* timing on the context's stream (hipEvent pair): begin .. end -> milliseconds */
int ecckd_timer_begin(ecckd_ctx* ctx);
int ecckd_timer_end(ecckd_ctx* ctx, float* ms);

/* ---- reorder_spectrum: sorting key ------------------------------------------
 * Replaces reorder_spectrum.cpp:111-228 (planck_function, radiative_transfer_lw
 * / radiative_transfer_direct_sw, heating_rate, peak-cooling height, thin-column
 * override, threshold height) for one column.
 *   h_pressure_hl[nlay+1], h_temperature_hl[nlay+1] (LW: the idealised profile of
 *   :121-124, see ecckd_idealised_temperature), d_wavenumber/d_d_wavenumber[nwav],
 *   d_od[nlay][od_stride] of type od_type, outputs d_key[nwav], d_col_od[nwav]. */
int ecckd_idealised_temperature(int nhl, const double* h_pressure_hl, double* h_temperature_hl);

int ecckd_reorder_key_lw_dev(ecckd_ctx* ctx, int nlay, size_t nwav,
                             const double* h_pressure_hl, const double* h_temperature_hl,
                             const double* d_wavenumber, const double* d_d_wavenumber,
                             const void* d_od, int od_type, size_t od_stride,
                             double threshold_optical_depth,
                             double* d_key, double* d_col_od);

/* SW (reorder_spectrum.cpp:150-158, :197-228): key = pseudo-height where the
 * optical depth from TOA reaches the threshold.  Returns ECCKD_PROCESSING_ERROR
 * where the reference would `throw;` (key > 30, :214-216). */
int ecckd_reorder_key_sw_dev(ecckd_ctx* ctx, int nlay, size_t nwav,
                             const double* h_pressure_hl,
                             const void* d_od, int od_type, size_t od_stride,
                             double threshold_optical_depth,
                             double* d_key, double* d_col_od);

/* ---- reorder_spectrum: per-band stable sort ----------------------------------
 * Replaces reorder_spectrum.cpp:262-300 (std::stable_sort per band + rank).
 * Bands are index ranges [h_band_begin[b], h_band_end[b]] (inclusive, as
 * index(0)..index(end) at :290-293).  Points outside every band keep
 * ordered_index[j] = rank[j] = j.  Stable; -0.0 == +0.0; NaN keys sort last
 * (undefined behaviour in the reference).  d_ordered_index may be NULL. */
int ecckd_stable_argsort_bands_dev(ecckd_ctx* ctx, size_t nwav, const double* d_key,
                                   int nband, const int64_t* h_band_begin,
                                   const int64_t* h_band_end,
                                   int32_t* d_rank, int32_t* d_ordered_index);

/* Band membership, reorder_spectrum.cpp:277-289: h_iband[nwav] (-1 outside) and
 * the inclusive index range of each band (begin > end if empty).  Host-side. */
int ecckd_band_ranges(size_t nwav, const double* h_wavenumber, int nband,
                      const double* h_band_bound1, const double* h_band_bound2,
                      int16_t* h_iband, int64_t* h_band_begin, int64_t* h_band_end);

/* Host-pointer convenience wrapper of the whole reorder hot path
 * (key + sort), reorder_spectrum.cpp:111-300.  h_ssi == NULL selects LW. */
int ecckd_reorder_spectrum(ecckd_ctx* ctx, int nlay, size_t nwav,
                           const double* h_pressure_hl, const double* h_wavenumber,
                           const double* h_d_wavenumber, const void* h_od, int od_type,
                           const double* h_ssi, double threshold_optical_depth,
                           int nband, const double* h_band_bound1,
                           const double* h_band_bound2,
                           double* h_key, double* h_col_od, int16_t* h_iband,
                           int32_t* h_rank);
/* the same with the optical depths already in device memory (ecckd_nc_read_dev) */
int ecckd_reorder_spectrum_od_dev(ecckd_ctx* ctx, int nlay, size_t nwav,
                           const double* h_pressure_hl, const double* h_wavenumber,
                           const double* h_d_wavenumber, const void* d_od, int od_type,
                           const double* h_ssi, double threshold_optical_depth,
                           int nband, const double* h_band_bound1,
                           const double* h_band_bound2,
                           double* h_key, double* h_col_od, int16_t* h_iband,
                           int32_t* h_rank);

/* ---- find_g_points: gas preparation (K4) -------------------------------------
 * Replaces find_g_points.cpp:872-1150 for one gas: invert the rank from the order
 * file (:779-780), gather-reorder background and target columns (:899, :927-929),
 * Planck function on the reordered wavenumbers (:970-979), LW radiative transfer of
 * background+target (:993-995), heating rate (:1041), surface/TOA flux rows
 * (:1044-1053), layer weights (:1093-1099) and the averaging metric (:1119-1150).
 * All inputs are in ORIGINAL wavenumber order; the handle keeps the results resident
 * on the device in SORTED order.  d_bg_od may be NULL (no background_input:
 * zeros, :902-905).  d_planck_hl_reuse: the planck_hl view of a previously created
 * gas; the reference computes planck_hl only for the first gas and reuses it
 * (:966-983) - pass NULL to compute it for this gas's ordering. */
typedef struct ecckd_gas ecckd_gas;

int ecckd_gas_create_lw(ecckd_ctx* ctx, int nlay, size_t nwav,
                        const double* h_pressure_hl, const double* h_temperature_hl,
                        const double* d_wavenumber, const double* d_d_wavenumber,
                        const int32_t* d_rank,
                        const void* d_bg_od, int bg_type,
                        const void* d_od, int od_type, size_t src_stride,
                        int averaging_method, double flux_weight, double min_pressure,
                        const double* d_planck_hl_reuse, ecckd_gas** gas);

/* The same gas from a background given as the list of spectra it is merged from (read_merged_spectrum.cpp:152-166)
 * instead of the merged matrix: nbg spectra d_bg_od[s] (bg_type[s] ECCKD_F32 or ECCKD_F64, row stride bg_stride[s] >= nwav,
 * ORIGINAL order) with the factors h_bg_scale[nbg][nlay] (ecckd_merge_scaling).  The gas is, array for array and bit for
 * bit, the one ecckd_gas_create_lw returns for the DOUBLE matrix that ecckd_merge_spectrum_dev leaves after nbg calls
 * (= ecckd_merge_scenario_dev): product rounded, then the sum, in the order of the list.  With 54 layers, a FLOAT target
 * and not the logarithmic method the merged matrix is never stored - the spectra are merged as their columns are brought
 * into rank order -; otherwise it is a temporary of the call.  nbg = 0: no background; at most 16 spectra. */
int ecckd_gas_create_lw_merged(ecckd_ctx* ctx, int nlay, size_t nwav,
                               const double* h_pressure_hl, const double* h_temperature_hl,
                               const double* d_wavenumber, const double* d_d_wavenumber,
                               const int32_t* d_rank,
                               int nbg, const void* const* d_bg_od, const int* bg_type,
                               const size_t* bg_stride, const double* h_bg_scale,
                               const void* d_od, int od_type, size_t src_stride,
                               int averaging_method, double flux_weight, double min_pressure,
                               const double* d_planck_hl_reuse, ecckd_gas** gas);

/* The Planck matrix alone, d_planck_hl[nlay+1][nwav] in the order given by d_rank: bit-identical to the "planck_hl" view
 * of a gas created with the same ordering and temperature profile.  The reference evaluates the matrix for the FIRST gas
 * and reuses it for every later one (find_g_points.cpp:529, :970-984); a process that searches only later gases (the
 * (gas, band) tasks are dealt to one process per GPU) builds it from the first gas's ordering file with this call and
 * passes it as d_planck_hl_reuse. */
int ecckd_planck_hl_sorted_dev(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_temperature_hl,
                               const double* d_wavenumber, const double* d_d_wavenumber, const int32_t* d_rank,
                               double* d_planck_hl);
/* Shortwave twin (find_g_points.cpp do_sw branches: radiative_transfer_direct_sw :1003-1006,
 * the two scaled truth fields of the total-transmission method :1008-1034, :1060-1090).
 * d_ssi and d_albedo (NULL = direct beam only) are per-wavenumber arrays in ORIGINAL order;
 * min_scaling/max_scaling are the values after the clamps of :666-667.  The band albedo used
 * by the fitted side (band_albedo(jband), :1169) is set with ecckd_gas_set_band_albedo before
 * evaluating a band. */
int ecckd_gas_create_sw(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_pressure_hl,
                        const double* d_ssi, const double* d_albedo, const int32_t* d_rank,
                        const void* d_bg_od, int bg_type, const void* d_od, int od_type,
                        size_t src_stride, int averaging_method, double flux_weight,
                        double min_pressure, double cos_sza, double min_scaling, double max_scaling,
                        ecckd_gas** gas);
int ecckd_gas_set_band_albedo(ecckd_gas* gas, double surf_albedo);
int ecckd_gas_destroy(ecckd_gas* gas);
/* device view of a resident array: "planck_hl", "bg_optical_depth", "weighted_metric",
 * "hr", "flux_dn_surf", "flux_up_toa", "wavenumber", "d_wavenumber" (LW), "ssi", "hr_low",
 * "hr_high", "flux_extras" (SW); "planck_hl_blocked": the line-blocked copy of planck_hl the 54- / 30-layer
 * longwave sweep reads, [nwav/16][nlay+1][16] as it lies in memory (an error for a gas that holds none) */
int ecckd_gas_view(ecckd_gas* gas, const char* name, const double** d_ptr, size_t* rows, size_t* cols);
int ecckd_gas_layer_weight(ecckd_gas* gas, double* h_layer_weight);
/* total_comp_cost of find_g_points.cpp:320 accumulated by ecckd_calc_error_batch */
double ecckd_gas_comp_cost(ecckd_gas* gas, int reset);

/* ---- find_g_points: batched interval error (K5) ------------------------------
 * Replaces the virtual Equipartition::calc_error (equipartition.h:95) as implemented
 * by CkdEquipartition::calc_error (find_g_points.cpp:291-405) and the loop over it,
 * Equipartition::calc_error_all (equipartition.h:98-116): error[k] for the n
 * intervals [bound1[k], bound2[k]] (fractions of the band) of the band that starts
 * at sorted index ibegin and has npoints points (CkdEquipartition::init_lw, :208-235).
 * Returns ECCKD_PROCESSING_ERROR on the reference's throw(PROCESSING_ERROR) paths
 * (:298-313).  Synchronous. */
int ecckd_calc_error_batch(ecckd_gas* gas, size_t ibegin, size_t npoints, int n,
                           const double* h_bound1, const double* h_bound2, double* h_error);
/* The same with a band per interval: interval k is the fraction [h_bound1[k], h_bound2[k]] of the band that starts at
 * sorted index h_ibegin[k] and has h_npoints[k] points.  One launch train for intervals of several bands.
 * h_band_albedo[k] (shortwave; NULL = the gas's band albedo for all): the surface albedo of interval k's band. */
int ecckd_calc_error_multi(ecckd_gas* gas, int n, const size_t* h_ibegin, const size_t* h_npoints,
                           const double* h_band_albedo, const double* h_bound1, const double* h_bound2,
                           double* h_error);

/* An interval's error depends on the interval alone (its bits are the same in any batch), so the library keeps a memo per
 * gas: an interval the search has asked for before - calc_error_all re-evaluates every interval of a partition of which
 * one bound has moved (equipartition.h:98-116) - is answered from it.  The reference's work counter (ecckd_gas_comp_cost,
 * find_g_points.cpp:320) counts every request all the same.  This call reports what the memo saved: intervals asked for /
 * answered from the memo, wavenumber points asked for / actually swept on the device.  Environment ECCKD_NO_ERROR_MEMO
 * (read per call) switches the memo off. */
int ecckd_gas_eval_stats(ecckd_gas* gas, long long* requests, long long* memo_hits, double* points_requested,
                         double* points_evaluated);
/* Forget the interval errors the gas has answered so far (its memo) and zero the counters above: the next search sweeps
 * every interval again - for timing the same prepared gas twice. */
int ecckd_gas_reset_memo(ecckd_gas* gas);
/* Bytes the error sweep reads per spectral point of an interval it evaluates.  Longwave: (nlay+1) Planck values in DOUBLE
 * plus nlay background optical depths - 4 bytes each when every background value of the gas is exactly a float (a FLOAT
 * spectrum as the CKDMIP files hold it: the gas then keeps them as FLOAT pairs and the sweep widens them, the same bits as
 * reading the DOUBLE rows), 8 bytes otherwise.  Shortwave: nlay background optical depths + the solar irradiance. */
int ecckd_gas_sweep_bytes_per_point(ecckd_gas* gas, double* bytes);

/* The fitted grey optical depth alone: replaces fit_optical_depth_lw / fit_optical_depth_sw /
 * fit_optical_depth_sw_total_trans (find_g_points.cpp:54-106, :112-165, :171-204) for n
 * intervals; h_od_fit[n][nlay]. */
int ecckd_fit_optical_depth(ecckd_gas* gas, size_t ibegin, size_t npoints, int n,
                            const double* h_bound1, const double* h_bound2, double* h_od_fit);

/* ---- equal-error partition search over a batched error callback ---------------
 * Replaces class Equipartition (equipartition.h:63-208, equipartition.cpp).  The
 * callback evaluates n intervals at once and returns non-zero to abort.  status
 * receives the EpStatus value (equipartition.h:32-40). */
typedef int (*ecckd_error_fn)(int n, const double* bound1, const double* bound2, double* error, void* user);
typedef struct ecckd_partition ecckd_partition;
int ecckd_partition_create(ecckd_error_fn fn, void* user, ecckd_partition** p);
int ecckd_partition_destroy(ecckd_partition* p);
int ecckd_partition_configure(ecckd_partition* p, double resolution, double partition_tolerance,
                              int partition_max_iterations, int line_search_max_iterations,
                              int cubic_interpolation, int minimize_frac_range);
int ecckd_partition_n(ecckd_partition* p, int ni, double* bounds, double* error, int* status);
int ecckd_partition_e(ecckd_partition* p, double target_error, double bound0, double boundn,
                      int* ni, double* bounds, double* error, int capacity, int* status);
const char* ecckd_partition_status_string(int status);
/* Audit hook: every floating-point comparison that steers the search is reported, in the order it is taken, as (site, lhs,
 * rhs, outcome); the sites are numbered in csrc/partition_search.cpp.  fn = NULL switches it off.  The search itself is
 * unchanged (tests/test_partition_search.py runs with and without). */
typedef void (*ecckd_trace_fn)(int site, double lhs, double rhs, int taken, void* user);
int ecckd_partition_set_trace(ecckd_partition* p, ecckd_trace_fn fn, void* user);

/* One band of the main loop, find_g_points.cpp:1152-1266 (no sub-bands / base split):
 * equipartition_e to the heating-rate tolerance, restart with equipartition_n from
 * bounds sqrt(i/ng) if ng is outside [min_g_points, max_g_points] (:1232-1257). */
int ecckd_find_g_band(ecckd_gas* gas, size_t ibegin, size_t iend, double heating_rate_tolerance,
                      double tolerance_tolerance, int max_iterations, int min_g_points,
                      int max_g_points, int* ng, double* bounds, double* error, int capacity,
                      int* status, double* comp_cost);

/* ---- read_spectrum / read_merged_spectrum arithmetic (a1) ------------------------
 * File access stays with the caller; these are the nwav-sized operations behind it.
 * ecckd_derive_d_wavenumber_dev: read_spectrum.cpp:55-65, the spacing of a grid stored without
 *   "d_wavenumber" (interior: half the distance between the neighbours; ends: half their neighbour's).
 * ecckd_merge_scaling: the scaling of one constituent, read_merged_spectrum.cpp:117-147 - a requested
 *   concentration profile (nconc > 0: interp in pressure, ends clamped, divided by the file's own mole
 *   fraction) or the scalar rules (conc == 0 -> 0; conc > 0 -> conc / reference_surface_vmr, PARAMETER_ERROR
 *   if the file has none; scaling < 0 -> 1).  h_vmr_fl_out[nlay] is the row of vmr_fl the reference
 *   stores (:153-165); may be NULL.
 * ecckd_merge_spectrum_dev: merged (+)= od * scaling(level), :152-166; `first` overwrites instead of
 *   accumulating.  od is FLOAT (as in the CKDMIP files) or DOUBLE, merged is DOUBLE [nlay][merged_stride]. */
int ecckd_derive_d_wavenumber_dev(ecckd_ctx* ctx, size_t nwav, const double* d_wavenumber, double* d_d_wavenumber);
int ecckd_merge_scaling(int nlay, const double* h_pressure_hl, double scaling, double conc, double reference_surface_vmr,
                        const double* h_vmr_fl_one_gas, int nconc, const double* h_pressure_conc,
                        const double* h_conc_req, double* h_scaling_profile, double* h_vmr_fl_out);
int ecckd_merge_spectrum_dev(ecckd_ctx* ctx, int nlay, size_t nwav, const void* d_od, int od_type, size_t od_stride,
                             const double* h_scaling_profile, int first, double* d_merged, size_t merged_stride);

/* The merged matrix of one scenario from all its gases in ONE pass over their rows, which stay where they are for the next
 * scenario: d_merged[l][j] = sum over g, in gas order, of d_od[g][l][j] * h_scale[g][l], the product rounded, then the sum
 * (the first gas assigned) - bit for bit the matrix that ngas calls of ecckd_merge_spectrum_dev leave, the first overwriting,
 * at 4 ngas + 8 bytes per point and layer for FLOAT gases instead of a read-modify-write of the DOUBLE matrix per gas.
 * d_od[g] is [nlay][od_stride[g]], od_type[g] ECCKD_F32 or ECCKD_F64 per gas, 1 <= ngas <= 16, every stride >= nwav;
 * h_scale is [ngas][nlay] on the host; d_merged is DOUBLE [nlay][merged_stride], merged_stride >= nwav, columns beyond nwav
 * untouched, and overlaps no gas.  Rows may begin at any element: 16-byte accesses where a row allows them, single elements
 * where it does not.  Anything else is ECCKD_PARAMETER_ERROR before any launch.  Synchronous, like ecckd_merge_spectrum_dev.
 * ecckd_merge_scenario_geometry (host only): the kernel's tile - consecutive wavenumbers per thread, threads per block - for
 * tests that place their sizes at its edges. */
int ecckd_merge_scenario_dev(ecckd_ctx* ctx, int nlay, size_t nwav, int ngas, const void* const* d_od, const int* od_type,
                             const size_t* od_stride, const double* h_scale, double* d_merged, size_t merged_stride);
int ecckd_merge_scenario_geometry(int* points_per_thread, int* threads_per_block);

/* ---- sub-bands and base split of find_g_points --------------------------------
 * find_g_points.cpp:786-870 (sub-bands of the optically thin part of a band) and :1311-1346
 * (wavenumber split of the base g point) both re-rank a contiguous range of ranks
 * [rank_lo, rank_hi] so that the points are grouped by wavenumber interval
 * [h_wn_bound[s], h_wn_bound[s+1]) while keeping their rank order inside each group (a stable
 * partition).  d_rank[nwav] (rank of every wavenumber, original order) is updated in place;
 * h_count[nsub] receives the group sizes.  Returns ECCKD_PARAMETER_ERROR ("Failed to account
 * for all wavenumbers in split", :855-858, :1335-1338) if a point of the range lies in no group. */
int ecckd_regroup_rank_by_wavenumber_dev(ecckd_ctx* ctx, size_t nwav, const double* d_wavenumber,
                                         int32_t* d_rank, size_t rank_lo, size_t rank_hi, int nsub,
                                         const double* h_wn_bound, int64_t* h_count);

/* Sub-band set-up of one band, find_g_points.cpp:799-868.  [ibegin, iend] is the rank range of
 * the band (ibandloc(0), ibandloc(end)); h_boundary[nboundary] the configured
 * subband_wavenumber_boundary.  Outputs: *nsubband (0 if the band is not split), the first /
 * last rank of every sub-band (capacity nboundary + 1 each) and *iupperindex (:812).
 * d_rank is re-ranked in place; create the gas from it afterwards. */
int ecckd_subband_setup_dev(ecckd_ctx* ctx, size_t nwav, const double* d_wavenumber, int32_t* d_rank,
                            size_t ibegin, size_t iend, double g_split, double band_bound1,
                            double band_bound2, int nboundary, const double* h_boundary,
                            int* nsubband, int64_t* h_isubband1, int64_t* h_isubband2,
                            int64_t* iupperindex);

/* Everything find_g_points does for one band after the gas is prepared (:1152-1414): the
 * partition search (plain, :1231-1258, or per sub-band, :1186-1229), the base split
 * (:1265-1383, incl. the re-ranking of the base g point by wavenumber) and the rank range of
 * every g point (:1396-1401).  Zero-initialise the struct for the plain case. */
typedef struct {
  int min_g_points, max_g_points;
  /* sub-bands, from ecckd_subband_setup_dev; nsubband <= 1: none */
  int nsubband;
  const int64_t* isubband1;
  const int64_t* isubband2;
  int64_t iupperindex;
  double g_split;
  /* base split: base_split == 1 and nbase_wn_bound < 3: none (:1268-1271) */
  double base_split;
  int nbase_wn_bound;             /* nwavsplit + 1 entries, or 0 */
  const double* base_wn_bound;    /* band_bound1, interior boundaries, band_bound2 + 1 (:1294-1301) */
  const double* d_wavenumber;     /* [nwav] original order; needed if nwavsplit > 1 */
  int32_t* d_rank;                /* [nwav] original order, re-ranked in place if nwavsplit > 1 */
  size_t nwav;
  double band_albedo;             /* ecckd_find_g_bands_ex on a shortwave gas: this band's surface albedo (init_sw's band_albedo(jband),
                                   * find_g_points.cpp:1177); the one-band call uses ecckd_gas_set_band_albedo instead */
} ecckd_band_options;
int ecckd_find_g_band_ex(ecckd_gas* gas, size_t ibegin, size_t iend, double heating_rate_tolerance,
                         double tolerance_tolerance, int max_iterations,
                         const ecckd_band_options* opt, int* ng, double* bounds, double* error,
                         int64_t* rank1, int64_t* rank2, int capacity, int* status,
                         double* comp_cost);

/* All bands of a gas at once.  The band loop of find_g_points.cpp:1152 runs its searches one after the other, but they
 * are independent: here every band's search (exactly ecckd_find_g_band_ex, same decisions) runs in its own host thread
 * and the error evaluations the searches ask for at the same time are merged into ONE batch (ecckd_calc_error_multi),
 * so that narrow bands, too small to fill the GPU on their own, share it: the 13 longwave bands of the ecRad structure
 * go from 3.0e9 to 3.65e9 wavenumber-points/s (one band of the same size on its own: 5.4e9; the tail of the searches,
 * when only the widest bands are still refining, stays latency-bound).  Shortwave gases too: every band brings its surface
 * albedo in opt[b].band_albedo and the sweep takes it per interval (the gas's own band albedo, ecckd_gas_set_band_albedo,
 * is neither used nor changed).  Results per band as ecckd_find_g_band_ex, arrays [nband] or [nband][capacity(+1)].
 * An interval's error has the same bits alone and in any batch (every interval is summed in chunks of ITS OWN size), so a
 * search side by side ends where it ends on its own, converged or not.
 * Measured: 13 longwave bands 3.0e9 -> 3.65e9 points/s, 32 shortwave bands 1.7e9 -> 3.2e9. */
int ecckd_find_g_bands_ex(ecckd_gas* gas, int nband, const size_t* ibegin, const size_t* iend,
                          const double* heating_rate_tolerance, double tolerance_tolerance, int max_iterations,
                          const ecckd_band_options* opt /* [nband] */, int* ng, double* bounds, double* error,
                          int64_t* rank1, int64_t* rank2, int capacity, int* status, double* comp_cost);

/* The gas loop of find_g_points.cpp:655-1266 with the searches of SEVERAL prepared gases side by side on one device.  The
 * reference searches gas after gas; the searches are independent (each gas has its own prepared rows, the shared Planck
 * matrix is only read) and one search cannot fill the chip - most of its error batches are one or two intervals, bound by
 * launch and memory latency, each depending on the one before.  Every gas gets a host thread and a HIP stream of its own
 * (with its own pinned result slots and timing events) and runs exactly the launch trains it runs alone, so every search
 * takes the decisions it takes alone (same g points, same errors to the last bit) while one gas's short batches run in the
 * shadow of another gas's whole-partition passes.  One request per gas: the arguments of ecckd_find_g_bands_ex.
 * max_concurrent: gases searched at a time; <= 0: as many as the host has cores for (a gas with several bands runs a
 * thread per band).  The gases may belong to one context or to several.  req[k].rc = the gas's own return code. */
typedef struct {
  ecckd_gas* gas;
  int nband;
  const size_t* ibegin;                    /* [nband] */
  const size_t* iend;                      /* [nband] */
  const double* heating_rate_tolerance;    /* [nband] */
  const ecckd_band_options* opt;           /* [nband] */
  int* ng;                                 /* [nband] */
  double* bounds;                          /* [nband][capacity + 1] */
  double* error;                           /* [nband][capacity] */
  int64_t* rank1;                          /* [nband][capacity] or NULL */
  int64_t* rank2;                          /* [nband][capacity] or NULL */
  int capacity;
  int* status;                             /* [nband] */
  double* comp_cost;                       /* [nband] or NULL */
  int rc;                                  /* out */
} ecckd_gas_search;
int ecckd_find_g_gases(int ngas, ecckd_gas_search* req, double tolerance_tolerance, int max_iterations, int max_concurrent);
/* The same in pieces, for a caller that reads and prepares the NEXT gas while the gases it has prepared are being searched (the
 * tool: a gas's files stream in and its preparation runs on the context's stream while the lanes search): _begin opens a job,
 * _add starts the search of one prepared gas at once (its request and everything it points to must stay where it is until
 * _wait), _wait joins the searches, returns the first failure and closes the job.  A gas whose search re-ranks its base g
 * point by wavenumber (opt.nbase_wn_bound > 2) needs the context itself and is searched inside _add. */
typedef struct ecckd_gas_search_job ecckd_gas_search_job;
int ecckd_find_g_gases_begin(double tolerance_tolerance, int max_iterations, int max_concurrent, ecckd_gas_search_job** job);
int ecckd_find_g_gases_add(ecckd_gas_search_job* job, ecckd_gas_search* req);
int ecckd_find_g_gases_wait(ecckd_gas_search_job* job);

/* ---- the tolerance that yields a wanted number of g points ---------------------
 * The reference takes heating_rate_tolerance and reports the number of g points; its scripts keep hand-found tables of the
 * tolerance per g-point count (test/do_all_lw.sh:44-65).  Here the count is the input.  fn(s) = the total number of g points
 * when every band's configured tolerance is multiplied by s (non-zero return aborts, and is returned).  The search, host code
 * (csrc/target_search.cpp):
 *   1. s = 1; 2. bracket the target: double s while fn(s) > target, halve it while fn(s) < target, within [2^-20, 2^20];
 *   3. bisect geometrically, mid = sqrt(lo * hi), lo the scaling with ng > target and hi the one with ng < target;
 *   4. without an exact hit the answer is the trial with the smallest |ng - target|, among equals the one with
 *      ng < target, then the larger scaling.
 * status: 0 the target was hit; 1 hi / lo <= 1 + resolution (the count steps over the target there: both neighbours are in
 * the trial list); 2 max_trials trials spent (those of the bracketing included); 3 the bracket did not close within
 * [2^-20, 2^20] (the target is out of reach).  fn need not be monotone.  Every trial is recorded in order as
 * (trial_scaling[i], trial_ng[i]), i < *ntrial <= capacity; a trial beyond capacity: PARAMETER_ERROR (as are target_ng < 1,
 * resolution <= 0, max_trials < 1, fn == NULL). */
typedef int (*ecckd_count_fn)(double scaling, int* ng, void* user);   /* non-zero aborts */
int ecckd_target_search(ecckd_count_fn fn, void* user, int target_ng, double resolution, int max_trials,
                        double* scaling, int* ng, int* status,
                        int* ntrial, double* trial_scaling, int* trial_ng, int capacity);
/* The same over the searches of prepared gases: a trial copies the requests, sets every band's tolerance to
 * scaling * req[k].heating_rate_tolerance[b] (one multiplication; its result is the double reported in h_tolerance_used),
 * runs ecckd_find_g_gases as it stands and counts ng_offset + sum of ng[k][b] (the overlap of the gases gives
 * sum over bands of (1 - ngas + sum over gases of n_g_points), single_gas_data.cpp:30-38: ng_offset = nband * (1 - ngas)).
 * The gases stay as prepared and keep their memos of interval errors from trial to trial, so a trial sweeps only intervals no
 * earlier trial asked for, and takes the decisions of a plain run at its tolerances bit for bit.  The caller's tolerance arrays
 * are not written.  On return the requests' outputs are those of the chosen scaling: if that was not the last trial run it is
 * searched once more, from the memos.  A trial whose searches fail ends the call with that code.  A request with
 * opt.nbase_wn_bound > 2 is refused (PARAMETER_ERROR) before anything runs: that split re-ranks the spectrum during a search. */
int ecckd_find_g_gases_target(int ngas, ecckd_gas_search* req, int ng_offset, int target_ng,
                              double resolution, int max_trials,
                              double tolerance_tolerance, int max_iterations, int max_concurrent,
                              double* scaling, int* ng_total, int* status,
                              double* h_tolerance_used /* [sum of nband] in request order */,
                              int* ntrial, double* trial_scaling, int* trial_ng, int capacity);
/* Progress hook of ecckd_find_g_gases_target for the calling thread: fn is called after every trial (0-based, in order) with
 * its scaling, total and the g points of every gas (ng_per_gas[ngas], summed over the gas's bands).  fn = NULL switches it off. */
typedef void (*ecckd_target_trial_fn)(int trial, double scaling, int ng_total, int ngas, const int* ng_per_gas, void* user);
int ecckd_find_g_gases_target_observe(ecckd_target_trial_fn fn, void* user);

/* calc_median_sorting_variable (find_g_points.cpp:35-49) for n g points: the sorting variable
 * at the point where the cumulative weight (LW: surface Planck function, SW: solar irradiance,
 * :1404-1409) first reaches half of the interval's total.  d_sorting_variable_sorted[n points]
 * is in the gas's sorted order (gather it with ecckd_gather_f64_dev).  The cumulative sum is a
 * blocked scan, so the index can differ from the reference's sequential sum only where the
 * cumulative weight is within ~1e-13 (relative) of one half. */
int ecckd_gas_median_sorting_variable(ecckd_gas* gas, const double* d_sorting_variable_sorted, int n,
                                      const int64_t* h_ind1, const int64_t* h_ind2, double* h_median);
/* The same two launches with the caller's own weights: d_weight[n] and d_sorting_variable_sorted[n] in one order,
 * nint intervals [h_ind1[k], h_ind2[k]] inside 0..n-1.  ecckd_gas_median_sorting_variable calls through it with the gas's
 * surface Planck row or reordered irradiance.  With weights whose partial sums are exact in any order (small integers)
 * the point chosen is the reference's at every placement, `cumulative == half` included. */
int ecckd_median_sorting_variable_dev(ecckd_ctx* ctx, size_t n, const double* d_weight,
                                      const double* d_sorting_variable_sorted, int nint,
                                      const int64_t* h_ind1, const int64_t* h_ind2, double* h_median);

/* Host only: the tiling of the index kernels as this process runs them.  K3 (ecckd_stable_argsort_bands_dev): keys per
 * tile (ECCKD_SORT_ITEMS honoured) and per wave, tile counts per round of the row scan, the largest number of bands that
 * one nine-pass sort takes; the tile of the median's weight sums; the largest number of groups of
 * ecckd_regroup_rank_by_wavenumber_dev. */
int ecckd_index_geometry(int* sort_keys_per_tile, int* sort_keys_per_wave, int* sort_scan_round_tiles,
                         int* sort_max_one_sort_bands, int* median_tile, int* max_groups);

/* d_dst[i] = d_src[d_index[i]], i < n (the reordering gathers of find_g_points.cpp:781,:865). */
int ecckd_gather_f64_dev(ecckd_ctx* ctx, size_t n, const double* d_src, const int32_t* d_index,
                         double* d_dst);
/* d_inverse[d_perm[i]] = i (ireorder(irank) = range(0,n-1), find_g_points.cpp:778-779). */
int ecckd_invert_permutation_dev(ecckd_ctx* ctx, size_t n, const int32_t* d_perm, int32_t* d_inverse);

/* ---- line-by-line band fluxes --------------------------------------
 * A stand-in for the external CKDMIP tool that makes the training fluxes (test/run_lw_lbl_evaluation.sh),
 * restricted to the no-scattering radiative transfer the reference itself contains.  One column; the
 * spectral fluxes are summed over the inclusive wavenumber index ranges [h_band_begin[b], h_band_end[b]]
 * (ecckd_band_ranges) -> h_flux_*[nband][nlay+1], i.e. "band_flux_dn_lw" / "band_flux_up_lw" of a flux file.
 *   longwave:  planck_function (planck_function.cpp:22-54) + radiative_transfer_lw (radiative_transfer_lw.cpp:27-60),
 *              unit surface emissivity, surface Planck function at temperature_hl(end);
 *   shortwave: radiative_transfer_direct_sw, and with d_albedo[nwav] != NULL radiative_transfer_norayleigh_sw
 *              (radiative_transfer_sw.cpp:26-77); h_flux_up may be NULL.  No Rayleigh scattering. */
int ecckd_lbl_band_fluxes_lw(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_temperature_hl,
                             const double* d_wavenumber, const double* d_d_wavenumber, const void* d_od, int od_type,
                             size_t od_stride, int nband, const int64_t* h_band_begin, const int64_t* h_band_end,
                             double* h_flux_dn, double* h_flux_up);
int ecckd_lbl_band_fluxes_sw(ecckd_ctx* ctx, int nlay, size_t nwav, double cos_sza, const double* d_ssi,
                             const double* d_albedo, const void* d_od, int od_type, size_t od_stride, int nband,
                             const int64_t* h_band_begin, const int64_t* h_band_end, double* h_flux_dn_direct,
                             double* h_flux_up);
/* The same with the spectral fluxes at the boundaries as well (the CKDMIP tool's do_write_spectral_boundary_fluxes: what
 * LblFluxes::read maps to g points, lbl_fluxes.cpp:183-246, :301-325): d_surf_dn[nwav] = downwelling (shortwave: direct) flux at
 * the surface, d_toa_up[nwav] = upwelling flux at the top of the atmosphere, per wavenumber, device arrays, either may be NULL;
 * zero outside the bands. */
int ecckd_lbl_band_fluxes_lw_ex(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_temperature_hl,
                                const double* d_wavenumber, const double* d_d_wavenumber, const void* d_od, int od_type,
                                size_t od_stride, int nband, const int64_t* h_band_begin, const int64_t* h_band_end,
                                double* h_flux_dn, double* h_flux_up, double* d_surf_dn, double* d_toa_up);
/* The same with the zenith-angle quadrature of the external CKDMIP tool (namelist key nangle, test/run_ckd_lw.sh:28,
 * test/copy_to_ckdmip_lw.sh:32): nangle = 0 is the classic two-stream form above (diffusivity 1.66); nangle = N > 0 integrates
 * N Gauss-Legendre angles per hemisphere, flux = sum_k 2 w_k mu_k L(mu_k), each L(mu_k) the no-scattering recurrence of
 * radiative_transfer_lw.cpp:27-60 along the slant path tau / mu_k.  N <= 16.  The CKDMIP tool is not part of the reference's
 * sources: its node set is unpinned. */
int ecckd_lbl_band_fluxes_lw_angles(ecckd_ctx* ctx, int nangle, int nlay, size_t nwav, const double* h_temperature_hl,
                                    const double* d_wavenumber, const double* d_d_wavenumber, const void* d_od, int od_type,
                                    size_t od_stride, int nband, const int64_t* h_band_begin, const int64_t* h_band_end,
                                    double* h_flux_dn, double* h_flux_up, double* d_surf_dn, double* d_toa_up);
/* Gauss-Legendre nodes mu_k (ascending) and weights w_k of n points on (0, 1): sum_k w_k f(mu_k) ~ int_0^1 f(mu) dmu. */
int ecckd_gauss_legendre_01(int n, double* h_mu, double* h_weight);
/* Fluxes per g point from what run_ckd wrote (optical depth [ncol][nlay][ng], Planck function [ncol][nlay+1][ng] or incoming
 * solar flux [ncol][ng]): the `--ckd` evaluation of the CKDMIP tools as the scripts use it (test/run_ckd_lw.sh:133-137,
 * test/run_ckd_sw.sh:125-128), restricted to the reference's own no-scattering transfer - radiative_transfer_lw.cpp:27-60 with
 * unit emissivity (nangle as ecckd_lbl_band_fluxes_lw_angles) and radiative_transfer_sw.cpp:45-77.  Host arrays in and out
 * ([ncol][nlay+1][ng] fluxes), the arithmetic on the device. */
int ecckd_rt_lw_gpoints(ecckd_ctx* ctx, int nangle, int ncol, int nlay, int ng, const double* h_planck_hl, const double* h_od,
                        double* h_flux_dn, double* h_flux_up);
int ecckd_rt_sw_gpoints(ecckd_ctx* ctx, int ncol, int nlay, int ng, double cos_sza, double albedo, const double* h_incoming,
                        const double* h_od, double* h_flux_dn, double* h_flux_up);

int ecckd_lbl_band_fluxes_sw_ex(ecckd_ctx* ctx, int nlay, size_t nwav, double cos_sza, const double* d_ssi,
                                const double* d_albedo, const void* d_od, int od_type, size_t od_stride, int nband,
                                const int64_t* h_band_begin, const int64_t* h_band_end, double* h_flux_dn_direct,
                                double* h_flux_up, double* d_surf_dn_direct, double* d_toa_up);

/* Shortwave band fluxes of one column WITH Rayleigh scattering, nsza = 1..8 solar zenith angles (every cos_sza in (0, 1]) per
 * call: per wavenumber and layer tau = od_abs + od_ray (each ECCKD_F32 or ECCKD_F64, converted to double and added once),
 * single-scattering albedo w = od_ray / tau, and the two-stream equations at asymmetry 0 with ecRad's shortwave coefficients
 * (Zdunkowski PIFM: g1 = 2 - 1.25 w, g2 = 0.75 w, g3 = g4 = 0.5), solved by Meador & Weaver's (1980) closed form per layer and
 * the adding method over the column, above a Lambertian surface (d_albedo[nwav], the same for direct and diffuse light; NULL:
 * albedo 0).  The reference has no such transfer (it masks the fluxes it cannot represent, LblFluxes::mask_rayleigh_up); the
 * external CKDMIP tool, which is not among its sources, scatters by the rayleigh_optical_depth run_ckd writes apart
 * (run_ckd.cpp:166-192): node-for-node agreement with that tool is unpinned.  Where od_ray = 0 this is the
 * arithmetic of ecckd_lbl_band_fluxes_sw_ex, and the direct beam has that call's bits on tau throughout.
 * Results: h_flux_dn_direct, h_flux_dn (direct plus diffuse), h_flux_up [nsza][nband][nlay+1]; d_surf_dn_direct, d_surf_dn
 * (direct plus diffuse), d_toa_up: NULL or device arrays [nsza][nwav], zero outside the bands.  An angle of a call has the
 * bits of that angle computed by a call of its own.  Per-level state lives in the context's scratch: 3 (nlay+1) doubles per
 * thread of a bounded grid (3 blocks per compute unit; ECCKD_RAYLEIGH_GRID = N blocks instead). */
int ecckd_lbl_band_fluxes_sw_rayleigh(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_cos_sza, const double* d_ssi,
                                      const double* d_albedo, const void* d_od_abs, int abs_type, size_t abs_stride,
                                      const void* d_od_ray, int ray_type, size_t ray_stride, int nband, const int64_t* h_band_begin,
                                      const int64_t* h_band_end, double* h_flux_dn_direct, double* h_flux_dn, double* h_flux_up,
                                      double* d_surf_dn_direct, double* d_surf_dn, double* d_toa_up);
/* ecckd_rt_sw_gpoints with the same scattering transfer: h_od (absorption) and h_od_rayleigh [ncol][nlay][ng] as run_ckd
 * writes optical_depth and rayleigh_optical_depth; h_flux_dn_direct, h_flux_dn (direct plus diffuse), h_flux_up
 * [ncol][nlay+1][ng]. */
int ecckd_rt_sw_gpoints_rayleigh(ecckd_ctx* ctx, int ncol, int nlay, int ng, double cos_sza, double albedo, const double* h_incoming,
                                 const double* h_od, const double* h_od_rayleigh, double* h_flux_dn_direct, double* h_flux_dn,
                                 double* h_flux_up);

/* The band fluxes of one column for nscen SCENARIOS from one read of the gases' spectra: the loop of
 * test/run_lw_lbl_evaluation.sh:286-323 / test/run_sw_lbl_evaluation.sh:70-260 (one call of the CKDMIP tool per scenario, a
 * scenario differing from the next in one scaling per gas file) as one call.  d_od[ngas]: the gases' device matrices
 * [nlay][od_stride[g]], od_type[g] ECCKD_F32 or ECCKD_F64 per gas, 1 <= ngas <= 16; h_scale[nscen][ngas][nlay]: the scaling
 * profiles (ecckd_merge_scaling).  Scenario s is computed on tau = sum_g od_g * scale[s][g][level], product and sum rounded
 * separately in gas order - bit for bit the DOUBLE matrix ngas calls of ecckd_merge_spectrum_dev leave (read_merged_spectrum.cpp:
 * 152-166), which is formed in registers and never written - with the arithmetic of ecckd_lbl_band_fluxes_lw_angles (nangle
 * 0..16) / ecckd_lbl_band_fluxes_sw_ex (nsza = 1..8 solar zenith angles at once, every cos_sza in (0, 1]; d_albedo NULL: no
 * upwelling sweep, h_flux_up all zero).  Results: h_flux_dn / h_flux_up [nscen][nband][nlay+1] (shortwave:
 * [nscen][nsza][nband][nlay+1]); d_surf_dn / d_toa_up: NULL or device arrays [nscen][nwav] (shortwave [nscen][nsza][nwav]), the
 * spectral boundary fluxes as the _ex / _angles calls write them.  Scenario s (and angle a) of a call has the bits of that
 * scenario (and angle) computed by a call of its own.
 * A launch carries T "slots" (longwave: scenarios; shortwave: scenario-angle pairs), T = ecckd_lbl_scenarios_slots(shortwave,
 * nlay) = min(8, 43008 / (64 (nlay+1))) longwave, min(16, 59392 / (64 (nlay+1))) shortwave: the 4 x T x 2 (nlay+1) doubles
 * of a block's LDS accumulator within 42 KB / 58 KB.  T = 0 - nlay > 671 longwave, > 927 shortwave - is a PARAMETER_ERROR.
 * More slots than T run as several launches, each reading the gas rows again: scenarios are split first (evenly over
 * ceil(nscen / T) launches; shortwave: min(T, 16) / nsza scenarios with all their angles per launch), the angles of one
 * scenario only where nsza > T. */
int ecckd_lbl_band_fluxes_lw_scenarios(ecckd_ctx* ctx, int nangle, int nlay, size_t nwav, const double* h_temperature_hl,
                                       const double* d_wavenumber, const double* d_d_wavenumber, int ngas, const void* const* d_od,
                                       const int* od_type, const size_t* od_stride, int nscen, const double* h_scale, int nband,
                                       const int64_t* h_band_begin, const int64_t* h_band_end, double* h_flux_dn, double* h_flux_up,
                                       double* d_surf_dn, double* d_toa_up);
int ecckd_lbl_band_fluxes_sw_scenarios(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_cos_sza, const double* d_ssi,
                                       const double* d_albedo, int ngas, const void* const* d_od, const int* od_type,
                                       const size_t* od_stride, int nscen, const double* h_scale, int nband,
                                       const int64_t* h_band_begin, const int64_t* h_band_end, double* h_flux_dn_direct,
                                       double* h_flux_up, double* d_surf_dn_direct, double* d_toa_up);
/* Slots per launch of the two calls above at nlay layers (0: more layers than the accumulator holds; no device needed). */
int ecckd_lbl_scenarios_slots(int shortwave, int nlay);

/* ecckd_lbl_band_fluxes_sw_rayleigh for nscen SCENARIOS from one read of the gases' spectra.  d_od[ngas], od_type, od_stride and
 * h_scale[nscen][ngas][nlay] are the absorbers and their scaling profiles as ecckd_lbl_band_fluxes_sw_scenarios takes them
 * (1 <= ngas <= 16); d_od_ray [nlay][ray_stride], ECCKD_F32 or ECCKD_F64, is what scatters, the same unscaled row in every
 * scenario.  Scenario s at angle a is what ngas calls of ecckd_merge_spectrum_dev with h_scale[s] followed by
 * ecckd_lbl_band_fluxes_sw_rayleigh on that DOUBLE matrix and d_od_ray give: tau_abs = sum_g od_g * scale[s][g][level] in gas
 * order as ecckd_lbl_band_fluxes_sw_scenarios forms it (bit for bit the matrix with one gas; with more, the product and sum of
 * a gas may be fused where the merge kernel rounds twice: a few 1e-14 of the incoming flux), formed once per
 * scenario in the kernel and never written as a matrix; tau = tau_abs + (double)od_ray, added once; the same layer terms,
 * adding sweeps and reduction order.  nsza = 1..8, every cos_sza in (0, 1]; d_albedo[nwav] or NULL (albedo 0).  Results:
 * h_flux_dn_direct, h_flux_dn (direct plus diffuse), h_flux_up [nscen][nsza][nband][nlay+1]; d_surf_dn_direct, d_surf_dn,
 * d_toa_up: NULL or device arrays [nscen][nsza][nwav], zero outside the bands.
 * Launch split: the chunk partials of a launch are nchunk x ns x nsza x 3 x (nlay+1) doubles (nchunk: 256-wavenumber chunks of
 * the bands), so a launch takes ns = ecckd_lbl_rayleigh_scenarios_per_launch(nlay, nsza, nchunk) whole scenarios with all their
 * angles: as many as fit 512 MB of partials (ECCKD_RAYLEIGH_SCENARIO_BYTES = N bytes instead), one at least.  Per-level state
 * lives in the context's scratch, 4 (nlay+1) doubles per thread of a bounded grid (4 blocks per compute unit;
 * ECCKD_RAYLEIGH_GRID = N blocks instead).
 * Bit equality: scenario s (and angle a) of a call has the bits of that scenario (and angle) computed by a call of its own;
 * neither the scenarios that share a launch, nor the grid, nor which block walks a chunk changes a bit of any result. */
int ecckd_lbl_band_fluxes_sw_rayleigh_scenarios(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_cos_sza,
                                                const double* d_ssi, const double* d_albedo, int ngas, const void* const* d_od,
                                                const int* od_type, const size_t* od_stride, const void* d_od_ray, int ray_type,
                                                size_t ray_stride, int nscen, const double* h_scale, int nband,
                                                const int64_t* h_band_begin, const int64_t* h_band_end, double* h_flux_dn_direct,
                                                double* h_flux_dn, double* h_flux_up, double* d_surf_dn_direct, double* d_surf_dn,
                                                double* d_toa_up);
/* Scenarios per launch of the call above under the current budget (0: nlay or nsza below 1; no device needed). */
int ecckd_lbl_rayleigh_scenarios_per_launch(int nlay, int nsza, size_t nchunk);

/* ---- NetCDF classic files (file parts of a1, a9, a21) ----------------------------
 * A self-contained reader / writer for the classic on-disk formats CDF-1, CDF-2 (64-bit offset)
 * and CDF-5 (64-bit data): what the reference reads / writes for *.nc, *.cdf names
 * (src/tools/DataFile.cpp:88-96, OutputDataFile.cpp:84-157).  NetCDF-4 files (HDF5 containers, the *.h5
 * names of the scripts) are recognised by their signature and READ through the system's HDF5 library,
 * loaded at run time (csrc/nc_hdf5.cpp; ECCKD_HDF5_LIB overrides the search); files are always WRITTEN in
 * the classic format, which the NetCDF library reads back whatever the file is called.  Reads convert every external type to double like
 * nc_get_vara_double (DataFileEngineNetcdf.cpp:593-599); slice >= 0 selects one index of the
 * slowest dimension like DataFile::read(M, "v", j) (:582-590), slice < 0 the whole variable.
 * var == NULL or "" addresses the global attributes.  nc_type: 1 byte, 2 char, 3 short, 4 int,
 * 5 float, 6 double (7-11: CDF-5 unsigned / 64-bit integers). */
typedef struct ecckd_nc ecckd_nc;
int ecckd_nc_open(const char* path, ecckd_nc** file);
int ecckd_nc_close(ecckd_nc* file);
int ecckd_nc_inq_dim(ecckd_nc* file, const char* name, size_t* length);
int ecckd_nc_inq_var(ecckd_nc* file, const char* name, int* exists, int* nc_type, int* ndims, size_t* shape,
                     int shape_capacity);
int ecckd_nc_read_double(ecckd_nc* file, const char* name, long long slice, double* out, size_t capacity);
/* One index of the slowest dimension (slice >= 0) or the whole variable straight into device memory as FLOAT (out_type 4)
 * or DOUBLE (8): replaces DataFile::read -> nc_get_vara_double -> element-wise copy (DataFileEngineNetcdf.cpp:593-608) for
 * the spectra.  A contiguous FLOAT / DOUBLE variable of a classic file is streamed - reader threads fill pinned buffers,
 * a copy stream ships them, a kernel decodes the big-endian values on the device, reading overlaps shipping; anything
 * else (NetCDF-4, record variables, integer types) is read on the host and uploaded once.  capacity in elements. */
int ecckd_nc_read_dev(ecckd_ctx* ctx, ecckd_nc* file, const char* name, long long slice, int out_type, void* d_out,
                      size_t capacity);
/* zlib streams (RFC 1950 / 1951: what HDF5's deflate filter leaves in a chunk) inflated on the device, one wavefront per
 * stream - the NetCDF-4 spectra are read this way by ecckd_nc_read_dev (the reference leaves it to the HDF5 library on the
 * reading thread, DataFileEngineNetcdf.cpp:593-608).  Host-pointer form: stream s is h_in[h_in_off[s] .. h_in_off[s + 1]) and
 * must inflate to exactly h_out_bytes[s] bytes, written one stream after the other to h_out; h_status[s] = 0, or 1 bad
 * header, 2 bad block, 3 bad code, 4 distance too far back, 5 more output than expected, 6 less, 7 input exhausted.
 * The Adler-32 trailer is not verified. */
int ecckd_inflate(ecckd_ctx* ctx, int nstreams, const void* h_in, const unsigned long long* h_in_off,
                  const unsigned long long* h_out_bytes, void* h_out, int* h_status);
/* One zlib stream inflated on the calling thread by the in-tree decoder the worker threads of ecckd_nc_read_dev use before
 * they fall back to zlib (csrc/fast_inflate.cpp; no device involved).  *ok = 1: the stream inflates to exactly out_bytes
 * bytes with the right Adler-32 and out holds them; 0: not taken or a check failed. */
int ecckd_inflate_host(const void* in, size_t in_bytes, void* out, size_t out_bytes, int* ok);
int ecckd_nc_read_att_text(ecckd_nc* file, const char* var, const char* att, int* exists, char* out, size_t capacity);
int ecckd_nc_read_att_double(ecckd_nc* file, const char* var, const char* att, int* nelems, double* out, size_t capacity);
/* writing: define, ecckd_nc_enddef (picks CDF-1 / CDF-2 / CDF-5 from the sizes), then whole variables */
int ecckd_nc_create(const char* path, ecckd_nc** file);
int ecckd_nc_def_dim(ecckd_nc* file, const char* name, size_t length, int* dimid);
int ecckd_nc_def_var(ecckd_nc* file, const char* name, int nc_type, int ndims, const int* dimids, int* varid);
int ecckd_nc_put_att_text(ecckd_nc* file, const char* var, const char* att, const char* text);
int ecckd_nc_put_att_double(ecckd_nc* file, const char* var, const char* att, int nc_type, int n, const double* values);
/* deflate_variable (OutputDataFile.cpp:345-359): shuffle + deflate level 2 for this variable when the file is written as
 * NetCDF-4 (a name ending in .h5 / .hdf where the HDF5 libraries can be loaded; ECCKD_CLASSIC_OUTPUT forces classic), nothing
 * otherwise.  ecckd_nc_is_netcdf4: which of the two an open handle is. */
int ecckd_nc_deflate_var(ecckd_nc* file, const char* name);
int ecckd_nc_is_netcdf4(ecckd_nc* file, int* is_netcdf4);
int ecckd_nc_enddef(ecckd_nc* file);
int ecckd_nc_write_double(ecckd_nc* file, const char* name, const double* data, size_t count);
/* one index of the slowest dimension of a variable (count = the elements below that dimension).  A dimension defined with
 * length 0 is the unlimited (record) dimension of a classic file - at most one, the slowest dimension of its variables; such
 * variables are written record by record through this call, a record past the last one extends the record count (records in
 * between and the other record variables of a new record read back as zeros).  In NetCDF-4 output the same calls make chunked
 * datasets with an unlimited first dimension that are extended record by record. */
int ecckd_nc_write_slice_double(ecckd_nc* file, const char* name, size_t slice, const double* data, size_t count);
/* One index of the slowest TWO dimensions (`count` = the product of the others): a (column, angle, level, wavenumber) record
 * angle by angle.  Refused for a variable that is deflated in NetCDF-4 output. */
int ecckd_nc_write_subslice_double(ecckd_nc* file, const char* name, size_t slice, size_t sub, const double* data, size_t count);
/* write_order (write_order.cpp:24-143): same variables, external types and attributes; `history` is the
 * line OutputDataFile::append_history would add (may be NULL); column_optical_depth may be NULL (:88). */
int ecckd_write_order_file(const char* path, const char* molecule, const char* config_str, const char* history, int nband,
                           const double* band_bound1, const double* band_bound2, size_t nwav, const double* wavenumber,
                           const double* d_wavenumber, const int16_t* iband, const int32_t* rank,
                           const double* column_optical_depth, const double* sorting_variable);

/* ---- configuration: `exe [key=value ...] [file.cfg]` (drop-in surface) ------
 * Host-only.  Replaces DataFile(argc, argv) -> DataFileEngineCfg (src/tools/DataFileEngineCfg.cpp:61-80) and
 * the rc_* functions of src/tools/readconfig.c it calls, one entry point per function used:
 *   ecckd_cfg_from_args     the constructor: rc_read(NULL) + rc_register_files + rc_get_file (first argument
 *                           without '=' whose name contains ".cfg") + rc_append + rc_register_args
 *   ecckd_cfg_append_file   rc_append (readconfig.c:557-880; grammar in csrc/config.cpp)
 *   ecckd_cfg_register      rc_register (:885-896); value NULL -> "1"
 *   ecckd_cfg_exists        rc_exists;   ecckd_cfg_get_boolean  rc_get_boolean (:1262-1287)
 *   ecckd_cfg_get_int/_real rc_assign_int / rc_assign_real (:1293-1407): *value untouched and *found = 0 when absent
 *   ecckd_cfg_get_string    rc_get_string (isub < 0) / rc_get_substring (isub >= 0) (:1481-1500, :1622-1633)
 *   ecckd_cfg_size          rc_size (:1653-1666): number of items and the declared [m][n]
 *   ecckd_cfg_get_real_vector / _int_vector   rc_get_real_vector / rc_get_int_vector (:1720-1790)
 *   ecckd_cfg_sprint        rc_sprint (:1113-1253): the string stored in the `config` attribute of every output file
 * `scope` (may be NULL) is the section of DataFile::read(x, scope, name): rc_set_section(scope) around the call.
 * Strings are copied into buf[cap] (always terminated) and *len receives the full length.
 * A file that cannot be opened or parsed returns ECCKD_CANNOT_OPEN_MANDATORY_FILE like open_absolute (:32-52). */
#define ECCKD_CANNOT_OPEN_MANDATORY_FILE 139
typedef struct ecckd_cfg ecckd_cfg;
int ecckd_cfg_create(ecckd_cfg** cfg);
int ecckd_cfg_from_args(int argc, const char* const* argv, ecckd_cfg** cfg);
int ecckd_cfg_append_file(ecckd_cfg* cfg, const char* path);
int ecckd_cfg_append_text(ecckd_cfg* cfg, const char* text, const char* name);
int ecckd_cfg_register(ecckd_cfg* cfg, const char* param, const char* value);
int ecckd_cfg_destroy(ecckd_cfg* cfg);
int ecckd_cfg_file_name(const ecckd_cfg* cfg, char* buf, size_t cap, size_t* len);
int ecckd_cfg_count(const ecckd_cfg* cfg, int* n);
int ecckd_cfg_entry(const ecckd_cfg* cfg, int i, char* param, size_t param_cap, char* value, size_t value_cap,
                    size_t* value_len, int* has_value, int* m, int* n);
int ecckd_cfg_exists(const ecckd_cfg* cfg, const char* scope, const char* param, int* exists);
int ecckd_cfg_get_boolean(const ecckd_cfg* cfg, const char* scope, const char* param, int* value);
int ecckd_cfg_get_int(const ecckd_cfg* cfg, const char* scope, const char* param, int* value, int* found);
int ecckd_cfg_get_real(const ecckd_cfg* cfg, const char* scope, const char* param, double* value, int* found);
int ecckd_cfg_get_string(const ecckd_cfg* cfg, const char* scope, const char* param, int isub, char* buf, size_t cap,
                         size_t* len, int* found);
int ecckd_cfg_size(const ecckd_cfg* cfg, const char* scope, const char* param, int* count, int* m, int* n);
int ecckd_cfg_get_real_vector(const ecckd_cfg* cfg, const char* scope, const char* param, double* buf, int cap, int* len);
int ecckd_cfg_get_int_vector(const ecckd_cfg* cfg, const char* scope, const char* param, int* buf, int cap, int* len);
int ecckd_cfg_sprint(const ecckd_cfg* cfg, char* buf, size_t cap, size_t* len);

/* ---- optimize_lut: cost function, gradient and minimisation (K8/K9) ------------
 * Replaces CkdOptimizable::calc_cost_function_gradient (solve_adept.cpp:240-292), i.e.
 * calc_cost_function_and_gradient (:72-211: CkdModel::calc_optical_depth ckd_model.cpp:925-1102,
 * negative-OD penalty, calc_cost_function_ckd_lw calc_cost_function_lw.cpp:116-232, Adept
 * reverse pass) plus CkdModel::calc_background_cost_function (ckd_model.cpp:840-877), and
 * solve_adept itself (:310-417).  Longwave (calc_cost_function_ckd_lw) and shortwave
 * (calc_cost_function_ckd_sw, calc_cost_function_sw.cpp:116-277), linear LUT interpolation.
 * All arrays here are HOST arrays; the handle uploads them once. */
typedef struct {
  int conc_dependence;          /* 0 none, 1 linear, 2 look-up table, 3 relative-linear (ckd_model.cpp:418-482) */
  int is_active;                /* in the gas list being optimised (optimize_lut.cpp:161) */
  int nconc;                    /* conc_dependence 2: number of mole fractions */
  const double* vmr;            /* [nconc], uniform in log (ckd_model.cpp:1006-1009) */
  double reference_vmr;         /* conc_dependence 3 */
  const double* molar_abs;      /* [(nconc)][nt][np][ng], g fastest */
  const double* min_molar_abs;  /* same shape or NULL */
  const double* max_molar_abs;
} ecckd_opt_gas;

typedef struct {
  int ng, nt, np;
  const double* log_pressure;        /* [np], evenly spaced (ckd_model.cpp:946-948) */
  const double* temperature;         /* [nt][np] */
  int ntp;
  const double* temperature_planck;  /* [ntp] */
  const double* planck_function;     /* [ntp][ng] */
  const int* iband_per_g;            /* [ng] g point -> band of the training fluxes (ckd_model.h:287-306) */
  int ngas;
  const ecckd_opt_gas* gases;
  int logarithmic_interpolation;     /* must be 0 (ckd_model.h:359) */
  /* shortwave (NULL / NULL = longwave model): solar irradiance per g point and the Rayleigh molar
   * scattering coefficient per g point (ckd_model.h:242-252; fixed unless the handle is made with
   * ECCKD_OPT_RAYLEIGH_ACTIVE) */
  const double* solar_irradiance;           /* [ng] */
  const double* rayleigh_molar_scattering;  /* [ng] or NULL */
} ecckd_opt_model;

typedef struct {
  int ncol, nlay, nband;
  const double* pressure_hl;     /* [ncol][nlay+1] */
  const double* temperature_hl;  /* [ncol][nlay+1] */
  const double* vmr_fl;          /* [ncol][ngas][nlay], gases in MODEL order (LblFluxes::gas_mapping applied) */
  const int* gas_present;        /* [ngas] 0 where the training file lacks the gas (gas_mapping < 0); NULL = all */
  const double* surf_emissivity; /* [ncol][nband] or NULL = 1 (lbl_fluxes.cpp:395-396) */
  const double* flux_dn;         /* [ncol][nlay+1][nband] LBL band fluxes (spectral_flux_dn_) */
  const double* flux_up;
  const double* spectral_flux_dn_surf;  /* [ncol][ng] or NULL (lbl_fluxes.cpp:301-328) */
  const double* spectral_flux_up_toa;
  /* shortwave scenes (lbl_fluxes.cpp:68-148): columns already replicated per solar zenith angle */
  const double* mu0;                        /* [ncol] */
  double tsi;                               /* total solar irradiance of the training file (:127) */
  const double* albedo;                     /* [nband] effective spectral albedo (:147-148, mask_rayleigh_up) */
  const double* spectral_boundary_weights;  /* [ng] erythemal_weight * erythemal_spectrum_ (solve_adept.cpp:182) or NULL */
  /* optional [ncol][nlay] full-level temperature; NULL = pressure-weighted mean of temperature_hl
   * (solve_adept.cpp:38-41, run_ckd.cpp:120-122).  scale_lut uses the plain mean (scale_lut.cpp:108). */
  const double* temperature_fl;
  /* optional [ncol][nlay+1][ng]: CKD fluxes of the "relative_to" scene at the initial coefficients
   * (optimize_lut.cpp:204-236, obtained with ecckd_opt_forward on that scene), subtracted from the forward
   * model per g point (solve_adept.cpp:118-148, calc_cost_function_lw.cpp:162-165); the caller subtracts the
   * relative-to LBL fluxes from flux_dn / flux_up itself (LblFluxes::subtract, optimize_lut.cpp:251-254) */
  const double* relative_flux_dn;
  const double* relative_flux_up;
} ecckd_opt_scene;

typedef struct {
  double flux_weight, flux_profile_weight, broadband_weight, spectral_boundary_weight;
  double negative_od_penalty;    /* optimize_lut.cpp:149 default 1e4 */
  double pressure_weight_power;  /* solve_adept.cpp:131-143 default 0.5 */
  double prior_error, min_prior_error, max_prior_error, prior_error_scaling;
  double pressure_corr, temperature_corr, conc_corr;
  double cap_relative_linear;    /* optimize_lut.cpp:185 passes 0.8; 0 disables */
} ecckd_opt_config;

typedef struct ecckd_opt ecckd_opt;
int ecckd_opt_create(ecckd_ctx* ctx, const ecckd_opt_model* model, int nscene,
                     const ecckd_opt_scene* scenes, const ecckd_opt_config* config, ecckd_opt** opt);
/* ecckd_opt_create with flags (ecckd_opt_create is flags = 0).
 * ECCKD_OPT_RAYLEIGH_SCATTERING: the shortwave forward model is the two-stream transfer with Rayleigh scattering that
 * ecckd_lbl_band_fluxes_sw_rayleigh and ecckd_rt_sw_gpoints_rayleigh compute, not radiative_transfer_norayleigh_sw.  Per
 * column and g point tau_abs is the gas optical depth after the clamp of negative values (and its penalty), tau_ray =
 * moles_per_layer * rayleigh_molar_scattering[g], the incoming flux mu0 * tsi_scaling * solar_irradiance[g], the surface
 * Lambertian with albedo[band of g] (a non-positive albedo counts as 0).  The cost is calc_cost_function_sw.cpp:116-277 on the
 * TOTAL downwelling (direct + diffuse) and the upwelling flux, with the heating rates of model and scenes from the net flux
 * dn - up; a scene's flux_dn, spectral_flux_dn_surf and relative_flux_dn are total downwelling fluxes.  ecckd_opt_forward(_ex)
 * return (total dn, up) in h_flux and tau_abs + tau_ray in h_od.  Refused with ECCKD_PARAMETER_ERROR unless the model is
 * shortwave with rayleigh_molar_scattering and at most 512 g points, every scene has mu0 and albedo, and the kernel's band and
 * cost arrays (lds_bytes of ecckd_opt_forward_plan, about 48 nlay nband bytes) fit 160 KB of LDS.  Rayleigh is a fixed
 * pseudo gas unless ECCKD_OPT_RAYLEIGH_ACTIVE is set as well.
 * ECCKD_OPT_RAYLEIGH_ACTIVE: the ng Rayleigh coefficients are optimised too.  The state carries ng more elements
 * x = ln(rayleigh_molar_scattering[g]) BEHIND the active gases' elements, in g order (ckd_model.cpp:109-111, :244-252), so
 * ecckd_opt_nx grows by ng; all gases may then be inactive (the state is the ng elements alone).  A coefficient of 0 is pinned
 * at MIN_X with gradient exactly 0.  The elements have NO bounds: ecckd_opt_initial_state gives them -inf / +inf whatever the
 * gases' min / max tables (the reference activates bounds it never sets, ckd_model.cpp:136-137, solve_adept.cpp:346-347).
 * Their prior is set with ecckd_opt_set_rayleigh_prior (none until then).  Gradient, by forward model:
 *   without ECCKD_OPT_RAYLEIGH_SCATTERING Rayleigh is one more absorber, added before the clamp of negative optical depths
 *     (solve_adept.cpp:32-35): dJ/dk_ray[g] = sum over all cells of moles_per_layer(cell) * dJ/dtau[cell][g], the clamped
 *     cells' penalty derivative included;
 *   with it tau_ray enters the two-stream layer terms beside tau_abs, after the clamp: dJ/dtau_ray of a cell is the adjoint
 *     of the five layer terms times their derivative with respect to tau_ray at fixed tau_abs, and a cell whose gas optical
 *     depth was clamped keeps it;
 *   then dJ/dx = dJ/dk * k, the prior's d / sigma^2, and |g| < 1e-80 -> 0 (solve_adept.cpp:286).
 * Every sum has a fixed order (no atomics): cost and gradient are bitwise reproducible.  Refused with ECCKD_PARAMETER_ERROR
 * unless the model is shortwave with rayleigh_molar_scattering.  Every other function works unchanged on the longer vector;
 * ecckd_opt_forward(_ex) take the coefficients from h_x. */
#define ECCKD_OPT_RAYLEIGH_SCATTERING 1u
#define ECCKD_OPT_RAYLEIGH_ACTIVE 2u
int ecckd_opt_create_ex(ecckd_ctx* ctx, const ecckd_opt_model* model, int nscene, const ecckd_opt_scene* scenes,
                        const ecckd_opt_config* config, unsigned flags, ecckd_opt** opt);
/* ecckd_opt_create_ex with the zenith-angle quadrature of the longwave truth (ecckd_opt_create_ex is nangle = 0, and nangle = 0
 * here gives the handle it makes: same kernels, same ecckd_opt_forward_plan, the same bits of cost and gradient).
 * nangle = N in 1..16: the longwave forward model integrates N Gauss-Legendre angles per hemisphere, the nodes of
 * ecckd_lbl_band_fluxes_lw_angles (sec_k = 1 / mu_k, wgt_k = 2 w_k mu_k, sum_k wgt_k = 1), not one path at the diffusivity 1.66
 * (nangle = 0 is "no quadrature", not "one angle at 1.66").  Per column, g point and angle k, with the Planck levels B_l and the
 * optical depth tau_l after clamp and penalty as without the key:
 *   eps_k = 1 - exp(-sec_k tau_l),  fac_k = eps_k > 1e-5 ? 1 - eps_k / (sec_k tau_l) : eps_k / 2
 *   dn_k[0] = 0,  dn_k[l+1] = dn_k[l] (1 - eps_k) + B_l (eps_k - fac_k) + B_l+1 fac_k,    dn[i] = sum_k wgt_k dn_k[i]
 *   up_k[nlay] = es B_nlay + (1 - es) dn[nlay]   (Lambertian surface, es = surf_emissivity of the g point's band)
 *   up_k[l] = up_k[l+1] (1 - eps_k) + B_l+1 (eps_k - fac_k) + B_l fac_k,                  up[i] = sum_k wgt_k up_k[i]
 * With es = 1 these are the fluxes of ecckd_rt_lw_gpoints(nangle = N).  Everything behind dn and up is unchanged (band sums,
 * relative_to, heating rates, every cost term, the penalty), and so is every other function of the handle.  The adjoint is
 * hand-derived: each angle receives the seeds scaled by wgt_k and runs the two reversed recurrences with sec_k in place of
 * 1.66; the surface couples them, dn_bar_k[nlay] += wgt_k (1 - es) sum_j up_bar_j[nlay]; dJ/dtau_l is the sum over the angles
 * in angle order.  Cost and gradient are bitwise reproducible.  One kernel, k_opt_forward_adjoint_lw_angles, serves the handle at
 * every shape (ecckd_opt_forward_plan: cells = 3, nc_template = nb = 0, threads = ngpad * lgroups from 1024 or ECCKD_K8A_THREADS
 * (64 ... 1024), lds_bytes = two flux rows of (nlay + 1) ng doubles and the band and cost arrays).  Its per-angle state lives in
 * a device workspace of the handle, ncol (5 nangle + 1) (nlay + 1) ng doubles, allocated here (ECCKD_OUT_OF_MEMORY if that fails).
 * Refused with ECCKD_PARAMETER_ERROR: nangle outside 0..16; nangle > 0 on a shortwave model (solar_irradiance), with any
 * ECCKD_OPT_RAYLEIGH flag, with more than 1024 g points, or with lds_bytes above 160 KB.  Nothing is refused at launch. */
int ecckd_opt_create_angles(ecckd_ctx* ctx, const ecckd_opt_model* model, int nscene, const ecckd_opt_scene* scenes,
                            const ecckd_opt_config* config, unsigned flags, int nangle, ecckd_opt** opt);
/* the nangle the handle was made with (0: ecckd_opt_create, ecckd_opt_create_ex) */
int ecckd_opt_nangle(ecckd_opt* opt);
int ecckd_opt_destroy(ecckd_opt* opt);
/* length of the state vector x = ln(molar_abs) of the active gases, in model gas order (ECCKD_OPT_RAYLEIGH_ACTIVE: then the ng
 * elements ln(rayleigh_molar_scattering)) */
size_t ecckd_opt_nx(ecckd_opt* opt);
/* initial state (MIN_X = -1e20 where the coefficient is 0) and log-space bounds, solve_adept.cpp:335-353 */
int ecckd_opt_initial_state(ecckd_opt* opt, double* h_x, double* h_x_min, double* h_x_max);
int ecckd_opt_cost_grad(ecckd_opt* opt, const double* h_x, double* J, double* h_grad);
/* Which forward kernel ecckd_opt_cost_grad / ecckd_opt_forward launch for this handle, and how: decided from the shapes
 * (shortwave?, nlay, ng, nband, entries per cell of the look-up tables) and from the environment, read at every call:
 * ECCKD_K8A_THREADS (64 ... 1024: threads per block in place of 1024 longwave / 512 shortwave), ECCKD_K8A_GENERIC=1 (the general
 * kernel).  cells: the cell-parallel kernel, instance <nc_template, shortwave, nb> (nc_template 4 or 8 cells per thread; nb 1 ... 4
 * eight-entry batches in straight-line code, 0 = the loop for more than 32 entries); cells == 0: the general kernel (nc_template
 * = nb = 0), which refuses lds_bytes > 160 KB when it is launched.  threads = ngpad * lgroups, ngpad = ng rounded up to 64.
 * A handle made with ECCKD_OPT_RAYLEIGH_SCATTERING runs one kernel at every shape, k_opt_forward_adjoint_rayleigh: cells = 2,
 * nc_template = nb = 0 (its cells and table entries are loops), threads = ngpad * lgroups from 512 or ECCKD_K8A_THREADS (64 ... 512),
 * lds_bytes = the band and cost arrays only (the per-level state lives in a device workspace of the handle; more than 160 KB
 * was refused when the handle was made); ECCKD_K8A_GENERIC is not read.
 * A handle made by ecckd_opt_create_angles with nangle > 0 runs k_opt_forward_adjoint_lw_angles at every shape: cells = 3,
 * nc_template = nb = 0, threads = ngpad * lgroups from 1024 or ECCKD_K8A_THREADS (64 ... 1024), lds_bytes = the angle-summed flux
 * rows and the band and cost arrays (checked against 160 KB when the handle was made); ECCKD_K8A_GENERIC is not read. */
typedef struct {
  int cells, nc_template, nb, threads, ngpad, lgroups;
  size_t lds_bytes;
} ecckd_forward_plan;
int ecckd_opt_forward_plan(ecckd_opt* opt, ecckd_forward_plan* plan);
/* total optical depth [ncol][nlay][ng] and CKD fluxes [ncol][2][nlay+1][ng] at state h_x
 * (calc_total_optical_depth, LblFluxes::calc_ckd_fluxes lbl_fluxes.cpp:443-471) */
int ecckd_opt_forward(ecckd_opt* opt, const double* h_x, double* h_od, double* h_flux);
/* the same with unclamped != 0: negative total optical depths are NOT set to zero before the radiative transfer - how the
 * reference evaluates its "relative_to" scene (optimize_lut.cpp:229-234: od = value(aod) -> LblFluxes::calc_ckd_fluxes;
 * the clamp belongs to the cost function alone, solve_adept.cpp:107-116) */
int ecckd_opt_forward_ex(ecckd_opt* opt, const double* h_x, int unclamped, double* h_od, double* h_flux);
int ecckd_opt_coefficients(ecckd_opt* opt, const double* h_x, int gas, double* h_molar_abs);
/* Handles made with ECCKD_OPT_RAYLEIGH_ACTIVE.  The prior of the ng Rayleigh elements: with prior_error = sigma > 0
 * J_b += 0.5 sum_g d_g^2 / sigma^2 and dJ_b/dx_g = d_g / sigma^2, d = x - ln(first guess) on the unpinned elements; <= 0: no
 * prior term on them.  The gradient IS included: the reference adds this term to the cost and drops its gradient
 * (ckd_model.cpp:869-874), and a cost whose gradient omits one of its terms is not a minimisation.  The term follows add_prior
 * of ecckd_opt_set_allreduce as the gases' prior does.  Refused (ECCKD_PARAMETER_ERROR) on a handle without the flag. */
int ecckd_opt_set_rayleigh_prior(ecckd_opt* opt, double prior_error);
/* Longwave handles, with or without nangle: the flux profile of every g point at every half level enters the cost (not in the
 * reference; the per-g twin of flux_profile_weight, the truth is what `lw_spectra gpoints=` writes).  Every column adds
 *   J_gp = weight sum_{i=0..nlay} hw_i sum_g [((dn[i][g] - rel_dn[i][g]) - T_dn[i][g])^2 + ((up[i][g] - rel_up[i][g]) - T_up[i][g])^2]
 *   hw_i = 0.5 (lw[i-1] + lw[i]) for 1 <= i <= nlay-1,  hw_0 = 0.5 lw[0],  hw_nlay = 0.5 lw[nlay-1]
 * with lw the column's normalised layer weights (sum_i hw_i = 1), dn and up the per-g fluxes of the forward model (after clamp
 * and penalty, summed over the angles when nangle > 0), rel the scene's relative_flux_* or 0, and T = h_truth, [columns of all
 * scenes in scene order][2: dn, up][nlay+1][ng] - the layout of h_flux of ecckd_opt_forward.  With relative_to the caller passes
 * truth minus the relative-to scene's truth, the convention of flux_dn.  The gradient is hand-derived: the reversed recurrences
 * receive 2 weight hw_i residual on dn_bar[i] / up_bar[i] (each angle scaled by wgt_k).  Nothing else in the cost changes, every
 * sum keeps a fixed order, cost and gradient stay bitwise reproducible.  weight <= 0 or h_truth == NULL removes the term and frees
 * its device block: the handle is then the handle it was, bit for bit.  ecckd_opt_forward_plan reports the same fields for a handle
 * with the term; of the cell-parallel kernel it runs the instance <nc_template, longwave, nb, with the term>.  Profile-sharded ranks
 * pass the truth of their own columns.  Refused with ECCKD_PARAMETER_ERROR: a shortwave handle, either ECCKD_OPT_RAYLEIGH flag, a
 * weight or (where the term is set) a truth value that is not finite. */
int ecckd_opt_set_gpoint_truth(ecckd_opt* opt, double weight, const double* h_truth);
/* h_coeff[ng] = rayleigh_molar_scattering at state h_x: exp of the state's tail (0 where pinned) for a handle made with
 * ECCKD_OPT_RAYLEIGH_ACTIVE, formed on the device by the kernel that feeds the forward model, so these are the numbers the
 * cost at h_x was computed from, bit for bit; the model's own values for any other handle or h_x = NULL.  Refused if the model
 * has none. */
int ecckd_opt_rayleigh_coefficients(ecckd_opt* opt, const double* h_x, double* h_coeff);
/* The shape of the fixed-order reduction that forms the Rayleigh gradient elements: first-level waves add chunk_rows
 * consecutive rows each (nrows rows: the cells of a plain handle, the columns of a scattering one) into npart partials per
 * g point, then finish_waves waves per 64 g points add ceil(npart / finish_waves) partials each, `batch` loads per round.
 * active = 0 (and nrows = npart = 0) for a handle without ECCKD_OPT_RAYLEIGH_ACTIVE. */
typedef struct {
  int active, chunk_rows, finish_waves, batch;
  size_t nrows, npart;
} ecckd_rayleigh_plan;
int ecckd_opt_rayleigh_plan(ecckd_opt* opt, ecckd_rayleigh_plan* plan);
/* status follows adept::MinimizerStatus: 0 success, 2 max iterations, 3 failed to converge,
 * >= 6 anomalous (optimize_lut.cpp:315-319 exits 1 for those) */
int ecckd_opt_minimize(ecckd_opt* opt, int max_iterations, double convergence_criterion, int is_bounded,
                       double* h_x, int* status, int* n_iterations, double* J_final, double* gnorm_final);

/* Profile-sharded optimisation over several GPUs (optimize_lut row, "profiles sharded"): the cost
 * function is a sum over training profiles (calc_cost_function_and_gradient accumulates it profile by profile,
 * solve_adept.cpp:157), so every rank creates its handle from ITS share of the columns of every scene and the
 * ranks only have to agree on  sum_ranks [dJ/dx (nx doubles), J]  after each evaluation.  `fn` is called once per
 * evaluation with that device buffer (count = nx + 1 doubles; the context's stream is idle when it is called)
 * and must return 0 after summing it in place over the ranks - one RCCL all-reduce (ecckd_amd/shard.py makes
 * the callback from torch.distributed).  The prior term (CkdModel::calc_background_cost_function) is not a sum over
 * profiles: exactly one rank passes add_prior = 1.  With identical reduced values on every rank the L-BFGS
 * iterations of ecckd_opt_minimize take the same decisions everywhere, so every rank returns the same state.
 * fn == NULL restores single-GPU behaviour.  ecckd_opt_forward never calls fn. */
typedef int (*ecckd_allreduce_fn)(void* d_buf, size_t count, void* stream, void* user);
int ecckd_opt_set_allreduce(ecckd_opt* opt, ecckd_allreduce_fn fn, void* user, int add_prior);

/* ecckd_opt_minimize over a cost function and gradient supplied by the caller (host arrays) instead of the library's
 * kernels: the L-BFGS iteration, its bounds and its line search stay exactly the library's.  With the reference's own
 * CkdOptimizable::calc_cost_function_gradient (solve_adept.cpp:240-292) behind fn this runs the library's minimizer over
 * the reference's cost function; the parity tests put the CPU oracle there and compare the two trajectories.
 * fn returns 0, or non-zero to abort (PROCESSING_ERROR).  fn == NULL restores the device evaluation. */
typedef int (*ecckd_evaluator_fn)(size_t nx, const double* h_x, double* J, double* h_grad, void* user);
int ecckd_opt_set_evaluator(ecckd_opt* opt, ecckd_evaluator_fn fn, void* user);

/* The minimizer's progress line and the three timed activities of the reference (solve_adept.cpp:216-218 "minimizer",
 * "a-priori", "radiative transfer"; report_progress :295-299 "Iteration n: cost function = ..., gradient norm = ...").
 * fn is called once per L-BFGS iteration of ecckd_opt_minimize, on the calling thread.  Setting it also starts the
 * activity timers (HIP events around the kernels: "radiative transfer" = look-up + sweeps + cost + their adjoint,
 * "a-priori" = the gradient kernel that carries the prior term, "minimizer" = the rest of ecckd_opt_minimize). */
typedef void (*ecckd_progress_fn)(int iteration, double cost, double gradient_norm, void* user);
int ecckd_opt_set_progress(ecckd_opt* opt, ecckd_progress_fn fn, void* user);
int ecckd_opt_timings(ecckd_opt* opt, double* minimizer_s, double* a_priori_s, double* radiative_transfer_s);

/* ---- run_ckd -------------------------------------------------------
 * Replaces the compute part of run_ckd.cpp:27-373 for the profiles of one scene (flux arrays
 * of the scene are ignored; mu0 and tsi are used for a shortwave model, run_ckd.cpp:92,:358
 * passes REFERENCE_COS_SZA).  Outputs, any of which may be NULL:
 *   h_od[ncol][nlay][ng]           sum of the gases' optical depths, clamped at 0 ("optical_depth", :318)
 *   h_rayleigh_od[ncol][nlay][ng]  shortwave only ("rayleigh_optical_depth")
 *   h_planck_hl[ncol][nlay+1][ng]  longwave "planck_hl" (row nlay = "planck_surf"); shortwave: row 0 of
 *                                  every column = "incoming_sw" = tsi / sum(ssi) * ssi
 *   h_flux[ncol][2][nlay+1][ng]    longwave: [0] = spectral_flux_dn_lw, [1] = spectral_flux_up_lw;
 *                                  shortwave: [0] = spectral_flux_dn_direct_sw, [1] = 0
 * Gases absent from the scene (gas_present[i] == 0) are skipped like run_ckd's "gases" list (:270-276);
 * call once per gas with a one-hot gas_present for the "<gas>_optical_depth" variables. */
int ecckd_run_ckd(ecckd_ctx* ctx, const ecckd_opt_model* model, const ecckd_opt_scene* scene, double* h_od,
                  double* h_rayleigh_od, double* h_planck_hl, double* h_flux);

/* ---- resident gas optics: a CKD model applied to columns in device memory -----------
 * Replaces CkdModel::calc_optical_depth (ckd_model.cpp:925-1102) and calc_planck_function (:1107-1145) for a host model
 * whose columns already sit on the device.  ecckd_gas_optics_create validates the model with the model part of
 * ecckd_opt_create's check (logarithmic interpolation is refused; min_molar_abs, max_molar_abs and is_active are ignored;
 * at most 32 gases) and uploads it once: all gases' tables in model order, the temperature grid, the Planck look-up table
 * or the Rayleigh coefficients (the solar irradiance stays on the host: only ecckd_gas_optics_incoming reads it).  Device
 * memory comes from the context's caching allocator.  The handle keeps no per-call state: calls of any shape may follow each
 * other, and a cell's result is a pure function of that cell's inputs and the model - the same bits whatever ncol, the cell's
 * place in the batch, or the calls before.
 *
 * ecckd_gas_optics_dev: one launch on the context's stream, no host wait (the host arrays are read before it returns).
 *   d_pressure_hl, d_temperature_hl [ncol][nlay+1]; d_temperature_fl [ncol][nlay] or NULL = the pressure-weighted mean of
 *   temperature_hl; d_vmr_fl [ncol][ngas][nlay] in model gas order - device doubles in the layouts of ecckd_opt_scene.
 *   h_gas_present[ngas] (NULL = all): a gas with 0 contributes nothing whatever its concentration dependence (run_ckd's
 *   rule, run_ckd.cpp:270-276); h_gas_scaling[ngas] (NULL = 1) multiplies the gas's mole fraction first.
 *   Outputs: device arrays [ncol][nlay][ng], g fastest, of out_type ECCKD_F64 or ECCKD_F32 (the double result rounded once):
 *   d_od the sum of the gases in model order; h_d_gas_od a host array of ngas device pointers, NULL entries or a NULL array
 *   skipped, every gas out of the same pass (an absent gas gives zeros); d_rayleigh_od, shortwave handles only,
 *   moles_per_layer * rayleigh_molar_scattering[g], zeros for a model without coefficients.  Any of them may be NULL, not all.
 *   Per cell: ln of the mean pressure, the pressure axis position held inside the table (the n - 1.0001 rule), the
 *   temperature axis on the table column interpolated at that pressure, for conc_dependence 2 the log-concentration axis;
 *   weight MOLES_PER_PA dp, times vmr, or times (vmr - reference_vmr); per gas one FMA chain over its 4 or 8 nodes.
 *   keep_negative 0: the SUM is clamped at 0 and each per-gas output on its own; 1: nothing is clamped.
 *   ECCKD_PARAMETER_ERROR: NULL pressure or temperature, non-positive sizes, d_rayleigh_od on a longwave handle, d_vmr_fl ==
 *   NULL with a concentration-dependent gas present, out_type or keep_negative outside their values, no output.
 * ecckd_gas_optics_planck_dev: d_planck[n][ng] at d_temperature[n], linear in the look-up table, (t / t0) * row 0 below it,
 *   extrapolated from the last two rows above it; refused on a shortwave handle.
 * ecckd_gas_optics_incoming: h_incoming[ng] = tsi / sum(ssi) * ssi (host only); refused on a longwave handle.
 * ecckd_gas_optics_geometry (host only): the launch tile - consecutive cells of the flattened (column, layer) index per
 *   block, threads per block - for tests that place their sizes at its edges. */
typedef struct ecckd_gas_optics ecckd_gas_optics;
int ecckd_gas_optics_create(ecckd_ctx* ctx, const ecckd_opt_model* model, ecckd_gas_optics** gas_optics);
int ecckd_gas_optics_destroy(ecckd_gas_optics* gas_optics);
int ecckd_gas_optics_info(ecckd_gas_optics* gas_optics, int* ng, int* ngas, int* is_sw, int* entries_per_cell);
int ecckd_gas_optics_geometry(ecckd_gas_optics* gas_optics, int* cells_per_block, int* threads);
int ecckd_gas_optics_dev(ecckd_gas_optics* gas_optics, int ncol, int nlay, const double* d_pressure_hl,
                         const double* d_temperature_hl, const double* d_temperature_fl, const double* d_vmr_fl,
                         const int* h_gas_present, const double* h_gas_scaling, int keep_negative, int out_type, void* d_od,
                         void* const* h_d_gas_od, void* d_rayleigh_od);
int ecckd_gas_optics_planck_dev(ecckd_gas_optics* gas_optics, size_t n, const double* d_temperature, int out_type,
                                void* d_planck);
int ecckd_gas_optics_incoming(ecckd_gas_optics* gas_optics, double tsi, double* h_incoming);

/* ---- resident fluxes: device columns to fluxes and heating rates in one launch ---------
 * The per-time-step call of a host model: from the inputs of ecckd_gas_optics_dev to broadband, band and per-g fluxes and
 * heating rates on the device.  No [ncol][nlay][ng] array is written, nothing is copied to the host, and the only memory used
 * beside the outputs is the context's scratch (which grows once and stops growing with ncol when the grid is saturated).  The
 * call is queued on the context's stream and does not wait; the host arrays are read before it returns.
 * Per (column, g point): the optical depth of every layer exactly as ecckd_gas_optics_dev forms it (keep_negative = 0: the
 * total clamped at 0), on shortwave handles moles_per_layer * rayleigh[g] beside it; the Planck function at the half levels as
 * ecckd_gas_optics_planck_dev forms it; then
 *   longwave                ecckd_rt_lw_gpoints(nangle): unit emissivity, surface Planck function = row nlay
 *   shortwave, scattering 0 ecckd_rt_sw_gpoints on max(od, 0) + rayleigh_od: the direct beam and its Lambertian reflection
 *   shortwave, scattering 1 ecckd_rt_sw_gpoints_rayleigh: the two-stream transfer with Rayleigh scattering
 * with incoming[g] = tsi / sum(ssi) * ssi[g], d_cos_sza[ncol] and d_albedo[ncol] (NULL = 0) per column.  A column whose
 * cos_sza is not positive gets zeros in every output.  Sums over g (broadband, and per band of iband_per_g) run over g in
 * ascending order, whatever the batch, the grid or the column's place: a column's results are a pure function of that column
 * and the model.  heating_rate[l] = -(g / cp) / (p[l+1] - p[l]) * (dn[l+1] - dn[l] - up[l+1] + up[l]) in K s-1 from the
 * broadband doubles (heating_rate_single, heating_rate.h:55-72), before any rounding to float.
 * ecckd_flux_outputs: device pointers, any may be NULL, not all; every array of out_type ECCKD_F64 or ECCKD_F32 (the double
 * result rounded once).  With scattering = 0 flux_dn / band_flux_dn / spectral_flux_dn hold the direct beam and the *_direct
 * fields must be NULL; with scattering = 1 they hold direct plus diffuse and the *_direct fields the beam.  nband = 1 +
 * max(iband_per_g); a model created without iband_per_g refuses the band outputs.
 * ECCKD_PARAMETER_ERROR, each with its own message: the wrong kind of handle, nangle outside 0..16, scattering outside {0, 1},
 * scattering = 1 on a model without Rayleigh coefficients, *_direct outputs with scattering = 0 or on a longwave call, no
 * output, NULL inputs, d_vmr_fl == NULL with a concentration-dependent gas present, a bad out_type, a shape the plan refuses
 * (non-positive sizes, more than 160 KB of LDS per block).
 * ECCKD_GAS_OPTICS_FLUXES_GRID = N (>= 1), read per call, forces N blocks in place of 3 per compute unit.
 * ecckd_gas_optics_fluxes_geometry (host only; mode 0 longwave, 1 shortwave direct, 2 shortwave two-stream): whole columns per
 * block, threads per block, layers per tile and the scratch of a saturated grid, for tests that sit on the edges.
 * ecckd_gas_optics_fluxes_plan (host only, no handle): the launch plan as a function of the shape alone; `wants` is a bit set
 * (1 broadband, 2 bands, 4 spectral, 8 heating rate, 16 direct); a refusal returns ECCKD_PARAMETER_ERROR and its message
 * in `message` (message_bytes including the terminator). */
typedef struct {
  void *flux_dn, *flux_up;                    /* [ncol][nlay+1]          broadband                                   */
  void *band_flux_dn, *band_flux_up;          /* [ncol][nlay+1][nband]   by iband_per_g                              */
  void *spectral_flux_dn, *spectral_flux_up;  /* [ncol][nlay+1][ng]                                                  */
  void *heating_rate;                         /* [ncol][nlay] K s-1                                                  */
  void *flux_dn_direct, *band_flux_dn_direct, *spectral_flux_dn_direct;   /* shortwave, scattering = 1 only          */
} ecckd_flux_outputs;
typedef struct {
  int columns_per_block, layer_tile, threads, g_passes;   /* g_passes > 1: ng > threads, a block loops over g */
  int state_rows, reduce_levels;                          /* per-thread scratch rows of nlay+1 doubles; levels per LDS reduction */
  unsigned grid;
  size_t ngroup, lds_bytes, scratch_bytes;
} ecckd_flux_plan;
int ecckd_gas_optics_fluxes_lw_dev(ecckd_gas_optics* gas_optics, int nangle, int ncol, int nlay, const double* d_pressure_hl,
                                   const double* d_temperature_hl, const double* d_temperature_fl, const double* d_vmr_fl,
                                   const int* h_gas_present, const double* h_gas_scaling, int out_type,
                                   const ecckd_flux_outputs* out);
int ecckd_gas_optics_fluxes_sw_dev(ecckd_gas_optics* gas_optics, int scattering, int ncol, int nlay, const double* d_pressure_hl,
                                   const double* d_temperature_hl, const double* d_temperature_fl, const double* d_vmr_fl,
                                   const int* h_gas_present, const double* h_gas_scaling, const double* d_cos_sza,
                                   const double* d_albedo, double tsi, int out_type, const ecckd_flux_outputs* out);
/* Resident fluxes under clouds and over a real surface: the two calls above with one more argument.  `sky` == NULL, or a
 * struct whose pointers are all NULL, runs the kernel of the clear call itself (the same bits); otherwise
 *   longwave   tau[l][g] = max(gas total, 0) + cloud_od[col][l][band(g)] (a cloud value that is not > 0 adds nothing; the
 *              absorption optical depth: longwave scattering is not treated).  All angles' down sweeps run first; every angle's
 *              up sweep starts from the Lambertian surface eps * B_skin + (1 - eps) * dn[nlay] with dn[nlay] the angle-summed
 *              flux, eps = surface_emissivity[col][band(g)] (NULL = 1) and B_skin the Planck function at skin_temperature[col]
 *              (NULL = temperature_hl[nlay]); the base of the bottom layer keeps temperature_hl[nlay].
 *   shortwave  always the two-stream transfer (the model must carry Rayleigh coefficients).  A layer whose cloud_od is > 0
 *              mixes (od, ssa, asymmetry) of its band into the gas: tau = tau_abs + tau_ray + t', sc = tau_ray + w' t',
 *              ssa = sc / tau, g = w' t' a' / sc, with ecRad's shortwave coefficients g1 = 2 - ssa (1.25 + 0.75 g),
 *              g2 = ssa (0.75 - 0.75 g), g3 = 0.5 - 0.75 g mu0, g4 = 1 - g3 in Meador and Weaver's closed form and the adding
 *              method of the clear call.  delta_eddington = 1: f = a a, t' = t (1 - w f), w' = w (1 - f) / (1 - w f),
 *              a' = a / (1 + a) formed in the kernel; 0: the inputs are used as they are.  Any other layer is the clear layer.
 * A g point takes the cloud and surface values of its band, iband_per_g[g]; nband = 1 + max(iband_per_g).  "Cloud" is any
 * particulate (aerosols are merged by the caller); columns are independent (McICA sub-columns are columns).  The values are
 * taken as they are: ssa and asymmetry are not validated on the device.
 * ECCKD_PARAMETER_ERROR, each with its own message, beside the refusals of the clear calls: a band-indexed input (cloud_*,
 * surface_emissivity) on a model created without iband_per_g; shortwave: cloud_od without cloud_ssa or cloud_asymmetry or
 * either without cloud_od, surface_emissivity, skin_temperature; longwave: cloud_ssa, cloud_asymmetry, delta_eddington != 0;
 * delta_eddington outside {0, 1}. */
typedef struct {
  const double* cloud_od;            /* [ncol][nlay][nband] device; NULL = no cloud.  SW: extinction; LW: absorption      */
  const double* cloud_ssa;           /* [ncol][nlay][nband] shortwave only: single-scattering albedo                      */
  const double* cloud_asymmetry;     /* [ncol][nlay][nband] shortwave only: asymmetry factor                              */
  const double* surface_emissivity;  /* [ncol][nband] longwave only; NULL = 1                                             */
  const double* skin_temperature;    /* [ncol] longwave only; NULL = temperature_hl[nlay]                                 */
  int delta_eddington;               /* shortwave: 1 = scale (od, ssa, g) in the kernel, 0 = they are already scaled       */
} ecckd_flux_sky;
int ecckd_gas_optics_fluxes_lw_sky_dev(ecckd_gas_optics* gas_optics, int nangle, int ncol, int nlay, const double* d_pressure_hl,
                                       const double* d_temperature_hl, const double* d_temperature_fl, const double* d_vmr_fl,
                                       const int* h_gas_present, const double* h_gas_scaling, int out_type,
                                       const ecckd_flux_outputs* out, const ecckd_flux_sky* sky);
int ecckd_gas_optics_fluxes_sw_sky_dev(ecckd_gas_optics* gas_optics, int ncol, int nlay, const double* d_pressure_hl,
                                       const double* d_temperature_hl, const double* d_temperature_fl, const double* d_vmr_fl,
                                       const int* h_gas_present, const double* h_gas_scaling, const double* d_cos_sza,
                                       const double* d_albedo, double tsi, int out_type, const ecckd_flux_outputs* out,
                                       const ecckd_flux_sky* sky);
int ecckd_gas_optics_fluxes_geometry(ecckd_gas_optics* gas_optics, int nlay, int mode, int* columns_per_block, int* threads,
                                     int* layer_tile, size_t* scratch_bytes);
int ecckd_gas_optics_fluxes_plan(long long ncol, int nlay, int ng, int nent, int nband, int mode, int nangle, unsigned wants,
                                 int cu_count, long long grid_override, ecckd_flux_plan* plan, char* message, size_t message_bytes);

/* ---- scale_lut -----------------------------------------------------
 * scale_lut.cpp:117-133 needs, per g point, the sum over its wavenumbers of every row of a
 * (nrows, nwav) matrix (the LBL direct-beam spectral flux at each half level): h_sums[nrows][ng].
 * Declared below, after ecckd_gmap: ecckd_gmap_sum_rows.
 *
 * ecckd_scale_lut does the rest of scale_lut.cpp:117-189 and CkdModel::scale_optical_depth
 * (ckd_model.cpp:1151-1176) for one reference profile: od_best = -mu0 log(flux_base / flux_top) per layer
 * and g point (-1 where the flux has vanished), od_total from the CKD model (NOT clamped at zero,
 * plain-mean full-level temperature), scaling = od_best / od_total (1 where od_best <= 0), interpolated in
 * log pressure to the model's grid (adept::interp restated as linear interpolation with linear
 * extrapolation) and applied to every gas, clamped to [min, max] where those exist.
 *   h_vmr_fl[ngas][nz] in model gas order; gas_present[ngas] = gas is in the LBL file's constituent list
 *   (or is "composite"); h_scaling[nz][ng] (optional output); h_molar_abs_out[ngas] = caller buffers shaped
 *   like each gas's molar_abs. */
int ecckd_scale_lut(ecckd_ctx* ctx, const ecckd_opt_model* model, int nz, const double* h_pressure_hl,
                    const double* h_temperature_hl, const double* h_vmr_fl, const int* gas_present, double mu0,
                    const double* h_flux_sums, double* h_scaling, double* const* h_molar_abs_out);

/* ---- create_look_up_table (K6/K7) ----------------------------------------------
 * A g-point map: the wavenumbers sorted by g point once (stable), so that every g point is a
 * contiguous segment.  d_g_point[nwav] as read from the g-points file (-1 = unassigned,
 * create_look_up_table.cpp:92-106); wavenumbers must ascend. */
typedef struct ecckd_gmap ecckd_gmap;
int ecckd_gmap_create(ecckd_ctx* ctx, size_t nwav, const int32_t* d_g_point, int ng,
                      const double* d_wavenumber, const double* d_d_wavenumber, ecckd_gmap** gmap);
int ecckd_gmap_destroy(ecckd_gmap* gmap);
/* wavenumbers per g point: zero = "occupies none of the spectrum" (create_look_up_table.cpp:111-118) */
int ecckd_gmap_counts(ecckd_gmap* gmap, int64_t* h_counts);

/* Replaces average_optical_depth_to_g_point (average_optical_depth.cpp:22-197) for one column:
 * weights are the Planck function at h_temperature_fl[nlay] (longwave,
 * create_look_up_table.cpp:316-327) or d_ssi[nwav] (shortwave, :335); exactly one of the two
 * must be given.  Outputs (nlay, ng) row-major; min/max may be NULL.  reference_surface_vmr <= 0
 * returns optical depths instead of molar absorption (:186-193). */
int ecckd_average_to_gpoints(ecckd_gmap* gmap, int nlay, const double* h_pressure_hl,
                             const double* h_temperature_fl, const double* d_ssi,
                             const void* d_od, int od_type, size_t od_stride, int averaging_method,
                             double reference_surface_vmr, double* h_molar_abs,
                             double* h_min_molar_abs, double* h_max_molar_abs);
/* h_sums[nrows][ng] = sum over the wavenumbers of each g point of d_rows[r][.] (scale_lut.cpp:119-124) */
int ecckd_gmap_sum_rows(ecckd_gmap* gmap, int nrows, const void* d_rows, int rows_type, size_t row_stride,
                        double* h_sums);
/* Line-by-line longwave fluxes of one column resolved per g point (lw_spectra.cpp:222-257): planck_function
 * (planck_function.cpp:22-54) + radiative_transfer_lw (radiative_transfer_lw.cpp:27-60, unit surface emissivity, surface
 * Planck function at temperature_hl(end), diffusivity 1.66 - the arithmetic of ecckd_lbl_band_fluxes_lw) and, in the same pass
 * over the optical depths, h_flux_*[nlay+1][ng] = the sum of the spectral flux at each half level over the wavenumbers of each
 * g point (exactly 0 for a g point without wavenumbers); h_bb_*[nlay+1] (may be NULL) = the sum over ALL wavenumbers, those
 * with g_point = -1 included.  No (nlay+1) x nwav flux matrix is formed.  Bitwise reproducible.  The per-block accumulator
 * (2 (nlay+1) x g points of doubles in 42 KB of LDS) bounds both entry points: nlay above 1 343 is refused with
 * PARAMETER_ERROR, and a map with more g points than fit (47 at nlay = 54) is swept in ceil((ng + 1) / columns) launches, each
 * repeating the radiative transfer. */
int ecckd_lbl_gpoint_fluxes_lw(ecckd_gmap* gmap, int nlay, const double* h_temperature_hl, const void* d_od, int od_type,
                               size_t od_stride, double* h_flux_dn, double* h_flux_up, double* h_bb_dn, double* h_bb_up);
/* The same kernel's other output: the spectral fluxes themselves, d_flux_dn / d_flux_up[nlay+1][flux_stride] FLOAT device
 * rows (what lw_spectra writes without g points, lw_spectra.cpp:236-237), and the broadband sums h_bb_*[nlay+1] (may be
 * NULL) of the DOUBLE fluxes. */
int ecckd_lbl_spectral_fluxes_lw(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_temperature_hl,
                                 const double* d_wavenumber, const double* d_d_wavenumber, const void* d_od, int od_type,
                                 size_t od_stride, float* d_flux_dn, float* d_flux_up, size_t flux_stride, double* h_bb_dn,
                                 double* h_bb_up);
/* Both with the zenith-angle quadrature of ecckd_lbl_band_fluxes_lw_angles: nangle = 0 is the two entry points above, bit for
 * bit; nangle = N in 1..16 integrates N Gauss-Legendre angles per hemisphere, flux = sum_k 2 w_k mu_k L(mu_k) formed in angle
 * order per wavenumber and level before it is binned or written.  A thread carries the N intensities of its wavenumber through
 * ONE walk of the layers (one load of the optical depth and one Planck function per level for all angles), so the
 * accumulator, the limits and the launch split above do not depend on nangle.  nangle outside 0..16: PARAMETER_ERROR before
 * any launch. */
int ecckd_lbl_gpoint_fluxes_lw_angles(ecckd_gmap* gmap, int nangle, int nlay, const double* h_temperature_hl, const void* d_od,
                                      int od_type, size_t od_stride, double* h_flux_dn, double* h_flux_up, double* h_bb_dn,
                                      double* h_bb_up);
int ecckd_lbl_spectral_fluxes_lw_angles(ecckd_ctx* ctx, int nangle, int nlay, size_t nwav, const double* h_temperature_hl,
                                        const double* d_wavenumber, const double* d_d_wavenumber, const void* d_od, int od_type,
                                        size_t od_stride, float* d_flux_dn, float* d_flux_up, size_t flux_stride, double* h_bb_dn,
                                        double* h_bb_up);
/* Line-by-line shortwave fluxes of one column resolved per g point, for nsza (1..8) solar zenith angles in one call:
 * radiative_transfer_direct_sw / _norayleigh_sw (radiative_transfer_sw.cpp:26-77, the arithmetic of ecckd_lbl_band_fluxes_sw) and,
 * in the same pass over the optical depths, h_flux_*[nsza][nlay+1][ng] = the sum of the spectral flux at each half level over
 * the wavenumbers of each g point (exactly 0 for a g point without wavenumbers); h_bb_*[nsza][nlay+1] (may be NULL) = the sum over
 * ALL wavenumbers, those with g_point = -1 included.  d_albedo[nwav] is the surface albedo per wavenumber; NULL: no upwelling
 * sweep, h_flux_up and h_bb_up exactly 0.  exp(-2 tau) of the upwelling sweep is evaluated once for all angles of a launch;
 * angle s of a call has the bits of a single-angle call with h_cos_sza[s].  Bitwise reproducible.  The per-block accumulator
 * (angles x 2 (nlay+1) x columns of doubles in 58 KB of LDS) is filled in several launches where it does not fit: angles are
 * split first, then g points (ng = 32 at nlay = 54, five angles: 3 launches).  PARAMETER_ERROR: nsza outside 1..8, a cos_sza
 * outside (0, 1], nlay above 1 855. */
int ecckd_lbl_gpoint_fluxes_sw(ecckd_gmap* gmap, int nlay, int nsza, const double* h_cos_sza, const double* d_ssi,
                               const double* d_albedo, const void* d_od, int od_type, size_t od_stride, double* h_flux_dn_direct,
                               double* h_flux_up, double* h_bb_dn, double* h_bb_up);
/* The same kernel's other output: the spectral fluxes themselves, d_flux_dn_direct / d_flux_up[nsza][nlay+1][flux_stride] FLOAT
 * device rows (d_flux_up all 0 without an albedo), and the broadband sums h_bb_*[nsza][nlay+1] (may be NULL) of the DOUBLE
 * fluxes. */
int ecckd_lbl_spectral_fluxes_sw(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_cos_sza, const double* d_ssi,
                                 const double* d_albedo, const void* d_od, int od_type, size_t od_stride, float* d_flux_dn_direct,
                                 float* d_flux_up, size_t flux_stride, double* h_bb_dn, double* h_bb_up);
/* The same per g point WITH Rayleigh scattering: the two-stream transfer of ecckd_lbl_band_fluxes_sw_rayleigh (d_od_abs
 * absorbs, d_od_ray scatters; each FLOAT or DOUBLE with its own stride) per wavenumber and, in the same pass,
 * h_flux_dn_direct / h_flux_dn (direct plus diffuse) / h_flux_up[nsza][nlay+1][ng] = the sums over the wavenumbers of each g
 * point (exactly 0 for a g point without wavenumbers); h_bb_*[nsza][nlay+1] (each may be NULL) = the sums over ALL
 * wavenumbers, those with g_point = -1 included.  d_albedo = NULL is albedo 0.  One angle per launch: angle s of a call has
 * the bits of a single-angle call with h_cos_sza[s].  Bitwise reproducible, whatever ECCKD_RAYLEIGH_GRID bounds the grid to.
 * The per-block accumulator (3 (nlay+1) x columns of doubles in 58 KB of LDS) is filled in ceil((ng + 1) / columns) launches
 * per angle where it does not fit (44 columns at nlay = 54), each repeating the transfer.  PARAMETER_ERROR: nsza outside
 * 1..8, a cos_sza outside (0, 1], an od type that is not 4 or 8, a stride below nwav, nlay above 1 236. */
int ecckd_lbl_gpoint_fluxes_sw_rayleigh(ecckd_gmap* gmap, int nlay, int nsza, const double* h_cos_sza, const double* d_ssi,
                                        const double* d_albedo, const void* d_od_abs, int abs_type, size_t abs_stride,
                                        const void* d_od_ray, int ray_type, size_t ray_stride, double* h_flux_dn_direct,
                                        double* h_flux_dn, double* h_flux_up, double* h_bb_dn_direct, double* h_bb_dn, double* h_bb_up);
/* The same kernel's other output: the spectral fluxes themselves, d_flux_dn_direct / d_flux_dn / d_flux_up[nsza][nlay+1]
 * [flux_stride] FLOAT device rows, and the broadband sums h_bb_*[nsza][nlay+1] (each may be NULL) of the DOUBLE fluxes. */
int ecckd_lbl_spectral_fluxes_sw_rayleigh(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_cos_sza, const double* d_ssi,
                                          const double* d_albedo, const void* d_od_abs, int abs_type, size_t abs_stride,
                                          const void* d_od_ray, int ray_type, size_t ray_stride, float* d_flux_dn_direct,
                                          float* d_flux_dn, float* d_flux_up, size_t flux_stride, double* h_bb_dn_direct,
                                          double* h_bb_dn, double* h_bb_up);
/* LblFluxes::read, lbl_fluxes.cpp:198-230: the square root of the erythemal action spectrum (Webb et al.
 * 2011) averaged over each g point with a 5777 K Planck weight, h_erythemal[ng]; NaN for an empty g point
 * (0/0 as in the reference). */
int ecckd_gmap_erythemal_spectrum(ecckd_gmap* gmap, double* h_erythemal);
/* create_look_up_table.cpp:537-548: h_gpoint_fraction[ng][nint] over the coarse intervals
 * (wavenumber1, wavenumber2] */
int ecckd_gpoint_fraction(ecckd_gmap* gmap, int nint, const double* h_wavenumber1,
                          const double* h_wavenumber2, double* h_gpoint_fraction);
/* create_look_up_table.cpp:581-591: h_planck_lut[nlut][ng] */
int ecckd_planck_lut(ecckd_gmap* gmap, int nlut, const double* h_temperature_lut, double* h_planck_lut);

/* ---- find_g_points: spectral overlap of the gases (a14) ----------------------
 * ecckd_overlap_g_points replaces overlap_g_points (single_gas_data.cpp:24-124), host-side:
 *   h_n_g_points[ngas][nband]; h_sorting_variable = the gases' per-g-point median sorting
 *   variables concatenated, gas i starting at h_gas_offset[i]; outputs *h_ng,
 *   h_band_number[capacity], h_g_min/h_g_max[ngas][capacity].
 * ecckd_gas_g_point_dev replaces SingleGasData::store_g_points (single_gas_data.h:56-62);
 * ecckd_merge_g_points_dev replaces find_g_points.cpp:1459-1475 (h_d_gas_g_point: host array
 * of ngas device pointers; g_min/g_max rows have `stride` elements). */
int ecckd_overlap_g_points(int ngas, int nband, const int* h_n_g_points, const int* h_gas_offset,
                           const double* h_sorting_variable, int capacity, int* h_ng,
                           int* h_band_number, int* h_g_min, int* h_g_max);
int ecckd_gas_g_point_dev(ecckd_ctx* ctx, size_t nwav, const int32_t* d_rank, int ng,
                          const int32_t* h_rank1, const int32_t* h_rank2, int32_t* d_g_point);
int ecckd_merge_g_points_dev(ecckd_ctx* ctx, size_t nwav, int ngas,
                             const int32_t* const* h_d_gas_g_point, int ng, int stride,
                             const int* h_g_min, const int* h_g_max, int32_t* d_g_point,
                             int64_t* h_n_unassigned);

/* ---- the cloud pseudo-gas (shortwave) ------------------------------------------
 * ecckd_cloud_sorting_variable_dev replaces reorder_cloud_spectrum.cpp:111-123: the absorptance
 * of an optically thick cloud, 1-(1-a)/(1+a) with a = sqrt((1-ssa_de)/(1-ssa_de*asymmetry_de)),
 * ssa_de = ssa*(1-g*g)/(1-ssa*g*g) and asymmetry_de = 1/(1+g) as the reference writes it, on the
 * Mie grid h_cloud_wavenumber[nknot] (strictly ascending, else ECCKD_PARAMETER_ERROR) from one
 * size bin h_ssa[nknot], h_asymmetry[nknot]; then adept::interp onto d_wavenumber[nwav] (linear,
 * extrapolated linearly outside the knots) -> d_sorting_variable[nwav].  Every operation is
 * rounded on its own: the keys equal a plain double-precision restatement bit for bit.  The
 * per-band stable sort of :150-188 is ecckd_stable_argsort_bands_dev.
 * ecckd_cloud_partition_dev replaces find_g_points.cpp:586-636 (the equal-solar-energy branch):
 * per band [h_band_begin[b], h_band_end[b]] (ascending, non-empty), ng_b = int((max-min of
 * the sorting variable)/max_reflectance_range) + 1 g points, each the rank range over which the
 * running sum of d_ssi in rank order (d_rank from the ordering file) lies in [jg*d, (jg+1)*d),
 * d = band irradiance*(1+1e-8)/ng_b.  Outputs h_n_g_points[nband], *h_ng and per g point (up to
 * capacity) h_band_number, h_rank1, h_rank2, h_error (max - min of the sorting variable) and
 * h_median (-2 + its unweighted mean).  The running sum is a blocked fp64 scan (fixed order, no
 * atomics), so a point can change g point only where the sum is within rounding of a boundary.
 * ECCKD_PARAMETER_ERROR for ssi < 0 (or NaN) anywhere, a rank outside its band or a NaN sorting
 * variable inside a band; ECCKD_PROCESSING_ERROR for a g point that holds no wavenumber (the
 * reference takes minval of an empty set there) and for more than `capacity` g points.
 * ecckd_cloud_geometry (host only) reports the tiling of these kernels: the longest Mie table
 * searched in LDS, points per thread and per tile of the scan, points per block of the g-point
 * statistics, boundary searches per block, and the points one pass of the grid-stride kernels
 * covers on ctx's device (with ctx NULL: on the 256 compute units of an MI355X). */
int ecckd_cloud_geometry(ecckd_ctx* ctx, int* lds_knots, int* scan_items, int* scan_tile,
                         int* stats_chunk, int* bounds_block, int64_t* grid_points);
int ecckd_cloud_sorting_variable_dev(ecckd_ctx* ctx, int nknot, const double* h_cloud_wavenumber,
                                     const double* h_ssa, const double* h_asymmetry, size_t nwav,
                                     const double* d_wavenumber, double* d_sorting_variable);
int ecckd_cloud_partition_dev(ecckd_ctx* ctx, size_t nwav, const double* d_ssi, const int32_t* d_rank,
                              const double* d_sorting_variable, int nband, const int64_t* h_band_begin,
                              const int64_t* h_band_end, double max_reflectance_range, int capacity,
                              int* h_n_g_points, int* h_ng, int* h_band_number, int64_t* h_rank1,
                              int64_t* h_rank2, double* h_error, double* h_median);

#ifdef __cplusplus
}
#endif
#endif
