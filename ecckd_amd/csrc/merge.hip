// merge.hip - the arithmetic of read_spectrum / read_merged_spectrum on the device:
// the wavenumber spacing derived from the grid (read_spectrum.cpp:55-65) and the merged optical depth
// sum_gas scaling(level) * optical_depth (read_merged_spectrum.cpp:117-166).  File access is the
// caller's business; these functions take the arrays the reader produced (FLOAT as stored in the CKDMIP
// files, or DOUBLE) and keep the merged matrix resident in HBM for find_g_points.
#include "common.hpp"
#include "lbl_gases.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace {

__global__ void __launch_bounds__(256)
k_derive_dwn(size_t n, const double* __restrict__ wn, double* __restrict__ dwn) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  // interior: half the distance between the neighbours; the two ends: half of their neighbour's value
  auto interior = [&](size_t i) { return 0.5 * (wn[i + 1] - wn[i - 1]); };
  double v;
  if (j == 0) v = 0.5 * interior(1);
  else if (j == n - 1) v = 0.5 * interior(n - 2);
  else v = interior(j);
  dwn[j] = v;
}

// merged[l][j] (+)= od[l][j] * scale[l]; product and sum rounded separately, as the expression
// `optical_depth += od * spread<1>(scaling_profile, n)` evaluates without contraction
template <typename T>
__global__ void __launch_bounds__(256)
k_merge(size_t n, size_t od_stride, size_t out_stride, const T* __restrict__ od, const double* __restrict__ scale,
        int first, double* __restrict__ merged) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int l = blockIdx.y;
  if (j >= n) return;
  const double v = __dmul_rn((double)od[(size_t)l * od_stride + j], scale[l]);
  double* o = merged + (size_t)l * out_stride + j;
  *o = first ? v : __dadd_rn(*o, v);
}

// ---- all gases of a scenario in one pass ----
// A thread takes MS_P consecutive wavenumbers of one layer: a FLOAT row is read 16 bytes at a time, a DOUBLE row and the merged
// row 16 bytes at a time twice.  Rows begin anywhere (strides are arbitrary and callers pass sub-views), so the windows of a
// layer begin `head` elements into the row, where gas 0's row reaches a 16-byte boundary; with equal strides and aligned
// allocations - what the tools pass - every other row and the merged row reach theirs there too.  A row that does not is read
// (the merged row: written) element by element.  Its address differs from lane to lane by a multiple of 16 bytes, so that
// choice is the whole wave's.  The head, at most 3 elements, and the windows that cross the row's end go point by point.
constexpr int MS_P = 4, MS_T = 256;

using ecckd::lbl::GasRows;

// In the two functions below the product is rounded, then the sum: they are written with * and + under `fp contract(off)`.
// __dmul_rn and __dadd_rn would not do: the compiler's header defines them as plain * and +, contractible where they are
// defined, so a sum that sees its product is fused whatever the caller asks (merged_tau, inlined here, becomes v_fmac_f64;
// k_merge above escapes through its select on `first`).  That is why the point-by-point path restates merged_tau's text
// instead of calling it.

// one point: merged_tau<1> (lbl_gases.hpp) with one scenario
__device__ __forceinline__ double merged_point(const GasRows& gr, int ngas, int nlay, int l, size_t j, const double* __restrict__ scale) {
#pragma clang fp contract(off)
  double tau = 0.0;
  for (int g = 0; g < ngas; ++g) {
    const size_t at = (size_t)l * gr.stride[g] + j;
    const double x = gr.type[g] == ECCKD_F64 ? static_cast<const double*>(gr.od[g])[at]
                                             : (double)static_cast<const float*>(gr.od[g])[at];
    const double v = x * scale[(size_t)g * nlay + l];
    tau = g == 0 ? v : tau + v;
  }
  return tau;
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((unsigned long long)p & 15ull) == 0; }

__device__ __forceinline__ void load_window(const float* __restrict__ p, double (&x)[MS_P]) {
  if (aligned16(p)) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    x[0] = (double)v.x; x[1] = (double)v.y; x[2] = (double)v.z; x[3] = (double)v.w;
  } else {
#pragma unroll
    for (int i = 0; i < MS_P; ++i) x[i] = (double)p[i];
  }
}

__device__ __forceinline__ void load_window(const double* __restrict__ p, double (&x)[MS_P]) {
  if (aligned16(p)) {
    const double2 a = *reinterpret_cast<const double2*>(p), b = *reinterpret_cast<const double2*>(p + 2);
    x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
  } else {
#pragma unroll
    for (int i = 0; i < MS_P; ++i) x[i] = p[i];
  }
}

// merged[l][j] = sum over the gases, in gas order, of od_g[l][j] * scale[g][l]: the arithmetic of merged_tau (lbl_gases.hpp) on MS_P
// points at once, and point by point outside a whole window
__global__ void __launch_bounds__(MS_T)
k_merge_scenario(size_t n, int ngas, int nlay, const GasRows gr, const double* __restrict__ scale, double* __restrict__ merged,
                 size_t out_stride) {
#pragma clang fp contract(off)
  const int l = blockIdx.y;
  double* __restrict__ out = merged + (size_t)l * out_stride;
  const unsigned long long a0 = (unsigned long long)gr.od[0] + (unsigned long long)l * gr.stride[0] * (unsigned)gr.type[0];
  size_t head = (size_t)(((16ull - (a0 & 15ull)) & 15ull) / (unsigned)gr.type[0]);   // the types are the element sizes
  if (head > n) head = n;
  if (blockIdx.x == 0 && threadIdx.x < head) out[threadIdx.x] = merged_point(gr, ngas, nlay, l, (size_t)threadIdx.x, scale);
  const size_t j0 = head + ((size_t)blockIdx.x * MS_T + threadIdx.x) * MS_P;
  if (j0 >= n) return;
  if (j0 + MS_P > n) {                          // the ragged end of the row
    for (size_t j = j0; j < n; ++j) out[j] = merged_point(gr, ngas, nlay, l, j, scale);
    return;
  }
  double acc[MS_P];
  for (int g = 0; g < ngas; ++g) {
    const size_t at = (size_t)l * gr.stride[g] + j0;
    const double sc = scale[(size_t)g * nlay + l];           // uniform: a scalar load
    double x[MS_P];
    if (gr.type[g] == ECCKD_F64) load_window(static_cast<const double*>(gr.od[g]) + at, x);
    else load_window(static_cast<const float*>(gr.od[g]) + at, x);
#pragma unroll
    for (int i = 0; i < MS_P; ++i) {
      const double v = x[i] * sc;
      acc[i] = g == 0 ? v : acc[i] + v;
    }
  }
  double* o = out + j0;
  if (aligned16(o)) {
    *reinterpret_cast<double2*>(o) = make_double2(acc[0], acc[1]);
    *reinterpret_cast<double2*>(o + 2) = make_double2(acc[2], acc[3]);
  } else {
#pragma unroll
    for (int i = 0; i < MS_P; ++i) o[i] = acc[i];
  }
}

}  // namespace

extern "C" {

int ecckd_derive_d_wavenumber_dev(ecckd_ctx* ctx, size_t nwav, const double* d_wavenumber, double* d_d_wavenumber) {
  ECCKD_REQUIRE(ctx && d_wavenumber && d_d_wavenumber, "ecckd_derive_d_wavenumber_dev: NULL argument");
  ECCKD_REQUIRE(nwav >= 3, "ecckd_derive_d_wavenumber_dev: at least 3 wavenumbers needed, got %zu", nwav);
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  hipLaunchKernelGGL(k_derive_dwn, dim3((unsigned)((nwav + 255) / 256)), dim3(256), 0, ctx->stream, nwav, d_wavenumber,
                     d_d_wavenumber);
  ECCKD_HIP_CHECK(hipGetLastError());
  return ECCKD_OK;
}

int ecckd_merge_scaling(int nlay, const double* h_pressure_hl, double scaling, double conc, double reference_surface_vmr,
                        const double* h_vmr_fl_one_gas, int nconc, const double* h_pressure_conc,
                        const double* h_conc_req, double* h_scaling_profile, double* h_vmr_fl_out) {
  ECCKD_REQUIRE(nlay > 0 && h_pressure_hl && h_scaling_profile, "ecckd_merge_scaling: bad argument");
  if (nconc > 0) {
    // a requested concentration profile (read_merged_spectrum.cpp:117-131): interp in pressure with the
    // ends clamped, then the ratio to the file's own profile
    ECCKD_REQUIRE(h_pressure_conc && h_conc_req && h_vmr_fl_one_gas, "ecckd_merge_scaling: concentration profile arrays missing");
    for (int l = 0; l < nlay; ++l) {
      const double pfl = 0.5 * (h_pressure_hl[l] + h_pressure_hl[l + 1]);
      double c;
      if (nconc == 1 || pfl < h_pressure_conc[0]) c = h_conc_req[0];
      else if (pfl > h_pressure_conc[nconc - 1]) c = h_conc_req[nconc - 1];
      else {
        int j = 0;
        while (j < nconc - 2 && pfl > h_pressure_conc[j + 1]) ++j;
        const double w = (pfl - h_pressure_conc[j]) / (h_pressure_conc[j + 1] - h_pressure_conc[j]);
        c = (1.0 - w) * h_conc_req[j] + w * h_conc_req[j + 1];
      }
      h_scaling_profile[l] = c / h_vmr_fl_one_gas[l];
      if (h_vmr_fl_out) h_vmr_fl_out[l] = c;
    }
    return ECCKD_OK;
  }
  // scalar rules, :132-147
  if (conc == 0.0) scaling = 0.0;
  else if (conc > 0.0) {
    if (reference_surface_vmr < 0.0)
      return ecckd::fail(ECCKD_PARAMETER_ERROR, "Attempt to specify concentration when no reference_surface_mole_fraction present");
    scaling = conc / reference_surface_vmr;
  } else if (scaling < 0.0) scaling = 1.0;
  for (int l = 0; l < nlay; ++l) {
    h_scaling_profile[l] = scaling;
    // :158-164: the mole fraction is scaled too (an absent profile, -1, scales with it as in the reference)
    if (h_vmr_fl_out) h_vmr_fl_out[l] = (scaling != 1.0) ? (h_vmr_fl_one_gas ? h_vmr_fl_one_gas[l] : -1.0) * scaling
                                                         : (h_vmr_fl_one_gas ? h_vmr_fl_one_gas[l] : -1.0);
  }
  return ECCKD_OK;
}

int ecckd_merge_spectrum_dev(ecckd_ctx* ctx, int nlay, size_t nwav, const void* d_od, int od_type, size_t od_stride,
                             const double* h_scaling_profile, int first, double* d_merged, size_t merged_stride) {
  ECCKD_REQUIRE(ctx && d_od && h_scaling_profile && d_merged && nlay > 0 && nlay < 65536,
                "ecckd_merge_spectrum_dev: bad argument");
  ECCKD_REQUIRE(od_type == ECCKD_F32 || od_type == ECCKD_F64, "ecckd_merge_spectrum_dev: od_type must be ECCKD_F32 or ECCKD_F64");
  ECCKD_REQUIRE(od_stride >= nwav && merged_stride >= nwav, "ecckd_merge_spectrum_dev: row stride shorter than nwav");
  if (nwav == 0) return ECCKD_OK;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  ECCKD_CHECK(ecckd::ensure_scratch(ctx, (size_t)nlay * sizeof(double)));
  double* d_scale = (double*)ctx->scratch;
  ECCKD_HIP_CHECK(hipMemcpyAsync(d_scale, h_scaling_profile, (size_t)nlay * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const dim3 grid((unsigned)((nwav + 255) / 256), (unsigned)nlay);
  if (od_type == ECCKD_F32)
    hipLaunchKernelGGL(k_merge<float>, grid, dim3(256), 0, ctx->stream, nwav, od_stride, merged_stride, (const float*)d_od,
                       d_scale, first, d_merged);
  else
    hipLaunchKernelGGL(k_merge<double>, grid, dim3(256), 0, ctx->stream, nwav, od_stride, merged_stride, (const double*)d_od,
                       d_scale, first, d_merged);
  ECCKD_HIP_CHECK(hipGetLastError());
  // h_scaling_profile is pageable: the copy has been staged, but keep the call synchronous so the caller may reuse it
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return ECCKD_OK;
}

int ecckd_merge_scenario_geometry(int* points_per_thread, int* threads_per_block) {
  ECCKD_REQUIRE(points_per_thread && threads_per_block, "ecckd_merge_scenario_geometry: NULL argument");
  *points_per_thread = MS_P;
  *threads_per_block = MS_T;
  return ECCKD_OK;
}

int ecckd_merge_scenario_dev(ecckd_ctx* ctx, int nlay, size_t nwav, int ngas, const void* const* d_od, const int* od_type,
                             const size_t* od_stride, const double* h_scale, double* d_merged, size_t merged_stride) {
  const char* who = "ecckd_merge_scenario_dev";
  ECCKD_REQUIRE(ctx && d_merged && nlay > 0 && nlay < 65536, "%s: bad argument", who);
  GasRows gr;
  ECCKD_CHECK(ecckd::lbl::check_gases(who, ngas, d_od, od_type, od_stride, nwav, 1, h_scale, gr));
  ECCKD_REQUIRE(merged_stride >= nwav, "%s: merged_stride (%zu) < nwav (%zu)", who, merged_stride, nwav);
  if (nwav == 0) return ECCKD_OK;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const size_t nscale = (size_t)ngas * nlay;
  ECCKD_CHECK(ecckd::ensure_scratch(ctx, nscale * sizeof(double)));
  double* d_scale = (double*)ctx->scratch;
  ECCKD_HIP_CHECK(hipMemcpyAsync(d_scale, h_scale, nscale * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const size_t per_block = (size_t)MS_P * MS_T;
  const dim3 grid((unsigned)((nwav + per_block - 1) / per_block), (unsigned)nlay);
  hipLaunchKernelGGL(k_merge_scenario, grid, dim3(MS_T), 0, ctx->stream, nwav, ngas, nlay, gr, d_scale, d_merged, merged_stride);
  ECCKD_HIP_CHECK(hipGetLastError());
  // h_scale is pageable: as in ecckd_merge_spectrum_dev, the call is synchronous so that the caller may reuse it
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return ECCKD_OK;
}

}  // extern "C"
