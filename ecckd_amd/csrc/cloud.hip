// cloud.hip - the cloud pseudo-gas of the shortwave chain on the device:
//   ecckd_cloud_sorting_variable_dev  reorder_cloud_spectrum.cpp:111-123: the absorptance of an optically thick cloud on the
//                                     Mie grid, interpolated onto the spectral grid (the key the per-band stable sort ranks)
//   ecckd_cloud_partition_dev         find_g_points.cpp:586-636 (the equal-solar-energy branch): the g points of the cloud
// Every nwav-sized pass runs here; the host sees per-band, per-tile and per-g-point numbers only.
#include "common.hpp"

#include <cmath>
#include <vector>

// No a*b + c of this file is fused into an fma: the keys (which are sorted next) must equal the double-precision restatement bit
// for bit.  (Plain operators on purpose: the _rn intrinsics are defined in a header outside the reach of this pragma, and the
// compiler fuses them.)
#pragma clang fp contract(off)

namespace {

constexpr int kLdsKnots = 2048;     // knots staged in LDS (2 x 16 KB); a longer Mie table is searched in HBM
constexpr int kScanItems = 8;       // consecutive points per thread in a scan tile
constexpr int kTile = 256 * kScanItems;
constexpr int kChunk = 8192;        // points per block of the per-g-point statistics
constexpr int kBoundsBlock = 64;    // boundary searches (one per thread) per block of k_cloud_bounds
constexpr int kGridBlocksPerCu = 16;  // blocks of 256 points per compute unit in one pass of the grid-stride kernels
constexpr int kMi355xCu = 256;      // ecckd_cloud_geometry without a context

// reorder_cloud_spectrum.cpp:115-120 per knot.  Every operation rounded on its own (no contraction), so that the keys equal a
// plain double-precision restatement bit for bit.  asymmetry_de = 1/(1+g) is what the reference writes (:117), not the
// textbook delta-Eddington g/(1+g): kept as written, since the ranks - and so the g points - follow from it.
__global__ void __launch_bounds__(256)
k_cloud_knots(int n, const double* __restrict__ ssa, const double* __restrict__ g, double* __restrict__ y) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const double s = ssa[k], a = g[k];
  const double f = a * a;
  const double g_de = 1.0 / (1.0 + a);
  const double ssa_de = s * (1.0 - f) / (1.0 - s * f);
  const double c = sqrt((1.0 - ssa_de) / (1.0 - ssa_de * g_de));   // f64 division and square root: correctly rounded
  y[k] = 1.0 - (1.0 - c) / (1.0 + c);
}

// adept::interp as the project restates it (context.hip, ecckd_idealised_temperature): j = the last knot with x_j <= xi,
// clamped to [0, n-2], so that outside the knots the end segments are extrapolated linearly
__device__ inline double interp_at(const double* x, const double* y, int n, double xi) {
  int lo = 0, len = n;
  while (len > 0) {                  // upper bound: the number of knots <= xi
    const int half = len >> 1;
    if (x[lo + half] <= xi) { lo += half + 1; len -= half + 1; }
    else len = half;
  }
  const int j = min(max(lo - 1, 0), n - 2);
  const double w = (xi - x[j]) / (x[j + 1] - x[j]);
  return (1.0 - w) * y[j] + w * y[j + 1];
}

template <bool kLds>
__global__ void __launch_bounds__(256)
k_cloud_interp(int n, const double* __restrict__ kx, const double* __restrict__ ky, size_t nwav, const double* __restrict__ wn,
               double* __restrict__ out) {
  __shared__ double sx[kLds ? kLdsKnots : 1], sy[kLds ? kLdsKnots : 1];
  const double *x = kx, *y = ky;
  if (kLds) {
    for (int k = threadIdx.x; k < n; k += blockDim.x) { sx[k] = kx[k]; sy[k] = ky[k]; }
    __syncthreads();
    x = sx; y = sy;
  }
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwav; i += (size_t)gridDim.x * blockDim.x)
    out[i] = interp_at(x, y, n, wn[i]);
}

// The band of index i: bands are ascending, disjoint index ranges [begin_b, end_b]; -1 between and outside them.
__device__ inline int band_of(int nband, const int64_t* begin, const int64_t* end, int64_t i) {
  int lo = 0, len = nband;
  while (len > 0) {
    const int half = len >> 1;
    if (begin[lo + half] <= i) { lo += half + 1; len -= half + 1; }
    else len = half;
  }
  const int b = lo - 1;
  return (b >= 0 && i <= end[b]) ? b : -1;
}

// Rank order (ireorder(irank(range(ibegin,iend))-ibegin) = range(ibegin,iend), :607): ssi and the sorting variable of every
// band point are scattered to their rank.  flag bit 1: a rank outside its band (or, outside every band, not the index itself,
// as write_order leaves it); bit 2: ssi < 0 (or NaN) somewhere; bit 4: the sorting variable of a band point is NaN (fmin / fmax
// would drop it from the band's range and from the g point's error, while the g point's mean became NaN).
__global__ void __launch_bounds__(256)
k_cloud_scatter(size_t nwav, const double* __restrict__ ssi, const double* __restrict__ sv, const int32_t* __restrict__ rank,
                int nband, const int64_t* __restrict__ begin, const int64_t* __restrict__ end, double* __restrict__ ssi_s,
                double* __restrict__ sv_s, int* __restrict__ flag) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwav; i += (size_t)gridDim.x * blockDim.x) {
    const double s = ssi[i];
    if (!(s >= 0.0)) atomicOr(flag, 2);
    const int64_t r = rank[i];
    const int b = band_of(nband, begin, end, (int64_t)i);
    if (b < 0) {
      if (r != (int64_t)i) atomicOr(flag, 1);
      continue;
    }
    if (r < begin[b] || r > end[b]) { atomicOr(flag, 1); continue; }
    const double v = sv[i];
    if (v != v) atomicOr(flag, 4);
    ssi_s[r] = s;
    sv_s[r] = v;
  }
}

// One scan tile: kScanItems consecutive points per thread, summed in order, then a Hillis-Steele scan of the 256 thread sums.
// The value of point k of thread t relative to the tile start is excl[t] + (its running sum); every quantity built from a
// tile (its total, the running sums) uses that one expression, so that the band total equals the last running sum bit for bit.
struct TileScan {
  double v[kScanItems];
  double excl;
  int nmine;
};

__device__ inline void tile_scan(const double* __restrict__ src, int64_t s, int64_t e, double* lds, TileScan& ts) {
  const int t = threadIdx.x;
  const int64_t p0 = s + (int64_t)t * kScanItems;
  double run = 0.0;
  ts.nmine = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    const int64_t p = p0 + k;
    if (p < e) { run += src[p]; ts.nmine = k + 1; }
    ts.v[k] = run;
  }
  lds[t] = run;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    const double add = t >= off ? lds[t - off] : 0.0;
    __syncthreads();
    if (t >= off) lds[t] = lds[t] + add;
    __syncthreads();
  }
  ts.excl = t > 0 ? lds[t - 1] : 0.0;
  __syncthreads();
}

// per tile: the total of ssi in rank order (as the scan forms it) and the extremes of the sorting variable
__global__ void __launch_bounds__(256)
k_cloud_tile_reduce(const int64_t* __restrict__ tile_s, const int64_t* __restrict__ tile_e, const double* __restrict__ ssi_s,
                    const double* __restrict__ sv_s, double* __restrict__ tile_sum, double* __restrict__ tile_min,
                    double* __restrict__ tile_max) {
  __shared__ double lds[256], lmin[256], lmax[256];
  const int64_t s = tile_s[blockIdx.x], e = tile_e[blockIdx.x];
  TileScan ts;
  tile_scan(ssi_s, s, e, lds, ts);
  const int t = threadIdx.x;
  if (ts.nmine > 0 && (s + (int64_t)t * kScanItems + ts.nmine == e)) tile_sum[blockIdx.x] = ts.excl + ts.v[ts.nmine - 1];
  double mn = INFINITY, mx = -INFINITY;
  for (int64_t p = s + t; p < e; p += 256) { const double v = sv_s[p]; mn = fmin(mn, v); mx = fmax(mx, v); }
  lmin[t] = mn; lmax[t] = mx;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) { lmin[t] = fmin(lmin[t], lmin[t + h]); lmax[t] = fmax(lmax[t], lmax[t + h]); }
    __syncthreads();
  }
  if (t == 0) { tile_min[blockIdx.x] = lmin[0]; tile_max[blockIdx.x] = lmax[0]; }
}

// running sums: cum[p] = offset(tile) + (excl[t] + running sum of thread t)
__global__ void __launch_bounds__(256)
k_cloud_tile_scan(const int64_t* __restrict__ tile_s, const int64_t* __restrict__ tile_e, const double* __restrict__ tile_off,
                  const double* __restrict__ ssi_s, double* __restrict__ cum) {
  __shared__ double lds[256];
  const int64_t s = tile_s[blockIdx.x], e = tile_e[blockIdx.x];
  const double off = tile_off[blockIdx.x];
  TileScan ts;
  tile_scan(ssi_s, s, e, lds, ts);
  const int64_t p0 = s + (int64_t)threadIdx.x * kScanItems;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k)
    if (k < ts.nmine) cum[p0 + k] = off + (ts.excl + ts.v[k]);
}

// the first p of [lo, hi) with cum[p] >= value (hi if none): the running sum is monotone where ssi >= 0
__global__ void __launch_bounds__(kBoundsBlock)
k_cloud_bounds(int nq, const double* __restrict__ cum, const int64_t* __restrict__ q_lo, const int64_t* __restrict__ q_hi,
               const double* __restrict__ q_val, int64_t* __restrict__ q_pos) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  int64_t lo = q_lo[q], len = q_hi[q] - lo;
  const double v = q_val[q];
  while (len > 0) {
    const int64_t half = len >> 1;
    if (cum[lo + half] < v) { lo += half + 1; len -= half + 1; }
    else len = half;
  }
  q_pos[q] = lo;
}

// per chunk of a g point's rank range: min, max and sum of the sorting variable, each formed in a fixed order
__global__ void __launch_bounds__(256)
k_cloud_chunk_stats(const int64_t* __restrict__ chunk_s, const int64_t* __restrict__ chunk_e, const double* __restrict__ sv_s,
                    double* __restrict__ out_min, double* __restrict__ out_max, double* __restrict__ out_sum) {
  __shared__ double lmin[256], lmax[256], lsum[256];
  const int64_t s = chunk_s[blockIdx.x], e = chunk_e[blockIdx.x];
  const int t = threadIdx.x;
  double mn = INFINITY, mx = -INFINITY, sum = 0.0;
  for (int64_t p = s + t; p < e; p += 256) {
    const double v = sv_s[p];
    mn = fmin(mn, v); mx = fmax(mx, v); sum += v;
  }
  lmin[t] = mn; lmax[t] = mx; lsum[t] = sum;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      lmin[t] = fmin(lmin[t], lmin[t + h]);
      lmax[t] = fmax(lmax[t], lmax[t + h]);
      lsum[t] = lsum[t] + lsum[t + h];
    }
    __syncthreads();
  }
  if (t == 0) { out_min[blockIdx.x] = lmin[0]; out_max[blockIdx.x] = lmax[0]; out_sum[blockIdx.x] = lsum[0]; }
}

// device buffers of one call, returned to the context's cache however the call ends
struct Scratch {
  ecckd_ctx* ctx;
  std::vector<void*> ptrs;
  explicit Scratch(ecckd_ctx* c) : ctx(c) {}
  ~Scratch() {
    (void)hipStreamSynchronize(ctx->stream);
    for (void* p : ptrs) ecckd::dev_release(ctx, p);
  }
  template <class T> hipError_t get(T** p, size_t n) {
    void* v = nullptr;
    const hipError_t e = ecckd::dev_malloc(ctx, &v, (n ? n : 1) * sizeof(T));
    if (e == hipSuccess) { ptrs.push_back(v); *p = (T*)v; }
    return e;
  }
};

template <class T> hipError_t upload(ecckd_ctx* ctx, T* d, const std::vector<T>& h) {
  return hipMemcpyAsync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream);
}
template <class T> hipError_t download(ecckd_ctx* ctx, std::vector<T>& h, const T* d) {
  return hipMemcpyAsync(h.data(), d, h.size() * sizeof(T), hipMemcpyDeviceToHost, ctx->stream);
}

unsigned grid_for(size_t n, int num_cu) {
  const size_t want = (n + 255) / 256, cap = (size_t)num_cu * kGridBlocksPerCu;
  return (unsigned)std::max<size_t>(1, std::min(want, cap));
}

}  // namespace

extern "C" {

int ecckd_cloud_geometry(ecckd_ctx* ctx, int* lds_knots, int* scan_items, int* scan_tile, int* stats_chunk, int* bounds_block,
                         int64_t* grid_points) {
  ECCKD_REQUIRE(lds_knots && scan_items && scan_tile && stats_chunk && bounds_block && grid_points,
                "ecckd_cloud_geometry: NULL argument");
  *lds_knots = kLdsKnots;
  *scan_items = kScanItems;
  *scan_tile = kTile;
  *stats_chunk = kChunk;
  *bounds_block = kBoundsBlock;
  *grid_points = (int64_t)kGridBlocksPerCu * (ctx ? ctx->num_cu : kMi355xCu) * 256;
  return ECCKD_OK;
}

int ecckd_cloud_sorting_variable_dev(ecckd_ctx* ctx, int nknot, const double* h_cloud_wavenumber, const double* h_ssa,
                                     const double* h_asymmetry, size_t nwav, const double* d_wavenumber, double* d_sorting_variable) {
  ECCKD_REQUIRE(ctx && h_cloud_wavenumber && h_ssa && h_asymmetry && (nwav == 0 || (d_wavenumber && d_sorting_variable)),
                "ecckd_cloud_sorting_variable_dev: NULL argument");
  ECCKD_REQUIRE(nknot >= 2, "ecckd_cloud_sorting_variable_dev: at least 2 cloud wavenumbers needed, got %d", nknot);
  for (int k = 1; k < nknot; ++k)
    ECCKD_REQUIRE(h_cloud_wavenumber[k] > h_cloud_wavenumber[k - 1],
                  "Cloud wavenumbers must be strictly ascending (wavenumber(%d) = %g, wavenumber(%d) = %g)", k - 1,
                  h_cloud_wavenumber[k - 1], k, h_cloud_wavenumber[k]);
  if (nwav == 0) return ECCKD_OK;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  Scratch sc(ctx);
  double *d_x = nullptr, *d_ssa = nullptr, *d_g = nullptr, *d_y = nullptr;
  ECCKD_HIP_CHECK(sc.get(&d_x, nknot));
  ECCKD_HIP_CHECK(sc.get(&d_ssa, nknot));
  ECCKD_HIP_CHECK(sc.get(&d_g, nknot));
  ECCKD_HIP_CHECK(sc.get(&d_y, nknot));
  const size_t kb = (size_t)nknot * sizeof(double);
  ECCKD_HIP_CHECK(hipMemcpyAsync(d_x, h_cloud_wavenumber, kb, hipMemcpyHostToDevice, ctx->stream));
  ECCKD_HIP_CHECK(hipMemcpyAsync(d_ssa, h_ssa, kb, hipMemcpyHostToDevice, ctx->stream));
  ECCKD_HIP_CHECK(hipMemcpyAsync(d_g, h_asymmetry, kb, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_cloud_knots, dim3((unsigned)((nknot + 255) / 256)), dim3(256), 0, ctx->stream, nknot, d_ssa, d_g, d_y);
  ECCKD_HIP_CHECK(hipGetLastError());
  const unsigned grid = grid_for(nwav, ctx->num_cu);
  if (nknot <= kLdsKnots)
    hipLaunchKernelGGL(k_cloud_interp<true>, dim3(grid), dim3(256), 0, ctx->stream, nknot, d_x, d_y, nwav, d_wavenumber,
                       d_sorting_variable);
  else
    hipLaunchKernelGGL(k_cloud_interp<false>, dim3(grid), dim3(256), 0, ctx->stream, nknot, d_x, d_y, nwav, d_wavenumber,
                       d_sorting_variable);
  ECCKD_HIP_CHECK(hipGetLastError());
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // the knot arrays are pageable host memory
  return ECCKD_OK;
}

int ecckd_cloud_partition_dev(ecckd_ctx* ctx, size_t nwav, const double* d_ssi, const int32_t* d_rank,
                              const double* d_sorting_variable, int nband, const int64_t* h_band_begin, const int64_t* h_band_end,
                              double max_reflectance_range, int capacity, int* h_n_g_points, int* h_ng, int* h_band_number,
                              int64_t* h_rank1, int64_t* h_rank2, double* h_error, double* h_median) {
  ECCKD_REQUIRE(ctx && d_ssi && d_rank && d_sorting_variable && h_band_begin && h_band_end && h_n_g_points && h_ng &&
                h_band_number && h_rank1 && h_rank2 && h_error && h_median, "ecckd_cloud_partition_dev: NULL argument");
  ECCKD_REQUIRE(nband > 0 && nwav > 0 && nwav < ((size_t)1 << 31), "ecckd_cloud_partition_dev: nband = %d, nwav = %zu", nband, nwav);
  ECCKD_REQUIRE(max_reflectance_range > 0.0, "max_reflectance_range must be positive (%g)", max_reflectance_range);
  *h_ng = 0;
  for (int b = 0; b < nband; ++b) {
    ECCKD_REQUIRE(h_band_begin[b] >= 0 && h_band_begin[b] <= h_band_end[b] && h_band_end[b] < (int64_t)nwav,
                  "Band %d contains no wavenumbers", b);
    ECCKD_REQUIRE(b == 0 || h_band_begin[b] > h_band_end[b - 1], "ecckd_cloud_partition_dev: bands %d and %d overlap", b - 1, b);
  }
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  Scratch sc(ctx);
  std::vector<int64_t> bb(h_band_begin, h_band_begin + nband), be(h_band_end, h_band_end + nband);
  int64_t *d_bb = nullptr, *d_be = nullptr;
  double *ssi_s = nullptr, *sv_s = nullptr, *cum = nullptr;
  int* d_flag = nullptr;
  ECCKD_HIP_CHECK(sc.get(&d_bb, nband));
  ECCKD_HIP_CHECK(sc.get(&d_be, nband));
  ECCKD_HIP_CHECK(sc.get(&ssi_s, nwav));
  ECCKD_HIP_CHECK(sc.get(&sv_s, nwav));
  ECCKD_HIP_CHECK(sc.get(&cum, nwav));
  ECCKD_HIP_CHECK(sc.get(&d_flag, 1));
  ECCKD_HIP_CHECK(upload(ctx, d_bb, bb));
  ECCKD_HIP_CHECK(upload(ctx, d_be, be));
  ECCKD_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(int), ctx->stream));
  ECCKD_HIP_CHECK(hipMemsetAsync(ssi_s, 0, nwav * sizeof(double), ctx->stream));
  ECCKD_HIP_CHECK(hipMemsetAsync(sv_s, 0, nwav * sizeof(double), ctx->stream));
  hipLaunchKernelGGL(k_cloud_scatter, dim3(grid_for(nwav, ctx->num_cu)), dim3(256), 0, ctx->stream, nwav, d_ssi, d_sorting_variable,
                     d_rank, nband, d_bb, d_be, ssi_s, sv_s, d_flag);
  ECCKD_HIP_CHECK(hipGetLastError());

  // scan tiles: every band cut into kTile-point tiles of its own
  std::vector<int64_t> ts, te;
  std::vector<int> tile_first(nband + 1, 0);
  for (int b = 0; b < nband; ++b) {
    tile_first[b] = (int)ts.size();
    for (int64_t s = bb[b]; s <= be[b]; s += kTile) { ts.push_back(s); te.push_back(std::min<int64_t>(s + kTile, be[b] + 1)); }
  }
  tile_first[nband] = (int)ts.size();
  const int ntile = (int)ts.size();
  int64_t *d_ts = nullptr, *d_te = nullptr;
  double *d_tsum = nullptr, *d_tmin = nullptr, *d_tmax = nullptr, *d_toff = nullptr;
  ECCKD_HIP_CHECK(sc.get(&d_ts, ntile));
  ECCKD_HIP_CHECK(sc.get(&d_te, ntile));
  ECCKD_HIP_CHECK(sc.get(&d_tsum, ntile));
  ECCKD_HIP_CHECK(sc.get(&d_tmin, ntile));
  ECCKD_HIP_CHECK(sc.get(&d_tmax, ntile));
  ECCKD_HIP_CHECK(sc.get(&d_toff, ntile));
  ECCKD_HIP_CHECK(upload(ctx, d_ts, ts));
  ECCKD_HIP_CHECK(upload(ctx, d_te, te));
  int flag = 0;
  ECCKD_HIP_CHECK(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (flag & 2) return ecckd::fail(ECCKD_PARAMETER_ERROR, "solar_spectral_irradiance is negative (or NaN) at some wavenumbers");
  if (flag & 1) return ecckd::fail(ECCKD_PARAMETER_ERROR, "The cloud ordering's rank does not permute the wavenumbers of each band among themselves");
  if (flag & 4) return ecckd::fail(ECCKD_PARAMETER_ERROR, "The cloud ordering's sorting variable is NaN at some wavenumbers of a band");
  hipLaunchKernelGGL(k_cloud_tile_reduce, dim3(ntile), dim3(256), 0, ctx->stream, d_ts, d_te, ssi_s, sv_s, d_tsum, d_tmin, d_tmax);
  ECCKD_HIP_CHECK(hipGetLastError());
  std::vector<double> tsum(ntile), tmin(ntile), tmax(ntile), toff(ntile);
  ECCKD_HIP_CHECK(download(ctx, tsum, d_tsum));
  ECCKD_HIP_CHECK(download(ctx, tmin, d_tmin));
  ECCKD_HIP_CHECK(download(ctx, tmax, d_tmax));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));

  // per band: the tiles' offsets in order, the band's irradiance (= its last running sum) and its number of g points (:591-596)
  std::vector<int> ngb(nband);
  std::vector<double> d_irr(nband);
  int ng = 0;
  for (int b = 0; b < nband; ++b) {
    double off = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int k = tile_first[b]; k < tile_first[b + 1]; ++k) {
      toff[k] = off;
      off = off + tsum[k];
      mn = std::fmin(mn, tmin[k]);
      mx = std::fmax(mx, tmax[k]);
    }
    const double nd = (mx - mn) / max_reflectance_range;
    if (!(nd >= 0.0) || nd >= (double)capacity)
      return ecckd::fail(ECCKD_PROCESSING_ERROR, "Band %d: sorting variable range %g-%g gives more g points than the %d allowed", b, mn, mx, capacity);
    ngb[b] = static_cast<int>(nd) + 1;
    d_irr[b] = off * (1.0 + 1.0e-8) / ngb[b];
    ng += ngb[b];
    if (ng > capacity) return ecckd::fail(ECCKD_PROCESSING_ERROR, "More than %d cloud g points", capacity);
  }
  ECCKD_HIP_CHECK(upload(ctx, d_toff, toff));
  hipLaunchKernelGGL(k_cloud_tile_scan, dim3(ntile), dim3(256), 0, ctx->stream, d_ts, d_te, d_toff, ssi_s, cum);
  ECCKD_HIP_CHECK(hipGetLastError());

  // g point jg of band b holds the points with jg*d <= cum < (jg+1)*d (:612-615): the boundaries jg*d, jg = 0..ng_b
  std::vector<int64_t> qlo, qhi;
  std::vector<double> qval;
  for (int b = 0; b < nband; ++b)
    for (int jg = 0; jg <= ngb[b]; ++jg) { qlo.push_back(bb[b]); qhi.push_back(be[b] + 1); qval.push_back(jg * d_irr[b]); }
  const int nq = (int)qval.size();
  int64_t *d_qlo = nullptr, *d_qhi = nullptr, *d_qpos = nullptr;
  double* d_qval = nullptr;
  ECCKD_HIP_CHECK(sc.get(&d_qlo, nq));
  ECCKD_HIP_CHECK(sc.get(&d_qhi, nq));
  ECCKD_HIP_CHECK(sc.get(&d_qval, nq));
  ECCKD_HIP_CHECK(sc.get(&d_qpos, nq));
  ECCKD_HIP_CHECK(upload(ctx, d_qlo, qlo));
  ECCKD_HIP_CHECK(upload(ctx, d_qhi, qhi));
  ECCKD_HIP_CHECK(upload(ctx, d_qval, qval));
  hipLaunchKernelGGL(k_cloud_bounds, dim3((unsigned)((nq + kBoundsBlock - 1) / kBoundsBlock)), dim3(kBoundsBlock), 0, ctx->stream,
                     nq, cum, d_qlo, d_qhi, d_qval, d_qpos);
  ECCKD_HIP_CHECK(hipGetLastError());
  std::vector<int64_t> qpos(nq);
  ECCKD_HIP_CHECK(download(ctx, qpos, d_qpos));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));

  // the g points: contiguous rank ranges, cut into chunks for the statistics of the sorting variable
  std::vector<int64_t> cs, ce;
  std::vector<int> chunk_first(ng + 1, 0);
  int ig = 0, q = 0;
  for (int b = 0; b < nband; ++b, ++q) {
    for (int jg = 0; jg < ngb[b]; ++jg, ++q, ++ig) {
      const int64_t r1 = qpos[q], r2 = qpos[q + 1] - 1;
      if (r2 < r1) return ecckd::fail(ECCKD_PROCESSING_ERROR, "Band %d, g point %d holds no wavenumber", b, jg);
      h_band_number[ig] = b;
      h_rank1[ig] = r1;
      h_rank2[ig] = r2;
      chunk_first[ig] = (int)cs.size();
      for (int64_t s = r1; s <= r2; s += kChunk) { cs.push_back(s); ce.push_back(std::min<int64_t>(s + kChunk, r2 + 1)); }
    }
    h_n_g_points[b] = ngb[b];
  }
  chunk_first[ng] = (int)cs.size();
  const int nchunk = (int)cs.size();
  int64_t *d_cs = nullptr, *d_ce = nullptr;
  double *d_cmin = nullptr, *d_cmax = nullptr, *d_csum = nullptr;
  ECCKD_HIP_CHECK(sc.get(&d_cs, nchunk));
  ECCKD_HIP_CHECK(sc.get(&d_ce, nchunk));
  ECCKD_HIP_CHECK(sc.get(&d_cmin, nchunk));
  ECCKD_HIP_CHECK(sc.get(&d_cmax, nchunk));
  ECCKD_HIP_CHECK(sc.get(&d_csum, nchunk));
  ECCKD_HIP_CHECK(upload(ctx, d_cs, cs));
  ECCKD_HIP_CHECK(upload(ctx, d_ce, ce));
  hipLaunchKernelGGL(k_cloud_chunk_stats, dim3(nchunk), dim3(256), 0, ctx->stream, d_cs, d_ce, sv_s, d_cmin, d_cmax, d_csum);
  ECCKD_HIP_CHECK(hipGetLastError());
  std::vector<double> cmin(nchunk), cmax(nchunk), csum(nchunk);
  ECCKD_HIP_CHECK(download(ctx, cmin, d_cmin));
  ECCKD_HIP_CHECK(download(ctx, cmax, d_cmax));
  ECCKD_HIP_CHECK(download(ctx, csum, d_csum));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  // error = max - min of the sorting variable; median = -2 + its unweighted mean, below every gas's sorting variable (:617-622)
  for (int k = 0; k < ng; ++k) {
    double mn = INFINITY, mx = -INFINITY, sum = 0.0;
    for (int c = chunk_first[k]; c < chunk_first[k + 1]; ++c) { mn = std::fmin(mn, cmin[c]); mx = std::fmax(mx, cmax[c]); sum += csum[c]; }
    h_error[k] = mx - mn;
    h_median[k] = -2.0 + sum / (double)(h_rank2[k] - h_rank1[k] + 1);
  }
  *h_ng = ng;
  return ECCKD_OK;
}

}  // extern "C"
