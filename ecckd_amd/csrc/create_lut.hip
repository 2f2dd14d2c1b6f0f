// create_lut.hip - K6/K7: the create_look_up_table hot path on gfx950.
//
// K6  ecckd_average_to_gpoints  average_optical_depth_to_g_point (reference
//       src/ecckd/average_optical_depth.cpp:22-197): for every g point and layer, the
//       Planck- or solar-weighted average of the line-by-line optical depth under one of nine
//       averaging methods, its min and max, and the conversion to molar absorption.
// K7  ecckd_gpoint_fraction     create_look_up_table.cpp:537-548
//     ecckd_planck_lut          create_look_up_table.cpp:581-591
//
// Design.  The reference does `find(g_point == ig)` and a gather per g point (and an
// O(ng*nint*nwav) triple loop for the fractions).  Here the wavenumbers are sorted by g point
// ONCE per g-point map with the stable radix sort of K3 (a stable sort keeps the wavenumbers
// ascending inside every g point), so each g point is a contiguous segment of a permutation
// and every quantity above is a segmented reduction: fixed-size chunks of a segment are reduced
// by one block each (fixed order), a second tiny kernel combines the chunk partials in order.
// The Planck weights are recomputed from (T, wavenumber) on the fly instead of being read from
// an (nlay, nwav) matrix: 8 B/point/layer of HBM traffic traded for one exp.
//
// Every piece of such a reduction is written once.  A partial kernel (k_gavg_partial, k_planck_lut_partial, k_rowsum_partial,
// k_erythemal_partial, k_width_chunk_sums) takes its positions from chunk_positions() and, but for K6a, meets its waves in
// block_sum_256 (rt_device.hpp); combine_chunks() adds the chunk partials of a g point, in k_combine_chunks (the Planck table,
// the row sums, the erythemal pair, the total widths) and in k_gavg_final.  On the host, carve_work() cuts the map's work
// buffer as gmap_layout.hpp sizes it and reduce_rows() runs partial kernel, combine and copy-back.  The map owns its device
// memory through ecckd_gmap::alloc (gmap.hpp).
#include "common.hpp"
#include "rt_device.hpp"
#include "gmap.hpp"

#include <cmath>
#include <memory>
#include <vector>

namespace {

constexpr double kD = ECCKD_LW_DIFFUSIVITY;
namespace L = ecckd::gmap_layout;       // the chunking and the sizes of the work buffer
using L::GA_THREADS; using L::GA_PPT;
static_assert(GA_THREADS == 256, "block_sum_256");

// averaging-method codes of the ABI (ECCKD_AVG_*)
constexpr int M_LINEAR = 0, M_TRANS = 1, M_TRANS2 = 2, M_SQRT = 3, M_LOG = 4, M_TRANS3 = 6, M_TRANS10 = 7, M_HYBRID = 8;

using ecckd::wave_sum; using ecckd::wave_min; using ecckd::wave_max; using ecckd::block_sum_256;   // rt_device.hpp
using Chunk = ecckd::GmapChunk;

// transmission-k averages 1 - exp(-k D tau): k of a layer's method, 0 where it is no transmission method
// (average_optical_depth.cpp:43-133)
__device__ __forceinline__ double transmission_factor(int lm) {
  return lm == M_TRANS ? 1.0 : lm == M_TRANS2 ? 2.0 : lm == M_TRANS3 ? 3.0 : lm == M_TRANS10 ? 10.0 : 0.0;
}

// The GA_PPT sorted positions that thread tid has in chunk c: c.p0 + p * GA_THREADS + tid, live[p] where that lies inside the
// chunk.  A dead one is clamped to c.p1: a load from ii[p] is always in bounds, what it returns counts only where live[p].
struct ChunkWalk { size_t ii[GA_PPT]; bool live[GA_PPT]; };
__device__ __forceinline__ ChunkWalk chunk_positions(const Chunk& c, int tid) {
  ChunkWalk w;
#pragma unroll
  for (int p = 0; p < GA_PPT; ++p) {
    const long long i = c.p0 + (long long)p * GA_THREADS + tid;
    w.live[p] = i <= c.p1;
    w.ii[p] = w.live[p] ? (size_t)i : (size_t)c.p1;
  }
  return w;
}

// The chunk partials q[c * stride], c0 <= c < c1, of one g point combined by a wave: lane j takes the chunks c0 + j,
// c0 + j + 64, ... in chunk order, the lanes' results are folded in a fixed tree (a function of the chunk count alone).  The
// result is valid in lane 0; no chunk gives `init`.
template <typename Op, typename Fold>
__device__ __forceinline__ double combine_chunks(const double* __restrict__ q, size_t stride, int c0, int c1, int lane, double init,
                                                 Op op, Fold fold) {
  double v = init;
  for (int c = c0 + lane; c < c1; c += 64) v = op(v, q[(size_t)c * stride]);
  return fold(v);
}
__device__ __forceinline__ double chunk_sum(const double* q, size_t stride, int c0, int c1, int lane) {
  return combine_chunks(q, stride, c0, c1, lane, 0.0, [](double a, double b) { return a + b; }, wave_sum);
}

__global__ void __launch_bounds__(256)
k_gmap_keys(size_t n, const int32_t* __restrict__ g_point, int ng, double* __restrict__ key, int* __restrict__ counts,
            int* __restrict__ flag) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int g = g_point[j];
  if (g >= ng) { atomicOr(flag, 1); key[j] = 1.0e300; return; }
  key[j] = (g >= 0) ? (double)g : 1.0e300;  // unassigned points sort last
  if (g >= 0) atomicAdd(&counts[g], 1);
}

__global__ void __launch_bounds__(256)
k_gmap_gather(size_t n, const int32_t* __restrict__ order, const double* __restrict__ wn, const double* __restrict__ dwn,
              double* __restrict__ wn_s, double* __restrict__ dwn_s) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t j = (size_t)order[i];
  wn_s[i] = wn[j];
  dwn_s[i] = dwn[j];
}

// flag |= 2 if the wavenumbers are not ascending inside some g-point segment
__global__ void __launch_bounds__(256)
k_gmap_check(size_t nassigned, const int32_t* __restrict__ order, const int32_t* __restrict__ g_point,
             const double* __restrict__ wn_s, int* __restrict__ flag) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i + 1 >= nassigned) return;
  if (g_point[order[i]] == g_point[order[i + 1]] && !(wn_s[i + 1] >= wn_s[i])) atomicOr(flag, 2);
}

// K6a.  partial[chunk][layer][6] = { num, den, den_nz, cnt_nz, min, max }.  Per layer and point: the Planck weight at the
// layer's temperature (planck_function.cpp:48-50) and the averaged quantity of the layer's method
// (average_optical_depth.cpp:43-133) - the same two exp per layer and point as K1, with the same < 1 ulp exp / division
// (fastmath.hpp) instead of the library's -; the six per-layer sums of a wave are folded together (fold_wave, rt_device.hpp), the waves' results
// wait in LDS and are combined in wave order once, after the last layer: no barrier inside the layer loop.
// dynamic LDS: [nlay][6][GA_THREADS / 64]
template <typename OdT>
__global__ void __launch_bounds__(GA_THREADS)
k_gavg_partial(int nlay, size_t od_stride, const Chunk* __restrict__ chunks, const int32_t* __restrict__ order,
               const double* __restrict__ wn_s, const double* __restrict__ dwn_s, const OdT* __restrict__ od,
               const double* __restrict__ hk /*[nlay] (h/k)/T_fl, LW*/, const double* __restrict__ ssi /*SW, original order*/,
               const int* __restrict__ layer_method, double* __restrict__ partial) {
  extern __shared__ double s_part[];
  constexpr int NW = GA_THREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const ChunkWalk at = chunk_positions(chunks[blockIdx.x], tid);
  size_t jj[GA_PPT];
  double freq[GA_PPT], pref[GA_PPT];
#pragma unroll
  for (int p = 0; p < GA_PPT; ++p) {
    jj[p] = (size_t)order[at.ii[p]];
    if (hk) {
      // planck_function.cpp:48-50
      freq[p] = ecckd::wn_to_freq(wn_s[at.ii[p]]);
      pref[p] = ecckd::planck_pref(dwn_s[at.ii[p]], freq[p]);
    } else {
      freq[p] = 0.0;
      pref[p] = ssi[jj[p]];
    }
  }
  const int kk = (int)(__brev((unsigned)lane) >> 26);           // which folded value this lane ends up with
  for (int l = 0; l < nlay; ++l) {
    const int lm = layer_method[l];
    // every optical depth of the layer first: the gathers are independent
    double o[GA_PPT];
#pragma unroll
    for (int p = 0; p < GA_PPT; ++p) o[p] = (double)od[(size_t)l * od_stride + jj[p]];
    double sums[4] = {0.0, 0.0, 0.0, 0.0};      // num, den, den_nz, cnt_nz
    double mm[2] = {INFINITY, INFINITY};        // min, -max
    const double hkl = hk ? hk[l] : 0.0;
    const double dscale = kD * transmission_factor(lm);
#pragma unroll
    for (int p = 0; p < GA_PPT; ++p) {
      if (!at.live[p]) continue;
      const double w = hk ? ecckd::planck(pref[p], freq[p], hkl) : pref[p];
      sums[1] += w;
      mm[0] = fmin(mm[0], o[p]);
      mm[1] = fmin(mm[1], -o[p]);
      if (dscale > 0.0) sums[0] += (1.0 - ecckd::exp_fast(-o[p] * dscale)) * w;
      else if (lm == M_LINEAR) sums[0] += o[p] * w;
      else if (lm == M_SQRT) sums[0] += sqrt(o[p]) * w;
      else if (o[p] > 0.0) { sums[0] += log(o[p]) * w; sums[2] += w; sums[3] += 1.0; }      // logarithmic
    }
    ecckd::fold_wave<4, false>(sums, lane, [](double a, double b) { return a + b; });
    ecckd::fold_wave<2, false>(mm, lane, [](double a, double b) { return fmin(a, b); });
    if (kk < 4) s_part[((size_t)l * 6 + kk) * NW + wave] = sums[0];
    if (kk < 2) s_part[((size_t)l * 6 + 4 + kk) * NW + wave] = kk == 0 ? mm[0] : -mm[0];
  }
  __syncthreads();
  for (int t = tid; t < nlay * 6; t += GA_THREADS) {
    const double* q = s_part + (size_t)t * NW;
    const int k = t % 6;
    double v = q[0];
    for (int w = 1; w < NW; ++w) v = k < 4 ? v + q[w] : (k == 4 ? fmin(v, q[w]) : fmax(v, q[w]));
    partial[(size_t)blockIdx.x * nlay * 6 + t] = v;
  }
}

// K6b.  grid (ng, nlay), block 64: the chunk partials of one g point and layer combined (combine_chunks), then fit, clamp,
// min/max repair and conversion to molar absorption (average_optical_depth.cpp:135-193).  (One block per g point walking its
// ~90 chunks layer by layer took 0.46 ms beside K6a's 1.8.)
__global__ void __launch_bounds__(64)
k_gavg_final(int nlay, int ng, const int* __restrict__ seg_chunk0 /*[ng+1]*/, const long long* __restrict__ seg_begin /*[ng+1]*/,
             const int* __restrict__ layer_method, const double* __restrict__ partial, const double* __restrict__ dp /*[nlay]*/,
             double scale /* (g*0.001*M/vmr) or <= 0: plain optical depth */, double* __restrict__ out /*[3][nlay][ng]*/) {
  const int g = blockIdx.x, l = blockIdx.y, lane = threadIdx.x;
  const int c0 = seg_chunk0[g], c1 = seg_chunk0[g + 1];
  const double ntot = (double)(seg_begin[g + 1] - seg_begin[g]);
  const double* q = partial + (size_t)l * 6;          // value k of the layer in chunk c: q[c * stride + k]
  const size_t stride = (size_t)nlay * 6;
  const double num = chunk_sum(q, stride, c0, c1, lane), den = chunk_sum(q + 1, stride, c0, c1, lane);
  const double den_nz = chunk_sum(q + 2, stride, c0, c1, lane), cnt = chunk_sum(q + 3, stride, c0, c1, lane);
  double mn = combine_chunks(q + 4, stride, c0, c1, lane, INFINITY, [](double a, double b) { return fmin(a, b); }, wave_min);
  double mx = combine_chunks(q + 5, stride, c0, c1, lane, -INFINITY, [](double a, double b) { return fmax(a, b); }, wave_max);
  if (lane != 0) return;
  double fit = 0.0;
  if (c1 > c0) {
    const int lm = layer_method[l];
    const double k = transmission_factor(lm);
    if (k > 0.0) fit = fabs(-log(1.0 - fmin(0.9999999999999999, num / den)) / (kD * k));
    else if (lm == M_LINEAR) fit = num / den;
    else if (lm == M_SQRT) { const double v = num / den; fit = v * v; }
    else if (cnt == ntot) fit = exp(num / den);       // logarithmic
    else if (cnt == 0.0) fit = 0.0;
    else fit = exp(num / den_nz) * (cnt / ntot);
    // :151-165
    fit = fmax(mn, fmin(fit, mx));
    if (mn > fit) mn = fit;
    if (mn > 0.0 && mn >= mx) { mn *= 0.99; mx *= 1.01; }
  } else {
    mn = 0.0; mx = 0.0;  // empty g point: zeros (:136-141)
  }
  const size_t o = (size_t)l * ng + g;
  // :170-184, same operation order: (const / vmr) * tau / dp
  const double tau[3] = {fit, mn, mx};
#pragma unroll
  for (int k = 0; k < 3; ++k) out[(size_t)k * nlay * ng + o] = scale > 0.0 ? scale * tau[k] / dp[l] : tau[k];
}

// K7a.  Planck LUT partials: partial[chunk][nlut]
__global__ void __launch_bounds__(GA_THREADS)
k_planck_lut_partial(int nlut, const Chunk* __restrict__ chunks, const double* __restrict__ wn_s,
                     const double* __restrict__ dwn_s, const double* __restrict__ hk_lut, double* __restrict__ partial) {
  __shared__ double s_red[4];
  const int tid = threadIdx.x;
  const ChunkWalk at = chunk_positions(chunks[blockIdx.x], tid);
  double freq[GA_PPT], pref[GA_PPT];
#pragma unroll
  for (int p = 0; p < GA_PPT; ++p) {
    freq[p] = ecckd::wn_to_freq(wn_s[at.ii[p]]);
    pref[p] = at.live[p] ? ecckd::planck_pref(dwn_s[at.ii[p]], freq[p]) : 0.0;
  }
  // (1.66e9 Planck evaluations for 231 temperatures x 7.2e6 points: 2.2 ms, ~60 % of the fp64 issue rate; the < 1 ulp exp and
  // division of fastmath.hpp with the waves' sums parked in LDS - no barrier in the loop - measured 2.4 ms: left as it was)
  for (int it = 0; it < nlut; ++it) {
    const double h = hk_lut[it];
    double v = 0.0;
#pragma unroll
    for (int p = 0; p < GA_PPT; ++p) v += pref[p] / (exp(freq[p] * h) - 1.0);
    v = block_sum_256(v, s_red);
    if (tid == 0) partial[(size_t)blockIdx.x * nlut + it] = v;
  }
}

// Row sums per g point (scale_lut.cpp:119-124): partial[chunk][nrows], gathered through the g-sorted order.
template <typename T>
__global__ void __launch_bounds__(GA_THREADS)
k_rowsum_partial(int nrows, size_t stride, const Chunk* __restrict__ chunks, const int32_t* __restrict__ order,
                 const T* __restrict__ rows, double* __restrict__ partial) {
  __shared__ double s_red[4];
  const int tid = threadIdx.x;
  const ChunkWalk at = chunk_positions(chunks[blockIdx.x], tid);
  size_t src[GA_PPT];
#pragma unroll
  for (int p = 0; p < GA_PPT; ++p) src[p] = (size_t)order[at.ii[p]];
  for (int r = 0; r < nrows; ++r) {
    double v = 0.0;
#pragma unroll
    for (int p = 0; p < GA_PPT; ++p) v += at.live[p] ? (double)rows[(size_t)r * stride + src[p]] : 0.0;
    v = block_sum_256(v, s_red);
    if (tid == 0) partial[(size_t)blockIdx.x * nrows + r] = v;
  }
}

// Erythemal weight per g point (lbl_fluxes.cpp:198-230): partial[chunk][2] = { sum ery * planck, sum planck }
__global__ void __launch_bounds__(GA_THREADS)
k_erythemal_partial(const Chunk* __restrict__ chunks, const double* __restrict__ wn_s, const double* __restrict__ dwn_s,
                    double* __restrict__ partial) {
  __shared__ double s_red[4];
  const int tid = threadIdx.x;
  const ChunkWalk at = chunk_positions(chunks[blockIdx.x], tid);
  double num = 0.0, den = 0.0;
#pragma unroll
  for (int p = 0; p < GA_PPT; ++p) {
    if (!at.live[p]) continue;
    const double wn = wn_s[at.ii[p]];
    const double wavelength_nm = 1.0e7 / wn;
    double ery = 0.0;
    if (wavelength_nm > 250.0 && wavelength_nm <= 298.0) ery = 1.0;
    if (wavelength_nm > 298.0 && wavelength_nm <= 328.0) ery = pow(10.0, 0.094 * (298.0 - wavelength_nm));
    if (wavelength_nm > 328.0 && wavelength_nm <= 400.0) ery = pow(10.0, 0.015 * (140.0 - wavelength_nm));
    ery = sqrt(ery);
    // planck_function(5777 K), planck_function.cpp:22-54
    const double freq = ecckd::wn_to_freq(wn);
    const double pref = ecckd::planck_pref(dwn_s[at.ii[p]], freq);
    const double pl = pref / (exp(ecckd::kPlanckOverBoltzmann * (freq / 5777.0)) - 1.0);
    num += ery * pl;
    den += pl;
  }
  num = block_sum_256(num, s_red);
  den = block_sum_256(den, s_red);
  if (tid == 0) {
    partial[(size_t)blockIdx.x * 2 + 0] = num;
    partial[(size_t)blockIdx.x * 2 + 1] = den;
  }
}

// K7b.  gpoint_fraction: the spectral width of every g point inside every interval (wavenumber1, wavenumber2], and its total
// width.  Inside its segment of the g-sorted order a g point's wavenumbers ascend, so an interval is a run of positions found by
// two binary searches; grid (nint, ng), block 64 (an interval holds n / (nint ng) points of a g point on average: a few hundred).
__global__ void __launch_bounds__(64)
k_gpoint_width(int nint, const long long* __restrict__ seg_begin /*[ng+1]*/, const double* __restrict__ wn_s,
               const double* __restrict__ dwn_s, const double* __restrict__ w1, const double* __restrict__ w2,
               double* __restrict__ width /*[ng][nint+1]*/) {
  const int iw = blockIdx.x, g = blockIdx.y;
  const long long b = seg_begin[g], e = seg_begin[g + 1];
  // wavenumbers ascend inside the segment: first position with wn > w1, first with wn > w2
  const double a1 = w1[iw], a2 = w2[iw];
  long long l = b, r = e;
  while (l < r) { long long m = (l + r) >> 1; if (wn_s[m] > a1) r = m; else l = m + 1; }
  const long long lo = l;
  r = e;
  while (l < r) { long long m = (l + r) >> 1; if (wn_s[m] > a2) r = m; else l = m + 1; }
  const long long hi = l;
  // four loads in flight per lane
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  long long i = lo + threadIdx.x;
  for (; i + 192 < hi; i += 256) { s0 += dwn_s[i]; s1 += dwn_s[i + 64]; s2 += dwn_s[i + 128]; s3 += dwn_s[i + 192]; }
  for (; i < hi; i += 64) s0 += dwn_s[i];
  const double s = wave_sum((s0 + s1) + (s2 + s3));
  if (threadIdx.x == 0) width[(size_t)g * (nint + 1) + iw] = s;
}

// The TOTAL width of a g point is a sum over its whole segment (n / ng points: 2e5 at 7.2e6 points and 38 g points), which one
// 64-thread block per g point used to walk with one load in flight per lane - 7.3 ms, 20 GB/s.  Now: the chunks of the segment
// (the same 2048-position chunks K6 works on) are summed by a block each, the chunk sums of a g point added in chunk order.
__global__ void __launch_bounds__(GA_THREADS)
k_width_chunk_sums(const Chunk* __restrict__ chunks, const double* __restrict__ dwn_s, double* __restrict__ partial) {
  __shared__ double s_red[4];
  const int tid = threadIdx.x;
  const ChunkWalk at = chunk_positions(chunks[blockIdx.x], tid);
  double s = 0.0;
#pragma unroll
  for (int p = 0; p < GA_PPT; ++p) s += at.live[p] ? dwn_s[at.ii[p]] : 0.0;
  s = block_sum_256(s, s_red);
  if (tid == 0) partial[blockIdx.x] = s;
}

// The second level of every reduction but K6's.  grid (ng, ceil(nrows / 4)), block 256: a wave per (g point, row) combines the
// chunk partials partial[chunk][nrows] of the g point (combine_chunks) into out[offset + row * row_stride + g * g_stride]:
// [nrows][ng] for the Planck table, the row sums and the erythemal pair, the last column of width[ng][nint + 1] for the totals.
__global__ void __launch_bounds__(256)
k_combine_chunks(int nrows, const int* __restrict__ seg_chunk0, const double* __restrict__ partial, double* __restrict__ out,
                 size_t row_stride, size_t g_stride, size_t offset) {
  const int g = blockIdx.x, lane = threadIdx.x & 63, r = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (r >= nrows) return;
  const double s = chunk_sum(partial + r, (size_t)nrows, seg_chunk0[g], seg_chunk0[g + 1], lane);
  if (lane == 0) out[offset + (size_t)r * row_stride + (size_t)g * g_stride] = s;
}

// the map back in wavenumber order: sorted position i holds wavenumber order[i]; its g point is the segment i lies in
__global__ void __launch_bounds__(256)
k_gmap_unsort(size_t n, size_t nassigned, int ng, const long long* __restrict__ seg_begin, const int32_t* __restrict__ order,
              const double* __restrict__ wn_s, const double* __restrict__ dwn_s, int32_t* __restrict__ g_point,
              double* __restrict__ wn, double* __restrict__ dwn) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int g = -1;
  if (i < nassigned) {
    int lo = 0, hi = ng;                       // the last g with seg_begin[g] <= i (empty g points share their begin with the next)
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (seg_begin[mid] <= (long long)i) lo = mid; else hi = mid; }
    g = lo;
  }
  const size_t j = (size_t)order[i];
  g_point[j] = g;
  wn[j] = wn_s[i];
  dwn[j] = dwn_s[i];
}

// ---------------------------------------------------------------------------------------------------------------- host
void gmap_free(ecckd_gmap* m) {
  if (!m) return;
  if (m->ctx) (void)hipStreamSynchronize(m->ctx->stream);
  for (void* b : m->blocks) (void)hipFree(b);
  delete m;
}

// A map under construction: whatever leaves the constructor early (ECCKD_HIP_CHECK, ECCKD_REQUIRE) frees it on the way out.
struct GmapDeleter { void operator()(ecckd_gmap* m) const { gmap_free(m); } };
typedef std::unique_ptr<ecckd_gmap, GmapDeleter> GmapPtr;

// a device array that lives as long as its scope: the temporaries of ecckd_gmap_create
template <typename T>
struct DevTemp {
  T* p = nullptr;
  DevTemp() = default;
  DevTemp(const DevTemp&) = delete;
  DevTemp& operator=(const DevTemp&) = delete;
  hipError_t alloc(size_t count) { return hipMalloc((void**)&p, count * sizeof(T)); }
  ~DevTemp() { if (p) (void)hipFree(p); }
};

// The work buffer holds at least `bytes` afterwards.  It is released before it is regrown, and a released buffer has size 0:
// a failed regrowth leaves nothing that a later, smaller request could take for a buffer.
int gmap_release_work(ecckd_gmap* m) {
  m->work_bytes = 0;
  if (!m->work) return ECCKD_OK;
  ECCKD_HIP_CHECK(hipStreamSynchronize(m->ctx->stream));
  ECCKD_HIP_CHECK(m->give_back(m->work));
  return ECCKD_OK;
}
int gmap_work(ecckd_gmap* m, size_t bytes) {
  if (bytes <= m->work_bytes) return ECCKD_OK;
  ECCKD_CHECK(gmap_release_work(m));
  ECCKD_HIP_CHECK(m->alloc(&m->work, bytes));
  m->work_bytes = bytes;
  return ECCKD_OK;
}

// The work buffer cut into N pieces of bytes[i] each (gmap_layout.hpp), every piece on a 256-byte boundary; ptr[i] is where
// piece i begins.  The pieces live until the next call that takes the work buffer.
template <size_t N>
int carve_work(ecckd_gmap* m, const size_t (&bytes)[N], double* (&ptr)[N]) {
  size_t off[N];
  ECCKD_CHECK(gmap_work(m, L::carve(bytes, off)));
  for (size_t i = 0; i < N; ++i) ptr[i] = (double*)((char*)m->work + off[i]);
  return ECCKD_OK;
}

// f with the device array p as the type it has (ECCKD_F32 or ECCKD_F64; the caller has checked that it is one of them)
template <typename F>
void with_type(const void* p, int type, F f) {
  if (type == ECCKD_F32) f((const float*)p); else f((const double*)p);
}

// where k_combine_chunks puts row r of g point g: out[offset + r * row_stride + g * g_stride]
struct OutPlace { size_t row_stride, g_stride, offset; };

// One segmented reduction of nrows rows over the map: launch_partial(grid, block) starts the partial kernel that fills
// d_part [nchunk][nrows] - if the map has a chunk at all -, k_combine_chunks adds the chunk partials per g point into d_out;
// with h_out, [nrows][ng] doubles from d_out are copied back.
template <typename LaunchPartial>
int reduce_rows(ecckd_gmap* m, int nrows, double* d_part, double* d_out, OutPlace at, double* h_out, LaunchPartial launch_partial) {
  ecckd_ctx* ctx = m->ctx;
  if (!m->chunks.empty()) launch_partial(dim3((unsigned)m->chunks.size()), dim3(GA_THREADS));
  hipLaunchKernelGGL(k_combine_chunks, dim3(m->ng, (nrows + 3) / 4), dim3(256), 0, ctx->stream, nrows, m->d_seg_chunk0, d_part,
                     d_out, at.row_stride, at.g_stride, at.offset);
  ECCKD_HIP_CHECK(hipGetLastError());
  return h_out ? ecckd_d2h(ctx, h_out, d_out, (size_t)nrows * m->ng * sizeof(double)) : ECCKD_OK;
}

}  // namespace

int ecckd::gmap_natural(ecckd_gmap* m, const int32_t** d_g_point, const double** d_wavenumber, const double** d_d_wavenumber) {
  if (!m->nat_g) {
    ecckd_ctx* ctx = m->ctx;
    ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
    // allocated into locals and published together: a failure on the way leaves the map as it was
    int32_t* g = nullptr; double* wn = nullptr; double* dwn = nullptr;
    hipError_t e = m->alloc(&g, m->n * sizeof(int32_t));
    if (e == hipSuccess) e = m->alloc(&wn, m->n * sizeof(double));
    if (e == hipSuccess) e = m->alloc(&dwn, m->n * sizeof(double));
    if (e == hipSuccess) {
      hipLaunchKernelGGL(k_gmap_unsort, dim3((unsigned)((m->n + 255) / 256)), dim3(256), 0, ctx->stream, m->n, m->nassigned, m->ng,
                         m->d_seg_begin, m->order, m->wn_s, m->dwn_s, g, wn, dwn);
      e = hipGetLastError();
    }
    if (e != hipSuccess) {
      (void)m->give_back(g); (void)m->give_back(wn); (void)m->give_back(dwn);
      return ecckd::fail(e == hipErrorOutOfMemory ? ECCKD_OUT_OF_MEMORY : ECCKD_UNEXPECTED_EXCEPTION,
                         "the g-point map in wavenumber order: %s", hipGetErrorString(e));
    }
    m->nat_g = g; m->nat_wn = wn; m->nat_dwn = dwn;
  }
  *d_g_point = m->nat_g; *d_wavenumber = m->nat_wn; *d_d_wavenumber = m->nat_dwn;
  return ECCKD_OK;
}

extern "C" {

int ecckd_gmap_create(ecckd_ctx* ctx, size_t nwav, const int32_t* d_g_point, int ng, const double* d_wavenumber,
                      const double* d_d_wavenumber, ecckd_gmap** out) {
  ECCKD_REQUIRE(ctx && out && d_g_point && d_wavenumber && d_d_wavenumber, "ecckd_gmap_create: NULL argument");
  *out = nullptr;
  ECCKD_REQUIRE(nwav > 0 && nwav < (size_t)0x7fffffff && ng > 0, "ecckd_gmap_create: bad sizes (nwav=%zu, ng=%d)", nwav, ng);
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  GmapPtr m(new ecckd_gmap());
  m->ctx = ctx; m->n = nwav; m->ng = ng;
  DevTemp<double> key;
  DevTemp<int> counts_flag;       // [ng] points per g point | [1] flag
  DevTemp<int32_t> rank;
  ECCKD_HIP_CHECK(key.alloc(nwav));
  ECCKD_HIP_CHECK(counts_flag.alloc((size_t)ng + 1));
  ECCKD_HIP_CHECK(rank.alloc(nwav));
  ECCKD_HIP_CHECK(m->alloc(&m->order, nwav * sizeof(int32_t)));
  ECCKD_HIP_CHECK(m->alloc(&m->wn_s, nwav * sizeof(double)));
  ECCKD_HIP_CHECK(m->alloc(&m->dwn_s, nwav * sizeof(double)));
  int* d_flag = counts_flag.p + ng;
  ECCKD_HIP_CHECK(hipMemsetAsync(counts_flag.p, 0, (size_t)(ng + 1) * sizeof(int), ctx->stream));
  const unsigned eb = (unsigned)((nwav + 255) / 256);
  hipLaunchKernelGGL(k_gmap_keys, dim3(eb), dim3(256), 0, ctx->stream, nwav, d_g_point, ng, key.p, counts_flag.p, d_flag);
  ECCKD_HIP_CHECK(hipGetLastError());
  const int64_t b0 = 0, b1 = (int64_t)nwav - 1;
  ECCKD_CHECK(ecckd_stable_argsort_bands_dev(ctx, nwav, key.p, 1, &b0, &b1, rank.p, m->order));
  hipLaunchKernelGGL(k_gmap_gather, dim3(eb), dim3(256), 0, ctx->stream, nwav, m->order, d_wavenumber, d_d_wavenumber,
                     m->wn_s, m->dwn_s);
  ECCKD_HIP_CHECK(hipGetLastError());
  std::vector<int> counts(ng + 1);
  ECCKD_CHECK(ecckd_d2h(ctx, counts.data(), counts_flag.p, (size_t)(ng + 1) * sizeof(int)));
  ECCKD_REQUIRE(!(counts[ng] & 1), "ecckd_gmap_create: g_point contains values >= ng (%d)", ng);
  m->seg_begin.assign(ng + 1, 0);
  for (int g = 0; g < ng; ++g) m->seg_begin[g + 1] = m->seg_begin[g] + counts[g];
  m->nassigned = (size_t)m->seg_begin[ng];
  // wavenumbers must ascend inside each g point (they do when the input grid ascends: the sort is stable)
  ECCKD_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(int), ctx->stream));
  if (m->nassigned > 1) {
    hipLaunchKernelGGL(k_gmap_check, dim3((unsigned)((m->nassigned + 255) / 256)), dim3(256), 0, ctx->stream, m->nassigned,
                       m->order, d_g_point, m->wn_s, d_flag);
    ECCKD_HIP_CHECK(hipGetLastError());
  }
  int flag = 0;
  ECCKD_CHECK(ecckd_d2h(ctx, &flag, d_flag, sizeof(int)));
  ECCKD_REQUIRE(!flag, "ecckd_gmap_create: wavenumber must be ascending");
  L::cut_chunks(m->seg_begin, m->chunks, m->seg_chunk0);
  ECCKD_HIP_CHECK(m->alloc(&m->d_chunks, std::max<size_t>(m->chunks.size(), 1) * sizeof(Chunk)));
  ECCKD_HIP_CHECK(m->alloc(&m->d_seg_chunk0, (size_t)(ng + 1) * sizeof(int)));
  ECCKD_HIP_CHECK(m->alloc(&m->d_seg_begin, (size_t)(ng + 1) * sizeof(long long)));
  ECCKD_HIP_CHECK(hipMemcpyAsync(m->d_chunks, m->chunks.data(), m->chunks.size() * sizeof(Chunk), hipMemcpyHostToDevice, ctx->stream));
  ECCKD_HIP_CHECK(hipMemcpyAsync(m->d_seg_chunk0, m->seg_chunk0.data(), (size_t)(ng + 1) * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  ECCKD_HIP_CHECK(hipMemcpyAsync(m->d_seg_begin, m->seg_begin.data(), (size_t)(ng + 1) * sizeof(long long), hipMemcpyHostToDevice, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  *out = m.release();
  return ECCKD_OK;
}

int ecckd_gmap_destroy(ecckd_gmap* m) {
  gmap_free(m);
  return ECCKD_OK;
}

// number of wavenumbers in each g point (create_look_up_table.cpp:111-118 detects empty ones)
int ecckd_gmap_counts(ecckd_gmap* m, int64_t* h_counts) {
  ECCKD_REQUIRE(m && h_counts, "ecckd_gmap_counts: NULL argument");
  for (int g = 0; g < m->ng; ++g) h_counts[g] = m->seg_begin[g + 1] - m->seg_begin[g];
  return ECCKD_OK;
}

int ecckd_average_to_gpoints(ecckd_gmap* m, int nlay, const double* h_pressure_hl, const double* h_temperature_fl,
                             const double* d_ssi, const void* d_od, int od_type, size_t od_stride,
                             int averaging_method, double reference_surface_vmr, double* h_molar_abs,
                             double* h_min_molar_abs, double* h_max_molar_abs) {
  ECCKD_REQUIRE(m && h_pressure_hl && d_od && h_molar_abs && nlay > 0, "ecckd_average_to_gpoints: bad argument");
  ECCKD_REQUIRE((h_temperature_fl != nullptr) != (d_ssi != nullptr),
                "ecckd_average_to_gpoints: give either temperature_fl (longwave) or ssi (shortwave)");
  ECCKD_REQUIRE(od_type == ECCKD_F32 || od_type == ECCKD_F64, "ecckd_average_to_gpoints: od_type must be 4 or 8");
  ECCKD_REQUIRE(od_stride >= m->n, "ecckd_average_to_gpoints: od_stride < nwav");
  const bool known = averaging_method == M_LINEAR || averaging_method == M_TRANS || averaging_method == M_TRANS2 ||
                     averaging_method == M_SQRT || averaging_method == M_LOG || averaging_method == M_TRANS3 ||
                     averaging_method == M_TRANS10 || averaging_method == M_HYBRID;
  // average_optical_depth.cpp:128-131
  ECCKD_REQUIRE(known, "averaging_method %d not understood", averaging_method);
  ecckd_ctx* ctx = m->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int ng = m->ng;
  const size_t nchunk = m->chunks.size();
  // host-side per-layer tables
  std::vector<double> hk(nlay, 0.0), dp(nlay);
  std::vector<int> lm(nlay, averaging_method);
  for (int l = 0; l < nlay; ++l) {
    dp[l] = h_pressure_hl[l + 1] - h_pressure_hl[l];
    if (h_temperature_fl) hk[l] = ecckd::kPlanckOverBoltzmann / h_temperature_fl[l];
    if (averaging_method == M_HYBRID) {
      // :101-126: logarithmic where pressure_fl > 100 hPa, transmission-3 above
      const double pfl = 0.5 * (h_pressure_hl[l] + h_pressure_hl[l + 1]);
      lm[l] = pfl > 100.0e2 ? M_LOG : M_TRANS3;
    }
  }
  double* piece[3];
  ECCKD_CHECK(carve_work(m, L::average(nchunk, ng, nlay).bytes, piece));
  double *d_part = piece[0], *d_out = piece[1], *d_hk = piece[2], *d_dp = d_hk + nlay;
  int* d_lm = (int*)(d_dp + nlay);
  ECCKD_HIP_CHECK(hipMemcpyAsync(d_hk, hk.data(), nlay * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ECCKD_HIP_CHECK(hipMemcpyAsync(d_dp, dp.data(), nlay * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ECCKD_HIP_CHECK(hipMemcpyAsync(d_lm, lm.data(), nlay * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // hk/dp/lm are stack-owned
  if (nchunk > 0)
    with_type(d_od, od_type, [&](auto* od) {
      hipLaunchKernelGGL(k_gavg_partial, dim3((unsigned)nchunk), dim3(GA_THREADS), (size_t)nlay * 6 * (GA_THREADS / 64) * sizeof(double),
                         ctx->stream, nlay, od_stride, m->d_chunks, m->order, m->wn_s, m->dwn_s, od,
                         h_temperature_fl ? d_hk : nullptr, d_ssi, d_lm, d_part);
    });
  // :170-173 (ACCEL_GRAVITY * 0.001 * MOLAR_MASS_DRY_AIR) / reference_surface_vmr
  const double scale = reference_surface_vmr > 0.0 ? (ECCKD_ACCEL_GRAVITY * 0.001 * 28.970) / reference_surface_vmr : -1.0;
  hipLaunchKernelGGL(k_gavg_final, dim3(ng, nlay), dim3(64), 0, ctx->stream, nlay, ng, m->d_seg_chunk0, m->d_seg_begin, d_lm,
                     d_part, d_dp, scale, d_out);
  ECCKD_HIP_CHECK(hipGetLastError());
  const size_t one = (size_t)nlay * ng * sizeof(double);
  ECCKD_HIP_CHECK(hipMemcpyAsync(h_molar_abs, d_out, one, hipMemcpyDeviceToHost, ctx->stream));
  if (h_min_molar_abs) ECCKD_HIP_CHECK(hipMemcpyAsync(h_min_molar_abs, d_out + (size_t)nlay * ng, one, hipMemcpyDeviceToHost, ctx->stream));
  if (h_max_molar_abs) ECCKD_HIP_CHECK(hipMemcpyAsync(h_max_molar_abs, d_out + 2 * (size_t)nlay * ng, one, hipMemcpyDeviceToHost, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return ECCKD_OK;
}

int ecckd_gpoint_fraction(ecckd_gmap* m, int nint, const double* h_wavenumber1, const double* h_wavenumber2,
                          double* h_gpoint_fraction) {
  ECCKD_REQUIRE(m && nint > 0 && h_wavenumber1 && h_wavenumber2 && h_gpoint_fraction, "ecckd_gpoint_fraction: bad argument");
  ecckd_ctx* ctx = m->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int ng = m->ng;
  double* piece[4];
  ECCKD_CHECK(carve_work(m, L::fraction(m->chunks.size(), ng, nint).bytes, piece));
  double *d_width = piece[0], *d_w1 = piece[1], *d_w2 = piece[2], *d_csum = piece[3];
  ECCKD_CHECK(ecckd_h2d(ctx, d_w1, h_wavenumber1, (size_t)nint * sizeof(double)));
  ECCKD_CHECK(ecckd_h2d(ctx, d_w2, h_wavenumber2, (size_t)nint * sizeof(double)));
  hipLaunchKernelGGL(k_gpoint_width, dim3(nint, ng), dim3(64), 0, ctx->stream, nint, m->d_seg_begin, m->wn_s, m->dwn_s,
                     d_w1, d_w2, d_width);
  // the total widths: one row, into the last column of width[ng][nint + 1]
  ECCKD_CHECK(reduce_rows(m, 1, d_csum, d_width, OutPlace{0, (size_t)nint + 1, (size_t)nint}, nullptr, [&](dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_width_chunk_sums, grid, block, 0, ctx->stream, m->d_chunks, m->dwn_s, d_csum);
  }));
  std::vector<double> width((size_t)ng * (nint + 1));
  ECCKD_CHECK(ecckd_d2h(ctx, width.data(), d_width, width.size() * sizeof(double)));
  for (int g = 0; g < ng; ++g)
    for (int iw = 0; iw < nint; ++iw)  // :542-546
      h_gpoint_fraction[(size_t)g * nint + iw] = width[(size_t)g * (nint + 1) + iw] / width[(size_t)g * (nint + 1) + nint];
  return ECCKD_OK;
}

int ecckd_planck_lut(ecckd_gmap* m, int nlut, const double* h_temperature_lut, double* h_planck_lut) {
  ECCKD_REQUIRE(m && nlut > 0 && h_temperature_lut && h_planck_lut, "ecckd_planck_lut: bad argument");
  ecckd_ctx* ctx = m->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  std::vector<double> hk(nlut);
  for (int i = 0; i < nlut; ++i) {
    ECCKD_REQUIRE(h_temperature_lut[i] > 0.0, "ecckd_planck_lut: temperatures must be positive");
    hk[i] = ecckd::kPlanckOverBoltzmann / h_temperature_lut[i];
  }
  double* piece[3];
  ECCKD_CHECK(carve_work(m, L::planck_lut(m->chunks.size(), m->ng, nlut).bytes, piece));
  double *d_part = piece[0], *d_hk = piece[2];
  ECCKD_CHECK(ecckd_h2d(ctx, d_hk, hk.data(), (size_t)nlut * sizeof(double)));
  return reduce_rows(m, nlut, d_part, piece[1], OutPlace{(size_t)m->ng, 1, 0}, h_planck_lut, [&](dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_planck_lut_partial, grid, block, 0, ctx->stream, nlut, m->d_chunks, m->wn_s, m->dwn_s, d_hk, d_part);
  });
}

int ecckd_gmap_sum_rows(ecckd_gmap* m, int nrows, const void* d_rows, int rows_type, size_t row_stride, double* h_sums) {
  ECCKD_REQUIRE(m && nrows > 0 && d_rows && h_sums, "ecckd_gmap_sum_rows: bad argument");
  ECCKD_REQUIRE(rows_type == ECCKD_F32 || rows_type == ECCKD_F64, "ecckd_gmap_sum_rows: rows_type must be ECCKD_F32 or ECCKD_F64");
  ECCKD_REQUIRE(row_stride >= m->n, "ecckd_gmap_sum_rows: row stride %zu shorter than the spectrum (%zu)", row_stride, m->n);
  ecckd_ctx* ctx = m->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  double* piece[2];
  ECCKD_CHECK(carve_work(m, L::rows(m->chunks.size(), m->ng, nrows).bytes, piece));
  return reduce_rows(m, nrows, piece[0], piece[1], OutPlace{(size_t)m->ng, 1, 0}, h_sums, [&](dim3 grid, dim3 block) {
    with_type(d_rows, rows_type, [&](auto* rows) {
      hipLaunchKernelGGL(k_rowsum_partial, grid, block, 0, ctx->stream, nrows, row_stride, m->d_chunks, m->order, rows, piece[0]);
    });
  });
}

int ecckd_gmap_erythemal_spectrum(ecckd_gmap* m, double* h_erythemal) {
  ECCKD_REQUIRE(m && h_erythemal, "ecckd_gmap_erythemal_spectrum: NULL argument");
  ecckd_ctx* ctx = m->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int ng = m->ng;
  double* piece[2];
  ECCKD_CHECK(carve_work(m, L::rows(m->chunks.size(), ng, 2).bytes, piece));
  std::vector<double> nd(2 * (size_t)ng);         // numerators [ng] | denominators [ng]
  ECCKD_CHECK(reduce_rows(m, 2, piece[0], piece[1], OutPlace{(size_t)ng, 1, 0}, nd.data(), [&](dim3 grid, dim3 block) {
    hipLaunchKernelGGL(k_erythemal_partial, grid, block, 0, ctx->stream, m->d_chunks, m->wn_s, m->dwn_s, piece[0]);
  }));
  for (int g = 0; g < ng; ++g) h_erythemal[g] = nd[g] / nd[(size_t)ng + g];
  return ECCKD_OK;
}

}  // extern "C"
