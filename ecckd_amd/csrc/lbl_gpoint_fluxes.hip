// lbl_gpoint_fluxes.hip - line-by-line longwave fluxes of one column resolved per g point (lw_spectra.cpp:222-257): the
// Planck function (planck_function.cpp:22-54), both sweeps of radiative_transfer_lw (radiative_transfer_lw.cpp:27-60, unit
// surface emissivity, diffusivity 1.66 - what k_lbl_fluxes_lw does with nangle = 0, expression by expression) and the sum of
// the spectral flux over the wavenumbers of every g point in ONE pass over the optical depths.  No (nlay+1) x nwav flux
// matrix exists on this path; the other output mode of the same kernel writes exactly that matrix (FLOAT rows) for the
// caller that wants the spectrum, with the broadband sums.
//
// Shape.  A g point is a scattered set of wavenumbers.  Walking the g-sorted permutation would make every load of the
// 2 x nlay optical depths of a point a 4-byte gather (one cache line per lane), so the kernel walks the spectrum in NATURAL
// order - one thread per wavenumber, 256 consecutive wavenumbers per tile, every row load 1 KB contiguous per block - and
// bins inside the block:
//   * once per tile the 256 points are ranked by (column, lane), column = g point of this launch / "no g point" / none: a
//     comparison count over the tile's keys in LDS, deterministic, the order inside a column is the wavenumber order;
//   * every flux a thread produces (nlay down, nlay + 1 up) goes to LDS at its RANK; after GF_LB levels the block turns
//     round: thread (level slot, segment of GF_SEG ranks) adds its segment left to right, one piece per column.  A piece
//     that starts its column is added to the block's accumulator acc[level][column] (LDS) by that thread alone; a piece
//     that continues a column from the segment before is parked and, after a barrier, added by the thread that owns the
//     column's first piece, segment after segment.  Every accumulator entry has one writer per batch and a fixed order:
//     no atomics, bitwise reproducible;
//   * a block walks `tiles_per_block` consecutive tiles (a function of nwav alone), then writes acc as its partial;
//     k_gf_combine adds the blocks' partials in block order.
// The accumulator has to fit into LDS: at most GF_ACC_BYTES / (16 (nlay+1)) columns per launch; a map with more g points is
// swept in several launches, each binning its own range of g points (ng = 32 ... 46 at 54 layers: one launch).
#include "common.hpp"
#include "fastmath.hpp"
#include "gmap.hpp"

#include <algorithm>
#include <vector>

namespace {

constexpr int GF_THREADS = 256;
constexpr int GF_LB = 8;                          // levels per batch
constexpr int GF_SEG = GF_THREADS / GF_LB;        // 32 segments ...
constexpr int GF_SEGLEN = GF_THREADS / GF_SEG;    // ... of 8 ranks
constexpr int GF_ROW = GF_THREADS + GF_SEG;       // a level's 256 fluxes, one pad per segment: segment stride 9 doubles = 18 banks
constexpr int GF_NONE = 0x7fffff;                 // column of a point that is binned nowhere
constexpr size_t GF_FIXED_LDS = (size_t)GF_LB * GF_ROW * 8 + (size_t)GF_LB * GF_SEG * 8 + 2 * GF_THREADS * 4;
constexpr size_t GF_ACC_BYTES = 65536 - GF_FIXED_LDS;   // static + dynamic LDS of a block stay within 64 KB
constexpr int GF_TARGET_BLOCKS = 2048;

__device__ constexpr double kPlanckH = 6.62606896e-34;
__device__ constexpr double kLightC = 2.99792458e8;
__device__ constexpr double kPi = 3.14159265358979323846;

// dynamic LDS: acc[2 * nhl][ncols]
template <typename OdT, bool SPECTRAL>
__global__ void __launch_bounds__(GF_THREADS)
k_lbl_gpoint_fluxes_lw(int nlay, size_t nwav, size_t od_stride, int tiles_per_block, const double* __restrict__ hk,
                       const double* __restrict__ wn, const double* __restrict__ dwn, const OdT* __restrict__ od,
                       const int32_t* __restrict__ g_point /* NULL: every point in column 0 */, int g0, int gcount,
                       int col_unassigned /* column of g_point < 0, or -1 */, int ncols, double* __restrict__ partial,
                       float* __restrict__ spec_dn, float* __restrict__ spec_up, size_t spec_stride) {
  extern __shared__ double s_acc[];
  __shared__ double s_f[GF_LB * GF_ROW];
  __shared__ double s_cont[GF_LB * GF_SEG];
  __shared__ __align__(16) int s_raw[GF_THREADS];
  __shared__ int s_key[GF_THREADS];
  const int nhl = nlay + 1;
  const int tid = threadIdx.x;
  const int nacc = 2 * nhl * ncols;
  for (int t = tid; t < nacc; t += GF_THREADS) s_acc[t] = 0.0;
  // this thread as an adder: level slot and segment
  const int slot = tid / GF_SEG, seg = tid % GF_SEG, base = seg * GF_SEGLEN;
  const double sec = ECCKD_LW_DIFFUSIVITY;
  const double rsec = 1.0 / sec;
  const double inv_cm_2_Hz = 100.0 * kLightC;
  const int nrows = 2 * nlay + 1;                 // fluxes a point produces: nlay down (levels 1..nlay), nlay + 1 up

  const size_t tile0 = (size_t)blockIdx.x * tiles_per_block;
  for (int it = 0; it < tiles_per_block; ++it) {
    const size_t i = (tile0 + it) * GF_THREADS + tid;
    if ((tile0 + it) * GF_THREADS >= nwav) break;                           // (block-uniform)
    const bool live = i < nwav;
    const size_t j = live ? i : nwav - 1;
    int key = GF_NONE;
    if (live) {
      if (!g_point) key = 0;
      else {
        const int g = g_point[j];
        if (g >= g0 && g < g0 + gcount) key = g - g0;
        else if (g < 0 && col_unassigned >= 0) key = col_unassigned;
      }
    }
    // ---- rank by (column, lane)
    const int mine = (key << 8) | tid;
    s_raw[tid] = mine;
    __syncthreads();
    int rank = 0;
    for (int q = 0; q < GF_THREADS; q += 4) {
      const int4 c = *reinterpret_cast<const int4*>(&s_raw[q]);
      rank += (c.x < mine) + (c.y < mine) + (c.z < mine) + (c.w < mine);
    }
    s_key[rank] = key;
    const int pos = rank + rank / GF_SEGLEN;
    __syncthreads();
    // ---- the pieces of this thread's segment: a break before rank base + q where the column changes
    unsigned brk = 0;
    for (int q = 1; q < GF_SEGLEN; ++q) brk |= (s_key[base + q] != s_key[base + q - 1]) ? (1u << q) : 0u;
    const bool cont_in = seg > 0 && s_key[base] == s_key[base - 1];
    const int tail_key = s_key[base + GF_SEGLEN - 1];
    // the column's first piece ends this segment and goes on in the next one: this thread collects the parked pieces
    const bool collects = seg + 1 < GF_SEG && s_key[base + GF_SEGLEN] == tail_key && tail_key != GF_NONE && !(brk == 0 && cont_in);

    // flux number `idx` of a point (in the order produced) -> accumulator row: down level l -> l, up level l -> nhl + l
    auto row_of = [&](int idx) { return idx < nlay ? idx + 1 : (idx == nlay ? nhl + nlay : nhl + 2 * nlay - idx); };
    auto reduce_batch = [&](int first_idx, int nb) {
      __syncthreads();
      const int r = row_of(first_idx + (slot < nb ? slot : 0));
      double* acc = s_acc + (size_t)r * ncols;
      if (slot < nb) {
        const double* f = s_f + slot * GF_ROW + base + seg;
        double sum = 0.0;
        int k = s_key[base];
        bool parked = cont_in;
        for (int q = 0; q < GF_SEGLEN; ++q) {
          if (q > 0 && ((brk >> q) & 1u)) {
            if (k != GF_NONE) { if (parked) s_cont[slot * GF_SEG + seg] = sum; else acc[k] += sum; }
            sum = 0.0; parked = false; k = s_key[base + q];
          }
          sum += f[q];
        }
        if (k != GF_NONE) { if (parked) s_cont[slot * GF_SEG + seg] = sum; else acc[k] += sum; }
      }
      __syncthreads();
      if (slot < nb && collects) {
        for (int s2 = seg + 1; s2 < GF_SEG && s_key[s2 * GF_SEGLEN] == tail_key; ++s2) {
          acc[tail_key] += s_cont[slot * GF_SEG + s2];
          if (s_key[s2 * GF_SEGLEN + GF_SEGLEN - 1] != tail_key) break;
        }
      }
    };
    int produced = 0;
    auto emit = [&](double f) {
      s_f[(produced % GF_LB) * GF_ROW + pos] = f;
      ++produced;
      if (produced % GF_LB == 0) reduce_batch(produced - GF_LB, GF_LB);
    };

    // ---- the column, as k_lbl_fluxes_lw computes it (nangle = 0)
    const double freq = wn[j] * inv_cm_2_Hz;
    const double pref = live ? (dwn[j] * 2.0 * kPlanckH * inv_cm_2_Hz * kPi / (kLightC * kLightC)) * (freq * freq * freq) : 0.0;
    auto planck = [&](int level) { return ecckd::div_fast(pref, ecckd::exp_fast(freq * hk[level]) - 1.0); };
    auto layer = [&](int l, double& eps, double& fac) {
      const double tau = (double)od[(size_t)l * od_stride + j];
      eps = 1.0 - ecckd::exp_fast(-sec * tau);
      fac = (eps > 1.0e-5) ? 1.0 - ecckd::div_fast(eps * rsec, tau) : 0.5 * eps;   // :41-43
    };
    double flux = 0.0;
    if (SPECTRAL && live) spec_dn[i] = 0.0f;                                  // nothing comes down at the top (:45)
    double b_prev = planck(0);
    for (int l = 0; l < nlay; ++l) {                                          // :45-50; dead lanes carry pref = 0
      double eps, fac;
      layer(l, eps, fac);
      const double b_next = planck(l + 1);
      flux = flux * (1.0 - eps) + b_prev * (eps - fac) + b_next * fac;
      if (SPECTRAL && live) spec_dn[(size_t)(l + 1) * spec_stride + i] = (float)flux;
      emit(flux);
      b_prev = b_next;
    }
    flux = b_prev * 1.0 + (1.0 - 1.0) * flux;                                 // :52-53
    if (SPECTRAL && live) spec_up[(size_t)nlay * spec_stride + i] = (float)flux;
    emit(flux);
    for (int l = nlay - 1; l >= 0; --l) {                                     // :55-59
      double eps, fac;
      layer(l, eps, fac);
      const double b_l = planck(l);
      flux = flux * (1.0 - eps) + b_prev * (eps - fac) + b_l * fac;
      if (SPECTRAL && live) spec_up[(size_t)l * spec_stride + i] = (float)flux;
      emit(flux);
      b_prev = b_l;
    }
    if (nrows % GF_LB) reduce_batch(nrows - nrows % GF_LB, nrows % GF_LB);
    __syncthreads();                                                          // s_raw / s_key / s_cont are rewritten by the next tile
  }
  __syncthreads();
  for (int t = tid; t < nacc; t += GF_THREADS) partial[(size_t)blockIdx.x * nacc + t] = s_acc[t];
}

// out[row][col_out(c)] = the blocks' partials added in block order; one thread per accumulator entry
__global__ void __launch_bounds__(256)
k_gf_combine(int nblk, int nacc, int ncols, int g0, int gcount, int out_cols, const double* __restrict__ partial,
             double* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nacc) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += partial[(size_t)b * nacc + e];
  const int r = e / ncols, c = e % ncols;
  out[(size_t)r * out_cols + (c < gcount ? g0 + c : out_cols - 1)] = s;
}

// One column.  d_g_point == NULL: one column of the accumulator (the broadband sum); otherwise ng g points + "none".
// h_out[2 * nhl][ng + 1]: rows 0..nhl-1 down, nhl.. up; column ng = the wavenumbers with no g point.
int run(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_temperature_hl, const double* d_wn, const double* d_dwn,
        const void* d_od, int od_type, size_t od_stride, const int32_t* d_g_point, int ng, float* d_spec_dn, float* d_spec_up,
        size_t spec_stride, std::vector<double>& h_out) {
  const int nhl = nlay + 1;
  const int out_cols = ng + 1;
  const int max_cols = (int)(GF_ACC_BYTES / ((size_t)2 * nhl * sizeof(double)));
  ECCKD_REQUIRE(max_cols >= 2, "line-by-line g-point fluxes: %d layers are more than the block's accumulator holds", nlay);
  std::vector<double> hk(nhl);
  for (int i = 0; i < nhl; ++i) {
    ECCKD_REQUIRE(h_temperature_hl[i] > 0.0, "line-by-line g-point fluxes: temperature_hl must be positive");
    hk[i] = (6.62606896e-34 / 1.3806504e-23) / h_temperature_hl[i];
  }
  const size_t ntiles = (nwav + GF_THREADS - 1) / GF_THREADS;
  const int tpb = (int)std::max<size_t>(1, (ntiles + GF_TARGET_BLOCKS - 1) / GF_TARGET_BLOCKS);   // a function of nwav alone
  const int nblk = (int)((ntiles + tpb - 1) / tpb);
  const size_t b_hk = ecckd_align_up((size_t)nhl * sizeof(double), 256);
  const size_t b_out = ecckd_align_up((size_t)2 * nhl * out_cols * sizeof(double), 256);
  const size_t b_part = ecckd_align_up((size_t)nblk * 2 * nhl * std::min(max_cols, out_cols) * sizeof(double), 256);
  ECCKD_CHECK(ecckd::ensure_scratch(ctx, b_hk + b_out + b_part));
  double* d_hk = (double*)ctx->scratch;
  double* d_out = (double*)((char*)ctx->scratch + b_hk);
  double* d_part = (double*)((char*)ctx->scratch + b_hk + b_out);
  ECCKD_CHECK(ecckd_h2d(ctx, d_hk, hk.data(), (size_t)nhl * sizeof(double)));
  ECCKD_HIP_CHECK(hipMemsetAsync(d_out, 0, (size_t)2 * nhl * out_cols * sizeof(double), ctx->stream));
  // the launches: g points [g0, g0 + gcount); the first one also bins the points without a g point
  for (int g0 = 0, pass = 0; pass == 0 || g0 < ng; ++pass) {
    const bool with_none = pass == 0;
    const int gcount = std::min(ng - g0, max_cols - (with_none ? 1 : 0));
    const int ncols = gcount + (with_none ? 1 : 0);
    const int col_un = (with_none && d_g_point) ? gcount : -1;
    const int nacc = 2 * nhl * ncols;
    const size_t lds = (size_t)nacc * sizeof(double);
    const bool spectral = d_spec_dn != nullptr;
#define GF_LAUNCH(T, S)                                                                                                        \
  hipLaunchKernelGGL((k_lbl_gpoint_fluxes_lw<T, S>), dim3((unsigned)nblk), dim3(GF_THREADS), lds, ctx->stream, nlay, nwav,     \
                     od_stride, tpb, (const double*)d_hk, d_wn, d_dwn, (const T*)d_od, d_g_point, g0, gcount, col_un, ncols,   \
                     d_part, d_spec_dn, d_spec_up, spec_stride)
    if (od_type == ECCKD_F32) { if (spectral) GF_LAUNCH(float, true); else GF_LAUNCH(float, false); }
    else { if (spectral) GF_LAUNCH(double, true); else GF_LAUNCH(double, false); }
#undef GF_LAUNCH
    ECCKD_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_gf_combine, dim3((unsigned)((nacc + 255) / 256)), dim3(256), 0, ctx->stream, nblk, nacc, ncols, g0, gcount,
                       out_cols, (const double*)d_part, d_out);
    ECCKD_HIP_CHECK(hipGetLastError());
    g0 += gcount;
  }
  h_out.resize((size_t)2 * nhl * out_cols);
  return ecckd_d2h(ctx, h_out.data(), d_out, h_out.size() * sizeof(double));
}

}  // namespace

extern "C" {

int ecckd_lbl_gpoint_fluxes_lw(ecckd_gmap* gmap, int nlay, const double* h_temperature_hl, const void* d_od, int od_type,
                               size_t od_stride, double* h_flux_dn, double* h_flux_up, double* h_bb_dn, double* h_bb_up) {
  ECCKD_REQUIRE(gmap && nlay > 0 && h_temperature_hl && d_od && h_flux_dn && h_flux_up, "ecckd_lbl_gpoint_fluxes_lw: bad argument");
  ECCKD_REQUIRE(od_type == ECCKD_F32 || od_type == ECCKD_F64, "ecckd_lbl_gpoint_fluxes_lw: od_type must be 4 or 8");
  ECCKD_REQUIRE(od_stride >= gmap->n, "ecckd_lbl_gpoint_fluxes_lw: od_stride (%zu) < nwav (%zu)", od_stride, gmap->n);
  ecckd_ctx* ctx = gmap->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int32_t* d_g = nullptr; const double* d_wn = nullptr; const double* d_dwn = nullptr;
  ECCKD_CHECK(ecckd::gmap_natural(gmap, &d_g, &d_wn, &d_dwn));
  const int nhl = nlay + 1, ng = gmap->ng;
  std::vector<double> out;
  ECCKD_CHECK(run(ctx, nlay, gmap->n, h_temperature_hl, d_wn, d_dwn, d_od, od_type, od_stride, d_g, ng, nullptr, nullptr, 0, out));
  for (int l = 0; l < nhl; ++l) {
    const double* dn = &out[(size_t)l * (ng + 1)];
    const double* up = &out[(size_t)(nhl + l) * (ng + 1)];
    double bdn = 0.0, bup = 0.0;                   // every wavenumber: the g points in order, then the points of none (:231-232)
    for (int g = 0; g <= ng; ++g) { bdn += dn[g]; bup += up[g]; }
    for (int g = 0; g < ng; ++g) { h_flux_dn[(size_t)l * ng + g] = dn[g]; h_flux_up[(size_t)l * ng + g] = up[g]; }
    if (h_bb_dn) h_bb_dn[l] = bdn;
    if (h_bb_up) h_bb_up[l] = bup;
  }
  return ECCKD_OK;
}

int ecckd_lbl_spectral_fluxes_lw(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_temperature_hl,
                                 const double* d_wavenumber, const double* d_d_wavenumber, const void* d_od, int od_type,
                                 size_t od_stride, float* d_flux_dn, float* d_flux_up, size_t flux_stride, double* h_bb_dn,
                                 double* h_bb_up) {
  ECCKD_REQUIRE(ctx && nlay > 0 && nwav > 0 && h_temperature_hl && d_wavenumber && d_d_wavenumber && d_od && d_flux_dn && d_flux_up,
                "ecckd_lbl_spectral_fluxes_lw: bad argument");
  ECCKD_REQUIRE(od_type == ECCKD_F32 || od_type == ECCKD_F64, "ecckd_lbl_spectral_fluxes_lw: od_type must be 4 or 8");
  ECCKD_REQUIRE(od_stride >= nwav, "ecckd_lbl_spectral_fluxes_lw: od_stride (%zu) < nwav (%zu)", od_stride, nwav);
  ECCKD_REQUIRE(flux_stride >= nwav, "ecckd_lbl_spectral_fluxes_lw: flux_stride (%zu) < nwav (%zu)", flux_stride, nwav);
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int nhl = nlay + 1;
  std::vector<double> out;
  ECCKD_CHECK(run(ctx, nlay, nwav, h_temperature_hl, d_wavenumber, d_d_wavenumber, d_od, od_type, od_stride, nullptr, 0, d_flux_dn,
                  d_flux_up, flux_stride, out));
  for (int l = 0; l < nhl; ++l) {
    if (h_bb_dn) h_bb_dn[l] = out[l];
    if (h_bb_up) h_bb_up[l] = out[nhl + l];
  }
  return ECCKD_OK;
}

}  // extern "C"
