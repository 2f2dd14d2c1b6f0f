// find_g.hip - K4/K5: the g-point search of find_g_points on gfx950.
//
// K4  ecckd_gas_create_lw    gas preparation, reference src/ecckd/find_g_points.cpp:872-1150:
//       gather-reorder the columns by rank, Planck function, LW radiative
//       transfer of background+target, heating rate, surface/TOA flux rows,
//       averaging metric.  One sweep; results stay resident in HBM in SORTED
//       order, (level, wavenumber) row-major.
// K5  ecckd_calc_error_batch the interval error of CkdEquipartition::calc_error
//       (find_g_points.cpp:291-405) = fit_optical_depth_lw (:54-106) +
//       calc_cost_function_lw (calc_cost_function_lw.cpp:24-110) +
//       radiative_transfer_lw_bb (radiative_transfer_lw.cpp:87-142), for a whole
//       BATCH of intervals per call (the reference evaluates them one by one
//       from OpenMP threads, equipartition.h:98-116).
//
// Design (MI355X): everything the fit and the "true" side of the cost need is a
// plain SUM over the interval of per-point rows that do not depend on the
// interval (metric*planck, planck, hr, flux rows).  K4 therefore also reduces
// those rows over fixed 256-point tiles once; K5a sums tiles + the two ragged
// ends, so the only pass that streams the band per evaluation is the grey-
// optical-depth radiative transfer K5c: it reads planck (nlay+1) and background
// optical depth (nlay) rows = (2*nlay+1)*8 B per point, coalesced 512-B wave
// loads, with per-half-level flux sums reduced wave -> block -> interval in a
// fixed order (bitwise reproducible; no float atomics).
#include "chunk_layout.hpp"
#include "sweep_layout.hpp"
#include "common.hpp"
#include "partition_search.hpp"
#include "rt_device.hpp"

#include <atomic>
#include <cmath>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <type_traits>
#include <vector>
#include <immintrin.h>

namespace {

constexpr int TILE = 256;          // points per tile sum
// wave priorities of the K5c phases (s_setprio): measured choices, see DESIGN.md
#ifndef ECCKD_PRIO_LOAD
#define ECCKD_PRIO_LOAD 3
#endif
#ifndef ECCKD_PRIO_SWEEP1
#define ECCKD_PRIO_SWEEP1 1
#endif
#ifndef ECCKD_PRIO_SWEEP2
#define ECCKD_PRIO_SWEEP2 0
#endif
typedef float float_x2 __attribute__((ext_vector_type(2)));
typedef float_x2 float_x2_store;
constexpr int RT_THREADS = 256;    // K5c block
constexpr int PREP_THREADS = 256;  // K4 block

__device__ constexpr double kD = ECCKD_LW_DIFFUSIVITY;

// ---------------------------------------------------------------------------
// deterministic reductions (rt_device.hpp)
using ecckd::wave_sum; using ecckd::block_sum_256; using ecckd::block_sum_256_x3;

}  // namespace

#include "gas.hpp"

namespace {

// ---------------------------------------------------------------------------
// K4 helpers
__global__ void __launch_bounds__(256)
k_invert_rank(size_t n, const int32_t* __restrict__ rank, int32_t* __restrict__ ireorder, int* __restrict__ err) {
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int32_t r = rank[j];
  if (r < 0 || (size_t)r >= n) { atomicOr(err, 2); return; }
  ireorder[r] = (int32_t)j;  // find_g_points.cpp:779-780
}

__global__ void __launch_bounds__(256)
k_check_perm(size_t n, const int32_t* __restrict__ ireorder, int* __restrict__ err) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && ireorder[i] < 0) atomicOr(err, 2);
}

// The Planck matrix of a gas's ordering alone: planck_hl[lev][i] for the wavenumber whose rank is i, evaluated exactly as
// the preparation kernels do (same expression, same exp / division), so that a process which does not search the FIRST
// gas can still hold the matrix the reference keeps from it for all later gases (find_g_points.cpp:529, :970-984).
__global__ void __launch_bounds__(256)
k_planck_sorted(int nhl, size_t n, const int32_t* __restrict__ ireorder, const double* __restrict__ hk,
                const double* __restrict__ wn, const double* __restrict__ dwn, double* __restrict__ planck_hl) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t j = (size_t)ireorder[i];
  const double w = wn[j], dw = dwn[j];
  const double freq = ecckd::wn_to_freq(w);
  const double pref = ecckd::planck_pref(dw, freq);
  for (int lev = 0; lev < nhl; ++lev) planck_hl[(size_t)lev * n + i] = ecckd::planck(pref, freq, hk[lev]);
}

__device__ __forceinline__ double metric_of(int method, double od) {
  // find_g_points.cpp:1119-1150
  switch (method) {
    case ECCKD_AVG_TRANSMISSION: return 1.0 - exp(-od * kD);
    case ECCKD_AVG_TRANSMISSION_2: return 1.0 - exp(-od * kD * 2.0);
    case ECCKD_AVG_SQUARE_ROOT: return sqrt(od);
    default: return od;  // linear, logarithmic, total-transmission
  }
}

// K4 (LW).  One thread per SORTED wavenumber i; source column j = ireorder[i].
// Dynamic LDS: double[nlay][blockDim.x] for the down-sweep flux increments.
template <typename BgT, typename OdT>
__global__ void __launch_bounds__(PREP_THREADS)
k_gas_prep_lw(int nlay, size_t n, size_t src_stride, int method,
              const int32_t* __restrict__ ireorder, const double* __restrict__ hk /*[nhl] (h/k)/T*/,
              const double* __restrict__ conv /*[nlay]*/,
              const double* __restrict__ wn, const double* __restrict__ dwn,
              const BgT* __restrict__ bg_src, const OdT* __restrict__ od_src,
              const double* __restrict__ planck_reuse,
              double* __restrict__ wn_sorted, double* __restrict__ dwn_sorted,
              double* __restrict__ planck_hl, double* __restrict__ bg_od, double* __restrict__ w1,
              double* __restrict__ w2, double* __restrict__ cnt,
              double* __restrict__ hr, double* __restrict__ fds, double* __restrict__ fut) {
  extern __shared__ double s_col[];
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int tid = threadIdx.x, bs = blockDim.x;
  const size_t j = (size_t)ireorder[i];
  const bool is_log = (method == ECCKD_AVG_LOGARITHMIC);

  // planck_function.cpp:48-50 on the reordered wavenumbers (find_g_points.cpp:970-979)
  const double w = wn[j], dw = dwn[j];
  wn_sorted[i] = w;
  dwn_sorted[i] = dw;
  const double freq = ecckd::wn_to_freq(w);
  const double pref = ecckd::planck_pref(dw, freq);
  auto planck_at = [&](int lev) -> double {
    if (planck_reuse) return planck_reuse[(size_t)lev * n + i];
    return ecckd::planck(pref, freq, hk[lev]);
  };

  double b_prev = planck_at(0);
  if (!planck_reuse) planck_hl[i] = b_prev;
  double dn = 0.0;
  // inputs are fetched eight layers at a time, ahead of that chunk's stores: a load issued after a store waits for the
  // store to complete on this hardware, so one load per layer would cost one store latency per layer
  constexpr int CH = 8;
  for (int l0 = 0; l0 < nlay; l0 += CH) {
  double bgv[CH], odv[CH], plv[CH];
#pragma unroll
  for (int q = 0; q < CH; ++q) {
    const int lq = l0 + q < nlay ? l0 + q : nlay - 1;
    bgv[q] = bg_src ? (double)bg_src[(size_t)lq * src_stride + j] : 0.0;
    odv[q] = (double)od_src[(size_t)lq * src_stride + j];
    plv[q] = planck_reuse ? planck_reuse[(size_t)(lq + 1) * n + i] : 0.0;
  }
#pragma unroll
  for (int q = 0; q < CH; ++q) {
    const int l = l0 + q;
    if (l >= nlay) break;
    const double bg = bgv[q];
    const double od = odv[q];
    const double tau = bg + od;  // find_g_points.cpp:993
    // radiative_transfer_lw.cpp:41-43
    double eps, fac;
    ecckd::lw_layer(kD, 1.0 / kD, tau, eps, fac);
    const double b_next = planck_reuse ? plv[q] : planck_at(l + 1);
    const double dn_next = ecckd::lw_step(dn, eps, fac, b_prev, b_next);
    s_col[l * bs + tid] = dn_next - dn;
    const size_t o = (size_t)l * n + i;
    bg_od[o] = bg;
    if (!planck_reuse) planck_hl[(size_t)(l + 1) * n + i] = b_next;
    const double m = metric_of(method, od);
    if (!is_log) {
      // numerator row of fit_optical_depth_lw (find_g_points.cpp:61-62): metric * planck_hl(l+1)
      w1[o] = m * b_next;
    } else {
      // find_g_points.cpp:81-98: log(metric) weighted by planck_hl(l+1) over planck_hl(l), metric > 0 only
      const bool pos = m > 0.0;
      w1[o] = pos ? log(m) * b_next : 0.0;
      w2[o] = pos ? b_prev : 0.0;
      cnt[o] = pos ? 1.0 : 0.0;
    }
    dn = dn_next;
    b_prev = b_next;
  }
  }
  fds[i] = dn;  // flux_dn(end,__), find_g_points.cpp:1045
  // surface: emissivity 1, surf_planck = planck at temperature_hl(end) (:976-978, :987-988)
  double up = ecckd::lw_surface(dn, b_prev);
  for (int l0 = nlay - 1; l0 >= 0; l0 -= CH) {
  double bgv[CH], odv[CH], plv[CH];
#pragma unroll
  for (int q = 0; q < CH; ++q) {
    const int lq = l0 - q >= 0 ? l0 - q : 0;
    bgv[q] = bg_src ? (double)bg_src[(size_t)lq * src_stride + j] : 0.0;
    odv[q] = (double)od_src[(size_t)lq * src_stride + j];
    plv[q] = planck_reuse ? planck_reuse[(size_t)lq * n + i] : 0.0;
  }
#pragma unroll
  for (int q = 0; q < CH; ++q) {
    const int l = l0 - q;
    if (l < 0) break;
    const double tau = bgv[q] + odv[q];
    double eps, fac;
    ecckd::lw_layer(kD, 1.0 / kD, tau, eps, fac);
    const double b_l = planck_reuse ? plv[q] : planck_at(l);
    const double up_l = ecckd::lw_step(up, eps, fac, b_prev, b_l);
    // heating_rate.h:47-48
    hr[(size_t)l * n + i] = conv[l] * (s_col[l * bs + tid] - up + up_l);
    up = up_l;
    b_prev = b_l;
  }
  }
  fut[i] = up;  // flux_up(0,__), find_g_points.cpp:1052
}


// The second half of the scatter kernels: the filled tile leaves column by column.  my_rank: the rank of the tile's point
// `lane`, -1 past the end.
template <int NLAY, int PARTS, typename T>
__device__ __forceinline__ void scatter_tile_out(const T (&s_tile)[NLAY][65], int my_rank, size_t npad, T* __restrict__ dst) {
  constexpr int HP = NLAY / PARTS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  const size_t part = (size_t)(lane / HP) * npad;
  const int within = lane % HP;
  for (int p = wave; p < 64; p += 4) {
    const int r = __shfl(my_rank, p, 64);
    if (r < 0) break;
    if (lane < NLAY) dst[(part + (size_t)r) * HP + within] = s_tile[lane][p];
  }
}

// K4 fast path, step 1: transposing scatter.  src is (layer, wavenumber) in ORIGINAL order; the column of wavenumber j goes to
// its SORTED position rank[j], as PARTS runs of NLAY / PARTS layers: dst[PARTS][npad][NLAY / PARTS] (npad: n rounded up to whole
// waves).  Reads are coalesced rows through an LDS tile, each point's values leave as one wave store of PARTS contiguous
// segments.  The block of one run for 64 consecutive ranks is contiguous: that is what the preparation kernels copy into LDS
// (instead of 2*NLAY random 4-byte gathers per point, or NLAY-element columns read at a stride of NLAY*4 bytes).
template <int NLAY, typename SrcT, int PARTS>
__global__ void __launch_bounds__(256)
k_scatter_column_halves(size_t n, size_t npad, size_t src_stride, const int32_t* __restrict__ rank, const SrcT* __restrict__ src,
                        SrcT* __restrict__ dst) {
  __shared__ SrcT s_tile[NLAY][65];
  const size_t j0 = (size_t)blockIdx.x * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int l = wave; l < NLAY; l += 4) {
    const size_t j = j0 + lane;
    s_tile[l][lane] = (j < n) ? src[(size_t)l * src_stride + j] : (SrcT)0;
  }
  // the ranks of the tile's 64 points: one coalesced load per wave, handed out lane by lane below (a load per point inside the
  // loop made every store wait for its own memory latency)
  scatter_tile_out<NLAY, PARTS>(s_tile, j0 + lane < n ? rank[j0 + lane] : -1, npad, dst);
}

// The background of a longwave gas as a list of spectra that are merged on the way (ecckd_gas_create_lw_merged): by value in
// the kernel arguments, indexed with the (uniform) source counter.
constexpr int BG_MAX_SOURCES = 16;
struct BgSources {
  const void* od[BG_MAX_SOURCES];
  unsigned long long stride[BG_MAX_SOURCES];
  int type[BG_MAX_SOURCES];
};

// k_scatter_column_halves<NLAY, double, PARTS> of the merged background that is never stored: the tile is filled with
// sum over the sources, in order, of od_s[l][j] * scale[s][l] - the value ecckd_merge_spectrum_dev leaves source after source
// (read_merged_spectrum.cpp:152-166): the product is rounded, then the sum, the first source assigns.  Written with * and +
// under `fp contract(off)`: see the comment above merged_point in merge.hip.  A wave takes every fourth layer as above; the
// loop over its layers is the inner, unrolled one, so the loads of one source are all out before the first is used.
template <int NLAY, int PARTS>
__global__ void __launch_bounds__(256)
k_scatter_merged_halves(size_t n, size_t npad, const int32_t* __restrict__ rank, const BgSources src, int nsrc,
                        const double* __restrict__ scale /* [nsrc][NLAY] */, double* __restrict__ dst) {
#pragma clang fp contract(off)
  constexpr int LPW = (NLAY + 3) / 4;           // layers per wave
  __shared__ double s_tile[NLAY][65];
  const size_t j0 = (size_t)blockIdx.x * 64;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const size_t j = j0 + lane;
  const size_t jj = j < n ? j : n - 1;
  double tau[LPW];
#pragma unroll
  for (int k = 0; k < LPW; ++k) tau[k] = 0.0;
  for (int s = 0; s < nsrc; ++s) {
    const size_t stride = (size_t)src.stride[s];
    const double* __restrict__ sc = scale + (size_t)s * NLAY;
    double x[LPW];
    if (src.type[s] == ECCKD_F64) {
      const double* __restrict__ od = static_cast<const double*>(src.od[s]);
#pragma unroll
      for (int k = 0; k < LPW; ++k) {
        const int l = wave + 4 * k < NLAY ? wave + 4 * k : wave;
        x[k] = od[(size_t)l * stride + jj];
      }
    } else {
      const float* __restrict__ od = static_cast<const float*>(src.od[s]);
#pragma unroll
      for (int k = 0; k < LPW; ++k) {
        const int l = wave + 4 * k < NLAY ? wave + 4 * k : wave;
        x[k] = (double)od[(size_t)l * stride + jj];
      }
    }
#pragma unroll
    for (int k = 0; k < LPW; ++k) {
      const int l = wave + 4 * k < NLAY ? wave + 4 * k : wave;
      const double v = x[k] * sc[l];
      tau[k] = s == 0 ? v : tau[k] + v;
    }
  }
#pragma unroll
  for (int k = 0; k < LPW; ++k)
    if (wave + 4 * k < NLAY) s_tile[wave + 4 * k][lane] = tau[k];
  scatter_tile_out<NLAY, PARTS>(s_tile, j < n ? rank[j] : -1, npad, dst);
}

// K4 mirror path (same idea as K5c's, see k_rt_lw_bb_mirror): a pair of waves shares 64 points, the even
// wave prepares the upper NLAY/2 layers top-down (first sweep = downwelling from the top of the
// atmosphere), the odd wave the lower NLAY/2 layers bottom-up (first sweep = upwelling from the surface,
// which emits its Planck function); the fluxes at the interface are exchanged through LDS and each wave
// sweeps back through its half in the other direction, forming the heating rate on the way
// (heating_rate_single, heating_rate.h:55-72, with the reference's order of operations).  Half the
// per-lane state of the one-wave version -> two waves per SIMD with half as long dependency chains.
// REUSE: the Planck matrix of an earlier gas is read instead of evaluated (find_g_points.cpp:970-984 keeps the first
// gas's matrix for all later gases); its rows are fetched with the other inputs and planck_hl is not written.
// BLK: the background leaves as the sweep reads it, line-blocked (sweep_layout.hpp) - DOUBLE rows into bg_blk [n/16][NLAY][16]
// instead of bg_od, FLOAT pairs into bg_blk [n/16][NLAY/2][16] instead of bg_pair - and a Planck matrix evaluated here goes
// to planck_blk [n/16][NLAY+1][16] as well as to the row-major planck_hl (the sums, the fit and the views read that one).  A
// wave's 64 consecutive ranks are four whole lines of every row.  A DOUBLE background is tested on the way for values that
// are no floats (the predicate of k_pack_bg32): a lane that met one stores 1 to *not_float.  n is a multiple of 16.
template <int NLAY, typename BgT, typename OdT, bool REUSE, bool BLK = false>
__global__ void __launch_bounds__(PREP_THREADS, 2)
k_gas_prep_lw_mirror(size_t n, int method, const int32_t* __restrict__ ireorder, const double* __restrict__ hk,
                     const double* __restrict__ conv, const double* __restrict__ wn, const double* __restrict__ dwn,
                     const BgT* __restrict__ bg_col /* [n][NLAY] sorted, or NULL */,
                     const OdT* __restrict__ od_col /* [n][NLAY] sorted */, const double* __restrict__ planck_reuse,
                     double* __restrict__ wn_sorted, double* __restrict__ dwn_sorted, double* __restrict__ planck_hl,
                     double* __restrict__ bg_od, double* __restrict__ w1, double* __restrict__ hr,
                     double* __restrict__ fds, double* __restrict__ fut,
                     double* __restrict__ wave_part /* [3*NLAY+2][nw]: sums over this wave's 64 points of every summable row */,
                     size_t nw,
                     float_x2_store* __restrict__ bg_pair /* FLOAT background only, or NULL: the rows as FLOAT pairs (layers 2p, 2p+1
                                                             of a point side by side) INSTEAD of the DOUBLE rows bg_od */,
                     void* __restrict__ bg_blk = nullptr, double* __restrict__ planck_blk = nullptr,
                     int* __restrict__ not_float = nullptr /* BLK only */) {
  static_assert(NLAY % 2 == 0 && PREP_THREADS == 256, "two wave pairs per block, equal halves");
  namespace sl = ecckd::sweep_layout;
  constexpr int H = NLAY / 2;
  constexpr bool BLK_PAIRS = BLK && sizeof(BgT) == 4;     // a FLOAT (or no) background on the blocked path always leaves as pairs
  constexpr bool STAGED = sizeof(OdT) == 4;   // the columns arrive in two runs of H layers, see below (always, on this path)
  __shared__ double s_x[4][64];
  // Row sums over the wave's 64 points, formed while the values are still in registers (they used to be re-read from
  // HBM by k_tile_sums: 1 312 B per point).  Sixteen rows at a time go through a wave-private transposed LDS tile: lane
  // (rr, qq) adds the 16 points qq*16.. of row rr in index order, the four quarters are combined by two xor-shuffles.
  constexpr int ROWW = 65;
  constexpr int NPUSH = 3 * H + 1;                 // w1 and Planck row per layer, heating rate per layer, boundary flux
  __shared__ double s_sum[4][8 * ROWW];
  // the first sweep's fluxes at the wave's H + 1 levels, [level][lane]: 56 registers that the kernel does not have (it spilled 120
  // bytes per lane with them); before the sweep the block holds the staged inputs
  __shared__ __attribute__((aligned(16))) double s_f1[4][(H + 1) * 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int half = wave & 1, pair = wave >> 1;
  const size_t i = (size_t)blockIdx.x * 128 + (size_t)pair * 64 + lane;
  const bool live = i < n;
  const size_t ii = live ? i : n - 1;
  const size_t j = (size_t)ireorder[ii];
  const double w = wn[j], dw = dwn[j];
  if (live && half == 0) { wn_sorted[i] = w; dwn_sorted[i] = dw; }
  const double freq = ecckd::wn_to_freq(w);
  const double pref = ecckd::planck_pref(dw, freq);
  // BLK: the byte offset of this lane's point in row 0 of the blocked matrices, one register each (a gas is blocked only
  // where sl::fits_32bit); row r is r * LINE_BYTES further on
  const unsigned at_bg = BLK ? (unsigned)sl::point_base(BLK_PAIRS ? H : NLAY, ii) : 0;
  const unsigned at_pl = BLK && !REUSE ? (unsigned)sl::point_base(NLAY + 1, ii) : 0;
  const auto blk_row = [](void* base, unsigned at, int r) { return (char*)base + ((size_t)at + (size_t)r * sl::LINE_BYTES); };
  const BgT* bgc = bg_col && !STAGED ? bg_col + ii * NLAY : nullptr;
  const OdT* odc = od_col + (STAGED ? 0 : ii * NLAY);
  const size_t wid = (size_t)blockIdx.x * 2 + pair;          // index of this pair's 64 points among the 64-point groups
  double* sum_tile = s_sum[wave];
  const int rr = lane & 7, qq = lane >> 3;
  int slot = 0;
  // rows of the table ecckd_gas_create_lw builds: A = w1 (0..NLAY), B = planck_hl(l+1) (NLAY..), H = hr (2 NLAY..), then the two boundary rows
  auto row_of_slot = [&](int sl) -> int {
    if (sl < 2 * H) { const int l = sl >> 1; const int L = half ? NLAY - 1 - l : l; return ((sl & 1) ? NLAY : 0) + L; }
    if (sl < 3 * H) { const int l = H - 1 - (sl - 2 * H); const int L = half ? NLAY - 1 - l : l; return 2 * NLAY + L; }
    return 3 * NLAY + (half ? 0 : 1);
  };
  auto push = [&](double v) {
    sum_tile[(slot & 7) * ROWW + lane] = live ? v : 0.0;
    if ((slot & 7) == 7 || slot == NPUSH - 1) {
      const int base = slot & ~7, count = slot - base + 1;
      __builtin_amdgcn_wave_barrier();
      double sum = 0.0;
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += sum_tile[rr * ROWW + qq * 8 + j];
      sum += __shfl_xor(sum, 8, 64);
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      if (wave_part && qq == 0 && rr < count && wid < nw) wave_part[(size_t)row_of_slot(base + rr) * nw + wid] = sum;
      __builtin_amdgcn_wave_barrier();
    }
    ++slot;
  };
  // polynomial coefficients and the other literals pinned in SGPRs (fastmath.hpp): without this a third of
  // the kernel's instructions were s_mov / v_mov pairs rebuilding 64-bit constants next to their uses
  const ecckd::ExpConsts ek = ecckd::exp_consts();
  const double neg_d = ecckd::sgpr_pin(-kD), inv_d = ecckd::sgpr_pin(1.0 / kD), thin = ecckd::sgpr_pin(1.0e-5);
  double pl_in[REUSE ? H + 1 : 1];
  if (REUSE) {
#pragma unroll
    for (int l = 0; l <= H; ++l) pl_in[REUSE ? l : 0] = planck_reuse[(size_t)(half ? NLAY - l : l) * n + ii];
  }
  // local level l is level l (even wave) or NLAY - l (odd wave)
  auto planck = [&](int level) {
    if (REUSE) return pl_in[REUSE ? (half ? NLAY - level : level) : 0];
    return ecckd::div_fast(pref, ecckd::exp_fast_s(freq * hk[level], ek) - 1.0);
  };
  // local layer l is layer l (even wave) or NLAY-1-l (odd wave); its near level is where the first sweep enters
  double ee[H], s2[H];
  double* const f1 = s_f1[wave] + lane;     // f1[level * 64]
  // All inputs of this wave's half column are fetched BEFORE the first store: on this hardware the counter a load
  // waits on also counts the stores issued before it, so a load inside the layer loop would wait for the previous
  // layer's four row stores to complete and the kernel would run at one store latency per layer.
  OdT od_in[H];
  BgT bg_in[H];
  __builtin_amdgcn_s_setprio(3);
  if (STAGED) {
    // Both inputs come as [2][npad][H] (k_scatter_column_halves), this wave's 64 x H block of each is one contiguous
    // piece.  It is copied into LDS (the row-sum tile, idle until the first push) with full-width loads and each lane takes
    // its column from there: read straight from memory a column costs 64 cache lines per load instruction.
    float* st = reinterpret_cast<float*>(s_f1[wave]);
    constexpr int NV = 16 * H;                                // float4s in the block
    static_assert(NV * 16 * 2 <= (H + 1) * 64 * 8, "a DOUBLE block fits too");
    const size_t widc = wid < nw ? wid : nw - 1;              // a pair past the end repeats the last point, as ii does
    const int lc = live ? lane : (int)((n - 1) - widc * 64);
    const size_t blk = ((size_t)half * (nw * 64) + widc * 64) * H;
    auto fill = [&](const float* col) {
#pragma unroll
      for (int t = 0; t < (NV + 63) / 64; ++t) {
        const int at = t * 64 + lane;
        if (at < NV) reinterpret_cast<float4*>(st)[at] = reinterpret_cast<const float4*>(col + blk)[at];
      }
      __builtin_amdgcn_wave_barrier();
    };
    if (sizeof(BgT) == 4) {
      // FLOAT (or no) background: both blocks side by side in the buffer, their loads out together - one memory round trip.
      // No background: the loads still happen, from the target's block (a branch round them would put a full wait behind each).
      static_assert(2 * NV * 16 <= (H + 1) * 64 * 8, "both FLOAT blocks fit side by side");
      const float4* so = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(od_col) + blk);
      const float4* sb = bg_col ? reinterpret_cast<const float4*>(reinterpret_cast<const float*>(bg_col) + blk) : so;
#pragma unroll
      for (int t = 0; t < (NV + 63) / 64; ++t) {
        const int at = t * 64 + lane;
        if (at < NV) {
          const float4 vo = so[at], vb = sb[at];
          reinterpret_cast<float4*>(st)[at] = vo;
          reinterpret_cast<float4*>(st)[NV + at] = vb;
        }
      }
      __builtin_amdgcn_wave_barrier();
      const bool has_bg = bg_col != nullptr;
#pragma unroll
      for (int l = 0; l < H; ++l) {
        const int kk = lc * H + (half ? H - 1 - l : l);
        od_in[l] = (OdT)st[kk];
        bg_in[l] = has_bg ? (BgT)st[64 * H + kk] : (BgT)0;
      }
      __builtin_amdgcn_wave_barrier();
    } else {
    fill(reinterpret_cast<const float*>(od_col));
#pragma unroll
    for (int l = 0; l < H; ++l) od_in[l] = (OdT)st[lc * H + (half ? H - 1 - l : l)];
    __builtin_amdgcn_wave_barrier();
    if (bg_col) {
      // DOUBLE (merged) background: the same with 16-byte pairs of doubles
      const double* colb = reinterpret_cast<const double*>(bg_col) + blk;
      double* std_ = s_f1[wave];
#pragma unroll
      for (int t = 0; t < (2 * NV + 63) / 64; ++t) {
        const int at = t * 64 + lane;
        if (at < 2 * NV) reinterpret_cast<double2*>(std_)[at] = reinterpret_cast<const double2*>(colb)[at];
      }
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int l = 0; l < H; ++l) bg_in[l] = (BgT)std_[lc * H + (half ? H - 1 - l : l)];
      __builtin_amdgcn_wave_barrier();
    } else {
#pragma unroll
      for (int l = 0; l < H; ++l) bg_in[l] = (BgT)0;
    }
    }
  } else {
#pragma unroll
    for (int l = 0; l < H; ++l) od_in[l] = odc[half ? NLAY - 1 - l : l];
    if (bg_col) {   // uniform: one block of loads
#pragma unroll
      for (int l = 0; l < H; ++l) bg_in[l] = bgc[half ? NLAY - 1 - l : l];
    } else {
#pragma unroll
      for (int l = 0; l < H; ++l) bg_in[l] = (BgT)0;
    }
  }
  __builtin_amdgcn_s_setprio(0);
  if (BLK && sizeof(BgT) == 8) {
    // what k_pack_bg32 asks of every value: it is a float, and not a subnormal one (a lane past the end holds the last point's)
    bool bad = false;
#pragma unroll
    for (int l = 0; l < H; ++l) {
      const double x = (double)bg_in[l];
      const float f = (float)x;
      bad |= !((double)f == x);
      bad |= f != 0.f && fabsf(f) < 1.17549435e-38f;
    }
    if (bad) *not_float = 1;      // every writer writes the same value
  }
  int lev_near = half ? NLAY : 0;
  double b_near = planck(lev_near);
  if (!REUSE && live) {
    planck_hl[(size_t)lev_near * n + i] = b_near;
    if (BLK) *(double*)blk_row(planck_blk, at_pl, lev_near) = b_near;
  }
  double flux = half ? b_near : 0.0;           // surface: emissivity 1 (radiative_transfer_lw.cpp:52-53)
  f1[0] = flux;
#pragma unroll
  for (int l = 0; l < H; ++l) {
    const int L = half ? NLAY - 1 - l : l;
    const int lev_far = half ? L : L + 1;
    const double bg = (double)bg_in[l];
    const double od = (double)od_in[l];
    const double tau = bg + od;
    const double eps = 1.0 - ecckd::exp_fast_s(neg_d * tau, ek);
    const double fac = (eps > thin) ? 1.0 - ecckd::div_fast(eps * inv_d, tau) : 0.5 * eps;
    const double b_far = planck(lev_far);
    const double emf = eps - fac;
    const double next = flux * (1.0 - eps) + b_near * emf + b_far * fac;
    ee[l] = eps;
    s2[l] = b_far * emf + b_near * fac;
    f1[(l + 1) * 64] = next;
    double m;
    switch (method) {
      case ECCKD_AVG_TRANSMISSION: m = 1.0 - ecckd::exp_fast_s(-od * kD, ek); break;
      case ECCKD_AVG_TRANSMISSION_2: m = 1.0 - ecckd::exp_fast_s(-od * kD * 2.0, ek); break;
      case ECCKD_AVG_SQUARE_ROOT: m = sqrt(od); break;
      default: m = od;
    }
    if (live) {
      const size_t o = (size_t)L * n + i;
      // written once, read by later kernels: streaming stores
      if (BLK_PAIRS || (sizeof(BgT) == 4 && bg_pair)) {
        // the background as the sweep reads it (k_rt_lw_bb_mirror<.., true>): a pair is complete at every second layer of the
        // half column - the even wave has met its layers in the pair's order, the odd wave the other way round; the middle
        // pair of an odd half belongs to both waves, each stores its own float
        float_x2_store* const pr = BLK_PAIRS ? (float_x2_store*)blk_row(bg_blk, at_bg, L / 2) : &bg_pair[(size_t)(L / 2) * n + i];
        if (l & 1) {
          float_x2_store v;
          v.x = half ? (float)bg_in[l] : (float)bg_in[l - 1];
          v.y = half ? (float)bg_in[l - 1] : (float)bg_in[l];
          __builtin_nontemporal_store(v, pr);
        } else if (l == H - 1) {
          ((float*)pr)[L & 1] = (float)bg_in[l];
        }
      } else {
        __builtin_nontemporal_store(bg, BLK ? (double*)blk_row(bg_blk, at_bg, L) : &bg_od[o]);
      }
      if (!REUSE) {
        __builtin_nontemporal_store(b_far, &planck_hl[(size_t)lev_far * n + i]);   // level NLAY/2 is written by both waves with the same bits
        if (BLK) __builtin_nontemporal_store(b_far, (double*)blk_row(planck_blk, at_pl, lev_far));
      }
      __builtin_nontemporal_store(m * (half ? b_near : b_far), &w1[o]);          // weight = Planck function at the base of the layer
    }
    push(m * (half ? b_near : b_far));
    push(half ? b_near : b_far);                    // planck_hl(L + 1), the denominator row of the fit
    flux = next;
    b_near = b_far;
  }
  s_x[wave][lane] = flux;
  __syncthreads();
  flux = s_x[wave ^ 1][lane];
#pragma unroll
  for (int l = H - 1; l >= 0; --l) {
    const int L = half ? NLAY - 1 - l : l;
    const double next = flux * (1.0 - ee[l]) + s2[l];
    // conv * (dn(L+1) - dn(L) - up(L+1) + up(L)), left to right
    const double f1a = f1[l * 64], f1b = f1[(l + 1) * 64];
    const double net = half ? (next - flux) - f1a + f1b        // second sweep is downwelling: flux = dn(L), next = dn(L+1)
                            : (f1b - f1a) - flux + next;       // second sweep is upwelling:   flux = up(L+1), next = up(L)
    const double hrv = conv[L] * net;
    if (live) __builtin_nontemporal_store(hrv, &hr[(size_t)L * n + i]);
    push(hrv);
    flux = next;
  }
  if (live) {
    if (half) fds[i] = flux; else fut[i] = flux;
  }
  push(flux);
}

// tile sums from the per-wave sums K4 leaves: TS[r][t] = ((W[4t] + W[4t+1]) + W[4t+2]) + W[4t+3]
__global__ void __launch_bounds__(256)
k_combine_wave_sums(int nrows, size_t nw, size_t ntiles, const double* __restrict__ wp, double* __restrict__ ts) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int r = blockIdx.y;
  if (t >= ntiles || r >= nrows) return;
  const double* w = wp + (size_t)r * nw + 4 * t;
  const size_t left = nw - 4 * t;
  double s = w[0];
  if (left > 1) s += w[1];
  if (left > 2) s += w[2];
  if (left > 3) s += w[3];
  ts[(size_t)r * ntiles + t] = s;
}

// tile sums of every row: TS[r][t] = sum_{i in tile t} rows[r][i]
__global__ void __launch_bounds__(TILE)
k_tile_sums(int nrows, size_t n, size_t ntiles, const double* const* __restrict__ rows,
            double* __restrict__ ts) {
  // four rows per round: four independent loads in flight, one barrier pair for the four block sums; each sum is the
  // same tree as block_sum_256 (wave shuffle tree, then ((w0 + w1) + w2) + w3)
  __shared__ double s4[4][4];
  const size_t t = blockIdx.x;
  const size_t i = t * TILE + threadIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r0 = 0; r0 < nrows; r0 += 4) {
    double v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = (r0 + q < nrows && i < n) ? rows[r0 + q][i] : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = wave_sum(v[q]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) s4[q][wave] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < 4 && r0 + (int)threadIdx.x < nrows) {
      const int q = threadIdx.x;
      ts[(size_t)(r0 + q) * ntiles + t] = ((s4[q][0] + s4[q][1]) + s4[q][2]) + s4[q][3];
    }
  }
}

// ---------------------------------------------------------------------------
// K5a: interval sums.  grid (nrows, nint); block 256.
// sums[k][r] = sum_{i=i1_k..i2_k} rows[r][i] = ragged head + whole tiles + ragged tail
struct Interval {
  long long i1, i2;      // inclusive global sorted indices
  int chunk0;            // first RT chunk of this interval (a batch has fewer than 2^31 chunks)
  int head;              // i1 mod 16 where the chunks are counted from the 128-byte line below i1 (chunk_layout.hpp), else 0
  long long chunk_pts;   // points per RT chunk of THIS interval: a function of the interval alone (chunk_layout::of_interval), so
                         // that the order in which its points are summed - and with it every bit of its error - does not depend
                         // on what else is evaluated in the same batch
  long long npoints;     // band length (for the logarithmic fit)
  double albedo;         // shortwave: surface albedo of the interval's band
};

// Batches of up to KARG_MAX intervals (nearly all of a search: next_bound_below / _above evaluate ONE interval per call,
// equipartition.cpp:638-805; calc_error_all a partition of a few dozen) hand their interval table to the first kernel of the
// train in its ARGUMENTS instead of a host-to-device copy in front of it (a blit kernel of ~18 us): one stream operation and
// one dependency gap less per batch.  The first kernel leaves the table in device memory for
// the kernels behind it.
constexpr int KARG_MAX = 64;     // 3 KB of the 4 KB argument segment
struct IntervalArgs { Interval iv[KARG_MAX]; };

// The argument table is read where it lies, in the kernel-argument segment, with scalar loads at a block-uniform offset:
// IntervalArgs MUST be the kernel's FIRST parameter (offset 0 of the segment).  Indexing the by-value struct itself makes the
// compiler copy it to scratch (392 bytes per lane: every wave launch then waits for a scratch slot and the kernel's time
// grows by ~2.3 us per interval of the batch).
__device__ __forceinline__ Interval interval_of(int use_ka, const Interval* __restrict__ iv, int k) {
  if (!use_ka) return iv[k];
  typedef const __attribute__((address_space(4))) long long* karg_ptr;
  karg_ptr q = (karg_ptr)__builtin_amdgcn_kernarg_segment_ptr() + (size_t)k * (sizeof(Interval) / sizeof(long long));
  static_assert(sizeof(Interval) == 6 * sizeof(long long) && offsetof(Interval, chunk0) == 16 && offsetof(Interval, head) == 20,
                "Interval is six 8-byte slots; chunk0 and head share the third");
  Interval me;
  me.i1 = q[0]; me.i2 = q[1]; me.chunk0 = (int)q[2]; me.head = (int)(q[2] >> 32); me.chunk_pts = q[3]; me.npoints = q[4];
  me.albedo = __longlong_as_double(q[5]);
  return me;
}

// this thread's share of sum_{i=i1..i2} row[i]: ragged head points, whole 256-point tiles up to the next 65 536-point
// super tile, whole super tiles, the tiles behind them, ragged tail points - at most one value of each kind per thread
// (the sums of tiles and super tiles were formed once per gas), so the sums of an interval cost a handful of loads
// however long it is.  trow / srow: the row's tile and super-tile sums.
constexpr int SUPER = 256;                     // tiles per super tile
__device__ __forceinline__ double interval_row_acc(const double* __restrict__ row, const double* __restrict__ trow,
                                                   const double* __restrict__ srow, long long i1, long long i2, int tid) {
  const long long t1 = (i1 + TILE - 1) / TILE;   // first whole tile
  const long long t2 = (i2 + 1) / TILE;          // one past the last whole tile
  double acc = 0.0;
  if (t1 >= t2) {
    // no whole tile inside: at most 2*TILE-2 raw points
    for (long long i = i1 + tid; i <= i2; i += 256) acc += row[i];
    return acc;
  }
  const long long head_end = t1 * TILE;  // exclusive
  if (i1 + tid < head_end) acc += row[i1 + tid];
  const long long s1 = (t1 + SUPER - 1) / SUPER;  // first whole super tile
  const long long s2 = t2 / SUPER;                // one past the last whole super tile
  if (s1 >= s2) {
    // no whole super tile inside: at most 2*SUPER-2 tiles
    for (long long t = t1 + tid; t < t2; t += 256) acc += trow[t];
  } else {
    if (t1 + tid < s1 * SUPER) acc += trow[t1 + tid];
    for (long long q = s1 + tid; q < s2; q += 256) acc += srow[q];
    if (s2 * SUPER + tid < t2) acc += trow[s2 * SUPER + tid];
  }
  const long long tail = t2 * TILE + tid;
  if (tail <= i2) acc += row[tail];
  return acc;
}

// super-tile sums of every row: SS[r][q] = sum of the row's tile sums q*SUPER .. q*SUPER+SUPER-1, grid (nsuper, nrows)
__global__ void __launch_bounds__(256)
k_super_sums(size_t ntiles, size_t nsuper, const double* __restrict__ ts, double* __restrict__ ss) {
  __shared__ double s4[4];
  const size_t q = blockIdx.x, r = blockIdx.y;
  const size_t t = q * SUPER + threadIdx.x;
  const double v = t < ntiles ? ts[r * ntiles + t] : 0.0;
  const double sum = block_sum_256(v, s4);
  if (threadIdx.x == 0) ss[r * nsuper + q] = sum;
}

__global__ void __launch_bounds__(256)
k_interval_sums(IntervalArgs ka, int nrows, size_t ntiles, size_t nsuper, const Interval* __restrict__ iv, int use_ka,
                Interval* __restrict__ iv_out, const double* const* __restrict__ rows, const double* __restrict__ ts,
                const double* __restrict__ ss, double* __restrict__ sums) {
  __shared__ double s4[4];
  const int r = blockIdx.x, k = blockIdx.y;
  const int tid = threadIdx.x;
  (void)ka;
  const Interval me = interval_of(use_ka, iv, k);
  if (use_ka && r == 0 && tid == 0) iv_out[k] = me;
  const double acc = interval_row_acc(rows[r], ts + (size_t)r * ntiles, ss + (size_t)r * nsuper, me.i1, me.i2, tid);
  const double s = block_sum_256(acc, s4);
  if (tid == 0) sums[(size_t)k * nrows + r] = s;
}

// fit_optical_depth_lw (find_g_points.cpp:54-106) for one layer from the interval's sums: a = sum of the weighted metric,
// b = sum of the weights, nnz = number of points with a positive metric (logarithmic method), ntot = points of the interval
__device__ __forceinline__ double fit_lw_layer(int method, double a, double b, double nnz, double ntot) {
#pragma clang fp contract(off)
  switch (method) {
    case ECCKD_AVG_LINEAR: return a / b;
    case ECCKD_AVG_TRANSMISSION: return fabs(-log(1.0 - fmin(0.9999999999999999, a / b)) / kD);             // :64-68
    case ECCKD_AVG_TRANSMISSION_2: return fabs(-log(1.0 - fmin(0.9999999999999999, a / b)) / (kD * 2.0));
    case ECCKD_AVG_SQUARE_ROOT: { const double v = a / b; return v * v; }
    case ECCKD_AVG_LOGARITHMIC:                                                                              // :79-99
      if (nnz == ntot) return exp(a / b);
      if (nnz == 0.0) return 0.0;
      return exp(a / b) * (nnz / ntot);
    default: return nan("");
  }
}

// The rows of a longwave gas by number, from their base pointers in the kernel arguments (the device table of row pointers
// costs a dependent load in front of every row's own loads).
struct LwRowBases {
  const double *w1, *w2, *cnt, *planck_hl, *hr, *fds, *fut;
  size_t n;
  int is_log;
  __device__ __forceinline__ const double* row(const RowMap& R, int nlay, int r) const {
    if (r < R.B) return w1 + (size_t)(r - R.A) * n;
    if (r < R.B + nlay) return is_log ? w2 + (size_t)(r - R.B) * n : planck_hl + (size_t)(r - R.B + 1) * n;
    if (is_log && r < R.H) return cnt + (size_t)(r - R.N) * n;
    if (r < R.FDS) return hr + (size_t)(r - R.H) * n;
    return r == R.FDS ? fds : fut;
  }
};

// K5a + K5b in one launch for the longwave: the fit of layer l needs only the sums of its own rows (A+l, B+l and, for the
// logarithmic method, N+l), so the block that owns layer l adds up those rows and finishes the fit itself; the remaining
// rows (heating rate, boundary fluxes) get one block each as before.  grid (nlay + rows from R.H on, nint), block 256.
__global__ void __launch_bounds__(256)
k_interval_sums_fit_lw(IntervalArgs ka, int nlay, int method, RowMap R, size_t ntiles, size_t nsuper, const Interval* __restrict__ iv,
                       int use_ka, Interval* __restrict__ iv_out, LwRowBases rows,
                       const double* __restrict__ ts, const double* __restrict__ ss, double* __restrict__ sums,
                       double* __restrict__ od_fit) {
  __shared__ double s4[4];
  const int bx = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  (void)ka;
  const Interval me = interval_of(use_ka, iv, k);
  if (use_ka && bx == 0 && tid == 0) iv_out[k] = me;
  const long long i1 = me.i1, i2 = me.i2;
  double* out = sums + (size_t)k * R.total;
  if (bx >= nlay) {
    const int r = R.H + (bx - nlay);
    const double s = block_sum_256(interval_row_acc(rows.row(R, nlay, r), ts + (size_t)r * ntiles, ss + (size_t)r * nsuper, i1, i2, tid), s4);
    if (tid == 0) out[r] = s;
    return;
  }
  const int l = bx;
  const bool is_log = method == ECCKD_AVG_LOGARITHMIC;
  // the loads of the two (three) rows go out together: one memory round trip and one pair of barriers instead of two (three)
  __shared__ double s43[3][4];
  double a = interval_row_acc(rows.row(R, nlay, R.A + l), ts + (size_t)(R.A + l) * ntiles, ss + (size_t)(R.A + l) * nsuper, i1, i2, tid);
  double b = interval_row_acc(rows.row(R, nlay, R.B + l), ts + (size_t)(R.B + l) * ntiles, ss + (size_t)(R.B + l) * nsuper, i1, i2, tid);
  double nnz = 0.0;
  if (is_log) nnz = interval_row_acc(rows.row(R, nlay, R.N + l), ts + (size_t)(R.N + l) * ntiles, ss + (size_t)(R.N + l) * nsuper, i1, i2, tid);
  block_sum_256_x3(a, b, nnz, s43);
  if (tid == 0) {
    out[R.A + l] = a;
    out[R.B + l] = b;
    if (is_log) out[R.N + l] = nnz;
    const double fit = fit_lw_layer(method, a, b, nnz, (double)(i2 - i1 + 1));
    od_fit[(size_t)k * nlay + l] = fit;
    // the same values bottom-up behind the table: the sweep's odd waves read their layers at ascending addresses too
    od_fit[((size_t)gridDim.y + k) * nlay + (nlay - 1 - l)] = fit;
  }
}

// K5b: fitted grey optical depth per (interval, layer).  grid nint, block 128.
__global__ void __launch_bounds__(128)
k_fit_lw(int nlay, int method, RowMap R, const Interval* __restrict__ iv,
         const double* __restrict__ sums, double* __restrict__ od_fit) {
#pragma clang fp contract(off)
  const int k = blockIdx.x;
  const double* s = sums + (size_t)k * R.total;
  for (int l = threadIdx.x; l < nlay; l += blockDim.x) {
    const double a = s[R.A + l], b = s[R.B + l];
    const double nnz = method == ECCKD_AVG_LOGARITHMIC ? s[R.N + l] : 0.0;
    const double fit = fit_lw_layer(method, a, b, nnz, (double)(iv[k].i2 - iv[k].i1 + 1));
    od_fit[(size_t)k * nlay + l] = fit;
  }
}

// K5c: grey-optical-depth LW radiative transfer with broadband sums,
// radiative_transfer_lw_bb (radiative_transfer_lw.cpp:87-142) for every interval.
// One block = one chunk of `chunk_pts` consecutive points of ONE interval,
// processed as sub-tiles of 256 points (one point per thread).  Per half-level
// the 64 lanes' fluxes are reduced in the wave and lane 0 accumulates into
// s_acc[wave][...]; the four waves are combined in order at the end and the
// block writes its 2*(nlay+1) partial sums to `partial[chunk]`.
// The up sweep re-evaluates emissivity and factor exactly as the reference does
// (:128-137) from re-loaded rows (second touch is served by L2/Infinity Cache).
__global__ void __launch_bounds__(RT_THREADS)
k_rt_lw_bb(int nlay, size_t n, int nint, const Interval* __restrict__ iv,
           const double* __restrict__ planck_hl, const double* __restrict__ bg_od,
           const double* __restrict__ od_fit, double* __restrict__ partial) {
  extern __shared__ double s_mem[];  // [4][2*nhl] accumulators | [nlay] grey od
  const int nhl = nlay + 1;
  double* s_acc = s_mem;
  double* s_grey = s_mem + 4 * 2 * nhl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  // locate this block's interval: chunk0 is ascending
  const long long chunk = blockIdx.x;
  int lo = 0, hi = nint - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (iv[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
  }
  const int k = lo;
  const long long chunk_pts = iv[k].chunk_pts;
  const long long c = chunk - iv[k].chunk0;
  const long long p0 = iv[k].i1 + c * chunk_pts;
  long long p1 = p0 + chunk_pts - 1;
  if (p1 > iv[k].i2) p1 = iv[k].i2;

  for (int t = tid; t < 4 * 2 * nhl; t += RT_THREADS) s_acc[t] = 0.0;
  for (int l = tid; l < nlay; l += RT_THREADS) s_grey[l] = od_fit[(size_t)k * nlay + l];
  __syncthreads();
  double* acc_dn = s_acc + wave * 2 * nhl;
  double* acc_up = acc_dn + nhl;

  constexpr double THRESHOLD_EMISSIVITY = 1.0e-5;
  for (long long base = p0; base <= p1; base += RT_THREADS) {
    const long long i = base + tid;
    const bool live = i <= p1;
    const size_t ii = live ? (size_t)i : (size_t)p1;
    // ---- down sweep (:109-124) ----
    double flux = 0.0;
    double b_prev = planck_hl[ii];
    for (int l = 0; l < nlay; ++l) {
      const double od = bg_od[(size_t)l * n + ii] + s_grey[l];
      const double b_next = planck_hl[(size_t)(l + 1) * n + ii];
      const double eps = 1.0 - exp(-kD * od);
      const double fac = fmax(1.0 - (1.0 / kD) * fmax(eps, THRESHOLD_EMISSIVITY) /
                                         fmax(od, THRESHOLD_EMISSIVITY / kD),
                              0.5 * THRESHOLD_EMISSIVITY);
      flux = flux * (1.0 - eps) + b_prev * (eps - fac) + b_next * fac;
      const double s = wave_sum(live ? flux : 0.0);
      if (lane == 0) acc_dn[l + 1] += s;
      b_prev = b_next;
    }
    // ---- surface (:126-128), emissivity 1, surf_planck = planck_hl(nlay) ----
    flux = b_prev * 1.0 + (1.0 - 1.0) * flux;
    {
      const double s = wave_sum(live ? flux : 0.0);
      if (lane == 0) acc_up[nlay] += s;
    }
    // ---- up sweep (:130-141) ----
    for (int l = nlay - 1; l >= 0; --l) {
      const double od = bg_od[(size_t)l * n + ii] + s_grey[l];
      const double b_l = planck_hl[(size_t)l * n + ii];
      const double eps = 1.0 - exp(-kD * od);
      const double fac = fmax(1.0 - (1.0 / kD) * fmax(eps, THRESHOLD_EMISSIVITY) /
                                         fmax(od, THRESHOLD_EMISSIVITY / kD),
                              0.5 * THRESHOLD_EMISSIVITY);
      flux = flux * (1.0 - eps) + b_prev * (eps - fac) + b_l * fac;
      const double s = wave_sum(live ? flux : 0.0);
      if (lane == 0) acc_up[l] += s;
      b_prev = b_l;
    }
  }
  __syncthreads();
  for (int t = tid; t < 2 * nhl; t += RT_THREADS) {
    partial[(size_t)chunk * 2 * nhl + t] =
        ((s_acc[t] + s_acc[2 * nhl + t]) + s_acc[4 * nhl + t]) + s_acc[6 * nhl + t];
  }
}


// Emissivity and factor of TWO layers at once with the two dependency chains interleaved in
// the source: at 2 waves/SIMD the fp64 FMA latency is not covered by other waves, so the
// instruction-level parallelism has to be in the stream itself (radiative_transfer_lw.cpp:114-119).
__device__ __forceinline__ void eps_fac_pair(double od0, double od1, double& eps0, double& fac0,
                                             double& eps1, double& fac1) {
  constexpr double TE = 1.0e-5;
  const double y0 = -kD * od0, y1 = -kD * od1;
  const double k0 = __builtin_rint(y0 * 1.4426950408889634074), k1 = __builtin_rint(y1 * 1.4426950408889634074);
  double r0 = __builtin_fma(k0, -6.93147180369123816490e-01, y0), r1 = __builtin_fma(k1, -6.93147180369123816490e-01, y1);
  r0 = __builtin_fma(k0, -1.90821492927058770002e-10, r0); r1 = __builtin_fma(k1, -1.90821492927058770002e-10, r1);
  // reciprocal seeds issued early: independent of the exp chains
  const double d0 = fmax(od0, TE / kD), d1 = fmax(od1, TE / kD);
  double q0 = __builtin_amdgcn_rcp(d0), q1 = __builtin_amdgcn_rcp(d1);
  double p0 = 2.08767569878680989792e-09, p1 = 2.08767569878680989792e-09;
#define ECCKD_STEP(c) p0 = __builtin_fma(p0, r0, c); p1 = __builtin_fma(p1, r1, c);
  ECCKD_STEP(2.50521083854417187751e-08)
  double e0 = __builtin_fma(-d0, q0, 1.0), e1 = __builtin_fma(-d1, q1, 1.0);
  ECCKD_STEP(2.75573192239858906526e-07)
  q0 = __builtin_fma(q0, e0, q0); q1 = __builtin_fma(q1, e1, q1);
  ECCKD_STEP(2.75573192239858906526e-06)
  e0 = __builtin_fma(-d0, q0, 1.0); e1 = __builtin_fma(-d1, q1, 1.0);
  ECCKD_STEP(2.48015873015873015873e-05)
  q0 = __builtin_fma(q0, e0, q0); q1 = __builtin_fma(q1, e1, q1);
  ECCKD_STEP(1.98412698412698412698e-04)
  ECCKD_STEP(1.38888888888888888889e-03)
  ECCKD_STEP(8.33333333333333333333e-03)
  ECCKD_STEP(4.16666666666666666667e-02)
  ECCKD_STEP(1.66666666666666666667e-01)
  ECCKD_STEP(0.5)
  ECCKD_STEP(1.0)
  ECCKD_STEP(1.0)
#undef ECCKD_STEP
  const int i0 = (int)fmax(k0, -1100.0), i1 = (int)fmax(k1, -1100.0);
  eps0 = 1.0 - __builtin_amdgcn_ldexp(p0, i0);
  eps1 = 1.0 - __builtin_amdgcn_ldexp(p1, i1);
  // max(eps, TE) / max(od, TE/D) with one residual correction
  const double n0 = fmax(eps0, TE), n1 = fmax(eps1, TE);
  double t0 = n0 * q0, t1 = n1 * q1;
  const double s0 = __builtin_fma(-d0, t0, n0), s1 = __builtin_fma(-d1, t1, n1);
  t0 = __builtin_fma(s0, q0, t0); t1 = __builtin_fma(s1, q1, t1);
  fac0 = fmax(1.0 - (1.0 / kD) * t0, 0.5 * TE);
  fac1 = fmax(1.0 - (1.0 / kD) * t1, 0.5 * TE);
}

// Emissivity and factor of one layer (the tail of an odd-length half column).
__device__ __forceinline__ void eps_fac_one(double od, double& eps, double& fac) {
  constexpr double TE = 1.0e-5;
  eps = 1.0 - ecckd::exp_nonpos(-kD * od);
  fac = fmax(1.0 - (1.0 / kD) * ecckd::div_fast(fmax(eps, TE), fmax(od, TE / kD)), 0.5 * TE);
}

// The background optical depths of a longwave gas as FLOAT pairs: out[p][i] = (bg_od[2p][i], bg_od[2p+1][i]).  A value that
// is not a float (or is a subnormal float: the conversion back may flush it) raises `inexact`, and the gas keeps to its
// DOUBLE rows.
__global__ void __launch_bounds__(256)
k_pack_bg32(int npair, size_t n, const double* __restrict__ bg_od, float_x2_store* __restrict__ out, int* __restrict__ inexact) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  bool bad = false;
#pragma unroll 3
  for (int p = 0; p < npair; ++p) {
    const double x = __builtin_nontemporal_load(&bg_od[(size_t)(2 * p) * n + i]);
    const double y = __builtin_nontemporal_load(&bg_od[(size_t)(2 * p + 1) * n + i]);
    const float fx = (float)x, fy = (float)y;
    bad |= !((double)fx == x) || !((double)fy == y);
    bad |= (fx != 0.f && fabsf(fx) < 1.17549435e-38f) || (fy != 0.f && fabsf(fy) < 1.17549435e-38f);
    float_x2_store v;
    v.x = fx; v.y = fy;
    __builtin_nontemporal_store(v, &out[(size_t)p * n + i]);
  }
  if (bad) atomicOr(inexact, 1);
}

// ... and back: the DOUBLE rows of a gas that holds only the pairs, when something asks for them (ecckd_gas_view, the
// run-time-nlay sweep).
__global__ void __launch_bounds__(256)
k_unpack_bg32(int npair, size_t n, const float_x2_store* __restrict__ pairs, double* __restrict__ bg_od) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (int p = 0; p < npair; ++p) {
    const float_x2_store v = pairs[(size_t)p * n + i];
    bg_od[(size_t)(2 * p) * n + i] = (double)v.x;
    bg_od[(size_t)(2 * p + 1) * n + i] = (double)v.y;
  }
}

// A row-major matrix [rows][n] of 8-byte elements (DOUBLE values or FLOAT pairs) into its line-blocked form
// [n / 16][rows][16] (sweep_layout.hpp), or back: one thread per element in the order of the blocked matrix, so every 16
// lanes read one whole 128-byte line and store one whole line, each line once.
template <bool TO_BLOCKED>
__global__ void __launch_bounds__(256)
k_reblock(unsigned rows, size_t n, const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst) {
  namespace sl = ecckd::sweep_layout;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)rows * n) return;
  const size_t per = (size_t)rows * sl::LINE_PTS;
  const size_t blk = e / per;
  const unsigned rem = (unsigned)(e - blk * per);
  const unsigned r = rem / (unsigned)sl::LINE_PTS;
  const size_t i = blk * sl::LINE_PTS + rem % (unsigned)sl::LINE_PTS;
  const size_t at_blocked = (size_t)(sl::offset(rows, r, i) / sl::ELEM_BYTES), at_rows = (size_t)r * n + i;
  if (TO_BLOCKED) __builtin_nontemporal_store(__builtin_nontemporal_load(&src[at_rows]), &dst[at_blocked]);
  else __builtin_nontemporal_store(__builtin_nontemporal_load(&src[at_blocked]), &dst[at_rows]);
}

// The DOUBLE rows of a gas that holds only the line-blocked FLOAT pairs (k_unpack_bg32 for the blocked matrix).
__global__ void __launch_bounds__(256)
k_unpack_bg32_blocked(int npair, size_t n, const float_x2_store* __restrict__ pairs, double* __restrict__ bg_od) {
  namespace sl = ecckd::sweep_layout;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float_x2_store* __restrict__ at = pairs + sl::point_base(npair, i) / sl::ELEM_BYTES;
  for (int p = 0; p < npair; ++p) {
    const float_x2_store v = at[(size_t)p * sl::LINE_PTS];
    bg_od[(size_t)(2 * p) * n + i] = (double)v.x;
    bg_od[(size_t)(2 * p + 1) * n + i] = (double)v.y;
  }
}

// ... and its inverse: the line-blocked FLOAT pairs from the line-blocked DOUBLE rows [n / 16][2 npair][16] that the
// preparation wrote, once its test has found every value to be a float (ecckd_gas_create_lw): one pass.
__global__ void __launch_bounds__(256)
k_pack_bg32_blocked(int npair, size_t n, const double* __restrict__ bg_blk, float_x2_store* __restrict__ pairs) {
  namespace sl = ecckd::sweep_layout;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* __restrict__ from = bg_blk + sl::point_base(2 * npair, i) / sl::ELEM_BYTES;
  float_x2_store* __restrict__ to = pairs + sl::point_base(npair, i) / sl::ELEM_BYTES;
  for (int p = 0; p < npair; ++p) {
    float_x2_store v;
    v.x = (float)from[(size_t)(2 * p) * sl::LINE_PTS];
    v.y = (float)from[(size_t)(2 * p + 1) * sl::LINE_PTS];
    to[(size_t)p * sl::LINE_PTS] = v;
  }
}

// K5c mirror path.  The two-stream equations are symmetric under turning the column upside down:
// the up sweep through layer l, up_l = up_{l+1} t + B_{l+1}(eps-fac) + B_l fac, is the down sweep
// dn_{l+1} = dn_l t + B_l(eps-fac) + B_{l+1} fac with the two Planck values exchanged
// (radiative_transfer_lw.cpp:121-123,:138-139).  So a PAIR of waves shares 64 spectral points: the even
// wave owns the upper NLAY/2 layers and loads them top-down, the odd wave owns the lower NLAY/2 layers
// and loads them bottom-up, and both run the SAME instruction stream:
//   first sweep  - even: downward from the top of the atmosphere (input 0),
//                  odd:  upward from the surface (input = surface Planck function, emissivity 1),
//                  keeping the layer transmittance and the source of the opposite direction;
//   exchange     - through LDS, one barrier per tile: each wave receives the true flux that enters its
//                  half from the other side;
//   second sweep - even: upward through its half, odd: downward through its half.
// Every flux is the exact sequential recurrence of the reference; nothing is recomputed.  Per-lane
// state is NLAY+1 doubles instead of 2*NLAY+1, which fits 3 waves per SIMD - the dependent
// v_fma_f64 chains need that (tools/fp64_latency.hip).  Level sums: as in the fast path, through a
// wave-private transposed LDS tile every 16 slots.
//
// BG32: the background optical depths come from the packed FLOAT rows (k_pack_bg32: row p holds the layers 2p and 2p+1 of
// a point side by side, 8 bytes per point like a DOUBLE row) instead of the DOUBLE rows - 656 instead of 872 bytes per point.
// The rows exist only when every value IS a float (a FLOAT background spectrum, as the CKDMIP files store it), so the
// converted value is the DOUBLE row's value bit for bit and so is everything computed from it.  The even wave takes the
// pairs top-down, the odd wave bottom-up with the two halves of a pair exchanged; with an odd number of layers per half the
// middle pair is shared: .x is the even wave's last layer, .y the odd wave's.
//
// BLK: planck_hl and bg_od / bg_pair are the line-blocked matrices (sweep_layout.hpp) of a gas that holds them
// (ecckd_gas::planck_blk, bg_blk); only the addresses of the loads differ - the same values reach the same lanes, and
// everything after the loads is the same code, so the partials have the same bits.
template <int NLAY, bool BG32, bool BLK>
__global__ void __launch_bounds__(RT_THREADS, 3)
k_rt_lw_bb_mirror(size_t n, int nint, long long nchunks, const Interval* __restrict__ iv,
                  const double* __restrict__ planck_hl, const double* __restrict__ bg_od,
                  const float_x2* __restrict__ bg_pair,
                  const double* __restrict__ od_fit, double* __restrict__ partial) {
  static_assert(NLAY % 2 == 0, "the column is split into two equal halves");
  constexpr int NHL = NLAY + 1;
  constexpr int H = NLAY / 2;
  constexpr int NSLOT = 2 * H + 1;               // slot 0: input of the first sweep, 1..H first sweep, H+1..2H second
  constexpr int NCH = (NSLOT + 15) / 16;
  constexpr int ROW = 65;
  constexpr int PTS = RT_THREADS / 2;            // points per block iteration: two wave pairs
  __shared__ double s_tile[4][16 * ROW];
  __shared__ double s_out[4][NCH * 16];
  __shared__ double s_x[2][4][64];               // [tile parity][wave][lane] flux handed to the partner wave
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = wave & 1, pair = wave >> 1;

  // rows of this wave: layers / levels 0,1,2,.. (even wave) or NLAY-1,NLAY-2,.. / NLAY,NLAY-1,.. (odd wave)
  const long long row_step = half ? -(long long)n : (long long)n;
  const double* __restrict__ od0 = bg_od + (half ? (size_t)(NLAY - 1) * n : 0);
  const float_x2* __restrict__ pr0 = bg_pair + (half ? (size_t)(NLAY / 2 - 1) * n : 0);
  const float* __restrict__ mid = (const float*)(bg_pair + (size_t)(H / 2) * n) + half;
  const double* __restrict__ pl0 = planck_hl + (half ? (size_t)NLAY * n : 0);
  double* tile = s_tile[wave];
  const int rr = lane & 15, qq = lane >> 4;
  int parity = 0;
  int klo = 0;

  // A block works through the chunks blockIdx.x, blockIdx.x + gridDim.x, ...; the launch gives every chunk its own block
  // (gridDim.x = nchunks) unless ECCKD_RT_PERSISTENT asks for one resident round of blocks (see the launch site).  A chunk is
  // what is summed by itself, in the same order, into its own row of `partial`, either way.
  for (long long chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
  int lo = klo, hi = nint - 1;
  while (lo < hi) {
    int mid_k = (lo + hi + 1) >> 1;
    if (iv[mid_k].chunk0 <= chunk) lo = mid_k; else hi = mid_k - 1;
  }
  const int k = lo;
  klo = k;
  // The chunk's tiles are counted from the interval's aligned origin (chunk_layout.hpp): with head = i1 mod 16 every tile
  // starts on a 128-byte line of every row, so a wave's 64 values of a row are four whole lines.  The `head` lanes below i1
  // (the first tile of the interval's first chunk only) are dead like the lanes past p1.
  const ecckd::chunk_layout::Span sp = ecckd::chunk_layout::chunk_span(iv[k].i1, iv[k].i2, iv[k].chunk_pts, iv[k].head, chunk - iv[k].chunk0);
  const long long p0 = sp.p0, p1 = sp.p1;
  // wave-uniform -> scalar loads; the odd waves read the bottom-up copy (k_interval_sums_fit_lw), so that both halves take
  // their layers at ascending constant offsets
  const double* __restrict__ grey = od_fit + ((size_t)(half ? nint : 0) + k) * NLAY;
  double acc[NCH];
#pragma unroll
  for (int j = 0; j < NCH; ++j) acc[j] = 0.0;

  for (long long base = sp.base; base <= p1; base += PTS, parity ^= 1) {
    const long long i = base + pair * 64 + lane;
    const bool live = i >= p0 && i <= p1;
    const size_t ii = (size_t)(i < p0 ? p0 : i > p1 ? p1 : i);      // a dead lane loads a point of the chunk
    double a[H];       // optical depth -> transmittance
    double b[H + 1];   // Planck function -> source of the second sweep
    __builtin_amdgcn_s_setprio(ECCKD_PRIO_LOAD);     // a wave that is about to issue its 55 loads goes ahead of the waves that are computing
    // Addresses: a wave-uniform row pointer (scalar registers, advanced row by row with scalar adds) + the point's 32-bit byte
    // offset in a row (8 bytes per point in the DOUBLE rows and in the FLOAT-pair rows alike).  The row step is made opaque
    // once per tile, otherwise the compiler keeps all 42-55 row pointers of the unrolled loads in scalar registers across the
    // tile loop and spills them.
    if constexpr (BLK) {
      // Line-blocked operands (sweep_layout.hpp; planck_hl, bg_od and bg_pair are then the blocked matrices): the lane's byte
      // offset of its point in row 0, once per tile and 32 bits wide, and every row a compile-time r * 128 bytes from it.  The
      // even wave counts up from row 0, the odd wave down from its last row: one arm of loads each, all within the immediate
      // offset of a load, no row pointer to advance.  A wave's 64 points of its half column are four contiguous pieces.
      namespace sl = ecckd::sweep_layout;
      constexpr int LB = (int)sl::LINE_BYTES;
      constexpr unsigned BG_ROWS = BG32 ? H : NLAY;
      static_assert(H * LB < 4096, "a half column's rows within a load's immediate offset");
      const unsigned line = (unsigned)(ii / sl::LINE_PTS), in_line = (unsigned)(ii % sl::LINE_PTS) * (unsigned)sl::ELEM_BYTES;
      const unsigned voff_p = line * (unsigned)(NHL * LB) + in_line;          // sweep_layout::point_base(NHL, ii), in 32 bits: the gas
      const unsigned voff_b = line * (BG_ROWS * LB) + in_line;                // has the matrices only where they hold every offset
      const char* const pl_blk = (const char*)planck_hl;
      const char* const bg_blk = BG32 ? (const char*)bg_pair : (const char*)bg_od;
      float_x2 v[H / 2];
      float vm = 0.f;
      auto loads = [&](auto dir) {
        constexpr int S = decltype(dir)::value;       // +1: rows 0, 1, ..; -1: the last row, the one before it, ..
        if constexpr (BG32) {
          const char* r0 = bg_blk + (S < 0 ? (H - 1) * LB : 0) + voff_b;
#pragma unroll
          for (int q = 0; q < H / 2; ++q) v[q] = __builtin_nontemporal_load((const float_x2*)(r0 + S * q * LB));
          if (H & 1) vm = __builtin_nontemporal_load((const float*)(bg_blk + ((H / 2) * LB + (S < 0 ? 4 : 0)) + voff_b));
        } else {
          const char* r0 = bg_blk + (S < 0 ? (NLAY - 1) * LB : 0) + voff_b;
#pragma unroll
          for (int l = 0; l < H; ++l) a[l] = __builtin_nontemporal_load((const double*)(r0 + S * l * LB));
        }
        const char* r0 = pl_blk + (S < 0 ? NLAY * LB : 0) + voff_p;
#pragma unroll
        for (int l = 0; l <= H; ++l) b[l] = __builtin_nontemporal_load((const double*)(r0 + S * l * LB));
      };
      // (Each arm ends in a marker of its own: two arms that end alike are merged by the compiler into one sequence of loads
      // whose row offsets are selected per wave - 55 address pairs in registers, and spills.)
      if (half) { loads(std::integral_constant<int, -1>{}); asm volatile("; the odd wave's loads are issued"); }
      else { loads(std::integral_constant<int, 1>{}); asm volatile("; the even wave's loads are issued"); }
      if constexpr (BG32) {
#pragma unroll
        for (int q = 0; q < H / 2; ++q) {
          a[2 * q] = (double)(half ? v[q].y : v[q].x);
          a[2 * q + 1] = (double)(half ? v[q].x : v[q].y);
        }
        if (H & 1) a[H - 1] = (double)vm;
      }
    } else {
    const unsigned voff = (unsigned)ii * 8u;
    long long step_b = row_step * 8;
    asm volatile("" : "+s"(step_b));
    if constexpr (BG32) {
      float_x2 v[H / 2];
      float vm = 0.f;
      {
        const char* rp = (const char*)pr0;
#pragma unroll
        for (int q = 0; q < H / 2; ++q, rp += step_b) v[q] = __builtin_nontemporal_load((const float_x2*)(rp + voff));
        if (H & 1) vm = __builtin_nontemporal_load((const float*)((const char*)mid + voff));
      }
      {
        const char* rp = (const char*)pl0;
#pragma unroll
        for (int l = 0; l <= H; ++l, rp += step_b) b[l] = __builtin_nontemporal_load((const double*)(rp + voff));
      }
#pragma unroll
      for (int q = 0; q < H / 2; ++q) {
        a[2 * q] = (double)(half ? v[q].y : v[q].x);
        a[2 * q + 1] = (double)(half ? v[q].x : v[q].y);
      }
      if (H & 1) a[H - 1] = (double)vm;
    } else {
      const char* rp = (const char*)od0;
#pragma unroll
      for (int l = 0; l < H; ++l, rp += step_b) a[l] = __builtin_nontemporal_load((const double*)(rp + voff));
      rp = (const char*)pl0;
#pragma unroll
      for (int l = 0; l <= H; ++l, rp += step_b) b[l] = __builtin_nontemporal_load((const double*)(rp + voff));
    }
    }
    __builtin_amdgcn_s_setprio(ECCKD_PRIO_SWEEP1);  // first sweep: the partner wave waits for its result

    // A lane past the end of the chunk or below the interval's first point (only the chunk's last tile and the interval's
    // first tile have any) sweeps zero Planck functions: every flux of its column is then an exact zero and adds nothing to
    // the level sums - no select per level.
    if (base + PTS - 1 > p1 || base < p0) {
      const double keep = live ? 1.0 : 0.0;
#pragma unroll
      for (int l = 0; l <= H; ++l) b[l] *= keep;
    }
    int slot = 0;
    auto push = [&](double flux) {
      tile[(slot & 15) * ROW + lane] = flux;
      if ((slot & 15) == 15 || slot == NSLOT - 1) {
        const int ch = slot >> 4;
        __builtin_amdgcn_wave_barrier();
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) sum += tile[rr * ROW + qq * 16 + j];
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        acc[ch] += sum;
        __builtin_amdgcn_wave_barrier();
      }
      ++slot;
    };

    // input of the first sweep: nothing comes down at the top; the surface emits its Planck function (:126-128)
    double flux = half ? b[0] : 0.0;
    push(flux);
    auto layer = [&](int l, double eps, double fac) {
      const double emf = eps - fac;
      const double t = 1.0 - eps;
      const double near = b[l], far = b[l + 1];
      flux = flux * t + near * emf + far * fac;
      a[l] = t;
      b[l] = far * emf + near * fac;          // source of the opposite direction, for the second sweep
      push(flux);
    };
#pragma unroll
    for (int l = 0; l + 1 < H; l += 2) {
      double eps0, fac0, eps1, fac1;
      eps_fac_pair(a[l] + grey[l], a[l + 1] + grey[l + 1], eps0, fac0, eps1, fac1);
      layer(l, eps0, fac0);
      layer(l + 1, eps1, fac1);
    }
    if (H & 1) {
      double eps0, fac0;
      eps_fac_one(a[H - 1] + grey[H - 1], eps0, fac0);
      layer(H - 1, eps0, fac0);
    }
    // the flux that enters this half from the other side is the partner wave's result
    s_x[parity][wave][lane] = flux;
    __builtin_amdgcn_s_setprio(ECCKD_PRIO_SWEEP2);
    __syncthreads();
    flux = s_x[parity][wave ^ 1][lane];
#pragma unroll
    for (int l = H - 1; l >= 0; --l) {
      flux = flux * a[l] + b[l];
      push(flux);
    }
    // (the rows NSLOT % 16 .. 15 of the last group keep the values of the group before: they reach only the sums of slots
    // >= NSLOT, which nothing reads)
  }

  if (lane < 16) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) s_out[wave][j * 16 + lane] = acc[j];
  }
  __syncthreads();      // the next chunk's s_out is written behind at least one more barrier (its tile loop)
  for (int t = tid; t < 2 * NHL; t += RT_THREADS) {
    // even waves (0, 2): slot 1+i = dn[i+1], slot H+1+k = up[H-1-k];
    // odd waves (1, 3):  slot 0 = up[NLAY], slot 1+i = up[NLAY-1-i], slot H+1+k = dn[H+1+k]
    int par = -1, sl = -1;
    if (t < NHL) {                       // flux_dn at level t
      if (t >= 1 && t <= H) { par = 0; sl = t; }
      else if (t > H) { par = 1; sl = t; }
    } else {                             // flux_up at level u
      const int u = t - NHL;
      if (u == NLAY) { par = 1; sl = 0; }
      else if (u >= H) { par = 1; sl = NLAY - u; }
      else { par = 0; sl = 2 * H - u; }
    }
    double v = 0.0;
    if (sl >= 0) v = s_out[par][sl] + s_out[par + 2][sl];
    partial[(size_t)chunk * 2 * NHL + t] = v;
  }
  }
}

constexpr int COST_GROUPS = ecckd::chunk_layout::COST_GROUPS;    // K5d: groups of 32 chunks per interval it has room for (2 048 chunks)

// K5d: combine chunk partials of each interval in order, heating rate, cost
// (calc_cost_function_lw.cpp:100-109).  grid nint, block 1024 = 8 groups x 128.
__global__ void __launch_bounds__(1024)
k_cost_lw(int nlay, RowMap R, const Interval* __restrict__ iv, long long nchunks_total,
          const double* __restrict__ partial, const double* __restrict__ sums,
          const double* __restrict__ conv, const double* __restrict__ layer_weight,
          double flux_weight, double* __restrict__ err) {
  extern __shared__ double s_mem[];  // [COST_GROUPS][2*nhl] | [2*nhl] | [nlay]
  const int nhl = nlay + 1;
  const int nv = 2 * nhl;
  double* s_grp = s_mem;
  double* s_flux = s_mem + COST_GROUPS * nv;
  double* s_term = s_flux + nv;
  const int k = blockIdx.x;
  const long long c0 = iv[k].chunk0;
  const long long c1 = (k + 1 < (int)gridDim.x) ? iv[k + 1].chunk0 : nchunks_total;
  const int tid = threadIdx.x;
  // The interval's chunks are added up in groups of 32 consecutive chunks (each group from 0.0 in chunk order), the groups
  // then in ascending order: a function of the interval's chunk count alone.  Thread group g (128 threads: one per flux
  // value) takes the chunk groups g, g + 8, ...; sixteen loads are in flight together.
  const int g = tid >> 7, t = tid & 127;
  const long long ncg = (c1 - c0 + 31) / 32;
  for (long long cg = g; cg < ncg; cg += 8) {
    const long long cb = c0 + cg * 32;
    const int cnt = (int)((c1 - cb) < 32 ? (c1 - cb) : 32);
    if (t < nv) {
      // sixteen loads in flight, unconditionally (behind the end of a short group: its last chunk again, the value replaced
      // by 0.0), added in chunk order.  (All 32 of a group in flight: 11.7 instead of 10.1 us per launch - the one CU that sums
      // an interval is bound by its own load path, not by the round trips.)
      double a = 0.0;
#pragma unroll 1
      for (int h = 0; h < 32; h += 16) {
        double q[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) q[u] = partial[(size_t)(cb + (h + u < cnt ? h + u : cnt - 1)) * nv + t];
#pragma unroll
        for (int u = 0; u < 16; ++u) a += h + u < cnt ? q[u] : 0.0;      // + 0.0 changes nothing
      }
      s_grp[(size_t)cg * nv + t] = a;
    }
  }
  __syncthreads();
  for (int v = tid; v < nv; v += 1024) {
    double a = 0.0;
    for (long long cg = 0; cg < ncg; ++cg) a += s_grp[(size_t)cg * nv + v];
    s_flux[v] = a;
  }
  __syncthreads();
  const double* s = sums + (size_t)k * R.total;
  const double* dn = s_flux;
  const double* up = s_flux + nhl;
  for (int l = tid; l < nlay; l += 1024) {
    // heating_rate_single (heating_rate.h:55-72) and the weighted squared difference
    const double hr_fit = conv[l] * (dn[l + 1] - dn[l] - up[l + 1] + up[l]);
    const double d = hr_fit - s[R.H + l];
    s_term[l] = layer_weight[l] * (d * d);
  }
  __syncthreads();
  if (tid == 0) {
    double ss = 0.0;
    for (int l = 0; l < nlay; ++l) ss += s_term[l];
    const double hr_weight = 3600.0 * 24.0;
    const double dsurf = dn[nlay] - s[R.FDS];
    const double dtoa = up[0] - s[R.FUT];
    err[k] = sqrt(hr_weight * hr_weight * ss + flux_weight * (dsurf * dsurf + dtoa * dtoa));
  }
}


// ===========================================================================
// Shortwave twins (find_g_points.cpp do_sw branches).
//
// K4-SW.  Gas preparation: direct-beam RT of background+target
// (radiative_transfer_direct_sw, radiative_transfer_sw.cpp:26-43), heating rate from
// the direct beam only (find_g_points.cpp:1003-1006, :1040-1041), metric * ssi rows, and
// for the total-transmission method the per-point direct fluxes that
// fit_optical_depth_sw_total_trans sums (:171-204) plus the two scaled "truth" fields
// (:1011-1034, :1060-1090).  One thread per sorted wavenumber.
// This is the general form (any number of layers, FLOAT or DOUBLE spectra): the (level, wavenumber) matrices are gathered
// through ireorder, the tile sums of the rows are made afterwards by k_tile_sums.  54 layers of FLOAT optical depths take
// k_gas_prep_sw_staged below.
template <typename BgT, typename OdT>
__global__ void __launch_bounds__(PREP_THREADS)
k_gas_prep_sw(int nlay, size_t n, size_t src_stride, int method, double cos_sza, double min_scaling,
              double max_scaling, const int32_t* __restrict__ ireorder, const double* __restrict__ conv,
              const double* __restrict__ ssi_src, const double* __restrict__ albedo_src,
              const BgT* __restrict__ bg_src, const OdT* __restrict__ od_src,
              double* __restrict__ ssi_s, double* __restrict__ bg_od, double* __restrict__ w1,
              double* __restrict__ w2, double* __restrict__ cnt, double* __restrict__ hr,
              double* __restrict__ fds, double* __restrict__ fut, double* __restrict__ tf,
              double* __restrict__ tg, double* __restrict__ hr_low, double* __restrict__ hr_high,
              double* __restrict__ fx) {
  // no contraction of a * b + c beyond the explicit fma of exp_fast: this kernel and the staged one then give the same bits
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t j = (size_t)ireorder[i];
  const bool is_log = method == ECCKD_AVG_LOGARITHMIC;
  const bool is_tt = method == ECCKD_AVG_TOTAL_TRANSMISSION;
  const double s = ssi_src[j];
  ssi_s[i] = s;
  const double minus_sec_sza = -1.0 / cos_sza;
  double flux = cos_sza * s;
  double fl_low = flux, fl_high = flux;
  double tfv = s, tgv = s;  // :178-179 start from ssi, not cos_sza*ssi
  // inputs are fetched nine layers at a time and one chunk ahead: a load issued after a store waits for that store on this
  // hardware (one counter, in order), so one load per layer would cost one store latency per layer; requested before the
  // chunk's own stores, the wait for them overlaps the chunk's arithmetic
  constexpr int CH = 9;
  BgT bgn[CH];
  OdT odn[CH];
  // no background: the loads still happen (from the target's own array, same shape, when its elements are at least as wide)
  // and their values are dropped - a branch round each load would put a full wait behind it
  const bool has_bg = bg_src != nullptr;
  constexpr bool BG_ALIAS = sizeof(BgT) <= sizeof(OdT);
  const BgT* __restrict__ bsrc = (has_bg || !BG_ALIAS) ? bg_src : reinterpret_cast<const BgT*>(od_src);
  auto load_bg = [&](size_t at) -> BgT {
    if (BG_ALIAS) { const BgT v = bsrc[at]; return has_bg ? v : (BgT)0; }
    return has_bg ? bg_src[at] : (BgT)0;
  };
  auto fetch = [&](int l0) {
#pragma unroll
    for (int q = 0; q < CH; ++q) {
      const int lq = l0 + q < nlay ? l0 + q : nlay - 1;
      bgn[q] = load_bg((size_t)lq * src_stride + j);
      odn[q] = od_src[(size_t)lq * src_stride + j];
    }
  };
  fetch(0);
  for (int l0 = 0; l0 < nlay; l0 += CH) {
  BgT bgv[CH];
  OdT odv[CH];
#pragma unroll
  for (int q = 0; q < CH; ++q) { bgv[q] = bgn[q]; odv[q] = odn[q]; }
  if (l0 + CH < nlay) fetch(l0 + CH);
#pragma unroll
  for (int q = 0; q < CH; ++q) {
    const int l = l0 + q;
    if (l >= nlay) continue;
    const double bg = (double)bgv[q];
    const double od = (double)odv[q];
    const size_t o = (size_t)l * n + i;
    __builtin_nontemporal_store(bg, &bg_od[o]);      // written once, read by later kernels: streaming stores
    const double flux_next = flux * ecckd::exp_fast(minus_sec_sza * (bg + od));
    const double hrv = conv[l] * (flux_next - flux);
    __builtin_nontemporal_store(hrv, &hr[o]);
    flux = flux_next;
    double m = od;                       // find_g_points.cpp:1119-1150: linear, logarithmic, total-transmission
    if (method == ECCKD_AVG_TRANSMISSION) m = 1.0 - ecckd::exp_fast(-od * kD);
    else if (method == ECCKD_AVG_TRANSMISSION_2) m = 1.0 - ecckd::exp_fast(-od * kD * 2.0);
    else if (method == ECCKD_AVG_SQUARE_ROOT) m = sqrt(od);
    if (!is_log) {
      const double a = m * s;
      __builtin_nontemporal_store(a, &w1[o]);
    } else {
      const bool pos = m > 0.0;
      const double a = pos ? log(m) * s : 0.0, b = pos ? s : 0.0, c = pos ? 1.0 : 0.0;
      __builtin_nontemporal_store(a, &w1[o]); __builtin_nontemporal_store(b, &w2[o]); __builtin_nontemporal_store(c, &cnt[o]);
    }
    if (is_tt) {
      // :191-192
      tgv *= ecckd::exp_fast(-2.0 * bg);
      tfv *= ecckd::exp_fast(-2.0 * (bg + od));
      const double lo_next = fl_low * ecckd::exp_fast(minus_sec_sza * (bg + min_scaling * od));
      const double hl = conv[l] * (lo_next - fl_low);
      fl_low = lo_next;
      const double hi_next = fl_high * ecckd::exp_fast(minus_sec_sza * (bg + max_scaling * od));
      const double hh = conv[l] * (hi_next - fl_high);
      fl_high = hi_next;
      __builtin_nontemporal_store(tgv, &tg[o]); __builtin_nontemporal_store(tfv, &tf[o]);
      __builtin_nontemporal_store(hl, &hr_low[o]); __builtin_nontemporal_store(hh, &hr_high[o]);
    }
  }
  }
  fds[i] = flux;
  fut[i] = 0.0;  // find_g_points.cpp:1047-1050: no upwelling in the base truth
  if (is_tt) {
    double up_low = 0.0, up_high = 0.0;
    if (albedo_src) {
      // radiative_transfer_norayleigh_sw (radiative_transfer_sw.cpp:72-76), two-stream secant 2
      const double alb = albedo_src[j];
      up_low = fl_low * alb;
      up_high = fl_high * alb;
      for (int l = nlay - 1; l >= 0; --l) {
        const double bg = (double)load_bg((size_t)l * src_stride + j);
        const double od = (double)od_src[(size_t)l * src_stride + j];
        up_low = up_low * ecckd::exp_fast(-2.0 * (bg + min_scaling * od));
        up_high = up_high * ecckd::exp_fast(-2.0 * (bg + max_scaling * od));
      }
    }
    fx[i] = fl_low;
    fx[2 * n + i] = fl_high;
    fx[n + i] = up_low;
    fx[3 * n + i] = up_high;
  }
}

// K4-SW, staged form (54 layers, FLOAT optical depths: the CKDMIP spectra).  The same arithmetic as k_gas_prep_sw, with the
// inputs brought in differently: k_scatter_column_halves leaves each point's column at its rank as PARTS runs of H = 54 / PARTS
// layers, [PARTS][npad][H], so that the H-layer block of a wave's 64 points is one contiguous, 256-byte aligned piece.  The wave
// copies it into LDS with full-width loads and every lane reads its own column back from there.  Reading the columns
// straight from memory, one 4-byte element per lane and layer at a stride of 216 bytes, took 64 cache lines per load
// instruction and more time than the arithmetic and the row stores together (ablation).  The upward
// sweep of the total-transmission truths starts on the part that is still staged and fetches the others once more.
// Row sums: the (at most seven) values a layer adds to the table go through a wave-private [7][65] tile, summed per layer.
// Three parts of 18 layers: 51 KB of LDS per block, three blocks (three waves per SIMD) per compute unit.
constexpr int SWS_TR = 7, SWS_TW = 65, SW_STAGE_PARTS = 3;
template <int PARTS, typename BgT>
__global__ void __launch_bounds__(PREP_THREADS, sizeof(BgT) == 4 ? PARTS : 2)
k_gas_prep_sw_staged(size_t n, size_t npad, int method, double cos_sza, double min_scaling, double max_scaling,
                     const int32_t* __restrict__ ireorder, const double* __restrict__ conv,
                     const double* __restrict__ ssi_src, const double* __restrict__ albedo_src,
                     const BgT* __restrict__ bg_half, const float* __restrict__ od_half,
                     double* __restrict__ ssi_s, double* __restrict__ bg_od, double* __restrict__ w1,
                     double* __restrict__ w2, double* __restrict__ cnt, double* __restrict__ hr,
                     double* __restrict__ fds, double* __restrict__ fut, double* __restrict__ tf,
                     double* __restrict__ tg, double* __restrict__ hr_low, double* __restrict__ hr_high,
                     double* __restrict__ fx, RowMap R, double* __restrict__ wave_part, size_t nw) {
#pragma clang fp contract(off)
  constexpr int H = 54 / PARTS;
  static_assert(H * PARTS == 54 && (64 * H) % 4 == 0, "whole parts, whole float4s");
  __shared__ __attribute__((aligned(16))) float s_od[4][64 * H];
  __shared__ __attribute__((aligned(16))) BgT s_bg[4][64 * H];     // a DOUBLE (merged) background: 70 KB per block, two blocks per CU
  __shared__ double s_sum[4][SWS_TR * SWS_TW];
  __shared__ int s_row[4][SWS_TR];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t wid = (size_t)blockIdx.x * 4 + wave;
  if (wid * 64 >= n) return;   // a whole wave past the end (no block-wide barrier below)
  const size_t i0 = wid * 64 + lane;
  const bool live = i0 < n;
  const size_t i = live ? i0 : n - 1;
  const bool has_bg = bg_half != nullptr;
  float* const my_od = s_od[wave];
  BgT* const my_bg = s_bg[wave];
  double* const my_sum = s_sum[wave];
  int* const my_row = s_row[wave];

  // this wave's 64 x H block of part h: contiguous and 256-byte aligned (npad is a multiple of 64)
  auto stage = [&](int h) {
    constexpr int NV = 64 * H / 4, NIT = (NV + 63) / 64;                    // float4s of the target's block
    constexpr int NVB = NV * (int)(sizeof(BgT) / 4);                        // 16-byte pieces of the background's block
    const float4* so = reinterpret_cast<const float4*>(od_half + ((size_t)h * npad + wid * 64) * H);
    // no background: the loads still happen, from the target's block (a branch round them would put a full wait behind each)
    const float4* sb = has_bg ? reinterpret_cast<const float4*>(bg_half + ((size_t)h * npad + wid * 64) * H) : so;
    __builtin_amdgcn_wave_barrier();   // the lanes are done with the part staged before
    // both arrays' loads go out together, then the LDS writes: one memory round trip per staging
#pragma unroll
    for (int t = 0; t < NIT; ++t) {
      const int at = t * 64 + lane;
      if (at < NV) {
        const float4 vo = so[at], vb = sb[at];
        reinterpret_cast<float4*>(my_od)[at] = vo;
        reinterpret_cast<float4*>(my_bg)[at] = vb;
      }
    }
    if (NVB > NV) {                    // a DOUBLE background: the second half of its block
#pragma unroll
      for (int t = 0; t < NIT; ++t) {
        const int at = NV + t * 64 + lane;
        if (at < NVB) reinterpret_cast<float4*>(my_bg)[at] = sb[at];
      }
    }
    __builtin_amdgcn_wave_barrier();
  };
  int slot = 0;
  auto push = [&](int row, double v) {
    my_sum[slot * SWS_TW + lane] = live ? v : 0.0;
    my_row[slot] = row;
    ++slot;
  };
  // the sums of the pushed rows over the wave's 64 points: lane (r, q) adds eight points of row r, three exchanges add the eighths
  auto flush = [&]() {
    const int rr = lane & 7, qq = lane >> 3;
    __builtin_amdgcn_wave_barrier();
    double sum = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) sum += rr < slot ? my_sum[rr * SWS_TW + qq * 8 + q] : 0.0;
    sum += __shfl_xor(sum, 8, 64);
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (qq == 0 && rr < slot) wave_part[(size_t)my_row[rr] * nw + wid] = sum;
    __builtin_amdgcn_wave_barrier();
    slot = 0;
  };

  const size_t j = (size_t)ireorder[i];
  const bool is_log = method == ECCKD_AVG_LOGARITHMIC;
  const bool is_tt = method == ECCKD_AVG_TOTAL_TRANSMISSION;
  const double s = ssi_src[j];
  if (live) ssi_s[i] = s;
  const double minus_sec_sza = -1.0 / cos_sza;
  double flux = cos_sza * s;
  double fl_low = flux, fl_high = flux;
  double tfv = s, tgv = s;  // :178-179 start from ssi, not cos_sza*ssi
  for (int h = 0; h < PARTS; ++h) {
    stage(h);
#pragma unroll 2
    for (int k = 0; k < H; ++k) {
      const int l = h * H + k;
      const double bg = has_bg ? (double)my_bg[lane * H + k] : 0.0;
      const double od = (double)my_od[lane * H + k];
      const size_t o = (size_t)l * n + i;
      if (live) __builtin_nontemporal_store(bg, &bg_od[o]);      // written once, read by later kernels: streaming stores
      const double flux_next = flux * ecckd::exp_fast(minus_sec_sza * (bg + od));
      const double hrv = conv[l] * (flux_next - flux);
      if (live) __builtin_nontemporal_store(hrv, &hr[o]);
      push(R.H + l, hrv);
      flux = flux_next;
      double m = od;                       // find_g_points.cpp:1119-1150: linear, logarithmic, total-transmission
      if (method == ECCKD_AVG_TRANSMISSION) m = 1.0 - ecckd::exp_fast(-od * kD);
      else if (method == ECCKD_AVG_TRANSMISSION_2) m = 1.0 - ecckd::exp_fast(-od * kD * 2.0);
      else if (method == ECCKD_AVG_SQUARE_ROOT) m = sqrt(od);
      if (!is_log) {
        const double a = m * s;
        if (live) __builtin_nontemporal_store(a, &w1[o]);
        push(R.A + l, a);
        push(R.B + l, s);
      } else {
        const bool pos = m > 0.0;
        const double a = pos ? log(m) * s : 0.0, b = pos ? s : 0.0, c = pos ? 1.0 : 0.0;
        if (live) { __builtin_nontemporal_store(a, &w1[o]); __builtin_nontemporal_store(b, &w2[o]); __builtin_nontemporal_store(c, &cnt[o]); }
        push(R.A + l, a);
        push(R.B + l, b);
        push(R.N + l, c);
      }
      if (is_tt) {
        // :191-192
        tgv *= ecckd::exp_fast(-2.0 * bg);
        tfv *= ecckd::exp_fast(-2.0 * (bg + od));
        const double lo_next = fl_low * ecckd::exp_fast(minus_sec_sza * (bg + min_scaling * od));
        const double hl = conv[l] * (lo_next - fl_low);
        fl_low = lo_next;
        const double hi_next = fl_high * ecckd::exp_fast(minus_sec_sza * (bg + max_scaling * od));
        const double hh = conv[l] * (hi_next - fl_high);
        fl_high = hi_next;
        if (live) {
          __builtin_nontemporal_store(tgv, &tg[o]); __builtin_nontemporal_store(tfv, &tf[o]);
          __builtin_nontemporal_store(hl, &hr_low[o]); __builtin_nontemporal_store(hh, &hr_high[o]);
        }
        push(R.TG + l, tgv);
        push(R.TF + l, tfv);
        push(R.HL + l, hl);
        push(R.HH + l, hh);
      }
      flush();
    }
  }
  if (live) {
    fds[i] = flux;
    fut[i] = 0.0;  // find_g_points.cpp:1047-1050: no upwelling in the base truth
  }
  push(R.FDS, flux);
  push(R.FUT, 0.0);
  if (is_tt) {
    double up_low = 0.0, up_high = 0.0;
    if (albedo_src) {
      // radiative_transfer_norayleigh_sw (radiative_transfer_sw.cpp:72-76), two-stream secant 2; the lowest part is still staged
      const double alb = albedo_src[j];
      up_low = fl_low * alb;
      up_high = fl_high * alb;
      for (int h = PARTS - 1; h >= 0; --h) {
        if (h != PARTS - 1) stage(h);
#pragma unroll 3
        for (int k = H - 1; k >= 0; --k) {
          const double bg = has_bg ? (double)my_bg[lane * H + k] : 0.0;
          const double od = (double)my_od[lane * H + k];
          up_low = up_low * ecckd::exp_fast(-2.0 * (bg + min_scaling * od));
          up_high = up_high * ecckd::exp_fast(-2.0 * (bg + max_scaling * od));
        }
      }
    }
    if (live) {
      fx[i] = fl_low;
      fx[2 * n + i] = fl_high;
      fx[n + i] = up_low;
      fx[3 * n + i] = up_high;
    }
    push(R.FDSL, fl_low);
    push(R.FUTL, up_low);
    push(R.FDSH, fl_high);
    push(R.FUTH, up_high);
  }
  flush();
}

// K5b-SW: fit_optical_depth_sw (find_g_points.cpp:112-165) and
// fit_optical_depth_sw_total_trans (:171-204) from the interval sums.
// Writes npass fits per interval: pass 0 (and pass 1 for total-transmission:
// fit*min_scaling, fit*max_scaling, :357 and :371).
__global__ void __launch_bounds__(128)
k_fit_sw(int nlay, int method, RowMap R, int nint, double min_scaling, double max_scaling,
         const Interval* __restrict__ iv, const double* __restrict__ sums, double* __restrict__ od_fit) {
#pragma clang fp contract(off)
  extern __shared__ double s_fit[];  // [nlay]
  const int k = blockIdx.x;
  const double* s = sums + (size_t)k * R.total;
  if (method != ECCKD_AVG_TOTAL_TRANSMISSION) {
    for (int l = threadIdx.x; l < nlay; l += blockDim.x) {
      const double a = s[R.A + l];
      double fit;
      if (method == ECCKD_AVG_LOGARITHMIC) {
        const double b = s[R.B + l];
        const double nnz = s[R.N + l];
        const double ntot = (double)(iv[k].i2 - iv[k].i1 + 1);
        if (nnz == ntot) fit = exp(a / b);
        else if (nnz == 0.0) fit = 0.0;
        else fit = exp(a / b) * (nnz / ntot);
      } else {
        const double norm_factor = 1.0 / s[R.B];  // sum(ssi(range(i1,i2)))
        switch (method) {
          case ECCKD_AVG_LINEAR: fit = a * norm_factor; break;
          // :123-124: the clamp is applied BEFORE the normalisation
          // contraction is OFF in this kernel: the product must be ROUNDED before the subtraction.
          // A fused 1 - a*(1/b) keeps the rounding error of 1/b and goes negative when a == b
          // (saturated interval), turning the reference's log(0) = -inf into log(<0) = NaN.
          case ECCKD_AVG_TRANSMISSION:
            fit = fabs(-log(1.0 - fmin(0.9999999999999999, a) * norm_factor) / kD); break;
          case ECCKD_AVG_TRANSMISSION_2:
            fit = fabs(-log(1.0 - fmin(0.9999999999999999, a) * norm_factor) / (kD * 2.0)); break;
          case ECCKD_AVG_SQUARE_ROOT: { const double v = a * norm_factor; fit = v * v; break; }
          default: fit = nan("");
        }
      }
      od_fit[(size_t)k * nlay + l] = fit;
    }
    return;
  }
  // total-transmission (:189-203).  The reference walks the layers in order; a layer whose direct beam has
  // vanished replaces the WHOLE vector by the linear average and the walk continues, so the outcome is:
  // layers above and at the LAST such layer carry the linear average, layers below it their own fit.
  // One thread per layer; the last invalid layer is found with an integer LDS max.
  __shared__ int s_last_invalid;
  if (threadIdx.x == 0) s_last_invalid = -1;
  __syncthreads();
  const double ssum = s[R.B];
  const double norm_factor = 1.0 / ssum;
  for (int iz = threadIdx.x; iz < nlay; iz += blockDim.x) {
    const double base_bg = s[R.TG + iz], base = s[R.TF + iz];
    if (!(base_bg > 0.0 && base > 0.0)) atomicMax(&s_last_invalid, iz);
  }
  __syncthreads();
  const int last_invalid = s_last_invalid;
  for (int iz = threadIdx.x; iz < nlay; iz += blockDim.x) {
    if (iz > last_invalid) {
      const double top = iz == 0 ? ssum : s[R.TF + iz - 1];
      const double top_bg = iz == 0 ? ssum : s[R.TG + iz - 1];
      const double bg_od_fit = -0.5 * log(s[R.TG + iz] / top_bg);
      s_fit[iz] = -0.5 * log(s[R.TF + iz] / top) - bg_od_fit;
    } else {
      s_fit[iz] = s[R.A + iz] * norm_factor;
    }
  }
  __syncthreads();
  for (int l = threadIdx.x; l < nlay; l += blockDim.x) {
    od_fit[(size_t)k * nlay + l] = s_fit[l] * min_scaling;
    od_fit[((size_t)nint + k) * nlay + l] = s_fit[l] * max_scaling;
  }
}

// K5c-SW: radiative_transfer_direct_sw_bb / _norayleigh_sw_bb
// (radiative_transfer_sw.cpp:118-141, :147-184) for every interval: reads ssi and the
// background optical depth rows, (nlay+1)*8 B per point.  partial[chunk] =
// { sum ssi, dn[1..nlay], up[0..nlay] } (dn[0] = cos_sza * sum ssi is formed in K5d as the
// reference does, :128).  Same chunking and reduction order as the LW kernel.
__global__ void __launch_bounds__(RT_THREADS)
k_rt_sw_bb(int nlay, size_t n, int nint, const Interval* __restrict__ iv,
           double cos_sza, const double* __restrict__ ssi, const double* __restrict__ bg_od,
           const double* __restrict__ od_fit, double* __restrict__ partial) {
  extern __shared__ double s_mem[];  // [4][2*nhl] | [nlay]
  const int nhl = nlay + 1;
  double* s_acc = s_mem;
  double* s_grey = s_mem + 4 * 2 * nhl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long chunk = blockIdx.x;
  int lo = 0, hi = nint - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (iv[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
  }
  const int k = lo;
  const double albedo = iv[k].albedo;
  const long long chunk_pts = iv[k].chunk_pts;
  const long long c = chunk - iv[k].chunk0;
  const long long p0 = iv[k].i1 + c * chunk_pts;
  long long p1 = p0 + chunk_pts - 1;
  if (p1 > iv[k].i2) p1 = iv[k].i2;
  for (int t = tid; t < 4 * 2 * nhl; t += RT_THREADS) s_acc[t] = 0.0;
  for (int l = tid; l < nlay; l += RT_THREADS) s_grey[l] = od_fit[(size_t)k * nlay + l];
  __syncthreads();
  double* acc_dn = s_acc + wave * 2 * nhl;
  double* acc_up = acc_dn + nhl;
  const double minus_sec_sza = -1.0 / cos_sza;
  for (long long base = p0; base <= p1; base += RT_THREADS) {
    const long long i = base + tid;
    const bool live = i <= p1;
    const size_t ii = live ? (size_t)i : (size_t)p1;
    const double sv = live ? ssi[ii] : 0.0;
    {
      const double s0 = wave_sum(sv);
      if (lane == 0) acc_dn[0] += s0;
    }
    double flux = cos_sza * sv;
    for (int l = 0; l < nlay; ++l) {
      flux = flux * exp(minus_sec_sza * (bg_od[(size_t)l * n + ii] + s_grey[l]));
      const double sl = wave_sum(flux);
      if (lane == 0) acc_dn[l + 1] += sl;
    }
    if (albedo > 0.0) {
      flux *= albedo;
      {
        const double sl = wave_sum(flux);
        if (lane == 0) acc_up[nlay] += sl;
      }
      for (int l = nlay - 1; l >= 0; --l) {
        flux = flux * exp(-2.0 * (bg_od[(size_t)l * n + ii] + s_grey[l]));
        const double sl = wave_sum(flux);
        if (lane == 0) acc_up[l] += sl;
      }
    }
  }
  __syncthreads();
  for (int t = tid; t < 2 * nhl; t += RT_THREADS) {
    partial[(size_t)chunk * 2 * nhl + t] =
        ((s_acc[t] + s_acc[2 * nhl + t]) + s_acc[4 * nhl + t]) + s_acc[6 * nhl + t];
  }
}



// K5c-SW fast path: NLAY known at compile time.  The column of total optical depths (background + grey) stays in
// registers for both sweeps (direct beam down, radiative_transfer_sw.cpp:134-139, reflected beam up, :176-183:
// two different exponents per layer, no sources), level sums through the wave-private transposed LDS tile of the
// longwave path.  Slots: 0 = sum of the solar irradiance, 1..NLAY = flux_dn below each layer, NLAY+1 = flux_up at the
// surface, NLAY+2.. = flux_up above each layer going up.
// NFIT = 2 (total-transmission with min_scaling != max_scaling, find_g_points.cpp:374-386): the column is fetched once and
// swept with both fitted optical depths, partial sums of the second fit nchunks * 2 NHL further on.
// SAME: cos_sza == 0.5, so -tau / cos_sza == -2 tau exactly and the transmittance of the way down is the one of the way up
// (radiative_transfer_sw.cpp:134-139 and :176-183): the last fit overwrites the column with it instead of evaluating it twice.
// (three blocks per CU only where the column's transmittance is shared by the two beams: without SAME the second exponential's
// temporaries do not fit 168 registers - 56 B per lane went to scratch - and the cosine is the reference's 0.5 everywhere but in tests)
template <int NLAY, int NFIT, bool SAME, int OCC = (NFIT == 1 && SAME ? 3 : 2)>
__global__ void __launch_bounds__(RT_THREADS, OCC)
k_rt_sw_bb_fast(size_t n, int nint, const Interval* __restrict__ iv, double cos_sza,
                const double* __restrict__ ssi, const double* __restrict__ bg_od, const double* __restrict__ od_fit,
                double* __restrict__ partial) {
  constexpr int NHL = NLAY + 1;
  constexpr int NSLOT = 2 * NLAY + 2;
  constexpr int NCH = (NSLOT + 15) / 16;
  constexpr int ROW = 65;
  __shared__ double s_tile[4][16 * ROW];
  __shared__ double s_out[NFIT][4][NCH * 16];
  __shared__ double s_grey[NFIT][NLAY];   // the fitted optical depths: LDS broadcasts (as scalars they take 2 NLAY SGPRs per fit and spill)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long chunk = blockIdx.x;
  int lo = 0, hi = nint - 1;
  while (lo < hi) {
    int mid = (lo + hi + 1) >> 1;
    if (iv[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
  }
  const int k = lo;
  const long long chunk_pts = iv[k].chunk_pts;
  const long long c = chunk - iv[k].chunk0;
  const long long p0 = iv[k].i1 + c * chunk_pts;
  long long p1 = p0 + chunk_pts - 1;
  if (p1 > iv[k].i2) p1 = iv[k].i2;
  for (int t = tid; t < NFIT * NLAY; t += RT_THREADS) {
    const int f = t / NLAY, l = t - f * NLAY;
    s_grey[f][l] = od_fit[((size_t)f * nint + k) * NLAY + l];
  }
  __syncthreads();
  double* tile = s_tile[wave];
  const int rr = lane & 15, qq = lane >> 4;
  double acc[NFIT][NCH];
#pragma unroll
  for (int f = 0; f < NFIT; ++f) {
#pragma unroll
    for (int j = 0; j < NCH; ++j) acc[f][j] = 0.0;
  }
  const double minus_sec_sza = -1.0 / cos_sza;
  // exp with its coefficients in scalar registers (fastmath.hpp).  A saturated interval fits an infinite optical depth
  // (log(0), find_g_points.cpp:123-124): the argument is held at -800, where the result has already underflowed to 0,
  // because exp_fast_s(-inf) would be inf - inf.
  const ecckd::ExpConsts ek = ecckd::exp_consts();
  auto trans = [&](double x) { return ecckd::exp_fast_s(fmax(x, -800.0), ek); };
  const double albedo = iv[k].albedo;
  const bool reflect = albedo > 0.0;                 // :366-373: no upwelling without a reflecting surface
  for (long long base = p0; base <= p1; base += RT_THREADS) {
    const long long i = base + tid;
    const bool live = i <= p1;
    const size_t ii = live ? (size_t)i : (size_t)p1;
    double tau[NLAY];
    __builtin_amdgcn_s_setprio(3);     // as in the longwave kernel: the wave that is about to fetch its column goes first
    {
      // one wave-uniform row pointer walked with scalar adds + the point's 32-bit byte offset (as in the longwave kernel: the
      // 54 row pointers of the unrolled loads otherwise live in scalar registers across the tile loop and spill)
      const unsigned voff = (unsigned)ii * 8u;
      long long step_b = (long long)n * 8;
      asm volatile("" : "+s"(step_b));
      const char* rp = (const char*)bg_od;
#pragma unroll
      for (int l = 0; l < NLAY; ++l, rp += step_b) tau[l] = __builtin_nontemporal_load((const double*)(rp + voff));
    }
    const double sv = live ? ssi[ii] : 0.0;   // a lane past the end carries zero flux through both sweeps: nothing else to mask
    __builtin_amdgcn_s_setprio(0);
#pragma unroll
    for (int f = 0; f < NFIT; ++f) {
      const double* grey = s_grey[f];
      int slot = 0;
      auto push = [&](double v) {
        tile[(slot & 15) * ROW + lane] = v;
        if ((slot & 15) == 15 || slot == NSLOT - 1) {
          const int ch = slot >> 4;
          __builtin_amdgcn_wave_barrier();
          double sum = 0.0;
#pragma unroll
          for (int j = 0; j < 16; ++j) sum += tile[rr * ROW + qq * 16 + j];
          sum += __shfl_xor(sum, 16, 64);
          sum += __shfl_xor(sum, 32, 64);
          acc[f][ch] += sum;
          __builtin_amdgcn_wave_barrier();
        }
        ++slot;
      };
      push(sv);
      double flux = cos_sza * sv;
      const bool last = f == NFIT - 1;          // compile time after unrolling: the column is free to be overwritten
      if (last && SAME) {
#pragma unroll
        for (int l = 0; l < NLAY; ++l) {
          const double xd = -2.0 * (tau[l] + grey[l]);
          tau[l] = trans(xd);
          flux = flux * tau[l];
          push(flux);
        }
      } else if (last) {
#pragma unroll
        for (int l = 0; l < NLAY; ++l) {
          tau[l] += grey[l];
          const double xd = minus_sec_sza * tau[l];
          flux = flux * trans(xd);
          push(flux);
        }
      } else {
#pragma unroll
        for (int l = 0; l < NLAY; ++l) {
          const double xd = minus_sec_sza * (tau[l] + grey[l]);
          flux = flux * trans(xd);
          push(flux);
        }
      }
      flux = reflect ? flux * albedo : 0.0;
      push(flux);
#pragma unroll
      for (int l = NLAY - 1; l >= 0; --l) {
        if (last && SAME) {
          if (reflect) flux = flux * tau[l];
        } else {
          const double xu = -2.0 * (last ? tau[l] : tau[l] + grey[l]);
          if (reflect) flux = flux * trans(xu);
        }
        push(flux);
      }
      if ((NSLOT & 15) != 0) {
#pragma unroll
        for (int j = (NSLOT & 15); j < 16; ++j) tile[j * ROW + lane] = 0.0;
      }
    }
  }
  if (lane < 16) {
#pragma unroll
    for (int f = 0; f < NFIT; ++f) {
#pragma unroll
      for (int j = 0; j < NCH; ++j) s_out[f][wave][j * 16 + lane] = acc[f][j];
    }
  }
  __syncthreads();
  for (int t = tid; t < NFIT * 2 * NHL; t += RT_THREADS) {
    // flux_dn level t = slot t; flux_up level u = slot NLAY + 1 + (NLAY - u)
    const int f = t / (2 * NHL), tt = t - f * 2 * NHL;
    const int sl = tt < NHL ? tt : NLAY + 1 + (NLAY - (tt - NHL));
    partial[((size_t)f * gridDim.x + chunk) * 2 * NHL + tt] = ((s_out[f][0][sl] + s_out[f][1][sl]) + s_out[f][2][sl]) + s_out[f][3][sl];
  }
}
struct SwTruthRows { int rH[2], rFDS[2], rFUT[2]; };

// K5d-SW: calc_cost_function_sw (calc_cost_function_sw.cpp:86-109): heating rate from the
// direct beam only (:92), truth rows selected by (rH, rFDS, rFUT).
__global__ void __launch_bounds__(1024)
k_cost_sw(int nlay, int ntotal, SwTruthRows rows, const Interval* __restrict__ iv,
          long long nchunks_total, const double* __restrict__ partial_all, size_t partial_pass_stride,
          const double* __restrict__ sums, const double* __restrict__ conv, const double* __restrict__ layer_weight,
          double flux_weight, double cos_sza, double* __restrict__ err_all) {
  // blockIdx.y: which of the (one or two) evaluations of the interval - its truth rows, its sweep's partial sums, its error slot
  const int pass = blockIdx.y;
  const int rH = rows.rH[pass], rFDS = rows.rFDS[pass], rFUT = rows.rFUT[pass];
  const double* __restrict__ partial = partial_all + (size_t)pass * partial_pass_stride;
  double* __restrict__ err = err_all + (size_t)pass * gridDim.x;
  extern __shared__ double s_mem[];
  const int nhl = nlay + 1;
  const int nv = 2 * nhl;
  double* s_grp = s_mem;
  double* s_flux = s_mem + COST_GROUPS * nv;
  double* s_term = s_flux + nv;
  const int k = blockIdx.x;
  const long long c0 = iv[k].chunk0;
  const long long c1 = (k + 1 < (int)gridDim.x) ? iv[k + 1].chunk0 : nchunks_total;
  const int tid = threadIdx.x;
  // The interval's chunks are added up in groups of 32 consecutive chunks (each group from 0.0 in chunk order), the groups
  // then in ascending order: a function of the interval's chunk count alone.  Thread group g (128 threads: one per flux
  // value) takes the chunk groups g, g + 8, ...; sixteen loads are in flight together.
  const int g = tid >> 7, t = tid & 127;
  const long long ncg = (c1 - c0 + 31) / 32;
  for (long long cg = g; cg < ncg; cg += 8) {
    const long long cb = c0 + cg * 32;
    const int cnt = (int)((c1 - cb) < 32 ? (c1 - cb) : 32);
    if (t < nv) {
      // sixteen loads in flight, unconditionally (behind the end of a short group: its last chunk again, the value replaced
      // by 0.0), added in chunk order.  (All 32 of a group in flight: 11.7 instead of 10.1 us per launch - the one CU that sums
      // an interval is bound by its own load path, not by the round trips.)
      double a = 0.0;
#pragma unroll 1
      for (int h = 0; h < 32; h += 16) {
        double q[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) q[u] = partial[(size_t)(cb + (h + u < cnt ? h + u : cnt - 1)) * nv + t];
#pragma unroll
        for (int u = 0; u < 16; ++u) a += h + u < cnt ? q[u] : 0.0;      // + 0.0 changes nothing
      }
      s_grp[(size_t)cg * nv + t] = a;
    }
  }
  __syncthreads();
  for (int v = tid; v < nv; v += 1024) {
    double a = 0.0;
    for (long long cg = 0; cg < ncg; ++cg) a += s_grp[(size_t)cg * nv + v];
    s_flux[v] = a;
  }
  __syncthreads();
  if (tid == 0) s_flux[0] = cos_sza * s_flux[0];  // flux_dn(0) = cos_sza*sum(ssi)
  __syncthreads();
  const double* s = sums + (size_t)k * ntotal;
  const double* dn = s_flux;
  const double* up = s_flux + nhl;
  for (int l = tid; l < nlay; l += 1024) {
    const double hr_fit = conv[l] * (dn[l + 1] - dn[l]);
    const double d = hr_fit - s[rH + l];
    s_term[l] = layer_weight[l] * (d * d);
  }
  __syncthreads();
  if (tid == 0) {
    double ss = 0.0;
    for (int l = 0; l < nlay; ++l) ss += s_term[l];
    const double hr_weight = 3600.0 * 24.0;
    const double dsurf = dn[nlay] - s[rFDS];
    const double dtoa = up[0] - s[rFUT];
    err[k] = sqrt(hr_weight * hr_weight * ss + flux_weight * (dsurf * dsurf + dtoa * dtoa));
  }
}

int gas_ensure_work(ecckd_gas* g, size_t dev_bytes, size_t pinned_bytes) {
  if (dev_bytes > g->work_bytes) {
    if (g->work) {
      ECCKD_HIP_CHECK(hipStreamSynchronize(g->eval_stream()));
      g->give_back(g->work);
      g->work_bytes = 0;
    }
    size_t want = ecckd_align_up(dev_bytes * 2, 1 << 20);
    ECCKD_HIP_CHECK(g->alloc(&g->work, want));
    g->work_bytes = want;
  }
  // the pinned staging area belongs to the context (one caller per context at a time) or to the lane the gas was lent
  if (g->lane) {
    ECCKD_CHECK(ecckd::lane_ensure_pinned(g->lane, pinned_bytes));
    g->pinned = g->lane->pinned;
    g->pinned_bytes = g->lane->pinned_bytes;
    return ECCKD_OK;
  }
  ECCKD_CHECK(ecckd::ensure_pinned(g->ctx, pinned_bytes));
  g->pinned = g->ctx->pinned;
  g->pinned_bytes = g->ctx->pinned_bytes;
  return ECCKD_OK;
}

// The context's table of line-blocked Planck matrices (ecckd_ctx::planck_blk): the gases of a job share the first gas's
// row-major matrix (d_planck_hl_reuse) and with it one blocked copy, which goes when its last holder goes, whichever that is.
// A reference to the copy made from the row-major matrix at `rowmajor`, or nullptr: none is known.
static double* planck_blk_attach(ecckd_ctx* ctx, const void* rowmajor) {
  std::lock_guard<std::mutex> lock(ctx->cache_mutex);
  for (ecckd_ctx::PlanckBlk& e : ctx->planck_blk)
    if (e.rowmajor == rowmajor) { e.refs += 1; return (double*)e.blocked; }
  return nullptr;
}
// A new copy, held once by the gas that made it.  rowmajor: the matrix later gases may name to share it, or nullptr (the
// gas was handed a matrix the table does not know: nobody can tell how long that one lives, the copy stays the gas's own).
static void planck_blk_register(ecckd_ctx* ctx, const void* rowmajor, void* blocked) {
  std::lock_guard<std::mutex> lock(ctx->cache_mutex);
  if (rowmajor)
    for (ecckd_ctx::PlanckBlk& e : ctx->planck_blk)
      if (e.rowmajor == rowmajor) e.rowmajor = nullptr;          // an address handed out again: the old copy is of another matrix
  ctx->planck_blk.push_back({rowmajor, blocked, 1});
}
// One holder less; owned_rowmajor: the holder also frees this row-major matrix, no later gas may attach through it.
static void planck_blk_drop(ecckd_ctx* ctx, void* blocked, const void* owned_rowmajor) {
  void* last = nullptr;
  {
    std::lock_guard<std::mutex> lock(ctx->cache_mutex);
    for (size_t k = 0; k < ctx->planck_blk.size(); ++k) {
      ecckd_ctx::PlanckBlk& e = ctx->planck_blk[k];
      if (owned_rowmajor && e.rowmajor == owned_rowmajor) e.rowmajor = nullptr;
      if (e.blocked == blocked && --e.refs == 0) {
        last = e.blocked;
        ctx->planck_blk.erase(ctx->planck_blk.begin() + (long)k);
        --k;
      }
    }
  }
  ecckd::dev_release(ctx, last);          // takes the mutex itself
}

void gas_free(ecckd_gas* g) {
  if (!g) return;
  ecckd_ctx* ctx = g->ctx;
  if (ctx) (void)hipStreamSynchronize(ctx->stream);
  bool owns_planck = false;
  for (void* b : g->blocks) owns_planck |= b == (void*)g->planck_hl;
  if (g->planck_blk) planck_blk_drop(ctx, g->planck_blk, owns_planck ? g->planck_hl : nullptr);
  for (void* b : g->blocks) ecckd::dev_release(ctx, b);
  delete g;
}

// A gas under construction: whatever leaves the constructor early (ECCKD_HIP_CHECK, ECCKD_REQUIRE) frees it on the way out.
struct GasDeleter { void operator()(ecckd_gas* g) const { gas_free(g); } };
typedef std::unique_ptr<ecckd_gas, GasDeleter> GasPtr;

// The DOUBLE rows of the background optical depths.  A longwave gas whose background is FLOAT holds the FLOAT pairs only
// (ecckd_gas_create_lw); the rows are made from them when something asks: ecckd_gas_view, the run-time-nlay sweep.
// A gas that holds its background line-blocked (bg_blk) has released both; the rows are made from the blocked matrix.
static int gas_bg_rows(ecckd_gas* g) {
  if (g->bg_od || (!g->bg_pair && !g->bg_blk)) return ECCKD_OK;
  ecckd_ctx* ctx = g->ctx;
  ECCKD_HIP_CHECK(g->alloc(&g->bg_od, (size_t)g->nlay * g->n * sizeof(double)));
  const dim3 per_point((unsigned)((g->n + 255) / 256));
  if (g->bg_pair)
    hipLaunchKernelGGL(k_unpack_bg32, per_point, dim3(256), 0, ctx->stream, g->nlay / 2, g->n, (const float_x2_store*)g->bg_pair, g->bg_od);
  else if (g->bg_blk_pairs)
    hipLaunchKernelGGL(k_unpack_bg32_blocked, per_point, dim3(256), 0, ctx->stream, g->nlay / 2, g->n, (const float_x2_store*)g->bg_blk,
                       g->bg_od);
  else
    hipLaunchKernelGGL(k_reblock<false>, dim3((unsigned)(((size_t)g->nlay * g->n + 255) / 256)), dim3(256), 0, ctx->stream, (unsigned)g->nlay,
                       g->n, (const unsigned long long*)g->bg_blk, (unsigned long long*)g->bg_od);
  ECCKD_HIP_CHECK(hipGetLastError());
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return ECCKD_OK;
}

// The operands of the mirror sweep of a prepared longwave gas, line-blocked (sweep_layout.hpp), where the aligned mirror path
// runs - otherwise the gas stays as it is.  The background: a blocked copy of what the sweep reads, the FLOAT pairs or the
// DOUBLE rows (one pass, every line read once and stored once), after which the row-major matrices are released; for its
// duration the gas holds its background twice.  The Planck matrix stays (the sums and the fit read it, and the views); its
// blocked copy is shared through the context's table by the gases that share the matrix.  ECCKD_RT_ROWMAJOR (read here, when
// the gas is made): no blocked operands, the row-major sweep - A/B knob and fallback.  Where the column-staged preparation
// kernel has written the blocked operands itself (sweep_layout::prep_writes_blocked) there is nothing left to do here.
static void gas_reblock(ecckd_gas* g, unsigned rows, const void* src, void* dst) {
  hipLaunchKernelGGL(k_reblock<true>, dim3((unsigned)(((size_t)rows * g->n + 255) / 256)), dim3(256), 0, g->ctx->stream, rows, g->n,
                     (const unsigned long long*)src, (unsigned long long*)dst);
}

// g->planck_blk: the blocked copy that the context's table holds of a reused matrix, or a new one, registered.  A new one is
// filled here from g->planck_hl unless the preparation kernel is about to write it (prep_fills: only a matrix the gas
// evaluates itself).
static int gas_planck_blocked(ecckd_gas* g, bool planck_reused, bool prep_fills) {
  namespace sl = ecckd::sweep_layout;
  ecckd_ctx* ctx = g->ctx;
  double* shared = planck_reused ? planck_blk_attach(ctx, g->planck_hl) : nullptr;
  if (shared) { g->planck_blk = shared; return ECCKD_OK; }
  void* mine = nullptr;
  ECCKD_HIP_CHECK(ecckd::dev_malloc(ctx, &mine, (size_t)sl::bytes((unsigned)g->nlay + 1, g->n)));
  planck_blk_register(ctx, planck_reused ? nullptr : g->planck_hl, mine);      // from here on gas_free lets go of it
  g->planck_blk = (double*)mine;
  if (planck_reused || !prep_fills) {
    gas_reblock(g, (unsigned)g->nlay + 1, g->planck_hl, mine);
    ECCKD_HIP_CHECK(hipGetLastError());
  }
  return ECCKD_OK;
}

static int gas_block_operands(ecckd_gas* g, bool planck_reused) {
  namespace sl = ecckd::sweep_layout;
  ecckd_ctx* ctx = g->ctx;
  const size_t n = g->n;
  const unsigned nlay = (unsigned)g->nlay;
  if (g->bg_blk) return ECCKD_OK;           // the preparation has written them blocked (ecckd_gas_create_lw)
  if (!sl::gas_can_block(g->nlay, g->chunks_from_line, std::getenv("ECCKD_RT_ROWMAJOR") != nullptr, n)) return ECCKD_OK;
  if (!sl::on_line(g->planck_hl) || !sl::on_line(g->bg_od) || !sl::on_line(g->bg_pair)) return ECCKD_OK;
  ECCKD_CHECK(gas_planck_blocked(g, planck_reused, false));
  const bool pairs = g->bg_pair != nullptr;
  const unsigned bg_rows = pairs ? nlay / 2 : nlay;
  void* blocked = nullptr;
  ECCKD_HIP_CHECK(g->alloc(&blocked, (size_t)sl::bytes(bg_rows, n)));
  gas_reblock(g, bg_rows, pairs ? (const void*)g->bg_pair : (const void*)g->bg_od, blocked);
  ECCKD_HIP_CHECK(hipGetLastError());
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  g->bg_blk = blocked;
  g->bg_blk_pairs = pairs;
  g->give_back(g->bg_pair);
  g->give_back(g->bg_od);
  return ECCKD_OK;
}

// ---------------------------------------------------------------------------
// The steps of gas construction that the longwave and the shortwave gas share.

// Temporaries of the column-staged preparation (54 layers of FLOAT optical depths).  Whatever is still held when the
// constructor returns (error paths included) goes back to the context's cache once the stream has drained.
struct Temps {
  ecckd_ctx* ctx;
  void *od_col = nullptr, *bg_col = nullptr;   // the columns of the target and the background, in rank order (scatter_columns)
  void* wave_part = nullptr;                   // per-wave row sums left by K4, combined into the tile sums (gas_sum_rows)
  void* bg_scale = nullptr;                    // the factors [nsrc][nlay] of a background that the scatter merges
  void drop(void*& q) {                        // the caller has synchronised the stream
    if (q) ecckd::dev_release(ctx, q);
    q = nullptr;
  }
  void drop_all() { drop(od_col); drop(bg_col); drop(wave_part); drop(bg_scale); }
  ~Temps() {
    if (!od_col && !bg_col && !wave_part && !bg_scale) return;
    (void)hipStreamSynchronize(ctx->stream);
    drop_all();
  }
};

// `who`: the entry point's name in front of every message.  arrays: none of the entry point's mandatory arrays is NULL.
// h_temperature_hl: NULL in the shortwave.
static int gas_check_args(const char* who, ecckd_ctx* ctx, ecckd_gas** out, int nlay, size_t nwav, bool arrays, int od_type,
                          bool has_bg, int bg_type, size_t src_stride, int averaging_method, int last_method,
                          const double* h_pressure_hl, const double* h_temperature_hl) {
  ECCKD_REQUIRE(ctx && out, "%s: NULL ctx/out", who);
  *out = nullptr;
  ECCKD_REQUIRE(nlay > 0 && nwav > 0, "%s: empty problem (nlay=%d, nwav=%zu)", who, nlay, nwav);
  ECCKD_REQUIRE(nwav < (size_t)0x7fffffff, "%s: nwav exceeds int32 rank range", who);
  ECCKD_REQUIRE(arrays, "%s: NULL array argument", who);
  ECCKD_REQUIRE(od_type == ECCKD_F32 || od_type == ECCKD_F64, "%s: od_type must be 4 or 8", who);
  ECCKD_REQUIRE(!has_bg || bg_type == ECCKD_F32 || bg_type == ECCKD_F64, "%s: bg_type must be 4 or 8", who);
  ECCKD_REQUIRE(src_stride >= nwav, "%s: src_stride < nwav", who);
  // find_g_points.cpp:1146-1149: unknown averaging method is a PARAMETER_ERROR
  ECCKD_REQUIRE(averaging_method >= ECCKD_AVG_LINEAR && averaging_method <= last_method,
                "Averaging method %d not understood", averaging_method);
  for (int i = 0; i <= nlay; ++i)
    ECCKD_REQUIRE(h_pressure_hl[i] > 0.0 && (!h_temperature_hl || h_temperature_hl[i] > 0.0) &&
                      (i == 0 || h_pressure_hl[i] > h_pressure_hl[i - 1]),
                  "%s: pressure_hl must be positive and increasing%s", who, h_temperature_hl ? ", temperature_hl positive" : "");
  return ECCKD_OK;
}

static GasPtr gas_new(ecckd_ctx* ctx, int do_sw, int averaging_method, int nlay, size_t nwav, double flux_weight,
                      const double* h_pressure_hl) {
  GasPtr g(new ecckd_gas());
  g->ctx = ctx;
  g->do_sw = do_sw;
  g->method = averaging_method;
  g->nlay = nlay;
  g->n = nwav;
  g->flux_weight = flux_weight;
  g->h_pressure_hl.assign(h_pressure_hl, h_pressure_hl + nlay + 1);
  return g;
}

// Per-level constants on the device, g->lev: hk[nhl] (longwave: h/k over the temperature; shortwave: unused) | conv[nlay] |
// layer_weight[nlay] | two int flags, zero.  Returns once they are there.
static int gas_layer_constants(ecckd_gas* g, const double* h_temperature_hl, double min_pressure) {
  const int nlay = g->nlay;
  const size_t nhl = nlay + 1;
  const std::vector<double>& p = g->h_pressure_hl;
  std::vector<double> lev(nhl + 2 * nlay + 1, 0.0);
  if (h_temperature_hl)
    for (size_t i = 0; i < nhl; ++i) lev[i] = ecckd::kPlanckOverBoltzmann / h_temperature_hl[i];
  g->h_layer_weight.resize(nlay);
  // find_g_points.cpp:1093-1099
  double s = 0.0;
  for (int l = 0; l < nlay; ++l) {
    lev[nhl + l] = -(ECCKD_ACCEL_GRAVITY / ECCKD_SPECIFIC_HEAT_AIR) / (p[l + 1] - p[l]);
    double lw = std::sqrt(p[l + 1]) - std::sqrt(p[l]);
    double pfl = 0.5 * (p[l + 1] + p[l]);
    if (pfl < min_pressure) lw = 0.0;
    g->h_layer_weight[l] = lw;
  }
  for (int l = 0; l < nlay; ++l) s += g->h_layer_weight[l];
  for (int l = 0; l < nlay; ++l) {
    g->h_layer_weight[l] /= s;
    lev[nhl + nlay + l] = g->h_layer_weight[l];
  }
  ECCKD_HIP_CHECK(g->alloc(&g->lev, lev.size() * sizeof(double)));
  ECCKD_HIP_CHECK(hipMemcpyAsync(g->lev, lev.data(), lev.size() * sizeof(double), hipMemcpyHostToDevice, g->ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(g->ctx->stream));
  return ECCKD_OK;
}

// d_ireorder = the inverse of d_rank, which must be a permutation: every slot of ireorder written exactly once.  Checked on
// the device BEFORE anything dereferences ireorder.  d_flag: an int on the device that the stream has zeroed.
static int invert_rank(ecckd_ctx* ctx, const char* who, size_t nwav, const int32_t* d_rank, int32_t* d_ireorder, int* d_flag) {
  const unsigned eblocks = (unsigned)((nwav + 255) / 256);
  ECCKD_HIP_CHECK(hipMemsetAsync(d_ireorder, 0xFF, nwav * sizeof(int32_t), ctx->stream));
  hipLaunchKernelGGL(k_invert_rank, dim3(eblocks), dim3(256), 0, ctx->stream, nwav, d_rank, d_ireorder, d_flag);
  hipLaunchKernelGGL(k_check_perm, dim3(eblocks), dim3(256), 0, ctx->stream, nwav, d_ireorder, d_flag);
  int flag = 0;
  ECCKD_HIP_CHECK(hipMemcpyAsync(&flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  ECCKD_REQUIRE(flag == 0, "%s: rank is not a permutation of 0..nwav-1", who);
  return ECCKD_OK;
}

// The 54-layer columns of the FLOAT target spectrum and of the background (if any) scattered into rank order, in PARTS runs
// of 54 / PARTS layers, [PARTS][ncol][54 / PARTS] with ncol = nwav rounded up to 64: K4 stages them through LDS.
// The background: the matrix d_bg_od, or (then d_bg_od is NULL) the nsrc spectra of `merged` with the factors
// h_bg_scale[nsrc][54], merged as they are scattered: DOUBLE columns, and no merged matrix anywhere.
template <int PARTS>
static int scatter_columns(Temps& temps, size_t nwav, size_t src_stride, const int32_t* d_rank, const void* d_od,
                           const void* d_bg_od, bool bg32, const BgSources* merged = nullptr, int nsrc = 0,
                           const double* h_bg_scale = nullptr) {
  ecckd_ctx* ctx = temps.ctx;
  const unsigned tblocks = (unsigned)((nwav + 63) / 64);
  const size_t ncol = (size_t)tblocks * 64;
  ECCKD_HIP_CHECK(ecckd::dev_malloc(ctx, &temps.od_col, ncol * 54 * sizeof(float)));
  if (d_bg_od || merged) ECCKD_HIP_CHECK(ecckd::dev_malloc(ctx, &temps.bg_col, ncol * 54 * (bg32 ? sizeof(float) : sizeof(double))));
  hipLaunchKernelGGL((k_scatter_column_halves<54, float, PARTS>), dim3(tblocks), dim3(256), 0, ctx->stream, nwav, ncol, src_stride,
                     d_rank, (const float*)d_od, (float*)temps.od_col);
  if (merged) {
    // the factors go to the device once per gas; the caller's table is pageable: the constructor waits for the stream
    // before it returns
    const size_t scale_bytes = (size_t)nsrc * 54 * sizeof(double);
    ECCKD_HIP_CHECK(ecckd::dev_malloc(ctx, &temps.bg_scale, scale_bytes));
    ECCKD_HIP_CHECK(hipMemcpyAsync(temps.bg_scale, h_bg_scale, scale_bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL((k_scatter_merged_halves<54, PARTS>), dim3(tblocks), dim3(256), 0, ctx->stream, nwav, ncol, d_rank, *merged,
                       nsrc, (const double*)temps.bg_scale, (double*)temps.bg_col);
  } else if (d_bg_od && bg32)
    hipLaunchKernelGGL((k_scatter_column_halves<54, float, PARTS>), dim3(tblocks), dim3(256), 0, ctx->stream, nwav, ncol, src_stride,
                       d_rank, (const float*)d_bg_od, (float*)temps.bg_col);
  else if (d_bg_od)
    hipLaunchKernelGGL((k_scatter_column_halves<54, double, PARTS>), dim3(tblocks), dim3(256), 0, ctx->stream, nwav, ncol, src_stride,
                       d_rank, (const double*)d_bg_od, (double*)temps.bg_col);
  return ECCKD_OK;
}

// Which summable rows a gas has, in the order of RowMap's members.
static RowMap make_row_map(int nlay, bool is_log, bool is_tt) {
  RowMap R;
  int next = 0;
  R.A = next; next += nlay;
  R.B = next; next += nlay;
  if (is_log) { R.N = next; next += nlay; }
  R.H = next; next += nlay;
  R.FDS = next++;
  R.FUT = next++;
  if (is_tt) {
    R.TF = next; next += nlay;
    R.TG = next; next += nlay;
    R.HL = next; next += nlay;
    R.HH = next; next += nlay;
    R.FDSL = next++; R.FUTL = next++; R.FDSH = next++; R.FUTH = next++;
  }
  R.total = next;
  return R;
}

// The rows of g->rm -> device table -> tile sums -> super sums.  denom + l * denom_stride: the denominator of the fit of
// layer l where the method is not the logarithmic one.  The tile sums come from the per-wave sums that the column-staged
// preparation left in temps.wave_part, if any.  sync: wait for the tile sums and give every temporary back.
static int gas_sum_rows(ecckd_gas* g, const double* denom, size_t denom_stride, Temps& temps, bool sync) {
  ecckd_ctx* ctx = g->ctx;
  const RowMap& R = g->rm;
  const size_t nwav = g->n;
  std::vector<const double*> rows(g->nrows);
  for (int l = 0; l < g->nlay; ++l) {
    rows[R.A + l] = g->w1 + (size_t)l * nwav;
    rows[R.B + l] = R.N >= 0 ? g->w2 + (size_t)l * nwav : denom + (size_t)l * denom_stride;
    if (R.N >= 0) rows[R.N + l] = g->cnt + (size_t)l * nwav;
    rows[R.H + l] = g->hr + (size_t)l * nwav;
    if (R.TF >= 0) {
      rows[R.TF + l] = g->tf + (size_t)l * nwav;
      rows[R.TG + l] = g->tg + (size_t)l * nwav;
      rows[R.HL + l] = g->hr_low + (size_t)l * nwav;
      rows[R.HH + l] = g->hr_high + (size_t)l * nwav;
    }
  }
  rows[R.FDS] = g->fds;
  rows[R.FUT] = g->fut;
  if (R.TF >= 0) {
    rows[R.FDSL] = g->fx;
    rows[R.FUTL] = g->fx + nwav;
    rows[R.FDSH] = g->fx + 2 * nwav;
    rows[R.FUTH] = g->fx + 3 * nwav;
  }
  ECCKD_HIP_CHECK(g->alloc(&g->rows, rows.size() * sizeof(double*)));
  ECCKD_HIP_CHECK(hipMemcpyAsync((void*)g->rows, rows.data(), rows.size() * sizeof(double*), hipMemcpyHostToDevice, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  g->ntiles = (nwav + TILE - 1) / TILE;
  ECCKD_HIP_CHECK(g->alloc(&g->tile_sums, (size_t)g->nrows * g->ntiles * sizeof(double)));
  if (temps.wave_part) {
    static_assert(TILE == 256, "a tile is four 64-point groups");
    hipLaunchKernelGGL(k_combine_wave_sums, dim3((unsigned)((g->ntiles + 255) / 256), (unsigned)g->nrows), dim3(256), 0, ctx->stream,
                       g->nrows, (nwav + 63) / 64, g->ntiles, (const double*)temps.wave_part, g->tile_sums);
  } else {
    hipLaunchKernelGGL(k_tile_sums, dim3((unsigned)g->ntiles), dim3(TILE), 0, ctx->stream, g->nrows, nwav, g->ntiles,
                       (const double* const*)g->rows, g->tile_sums);
  }
  ECCKD_HIP_CHECK(hipGetLastError());
  if (sync) {
    ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    temps.drop_all();
  }
  g->nsuper = (g->ntiles + SUPER - 1) / SUPER;
  ECCKD_HIP_CHECK(g->alloc(&g->super_sums, (size_t)g->nrows * g->nsuper * sizeof(double)));
  hipLaunchKernelGGL(k_super_sums, dim3((unsigned)g->nsuper, (unsigned)g->nrows), dim3(256), 0, ctx->stream, g->ntiles, g->nsuper,
                     (const double*)g->tile_sums, g->super_sums);
  ECCKD_HIP_CHECK(hipGetLastError());
  return ECCKD_OK;
}

// ---------------------------------------------------------------------------
// What the entry points that take interval bounds share.

// The interval [b1, b2] (fractions) of the band of npoints points that starts at sorted index ibegin: index mapping and
// error paths of CkdEquipartition::calc_error (find_g_points.cpp:282-320).  The chunking is the sweep's to fill in.
static int make_interval(const ecckd_gas* g, size_t ibegin, size_t npoints, double b1, double b2, double albedo, Interval& iv) {
  ECCKD_REQUIRE(npoints > 0 && ibegin + npoints <= g->n,
                "ecckd_calc_error_batch: band [%zu,%zu) outside the spectrum (%zu points)", ibegin, ibegin + npoints, g->n);
  long long i1 = (long long)std::ceil(b1 * (double)(npoints - 1));
  long long i2 = (long long)std::floor(b2 * (double)(npoints - 1));
  if (i1 < 0 || i2 >= (long long)npoints || !(b1 == b1) || !(b2 == b2))
    return ecckd::fail(ECCKD_PROCESSING_ERROR,
                       "requested bounds %.17g-%.17g corresponding to indices %lld-%lld outside valid range 0-%zu",
                       b1, b2, i1, i2, npoints - 1);
  if (b2 < b1) return ecckd::fail(ECCKD_PROCESSING_ERROR, "requested bounds out of order: %.17g-%.17g", b1, b2);
  if (i2 + 1 < i1) return ecckd::fail(ECCKD_PROCESSING_ERROR, "requested indices out of order: %lld-%lld", i1, i2);
  if (i2 < i1) i2 = i1;
  iv.i1 = (long long)ibegin + i1;
  iv.i2 = (long long)ibegin + i2;
  iv.chunk0 = 0;
  iv.head = 0;
  iv.chunk_pts = 0;
  iv.npoints = (long long)npoints;
  iv.albedo = albedo;
  return ECCKD_OK;
}

// what an interval's error depends on (gas.hpp); the longwave knows no albedo
static IntervalKey interval_key(const ecckd_gas* g, const Interval& iv) {
  IntervalKey key;
  key.i1 = iv.i1;
  key.i2 = iv.i2;
  key.albedo_bits = 0;
  if (g->do_sw) std::memcpy(&key.albedo_bits, &iv.albedo, sizeof(double));
  return key;
}

// The device work buffer of a batch of n intervals: intervals | sums[n][nrows] | od_fit[2][n][nlay] |
// partial[2][nchunks][2 nhl] (x2: both fits of the dual shortwave sweep).  The pinned buffer starts with the intervals too.
struct WorkLayout {
  size_t iv_bytes, sums_bytes, fit_bytes, part_bytes;
  WorkLayout(int n, int nrows, int nlay, long long nchunks)
      : iv_bytes(ecckd_align_up((size_t)n * sizeof(Interval), 256)),
        sums_bytes(ecckd_align_up((size_t)n * nrows * sizeof(double), 256)),
        fit_bytes(ecckd_align_up((size_t)2 * n * nlay * sizeof(double), 256)),
        part_bytes(ecckd_align_up((size_t)2 * nchunks * 2 * (nlay + 1) * sizeof(double), 256)) {}
  size_t dev_bytes() const { return iv_bytes + sums_bytes + fit_bytes + part_bytes; }
  Interval* iv(void* work) const { return (Interval*)work; }
  double* sums(void* work) const { return (double*)((char*)work + iv_bytes); }
  double* fit(void* work) const { return (double*)((char*)work + iv_bytes + sums_bytes); }
  double* part(void* work) const { return (double*)((char*)work + iv_bytes + sums_bytes + fit_bytes); }
};

// The column-staged preparation runs: 54 layers, FLOAT target spectrum (as stored in the CKDMIP files), FLOAT or DOUBLE
// (merged) background, with or without the Planck matrix of an earlier gas, no log metric.
static bool lw_fast_path(int nlay, int od_type, int averaging_method) {
  return nlay == 54 && od_type == ECCKD_F32 && averaging_method != ECCKD_AVG_LOGARITHMIC;
}

// The body of the longwave constructors.  The background is the matrix d_bg_od (or none: NULL), or, on the column-staged
// path only (lw_fast_path), the nsrc spectra of `merged` with the factors h_bg_scale[nsrc][nlay], which the scatter merges:
// the gas is the one the DOUBLE matrix of their sum would give.  The arguments are checked.
static int gas_create_lw(const char* who, ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_pressure_hl,
                         const double* h_temperature_hl, const double* d_wavenumber, const double* d_d_wavenumber,
                         const int32_t* d_rank, const void* d_bg_od, int bg_type, const BgSources* merged, int nsrc,
                         const double* h_bg_scale, const void* d_od, int od_type, size_t src_stride, int averaging_method,
                         double flux_weight, double min_pressure, const double* d_planck_hl_reuse, ecckd_gas** out) {
  namespace sl = ecckd::sweep_layout;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  if ((size_t)nlay * 64 * sizeof(double) > 160 * 1024)
    return ecckd::fail(ECCKD_PARAMETER_ERROR, "%s: nlay = %d exceeds the supported maximum (320)", who, nlay);

  GasPtr gas = gas_new(ctx, 0, averaging_method, nlay, nwav, flux_weight, h_pressure_hl);
  ecckd_gas* const g = gas.get();
  const bool is_log = averaging_method == ECCKD_AVG_LOGARITHMIC;
  const size_t nhl = nlay + 1;
  const size_t mat = (size_t)nlay * nwav * sizeof(double);
  g->chunks_from_line = std::getenv("ECCKD_RT_UNALIGNED") == nullptr;
  if (d_planck_hl_reuse) g->planck_hl = const_cast<double*>(d_planck_hl_reuse);   // not recorded: its owner frees it
  else ECCKD_HIP_CHECK(g->alloc(&g->planck_hl, nhl * nwav * sizeof(double)));
  // The background rows.  FLOAT pairs for the sweep (k_rt_lw_bb_mirror<.., true>) whenever every value is a float: with a
  // FLOAT background (or none) on the 54-layer path K4 writes them itself INSTEAD of the DOUBLE rows (which are then made on
  // demand only, gas_bg_rows: 3.1 GB less to write and to hold per gas at 7.2e6 points); otherwise the DOUBLE rows are
  // written and k_pack_bg32 tries to pack them below.  ECCKD_BG64: DOUBLE rows only.
  const bool has_bg = d_bg_od || merged;
  const bool bg32 = d_bg_od && bg_type == ECCKD_F32;
  const bool fast = lw_fast_path(nlay, od_type, averaging_method);
  const bool bg64_knob = std::getenv("ECCKD_BG64") != nullptr;
  const bool want_pairs = (nlay == 54 || nlay == 30) && !bg64_knob;
  const bool pairs_in_k4 = want_pairs && fast && (!has_bg || bg32);
  // Where the gas will hold its sweep operands line-blocked (gas_block_operands) and K4's column-staged kernel runs, K4
  // writes them blocked itself - the background blocked ONLY, FLOAT pairs or DOUBLE rows as above, and the Planck matrix it
  // evaluates in both layouts - and tests a DOUBLE background for values that are no floats on the way: no row-major
  // background, no k_pack_bg32 and no k_reblock pass.
  bool prep_blocks = sl::prep_writes_blocked(nlay, od_type == ECCKD_F32, is_log, bg64_knob, g->chunks_from_line,
                                             std::getenv("ECCKD_RT_ROWMAJOR") != nullptr, nwav) && sl::on_line(g->planck_hl);
  if (prep_blocks) {
    ECCKD_HIP_CHECK(g->alloc(&g->bg_blk, (size_t)sl::bytes(pairs_in_k4 ? nlay / 2 : nlay, nwav)));
    if (!sl::on_line(g->bg_blk)) { g->give_back(g->bg_blk); prep_blocks = false; }
  }
  if (prep_blocks) {
    g->bg_blk_pairs = pairs_in_k4;
    ECCKD_CHECK(gas_planck_blocked(g, d_planck_hl_reuse != nullptr, true));
  } else {
    if (want_pairs) ECCKD_HIP_CHECK(g->alloc(&g->bg_pair, (size_t)(nlay / 2) * nwav * 2 * sizeof(float)));
    if (!pairs_in_k4) ECCKD_HIP_CHECK(g->alloc(&g->bg_od, mat));
  }
  ECCKD_HIP_CHECK(g->alloc(&g->w1, mat));
  if (is_log) {
    ECCKD_HIP_CHECK(g->alloc(&g->w2, mat));
    ECCKD_HIP_CHECK(g->alloc(&g->cnt, mat));
  }
  ECCKD_HIP_CHECK(g->alloc(&g->hr, mat));
  ECCKD_HIP_CHECK(g->alloc(&g->fds, nwav * sizeof(double)));
  ECCKD_HIP_CHECK(g->alloc(&g->fut, nwav * sizeof(double)));
  ECCKD_HIP_CHECK(g->alloc(&g->wn_sorted, nwav * sizeof(double)));
  ECCKD_HIP_CHECK(g->alloc(&g->dwn_sorted, nwav * sizeof(double)));
  ECCKD_HIP_CHECK(g->alloc(&g->ireorder, nwav * sizeof(int32_t)));
  ECCKD_CHECK(gas_layer_constants(g, h_temperature_hl, min_pressure));
  const double* hkd = g->lev;
  const double* convd = g->lev + nhl;
  int* d_flag = (int*)(g->lev + nhl + 2 * nlay);
  ECCKD_CHECK(invert_rank(ctx, who, nwav, d_rank, g->ireorder, d_flag));

  int threads = PREP_THREADS;
  while ((size_t)nlay * threads * sizeof(double) > 160 * 1024 && threads > 64) threads /= 2;
  const size_t lds = (size_t)nlay * threads * sizeof(double);
  const unsigned pblocks = (unsigned)((nwav + threads - 1) / threads);
#define LAUNCH_PREP(BG, OD)                                                                                   \
  do {                                                                                                        \
    ECCKD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_gas_prep_lw<BG, OD>),                 \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));             \
    hipLaunchKernelGGL((k_gas_prep_lw<BG, OD>), dim3(pblocks), dim3(threads), lds, ctx->stream, nlay, nwav,   \
                       src_stride, averaging_method, g->ireorder, hkd, convd, d_wavenumber, d_d_wavenumber,   \
                       (const BG*)d_bg_od, (const OD*)d_od, d_planck_hl_reuse, g->wn_sorted, g->dwn_sorted,   \
                       g->planck_hl, g->bg_od, g->w1, g->w2, g->cnt, g->hr, g->fds, g->fut);                  \
  } while (0)
  Temps temps{ctx};
  if (fast) {
    // the columns in two runs of 27 layers
    ECCKD_CHECK(scatter_columns<2>(temps, nwav, src_stride, d_rank, d_od, d_bg_od, bg32, merged, nsrc, h_bg_scale));
    const size_t nw64 = (nwav + 63) / 64;
    const unsigned fblocks = (unsigned)((nwav + 127) / 128);
    ECCKD_HIP_CHECK(ecckd::dev_malloc(ctx, &temps.wave_part, (size_t)(3 * 54 + 2) * nw64 * sizeof(double)));
#define LAUNCH_MIRROR(BG, REUSE, BLK)                                                                                         \
  hipLaunchKernelGGL((k_gas_prep_lw_mirror<54, BG, float, REUSE, BLK>), dim3(fblocks), dim3(PREP_THREADS), 0, ctx->stream,     \
                     nwav, averaging_method, g->ireorder, hkd, convd, d_wavenumber, d_d_wavenumber, (const BG*)temps.bg_col,   \
                     (const float*)temps.od_col, d_planck_hl_reuse, g->wn_sorted, g->dwn_sorted, g->planck_hl, g->bg_od,       \
                     g->w1, g->hr, g->fds, g->fut, (double*)temps.wave_part, nw64,                                             \
                     pairs_in_k4 && !(BLK) ? (float_x2_store*)g->bg_pair : nullptr, (BLK) ? g->bg_blk : nullptr,               \
                     (BLK) ? g->planck_blk : nullptr, (BLK) ? d_flag + 1 : nullptr)
#define LAUNCH_MIRROR_BG(BG)                                                                   \
  do {                                                                                         \
    if (d_planck_hl_reuse) { if (prep_blocks) LAUNCH_MIRROR(BG, true, true); else LAUNCH_MIRROR(BG, true, false); }   \
    else { if (prep_blocks) LAUNCH_MIRROR(BG, false, true); else LAUNCH_MIRROR(BG, false, false); }                   \
  } while (0)
    if (bg32 || !has_bg) LAUNCH_MIRROR_BG(float);
    else LAUNCH_MIRROR_BG(double);
#undef LAUNCH_MIRROR_BG
#undef LAUNCH_MIRROR
    ECCKD_HIP_CHECK(hipGetLastError());
    ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    temps.drop(temps.od_col);
    temps.drop(temps.bg_col);
  } else if (bg32 && od_type == ECCKD_F32) LAUNCH_PREP(float, float);
  else if (bg32) LAUNCH_PREP(float, double);
  else if (od_type == ECCKD_F32) LAUNCH_PREP(double, float);
  else LAUNCH_PREP(double, double);
#undef LAUNCH_PREP
  ECCKD_HIP_CHECK(hipGetLastError());

  g->rm = make_row_map(nlay, is_log, false);
  g->nrows = g->rm.total;
  // denominator of the fit: planck_hl(l+1) (find_g_points.cpp:62), or for the logarithmic method planck_hl(l) masked by
  // metric > 0 (:87), which K4 has left in w2.  The per-wave sums go back as soon as they are combined.
  ECCKD_CHECK(gas_sum_rows(g, g->planck_hl + nwav, nwav, temps, temps.wave_part != nullptr));
  // FLOAT pairs from the DOUBLE rows where K4 has not written them itself: kept if every value is a float
  if (want_pairs && !pairs_in_k4 && !prep_blocks) {
    hipLaunchKernelGGL(k_pack_bg32, dim3((unsigned)((nwav + 255) / 256)), dim3(256), 0, ctx->stream, nlay / 2, nwav,
                       (const double*)g->bg_od, (float_x2_store*)g->bg_pair, d_flag + 1);
    ECCKD_HIP_CHECK(hipGetLastError());
  }
  int not_float = 0;
  ECCKD_HIP_CHECK(hipMemcpyAsync(&not_float, d_flag + 1, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  if (want_pairs && !pairs_in_k4 && not_float) g->give_back(g->bg_pair);   // a DOUBLE background with values between the floats: the DOUBLE rows serve
  if (prep_blocks && !pairs_in_k4 && !not_float) {
    // K4 met floats only in the blocked DOUBLE rows (rare: say a single unscaled FLOAT spectrum handed over as DOUBLE): the
    // gas ends where k_pack_bg32 would have left it, with the blocked FLOAT pairs
    float_x2_store* pairs = nullptr;
    ECCKD_HIP_CHECK(g->alloc(&pairs, (size_t)sl::bytes(nlay / 2, nwav)));
    hipLaunchKernelGGL(k_pack_bg32_blocked, dim3((unsigned)((nwav + 255) / 256)), dim3(256), 0, ctx->stream, nlay / 2, nwav,
                       (const double*)g->bg_blk, pairs);
    ECCKD_HIP_CHECK(hipGetLastError());
    ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    g->give_back(g->bg_blk);
    g->bg_blk = pairs;
    g->bg_blk_pairs = true;
  }
  ECCKD_CHECK(gas_block_operands(g, d_planck_hl_reuse != nullptr));
  *out = gas.release();
  return ECCKD_OK;
}

// What ecckd_gas_create_lw_merged checks of its list of background spectra, in the words of gas_check_args.
static int check_bg_sources(const char* who, int nbg, const void* const* d_bg_od, const int* bg_type, const size_t* bg_stride,
                            const double* h_bg_scale, size_t nwav, BgSources& src) {
  ECCKD_REQUIRE(nbg >= 0 && nbg <= BG_MAX_SOURCES, "%s: nbg (%d) must be between 0 and %d", who, nbg, BG_MAX_SOURCES);
  ECCKD_REQUIRE(nbg == 0 || (d_bg_od && bg_type && bg_stride && h_bg_scale), "%s: NULL array argument", who);
  for (int s = 0; s < BG_MAX_SOURCES; ++s) { src.od[s] = nullptr; src.stride[s] = 0; src.type[s] = ECCKD_F64; }
  for (int s = 0; s < nbg; ++s) {
    ECCKD_REQUIRE(d_bg_od[s], "%s: d_bg_od[%d] is NULL", who, s);
    ECCKD_REQUIRE(bg_type[s] == ECCKD_F32 || bg_type[s] == ECCKD_F64, "%s: bg_type[%d] must be 4 or 8", who, s);
    ECCKD_REQUIRE(bg_stride[s] >= nwav, "%s: bg_stride[%d] (%zu) < nwav (%zu)", who, s, bg_stride[s], nwav);
    src.od[s] = d_bg_od[s]; src.stride[s] = bg_stride[s]; src.type[s] = bg_type[s];
  }
  return ECCKD_OK;
}

}  // namespace

extern "C" {

int ecckd_gas_create_lw(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_pressure_hl,
                        const double* h_temperature_hl, const double* d_wavenumber,
                        const double* d_d_wavenumber, const int32_t* d_rank, const void* d_bg_od,
                        int bg_type, const void* d_od, int od_type, size_t src_stride,
                        int averaging_method, double flux_weight, double min_pressure,
                        const double* d_planck_hl_reuse, ecckd_gas** out) {
  static const char who[] = "ecckd_gas_create_lw";
  // total-transmission is shortwave-only (fit_optical_depth_lw has no such branch, find_g_points.cpp:101-104)
  ECCKD_CHECK(gas_check_args(who, ctx, out, nlay, nwav,
                             h_pressure_hl && h_temperature_hl && d_wavenumber && d_d_wavenumber && d_rank && d_od, od_type,
                             d_bg_od != nullptr, bg_type, src_stride, averaging_method, ECCKD_AVG_LOGARITHMIC, h_pressure_hl,
                             h_temperature_hl));
  return gas_create_lw(who, ctx, nlay, nwav, h_pressure_hl, h_temperature_hl, d_wavenumber, d_d_wavenumber, d_rank, d_bg_od,
                       bg_type, nullptr, 0, nullptr, d_od, od_type, src_stride, averaging_method, flux_weight, min_pressure,
                       d_planck_hl_reuse, out);
}

int ecckd_gas_create_lw_merged(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_pressure_hl,
                               const double* h_temperature_hl, const double* d_wavenumber,
                               const double* d_d_wavenumber, const int32_t* d_rank, int nbg,
                               const void* const* d_bg_od, const int* bg_type, const size_t* bg_stride,
                               const double* h_bg_scale, const void* d_od, int od_type, size_t src_stride,
                               int averaging_method, double flux_weight, double min_pressure,
                               const double* d_planck_hl_reuse, ecckd_gas** out) {
  static const char who[] = "ecckd_gas_create_lw_merged";
  ECCKD_CHECK(gas_check_args(who, ctx, out, nlay, nwav,
                             h_pressure_hl && h_temperature_hl && d_wavenumber && d_d_wavenumber && d_rank && d_od, od_type,
                             false, 0, src_stride, averaging_method, ECCKD_AVG_LOGARITHMIC, h_pressure_hl, h_temperature_hl));
  BgSources src;
  ECCKD_CHECK(check_bg_sources(who, nbg, d_bg_od, bg_type, bg_stride, h_bg_scale, nwav, src));
  const auto create = [&](const void* d_bg, const BgSources* merged) {
    return gas_create_lw(who, ctx, nlay, nwav, h_pressure_hl, h_temperature_hl, d_wavenumber, d_d_wavenumber, d_rank, d_bg,
                         ECCKD_F64, merged, nbg, h_bg_scale, d_od, od_type, src_stride, averaging_method, flux_weight,
                         min_pressure, d_planck_hl_reuse, out);
  };
  if (nbg == 0) return create(nullptr, nullptr);
  if (lw_fast_path(nlay, od_type, averaging_method)) return create(nullptr, &src);
  // off the column-staged path: the merged matrix in a temporary (the one-pass merge), the constructor, the temporary back
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  void* d_merged = nullptr;
  ECCKD_HIP_CHECK(ecckd::dev_malloc(ctx, &d_merged, (size_t)nlay * src_stride * sizeof(double)));
  int rc = ecckd_merge_scenario_dev(ctx, nlay, nwav, nbg, d_bg_od, bg_type, bg_stride, h_bg_scale, (double*)d_merged, src_stride);
  if (rc == ECCKD_OK) rc = create(d_merged, nullptr);
  (void)hipStreamSynchronize(ctx->stream);
  ecckd::dev_release(ctx, d_merged);
  return rc;
}


// planck_hl[nlay+1][nwav] in the order given by d_rank, bit-identical to the matrix ecckd_gas_create_lw builds for a gas
// with that ordering and temperature profile (planck_function.cpp:22-54 on the reordered grid, find_g_points.cpp:970-979).
int ecckd_planck_hl_sorted_dev(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_temperature_hl,
                               const double* d_wavenumber, const double* d_d_wavenumber, const int32_t* d_rank,
                               double* d_planck_hl) {
  ECCKD_REQUIRE(ctx && h_temperature_hl && d_wavenumber && d_d_wavenumber && d_rank && d_planck_hl,
                "ecckd_planck_hl_sorted_dev: NULL argument");
  ECCKD_REQUIRE(nlay > 0 && nwav > 0 && nwav < (size_t)0x7fffffff, "ecckd_planck_hl_sorted_dev: bad size (nlay=%d, nwav=%zu)", nlay, nwav);
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int nhl = nlay + 1;
  std::vector<double> hk;
  ECCKD_CHECK(ecckd::make_hk("ecckd_planck_hl_sorted_dev", nhl, h_temperature_hl, hk));
  const size_t hk_bytes = ecckd_align_up(nhl * sizeof(double), 256), flag_bytes = 256;
  ECCKD_CHECK(ecckd::ensure_scratch(ctx, hk_bytes + flag_bytes + nwav * sizeof(int32_t)));
  double* d_hk = (double*)ctx->scratch;
  int* d_flag = (int*)((char*)ctx->scratch + hk_bytes);
  int32_t* d_ireorder = (int32_t*)((char*)ctx->scratch + hk_bytes + flag_bytes);
  ECCKD_HIP_CHECK(hipMemcpyAsync(d_hk, hk.data(), nhl * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  ECCKD_HIP_CHECK(hipMemsetAsync(d_flag, 0, sizeof(int), ctx->stream));
  ECCKD_CHECK(invert_rank(ctx, "ecckd_planck_hl_sorted_dev", nwav, d_rank, d_ireorder, d_flag));   // its wait also: hk is a local
  hipLaunchKernelGGL(k_planck_sorted, dim3((unsigned)((nwav + 255) / 256)), dim3(256), 0, ctx->stream, nhl, nwav, d_ireorder, d_hk,
                     d_wavenumber, d_d_wavenumber, d_planck_hl);
  ECCKD_HIP_CHECK(hipGetLastError());
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  return ECCKD_OK;
}

// Shortwave gas (find_g_points.cpp do_sw branches of :872-1150).  d_albedo: per-wavenumber
// surface albedo in ORIGINAL order (:921-923), used only for the up-welling of the two scaled
// truth fields of the total-transmission method; NULL = direct beam only (:1027-1034).
// min_scaling / max_scaling are the values AFTER the clamps of :666-667.
int ecckd_gas_create_sw(ecckd_ctx* ctx, int nlay, size_t nwav, const double* h_pressure_hl,
                        const double* d_ssi, const double* d_albedo, const int32_t* d_rank,
                        const void* d_bg_od, int bg_type, const void* d_od, int od_type,
                        size_t src_stride, int averaging_method, double flux_weight,
                        double min_pressure, double cos_sza, double min_scaling, double max_scaling,
                        ecckd_gas** out) {
  static const char who[] = "ecckd_gas_create_sw";
  ECCKD_CHECK(gas_check_args(who, ctx, out, nlay, nwav, h_pressure_hl && d_ssi && d_rank && d_od, od_type, d_bg_od != nullptr,
                             bg_type, src_stride, averaging_method, ECCKD_AVG_TOTAL_TRANSMISSION, h_pressure_hl, nullptr));
  ECCKD_REQUIRE(cos_sza > 0.0, "ecckd_gas_create_sw: cos_sza must be positive");
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));

  GasPtr gas = gas_new(ctx, 1, averaging_method, nlay, nwav, flux_weight, h_pressure_hl);
  ecckd_gas* const g = gas.get();
  g->cos_sza = cos_sza;
  g->min_scaling = min_scaling;
  g->max_scaling = max_scaling;
  const bool is_log = averaging_method == ECCKD_AVG_LOGARITHMIC;
  const bool is_tt = averaging_method == ECCKD_AVG_TOTAL_TRANSMISSION;
  const size_t nhl = nlay + 1;
  const size_t mat = (size_t)nlay * nwav * sizeof(double);
  ECCKD_HIP_CHECK(g->alloc(&g->ssi, nwav * sizeof(double)));
  ECCKD_HIP_CHECK(g->alloc(&g->bg_od, mat));
  ECCKD_HIP_CHECK(g->alloc(&g->w1, mat));
  if (is_log) {
    ECCKD_HIP_CHECK(g->alloc(&g->w2, mat));
    ECCKD_HIP_CHECK(g->alloc(&g->cnt, mat));
  }
  ECCKD_HIP_CHECK(g->alloc(&g->hr, mat));
  ECCKD_HIP_CHECK(g->alloc(&g->fds, nwav * sizeof(double)));
  ECCKD_HIP_CHECK(g->alloc(&g->fut, nwav * sizeof(double)));
  if (is_tt) {
    ECCKD_HIP_CHECK(g->alloc(&g->tf, mat));
    ECCKD_HIP_CHECK(g->alloc(&g->tg, mat));
    ECCKD_HIP_CHECK(g->alloc(&g->hr_low, mat));
    ECCKD_HIP_CHECK(g->alloc(&g->hr_high, mat));
    ECCKD_HIP_CHECK(g->alloc(&g->fx, 4 * nwav * sizeof(double)));
  }
  ECCKD_HIP_CHECK(g->alloc(&g->ireorder, nwav * sizeof(int32_t)));
  ECCKD_CHECK(gas_layer_constants(g, nullptr, min_pressure));
  ECCKD_CHECK(invert_rank(ctx, who, nwav, d_rank, g->ireorder, (int*)(g->lev + nhl + 2 * nlay)));
  const RowMap R = make_row_map(nlay, is_log, is_tt);   // B: rows of ssi (masked by metric > 0 for the logarithmic method)
  g->rm = R;
  g->nrows = R.total;

  const unsigned pblocks = (unsigned)((nwav + PREP_THREADS - 1) / PREP_THREADS);
  const bool bg32 = d_bg_od && bg_type == ECCKD_F32;
  // 54 layers of FLOAT optical depths (the CKDMIP spectra): the columns are scattered into rank order first, staged through
  // LDS by the preparation, and the row sums are taken from registers (ECCKD_SW_PREP_GATHER: the general, gathering kernel)
  const bool cols = nlay == 54 && od_type == ECCKD_F32 && std::getenv("ECCKD_SW_PREP_GATHER") == nullptr;
  Temps temps{ctx};
#define LAUNCH_PREP_SW(BG, OD)                                                                                    \
  hipLaunchKernelGGL((k_gas_prep_sw<BG, OD>), dim3(pblocks), dim3(PREP_THREADS), 0, ctx->stream, nlay, nwav,       \
                     src_stride, averaging_method, cos_sza, min_scaling, max_scaling, g->ireorder,                 \
                     g->lev + nhl, d_ssi, d_albedo, (const BG*)d_bg_od, (const OD*)d_od, g->ssi, g->bg_od,         \
                     g->w1, g->w2, g->cnt, g->hr, g->fds, g->fut, g->tf, g->tg, g->hr_low, g->hr_high, g->fx)
  if (cols) {
    // the columns in runs of 18 layers
    ECCKD_CHECK(scatter_columns<SW_STAGE_PARTS>(temps, nwav, src_stride, d_rank, d_od, d_bg_od, bg32));
    const size_t nw64 = (nwav + 63) / 64, npad = nw64 * 64;
    ECCKD_HIP_CHECK(ecckd::dev_malloc(ctx, &temps.wave_part, (size_t)g->nrows * nw64 * sizeof(double)));
#define LAUNCH_PREP_SW_STAGED(BG)                                                                                                     \
  hipLaunchKernelGGL((k_gas_prep_sw_staged<SW_STAGE_PARTS, BG>), dim3(pblocks), dim3(PREP_THREADS), 0, ctx->stream, nwav, npad,        \
                     averaging_method, cos_sza, min_scaling, max_scaling, g->ireorder, g->lev + nhl, d_ssi, d_albedo,                  \
                     (const BG*)temps.bg_col, (const float*)temps.od_col, g->ssi, g->bg_od, g->w1, g->w2, g->cnt, g->hr, g->fds,       \
                     g->fut, g->tf, g->tg, g->hr_low, g->hr_high, g->fx, R, (double*)temps.wave_part, nw64)
    if (bg32 || !d_bg_od) LAUNCH_PREP_SW_STAGED(float); else LAUNCH_PREP_SW_STAGED(double);
#undef LAUNCH_PREP_SW_STAGED
  }
  else if (bg32 && od_type == ECCKD_F32) LAUNCH_PREP_SW(float, float);
  else if (bg32) LAUNCH_PREP_SW(float, double);
  else if (od_type == ECCKD_F32) LAUNCH_PREP_SW(double, float);
  else LAUNCH_PREP_SW(double, double);
#undef LAUNCH_PREP_SW
  ECCKD_HIP_CHECK(hipGetLastError());

  // the three temporaries go back together, once the tile sums are there
  ECCKD_CHECK(gas_sum_rows(g, g->ssi, 0, temps, true));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  *out = gas.release();
  return ECCKD_OK;
}

// band albedo of CkdEquipartition::init_sw (find_g_points.cpp:237-261, band_albedo(jband) :1169)
int ecckd_gas_set_band_albedo(ecckd_gas* gas, double surf_albedo) {
  ECCKD_REQUIRE(gas, "ecckd_gas_set_band_albedo: NULL handle");
  gas->surf_albedo = surf_albedo;
  return ECCKD_OK;
}

int ecckd_gas_destroy(ecckd_gas* gas) {
  gas_free(gas);
  return ECCKD_OK;
}

// device views of the resident, sorted arrays (for tests and for reuse of planck_hl)
int ecckd_gas_view(ecckd_gas* gas, const char* name, const double** d_ptr, size_t* rows, size_t* cols) {
  ECCKD_REQUIRE(gas && name && d_ptr, "ecckd_gas_view: NULL argument");
  const size_t nlay = gas->nlay, n = gas->n;
  size_t r = 0;
  const double* p = nullptr;
  if (!strcmp(name, "planck_hl")) { p = gas->planck_hl; r = nlay + 1; }
  else if (!strcmp(name, "bg_optical_depth")) { ECCKD_CHECK(gas_bg_rows(gas)); p = gas->bg_od; r = nlay; }
  // the sweep's line-blocked Planck matrix as it lies in memory, [n/16][nlay+1][16] (tests): only a gas that holds one has it
  else if (!strcmp(name, "planck_hl_blocked")) { p = gas->planck_blk; r = nlay + 1; }
  else if (!strcmp(name, "weighted_metric")) { p = gas->w1; r = nlay; }
  else if (!strcmp(name, "hr")) { p = gas->hr; r = nlay; }
  else if (!strcmp(name, "flux_dn_surf")) { p = gas->fds; r = 1; }
  else if (!strcmp(name, "flux_up_toa")) { p = gas->fut; r = 1; }
  else if (!strcmp(name, "wavenumber")) { p = gas->wn_sorted; r = 1; }
  else if (!strcmp(name, "d_wavenumber")) { p = gas->dwn_sorted; r = 1; }
  else if (!strcmp(name, "ssi")) { p = gas->ssi; r = 1; }
  else if (!strcmp(name, "hr_low")) { p = gas->hr_low; r = nlay; }
  else if (!strcmp(name, "hr_high")) { p = gas->hr_high; r = nlay; }
  else if (!strcmp(name, "flux_extras")) { p = gas->fx; r = 4; }
  if (!p) return ecckd::fail(ECCKD_PARAMETER_ERROR, "ecckd_gas_view: no array named \"%s\"", name);
  *d_ptr = p;
  if (rows) *rows = r;
  if (cols) *cols = n;
  return ECCKD_OK;
}

int ecckd_gas_layer_weight(ecckd_gas* gas, double* h_layer_weight) {
  ECCKD_REQUIRE(gas && h_layer_weight, "ecckd_gas_layer_weight: NULL argument");
  std::memcpy(h_layer_weight, gas->h_layer_weight.data(), gas->h_layer_weight.size() * sizeof(double));
  return ECCKD_OK;
}

double ecckd_gas_comp_cost(ecckd_gas* gas, int reset) {
  if (!gas) return 0.0;
  double c = gas->total_comp_cost;
  if (reset) gas->total_comp_cost = 0.0;
  return c;
}


// The fitted grey optical depth alone: fit_optical_depth_lw / _sw / _sw_total_trans
// (find_g_points.cpp:54-106, :112-165, :171-204) for n intervals -> h_od_fit[n][nlay]
// (total-transmission: the unscaled fit).  Runs K5a + K5b only.
int ecckd_fit_optical_depth(ecckd_gas* g, size_t ibegin, size_t npoints, int n, const double* bound1,
                            const double* bound2, double* h_od_fit) {
  ECCKD_REQUIRE(g && n > 0 && bound1 && bound2 && h_od_fit, "ecckd_fit_optical_depth: bad argument");
  ecckd_ctx* ctx = g->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int nlay = g->nlay;
  std::vector<Interval> iv(n);
  for (int k = 0; k < n; ++k) ECCKD_CHECK(make_interval(g, ibegin, npoints, bound1[k], bound2[k], 0.0, iv[k]));
  const WorkLayout L(n, g->nrows, nlay, 0);   // no sweep in this call
  ECCKD_CHECK(gas_ensure_work(g, L.dev_bytes(), L.iv_bytes + L.fit_bytes));
  Interval* d_iv = L.iv(g->work);
  double* d_sums = L.sums(g->work);
  double* d_fit = L.fit(g->work);
  std::memcpy(g->pinned, iv.data(), (size_t)n * sizeof(Interval));
  ECCKD_HIP_CHECK(hipMemcpyAsync(d_iv, g->pinned, (size_t)n * sizeof(Interval), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_interval_sums, dim3(g->nrows, n), dim3(256), 0, ctx->stream, IntervalArgs(), g->nrows, g->ntiles, g->nsuper, d_iv, 0,
                     d_iv, (const double* const*)g->rows, g->tile_sums, g->super_sums, d_sums);
  if (g->do_sw) {
    // unscaled fit: scaling factors of 1
    hipLaunchKernelGGL(k_fit_sw, dim3(n), dim3(128), nlay * sizeof(double), ctx->stream, nlay, g->method, g->rm, n,
                       1.0, 1.0, d_iv, d_sums, d_fit);
  } else {
    hipLaunchKernelGGL(k_fit_lw, dim3(n), dim3(128), 0, ctx->stream, nlay, g->method, g->rm, d_iv, d_sums, d_fit);
  }
  ECCKD_HIP_CHECK(hipGetLastError());
  double* h = (double*)((char*)g->pinned + L.iv_bytes);
  ECCKD_HIP_CHECK(hipMemcpyAsync(h, d_fit, (size_t)n * nlay * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  std::memcpy(h_od_fit, h, (size_t)n * nlay * sizeof(double));
  return ECCKD_OK;
}

int ecckd_calc_error_batch(ecckd_gas* g, size_t ibegin, size_t npoints, int n, const double* bound1,
                           const double* bound2, double* error) {
  ECCKD_REQUIRE(g && (n == 0 || (bound1 && bound2 && error)), "ecckd_calc_error_batch: NULL argument");
  if (n <= 0) return ECCKD_OK;
  const std::vector<size_t> ib((size_t)n, ibegin), np((size_t)n, npoints);
  return ecckd_calc_error_multi(g, n, ib.data(), np.data(), nullptr, bound1, bound2, error);
}

// ECCKD_TURNAROUND_LOG=1: where the host's time between two batches of a longwave search goes (printed when the process ends)
struct TurnaroundLog {
  typedef std::chrono::steady_clock::time_point time_point;
  bool on = std::getenv("ECCKD_TURNAROUND_LOG") != nullptr;
  time_point seen;
  bool have_seen = false;
  double to_entry = 0, to_first = 0, to_last = 0, wait = 0;
  long long n = 0;
  time_point now() const { return on ? std::chrono::steady_clock::now() : time_point(); }
  // a batch entered at t_entry, whose first and last launch were issued at t_first and t_last, has delivered its errors
  void delivered(time_point t_entry, time_point t_first, time_point t_last) {
    const time_point t = std::chrono::steady_clock::now();
    if (have_seen && std::chrono::duration<double>(t_entry - seen).count() < 500e-6) {   // not the pause between two searches
      to_entry += std::chrono::duration<double>(t_entry - seen).count();
      to_first += std::chrono::duration<double>(t_first - seen).count();
      to_last += std::chrono::duration<double>(t_last - seen).count();
      wait += std::chrono::duration<double>(t - t_last).count();
      n += 1;
    }
    seen = t;
    have_seen = true;
  }
  ~TurnaroundLog() {
    if (on && n)
      std::fprintf(stderr, "search batches %lld: errors seen -> next evaluation entered %.2f us, -> first launch issued %.2f us, -> last launch "
                           "issued %.2f us, waiting for the errors %.2f us\n", n, 1e6 * to_entry / n, 1e6 * to_first / n, 1e6 * to_last / n, 1e6 * wait / n);
  }
};
static TurnaroundLog g_turn;

// HIP events round the sweep launches of every profile_stride-th batch (ecckd_profile_enable), on the lane of the evaluation:
// the context's own events and counters, or the ones this gas was lent (ecckd_find_g_gases).
struct SweepTimer {
  hipEvent_t ev0, ev1;
  ecckd_lane_stat& stat;
  double units;
  bool timed;
  SweepTimer(ecckd_gas* g, double total_pts)
      : ev0(g->lane ? g->lane->pev0 : g->ctx->pev0), ev1(g->lane ? g->lane->pev1 : g->ctx->pev1),
        stat(g->lane ? (g->do_sw ? g->lane->stat_rt_sw : g->lane->stat_rt_lw) : (g->do_sw ? g->ctx->stat_rt_sw : g->ctx->stat_rt_lw)),
        units(total_pts) {
    const ecckd_ctx* ctx = g->ctx;
    long long& profile_seq = g->lane ? g->lane->profile_seq : g->ctx->profile_seq;
    timed = ctx->profile && (profile_seq++ % ctx->profile_stride) == 0;
    if (ctx->profile) { stat.all_calls += 1; stat.all_units += units; }
  }
  int begin(hipStream_t stream) const {
    if (timed) ECCKD_HIP_CHECK(hipEventRecord(ev0, stream));
    return ECCKD_OK;
  }
  int end(hipStream_t stream) const {
    if (timed) ECCKD_HIP_CHECK(hipEventRecord(ev1, stream));
    return ECCKD_OK;
  }
  // after the errors have arrived (the cost kernel behind ev1 has delivered): the sweep's time into the counters and *ms
  int finish(float* ms) {
    if (!timed) return ECCKD_OK;
    ECCKD_HIP_CHECK(hipEventSynchronize(ev1));
    ECCKD_HIP_CHECK(hipEventElapsedTime(ms, ev0, ev1));
    stat.ms += *ms;
    stat.units += units;
    stat.calls += 1;
    return ECCKD_OK;
  }
};

// A batch of intervals on its way through the launch train: what eval_intervals has laid out for the sweeps.
struct Batch {
  int n;                       // intervals
  long long total_pts, nchunks, target_blocks;
  bool fast_path;              // the compile-time-nlay sweeps
  int use_ka;                  // the interval table travels in the first kernel's arguments
  hipStream_t stream;
  Interval* d_iv;
  double *d_sums, *d_fit, *d_part;
  double* h_err_dev;           // device alias of the pinned error slots
  size_t cost_lds;
  TurnaroundLog::time_point t_first;
};

// CkdEquipartition::calc_error, longwave (find_g_points.cpp:322-340): sums and fit, sweep, cost
static int sweep_lw(ecckd_gas* g, Batch& b, const IntervalArgs& ka, const SweepTimer& timer) {
  const int nlay = g->nlay, nhl = nlay + 1, n = b.n;
  const hipStream_t stream = b.stream;
  LwRowBases lw_rows;
  lw_rows.w1 = g->w1; lw_rows.w2 = g->w2; lw_rows.cnt = g->cnt; lw_rows.planck_hl = g->planck_hl; lw_rows.hr = g->hr;
  lw_rows.fds = g->fds; lw_rows.fut = g->fut; lw_rows.n = g->n; lw_rows.is_log = g->method == ECCKD_AVG_LOGARITHMIC;
  hipLaunchKernelGGL(k_interval_sums_fit_lw, dim3(nlay + (g->rm.total - g->rm.H), n), dim3(256), 0, stream, ka, nlay, g->method,
                     g->rm, g->ntiles, g->nsuper, b.d_iv, b.use_ka, b.d_iv, lw_rows, g->tile_sums, g->super_sums,
                     b.d_sums, b.d_fit);
  b.t_first = g_turn.now();
  ECCKD_CHECK(timer.begin(stream));
  // a gas that holds its operands line-blocked (ecckd_gas::bg_blk) is swept from them; `aligned` holds for it by construction
  const bool blk = g->bg_blk != nullptr && b.fast_path;
#define ECCKD_LW_MIRROR(NL, P32)                                                                                          \
  do {                                                                                                                    \
    if (blk)                                                                                                              \
      hipLaunchKernelGGL((k_rt_lw_bb_mirror<NL, P32, true>), dim3(mirror_grid), dim3(RT_THREADS), 0, stream, g->n, n, b.nchunks, b.d_iv, \
                         g->planck_blk, P32 ? nullptr : (const double*)g->bg_blk, P32 ? (const float_x2*)g->bg_blk : nullptr, b.d_fit, b.d_part); \
    else                                                                                                                  \
      hipLaunchKernelGGL((k_rt_lw_bb_mirror<NL, P32, false>), dim3(mirror_grid), dim3(RT_THREADS), 0, stream, g->n, n, b.nchunks, b.d_iv, \
                         g->planck_hl, g->bg_od, (const float_x2*)g->bg_pair, b.d_fit, b.d_part);                        \
  } while (0)
  // a block per chunk.  (ECCKD_RT_PERSISTENT: one resident round of blocks, each taking every mirror_grid-th chunk - measured
  // SLOWER on a partition of unequal intervals, 1 069 against 1 015 us per pass of 38 intervals over 7.2e6 points, equal on
  // equal intervals: the hardware's block dispatcher balances chunks of one to three tiles better than a fixed deal.)
  static const bool persistent = std::getenv("ECCKD_RT_PERSISTENT") != nullptr;
  const unsigned mirror_grid = (unsigned)(persistent ? std::min<long long>(b.nchunks, b.target_blocks) : b.nchunks);
  if (b.fast_path && nlay == 54) {
    if (g->bg_as_pairs()) ECCKD_LW_MIRROR(54, true); else ECCKD_LW_MIRROR(54, false);
  } else if (b.fast_path && nlay == 30) {
    if (g->bg_as_pairs()) ECCKD_LW_MIRROR(30, true); else ECCKD_LW_MIRROR(30, false);
#undef ECCKD_LW_MIRROR
  } else {
    ECCKD_CHECK(gas_bg_rows(g));
    const size_t rt_lds = (size_t)(4 * 2 * nhl + nlay) * sizeof(double);
    hipLaunchKernelGGL(k_rt_lw_bb, dim3((unsigned)b.nchunks), dim3(RT_THREADS), rt_lds, stream, nlay, g->n,
                       n, b.d_iv, g->planck_hl, g->bg_od, b.d_fit, b.d_part);
  }
  ECCKD_CHECK(timer.end(stream));
  hipLaunchKernelGGL(k_cost_lw, dim3(n), dim3(1024), b.cost_lds, stream, nlay, g->rm, b.d_iv,
                     b.nchunks, b.d_part, b.d_sums, g->lev + nhl, g->lev + nhl + nlay, g->flux_weight, b.h_err_dev);
  return ECCKD_OK;
}

// CkdEquipartition::calc_error, shortwave branches (find_g_points.cpp:341-402): sums, fit, sweep(s), cost
static int sweep_sw(ecckd_gas* g, Batch& b, const IntervalArgs& ka, const SweepTimer& timer) {
  const int nlay = g->nlay, nhl = nlay + 1, n = b.n;
  const hipStream_t stream = b.stream;
  Interval* const d_iv = b.d_iv;
  double* const d_fit = b.d_fit;
  const long long nchunks = b.nchunks;
  const bool is_tt = g->method == ECCKD_AVG_TOTAL_TRANSMISSION;
  const RowMap& R = g->rm;
  hipLaunchKernelGGL(k_interval_sums, dim3(g->nrows, n), dim3(256), 0, stream, ka, g->nrows, g->ntiles, g->nsuper, d_iv, b.use_ka,
                     d_iv, (const double* const*)g->rows, g->tile_sums, g->super_sums, b.d_sums);
  hipLaunchKernelGGL(k_fit_sw, dim3(n), dim3(128), nlay * sizeof(double), stream, nlay, g->method, R, n,
                     g->min_scaling, g->max_scaling, d_iv, b.d_sums, d_fit);
  const size_t rt_lds_sw = (size_t)(4 * 2 * nhl + nlay) * sizeof(double);
  const int npass = is_tt ? 2 : 1;
  // total-transmission evaluates the interval with the fit scaled by min_scaling and by max_scaling (:374-386; never equal
  // in the reference: min <= 0.5, max >= 2.5, :666-667): one launch that fetches the column once and sweeps it with both
  // fits (the compile-time-nlay kernels).  At the reference's cos_sza = 0.5 the direct and the reflected beam see the same
  // transmittance exp(-2 tau), bit for bit: the kernels then keep it from the way down (SAME).
  const bool dual = is_tt && b.fast_path;
  const size_t part_stride = (size_t)nchunks * 2 * nhl;
  static const bool no_same = std::getenv("ECCKD_SW_NO_SAME") != nullptr;   // A/B knob
  const bool same_exp = g->cos_sza == 0.5 && !no_same;
  ECCKD_CHECK(timer.begin(stream));
  for (int pass = 0; pass < (dual ? 1 : npass); ++pass) {
    double* part = b.d_part + (size_t)pass * part_stride;
#define ECCKD_SW_SWEEP(NL, NF, SM, FIT)                                                                                         \
  hipLaunchKernelGGL((k_rt_sw_bb_fast<NL, NF, SM>), dim3((unsigned)nchunks), dim3(RT_THREADS), 0, stream, g->n, n, \
                     d_iv, g->cos_sza, g->ssi, g->bg_od, FIT, part)
    const double* fit1 = d_fit + (size_t)pass * n * nlay;
    if (!b.fast_path)
      hipLaunchKernelGGL(k_rt_sw_bb, dim3((unsigned)nchunks), dim3(RT_THREADS), rt_lds_sw, stream, nlay, g->n,
                         n, d_iv, g->cos_sza, g->ssi, g->bg_od, fit1, part);
    else if (nlay == 54 && dual) { if (same_exp) ECCKD_SW_SWEEP(54, 2, true, d_fit); else ECCKD_SW_SWEEP(54, 2, false, d_fit); }
    else if (nlay == 30 && dual) { if (same_exp) ECCKD_SW_SWEEP(30, 2, true, d_fit); else ECCKD_SW_SWEEP(30, 2, false, d_fit); }
    else if (nlay == 54) { if (same_exp) ECCKD_SW_SWEEP(54, 1, true, fit1); else ECCKD_SW_SWEEP(54, 1, false, fit1); }
    else if (nlay == 30) { if (same_exp) ECCKD_SW_SWEEP(30, 1, true, fit1); else ECCKD_SW_SWEEP(30, 1, false, fit1); }
#undef ECCKD_SW_SWEEP
  }
  ECCKD_CHECK(timer.end(stream));
  // both evaluations in one launch; the errors go straight into the pinned host buffer (a few bytes over PCIe)
  SwTruthRows rows;
  rows.rH[0] = is_tt ? R.HL : R.H;      rows.rH[1] = R.HH;
  rows.rFDS[0] = is_tt ? R.FDSL : R.FDS; rows.rFDS[1] = R.FDSH;
  rows.rFUT[0] = is_tt ? R.FUTL : R.FUT; rows.rFUT[1] = R.FUTH;
  hipLaunchKernelGGL(k_cost_sw, dim3(n, npass), dim3(1024), b.cost_lds, stream, nlay, R.total, rows, d_iv, nchunks,
                     b.d_part, part_stride, b.d_sums, g->lev + nhl, g->lev + nhl + nlay, g->flux_weight, g->cos_sza, b.h_err_dev);
  return ECCKD_OK;
}

// Errors of the intervals iv[0..n) (first / last sorted index and albedo filled in) on the device -> error[0..n).
static int eval_intervals(ecckd_gas* g, std::vector<Interval>& iv, double* error) {
  const TurnaroundLog::time_point t_entry = g_turn.now();
  ecckd_ctx* ctx = g->ctx;
  const int nlay = g->nlay, nhl = nlay + 1;
  Batch b;
  const int n = b.n = (int)iv.size();
  b.stream = g->eval_stream();
  b.total_pts = 0;
  for (int k = 0; k < n; ++k) b.total_pts += iv[k].i2 - iv[k].i1 + 1;

  // Chunking.  Every interval is cut into chunks of ITS OWN size: the smallest multiple of what one block iteration covers
  // (the longwave mirror kernel: two wave pairs = 128 points; the other sweeps: 256) with which the interval fills at most
  // one round of resident blocks.  The chunk size - and with it the order in which the interval's points are added up, chunk
  // by chunk in K5c and partial by partial in K5d - is a function of the interval alone (its first index and its length,
  // chunk_layout.hpp), so an interval's error has the same bits whether it is evaluated alone, with its neighbours
  // (calc_error_all, equipartition.h:98-116) or next to other bands' intervals (ecckd_calc_error_multi).  A batch of n
  // intervals launches up to n rounds of small blocks; the hardware's block dispatcher balances them.
  // The longwave mirror sweep counts the chunks from the 128-byte line that holds the interval's first point, so that every
  // row load of every tile is four whole lines: where the rows start on a line and a row is a whole number of lines.
  // ECCKD_RT_GENERIC (read per call): the run-time-nlay sweeps instead of the compile-time ones, for cross-checks at full size
  b.fast_path = (nlay == 54 || nlay == 30) && std::getenv("ECCKD_RT_GENERIC") == nullptr;
  // mirror path: 3 resident blocks per CU (3 waves/SIMD); the two-fit shortwave sweep holds 2
  static const int rt_bpc = std::getenv("ECCKD_RT_BPC") ? std::max(1, std::atoi(std::getenv("ECCKD_RT_BPC"))) : 3;   // tuning knob
  static const int sw2_bpc = std::getenv("ECCKD_SW2_BPC") ? std::max(1, std::atoi(std::getenv("ECCKD_SW2_BPC"))) : 2;   // tuning knob
  const bool is_tt = g->do_sw && g->method == ECCKD_AVG_TOTAL_TRANSMISSION;
  b.target_blocks = (long long)ctx->num_cu * (is_tt && b.fast_path ? sw2_bpc : b.fast_path ? rt_bpc : 8);
  const long long gran = (!g->do_sw && b.fast_path) ? RT_THREADS / 2 : RT_THREADS;
  const auto on_line = [](const void* q) { return (uintptr_t)q % (ecckd::chunk_layout::LINE_PTS * sizeof(double)) == 0; };
  const bool aligned = !g->do_sw && b.fast_path && g->chunks_from_line && g->n % ecckd::chunk_layout::LINE_PTS == 0 &&
                       (g->bg_blk /* made only where all of this held */ || (on_line(g->planck_hl) && on_line(g->bg_od) && on_line(g->bg_pair)));
  b.nchunks = 0;
  for (int k = 0; k < n; ++k) {
    const ecckd::chunk_layout::Layout lay = ecckd::chunk_layout::of_interval(iv[k].i1, iv[k].i2, b.target_blocks, gran, aligned);
    iv[k].chunk_pts = lay.chunk_pts;
    iv[k].head = (int)lay.head;
    iv[k].chunk0 = (int)std::min<long long>(b.nchunks, 0x7fffffffLL);
    b.nchunks += lay.nchunks;
  }
  ECCKD_REQUIRE(b.nchunks < 0x7fffffffLL, "ecckd_calc_error_batch: %lld chunks in one batch", b.nchunks);
  b.cost_lds = (size_t)(COST_GROUPS * 2 * nhl + 2 * nhl + nlay) * sizeof(double);
  ECCKD_REQUIRE(b.target_blocks <= 32 * COST_GROUPS && b.cost_lds <= 64 * 1024, "ecckd_calc_error_batch: %lld chunks per interval / %d layers exceed the cost kernel's room",
                b.target_blocks, nlay);

  // The errors are written straight into the pinned host buffer by the last kernel (a few bytes over PCIe): no device-to-host
  // copy in the stream.  err_bytes count in the device request too: it sizes the block the context's cache later hands on.
  const WorkLayout L(n, g->nrows, nlay, b.nchunks);
  const size_t err_bytes = ecckd_align_up((size_t)2 * n * sizeof(double), 256);
  ECCKD_CHECK(gas_ensure_work(g, L.dev_bytes() + err_bytes, L.iv_bytes + err_bytes));
  b.d_iv = L.iv(g->work);
  b.d_sums = L.sums(g->work);
  b.d_fit = L.fit(g->work);
  b.d_part = L.part(g->work);
  Interval* h_iv = (Interval*)g->pinned;
  double* h_err = (double*)((char*)g->pinned + L.iv_bytes);
  if (g->pinned_dev_of != g->pinned) {        // the device alias of the pinned buffer, looked up once per (re)allocation
    ECCKD_HIP_CHECK(hipHostGetDevicePointer((void**)&g->pinned_dev, g->pinned, 0));
    g->pinned_dev_of = g->pinned;
  }
  b.h_err_dev = (double*)((char*)g->pinned_dev + L.iv_bytes);
  const int nslots = is_tt ? 2 * n : n;
  ecckd::slots_mark_pending(h_err, nslots);
  static const bool no_karg = std::getenv("ECCKD_NO_KARG") != nullptr;   // A/B knob: always copy the interval table
  b.use_ka = (n <= KARG_MAX && !no_karg) ? 1 : 0;
  IntervalArgs ka;
  if (b.use_ka) {
    for (int k = 0; k < KARG_MAX; ++k) ka.iv[k] = iv[k < n ? k : n - 1];
  } else {
    std::memset(&ka, 0, sizeof ka);
    std::memcpy(h_iv, iv.data(), (size_t)n * sizeof(Interval));
    ECCKD_HIP_CHECK(hipMemcpyAsync(b.d_iv, h_iv, (size_t)n * sizeof(Interval), hipMemcpyHostToDevice, b.stream));
  }

  SweepTimer timer(g, (double)b.total_pts);
  ECCKD_CHECK(g->do_sw ? sweep_sw(g, b, ka, timer) : sweep_lw(g, b, ka, timer));
  ECCKD_HIP_CHECK(hipGetLastError());
  const TurnaroundLog::time_point t_last = g_turn.now();
  ECCKD_CHECK(ecckd::slots_wait(b.stream, h_err, nslots, "interval errors"));
  if (g_turn.on && !g->do_sw) g_turn.delivered(t_entry, b.t_first, t_last);
  if (is_tt)
    for (int k = 0; k < n; ++k) error[k] = 0.5 * (h_err[k] + h_err[n + k]);  // find_g_points.cpp:386
  else
    std::memcpy(error, h_err, (size_t)n * sizeof(double));
  float ms = 0.f;
  ECCKD_CHECK(timer.finish(&ms));
  if (timer.timed && !g->do_sw) {
    // ECCKD_SWEEP_LOG=<file>: one line per longwave sweep launch (intervals, points, chunks, ms) for tools/sweep_sizes.py
    static FILE* sweep_log = std::getenv("ECCKD_SWEEP_LOG") ? std::fopen(std::getenv("ECCKD_SWEEP_LOG"), "a") : nullptr;
    if (sweep_log) std::fprintf(sweep_log, "%d %lld %lld %.6f\n", n, b.total_pts, b.nchunks, (double)ms);
  }
  return ECCKD_OK;
}

// The same for intervals of DIFFERENT bands in one batch: interval k is the fraction [bound1[k], bound2[k]] of the band
// that starts at sorted index ibegin[k] and has npoints[k] points.  One launch train for all of them - the band searches
// of a gas are independent (find_g_points.cpp:1152), so their error evaluations can share the GPU (ecckd_find_g_bands_ex).
int ecckd_calc_error_multi(ecckd_gas* g, int n, const size_t* ibegin_k, const size_t* npoints_k, const double* albedo_k,
                           const double* bound1, const double* bound2, double* error) {
  ECCKD_REQUIRE(g && (n == 0 || (ibegin_k && npoints_k && bound1 && bound2 && error)), "ecckd_calc_error_multi: NULL argument");
  if (n <= 0) return ECCKD_OK;
  ecckd_ctx* ctx = g->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));

  std::vector<Interval> iv(n);
  for (int k = 0; k < n; ++k)
    ECCKD_CHECK(make_interval(g, ibegin_k[k], npoints_k[k], bound1[k], bound2[k], albedo_k ? albedo_k[k] : g->surf_albedo, iv[k]));
  for (int k = 0; k < n; ++k) g->total_comp_cost += bound2[k] - bound1[k];  // :320: the reference's counter counts every request

  // The memo: only intervals not seen before (and once each) go to the device.  ECCKD_NO_ERROR_MEMO (read per call): every
  // request is evaluated, as the reference does - for cross-checks.
  const bool use_memo = std::getenv("ECCKD_NO_ERROR_MEMO") == nullptr;
  if (g->error_memo.size() > (size_t)4000000) g->error_memo.clear();
  std::vector<Interval> todo;
  std::vector<int> slot(n, -1);            // index into todo, or -1: served from the memo
  std::unordered_map<IntervalKey, int, IntervalKeyHash> in_batch;
  for (int k = 0; k < n; ++k) {
    const IntervalKey key = interval_key(g, iv[k]);
    const double len = (double)(iv[k].i2 - iv[k].i1 + 1);
    g->memo_requests += 1;
    g->points_requested += len;
    if (use_memo) {
      auto hit = g->error_memo.find(key);
      if (hit != g->error_memo.end()) { error[k] = hit->second; g->memo_hits += 1; continue; }
      auto dup = in_batch.find(key);
      if (dup != in_batch.end()) { slot[k] = dup->second; g->memo_hits += 1; continue; }
      in_batch.emplace(key, (int)todo.size());
    }
    slot[k] = (int)todo.size();
    todo.push_back(iv[k]);
    g->points_evaluated += len;
  }
  if (todo.empty()) return ECCKD_OK;
  std::vector<double> fresh(todo.size());
  ECCKD_CHECK(eval_intervals(g, todo, fresh.data()));
  for (int k = 0; k < n; ++k)
    if (slot[k] >= 0) error[k] = fresh[slot[k]];
  if (use_memo)
    for (size_t t = 0; t < todo.size(); ++t) g->error_memo.emplace(interval_key(g, todo[t]), fresh[t]);
  return ECCKD_OK;
}

// What the memo of interval errors saved: intervals asked for / found in the memo, wavenumber points asked for (what the
// reference would have swept) / actually swept on the device.
int ecckd_gas_eval_stats(ecckd_gas* gas, long long* requests, long long* memo_hits, double* points_requested, double* points_evaluated) {
  ECCKD_REQUIRE(gas, "ecckd_gas_eval_stats: NULL handle");
  if (requests) *requests = gas->memo_requests;
  if (memo_hits) *memo_hits = gas->memo_hits;
  if (points_requested) *points_requested = gas->points_requested;
  if (points_evaluated) *points_evaluated = gas->points_evaluated;
  return ECCKD_OK;
}

// Forget every interval error this gas has answered and zero the counters of ecckd_gas_eval_stats: the next search sweeps
// every interval again (timing one prepared gas twice; the reference has no memo at all).
int ecckd_gas_reset_memo(ecckd_gas* gas) {
  ECCKD_REQUIRE(gas, "ecckd_gas_reset_memo: NULL handle");
  gas->error_memo.clear();
  gas->memo_requests = gas->memo_hits = 0;
  gas->points_requested = gas->points_evaluated = 0.0;
  gas->total_comp_cost = 0.0;
  return ECCKD_OK;
}

// Bytes the error sweep (K5c) reads per spectral point of an interval: the Planck rows and the background rows as this gas
// holds them (FLOAT pairs if every background value is a float, DOUBLE rows otherwise); shortwave: background rows + ssi.
int ecckd_gas_sweep_bytes_per_point(ecckd_gas* gas, double* bytes) {
  ECCKD_REQUIRE(gas && bytes, "ecckd_gas_sweep_bytes_per_point: NULL argument");
  const int nlay = gas->nlay;
  if (gas->do_sw) *bytes = (double)(nlay + 1) * 8.0;
  else *bytes = (double)(nlay + 1) * 8.0 + (double)nlay * (gas->bg_as_pairs() ? 4.0 : 8.0);
  return ECCKD_OK;
}

// ---------------------------------------------------------------------------
// partition search over a host callback (replaces Equipartition, equipartition.h:63-208)
struct ecckd_partition {
  ecckd_error_fn fn = nullptr;
  void* user = nullptr;
  ecckd::PartitionSearch* ps = nullptr;
};

int ecckd_partition_create(ecckd_error_fn fn, void* user, ecckd_partition** out) {
  ECCKD_REQUIRE(fn && out, "ecckd_partition_create: NULL argument");
  ecckd_partition* p = new ecckd_partition();
  p->fn = fn;
  p->user = user;
  p->ps = new ecckd::PartitionSearch(
      [p](int n, const double* b1, const double* b2, double* e) { return p->fn(n, b1, b2, e, p->user); });
  *out = p;
  return ECCKD_OK;
}

int ecckd_partition_destroy(ecckd_partition* p) {
  if (p) {
    delete p->ps;
    delete p;
  }
  return ECCKD_OK;
}

int ecckd_partition_configure(ecckd_partition* p, double resolution, double partition_tolerance,
                              int partition_max_iterations, int line_search_max_iterations,
                              int cubic_interpolation, int minimize_frac_range) {
  ECCKD_REQUIRE(p, "ecckd_partition_configure: NULL handle");
  p->ps->set_resolution(resolution);
  p->ps->set_partition_tolerance(partition_tolerance);
  p->ps->set_partition_max_iterations(partition_max_iterations);
  p->ps->set_line_search_max_iterations(line_search_max_iterations);
  p->ps->set_cubic_interpolation(cubic_interpolation != 0);
  p->ps->set_minimize_frac_range(minimize_frac_range != 0);
  return ECCKD_OK;
}

int ecckd_partition_n(ecckd_partition* p, int ni, double* bounds, double* error, int* status) {
  ECCKD_REQUIRE(p && ni > 0 && bounds && error && status, "ecckd_partition_n: bad argument");
  *status = p->ps->equipartition_n(ni, bounds, error);
  if (p->ps->evaluator_status()) return p->ps->evaluator_status();
  return ECCKD_OK;
}

int ecckd_partition_e(ecckd_partition* p, double target_error, double bound0, double boundn, int* ni,
                      double* bounds, double* error, int capacity, int* status) {
  ECCKD_REQUIRE(p && ni && bounds && error && status, "ecckd_partition_e: NULL argument");
  std::vector<double> b, e;
  int n = 0;
  *status = p->ps->equipartition_e(target_error, bound0, boundn, n, b, e);
  if (p->ps->evaluator_status()) return p->ps->evaluator_status();
  *ni = n;
  if (*status == ecckd::PS_INPUT_ERROR) return ECCKD_OK;
  ECCKD_REQUIRE(n <= capacity, "ecckd_partition_e: %d intervals exceed the caller's capacity %d", n, capacity);
  std::memcpy(bounds, b.data(), (size_t)(n + 1) * sizeof(double));
  std::memcpy(error, e.data(), (size_t)n * sizeof(double));
  return ECCKD_OK;
}

int ecckd_partition_set_trace(ecckd_partition* p, ecckd_trace_fn fn, void* user) {
  ECCKD_REQUIRE(p, "ecckd_partition_set_trace: NULL handle");
  if (fn) p->ps->set_trace([fn, user](int site, double lhs, double rhs, int taken) { fn(site, lhs, rhs, taken, user); });
  else p->ps->set_trace(nullptr);
  return ECCKD_OK;
}

const char* ecckd_partition_status_string(int status) { return ecckd::partition_status_string(status); }

}  // extern "C"
