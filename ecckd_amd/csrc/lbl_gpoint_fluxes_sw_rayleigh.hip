// lbl_gpoint_fluxes_sw_rayleigh.hip - line-by-line shortwave fluxes of one column WITH Rayleigh scattering resolved per g
// point, for up to LBL_MAX_SZA solar zenith angles: the two-stream transfer of k_lbl_fluxes_sw_rayleigh
// (lbl_fluxes_sw_rayleigh.hip; rayleigh_layer, rayleigh_up, rayleigh_down of lbl_rt.hpp) per wavenumber, and the sum of its
// three flux rows per level - direct, total downwelling, upwelling - over the wavenumbers of every g point in the shape of
// k_lbl_gpoint_fluxes_sw (lbl_gpoint_fluxes_sw.hip): one thread per wavenumber in natural order, 256 per tile, binned into
// the g points inside the block by the scheme of gpoint_bin.hpp.  The other output mode of the same kernel writes the
// spectral fluxes themselves (FLOAT rows) with the broadband sums.  Bitwise reproducible.
//
// Transfer.  Expression by expression that of the band kernel: the direct chain on (double)tau_abs + (double)tau_ray stored
// per level, the sweep up that leaves the albedo A and the source S below every level, and the sweep down that yields the
// three fluxes of a level in turn, the direct one taken from the stored value.
//
// Rows.  The down sweep hands the binner the rows 3 * level + flux in that order; a batch is GB_LB = 8 consecutive rows
// (levels are not kept whole: 8 rows are 2 2/3 levels), the last batch what is left of 3 (nlay + 1).  The accumulator is
// acc[3][nhl][ncols], one angle.
//
// Workspace.  D, A and S per level are 3 (nlay + 1) doubles per thread: in a device workspace [physical block][slot][level]
// [thread], own element only, coalesced, no barrier, as in the band kernel.  The PHYSICAL grid is bounded (rayleigh_grid of
// lbl_rt.hpp: blocks per compute unit, or ECCKD_RAYLEIGH_GRID) and sizes the workspace; its blocks loop over the LOGICAL
// blocks of tile_grid(nwav), each of which writes its own partial, and k_gpoint_combine adds the partials in logical order:
// the bits of the result do not depend on the bound.  Blocks per compute unit: what fits of RAYLEIGH_BLOCKS_PER_CU = 3 into
// the CU's 160 KB of LDS beside the binner's 22 KB static arrays, i.e. min(3, 160 KB / (22 KB + accumulator)).
//
// Angles and launches.  One angle per launch, angle outermost, the column ranges inside; the workspace holds one angle.  A
// tile is ranked again for every angle: 64 int4 comparisons per thread against 3 nlay rayleigh_layer evaluations.  The split
// into launches is a function of (nlay, nsza, ng) alone:
//   cap = SF_ACC_BYTES / (24 (nlay+1))   columns per launch (44 at 54 layers, 117 at 20)
//   launches = nsza * ceil((ng + 1) / cap): per angle the column ranges of bin_column_ranges(ng, min(cap, ng + 1)) - the
//              first range holds cap - 1 g points and the column of the points without one, every later one cap g points
//              (54 layers: ng = 43 -> [43]; 44 -> [43, 1]; 87 -> [43, 44]; 88 -> [43, 44, 1]).
// Splitting columns repeats the whole transfer.  Neither the ranges nor a launch depend on nsza, so angle s of a multi-angle
// call has the bits of a single-angle call.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage), the same for all four type pairings: binned mode 135
// VGPRs, spectral mode 137; 106 SGPRs with 43 / 55 of them spilled to VGPR lanes; scratch 0 bytes per lane, no VGPR spill;
// static LDS 22 528 B; occupancy by registers 3 waves per SIMD = 3 blocks per compute unit, which is RAYLEIGH_BLOCKS_PER_CU.
// It runs at that residency while 22 KB + accumulator <= 53.3 KB (up to 24 columns at 54 layers: ng = 16, the spectral
// mode); from 25 columns on (ng = 32: 64.5 KB) the LDS allows 2 blocks per compute unit, 2 waves per SIMD, and the grid is
// bounded to match: with 3 blocks per compute unit asked for there, the third waits for a slot and the call takes 71.5
// instead of 62.5 ms (DESIGN.md "Rayleigh scattering in sw_spectra" has the measurements).
#include "common.hpp"
#include "gmap.hpp"
#include "gpoint_bin.hpp"
#include "lbl_rt.hpp"

#include <algorithm>
#include <vector>

namespace {

using namespace ecckd::lbl;

constexpr size_t CU_LDS_BYTES = 160 * 1024;      // LDS of a compute unit (gfx950)
constexpr int GR_ROWS = RAYLEIGH_FLUXES;         // rows per level that the down sweep hands the binner

// dynamic LDS: acc[3][nhl][ncols]; ws: [gridDim.x][3][nhl][GB_THREADS]; partial: [nlogical][3][nhl][ncols]
template <typename AbsT, typename RayT, bool SPECTRAL>
__global__ void __launch_bounds__(GB_THREADS)
k_lbl_gpoint_fluxes_sw_rayleigh(int nlay, size_t nwav, size_t abs_stride, size_t ray_stride, int tiles_per_block, int nlogical,
                                double cos_sza, double minus_sec_sza /* -1.0 / cos_sza */, const double* __restrict__ ssi,
                                const double* __restrict__ albedo /* per wavenumber or NULL: 0 */, const AbsT* __restrict__ od_abs,
                                const RayT* __restrict__ od_ray, const int32_t* __restrict__ g_point /* NULL: every point in column 0 */,
                                int g0, int gcount, int col_unassigned /* column of g_point < 0, or -1 */, int ncols, double* ws,
                                double* __restrict__ partial, float* __restrict__ spec_dir, float* __restrict__ spec_dn,
                                float* __restrict__ spec_up /* [nhl][stride] */, size_t spec_stride) {
  extern __shared__ double s_acc[];
  const int nhl = nlay + 1;
  const int tid = threadIdx.x;
  const int nacc = GR_ROWS * nhl * ncols;
  const int nrows = GR_ROWS * nhl;                // row k = 3 * level + flux
  // this thread as an adder: row slot of the batch and segment
  const int slot = tid / GB_SEG, seg = tid % GB_SEG, base = seg * GB_SEGLEN;
  double* my = ws + (size_t)blockIdx.x * RAYLEIGH_SLOTS * nhl * GB_THREADS + tid;
  double* w_d = my;                               // element (slot, level) of this thread: [(slot * nhl + level) * GB_THREADS]
  double* w_a = my + (size_t)nhl * GB_THREADS;
  double* w_s = my + (size_t)2 * nhl * GB_THREADS;

  for (int lb = blockIdx.x; lb < nlogical; lb += gridDim.x) {
    for (int t = tid; t < nacc; t += GB_THREADS) s_acc[t] = 0.0;
    const size_t tile0 = (size_t)lb * tiles_per_block;
    for (int it = 0; it < tiles_per_block; ++it) {
      const size_t i = (tile0 + it) * GB_THREADS + tid;
      if ((tile0 + it) * GB_THREADS >= nwav) break;                           // (block-uniform)
      const bool live = i < nwav;
      const size_t j = live ? i : nwav - 1;
      const int pos = tile_rank(tid, tile_key(live, g_point, j, g0, gcount, col_unassigned));
      const TilePieces pieces = tile_pieces(seg, base);

      // the batch of n rows that ends with row `last`: row k goes to the accumulator row (flux, level)
      auto reduce = [&](int last, int n) {
        const bool on = slot < n;
        const int k = last - (n - 1) + (on ? slot : 0);
        const int r = (k % GR_ROWS) * nhl + k / GR_ROWS;
        reduce_batch(pieces, on, slot, seg, base, s_acc + (size_t)r * ncols);
      };
      // row k of this thread's point; the batch is added when it is full or the rows end.  A dead lane carries exactly 0.
      auto put = [&](int k, double v) {
        s_f[(size_t)(k % GB_LB) * GB_ROW + pos] = live ? v : 0.0;
        if ((k + 1) % GB_LB == 0) reduce(k, GB_LB);
        else if (k + 1 == nrows) reduce(k, (k % GB_LB) + 1);
      };
      auto emit = [&](int level, double direct, double dn, double up) {
        if (SPECTRAL && live) {
          spec_dir[(size_t)level * spec_stride + i] = (float)direct;
          spec_dn[(size_t)level * spec_stride + i] = (float)dn;
          spec_up[(size_t)level * spec_stride + i] = (float)up;
        }
        put(GR_ROWS * level, direct);
        put(GR_ROWS * level + 1, dn);
        put(GR_ROWS * level + 2, up);
      };

      // ---- the column: the Rayleigh steps of lbl_rt.hpp as k_lbl_fluxes_sw_rayleigh takes them
      const double inc = ssi[j];
      const double alb = albedo ? albedo[j] : 0.0;
      auto layer = [&](int l) {
        return rayleigh_layer((double)od_abs[(size_t)l * abs_stride + j], (double)od_ray[(size_t)l * ray_stride + j], cos_sza,
                              minus_sec_sza);
      };
      // the direct beam, as k_lbl_fluxes_sw on tau_abs + tau_ray; dead lanes carry no flux at all
      double flux = live ? cos_sza * inc : 0.0;
      w_d[0] = flux;
      for (int l = 0; l < nlay; ++l) {
        const double tau = (double)od_abs[(size_t)l * abs_stride + j] + (double)od_ray[(size_t)l * ray_stride + j];
        flux = flux * exp(minus_sec_sza * tau);
        w_d[(size_t)(l + 1) * GB_THREADS] = flux;
      }
      // up: the albedo and the source below every level
      double a = alb, src = alb * flux;
      w_a[(size_t)nlay * GB_THREADS] = a;
      w_s[(size_t)nlay * GB_THREADS] = src;
      for (int l = nlay - 1; l >= 0; --l) {
        const RayleighLayer L = layer(l);
        rayleigh_up(L, w_d[(size_t)l * GB_THREADS], a, src, a, src);
        w_a[(size_t)l * GB_THREADS] = a;
        w_s[(size_t)l * GB_THREADS] = src;
      }
      // down: the three fluxes of every level in turn, the direct one from the value the first sweep stored
      double dn = 0.0, up = src;
      double d_top = w_d[0];
      emit(0, d_top, dn + d_top, up);
      for (int l = 0; l < nlay; ++l) {
        const RayleighLayer L = layer(l);
        rayleigh_down(L, d_top, w_a[(size_t)(l + 1) * GB_THREADS], w_s[(size_t)(l + 1) * GB_THREADS], dn, dn, up);
        d_top = w_d[(size_t)(l + 1) * GB_THREADS];
        emit(l + 1, d_top, dn + d_top, up);
      }
      __syncthreads();                                                        // the next tile rewrites the binner's arrays
    }
    __syncthreads();
    for (int t = tid; t < nacc; t += GB_THREADS) partial[(size_t)lb * nacc + t] = s_acc[t];
    __syncthreads();                                                          // the next logical block zeroes the accumulator
  }
}

// One column.  d_g_point == NULL: one column of the accumulator (the broadband sum); otherwise ng g points + "none".
// h_out[nsza][3][nhl][ng + 1]: flux 0 direct, 1 total down, 2 up; column ng = the wavenumbers with no g point.
int run(ecckd_ctx* ctx, const char* who, int nlay, size_t nwav, int nsza, const double* h_ang /* sw_angle_table */, const double* d_ssi,
        const double* d_albedo, const void* d_od_abs, int abs_type, size_t abs_stride, const void* d_od_ray, int ray_type,
        size_t ray_stride, const int32_t* d_g_point, int ng, float* d_spec_dir, float* d_spec_dn, float* d_spec_up, size_t spec_stride,
        std::vector<double>& h_out) {
  const int nhl = nlay + 1;
  const int out_cols = ng + 1;
  const int cap = (int)std::min<size_t>(SF_ACC_BYTES / ((size_t)GR_ROWS * nhl * sizeof(double)), 1u << 20);   // columns per launch
  ECCKD_REQUIRE(cap >= 2, "%s: %d layers are more than the block's accumulator holds", who, nlay);
  const int cols_per_launch = std::min(cap, out_cols);              // the split (see the header): a function of (nlay, ng) alone
  const TileGrid grid = tile_grid(nwav);
  const int tpb = grid.tpb, nblk = grid.nblk;
  const size_t nrows = (size_t)nsza * GR_ROWS * nhl;
  const size_t max_acc = (size_t)GR_ROWS * nhl * cols_per_launch;
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(RAYLEIGH_BLOCKS_PER_CU, CU_LDS_BYTES / (GB_FIXED_LDS + max_acc * sizeof(double))));
  const size_t pgrid = rayleigh_grid(ctx, (size_t)nblk, per_cu);
  void* d[3];
  ECCKD_CHECK(ecckd::carve_scratch(ctx, {nrows * out_cols * sizeof(double), (size_t)nblk * max_acc * sizeof(double),
                                         pgrid * RAYLEIGH_SLOTS * nhl * GB_THREADS * sizeof(double)}, d));
  double* d_out = (double*)d[0];
  double* d_part = (double*)d[1];
  double* d_ws = (double*)d[2];
  ECCKD_HIP_CHECK(hipMemsetAsync(d_out, 0, nrows * out_cols * sizeof(double), ctx->stream));
  const bool spectral = d_spec_dir != nullptr;
  for (int s = 0; s < nsza; ++s) {
    const size_t so = (size_t)s * nhl * spec_stride;
    auto launch = [&](int g0, int gcount, int col_un, int ncols) {
      const size_t lds = (size_t)GR_ROWS * nhl * ncols * sizeof(double);
      return with_od_type(abs_type, [&](auto ta) {
        return with_od_type(ray_type, [&](auto tr) {
          using AbsT = decltype(ta);
          using RayT = decltype(tr);
          const auto kernel = spectral ? k_lbl_gpoint_fluxes_sw_rayleigh<AbsT, RayT, true> : k_lbl_gpoint_fluxes_sw_rayleigh<AbsT, RayT, false>;
          ECCKD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)SF_ACC_BYTES));
          hipLaunchKernelGGL(kernel, dim3((unsigned)pgrid), dim3(GB_THREADS), lds, ctx->stream, nlay, nwav, abs_stride, ray_stride, tpb,
                             nblk, h_ang[s], h_ang[LBL_MAX_SZA + s], d_ssi, d_albedo, (const AbsT*)d_od_abs, (const RayT*)d_od_ray,
                             d_g_point, g0, gcount, col_un, ncols, d_ws, d_part, spectral ? d_spec_dir + so : nullptr,
                             spectral ? d_spec_dn + so : nullptr, spectral ? d_spec_up + so : nullptr, spec_stride);
          return (int)ECCKD_OK;
        });
      });
    };
    ECCKD_CHECK(bin_column_ranges(ctx, ng, d_g_point != nullptr, cols_per_launch, nblk, GR_ROWS * nhl, s * GR_ROWS * nhl, d_part, d_out,
                                  launch));
  }
  h_out.resize(nrows * out_cols);
  return ecckd_d2h(ctx, h_out.data(), d_out, h_out.size() * sizeof(double));
}

}  // namespace

extern "C" {

int ecckd_lbl_gpoint_fluxes_sw_rayleigh(ecckd_gmap* gmap, int nlay, int nsza, const double* h_cos_sza, const double* d_ssi,
                                        const double* d_albedo, const void* d_od_abs, int abs_type, size_t abs_stride,
                                        const void* d_od_ray, int ray_type, size_t ray_stride, double* h_flux_dn_direct,
                                        double* h_flux_dn, double* h_flux_up, double* h_bb_dn_direct, double* h_bb_dn, double* h_bb_up) {
  const char* who = "ecckd_lbl_gpoint_fluxes_sw_rayleigh";
  ECCKD_REQUIRE(gmap && nlay > 0 && h_cos_sza && d_ssi && d_od_abs && d_od_ray && h_flux_dn_direct && h_flux_dn && h_flux_up,
                "%s: bad argument", who);
  double h_ang[2 * LBL_MAX_SZA];
  ECCKD_CHECK(sw_angle_table(who, nsza, h_cos_sza, h_ang));
  ECCKD_CHECK(check_od(who, abs_type, abs_stride, gmap->n));
  ECCKD_CHECK(check_od(who, ray_type, ray_stride, gmap->n));
  ecckd_ctx* ctx = gmap->ctx;
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int32_t* d_g = nullptr; const double* d_wn = nullptr; const double* d_dwn = nullptr;
  ECCKD_CHECK(ecckd::gmap_natural(gmap, &d_g, &d_wn, &d_dwn));
  const int nhl = nlay + 1, ng = gmap->ng;
  std::vector<double> out;
  ECCKD_CHECK(run(ctx, who, nlay, gmap->n, nsza, h_ang, d_ssi, d_albedo, d_od_abs, abs_type, abs_stride, d_od_ray, ray_type, ray_stride,
                  d_g, ng, nullptr, nullptr, nullptr, 0, out));
  unpack_gpoint_out3(out.data(), nsza, nhl, ng, {h_flux_dn_direct, h_flux_dn, h_flux_up}, {h_bb_dn_direct, h_bb_dn, h_bb_up});
  return ECCKD_OK;
}

int ecckd_lbl_spectral_fluxes_sw_rayleigh(ecckd_ctx* ctx, int nlay, size_t nwav, int nsza, const double* h_cos_sza, const double* d_ssi,
                                          const double* d_albedo, const void* d_od_abs, int abs_type, size_t abs_stride,
                                          const void* d_od_ray, int ray_type, size_t ray_stride, float* d_flux_dn_direct,
                                          float* d_flux_dn, float* d_flux_up, size_t flux_stride, double* h_bb_dn_direct,
                                          double* h_bb_dn, double* h_bb_up) {
  const char* who = "ecckd_lbl_spectral_fluxes_sw_rayleigh";
  ECCKD_REQUIRE(ctx && nlay > 0 && nwav > 0 && h_cos_sza && d_ssi && d_od_abs && d_od_ray && d_flux_dn_direct && d_flux_dn && d_flux_up,
                "%s: bad argument", who);
  double h_ang[2 * LBL_MAX_SZA];
  ECCKD_CHECK(sw_angle_table(who, nsza, h_cos_sza, h_ang));
  ECCKD_CHECK(check_od(who, abs_type, abs_stride, nwav));
  ECCKD_CHECK(check_od(who, ray_type, ray_stride, nwav));
  ECCKD_REQUIRE(flux_stride >= nwav, "%s: flux_stride (%zu) < nwav (%zu)", who, flux_stride, nwav);
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  const int nhl = nlay + 1;
  std::vector<double> out;
  ECCKD_CHECK(run(ctx, who, nlay, nwav, nsza, h_ang, d_ssi, d_albedo, d_od_abs, abs_type, abs_stride, d_od_ray, ray_type, ray_stride,
                  nullptr, 0, d_flux_dn_direct, d_flux_dn, d_flux_up, flux_stride, out));
  unpack_gpoint_out3(out.data(), nsza, nhl, 0, {nullptr, nullptr, nullptr}, {h_bb_dn_direct, h_bb_dn, h_bb_up});   // one column
  return ECCKD_OK;
}

}  // extern "C"
