// gas_optics.hip - the resident gas-optics handle: a CKD model uploaded once and applied to atmospheric columns that already sit
// in device memory (CkdModel::calc_optical_depth, ckd_model.cpp:925-1102, and calc_planck_function, :1107-1145).  The host step
// (flattening the model, the refusals, the launch plan) is gas_optics_tables.cpp; the device code shared with the fused fluxes
// of gas_optics_fluxes.hip, and the handle itself, are gas_optics_device.hpp.
//
// k_gas_optics: a block takes a tile of CELLS_PER_BLOCK consecutive cells of the flattened (column, layer) index.  One lane per
// cell forms what all g points of the cell share - the three axis positions, their logarithms and the cell's (table row,
// coefficient) entries, build_entries of opt_tables.cpp line for line - and leaves it in LDS.  After one barrier the block's
// threads run over the flat (cell, g) index of the tile, so any ng keeps every lane busy and a wave reads the entries of at most
// a few cells (an LDS broadcast per cell).  Per (cell, g): one FMA chain per gas over its 4 or 8 entries, in build_entries' node
// order; the total is the sum of the gases' chains in model order; the stores are consecutive over the tile.  No atomics, and
// nothing a cell computes depends on the batch, the tile or the grid.
#include "gas_optics_device.hpp"

#include <memory>
#include <string>

namespace go = ecckd::gas_optics;

namespace {

// the model and the call as the kernels read them, cell_entries, chain4, put, planck_value: gas_optics_device.hpp
using go::GoModel; using go::GoCall; using go::cell_entries; using go::chain4; using go::put; using go::planck_value;

constexpr int CELLS = go::CELLS_PER_BLOCK, THREADS = go::THREADS;

template <bool F32, bool PER_GAS>
__global__ __launch_bounds__(THREADS) void k_gas_optics(const GoModel m, const GoCall c) {
#pragma clang fp contract(off)
  extern __shared__ double s_mem[];
  const int nent = m.nent, ng = m.ng;
  double* s_coef = s_mem;                                  // [CELLS][nent]
  double* s_moles = s_coef + (size_t)CELLS * nent;         // [CELLS]
  uint32_t* s_idx = (uint32_t*)(s_moles + CELLS);          // [CELLS][nent]
  const size_t cell0 = (size_t)blockIdx.x * CELLS;
  const unsigned ncl = (unsigned)(c.ncell - cell0 < (size_t)CELLS ? c.ncell - cell0 : (size_t)CELLS);
  const unsigned t = threadIdx.x;
  if (t < ncl) cell_entries(m, c, cell0 + t, s_coef + (size_t)t * nent, s_idx + (size_t)t * nent, s_moles + t);
  __syncthreads();
  const unsigned nitem = ncl * (unsigned)ng;               // <= 64 * 1024
  unsigned cl = t / (unsigned)ng, g = t % (unsigned)ng;
  const unsigned dcl = THREADS / (unsigned)ng, dg = THREADS % (unsigned)ng;
  const size_t out0 = cell0 * (size_t)ng;
  for (unsigned j = t; j < nitem; j += THREADS) {
    const double* coef = s_coef + (size_t)cl * nent;
    const uint32_t* idx = s_idx + (size_t)cl * nent;
    const double* kg = m.k + g;
    const size_t o = out0 + j;
    double total = 0.0;
    for (int i = 0; i < m.ngas; ++i) {
      double part = 0.0;
      if ((c.present >> i) & 1u) {
        const int e0 = m.gases[i].ent0;
        part = chain4(kg, coef + e0, idx + e0, part);
        if (m.gases[i].nent == 8) part = chain4(kg, coef + e0 + 4, idx + e0 + 4, part);
        total += part;
      }
      if (PER_GAS) {
        void* out = c.gas_od[i];
        if (out) put<F32>(out, o, (!c.keep_negative && part < 0.0) ? 0.0 : part);
      }
    }
    if (c.od) put<F32>(c.od, o, (!c.keep_negative && total < 0.0) ? 0.0 : total);
    // CkdModel::calc_rayleigh_optical_depth (ckd_model.h:242-252); zeros without coefficients, as run_ckd writes
    if (c.ray_od) put<F32>(c.ray_od, o, m.rayleigh ? s_moles[cl] * m.rayleigh[g] : 0.0);
    g += dg;
    cl += dcl;
    if (g >= (unsigned)ng) { g -= (unsigned)ng; ++cl; }
  }
}

// planck_lut of opt_tables.cpp (CkdModel::calc_planck_function, ckd_model.cpp:1121-1145) per (temperature, g)
template <bool F32>
__global__ __launch_bounds__(256) void k_gas_optics_planck(int ntp, const double* tpl, const double* pf, int ng, size_t n,
                                                           const double* temperature, void* out) {
#pragma clang fp contract(off)
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n * (size_t)ng) return;
  const size_t i = j / (size_t)ng;
  const size_t g = j - i * (size_t)ng;
  const double v = planck_value(ntp, tpl, pf, ng, g, temperature[i]);
  put<F32>(out, j, v);
}

void go_free(ecckd_gas_optics* h) {
  if (!h) return;
  if (h->ctx) (void)hipStreamSynchronize(h->ctx->stream);
  for (void* p : h->blocks) ecckd::dev_release(h->ctx, p);
  delete h;
}
struct GoDelete { void operator()(ecckd_gas_optics* h) const { go_free(h); } };

template <bool F32, bool PER_GAS>
int launch(ecckd_gas_optics* h, const go::Plan& plan, const GoModel& m, const GoCall& c) {
  const auto kernel = k_gas_optics<F32, PER_GAS>;
  if (plan.lds_bytes > 48 * 1024)
    ECCKD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds_bytes));
  hipLaunchKernelGGL(kernel, dim3(plan.blocks), dim3(plan.threads), plan.lds_bytes, h->ctx->stream, m, c);
  ECCKD_HIP_CHECK(hipGetLastError());
  return ECCKD_OK;
}

}  // namespace

extern "C" {

int ecckd_gas_optics_create(ecckd_ctx* ctx, const ecckd_opt_model* model, ecckd_gas_optics** out) {
  ECCKD_REQUIRE(ctx && model && out, "ecckd_gas_optics_create: NULL argument");
  *out = nullptr;
  std::unique_ptr<ecckd_gas_optics, GoDelete> h(new ecckd_gas_optics);
  h->ctx = ctx;
  std::string err;
  const int rc = go::flatten_model(model, h->f, err);
  if (rc != ECCKD_OK) return ecckd::fail(rc, "%s", err.c_str());
  ECCKD_HIP_CHECK(hipSetDevice(ctx->device));
  go::Flat& f = h->f;
  ECCKD_CHECK(h->upload(&h->d_k, f.k));
  ECCKD_CHECK(h->upload(&h->d_gases, f.gases));
  ECCKD_CHECK(h->upload(&h->d_temperature, f.temperature));
  if (!f.is_sw) {
    ECCKD_CHECK(h->upload(&h->d_tpl, f.temperature_planck));
    ECCKD_CHECK(h->upload(&h->d_planck, f.planck_function));
  }
  if (f.has_rayleigh) ECCKD_CHECK(h->upload(&h->d_rayleigh, f.rayleigh));
  if (f.is_sw) ECCKD_CHECK(h->upload(&h->d_solar, f.solar_irradiance));      // the fused fluxes form incoming_sw per g point
  if (f.nband > 0) ECCKD_CHECK(h->upload(&h->d_iband, f.iband));
  // (the sources are pageable vectors: the copies have left them when the stream has drained)
  ECCKD_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  for (std::vector<double>* v : {&f.k, &f.temperature, &f.planck_function}) std::vector<double>().swap(*v);
  *out = h.release();
  return ECCKD_OK;
}

int ecckd_gas_optics_destroy(ecckd_gas_optics* h) {
  go_free(h);
  return ECCKD_OK;
}

int ecckd_gas_optics_info(ecckd_gas_optics* h, int* ng, int* ngas, int* is_sw, int* entries_per_cell) {
  ECCKD_REQUIRE(h, "ecckd_gas_optics_info: handle is NULL");
  if (ng) *ng = h->f.ng;
  if (ngas) *ngas = h->f.ngas;
  if (is_sw) *is_sw = h->f.is_sw ? 1 : 0;
  if (entries_per_cell) *entries_per_cell = h->f.nent;
  return ECCKD_OK;
}

int ecckd_gas_optics_geometry(ecckd_gas_optics* h, int* cells_per_block, int* threads) {
  ECCKD_REQUIRE(h, "ecckd_gas_optics_geometry: handle is NULL");
  if (cells_per_block) *cells_per_block = go::CELLS_PER_BLOCK;
  if (threads) *threads = go::THREADS;
  return ECCKD_OK;
}

int ecckd_gas_optics_dev(ecckd_gas_optics* h, int ncol, int nlay, const double* d_pressure_hl, const double* d_temperature_hl,
                         const double* d_temperature_fl, const double* d_vmr_fl, const int* h_gas_present,
                         const double* h_gas_scaling, int keep_negative, int out_type, void* d_od, void* const* h_d_gas_od,
                         void* d_rayleigh_od) {
  ECCKD_REQUIRE(h, "ecckd_gas_optics_dev: handle is NULL");
  const go::Flat& f = h->f;
  const go::CallArgs a = {ncol, nlay, d_pressure_hl != nullptr, d_temperature_hl != nullptr, d_vmr_fl != nullptr, d_od != nullptr,
                          d_rayleigh_od != nullptr, h_gas_present, h_gas_scaling, (const void* const*)h_d_gas_od, keep_negative, out_type};
  std::string err;
  uint32_t present = 0;
  bool any_gas_od = false;
  go::Plan plan;
  int rc = go::check_call(f, a, present, any_gas_od, err);
  if (rc == ECCKD_OK) rc = go::launch_plan(ncol, nlay, f.ng, f.nent, plan, err);
  if (rc != ECCKD_OK) return ecckd::fail(rc, "%s", err.c_str());
  const GoModel m = {h->d_k, h->d_temperature, h->d_rayleigh, h->d_gases, f.log_p_0, f.d_log_p, f.d_t, f.ng, f.nt, f.np, f.ngas, f.nent};
  GoCall c{};
  c.p_hl = d_pressure_hl; c.t_hl = d_temperature_hl; c.t_fl = d_temperature_fl; c.vmr = d_vmr_fl;
  c.od = d_od; c.ray_od = d_rayleigh_od;
  for (int i = 0; i < f.ngas; ++i) {
    c.gas_od[i] = h_d_gas_od ? h_d_gas_od[i] : nullptr;
    c.scaling[i] = h_gas_scaling ? h_gas_scaling[i] : 1.0;
  }
  c.ncell = plan.ncell; c.present = present; c.nlay = nlay; c.keep_negative = keep_negative;
  ECCKD_HIP_CHECK(hipSetDevice(h->ctx->device));
  const bool f32 = out_type == ECCKD_F32;
  if (f32) return any_gas_od ? launch<true, true>(h, plan, m, c) : launch<true, false>(h, plan, m, c);
  return any_gas_od ? launch<false, true>(h, plan, m, c) : launch<false, false>(h, plan, m, c);
}

int ecckd_gas_optics_planck_dev(ecckd_gas_optics* h, size_t n, const double* d_temperature, int out_type, void* d_planck) {
  ECCKD_REQUIRE(h, "ecckd_gas_optics_planck_dev: handle is NULL");
  ECCKD_REQUIRE(!h->f.is_sw, "ecckd_gas_optics_planck_dev: a shortwave handle has no Planck look-up table");
  ECCKD_REQUIRE(n > 0 && d_temperature && d_planck, "ecckd_gas_optics_planck_dev: NULL or empty argument");
  ECCKD_REQUIRE(out_type == ECCKD_F64 || out_type == ECCKD_F32, "ecckd_gas_optics_planck_dev: out_type %d is neither ECCKD_F32 nor ECCKD_F64",
                out_type);
  const size_t blocks = (n * (size_t)h->f.ng + 255) / 256;
  ECCKD_REQUIRE(blocks <= (size_t)0x7fffffff, "ecckd_gas_optics_planck_dev: %zu temperatures are more than one launch holds", n);
  ECCKD_HIP_CHECK(hipSetDevice(h->ctx->device));
  const auto kernel = out_type == ECCKD_F32 ? k_gas_optics_planck<true> : k_gas_optics_planck<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, h->ctx->stream, h->f.ntp, h->d_tpl, h->d_planck, h->f.ng, n,
                     d_temperature, d_planck);
  ECCKD_HIP_CHECK(hipGetLastError());
  return ECCKD_OK;
}

int ecckd_gas_optics_incoming(ecckd_gas_optics* h, double tsi, double* h_incoming) {
  ECCKD_REQUIRE(h && h_incoming, "ecckd_gas_optics_incoming: NULL argument");
  ECCKD_REQUIRE(h->f.is_sw, "ecckd_gas_optics_incoming: a longwave handle has no solar irradiance");
  go::incoming(h->f, tsi, h_incoming);
  return ECCKD_OK;
}

}  // extern "C"
