// gas_optics.hip - the resident gas-optics handle: a CKD model uploaded once and applied to atmospheric columns that already sit
// in device memory (CkdModel::calc_optical_depth, ckd_model.cpp:925-1102, and calc_planck_function, :1107-1145).  The host step
// (flattening the model, the refusals, the launch plan) is gas_optics_tables.cpp.
//
// k_gas_optics: a block takes a tile of CELLS_PER_BLOCK consecutive cells of the flattened (column, layer) index.  One lane per
// cell forms what all g points of the cell share - the three axis positions, their logarithms and the cell's (table row,
// coefficient) entries, build_entries of opt_tables.cpp line for line - and leaves it in LDS.  After one barrier the block's
// threads run over the flat (cell, g) index of the tile, so any ng keeps every lane busy and a wave reads the entries of at most
// a few cells (an LDS broadcast per cell).  Per (cell, g): one FMA chain per gas over its 4 or 8 entries, in build_entries' node
// order; the total is the sum of the gases' chains in model order; the stores are consecutive over the tile.  No atomics, and
// nothing a cell computes depends on the batch, the tile or the grid.
#include "common.hpp"
#include "gas_optics_tables.hpp"
#include "opt_tables.hpp"

#include <memory>
#include <string>

namespace go = ecckd::gas_optics;

namespace {

constexpr int CELLS = go::CELLS_PER_BLOCK, THREADS = go::THREADS;
constexpr double MOLES_PER_PA = ecckd::opt_tables::MOLES_PER_PA;

struct GoModel {
  const double* k;
  const double* temperature;    // [nt][np]; the temperature axis hangs on row 0
  const double* rayleigh;       // [ng] or NULL
  const go::GasDesc* gases;
  double log_p_0, d_log_p, d_t;
  int ng, nt, np, ngas, nent;
};

struct GoCall {
  const double *p_hl, *t_hl, *t_fl, *vmr;
  void* od;
  void* ray_od;
  void* gas_od[go::MAX_GASES];
  double scaling[go::MAX_GASES];
  size_t ncell;
  uint32_t present;
  int nlay, keep_negative;
};

struct AxisPos { int i0; double w0, w1; };

// opt_tables.cpp axis_pos: the position on an evenly spaced axis of n nodes, held inside it
__device__ inline AxisPos axis_pos(double index0, int n) {
#pragma clang fp contract(off)
  index0 = fmax(0.0, fmin(index0, n - 1.0001));
  const int i0 = (int)index0;
  const double w1 = index0 - i0;
  return {i0, 1.0 - w1, w1};
}

// One cell's entries: opt_tables.cpp build_entries, with run_ckd's rule for absent gases (the caller skips them: their slots
// are never read).  No contraction, so that every product and sum rounds as the host's.
__device__ inline void cell_entries(const GoModel& m, const GoCall& c, size_t cell, double* coef, uint32_t* idx, double* moles) {
#pragma clang fp contract(off)
  const size_t col = cell / (size_t)c.nlay;
  const int l = (int)(cell - col * (size_t)c.nlay);
  const double* p = c.p_hl + col * (size_t)(c.nlay + 1);
  const double* T = c.t_hl + col * (size_t)(c.nlay + 1);
  const double p0 = p[l], p1 = p[l + 1];
  const double t_fl = c.t_fl ? c.t_fl[cell] : (T[l] * p0 + T[l + 1] * p1) / (p0 + p1);
  const double log_pressure_fl = log(0.5 * (p1 + p0));
  const AxisPos ap = axis_pos((log_pressure_fl - m.log_p_0) / m.d_log_p, m.np);
  const double t_0 = ap.w0 * m.temperature[ap.i0] + ap.w1 * m.temperature[ap.i0 + 1];
  const AxisPos at = axis_pos((t_fl - t_0) / m.d_t, m.nt);
  const double simple_weight = MOLES_PER_PA * (p1 - p0);
  *moles = simple_weight;
  for (int i = 0; i < m.ngas; ++i) {
    if (!((c.present >> i) & 1u)) continue;
    const go::GasDesc gd = m.gases[i];
    double weight = simple_weight, vm = 0.0;
    if (gd.conc != 0) {
      vm = c.vmr[(col * (size_t)m.ngas + (size_t)i) * (size_t)c.nlay + (size_t)l] * c.scaling[i];
      weight = (gd.conc == 3) ? simple_weight * (vm - gd.reference_vmr) : simple_weight * vm;
    }
    AxisPos ac = {0, 1.0, 1.0};
    if (gd.conc == 2) ac = axis_pos((log(vm) - gd.log_vmr0) / gd.d_log_c, gd.nconc);
    const int nc = gd.conc == 2 ? 2 : 1;
    int q = gd.ent0;
    for (int dc = 0; dc < nc; ++dc)
      for (int dt = 0; dt < 2; ++dt)
        for (int dp = 0; dp < 2; ++dp) {
          const uint32_t node = ((uint32_t)(ac.i0 + dc) * (uint32_t)m.nt + (uint32_t)(at.i0 + dt)) * (uint32_t)m.np + (uint32_t)(ap.i0 + dp);
          idx[q] = gd.ix + node * (uint32_t)m.ng;
          coef[q] = weight * (dc ? ac.w1 : ac.w0) * (dt ? at.w1 : at.w0) * (dp ? ap.w1 : ap.w0);
          ++q;
        }
  }
}

template <bool F32>
__device__ inline void put(void* out, size_t i, double v) {
  if (F32) ((float*)out)[i] = (float)v;
  else ((double*)out)[i] = v;
}

// four entries of a chain: the loads go out together, the FMAs follow in entry order
__device__ inline double chain4(const double* kg, const double* coef, const uint32_t* idx, double acc) {
  const double k0 = kg[idx[0]], k1 = kg[idx[1]], k2 = kg[idx[2]], k3 = kg[idx[3]];
  acc = fma(coef[0], k0, acc);
  acc = fma(coef[1], k1, acc);
  acc = fma(coef[2], k2, acc);
  return fma(coef[3], k3, acc);
}

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
  const double t = temperature[i];
  const double d_t = tpl[1] - tpl[0], t0 = tpl[0];
  const double tindex0 = (t - t0) / d_t;
  double v;
  if (tindex0 >= 0) {
    const int it0 = min((int)tindex0, ntp - 2);
    const double w1 = tindex0 - it0, w0 = 1.0 - w1;
    v = w0 * pf[(size_t)it0 * ng + g] + w1 * pf[(size_t)(it0 + 1) * ng + g];
  } else {
    v = (t / t0) * pf[g];
  }
  put<F32>(out, j, v);
}

}  // namespace

struct ecckd_gas_optics {
  ecckd_ctx* ctx = nullptr;
  go::Flat f;                       // the model's small arrays; the tables themselves live on the device only
  std::vector<void*> blocks;        // every device block of the handle, from the context's allocator
  double *d_k = nullptr, *d_temperature = nullptr, *d_tpl = nullptr, *d_planck = nullptr, *d_rayleigh = nullptr;
  go::GasDesc* d_gases = nullptr;
  template <typename T> int upload(T** d, const std::vector<T>& h) {
    void* v = nullptr;
    ECCKD_HIP_CHECK(ecckd::dev_malloc(ctx, &v, std::max<size_t>(h.size(), 1) * sizeof(T)));
    blocks.push_back(v);
    *d = (T*)v;
    if (!h.empty()) ECCKD_HIP_CHECK(hipMemcpyAsync(v, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return ECCKD_OK;
  }
};

namespace {

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
