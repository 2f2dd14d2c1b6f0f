// gmap.hpp - the g-point map handle (ecckd_gmap) as the translation units that work on it see it:
// create_lut.hip owns it (creation, the segmented reductions over the g-sorted permutation), lbl_gpoint_fluxes.hip and
// lbl_gpoint_fluxes_sw.hip walk the spectrum in natural order and need the map per wavenumber.  The chunking of the
// segments and the sizes of the work buffer: gmap_layout.hpp.
#pragma once
#include "common.hpp"
#include "gmap_layout.hpp"

#include <vector>

struct ecckd_gmap {
  ecckd_ctx* ctx = nullptr;
  size_t n = 0;          // wavenumbers
  size_t nassigned = 0;  // with g >= 0
  int ng = 0;
  int32_t* order = nullptr;   // [n] original index of each sorted position
  double* wn_s = nullptr;     // [n]
  double* dwn_s = nullptr;    // [n]
  std::vector<long long> seg_begin;  // [ng+1] in sorted positions
  std::vector<ecckd::GmapChunk> chunks;
  std::vector<int> seg_chunk0;       // [ng+1]
  ecckd::GmapChunk* d_chunks = nullptr;
  int* d_seg_chunk0 = nullptr;
  long long* d_seg_begin = nullptr;
  // per-call work buffer, grown on demand (gmap_work, create_lut.hip): work_bytes > 0 only while `work` holds that many
  void* work = nullptr;
  size_t work_bytes = 0;
  // the map in natural (wavenumber) order, rebuilt from the sorted arrays on first use (ecckd::gmap_natural)
  int32_t* nat_g = nullptr;   // [n] g point of each wavenumber, -1 = unassigned
  double* nat_wn = nullptr;   // [n]
  double* nat_dwn = nullptr;  // [n]
  // Every device block of the map comes from alloc() (hipMalloc), which records it; gmap_free (create_lut.hip) releases what
  // is recorded, give_back() one block early.  The named members above are views for the launch sites.
  std::vector<void*> blocks;
  template <typename T> hipError_t alloc(T** p, size_t bytes) {
    void* v = nullptr;
    const hipError_t e = hipMalloc(&v, bytes);
    if (e == hipSuccess) blocks.push_back(v);
    *p = (T*)v;
    return e;
  }
  template <typename T> hipError_t give_back(T*& p) {
    hipError_t e = hipSuccess;
    for (void*& b : blocks)
      if (b && b == (void*)p) { e = hipFree(b); b = blocks.back(); blocks.pop_back(); break; }
    p = nullptr;
    return e;
  }
};

namespace ecckd {
// Device arrays [n] in wavenumber order: g point (-1 = none), wavenumber, d_wavenumber.  Owned by the map.
int gmap_natural(ecckd_gmap* m, const int32_t** d_g_point, const double** d_wavenumber, const double** d_d_wavenumber);
}  // namespace ecckd
