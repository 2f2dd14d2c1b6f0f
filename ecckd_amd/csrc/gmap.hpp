// gmap.hpp - the g-point map handle (ecckd_gmap) as the translation units that work on it see it:
// create_lut.hip owns it (creation, the segmented reductions over the g-sorted permutation), lbl_gpoint_fluxes.hip
// walks the spectrum in natural order and needs the map per wavenumber.
#pragma once
#include "common.hpp"

#include <vector>

namespace ecckd {
struct GmapChunk { long long p0, p1; int g; int pad; };
}  // namespace ecckd

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
  long long* d_seg_count = nullptr;
  long long* d_seg_begin = nullptr;
  void* work = nullptr;
  size_t work_bytes = 0;
  // the map in natural (wavenumber) order, rebuilt from the sorted arrays on first use (ecckd::gmap_natural)
  int32_t* nat_g = nullptr;   // [n] g point of each wavenumber, -1 = unassigned
  double* nat_wn = nullptr;   // [n]
  double* nat_dwn = nullptr;  // [n]
};

namespace ecckd {
// Device arrays [n] in wavenumber order: g point (-1 = none), wavenumber, d_wavenumber.  Owned by the map.
int gmap_natural(ecckd_gmap* m, const int32_t** d_g_point, const double** d_wavenumber, const double** d_d_wavenumber);
}  // namespace ecckd
