// gmap_layout.hpp - the host arithmetic of the g-point map (create_lut.hip), written once: how the segments of the g-sorted
// order are cut into chunks, and what every entry point asks of the map's work buffer.  Plain C++ (no HIP in it):
// tools/check_gmap_layout.cpp includes it as it is; tests/create_lut_cases.py restates the chunk size and the sizes.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

namespace ecckd {

struct GmapChunk { long long p0, p1; int g; int pad; };   // sorted positions p0 .. p1 (inclusive) of g point g

namespace gmap_layout {

constexpr int GA_THREADS = 256;
constexpr int GA_PPT = 8;                       // points per thread (halves the cross-lane reductions per point)
constexpr int GA_CHUNK = GA_THREADS * GA_PPT;   // sorted positions per block

// seg_begin [ng + 1] (sorted positions) -> the chunks of every segment in order, at most GA_CHUNK positions each and none
// across a segment's end; seg_chunk0 [ng + 1]: the chunks of g point g are seg_chunk0[g] .. seg_chunk0[g + 1] - 1
inline void cut_chunks(const std::vector<long long>& seg_begin, std::vector<GmapChunk>& chunks, std::vector<int>& seg_chunk0) {
  const int ng = (int)seg_begin.size() - 1;
  chunks.clear();
  seg_chunk0.assign(ng + 1, 0);
  for (int g = 0; g < ng; ++g) {
    seg_chunk0[g] = (int)chunks.size();
    for (long long p = seg_begin[g]; p < seg_begin[g + 1]; p += GA_CHUNK)
      chunks.push_back(GmapChunk{p, std::min<long long>(p + GA_CHUNK, seg_begin[g + 1]) - 1, g, 0});
  }
  seg_chunk0[ng] = (int)chunks.size();
}

// N pieces of bytes[i] each, in order, every piece on a 256-byte boundary: off[i] is where piece i begins -> the total
template <size_t N>
inline size_t carve(const size_t (&bytes)[N], size_t (&off)[N]) {
  size_t total = 0;
  for (size_t i = 0; i < N; ++i) { off[i] = total; total += (bytes[i] + 255) / 256 * 256; }
  return total;
}

// The pieces of the work buffer per call, in bytes.  A map without a chunk still has room for one: no piece is empty.
template <size_t N> struct Pieces { size_t bytes[N]; };
constexpr size_t D = sizeof(double);
inline size_t at_least_one(size_t nchunk) { return std::max<size_t>(nchunk, 1); }
// partial [nchunk][nlay][6] | out [3][nlay][ng] | hk [nlay], dp [nlay], int layer_method [nlay]
inline Pieces<3> average(size_t nchunk, size_t ng, size_t nlay) {
  return {{at_least_one(nchunk) * nlay * 6 * D, 3 * nlay * ng * D, nlay * (2 * D + sizeof(int))}};
}
// partial [nchunk][nrows] | out [nrows][ng]: the row sums, and the erythemal pair with two rows
inline Pieces<2> rows(size_t nchunk, size_t ng, size_t nrows) { return {{at_least_one(nchunk) * nrows * D, nrows * ng * D}}; }
// the rows of the Planck table | hk [nlut]
inline Pieces<3> planck_lut(size_t nchunk, size_t ng, size_t nlut) { return {{at_least_one(nchunk) * nlut * D, nlut * ng * D, nlut * D}}; }
// width [ng][nint + 1] | wavenumber1 [nint] | wavenumber2 [nint] | chunk sums [nchunk]
inline Pieces<4> fraction(size_t nchunk, size_t ng, size_t nint) {
  return {{ng * (nint + 1) * D, nint * D, nint * D, at_least_one(nchunk) * D}};
}

}  // namespace gmap_layout
}  // namespace ecckd
