// ASan/UBSan harness for the host arithmetic of the g-point map (csrc/gmap_layout.hpp, which has no HIP in it and is included as
// it is).  The chunking: for the g-point counts of LAYOUTS in tests/create_lut_cases.py (EDGE, STRIDE, NONE_ONLY) the chunks per g
// point are those of CHUNKS there, every chunk lies inside its segment, holds at most GA_CHUNK positions and begins where the
// one before it ended.  The work buffer: for nchunk 0 / 1 / 8 / 260 x ng 1 / 8 / 38 x n 1 / 3 / 54 / 231 / 326 every call's total
// is the formula that tests/create_lut_cases.py::work_bytes restates (written out below, not taken from the header), and every
// piece begins on a 256-byte boundary behind the piece before it.
// build: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iecckd_amd/csrc
//        tools/check_gmap_layout.cpp -o /tmp/check_gmap_layout && /tmp/check_gmap_layout
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "gmap_layout.hpp"
namespace gl = ecckd::gmap_layout;

#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    if (!(cond)) { std::printf("%s:%d: %s does not hold (%s)\n", __FILE__, __LINE__, #cond, what); std::exit(1); } \
  } while (0)

static char what[128] = "";

static void check_chunks(const char* name, const std::vector<long long>& counts, const std::vector<int>& want) {
  std::snprintf(what, sizeof what, "%s", name);
  const int ng = (int)counts.size();
  std::vector<long long> seg_begin(ng + 1, 0);
  for (int g = 0; g < ng; ++g) seg_begin[g + 1] = seg_begin[g] + counts[g];
  std::vector<ecckd::GmapChunk> chunks(3);        // what a map held before is replaced
  std::vector<int> seg_chunk0(1, 7);
  gl::cut_chunks(seg_begin, chunks, seg_chunk0);
  REQUIRE((int)seg_chunk0.size() == ng + 1 && (int)want.size() == ng);
  REQUIRE(seg_chunk0[0] == 0 && seg_chunk0[ng] == (int)chunks.size());
  for (int g = 0; g < ng; ++g) {
    REQUIRE(seg_chunk0[g + 1] - seg_chunk0[g] == want[g]);
    long long next = seg_begin[g];
    for (int c = seg_chunk0[g]; c < seg_chunk0[g + 1]; ++c) {
      const ecckd::GmapChunk& k = chunks[c];
      REQUIRE(k.g == g && k.pad == 0);
      REQUIRE(k.p0 == next && k.p1 >= k.p0 && k.p1 < seg_begin[g + 1]);
      REQUIRE(k.p1 - k.p0 + 1 <= gl::GA_CHUNK);
      REQUIRE(k.p1 - k.p0 + 1 == gl::GA_CHUNK || c + 1 == seg_chunk0[g + 1]);     // only the last one is short
      next = k.p1 + 1;
    }
    REQUIRE(next == seg_begin[g + 1]);
  }
}

static size_t up(size_t n) { return (n + 255) / 256 * 256; }

template <size_t N>
static void check_pieces(const size_t (&bytes)[N], size_t want_total) {
  size_t off[N];
  const size_t total = gl::carve(bytes, off);
  REQUIRE(total == want_total && total % 256 == 0);
  size_t end = 0;
  for (size_t i = 0; i < N; ++i) {
    REQUIRE(bytes[i] > 0 && off[i] % 256 == 0 && off[i] >= end);
    end = off[i] + bytes[i];
  }
  REQUIRE(end <= total);
}

int main() {
  const long long C = gl::GA_CHUNK, L = 64;
  REQUIRE(gl::GA_THREADS == 256 && gl::GA_PPT == 8 && C == 2048);
  check_chunks("EDGE", {0, 1, C - 1, C, C + 1, 2 * C, 2 * C + 1, 0}, {0, 1, 1, 1, 2, 2, 3, 0});
  check_chunks("STRIDE", {L * C - 1, L * C, L * C + 1, (L + 1) * C + 1, 3}, {64, 64, 65, 66, 1});
  check_chunks("NONE_ONLY", {0, 0, 0}, {0, 0, 0});

  for (size_t nchunk : {0, 1, 8, 260})
    for (int ng : {1, 8, 38})
      for (int n : {1, 3, 54, 231, 326}) {
        std::snprintf(what, sizeof what, "nchunk %zu, ng %d, n %d", nchunk, ng, n);
        const size_t nc = nchunk > 0 ? nchunk : 1, sn = (size_t)n, sg = (size_t)ng;
        check_pieces(gl::average(nchunk, ng, n).bytes, up(nc * sn * 6 * 8) + up(3 * sn * sg * 8) + up(sn * (2 * 8 + 4)));
        check_pieces(gl::planck_lut(nchunk, ng, n).bytes, up(nc * sn * 8) + up(sn * sg * 8) + up(sn * 8));
        // ecckd_gmap_sum_rows; the erythemal weights are its case n = 2
        check_pieces(gl::rows(nchunk, ng, n).bytes, up(nc * sn * 8) + up(sn * sg * 8));
        check_pieces(gl::fraction(nchunk, ng, n).bytes, up(sg * (sn + 1) * 8) + 2 * up(sn * 8) + up(nc * 8));
      }
  std::printf("check_gmap_layout: ok\n");
  return 0;
}
