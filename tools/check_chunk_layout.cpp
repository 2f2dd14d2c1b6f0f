// ASan/UBSan harness for the chunk layout of the error sweep (csrc/chunk_layout.hpp, which has no HIP in it apart from the
// host / device marks and is included as it is).  For first indices at 0, 1 and 15 modulo 16, the lengths
// 1, 15, 16, 17, 127, 128, 129, 2 * 128, L0 - 1, L0, L0 + 1, L0 + 129 (L0 = target_blocks * 128: the longest interval whose
// chunk is one granule) and rounds of 3 and of 768 blocks:
//   * every point of [i1, i2] lies in exactly one chunk: the chunks are not empty, the first begins at i1, each begins where
//     the one before it ended, the last ends at i2 (and, counted point by point, every point is met once);
//   * aligned: every chunk's tiles begin on a multiple of 16, so does every chunk but the first; only the first chunk has
//     points below its first one, head = i1 mod 16 of them;
//   * the chunk count is at most target_blocks (+ 1 allowed where the head pushes it over: it never does, the chunk size is
//     chosen for len + head) and at most the 32 * COST_GROUPS chunks the cost kernels have room for;
//   * not aligned: the layout is the one written out below - chunks of the smallest multiple of the granule with at most
//     target_blocks chunks, counted from i1 -, for granules of 128 and 256 points.
// build: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iecckd_amd/csrc
//        tools/check_chunk_layout.cpp -o /tmp/check_chunk_layout && /tmp/check_chunk_layout
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "chunk_layout.hpp"
namespace cl = ecckd::chunk_layout;

static char what[160] = "";

#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    if (!(cond)) { std::printf("%s:%d: %s does not hold (%s)\n", __FILE__, __LINE__, #cond, what); std::exit(1); } \
  } while (0)

static long long check_cover(long long i1, long long i2, const cl::Layout& L, bool aligned) {
  const long long len = i2 - i1 + 1;
  std::vector<unsigned char> met((size_t)len, 0);
  long long next = i1;
  for (long long c = 0; c < L.nchunks; ++c) {
    const cl::Span s = cl::chunk_span(i1, i2, L.chunk_pts, L.head, c);
    REQUIRE(s.p0 == next && s.p1 >= s.p0 && s.p1 <= i2);
    REQUIRE(s.base <= s.p0 && s.p0 - s.base == (c == 0 ? L.head : 0));
    REQUIRE(s.p1 == i2 || s.p1 == s.base + L.chunk_pts - 1);                  // only the last chunk is cut short
    if (aligned) REQUIRE(s.base % 16 == 0 && (c == 0 || s.p0 % 16 == 0));
    for (long long i = s.p0; i <= s.p1; ++i) met[(size_t)(i - i1)] += 1;
    next = s.p1 + 1;
  }
  REQUIRE(next == i2 + 1);
  for (long long i = 0; i < len; ++i) REQUIRE(met[(size_t)i] == 1);
  return L.nchunks;
}

int main() {
  REQUIRE(cl::LINE_PTS == 16 && cl::COST_GROUPS == 64);
  const long long G = 128;
  int cases = 0;
  for (long long blocks : {3LL, 768LL}) {
    REQUIRE(blocks <= 32 * cl::COST_GROUPS);
    const long long L0 = blocks * G;
    for (long long i1 : {4320LL, 4321LL, 4335LL, 0LL, 1LL, 15LL}) {
      for (long long len : {1LL, 15LL, 16LL, 17LL, 127LL, 128LL, 129LL, 2 * G, L0 - 1, L0, L0 + 1, L0 + 129}) {
        const long long i2 = i1 + len - 1;
        std::snprintf(what, sizeof what, "blocks %lld, i1 %lld, len %lld, aligned", blocks, i1, len);
        const cl::Layout a = cl::of_interval(i1, i2, blocks, G, true);
        REQUIRE(a.head == i1 % 16 && a.chunk_pts % G == 0 && a.chunk_pts >= G);
        REQUIRE(a.chunk_pts == cl::interval_chunk_pts(len + a.head, blocks, G));
        REQUIRE(a.nchunks == (len + a.head + a.chunk_pts - 1) / a.chunk_pts);
        const long long na = check_cover(i1, i2, a, true);
        REQUIRE(na >= 1 && na <= blocks + 1 && na <= 32 * cl::COST_GROUPS);
        REQUIRE(na <= blocks);                                                  // in fact the head never pushes it over
        // the head costs at most one granule per chunk: no smaller multiple of G would do for len + head points
        REQUIRE(a.chunk_pts == G || (a.chunk_pts - G) * blocks < len + a.head);

        for (long long gran : {128LL, 256LL}) {
          std::snprintf(what, sizeof what, "blocks %lld, i1 %lld, len %lld, gran %lld, not aligned", blocks, i1, len, gran);
          const cl::Layout u = cl::of_interval(i1, i2, blocks, gran, false);
          // the layout before there was a head, written out: per_block = ceil(len / blocks), chunk = that rounded up to gran
          long long want = (len + blocks - 1) / blocks;
          want = (want + gran - 1) / gran * gran;
          if (want < gran) want = gran;
          REQUIRE(u.head == 0 && u.chunk_pts == want && u.nchunks == (len + want - 1) / want);
          for (long long c = 0; c < u.nchunks; ++c) {
            const cl::Span s = cl::chunk_span(i1, i2, u.chunk_pts, u.head, c);
            REQUIRE(s.base == i1 + c * want && s.p0 == s.base);
            REQUIRE(s.p1 == (s.base + want - 1 < i2 ? s.base + want - 1 : i2));
          }
          const long long nu = check_cover(i1, i2, u, false);
          REQUIRE(nu <= blocks && nu <= 32 * cl::COST_GROUPS);
        }
        // an interval that starts on a line has the same layout either way
        if (i1 % 16 == 0) {
          const cl::Layout u = cl::of_interval(i1, i2, blocks, G, false);
          REQUIRE(u.chunk_pts == a.chunk_pts && u.head == a.head && u.nchunks == a.nchunks);
        }
        ++cases;
      }
    }
  }
  // where the head does change the layout: L0 points from i1 = 1 (mod 16) no longer fit into chunks of one granule
  {
    std::snprintf(what, sizeof what, "the head moves the step from one granule to two");
    const cl::Layout a = cl::of_interval(4321, 4321 + 3 * G - 1, 3, G, true), u = cl::of_interval(4321, 4321 + 3 * G - 1, 3, G, false);
    REQUIRE(u.chunk_pts == G && u.nchunks == 3 && a.chunk_pts == 2 * G && a.nchunks == 2 && a.head == 1);
  }
  std::printf("check_chunk_layout: ok (%d intervals)\n", cases);
  return 0;
}
