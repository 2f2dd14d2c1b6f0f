// ASan/UBSan harness for the line-blocked layout of the longwave sweep's operands (csrc/sweep_layout.hpp, which has no HIP
// in it apart from the host / device marks and is included as it is).  For matrices of 55, 54, 27, 31 and 1 rows and
// n = 16, 32 and 16 * 37 points, against the layout written out by brute force (a counter walked through
// [n / 16][rows][16]):
//   * the map (row, point) -> byte offset is a bijection onto the 8-byte slots of [0, bytes): every offset is a multiple
//     of 8 below bytes(rows, n), and a blocked matrix filled through the map holds every element exactly once;
//   * offset(rows, r, i) = point_base(rows, i) + r * 128: a row is a constant away from the lane's base;
//   * a 64-point tile that starts on a line is four contiguous blocks: in each of them the rows r0 .. r1 of the 16 points
//     are (r1 - r0 + 1) * 128 consecutive bytes in ascending (row, point) order, and the blocks lie rows * 128 bytes apart;
//   * the 32-bit condition holds at 7.2e6 x 55 and fails at 16 * 600 000 x 56 (and just past 2^32 bytes), where
//     offsets beyond 32 bits do exist.
// build: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iecckd_amd/csrc
//        tools/check_sweep_layout.cpp -o /tmp/check_sweep_layout && /tmp/check_sweep_layout
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sweep_layout.hpp"
namespace sl = ecckd::sweep_layout;
typedef unsigned long long u64;

static char what[160] = "";

#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    if (!(cond)) { std::printf("%s:%d: %s does not hold (%s)\n", __FILE__, __LINE__, #cond, what); std::exit(1); } \
  } while (0)

static void check_matrix(u64 rows, u64 n) {
  std::snprintf(what, sizeof what, "rows %llu, n %llu", rows, n);
  REQUIRE(sl::whole_lines(n));
  const u64 size = sl::bytes(rows, n);
  REQUIRE(size == rows * n * 8 && size % 128 == 0);
  // the brute-force reference: slot number of (r, i), counting through [n / 16][rows][16]
  std::vector<u64> want((size_t)(rows * n));
  u64 slot = 0;
  for (u64 blk = 0; blk < n / 16; ++blk)
    for (u64 r = 0; r < rows; ++r)
      for (u64 j = 0; j < 16; ++j) want[(size_t)(r * n + blk * 16 + j)] = slot++;
  REQUIRE(slot * 8 == size);
  // the blocked matrix filled through the map from a row-major one: every slot written once, with the right element
  std::vector<long long> blocked((size_t)(rows * n), -1);
  for (u64 r = 0; r < rows; ++r)
    for (u64 i = 0; i < n; ++i) {
      const u64 off = sl::offset(rows, r, i);
      REQUIRE(off % 8 == 0 && off < size);
      REQUIRE(off == want[(size_t)(r * n + i)] * 8);
      REQUIRE(off == sl::point_base(rows, i) + r * 128);
      REQUIRE(blocked[(size_t)(off / 8)] == -1);
      blocked[(size_t)(off / 8)] = (long long)(r * n + i);
    }
  for (u64 s = 0; s < rows * n; ++s) REQUIRE(blocked[(size_t)s] >= 0);
  // tiles of 64 points from a line (the last tile of a short matrix: what there is of it)
  for (u64 base = 0; base < n; base += 16) {
    const u64 pts = n - base < 64 ? n - base : 64;
    for (u64 r0 : {(u64)0, rows / 2}) {
      const u64 r1 = r0 == 0 ? (rows - 1) / 2 : rows - 1;       // the upper and the lower half column
      for (u64 q = 0; q < pts / 16; ++q) {
        const u64 first = sl::offset(rows, r0, base + q * 16);
        REQUIRE(first % 128 == 0);
        REQUIRE(first == sl::offset(rows, r0, base) + q * rows * 128);
        u64 next = first;
        for (u64 r = r0; r <= r1; ++r)
          for (u64 j = 0; j < 16; ++j, next += 8) REQUIRE(sl::offset(rows, r, base + q * 16 + j) == next);
        REQUIRE(next - first == (r1 - r0 + 1) * 128);
      }
    }
  }
}

int main() {
  REQUIRE(sl::LINE_PTS == 16 && sl::ELEM_BYTES == 8 && sl::LINE_BYTES == 128);
  int cases = 0;
  for (u64 rows : {55ULL, 54ULL, 27ULL, 31ULL, 1ULL})
    for (u64 n : {16ULL, 32ULL, 16ULL * 37}) { check_matrix(rows, n); ++cases; }
  std::snprintf(what, sizeof what, "whole lines");
  REQUIRE(!sl::whole_lines(0) && !sl::whole_lines(601) && !sl::whole_lines(15) && sl::whole_lines(592));
  // a half column of 28 rows is within the 13-bit signed immediate of a load, counted up and counted down
  REQUIRE(27 * sl::LINE_BYTES < 4096);
  std::snprintf(what, sizeof what, "32-bit condition");
  REQUIRE(sl::fits_32bit(55, 7200000) && sl::fits_32bit(54, 7200000) && sl::fits_32bit(27, 7200000));
  REQUIRE(sl::offset(55, 54, 7200000 - 1) < (1ULL << 32));
  const u64 big = 16ULL * 600000;                                   // 9.6e6 points x 56 rows = 4.3e9 bytes
  REQUIRE(sl::whole_lines(big) && !sl::fits_32bit(56, big) && sl::offset(56, 55, big - 1) >= (1ULL << 32));
  REQUIRE(sl::offset(56, 55, big - 1) == sl::bytes(56, big) - 8);   // the last element is the last slot, without wrapping
  REQUIRE(sl::fits_32bit(1, (1ULL << 29) - 16) && !sl::fits_32bit(1, 1ULL << 29) && !sl::fits_32bit(2, 1ULL << 28));
  std::printf("check_sweep_layout: ok (%d matrices)\n", cases);
  return 0;
}
