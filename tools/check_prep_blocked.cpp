// ASan/UBSan harness for the host side of the blocked-store gas preparation (csrc/sweep_layout.hpp, included as it is):
//   * gas_can_block / prep_writes_blocked / on_line: the decision ecckd_gas_create_lw takes in front of the preparation
//     kernel - 54 (and, for the copy afterwards, 30) layers, chunks counted from a line, no ECCKD_RT_ROWMAJOR, rows of
//     whole lines, 32-bit offsets; FLOAT target, not the logarithmic method, no ECCKD_BG64 for the kernel's own stores;
//   * the addresses k_gas_prep_lw_mirror<.., true> stores to, restated lane by lane: a block is two pairs of waves, a pair
//     holds 64 consecutive ranks, a lane keeps (unsigned)point_base(rows, i) and adds r * 128.  For n = 16, 1 168 and
//     4 112 and the matrices of 54 (DOUBLE background), 27 (FLOAT pairs) and 55 (Planck) rows, stored into heap blocks of
//     exactly bytes(rows, n): every store is inside its block (ASan), every element is written, with the value the
//     row-major matrix has there, level 27 of the Planck matrix by both waves of a pair, the middle pair one float from
//     each; and the 32-bit offset is the 64-bit one up to 7.2e6 points.
// build: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -Iecckd_amd/csrc
//        tools/check_prep_blocked.cpp -o /tmp/check_prep_blocked && /tmp/check_prep_blocked
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sweep_layout.hpp"
namespace sl = ecckd::sweep_layout;
typedef unsigned long long u64;

static char what[160] = "";

#define REQUIRE(cond)                                                                  \
  do {                                                                                 \
    if (!(cond)) { std::printf("%s:%d: %s does not hold (%s)\n", __FILE__, __LINE__, #cond, what); std::exit(1); } \
  } while (0)

static char* blk_row(void* base, unsigned at, int r) { return (char*)base + ((size_t)at + (size_t)r * sl::LINE_BYTES); }

// the value of (row r, point i) of a matrix: any injective map will do
static double value(u64 r, u64 i) { return (double)(r * 10000000ULL + i) + 0.25; }

static void check_stores(u64 n) {
  std::snprintf(what, sizeof what, "stores, n %llu", n);
  constexpr int NLAY = 54, H = 27;
  REQUIRE(sl::prep_writes_blocked(NLAY, true, false, false, true, false, n));
  // heap blocks of exactly the matrices' sizes: a store outside is ASan's to report
  double* bg = (double*)std::malloc((size_t)sl::bytes(NLAY, n));
  float* pairs = (float*)std::malloc((size_t)sl::bytes(H, n));
  double* planck = (double*)std::malloc((size_t)sl::bytes(NLAY + 1, n));
  REQUIRE(bg && pairs && planck);
  std::memset(bg, 0xFF, (size_t)sl::bytes(NLAY, n));
  std::memset(pairs, 0xFF, (size_t)sl::bytes(H, n));
  std::memset(planck, 0xFF, (size_t)sl::bytes(NLAY + 1, n));
  std::vector<int> planck_writes((size_t)((NLAY + 1) * n), 0);
  const u64 blocks = (n + 127) / 128;
  for (u64 b = 0; b < blocks; ++b)
    for (int wave = 0; wave < 4; ++wave)
      for (int lane = 0; lane < 64; ++lane) {
        const int half = wave & 1, pair = wave >> 1;
        const u64 i = b * 128 + (u64)pair * 64 + (u64)lane;
        const bool live = i < n;
        const u64 ii = live ? i : n - 1;
        const unsigned at_bg = (unsigned)sl::point_base(NLAY, ii), at_pr = (unsigned)sl::point_base(H, ii);
        const unsigned at_pl = (unsigned)sl::point_base(NLAY + 1, ii);
        if (!live) continue;
        const int lev_near = half ? NLAY : 0;
        *(double*)blk_row(planck, at_pl, lev_near) = value((u64)lev_near, i);
        planck_writes[(size_t)((u64)lev_near * n + i)] += 1;
        for (int l = 0; l < H; ++l) {
          const int L = half ? NLAY - 1 - l : l;
          const int lev_far = half ? L : L + 1;
          *(double*)blk_row(bg, at_bg, L) = value((u64)L, i);
          float* pr = (float*)blk_row(pairs, at_pr, L / 2);
          if (l & 1) {
            pr[0] = (float)(2 * (L / 2));
            pr[1] = (float)(2 * (L / 2) + 1);
          } else if (l == H - 1) {
            pr[L & 1] = (float)L;
          }
          *(double*)blk_row(planck, at_pl, lev_far) = value((u64)lev_far, i);
          planck_writes[(size_t)((u64)lev_far * n + i)] += 1;
        }
      }
  for (u64 i = 0; i < n; ++i) {
    for (u64 r = 0; r < NLAY; ++r) REQUIRE(bg[sl::offset(NLAY, r, i) / 8] == value(r, i));
    for (u64 r = 0; r <= NLAY; ++r) {
      REQUIRE(planck[sl::offset(NLAY + 1, r, i) / 8] == value(r, i));
      REQUIRE(planck_writes[(size_t)(r * n + i)] == (r == H ? 2 : 1));
    }
    for (u64 p = 0; p < H; ++p) {
      const float* pr = pairs + sl::offset(H, p, i) / 4;
      REQUIRE(pr[0] == (float)(2 * p) && pr[1] == (float)(2 * p + 1));
    }
  }
  std::free(bg);
  std::free(pairs);
  std::free(planck);
}

int main() {
  std::snprintf(what, sizeof what, "decision");
  // gas_can_block(nlay, chunks_from_line, rowmajor_knob, n)
  REQUIRE(sl::gas_can_block(54, true, false, 16) && sl::gas_can_block(30, true, false, 1168) && sl::gas_can_block(54, true, false, 7200000));
  REQUIRE(!sl::gas_can_block(53, true, false, 1168) && !sl::gas_can_block(54, false, false, 1168) && !sl::gas_can_block(54, true, true, 1168));
  REQUIRE(!sl::gas_can_block(54, true, false, 1000) && !sl::gas_can_block(54, true, false, 0));
  REQUIRE(!sl::gas_can_block(54, true, false, 16ULL * 700000));                 // 55 rows of 1.12e7 points: past 32 bits
  REQUIRE(sl::fits_32bit(54, 16ULL * 620000) && !sl::fits_32bit(55, 16ULL * 620000) && !sl::gas_can_block(54, true, false, 16ULL * 620000));
  // prep_writes_blocked(nlay, od_is_float, is_log, bg64_knob, chunks_from_line, rowmajor_knob, n)
  REQUIRE(sl::prep_writes_blocked(54, true, false, false, true, false, 1168));
  REQUIRE(!sl::prep_writes_blocked(30, true, false, false, true, false, 1168));   // 30 layers: the copy afterwards
  REQUIRE(!sl::prep_writes_blocked(54, false, false, false, true, false, 1168));  // DOUBLE target: the generic kernel
  REQUIRE(!sl::prep_writes_blocked(54, true, true, false, true, false, 1168));    // the logarithmic method
  REQUIRE(!sl::prep_writes_blocked(54, true, false, true, true, false, 1168));    // ECCKD_BG64
  REQUIRE(!sl::prep_writes_blocked(54, true, false, false, false, false, 1168));  // ECCKD_RT_UNALIGNED
  REQUIRE(!sl::prep_writes_blocked(54, true, false, false, true, true, 1168));    // ECCKD_RT_ROWMAJOR
  REQUIRE(!sl::prep_writes_blocked(54, true, false, false, true, false, 1000));   // rows that are no whole lines
  alignas(128) static char line[256];
  REQUIRE(sl::on_line(line) && sl::on_line(line + 128) && !sl::on_line(line + 8) && !sl::on_line(line + 127) && sl::on_line(nullptr));

  std::snprintf(what, sizeof what, "32-bit offsets");
  for (u64 rows : {54ULL, 27ULL, 55ULL})
    for (u64 i : {0ULL, 15ULL, 16ULL, 1167ULL, 7199999ULL}) {
      REQUIRE(sl::fits_32bit(rows, 7200000));
      REQUIRE((u64)(unsigned)sl::point_base(rows, i) == sl::point_base(rows, i));
      REQUIRE((u64)(unsigned)sl::point_base(rows, i) + (rows - 1) * sl::LINE_BYTES == sl::offset(rows, rows - 1, i));
    }

  int cases = 0;
  for (u64 n : {16ULL, 1168ULL, 4112ULL}) { check_stores(n); ++cases; }
  std::printf("check_prep_blocked: ok (%d sizes)\n", cases);
  return 0;
}
