// ASan/UBSan harness for the part-file protocol of a several-process bin/find_g_points (ecckd_amd/cli/find_g_parts.hpp):
// round trips (no result, one result of empty vectors and a one-element rank_slice, several results with ng = 0 among them);
// a valid part cut short at EVERY byte - inside the header it "is not a find_g_points part file", anywhere after it "is
// truncated", and nothing is read past what the file holds; a wrong magic, a wrong identity, a vector length above 2^33 (refused,
// not allocated); a part that cannot be written; the failure marker of this run (acted on and removed), of another run
// (ignored: the wait goes on to its time-out), and a time-out of 0 s with nothing there; job_identity under a change of each of
// its arguments.  run_identity is not checked: it needs a Config, which needs the library.
// The header uses nothing of the library but its error codes, so the program links against nothing.
// build: g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -std=c++17 -static-libasan -static-libubsan
//        tools/check_find_g_parts.cpp -o /tmp/check_find_g_parts && /tmp/check_find_g_parts
// (tests/test_find_g_parts.py does that; the runtimes are linked statically so that the program starts whatever is preloaded)
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <string>

#include "../ecckd_amd/cli/find_g_parts.hpp"

using namespace tool;

#define REQUIRE(cond)                                                                           \
  do {                                                                                          \
    if (!(cond)) { std::printf("%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

static const uint64_t RUN = 0x1234567890abcdefull, ID = 0x0fedcba987654321ull;

static std::string tmp_path(const char* name) {
  const char* tmp = std::getenv("TMPDIR");
  return std::string(tmp ? tmp : "/tmp") + "/check_find_g_parts_" + std::to_string((long)getpid()) + "_" + name;
}

static bool exists(const std::string& path) { return access(path.c_str(), F_OK) == 0; }
static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

static std::string slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}
static void spit(const std::string& path, const std::string& bytes) {
  std::ofstream f(path, std::ios::binary);
  f.write(bytes.data(), (std::streamsize)bytes.size());
}

// the message with which read_part refuses, or "" when it returns
static std::string refusal(const std::string& path, double timeout_s, uint64_t run_id = RUN, uint64_t identity = ID) {
  try {
    read_part(path, timeout_s, run_id, identity);
  } catch (const Fatal& f) {
    REQUIRE(f.code == ECCKD_PROCESSING_ERROR);
    return f.msg;
  }
  return "";
}

static BandResult result(int gas, int band, int ng, size_t nslice) {
  BandResult r;
  r.gas = gas; r.band = band; r.ng = ng; r.status = 3 - band; r.comp_cost = 1.5 * gas + 0.25 * band;
  r.ibegin = 1000 * band; r.iend = r.ibegin + (int64_t)nslice - 1;
  for (int k = 0; k < ng; ++k) {
    r.rank1.push_back(r.ibegin + 10 * k);
    r.rank2.push_back(r.ibegin + 10 * k + 9);
    r.error.push_back(0.01 * (k + 1) + gas);
    r.median.push_back(-2.5 * k);
  }
  for (size_t i = 0; i < nslice; ++i) r.rank_slice.push_back((int32_t)(r.ibegin + (int64_t)((i * 7) % nslice)));
  return r;
}

static bool same(const BandResult& a, const BandResult& b) {
  return a.gas == b.gas && a.band == b.band && a.ng == b.ng && a.status == b.status && a.comp_cost == b.comp_cost && a.ibegin == b.ibegin &&
         a.iend == b.iend && a.rank1 == b.rank1 && a.rank2 == b.rank2 && a.error == b.error && a.median == b.median && a.rank_slice == b.rank_slice;
}

static void round_trip(const std::string& path, const std::vector<BandResult>& res) {
  write_part(path, res, ID);
  REQUIRE(exists(path) && !exists(path + ".tmp"));
  const std::vector<BandResult> back = read_part(path, 0.0, RUN, ID);
  REQUIRE(back.size() == res.size());
  for (size_t k = 0; k < res.size(); ++k) REQUIRE(same(back[k], res[k]));
  std::remove(path.c_str());
}

int main() {
  const std::string path = tmp_path("part1");
  std::remove(path.c_str());
  std::remove((path + ".failed").c_str());

  // ---- round trips ----
  round_trip(path, {});
  round_trip(path, {result(0, 0, 0, 1)});                       // every vector empty but a rank_slice of one element
  {
    BandResult bare;                                            // nothing at all: iend = ibegin - 1, an empty rank_slice too
    round_trip(path, {bare});
  }
  round_trip(path, {result(0, 0, 3, 17), result(0, 1, 0, 5), result(1, 0, 0, 1), result(1, 1, 4, 33), result(2, 1, 1, 2)});

  // ---- a valid part cut short at every byte ----
  write_part(path, {result(0, 1, 2, 9), result(1, 0, 0, 3), result(1, 1, 3, 4)}, ID);
  const std::string whole = slurp(path);
  const size_t header = 3 * sizeof(uint64_t);                   // magic, identity, number of results
  REQUIRE(whole.size() > header + 3 * (40 + 5 * 8));            // three results: 40 bytes of scalars and five vector lengths each
  for (size_t cut = 0; cut < whole.size(); ++cut) {
    spit(path, whole.substr(0, cut));
    const std::string msg = refusal(path, 0.0);
    REQUIRE(has(msg, cut < header ? "is not a find_g_points part file" : "is truncated"));
  }
  spit(path, whole);
  REQUIRE(refusal(path, 0.0).empty());

  // ---- bad headers ----
  {
    std::string bad = whole;
    bad[0] ^= 1;
    spit(path, bad);
    REQUIRE(has(refusal(path, 0.0), "is not a find_g_points part file"));
    spit(path, whole);
    REQUIRE(has(refusal(path, 0.0, RUN, ID + 1), "belongs to another run"));
    // the length of the first result's rank1 (after the header and 40 bytes of scalars): above 2^33 it is refused before the
    // vector is sized - 2^33 + 1 int64 would be 64 GiB to clear, 2^60 cannot be allocated at all
    for (uint64_t n : {((uint64_t)1 << 33) + 1, (uint64_t)1 << 60, ~(uint64_t)0}) {
      bad = whole;
      std::memcpy(&bad[header + 40], &n, sizeof n);
      spit(path, bad);
      REQUIRE(has(refusal(path, 0.0), "is truncated"));
    }
  }
  std::remove(path.c_str());
  {
    std::string msg;
    try { write_part("/nonexistent-directory/part1", {}, ID); } catch (const Fatal& f) { REQUIRE(f.code == ECCKD_PROCESSING_ERROR); msg = f.msg; }
    REQUIRE(has(msg, "Cannot write /nonexistent-directory/part1.tmp"));
  }

  // ---- failure markers and the wait ----
  REQUIRE(has(refusal(path, 0.0), "Timed out after 0 s waiting for "));
  write_failure_marker(path + ".failed", RUN, 147);
  REQUIRE(has(refusal(path, 30.0), "ended with exit code 147"));       // at once, not after the 30 s
  REQUIRE(!exists(path + ".failed"));                                   // and the marker is removed
  write_failure_marker(path + ".failed", RUN + 1, 147);                 // another run's: not ours to act on
  REQUIRE(has(refusal(path, 0.05), "Timed out after 0.05 s"));
  REQUIRE(exists(path + ".failed"));
  spit(path + ".failed", std::string(5, '\1'));                         // a marker cut short is no marker
  REQUIRE(has(refusal(path, 0.05), "Timed out"));
  std::remove((path + ".failed").c_str());

  // ---- identities ----
  const uint64_t base = job_identity(RUN, 6, 13, 7200000);
  REQUIRE(base == job_identity(RUN, 6, 13, 7200000));
  REQUIRE(base != job_identity(RUN, 7, 13, 7200000) && base != job_identity(RUN, 6, 14, 7200000) && base != job_identity(RUN, 6, 13, 7200001));
  REQUIRE(base != job_identity(RUN + 1, 6, 13, 7200000) && job_identity(RUN, 13, 6, 7200000) != base);

  std::printf("check_find_g_parts: ok\n");
  return 0;
}
