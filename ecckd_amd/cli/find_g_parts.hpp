// The part files of a several-process find_g_points (see the head of find_g_points.cpp): every process other than 0 leaves
// the results of its (gas, band) searches in "<output>.part<rank>", process 0 waits for the parts and reads them.  Plain host
// file I/O: nothing of the device is used, and tools/check_find_g_parts.cpp runs all of it without the library.
//
// A part: [magic "ECKDPART"][identity][n] and n results, each [gas][band][ng][status][comp_cost][ibegin][iend] followed by
// the vectors rank1, rank2, error, median, rank_slice as [length][elements]; written to "<part>.tmp" and renamed, so that a
// part is complete or absent.  A process that ends with an error leaves "<part>.failed" = [run identity][exit code] instead.
#pragma once
#include <fstream>
#include <thread>
#include <unistd.h>

#include "tool.hpp"

namespace tool {

// what one (gas, band) search hands back
struct BandResult {
  int gas = 0, band = 0, ng = 0, status = 0;
  double comp_cost = 0.0;
  int64_t ibegin = 0, iend = -1;
  std::vector<int64_t> rank1, rank2;
  std::vector<double> error, median;
  std::vector<int32_t> rank_slice;     // rank of the wavenumbers ibegin..iend after the search (sub-band / base-split re-ranking)
};

template <class T> void put(std::ofstream& f, const T& v) { f.write(reinterpret_cast<const char*>(&v), sizeof v); }
template <class T> void put_vec(std::ofstream& f, const std::vector<T>& v) {
  const uint64_t n = v.size();
  put(f, n);
  if (n) f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(n * sizeof(T)));
}
template <class T> bool get(std::ifstream& f, T& v) { return (bool)f.read(reinterpret_cast<char*>(&v), sizeof v); }
template <class T> bool get_vec(std::ifstream& f, std::vector<T>& v) {
  uint64_t n = 0;
  if (!get(f, n) || n > ((uint64_t)1 << 33)) return false;
  v.resize((size_t)n);
  return n == 0 || (bool)f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
}

// A part file carries the identity of its run: a hash of the configuration text, the launcher's rendezvous (MASTER_ADDR,
// MASTER_PORT, TORCHELASTIC_RUN_ID, ECCKD_RUN_ID), WORLD_SIZE and - known once the ordering files are read - the numbers of
// gases, bands and wavenumbers.  Process 0 refuses a part whose identity is not its own (a stale file of an aborted earlier
// run, ordering files that disagree between the processes).
inline uint64_t run_identity(const Config& config, int world) {
  uint64_t h = fnv1a(config.str());
  for (const char* name : {"MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID", "ECCKD_RUN_ID"}) {
    const char* e = std::getenv(name);
    h = fnv1a(std::string(e ? e : ""), h);
  }
  return fnv1a(&world, sizeof world, h);
}
inline uint64_t job_identity(uint64_t run_id, int ngas, int nband, uint64_t nwav) {
  uint64_t h = fnv1a(&ngas, sizeof ngas, run_id);
  h = fnv1a(&nband, sizeof nband, h);
  return fnv1a(&nwav, sizeof nwav, h);
}

inline void write_part(const std::string& path, const std::vector<BandResult>& res, uint64_t identity) {
  const std::string tmp = path + ".tmp";
  {
    std::ofstream f(tmp, std::ios::binary);
    if (!f) fail(ECCKD_PROCESSING_ERROR, "Cannot write %s", tmp.c_str());
    const uint64_t magic = 0x45434b4450415254ull, n = res.size();   // "ECKDPART"
    put(f, magic); put(f, identity); put(f, n);
    for (const BandResult& r : res) {
      put(f, r.gas); put(f, r.band); put(f, r.ng); put(f, r.status); put(f, r.comp_cost); put(f, r.ibegin); put(f, r.iend);
      put_vec(f, r.rank1); put_vec(f, r.rank2); put_vec(f, r.error); put_vec(f, r.median); put_vec(f, r.rank_slice);
    }
    if (!f) fail(ECCKD_PROCESSING_ERROR, "Short write of %s", tmp.c_str());
  }
  if (std::rename(tmp.c_str(), path.c_str()) != 0) fail(ECCKD_PROCESSING_ERROR, "Cannot rename %s", tmp.c_str());   // complete or absent
}

// the marker a process other than 0 leaves when it ends with an error: "<output>.part<r>.failed" = [run identity, exit code]
inline void write_failure_marker(const std::string& path, uint64_t run_id, int code) {
  std::ofstream f(path, std::ios::binary);
  put(f, run_id); put(f, code);
}

inline std::vector<BandResult> read_part(const std::string& path, double timeout_s, uint64_t run_id, uint64_t identity) {
  const auto t0 = std::chrono::steady_clock::now();
  const std::string failed = path + ".failed";
  while (access(path.c_str(), R_OK) != 0) {
    if (access(failed.c_str(), R_OK) == 0) {
      std::ifstream m(failed, std::ios::binary);
      uint64_t id = 0; int code = 0;
      if (get(m, id) && get(m, code) && id == run_id) {
        m.close();
        std::remove(failed.c_str());
        fail(ECCKD_PROCESSING_ERROR, "The process that was to write %s ended with exit code %d", path.c_str(), code);
      }                                         // a marker of another run: not ours to act on
    }
    if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
      fail(ECCKD_PROCESSING_ERROR, "Timed out after %g s waiting for %s (was the process of that rank started?)", timeout_s, path.c_str());
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
  }
  std::ifstream f(path, std::ios::binary);
  uint64_t magic = 0, id = 0, n = 0;
  if (!get(f, magic) || magic != 0x45434b4450415254ull || !get(f, id) || !get(f, n)) fail(ECCKD_PROCESSING_ERROR, "%s is not a find_g_points part file", path.c_str());
  if (id != identity)
    fail(ECCKD_PROCESSING_ERROR, "%s belongs to another run (configuration, launcher rendezvous, WORLD_SIZE or the numbers of gases / bands / "
         "wavenumbers differ from this process's): remove it, and start every process of a run with the same configuration", path.c_str());
  std::vector<BandResult> res((size_t)n);
  for (BandResult& r : res) {
    const bool ok = get(f, r.gas) && get(f, r.band) && get(f, r.ng) && get(f, r.status) && get(f, r.comp_cost) && get(f, r.ibegin) && get(f, r.iend) &&
                    get_vec(f, r.rank1) && get_vec(f, r.rank2) && get_vec(f, r.error) && get_vec(f, r.median) && get_vec(f, r.rank_slice);
    if (!ok) fail(ECCKD_PROCESSING_ERROR, "%s is truncated", path.c_str());
  }
  return res;
}

}  // namespace tool
