// find_g_points [key=value ...] [file.cfg]
//
// Drop-in for the reference executable of the same name (src/ecckd/find_g_points.cpp:407-1664): for every gas in
// `gases` and every band of its reordering file, partition the reordered spectrum into g points whose heating-
// rate error is within `heating_rate_tolerance`, then overlap the gases' g points and write the g-points file.
// In the shortwave, `cloud <name>` adds the cloud pseudo-gas of :541-652 (<name>.reordering_input from
// reorder_cloud_spectrum, <name>.max_reflectance_range): bands split into g points of equal solar energy along the cloud's
// ordering (ecckd_cloud_partition_dev), the first constituent of the overlap.
// Keys (:443-523, :655-771): output, ssi, iprofile, heating_rate_tolerance, tolerance_tolerance, max_iterations,
// averaging_method, flux_weight, min_pressure, max_no_rayleigh_wavenumber, gases, prepend_path, append_path,
// log_level; per gas <gas>.input / scaling / conc, <gas>.background_input / _scaling / _conc, reordering_input,
// min_scaling, max_scaling, g_split + subband_wavenumber_boundary, base_split, base_wavenumber_boundary,
// min_g_points, max_g_points.
// Extension keys for asking for a NUMBER of g points instead of a tolerance (the reference's scripts keep hand-found tables of
// the tolerance per g-point count, test/do_all_lw.sh:44-65): target_g_points = n switches the mode on: every gas is read and
// prepared first and stays resident, then ONE call (ecckd_find_g_gases_target) searches the gases again and again with all
// tolerances multiplied by one factor - heating_rate_tolerance is the first guess and fixes the ratio between the bands - until
// the overlap of the gases has n g points; target_resolution (1e-3: the factor is not refined below this relative width) and
// target_max_trials (40) bound the search; target_exact = 1 makes a search that does not hit n exactly a PROCESSING_ERROR that
// writes no file.  The g-points file then also holds target_g_points, target_search_status (0 hit, 1 resolution reached,
// 2 trials spent, 3 out of reach), heating_rate_tolerance_scaling, heating_rate_tolerance(band) - the tolerances used, with
// which a plain run gives the same file - and the trials, target_trial_scaling / target_trial_n_g_points(target_trial).
// Not with WORLD_SIZE > 1, cloud, sequential_bands or a base_wavenumber_boundary inside a band (PARAMETER_ERROR).
// All nwav-sized work runs on the GPU through include/ecckd_hip.h; this file is the driver around it.
//
// Several processes, one per GPU (RANK / WORLD_SIZE / LOCAL_RANK from the launcher, e.g. torchrun --no-python): the (gas, band)
// searches are independent problems (:655, :1152); every process takes a contiguous share of the task table, reads and prepares
// only the gases of which it searches a band, and leaves its per-band results (a few numbers per g point and the band's slice
// of the - possibly re-ranked - rank) in "<output>.part<rank>" (find_g_parts.hpp); rank 0 collects the parts, does what follows
// the gas loop (:1452-1660) and prints the final cost (sum of the g points' errors).  The g-points file does not depend on
// WORLD_SIZE.
//
// The driver ("Where the find_g_points tool's driver lives"): Settings are read once; every gas's Ordering is a
// value; a GasJob owns what a gas's searches read and write and lends pointers into itself to the library; the SearchQueue owns
// the jobs whose searches are in flight; what follows the gas loop are functions from values to values.
#include <algorithm>
#include <cctype>
#include <future>
#include <memory>

#include "find_g_parts.hpp"

using namespace tool;

namespace {

const int band_capacity = 1024;           // g points one band's search can hand back
const double cos_sza = 0.5;               // REFERENCE_COS_SZA, calc_cost_function_sw.h:20
const double reference_albedo = 0.15;     // :469

struct GasResult {   // SingleGasData (single_gas_data.h:24-80)
  std::string molecule;
  std::vector<int> n_g_points;        // per band
  std::vector<int> band_number;       // per gas g point
  std::vector<int64_t> rank1, rank2;
  std::vector<double> error, sorting_variable;
  std::vector<int> g_min, g_max;      // per merged g point
  DevBuf d_g_point;                   // int32 [nwav]
};

template <class T>
std::vector<T> per_band(const Config& config, const std::string& gas, const char* key, int nband, T fill, bool* present = nullptr) {
  std::vector<T> raw, out(nband, fill);
  const bool have = config.read(raw, key, gas.c_str());
  if (present) *present = have;
  if (have)
    for (int b = 0; b < std::min<int>(nband, (int)raw.size()); ++b) out[b] = raw[b];
  return out;
}

std::string upper(std::string s) {
  std::transform(s.begin(), s.end(), s.begin(), ::toupper);
  return s;
}

// ---- settings: what the configuration and the environment say, whatever the files hold ----
struct Settings {
  std::string output, ssi_file_name, cloud;
  bool do_sw = false, have_cloud = false;
  int iprofile = 0;
  std::vector<double> tolerance_in;
  double tolerance_tolerance = 0.02, flux_weight = 0.02, min_pressure = 0.0, max_no_rayleigh_wavenumber = 10000.0;
  int max_iterations = 60, method = -1;
  int world = 1, my_rank = 0;
  // target_g_points: the tolerance is searched for (see the head of this file)
  bool target_mode = false, target_exact = false;
  int target_g_points = 0, target_max_trials = 40;
  double target_resolution = 1.0e-3;
  // Extension keys: gases_side_by_side = n (gases searched at a time; 1 = the reference's order, 0 = what the host has cores
  // for), sequential_bands (the reference's one-band-at-a-time order of evaluation, which also means gas after gas)
  bool sequential_bands = false;
  int gases_side_by_side = 0;
  // extension key: how long process 0 waits for a part that has not appeared, in seconds.  A process that FAILS through an
  // error path says so through its marker at once; one that is killed (a signal, the out-of-memory killer, a HIP abort) leaves
  // none, so the wait is what bounds that case - the reference-sized default stays an hour
  double part_timeout = 3600.0;
  std::vector<std::string> gas_list;
  uint64_t run_id = 0;
  std::string part(int rank) const { return output + ".part" + std::to_string(rank); }
};

// The refusals come in the reference's order, and the spectral region is logged where the reference logs it: before them.
Settings read_settings(const Config& config) {
  Settings st;
  if (!config.read(st.output, "output")) fail(ECCKD_PARAMETER_ERROR, "\"output\" file not specified");
  st.do_sw = config.read(st.ssi_file_name, "ssi");
  if (st.do_sw) LOG("Assuming shortwave spectral region (ssi provided)\nReading %s\n", st.ssi_file_name.c_str());
  else LOG("Assuming longwave spectral region (ssi not provided)\n");
  // the cloud pseudo-gas (:543-652): shortwave only; its g points are found by process 0 once the gases' searches are in
  st.have_cloud = config.read(st.cloud, "cloud");
  if (st.have_cloud && !st.do_sw) fail(ECCKD_PARAMETER_ERROR, "Don't yet know how to sort cloud properties in the longwave");
  config.read(st.iprofile, "iprofile");
  if (!config.read(st.tolerance_in, "heating_rate_tolerance")) fail(ECCKD_PARAMETER_ERROR, "heating_rate_tolerance not defined");
  std::string averaging_method = "linear";
  config.read(st.tolerance_tolerance, "tolerance_tolerance");
  config.read(st.max_iterations, "max_iterations");
  config.read(averaging_method, "averaging_method");
  config.read(st.flux_weight, "flux_weight");
  config.read(st.min_pressure, "min_pressure");
  config.read(st.max_no_rayleigh_wavenumber, "max_no_rayleigh_wavenumber");
  static const char* const methods[] = {"linear", "transmission", "transmission-2", "square-root", "logarithmic",
                                        "total-transmission", "transmission-3", "transmission-10", "hybrid-logarithmic-transmission-3"};
  for (int k = 0; k < 9; ++k) if (averaging_method == methods[k]) st.method = k;
  if (st.method < 0) fail(ECCKD_PARAMETER_ERROR, "Averaging method \"%s\" not understood", averaging_method.c_str());
  st.world = std::max(1, env_int("WORLD_SIZE", 1));
  st.my_rank = env_int("RANK", 0);
  if (st.my_rank < 0 || st.my_rank >= st.world) fail(ECCKD_PARAMETER_ERROR, "RANK=%d outside WORLD_SIZE=%d", st.my_rank, st.world);
  st.target_mode = config.read(st.target_g_points, "target_g_points");
  config.read(st.target_resolution, "target_resolution");
  config.read(st.target_max_trials, "target_max_trials");
  config.read(st.target_exact, "target_exact");
  config.read(st.sequential_bands, "sequential_bands");
  config.read(st.gases_side_by_side, "gases_side_by_side");
  if (st.sequential_bands) st.gases_side_by_side = 1;
  config.read(st.part_timeout, "part_timeout");
  st.gas_list = config.read_list("gases");
  st.run_id = run_identity(config, st.world);
  return st;
}

// target_g_points is refused here, before the device starts and before any other process is waited for
void refuse_unsearchable_target(const Config& config, const SearchPath& paths, const Settings& st) {
  if (st.world > 1) fail(ECCKD_PARAMETER_ERROR, "target_g_points needs all gases in one process (WORLD_SIZE=%d): a trial would need an all-reduce", st.world);
  if (st.have_cloud) fail(ECCKD_PARAMETER_ERROR, "target_g_points cannot be combined with cloud");
  if (st.sequential_bands) fail(ECCKD_PARAMETER_ERROR, "target_g_points cannot be combined with sequential_bands");
  if (st.target_g_points < 1) fail(ECCKD_PARAMETER_ERROR, "target_g_points = %d, must be at least 1", st.target_g_points);
  for (const std::string& gas_str : st.gas_list) {
    std::vector<double> boundary;
    std::string reordering_input;
    if (!config.read(boundary, "base_wavenumber_boundary", gas_str.c_str()) || boundary.empty()) continue;
    if (!config.read(reordering_input, "reordering_input", gas_str.c_str())) fail(ECCKD_PARAMETER_ERROR, "No reordering_input found");
    NcIn f(paths.find(reordering_input));
    const std::vector<double> b1 = f.read("wavenumber1_band"), b2 = f.read("wavenumber2_band");
    for (size_t b = 0; b < b1.size() && b < b2.size(); ++b)
      for (double w : boundary)
        if (w > b1[b] && w < b2[b])
          fail(ECCKD_PARAMETER_ERROR, "target_g_points: %s.base_wavenumber_boundary %g lies inside band %zu: that split re-ranks the "
               "spectrum during the search, so the gas cannot be searched more than once", gas_str.c_str(), w, b);
  }
}

// Several processes, before anything that can fail (device start-up, the gas list, the files): never a stale part or marker of
// an earlier run under this process's name, and from here on a failure of this process is visible to process 0
void claim_part_files(const Settings& st) {
  if (st.world <= 1) return;
  const std::string my_part = st.part(st.my_rank);
  std::remove(my_part.c_str());
  std::remove((my_part + ".tmp").c_str());
  std::remove((my_part + ".failed").c_str());
  const uint64_t run_id = st.run_id;
  if (st.my_rank != 0) on_failure() = [my_part, run_id](int code) { write_failure_marker(my_part + ".failed", run_id, code); };
}

// what every step is handed: nothing in it is written after the device has started
struct Run {
  const Config& config;
  const SearchPath& paths;
  const Device& dev;
  const Settings& st;
  int argc;
  const char* const* argv;
};

// ---- orderings ----
struct BandTable {
  std::vector<double> bound1, bound2, wavenumber;
  int nband = 0;
  size_t nwav = 0;
};

// the ordering file of a gas (:669-683) and the sub-bands of the optically thin part of `bands` (:788-870), which re-rank
// d_rank before anything is reordered
struct Ordering {
  BandTable bands;                     // of this file, and of nothing else
  std::vector<int32_t> rank;
  std::vector<int> iband;
  std::vector<double> sorting_variable, subband_wavenumber_boundary, g_split;
  std::vector<int64_t> ibegin, iend;   // first / last index of every band: the members of a band are contiguous in rank
  bool have_g_split = false;
  int nsb = 1;
  std::vector<int> nsubband;
  std::vector<int64_t> iupperindex, isubband1, isubband2;
  DevBuf d_rank, d_wn;
};

Ordering read_ordering(const Config& config, const SearchPath& paths, const std::string& gas_str) {
  Ordering o;
  const char* scope = gas_str.c_str();
  std::string reordering_input;
  if (!config.read(reordering_input, "reordering_input", scope)) fail(ECCKD_PARAMETER_ERROR, "No reordering_input found");
  LOG("Reading %s\n", reordering_input.c_str());
  {
    // the four per-wavenumber variables side by side, each through a handle of its own: a 7.2e6-point variable costs
    // ~20 ms, most of it the first touch of the 58 MB it is decoded into
    // (a classic file only: a NetCDF-4 one is read through the HDF5 library, which must not be entered by two threads)
    const std::string order_path = paths.find(reordering_input);
    bool classic = false;
    if (FILE* fp = std::fopen(order_path.c_str(), "rb")) {
      char magic[4] = {0, 0, 0, 0};
      classic = std::fread(magic, 1, 4, fp) == 4 && magic[0] == 'C' && magic[1] == 'D' && magic[2] == 'F';
      std::fclose(fp);
    }
    const std::launch how = classic ? std::launch::async : std::launch::deferred;
    auto read_var = [order_path](const char* name) { NcIn g(order_path); return g.read(name); };
    auto f_rank = std::async(how, [&] { std::vector<double> r = read_var("rank"); return std::vector<int32_t>(r.begin(), r.end()); });
    auto f_band = std::async(how, [&] { std::vector<double> b = read_var("band_number"); return std::vector<int>(b.begin(), b.end()); });
    auto f_sort = std::async(how, [&] { return read_var("sorting_variable"); });
    NcIn f(order_path);
    o.bands.bound1 = f.read("wavenumber1_band");
    o.bands.bound2 = f.read("wavenumber2_band");
    o.bands.wavenumber = f.read("wavenumber");
    o.rank = f_rank.get();
    o.iband = f_band.get();
    o.sorting_variable = f_sort.get();
  }
  const int nband = o.bands.nband = (int)o.bands.bound1.size();
  const size_t nwav = o.bands.nwav = o.rank.size();
  o.g_split = per_band<double>(config, gas_str, "g_split", nband, -1.0, &o.have_g_split);
  if (o.have_g_split && !config.read(o.subband_wavenumber_boundary, "subband_wavenumber_boundary", scope))
    fail(ECCKD_PARAMETER_ERROR, "g_split must be accompanied by subband_wavenumber_boundary");
  o.ibegin.assign(nband, -1);
  o.iend.assign(nband, -1);
  for (size_t i = 0; i < nwav; ++i) {
    const int b = o.iband[i];
    if (b < 0 || b >= nband) continue;
    if (o.ibegin[b] < 0) o.ibegin[b] = (int64_t)i;
    o.iend[b] = (int64_t)i;
  }
  o.nsb = (int)o.subband_wavenumber_boundary.size() + 1;
  o.nsubband.assign(nband, 0);
  o.iupperindex.assign(nband, -1);
  o.isubband1.assign((size_t)nband * o.nsb, -1);
  o.isubband2.assign((size_t)nband * o.nsb, -1);
  return o;
}

void subband_setup(const Device& dev, Ordering& o, const std::vector<char>& bands) {
  const BandTable& t = o.bands;
  o.d_rank.upload(dev, o.rank);
  o.d_wn.upload(dev, t.wavenumber);
  if (!o.have_g_split) return;
  for (int b = 0; b < t.nband; ++b)
    if (bands[b] && o.g_split[b] > 0.0 && o.ibegin[b] >= 0)
      ck(ecckd_subband_setup_dev(dev.ctx(), t.nwav, o.d_wn.as<double>(), o.d_rank.as<int32_t>(), o.ibegin[b], o.iend[b], o.g_split[b],
                                 t.bound1[b], t.bound2[b], (int)o.subband_wavenumber_boundary.size(),
                                 o.subband_wavenumber_boundary.data(), &o.nsubband[b], &o.isubband1[(size_t)b * o.nsb],
                                 &o.isubband2[(size_t)b * o.nsb], &o.iupperindex[b]));
}

// ---- band-specific configuration of a gas (:687-771) ----
struct BandConfig {
  std::vector<double> base_wavenumber_boundary, base_split, band_albedo, tolerance;
  std::vector<int> min_g_points, max_g_points;
  double no_rayleigh_limit = -1.0e300;
};

BandConfig read_band_config(const Run& run, const std::string& gas_str, const Ordering& ord) {
  const Settings& st = run.st;
  const int nband = ord.bands.nband;
  BandConfig c;
  run.config.read(c.base_wavenumber_boundary, "base_wavenumber_boundary", gas_str.c_str());
  bool have_base_split = false;
  c.base_split = per_band<double>(run.config, gas_str, "base_split", nband, 1.0, &have_base_split);
  if (have_base_split && ord.have_g_split) fail(ECCKD_PARAMETER_ERROR, "Cannot use both g_split and base_split");
  c.min_g_points = per_band<int>(run.config, gas_str, "min_g_points", nband, 1);
  c.max_g_points = per_band<int>(run.config, gas_str, "max_g_points", nband, 256);
  c.band_albedo.assign(nband, 0.0);
  for (int b = 0; b < nband; ++b)
    if (ord.bands.bound2[b] <= st.max_no_rayleigh_wavenumber) {
      c.band_albedo[b] = reference_albedo;
      c.no_rayleigh_limit = std::max(c.no_rayleigh_limit, ord.bands.bound2[b]);
    }
  if ((int)st.tolerance_in.size() == nband) c.tolerance = st.tolerance_in;   // :762-771
  else if (st.tolerance_in.size() == 1) c.tolerance.assign(nband, st.tolerance_in[0]);
  else fail(ECCKD_PARAMETER_ERROR, "heating_rate_tolerance must have either one element or one per band (%d)", nband);
  return c;
}

// ---- a gas and its searches ----
// Everything the searches of one gas read and write.  The library is lent pointers into the job (set_up_search) and its search
// threads use them until the searches are waited for, so a job is built where it stays: it is neither copied nor moved.
struct GasJob {
  GasJob(int gas_index, Ordering&& ordering, std::vector<int> bands) : gi(gas_index), ord(std::move(ordering)), mine(std::move(bands)) {}
  GasJob(const GasJob&) = delete;
  GasJob& operator=(const GasJob&) = delete;
  GasJob(GasJob&&) = delete;
  GasJob& operator=(GasJob&&) = delete;

  const int gi;
  Ordering ord;
  const std::vector<int> mine;       // the bands of this gas that this process searches
  ecckd_gas* gas = nullptr;          // destroyed when the searches are finished (SearchQueue::finish)
  bool keeps_gas = false;            // unless it is the first longwave gas, which lends its Planck matrix (PlanckSource)
  DevBuf d_sv_sorted;
  std::vector<ecckd_band_options> opts;
  std::vector<std::vector<double>> wn_bounds;
  std::vector<size_t> ib, ie;
  std::vector<double> tol, comp_costs, bounds, error;
  std::vector<int> ngs, statuses;
  std::vector<int64_t> r1, r2;
  ecckd_gas_search req;

  void set_up_search(const BandConfig& cfg, bool do_sw);
};

// Options of every band (:1152-1414): the bands are then searched side by side (ecckd_find_g_bands_ex); a shortwave band brings
// its albedo (init_sw(..., band_albedo(jband), ...), :1177) with it.
// What the library borrows from this job, from here until the searches are waited for (SearchQueue::flush):
//   opts[m].isubband1 / isubband2         -> ord.isubband1 / ord.isubband2
//   opts[m].base_wn_bound                 -> wn_bounds[m]          (base_split != 1 or a base_wavenumber_boundary inside the band)
//   opts[m].d_wavenumber / d_rank         -> ord.d_wn / ord.d_rank (device memory; d_rank is re-ranked in place by that split)
//   req.ibegin / iend / heating_rate_tolerance / opt  -> ib / ie / tol / opts
//   req.ng / bounds / error / rank1 / rank2 / status / comp_cost -> ngs / bounds / error / r1 / r2 / statuses / comp_costs
//   req.gas                               -> gas
// and &req itself (ecckd_find_g_gases_add).  None of these vectors is resized after this function.
void GasJob::set_up_search(const BandConfig& cfg, bool do_sw) {
  const int nmine = (int)mine.size();
  const BandTable& t = ord.bands;
  opts.resize(nmine);
  wn_bounds.resize(nmine);
  ib.resize(nmine); ie.resize(nmine); tol.resize(nmine);
  for (int m = 0; m < nmine; ++m) {
    const int b = mine[m];
    if (ord.ibegin[b] < 0) fail(ECCKD_PARAMETER_ERROR, "Band %d contains no wavenumbers", b);
    ib[m] = (size_t)ord.ibegin[b];
    ie[m] = (size_t)ord.iend[b];
    tol[m] = cfg.tolerance[b];
    ecckd_band_options& opt = opts[m];
    std::memset(&opt, 0, sizeof opt);
    opt.min_g_points = cfg.min_g_points[b];
    opt.max_g_points = cfg.max_g_points[b];
    if (ord.nsubband[b] > 1) {
      opt.nsubband = ord.nsubband[b];
      opt.isubband1 = &ord.isubband1[(size_t)b * ord.nsb];
      opt.isubband2 = &ord.isubband2[(size_t)b * ord.nsb];
      opt.iupperindex = ord.iupperindex[b];
      opt.g_split = ord.g_split[b];
    }
    opt.base_split = cfg.base_split[b];
    opt.band_albedo = do_sw ? cfg.band_albedo[b] : 0.0;
    std::vector<double>& wn_bound = wn_bounds[m];
    std::vector<double> interior;
    for (double w : cfg.base_wavenumber_boundary) if (w > t.bound1[b] && w < t.bound2[b]) interior.push_back(w);
    if (cfg.base_split[b] != 1.0 || !interior.empty()) {   // :1268-1301
      wn_bound.push_back(t.bound1[b]);
      wn_bound.insert(wn_bound.end(), interior.begin(), interior.end());
      wn_bound.push_back(t.bound2[b] + 1.0);
      opt.nbase_wn_bound = (int)wn_bound.size();
      opt.base_wn_bound = wn_bound.data();
      opt.d_wavenumber = ord.d_wn.as<double>();
      opt.d_rank = ord.d_rank.as<int32_t>();
      opt.nwav = t.nwav;
    }
  }
  ngs.assign(nmine, 0); statuses.assign(nmine, 0);
  comp_costs.assign(nmine, 0.0);
  bounds.assign((size_t)nmine * (band_capacity + 1), 0.0); error.assign((size_t)nmine * band_capacity, 0.0);
  r1.assign((size_t)nmine * band_capacity, 0); r2.assign((size_t)nmine * band_capacity, 0);
  std::memset(&req, 0, sizeof req);
  req.gas = gas; req.nband = nmine; req.ibegin = ib.data(); req.iend = ie.data(); req.heating_rate_tolerance = tol.data();
  req.opt = opts.data(); req.ng = ngs.data(); req.bounds = bounds.data(); req.error = error.data();
  req.rank1 = r1.data(); req.rank2 = r2.data(); req.capacity = band_capacity; req.status = statuses.data();
  req.comp_cost = comp_costs.data();
}

// The reference evaluates the Planck function once, on the FIRST gas's reordered grid (:529, :970-984): the first longwave gas
// stays alive after its searches and lends its matrix to the later ones; a process that does not search the first gas rebuilds
// the matrix instead (rebuild_first_planck).
struct PlanckSource {
  ecckd_gas* first_gas = nullptr;    // owned
  DevBuf rebuilt;
  const double* d_planck = nullptr;  // into first_gas or rebuilt
  void release() {
    if (first_gas) ck(ecckd_gas_destroy(first_gas));
    first_gas = nullptr;
    rebuilt.release();
    d_planck = nullptr;
  }
};

// device buffers of a gas's turn in the gas loop that the gas does not keep: released when the turn ends, after its searches
// have started
struct TurnBuffers {
  DevBuf d_dwn, d_ssi, d_albedo, d_ireorder, d_sv;
};

// This process does not search the first gas: the Planck matrix is rebuilt from that gas's ordering file and temperatures, bit
// for bit.  The first gas's ordering is prepared in every band, as by the process that searches it.
void rebuild_first_planck(const Run& run, const std::string& gas_str, const Spectrum& s, size_t nwav, PlanckSource& planck) {
  const std::string first = run.st.gas_list[0];
  Ordering o0 = read_ordering(run.config, run.paths, first);
  subband_setup(run.dev, o0, std::vector<char>(o0.bands.nband, 1));
  const std::vector<std::string> files0 = run.config.read_list(first + ".input");
  if (files0.empty()) fail(ECCKD_PARAMETER_ERROR, "%s.input not found", first.c_str());
  const Spectrum s0 = read_spectrum(run.paths.find(files0[0]), run.st.iprofile, false);
  if (s0.nwav != nwav || o0.bands.nwav != nwav || s0.nlay != s.nlay || s0.temperature_hl.empty())
    fail(ECCKD_PARAMETER_ERROR, "The spectrum of %s does not match that of %s", first.c_str(), gas_str.c_str());
  DevBuf d_wn0, d_dwn0;
  d_wn0.upload(run.dev, s0.wavenumber_cm_1);
  d_dwn0.upload(run.dev, s0.d_wavenumber_cm_1);
  planck.rebuilt.alloc(run.dev, (size_t)(s0.nlay + 1) * nwav * sizeof(double));
  ck(ecckd_planck_hl_sorted_dev(run.dev.ctx(), s0.nlay, nwav, s0.temperature_hl.data(), d_wn0.as<double>(), d_dwn0.as<double>(),
                                o0.d_rank.as<int32_t>(), planck.rebuilt.as<double>()));
  ck(ecckd_synchronize(run.dev.ctx()));
  planck.d_planck = planck.rebuilt.as<double>();
}

// background and target optical depths (:872-915) and the gas preparation on the device (:917-1150): sets job.gas
void prepare_gas(const Run& run, GasJob& job, const BandConfig& cfg, const std::vector<double>& ssi, PlanckSource& planck, TurnBuffers& turn) {
  const Settings& st = run.st;
  const Device& dev = run.dev;
  const std::string& gas_str = st.gas_list[job.gi];
  const size_t nwav = job.ord.bands.nwav;
  DevBuf& d_rank = job.ord.d_rank;
  DevBuf& d_wn = job.ord.d_wn;
  Merged bg;
  const bool have_bg = run.config.exist(gas_str + ".background_input");
  if (have_bg) {
    LOG("Generating background optical depth\n");
    bg = read_merged_spectrum(dev, run.config, run.paths, st.iprofile, gas_str + ".background_");
  }
  LOG("Generating target optical depth\n");
  Merged target = read_merged_spectrum(dev, run.config, run.paths, st.iprofile, gas_str + ".");
  const Spectrum& s = target.first;
  if (s.nwav != nwav) fail(ECCKD_PARAMETER_ERROR, "%s: %zu spectral points, the reordering file has %zu", gas_str.c_str(), s.nwav, nwav);
  if (have_bg && bg.first.nwav != nwav) fail(ECCKD_PARAMETER_ERROR, "%s: background spectra on a different grid", gas_str.c_str());
  d_wn.upload(dev, s.wavenumber_cm_1);
  turn.d_dwn.upload(dev, s.d_wavenumber_cm_1);

  LOG("  Reordering and computing the reference fluxes and heating rates\n");
  if (!st.do_sw) {
    if (s.temperature_hl.empty()) fail(ECCKD_PARAMETER_ERROR, "temperature_hl missing from the spectrum of %s", gas_str.c_str());
    if (job.gi > 0 && !planck.d_planck) rebuild_first_planck(run, gas_str, s, nwav, planck);
    ck(ecckd_gas_create_lw(dev.ctx(), s.nlay, nwav, s.pressure_hl.data(), s.temperature_hl.data(), d_wn.as<double>(),
                           turn.d_dwn.as<double>(), d_rank.as<int32_t>(), have_bg ? bg.od_ptr() : nullptr, have_bg ? bg.od_type() : 0,
                           target.od_ptr(), target.od_type(), nwav, st.method, st.flux_weight, st.min_pressure, planck.d_planck, &job.gas));
    if (job.gi == 0) {
      // the first gas stays alive and lends its matrix
      job.keeps_gas = true;
      planck.first_gas = job.gas;
      size_t rows = 0, cols = 0;
      ck(ecckd_gas_view(job.gas, "planck_hl", &planck.d_planck, &rows, &cols));
    }
  } else {
    double min_scaling = 1.0, max_scaling = 1.0;
    run.config.read(min_scaling, "min_scaling", gas_str.c_str());
    run.config.read(max_scaling, "max_scaling", gas_str.c_str());
    min_scaling = std::min(0.5, min_scaling);   // :666-667
    max_scaling = std::max(2.5, max_scaling);
    if (ssi.size() != nwav) fail(ECCKD_PARAMETER_ERROR, "solar_spectral_irradiance has %zu points, the spectrum %zu", ssi.size(), nwav);
    std::vector<double> albedo(nwav, 0.0);   // :919-923
    for (size_t i = 0; i < nwav; ++i) if (s.wavenumber_cm_1[i] < cfg.no_rayleigh_limit) albedo[i] = reference_albedo;
    turn.d_ssi.upload(dev, ssi);
    turn.d_albedo.upload(dev, albedo);
    ck(ecckd_gas_create_sw(dev.ctx(), s.nlay, nwav, s.pressure_hl.data(), turn.d_ssi.as<double>(), turn.d_albedo.as<double>(),
                           d_rank.as<int32_t>(), have_bg ? bg.od_ptr() : nullptr, have_bg ? bg.od_type() : 0, target.od_ptr(),
                           target.od_type(), nwav, st.method, st.flux_weight, st.min_pressure, cos_sza, min_scaling, max_scaling, &job.gas));
  }
  bg = Merged();                      // the spectra go before the sorting variable is gathered
  target.d_od.release();
  target.single.buf.release();
}

// sorting variable in sorted order (:781): sorted[r] = orig[ireorder[r]]
void gather_sorting_variable(const Device& dev, GasJob& job, TurnBuffers& turn) {
  const size_t nwav = job.ord.bands.nwav;
  turn.d_ireorder.alloc(dev, nwav * sizeof(int32_t));
  job.d_sv_sorted.alloc(dev, nwav * sizeof(double));
  turn.d_sv.upload(dev, job.ord.sorting_variable);
  ck(ecckd_invert_permutation_dev(dev.ctx(), nwav, job.ord.d_rank.as<int32_t>(), turn.d_ireorder.as<int32_t>()));
  ck(ecckd_gather_f64_dev(dev.ctx(), nwav, turn.d_sv.as<double>(), turn.d_ireorder.as<int32_t>(), job.d_sv_sorted.as<double>()));
  ck(ecckd_synchronize(dev.ctx()));
}

// The searches of a gas start as soon as the gas is prepared and run - a host thread and a HIP stream per gas
// (ecckd_find_g_gases_begin / _add / _wait) - while the next gas's files are read, merged and prepared: the reference's loop
// (:655) takes gas after gas, but a search is a chain of small dependent evaluations that cannot fill the device, and the
// reading of the next gas needs the host.  Every search takes the decisions it takes alone.
// The queue owns the jobs whose searches are in flight (or, for a target search, wait for it) and finishes them in the order of
// the gas list; a job handed to add() is out of the caller's reach, so nothing of it can be held across a flush().
class SearchQueue {
 public:
  explicit SearchQueue(const Run& run) : run_(run) {}
  SearchQueue(const SearchQueue&) = delete;
  SearchQueue& operator=(const SearchQueue&) = delete;
  // the search threads read the jobs: they end before the jobs go (an error elsewhere unwinds through here)
  ~SearchQueue() {
    if (job_ && !leaving()) (void)ecckd_find_g_gases_wait(job_);
  }

  // All gases of the run stay resident until their searches are over: when the device runs short (3 x nlay + 8 rows of doubles
  // per gas, and the spectra it is made from while it is prepared), the searches in flight are finished first.
  // (a target search needs every gas resident: it fails rather than flush)
  void make_room(size_t nwav) {
    if (pending_.empty() || nwav == 0 || run_.st.target_mode) return;
    size_t free_b = 0, total_b = 0;
    const double need = 6.0 * 60.0 * 8.0 * (double)nwav;
    ck(ecckd_mem_info(run_.dev.ctx(), &free_b, &total_b));
    if ((double)free_b < need) {           // (blocks parked in the library's allocator count as used: hand them back first)
      ck(ecckd_trim_cache(run_.dev.ctx()));
      ck(ecckd_mem_info(run_.dev.ctx(), &free_b, &total_b));
    }
    if ((double)free_b < need) flush();
  }

  // takes a prepared gas and starts its searches
  void add(std::unique_ptr<GasJob> job) {
    const Settings& st = run_.st;
    pending_.push_back(std::move(job));
    GasJob& gj = *pending_.back();
    if (st.sequential_bands) {
      // one band at a time, here and now
      for (int m = 0; m < (int)gj.mine.size(); ++m) {
        const size_t o = (size_t)m * band_capacity;
        if (st.do_sw) ck(ecckd_gas_set_band_albedo(gj.gas, gj.opts[m].band_albedo));
        ck(ecckd_find_g_band_ex(gj.gas, gj.ib[m], gj.ie[m], gj.tol[m], st.tolerance_tolerance, st.max_iterations, &gj.opts[m], &gj.ngs[m],
                                &gj.bounds[(size_t)m * (band_capacity + 1)], &gj.error[o], &gj.r1[o], &gj.r2[o], band_capacity, &gj.statuses[m],
                                &gj.comp_costs[m]));
      }
    } else if (!st.target_mode) {
      // the bands of this gas side by side, next to the gases whose searches are still running
      if (!job_) ck(ecckd_find_g_gases_begin(st.tolerance_tolerance, st.max_iterations, st.gases_side_by_side, &job_));
      ck(ecckd_find_g_gases_add(job_, &gj.req));
    }                                     // (target_g_points: searched by search_target, once every gas is prepared)
    if (st.sequential_bands || (!st.target_mode && st.gases_side_by_side == 1)) flush();
  }

  // wait for the searches in flight and finish their gases, in the order of the gas list
  void flush() {
    if (job_) {
      ecckd_gas_search_job* j = job_;
      job_ = nullptr;
      ck(ecckd_find_g_gases_wait(j));
    }
    for (std::unique_ptr<GasJob>& gj : pending_) finish(*gj);
    pending_.clear();
  }

  // the requests of the gases that wait (a target search runs them itself, again and again)
  std::vector<ecckd_gas_search> requests() const {
    std::vector<ecckd_gas_search> reqs;
    for (const std::unique_ptr<GasJob>& gj : pending_) reqs.push_back(gj->req);
    return reqs;
  }

  std::vector<BandResult> take_results() { return std::move(results_); }

 private:
  // what follows a gas's searches (:1396-1414): log, median sorting variable of every g point, the ranks as the searches left them
  void finish(GasJob& gj) {
    const Device& dev = run_.dev;
    const int nmine = (int)gj.mine.size();
    LOG("*** G POINTS OF %s\n", upper(run_.st.gas_list[gj.gi]).c_str());
    for (int m = 0; m < nmine; ++m) {
      const int b = gj.mine[m];
      LOG("  Band %d: %g-%g cm-1\n", b, gj.ord.bands.bound1[b], gj.ord.bands.bound2[b]);
      const size_t o = (size_t)m * band_capacity;
      const int ng = gj.ngs[m];
      LOG("    %s: %d g points, computational cost = %g\n", ecckd_partition_status_string(gj.statuses[m]), ng, gj.comp_costs[m]);
      BandResult br;
      br.gas = gj.gi; br.band = b; br.ng = ng; br.status = gj.statuses[m]; br.comp_cost = gj.comp_costs[m];
      br.ibegin = gj.ord.ibegin[b]; br.iend = gj.ord.iend[b];
      br.median.resize(ng);
      ck(ecckd_gas_median_sorting_variable(gj.gas, gj.d_sv_sorted.as<double>(), ng, &gj.r1[o], &gj.r2[o], br.median.data()));
      br.rank1.assign(gj.r1.begin() + o, gj.r1.begin() + o + ng);
      br.rank2.assign(gj.r2.begin() + o, gj.r2.begin() + o + ng);
      br.error.assign(gj.error.begin() + o, gj.error.begin() + o + ng);
      for (int k = 0; k < ng; ++k)
        LOG("    g point %d: ranks %lld-%lld, error %g K d-1\n", k, (long long)gj.r1[o + k], (long long)gj.r2[o + k], gj.error[o + k]);
      // the ranks of this band as the search left them (sub-bands and base splits re-rank inside a band)
      br.rank_slice.resize((size_t)(br.iend - br.ibegin + 1));
      ck(ecckd_d2h(dev.ctx(), br.rank_slice.data(), gj.ord.d_rank.as<int32_t>() + br.ibegin, br.rank_slice.size() * sizeof(int32_t)));
      results_.push_back(std::move(br));
    }
    if (!gj.keeps_gas) ck(ecckd_gas_destroy(gj.gas));
    gj.gas = nullptr;
    LOG("\n");
  }

  const Run& run_;
  std::vector<BandResult> results_;                 // the searches of this process, finished
  ecckd_gas_search_job* job_ = nullptr;             // declared before the jobs: they are destroyed first, after ~SearchQueue waited
  std::vector<std::unique_ptr<GasJob>> pending_;
};

// ---- target_g_points: all gases are prepared and resident; one blocking call searches them, trial after trial ----
struct TargetOutcome {
  int status = 0, ng = 0;
  double scaling = 1.0;
  std::vector<double> tolerance, trial_scaling;   // the tolerances used [nband]; the scaling of every trial
  std::vector<int> trial_ng;
};

TargetOutcome search_target(const Settings& st, std::vector<ecckd_gas_search> reqs, int ngas, int nband) {
  TargetOutcome t;
  LOG("*** SEARCHING FOR THE TOLERANCE SCALING THAT GIVES %d G POINTS\n", st.target_g_points);
  const int capacity = std::max(1, st.target_max_trials) + 1;
  int ntrial = 0;
  t.tolerance.assign((size_t)ngas * nband, 0.0);
  t.trial_scaling.assign(capacity, 0.0);
  t.trial_ng.assign(capacity, 0);
  struct Names { const std::vector<std::string>* gas; } names{&st.gas_list};
  ck(ecckd_find_g_gases_target_observe(
      [](int trial, double scaling, int ng_total, int n, const int* ng_per_gas, void* user) {
        std::string per_gas;
        for (int k = 0; k < n; ++k) per_gas += " " + (*static_cast<Names*>(user)->gas)[k] + " " + std::to_string(ng_per_gas[k]);
        LOG("  Trial %d: scaling %.17g: %d g points (%s )\n", trial, scaling, ng_total, per_gas.c_str());
      },
      &names));
  const int rc = ecckd_find_g_gases_target((int)reqs.size(), reqs.data(), nband * (1 - ngas), st.target_g_points, st.target_resolution,
                                           st.target_max_trials, st.tolerance_tolerance, st.max_iterations, st.gases_side_by_side, &t.scaling,
                                           &t.ng, &t.status, t.tolerance.data(), &ntrial, t.trial_scaling.data(),
                                           t.trial_ng.data(), capacity);
  ecckd_find_g_gases_target_observe(nullptr, nullptr);
  ck(rc);
  t.trial_scaling.resize(ntrial);
  t.trial_ng.resize(ntrial);
  t.tolerance.resize(nband);         // every gas has the same tolerances: those of the first
  static const char* const outcome[] = {"the target was hit", "the scaling is resolved and the count steps over the target",
                                        "the trials are spent", "the target is out of reach"};
  LOG("  %d trials: %d g points at scaling %.17g (%s)\n", ntrial, t.ng, t.scaling, outcome[t.status & 3]);
  std::string used;
  for (double tol : t.tolerance) {
    char buf[40];
    std::snprintf(buf, sizeof buf, " %.17g", tol);
    used += buf;
  }
  LOG("  heating_rate_tolerance used:%s\n\n", used.c_str());
  if (st.target_exact && t.status != 0)
    fail(ECCKD_PROCESSING_ERROR, "target_exact: no tolerance scaling gives %d g points (nearest: %d at scaling %.17g, search status %d)",
         st.target_g_points, t.ng, t.scaling, t.status);
  return t;
}

// ---- several processes: process 0 adds the others' searches to its own ----
// -> the result of every (gas, band), [ngas][nband]: pointers into `results`, which is not to change while they are used
std::vector<const BandResult*> collect_parts(const Settings& st, uint64_t identity, int ngas, int nband, std::vector<BandResult>& results) {
  for (int r = 1; r < st.world; ++r) {
    const std::string path = st.part(r);
    std::vector<BandResult> part = read_part(path, st.part_timeout, st.run_id, identity);
    for (BandResult& br : part) results.push_back(std::move(br));
    std::remove(path.c_str());
  }
  std::vector<const BandResult*> by_task((size_t)ngas * nband, nullptr);
  for (const BandResult& br : results) {
    if (br.gas < 0 || br.gas >= ngas || br.band < 0 || br.band >= nband || by_task[(size_t)br.gas * nband + br.band])
      fail(ECCKD_PROCESSING_ERROR, "Search of gas %d, band %d reported twice or out of range", br.gas, br.band);
    by_task[(size_t)br.gas * nband + br.band] = &br;
  }
  return by_task;
}

// ---- the constituents of the overlap ----
// the cloud (:552-652): bands split into g points of equal solar energy along the cloud's own ordering
GasResult cloud_constituent(const Run& run, const BandTable& bands, const std::vector<double>& ssi) {
  const Device& dev = run.dev;
  const std::string& cloud_str = run.st.cloud;
  const int nband = bands.nband;
  const size_t nwav = bands.nwav;
  GasResult res;
  res.molecule = cloud_str;
  LOG("*** FINDING G POINTS FOR %s\n", cloud_str.c_str());
  double max_reflectance_range = 0.26;
  run.config.read(max_reflectance_range, "max_reflectance_range", cloud_str.c_str());
  Ordering co = read_ordering(run.config, run.paths, cloud_str);
  // (the reference does not check this)
  if (co.bands.nwav != nwav || ssi.size() != nwav || co.bands.nband != nband)
    fail(ECCKD_PARAMETER_ERROR, "The ordering of %s has %zu wavenumbers in %d bands, the gases %zu in %d (ssi %zu)", cloud_str.c_str(),
         co.bands.nwav, co.bands.nband, nwav, nband, ssi.size());
  DevBuf d_ssi_c, d_sv_c;
  d_ssi_c.upload(dev, ssi);
  d_sv_c.upload(dev, co.sorting_variable);
  co.d_rank.upload(dev, co.rank);
  const int cloud_capacity = 4096;
  std::vector<int> band_number(cloud_capacity), ngb(nband);
  std::vector<int64_t> r1(cloud_capacity), r2(cloud_capacity);
  std::vector<double> err(cloud_capacity), med(cloud_capacity);
  int ngc = 0;
  ck(ecckd_cloud_partition_dev(dev.ctx(), nwav, d_ssi_c.as<double>(), co.d_rank.as<int32_t>(), d_sv_c.as<double>(), nband,
                               co.ibegin.data(), co.iend.data(), max_reflectance_range, cloud_capacity, ngb.data(), &ngc,
                               band_number.data(), r1.data(), r2.data(), err.data(), med.data()));
  res.n_g_points = ngb;
  res.band_number.assign(band_number.begin(), band_number.begin() + ngc);
  res.rank1.assign(r1.begin(), r1.begin() + ngc);
  res.rank2.assign(r2.begin(), r2.begin() + ngc);
  res.error.assign(err.begin(), err.begin() + ngc);
  res.sorting_variable.assign(med.begin(), med.begin() + ngc);
  for (int k = 0; k < ngc; ++k)
    LOG("  Band %d, g point %d: ranks %lld-%lld, sorting variable range %g\n", res.band_number[k], k, (long long)res.rank1[k],
        (long long)res.rank2[k], res.error[k]);
  std::vector<int32_t> gr1(res.rank1.begin(), res.rank1.end()), gr2(res.rank2.begin(), res.rank2.end());
  res.d_g_point.alloc(dev, nwav * sizeof(int32_t));
  ck(ecckd_gas_g_point_dev(dev.ctx(), nwav, co.d_rank.as<int32_t>(), ngc, gr1.data(), gr2.data(), res.d_g_point.as<int32_t>()));
  ck(ecckd_synchronize(dev.ctx()));
  LOG("\n");
  return res;
}

// a gas from the results of its bands; `rank`: the rank of its ordering file, into which the bands' slices go
GasResult gas_constituent(const Run& run, int gi, const BandResult* const* by_band, const BandTable& bands, std::vector<int32_t> rank) {
  const std::string& name = run.st.gas_list[gi];
  GasResult res;
  res.molecule = name;
  for (int b = 0; b < bands.nband; ++b) {
    const BandResult* br = by_band[b];
    if (!br) fail(ECCKD_PROCESSING_ERROR, "No process searched band %d of %s", b, name.c_str());
    if (br->ibegin < 0 || br->iend >= (int64_t)bands.nwav || (int64_t)br->rank_slice.size() != br->iend - br->ibegin + 1)
      fail(ECCKD_PROCESSING_ERROR, "Rank slice of band %d of %s does not fit", b, name.c_str());
    std::copy(br->rank_slice.begin(), br->rank_slice.end(), rank.begin() + br->ibegin);
    res.n_g_points.push_back(br->ng);
    for (int k = 0; k < br->ng; ++k) {
      res.band_number.push_back(b);
      res.rank1.push_back(br->rank1[k]);
      res.rank2.push_back(br->rank2[k]);
      res.error.push_back(br->error[k]);
      res.sorting_variable.push_back(br->median[k]);
    }
  }
  // SingleGasData::store_g_points (single_gas_data.h:56-62) with the (possibly re-ranked) ranks
  const int ngp = (int)res.rank1.size();
  std::vector<int32_t> gr1(res.rank1.begin(), res.rank1.end()), gr2(res.rank2.begin(), res.rank2.end());
  DevBuf d_rank;
  d_rank.upload(run.dev, rank);
  res.d_g_point.alloc(run.dev, bands.nwav * sizeof(int32_t));
  ck(ecckd_gas_g_point_dev(run.dev.ctx(), bands.nwav, d_rank.as<int32_t>(), ngp, gr1.data(), gr2.data(), res.d_g_point.as<int32_t>()));
  ck(ecckd_synchronize(run.dev.ctx()));
  return res;
}

// ---- spectral overlap of the constituents (:1452-1483) and the merged map; fills every constituent's g_min / g_max ----
struct MergedMap {
  int ng = 0;
  std::vector<int> band_number;      // per merged g point
  DevBuf d_g_point;
  std::vector<int32_t> g_point;      // per wavenumber
};

MergedMap overlap_constituents(const Device& dev, std::vector<GasResult>& gases, const BandTable& bands) {
  const int nconst = (int)gases.size();
  MergedMap map;
  LOG("*** COMPUTING SPECTRAL OVERLAP OF GASES\n");
  std::vector<int> n_g_points, gas_offset;
  std::vector<double> sorting_all;
  int capacity = 1;
  for (const GasResult& g : gases) {
    n_g_points.insert(n_g_points.end(), g.n_g_points.begin(), g.n_g_points.end());
    gas_offset.push_back((int)sorting_all.size());
    sorting_all.insert(sorting_all.end(), g.sorting_variable.begin(), g.sorting_variable.end());
    capacity += (int)g.rank1.size();
  }
  int ng = 0;
  std::vector<int> g_min((size_t)nconst * capacity), g_max((size_t)nconst * capacity);
  map.band_number.resize(capacity);
  ck(ecckd_overlap_g_points(nconst, bands.nband, n_g_points.data(), gas_offset.data(), sorting_all.data(), capacity, &ng, map.band_number.data(),
                            g_min.data(), g_max.data()));
  map.band_number.resize(ng);
  std::vector<const int32_t*> d_gp;
  for (int k = 0; k < nconst; ++k) {
    gases[k].g_min.assign(g_min.begin() + (size_t)k * capacity, g_min.begin() + (size_t)k * capacity + ng);
    gases[k].g_max.assign(g_max.begin() + (size_t)k * capacity, g_max.begin() + (size_t)k * capacity + ng);
    d_gp.push_back(gases[k].d_g_point.as<int32_t>());
  }
  map.d_g_point.alloc(dev, bands.nwav * sizeof(int32_t));
  int64_t n_unassigned = 0;
  ck(ecckd_merge_g_points_dev(dev.ctx(), bands.nwav, nconst, d_gp.data(), ng, capacity, g_min.data(), g_max.data(), map.d_g_point.as<int32_t>(),
                              &n_unassigned));
  map.g_point = map.d_g_point.download<int32_t>();
  if (n_unassigned > 0) WARN("%lld wavenumbers are not assigned to a g point", (long long)n_unassigned);
  LOG("%d g points in total\n", ng);
  map.ng = ng;
  return map;
}

// ---- the g-points file (:1485-1660) ----
void write_g_points_file(const Run& run, const BandTable& bands, const std::vector<double>& ssi, const std::vector<GasResult>& gases,
                         const MergedMap& map, const TargetOutcome& target) {
  const Settings& st = run.st;
  const int ng = map.ng;
  LOG("Writing %s\n", st.output.c_str());
  NcOut file(st.output);
  file.dim("band", bands.nband);
  if (ng > 0) file.dim("g_point", ng);
  std::string molecule_list;
  for (const GasResult& g : gases) {
    file.dim(g.molecule + "_g_point", g.rank1.size());
    molecule_list += (molecule_list.empty() ? "" : " ") + g.molecule;
  }
  file.dim("wavenumber", bands.nwav);
  file.var("n_gases", NC_INT_T, {}, "Number of gases treated");
  file.var("wavenumber1_band", NC_FLOAT_T, {"band"}, "Lower wavenumber bound of band", "cm-1");
  file.var("wavenumber2_band", NC_FLOAT_T, {"band"}, "Upper wavenumber bound of band", "cm-1");
  file.var("band_number", NC_SHORT_T, {"g_point"}, "Band number of each g point");
  if (st.do_sw) file.var("solar_irradiance", NC_FLOAT_T, {"g_point"}, "Solar irradiance across each g point", "W m-2");
  for (const GasResult& g : gases) {
    const std::string m = g.molecule, d = m + "_g_point";
    file.var(m + "_n_g_points", NC_INT_T, {"band"}, "Number of g points in each band");
    file.var(m + "_band_number", NC_SHORT_T, {d}, "Band number of each g point");
    file.var(m + "_rank1", NC_INT_T, {d}, "Rank of first wavenumber in each g point");
    file.var(m + "_rank2", NC_INT_T, {d}, "Rank of last wavenumber in each g point");
    file.var(m + "_error", NC_FLOAT_T, {d}, "Root-mean-squared heating-rate error of each g point", "K d-1");
    file.var(m + "_sorting_variable", NC_FLOAT_T, {d}, "Median sorting variable of each g point");
    file.var(m + "_g_min", NC_INT_T, {"g_point"}, "First single-gas g point contributing to each merged g point");
    file.var(m + "_g_max", NC_INT_T, {"g_point"}, "Last single-gas g point contributing to each merged g point");
  }
  if (st.target_mode) {
    file.dim("target_trial", target.trial_scaling.size());
    file.var("target_g_points", NC_INT_T, {}, "Number of g points asked for");
    file.var("target_search_status", NC_INT_T, {}, "Outcome of the search for the tolerance scaling (0 target hit, 1 resolution reached, 2 trials spent, 3 out of reach)");
    file.var("heating_rate_tolerance_scaling", NC_DOUBLE_T, {}, "Factor applied to the configured heating-rate tolerance");
    file.var("heating_rate_tolerance", NC_DOUBLE_T, {"band"}, "Heating-rate tolerance used in each band", "K d-1");
    file.var("target_trial_scaling", NC_DOUBLE_T, {"target_trial"}, "Tolerance scaling of each trial");
    file.var("target_trial_n_g_points", NC_INT_T, {"target_trial"}, "Total number of g points of each trial");
  }
  file.var("wavenumber", NC_DOUBLE_T, {"wavenumber"}, "Wavenumber", "cm-1");
  file.var("g_point", NC_SHORT_T, {"wavenumber"}, "G point of each wavenumber");
  file.deflate("g_point");                                               // find_g_points.cpp:1580
  for (const GasResult& g : gases) {
    file.var(g.molecule + "_g_point", NC_SHORT_T, {"wavenumber"}, "Single-gas g point of each wavenumber");
    file.deflate(g.molecule + "_g_point");                               // :1587
  }
  file.att(st.do_sw ? "Definition of the spectral intervals of a shortwave CKD model"
                    : "Definition of the spectral intervals of a longwave CKD model", "title");
  file.att(molecule_list, "constituent_id");
  file.att(history_line(run.argc, run.argv), "history");
  file.att(run.config.str(), "config");
  file.end_define();
  file.write("n_gases", {(double)gases.size()});
  file.write("wavenumber1_band", bands.bound1);
  file.write("wavenumber2_band", bands.bound2);
  file.write_as_double("band_number", map.band_number);
  if (st.do_sw) {   // :1620-1633
    std::vector<double> solar(ng, 0.0);
    for (size_t i = 0; i < bands.nwav; ++i) if (map.g_point[i] >= 0) solar[map.g_point[i]] += ssi[i];
    int nbad = 0;
    for (double v : solar) if (v <= 0.0) ++nbad;
    if (nbad) WARN("%d g points have no solar irradiance", nbad);
    file.write("solar_irradiance", solar);
  }
  for (const GasResult& g : gases) {
    const std::string m = g.molecule;
    file.write_as_double(m + "_n_g_points", g.n_g_points);
    file.write_as_double(m + "_band_number", g.band_number);
    file.write_as_double(m + "_rank1", g.rank1);
    file.write_as_double(m + "_rank2", g.rank2);
    file.write(m + "_error", g.error);
    file.write(m + "_sorting_variable", g.sorting_variable);
    file.write_as_double(m + "_g_min", g.g_min);
    file.write_as_double(m + "_g_max", g.g_max);
    file.write_as_double(m + "_g_point", g.d_g_point.download<int32_t>());
  }
  if (st.target_mode) {
    file.write("target_g_points", {(double)st.target_g_points});
    file.write("target_search_status", {(double)target.status});
    file.write("heating_rate_tolerance_scaling", {target.scaling});
    file.write("heating_rate_tolerance", target.tolerance);
    file.write("target_trial_scaling", target.trial_scaling);
    file.write_as_double("target_trial_n_g_points", target.trial_ng);
  }
  file.write("wavenumber", bands.wavenumber);
  file.write_as_double("g_point", map.g_point);
  file.close();
}

}  // namespace

int main(int argc, char** argv) {
  return run(argc, argv, [&](Config& config) -> int {
    SearchPath paths;
    paths.configure(config);
    const Settings st = read_settings(config);
    std::vector<double> ssi;
    if (st.do_sw) ssi = NcIn(paths.find(st.ssi_file_name)).read("solar_spectral_irradiance");
    if (st.target_mode) refuse_unsearchable_target(config, paths, st);
    claim_part_files(st);
    Device dev;
    dev.enable_od_cache();       // a gas's spectrum is the target once and part of the other gases' backgrounds: read once
    const int ngas = (int)st.gas_list.size();
    if (ngas == 0) fail(ECCKD_PARAMETER_ERROR, "No gases specified in \"gases\"");
    if (st.world > 1) LOG("Process %d of %d: the (gas, band) searches are dealt in contiguous shares\n", st.my_rank, st.world);
    const Run run{config, paths, dev, st, argc, argv};

    // ---- the gas loop (:655-1414): read, prepare, start the searches, go on to the next gas ----
    BandTable bands;                                      // of the gases: the first gas's ordering sets it, nothing else does
    int task_begin = 0, task_end = 0;                     // this process's share of the [ngas][nband] searches
    std::vector<std::vector<int32_t>> order_rank(ngas);   // process 0: the rank of every gas as its ordering file has it
    PlanckSource planck;
    SearchQueue queue(run);
    for (int gi = 0; gi < ngas; ++gi) {
      const std::string& gas_str = st.gas_list[gi];
      LOG("*** FINDING G POINTS FOR %s\n", upper(gas_str).c_str());
      queue.make_room(bands.nwav);
      Ordering ord = read_ordering(config, paths, gas_str);
      if (gi == 0) {
        bands = ord.bands;
        deal_tasks(ngas * bands.nband, st.my_rank, st.world, task_begin, task_end);
      } else if (ord.bands.nband != bands.nband || ord.bands.nwav != bands.nwav) {   // (nothing downstream can hold two tables)
        fail(ECCKD_PARAMETER_ERROR, "The ordering of %s has %zu wavenumbers in %d bands, that of %s %zu in %d", gas_str.c_str(),
             ord.bands.nwav, ord.bands.nband, st.gas_list[0].c_str(), bands.nwav, bands.nband);
      }
      if (st.my_rank == 0) order_rank[gi] = ord.rank;
      std::vector<int> mine;
      std::vector<char> is_mine(bands.nband, 0);
      for (int b = 0; b < bands.nband; ++b)
        if (gi * bands.nband + b >= task_begin && gi * bands.nband + b < task_end) {
          mine.push_back(b);
          is_mine[b] = 1;
        }
      if (mine.empty()) {
        LOG("  (searched by other processes)\n\n");
        continue;
      }
      TurnBuffers turn;
      auto job = std::make_unique<GasJob>(gi, std::move(ord), std::move(mine));
      const BandConfig cfg = read_band_config(run, gas_str, job->ord);
      // The first longwave gas lends its Planck matrix to the later ones, whichever process searches them: its ordering is
      // prepared in every band, so that the matrix does not depend on how the tasks were dealt
      subband_setup(dev, job->ord, (gi == 0 && !st.do_sw) ? std::vector<char>(bands.nband, 1) : is_mine);
      prepare_gas(run, *job, cfg, ssi, planck, turn);
      gather_sorting_variable(dev, *job, turn);
      job->set_up_search(cfg, st.do_sw);
      queue.add(std::move(job));
      LOG("\n");
    }
    TargetOutcome target;
    if (st.target_mode) target = search_target(st, queue.requests(), ngas, bands.nband);
    queue.flush();
    planck.release();

    // ---- several processes: the others leave their searches for process 0 ----
    std::vector<BandResult> results = queue.take_results();
    double my_cost = 0.0;
    for (const BandResult& r : results) for (double e : r.error) my_cost += e;
    if (st.world > 1) LOG("Process %d: %zu searches, sum of the g points' errors %.17g K d-1\n", st.my_rank, results.size(), my_cost);
    const uint64_t identity = job_identity(st.run_id, ngas, bands.nband, (uint64_t)bands.nwav);
    if (st.my_rank != 0) {
      write_part(st.part(st.my_rank), results, identity);
      return done(0);
    }
    const std::vector<const BandResult*> by_task = collect_parts(st, identity, ngas, bands.nband, results);

    // ---- the constituents: the cloud, if any, is the first (:650, :1448-1451): first in constituent_id, the overlap and n_gases
    std::vector<GasResult> gases;
    if (st.have_cloud) gases.push_back(cloud_constituent(run, bands, ssi));
    double final_cost = 0.0;
    for (int gi = 0; gi < ngas; ++gi) {
      gases.push_back(gas_constituent(run, gi, &by_task[(size_t)gi * bands.nband], bands, std::move(order_rank[gi])));
      for (double e : gases.back().error) final_cost += e;
    }
    results.clear();
    if (st.world > 1) LOG("Final cost (sum of the g points' errors over all processes): %.17g K d-1\n", final_cost);

    const MergedMap map = overlap_constituents(dev, gases, bands);
    write_g_points_file(run, bands, ssi, gases, map, target);
    return done(0);
  });
}
