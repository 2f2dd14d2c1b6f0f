// target_search.cpp - the heating-rate tolerance that yields a wanted number of g points.  Host-only code.
//
// The reference takes a tolerance and reports how many g points came out; its scripts carry hand-found tables of the
// tolerance per g-point count (test/do_all_lw.sh:44-65), valid for one gas list, band structure and continuum.  Here the
// count is the input: f(s) = the total number of g points when every band's configured tolerance is multiplied by s, and
// the search below looks for the s with f(s) = target.
//
//   1. s = 1.  f == target: status 0.
//   2. Bracket: while f(s) > target double s, while f(s) < target halve s, until the other side of the target (or the
//      target) is met.  s stays in [2^-20, 2^20]; a bracket that does not close in that range: status 3.
//   3. Geometric bisection between lo (ng > target) and hi (ng < target): mid = sqrt(lo * hi) replaces the end of its
//      side.  A hit: status 0.  hi / lo <= 1 + resolution: status 1.  max_trials trials spent (those of step 2
//      included): status 2.
//   4. Without a hit the answer is the trial with the smallest |ng - target|; among equals the one with ng < target, then
//      the larger scaling.
// f is a step function and need not be monotone: nothing below assumes it is.  A step over the target ends with status 1
// and the trials either side of the step are in the trial list.
#include <cmath>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "common.hpp"

namespace {

enum { TS_HIT = 0, TS_RESOLUTION = 1, TS_MAX_TRIALS = 2, TS_NO_BRACKET = 3 };

struct Trial { double scaling; int ng; };

// is trial a a better answer than trial b (step 4)
inline bool better(const Trial& a, const Trial& b, int target) {
  const long long da = std::llabs((long long)a.ng - target), db = std::llabs((long long)b.ng - target);
  if (da != db) return da < db;
  if ((a.ng < target) != (b.ng < target)) return a.ng < target;
  return a.scaling > b.scaling;
}

// The search over a count function; returns the count function's code if it fails, PARAMETER_ERROR when the trial list
// overflows.  *best = index of the answer in `trials`.
int target_search(const std::function<int(double, int*)>& count, int target, double resolution, int max_trials, int capacity,
                  std::vector<Trial>& trials, int* best, int* status) {
  const double s_min = std::ldexp(1.0, -20), s_max = std::ldexp(1.0, 20);
  int rc = ECCKD_OK;
  int ibest = -1;
  auto try_scaling = [&](double s, int* ng) {
    if ((int)trials.size() >= capacity)
      return ecckd::fail(ECCKD_PARAMETER_ERROR, "target search: trial %zu exceeds the caller's capacity %d", trials.size() + 1, capacity);
    *ng = 0;
    const int r = count(s, ng);
    if (r != ECCKD_OK) return r;
    trials.push_back({s, *ng});
    if (ibest < 0 || better(trials.back(), trials[ibest], target)) ibest = (int)trials.size() - 1;
    return (int)ECCKD_OK;
  };
  auto finish = [&](int st) {
    *status = st;
    *best = ibest;
    return (int)ECCKD_OK;
  };

  double s = 1.0;
  int ng = 0;
  if ((rc = try_scaling(s, &ng)) != ECCKD_OK) return rc;
  if (ng == target) return finish(TS_HIT);
  // ---- step 2: bracket ----
  const bool upwards = ng > target;
  double lo = 0.0, hi = 0.0;
  for (;;) {
    const double next = upwards ? 2.0 * s : 0.5 * s;
    if (next > s_max || next < s_min) return finish(TS_NO_BRACKET);
    if ((int)trials.size() >= max_trials) return finish(TS_MAX_TRIALS);
    const double prev = s;
    s = next;
    if ((rc = try_scaling(s, &ng)) != ECCKD_OK) return rc;
    if (ng == target) return finish(TS_HIT);
    if (upwards && ng < target) { lo = prev; hi = s; break; }
    if (!upwards && ng > target) { lo = s; hi = prev; break; }
  }
  // ---- step 3: geometric bisection ----
  for (;;) {
    if (hi / lo <= 1.0 + resolution) return finish(TS_RESOLUTION);
    if ((int)trials.size() >= max_trials) return finish(TS_MAX_TRIALS);
    const double mid = std::sqrt(lo * hi);
    if (!(mid > lo && mid < hi)) return finish(TS_RESOLUTION);      // the ends are neighbouring doubles
    if ((rc = try_scaling(mid, &ng)) != ECCKD_OK) return rc;
    if (ng == target) return finish(TS_HIT);
    if (ng > target) lo = mid; else hi = mid;
  }
}

int check_search_arguments(const char* who, int target_ng, double resolution, int max_trials) {
  ECCKD_REQUIRE(target_ng >= 1, "%s: target_ng = %d, must be at least 1", who, target_ng);
  ECCKD_REQUIRE(resolution > 0.0, "%s: resolution = %g, must be positive", who, resolution);
  ECCKD_REQUIRE(max_trials >= 1, "%s: max_trials = %d, must be at least 1", who, max_trials);
  return ECCKD_OK;
}

void copy_trials(const std::vector<Trial>& trials, int* ntrial, double* trial_scaling, int* trial_ng) {
  *ntrial = (int)trials.size();
  for (size_t i = 0; i < trials.size(); ++i) {
    trial_scaling[i] = trials[i].scaling;
    trial_ng[i] = trials[i].ng;
  }
}

thread_local ecckd_target_trial_fn tl_observer = nullptr;
thread_local void* tl_observer_user = nullptr;

}  // namespace

extern "C" {

int ecckd_target_search(ecckd_count_fn fn, void* user, int target_ng, double resolution, int max_trials, double* scaling,
                        int* ng, int* status, int* ntrial, double* trial_scaling, int* trial_ng, int capacity) {
  ECCKD_REQUIRE(fn, "ecckd_target_search: fn == NULL");
  ECCKD_CHECK(check_search_arguments("ecckd_target_search", target_ng, resolution, max_trials));
  ECCKD_REQUIRE(scaling && ng && status && ntrial && trial_scaling && trial_ng && capacity >= 0, "ecckd_target_search: NULL argument");
  std::vector<Trial> trials;
  int best = -1;
  *ntrial = 0;
  const int rc = target_search(
      [&](double s, int* n) {
        const int r = fn(s, n, user);
        if (r != ECCKD_OK) ecckd::fail(r, "ecckd_target_search: the count function returned %d at scaling %.17g", r, s);
        return r;
      },
      target_ng, resolution, max_trials, capacity, trials, &best, status);
  copy_trials(trials, ntrial, trial_scaling, trial_ng);
  if (rc != ECCKD_OK) return rc;
  *scaling = trials[best].scaling;
  *ng = trials[best].ng;
  return ECCKD_OK;
}

int ecckd_find_g_gases_target_observe(ecckd_target_trial_fn fn, void* user) {
  tl_observer = fn;
  tl_observer_user = user;
  return ECCKD_OK;
}

int ecckd_find_g_gases_target(int ngas, ecckd_gas_search* req, int ng_offset, int target_ng, double resolution, int max_trials,
                              double tolerance_tolerance, int max_iterations, int max_concurrent, double* scaling, int* ng_total,
                              int* status, double* h_tolerance_used, int* ntrial, double* trial_scaling, int* trial_ng, int capacity) {
  ECCKD_REQUIRE(ngas > 0 && req, "ecckd_find_g_gases_target: bad argument");
  ECCKD_CHECK(check_search_arguments("ecckd_find_g_gases_target", target_ng, resolution, max_trials));
  ECCKD_REQUIRE(scaling && ng_total && status && h_tolerance_used && ntrial && trial_scaling && trial_ng && capacity >= 0,
                "ecckd_find_g_gases_target: NULL argument");
  *ntrial = 0;
  std::vector<size_t> tol_offset(ngas);
  size_t ntol = 0;
  for (int k = 0; k < ngas; ++k) {
    const ecckd_gas_search& r = req[k];
    ECCKD_REQUIRE(r.gas && r.nband > 0 && r.heating_rate_tolerance && r.opt && r.ng, "ecckd_find_g_gases_target: request %d is incomplete", k);
    // the base split by wavenumber re-ranks the spectrum in place during a search: such a gas cannot be searched twice
    for (int b = 0; b < r.nband; ++b)
      ECCKD_REQUIRE(r.opt[b].nbase_wn_bound <= 2,
                    "ecckd_find_g_gases_target: request %d, band %d splits its base g point by wavenumber, which re-ranks the spectrum "
                    "during the search: the gas cannot be searched more than once", k, b);
    tol_offset[k] = ntol;
    ntol += (size_t)r.nband;
  }

  // a trial: the requests as they are, with every band's tolerance multiplied by the scaling
  std::vector<ecckd_gas_search> trial_req(ngas);
  std::vector<double> tol(ntol);
  std::vector<int> per_gas(ngas);
  double last_run = 0.0;
  auto run = [&](double s, int* total) {
    for (int k = 0; k < ngas; ++k) {
      trial_req[k] = req[k];
      for (int b = 0; b < req[k].nband; ++b) tol[tol_offset[k] + b] = s * req[k].heating_rate_tolerance[b];
      trial_req[k].heating_rate_tolerance = &tol[tol_offset[k]];
    }
    const int rc = ecckd_find_g_gases(ngas, trial_req.data(), tolerance_tolerance, max_iterations, max_concurrent);
    for (int k = 0; k < ngas; ++k) req[k].rc = trial_req[k].rc;
    if (rc != ECCKD_OK) {
      const std::string message = ecckd_last_error();
      return ecckd::fail(rc, "ecckd_find_g_gases_target: at tolerance scaling %.17g: %s", s, message.c_str());
    }
    long long n = ng_offset;
    for (int k = 0; k < ngas; ++k) {
      per_gas[k] = 0;
      for (int b = 0; b < req[k].nband; ++b) per_gas[k] += req[k].ng[b];
      n += per_gas[k];
    }
    *total = (int)n;
    last_run = s;
    return (int)ECCKD_OK;
  };

  std::vector<Trial> trials;
  int best = -1;
  const int rc = target_search(
      [&](double s, int* n) {
        const int r = run(s, n);
        if (r == ECCKD_OK && tl_observer) tl_observer((int)trials.size(), s, *n, ngas, per_gas.data(), tl_observer_user);
        return r;
      },
      target_ng, resolution, max_trials, capacity, trials, &best, status);
  copy_trials(trials, ntrial, trial_scaling, trial_ng);
  if (rc != ECCKD_OK) return rc;
  const Trial chosen = trials[best];
  if (chosen.scaling != last_run) {
    // the requests' outputs are those of the last trial: search the chosen scaling once more (every interval it asks for is
    // in the gases' memos, so nothing is swept)
    int n = 0;
    ECCKD_CHECK(run(chosen.scaling, &n));
    if (n != chosen.ng)
      return ecckd::fail(ECCKD_PROCESSING_ERROR, "ecckd_find_g_gases_target: scaling %.17g gave %d g points and now gives %d",
                         chosen.scaling, chosen.ng, n);
  }
  for (int k = 0; k < ngas; ++k)
    for (int b = 0; b < req[k].nband; ++b) h_tolerance_used[tol_offset[k] + b] = tol[tol_offset[k] + b];
  *scaling = chosen.scaling;
  *ng_total = chosen.ng;
  return ECCKD_OK;
}

}  // extern "C"
