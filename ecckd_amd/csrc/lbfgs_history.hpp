// lbfgs_history.hpp - the host side of the compact L-BFGS representation of ecckd_opt_minimize (optimize.hip): S^T Y and
// Y^T Y of the stored curvature pairs, by ring slot, and the small dense algebra on them.  The pairs themselves live on the
// device; the host only sees their dot products, which the k_lb_update / k_lb_finish pair delivers as
//   dots[0] |q|^2, dots[1 .. 1+M) S_a.q, dots[1+M .. 1+2M) Y_a.q  (a: the pairs of the direction, oldest first, the pending last)
//   dots[1+2M ..] of the pending pair (s, y): s.y, y.y, then s.Y_a, S_a.y, y.Y_a (M each) for the stored pairs a.
// Plain C++, no device code: tools/check_opt_tables.cpp runs it on its own.
#pragma once

namespace ecckd {

struct LbfgsHistory {
  static constexpr int M = 6;   // = LB_M of the k_lb_* kernels
  double SY[M][M] = {}, YY[M][M] = {};
  int ord[M] = {};        // ring slots of the stored pairs, oldest first
  int n = 0;              // stored pairs
  double gamma = 1.0;
  bool pending = false;   // a pair has been written to `pend_slot`; its dots arrive with the next direction's
  int pend_slot = 0;

  // Take the pending pair in as the newest if its curvature s.y is positive, else drop it.
  void absorb_pending(const double* dots) {
    if (!pending) return;
    pending = false;
    const double* rp = dots + 1 + 2 * M;
    const double sy = rp[0], yy = rp[1];
    if (!(sy > 1.0e-12)) return;
    for (int a = 0; a < n; ++a) {
      SY[pend_slot][ord[a]] = rp[2 + a];
      SY[ord[a]][pend_slot] = rp[2 + M + a];
      YY[pend_slot][ord[a]] = YY[ord[a]][pend_slot] = rp[2 + 2 * M + a];
    }
    SY[pend_slot][pend_slot] = sy;
    YY[pend_slot][pend_slot] = yy;
    ord[n++] = pend_slot;
    gamma = sy / yy;
  }

  // forget every pair: the next direction is the projected steepest descent
  void restart() { n = 0; }

  // ring slots of the stored pairs, oldest first, padded with 0 to M
  void slots(int* slot) const {
    for (int a = 0; a < M; ++a) slot[a] = a < n ? ord[a] : 0;
  }

  // Coefficients of the direction d = -gamma q + sum_a (cy[a] Y_a - cs[a] S_a), R the upper triangle of S^T Y, D its diagonal:
  // u = R^-1 p, top = R^-T ((D + gamma YY) u - gamma qy), cs = top, cy = gamma u.  Returns the gamma to use.
  double coefficients(const double* dots, double* cs, double* cy) const {
    const double g = n > 0 ? gamma : 1.0;
    for (int a = 0; a < M; ++a) { cs[a] = 0.0; cy[a] = 0.0; }
    if (n == 0) return g;
    const double* pv = dots + 1;
    const double* qv = dots + 1 + M;
    double u[M], w[M], top[M];
    for (int a = n - 1; a >= 0; --a) {
      double v = pv[a];
      for (int c = a + 1; c < n; ++c) v -= SY[ord[a]][ord[c]] * u[c];
      u[a] = v / SY[ord[a]][ord[a]];
    }
    for (int a = 0; a < n; ++a) {
      double v = SY[ord[a]][ord[a]] * u[a] - g * qv[a];
      for (int c = 0; c < n; ++c) v += g * YY[ord[a]][ord[c]] * u[c];
      w[a] = v;
    }
    for (int a = 0; a < n; ++a) {
      double v = w[a];
      for (int c = 0; c < a; ++c) v -= SY[ord[c]][ord[a]] * top[c];
      top[a] = v / SY[ord[a]][ord[a]];
    }
    for (int a = 0; a < n; ++a) { cs[a] = top[a]; cy[a] = g * u[a]; }
    return g;
  }

  // The ring slot the next pair goes to: a free one, or the oldest pair's when the ring is full (that pair is dropped).
  // The pair is pending until absorb_pending sees its dots.
  int next_slot() {
    if (n == M) {
      pend_slot = ord[0];
      for (int a = 1; a < M; ++a) ord[a - 1] = ord[a];
      --n;
    } else {
      bool used[M] = {};
      for (int a = 0; a < n; ++a) used[ord[a]] = true;
      pend_slot = 0;
      while (used[pend_slot]) ++pend_slot;
    }
    pending = true;
    return pend_slot;
  }
};

}  // namespace ecckd
