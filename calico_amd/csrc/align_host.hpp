// align_host.hpp — what the hosts of the alignment family share (imu_align.cpp, camera_align.cpp, accel_align.cpp; their kernels
// share point_lm_dev.hpp): the trajectory's upload, who stays on its valid knots, the control word's head, the loop's launches
// and the covariance's way out. Argument checks and summaries stay with each call.
#pragma once
#include <algorithm>
#include <cstdint>

#include "arg_rules.hpp"
#include "free_call.hpp"
#include "kernels.hpp"
#include "lm_rule.hpp"

namespace cal {

// The spline on the device; `spline` is what the kernels take.
struct SplineOnDevice {
  FreeBuf<double> knots, basis, ctrl;
  AlignSpline spline = {};
  hipError_t upload(int order, int n_knots, const double* h_knots, const double* h_basis, const double* h_ctrl) {
    const int n_valid = spline_valid_knots(order, n_knots);
    hipError_t e = knots.upload(h_knots, size_t(n_knots));
    if (e == hipSuccess) e = basis.upload(h_basis, size_t(n_valid - 1) * order * order);
    if (e == hipSuccess) e = ctrl.upload(h_ctrl, size_t(n_knots - order) * 6);
    spline.k = order; spline.n_valid = n_valid; spline.knots = knots.p; spline.basis = basis.p; spline.ctrl = ctrl.p;
    return e;
  }
};

// The stamps that every latency of [lat_lo, lat_hi] keeps on the valid knots -- and that lie there themselves: the stamp's
// segment is the one the optimiser evaluates.
struct ValidKnots {
  double t0, t1, lat_lo, lat_hi;
  ValidKnots(int order, int n_knots, const double* knots, double lo, double hi)
      : t0(knots[order - 1]), t1(knots[order - 1 + spline_valid_knots(order, n_knots) - 1]), lat_lo(lo), lat_hi(hi) {}
  bool from(double s) const { return s - lat_hi >= t0 && s >= t0; }
  bool until(double s) const { return s - lat_lo <= t1 && s <= t1; }
  // [*first, *end) of the sorted stamps
  void trim(const double* stamps, int64_t n, int64_t* first, int64_t* end) const {
    *first = 0; *end = n;
    while (*first < n && !from(stamps[*first])) ++*first;
    while (*end > *first && !until(stamps[*end - 1])) --*end;
  }
};

// the head of a control word that is otherwise zero: the loop has not evaluated its start
inline void start_point_lm(PointLmControl* h) { h->status = CALICO_ALIGN_NOT_CONVERGED; h->first = 1; h->lambda = kLmLambda0; }

// n iterations enqueued without a read: the first launch evaluates the start, every later one a candidate, launches behind the end
// of the loop return at once. The call's final launches follow, then ONE download of the control word.
template <class Iterate>
hipError_t enqueue_point_lm(int n, Iterate iterate) {
  hipError_t e = hipSuccess;
  for (int it = 0; it < n && e == hipSuccess; ++it) e = iterate();
  return e;
}

// the N x N covariance, or zeros where there is none
inline void give_covariance(double* out, const double* cov, int N, bool ok) {
  if (!out) return;
  if (ok) std::copy(cov, cov + N * N, out);
  else std::fill(out, out + N * N, 0.0);
}

}  // namespace cal
