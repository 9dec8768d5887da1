// point_lm_dev.hpp — the Levenberg-Marquardt loop over ONE point with a dense normal matrix, as the alignment kernels run it
// (align_kernels.hip: 7 unknowns; camalign_kernels.hip: 7; accalign_kernels.hip: 13). The control word begins with kernels.hpp's
// PointLmControl and lives in device memory; there are two slots, the current point and the candidate. One iteration is two
// launches, enqueued without the host reading anything back: the estimator's own evaluation of the candidate (a Gram matrix of
// the rows [J | r], summed in a fixed order), then ONE wave that decides and steps:
//   point_lm_state        the head after the rule's decision -- the kernel asks lm_rule.hpp's lm_point_decision (the camera, whose
//                         pairs can drop out, lm_loop_decision): accept or reject, the next damping, the end of the loop --, with
//                         the one mapping of the outcome to CALICO_ALIGN_*
//   point_lm_restore      rejected: the step starts at the old point's Gram matrix again
//   point_lm_damped_step  the normal equations at (1 + lambda) diag, ten times the damping while they are not positive definite,
//                         the step solved into the right-hand side
//   point_lm_rotate, _add3, _add1   the pieces of the retraction, each returning its relative step size; point_lm_step_size
//   point_lm_write        lane 0 writes the head
// and after the loop point_lm_finish: the undamped inverse normal matrix, column by column. What stays with an estimator: how
// its partials are summed, which fields its point has, and what else its final kernel reports. Device code only.
#pragma once
#include "kernels.hpp"
#include "lm_rule.hpp"
#include "resect_dev.hpp"

namespace cal {

namespace {

DEV bool point_lm_free(unsigned bits, int i) { return ((bits >> i) & 1u) != 0u; }
DEV double point_lm_amax3(const double* v) { return fmax(fabs(v[0]), fmax(fabs(v[1]), fabs(v[2]))); }
DEV bool point_lm_finite(const double* p, int n) {
  bool ok = true;
  for (int j = 0; j < n; ++j) ok = ok && __builtin_isfinite(p[j]);
  return ok;
}

// ---- how entry (i, j) of the Gram matrix of [J | r] is read; the last column is r ------------------------------------------------
// the upper triangle of 8 columns, row-major
struct GramTriangle8 {
  const double* g;
  static constexpr int kLast = 7;
  DEV static int at(int r, int c) { return r * 8 - (r * (r - 1)) / 2 + (c - r); }      // r <= c
  DEV double operator()(int i, int j) const { return g[i < j ? at(i, j) : at(j, i)]; }
};
// full and symmetric, 14 x 14
struct GramFull14 {
  const double* g;
  static constexpr int kLast = 13;
  DEV double operator()(int i, int j) const { return g[i * 14 + j]; }
};

// The N x N normal matrix (row-major) and the right-hand side -gradient of the parameters first .. first + N - 1; a parameter
// that is not estimated has a unit row; the diagonal is scaled by diag_scale.
template <class Gram>
DEV void point_lm_normal(Gram g, int first, int N, unsigned free_bits, double diag_scale, double* H, double* rhs, int lane) {
  for (int e = lane; e < N * N; e += 64) {
    const int i = e / N, j = e - N * i;
    const bool both = point_lm_free(free_bits, first + i) && point_lm_free(free_bits, first + j);
    const double v = both ? g(first + i, first + j) : (i == j ? 1.0 : 0.0);
    H[e] = i == j ? v * diag_scale : v;
  }
  if (lane < N) rhs[lane] = point_lm_free(free_bits, first + lane) ? -g(first + lane, Gram::kLast) : 0.0;
  wave_fence();
}

// ---- the decision ---------------------------------------------------------------------------------------------------------------
// What lane 0 writes to the head after the decision and the step.
struct PointLmState { int done, status, cur, iterations; double lambda, initial_cost; };

// The head after the rule's decision s, with the one mapping of its outcome to CALICO_ALIGN_*; cost: the candidate's, the loop's
// initial cost if this is the start.
DEV PointLmState point_lm_state(const PointLmControl& h, const LmLoopStep& s, double cost) {
  const bool first = h.first != 0;
  PointLmState st;
  st.done = s.outcome != kLmRunning ? 1 : 0;
  st.status = s.outcome == kLmConverged ? CALICO_ALIGN_OK : s.outcome == kLmBadStart ? CALICO_ALIGN_DEGENERATE
              : s.outcome == kLmOutOfIterations ? CALICO_ALIGN_NOT_CONVERGED : h.status;
  st.cur = s.accept ? h.cur ^ 1 : h.cur;
  st.iterations = s.iterations; st.lambda = s.lambda;
  st.initial_cost = first ? cost : h.initial_cost;
  return st;
}

// rejected: the step starts at the old point again
DEV void point_lm_restore(double* g, const double* kept_g, int n, bool rejected, int lane) {
  if (rejected)
    for (int e = lane; e < n; e += 64) g[e] = kept_g[e];
  wave_fence();
}

// The damped step of the N parameters into rhs. false: not positive definite at any damping; the loop ends.
template <class Gram>
DEV bool point_lm_damped_step(Gram g, int N, unsigned free_bits, PointLmState* st, double* H, double* rhs, int lane) {
  bool pd = false;
#pragma unroll 1
  for (int tries = 0; tries < 26 && !pd; ++tries) {
    point_lm_normal(g, 0, N, free_bits, 1.0 + st->lambda, H, rhs, lane);
    pd = lds_chol(H, N, lane);
    if (!pd) {
      if (st->lambda >= kLmLambdaMax) break;
      st->lambda = fmin(st->lambda * 10.0, kLmLambdaMax);
    }
  }
  if (pd) lds_chol_solve(H, rhs, N, lane);
  else { st->status = CALICO_ALIGN_NOT_POSITIVE_DEFINITE; st->done = 1; }
  return pd;
}

// ---- the retraction: lane 0 writes the candidate, every lane gets the group's relative step size ---------------------------------
// q_to <- canonical(exp([d]x) q); held: the same bits, not the product with the identity normalised again
DEV double point_lm_rotate(const double* q, const double* d, bool held, double* q_to, int lane) {
  const Q4 q0 = quat_at(q), qc = canonical(quat_mul(angle_axis_to_quat(mk(d[0], d[1], d[2])), q0));
  if (lane == 0) { q_to[0] = held ? q0.x : qc.x; q_to[1] = held ? q0.y : qc.y; q_to[2] = held ? q0.z : qc.z; q_to[3] = held ? q0.w : qc.w; }
  return point_lm_amax3(d);
}
// x_to <- x + d, max |d_i| / max(1, max |x_i|)
DEV double point_lm_add3(const double* x, const double* d, double* x_to, int lane) {
  const double x0 = x[0], x1 = x[1], x2 = x[2];
  if (lane == 0) { x_to[0] = x0 + d[0]; x_to[1] = x1 + d[1]; x_to[2] = x2 + d[2]; }
  return point_lm_amax3(d) / fmax(1.0, fmax(fabs(x0), fmax(fabs(x1), fabs(x2))));
}
DEV double point_lm_add1(double x, double d, double* x_to, int lane) {
  if (lane == 0) *x_to = x + d;
  return fabs(d) / fmax(1.0, fabs(x));
}
// the largest of the groups' sizes; a step that is not finite is a large one (the size is only ever compared with the tolerance)
DEV double point_lm_step_size(double a, double b, double c) {
  const double step = fmax(a, fmax(b, c));
  return __builtin_isfinite(step) ? step : 1e300;
}

DEV void point_lm_write(PointLmControl* h, int lane, const PointLmState& st, double step) {
  if (lane != 0) return;
  h->done = st.done; h->status = st.status; h->cur = st.cur; h->first = 0; h->iterations = st.iterations; h->lambda = st.lambda;
  h->initial_cost = st.initial_cost; h->step = step;
}

// ---- after the loop ---------------------------------------------------------------------------------------------------------------
// The undamped inverse normal matrix at the result into cov (N x N; zero rows and columns for what is not estimated), cov_ok,
// the final cost, and NOT_POSITIVE_DEFINITE where there is no inverse. Returns whether there is.
template <class Gram>
DEV bool point_lm_finish(PointLmControl* h, Gram g, int N, unsigned free_bits, double cost, double* H, double* rhs, double* cov, int lane) {
  point_lm_normal(g, 0, N, free_bits, 1.0, H, rhs, lane);
  const bool pd = lds_chol(H, N, lane);
  if (pd) {
#pragma unroll 1
    for (int j = 0; j < N; ++j) {
      if (lane < N) rhs[lane] = lane == j ? 1.0 : 0.0;
      wave_fence();
      lds_chol_solve(H, rhs, N, lane);
      if (lane < N) cov[lane * N + j] = point_lm_free(free_bits, lane) && point_lm_free(free_bits, j) ? rhs[lane] : 0.0;
      wave_fence();
    }
  }
  if (lane == 0) {
    h->cov_ok = pd ? 1 : 0;
    if (!pd) h->status = CALICO_ALIGN_NOT_POSITIVE_DEFINITE;
    h->final_cost = cost;
  }
  return pd;
}

}  // namespace
}  // namespace cal
