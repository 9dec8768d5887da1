// lm_rule.hpp — the Levenberg-Marquardt step rule of the estimators that run their loop on the device (resect_kernels.hip calls it
// itself, calib_kernels.hip and rig_kernels.hip through arrowhead_dev.hpp's lm_control_decide, the three alignments --
// align_kernels.hip, camalign_kernels.hip, accalign_kernels.hip -- with point_lm_dev.hpp's point_lm_state behind it):
// accept or reject a candidate, the next damping, and whether the loop has converged.
// What differs between them stays with them: the first evaluation, the iteration cap and the status codes, and the retry while
// a damped system is not positive definite. Host and device code (the host sets the control word's first damping).
#pragma once
#include "device_math.hpp"

namespace cal {

constexpr double kLmLambda0 = 1e-4, kLmLambdaMin = 1e-12, kLmLambdaMax = 1e12;
// A cost cannot tell two points apart whose costs differ by less than its own rounding error: a residual of e pixels at a pixel
// coordinate u carries an error of about eps |u|, its square one of 2 |e| eps |u|. A candidate within kCostSlack eps Sum |e| |u|
// of the current cost is accepted on the model's word (its gradient is known far better than its cost). `noise` is that sum.
constexpr double kCostSlack = 8.0 * 2.220446049250313e-16;

// accept: the candidate becomes the current point; converged: the loop ends, there or at the point kept; lambda: the next damping
struct LmVerdict { bool accept, converged; double lambda; };

// kept: the candidate is finite and lost no observation; small: the step that made it was below the tolerance. At
// lambda <= kLmLambda0 the damped step is the Gauss-Newton step to 1e-4, so a small one means converged -- accepted or not.
DEV LmVerdict lm_rule(bool kept, double candidate, double current, double noise, bool small, double lambda) {
  LmVerdict v;
  v.accept = kept && candidate <= current + kCostSlack * noise;
  v.converged = small && kept && lambda <= kLmLambda0;
  v.lambda = v.accept ? fmax(lambda * 0.1, kLmLambdaMin) : v.converged ? lambda : fmin(lambda * 10.0, kLmLambdaMax);
  return v;
}

// One decision of a loop whose control word lives in device memory and whose candidate is judged for all blocks at once (the
// arrowhead estimators: arrowhead_dev.hpp's lm_control_decide calls it): the first evaluation only installs the start -- a start
// that is not kept, or that has no valid observation, ends the loop --, every later one asks lm_rule, and the iteration cap ends
// the loop at the point kept. The status codes stay with the caller: it maps `outcome`.
enum LmOutcome { kLmRunning = 0, kLmConverged = 1, kLmBadStart = 2, kLmOutOfIterations = 3 };
struct LmLoopStep { bool accept; int outcome; double lambda; int iterations; };
DEV LmLoopStep lm_loop_decision(bool first, bool kept, bool any_valid, double candidate, double current, double noise, bool small, double lambda,
                                int iterations, int max_iterations) {
  LmLoopStep s;
  s.accept = first; s.outcome = kLmRunning; s.lambda = lambda; s.iterations = iterations;
  if (first) {
    if (!kept || !any_valid) s.outcome = kLmBadStart;
  } else {
    const LmVerdict v = lm_rule(kept, candidate, current, noise, small, lambda);
    s.accept = v.accept; s.lambda = v.lambda;
    if (v.converged) s.outcome = kLmConverged;
  }
  if (s.outcome == kLmRunning && iterations >= max_iterations) s.outcome = kLmOutOfIterations;
  if (s.outcome == kLmRunning) ++s.iterations;
  return s;
}

// The same decision for a loop over ONE point (point_lm_dev.hpp; tests/cpp/arg_rules_check.cpp holds it to the decision that
// align_kernels.hip once spelt out): there is no block that could be left without a valid
// observation, the samples that take part are fixed by the host.
DEV LmLoopStep lm_point_decision(bool first, bool kept, double candidate, double current, double noise, bool small, double lambda, int iterations,
                                 int max_iterations) {
  return lm_loop_decision(first, kept, true, candidate, current, noise, small, lambda, iterations, max_iterations);
}

}  // namespace cal
