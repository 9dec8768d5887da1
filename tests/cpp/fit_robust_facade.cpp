// fit_robust_facade.cpp — Trajectory::FitSplineRobust / BSpline6::FitToDataRobust (include/calico/calico.hpp) from C++.
// Without arguments, host only: the solve is replaced through BSpline6::robust_fit_solver() by a recorder, so that what the facade
// hands to calico_fit_spline_robust (knots and basis as FitSpline builds them, the unwrapped axis-angle data, the weights, both
// option structs) and what it makes of every return code are checked on a machine without a GPU.
// With the argument "device": the call itself on device 0 -- poses with a tenth turned by 0.5 rad come back with robust weights
// that single out the turned poses, and max_iterations 0 is FitSplineSmooth. Built with -DCALICO_TEST_HOOKS.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "calico/calico.hpp"

using namespace calico;  // NOLINT

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

namespace {
struct Recorded {
  int calls = 0, order = 0;
  std::vector<double> knots, basis, stamps, data, weights;
  bool has_weights = false;
  calico_spline_fit_options fit{};
  calico_spline_robust_options robust{};
  int32_t code = CALICO_OK;
} rec;

int32_t recorder(int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n, const double* stamps, const double* data6,
                 const double* weights, const calico_spline_fit_options* fit, const calico_spline_robust_options* robust, double* ctrl_out,
                 double* robust_weights_out, double* residuals_out, calico_spline_robust_summary* summary) {
  rec.calls += 1; rec.order = order;
  rec.knots.assign(knots, knots + n_knots);
  rec.basis.assign(basis, basis + size_t(n_knots - 2 * order + 1) * order * order);
  rec.stamps.assign(stamps, stamps + n); rec.data.assign(data6, data6 + n * 6);
  rec.has_weights = weights != nullptr;
  if (weights) rec.weights.assign(weights, weights + n * 2); else rec.weights.clear();
  rec.fit = *fit; rec.robust = *robust;
  if (rec.code != CALICO_OK && rec.code != CALICO_INTERNAL) return rec.code;
  for (int i = 0; i < (n_knots - order) * 6; ++i) ctrl_out[i] = 0.5 * i;
  for (int64_t j = 0; j < n * 2; ++j) { robust_weights_out[j] = 1.0 / double(j + 1); residuals_out[j] = 0.25 * double(j); }
  for (int g = 0; g < 2; ++g) {
    summary->status[g] = g == 0 ? CALICO_FIT_OK : CALICO_FIT_MAX_ITERATIONS; summary->iterations[g] = 7 + g; summary->n_used[g] = n - g;
    summary->n_downweighted[g] = 3 + g; summary->n_rejected[g] = g; summary->scale[g] = 0.1 * (g + 1);
  }
  return rec.code;
}

std::vector<double> plain_knots, plain_basis, plain_data;
int32_t plain_recorder(int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n, const double*, const double* data6,
                       double* ctrl_out) {
  plain_knots.assign(knots, knots + n_knots);
  plain_basis.assign(basis, basis + size_t(n_knots - 2 * order + 1) * order * order);
  plain_data.assign(data6, data6 + n * 6);
  for (int i = 0; i < (n_knots - order) * 6; ++i) ctrl_out[i] = 0.0;
  return CALICO_OK;
}

int host() {
  BSpline6::robust_fit_solver() = &recorder;
  BSpline6::fit_solver() = &plain_recorder;
  // a rig that turns about z through more than a full turn (the axis-angle vector must be unwrapped past pi) while it moves
  std::map<double, Pose3d> poses;
  std::vector<std::array<double, 2>> weights;
  const int n = 41;
  for (int i = 0; i < n; ++i) {
    const double t = 3.0 + 0.05 * i, angle = 0.2 * i;
    poses[t] = Pose3d(Quaterniond(std::cos(angle / 2), 0.0, 0.0, std::sin(angle / 2)), Vector3d(0.1 * i, -0.2 * i, 1.0));
    weights.push_back({1.0 + i, 0.5 * i});
  }
  calico_spline_fit_options o;
  calico_default_spline_fit_options(&o);
  calico_spline_robust_options r;
  calico_default_spline_robust_options(&r);
  CHECK(r.loss == CALICO_ROBUST_HUBER && r.max_iterations == 20 && r.step_tolerance == 1e-9);
  CHECK(r.tuning_rot == 0.0 && r.tuning_pos == 0.0 && r.scale_rot == 0.0 && r.scale_pos == 0.0 && r.min_scale_rot == 0.0 && r.min_scale_pos == 0.0);
  o.derivative = 3; o.lambda_rot[0] = 1e-4; o.lambda_pos[0] = 1e-2;
  r.loss = CALICO_ROBUST_TUKEY; r.max_iterations = 11; r.tuning_pos = 3.5; r.scale_rot = 0.02; r.min_scale_pos = 1e-4; r.step_tolerance = 1e-7;

  Trajectory trajectory;
  auto fit = trajectory.FitSplineRobust(poses, 5.0, 4, o, r, weights);
  CHECK(fit.ok() && rec.calls == 1 && rec.order == 4);
  // the knots and basis are FitSpline's
  Trajectory plain;
  CHECK(plain.FitSpline(poses, 5.0, 4).ok());
  CHECK(rec.knots == plain_knots && rec.basis == plain_basis && rec.data == plain_data);
  CHECK(rec.knots.size() == size_t(1 + 10 + 2 * 3) && rec.knots[3] == 3.0);
  // the data: unwrapped axis-angle (0, 0, angle) past pi and 2 pi, the positions; the stamps sorted
  CHECK(rec.stamps.size() == size_t(n) && rec.data.size() == size_t(n) * 6);
  for (int i = 0; i < n; ++i) {
    const double* d = &rec.data[size_t(i) * 6];
    CHECK(rec.stamps[size_t(i)] == 3.0 + 0.05 * i);
    CHECK(d[0] == 0.0 && d[1] == 0.0 && std::fabs(d[2] - 0.2 * i) < 1e-12);
    CHECK(d[3] == 0.1 * i && d[4] == -0.2 * i && d[5] == 1.0);
  }
  CHECK(rec.data[size_t(n - 1) * 6 + 2] > 6.2831);
  // the weights and both option structs, unchanged
  CHECK(rec.has_weights && rec.weights.size() == size_t(n) * 2);
  for (int i = 0; i < n; ++i) CHECK(rec.weights[size_t(i) * 2] == 1.0 + i && rec.weights[size_t(i) * 2 + 1] == 0.5 * i);
  CHECK(std::memcmp(&rec.fit, &o, sizeof o) == 0 && std::memcmp(&rec.robust, &r, sizeof r) == 0);
  // what comes back: the control points, the summary, and the per-pose weights and residual norms in time order
  const auto& ctrl = trajectory.spline().control_points();
  CHECK(ctrl.size() == rec.knots.size() - 4);
  for (size_t i = 0; i < ctrl.size(); ++i) for (size_t c = 0; c < 6; ++c) CHECK(ctrl[i][c] == 0.5 * double(i * 6 + c));
  CHECK(fit->summary.status[0] == CALICO_FIT_OK && fit->summary.status[1] == CALICO_FIT_MAX_ITERATIONS && fit->summary.iterations[1] == 8);
  CHECK(fit->summary.n_used[1] == n - 1 && fit->summary.n_downweighted[0] == 3 && fit->summary.n_rejected[1] == 1 && fit->summary.scale[1] == 0.2);
  CHECK(fit->robust_weights.size() == size_t(n) && fit->residuals.size() == size_t(n));
  for (int i = 0; i < n; ++i) {
    CHECK(fit->robust_weights[size_t(i)][0] == 1.0 / double(2 * i + 1) && fit->robust_weights[size_t(i)][1] == 1.0 / double(2 * i + 2));
    CHECK(fit->residuals[size_t(i)][0] == 0.25 * double(2 * i) && fit->residuals[size_t(i)][1] == 0.25 * double(2 * i + 1));
  }
  // no weights: a null pointer
  CHECK(trajectory.FitSplineRobust(poses, 5.0, 4, o, r).ok() && rec.calls == 2 && !rec.has_weights);
  // the return codes
  rec.code = CALICO_INVALID_ARGUMENT;
  auto bad = trajectory.FitSplineRobust(poses, 5.0, 4, o, r, weights);
  CHECK(!bad.ok() && bad.status().code() == StatusCode::kInvalidArgument);
  rec.code = CALICO_UNIMPLEMENTED;
  bad = trajectory.FitSplineRobust(poses, 5.0, 6, o, r, weights);
  CHECK(bad.status().code() == StatusCode::kUnimplemented);
  CHECK(bad.status().message().find("too many for the on-device solve; order 6 fits at most 2218") != std::string::npos);
  rec.code = CALICO_INTERNAL;
  bad = trajectory.FitSplineRobust(poses, 5.0, 4, o, r, weights);
  CHECK(bad.status().code() == StatusCode::kInternal);
  // what the facade refuses itself, before the solve
  rec.code = CALICO_OK;
  const int calls = rec.calls;
  weights.pop_back();
  CHECK(trajectory.FitSplineRobust(poses, 5.0, 4, o, r, weights).status().code() == StatusCode::kInvalidArgument);
  CHECK(trajectory.FitSplineRobust({}, 5.0, 4, o, r).status().code() == StatusCode::kInvalidArgument);
  CHECK(trajectory.FitSplineRobust(poses, 0.0, 4, o, r).status().code() == StatusCode::kInvalidArgument);
  CHECK(trajectory.FitSplineRobust(poses, 5.0, 1, o, r).status().code() == StatusCode::kInvalidArgument);
  CHECK(rec.calls == calls);
  std::printf("OK\n");
  return 0;
}

// uniform in [-1, 1): a linear congruential generator, so that the poses are the same everywhere
double noise() {
  static uint64_t state = 12345;
  state = state * 6364136223846793005ull + 1442695040888963407ull;
  return double(state >> 11) / double(1ull << 52) - 1.0;
}

// every tenth pose, away from the ends (where a pose has the leverage to be followed)
bool is_turned(int i, int n) { return i % 10 == 4 && i > 10 && i < n - 10; }

// The call on device 0: 200 poses of a smooth motion over 10 s with noise (0.02 rad and 0.01 m uniform per axis: without noise the
// scale estimate is the spline's approximation error and Huber an L1 fit), every tenth turned by 0.5 rad about x. Knots at 4 Hz: five poses per
// segment (a spline that can follow every pose has no outliers).
int device() {
  std::map<double, Pose3d> poses;
  const int n = 200;
  const Quaterniond turn(std::cos(0.25), std::sin(0.25), 0.0, 0.0);
  for (int i = 0; i < n; ++i) {
    const double t = 0.05 * i, angle = 0.3 * std::sin(0.8 * t) + 0.1 * t;
    const double v[3] = {0.02 * noise(), 0.02 * noise(), angle + 0.02 * noise()};
    const double norm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), s = norm > 0 ? std::sin(norm / 2) / norm : 0.5;
    const Quaterniond q(std::cos(norm / 2), s * v[0], s * v[1], s * v[2]);
    poses[t] = Pose3d(is_turned(i, n) ? q * turn : q,
                      Vector3d(std::sin(0.5 * t) + 0.01 * noise(), std::cos(0.7 * t) + 0.01 * noise(), 0.1 * t + 0.01 * noise()));
  }
  calico_spline_fit_options o;
  calico_default_spline_fit_options(&o);
  calico_spline_robust_options r;
  calico_default_spline_robust_options(&r);
  Trajectory robust;
  auto fit = robust.FitSplineRobust(poses, 4.0, 6, o, r);
  if (!fit.ok()) std::printf("%s\n", fit.status().message().c_str());
  CHECK(fit.ok() && fit->robust_weights.size() == size_t(n) && fit->summary.n_used[0] == n);
  // the robust weight falls with the residual norm: the turned poses are singled out when each has a smaller rotation weight
  // than every other pose (and a small one); their positions are as good as anyone's
  double turned_max = 0.0, others_min = 1.0, turned_pos_min = 1.0;
  for (int i = 0; i < n; ++i) {
    const double u = fit->robust_weights[size_t(i)][0];
    if (is_turned(i, n)) { turned_max = std::fmax(turned_max, u); turned_pos_min = std::fmin(turned_pos_min, fit->robust_weights[size_t(i)][1]); }
    else others_min = std::fmin(others_min, u);
    CHECK(!is_turned(i, n) || fit->residuals[size_t(i)][0] > 0.4);
  }
  std::printf("turned poses: rotation weight <= %.3e, every other pose >= %.3e; status %d %d after %d %d iterations\n", turned_max, others_min,
              fit->summary.status[0], fit->summary.status[1], fit->summary.iterations[0], fit->summary.iterations[1]);
  CHECK(turned_max < others_min && turned_max <= 0.1 && turned_pos_min > turned_max);
  CHECK(fit->summary.n_downweighted[0] >= 18);
  // max_iterations 0 is the smoothing fit
  r.max_iterations = 0;
  Trajectory zero, smooth;
  auto none = zero.FitSplineRobust(poses, 4.0, 6, o, r);
  CHECK(none.ok() && none->summary.iterations[0] == 0 && smooth.FitSplineSmooth(poses, 4.0, 6, o).ok());
  const auto &a = zero.spline().control_points(), &b = smooth.spline().control_points();
  CHECK(a.size() == b.size() && !a.empty());
  for (size_t i = 0; i < a.size(); ++i) CHECK(std::memcmp(a[i].data(), b[i].data(), 6 * sizeof(double)) == 0);
  for (int i = 0; i < n; ++i) CHECK(none->robust_weights[size_t(i)][0] == 1.0 && none->robust_weights[size_t(i)][1] == 1.0);
  // and differs from the robust result
  bool differs = false;
  const auto& c = robust.spline().control_points();
  for (size_t i = 0; i < a.size(); ++i) differs = differs || std::fabs(a[i][0] - c[i][0]) > 1e-3;
  CHECK(differs);
  std::printf("OK\n");
  return 0;
}
}  // namespace

int main(int argc, char** argv) { return argc > 1 && std::string(argv[1]) == "device" ? device() : host(); }
