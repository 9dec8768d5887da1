// fit_smooth_facade.cpp — Trajectory::FitSplineSmooth / BSpline6::FitToDataSmooth (include/calico/calico.hpp) from C++, host only: the
// solve is replaced through BSpline6::smooth_fit_solver() by a recorder, so that what the facade hands to calico_fit_spline_smooth
// (knots and basis as FitSpline builds them, the unwrapped axis-angle data, the weights, the options) and what it makes of every
// return code are checked on a machine without a GPU. Built with -DCALICO_TEST_HOOKS.
#include <cmath>
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
  bool has_weights = false, has_rows = false;
  calico_spline_fit_options options{};
  int32_t code = CALICO_OK;
} rec;

int32_t recorder(int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n, const double* stamps, const double* data6,
                 const double* weights, const calico_spline_fit_options* options, double* ctrl_out, double*, calico_spline_fit_row* rows_out,
                 calico_spline_fit_summary* summary) {
  rec.calls += 1; rec.order = order;
  rec.knots.assign(knots, knots + n_knots);
  rec.basis.assign(basis, basis + size_t(n_knots - 2 * order + 1) * order * order);
  rec.stamps.assign(stamps, stamps + n); rec.data.assign(data6, data6 + n * 6);
  rec.has_weights = weights != nullptr;
  if (weights) rec.weights.assign(weights, weights + n * 2); else rec.weights.clear();
  rec.options = *options;
  rec.has_rows = rows_out != nullptr;
  if (rec.code != CALICO_OK) return rec.code;
  for (int i = 0; i < (n_knots - order) * 6; ++i) ctrl_out[i] = 0.5 * i;
  for (int g = 0; g < 2; ++g) {
    summary->status[g] = g == 0 ? CALICO_FIT_OK : CALICO_FIT_TARGET_NOT_MET; summary->chosen[g] = g; summary->n_used[g] = n - g;
    for (int l = 0; l < options->n_lambda; ++l) rows_out[g * options->n_lambda + l] = {0, 0, 10.0 * g + l, 1.0, 2.0, 3.0};
  }
  return CALICO_OK;
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
}  // namespace

int main() {
  BSpline6::smooth_fit_solver() = &recorder;
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
  CHECK(o.derivative == 2 && o.relative == 1 && o.n_lambda == 1 && o.lambda_rot[0] == 1e-3 && o.lambda_pos[0] == 1e-3);
  CHECK(o.lambda_rot[1] == 0.0 && o.target_rms_rot == 0.0 && o.target_rms_pos == 0.0);
  o.derivative = 3; o.n_lambda = 3; o.target_rms_pos = 0.25;
  for (int l = 0; l < 3; ++l) { o.lambda_rot[l] = 1e-4 * (l + 1); o.lambda_pos[l] = 1e-2 * (l + 1); }

  Trajectory trajectory;
  auto fit = trajectory.FitSplineSmooth(poses, 5.0, 4, o, weights);
  CHECK(fit.ok() && rec.calls == 1 && rec.order == 4 && rec.has_rows);
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
  // the weights and the options, unchanged
  CHECK(rec.has_weights && rec.weights.size() == size_t(n) * 2);
  for (int i = 0; i < n; ++i) CHECK(rec.weights[size_t(i) * 2] == 1.0 + i && rec.weights[size_t(i) * 2 + 1] == 0.5 * i);
  CHECK(std::memcmp(&rec.options, &o, sizeof o) == 0);
  // what comes back: the control points, the summary and the rows
  const auto& ctrl = trajectory.spline().control_points();
  CHECK(ctrl.size() == rec.knots.size() - 4);
  for (size_t i = 0; i < ctrl.size(); ++i) for (size_t c = 0; c < 6; ++c) CHECK(ctrl[i][c] == 0.5 * double(i * 6 + c));
  CHECK(fit->summary.status[0] == CALICO_FIT_OK && fit->summary.status[1] == CALICO_FIT_TARGET_NOT_MET && fit->summary.chosen[1] == 1);
  CHECK(fit->summary.n_used[0] == n && fit->summary.n_used[1] == n - 1 && fit->rows.size() == 6);
  CHECK(fit->rows[2].lambda == 2.0 && fit->rows[3].lambda == 10.0 && fit->rows[5].rms == 3.0);
  // no weights: a null pointer
  CHECK(trajectory.FitSplineSmooth(poses, 5.0, 4, o).ok() && rec.calls == 2 && !rec.has_weights);
  // the return codes
  rec.code = CALICO_INVALID_ARGUMENT;
  auto bad = trajectory.FitSplineSmooth(poses, 5.0, 4, o, weights);
  CHECK(!bad.ok() && bad.status().code() == StatusCode::kInvalidArgument);
  rec.code = CALICO_UNIMPLEMENTED;
  bad = trajectory.FitSplineSmooth(poses, 5.0, 6, o, weights);
  CHECK(bad.status().code() == StatusCode::kUnimplemented);
  CHECK(bad.status().message().find("too many for the on-device solve; order 6 fits at most 2218") != std::string::npos);
  rec.code = CALICO_INTERNAL;
  bad = trajectory.FitSplineSmooth(poses, 5.0, 4, o, weights);
  CHECK(bad.status().code() == StatusCode::kInternal);
  // what the facade refuses itself, before the solve
  rec.code = CALICO_OK;
  const int calls = rec.calls;
  weights.pop_back();
  CHECK(trajectory.FitSplineSmooth(poses, 5.0, 4, o, weights).status().code() == StatusCode::kInvalidArgument);
  CHECK(trajectory.FitSplineSmooth({}, 5.0, 4, o).status().code() == StatusCode::kInvalidArgument);
  CHECK(trajectory.FitSplineSmooth(poses, 0.0, 4, o).status().code() == StatusCode::kInvalidArgument);
  CHECK(trajectory.FitSplineSmooth(poses, 5.0, 1, o).status().code() == StatusCode::kInvalidArgument);
  CHECK(rec.calls == calls);
  std::printf("OK\n");
  return 0;
}
