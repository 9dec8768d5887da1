// fit_cv_facade.cpp — Trajectory::FitSplineCV / BSpline6::FitToDataCV (include/calico/calico.hpp) from C++.
// Without arguments, host only: the solve is replaced through BSpline6::cv_fit_solver() by a recorder, so that what the facade
// hands to calico_fit_spline_cv (knots and basis as FitSpline builds them, the unwrapped axis-angle data, the weights, both option
// structs) and what it makes of every return code are checked on a machine without a GPU.
// With the argument "device": the recorder forwards to calico_fit_spline_cv on device 0 and keeps what it returned -- the facade's
// control points, rows, cv rows, leverages and leave-one-out residuals are those bits, and noisy poses of a smooth motion get an
// interior lambda of a 13-point grid under both criteria. Built with -DCALICO_TEST_HOOKS.
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
  bool has_weights = false, ctrl_all_null = false;
  calico_spline_fit_options fit{};
  calico_spline_cv_options cv{};
  int32_t code = CALICO_OK;
  // the forwarding recorder's copy of what the library returned
  std::vector<double> ctrl, leverage, loo;
  std::vector<calico_spline_fit_row> rows;
  std::vector<calico_spline_cv_row> cv_rows;
  calico_spline_cv_summary summary{};
} rec;

void record_inputs(int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n, const double* stamps, const double* data6,
                   const double* weights, const calico_spline_fit_options* fit, const calico_spline_cv_options* cv, const double* ctrl_all_out) {
  rec.calls += 1; rec.order = order;
  rec.knots.assign(knots, knots + n_knots);
  rec.basis.assign(basis, basis + size_t(n_knots - 2 * order + 1) * order * order);
  rec.stamps.assign(stamps, stamps + n); rec.data.assign(data6, data6 + n * 6);
  rec.has_weights = weights != nullptr;
  if (weights) rec.weights.assign(weights, weights + n * 2); else rec.weights.clear();
  rec.fit = *fit; rec.cv = *cv; rec.ctrl_all_null = ctrl_all_out == nullptr;
}

int32_t recorder(int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n, const double* stamps, const double* data6,
                 const double* weights, const calico_spline_fit_options* fit, const calico_spline_cv_options* cv, double* ctrl_out,
                 double* ctrl_all_out, calico_spline_fit_row* rows_out, calico_spline_cv_row* cv_rows_out, double* leverage_out,
                 double* loo_residuals_out, calico_spline_cv_summary* summary) {
  record_inputs(order, n_knots, knots, basis, n, stamps, data6, weights, fit, cv, ctrl_all_out);
  if (rec.code != CALICO_OK && rec.code != CALICO_INTERNAL) return rec.code;
  for (int i = 0; i < (n_knots - order) * 6; ++i) ctrl_out[i] = 0.5 * i;
  for (int64_t j = 0; j < n * 2; ++j) { leverage_out[j] = 1.0 / double(j + 2); loo_residuals_out[j] = 0.25 * double(j); }
  for (int i = 0; i < 2 * fit->n_lambda; ++i) {
    rows_out[i] = calico_spline_fit_row{0, 0, 1.0 + i, 2.0 + i, 3.0 + i, 4.0 + i};
    cv_rows_out[i] = calico_spline_cv_row{10.0 + i, 20.0 + i, 30.0 + i, 0.01 * i};
  }
  for (int g = 0; g < 2; ++g) {
    summary->status[g] = g == 0 ? CALICO_FIT_OK : CALICO_FIT_CV_AT_GRID_END; summary->chosen[g] = 1 + g; summary->n_used[g] = n - g;
    summary->edf[g] = 11.5 + g; summary->score[g] = 0.125 * (g + 1);
  }
  return rec.code;
}

int32_t forwarder(int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n, const double* stamps, const double* data6,
                  const double* weights, const calico_spline_fit_options* fit, const calico_spline_cv_options* cv, double* ctrl_out,
                  double* ctrl_all_out, calico_spline_fit_row* rows_out, calico_spline_cv_row* cv_rows_out, double* leverage_out,
                  double* loo_residuals_out, calico_spline_cv_summary* summary) {
  record_inputs(order, n_knots, knots, basis, n, stamps, data6, weights, fit, cv, ctrl_all_out);
  const int32_t rc = calico_fit_spline_cv(0, order, n_knots, knots, basis, n, stamps, data6, weights, fit, cv, ctrl_out, ctrl_all_out, rows_out,
                                          cv_rows_out, leverage_out, loo_residuals_out, summary);
  rec.ctrl.assign(ctrl_out, ctrl_out + size_t(n_knots - order) * 6);
  rec.leverage.assign(leverage_out, leverage_out + n * 2); rec.loo.assign(loo_residuals_out, loo_residuals_out + n * 2);
  rec.rows.assign(rows_out, rows_out + 2 * fit->n_lambda); rec.cv_rows.assign(cv_rows_out, cv_rows_out + 2 * fit->n_lambda);
  rec.summary = *summary;
  return rc;
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
  BSpline6::cv_fit_solver() = &recorder;
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
  calico_spline_cv_options c;
  c.criterion = 77; c.reserved = 77;
  calico_default_spline_cv_options(&c);
  CHECK(c.criterion == CALICO_FIT_CV_GCV && c.reserved == 0);
  o.derivative = 3; o.n_lambda = 3;
  for (int l = 0; l < 3; ++l) { o.lambda_rot[l] = 1e-4 * (l + 1); o.lambda_pos[l] = 1e-2 * (l + 1); }
  c.criterion = CALICO_FIT_CV_PRESS;

  Trajectory trajectory;
  auto fit = trajectory.FitSplineCV(poses, 5.0, 4, o, c, weights);
  CHECK(fit.ok() && rec.calls == 1 && rec.order == 4 && rec.ctrl_all_null);
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
  CHECK(std::memcmp(&rec.fit, &o, sizeof o) == 0 && std::memcmp(&rec.cv, &c, sizeof c) == 0);
  // what comes back: the control points, the summary, both kinds of rows, and the per-pose leverages and residuals in time order
  const auto& ctrl = trajectory.spline().control_points();
  CHECK(ctrl.size() == rec.knots.size() - 4);
  for (size_t i = 0; i < ctrl.size(); ++i) for (size_t ch = 0; ch < 6; ++ch) CHECK(ctrl[i][ch] == 0.5 * double(i * 6 + ch));
  CHECK(fit->summary.status[0] == CALICO_FIT_OK && fit->summary.status[1] == CALICO_FIT_CV_AT_GRID_END);
  CHECK(fit->summary.chosen[0] == 1 && fit->summary.chosen[1] == 2 && fit->summary.n_used[1] == n - 1);
  CHECK(fit->summary.edf[1] == 12.5 && fit->summary.score[0] == 0.125 && fit->summary.score[1] == 0.25);
  CHECK(fit->rows.size() == 6 && fit->cv_rows.size() == 6);
  for (int i = 0; i < 6; ++i) {
    CHECK(fit->rows[size_t(i)].lambda == 1.0 + i && fit->rows[size_t(i)].rms == 4.0 + i);
    CHECK(fit->cv_rows[size_t(i)].edf == 10.0 + i && fit->cv_rows[size_t(i)].gcv == 20.0 + i && fit->cv_rows[size_t(i)].press == 30.0 + i &&
          fit->cv_rows[size_t(i)].max_leverage == 0.01 * i);
  }
  CHECK(fit->leverage.size() == size_t(n) && fit->loo_residuals.size() == size_t(n));
  for (int i = 0; i < n; ++i) {
    CHECK(fit->leverage[size_t(i)][0] == 1.0 / double(2 * i + 2) && fit->leverage[size_t(i)][1] == 1.0 / double(2 * i + 3));
    CHECK(fit->loo_residuals[size_t(i)][0] == 0.25 * double(2 * i) && fit->loo_residuals[size_t(i)][1] == 0.25 * double(2 * i + 1));
  }
  // no weights: a null pointer
  CHECK(trajectory.FitSplineCV(poses, 5.0, 4, o, c).ok() && rec.calls == 2 && !rec.has_weights);
  // the return codes
  rec.code = CALICO_INVALID_ARGUMENT;
  auto bad = trajectory.FitSplineCV(poses, 5.0, 4, o, c, weights);
  CHECK(!bad.ok() && bad.status().code() == StatusCode::kInvalidArgument);
  rec.code = CALICO_UNIMPLEMENTED;
  bad = trajectory.FitSplineCV(poses, 5.0, 6, o, c, weights);
  CHECK(bad.status().code() == StatusCode::kUnimplemented);
  CHECK(bad.status().message().find("too many for the on-device solve; order 6 fits at most 2218") != std::string::npos);
  rec.code = CALICO_INTERNAL;
  bad = trajectory.FitSplineCV(poses, 5.0, 4, o, c, weights);
  CHECK(bad.status().code() == StatusCode::kInternal);
  // what the facade refuses itself, before the solve
  rec.code = CALICO_OK;
  const int calls = rec.calls;
  weights.pop_back();
  CHECK(trajectory.FitSplineCV(poses, 5.0, 4, o, c, weights).status().code() == StatusCode::kInvalidArgument);
  CHECK(trajectory.FitSplineCV({}, 5.0, 4, o, c).status().code() == StatusCode::kInvalidArgument);
  CHECK(trajectory.FitSplineCV(poses, 0.0, 4, o, c).status().code() == StatusCode::kInvalidArgument);
  CHECK(trajectory.FitSplineCV(poses, 5.0, 1, o, c).status().code() == StatusCode::kInvalidArgument);
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

// The call on device 0: 200 poses of a smooth motion over 10 s with noise (0.02 rad and 0.01 m uniform per axis), knots at 10 Hz (two
// poses per segment: without a penalty the spline follows the noise), lambda from 1e-6 to 1e6 relative in 13 steps.
int device() {
  BSpline6::cv_fit_solver() = &forwarder;
  std::map<double, Pose3d> poses;
  const int n = 200;
  for (int i = 0; i < n; ++i) {
    const double t = 0.05 * i, angle = 0.3 * std::sin(0.8 * t) + 0.1 * t;
    const double v[3] = {0.02 * noise(), 0.02 * noise(), angle + 0.02 * noise()};
    const double norm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]), s = norm > 0 ? std::sin(norm / 2) / norm : 0.5;
    poses[t] = Pose3d(Quaterniond(std::cos(norm / 2), s * v[0], s * v[1], s * v[2]),
                      Vector3d(std::sin(0.5 * t) + 0.01 * noise(), std::cos(0.7 * t) + 0.01 * noise(), 0.1 * t + 0.01 * noise()));
  }
  calico_spline_fit_options o;
  calico_default_spline_fit_options(&o);
  o.n_lambda = 13;
  for (int l = 0; l < 13; ++l) o.lambda_rot[l] = o.lambda_pos[l] = std::pow(10.0, l - 6);
  for (int criterion : {CALICO_FIT_CV_GCV, CALICO_FIT_CV_PRESS}) {
    calico_spline_cv_options c;
    calico_default_spline_cv_options(&c);
    c.criterion = criterion;
    Trajectory trajectory;
    auto fit = trajectory.FitSplineCV(poses, 10.0, 6, o, c);
    if (!fit.ok()) std::printf("%s\n", fit.status().message().c_str());
    CHECK(fit.ok() && fit->summary.n_used[0] == n && fit->rows.size() == 26 && fit->cv_rows.size() == 26);
    // the library's bits
    const auto& ctrl = trajectory.spline().control_points();
    CHECK(ctrl.size() * 6 == rec.ctrl.size());
    for (size_t i = 0; i < ctrl.size(); ++i) CHECK(std::memcmp(ctrl[i].data(), &rec.ctrl[i * 6], 6 * sizeof(double)) == 0);
    CHECK(std::memcmp(&fit->summary, &rec.summary, sizeof rec.summary) == 0);
    CHECK(std::memcmp(fit->rows.data(), rec.rows.data(), 26 * sizeof(calico_spline_fit_row)) == 0);
    CHECK(std::memcmp(fit->cv_rows.data(), rec.cv_rows.data(), 26 * sizeof(calico_spline_cv_row)) == 0);
    CHECK(fit->leverage.size() == size_t(n) && fit->loo_residuals.size() == size_t(n));
    CHECK(std::memcmp(fit->leverage.data(), rec.leverage.data(), size_t(n) * 2 * sizeof(double)) == 0);
    CHECK(std::memcmp(fit->loo_residuals.data(), rec.loo.data(), size_t(n) * 2 * sizeof(double)) == 0);
    // an interior choice, whose score is the smallest of its column and whose leverages add up to its edf
    for (int g = 0; g < 2; ++g) {
      const int chosen = fit->summary.chosen[g];
      std::printf("criterion %d group %d: chosen %d (lambda %.3e), edf %.3f, score %.6e\n", criterion, g, chosen,
                  fit->rows[size_t(g * 13 + chosen)].lambda, fit->summary.edf[g], fit->summary.score[g]);
      CHECK(fit->summary.status[g] == CALICO_FIT_OK && chosen > 0 && chosen < 12);
      double sum = 0.0;
      for (int i = 0; i < n; ++i) {
        sum += fit->leverage[size_t(i)][size_t(g)];
        CHECK(fit->leverage[size_t(i)][size_t(g)] > 0.0 && fit->leverage[size_t(i)][size_t(g)] < 1.0 && fit->loo_residuals[size_t(i)][size_t(g)] >= 0.0);
      }
      CHECK(std::fabs(sum - fit->summary.edf[g]) <= 1e-9 * fit->summary.edf[g]);
      for (int l = 0; l < 13; ++l) {
        const calico_spline_cv_row& r = fit->cv_rows[size_t(g * 13 + l)];
        CHECK((criterion == CALICO_FIT_CV_GCV ? r.gcv : r.press) >= fit->summary.score[g]);
      }
      CHECK(fit->cv_rows[size_t(g * 13 + chosen)].edf == fit->summary.edf[g]);
    }
  }
  std::printf("OK\n");
  return 0;
}
}  // namespace

int main(int argc, char** argv) { return argc > 1 && std::string(argv[1]) == "device" ? device() : host(); }
