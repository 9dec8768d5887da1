// fit.cpp — calico_fit_spline (this part of the C ABI of include/calico_hip.h): the control points of a spline from sorted samples
// (kernels: fit_kernels.hip). Everything that can be checked without a device is checked before the first HIP call. The host
// finds the segment of every sample (the samples are sorted: a CSR over the segments), uploads, launches and reads back.
// calico_fit_spline_smooth is the same call with sample weights, a roughness penalty and a grid of lambda per channel group: the
// device solves every (group, lambda), the host applies the selection rule to the rows it downloads. calico_fit_spline_robust is
// the smoothing fit with one lambda followed by reweighted solves (kernels: fit_robust_kernels.hip): the host enqueues every
// iteration, the device decides which of them still run, and the host reads back once. calico_fit_spline_cv is the smoothing fit's
// grid with the choice made on the device by cross-validation (kernels: fit_cv_kernels.hip), and one readback.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/calico_hip.h"
#include "arg_rules.hpp"
#include "device_math.hpp"
#include "free_call.hpp"
#include "kernels.hpp"

// The segment of every sample and the CSR of the (sorted) samples over the segments, shared by both fits; or the rule's message.
static std::string bin_samples(int k, int n_valid, const double* knots, int64_t n, const double* stamps, std::vector<int>* seg,
                               std::vector<int>* seg_ptr) {
  const int n_seg = n_valid - 1;
  seg->assign(static_cast<size_t>(n), 0);
  seg_ptr->assign(static_cast<size_t>(n_seg) + 1, 0);
  for (int64_t j = 0; j < n; ++j) {
    const int s = cal::spline_segment(knots + (k - 1), n_valid, stamps[j]);
    if (s < 0) return "sample stamp " + std::to_string(j) + " lies off the valid knots";
    (*seg)[size_t(j)] = s;
    (*seg_ptr)[size_t(s) + 1] += 1;
  }
  for (int s = 0; s < n_seg; ++s) (*seg_ptr)[size_t(s) + 1] += (*seg_ptr)[size_t(s)];
  return "";
}

extern "C" int32_t calico_fit_spline(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis,
                                     int64_t n, const double* stamps, const double* data6, double* ctrl_out) {
  using namespace cal;
  const FreeCall call{"calico_fit_spline"};
  std::string error = spline_shape_error(order, n_knots, kMaxOrder);
  if (error.empty() && (!knots || !basis || !stamps || !data6 || !ctrl_out)) error = "null knots, basis, stamps, data or ctrl_out";
  if (error.empty() && n <= 0) error = "n must be > 0";
  if (!error.empty()) return call.invalid(error);
  if (n > INT32_MAX) return call.fail(CALICO_UNIMPLEMENTED, "more than 2^31 - 1 samples");      // the kernels and seg_ptr index the samples with int
  if (!(error = stamps_error("sample", n, stamps)).empty()) return call.invalid(error);      // samples must be sorted (trajectory.cpp:24)
  const int k = order, n_ctrl = n_knots - k, n_valid = spline_valid_knots(k, n_knots), n_seg = n_valid - 1;
  std::vector<int> seg, seg_ptr;
  if (!(error = bin_samples(k, n_valid, knots, n, stamps, &seg, &seg_ptr)).empty()) return call.invalid(error);
  if (fit_solve_lds_bytes(n_ctrl, k) > 156 * 1024) return call.fail(CALICO_UNIMPLEMENTED, "the trajectory is too long for the banded solve in LDS");
  if (int rc = call.select_device(device)) return rc;
  FreeBuf<double> d_stamps, d_data, d_knots, d_basis, d_W, d_band, d_rhs, d_ctrl;
  FreeBuf<int> d_seg, d_ptr, d_status;
  FREE_TRY(call, d_stamps.upload(stamps, size_t(n))); FREE_TRY(call, d_data.upload(data6, size_t(n) * 6));
  FREE_TRY(call, d_knots.upload(knots, size_t(n_knots))); FREE_TRY(call, d_basis.upload(basis, size_t(n_seg) * k * k));
  FREE_TRY(call, d_seg.upload(seg.data(), seg.size())); FREE_TRY(call, d_ptr.upload(seg_ptr.data(), seg_ptr.size()));
  FREE_TRY(call, d_W.alloc(size_t(n) * k)); FREE_TRY(call, d_band.alloc(size_t(n_ctrl) * k)); FREE_TRY(call, d_rhs.alloc(size_t(n_ctrl) * 6));
  FREE_TRY(call, d_ctrl.alloc(size_t(n_ctrl) * 6)); FREE_TRY(call, d_status.alloc(1));
  FitArgs a = {};
  a.n = int(n); a.k = k; a.n_ctrl = n_ctrl; a.n_seg = n_seg;
  a.stamps = d_stamps.p; a.seg = d_seg.p; a.seg_ptr = d_ptr.p; a.knots = d_knots.p; a.basis = d_basis.p; a.data = d_data.p;
  a.W = d_W.p; a.band = d_band.p; a.rhs = d_rhs.p; a.ctrl = d_ctrl.p; a.status = d_status.p;
  FREE_TRY(call, launch_fit_spline(device, a, nullptr));
  int status = 0;
  FREE_TRY(call, d_status.download(&status, 1)); FREE_TRY(call, d_ctrl.download(ctrl_out, size_t(n_ctrl) * 6));
  return status == 0 ? CALICO_OK : call.fail(CALICO_INTERNAL, "a pivot of the normal equations was not finite");
}

extern "C" void calico_default_spline_fit_options(calico_spline_fit_options* o) {
  if (!o) return;
  *o = calico_spline_fit_options{};
  o->derivative = 2; o->relative = 1; o->n_lambda = 1;
  o->lambda_rot[0] = 1e-3; o->lambda_pos[0] = 1e-3;
}

static_assert(sizeof(cal::FitSmoothRow) == sizeof(calico_spline_fit_row) && cal::kFitMaxLambdas == CALICO_FIT_MAX_LAMBDAS,
              "the kernels write calico_spline_fit_row");

// The selection rule of one group over its rows: (status, chosen). target 0: the first usable lambda; otherwise the largest
// usable lambda whose rms <= target, or TARGET_NOT_MET and the smallest usable one. No usable lambda: NOT_POSITIVE_DEFINITE, -1.
static void choose_lambda(const cal::FitSmoothRow* rows, int n_lambda, double target, int32_t* status, int32_t* chosen) {
  int first = -1, met = -1;
  for (int l = 0; l < n_lambda; ++l) {
    if (rows[l].status != CALICO_FIT_OK) continue;
    if (first < 0) first = l;
    if (target > 0.0 && rows[l].rms <= target) met = l;
  }
  *chosen = target > 0.0 && met >= 0 ? met : first;
  *status = first < 0 ? CALICO_FIT_NOT_POSITIVE_DEFINITE : target > 0.0 && met < 0 ? CALICO_FIT_TARGET_NOT_MET : CALICO_FIT_OK;
}

extern "C" int32_t calico_fit_spline_smooth(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n,
                                            const double* stamps, const double* data6, const double* weights,
                                            const calico_spline_fit_options* options, double* ctrl_out, double* ctrl_all_out,
                                            calico_spline_fit_row* rows_out, calico_spline_fit_summary* summary) {
  using namespace cal;
  const FreeCall call{"calico_fit_spline_smooth"};
  calico_spline_fit_options o;
  if (options) o = *options; else calico_default_spline_fit_options(&o);
  std::string error = spline_shape_error(order, n_knots, kMaxOrder);
  if (error.empty() && (!knots || !basis || !stamps || !data6 || !ctrl_out || !summary)) error = "null knots, basis, stamps, data, ctrl_out or summary";
  if (error.empty() && n <= 0) error = "n must be > 0";
  if (error.empty()) error = spline_fit_options_error(order, o);
  if (!error.empty()) return call.invalid(error);
  if (n > INT32_MAX) return call.fail(CALICO_UNIMPLEMENTED, "more than 2^31 - 1 samples");      // the kernels and seg_ptr index the samples with int
  if (!(error = stamps_error("sample", n, stamps)).empty()) return call.invalid(error);
  int64_t n_used[2];
  if (!(error = sample_weights_error(n, weights, n_used)).empty()) return call.invalid(error);
  const int k = order, n_ctrl = n_knots - k, n_valid = spline_valid_knots(k, n_knots), n_seg = n_valid - 1, nl = o.n_lambda;
  std::vector<int> seg, seg_ptr;
  if (!(error = bin_samples(k, n_valid, knots, n, stamps, &seg, &seg_ptr)).empty()) return call.invalid(error);
  if (fit_solve_smooth_lds_bytes(n_ctrl, k) > 156 * 1024) return call.fail(CALICO_UNIMPLEMENTED, "the trajectory is too long for the banded solve in LDS");
  if (int rc = call.select_device(device)) return rc;
  FreeBuf<double> d_stamps, d_data, d_weights, d_knots, d_basis, d_W, d_P, d_band, d_rhs, d_ctrl;
  FreeBuf<int> d_seg, d_ptr;
  FreeBuf<FitSmoothRow> d_rows;
  FREE_TRY(call, d_stamps.upload(stamps, size_t(n))); FREE_TRY(call, d_data.upload(data6, size_t(n) * 6));
  if (weights) FREE_TRY(call, d_weights.upload(weights, size_t(n) * 2));
  FREE_TRY(call, d_knots.upload(knots, size_t(n_knots))); FREE_TRY(call, d_basis.upload(basis, size_t(n_seg) * k * k));
  FREE_TRY(call, d_seg.upload(seg.data(), seg.size())); FREE_TRY(call, d_ptr.upload(seg_ptr.data(), seg_ptr.size()));
  FREE_TRY(call, d_W.alloc(size_t(n) * k)); FREE_TRY(call, d_P.alloc(size_t(n_ctrl) * k));
  FREE_TRY(call, d_band.alloc(size_t(2) * n_ctrl * k)); FREE_TRY(call, d_rhs.alloc(size_t(2) * n_ctrl * 3));
  FREE_TRY(call, d_ctrl.alloc(size_t(nl) * n_ctrl * 6)); FREE_TRY(call, d_rows.alloc(size_t(2) * nl));
  FitSmoothArgs a = {};
  a.n = int(n); a.k = k; a.n_ctrl = n_ctrl; a.n_seg = n_seg; a.derivative = o.derivative; a.relative = o.relative != 0; a.n_lambda = nl;
  a.n_used_rot = int(n_used[0]); a.n_used_pos = int(n_used[1]);
  for (int l = 0; l < nl; ++l) { a.lambda_rot[l] = o.lambda_rot[l]; a.lambda_pos[l] = o.lambda_pos[l]; }
  a.stamps = d_stamps.p; a.seg = d_seg.p; a.seg_ptr = d_ptr.p; a.knots = d_knots.p; a.basis = d_basis.p; a.data = d_data.p; a.weights = d_weights.p;
  a.W = d_W.p; a.P = d_P.p; a.band = d_band.p; a.rhs = d_rhs.p; a.ctrl_all = d_ctrl.p; a.rows = d_rows.p;
  FREE_TRY(call, launch_fit_spline_smooth(device, a, nullptr));
  std::vector<FitSmoothRow> rows(size_t(2) * nl);
  std::vector<double> ctrl(size_t(nl) * n_ctrl * 6);
  FREE_TRY(call, d_rows.download(rows.data(), rows.size())); FREE_TRY(call, d_ctrl.download(ctrl.data(), ctrl.size()));
  // the host's part: the selection rule per group, and the columns of the lambdas that have control points
  for (int g = 0; g < 2; ++g) {
    choose_lambda(rows.data() + size_t(g) * nl, nl, g == 0 ? o.target_rms_rot : o.target_rms_pos, &summary->status[g], &summary->chosen[g]);
    summary->n_used[g] = n_used[g];
    for (int l = 0; l < nl; ++l) {
      if (rows[size_t(g) * nl + l].status != CALICO_FIT_OK) continue;
      const double* src = ctrl.data() + size_t(l) * n_ctrl * 6 + 3 * g;
      double* const targets[2] = {ctrl_all_out ? ctrl_all_out + size_t(l) * n_ctrl * 6 + 3 * g : nullptr,
                                  l == summary->chosen[g] ? ctrl_out + 3 * g : nullptr};
      for (double* out : targets)
        if (out) for (int i = 0; i < n_ctrl; ++i) for (int c = 0; c < 3; ++c) out[size_t(i) * 6 + c] = src[size_t(i) * 6 + c];
    }
  }
  if (rows_out) for (size_t i = 0; i < rows.size(); ++i) rows_out[i] = {rows[i].status, rows[i].replaced_pivots, rows[i].lambda, rows[i].rss, rows[i].penalty, rows[i].rms};
  for (int g = 0; g < 2; ++g)
    if (summary->status[g] == CALICO_FIT_NOT_POSITIVE_DEFINITE)
      return call.fail(CALICO_INTERNAL, std::string("no lambda of the ") + (g == 0 ? "rotation" : "position") + " grid has a finite factorisation");
  return CALICO_OK;
}

extern "C" void calico_default_spline_robust_options(calico_spline_robust_options* o) {
  if (!o) return;
  *o = calico_spline_robust_options{};
  o->loss = CALICO_ROBUST_HUBER; o->max_iterations = 20; o->step_tolerance = 1e-9;
}

// calico_fit_spline_robust: the smoothing fit's checks, uploads and launch arguments with n_lambda 1; the loop itself is the
// device's (fit_robust_kernels.hip): iteration 0 plus max_iterations reweighted ones are enqueued, then one readback.
extern "C" int32_t calico_fit_spline_robust(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n,
                                            const double* stamps, const double* data6, const double* weights,
                                            const calico_spline_fit_options* fit, const calico_spline_robust_options* robust, double* ctrl_out,
                                            double* robust_weights_out, double* residuals_out, calico_spline_robust_summary* summary) {
  using namespace cal;
  const FreeCall call{"calico_fit_spline_robust"};
  calico_spline_fit_options o;
  calico_spline_robust_options ro;
  if (fit) o = *fit; else calico_default_spline_fit_options(&o);
  if (robust) ro = *robust; else calico_default_spline_robust_options(&ro);
  std::string error = spline_shape_error(order, n_knots, kMaxOrder);
  if (error.empty() && (!knots || !basis || !stamps || !data6 || !ctrl_out || !summary)) error = "null knots, basis, stamps, data, ctrl_out or summary";
  if (error.empty() && n <= 0) error = "n must be > 0";
  if (error.empty()) error = spline_fit_options_error(order, o);
  if (error.empty()) error = spline_robust_options_error(o, ro);
  if (!error.empty()) return call.invalid(error);
  if (n > INT32_MAX) return call.fail(CALICO_UNIMPLEMENTED, "more than 2^31 - 1 samples");      // the kernels and seg_ptr index the samples with int
  if (!(error = stamps_error("sample", n, stamps)).empty()) return call.invalid(error);
  int64_t n_used[2];
  if (!(error = sample_weights_error(n, weights, n_used)).empty()) return call.invalid(error);
  const int k = order, n_ctrl = n_knots - k, n_valid = spline_valid_knots(k, n_knots), n_seg = n_valid - 1;
  std::vector<int> seg, seg_ptr;
  if (!(error = bin_samples(k, n_valid, knots, n, stamps, &seg, &seg_ptr)).empty()) return call.invalid(error);
  if (fit_solve_smooth_lds_bytes(n_ctrl, k) > 156 * 1024) return call.fail(CALICO_UNIMPLEMENTED, "the trajectory is too long for the banded solve in LDS");
  if (int rc = call.select_device(device)) return rc;
  FreeBuf<double> d_stamps, d_data, d_weights, d_knots, d_basis, d_W, d_P, d_band, d_rhs, d_ctrl, d_e, d_u, d_wu;
  FreeBuf<int> d_seg, d_ptr, d_hist;
  FreeBuf<FitSmoothRow> d_rows;
  FreeBuf<FitRobustState> d_state;
  std::vector<double> u(size_t(n) * 2, 1.0);      // the robust weights before any reweighting: 1, and 0 where the prior weight is 0
  if (weights) for (size_t i = 0; i < u.size(); ++i) u[i] = weights[i] > 0.0 ? 1.0 : 0.0;
  FREE_TRY(call, d_stamps.upload(stamps, size_t(n))); FREE_TRY(call, d_data.upload(data6, size_t(n) * 6));
  if (weights) FREE_TRY(call, d_weights.upload(weights, size_t(n) * 2));
  FREE_TRY(call, d_knots.upload(knots, size_t(n_knots))); FREE_TRY(call, d_basis.upload(basis, size_t(n_seg) * k * k));
  FREE_TRY(call, d_seg.upload(seg.data(), seg.size())); FREE_TRY(call, d_ptr.upload(seg_ptr.data(), seg_ptr.size()));
  FREE_TRY(call, d_W.alloc(size_t(n) * k)); FREE_TRY(call, d_P.alloc(size_t(n_ctrl) * k));
  FREE_TRY(call, d_band.alloc(size_t(2) * n_ctrl * k)); FREE_TRY(call, d_rhs.alloc(size_t(2) * n_ctrl * 3));
  FREE_TRY(call, d_ctrl.alloc(size_t(n_ctrl) * 6)); FREE_TRY(call, d_ctrl.zero(size_t(n_ctrl) * 6)); FREE_TRY(call, d_rows.alloc(2));
  FREE_TRY(call, d_e.alloc(size_t(n) * 2)); FREE_TRY(call, d_u.upload(u.data(), u.size())); FREE_TRY(call, d_wu.alloc(size_t(n) * 2));
  FREE_TRY(call, d_hist.alloc(size_t(2) * 8 * 256)); FREE_TRY(call, d_state.alloc(2));
  FitSmoothArgs a = {};
  a.n = int(n); a.k = k; a.n_ctrl = n_ctrl; a.n_seg = n_seg; a.derivative = o.derivative; a.relative = o.relative != 0; a.n_lambda = 1;
  a.n_used_rot = int(n_used[0]); a.n_used_pos = int(n_used[1]);
  a.lambda_rot[0] = o.lambda_rot[0]; a.lambda_pos[0] = o.lambda_pos[0];
  a.stamps = d_stamps.p; a.seg = d_seg.p; a.seg_ptr = d_ptr.p; a.knots = d_knots.p; a.basis = d_basis.p; a.data = d_data.p; a.weights = d_weights.p;
  a.W = d_W.p; a.P = d_P.p; a.band = d_band.p; a.rhs = d_rhs.p; a.ctrl_all = d_ctrl.p; a.rows = d_rows.p;
  FitRobustArgs r = {};
  r.loss = ro.loss; r.max_iterations = ro.max_iterations; r.step_tolerance = ro.step_tolerance;
  const double default_tuning = ro.loss == CALICO_ROBUST_HUBER ? 2.7955 : 2.0 * 2.7955;
  for (int g = 0; g < 2; ++g) {
    const double tuning = g == 0 ? ro.tuning_rot : ro.tuning_pos;
    r.rank[g] = int((n_used[g] - 1) / 2);
    r.tuning[g] = tuning > 0.0 ? tuning : default_tuning;
    r.fixed_scale[g] = g == 0 ? ro.scale_rot : ro.scale_pos;
    r.min_scale[g] = g == 0 ? ro.min_scale_rot : ro.min_scale_pos;
  }
  r.e = d_e.p; r.u = d_u.p; r.wu = d_wu.p; r.hist = d_hist.p; r.state = d_state.p;
  FREE_TRY(call, launch_fit_spline_robust(device, a, r, nullptr));
  FitRobustState state[2];
  std::vector<double> ctrl(size_t(n_ctrl) * 6);
  FREE_TRY(call, d_state.download(state, 2)); FREE_TRY(call, d_ctrl.download(ctrl.data(), ctrl.size()));
  std::vector<double> e;
  if (robust_weights_out) FREE_TRY(call, d_u.download(u.data(), u.size()));
  if (residuals_out) { e.resize(size_t(n) * 2); FREE_TRY(call, d_e.download(e.data(), e.size())); }
  int failed = -1;
  for (int g = 0; g < 2; ++g) {
    const FitRobustState& st = state[g];
    summary->status[g] = st.status; summary->iterations[g] = st.iterations; summary->replaced_pivots[g] = st.replaced_pivots;
    summary->n_used[g] = n_used[g]; summary->n_downweighted[g] = st.n_downweighted; summary->n_rejected[g] = st.n_rejected;
    summary->lambda[g] = st.lambda; summary->scale[g] = st.scale; summary->median_residual[g] = st.median; summary->last_step[g] = st.last_step;
    summary->rss[g] = st.rss;
    if (st.status == CALICO_FIT_NOT_POSITIVE_DEFINITE && failed < 0) failed = g;
    if (st.status == CALICO_FIT_NOT_POSITIVE_DEFINITE && st.iterations == 0 && st.done_iter == 1) continue;      // iteration 0 wrote no control points
    for (int i = 0; i < n_ctrl; ++i) for (int c = 0; c < 3; ++c) ctrl_out[size_t(i) * 6 + 3 * g + c] = ctrl[size_t(i) * 6 + 3 * g + c];
    for (int64_t j = 0; j < n; ++j) {
      if (robust_weights_out) robust_weights_out[j * 2 + g] = u[size_t(j) * 2 + g];
      if (residuals_out) residuals_out[j * 2 + g] = e[size_t(j) * 2 + g];
    }
  }
  if (failed >= 0)
    return call.fail(CALICO_INTERNAL, std::string("a pivot of the ") + (failed == 0 ? "rotation" : "position") + " group's normal equations was not finite");
  return CALICO_OK;
}

extern "C" void calico_default_spline_cv_options(calico_spline_cv_options* o) {
  if (!o) return;
  *o = calico_spline_cv_options{};
  o->criterion = CALICO_FIT_CV_GCV;
}

static_assert(sizeof(cal::FitCvRow) == sizeof(calico_spline_cv_row), "the kernels write calico_spline_cv_row");

// calico_fit_spline_cv: the smoothing fit's checks, uploads and launch arguments; the solve kernel also inverts on the band, the
// scores and the choice are the device's (fit_cv_kernels.hip); one readback.
extern "C" int32_t calico_fit_spline_cv(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n,
                                        const double* stamps, const double* data6, const double* weights, const calico_spline_fit_options* fit,
                                        const calico_spline_cv_options* cv, double* ctrl_out, double* ctrl_all_out, calico_spline_fit_row* rows_out,
                                        calico_spline_cv_row* cv_rows_out, double* leverage_out, double* loo_residuals_out,
                                        calico_spline_cv_summary* summary) {
  using namespace cal;
  const FreeCall call{"calico_fit_spline_cv"};
  calico_spline_fit_options o;
  calico_spline_cv_options co;
  if (fit) o = *fit; else calico_default_spline_fit_options(&o);
  if (cv) co = *cv; else calico_default_spline_cv_options(&co);
  std::string error = spline_shape_error(order, n_knots, kMaxOrder);
  if (error.empty() && (!knots || !basis || !stamps || !data6 || !ctrl_out || !summary)) error = "null knots, basis, stamps, data, ctrl_out or summary";
  if (error.empty() && n <= 0) error = "n must be > 0";
  if (error.empty()) error = spline_fit_options_error(order, o);
  if (error.empty()) error = spline_cv_options_error(o, co);
  if (!error.empty()) return call.invalid(error);
  if (n > INT32_MAX) return call.fail(CALICO_UNIMPLEMENTED, "more than 2^31 - 1 samples");      // the kernels and seg_ptr index the samples with int
  if (!(error = stamps_error("sample", n, stamps)).empty()) return call.invalid(error);
  int64_t n_used[2];
  if (!(error = sample_weights_error(n, weights, n_used)).empty()) return call.invalid(error);
  const int k = order, n_ctrl = n_knots - k, n_valid = spline_valid_knots(k, n_knots), n_seg = n_valid - 1, nl = o.n_lambda;
  std::vector<int> seg, seg_ptr;
  if (!(error = bin_samples(k, n_valid, knots, n, stamps, &seg, &seg_ptr)).empty()) return call.invalid(error);
  if (fit_solve_smooth_lds_bytes(n_ctrl, k) > 156 * 1024) return call.fail(CALICO_UNIMPLEMENTED, "the trajectory is too long for the banded solve in LDS");
  if (int rc = call.select_device(device)) return rc;
  const int n_blocks = int((n + 255) / 256);
  FreeBuf<double> d_stamps, d_data, d_weights, d_knots, d_basis, d_W, d_P, d_band, d_rhs, d_ctrl, d_zband, d_edf, d_partial, d_leverage, d_loo;
  FreeBuf<int> d_seg, d_ptr;
  FreeBuf<FitSmoothRow> d_rows;
  FreeBuf<FitCvRow> d_cv_rows;
  FreeBuf<FitCvSummary> d_summary;
  FREE_TRY(call, d_stamps.upload(stamps, size_t(n))); FREE_TRY(call, d_data.upload(data6, size_t(n) * 6));
  if (weights) FREE_TRY(call, d_weights.upload(weights, size_t(n) * 2));
  FREE_TRY(call, d_knots.upload(knots, size_t(n_knots))); FREE_TRY(call, d_basis.upload(basis, size_t(n_seg) * k * k));
  FREE_TRY(call, d_seg.upload(seg.data(), seg.size())); FREE_TRY(call, d_ptr.upload(seg_ptr.data(), seg_ptr.size()));
  FREE_TRY(call, d_W.alloc(size_t(n) * k)); FREE_TRY(call, d_P.alloc(size_t(n_ctrl) * k));
  FREE_TRY(call, d_band.alloc(size_t(2) * n_ctrl * k)); FREE_TRY(call, d_rhs.alloc(size_t(2) * n_ctrl * 3));
  FREE_TRY(call, d_ctrl.alloc(size_t(nl) * n_ctrl * 6)); FREE_TRY(call, d_rows.alloc(size_t(2) * nl));
  FREE_TRY(call, d_zband.alloc(size_t(2) * nl * n_ctrl * k)); FREE_TRY(call, d_edf.alloc(size_t(2) * nl));
  FREE_TRY(call, d_partial.alloc(size_t(2) * nl * n_blocks * 2)); FREE_TRY(call, d_cv_rows.alloc(size_t(2) * nl)); FREE_TRY(call, d_summary.alloc(1));
  FREE_TRY(call, d_leverage.alloc(size_t(n) * 2)); FREE_TRY(call, d_loo.alloc(size_t(n) * 2));
  FitSmoothArgs a = {};
  a.n = int(n); a.k = k; a.n_ctrl = n_ctrl; a.n_seg = n_seg; a.derivative = o.derivative; a.relative = o.relative != 0; a.n_lambda = nl;
  a.n_used_rot = int(n_used[0]); a.n_used_pos = int(n_used[1]);
  for (int l = 0; l < nl; ++l) { a.lambda_rot[l] = o.lambda_rot[l]; a.lambda_pos[l] = o.lambda_pos[l]; }
  a.stamps = d_stamps.p; a.seg = d_seg.p; a.seg_ptr = d_ptr.p; a.knots = d_knots.p; a.basis = d_basis.p; a.data = d_data.p; a.weights = d_weights.p;
  a.W = d_W.p; a.P = d_P.p; a.band = d_band.p; a.rhs = d_rhs.p; a.ctrl_all = d_ctrl.p; a.rows = d_rows.p;
  FitCvArgs c = {};
  c.criterion = co.criterion; c.n_blocks = n_blocks;
  c.zband = d_zband.p; c.edf = d_edf.p; c.partial = d_partial.p; c.cv_rows = d_cv_rows.p; c.summary = d_summary.p; c.leverage = d_leverage.p; c.loo = d_loo.p;
  FREE_TRY(call, launch_fit_spline_cv(device, a, c, nullptr));
  std::vector<FitSmoothRow> rows(size_t(2) * nl);
  std::vector<FitCvRow> cv_rows(size_t(2) * nl);
  std::vector<double> ctrl(size_t(nl) * n_ctrl * 6), leverage, loo;
  FitCvSummary sm;
  FREE_TRY(call, d_summary.download(&sm, 1)); FREE_TRY(call, d_rows.download(rows.data(), rows.size()));
  FREE_TRY(call, d_cv_rows.download(cv_rows.data(), cv_rows.size())); FREE_TRY(call, d_ctrl.download(ctrl.data(), ctrl.size()));
  if (leverage_out) { leverage.resize(size_t(n) * 2); FREE_TRY(call, d_leverage.download(leverage.data(), leverage.size())); }
  if (loo_residuals_out) { loo.resize(size_t(n) * 2); FREE_TRY(call, d_loo.download(loo.data(), loo.size())); }
  // the host's part: the columns of the lambdas that have control points, and the per-sample columns of the groups that chose
  for (int g = 0; g < 2; ++g) {
    summary->status[g] = sm.status[g]; summary->chosen[g] = sm.chosen[g]; summary->n_used[g] = n_used[g];
    summary->edf[g] = sm.edf[g]; summary->score[g] = sm.score[g];
    for (int l = 0; l < nl; ++l) {
      if (rows[size_t(g) * nl + l].status != CALICO_FIT_OK) continue;
      const double* src = ctrl.data() + size_t(l) * n_ctrl * 6 + 3 * g;
      double* const targets[2] = {ctrl_all_out ? ctrl_all_out + size_t(l) * n_ctrl * 6 + 3 * g : nullptr,
                                  l == sm.chosen[g] ? ctrl_out + 3 * g : nullptr};
      for (double* out : targets)
        if (out) for (int i = 0; i < n_ctrl; ++i) for (int ch = 0; ch < 3; ++ch) out[size_t(i) * 6 + ch] = src[size_t(i) * 6 + ch];
    }
    if (sm.chosen[g] < 0) continue;
    for (int64_t j = 0; j < n; ++j) {
      if (leverage_out) leverage_out[j * 2 + g] = leverage[size_t(j) * 2 + g];
      if (loo_residuals_out) loo_residuals_out[j * 2 + g] = loo[size_t(j) * 2 + g];
    }
  }
  if (rows_out) for (size_t i = 0; i < rows.size(); ++i) rows_out[i] = {rows[i].status, rows[i].replaced_pivots, rows[i].lambda, rows[i].rss, rows[i].penalty, rows[i].rms};
  if (cv_rows_out) for (size_t i = 0; i < cv_rows.size(); ++i) cv_rows_out[i] = {cv_rows[i].edf, cv_rows[i].gcv, cv_rows[i].press, cv_rows[i].max_leverage};
  for (int g = 0; g < 2; ++g)
    if (summary->status[g] == CALICO_FIT_NOT_POSITIVE_DEFINITE)
      return call.fail(CALICO_INTERNAL, std::string("no lambda of the ") + (g == 0 ? "rotation" : "position") + " grid has a factorisation cross-validation can use");
  return CALICO_OK;
}
