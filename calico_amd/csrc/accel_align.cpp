// accel_align.cpp — calico_accel_align (this part of the C ABI of include/calico_hip.h): rotation, lever arm, bias, gravity and
// latency of an accelerometer against a fitted trajectory (kernels: accalign_kernels.hip). Everything that can be checked
// without a device is checked before the first HIP call. The host picks the range of samples that take part (the stamps are
// sorted), uploads it, enqueues stage L and every iteration of the loop, and reads the control word back once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/calico_hip.h"
#include "align_host.hpp"
#include "arg_rules.hpp"
#include "device_math.hpp"
#include "free_call.hpp"
#include "kernels.hpp"
#include "lm_rule.hpp"

namespace {
using namespace cal;
const FreeCall call{"calico_accel_align"};
bool finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }
}  // namespace

extern "C" {

void calico_default_accel_alignment_options(calico_accel_alignment_options* o) {
  // max_iterations, step_tolerance, estimate_rotation / _lever_arm / _bias / _gravity / _latency, min_samples, sigma_accel
  if (o) *o = {50, 1e-10, 1, 1, 1, 1, 1, 16, 1.0};
}

int32_t calico_accel_align(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis, const double* ctrl,
                           int64_t n_all, const double* stamps, const double* accel, const double* q_init, const double* latency_init,
                           const double* t_init, const double* bias_init, const double* gravity_init,
                           const calico_accel_alignment_options* opt, double* q_out, double* t_out, double* bias_out, double* gravity_out,
                           double* latency_out, double* cov_out, calico_accel_alignment_summary* summary) {
  std::string error = spline_shape_error(order, n_knots, kMaxOrder);
  if (!error.empty()) return call.invalid(error);
  if (!knots || !basis || !ctrl) return call.invalid("null knots, basis or ctrl");
  if (n_all < 0) return call.invalid("n must be >= 0");
  if (n_all > INT32_MAX) return call.fail(CALICO_UNIMPLEMENTED, "more than 2^31 - 1 samples");
  if (n_all > 0 && (!stamps || !accel)) return call.invalid("null stamps or accel");
  if (!q_out || !t_out || !bias_out || !gravity_out || !latency_out || !summary)
    return call.invalid("null q_rig_accel_out, t_rig_accel_out, bias_out, gravity_world_out, latency_out or summary");
  calico_accel_alignment_options o;
  calico_default_accel_alignment_options(&o);
  if (opt) o = *opt;
  if (!std::isfinite(o.step_tolerance) || !(o.step_tolerance > 0.0)) return call.invalid("step_tolerance must be finite and > 0");
  if (!std::isfinite(o.sigma_accel) || !(o.sigma_accel > 0.0)) return call.invalid("sigma_accel must be finite and > 0");
  if (o.max_iterations < 1) return call.invalid("max_iterations must be >= 1");
  if (o.min_samples < 5) return call.invalid("min_samples must be >= 5");
  if (!q_init || !latency_init) return call.invalid("q_init and latency_init are required");
  const double nrm = quat_norm(q_init);
  if (!std::isfinite(nrm) || !(nrm > 0.0)) return call.invalid("q_init must be finite and of non-zero length");
  if (!std::isfinite(*latency_init)) return call.invalid("latency_init must be finite");
  const int given = (t_init ? 1 : 0) + (bias_init ? 1 : 0) + (gravity_init ? 1 : 0);
  if (given != 0 && given != 3) return call.invalid("t_init, bias_init and gravity_init are given together or not at all");
  const bool linear = given == 0;
  if (linear && (o.estimate_lever_arm == 0 || o.estimate_bias == 0 || o.estimate_gravity == 0))
    return call.invalid("without t_init, bias_init and gravity_init the lever arm, the bias and gravity must all be estimated");
  if (!linear && !(finite3(t_init) && finite3(bias_init) && finite3(gravity_init))) return call.invalid("t_init, bias_init and gravity_init must be finite");
  if (!(error = stamps_error("accel", n_all, stamps)).empty()) return call.invalid(error);
  double q0[4];
  canonical_unit_quat(q_init, nrm, q0);
  const double lat0 = *latency_init;

  int64_t first, end;
  ValidKnots(order, n_knots, knots, lat0, lat0).trim(stamps, n_all, &first, &end);
  const int64_t n_used = end - first;

  *summary = calico_accel_alignment_summary{};
  summary->status = CALICO_ALIGN_TOO_FEW_SAMPLES; summary->linear_status = -1; summary->samples = n_used; summary->first_sample = first;
  summary->lambda = kLmLambda0;
  const auto give_start = [&]() {
    std::copy(q0, q0 + 4, q_out);
    for (int i = 0; i < 3; ++i) { t_out[i] = linear ? 0.0 : t_init[i]; bias_out[i] = linear ? 0.0 : bias_init[i]; gravity_out[i] = linear ? 0.0 : gravity_init[i]; }
    *latency_out = lat0;
    give_covariance(cov_out, nullptr, kAccAlignParams, false);
    summary->gravity_norm = std::sqrt(gravity_out[0] * gravity_out[0] + gravity_out[1] * gravity_out[1] + gravity_out[2] * gravity_out[2]);
  };
  if (n_used < o.min_samples) { give_start(); return CALICO_OK; }

  if (int rc = call.select_device(device)) return rc;

  const int n = int(n_used), chunks = accalign_chunks(n);
  SplineOnDevice d_spline;
  FreeBuf<double> d_stamps, d_meas, d_part;
  FreeBuf<AccAlignControl> d_c;
  FREE_TRY(call, d_spline.upload(order, n_knots, knots, basis, ctrl)); FREE_TRY(call, d_stamps.upload(stamps + first, size_t(n)));
  FREE_TRY(call, d_meas.upload(accel + 3 * first, size_t(n) * 3)); FREE_TRY(call, d_part.alloc(size_t(chunks) * kAccAlignPart));

  AccAlignControl c;
  std::memset(&c, 0, sizeof(c));
  start_point_lm(&c.lm);
  c.linear_status = -1;
  c.stage = linear ? kAccAlignStageLinear : kAccAlignStageLoop;
  for (int s = 0; s < 2; ++s) {
    for (int i = 0; i < 4; ++i) c.q[s][i] = q0[i];
    for (int i = 0; i < 3; ++i) { c.t[s][i] = linear ? 0.0 : t_init[i]; c.bias[s][i] = linear ? 0.0 : bias_init[i]; c.gravity[s][i] = linear ? 0.0 : gravity_init[i]; }
    c.latency[s] = lat0;
  }
  FREE_TRY(call, d_c.upload(&c, 1));

  AccAlignArgs a = {};
  a.ctrl = d_c.p; a.spline = d_spline.spline;
  a.stamps = d_stamps.p; a.meas = d_meas.p; a.n = n; a.part = d_part.p;
  a.free_bits = (o.estimate_rotation != 0 ? 0x7u : 0u) | (o.estimate_lever_arm != 0 ? 0x38u : 0u) | (o.estimate_bias != 0 ? 0x1c0u : 0u) |
                (o.estimate_gravity != 0 ? 0xe00u : 0u) | (o.estimate_latency != 0 ? 0x1000u : 0u);
  a.max_iterations = o.max_iterations; a.step_tolerance = o.step_tolerance; a.inv_sigma = 1.0 / o.sigma_accel;

  // stage L is two launches; the loop's first launch evaluates the start, every later one a candidate; launches behind the end
  // return at once
  FREE_TRY(call, enqueue_point_lm((linear ? 2 : 0) + o.max_iterations + 2, [&] { return launch_accalign_iteration(a, nullptr); }));
  FREE_TRY(call, launch_accalign_finish(a, nullptr));
  FREE_TRY(call, d_c.download(&c, 1));

  summary->status = c.lm.status; summary->linear_status = c.linear_status; summary->iterations = c.lm.iterations;
  summary->initial_cost = c.lm.initial_cost; summary->final_cost = c.lm.final_cost; summary->lambda = c.lm.lambda; summary->rms = c.rms;
  summary->linear_rms = c.linear_rms;
  if (c.lm.first != 0 || c.lm.status == CALICO_ALIGN_DEGENERATE) {
    give_start();
  } else {
    const int cur = c.lm.cur;
    std::copy(c.q[cur], c.q[cur] + 4, q_out);
    std::copy(c.t[cur], c.t[cur] + 3, t_out);
    std::copy(c.bias[cur], c.bias[cur] + 3, bias_out);
    std::copy(c.gravity[cur], c.gravity[cur] + 3, gravity_out);
    *latency_out = c.latency[cur];
    give_covariance(cov_out, c.cov, kAccAlignParams, point_lm_ran(c.lm.status) && c.lm.cov_ok);
  }
  summary->gravity_norm = std::sqrt(gravity_out[0] * gravity_out[0] + gravity_out[1] * gravity_out[1] + gravity_out[2] * gravity_out[2]);
  return CALICO_OK;
}

}  // extern "C"
