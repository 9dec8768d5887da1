// imu_align.cpp — calico_imu_align (this part of the C ABI of include/calico_hip.h): rotation, gyroscope bias, latency and gravity
// of an IMU against a fitted trajectory (kernels: align_kernels.hip). Everything that can be checked without a device is checked
// before the first HIP call. The host picks the range of samples that take part (the stamps are sorted), uploads it, enqueues
// every stage and every iteration of the refinement, and reads the control word back once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/calico_hip.h"
#include "align_host.hpp"
#include "arg_rules.hpp"
#include "device_math.hpp"
#include "free_call.hpp"
#include "kernels.hpp"
#include "lm_rule.hpp"

namespace {
using namespace cal;
const FreeCall call{"calico_imu_align"};
static_assert(kAlignMaxLags == CALICO_ALIGN_MAX_LAGS, "the peak kernel's curve holds what the header promises");
}  // namespace

extern "C" {

void calico_default_imu_alignment_options(calico_imu_alignment_options* o) {
  // max_lag, lag_step, max_iterations, step_tolerance, estimate_latency / _gyro_bias / _accel_bias, min_samples, sigma_gyro
  if (o) *o = {0.1, 1e-3, 50, 1e-10, 1, 1, 1, 16, 1.0};
}

int32_t calico_imu_align(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis, const double* ctrl,
                         int64_t n_gyro, const double* gyro_stamps, const double* gyro, int64_t n_accel, const double* accel_stamps,
                         const double* accel, const double* t_rig_accel, const double* q_init, const double* latency_init,
                         const calico_imu_alignment_options* opt, double* q_out, double* bias_out, double* latency_out,
                         double* gravity_out, double* accel_bias_out, double* cov_out, double* curve_out,
                         calico_imu_alignment_summary* summary) {
  std::string error = spline_shape_error(order, n_knots, kMaxOrder);
  if (!error.empty()) return call.invalid(error);
  if (!knots || !basis || !ctrl) return call.invalid("null knots, basis or ctrl");
  if (n_gyro < 0 || n_accel < 0) return call.invalid("n_gyro and n_accel must be >= 0");
  if (n_gyro > INT32_MAX || n_accel > INT32_MAX) return call.fail(CALICO_UNIMPLEMENTED, "more than 2^31 - 1 samples");
  if (n_gyro > 0 && (!gyro_stamps || !gyro)) return call.invalid("null gyro_stamps or gyro");
  if (n_accel > 0 && (!accel_stamps || !accel)) return call.invalid("null accel_stamps or accel");
  if (!q_out || !bias_out || !latency_out || !summary) return call.invalid("null q_rig_gyro_out, gyro_bias_out, latency_out or summary");
  if (n_accel > 0 && (!gravity_out || !accel_bias_out)) return call.invalid("null gravity_world_out or accel_bias_out");
  calico_imu_alignment_options o;
  calico_default_imu_alignment_options(&o);
  if (opt) o = *opt;
  if (!std::isfinite(o.lag_step) || !(o.lag_step > 0.0)) return call.invalid("lag_step must be finite and > 0");
  if (!std::isfinite(o.max_lag) || o.max_lag < 0.0) return call.invalid("max_lag must be finite and >= 0");
  const double half = std::floor(o.max_lag / o.lag_step * (1.0 + 1e-9));
  if (!(2.0 * half + 1.0 <= double(kAlignMaxLags))) return call.invalid("max_lag / lag_step gives more than " + std::to_string(kAlignMaxLags) + " lags");
  if (!std::isfinite(o.step_tolerance) || !(o.step_tolerance > 0.0)) return call.invalid("step_tolerance must be finite and > 0");
  if (!std::isfinite(o.sigma_gyro) || !(o.sigma_gyro > 0.0)) return call.invalid("sigma_gyro must be finite and > 0");
  if (o.max_iterations < 1) return call.invalid("max_iterations must be >= 1");
  if (o.min_samples < 3) return call.invalid("min_samples must be >= 3");
  if ((q_init == nullptr) != (latency_init == nullptr)) return call.invalid("q_init and latency_init are given together or not at all");
  double q0[4] = {0.0, 0.0, 0.0, 1.0};
  double lat0 = 0.0;
  if (q_init) {
    const double nrm = quat_norm(q_init);
    if (!std::isfinite(nrm) || !(nrm > 0.0)) return call.invalid("q_init must be finite and of non-zero length");
    if (!std::isfinite(*latency_init)) return call.invalid("latency_init must be finite");
    canonical_unit_quat(q_init, nrm, q0);
    lat0 = *latency_init;
  }
  if (!(error = stamps_error("gyro", n_gyro, gyro_stamps)).empty()) return call.invalid(error);
  if (!(error = stamps_error("accel", n_accel, accel_stamps)).empty()) return call.invalid(error);

  // the grid, and the samples every latency of it keeps on the valid knots
  const int L = int(half), n_lags = 2 * L + 1;
  std::vector<double> lags(static_cast<size_t>(n_lags));
  for (int l = 0; l < n_lags; ++l) lags[size_t(l)] = lat0 + double(l - L) * o.lag_step;
  const bool search = !q_init && o.estimate_latency != 0;
  const double lat_lo = search ? lags.front() : lat0, lat_hi = search ? lags.back() : lat0;      // (no search: no grid to keep on the knots)
  int64_t first, end;
  ValidKnots(order, n_knots, knots, lat_lo, lat_hi).trim(gyro_stamps, n_gyro, &first, &end);
  const int64_t n_used = end - first;

  *summary = calico_imu_alignment_summary{};
  summary->gyro_status = CALICO_ALIGN_TOO_FEW_SAMPLES; summary->accel_status = CALICO_ALIGN_TOO_FEW_SAMPLES;
  summary->gyro_samples = n_used; summary->first_sample = first; summary->peak_index = -1; summary->coarse_latency = lat0;
  summary->lambda = kLmLambda0;
  const auto give_start = [&]() {
    std::copy(q0, q0 + 4, q_out);
    bias_out[0] = bias_out[1] = bias_out[2] = 0.0;
    *latency_out = lat0;
    give_covariance(cov_out, nullptr, 7, false);
  };
  if (n_used < o.min_samples) { give_start(); return CALICO_OK; }

  if (int rc = call.select_device(device)) return rc;

  const int n = int(n_used), chunks = align_chunks(n), accel_chunks = align_chunks(int(n_accel));
  SplineOnDevice d_spline;
  FreeBuf<double> d_stamps, d_meas, d_lags, d_corr, d_corr_m, d_curve, d_part, d_as, d_am;
  FreeBuf<AlignControl> d_c;
  FREE_TRY(call, d_spline.upload(order, n_knots, knots, basis, ctrl)); FREE_TRY(call, d_stamps.upload(gyro_stamps + first, size_t(n)));
  FREE_TRY(call, d_meas.upload(gyro + 3 * first, size_t(n) * 3)); FREE_TRY(call, d_lags.upload(lags.data(), lags.size()));
  FREE_TRY(call, d_corr.alloc(search ? size_t(chunks) * n_lags * 3 : 0)); FREE_TRY(call, d_corr_m.alloc(size_t(chunks) * 2));
  FREE_TRY(call, d_curve.alloc(size_t(n_lags))); FREE_TRY(call, d_part.alloc(size_t(std::max(chunks, accel_chunks)) * kAlignPart));
  FREE_TRY(call, d_as.upload(accel_stamps, size_t(n_accel))); FREE_TRY(call, d_am.upload(accel, size_t(n_accel) * 3));

  AlignControl c;
  std::memset(&c, 0, sizeof(c));
  start_point_lm(&c.lm);
  c.accel_status = CALICO_ALIGN_TOO_FEW_SAMPLES; c.peak_index = -1; c.coarse_latency = lat0;
  for (int s = 0; s < 2; ++s) {
    for (int i = 0; i < 4; ++i) c.q[s][i] = q0[i];
    c.latency[s] = lat0;
  }
  FREE_TRY(call, d_c.upload(&c, 1));

  AlignArgs a = {};
  a.ctrl = d_c.p; a.spline = d_spline.spline;
  a.stamps = d_stamps.p; a.meas = d_meas.p; a.n = n; a.lags = d_lags.p; a.n_lags = n_lags; a.lag_step = o.lag_step;
  a.corr_part = d_corr.p; a.corr_m = d_corr_m.p; a.curve = d_curve.p; a.part = d_part.p;
  a.free_bits = 7u | (o.estimate_gyro_bias != 0 ? 0x38u : 0u) | (o.estimate_latency != 0 ? 0x40u : 0u);
  a.max_iterations = o.max_iterations; a.step_tolerance = o.step_tolerance; a.inv_sigma = 1.0 / o.sigma_gyro;
  a.accel_stamps = d_as.p; a.accel = d_am.p; a.n_accel = int(n_accel);
  for (int i = 0; i < 3; ++i) a.t_ra[i] = t_rig_accel ? t_rig_accel[i] : 0.0;
  a.estimate_accel_bias = o.estimate_accel_bias; a.min_samples = o.min_samples;

  if (search) FREE_TRY(call, launch_align_correlate(a, nullptr));
  if (!q_init) FREE_TRY(call, launch_align_horn(a, nullptr));
  // the first launch evaluates the start, every later one a candidate; launches behind the end return at once
  FREE_TRY(call, enqueue_point_lm(o.max_iterations + 2, [&] { return launch_align_iteration(a, nullptr); }));
  FREE_TRY(call, launch_align_finish(a, nullptr));
  FREE_TRY(call, launch_align_gravity(a, nullptr));
  FREE_TRY(call, d_c.download(&c, 1));
  if (search) {
    summary->n_lags = n_lags;
    if (curve_out) FREE_TRY(call, d_curve.download(curve_out, size_t(n_lags)));
  }

  summary->gyro_status = c.lm.status; summary->iterations = c.lm.iterations; summary->peak_index = c.peak_index;
  summary->coarse_latency = c.coarse_latency; summary->peak_correlation = c.peak_correlation; summary->scatter_pivot = c.scatter_pivot;
  summary->initial_cost = c.lm.initial_cost; summary->final_cost = c.lm.final_cost; summary->lambda = c.lm.lambda; summary->gyro_rms = c.gyro_rms;
  const bool ran = point_lm_ran(c.lm.status);
  if (c.lm.first != 0 || c.lm.status == CALICO_ALIGN_DEGENERATE || c.lm.status == CALICO_ALIGN_NO_PEAK) {
    give_start();
  } else {
    const int cur = c.lm.cur;
    std::copy(c.q[cur], c.q[cur] + 4, q_out);
    std::copy(c.bias[cur], c.bias[cur] + 3, bias_out);
    *latency_out = c.latency[cur];
    give_covariance(cov_out, c.cov, 7, ran && c.lm.cov_ok);
  }
  if (!ran) {
    summary->accel_status = c.lm.status;
  } else if (n_accel > 0) {
    summary->accel_status = c.accel_status; summary->accel_samples = c.accel_samples;
    if (c.accel_status == CALICO_ALIGN_OK) {
      std::copy(c.gravity, c.gravity + 3, gravity_out);
      std::copy(c.accel_bias, c.accel_bias + 3, accel_bias_out);
      summary->accel_rms = c.accel_rms;
      summary->gravity_norm = std::sqrt(c.gravity[0] * c.gravity[0] + c.gravity[1] * c.gravity[1] + c.gravity[2] * c.gravity[2]);
    }
  }
  return CALICO_OK;
}

}  // extern "C"
