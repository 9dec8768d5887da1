// camera_align.cpp — calico_camera_align (this part of the C ABI of include/calico_hip.h): the extrinsics T_rig_camera and the
// latency of a camera against a fitted trajectory from its raw chart detections (kernels: camalign_kernels.hip, started from a
// resection of every frame, resect_kernels.hip). Everything that can be checked without a device is checked before the first
// HIP call (arg_rules.hpp). The host picks the frames that take part and packs them, uploads, enqueues every stage and every
// iteration of the refinement, and reads the control word back once.
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
#include "lm_host.hpp"
#include "lm_rule.hpp"

namespace {
using namespace cal;
const FreeCall call{"calico_camera_align"};
}  // namespace

extern "C" {

void calico_default_camera_alignment_options(calico_camera_alignment_options* o) {
  // max_lag, lag_step, max_iterations, step_tolerance, estimate_latency, estimate_translation, huber_scale, min_points, min_frames, sigma_pixel
  if (o) *o = {0.1, 1e-3, 50, 1e-10, 1, 1, 0.0, 4, 8, 1.0};
}

int32_t calico_camera_align(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis, const double* ctrl,
                            int32_t model, const double* intrinsics, int32_t n_intrinsics, const double* q_world_chart,
                            const double* t_world_chart, int64_t n_frames, const double* frame_stamps, const int64_t* frame_offsets,
                            const double* pixels, const double* points, const double* q_init, const double* t_init,
                            const double* latency_init, const calico_camera_alignment_options* opt, double* q_out, double* t_out,
                            double* latency_out, double* frame_rms_out, int32_t* frame_n_used_out, uint8_t* frame_status_out,
                            double* cov_out, double* curve_out, calico_camera_alignment_summary* summary) {
  calico_camera_alignment_options o;
  calico_default_camera_alignment_options(&o);
  if (opt) o = *opt;
  int half = 0;
  std::string error = spline_shape_error(order, n_knots, kMaxOrder);
  if (error.empty() && (!knots || !basis || !ctrl)) error = "null knots, basis or ctrl";
  if (error.empty()) error = camera_model_error(model, camera_model_num_params(model), intrinsics, n_intrinsics);
  if (error.empty()) error = chart_options_error(n_frames, o, nullptr, nullptr);
  if (error.empty()) error = camera_alignment_options_error(o, kAlignMaxLags, &half);
  if (error.empty()) error = camera_alignment_start_error(q_world_chart, t_world_chart, q_init, t_init, latency_init);
  if (error.empty() && !(q_out && t_out && latency_out && summary)) error = "null q_rig_camera_out, t_rig_camera_out, latency_out or summary";
  if (error.empty() && n_frames > INT32_MAX) return call.fail(CALICO_UNIMPLEMENTED, "more than 2^31 - 1 frames");
  if (error.empty() && n_frames > 0) {
    if (!frame_stamps) error = "null frame_stamps";
    if (error.empty())
      error = chart_frames_error(n_frames, frame_offsets, frame_rms_out && frame_n_used_out && frame_status_out,
                                 "null frame offsets or frame output buffer", pixels, points);
    if (error.empty()) error = stamps_error("frame", n_frames, frame_stamps);
  }
  if (!error.empty()) return call.invalid(error);

  double q0[4] = {0.0, 0.0, 0.0, 1.0}, t0[3] = {0.0, 0.0, 0.0}, lat0 = 0.0, q_wm[4] = {0.0, 0.0, 0.0, 1.0}, t_wm[3] = {0.0, 0.0, 0.0};
  if (q_init) {
    canonical_unit_quat(q_init, quat_norm(q_init), q0);
    std::copy(t_init, t_init + 3, t0);
    lat0 = *latency_init;
  }
  if (q_world_chart) canonical_unit_quat(q_world_chart, quat_norm(q_world_chart), q_wm);
  if (t_world_chart) std::copy(t_world_chart, t_world_chart + 3, t_wm);

  // the grid, and the frames every latency of it keeps on the valid knots
  const int n_lags = 2 * half + 1;
  std::vector<double> lags(static_cast<size_t>(n_lags));
  for (int l = 0; l < n_lags; ++l) lags[size_t(l)] = lat0 + double(l - half) * o.lag_step;
  const bool search = !q_init && o.estimate_latency != 0;
  const double lat_lo = search ? lags.front() : lat0, lat_hi = search ? lags.back() : lat0;      // (no search: no grid to keep on the knots)
  const ValidKnots on_knots(order, n_knots, knots, lat_lo, lat_hi);
  const size_t F = size_t(n_frames);
  std::vector<int64_t> part;      // the frames that take part, in stamp order
  std::vector<int64_t> off(1, 0);
  for (size_t f = 0; f < F; ++f) {
    const double s = frame_stamps[f];
    const int64_t n = frame_offsets[f + 1] - frame_offsets[f];
    uint8_t st = CALICO_RESECT_OK;
    if (n < o.min_points) st = CALICO_RESECT_TOO_FEW_POINTS;
    else if (!(on_knots.from(s) && on_knots.until(s))) st = CALICO_CAMERA_ALIGN_FRAME_OUTSIDE;
    frame_status_out[f] = st; frame_rms_out[f] = 0.0; frame_n_used_out[f] = 0;
    if (st == CALICO_RESECT_OK) { part.push_back(int64_t(f)); off.push_back(off.back() + n); }
  }
  const size_t nf = part.size(), np = size_t(off.back());

  *summary = calico_camera_alignment_summary{};
  summary->status = CALICO_ALIGN_TOO_FEW_SAMPLES; summary->frames_used = int64_t(nf); summary->peak_index = -1;
  summary->coarse_latency = lat0; summary->lambda = kLmLambda0;
  const auto give_start = [&]() {
    std::copy(q0, q0 + 4, q_out); std::copy(t0, t0 + 3, t_out);
    *latency_out = lat0;
    give_covariance(cov_out, nullptr, 7, false);
  };
  if (int64_t(nf) < o.min_frames) { give_start(); return CALICO_OK; }
  if (np > size_t(INT32_MAX)) return call.fail(CALICO_UNIMPLEMENTED, "more than 2^31 - 1 pairs");

  if (int rc = call.select_device(device)) return rc;

  // the frames that take part, packed
  std::vector<double> stamps(nf), px(np * 2), pt(np * 3);
  for (size_t i = 0; i < nf; ++i) {
    const size_t f = size_t(part[i]);
    const int64_t b = frame_offsets[f], n = frame_offsets[f + 1] - b;
    stamps[i] = frame_stamps[f];
    std::copy(pixels + 2 * b, pixels + 2 * (b + n), px.begin() + 2 * off[i]);
    std::copy(points + 3 * b, points + 3 * (b + n), pt.begin() + 3 * off[i]);
  }
  const int n = int(nf), chunks = camalign_chunks(n);
  SplineOnDevice d_spline;
  FreeBuf<double> d_k, d_stamps, d_px, d_pt, d_lags, d_pose, d_curve, d_frames, d_rms;
  FreeBuf<int64_t> d_off;
  FreeBuf<int32_t> d_used;
  FreeBuf<uint8_t> d_fl, d_rfl, d_active, d_status;
  FreeBuf<CamAlignControl> d_c;
  ResectRun run;
  FREE_TRY(call, d_spline.upload(order, n_knots, knots, basis, ctrl)); FREE_TRY(call, d_k.upload(intrinsics, size_t(n_intrinsics)));
  FREE_TRY(call, d_stamps.upload(stamps.data(), nf)); FREE_TRY(call, d_px.upload(px.data(), np * 2)); FREE_TRY(call, d_pt.upload(pt.data(), np * 3));
  FREE_TRY(call, d_off.upload(off.data(), nf + 1)); FREE_TRY(call, d_lags.upload(lags.data(), lags.size()));
  FREE_TRY(call, d_pose.alloc(size_t(chunks) * size_t(n_lags) * kCamAlignPoseSums)); FREE_TRY(call, d_curve.alloc(size_t(n_lags)));
  FREE_TRY(call, d_frames.alloc(nf * kCamAlignFrameDoubles)); FREE_TRY(call, d_frames.zero(nf * kCamAlignFrameDoubles));
  FREE_TRY(call, d_rms.alloc(nf)); FREE_TRY(call, d_used.alloc(nf));
  FREE_TRY(call, d_fl.alloc(np)); FREE_TRY(call, d_fl.zero(np));
  std::vector<uint8_t> ones(nf, uint8_t(1)), st_part(nf, uint8_t(CALICO_RESECT_OK));
  FREE_TRY(call, d_active.upload(ones.data(), nf)); FREE_TRY(call, d_status.upload(st_part.data(), nf));

  CamAlignControl c;
  std::memset(&c, 0, sizeof(c));
  start_point_lm(&c.lm);
  c.peak_index = -1; c.frames_used = n; c.coarse_latency = lat0;
  for (int s = 0; s < 2; ++s) {
    std::copy(q0, q0 + 4, c.q[s]); std::copy(t0, t0 + 3, c.t[s]);
    c.latency[s] = lat0;
  }
  FREE_TRY(call, d_c.upload(&c, 1));

  CamAlignArgs a = {};
  a.ctrl = d_c.p; a.spline = d_spline.spline; a.k = d_k.p;
  std::copy(q_wm, q_wm + 4, a.q_wm); std::copy(t_wm, t_wm + 3, a.t_wm);
  a.n_frames = n; a.stamps = d_stamps.p; a.offsets = d_off.p; a.pixels = d_px.p; a.points = d_pt.p; a.flags = d_fl.p;
  a.active = d_active.p; a.frame_status = d_status.p;
  a.lags = d_lags.p; a.n_lags = n_lags; a.lag_step = o.lag_step; a.pose_part = d_pose.p; a.curve = d_curve.p; a.frames = d_frames.p;
  a.free_bits = 7u | (o.estimate_translation != 0 ? 0x38u : 0u) | (o.estimate_latency != 0 ? 0x40u : 0u);
  a.max_iterations = o.max_iterations; a.step_tolerance = o.step_tolerance; a.inv_sigma = 1.0 / o.sigma_pixel;
  a.huber_scale = o.huber_scale; a.min_frames = o.min_frames;
  a.frame_rms_out = d_rms.p; a.frame_n_used_out = d_used.p;

  if (!q_init) {
    calico_resection_options ro;
    calico_default_resection_options(&ro);
    ro.huber_scale = o.huber_scale; ro.min_points = o.min_points;
    FREE_TRY(call, d_rfl.alloc(np)); FREE_TRY(call, d_rfl.zero(np));
    FREE_TRY(call, run.alloc(nf, np, false));
    FREE_TRY(call, launch_camera_resect(model, run.args(ro, d_k.p, int64_t(nf), d_off.p, d_px.p, d_pt.p, d_rfl.p, nullptr, nullptr), nullptr));
    a.q_cm = run.q.p; a.t_cm = run.t.p; a.resect_status = run.status.p;
    FREE_TRY(call, launch_camalign_gate(a, nullptr));
    if (search) FREE_TRY(call, launch_camalign_search(a, nullptr));
    FREE_TRY(call, launch_camalign_mean(a, nullptr));
  }
  // the first launch evaluates the start, every later one a candidate; launches behind the end return at once
  FREE_TRY(call, enqueue_point_lm(o.max_iterations + 2, [&] { return launch_camalign_iteration(model, a, nullptr); }));
  FREE_TRY(call, launch_camalign_finish(a, nullptr));
  FREE_TRY(call, d_c.download(&c, 1));
  if (search && c.lm.status != CALICO_ALIGN_TOO_FEW_SAMPLES && (c.peak_index >= 0)) {
    summary->n_lags = n_lags;
    if (curve_out) FREE_TRY(call, d_curve.download(curve_out, size_t(n_lags)));
  }
  std::vector<double> rms(nf);
  std::vector<int32_t> used(nf);
  FREE_TRY(call, d_rms.download(rms.data(), nf)); FREE_TRY(call, d_used.download(used.data(), nf));
  FREE_TRY(call, d_status.download(st_part.data(), nf));
  for (size_t i = 0; i < nf; ++i) {
    const size_t f = size_t(part[i]);
    frame_rms_out[f] = rms[i]; frame_n_used_out[f] = used[i]; frame_status_out[f] = st_part[i];
  }

  summary->status = c.lm.status; summary->iterations = c.lm.iterations; summary->frames_used = c.frames_used; summary->pairs_used = c.pairs_used;
  summary->peak_index = c.peak_index; summary->coarse_latency = c.coarse_latency; summary->peak_score = c.peak_score;
  summary->rms = c.rms; summary->initial_cost = c.lm.initial_cost; summary->final_cost = c.lm.final_cost; summary->lambda = c.lm.lambda;
  if (c.lm.first != 0 || c.lm.status == CALICO_ALIGN_DEGENERATE || c.lm.status == CALICO_ALIGN_NO_PEAK || c.lm.status == CALICO_ALIGN_TOO_FEW_SAMPLES) {
    give_start();
  } else {
    const int cur = c.lm.cur;
    std::copy(c.q[cur], c.q[cur] + 4, q_out); std::copy(c.t[cur], c.t[cur] + 3, t_out);
    *latency_out = c.latency[cur];
    give_covariance(cov_out, c.cov, 7, point_lm_ran(c.lm.status) && c.lm.cov_ok);
  }
  return CALICO_OK;
}

}  // extern "C"
