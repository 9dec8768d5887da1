// chart.cpp — the calls over a ragged batch of chart frames (this part of the C ABI of include/calico_hip.h): the chart resection
// (calico_camera_resect, resect_kernels.hip) and the intrinsic calibration (calico_camera_calibrate, calib_kernels.hip), which
// starts from a resection of its own. What can be checked without a device is checked before the first HIP call (arg_rules.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/calico_hip.h"
#include "arg_rules.hpp"
#include "calico_hip_testing.h"
#include "free_call.hpp"
#include "kernels.hpp"
#include "lm_host.hpp"
#include "lm_rule.hpp"

namespace {

using namespace cal;

// pairs per pass of calico_camera_resect: upload, kernel, download (2^20 pairs: 40 MB in, 17 MB of workspace). A frame is never
// split; one with more pairs than this travels alone.
constexpr int64_t kResectChunkPairs = int64_t(1) << 20;
// calico_camera_calibrate: the whole batch lives on the device for the length of the call (every iteration reads every pair:
// nothing is chunked).

}  // namespace

extern "C" {

// calico_camera_resect with the pairs per pass given (test hook, calico_hip_testing.h)
int32_t calico_debug_camera_resect_chunked(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n_frames,
                                           const int64_t* offsets, const double* pixels, const double* points, const double* q_init,
                                           const double* t_init, const calico_resection_options* opt, double* q_out, double* t_out,
                                           double* rms_out, int32_t* n_used_out, int32_t* iterations_out, uint8_t* status_out,
                                           double* cov_out, int64_t chunk_pairs) {
  const FreeCall call{"calico_camera_resect"};
  calico_resection_options o;
  calico_default_resection_options(&o);
  if (opt) o = *opt;
  std::string error = camera_model_error(model, camera_model_num_params(model), intrinsics, n_intrinsics);
  if (error.empty()) error = chart_options_error(n_frames, o, q_init, t_init);
  if (error.empty() && chunk_pairs < 1) error = "chunk must be >= 1";
  if (!error.empty()) return call.invalid(error);
  if (n_frames == 0) return CALICO_OK;
  error = chart_frames_error(n_frames, offsets, q_out && t_out && rms_out && n_used_out && iterations_out && status_out,
                             "null frame offsets or output buffer", pixels, points);
  if (!error.empty()) return call.invalid(error);
  if (int rc = call.select_device(device)) return rc;
  // chunks of whole frames: [f0, f1) with at most chunk_pairs pairs, or one frame
  std::vector<int64_t> cuts(1, 0);
  int64_t max_pairs = 0, max_frames = 0;
  for (int64_t f0 = 0; f0 < n_frames;) {
    int64_t f1 = f0 + 1;
    while (f1 < n_frames && offsets[f1 + 1] - offsets[f0] <= chunk_pairs) ++f1;
    cuts.push_back(f1);
    max_pairs = std::max(max_pairs, offsets[f1] - offsets[f0]);
    max_frames = std::max(max_frames, f1 - f0);
    f0 = f1;
  }
  const size_t K = size_t(n_intrinsics), F = size_t(max_frames), P = size_t(max_pairs);
  FreeBuf<double> d_k, d_px, d_pt, d_qi, d_ti;
  FreeBuf<int64_t> d_off;
  FreeBuf<uint8_t> d_fl;
  ResectRun run;
  FREE_TRY(call, d_k.upload(intrinsics, K)); FREE_TRY(call, d_px.alloc(P * 2)); FREE_TRY(call, d_pt.alloc(P * 3));
  FREE_TRY(call, d_fl.alloc(P)); FREE_TRY(call, d_off.alloc(F + 1));
  if (q_init) { FREE_TRY(call, d_qi.alloc(F * 4)); FREE_TRY(call, d_ti.alloc(F * 3)); }
  FREE_TRY(call, run.alloc(F, P, cov_out != nullptr));
  std::vector<int64_t> local;
  for (size_t c = 0; c + 1 < cuts.size(); ++c) {
    const int64_t f0 = cuts[c], f1 = cuts[c + 1], p0 = offsets[f0];
    const size_t nf = size_t(f1 - f0), np = size_t(offsets[f1] - p0);
    local.assign(nf + 1, 0);
    for (size_t f = 0; f <= nf; ++f) local[f] = offsets[size_t(f0) + f] - p0;
    FREE_TRY(call, d_off.put(local.data(), local.size()));
    FREE_TRY(call, d_px.put(pixels + 2 * p0, np * 2)); FREE_TRY(call, d_pt.put(points + 3 * p0, np * 3));
    if (np > 0) FREE_TRY(call, d_fl.zero(np));
    if (q_init) { FREE_TRY(call, d_qi.put(q_init + 4 * f0, nf * 4)); FREE_TRY(call, d_ti.put(t_init + 3 * f0, nf * 3)); }
    FREE_TRY(call, launch_camera_resect(model, run.args(o, d_k.p, int64_t(nf), d_off.p, d_px.p, d_pt.p, d_fl.p, d_qi.p, d_ti.p), nullptr));
    FREE_TRY(call, run.q.download(q_out + 4 * f0, nf * 4)); FREE_TRY(call, run.t.download(t_out + 3 * f0, nf * 3));
    FREE_TRY(call, run.rms.download(rms_out + f0, nf)); FREE_TRY(call, run.used.download(n_used_out + f0, nf));
    FREE_TRY(call, run.iterations.download(iterations_out + f0, nf)); FREE_TRY(call, run.status.download(status_out + f0, nf));
    if (cov_out) FREE_TRY(call, run.cov.download(cov_out + 36 * f0, nf * 36));
  }
  return CALICO_OK;
}

int32_t calico_camera_calibrate(int32_t device, int32_t model, const double* k_init, int32_t n_intrinsics, const uint8_t* free_mask,
                                int64_t n_frames, const int64_t* offsets, const double* pixels, const double* points, const double* q_init,
                                const double* t_init, const calico_calibration_options* opt, double* k_out, double* q_out, double* t_out,
                                double* rms_out, int32_t* n_used_out, uint8_t* status_out, double* cov_out,
                                calico_calibration_summary* summary) {
  const FreeCall call{"calico_camera_calibrate"};
  calico_calibration_options o;
  calico_default_calibration_options(&o);
  if (opt) o = *opt;
  std::string error = camera_model_error(model, camera_model_num_params(model), k_init, n_intrinsics);
  if (error.empty()) error = chart_options_error(n_frames, o, q_init, t_init);
  if (!error.empty()) return call.invalid(error);
  const int K = n_intrinsics;
  unsigned free_bits = 0;
  for (int i = 0; i < K; ++i)
    if (!free_mask || free_mask[i]) free_bits |= 1u << i;
  if (free_bits == 0) return call.invalid("free_mask leaves no intrinsic free");
  if (n_frames == 0) return CALICO_OK;
  error = chart_frames_error(n_frames, offsets, k_out && q_out && t_out && rms_out && n_used_out && status_out && summary,
                             "null frame offsets, output buffer or summary", pixels, points);
  if (!error.empty()) return call.invalid(error);
  if (int rc = call.select_device(device)) return rc;
  const size_t F = size_t(n_frames), P = size_t(offsets[n_frames]), N = size_t(K) + 7;
  FreeBuf<double> d_px, d_pt, d_q, d_t, d_rms, d_frames, d_gram, d_share, d_cov;
  FreeBuf<int64_t> d_off;
  FreeBuf<int32_t> d_used;
  FreeBuf<uint8_t> d_fl, d_st, d_act;
  FreeBuf<CalibControl> d_ctrl;
  FREE_TRY(call, d_px.upload(pixels, P * 2)); FREE_TRY(call, d_pt.upload(points, P * 3));
  FREE_TRY(call, d_fl.alloc(P)); FREE_TRY(call, d_off.upload(offsets, F + 1)); FREE_TRY(call, d_q.alloc(F * 4)); FREE_TRY(call, d_t.alloc(F * 3));
  FREE_TRY(call, d_rms.alloc(F)); FREE_TRY(call, d_used.alloc(F)); FREE_TRY(call, d_st.alloc(F)); FREE_TRY(call, d_act.alloc(F)); FREE_TRY(call, d_ctrl.alloc(1));
  FREE_TRY(call, d_frames.alloc(F * kCalibFrameDoubles)); FREE_TRY(call, d_gram.alloc(F * 2 * N * N));
  FREE_TRY(call, d_share.alloc(F * kCalibShare)); FREE_TRY(call, d_cov.alloc(size_t(K) * size_t(K)));
  FREE_TRY(call, d_fl.zero(P));

  // the start: poses and who takes part
  std::vector<double> q0(F * 4, 0.0), t0(F * 3, 0.0);
  std::vector<uint8_t> status(F, uint8_t(CALICO_RESECT_OK));
  if (q_init) {
    for (size_t f = 0; f < F; ++f) {
      if (offsets[f + 1] - offsets[f] < o.min_points) { status[f] = CALICO_RESECT_TOO_FEW_POINTS; continue; }
      canonical_unit_quat(q_init + 4 * f, quat_norm(q_init + 4 * f), &q0[4 * f]);
      std::copy(t_init + 3 * f, t_init + 3 * f + 3, &t0[3 * f]);
    }
  } else {
    calico_resection_options ro;
    calico_default_resection_options(&ro);
    ro.huber_scale = o.huber_scale; ro.min_points = o.min_points;
    FreeBuf<double> d_k;
    ResectRun run;
    FREE_TRY(call, d_k.upload(k_init, size_t(K))); FREE_TRY(call, run.alloc(F, P, false));
    FREE_TRY(call, run.start(model, ro, d_k.p, F, d_off.p, d_px.p, d_pt.p, d_fl.p, q0.data(), t0.data(), status.data()));
    FREE_TRY(call, d_fl.zero(P));      // (the validity bits start clean)
  }
  std::vector<uint8_t> active(F, 0);
  int64_t usable = 0;
  for (size_t f = 0; f < F; ++f) {
    active[f] = status[f] == CALICO_RESECT_OK ? 1 : 0;
    usable += active[f];
    if (!active[f]) { q0[4 * f] = q0[4 * f + 1] = q0[4 * f + 2] = 0.0; q0[4 * f + 3] = 1.0; t0[3 * f] = t0[3 * f + 1] = t0[3 * f + 2] = 0.0; }
  }
  // the outputs that are the inputs (too few frames, a degenerate problem)
  const auto give_inputs = [&](int calib_status, int iterations, double lambda) {
    std::copy(k_init, k_init + K, k_out);
    std::copy(q0.begin(), q0.end(), q_out); std::copy(t0.begin(), t0.end(), t_out);
    if (q_init)      // (as given, not normalised)
      for (size_t f = 0; f < F; ++f)
        if (active[f]) { std::copy(q_init + 4 * f, q_init + 4 * f + 4, q_out + 4 * f); std::copy(t_init + 3 * f, t_init + 3 * f + 3, t_out + 3 * f); }
    std::fill(rms_out, rms_out + F, 0.0); std::fill(n_used_out, n_used_out + F, 0);
    std::copy(status.begin(), status.end(), status_out);
    if (cov_out) std::fill(cov_out, cov_out + size_t(K) * size_t(K), 0.0);
    *summary = calico_calibration_summary{};
    summary->status = calib_status; summary->iterations = iterations; summary->lambda = lambda;
    summary->frames_used = int32_t(usable);
  };
  if (usable < 3) { give_inputs(CALICO_CALIB_TOO_FEW_FRAMES, 0, kLmLambda0); return CALICO_OK; }

  std::vector<double> frames(F * kCalibFrameDoubles, 0.0);
  for (size_t f = 0; f < F; ++f) {      // the start is the candidate of the first evaluation: slot 1
    double* ns = frames.data() + f * kCalibFrameDoubles + kCalibSlot;
    std::copy(&q0[4 * f], &q0[4 * f] + 4, ns);
    std::copy(&t0[3 * f], &t0[3 * f] + 3, ns + 4);
  }
  CalibControl ctrl = {};
  ctrl.lm.status = CALICO_CALIB_NOT_CONVERGED; ctrl.lm.first = 1; ctrl.lm.lambda = kLmLambda0;
  for (int i = 0; i < K; ++i) ctrl.k[0][i] = ctrl.k[1][i] = k_init[i];
  FREE_TRY(call, d_frames.put(frames.data(), frames.size())); FREE_TRY(call, d_act.put(active.data(), F));
  FREE_TRY(call, d_st.put(status.data(), F)); FREE_TRY(call, d_ctrl.put(&ctrl, 1));
  FREE_TRY(call, d_gram.zero(F * 2 * N * N)); FREE_TRY(call, d_share.zero(F * kCalibShare));

  CalibArgs a = {};
  a.ctrl = d_ctrl.p; a.K = K; a.free_bits = free_bits; a.n_frames = n_frames; a.offsets = d_off.p; a.pixels = d_px.p; a.points = d_pt.p;
  a.flags = d_fl.p; a.active = d_act.p; a.status = d_st.p; a.frames = d_frames.p; a.gram = d_gram.p; a.share = d_share.p;
  a.max_iterations = o.max_iterations; a.step_tolerance = o.step_tolerance; a.huber_scale = o.huber_scale;
  a.q_out = d_q.p; a.t_out = d_t.p; a.rms_out = d_rms.p; a.n_used_out = d_used.p; a.cov_out = d_cov.p;
  const int rc = run_device_lm(call, &d_ctrl.p->lm.done, o.max_iterations, [&] {
    hipError_t e = launch_calib_evaluate(model, a, nullptr);
    if (e == hipSuccess) e = launch_calib_decide(a, nullptr);
    if (e == hipSuccess) e = launch_calib_eliminate(a, false, nullptr);
    return e != hipSuccess ? e : launch_calib_reduce(a, false, nullptr);
  });
  if (rc != CALICO_OK) return rc;
  FREE_TRY(call, d_ctrl.download(&ctrl, 1));
  const LmControl& lm = ctrl.lm;
  if (lm.status != CALICO_CALIB_DEGENERATE) {
    FREE_TRY(call, launch_calib_eliminate(a, true, nullptr)); FREE_TRY(call, launch_calib_reduce(a, true, nullptr));
    FREE_TRY(call, d_ctrl.download(&ctrl, 1));
  }
  if (lm.status == CALICO_CALIB_DEGENERATE || !lm.final_ok) {
    give_inputs(CALICO_CALIB_DEGENERATE, lm.iterations, lm.lambda);
    return CALICO_OK;
  }
  for (int i = 0; i < K; ++i) k_out[i] = ((free_bits >> i) & 1u) ? ctrl.k[lm.cur][i] : k_init[i];
  FREE_TRY(call, d_q.download(q_out, F * 4)); FREE_TRY(call, d_t.download(t_out, F * 3));
  FREE_TRY(call, d_rms.download(rms_out, F)); FREE_TRY(call, d_used.download(n_used_out, F));
  FREE_TRY(call, d_st.download(status_out, F));
  if (cov_out) FREE_TRY(call, d_cov.download(cov_out, size_t(K) * size_t(K)));
  summary->status = lm.status; summary->iterations = lm.iterations; summary->initial_cost = lm.initial_cost;
  summary->final_cost = lm.final_cost; summary->rms = lm.rms; summary->frames_used = lm.frames_used;
  summary->pairs_used = lm.pairs_used; summary->lambda = lm.lambda;
  return CALICO_OK;
}

// max_iterations, step_tolerance, huber_scale, min_points
void calico_default_calibration_options(calico_calibration_options* o) { if (o) *o = {50, 1e-10, 0.0, 4}; }
void calico_default_resection_options(calico_resection_options* o) { if (o) *o = {30, 1e-11, 0.0, 4}; }

int32_t calico_camera_resect(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n_frames,
                             const int64_t* frame_offsets, const double* pixels, const double* points, const double* q_init,
                             const double* t_init, const calico_resection_options* o, double* q_out, double* t_out, double* rms_out,
                             int32_t* n_used_out, int32_t* iterations_out, uint8_t* status_out, double* cov_out) {
  return calico_debug_camera_resect_chunked(device, model, intrinsics, n_intrinsics, n_frames, frame_offsets, pixels, points, q_init, t_init, o,
                                            q_out, t_out, rms_out, n_used_out, iterations_out, status_out, cov_out, kResectChunkPairs);
}

}  // extern "C"
