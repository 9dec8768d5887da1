// camera.cpp — the camera model over free pixels and points (this part of the C ABI of include/calico_hip.h): unprojection,
// the forward model with its derivatives, the projection uncertainty map of a solved problem (kernels: camera_kernels.hip) and
// the chart resection (resect_kernels.hip) and the intrinsic calibration (calib_kernels.hip). Everything that can be checked
// without a device is checked before the first HIP call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/calico_hip.h"
#include "calico_hip_testing.h"
#include "kernels.hpp"
#include "problem_dev.hpp"
#include "problem_host.hpp"

namespace cal {
std::string& handle_free_error() { static thread_local std::string e; return e; }
}  // namespace cal

namespace {

// pixels or points per pass of a call: upload, kernel, download. A full-resolution map needs no giant allocation
// (2^20 pixels: 16 MB in, 25 MB out).
constexpr int64_t kCameraChunk = int64_t(1) << 20;

// a non-OK status of a call that may have no handle: the message goes to the handle if there is one, else to the thread's slot
// (which a later success does not clear, as a handle's message is not)
int fail(calico_problem* p, int code, const std::string& msg) {
  if (p) return p->set_error(code, msg);
  handle_free_error() = msg;
  return code;
}

// The argument rules the four calls share. `what` names the call in the message.
int check_model(calico_problem* p, const char* what, int model, const double* intrinsics, int n_intrinsics) {
  const int K = camera_model_num_params(model);
  if (K < 0) return fail(p, CALICO_INVALID_ARGUMENT, std::string(what) + ": unknown camera model " + std::to_string(model));
  if (n_intrinsics != K)
    return fail(p, CALICO_INVALID_ARGUMENT, std::string(what) + ": camera model " + std::to_string(model) + " has " + std::to_string(K) +
                                                " intrinsics, got " + std::to_string(n_intrinsics));
  if (!intrinsics) return fail(p, CALICO_INVALID_ARGUMENT, std::string(what) + ": null intrinsics");
  return CALICO_OK;
}
int check_count(calico_problem* p, const char* what, int64_t n, bool pointers_ok) {
  if (n < 0) return fail(p, CALICO_INVALID_ARGUMENT, std::string(what) + ": n must be >= 0");
  if (n > 0 && !pointers_ok) return fail(p, CALICO_INVALID_ARGUMENT, std::string(what) + ": null input or output buffer");
  return CALICO_OK;
}
int check_camera(calico_problem* p, const char* what, int sid) {
  if (!p) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": null problem handle");
  if (sid < 0 || sid >= int(p->sensors.size())) return fail(p, CALICO_INVALID_ARGUMENT, std::string(what) + ": unknown sensor id");
  if (p->sensors[size_t(sid)].kind != CALICO_SENSOR_CAMERA) return fail(p, CALICO_INVALID_ARGUMENT, std::string(what) + ": the sensor is not a camera");
  return CALICO_OK;
}

template <class T> struct Buf {      // the handle-free calls' own device memory (as calico_fit_spline's)
  T* p = nullptr;
  ~Buf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(&p), (n ? n : 1) * sizeof(T)); }
};

int hip_fail(const char* what, hipError_t e) { return fail(nullptr, CALICO_INTERNAL, std::string(what) + ": " + hipGetErrorString(e)); }
#define FREE_TRY(what, x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return hip_fail(what, e_); } while (0)

int select_device(const char* what, int device) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count || hipSetDevice(device) != hipSuccess)
    return fail(nullptr, CALICO_INTERNAL, std::string(what) + ": no usable HIP device " + std::to_string(device));
  return CALICO_OK;
}

int unproject_free(int device, int model, const double* intrinsics, int n_intrinsics, int64_t n, const double* pixels, double* bearings,
                   uint8_t* valid, int64_t chunk) {
  const char* what = "calico_camera_unproject";
  if (int rc = check_model(nullptr, what, model, intrinsics, n_intrinsics)) return rc;
  if (int rc = check_count(nullptr, what, n, pixels && bearings && valid)) return rc;
  if (chunk < 1) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": chunk must be >= 1");
  if (n == 0) return CALICO_OK;
  if (int rc = select_device(what, device)) return rc;
  const int64_t cap = std::min(n, chunk);
  Buf<double> d_k, d_px, d_b;
  Buf<uint8_t> d_v;
  FREE_TRY(what, d_k.alloc(size_t(n_intrinsics))); FREE_TRY(what, d_px.alloc(size_t(cap) * 2)); FREE_TRY(what, d_b.alloc(size_t(cap) * 3));
  FREE_TRY(what, d_v.alloc(size_t(cap)));
  FREE_TRY(what, hipMemcpy(d_k.p, intrinsics, size_t(n_intrinsics) * sizeof(double), hipMemcpyHostToDevice));
  for (int64_t at = 0; at < n; at += cap) {
    const int64_t m = std::min(cap, n - at);
    FREE_TRY(what, hipMemcpy(d_px.p, pixels + 2 * at, size_t(m) * 2 * sizeof(double), hipMemcpyHostToDevice));
    FREE_TRY(what, launch_camera_unproject(model, d_k.p, m, d_px.p, d_b.p, d_v.p, nullptr));
    FREE_TRY(what, hipMemcpy(bearings + 3 * at, d_b.p, size_t(m) * 3 * sizeof(double), hipMemcpyDeviceToHost));
    FREE_TRY(what, hipMemcpy(valid + at, d_v.p, size_t(m), hipMemcpyDeviceToHost));
  }
  return CALICO_OK;
}

// pairs per pass of calico_camera_resect: upload, kernel, download (2^20 pairs: 40 MB in, 17 MB of workspace). A frame is never
// split; one with more pairs than this travels alone.
constexpr int64_t kResectChunkPairs = int64_t(1) << 20;

int resect_free(int device, int model, const double* intrinsics, int n_intrinsics, int64_t n_frames, const int64_t* offsets,
                const double* pixels, const double* points, const double* q_init, const double* t_init,
                const calico_resection_options* opt, double* q_out, double* t_out, double* rms_out, int32_t* n_used_out,
                int32_t* iterations_out, uint8_t* status_out, double* cov_out, int64_t chunk_pairs) {
  const char* what = "calico_camera_resect";
  if (int rc = check_model(nullptr, what, model, intrinsics, n_intrinsics)) return rc;
  if (n_frames < 0) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": n_frames must be >= 0");
  calico_resection_options o;
  calico_default_resection_options(&o);
  if (opt) o = *opt;
  if (!std::isfinite(o.step_tolerance) || !(o.step_tolerance > 0.0))
    return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": step_tolerance must be finite and > 0");
  if (o.max_iterations < 1) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": max_iterations must be >= 1");
  if (!std::isfinite(o.huber_scale) || o.huber_scale < 0.0)
    return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": huber_scale must be finite and >= 0");
  if (o.min_points < 4) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": min_points must be >= 4");
  if ((q_init == nullptr) != (t_init == nullptr))
    return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": q_init and t_init are given together or not at all");
  if (chunk_pairs < 1) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": chunk must be >= 1");
  if (n_frames == 0) return CALICO_OK;
  if (!offsets || !q_out || !t_out || !rms_out || !n_used_out || !iterations_out || !status_out)
    return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": null frame offsets or output buffer");
  if (offsets[0] != 0) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": frame_offsets must start at 0");
  for (int64_t f = 0; f < n_frames; ++f)
    if (offsets[f + 1] < offsets[f])
      return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": frame_offsets decrease at frame " + std::to_string(f));
  const int64_t N = offsets[n_frames];
  if (N > 0 && (!pixels || !points)) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": null pixels or points");
  if (int rc = select_device(what, device)) return rc;
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
  Buf<double> d_k, d_px, d_pt, d_ws, d_qi, d_ti, d_q, d_t, d_rms, d_cov;
  Buf<int64_t> d_off;
  Buf<int32_t> d_used, d_it;
  Buf<uint8_t> d_fl, d_st;
  FREE_TRY(what, d_k.alloc(K)); FREE_TRY(what, d_px.alloc(P * 2)); FREE_TRY(what, d_pt.alloc(P * 3)); FREE_TRY(what, d_ws.alloc(P * 2));
  FREE_TRY(what, d_fl.alloc(P)); FREE_TRY(what, d_off.alloc(F + 1));
  if (q_init) { FREE_TRY(what, d_qi.alloc(F * 4)); FREE_TRY(what, d_ti.alloc(F * 3)); }
  FREE_TRY(what, d_q.alloc(F * 4)); FREE_TRY(what, d_t.alloc(F * 3)); FREE_TRY(what, d_rms.alloc(F)); FREE_TRY(what, d_used.alloc(F));
  FREE_TRY(what, d_it.alloc(F)); FREE_TRY(what, d_st.alloc(F));
  if (cov_out) FREE_TRY(what, d_cov.alloc(F * 36));
  FREE_TRY(what, hipMemcpy(d_k.p, intrinsics, K * sizeof(double), hipMemcpyHostToDevice));
  ResectArgs a = {};
  a.k = d_k.p; a.offsets = d_off.p; a.pixels = d_px.p; a.points = d_pt.p; a.ws = d_ws.p; a.flags = d_fl.p;
  a.q_init = q_init ? d_qi.p : nullptr; a.t_init = q_init ? d_ti.p : nullptr;
  a.max_iterations = o.max_iterations; a.step_tolerance = o.step_tolerance; a.huber_scale = o.huber_scale; a.min_points = o.min_points;
  a.q_out = d_q.p; a.t_out = d_t.p; a.rms_out = d_rms.p; a.n_used_out = d_used.p; a.iterations_out = d_it.p; a.status_out = d_st.p;
  a.cov_out = cov_out ? d_cov.p : nullptr;
  std::vector<int64_t> local;
  for (size_t c = 0; c + 1 < cuts.size(); ++c) {
    const int64_t f0 = cuts[c], f1 = cuts[c + 1], nf = f1 - f0, p0 = offsets[f0], np = offsets[f1] - p0;
    local.assign(size_t(nf) + 1, 0);
    for (int64_t f = 0; f <= nf; ++f) local[size_t(f)] = offsets[f0 + f] - p0;
    FREE_TRY(what, hipMemcpy(d_off.p, local.data(), local.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    if (np > 0) {
      FREE_TRY(what, hipMemcpy(d_px.p, pixels + 2 * p0, size_t(np) * 2 * sizeof(double), hipMemcpyHostToDevice));
      FREE_TRY(what, hipMemcpy(d_pt.p, points + 3 * p0, size_t(np) * 3 * sizeof(double), hipMemcpyHostToDevice));
      FREE_TRY(what, hipMemset(d_fl.p, 0, size_t(np)));
    }
    if (q_init) {
      FREE_TRY(what, hipMemcpy(d_qi.p, q_init + 4 * f0, size_t(nf) * 4 * sizeof(double), hipMemcpyHostToDevice));
      FREE_TRY(what, hipMemcpy(d_ti.p, t_init + 3 * f0, size_t(nf) * 3 * sizeof(double), hipMemcpyHostToDevice));
    }
    a.n_frames = nf;
    FREE_TRY(what, launch_camera_resect(model, a, nullptr));
    FREE_TRY(what, hipMemcpy(q_out + 4 * f0, d_q.p, size_t(nf) * 4 * sizeof(double), hipMemcpyDeviceToHost));
    FREE_TRY(what, hipMemcpy(t_out + 3 * f0, d_t.p, size_t(nf) * 3 * sizeof(double), hipMemcpyDeviceToHost));
    FREE_TRY(what, hipMemcpy(rms_out + f0, d_rms.p, size_t(nf) * sizeof(double), hipMemcpyDeviceToHost));
    FREE_TRY(what, hipMemcpy(n_used_out + f0, d_used.p, size_t(nf) * sizeof(int32_t), hipMemcpyDeviceToHost));
    FREE_TRY(what, hipMemcpy(iterations_out + f0, d_it.p, size_t(nf) * sizeof(int32_t), hipMemcpyDeviceToHost));
    FREE_TRY(what, hipMemcpy(status_out + f0, d_st.p, size_t(nf), hipMemcpyDeviceToHost));
    if (cov_out) FREE_TRY(what, hipMemcpy(cov_out + 36 * f0, d_cov.p, size_t(nf) * 36 * sizeof(double), hipMemcpyDeviceToHost));
  }
  return CALICO_OK;
}

// calico_camera_calibrate. The whole batch lives on the device for the length of the call (every iteration reads every pair:
// nothing is chunked). LM cycles -- evaluate, decide, eliminate, reduce -- are enqueued kCalibPollCycles at a time; between the
// groups the host reads the control word's first field, only to stop enqueuing (launches behind the end return at once).
constexpr int kCalibPollCycles = 6;

int calibrate_free(int device, int model, const double* k_init, int n_intrinsics, const uint8_t* free_mask, int64_t n_frames,
                   const int64_t* offsets, const double* pixels, const double* points, const double* q_init, const double* t_init,
                   const calico_calibration_options* opt, double* k_out, double* q_out, double* t_out, double* rms_out,
                   int32_t* n_used_out, uint8_t* status_out, double* cov_out, calico_calibration_summary* summary) {
  const char* what = "calico_camera_calibrate";
  if (int rc = check_model(nullptr, what, model, k_init, n_intrinsics)) return rc;
  if (n_frames < 0) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": n_frames must be >= 0");
  calico_calibration_options o;
  calico_default_calibration_options(&o);
  if (opt) o = *opt;
  if (!std::isfinite(o.step_tolerance) || !(o.step_tolerance > 0.0))
    return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": step_tolerance must be finite and > 0");
  if (o.max_iterations < 1) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": max_iterations must be >= 1");
  if (!std::isfinite(o.huber_scale) || o.huber_scale < 0.0)
    return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": huber_scale must be finite and >= 0");
  if (o.min_points < 4) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": min_points must be >= 4");
  if ((q_init == nullptr) != (t_init == nullptr))
    return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": q_init and t_init are given together or not at all");
  const int K = n_intrinsics;
  unsigned free_bits = 0;
  for (int i = 0; i < K; ++i)
    if (!free_mask || free_mask[i]) free_bits |= 1u << i;
  if (free_bits == 0) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": free_mask leaves no intrinsic free");
  if (n_frames == 0) return CALICO_OK;
  if (!offsets || !k_out || !q_out || !t_out || !rms_out || !n_used_out || !status_out || !summary)
    return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": null frame offsets, output buffer or summary");
  if (offsets[0] != 0) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": frame_offsets must start at 0");
  for (int64_t f = 0; f < n_frames; ++f)
    if (offsets[f + 1] < offsets[f])
      return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": frame_offsets decrease at frame " + std::to_string(f));
  const int64_t NP = offsets[n_frames];
  if (NP > 0 && (!pixels || !points)) return fail(nullptr, CALICO_INVALID_ARGUMENT, std::string(what) + ": null pixels or points");
  if (int rc = select_device(what, device)) return rc;

  const size_t F = size_t(n_frames), P = size_t(NP), N = size_t(K) + 7;
  Buf<double> d_k, d_px, d_pt, d_ws, d_q, d_t, d_rms, d_frames, d_gram, d_share, d_cov;
  Buf<int64_t> d_off;
  Buf<int32_t> d_used, d_it;
  Buf<uint8_t> d_fl, d_st, d_act;
  Buf<CalibControl> d_ctrl;
  FREE_TRY(what, d_k.alloc(size_t(K))); FREE_TRY(what, d_px.alloc(P * 2)); FREE_TRY(what, d_pt.alloc(P * 3)); FREE_TRY(what, d_fl.alloc(P));
  FREE_TRY(what, d_off.alloc(F + 1)); FREE_TRY(what, d_q.alloc(F * 4)); FREE_TRY(what, d_t.alloc(F * 3)); FREE_TRY(what, d_rms.alloc(F));
  FREE_TRY(what, d_used.alloc(F)); FREE_TRY(what, d_st.alloc(F)); FREE_TRY(what, d_act.alloc(F)); FREE_TRY(what, d_ctrl.alloc(1));
  FREE_TRY(what, d_frames.alloc(F * kCalibFrameDoubles)); FREE_TRY(what, d_gram.alloc(F * 2 * N * N));
  FREE_TRY(what, d_share.alloc(F * kCalibShare)); FREE_TRY(what, d_cov.alloc(size_t(K) * size_t(K)));
  FREE_TRY(what, hipMemcpy(d_off.p, offsets, (F + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
  if (NP > 0) {
    FREE_TRY(what, hipMemcpy(d_px.p, pixels, P * 2 * sizeof(double), hipMemcpyHostToDevice));
    FREE_TRY(what, hipMemcpy(d_pt.p, points, P * 3 * sizeof(double), hipMemcpyHostToDevice));
  }
  FREE_TRY(what, hipMemset(d_fl.p, 0, P ? P : 1));

  // the start: poses and who takes part
  std::vector<double> q0(F * 4, 0.0), t0(F * 3, 0.0);
  std::vector<uint8_t> status(F, uint8_t(CALICO_RESECT_OK));
  if (q_init) {
    for (size_t f = 0; f < F; ++f) {
      if (offsets[f + 1] - offsets[f] < o.min_points) { status[f] = CALICO_RESECT_TOO_FEW_POINTS; continue; }
      const double* q = q_init + 4 * f;
      const double nrm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      const double sg = (q[3] < 0.0 ? -1.0 : 1.0) / nrm;
      for (int i = 0; i < 4; ++i) q0[4 * f + size_t(i)] = sg * q[i];
      for (int i = 0; i < 3; ++i) t0[3 * f + size_t(i)] = t_init[3 * f + size_t(i)];
    }
  } else {
    calico_resection_options ro;
    calico_default_resection_options(&ro);
    ro.huber_scale = o.huber_scale; ro.min_points = o.min_points;
    FREE_TRY(what, d_ws.alloc(P * 2)); FREE_TRY(what, d_it.alloc(F));
    FREE_TRY(what, hipMemcpy(d_k.p, k_init, size_t(K) * sizeof(double), hipMemcpyHostToDevice));
    ResectArgs ra = {};
    ra.k = d_k.p; ra.n_frames = n_frames; ra.offsets = d_off.p; ra.pixels = d_px.p; ra.points = d_pt.p; ra.ws = d_ws.p; ra.flags = d_fl.p;
    ra.max_iterations = ro.max_iterations; ra.step_tolerance = ro.step_tolerance; ra.huber_scale = ro.huber_scale; ra.min_points = ro.min_points;
    ra.q_out = d_q.p; ra.t_out = d_t.p; ra.rms_out = d_rms.p; ra.n_used_out = d_used.p; ra.iterations_out = d_it.p; ra.status_out = d_st.p;
    FREE_TRY(what, launch_camera_resect(model, ra, nullptr));
    FREE_TRY(what, hipMemcpy(q0.data(), d_q.p, F * 4 * sizeof(double), hipMemcpyDeviceToHost));
    FREE_TRY(what, hipMemcpy(t0.data(), d_t.p, F * 3 * sizeof(double), hipMemcpyDeviceToHost));
    FREE_TRY(what, hipMemcpy(status.data(), d_st.p, F, hipMemcpyDeviceToHost));
    FREE_TRY(what, hipMemset(d_fl.p, 0, P ? P : 1));      // (the validity bits start clean)
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
  if (usable < 3) { give_inputs(CALICO_CALIB_TOO_FEW_FRAMES, 0, kCalibLambda0); return CALICO_OK; }

  std::vector<double> frames(F * kCalibFrameDoubles, 0.0);
  for (size_t f = 0; f < F; ++f) {      // the start is the candidate of the first evaluation: slot 1
    double* ns = frames.data() + f * kCalibFrameDoubles + kCalibSlot;
    for (int i = 0; i < 4; ++i) ns[i] = q0[4 * f + size_t(i)];
    for (int i = 0; i < 3; ++i) ns[4 + i] = t0[3 * f + size_t(i)];
  }
  CalibControl ctrl = {};
  ctrl.status = CALICO_CALIB_NOT_CONVERGED; ctrl.first = 1; ctrl.lambda = kCalibLambda0;
  for (int i = 0; i < K; ++i) ctrl.k[0][i] = ctrl.k[1][i] = k_init[i];
  FREE_TRY(what, hipMemcpy(d_frames.p, frames.data(), frames.size() * sizeof(double), hipMemcpyHostToDevice));
  FREE_TRY(what, hipMemcpy(d_act.p, active.data(), F, hipMemcpyHostToDevice));
  FREE_TRY(what, hipMemcpy(d_st.p, status.data(), F, hipMemcpyHostToDevice));
  FREE_TRY(what, hipMemcpy(d_ctrl.p, &ctrl, sizeof(ctrl), hipMemcpyHostToDevice));
  FREE_TRY(what, hipMemset(d_gram.p, 0, F * 2 * N * N * sizeof(double)));
  FREE_TRY(what, hipMemset(d_share.p, 0, F * kCalibShare * sizeof(double)));

  CalibArgs a = {};
  a.ctrl = d_ctrl.p; a.K = K; a.free_bits = free_bits; a.n_frames = n_frames; a.offsets = d_off.p; a.pixels = d_px.p; a.points = d_pt.p;
  a.flags = d_fl.p; a.active = d_act.p; a.status = d_st.p; a.frames = d_frames.p; a.gram = d_gram.p; a.share = d_share.p;
  a.max_iterations = o.max_iterations; a.step_tolerance = o.step_tolerance; a.huber_scale = o.huber_scale;
  a.q_out = d_q.p; a.t_out = d_t.p; a.rms_out = d_rms.p; a.n_used_out = d_used.p; a.cov_out = d_cov.p;
  // every cycle tries a step or raises lambda tenfold after a reduced system that was not positive definite (at most 24 times
  // in a row): the loop ends on its own; the bound only guards the host against a control word that never moves
  const int64_t max_cycles = 26 * (int64_t(o.max_iterations) + 2);
  int done = 0;
  for (int64_t cycle = 0; !done; cycle += kCalibPollCycles) {
    if (cycle > max_cycles) return fail(nullptr, CALICO_INTERNAL, std::string(what) + ": the device loop did not end");
    for (int i = 0; i < kCalibPollCycles; ++i) {
      FREE_TRY(what, launch_calib_evaluate(model, a, nullptr));
      FREE_TRY(what, launch_calib_decide(a, nullptr));
      FREE_TRY(what, launch_calib_eliminate(a, false, nullptr));
      FREE_TRY(what, launch_calib_reduce(a, false, nullptr));
    }
    FREE_TRY(what, hipMemcpy(&done, &d_ctrl.p->done, sizeof(int), hipMemcpyDeviceToHost));
  }
  FREE_TRY(what, hipMemcpy(&ctrl, d_ctrl.p, sizeof(ctrl), hipMemcpyDeviceToHost));
  if (ctrl.status != CALICO_CALIB_DEGENERATE) {
    FREE_TRY(what, launch_calib_eliminate(a, true, nullptr));
    FREE_TRY(what, launch_calib_reduce(a, true, nullptr));
    FREE_TRY(what, hipMemcpy(&ctrl, d_ctrl.p, sizeof(ctrl), hipMemcpyDeviceToHost));
  }
  if (ctrl.status == CALICO_CALIB_DEGENERATE || !ctrl.final_ok) {
    give_inputs(CALICO_CALIB_DEGENERATE, ctrl.iterations, ctrl.lambda);
    return CALICO_OK;
  }
  for (int i = 0; i < K; ++i) k_out[i] = ((free_bits >> i) & 1u) ? ctrl.k[ctrl.cur][i] : k_init[i];
  FREE_TRY(what, hipMemcpy(q_out, d_q.p, F * 4 * sizeof(double), hipMemcpyDeviceToHost));
  FREE_TRY(what, hipMemcpy(t_out, d_t.p, F * 3 * sizeof(double), hipMemcpyDeviceToHost));
  FREE_TRY(what, hipMemcpy(rms_out, d_rms.p, F * sizeof(double), hipMemcpyDeviceToHost));
  FREE_TRY(what, hipMemcpy(n_used_out, d_used.p, F * sizeof(int32_t), hipMemcpyDeviceToHost));
  FREE_TRY(what, hipMemcpy(status_out, d_st.p, F, hipMemcpyDeviceToHost));
  if (cov_out) FREE_TRY(what, hipMemcpy(cov_out, d_cov.p, size_t(K) * size_t(K) * sizeof(double), hipMemcpyDeviceToHost));
  summary->status = ctrl.status; summary->iterations = ctrl.iterations; summary->initial_cost = ctrl.initial_cost;
  summary->final_cost = ctrl.final_cost; summary->rms = ctrl.rms; summary->frames_used = ctrl.frames_used;
  summary->pairs_used = ctrl.pairs_used; summary->lambda = ctrl.lambda;
  return CALICO_OK;
}

}  // namespace

extern "C" {

void calico_default_calibration_options(calico_calibration_options* o) {
  if (!o) return;
  o->max_iterations = 50; o->step_tolerance = 1e-10; o->huber_scale = 0.0; o->min_points = 4;
}

int32_t calico_camera_calibrate(int32_t device, int32_t model, const double* intrinsics_init, int32_t n_intrinsics, const uint8_t* free_mask,
                                int64_t n_frames, const int64_t* frame_offsets, const double* pixels, const double* points,
                                const double* q_init, const double* t_init, const calico_calibration_options* o, double* intrinsics_out,
                                double* q_out, double* t_out, double* rms_out, int32_t* n_used_out, uint8_t* status_out,
                                double* intrinsics_cov_out, calico_calibration_summary* summary) {
  return calibrate_free(device, model, intrinsics_init, n_intrinsics, free_mask, n_frames, frame_offsets, pixels, points, q_init, t_init,
                        o, intrinsics_out, q_out, t_out, rms_out, n_used_out, status_out, intrinsics_cov_out, summary);
}

void calico_default_resection_options(calico_resection_options* o) {
  if (!o) return;
  o->max_iterations = 30; o->step_tolerance = 1e-11; o->huber_scale = 0.0; o->min_points = 4;
}

int32_t calico_camera_resect(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n_frames,
                             const int64_t* frame_offsets, const double* pixels, const double* points, const double* q_init,
                             const double* t_init, const calico_resection_options* o, double* q_out, double* t_out, double* rms_out,
                             int32_t* n_used_out, int32_t* iterations_out, uint8_t* status_out, double* cov_out) {
  return resect_free(device, model, intrinsics, n_intrinsics, n_frames, frame_offsets, pixels, points, q_init, t_init, o, q_out, t_out,
                     rms_out, n_used_out, iterations_out, status_out, cov_out, kResectChunkPairs);
}

// test hook (calico_hip_testing.h)
int32_t calico_debug_camera_resect_chunked(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n_frames,
                                           const int64_t* frame_offsets, const double* pixels, const double* points, const double* q_init,
                                           const double* t_init, const calico_resection_options* o, double* q_out, double* t_out,
                                           double* rms_out, int32_t* n_used_out, int32_t* iterations_out, uint8_t* status_out,
                                           double* cov_out, int64_t chunk_pairs) {
  return resect_free(device, model, intrinsics, n_intrinsics, n_frames, frame_offsets, pixels, points, q_init, t_init, o, q_out, t_out,
                     rms_out, n_used_out, iterations_out, status_out, cov_out, chunk_pairs);
}

int32_t calico_camera_unproject(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n,
                                const double* pixels, double* bearings_out, uint8_t* valid_out) {
  return unproject_free(device, model, intrinsics, n_intrinsics, n, pixels, bearings_out, valid_out, kCameraChunk);
}

// test hook (calico_hip_testing.h)
int32_t calico_debug_camera_unproject_chunked(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n,
                                              const double* pixels, double* bearings_out, uint8_t* valid_out, int64_t chunk) {
  return unproject_free(device, model, intrinsics, n_intrinsics, n, pixels, bearings_out, valid_out, chunk);
}

int32_t calico_camera_project_points(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n,
                                     const double* points, double* pixels_out, uint8_t* valid_out, double* d_point_out,
                                     double* d_intrinsics_out) {
  const char* what = "calico_camera_project_points";
  if (int rc = check_model(nullptr, what, model, intrinsics, n_intrinsics)) return rc;
  if (int rc = check_count(nullptr, what, n, points && pixels_out)) return rc;
  if (n == 0) return CALICO_OK;
  if (int rc = select_device(what, device)) return rc;
  const int64_t cap = std::min(n, kCameraChunk);
  const size_t K = size_t(n_intrinsics);
  Buf<double> d_k, d_pt, d_px, d_dp, d_dk;
  Buf<uint8_t> d_v;
  FREE_TRY(what, d_k.alloc(K)); FREE_TRY(what, d_pt.alloc(size_t(cap) * 3)); FREE_TRY(what, d_px.alloc(size_t(cap) * 2));
  FREE_TRY(what, d_v.alloc(size_t(cap)));
  if (d_point_out) FREE_TRY(what, d_dp.alloc(size_t(cap) * 6));
  if (d_intrinsics_out) FREE_TRY(what, d_dk.alloc(size_t(cap) * 2 * K));
  FREE_TRY(what, hipMemcpy(d_k.p, intrinsics, K * sizeof(double), hipMemcpyHostToDevice));
  for (int64_t at = 0; at < n; at += cap) {
    const int64_t m = std::min(cap, n - at);
    FREE_TRY(what, hipMemcpy(d_pt.p, points + 3 * at, size_t(m) * 3 * sizeof(double), hipMemcpyHostToDevice));
    FREE_TRY(what, launch_camera_project_points(model, d_k.p, m, d_pt.p, d_px.p, d_v.p, d_dp.p, d_dk.p, nullptr));
    FREE_TRY(what, hipMemcpy(pixels_out + 2 * at, d_px.p, size_t(m) * 2 * sizeof(double), hipMemcpyDeviceToHost));
    if (valid_out) FREE_TRY(what, hipMemcpy(valid_out + at, d_v.p, size_t(m), hipMemcpyDeviceToHost));
    if (d_point_out) FREE_TRY(what, hipMemcpy(d_point_out + 6 * at, d_dp.p, size_t(m) * 6 * sizeof(double), hipMemcpyDeviceToHost));
    if (d_intrinsics_out)
      FREE_TRY(what, hipMemcpy(d_intrinsics_out + 2 * int64_t(K) * at, d_dk.p, size_t(m) * 2 * K * sizeof(double), hipMemcpyDeviceToHost));
  }
  return CALICO_OK;
}

// The unprojection kernel at the intrinsics as they stand in the handle's parameter vector on the device (d_x), on the handle's
// stream: behind whatever a solve left there.
int32_t calico_sensor_unproject(calico_problem* p, int32_t sid, int64_t n, const double* pixels, double* bearings_out, uint8_t* valid_out) {
  const char* what = "calico_sensor_unproject";
  if (int rc = check_camera(p, what, sid)) return rc;
  if (int rc = check_count(p, what, n, pixels && bearings_out && valid_out)) return rc;
  if (n == 0) return CALICO_OK;
  if (int rc = finalize(p)) return rc;
  HIP_TRY(p, hipSetDevice(p->device));
  if (int rc = upload_x(p)) return rc;
  const HSensor& hs = p->sensors[size_t(sid)];
  const double* k = p->d_x.p + p->blocks[size_t(hs.intr)].amb_off;
  hipStream_t s = p->stream;
  const int64_t cap = std::min(n, kCameraChunk);
  DevBuf<double> d_px, d_b;
  DevBuf<uint8_t> d_v;
  HIP_TRY(p, d_px.alloc(size_t(cap) * 2)); HIP_TRY(p, d_b.alloc(size_t(cap) * 3)); HIP_TRY(p, d_v.alloc(size_t(cap)));
  (void)hipGetLastError();
  for (int64_t at = 0; at < n; at += cap) {
    const int64_t m = std::min(cap, n - at);
    HIP_TRY(p, hipMemcpyAsync(d_px.p, pixels + 2 * at, size_t(m) * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(p, launch_camera_unproject(hs.model, k, m, d_px.p, d_b.p, d_v.p, s));
    HIP_TRY(p, hipMemcpyAsync(bearings_out + 3 * at, d_b.p, size_t(m) * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(p, hipMemcpyAsync(valid_out + at, d_v.p, size_t(m), hipMemcpyDeviceToHost, s));
    HIP_TRY(p, hipStreamSynchronize(s));
  }
  return CALICO_OK;
}

// S_pix = G S_tt G^T per pixel (projection_uncertainty_kernel). S_tt is cut out of the host copy of the border's covariance
// (tangent form) by the block offsets the compute recorded: [intrinsics | q | t] of the camera, zeros for a block that is not
// in the border (constant) and, in the camera frame, for q and t. G is evaluated at the current values in d_x.
int32_t calico_projection_uncertainty(calico_problem* p, int32_t sid, int32_t frame, double range, int64_t n, const double* pixels,
                                      double* cov_out, uint8_t* valid_out) {
  const char* what = "calico_projection_uncertainty";
  if (frame != CALICO_FRAME_CAMERA && frame != CALICO_FRAME_RIG)
    return fail(p, CALICO_INVALID_ARGUMENT, std::string(what) + ": frame must be CALICO_FRAME_CAMERA (0) or CALICO_FRAME_RIG (1)");
  if (!std::isfinite(range) || !(range > 0.0)) return fail(p, CALICO_INVALID_ARGUMENT, std::string(what) + ": range must be finite and > 0");
  if (int rc = check_count(p, what, n, pixels && cov_out && valid_out)) return rc;
  if (int rc = check_camera(p, what, sid)) return rc;
  if (n == 0) return CALICO_OK;      // (touches nothing: not even the stored covariance is asked for)
  const calico_problem::Covariance& cv = p->cov;
  if (!cv.valid || p->dirty || cv.blocks.size() != p->blocks.size())
    return fail(p, CALICO_FAILED_PRECONDITION, std::string(what) + ": no covariance of this problem: call calico_covariance_compute (again, if the "
                                               "problem changed) and check its status");
  const HSensor& hs = p->sensors[size_t(sid)];
  const int K = hs.K, NT = K + 6, dim = cv.dim;
  if (K != camera_model_num_params(hs.model)) return fail(p, CALICO_INTERNAL, std::string(what) + ": the sensor's intrinsics do not match its model");
  // rows of theta in the border (-1: not there)
  std::vector<int> row(size_t(NT), -1);
  const auto place = [&](int block, int at, int size, bool wanted) {
    const calico_problem::BlockSnapshot& B = cv.blocks[size_t(block)];
    if (!wanted || B.off < 0 || B.tsize != size || B.off + size > dim) return;
    for (int j = 0; j < size; ++j) row[size_t(at + j)] = B.off + j;
  };
  place(hs.intr, 0, K, true);
  place(hs.q, K, 3, frame == CALICO_FRAME_RIG);
  place(hs.t, K + 3, 3, frame == CALICO_FRAME_RIG);
  std::vector<double> sig(size_t(NT) * NT, 0.0);
  for (int i = 0; i < NT; ++i)
    for (int j = 0; j < NT; ++j)
      if (row[size_t(i)] >= 0 && row[size_t(j)] >= 0) sig[size_t(i) * NT + j] = cv.sigma[size_t(row[size_t(i)]) * dim + row[size_t(j)]];
  if (int rc = finalize(p)) return rc;
  HIP_TRY(p, hipSetDevice(p->device));
  if (int rc = upload_x(p)) return rc;
  hipStream_t s = p->stream;
  const int64_t cap = std::min(n, kCameraChunk);
  DevBuf<double> d_sig, d_px, d_cov;
  DevBuf<uint8_t> d_v;
  HIP_TRY(p, d_sig.upload(sig, s));
  HIP_TRY(p, d_px.alloc(size_t(cap) * 2)); HIP_TRY(p, d_cov.alloc(size_t(cap) * 3)); HIP_TRY(p, d_v.alloc(size_t(cap)));
  (void)hipGetLastError();
  UncertaintyArgs a = {};
  a.k = p->d_x.p + p->blocks[size_t(hs.intr)].amb_off;
  a.q = p->d_x.p + p->blocks[size_t(hs.q)].amb_off;
  a.sigma = d_sig.p; a.pixels = d_px.p; a.cov = d_cov.p; a.valid = d_v.p; a.range = range; a.frame = frame;
  for (int64_t at = 0; at < n; at += cap) {
    a.n = std::min(cap, n - at);
    HIP_TRY(p, hipMemcpyAsync(d_px.p, pixels + 2 * at, size_t(a.n) * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(p, launch_projection_uncertainty(hs.model, a, s));
    HIP_TRY(p, hipMemcpyAsync(cov_out + 3 * at, d_cov.p, size_t(a.n) * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(p, hipMemcpyAsync(valid_out + at, d_v.p, size_t(a.n), hipMemcpyDeviceToHost, s));
    HIP_TRY(p, hipStreamSynchronize(s));
  }
  return CALICO_OK;
}

}  // extern "C"
