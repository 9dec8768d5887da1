// camera.cpp — the camera model over free pixels and points (this part of the C ABI of include/calico_hip.h): unprojection,
// the forward model with its derivatives, and the projection uncertainty map of a solved problem (kernels: camera_kernels.hip).
// Everything that can be checked without a device is checked before the first HIP call. (Calls over chart frames: chart.cpp.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/calico_hip.h"
#include "arg_rules.hpp"
#include "calico_hip_testing.h"
#include "free_call.hpp"
#include "kernels.hpp"
#include "problem_dev.hpp"
#include "problem_host.hpp"

namespace {

using namespace cal;

// pixels or points per pass of a call: upload, kernel, download. A full-resolution map needs no giant allocation
// (2^20 pixels: 16 MB in, 25 MB out).
constexpr int64_t kCameraChunk = int64_t(1) << 20;

// a non-OK status of a call that may have no handle: the message goes to the handle if there is one, else to the thread's slot
int fail(calico_problem* p, const FreeCall& call, int code, const std::string& msg) {
  return p ? p->set_error(code, std::string(call.name) + ": " + msg) : call.fail(code, msg);
}
int check(calico_problem* p, const FreeCall& call, const std::string& error) {
  return error.empty() ? CALICO_OK : fail(p, call, CALICO_INVALID_ARGUMENT, error);
}
int check_camera(calico_problem* p, const FreeCall& call, int sid) {
  if (!p) return call.invalid("null problem handle");
  if (sid < 0 || sid >= int(p->sensors.size())) return fail(p, call, CALICO_INVALID_ARGUMENT, "unknown sensor id");
  if (p->sensors[size_t(sid)].kind != CALICO_SENSOR_CAMERA) return fail(p, call, CALICO_INVALID_ARGUMENT, "the sensor is not a camera");
  return CALICO_OK;
}

}  // namespace

extern "C" {

// calico_camera_unproject with the pixels per pass given (test hook, calico_hip_testing.h)
int32_t calico_debug_camera_unproject_chunked(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n,
                                              const double* pixels, double* bearings, uint8_t* valid, int64_t chunk) {
  const FreeCall call{"calico_camera_unproject"};
  if (int rc = check(nullptr, call, camera_model_error(model, camera_model_num_params(model), intrinsics, n_intrinsics))) return rc;
  if (int rc = check(nullptr, call, count_error(n, pixels && bearings && valid))) return rc;
  if (chunk < 1) return call.invalid("chunk must be >= 1");
  if (n == 0) return CALICO_OK;
  if (int rc = call.select_device(device)) return rc;
  const int64_t cap = std::min(n, chunk);
  FreeBuf<double> d_k, d_px, d_b;
  FreeBuf<uint8_t> d_v;
  FREE_TRY(call, d_k.upload(intrinsics, size_t(n_intrinsics))); FREE_TRY(call, d_px.alloc(size_t(cap) * 2)); FREE_TRY(call, d_b.alloc(size_t(cap) * 3));
  FREE_TRY(call, d_v.alloc(size_t(cap)));
  for (int64_t at = 0; at < n; at += cap) {
    const int64_t m = std::min(cap, n - at);
    FREE_TRY(call, d_px.put(pixels + 2 * at, size_t(m) * 2));
    FREE_TRY(call, launch_camera_unproject(model, d_k.p, m, d_px.p, d_b.p, d_v.p, nullptr));
    FREE_TRY(call, d_b.download(bearings + 3 * at, size_t(m) * 3)); FREE_TRY(call, d_v.download(valid + at, size_t(m)));
  }
  return CALICO_OK;
}

int32_t calico_camera_unproject(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n,
                                const double* pixels, double* bearings_out, uint8_t* valid_out) {
  return calico_debug_camera_unproject_chunked(device, model, intrinsics, n_intrinsics, n, pixels, bearings_out, valid_out, kCameraChunk);
}

int32_t calico_camera_project_points(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n,
                                     const double* points, double* pixels_out, uint8_t* valid_out, double* d_point_out,
                                     double* d_intrinsics_out) {
  const FreeCall call{"calico_camera_project_points"};
  if (int rc = check(nullptr, call, camera_model_error(model, camera_model_num_params(model), intrinsics, n_intrinsics))) return rc;
  if (int rc = check(nullptr, call, count_error(n, points && pixels_out))) return rc;
  if (n == 0) return CALICO_OK;
  if (int rc = call.select_device(device)) return rc;
  const int64_t cap = std::min(n, kCameraChunk);
  const size_t K = size_t(n_intrinsics);
  FreeBuf<double> d_k, d_pt, d_px, d_dp, d_dk;
  FreeBuf<uint8_t> d_v;
  FREE_TRY(call, d_k.upload(intrinsics, K)); FREE_TRY(call, d_pt.alloc(size_t(cap) * 3)); FREE_TRY(call, d_px.alloc(size_t(cap) * 2));
  FREE_TRY(call, d_v.alloc(size_t(cap)));
  if (d_point_out) FREE_TRY(call, d_dp.alloc(size_t(cap) * 6));
  if (d_intrinsics_out) FREE_TRY(call, d_dk.alloc(size_t(cap) * 2 * K));
  for (int64_t at = 0; at < n; at += cap) {
    const int64_t m = std::min(cap, n - at);
    FREE_TRY(call, d_pt.put(points + 3 * at, size_t(m) * 3));
    FREE_TRY(call, launch_camera_project_points(model, d_k.p, m, d_pt.p, d_px.p, d_v.p, d_dp.p, d_dk.p, nullptr));
    FREE_TRY(call, d_px.download(pixels_out + 2 * at, size_t(m) * 2));
    if (valid_out) FREE_TRY(call, d_v.download(valid_out + at, size_t(m)));
    if (d_point_out) FREE_TRY(call, d_dp.download(d_point_out + 6 * at, size_t(m) * 6));
    if (d_intrinsics_out) FREE_TRY(call, d_dk.download(d_intrinsics_out + 2 * int64_t(K) * at, size_t(m) * 2 * K));
  }
  return CALICO_OK;
}

// The unprojection kernel at the intrinsics as they stand in the handle's parameter vector on the device (d_x), on the handle's
// stream: behind whatever a solve left there.
int32_t calico_sensor_unproject(calico_problem* p, int32_t sid, int64_t n, const double* pixels, double* bearings_out, uint8_t* valid_out) {
  const FreeCall call{"calico_sensor_unproject"};
  if (int rc = check_camera(p, call, sid)) return rc;
  if (int rc = check(p, call, count_error(n, pixels && bearings_out && valid_out))) return rc;
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
  const FreeCall call{"calico_projection_uncertainty"};
  if (frame != CALICO_FRAME_CAMERA && frame != CALICO_FRAME_RIG)
    return fail(p, call, CALICO_INVALID_ARGUMENT, "frame must be CALICO_FRAME_CAMERA (0) or CALICO_FRAME_RIG (1)");
  if (!std::isfinite(range) || !(range > 0.0)) return fail(p, call, CALICO_INVALID_ARGUMENT, "range must be finite and > 0");
  if (int rc = check(p, call, count_error(n, pixels && cov_out && valid_out))) return rc;
  if (int rc = check_camera(p, call, sid)) return rc;
  if (n == 0) return CALICO_OK;      // (touches nothing: not even the stored covariance is asked for)
  const calico_problem::Covariance& cv = p->cov;
  if (!cv.valid || p->dirty || cv.blocks.size() != p->blocks.size())
    return fail(p, call, CALICO_FAILED_PRECONDITION, "no covariance of this problem: call calico_covariance_compute (again, if the problem changed) "
                                                     "and check its status");
  const HSensor& hs = p->sensors[size_t(sid)];
  const int K = hs.K, NT = K + 6, dim = cv.dim;
  if (K != camera_model_num_params(hs.model)) return fail(p, call, CALICO_INTERNAL, "the sensor's intrinsics do not match its model");
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
