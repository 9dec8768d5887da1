// sensors::CameraModel::CalibrateFromChart and sensors::Camera::CalibrateIntrinsics (include/calico/calico.hpp): the facade
// returns the bits of calico_camera_calibrate and sets the camera's intrinsics, and the library's argument errors arrive with
// their messages. Models 1 (OpenCv5) and 4 (DoubleSphere), from the tests' standard start: the truth with f x 1.01, cx + 3,
// cy - 2 and the remaining entries x 0.9, every frame resected there.
// Usage: calib_facade [--host-only]      (--host-only: the calls that need no GPU)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>

#include "calico/calico.hpp"

using namespace calico;

static int failures = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) { std::printf("CHECK FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

using sensors::CameraIntrinsicsModel;
using sensors::CameraModel;

// a 6 x 6 chart of 0.3 m pitch, seen from about a metre under changing tilts, in eight frames
static std::map<int, Vector3d> chart() {
  std::map<int, Vector3d> model;
  for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) model[6 * i + j] = Vector3d(0.3 * i - 0.75, 0.3 * j - 0.75, 0.0);
  return model;
}
static std::vector<std::map<int, Vector2d>> detections(CameraIntrinsicsModel m, const VectorXd& k, const std::map<int, Vector3d>& model) {
  std::vector<std::map<int, Vector2d>> frames;
  for (int f = 0; f < 8; ++f) {
    const Vector3d axis(std::cos(0.8 * f), std::sin(0.8 * f), 0.0);
    const Quaterniond q = Quaterniond::FromAngleAxis(M_PI, Vector3d(1, 0, 0)) * Quaterniond::FromAngleAxis(0.35, axis);
    const Vector3d t(0.08 * std::sin(1.3 * f), 0.06 * std::cos(0.7 * f), 1.0 + 0.04 * f);
    std::map<int, Vector2d> frame;
    for (const auto& kv : model) {
      const Vector3d p = q * kv.second + t;
      double pix[2] = {0.0, 0.0};
      CHECK(sensors::ProjectPointHost(m, k.data(), cal::mk(p[0], p[1], p[2]), pix));
      frame[kv.first] = Vector2d(pix[0] + 0.05 * std::sin(7.0 * kv.first + f), pix[1] + 0.05 * std::cos(3.0 * kv.first - f));
    }
    frames.push_back(frame);
  }
  return frames;
}
static VectorXd standard_start(const VectorXd& k) {
  VectorXd k0 = k;
  for (size_t i = 3; i < k0.size(); ++i) k0[i] = 0.9 * k[i];
  k0[0] = 1.01 * k[0]; k0[1] = k[1] + 3.0; k0[2] = k[2] - 2.0;
  return k0;
}

static void run(CameraIntrinsicsModel m, const VectorXd& truth) {
  const std::map<int, Vector3d> model = chart();
  const auto frames = detections(m, truth, model);
  const VectorXd k0 = standard_start(truth);
  const size_t K = truth.size();
  sensors::Camera cam;
  CHECK(cam.SetModel(m).ok() && cam.SetIntrinsics(k0).ok());
  CameraModel::ChartCalibration r;
  CHECK(cam.CalibrateIntrinsics(frames, model, nullptr, &r, true).ok());
  CHECK(r.Ok() && r.NumFrames() == 8 && r.summary.frames_used == 8 && r.summary.pairs_used == 8 * 36);
  CHECK(r.summary.rms > 0.01 && r.summary.rms < 0.1 && r.summary.final_cost < r.summary.initial_cost);
  std::printf("model %d status %d iterations %d rms %.3e\n", int(m), r.summary.status, r.summary.iterations, r.summary.rms);
  // the camera carries the estimate, close to the truth (the pixels carry a 0.05 px ripple)
  const VectorXd got = cam.GetIntrinsics();
  CHECK(got.size() == K && !std::memcmp(got.data(), r.intrinsics.data(), sizeof(double) * K));
  for (size_t i = 0; i < K; ++i) CHECK(std::fabs(got[i] - truth[i]) <= 2e-2 * std::fmax(1.0, std::fabs(truth[i])));
  for (size_t f = 0; f < 8; ++f) CHECK(r.Used(f) && r.n_used[f] == 36 && std::fabs(r.t[3 * f + 2] - (1.0 + 0.04 * f)) < 2e-2);
  // the same arrays through the C ABI
  std::vector<int64_t> off(1, 0);
  std::vector<double> px, pt;
  for (const auto& frame : frames) {
    for (const auto& kv : frame) {
      px.push_back(kv.second.x()); px.push_back(kv.second.y());
      for (int c = 0; c < 3; ++c) pt.push_back(model.at(kv.first)[c]);
    }
    off.push_back(int64_t(px.size() / 2));
  }
  std::vector<double> k(K), q(32), t(24), rms(8), cov(K * K);
  std::vector<int32_t> used(8);
  std::vector<uint8_t> status(8);
  calico_calibration_summary s;
  CHECK(calico_camera_calibrate(0, int(m), k0.data(), int(K), nullptr, 8, off.data(), px.data(), pt.data(), nullptr, nullptr, nullptr, k.data(),
                                q.data(), t.data(), rms.data(), used.data(), status.data(), cov.data(), &s) == CALICO_OK);
  CHECK(!std::memcmp(k.data(), r.intrinsics.data(), sizeof(double) * K) && !std::memcmp(q.data(), r.q.data(), sizeof(double) * 32));
  CHECK(!std::memcmp(t.data(), r.t.data(), sizeof(double) * 24) && !std::memcmp(rms.data(), r.rms.data(), sizeof(double) * 8));
  CHECK(!std::memcmp(cov.data(), r.cov.data(), sizeof(double) * K * K) && used == r.n_used && status == r.status);
  CHECK(s.status == r.summary.status && s.iterations == r.summary.iterations && s.final_cost == r.summary.final_cost);
  // a constant stays what it was, bit for bit, and the camera keeps its intrinsics when the call fails
  std::vector<uint8_t> mask(K, 1);
  mask[K - 1] = 0;
  CameraModel::ChartCalibration c;
  CHECK(cam.SetIntrinsics(k0).ok() && cam.CalibrateIntrinsics(frames, model, nullptr, &c, true, mask).ok());
  CHECK(c.intrinsics[K - 1] == k0[K - 1] && c.cov[K * K - 1] == 0.0 && c.cov[K - 1] == 0.0);
}

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && !std::strcmp(argv[1], "--host-only");
  const VectorXd opencv5 = {785.0, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2};
  const VectorXd ds = {400.0, 640, 400, -0.2, 0.55};
  {   // argument errors arrive with their messages, without a device
    const std::map<int, Vector3d> model = chart();
    const auto frames = detections(CameraIntrinsicsModel::kOpenCv5, opencv5, model);
    sensors::Camera cam;
    CameraModel::ChartCalibration r;
    CHECK(cam.CalibrateIntrinsics(frames, model, nullptr, &r).code() == StatusCode::kFailedPrecondition);
    CHECK(cam.SetModel(CameraIntrinsicsModel::kOpenCv5).ok() && cam.SetIntrinsics(opencv5).ok());
    calico_calibration_options o;
    calico_default_calibration_options(&o);
    CHECK(o.max_iterations == 50 && o.step_tolerance == 1e-10 && o.huber_scale == 0.0 && o.min_points == 4);
    o.min_points = 3;
    const Status bad = cam.CalibrateIntrinsics(frames, model, &o, &r);
    CHECK(bad.code() == StatusCode::kInvalidArgument && bad.message().find("min_points") != std::string::npos);
    const Status none = cam.CalibrateIntrinsics(frames, model, nullptr, &r, false, std::vector<uint8_t>(8, 0));
    CHECK(none.code() == StatusCode::kInvalidArgument && none.message().find("free_mask") != std::string::npos);
    CHECK(cam.CalibrateIntrinsics(frames, model, nullptr, &r, false, std::vector<uint8_t>(7, 1)).code() == StatusCode::kInvalidArgument);
    std::map<int, Vector3d> partial = model;
    partial.erase(2);
    CHECK(cam.CalibrateIntrinsics(frames, partial, nullptr, &r).code() == StatusCode::kInvalidArgument);
    CHECK(CameraModel::CalibrateFromChart(CameraIntrinsicsModel::kOpenCv5, opencv5, {0, 2}, {Vector2d(1, 2)}, {Vector3d(0, 0, 0)}, nullptr, &r).code() ==
          StatusCode::kInvalidArgument);
    CHECK(cam.CalibrateIntrinsics({}, model, nullptr, &r).ok() && r.NumFrames() == 0);
    const VectorXd kept = cam.GetIntrinsics();
    CHECK(!std::memcmp(kept.data(), opencv5.data(), sizeof(double) * 8));
  }
  if (!host_only) {
    run(CameraIntrinsicsModel::kOpenCv5, opencv5);
    run(CameraIntrinsicsModel::kDoubleSphere, ds);
  }
  std::printf(failures ? "FAILED (%d)\n" : "OK\n", failures);
  return failures ? 1 : 0;
}
