// sensors::CameraModel::ResectChart and sensors::Camera::EstimateChartPoses (include/calico/calico.hpp): the facade returns the
// bits of calico_camera_resect, and the library's argument errors with their messages.
// Usage: resect_facade [--host-only]      (--host-only: the calls that need no GPU)
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

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && !std::strcmp(argv[1], "--host-only");
  using sensors::CameraIntrinsicsModel;
  using sensors::CameraModel;
  const VectorXd kb = {785.0, 640, 400, -1.3e-2, 2.1e-3, -8.0e-4, 1.0e-4};
  // a 6 x 6 chart of 0.3 m pitch, seen from about a metre, in five frames; frame 3 keeps only three of its points
  std::map<int, Vector3d> model;
  for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) model[6 * i + j] = Vector3d(0.3 * i - 0.75, 0.3 * j - 0.75, 0.0);
  std::vector<std::map<int, Vector2d>> frames;
  for (int f = 0; f < 5; ++f) {
    const Quaterniond q = Quaterniond::FromAngleAxis(M_PI, Vector3d(1, 0, 0)) * Quaterniond::FromAngleAxis(0.1 * f - 0.2, Vector3d(0.6, 0.8, 0));
    const Vector3d t(0.05 * f, -0.03 * f, 1.0 + 0.1 * f);
    std::map<int, Vector2d> frame;
    for (const auto& kv : model) {
      if (f == 3 && kv.first >= 3) break;
      const Vector3d p = q * kv.second + t;
      double pix[2] = {0.0, 0.0};
      const cal::V3 pc = cal::mk(p[0], p[1], p[2]);
      CHECK(sensors::ProjectPointHost(CameraIntrinsicsModel::kKannalaBrandt, kb.data(), pc, pix));
      frame[kv.first] = Vector2d(pix[0] + 0.05 * std::sin(7.0 * kv.first + f), pix[1] + 0.05 * std::cos(3.0 * kv.first - f));
    }
    frames.push_back(frame);
  }
  sensors::Camera cam;
  CameraModel::ChartResection r;
  {   // argument errors arrive with their messages, without a device
    CHECK(cam.EstimateChartPoses(frames, model, nullptr, &r).code() == StatusCode::kFailedPrecondition);
    CHECK(cam.SetModel(CameraIntrinsicsModel::kKannalaBrandt).ok() && cam.SetIntrinsics(kb).ok());
    calico_resection_options o;
    calico_default_resection_options(&o);
    CHECK(o.max_iterations == 30 && o.step_tolerance == 1e-11 && o.huber_scale == 0.0 && o.min_points == 4);
    o.min_points = 3;
    const Status bad = cam.EstimateChartPoses(frames, model, &o, &r);
    CHECK(bad.code() == StatusCode::kInvalidArgument && bad.message().find("min_points") != std::string::npos);
    std::map<int, Vector3d> partial = model;
    partial.erase(2);
    CHECK(cam.EstimateChartPoses(frames, partial, nullptr, &r).code() == StatusCode::kInvalidArgument);
    CHECK(CameraModel::ResectChart(CameraIntrinsicsModel::kKannalaBrandt, kb, {0, 2}, {Vector2d(1, 2)}, {Vector3d(0, 0, 0)}, nullptr, &r).code() ==
          StatusCode::kInvalidArgument);
    CHECK(cam.EstimateChartPoses({}, model, nullptr, &r).ok() && r.NumFrames() == 0);
  }
  if (!host_only) {
    CHECK(cam.EstimateChartPoses(frames, model, nullptr, &r, true).ok());
    CHECK(r.NumFrames() == 5);
    // the same arrays through the C ABI
    std::vector<int64_t> off(1, 0);
    std::vector<double> px, pt;
    for (const auto& frame : frames) {
      for (const auto& kv : frame) {
        px.push_back(kv.second.x()); px.push_back(kv.second.y());
        for (int c = 0; c < 3; ++c) pt.push_back(model[kv.first][c]);
      }
      off.push_back(int64_t(px.size() / 2));
    }
    std::vector<double> q(20), t(15), rms(5), cov(180);
    std::vector<int32_t> used(5), its(5);
    std::vector<uint8_t> status(5);
    CHECK(calico_camera_resect(0, 3, kb.data(), 7, 5, off.data(), px.data(), pt.data(), nullptr, nullptr, nullptr, q.data(), t.data(), rms.data(),
                               used.data(), its.data(), status.data(), cov.data()) == CALICO_OK);
    CHECK(!std::memcmp(q.data(), r.q.data(), sizeof(double) * 20) && !std::memcmp(t.data(), r.t.data(), sizeof(double) * 15));
    CHECK(!std::memcmp(rms.data(), r.rms.data(), sizeof(double) * 5) && !std::memcmp(cov.data(), r.cov.data(), sizeof(double) * 180));
    CHECK(used == r.n_used && its == r.iterations && status == r.status);
    for (size_t f = 0; f < 5; ++f) {
      std::printf("frame %zu status %d used %d iterations %d rms %.3e\n", f, int(r.status[f]), r.n_used[f], r.iterations[f], r.rms[f]);
      if (f == 3) { CHECK(r.status[f] == CALICO_RESECT_TOO_FEW_POINTS && !r.Ok(f) && r.q[4 * f + 3] == 1.0 && r.rms[f] == 0.0); continue; }
      CHECK(r.Ok(f) && r.n_used[f] == 36 && r.rms[f] > 0.01 && r.rms[f] < 0.1);
      CHECK(std::fabs(r.t[3 * f + 2] - (1.0 + 0.1 * f)) < 1e-3);      // (the pose the pixels were made at, up to their 0.05 px ripple)
    }
    // a warm start at the result: one small step, the same pose to the step tolerance
    CameraModel::ChartResection w;
    std::vector<int64_t> off1 = {0, 36};
    std::vector<Vector2d> pix1;
    std::vector<Vector3d> pts1;
    for (const auto& kv : frames[0]) { pix1.push_back(kv.second); pts1.push_back(model[kv.first]); }
    const std::vector<double> q0(r.q.begin(), r.q.begin() + 4), t0(r.t.begin(), r.t.begin() + 3);
    CHECK(CameraModel::ResectChart(CameraIntrinsicsModel::kKannalaBrandt, kb, off1, pix1, pts1, nullptr, &w, false, &q0, &t0).ok());
    CHECK(w.Ok(0) && w.cov.empty());
    for (int c = 0; c < 3; ++c) CHECK(std::fabs(w.t[c] - r.t[c]) < 1e-10);
  }
  std::printf(failures ? "FAILED (%d)\n" : "OK\n", failures);
  return failures ? 1 : 0;
}
