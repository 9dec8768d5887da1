// rig_facade.cpp — calico::CalibrateRig and CameraModel::CalibrateRigFromChart (include/calico/calico.hpp) from C++: an OpenCv5
// and a UnifiedCamera camera on one rig, eight rig frames of a 6 x 6 planar chart, pixels from the facade's own projection.
// --host-only: what needs no device (the facade's own argument errors, an argument error of the library with its message, no
// views at all). Otherwise, on the device: the extrinsics and the frames against the truth, SetExtrinsics on the camera that
// took part and on no other, a run that does not end OK leaves the cameras alone, and the facade's bits against a direct call of
// calico_rig_calibrate with the arrays packed by hand.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "calico/calico.hpp"

using namespace calico;           // NOLINT
using namespace calico::sensors;  // NOLINT

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

namespace {

Pose3d pose_of(double rx, double ry, double rz, double tx, double ty, double tz) {
  const cal::Q4 q = cal::angle_axis_to_quat(cal::mk(rx, ry, rz));
  return Pose3d(Quaterniond(q.w, q.x, q.y, q.z), Vector3d(tx, ty, tz));
}
double distance(const Pose3d& a, const Pose3d& b) {
  const Pose3d d = a * b.inverse();
  const Vector3d t = d.translation();
  const Quaterniond q = d.rotation();
  return std::max(2.0 * std::sqrt(q.x() * q.x() + q.y() * q.y() + q.z() * q.z()), std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]));
}

bool same(const Pose3d& a, const Pose3d& b) {
  const Vector3d ta = a.GetTranslation(), tb = b.GetTranslation();
  return a.GetRotation() == b.GetRotation() && ta[0] == tb[0] && ta[1] == tb[1] && ta[2] == tb[2];
}

}  // namespace

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && std::strcmp(argv[1], "--host-only") == 0;
  Camera cam0, cam1;
  std::map<int, Vector3d> chart;
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) chart[10 * i + j] = Vector3d(0.1 * i - 0.25, 0.1 * j - 0.25, 0.0);
  // a camera without a model, a camera index out of range, a feature the chart does not define
  {
    auto r = CalibrateRig({&cam0, &cam1}, {}, chart);
    CHECK(!r.ok() && r.status().message().find("Camera model has not been set") != std::string::npos);
  }
  CHECK(cam0.SetModel(CameraIntrinsicsModel::kOpenCv5).ok() && cam1.SetModel(CameraIntrinsicsModel::kUnifiedCamera).ok());
  CHECK(cam0.SetIntrinsics({785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2}).ok());
  CHECK(cam1.SetIntrinsics({500, 640, 400, 0.6}).ok());
  const Pose3d before0 = pose_of(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), before1 = pose_of(0.3, 0.0, 0.0, 1.0, 2.0, 3.0);
  cam0.SetExtrinsics(before0);
  cam1.SetExtrinsics(before1);
  const auto untouched = [&] { return same(cam0.GetExtrinsics(), before0) && same(cam1.GetExtrinsics(), before1); };
  {
    auto r = CalibrateRig({&cam0, &cam1}, {{{2, {{0, Vector2d(1.0, 2.0)}}}}}, chart);
    CHECK(!r.ok() && r.status().message().find("names camera 2") != std::string::npos);
    r = CalibrateRig({&cam0, &cam1}, {{{1, {{77, Vector2d(1.0, 2.0)}}}}}, chart);
    CHECK(!r.ok() && r.status().message().find("feature 77 is not in the model definition") != std::string::npos);
    r = CalibrateRig({&cam0, nullptr}, {}, chart);
    CHECK(!r.ok() && r.status().message().find("null camera") != std::string::npos);
  }
  // the library's argument rules reach the caller with their message; no views is OK and changes nothing
  {
    calico_rig_options o;
    calico_default_rig_options(&o);
    o.min_points = 3;
    auto r = CalibrateRig({&cam0, &cam1}, {}, chart, &o);
    CHECK(!r.ok() && r.status().message().find("calico_rig_calibrate: min_points") != std::string::npos);
    RigCalibration out;
    r = CalibrateRig({&cam0, &cam1}, {{}, {}}, chart, nullptr, &out);
    CHECK(r.ok() && r.value().size() == 2 && out.summary.status == CALICO_RIG_TOO_FEW_VIEWS && out.NumViews() == 0 && out.NumCameras() == 2);
    CHECK(out.frame_status[0] == CALICO_RIG_FRAME_NO_VIEW && out.camera_status[1] == CALICO_RIG_CAMERA_UNCONNECTED && untouched());
    RigCalibration raw;
    CHECK(!CameraModel::CalibrateRigFromChart({CameraIntrinsicsModel::kOpenCv5}, {}, 0, {}, {}, {0}, {}, {}, nullptr, &raw).ok());
    CHECK(!CameraModel::CalibrateRigFromChart({CameraIntrinsicsModel::kOpenCv5}, {cam0.GetIntrinsics()}, 0, {0}, {}, {0}, {}, {}, nullptr, &raw).ok());
  }
  if (host_only) { std::printf("OK\n"); return 0; }

  // the truth: camera 1 a hand's breadth to the right, slightly turned; eight rig frames with the chart a metre ahead
  const Pose3d T_rig_cam1 = pose_of(0.02, -0.03, 0.05, 0.12, 0.0, 0.01);
  std::vector<Pose3d> T_rig_chart;
  for (int f = 0; f < 8; ++f)
    T_rig_chart.push_back(pose_of(0.25 * std::sin(1.1 * f), 0.3 * std::cos(0.7 * f), 0.2 * std::sin(0.5 * f + 1.0), 0.05 * std::sin(0.9 * f),
                                  0.04 * std::cos(1.3 * f), 1.0 + 0.05 * f));
  std::vector<std::map<int, std::map<int, Vector2d>>> rig_frames(8);
  const Camera* cams[2] = {&cam0, &cam1};
  for (int f = 0; f < 8; ++f)
    for (int c = 0; c < 2; ++c) {
      if (c == 0 && f == 6) continue;      // (a frame the reference camera did not see)
      const Pose3d T_cam_chart = (c == 0 ? Pose3d(before0) : T_rig_cam1).inverse() * T_rig_chart[size_t(f)];
      for (const auto& [id, p] : chart) {
        const Vector3d pc = T_cam_chart * p;
        double pix[2];
        CHECK(ProjectPointHost(cams[c]->GetModel(), cams[c]->GetIntrinsics().data(), cal::mk(pc[0], pc[1], pc[2]), pix));
        rig_frames[size_t(f)][c][id] = Vector2d(pix[0], pix[1]);
      }
    }
  // a run that does not end OK leaves the cameras alone: one iteration on disturbed pixels (the exact ones converge at once),
  // and a rig whose cameras share fewer frames than asked for
  {
    auto disturbed = rig_frames;
    for (size_t f = 0; f < disturbed.size(); ++f)
      for (auto& [c, detections] : disturbed[f])
        for (auto& [id, pixel] : detections) pixel = Vector2d(pixel.x() + 0.3 * std::sin(1.7 * id + double(f) + c), pixel.y() + 0.3 * std::cos(2.3 * id - double(f)));
    calico_rig_options o;
    calico_default_rig_options(&o);
    o.max_iterations = 1;
    RigCalibration out;
    auto r = CalibrateRig({&cam0, &cam1}, disturbed, chart, &o, &out);
    CHECK(r.ok() && out.summary.status == CALICO_RIG_NOT_CONVERGED);
    CHECK(untouched());
    calico_default_rig_options(&o);
    o.min_shared_frames = 8;      // (the cameras share seven)
    r = CalibrateRig({&cam0, &cam1}, rig_frames, chart, &o, &out);
    CHECK(r.ok() && out.summary.status == CALICO_RIG_TOO_FEW_VIEWS && out.camera_status[1] == CALICO_RIG_CAMERA_UNCONNECTED);
    CHECK(untouched());
  }
  RigCalibration out;
  auto frames = CalibrateRig({&cam0, &cam1}, rig_frames, chart, nullptr, &out, true);
  CHECK(frames.ok() && out.Ok() && out.summary.views_used == 15 && out.summary.pairs_used == 15 * 36 && out.summary.frames_used == 8);
  CHECK(out.camera_status[0] == CALICO_RIG_CAMERA_REFERENCE && out.camera_status[1] == CALICO_RIG_CAMERA_OK && out.cov.size() == 144);
  CHECK(same(cam0.GetExtrinsics(), before0));      // the reference camera keeps what it had
  CHECK(same(cam1.GetExtrinsics(), out.CameraPose(1)) && distance(cam1.GetExtrinsics(), T_rig_cam1) < 1e-9);
  CHECK(frames.value().size() == 8);
  for (size_t f = 0; f < 8; ++f) CHECK(out.frame_status[f] == CALICO_RIG_FRAME_OK && distance(frames.value()[f], T_rig_chart[f]) < 1e-9);
  std::printf("extrinsics within %.3g of the truth, rms %.3g px, %d iterations\n", distance(cam1.GetExtrinsics(), T_rig_cam1), out.summary.rms,
              out.summary.iterations);

  // the same arrays packed by hand, through the C ABI: the facade adds nothing and loses nothing
  std::vector<int32_t> models = {1, 6}, view_camera;
  std::vector<int64_t> koff = {0, 8, 12}, view_frame, view_offsets(1, 0);
  std::vector<double> k = cam0.GetIntrinsics(), px, pt;
  k.insert(k.end(), cam1.GetIntrinsics().begin(), cam1.GetIntrinsics().end());
  for (int f = 0; f < 8; ++f)
    for (const auto& [c, detections] : rig_frames[size_t(f)]) {
      for (const auto& [id, pixel] : detections) {
        px.insert(px.end(), {pixel.x(), pixel.y()});
        pt.insert(pt.end(), {chart[id][0], chart[id][1], chart[id][2]});
      }
      view_camera.push_back(c); view_frame.push_back(f); view_offsets.push_back(int64_t(px.size() / 2));
    }
  RigCalibration d;
  d.q_rig_camera.assign(8, 0.0); d.t_rig_camera.assign(6, 0.0); d.camera_status.assign(2, 0); d.q_frame.assign(32, 0.0); d.t_frame.assign(24, 0.0);
  d.frame_status.assign(8, 0); d.view_rms.assign(15, 0.0); d.view_n_used.assign(15, 0); d.view_status.assign(15, 0); d.cov.assign(144, 0.0);
  CHECK(calico_rig_calibrate(0, 2, models.data(), koff.data(), k.data(), 8, 15, view_camera.data(), view_frame.data(), view_offsets.data(), px.data(),
                             pt.data(), nullptr, nullptr, nullptr, nullptr, nullptr, d.q_rig_camera.data(), d.t_rig_camera.data(),
                             d.camera_status.data(), d.q_frame.data(), d.t_frame.data(), d.frame_status.data(), d.view_rms.data(),
                             d.view_n_used.data(), d.view_status.data(), d.cov.data(), &d.summary) == CALICO_OK);
  CHECK(d.q_rig_camera == out.q_rig_camera && d.t_rig_camera == out.t_rig_camera && d.camera_status == out.camera_status);
  CHECK(d.q_frame == out.q_frame && d.t_frame == out.t_frame && d.frame_status == out.frame_status && d.cov == out.cov);
  CHECK(d.view_rms == out.view_rms && d.view_n_used == out.view_n_used && d.view_status == out.view_status);
  CHECK(std::memcmp(&d.summary, &out.summary, sizeof(d.summary)) == 0);
  std::printf("OK\n");
  return 0;
}
