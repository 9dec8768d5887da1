// sensors::CameraModel::UnprojectPixel(s), sensors::Camera::UnprojectPixels and Covariance::ProjectionUncertainty
// (include/calico/calico.hpp) on the toy stereo + IMU rig of toy_stereo_imu.cpp, at the true values: the facade returns the
// numbers of calico_camera_unproject / calico_sensor_unproject / calico_projection_uncertainty, bit for bit, and the library's
// argument errors with their messages.
// Usage: camera_maps_facade [--host-only]      (--host-only: the calls that need no GPU)
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

// test_utils.h:11-116 DefaultSyntheticTest, one axis of it
static std::map<double, Pose3d> toy_trajectory() {
  std::map<double, Pose3d> trajectory;
  const double kDeg2Rad = M_PI / 180.0;
  const Quaterniond q0 = Quaterniond::FromAngleAxis(M_PI, Vector3d(0, 0, 1)) * Quaterniond::FromAngleAxis(M_PI, Vector3d(1, 0, 0));
  const Vector3d t0(0, 0, 1);
  const double ang[5] = {0, 30 * kDeg2Rad, 0, -30 * kDeg2Rad, 0}, pos[5] = {0, 0.5, 0, -0.5, 0};
  const int n = 10;
  const double dti = 1.0 / n, dta = dti * 0.75;
  double interp[10];
  for (int i = 0; i < n; ++i) interp[i] = (std::sin(dti * i * M_PI - M_PI_2) + 1.0) / 2.0;
  double t = 0;
  for (int ax = 0; ax < 3; ++ax) {
    Vector3d axis(ax == 0, ax == 1, ax == 2);
    for (int i = 1; i < 5; ++i) for (int s = 0; s < n; ++s) {
      const double th = (ang[i] - ang[i - 1]) * interp[s] + ang[i - 1];
      trajectory[t] = Pose3d(q0 * Quaterniond::FromAngleAxis(th, axis), t0); t += dta;
    }
    for (int i = 1; i < 5; ++i) for (int s = 0; s < n; ++s) {
      const double p = (pos[i] - pos[i - 1]) * interp[s] + pos[i - 1];
      trajectory[t] = Pose3d(q0, p * axis + t0); t += dta;
    }
  }
  return trajectory;
}

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && !std::strcmp(argv[1], "--host-only");
  using sensors::CameraIntrinsicsModel;
  using sensors::CameraModel;
  const VectorXd cam_k = {785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2};
  std::vector<Vector2d> pixels;
  for (int j = 0; j < 5; ++j) for (int i = 0; i < 7; ++i) pixels.push_back(Vector2d(40.0 + 200.0 * i, 30.0 + 185.0 * j));
  {   // the library's argument errors arrive with their messages, without a device
    const auto bad = CameraModel::UnprojectPixel(CameraIntrinsicsModel::kOpenCv5, VectorXd(7, 0.0), Vector2d(1, 2));
    CHECK(!bad.ok() && bad.status().code() == StatusCode::kInvalidArgument && bad.status().message().find("8 intrinsics") != std::string::npos);
    std::vector<Vector3d> b; std::vector<uint8_t> v;
    CHECK(CameraModel::UnprojectPixels(CameraIntrinsicsModel::kNone, cam_k, pixels, &b, &v).code() == StatusCode::kInvalidArgument);
    CHECK(CameraModel::UnprojectPixels(CameraIntrinsicsModel::kOpenCv5, cam_k, {}, &b, &v).ok() && b.empty() && v.empty());
    sensors::Camera cam;
    CHECK(cam.UnprojectPixels(pixels, &b, &v).code() == StatusCode::kFailedPrecondition);
    Covariance none;
    std::vector<std::array<double, 3>> c;
    CHECK(none.ProjectionUncertainty(0, pixels, 2.0, ProjectionFrame::kRig, &c, &v).code() == StatusCode::kFailedPrecondition);
    CHECK(none.ProjectionUncertainty(cam, pixels, 2.0, ProjectionFrame::kCamera, &c, &v).code() == StatusCode::kFailedPrecondition);
    CHECK(int(ProjectionFrame::kCamera) == CALICO_FRAME_CAMERA && int(ProjectionFrame::kRig) == CALICO_FRAME_RIG);
  }
  if (!host_only) {
    const size_t n = pixels.size();
    std::vector<double> flat(2 * n);
    for (size_t i = 0; i < n; ++i) { flat[2 * i] = pixels[i].x(); flat[2 * i + 1] = pixels[i].y(); }
    {   // the model's inverse against the C ABI, and back through the host's forward model
      std::vector<Vector3d> b; std::vector<uint8_t> v;
      CHECK(CameraModel::UnprojectPixels(CameraIntrinsicsModel::kOpenCv5, cam_k, pixels, &b, &v).ok() && b.size() == n && v.size() == n);
      std::vector<double> b2(3 * n); std::vector<uint8_t> v2(n);
      CHECK(calico_camera_unproject(0, CALICO_CAMERA_OPENCV5, cam_k.data(), 8, int64_t(n), flat.data(), b2.data(), v2.data()) == CALICO_OK);
      size_t n_valid = 0;
      for (size_t i = 0; i < n; ++i) {
        CHECK(v[i] == v2[i] && !std::memcmp(b[i].data(), &b2[3 * i], 3 * sizeof(double)));
        const auto one = CameraModel::UnprojectPixel(CameraIntrinsicsModel::kOpenCv5, cam_k, pixels[i]);
        CHECK(one.ok() == (v[i] != 0));
        if (!v[i]) { CHECK(one.status().code() == StatusCode::kInvalidArgument); continue; }
        ++n_valid;
        CHECK(!std::memcmp(one->data(), b[i].data(), 3 * sizeof(double)));
        double pix[2];
        CHECK(sensors::ProjectPointHost(CameraIntrinsicsModel::kOpenCv5, cam_k.data(), cal::mk(b[i][0], b[i][1], b[i][2]), pix));
        CHECK(std::fabs(pix[0] - pixels[i].x()) < 1e-9 && std::fabs(pix[1] - pixels[i].y()) < 1e-9);
        CHECK(std::fabs(b[i].norm() - 1.0) < 1e-15);
      }
      CHECK(n_valid >= 30);
    }
    const std::map<double, Pose3d> poses = toy_trajectory();
    std::vector<double> stamps;
    for (const auto& kv : poses) stamps.push_back(kv.first);
    Trajectory* trajectory = new Trajectory;
    CHECK(trajectory->FitSpline(poses).ok());
    RigidBody target; target.world_pose_is_constant = true; target.model_definition_is_constant = true;
    for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) target.model_definition[6 * i + j] = Vector3d(i * 0.3 - 0.75, j * 0.3 - 0.75, 0.0);
    WorldModel* world_model = new WorldModel;
    CHECK(world_model->AddRigidBody(&target, /*take_ownership=*/false).ok());
    const VectorXd cam_k = {785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2};
    const VectorXd imu_k = {1.3, 0.01, -0.01, 0.01};
    Pose3d ex_right(Quaterniond(), Vector3d(0.05, -0.02, 0.01)), ex_acc(Quaterniond(), Vector3d(0.01, 0.02, 0.0));
    auto* left = new sensors::Camera; auto* right = new sensors::Camera;
    auto* gyro = new sensors::Gyroscope; auto* acc = new sensors::Accelerometer;
    CHECK(left->SetModel(sensors::CameraIntrinsicsModel::kOpenCv5).ok() && left->SetIntrinsics(cam_k).ok());
    CHECK(right->SetModel(sensors::CameraIntrinsicsModel::kOpenCv5).ok() && right->SetIntrinsics(cam_k).ok());
    right->SetExtrinsics(ex_right);
    CHECK(gyro->SetModel(sensors::GyroscopeIntrinsicsModel::kGyroscopeScaleAndBias).ok() && gyro->SetIntrinsics(imu_k).ok());
    CHECK(acc->SetModel(sensors::AccelerometerIntrinsicsModel::kAccelerometerScaleAndBias).ok() && acc->SetIntrinsics(imu_k).ok());
    acc->SetExtrinsics(ex_acc);
    left->EnableIntrinsicsEstimation(true);
    right->EnableIntrinsicsEstimation(true); right->EnableExtrinsicsEstimation(true);
    gyro->EnableIntrinsicsEstimation(true); gyro->EnableExtrinsicsEstimation(true);
    acc->EnableIntrinsicsEstimation(true); acc->EnableExtrinsicsEstimation(true);
    size_t counts[4] = {0, 0, 0, 0};
    { auto m = left->Project(stamps, *trajectory, *world_model); CHECK(m.ok() && left->AddMeasurements(*m).ok()); counts[0] = m->size(); }
    { auto m = right->Project(stamps, *trajectory, *world_model); CHECK(m.ok() && right->AddMeasurements(*m).ok()); counts[1] = m->size(); }
    { auto m = gyro->Project(stamps, *trajectory, *world_model); CHECK(m.ok() && gyro->AddMeasurements(*m).ok()); counts[2] = m->size(); }
    { auto m = acc->Project(stamps, *trajectory, *world_model); CHECK(m.ok() && acc->AddMeasurements(*m).ok()); counts[3] = m->size(); }
    BatchOptimizer optimizer;
    optimizer.AddSensor(left); optimizer.AddSensor(right); optimizer.AddSensor(gyro); optimizer.AddSensor(acc);
    optimizer.AddWorldModel(world_model); optimizer.AddTrajectory(trajectory);
    auto cov = optimizer.ComputeCovariance(DefaultCovarianceOptions());
    CHECK(cov.ok());
    if (cov.ok()) {
      const sensors::Camera* cams[2] = {left, right};
      for (int ci = 0; ci < 2; ++ci) {
        CHECK(cams[ci]->ProblemSensor() == ci);
        // the camera's own call is the handle's call at the same intrinsics
        std::vector<Vector3d> b; std::vector<uint8_t> v;
        CHECK(cams[ci]->UnprojectPixels(pixels, &b, &v).ok());
        std::vector<double> b2(3 * n); std::vector<uint8_t> v2(n);
        CHECK(calico_sensor_unproject(cov->handle(), ci, int64_t(n), flat.data(), b2.data(), v2.data()) == CALICO_OK);
        for (size_t i = 0; i < n; ++i) CHECK(v[i] == v2[i] && !std::memcmp(b[i].data(), &b2[3 * i], 3 * sizeof(double)));
        for (int frame = 0; frame < 2; ++frame) {
          std::vector<std::array<double, 3>> c; std::vector<uint8_t> cv;
          CHECK(cov->ProjectionUncertainty(*cams[ci], pixels, 2.0, static_cast<ProjectionFrame>(frame), &c, &cv).ok());
          std::vector<double> c2(3 * n); std::vector<uint8_t> cv2(n);
          CHECK(calico_projection_uncertainty(cov->handle(), ci, frame, 2.0, int64_t(n), flat.data(), c2.data(), cv2.data()) == CALICO_OK);
          CHECK(c.size() == n && cv.size() == n);
          double worst = 0.0;
          for (size_t i = 0; i < n; ++i) {
            CHECK(cv[i] == cv2[i] && cv[i] == v[i] && !std::memcmp(c[i].data(), &c2[3 * i], 3 * sizeof(double)));
            if (cv[i]) { CHECK(c[i][0] > 0.0 && c[i][2] > 0.0 && c[i][0] * c[i][2] >= c[i][1] * c[i][1] * (1.0 - 1e-9)); worst = std::fmax(worst, std::fmax(c[i][0], c[i][2])); }
          }
          std::printf("camera %d frame %d: largest pixel variance of the map %.3e px^2\n", ci, frame, worst);
        }
      }
      std::vector<std::array<double, 3>> c; std::vector<uint8_t> cv;
      CHECK(gyro->ProblemSensor() == 2);      // (a gyroscope is no camera: the type says so here, the library through the index)
      const Status not_cam = cov->ProjectionUncertainty(2, pixels, 2.0, ProjectionFrame::kRig, &c, &cv);
      CHECK(not_cam.code() == StatusCode::kInvalidArgument && not_cam.message().find("not a camera") != std::string::npos);
      CHECK(cov->ProjectionUncertainty(7, pixels, 2.0, ProjectionFrame::kRig, &c, &cv).code() == StatusCode::kInvalidArgument);
      const Status neg = cov->ProjectionUncertainty(*left, pixels, -1.0, ProjectionFrame::kRig, &c, &cv);
      CHECK(neg.code() == StatusCode::kInvalidArgument && neg.message().find("range") != std::string::npos);
    }
  }
  std::printf(failures ? "FAILED (%d)\n" : "OK\n", failures);
  return failures ? 1 : 0;
}
