// calico::Covariance::Predictions (include/calico/calico.hpp) on the toy stereo + IMU rig of toy_stereo_imu.cpp, at the true
// values: the facade returns the numbers of calico_prediction_covariance on its handle, in the order of the sensors'
// residual write-back; without control_points it is FailedPrecondition.
// Usage: prediction_facade [--host-only]      (--host-only: the calls that need no GPU)
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
  {   // a result that was never computed
    Covariance none;
    std::vector<double> c, l; std::vector<uint8_t> v;
    CHECK(none.Predictions(0, true, &c, &l, &v).code() == StatusCode::kFailedPrecondition);
    CHECK(none.NumSensors() == 0 && none.NumObservations(0) == 0 && none.SensorDimension(0) == 0 && none.handle() == nullptr);
    sensors::Camera cam;
    CHECK(cam.ProblemSensor() == -1);
    CHECK(SensorPredictions(none, cam, true, &c, &l, &v).code() == StatusCode::kFailedPrecondition);
    calico_prediction_options o;
    calico_default_prediction_options(&o);
    CHECK(o.apply_loss == 1);
  }
  if (!host_only) {
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
    calico_covariance_options o = DefaultCovarianceOptions();
    {
      auto plain = optimizer.ComputeCovariance(o);
      CHECK(plain.ok());
      std::vector<double> c, l; std::vector<uint8_t> v;
      if (plain.ok()) CHECK(SensorPredictions(*plain, *left, true, &c, &l, &v).code() == StatusCode::kFailedPrecondition);
    }
    o.control_points = 1;
    auto cov = optimizer.ComputeCovariance(o);
    CHECK(cov.ok());
    if (cov.ok()) {
      CHECK(cov->NumSensors() == 4);
      const sensors::SensorCommon* all[4] = {left, right, gyro, acc};
      double total = 0.0;
      for (int si = 0; si < 4; ++si) {
        const int d = si < 2 ? 2 : 3;
        CHECK(all[si]->ProblemSensor() == si && cov->SensorDimension(si) == d);
        const size_t n = size_t(cov->NumObservations(si));
        CHECK(n == counts[si] && n > 0);
        for (int apply_loss = 0; apply_loss < 2; ++apply_loss) {
          std::vector<double> c, l; std::vector<uint8_t> v;
          CHECK(SensorPredictions(*cov, *all[si], apply_loss != 0, &c, &l, &v).ok());
          CHECK(c.size() == n * size_t(d * d) && l.size() == n && v.size() == n);
          // the C ABI on the same handle (the library numbers the sensors in the order they were added)
          std::vector<double> c2(c.size()), l2(n); std::vector<uint8_t> v2(n);
          calico_prediction_options po;
          calico_default_prediction_options(&po);
          po.apply_loss = apply_loss;
          CHECK(calico_prediction_covariance(cov->handle(), si, &po, c2.data(), l2.data(), v2.data()) == CALICO_OK);
          CHECK(c == c2 && l == l2 && v == v2);
          for (size_t i = 0; i < n; ++i) {
            CHECK(v[i] == 1);
            double tr = 0.0;
            for (int a = 0; a < d; ++a) tr += c[i * size_t(d * d) + size_t(a * d + a)];
            CHECK(tr == l[i] && tr >= 0.0 && tr <= double(d) * (1.0 + 1e-9));
          }
          if (apply_loss) for (double x : l) total += x;
        }
      }
      std::vector<double> c;
      CHECK(cov->Predictions(4, true, &c, nullptr, nullptr).code() == StatusCode::kInvalidArgument);
      const int want = 6 * int(trajectory->spline().control_points().size()) + cov->Dimension() - cov->NumUnobserved();
      std::printf("sum of the leverages %.10f, 6 n_cp + Dimension() - NumUnobserved() = %d\n", total, want);
      CHECK(std::fabs(total - want) < 1e-3 * want);      // (the bound proper needs a reference: tests/test_gpu_prediction_covariance.py)
    }
  }
  std::printf(failures ? "FAILED (%d)\n" : "OK\n", failures);
  return failures ? 1 : 0;
}
