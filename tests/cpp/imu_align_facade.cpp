// imu_align_facade.cpp — Trajectory::AlignImu (include/calico/calico.hpp) from C++: a trajectory that turns about all three axes,
// a gyroscope and an accelerometer mounted at 40 degrees with a latency of 13.7 ms, their measurements from the facade's own
// Project(). --host-only: what needs no device (an argument error of the library with its message, the measurements in time order).
// Otherwise, on the device (Trajectory::FitSpline runs there): too few samples, an option error, the estimates against the truth,
// and the facade's bits against a direct call of calico_imu_align with the same arrays.
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

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && std::strcmp(argv[1], "--host-only") == 0;
  // a trajectory without a spline is an argument error of the library, with its message
  {
    Trajectory empty;
    Gyroscope g;
    auto r = empty.AlignImu(g);
    CHECK(!r.ok() && r.status().message().find("calico_imu_align: order") != std::string::npos);
  }
  // the measurements are read in time order, whatever order they were added in
  {
    Gyroscope g;
    CHECK(g.SetModel(GyroscopeIntrinsicsModel::kGyroscopeScaleAndBias).ok());
    for (int i = 0; i < 20; ++i) CHECK(g.AddMeasurement({Vector3d(double(19 - i), 0.0, 0.0), {0.01 * (19 - i), i}}).ok());
    std::vector<double> st, v;
    g.SortedMeasurements(&st, &v);
    CHECK(st.size() == 20 && v.size() == 60);
    for (size_t i = 0; i < st.size(); ++i) CHECK(st[i] == 0.01 * double(i) && v[3 * i] == double(i));
  }
  if (host_only) { std::printf("OK\n"); return 0; }      // (Trajectory::FitSpline runs on the device)

  std::map<double, Pose3d> poses;
  for (int i = 0; i <= 140; ++i) {
    const double t = 0.05 * i;
    const cal::Q4 q = cal::angle_axis_to_quat(cal::mk(0.4 * std::sin(1.3 * t), 0.3 * std::sin(0.9 * t + 1.0), 0.5 * std::sin(1.7 * t + 2.0)));
    poses[t] = Pose3d(Quaterniond(q.w, q.x, q.y, q.z), Vector3d(0.3 * std::sin(0.7 * t), 0.2 * std::cos(0.5 * t), 1.0 + 0.1 * std::sin(1.1 * t)));
  }
  Trajectory trajectory;
  CHECK(trajectory.FitSpline(poses).ok());
  WorldModel world;
  world.SetGravity(Vector3d(0.3, -9.7, 0.9));
  const double half = 0.5 * 40.0 * M_PI / 180.0, latency = 0.0137;
  const Quaterniond q_true(std::cos(half), std::sin(half) / 3.0, -2.0 * std::sin(half) / 3.0, 2.0 * std::sin(half) / 3.0);
  const Pose3d mount(q_true, Vector3d(0.0, 0.0, 0.0));
  std::vector<double> times;
  for (int i = 0; i < 640; ++i) times.push_back(0.3 + 0.01 * i);

  Gyroscope gyro_true, gyro;
  Accelerometer accel_true, accel;
  CHECK(gyro_true.SetModel(GyroscopeIntrinsicsModel::kGyroscopeScaleAndBias).ok() && gyro.SetModel(GyroscopeIntrinsicsModel::kGyroscopeScaleAndBias).ok());
  CHECK(accel_true.SetModel(AccelerometerIntrinsicsModel::kAccelerometerScaleAndBias).ok());
  CHECK(accel.SetModel(AccelerometerIntrinsicsModel::kAccelerometerScaleAndBias).ok());
  CHECK(gyro_true.SetIntrinsics({1.0, 0.01, -0.02, 0.015}).ok() && accel_true.SetIntrinsics({1.0, 0.05, -0.03, 0.02}).ok());
  gyro_true.SetExtrinsics(mount); accel_true.SetExtrinsics(mount);
  CHECK(gyro_true.SetLatency(latency).ok() && accel_true.SetLatency(latency).ok());
  auto gm = gyro_true.Project(times, trajectory, world);
  auto am = accel_true.Project(times, trajectory, world);
  CHECK(gm.ok() && am.ok() && gm.value().size() == times.size());

  // too few samples: OK, with the status in the summary and the start in the outputs; no device is touched
  {
    std::vector<ImuMeasurement> few(gm.value().begin(), gm.value().begin() + 10);
    Gyroscope g;
    CHECK(g.SetModel(GyroscopeIntrinsicsModel::kGyroscopeScaleAndBias).ok() && g.AddMeasurements(few).ok());
    auto r = trajectory.AlignImu(g, nullptr, nullptr, true, true, 1000000);
    CHECK(r.ok() && r.value().summary.gyro_status == CALICO_ALIGN_TOO_FEW_SAMPLES && r.value().summary.gyro_samples == 10);
    CHECK(r.value().q_rig_gyro.w() == 1.0 && r.value().latency == 0.0 && r.value().cov.size() == 49 && r.value().curve.empty());
    calico_imu_alignment_options o;
    calico_default_imu_alignment_options(&o);
    o.lag_step = 0.0;
    auto bad = trajectory.AlignImu(g, nullptr, &o);
    CHECK(!bad.ok() && bad.status().message().find("lag_step") != std::string::npos);
  }
  // the measurements go in out of order: AlignImu reads them in time order
  std::vector<ImuMeasurement> shuffled(gm.value().rbegin(), gm.value().rend());
  CHECK(gyro.AddMeasurements(shuffled).ok() && accel.AddMeasurements(am.value()).ok());
  std::vector<double> gs, g;
  gyro.SortedMeasurements(&gs, &g);
  CHECK(gs.size() == times.size() && g.size() == 3 * times.size());
  for (size_t i = 1; i < gs.size(); ++i) CHECK(gs[i] > gs[i - 1]);

  calico_imu_alignment_options o;
  calico_default_imu_alignment_options(&o);
  o.max_lag = 0.05; o.lag_step = 0.0025;
  auto res = trajectory.AlignImu(gyro, &accel, &o, true, true);
  CHECK(res.ok());
  const Trajectory::ImuAlignment& r = res.value();
  std::printf("status %d %d, %lld samples, %d iterations, latency %.9f, gyro rms %.3e, accel rms %.3e, |g| %.6f\n", r.summary.gyro_status,
              r.summary.accel_status, (long long)r.summary.gyro_samples, r.summary.iterations, r.latency, r.summary.gyro_rms, r.summary.accel_rms,
              r.summary.gravity_norm);
  CHECK(r.summary.gyro_status == CALICO_ALIGN_OK && r.summary.accel_status == CALICO_ALIGN_OK && r.summary.gyro_samples == 640);
  // Project() takes the spline segment of the true time, the alignment (as the optimiser) that of the stamp: 13.7 ms past a knot
  // the two polynomials differ by some 1e-10 of the rate, and so do the data and the estimate (measured: 6e-12 rad, 3e-11 s, 2e-10 m/s^2)
  const Quaterniond dq = r.q_rig_gyro * q_true.conjugate();
  const double angle = 2.0 * std::atan2(std::sqrt(dq.x() * dq.x() + dq.y() * dq.y() + dq.z() * dq.z()), std::fabs(dq.w()));
  std::printf("rotation off by %.3e rad, latency by %.3e s, gravity by %.3e\n", angle, r.latency - latency, (r.gravity_world - world.GetGravity()).norm());
  CHECK(angle < 1e-8 && std::fabs(r.latency - latency) < 1e-8);
  CHECK(std::fabs(r.gyro_bias[0] - 0.01) < 1e-8 && std::fabs(r.gyro_bias[1] + 0.02) < 1e-8 && std::fabs(r.gyro_bias[2] - 0.015) < 1e-8);
  CHECK((r.gravity_world - world.GetGravity()).norm() < 1e-7 && std::fabs(r.accel_bias[0] - 0.05) < 1e-7);
  CHECK(r.curve.size() == 41 && r.summary.n_lags == 41 && r.cov.size() == 49 && r.cov[0] > 0.0);
  // the sensors are read, not changed
  CHECK(gyro.GetLatency() == 0.0 && gyro.GetExtrinsics().rotation().w() == 1.0);

  // the same arrays through the C ABI: the same bits
  std::vector<double> as, a, ctrl;
  accel.SortedMeasurements(&as, &a);
  for (const auto& c : trajectory.spline().control_points()) ctrl.insert(ctrl.end(), c.begin(), c.end());
  double q[4], bias[3], lat, grav[3], ab[3], cov[49], curve[41], t_ra[3] = {0, 0, 0};
  calico_imu_alignment_summary sm;
  const BSpline6& sp = trajectory.spline();
  CHECK(calico_imu_align(0, sp.GetSplineOrder(), int(sp.knots().size()), sp.knots().data(), sp.basis_matrices().data(), ctrl.data(),
                         int64_t(gs.size()), gs.data(), g.data(), int64_t(as.size()), as.data(), a.data(), t_ra, nullptr, nullptr, &o, q, bias, &lat,
                         grav, ab, cov, curve, &sm) == CALICO_OK);
  CHECK(q[0] == r.q_rig_gyro.x() && q[1] == r.q_rig_gyro.y() && q[2] == r.q_rig_gyro.z() && q[3] == r.q_rig_gyro.w() && lat == r.latency);
  CHECK(std::memcmp(bias, r.gyro_bias.data(), sizeof(bias)) == 0 && std::memcmp(grav, r.gravity_world.data(), sizeof(grav)) == 0);
  CHECK(std::memcmp(ab, r.accel_bias.data(), sizeof(ab)) == 0 && std::memcmp(cov, r.cov.data(), sizeof(cov)) == 0);
  CHECK(std::memcmp(curve, r.curve.data(), sizeof(curve)) == 0 && sm.iterations == r.summary.iterations && sm.gyro_rms == r.summary.gyro_rms);
  std::printf("OK\n");
  return 0;
}
