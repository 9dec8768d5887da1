// accel_align_facade.cpp — Trajectory::AlignAccelerometer (include/calico/calico.hpp) from C++: a trajectory that turns about all
// three axes, an accelerometer mounted at 40 degrees with a lever arm of (0.05, -0.08, 0.03) m and a latency of 13.7 ms, its
// measurements from the facade's own Project(). --host-only: what needs no device (an argument error of the library with its
// message). Otherwise, on the device (Trajectory::FitSpline runs there): too few samples, an option error, the mounting against
// the truth, and the facade's bits against a direct call of calico_accel_align with the same arrays.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "calico/calico.hpp"

using namespace calico;           // NOLINT
using namespace calico::sensors;  // NOLINT

static double max_abs_diff(const Vector3d& a, const Vector3d& b) {
  return std::max(std::fabs(a[0] - b[0]), std::max(std::fabs(a[1] - b[1]), std::fabs(a[2] - b[2])));
}

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && std::strcmp(argv[1], "--host-only") == 0;
  // a trajectory without a spline is an argument error of the library, with its message
  {
    Trajectory empty;
    Accelerometer a;
    auto r = empty.AlignAccelerometer(a);
    CHECK(!r.ok() && r.status().message().find("calico_accel_align: order") != std::string::npos);
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
  const Vector3d lever(0.05, -0.08, 0.03), bias(0.05, -0.03, 0.02);
  std::vector<double> times;
  for (int i = 0; i < 640; ++i) times.push_back(0.3 + 0.01 * i);

  Accelerometer accel_true, accel;
  CHECK(accel_true.SetModel(AccelerometerIntrinsicsModel::kAccelerometerScaleAndBias).ok());
  CHECK(accel.SetModel(AccelerometerIntrinsicsModel::kAccelerometerScaleAndBias).ok());
  CHECK(accel_true.SetIntrinsics({1.0, bias[0], bias[1], bias[2]}).ok());
  accel_true.SetExtrinsics(Pose3d(q_true, lever));
  CHECK(accel_true.SetLatency(latency).ok());
  auto am = accel_true.Project(times, trajectory, world);
  CHECK(am.ok() && am.value().size() == times.size());

  // the start InitializeImu leaves: the gyroscope's rotation (here 1 degree off) and latency (1 ms off), the translation untouched
  const double dh = 0.5 * M_PI / 180.0;
  const Quaterniond q_start = Quaterniond(std::cos(dh), std::sin(dh) * 0.6, -std::sin(dh) * 0.48, std::sin(dh) * 0.64) * q_true;
  accel.SetExtrinsics(Pose3d(q_start, Vector3d(0.0, 0.0, 0.0)));
  CHECK(accel.SetLatency(latency + 1e-3).ok());

  // too few samples: OK, with the status in the summary and the start in the outputs; no device is touched
  {
    std::vector<ImuMeasurement> few(am.value().begin(), am.value().begin() + 10);
    Accelerometer a;
    CHECK(a.SetModel(AccelerometerIntrinsicsModel::kAccelerometerScaleAndBias).ok() && a.AddMeasurements(few).ok());
    CHECK(a.SetLatency(0.002).ok());
    auto r = trajectory.AlignAccelerometer(a, nullptr, true, 1000000);
    CHECK(r.ok() && r.value().summary.status == CALICO_ALIGN_TOO_FEW_SAMPLES && r.value().summary.samples == 10 && !r.value().Ok());
    CHECK(r.value().T_rig_accel.rotation().w() == 1.0 && r.value().latency == 0.002 && r.value().cov.size() == 169);
    calico_accel_alignment_options o;
    calico_default_accel_alignment_options(&o);
    o.estimate_bias = 0;      // (the facade gives no start of lever arm, bias and gravity: all three are estimated)
    auto bad = trajectory.AlignAccelerometer(a, &o);
    CHECK(!bad.ok() && bad.status().message().find("must all be estimated") != std::string::npos);
  }
  // the measurements go in out of order: AlignAccelerometer reads them in time order
  std::vector<ImuMeasurement> shuffled(am.value().rbegin(), am.value().rend());
  CHECK(accel.AddMeasurements(shuffled).ok());
  std::vector<double> as, a;
  accel.SortedMeasurements(&as, &a);
  CHECK(as.size() == times.size() && a.size() == 3 * times.size());
  for (size_t i = 1; i < as.size(); ++i) CHECK(as[i] > as[i - 1]);

  auto res = trajectory.AlignAccelerometer(accel, nullptr, true);
  CHECK(res.ok());
  const Trajectory::AccelerometerAlignment& r = res.value();
  std::printf("status %d (linear %d), %lld samples, %d iterations, latency %.9f, rms %.3e, linear rms %.3e, |g| %.6f\n", r.summary.status,
              r.summary.linear_status, (long long)r.summary.samples, r.summary.iterations, r.latency, r.summary.rms, r.summary.linear_rms,
              r.summary.gravity_norm);
  CHECK(r.Ok() && r.summary.linear_status == CALICO_ALIGN_OK && r.summary.samples == 640);
  // Project() takes the spline segment of the true time, the alignment (as the optimiser) that of the stamp: 13.7 ms past a knot
  // the two polynomials differ, so the data lie outside the model (rms 2.3e-9 m/s^2). On the same data (this trajectory's poses
  // fitted and projected in numpy) the numpy reference comes to within 2.8e-9 of the truth, the largest of its differences in
  // rad, m, m/s^2 and s (test_cpp_accel_align_facade.py measures it): the bound is ten times that.
  const double bound = 10.0 * 2.8e-9;
  const Quaterniond dq = r.T_rig_accel.rotation() * q_true.conjugate();
  const double angle = 2.0 * std::atan2(std::sqrt(dq.x() * dq.x() + dq.y() * dq.y() + dq.z() * dq.z()), std::fabs(dq.w()));
  const double d_lever = max_abs_diff(r.T_rig_accel.translation(), lever), d_bias = max_abs_diff(r.bias, bias);
  const double d_gravity = max_abs_diff(r.gravity_world, world.GetGravity());
  std::printf("rotation off by %.3e rad, lever arm by %.3e m, bias by %.3e, gravity by %.3e, latency by %.3e s\n", angle, d_lever, d_bias,
              d_gravity, r.latency - latency);
  CHECK(angle < bound && d_lever < bound && d_bias < bound && d_gravity < bound && std::fabs(r.latency - latency) < bound);
  CHECK(r.cov.size() == 169 && r.cov[0] > 0.0 && r.cov[168] > 0.0);
  // the sensor is read, not changed
  CHECK(accel.GetLatency() == latency + 1e-3 && accel.GetExtrinsics().translation()[0] == 0.0 && accel.GetExtrinsics().rotation().w() == q_start.w());

  // the same arrays through the C ABI: the same bits
  std::vector<double> ctrl;
  for (const auto& c : trajectory.spline().control_points()) ctrl.insert(ctrl.end(), c.begin(), c.end());
  const double q_init[4] = {q_start.x(), q_start.y(), q_start.z(), q_start.w()}, latency_init = latency + 1e-3;
  double q[4], t[3], b[3], g[3], lat, cov[169];
  calico_accel_alignment_summary sm;
  const BSpline6& sp = trajectory.spline();
  CHECK(calico_accel_align(0, sp.GetSplineOrder(), int(sp.knots().size()), sp.knots().data(), sp.basis_matrices().data(), ctrl.data(),
                           int64_t(as.size()), as.data(), a.data(), q_init, &latency_init, nullptr, nullptr, nullptr, nullptr, q, t, b, g, &lat,
                           cov, &sm) == CALICO_OK);
  const Quaterniond& qr = r.T_rig_accel.rotation();
  CHECK(q[0] == qr.x() && q[1] == qr.y() && q[2] == qr.z() && q[3] == qr.w() && lat == r.latency);
  CHECK(std::memcmp(t, r.T_rig_accel.translation().data(), sizeof(t)) == 0 && std::memcmp(b, r.bias.data(), sizeof(b)) == 0);
  CHECK(std::memcmp(g, r.gravity_world.data(), sizeof(g)) == 0 && std::memcmp(cov, r.cov.data(), sizeof(cov)) == 0);
  CHECK(sm.iterations == r.summary.iterations && sm.rms == r.summary.rms && sm.final_cost == r.summary.final_cost);
  std::printf("OK\n");
  return 0;
}
