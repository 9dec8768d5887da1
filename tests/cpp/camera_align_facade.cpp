// camera_align_facade.cpp — Trajectory::AlignCamera (include/calico/calico.hpp) from C++: a trajectory that turns about all three
// axes, a camera mounted at 12 degrees and 13.7 ms late that sees a small chart, its measurements from the facade's own Project().
// --host-only: what needs no device (an argument error of the library with its message, a body the world model does not have).
// Otherwise, on the device (Trajectory::FitSpline runs there): too few frames, an option error, the estimates against the truth
// within the distance of the two segment polynomials (Project() takes the segment of the true time, the alignment that of the
// stamp), and the facade's bits against a direct call of calico_camera_align with the same arrays.
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

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

// the polynomial of segment seg of the spline at time t (inside its knots or not)
static std::array<double, 6> segment_pose(const BSpline6& sp, int seg, double t) {
  const int k = sp.GetSplineOrder(), ki = sp.GetKnotIndexFromSplineIndex(seg);
  const double u = (t - sp.knots()[size_t(ki)]) / (sp.knots()[size_t(ki) + 1] - sp.knots()[size_t(ki)]);
  std::array<double, 6> out{};
  for (int j = 0; j < k; ++j) {
    double w = 0.0, up = 1.0;
    for (int i = 0; i < k; ++i) { w += up * sp.basis_matrices()[(size_t(seg) * k + i) * k + j]; up *= u; }
    for (int c = 0; c < 6; ++c) out[size_t(c)] += w * sp.control_points()[size_t(seg + j)][size_t(c)];
  }
  return out;
}

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && std::strcmp(argv[1], "--host-only") == 0;
  RigidBody chart;
  chart.id = 0;
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 5; ++j) chart.model_definition[5 * i + j] = Vector3d(0.1 * (i - 2), 0.1 * (j - 2), 0.0);
  chart.T_world_rigidbody = Pose3d(Quaterniond::FromAngleAxis(0.1, Vector3d(0.6, 0.8, 0.0)), Vector3d(0.05, -0.1, 2.2));
  WorldModel world;
  CHECK(world.AddRigidBody(&chart, false).ok());
  Camera cam_true, cam;
  const VectorXd k = {785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2};
  // a trajectory without a spline is an argument error of the library, with its message; so is a body that does not exist
  {
    Trajectory empty;
    Camera none;
    auto r = empty.AlignCamera(none, world);
    CHECK(!r.ok() && r.status().message().find("model has not been set") != std::string::npos);
    CHECK(cam.SetModel(CameraIntrinsicsModel::kOpenCv5).ok() && cam.SetIntrinsics(k).ok());
    r = empty.AlignCamera(cam, world);
    CHECK(!r.ok() && r.status().message().find("calico_camera_align: order") != std::string::npos);
    r = empty.AlignCamera(cam, world, nullptr, 3);
    CHECK(!r.ok() && r.status().message().find("no rigid body with id 3") != std::string::npos);
  }
  if (host_only) { std::printf("OK\n"); return 0; }      // (Trajectory::FitSpline runs on the device)

  std::map<double, Pose3d> poses;
  for (int i = 0; i <= 140; ++i) {
    const double t = 0.05 * i;
    const cal::Q4 q = cal::angle_axis_to_quat(cal::mk(0.2 * std::sin(1.3 * t), 0.15 * std::sin(0.9 * t + 1.0), 0.25 * std::sin(1.7 * t + 2.0)));
    poses[t] = Pose3d(Quaterniond(q.w, q.x, q.y, q.z), Vector3d(0.2 * std::sin(0.7 * t), 0.15 * std::cos(0.5 * t), 0.1 * std::sin(1.1 * t)));
  }
  Trajectory trajectory;
  CHECK(trajectory.FitSpline(poses).ok());
  const double half = 0.5 * 12.0 * M_PI / 180.0, latency = 0.0137;
  const Quaterniond q_true(std::cos(half), 2.0 * std::sin(half) / 3.0, -std::sin(half) / 3.0, 2.0 * std::sin(half) / 3.0);
  const Pose3d mount(q_true, Vector3d(0.08, -0.05, 0.03));
  std::vector<double> times;
  for (int i = 0; i < 128; ++i) times.push_back(0.3 + 0.0517 * i + 0.0071);      // (none of them a stamp of the poses; some 14 ms before a knot)
  CHECK(cam_true.SetModel(CameraIntrinsicsModel::kOpenCv5).ok() && cam_true.SetIntrinsics(k).ok());
  cam_true.SetExtrinsics(mount);
  CHECK(cam_true.SetLatency(latency).ok());
  auto ms = cam_true.Project(times, trajectory, world);
  CHECK(ms.ok() && ms.value().size() == times.size() * 25);

  // too few frames: OK, with the status in the summary and the start in the outputs; no device is touched
  {
    std::vector<CameraMeasurement> few(ms.value().begin(), ms.value().begin() + 5 * 25);
    Camera c;
    CHECK(c.SetModel(CameraIntrinsicsModel::kOpenCv5).ok() && c.SetIntrinsics(k).ok() && c.AddMeasurements(few).ok());
    auto r = trajectory.AlignCamera(c, world, nullptr, 0, true, true, 1000000);
    CHECK(r.ok() && r.value().summary.status == CALICO_ALIGN_TOO_FEW_SAMPLES && r.value().summary.frames_used == 5);
    CHECK(r.value().T_rig_camera.rotation().w() == 1.0 && r.value().latency == 0.0 && r.value().cov.size() == 49 && r.value().curve.empty());
    CHECK(r.value().image_ids.size() == 5 && r.value().image_ids[4] == 4 && r.value().frame_status[0] == CALICO_RESECT_OK);
    calico_camera_alignment_options o;
    calico_default_camera_alignment_options(&o);
    o.sigma_pixel = 0.0;
    auto bad = trajectory.AlignCamera(c, world, &o);
    CHECK(!bad.ok() && bad.status().message().find("sigma_pixel") != std::string::npos);
  }
  // the measurements go in out of order, with one marked as an outlier: AlignCamera reads the others by image, in time order
  std::vector<CameraMeasurement> shuffled(ms.value().rbegin(), ms.value().rend());
  CHECK(cam.AddMeasurements(shuffled).ok() && cam.MarkOutlierById(ms.value()[30].id).ok());
  calico_camera_alignment_options o;
  calico_default_camera_alignment_options(&o);
  o.max_lag = 0.05; o.lag_step = 0.0025;
  auto res = trajectory.AlignCamera(cam, world, &o, 0, true, true);
  CHECK(res.ok());
  const Trajectory::CameraAlignment& r = res.value();
  std::printf("status %d, %lld frames, %lld pairs, %d iterations, latency %.9f, rms %.3e\n", r.summary.status, (long long)r.summary.frames_used,
              (long long)r.summary.pairs_used, r.summary.iterations, r.latency, r.summary.rms);
  CHECK(r.Ok() && r.summary.frames_used == 128 && r.summary.pairs_used == 128 * 25 - 1 && r.frame_n_used[1] == 24);
  for (size_t f = 0; f < r.stamps.size(); ++f) CHECK(r.image_ids[f] == int(f) && r.stamps[f] == times[f] + latency);
  // the distance of the two polynomials where a stamp lies in the segment behind its true time's
  const BSpline6& sp = trajectory.spline();
  double bound = 0.0;
  for (double t : times) {
    const int a = sp.GetSplineIndex(t), b = sp.GetSplineIndex(t + latency);
    if (a == b) continue;
    const auto pa = segment_pose(sp, a, t), pb = segment_pose(sp, b, t);
    for (size_t c = 0; c < 6; ++c) bound = std::max(bound, std::fabs(pa[c] - pb[c]));
  }
  const Quaterniond dq = r.T_rig_camera.rotation() * q_true.conjugate();
  const double angle = 2.0 * std::atan2(std::sqrt(dq.x() * dq.x() + dq.y() * dq.y() + dq.z() * dq.z()), std::fabs(dq.w()));
  const double dt = (r.T_rig_camera.translation() - mount.translation()).norm();
  std::printf("rotation off by %.3e rad, translation by %.3e m, latency by %.3e s; the segment polynomials differ by %.3e\n", angle, dt,
              r.latency - latency, bound);
  CHECK(bound > 0.0 && bound < 1e-6);
  // (a pose error of `bound` in a few frames moves the estimate by less; 1e-10 for the refinement's own tolerance)
  CHECK(angle <= bound + 1e-10 && dt <= bound + 1e-10 && std::fabs(r.latency - latency) <= bound + 1e-10);
  CHECK(r.curve.size() == 41 && r.summary.n_lags == 41 && r.cov.size() == 49 && r.cov[0] > 0.0);
  // the camera is read, not changed
  CHECK(cam.GetLatency() == 0.0 && cam.GetExtrinsics().rotation().w() == 1.0);

  // the same arrays through the C ABI: the same bits
  std::map<int, std::map<int, Vector2d>> frames;
  for (const auto& m : ms.value())
    if (!(m.id == ms.value()[30].id)) frames[m.id.image_id][m.id.feature_id] = m.pixel;
  std::vector<int64_t> offsets(1, 0);
  std::vector<double> px, pt, stamps, ctrl;
  for (const auto& [image, frame] : frames) {
    for (const auto& [feature, pixel] : frame) {
      px.insert(px.end(), {pixel.x(), pixel.y()});
      const Vector3d& p = chart.model_definition.at(feature);
      pt.insert(pt.end(), {p[0], p[1], p[2]});
    }
    stamps.push_back(times[size_t(image)] + latency);
    offsets.push_back(int64_t(px.size() / 2));
  }
  for (const auto& c : sp.control_points()) ctrl.insert(ctrl.end(), c.begin(), c.end());
  double q[4], t[3], lat, cov[49], curve[41];
  std::vector<double> rms(stamps.size());
  std::vector<int32_t> used(stamps.size());
  std::vector<uint8_t> status(stamps.size());
  calico_camera_alignment_summary sm;
  CHECK(calico_camera_align(0, sp.GetSplineOrder(), int(sp.knots().size()), sp.knots().data(), sp.basis_matrices().data(), ctrl.data(), 1, k.data(), 8,
                            chart.T_world_rigidbody.rotation().data(), chart.T_world_rigidbody.translation().data(), int64_t(stamps.size()),
                            stamps.data(), offsets.data(), px.data(), pt.data(), nullptr, nullptr, nullptr, &o, q, t, &lat, rms.data(), used.data(),
                            status.data(), cov, curve, &sm) == CALICO_OK);
  const Quaterniond& qr = r.T_rig_camera.rotation();
  CHECK(q[0] == qr.x() && q[1] == qr.y() && q[2] == qr.z() && q[3] == qr.w() && lat == r.latency);
  CHECK(std::memcmp(t, r.T_rig_camera.translation().data(), sizeof(t)) == 0 && std::memcmp(cov, r.cov.data(), sizeof(cov)) == 0);
  CHECK(std::memcmp(curve, r.curve.data(), sizeof(curve)) == 0 && sm.iterations == r.summary.iterations && sm.rms == r.summary.rms);
  CHECK(rms == r.frame_rms && used == r.frame_n_used && status == r.frame_status);
  std::printf("OK\n");
  return 0;
}
