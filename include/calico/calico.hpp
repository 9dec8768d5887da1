// calico.hpp — header-only C++ host side above the C ABI of libcalico_hip.so.
//
// Mirrors the reference's own interface for the BatchOptimizer path — same class
// and method names, argument order, enum values and error behaviour — so code
// (and tests) written against yangjames/Calico's C++ API read the same:
//   calico::BatchOptimizer              calico/batch_optimizer.h:23-73
//   calico::sensors::Sensor             calico/sensors/sensor_base.h:22-102
//   calico::sensors::Camera / Gyroscope / Accelerometer   calico/sensors/*.h
//   calico::Trajectory, WorldModel, RigidBody, Landmark, Pose3d
// What differs, because Eigen / abseil / Ceres are not dependencies here:
//   Eigen::VectorXd -> std::vector<double>, Eigen::Vector3d -> calico::Vector3d,
//   absl::Status(Or) -> calico::Status(Or) (absl code numbering),
//   ceres::Problem -> calico::Problem (records blocks by pointer like Ceres and
//   forwards them to the C ABI), ceres::Solver::Options/Summary -> the C structs.
// Link with -lcalico_hip. There is no CPU fallback: Optimize() fails with
// kInternal when no HIP device is usable.
#ifndef CALICO_CALICO_HPP_
#define CALICO_CALICO_HPP_

#include <algorithm>
#include <array>
#include <cmath>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <utility>
#include <vector>

#include "../calico_hip.h"
#include "../../calico_amd/csrc/device_math.hpp"  // sensor models shared with the device code

namespace calico {

// ---------------------------------------------------------------------------
// Status (absl numbering)
// ---------------------------------------------------------------------------
enum class StatusCode : int { kOk = 0, kInvalidArgument = 3, kFailedPrecondition = 9, kUnimplemented = 12, kInternal = 13 };
class Status {
 public:
  Status() = default;
  Status(StatusCode c, std::string m) : code_(c), msg_(std::move(m)) {}
  bool ok() const { return code_ == StatusCode::kOk; }
  StatusCode code() const { return code_; }
  const std::string& message() const { return msg_; }
 private:
  StatusCode code_ = StatusCode::kOk;
  std::string msg_;
};
inline Status OkStatus() { return Status(); }
inline Status InvalidArgumentError(const std::string& m) { return Status(StatusCode::kInvalidArgument, m); }
inline Status FailedPreconditionError(const std::string& m) { return Status(StatusCode::kFailedPrecondition, m); }
inline Status UnimplementedError(const std::string& m) { return Status(StatusCode::kUnimplemented, m); }
inline Status InternalError(const std::string& m) { return Status(StatusCode::kInternal, m); }
template <class T> class StatusOr {
 public:
  StatusOr(const Status& s) : st_(s) {}  // NOLINT
  StatusOr(const T& v) : v_(v) {}        // NOLINT
  StatusOr(T&& v) : v_(std::move(v)) {}  // NOLINT
  bool ok() const { return st_.ok(); }
  const Status& status() const { return st_; }
  T& value() { return *v_; }
  const T& value() const { return *v_; }
  T& operator*() { return *v_; }
  const T& operator*() const { return *v_; }
  T* operator->() { return &*v_; }
  const T* operator->() const { return &*v_; }
 private:
  Status st_;
  std::optional<T> v_;
};

// ---------------------------------------------------------------------------
// Small fixed-size algebra (stand-ins for the Eigen types of typedefs.h)
// ---------------------------------------------------------------------------
using VectorXd = std::vector<double>;
struct Vector2d {
  double v[2] = {0, 0};
  Vector2d() = default;
  Vector2d(double a, double b) : v{a, b} {}
  double& x() { return v[0]; } double& y() { return v[1]; }
  double x() const { return v[0]; } double y() const { return v[1]; }
  double* data() { return v; } const double* data() const { return v; }
};
struct Vector3d {
  double v[3] = {0, 0, 0};
  Vector3d() = default;
  Vector3d(double a, double b, double c) : v{a, b, c} {}
  double& x() { return v[0]; } double& y() { return v[1]; } double& z() { return v[2]; }
  double x() const { return v[0]; } double y() const { return v[1]; } double z() const { return v[2]; }
  double& operator[](int i) { return v[i]; } double operator[](int i) const { return v[i]; }
  double* data() { return v; } const double* data() const { return v; }
  int size() const { return 3; }
  double norm() const { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
};
inline Vector3d operator+(const Vector3d& a, const Vector3d& b) { return Vector3d(a[0] + b[0], a[1] + b[1], a[2] + b[2]); }
inline Vector3d operator-(const Vector3d& a, const Vector3d& b) { return Vector3d(a[0] - b[0], a[1] - b[1], a[2] - b[2]); }
inline Vector3d operator-(const Vector3d& a) { return Vector3d(-a[0], -a[1], -a[2]); }
inline Vector3d operator*(double s, const Vector3d& a) { return Vector3d(s * a[0], s * a[1], s * a[2]); }
inline Vector3d cross(const Vector3d& a, const Vector3d& b) {
  return Vector3d(a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]);
}
// Eigen::Quaterniond: coeffs() storage x,y,z,w; constructor order w,x,y,z.
struct Quaterniond {
  double c[4] = {0, 0, 0, 1};
  Quaterniond() = default;
  Quaterniond(double w, double x, double y, double z) : c{x, y, z, w} {}
  double& x() { return c[0]; } double& y() { return c[1]; } double& z() { return c[2]; } double& w() { return c[3]; }
  double x() const { return c[0]; } double y() const { return c[1]; } double z() const { return c[2]; } double w() const { return c[3]; }
  struct Coeffs { double* p; double* data() { return p; } int size() const { return 4; } };
  Coeffs coeffs() { return Coeffs{c}; }
  const double* data() const { return c; }
  void setIdentity() { c[0] = c[1] = c[2] = 0; c[3] = 1; }
  Quaterniond conjugate() const { return Quaterniond(w(), -x(), -y(), -z()); }
  Quaterniond inverse() const {
    const double n2 = c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3];
    return n2 > 0 ? Quaterniond(w() / n2, -x() / n2, -y() / n2, -z() / n2) : Quaterniond(0, 0, 0, 0);
  }
  Quaterniond operator*(const Quaterniond& b) const {
    return Quaterniond(w() * b.w() - x() * b.x() - y() * b.y() - z() * b.z(), w() * b.x() + x() * b.w() + y() * b.z() - z() * b.y(),
                       w() * b.y() + y() * b.w() + z() * b.x() - x() * b.z(), w() * b.z() + z() * b.w() + x() * b.y() - y() * b.x());
  }
  Vector3d operator*(const Vector3d& v) const {  // Eigen _transformVector
    const Vector3d u(x(), y(), z());
    Vector3d uv = cross(u, v);
    uv = uv + uv;
    return v + w() * uv + cross(u, uv);
  }
  // AngleAxisd(angle, axis) -> quaternion
  static Quaterniond FromAngleAxis(double angle, const Vector3d& axis) {
    const double s = std::sin(0.5 * angle);
    return Quaterniond(std::cos(0.5 * angle), s * axis[0], s * axis[1], s * axis[2]);
  }
};

/// typedefs.h:38-153
class Pose3d {
 public:
  Pose3d() = default;
  Pose3d(const Quaterniond& q, const Vector3d& t) : q_(q), t_(t) {}
  Quaterniond& rotation() { return q_; }
  const Quaterniond& rotation() const { return q_; }
  Vector3d& translation() { return t_; }
  const Vector3d& translation() const { return t_; }
  /// [w, x, y, z], normalised (typedefs.h:69-75)
  void SetRotation(const std::array<double, 4>& q) {
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    q_ = Quaterniond(q[0] / n, q[1] / n, q[2] / n, q[3] / n);
  }
  std::array<double, 4> GetRotation() const { return {q_.w(), q_.x(), q_.y(), q_.z()}; }
  void SetTranslation(const Vector3d& t) { t_ = t; }
  Vector3d GetTranslation() const { return t_; }
  Pose3d operator*(const Pose3d& T_b_a) const { return Pose3d(q_ * T_b_a.q_, q_ * T_b_a.t_ + t_); }
  Vector3d operator*(const Vector3d& p) const { return q_ * p + t_; }
  Pose3d inverse() const { const Quaterniond qi = q_.conjugate(); return Pose3d(qi, -(qi * t_)); }
 private:
  Quaterniond q_;
  Vector3d t_;
};

namespace utils {
/// optimization_utils.h:15-22
enum class LossFunctionType : int { kNone = 0, kHuber = 1, kCauchy = 2 };
}  // namespace utils

using SolverOptions = calico_solver_options;
struct Summary : calico_summary {
  std::string BriefReport() const {
    return "Calico-HIP Solver Report: Iterations: " + std::to_string(num_iterations) + ", Initial cost: " +
           std::to_string(initial_cost) + ", Final cost: " + std::to_string(final_cost) + ", Termination: " +
           (termination_type == CALICO_CONVERGENCE ? "CONVERGENCE" : (termination_type == CALICO_NO_CONVERGENCE ? "NO_CONVERGENCE" : "FAILURE"));
  }
  std::string FullReport() const { return BriefReport() + " (" + message + ")"; }
  bool IsSolutionUsable() const { return termination_type == CALICO_CONVERGENCE || termination_type == CALICO_NO_CONVERGENCE; }
};
/// batch_optimizer.cpp:10-17
inline SolverOptions DefaultSolverOptions() { SolverOptions o; calico_default_solver_options(&o); return o; }

// ---------------------------------------------------------------------------
// Problem: what ceres::Problem is to the reference. Blocks are identified by
// their address (Ceres semantics); Solve() flattens everything through the C
// ABI, runs the device LM and writes the estimates back IN PLACE.
// ---------------------------------------------------------------------------
class Covariance;
class Observability;
namespace sensors { class Camera; }
/// Frame the 3-D point of a projection uncertainty map is fixed in (CALICO_FRAME_*)
enum class ProjectionFrame : int { kCamera = CALICO_FRAME_CAMERA, kRig = CALICO_FRAME_RIG };
class Problem {
 public:
  Problem() = default;
  Problem(const Problem&) = delete;
  Problem& operator=(const Problem&) = delete;
  ~Problem() { if (h_) calico_problem_destroy(h_); }

  void AddParameterBlock(double* values, int size, int manifold = CALICO_MANIFOLD_EUCLIDEAN) {
    if (index_.count(values)) return;
    index_[values] = int(blocks_.size());
    blocks_.push_back({values, size, manifold, false});
  }
  void SetParameterBlockConstant(double* values) { blocks_[size_t(index_.at(values))].constant = true; }
  int NumParameterBlocks() const { return int(blocks_.size()); }
  int NumResidualBlocks() const { int n = 0; for (const auto& s : sensors_) n += int(s.stamps.size()); return n; }
  int NumResiduals() const { int n = 0; for (const auto& s : sensors_) n += int(s.stamps.size()) * (s.kind == CALICO_SENSOR_CAMERA ? 2 : 3); return n; }

  void SetSpline(int order, const std::vector<double>& knots, const std::vector<double>& basis, const std::vector<double*>& ctrl) {
    order_ = order; knots_ = knots; basis_ = basis; ctrl_ = ctrl;
  }
  int AddSensor(int kind, int model, double* intr, double* q, double* t, double* latency, double* gravity, double sigma,
                int loss, double loss_scale) {
    sensors_.push_back({kind, model, intr, q, t, latency, gravity, sigma, loss, loss_scale, {}, {}, {}, {}, {}});
    return int(sensors_.size()) - 1;
  }
  void AddCameraResidual(int sensor, const Vector2d& pixel, double stamp, double* point, double* body_q, double* body_t) {
    SensorRec& s = sensors_[size_t(sensor)];
    s.meas.push_back(pixel.x()); s.meas.push_back(pixel.y()); s.stamps.push_back(stamp);
    s.point.push_back(point); s.body_q.push_back(body_q); s.body_t.push_back(body_t);
  }
  void AddImuResidual(int sensor, const Vector3d& m, double stamp) {
    SensorRec& s = sensors_[size_t(sensor)];
    s.meas.push_back(m[0]); s.meas.push_back(m[1]); s.meas.push_back(m[2]); s.stamps.push_back(stamp);
  }

  /// ceres::Solve(options, &problem, &summary)
  Status Solve(const SolverOptions& options, Summary* summary, int device = 0) {
    if (Status b = Build(device); !b.ok()) return b;
    if (int st = calico_solve(h_, &options, summary)) return Err(st);
    for (size_t i = 0; i < blocks_.size(); ++i)  // in-place update, as Ceres does
      if (int st = calico_get_param_block(h_, ids_[i], blocks_[i].ptr)) return Err(st);
    return OkStatus();
  }
  /// ceres::Covariance::Compute over the problem as it stands (a fresh handle; the values are not changed): see Covariance
  Status ComputeCovariance(const calico_covariance_options& options, Covariance* out, int device = 0);
  /// calico_observability_compute over the problem as it stands (a fresh handle; the values are not changed): see Observability
  Status AnalyzeObservability(const calico_observability_options& options, Observability* out, int device = 0);
  /// problem.EvaluateResidualBlock(id, /*apply_loss_function=*/false, ...) for every block of a sensor.
  Status EvaluateResiduals(int sensor, std::vector<double>* out, std::vector<uint8_t>* valid) {
    if (!h_) return FailedPreconditionError("problem has not been solved");
    const SensorRec& s = sensors_[size_t(sensor)];
    const size_t n = s.stamps.size();
    out->assign(n * (s.kind == CALICO_SENSOR_CAMERA ? 2 : 3), 0.0); valid->assign(n, 0);
    const int st = calico_get_residuals(h_, sensor_ids_[size_t(sensor)], out->data(), valid->data());
    return st == CALICO_OK ? OkStatus() : Err(st);
  }
  calico_problem* handle() { return h_; }

 private:
  // a new handle with every block, the spline, the sensors and their residuals
  Status Build(int device) {
    if (h_) { calico_problem_destroy(h_); h_ = nullptr; }
    if (calico_problem_create(&h_, device) != CALICO_OK) return InternalError("calico_problem_create failed: no usable HIP device");
    ids_.assign(blocks_.size(), -1);
    for (size_t i = 0; i < blocks_.size(); ++i) {
      const BlockRec& b = blocks_[i];
      if (int st = calico_problem_add_param_block(h_, b.ptr, b.size, b.manifold, b.constant ? 1 : 0, &ids_[i])) return Err(st);
    }
    std::vector<int32_t> ctrl_ids;
    for (double* p : ctrl_) ctrl_ids.push_back(ids_[size_t(index_.at(p))]);
    if (int st = calico_problem_set_spline(h_, order_, int(knots_.size()), knots_.data(), basis_.data(), ctrl_ids.data())) return Err(st);
    std::map<std::pair<double*, double*>, int> bodies;
    sensor_ids_.clear();
    for (SensorRec& s : sensors_) {
      int sid = -1;
      if (int st = calico_problem_add_sensor(h_, s.kind, s.model, Id(s.intr), Id(s.q), Id(s.t), Id(s.latency),
                                             s.gravity ? Id(s.gravity) : -1, s.sigma, s.loss, s.loss_scale, &sid)) return Err(st);
      sensor_ids_.push_back(sid);
      const int64_t n = int64_t(s.stamps.size());
      if (s.kind == CALICO_SENSOR_CAMERA) {
        std::vector<int32_t> body(static_cast<size_t>(n)), point(static_cast<size_t>(n));
        for (int64_t i = 0; i < n; ++i) {
          const auto key = std::make_pair(s.body_q[size_t(i)], s.body_t[size_t(i)]);
          auto it = bodies.find(key);
          if (it == bodies.end()) {
            int bid = -1;
            if (int st = calico_problem_add_rigid_body(h_, Id(key.first), Id(key.second), &bid)) return Err(st);
            it = bodies.emplace(key, bid).first;
          }
          body[size_t(i)] = it->second; point[size_t(i)] = Id(s.point[size_t(i)]);
        }
        if (int st = calico_problem_add_camera_residuals(h_, sid, n, s.meas.data(), s.stamps.data(), body.data(), point.data())) return Err(st);
      } else {
        if (int st = calico_problem_add_imu_residuals(h_, sid, n, s.meas.data(), s.stamps.data())) return Err(st);
      }
    }
    return OkStatus();
  }
  struct BlockRec { double* ptr; int size; int manifold; bool constant; };
  struct SensorRec {
    int kind, model; double *intr, *q, *t, *latency, *gravity; double sigma; int loss; double loss_scale;
    std::vector<double> meas, stamps; std::vector<double*> point, body_q, body_t;
  };
  int Id(double* p) const { return ids_[size_t(index_.at(p))]; }
  Status Err(int st) const { return Status(static_cast<StatusCode>(st), calico_last_error(h_)); }
  std::vector<BlockRec> blocks_;
  std::unordered_map<double*, int> index_;
  std::vector<int32_t> ids_;
  std::vector<SensorRec> sensors_;
  std::vector<int> sensor_ids_;
  int order_ = 0;
  std::vector<double> knots_, basis_;
  std::vector<double*> ctrl_;
  calico_problem* h_ = nullptr;
};

/// ceres::Covariance's result (calico_covariance_* in include/calico_hip.h for the semantics): blocks keyed by the parameter
/// pointers the Problem was given. It keeps the library handle it was computed on (and its device buffers) until destroyed.
class Covariance {
 public:
  /// GetCovarianceBlock: ambient form (a quaternion block lifted as P Σ Pᵀ), row-major size_a x size_b
  bool GetCovarianceBlock(const double* a, const double* b, double* out) const { return Get(a, b, 0, out).ok(); }
  /// GetCovarianceBlockInTangentSpace: 3 rows / columns per quaternion block
  bool GetCovarianceBlockInTangentSpace(const double* a, const double* b, double* out) const { return Get(a, b, 1, out).ok(); }
  /// the same, with the library's status (control points: after a compute with control_points = 1, with border blocks and
  /// with control points less than the spline order apart, else UNIMPLEMENTED; INVALID_ARGUMENT for an unknown pointer)
  Status Get(const double* a, const double* b, int tangent, double* out) const {
    if (!h_) return FailedPreconditionError("covariance has not been computed");
    const auto ia = ids_.find(a), ib = ids_.find(b);
    if (ia == ids_.end() || ib == ids_.end()) return InvalidArgumentError("covariance: parameter block not in the problem");
    const int st = calico_covariance_get_block(h_.get(), ia->second, ib->second, tangent, out);
    return st == CALICO_OK ? OkStatus() : Status(static_cast<StatusCode>(st), calico_last_error(h_.get()));
  }
  int Dimension() const { int32_t d = 0; if (h_) calico_covariance_info(h_.get(), &d, nullptr, nullptr); return d; }
  int NumUnobserved() const { int32_t n = 0; if (h_) calico_covariance_info(h_.get(), nullptr, &n, nullptr); return n; }
  double MinRelativePivot() const { double v = 0.0; if (h_) calico_covariance_info(h_.get(), nullptr, nullptr, &v); return v; }
  /// 6 x 6 block of control points i and j (by their index in the spline), row-major (control_points = 1)
  Status ControlPoints(int i, int j, double* out) const {
    if (!h_) return FailedPreconditionError("covariance has not been computed");
    if (i < 0 || j < 0 || size_t(i) >= ctrl_ids_.size() || size_t(j) >= ctrl_ids_.size())
      return InvalidArgumentError("covariance: control point index out of range");
    const int st = calico_covariance_get_block(h_.get(), ctrl_ids_[size_t(i)], ctrl_ids_[size_t(j)], 1, out);
    return st == CALICO_OK ? OkStatus() : Status(static_cast<StatusCode>(st), calico_last_error(h_.get()));
  }
  /// Covariance of the spline's 6-vector at each stamp (calico_covariance_trajectory): stamps.size() row-major 6 x 6 blocks
  Status TrajectoryCovariance(const std::vector<double>& stamps, std::vector<double>* out) const {
    if (!h_) return FailedPreconditionError("covariance has not been computed");
    out->assign(stamps.size() * 36, 0.0);
    const int st = calico_covariance_trajectory(h_.get(), int64_t(stamps.size()), stamps.data(), out->data());
    return st == CALICO_OK ? OkStatus() : Status(static_cast<StatusCode>(st), calico_last_error(h_.get()));
  }
  /// Prediction covariance and leverage of every residual block of a sensor (calico_prediction_covariance; control_points =
  /// 1): `sensor` is the index Problem::AddSensor returned (sensors::SensorCommon::ProblemSensor() for a sensor of the
  /// optimizer the covariance came from; SensorPredictions below). cov: n row-major d x d blocks, leverage: n traces, valid:
  /// n flags, in the order the residuals were added -- the order and selection of the facade's residual write-back.
  calico_problem* handle() const { return h_.get(); }      // the library handle the result lives on (C ABI readers)
  int NumSensors() const { return int(sensor_ids_.size()); }
  int SensorDimension(int sensor) const { return sensor >= 0 && sensor < NumSensors() ? sensor_dim_[size_t(sensor)] : 0; }
  int64_t NumObservations(int sensor) const { return sensor >= 0 && sensor < NumSensors() ? sensor_n_[size_t(sensor)] : 0; }
  Status Predictions(int sensor, bool apply_loss, std::vector<double>* cov, std::vector<double>* leverage,
                     std::vector<uint8_t>* valid) const {
    if (!h_) return FailedPreconditionError("covariance has not been computed");
    if (sensor < 0 || sensor >= NumSensors()) return InvalidArgumentError("covariance: sensor not in the problem");
    const size_t n = size_t(sensor_n_[size_t(sensor)]), d = size_t(sensor_dim_[size_t(sensor)]);
    std::vector<double> c(n * d * d, 0.0), l(n, 0.0);
    std::vector<uint8_t> v(n, 0);
    calico_prediction_options o;
    calico_default_prediction_options(&o);
    o.apply_loss = apply_loss ? 1 : 0;
    const int st = calico_prediction_covariance(h_.get(), sensor_ids_[size_t(sensor)], &o, c.data(), l.data(), v.data());
    if (st != CALICO_OK) return Status(static_cast<StatusCode>(st), calico_last_error(h_.get()));
    if (cov) cov->swap(c);
    if (leverage) leverage->swap(l);
    if (valid) valid->swap(v);
    return OkStatus();
  }
  /// Projection uncertainty map of a camera (calico_projection_uncertainty): for every pixel [s_uu, s_uv, s_vv] (pixels^2) of
  /// the projection of a point `range` metres along the pixel's ray, fixed in the camera frame (intrinsics only) or in the
  /// sensor-rig frame (intrinsics and extrinsics); valid = 0 with zeros where the pixel does not unproject. `sensor` as for
  /// Predictions; the overload below takes a camera of the optimizer the covariance came from.
  Status ProjectionUncertainty(int sensor, const std::vector<Vector2d>& pixels, double range, ProjectionFrame frame,
                               std::vector<std::array<double, 3>>* cov, std::vector<uint8_t>* valid) const {
    if (!h_) return FailedPreconditionError("covariance has not been computed");
    if (sensor < 0 || sensor >= NumSensors()) return InvalidArgumentError("covariance: sensor not in the problem");
    const size_t n = pixels.size();
    std::vector<double> px(2 * n);
    for (size_t i = 0; i < n; ++i) { px[2 * i] = pixels[i].x(); px[2 * i + 1] = pixels[i].y(); }
    std::vector<std::array<double, 3>> c(n);
    std::vector<uint8_t> v(n, 0);
    const int st = calico_projection_uncertainty(h_.get(), sensor_ids_[size_t(sensor)], int(frame), range, int64_t(n), px.data(),
                                                 n ? c[0].data() : nullptr, v.data());
    if (st != CALICO_OK) return Status(static_cast<StatusCode>(st), calico_last_error(h_.get()));
    if (cov) cov->swap(c);
    if (valid) valid->swap(v);
    return OkStatus();
  }
  inline Status ProjectionUncertainty(const sensors::Camera& camera, const std::vector<Vector2d>& pixels, double range, ProjectionFrame frame,
                                      std::vector<std::array<double, 3>>* cov, std::vector<uint8_t>* valid) const;

 private:
  friend class Problem;
  std::shared_ptr<calico_problem> h_;
  std::map<const double*, int32_t> ids_;
  std::vector<int32_t> ctrl_ids_;      // block ids of the control points, in spline order
  std::vector<int32_t> sensor_ids_;    // library ids of the problem's sensors, their residual dimensions and block counts
  std::vector<int> sensor_dim_;
  std::vector<int64_t> sensor_n_;
};

inline Status Problem::ComputeCovariance(const calico_covariance_options& options, Covariance* out, int device) {
  if (Status b = Build(device); !b.ok()) return b;
  if (int st = calico_covariance_compute(h_, &options)) return Err(st);
  out->ids_.clear();
  for (size_t i = 0; i < blocks_.size(); ++i) out->ids_[blocks_[i].ptr] = ids_[i];
  out->ctrl_ids_.clear();
  for (double* c : ctrl_) {
    const auto it = out->ids_.find(c);
    out->ctrl_ids_.push_back(it == out->ids_.end() ? -1 : it->second);
  }
  out->sensor_ids_.assign(sensor_ids_.begin(), sensor_ids_.end());
  out->sensor_dim_.clear(); out->sensor_n_.clear();
  for (const SensorRec& s : sensors_) {
    out->sensor_dim_.push_back(s.kind == CALICO_SENSOR_CAMERA ? 2 : 3);
    out->sensor_n_.push_back(int64_t(s.stamps.size()));
  }
  out->h_ = std::shared_ptr<calico_problem>(h_, calico_problem_destroy);      // the result stays with its handle
  h_ = nullptr;
  return OkStatus();
}
inline calico_covariance_options DefaultCovarianceOptions() { calico_covariance_options o; calico_default_covariance_options(&o); return o; }

/// The observability report (calico_observability_* in include/calico_hip.h for the definition): the spectrum of the
/// calibration's equilibrated Schur complement, ascending, and its directions; blocks keyed by the parameter pointers the
/// Problem was given. A rank-deficient calibration is not an error: NumWeak() > 0 and Describe() says where the weak
/// directions live. It keeps the library handle it was computed on until destroyed.
class Observability {
 public:
  struct Entry { std::string name, part; double share; };      // e.g. {"gyroscope", "intrinsics", 0.52}
  int Dimension() const { int32_t v = 0; if (h_) calico_observability_info(h_.get(), &v, nullptr, nullptr, nullptr, nullptr, nullptr); return v; }
  int NumUnobserved() const { int32_t v = 0; if (h_) calico_observability_info(h_.get(), nullptr, &v, nullptr, nullptr, nullptr, nullptr); return v; }
  int NumWeak() const { int32_t v = 0; if (h_) calico_observability_info(h_.get(), nullptr, nullptr, &v, nullptr, nullptr, nullptr); return v; }
  int Sweeps() const { int32_t v = 0; if (h_) calico_observability_info(h_.get(), nullptr, nullptr, nullptr, nullptr, nullptr, &v); return v; }
  /// the eigenvalues, ascending (Dimension() - NumUnobserved() of them)
  std::vector<double> Eigenvalues() const {
    std::vector<double> v(static_cast<size_t>(std::max(0, Dimension() - NumUnobserved())), 0.0);
    if (h_ && !v.empty()) calico_observability_get_spectrum(h_.get(), v.data());
    return v;
  }
  /// direction i of the ascending list over the border's tangent rows: the unit eigenvector, or (tangent_units) δ_i in the
  /// parameters' own units; empty on error
  std::vector<double> Direction(int i, bool tangent_units = false) const {
    std::vector<double> v(static_cast<size_t>(Dimension()), 0.0);
    if (!h_ || v.empty() || calico_observability_get_directions(h_.get(), i, 1, tangent_units ? 1 : 0, v.data()) != CALICO_OK) v.clear();
    return v;
  }
  /// the share of direction i's unit eigenvector that lies in one parameter block (0 for a constant block)
  StatusOr<double> BlockShare(int i, const double* parameter) const {
    if (!h_) return FailedPreconditionError("observability has not been computed");
    const auto it = ids_.find(parameter);
    if (it == ids_.end()) return InvalidArgumentError("observability: parameter block not in the problem");
    double share = 0.0;
    const int st = calico_observability_get_block(h_.get(), i, it->second, 0, nullptr, &share);
    if (st != CALICO_OK) return Status(static_cast<StatusCode>(st), calico_last_error(h_.get()));
    return share;
  }
  /// the entries of direction i in one parameter block (tangent size: 3 for a quaternion)
  Status Block(int i, const double* parameter, bool tangent_units, double* out) const {
    if (!h_) return FailedPreconditionError("observability has not been computed");
    const auto it = ids_.find(parameter);
    if (it == ids_.end()) return InvalidArgumentError("observability: parameter block not in the problem");
    const int st = calico_observability_get_block(h_.get(), i, it->second, tangent_units ? 1 : 0, out, nullptr);
    return st == CALICO_OK ? OkStatus() : Status(static_cast<StatusCode>(st), calico_last_error(h_.get()));
  }
  /// a name for a block in Describe(): BatchOptimizer::AnalyzeObservability labels every sensor's blocks
  void Label(const double* parameter, const std::string& name, const std::string& part) { labels_.push_back({parameter, name, part}); }
  /// where direction i lives: the labelled blocks with a share above min_share, largest share first
  std::vector<Entry> Describe(int i, double min_share = 1e-12) const {
    std::vector<Entry> out;
    for (const LabelRec& l : labels_) {
      const auto sh = BlockShare(i, l.ptr);
      if (sh.ok() && sh.value() > min_share) out.push_back({l.name, l.part, sh.value()});
    }
    std::stable_sort(out.begin(), out.end(), [](const Entry& a, const Entry& b) { return a.share > b.share; });
    return out;
  }

 private:
  friend class Problem;
  struct LabelRec { const double* ptr; std::string name, part; };
  std::shared_ptr<calico_problem> h_;
  std::map<const double*, int32_t> ids_;
  std::vector<LabelRec> labels_;
};

inline Status Problem::AnalyzeObservability(const calico_observability_options& options, Observability* out, int device) {
  if (Status b = Build(device); !b.ok()) return b;
  if (int st = calico_observability_compute(h_, &options)) return Err(st);
  out->ids_.clear();
  for (size_t i = 0; i < blocks_.size(); ++i) out->ids_[blocks_[i].ptr] = ids_[i];
  out->h_ = std::shared_ptr<calico_problem>(h_, calico_problem_destroy);      // the result stays with its handle
  h_ = nullptr;
  return OkStatus();
}
inline calico_observability_options DefaultObservabilityOptions() { calico_observability_options o; calico_default_observability_options(&o); return o; }

namespace utils {
/// optimization_utils.h:51-68
inline int AddPoseToProblem(Problem& problem, Pose3d& pose) {
  problem.AddParameterBlock(pose.translation().data(), 3);
  problem.AddParameterBlock(pose.rotation().coeffs().data(), 4, CALICO_MANIFOLD_EIGEN_QUATERNION);
  return 7;
}
inline void SetPoseConstantInProblem(Problem& problem, Pose3d& pose) {
  problem.SetParameterBlockConstant(pose.translation().data());
  problem.SetParameterBlockConstant(pose.rotation().coeffs().data());
}
}  // namespace utils

// ---------------------------------------------------------------------------
// Trajectory: 6-DOF B-spline of [axis-angle; position] (trajectory.{h,cpp}, bspline.{h,hpp})
// ---------------------------------------------------------------------------
class BSpline6 {
 public:
#ifdef CALICO_TEST_HOOKS
  /// Test builds only (-DCALICO_TEST_HOOKS, tests/cpp): the least-squares solve behind FitToData can be replaced, so
  /// that the host-only unit test runs the surrounding logic on a machine without a GPU with a checker-backed solver.
  /// A product build calls calico_fit_spline on device 0 -- the library has no host fallback.
  using FitSolver = int32_t (*)(int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n,
                                const double* stamps, const double* data6, double* ctrl_out);
  static FitSolver& fit_solver() {
    static FitSolver solver = nullptr;
    return solver;
  }
#endif
  int GetSplineOrder() const { return order_; }
  const std::vector<double>& knots() const { return knots_; }
  const std::vector<double>& valid_knots() const { return valid_knots_; }
  std::vector<std::array<double, 6>>& control_points() { return ctrl_; }
  const std::vector<std::array<double, 6>>& control_points() const { return ctrl_; }
  const std::vector<double>& basis_matrices() const { return basis_; }  // n_seg × k × k
  /// bspline.hpp:138-150
  int GetSplineIndex(double t) const {
    if (t == valid_knots_.back()) return int(valid_knots_.size()) - 2;
    if (t < valid_knots_.back()) return int(std::upper_bound(valid_knots_.begin(), valid_knots_.end(), t) - valid_knots_.begin()) - 1;
    return -1;
  }
  int GetKnotIndexFromSplineIndex(int i) const { return i + order_ - 1; }
  int AddParametersToProblem(Problem& problem) {  // bspline.hpp:10-17
    int n = 0;
    for (auto& c : ctrl_) { problem.AddParameterBlock(c.data(), 6); n += 6; }
    return n;
  }
  /// bspline.hpp:19-37,163-297 (knot vector and basis matrices here, the least-squares solve on the device)
  Status FitToData(const std::vector<double>& time, const std::vector<std::array<double, 6>>& data, int order, double knot_frequency) {
    if (time.empty()) return InvalidArgumentError("Attempted to fit data on empty time vector.");
    if (data.empty()) return InvalidArgumentError("Attempted to fit on empty data.");
    if (time.size() != data.size()) return InvalidArgumentError("Data and time vectors are not the same size.");
    if (order < 2) return InvalidArgumentError("Spline order must be greater than 2. Got " + std::to_string(order));
    if (knot_frequency <= 0) return InvalidArgumentError("Knot frequency must be greater than 0.");
    const int nk = BuildKnots(time, order, knot_frequency);
    // least-squares control points on the device (calico_fit_spline: banded normal equations + banded Cholesky; the
    // reference factors the dense normal equations by column-pivoted QR, bspline.hpp:287-293)
    const int ncp = nk - order;
    const int64_t nd = int64_t(time.size());
    std::vector<double> flat(size_t(nd) * 6), ctrl(size_t(ncp) * 6);
    for (int64_t j = 0; j < nd; ++j) for (int c = 0; c < 6; ++c) flat[size_t(j) * 6 + c] = data[size_t(j)][size_t(c)];
#ifdef CALICO_TEST_HOOKS
    const int32_t rc = fit_solver() ? fit_solver()(order, nk, knots_.data(), basis_.data(), nd, time.data(), flat.data(), ctrl.data())
                                    : calico_fit_spline(0, order, nk, knots_.data(), basis_.data(), nd, time.data(), flat.data(), ctrl.data());
#else
    const int32_t rc = calico_fit_spline(0, order, nk, knots_.data(), basis_.data(), nd, time.data(), flat.data(), ctrl.data());
#endif
    if (rc == CALICO_INVALID_ARGUMENT) return InvalidArgumentError("spline fit: stamps must be sorted and inside the knot range");
    if (rc == CALICO_UNIMPLEMENTED)      // calico_fit_spline's on-chip solve holds [band | rhs]: n_ctrl (order + 6) doubles in 156 KiB
      return UnimplementedError("spline fit: " + std::to_string(ncp) + " control points are too many for the on-device solve; order " +
                                std::to_string(order) + " fits at most " + std::to_string(156 * 1024 / ((order + 6) * 8)));
    if (rc != CALICO_OK) return InternalError("spline fit failed on the device");
    ctrl_.assign(size_t(ncp), {});
    for (int i = 0; i < ncp; ++i) for (int c = 0; c < 6; ++c) ctrl_[size_t(i)][size_t(c)] = ctrl[size_t(i) * 6 + c];
    return OkStatus();
  }
  /// What a smoothing fit found: the summary (per group status, chosen lambda, samples used) and the row of every (group, lambda).
  struct SmoothFit {
    calico_spline_fit_summary summary{};
    std::vector<calico_spline_fit_row> rows;      // 2 x n_lambda, group-major
  };
#ifdef CALICO_TEST_HOOKS
  /// Test builds only, as fit_solver(): the solve behind FitToDataSmooth (calico_fit_spline_smooth without its device argument).
  using SmoothFitSolver = int32_t (*)(int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n, const double* stamps,
                                      const double* data6, const double* weights, const calico_spline_fit_options* options, double* ctrl_out,
                                      double* ctrl_all_out, calico_spline_fit_row* rows_out, calico_spline_fit_summary* summary);
  static SmoothFitSolver& smooth_fit_solver() {
    static SmoothFitSolver solver = nullptr;
    return solver;
  }
#endif
  /// The smoothing (penalised) fit on the knot vector and basis of FitToData: calico_fit_spline_smooth on device 0. weights: one
  /// [rotation, position] pair per sample, or empty (all 1). The control points are each group's chosen lambda's.
  Status FitToDataSmooth(const std::vector<double>& time, const std::vector<std::array<double, 6>>& data, int order, double knot_frequency,
                         const calico_spline_fit_options& options, const std::vector<std::array<double, 2>>& weights, SmoothFit* fit = nullptr) {
    if (time.empty()) return InvalidArgumentError("Attempted to fit data on empty time vector.");
    if (data.empty()) return InvalidArgumentError("Attempted to fit on empty data.");
    if (time.size() != data.size()) return InvalidArgumentError("Data and time vectors are not the same size.");
    if (!weights.empty() && weights.size() != time.size()) return InvalidArgumentError("Weights and time vectors are not the same size.");
    if (order < 2) return InvalidArgumentError("Spline order must be greater than 2. Got " + std::to_string(order));
    if (knot_frequency <= 0) return InvalidArgumentError("Knot frequency must be greater than 0.");
    const int nk = BuildKnots(time, order, knot_frequency), ncp = nk - order;
    const int64_t nd = int64_t(time.size());
    std::vector<double> flat(size_t(nd) * 6), w(weights.size() * 2), ctrl(size_t(ncp) * 6);
    for (int64_t j = 0; j < nd; ++j) for (int c = 0; c < 6; ++c) flat[size_t(j) * 6 + c] = data[size_t(j)][size_t(c)];
    for (size_t j = 0; j < weights.size(); ++j) { w[j * 2] = weights[j][0]; w[j * 2 + 1] = weights[j][1]; }
    SmoothFit found;
    found.rows.assign(size_t(2) * size_t(std::min(std::max(options.n_lambda, 1), CALICO_FIT_MAX_LAMBDAS)), calico_spline_fit_row{});
    const double* wp = w.empty() ? nullptr : w.data();
#ifdef CALICO_TEST_HOOKS
    const int32_t rc = smooth_fit_solver()
        ? smooth_fit_solver()(order, nk, knots_.data(), basis_.data(), nd, time.data(), flat.data(), wp, &options, ctrl.data(), nullptr, found.rows.data(), &found.summary)
        : calico_fit_spline_smooth(0, order, nk, knots_.data(), basis_.data(), nd, time.data(), flat.data(), wp, &options, ctrl.data(), nullptr, found.rows.data(), &found.summary);
#else
    const int32_t rc = calico_fit_spline_smooth(0, order, nk, knots_.data(), basis_.data(), nd, time.data(), flat.data(), wp, &options, ctrl.data(),
                                                nullptr, found.rows.data(), &found.summary);
#endif
    if (fit) *fit = found;
    const char* why = calico_last_error(nullptr);
    if (rc == CALICO_INVALID_ARGUMENT) return InvalidArgumentError(std::string("smoothing spline fit: ") + (why ? why : "invalid argument"));
    if (rc == CALICO_UNIMPLEMENTED)      // the on-chip solve holds one group's [band | 3 rhs]: n_ctrl (order + 3) doubles in 156 KiB
      return UnimplementedError("smoothing spline fit: " + std::to_string(ncp) + " control points are too many for the on-device solve; order " +
                                std::to_string(order) + " fits at most " + std::to_string(156 * 1024 / ((order + 3) * 8)));
    if (rc != CALICO_OK) return InternalError("smoothing spline fit failed on the device");
    ctrl_.assign(size_t(ncp), {});
    for (int i = 0; i < ncp; ++i) for (int c = 0; c < 6; ++c) ctrl_[size_t(i)][size_t(c)] = ctrl[size_t(i) * 6 + c];
    return OkStatus();
  }
  /// What a robust fit found: the summary (per group status, iterations, scale, counts), and per sample in time order the robust
  /// weight of the last solve (0 where the prior weight is 0) and the residual norm at the result (NaN there), [rotation, position].
  struct RobustFit {
    calico_spline_robust_summary summary{};
    std::vector<std::array<double, 2>> robust_weights, residuals;
  };
#ifdef CALICO_TEST_HOOKS
  /// Test builds only, as fit_solver(): the solve behind FitToDataRobust (calico_fit_spline_robust without its device argument).
  using RobustFitSolver = int32_t (*)(int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n, const double* stamps,
                                      const double* data6, const double* weights, const calico_spline_fit_options* fit,
                                      const calico_spline_robust_options* robust, double* ctrl_out, double* robust_weights_out,
                                      double* residuals_out, calico_spline_robust_summary* summary);
  static RobustFitSolver& robust_fit_solver() {
    static RobustFitSolver solver = nullptr;
    return solver;
  }
#endif
  /// The robust fit on the knot vector and basis of FitToData: calico_fit_spline_robust on device 0 (iteratively reweighted least
  /// squares around the smoothing fit; `options` takes one lambda per group and no target). weights: prior weights, as FitToDataSmooth's.
  Status FitToDataRobust(const std::vector<double>& time, const std::vector<std::array<double, 6>>& data, int order, double knot_frequency,
                         const calico_spline_fit_options& options, const calico_spline_robust_options& robust,
                         const std::vector<std::array<double, 2>>& weights, RobustFit* fit = nullptr) {
    if (time.empty()) return InvalidArgumentError("Attempted to fit data on empty time vector.");
    if (data.empty()) return InvalidArgumentError("Attempted to fit on empty data.");
    if (time.size() != data.size()) return InvalidArgumentError("Data and time vectors are not the same size.");
    if (!weights.empty() && weights.size() != time.size()) return InvalidArgumentError("Weights and time vectors are not the same size.");
    if (order < 2) return InvalidArgumentError("Spline order must be greater than 2. Got " + std::to_string(order));
    if (knot_frequency <= 0) return InvalidArgumentError("Knot frequency must be greater than 0.");
    const int nk = BuildKnots(time, order, knot_frequency), ncp = nk - order;
    const int64_t nd = int64_t(time.size());
    std::vector<double> flat(size_t(nd) * 6), w(weights.size() * 2), ctrl(size_t(ncp) * 6), u(size_t(nd) * 2), e(size_t(nd) * 2);
    for (int64_t j = 0; j < nd; ++j) for (int c = 0; c < 6; ++c) flat[size_t(j) * 6 + c] = data[size_t(j)][size_t(c)];
    for (size_t j = 0; j < weights.size(); ++j) { w[j * 2] = weights[j][0]; w[j * 2 + 1] = weights[j][1]; }
    RobustFit found;
    const double* wp = w.empty() ? nullptr : w.data();
#ifdef CALICO_TEST_HOOKS
    const int32_t rc = robust_fit_solver()
        ? robust_fit_solver()(order, nk, knots_.data(), basis_.data(), nd, time.data(), flat.data(), wp, &options, &robust, ctrl.data(), u.data(), e.data(), &found.summary)
        : calico_fit_spline_robust(0, order, nk, knots_.data(), basis_.data(), nd, time.data(), flat.data(), wp, &options, &robust, ctrl.data(), u.data(), e.data(), &found.summary);
#else
    const int32_t rc = calico_fit_spline_robust(0, order, nk, knots_.data(), basis_.data(), nd, time.data(), flat.data(), wp, &options, &robust,
                                                ctrl.data(), u.data(), e.data(), &found.summary);
#endif
    const char* why = calico_last_error(nullptr);
    if (rc == CALICO_INVALID_ARGUMENT) return InvalidArgumentError(std::string("robust spline fit: ") + (why ? why : "invalid argument"));
    if (rc == CALICO_UNIMPLEMENTED)      // the smoothing fit's ceiling: one group's [band | 3 rhs], n_ctrl (order + 3) doubles in 156 KiB
      return UnimplementedError("robust spline fit: " + std::to_string(ncp) + " control points are too many for the on-device solve; order " +
                                std::to_string(order) + " fits at most " + std::to_string(156 * 1024 / ((order + 3) * 8)));
    found.robust_weights.resize(size_t(nd));
    found.residuals.resize(size_t(nd));
    for (int64_t j = 0; j < nd; ++j) {
      found.robust_weights[size_t(j)] = {u[size_t(j) * 2], u[size_t(j) * 2 + 1]};
      found.residuals[size_t(j)] = {e[size_t(j) * 2], e[size_t(j) * 2 + 1]};
    }
    if (fit) *fit = found;
    if (rc != CALICO_OK) return InternalError("robust spline fit failed on the device");
    ctrl_.assign(size_t(ncp), {});
    for (int i = 0; i < ncp; ++i) for (int c = 0; c < 6; ++c) ctrl_[size_t(i)][size_t(c)] = ctrl[size_t(i) * 6 + c];
    return OkStatus();
  }
  /// What a cross-validated fit found: the summary (per group status, chosen lambda, edf and score there), the smoothing fit's row
  /// and the cross-validation row of every (group, lambda), and per sample in time order the leverage h_j at the chosen lambda (0
  /// where the weight is 0) and the leave-one-out residual e_j / (1 - h_j) (NaN there), [rotation, position].
  struct CvFit {
    calico_spline_cv_summary summary{};
    std::vector<calico_spline_fit_row> rows;      // 2 x n_lambda, group-major
    std::vector<calico_spline_cv_row> cv_rows;    // 2 x n_lambda, group-major
    std::vector<std::array<double, 2>> leverage, loo_residuals;
  };
#ifdef CALICO_TEST_HOOKS
  /// Test builds only, as fit_solver(): the solve behind FitToDataCV (calico_fit_spline_cv without its device argument).
  using CvFitSolver = int32_t (*)(int32_t order, int32_t n_knots, const double* knots, const double* basis, int64_t n, const double* stamps,
                                  const double* data6, const double* weights, const calico_spline_fit_options* fit,
                                  const calico_spline_cv_options* cv, double* ctrl_out, double* ctrl_all_out, calico_spline_fit_row* rows_out,
                                  calico_spline_cv_row* cv_rows_out, double* leverage_out, double* loo_residuals_out,
                                  calico_spline_cv_summary* summary);
  static CvFitSolver& cv_fit_solver() {
    static CvFitSolver solver = nullptr;
    return solver;
  }
#endif
  /// The smoothing fit with each group's lambda chosen from `options`' grid by cross-validation (calico_fit_spline_cv on device 0:
  /// generalised cross-validation or the leave-one-out score, `cv.criterion`); `options` takes no target. weights: as FitToDataSmooth's.
  Status FitToDataCV(const std::vector<double>& time, const std::vector<std::array<double, 6>>& data, int order, double knot_frequency,
                     const calico_spline_fit_options& options, const calico_spline_cv_options& cv,
                     const std::vector<std::array<double, 2>>& weights, CvFit* fit = nullptr) {
    if (time.empty()) return InvalidArgumentError("Attempted to fit data on empty time vector.");
    if (data.empty()) return InvalidArgumentError("Attempted to fit on empty data.");
    if (time.size() != data.size()) return InvalidArgumentError("Data and time vectors are not the same size.");
    if (!weights.empty() && weights.size() != time.size()) return InvalidArgumentError("Weights and time vectors are not the same size.");
    if (order < 2) return InvalidArgumentError("Spline order must be greater than 2. Got " + std::to_string(order));
    if (knot_frequency <= 0) return InvalidArgumentError("Knot frequency must be greater than 0.");
    const int nk = BuildKnots(time, order, knot_frequency), ncp = nk - order;
    const int64_t nd = int64_t(time.size());
    std::vector<double> flat(size_t(nd) * 6), w(weights.size() * 2), ctrl(size_t(ncp) * 6), h(size_t(nd) * 2), loo(size_t(nd) * 2);
    for (int64_t j = 0; j < nd; ++j) for (int c = 0; c < 6; ++c) flat[size_t(j) * 6 + c] = data[size_t(j)][size_t(c)];
    for (size_t j = 0; j < weights.size(); ++j) { w[j * 2] = weights[j][0]; w[j * 2 + 1] = weights[j][1]; }
    CvFit found;
    const size_t n_rows = size_t(2) * size_t(std::min(std::max(options.n_lambda, 1), CALICO_FIT_MAX_LAMBDAS));
    found.rows.assign(n_rows, calico_spline_fit_row{});
    found.cv_rows.assign(n_rows, calico_spline_cv_row{});
    const double* wp = w.empty() ? nullptr : w.data();
#ifdef CALICO_TEST_HOOKS
    const int32_t rc = cv_fit_solver()
        ? cv_fit_solver()(order, nk, knots_.data(), basis_.data(), nd, time.data(), flat.data(), wp, &options, &cv, ctrl.data(), nullptr, found.rows.data(), found.cv_rows.data(), h.data(), loo.data(), &found.summary)
        : calico_fit_spline_cv(0, order, nk, knots_.data(), basis_.data(), nd, time.data(), flat.data(), wp, &options, &cv, ctrl.data(), nullptr, found.rows.data(), found.cv_rows.data(), h.data(), loo.data(), &found.summary);
#else
    const int32_t rc = calico_fit_spline_cv(0, order, nk, knots_.data(), basis_.data(), nd, time.data(), flat.data(), wp, &options, &cv, ctrl.data(),
                                            nullptr, found.rows.data(), found.cv_rows.data(), h.data(), loo.data(), &found.summary);
#endif
    const char* why = calico_last_error(nullptr);
    if (rc == CALICO_INVALID_ARGUMENT) return InvalidArgumentError(std::string("cross-validated spline fit: ") + (why ? why : "invalid argument"));
    if (rc == CALICO_UNIMPLEMENTED)      // the smoothing fit's ceiling: one group's [band | 3 rhs], n_ctrl (order + 3) doubles in 156 KiB
      return UnimplementedError("cross-validated spline fit: " + std::to_string(ncp) + " control points are too many for the on-device solve; order " +
                                std::to_string(order) + " fits at most " + std::to_string(156 * 1024 / ((order + 3) * 8)));
    found.leverage.resize(size_t(nd));
    found.loo_residuals.resize(size_t(nd));
    for (int64_t j = 0; j < nd; ++j) {
      found.leverage[size_t(j)] = {h[size_t(j) * 2], h[size_t(j) * 2 + 1]};
      found.loo_residuals[size_t(j)] = {loo[size_t(j) * 2], loo[size_t(j) * 2 + 1]};
    }
    if (fit) *fit = found;
    if (rc != CALICO_OK) return InternalError("cross-validated spline fit failed on the device");
    ctrl_.assign(size_t(ncp), {});
    for (int i = 0; i < ncp; ++i) for (int c = 0; c < 6; ++c) ctrl_[size_t(i)][size_t(c)] = ctrl[size_t(i) * 6 + c];
    return OkStatus();
  }
  /// bspline.hpp:39-72 at one time; error codes of bspline.hpp:74-85
  Status Evaluate(double t, int derivative, double out[6]) const {
    if (derivative < 0 || derivative > order_ - 1) return InvalidArgumentError("Invalid derivative for interpolation.");
    if (t < valid_knots_.front() || t > valid_knots_.back())
      return InvalidArgumentError("Cannot interpolate " + std::to_string(t) + ". Value is not within valid knots.");
    const int si = GetSplineIndex(t), ki = si + order_ - 1, k = order_;
    const double dti = 1.0 / (knots_[size_t(ki + 1)] - knots_[size_t(ki)]), u = (t - knots_[size_t(ki)]) * dti;
    double scale = 1.0; for (int j = 0; j < derivative; ++j) scale *= dti;
    std::vector<double> U(size_t(k), 0.0);
    for (int i = derivative; i < k; ++i) { double coeff = 1.0; for (int j = i - derivative; j < i; ++j) coeff *= (j + 1); U[size_t(i)] = coeff * std::pow(u, i - derivative) * scale; }
    for (int c = 0; c < 6; ++c) out[c] = 0.0;
    for (int j = 0; j < k; ++j) {
      double w = 0.0; for (int i = 0; i < k; ++i) w += U[size_t(i)] * basis_[(size_t(si) * k + i) * k + j];
      for (int c = 0; c < 6; ++c) out[c] += w * ctrl_[size_t(si + j)][size_t(c)];
    }
    return OkStatus();
  }
 private:
  /// bspline.hpp:163-189: the knot vector over [time.front(), time.back()] and the basis matrix of every segment. Returns n_knots.
  int BuildKnots(const std::vector<double>& time, int order, double knot_frequency) {
    order_ = order;
    const int deg = order - 1;
    const double duration = time.back() - time.front(), dt = 1.0 / knot_frequency;
    const int nvalid = 1 + int(std::ceil(duration * knot_frequency)), nk = nvalid + 2 * deg;
    knots_.assign(size_t(nk), 0.0); valid_knots_.assign(size_t(nvalid), 0.0);
    for (int i = -deg; i < nk - deg; ++i) {
      knots_[size_t(i + deg)] = time.front() + dt * i;
      if (i > -1 && i < nvalid) valid_knots_[size_t(i)] = knots_[size_t(i + deg)];
    }
    const int nseg = nvalid - 1;
    basis_.assign(size_t(nseg) * order * order, 0.0);
    for (int s = 0; s < nseg; ++s) {
      const std::vector<double> M = Basis(order, s + deg);
      std::copy(M.begin(), M.end(), basis_.begin() + size_t(s) * order * order);
    }
    return nk;
  }
  std::vector<double> Basis(int k, int i) const {  // bspline.hpp:191-244
    if (k == 1) return {1.0};
    const std::vector<double> P = Basis(k - 1, i);
    std::vector<double> M(size_t(k) * k, 0.0);
    for (int index = 0; index < k - 1; ++index) {
      const int j = i - k + 2 + index;
      const double den = knots_[size_t(j + k - 1)] - knots_[size_t(j)];
      const double d0 = den <= 0 ? 0.0 : (knots_[size_t(i)] - knots_[size_t(j)]) / den;
      const double d1 = den <= 0 ? 0.0 : (knots_[size_t(i + 1)] - knots_[size_t(i)]) / den;
      for (int r = 0; r < k; ++r) {
        const double m1 = r < k - 1 ? P[size_t(r) * (k - 1) + index] : 0.0;  // [M;0]
        const double m2 = r > 0 ? P[size_t(r - 1) * (k - 1) + index] : 0.0;  // [0;M]
        M[size_t(r) * k + index] += m1 * (1.0 - d0) - m2 * d1;
        M[size_t(r) * k + index + 1] += m1 * d0 + m2 * d1;
      }
    }
    return M;
  }
  int order_ = 0;
  std::vector<double> knots_, valid_knots_, basis_;
  std::vector<std::array<double, 6>> ctrl_;
};

namespace sensors { class Gyroscope; class Accelerometer; }
class WorldModel;

class Trajectory {
 public:
  static constexpr int kDefaultSplineOrder = 6;       // trajectory.h:28
  static constexpr double kDefaultKnotFrequency = 10;  // trajectory.h:31
  /// trajectory.cpp:14-49
  Status FitSpline(const std::map<double, Pose3d>& poses_world_sensorrig, double knot_frequency = kDefaultKnotFrequency,
                   int spline_order = kDefaultSplineOrder) {
    poses_ = poses_world_sensorrig;
    std::vector<double> stamps;
    std::vector<std::array<double, 6>> data;
    PosesToData(&stamps, &data);
    return spline_.FitToData(stamps, data, spline_order, knot_frequency);
  }
  /// FitSpline with the smoothing fit (calico_fit_spline_smooth): the same axis-angle conversion and phase unwrapping, then the
  /// penalised fit with `options` (calico_default_spline_fit_options for the defaults) and one [rotation, position] weight pair
  /// per pose in time order, or none (all 1). Poses that are unknown are simply left out: the penalty carries the spline across.
  StatusOr<BSpline6::SmoothFit> FitSplineSmooth(const std::map<double, Pose3d>& poses_world_sensorrig, double knot_frequency,
                                                int spline_order, const calico_spline_fit_options& options,
                                                const std::vector<std::array<double, 2>>& weights = {}) {
    poses_ = poses_world_sensorrig;
    std::vector<double> stamps;
    std::vector<std::array<double, 6>> data;
    PosesToData(&stamps, &data);
    BSpline6::SmoothFit fit;
    const Status st = spline_.FitToDataSmooth(stamps, data, spline_order, knot_frequency, options, weights, &fit);
    if (!st.ok()) return st;
    return fit;
  }
  /// FitSpline with the robust fit (calico_fit_spline_robust): the same axis-angle conversion and phase unwrapping, then
  /// iteratively reweighted least squares (Huber or Tukey) around the smoothing fit -- for poses that are wrong and not known to
  /// be (a resection on the other branch of the planar ambiguity reports a small RMS). `fit_options` takes one lambda per group;
  /// the result's robust_weights single out the poses the fit set aside, in time order.
  StatusOr<BSpline6::RobustFit> FitSplineRobust(const std::map<double, Pose3d>& poses_world_sensorrig, double knot_frequency,
                                                int spline_order, const calico_spline_fit_options& fit_options,
                                                const calico_spline_robust_options& robust_options,
                                                const std::vector<std::array<double, 2>>& weights = {}) {
    poses_ = poses_world_sensorrig;
    std::vector<double> stamps;
    std::vector<std::array<double, 6>> data;
    PosesToData(&stamps, &data);
    BSpline6::RobustFit fit;
    const Status st = spline_.FitToDataRobust(stamps, data, spline_order, knot_frequency, fit_options, robust_options, weights, &fit);
    if (!st.ok()) return st;
    return fit;
  }
  /// FitSpline with the smoothing fit's lambda chosen by cross-validation (calico_fit_spline_cv): the same axis-angle conversion
  /// and phase unwrapping, then every lambda of `fit_options`' grid (no target), and per group the one with the smallest
  /// generalised cross-validation or leave-one-out score -- no noise level of the poses is needed. The result carries the scores of
  /// the whole grid, and per pose in time order its leverage and leave-one-out residual at the choice.
  StatusOr<BSpline6::CvFit> FitSplineCV(const std::map<double, Pose3d>& poses_world_sensorrig, double knot_frequency, int spline_order,
                                        const calico_spline_fit_options& fit_options, const calico_spline_cv_options& cv_options,
                                        const std::vector<std::array<double, 2>>& weights = {}) {
    poses_ = poses_world_sensorrig;
    std::vector<double> stamps;
    std::vector<std::array<double, 6>> data;
    PosesToData(&stamps, &data);
    BSpline6::CvFit fit;
    const Status st = spline_.FitToDataCV(stamps, data, spline_order, knot_frequency, fit_options, cv_options, weights, &fit);
    if (!st.ok()) return st;
    return fit;
  }
  int AddParametersToProblem(Problem& problem) {  // trajectory.cpp:51 (+ the evaluation tables of :63-79)
    const int n = spline_.AddParametersToProblem(problem);
    std::vector<double*> ctrl;
    for (auto& c : spline_.control_points()) ctrl.push_back(c.data());
    problem.SetSpline(spline_.GetSplineOrder(), spline_.knots(), spline_.basis_matrices(), ctrl);
    return n;
  }
  const BSpline6& spline() const { return spline_; }
  BSpline6& spline() { return spline_; }
 private:
  /// trajectory.cpp:24-46: poses_ in time order as [unwrapped axis-angle; position]
  void PosesToData(std::vector<double>* stamps, std::vector<std::array<double, 6>>* data) const {
    std::array<double, 3> prev{};
    bool first = true;
    for (const auto& [stamp, T] : poses_) {  // std::map iterates sorted (trajectory.cpp:24 sorts)
      const Quaterniond& q = T.rotation();
      const double n = std::sqrt(q.x() * q.x() + q.y() * q.y() + q.z() * q.z());
      std::array<double, 3> phi{0, 0, 0};
      if (n != 0.0) {  // Eigen::AngleAxisd(Quaterniond)
        const double angle = 2.0 * std::atan2(n, std::fabs(q.w())), s = (q.w() < 0 ? -1.0 : 1.0) / n;
        phi = {q.x() * s * angle, q.y() * s * angle, q.z() * s * angle};
      }
      if (!first) {  // UnwrapPhaseLogMap, trajectory.cpp:81-93
        const double theta = std::sqrt(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]);
        if (theta != 0) {
          const double k = std::round((phi[0] * prev[0] + phi[1] * prev[1] + phi[2] * prev[2] - theta * theta) / (2.0 * M_PI * theta));
          for (double& p : phi) p *= (1.0 + 2.0 * M_PI * k / theta);
        }
      }
      prev = phi; first = false;
      stamps->push_back(stamp);
      data->push_back({phi[0], phi[1], phi[2], T.translation()[0], T.translation()[1], T.translation()[2]});
    }
  }
 public:
  /// trajectory.h:93-101
  static Pose3d VectorToPose3(const double v[6]) {
    const cal::Q4 q = cal::angle_axis_to_quat(cal::mk(v[0], v[1], v[2]));
    return Pose3d(Quaterniond(q.w, q.x, q.y, q.z), Vector3d(v[3], v[4], v[5]));
  }
  StatusOr<std::vector<Pose3d>> Interpolate(const std::vector<double>& interp_times) const {
    std::vector<Pose3d> out(interp_times.size());
    for (size_t i = 0; i < interp_times.size(); ++i) {
      double v[6];
      const Status st = spline_.Evaluate(interp_times[i], 0, v);
      if (!st.ok()) return st;
      out[i] = VectorToPose3(v);
    }
    return out;
  }
  const std::map<double, Pose3d>& trajectory() const { return poses_; }
  /// What AlignImu returns: calico_imu_align's outputs. gravity_world and accel_bias are meaningful when
  /// summary.accel_status == CALICO_ALIGN_OK; cov (7 x 7, row-major: rotation 3, bias 3, latency 1) and curve (summary.n_lags
  /// correlations) are filled on request.
  struct ImuAlignment {
    Quaterniond q_rig_gyro{1, 0, 0, 0};
    Vector3d gyro_bias{0, 0, 0}, gravity_world{0, 0, 0}, accel_bias{0, 0, 0};
    double latency = 0.0;
    std::vector<double> cov, curve;
    calico_imu_alignment_summary summary{};
  };
  /// Camera-IMU alignment against this trajectory (calico_imu_align, on the device): the rotation rig <- gyroscope, the
  /// gyroscope's bias, the IMU's latency and, with an accelerometer, the world's gravity and the accelerometer's bias, from the
  /// sensors' registered measurements (AddMeasurement), in time order. The sensors are read, not changed
  /// (utils.InitializeImu / the caller sets them). A Status that is not OK is an argument error or a device error; how the
  /// estimation ended is summary.gyro_status / accel_status.
  StatusOr<ImuAlignment> AlignImu(const sensors::Gyroscope& gyroscope, const sensors::Accelerometer* accelerometer = nullptr,
                                  const calico_imu_alignment_options* options = nullptr, bool covariance = false, bool curve = false,
                                  int device = 0) const;
  /// What AlignAccelerometer returns: calico_accel_align's outputs; cov (13 x 13, row-major: rotation 3, lever arm 3, bias 3,
  /// gravity 3, latency 1) is filled on request.
  struct AccelerometerAlignment {
    Pose3d T_rig_accel;
    Vector3d bias{0, 0, 0}, gravity_world{0, 0, 0};
    double latency = 0.0;
    std::vector<double> cov;
    calico_accel_alignment_summary summary{};
    bool Ok() const { return summary.status == CALICO_ALIGN_OK; }
  };
  /// Alignment of an accelerometer against this trajectory (calico_accel_align, on the device): its rotation, its lever arm, its
  /// bias, the world's gravity and its latency, from its registered measurements (AddMeasurement) in time order. The start is
  /// the sensor's current rotation and latency (what AlignImu / utils.InitializeImu found for the gyroscope of the same unit);
  /// lever arm, bias and gravity start from the call's own linear stage, so all three are estimated. The sensor is read, not
  /// changed (utils.InitializeAccelerometer / the caller sets it). A Status that is not OK is an argument error or a device
  /// error; how the estimation ended is summary.status.
  StatusOr<AccelerometerAlignment> AlignAccelerometer(const sensors::Accelerometer& accelerometer,
                                                      const calico_accel_alignment_options* options = nullptr, bool covariance = false,
                                                      int device = 0) const;
  /// What AlignCamera returns: calico_camera_align's outputs. The frames are the camera's images of the rigid body, in stamp
  /// order: image_ids, stamps and, per frame, the RMS pixel residual, the pairs used and the status (CALICO_RESECT_* or
  /// CALICO_CAMERA_ALIGN_FRAME_OUTSIDE); cov (7 x 7, row-major: rotation 3, translation 3, latency 1) and curve (summary.n_lags
  /// scores) are filled on request.
  struct CameraAlignment {
    Pose3d T_rig_camera;
    double latency = 0.0;
    std::vector<int> image_ids;
    std::vector<double> stamps, frame_rms;
    std::vector<int32_t> frame_n_used;
    std::vector<uint8_t> frame_status;
    std::vector<double> cov, curve;
    calico_camera_alignment_summary summary{};
    bool Ok() const { return summary.status == CALICO_ALIGN_OK; }
  };
  /// Alignment of a camera that is not synchronised with this trajectory (calico_camera_align, on the device): its extrinsics
  /// T_rig_camera and its latency at its current intrinsics, from its registered measurements (AddMeasurement) of the rigid body
  /// model_id that are not marked as outliers, grouped by image_id (a frame's stamp is its measurements'), with the body's
  /// model definition and pose. The camera is read, not changed (utils.InitializeCamera / the caller sets it). A Status that is
  /// not OK is an argument error or a device error; how the estimation ended is summary.status.
  StatusOr<CameraAlignment> AlignCamera(const sensors::Camera& camera, const WorldModel& world_model,
                                        const calico_camera_alignment_options* options = nullptr, int model_id = 0, bool covariance = false,
                                        bool curve = false, int device = 0) const;
 private:
  std::map<double, Pose3d> poses_;
  BSpline6 spline_;
};

// ---------------------------------------------------------------------------
// WorldModel (world_model.{h,cpp})
// ---------------------------------------------------------------------------
constexpr int kLandmarkFrameId = -1;
struct Landmark { Vector3d point; int id = 0; bool point_is_constant = false; };
struct RigidBody {
  std::unordered_map<int, Vector3d> model_definition;
  Pose3d T_world_rigidbody;
  int id = 0;
  bool world_pose_is_constant = false;
  bool model_definition_is_constant = false;
};
class WorldModel {
 public:
  static constexpr double kGravityDefaultZ = -9.80665;
  WorldModel() : gravity_(0.0, 0.0, kGravityDefaultZ) {}
  ~WorldModel() { Clear(); }
  Status AddLandmark(Landmark* landmark, bool take_ownership = true) {
    if (landmarks_.count(landmark->id)) return InvalidArgumentError("Landmark with id " + std::to_string(landmark->id) + " already exists in world model.");
    landmarks_[landmark->id] = landmark; own_l_[landmark->id] = take_ownership; return OkStatus();
  }
  Status AddRigidBody(RigidBody* rigidbody, bool take_ownership = true) {
    if (bodies_.count(rigidbody->id)) return InvalidArgumentError("Rigid body with id " + std::to_string(rigidbody->id) + "already exists in world model.");
    bodies_[rigidbody->id] = rigidbody; own_b_[rigidbody->id] = take_ownership; return OkStatus();
  }
  int AddParametersToProblem(Problem& problem) {  // world_model.cpp:40-77
    int n = 0;
    for (auto& [_, l] : landmarks_) {
      problem.AddParameterBlock(l->point.data(), 3); n += 3;
      if (l->point_is_constant) problem.SetParameterBlockConstant(l->point.data());
    }
    for (auto& [_, b] : bodies_) {
      for (auto& [__, p] : b->model_definition) { problem.AddParameterBlock(p.data(), 3); n += 3; }
      n += utils::AddPoseToProblem(problem, b->T_world_rigidbody);
      if (b->model_definition_is_constant) for (auto& [__, p] : b->model_definition) problem.SetParameterBlockConstant(p.data());
      if (b->world_pose_is_constant) utils::SetPoseConstantInProblem(problem, b->T_world_rigidbody);
    }
    problem.AddParameterBlock(gravity_.data(), 3); n += 3;
    if (!gravity_enabled_) problem.SetParameterBlockConstant(gravity_.data());
    return n;
  }
  std::map<int, Landmark*>& landmarks() { return landmarks_; }
  const std::map<int, Landmark*>& landmarks() const { return landmarks_; }
  std::map<int, RigidBody*>& rigidbodies() { return bodies_; }
  const std::map<int, RigidBody*>& rigidbodies() const { return bodies_; }
  void EnableGravityEstimation(bool) { /* a no-op in the reference too (world_model.cpp:79-81, quirk Q6) */ }
  Vector3d& gravity() { return gravity_; }
  const Vector3d& gravity() const { return gravity_; }
  void SetGravity(const Vector3d& g) { gravity_ = g; }
  const Vector3d& GetGravity() const { return gravity_; }
  int NumberOfLandmarks() const { return int(landmarks_.size()); }
  int NumberOfRigidBodies() const { return int(bodies_.size()); }
  void ClearLandmarks() { for (auto& [id, l] : landmarks_) if (own_l_[id]) delete l; landmarks_.clear(); own_l_.clear(); }
  void ClearRigidBodies() { for (auto& [id, b] : bodies_) if (own_b_[id]) delete b; bodies_.clear(); own_b_.clear(); }
  void Clear() { ClearLandmarks(); ClearRigidBodies(); }
 private:
  std::map<int, Landmark*> landmarks_;
  std::map<int, RigidBody*> bodies_;
  std::map<int, bool> own_l_, own_b_;
  Vector3d gravity_;
  bool gravity_enabled_ = false;
};

// ---------------------------------------------------------------------------
// Sensors (sensor_base.h, camera.{h,cpp}, gyroscope.{h,cpp}, accelerometer.{h,cpp})
// ---------------------------------------------------------------------------
namespace sensors {

enum class CameraIntrinsicsModel : int { kNone = 0, kOpenCv5, kOpenCv8, kKannalaBrandt, kDoubleSphere, kFieldOfView, kUnifiedCamera, kExtendedUnifiedCamera };
enum class GyroscopeIntrinsicsModel : int { kNone = 0, kGyroscopeScaleOnly, kGyroscopeScaleAndBias, kGyroscopeVectorNav };
enum class AccelerometerIntrinsicsModel : int { kNone = 0, kAccelerometerScaleOnly, kAccelerometerScaleAndBias, kAccelerometerVectorNav };
inline int NumberOfParameters(CameraIntrinsicsModel m) { static const int k[] = {-1, 8, 11, 7, 5, 4, 4, 5}; return k[int(m)]; }
inline int NumberOfImuParameters(int m) { return m == 1 ? 1 : (m == 2 ? 4 : (m == 3 ? 12 : -1)); }

/// sensor_base.h:22-102 — the plugin contract consumed by BatchOptimizer.
class Sensor {
 public:
  virtual ~Sensor() = default;
  virtual void SetName(const std::string& name) = 0;
  virtual const std::string& GetName() const = 0;
  virtual void SetExtrinsics(const Pose3d& T_sensorrig_sensor) = 0;
  virtual const Pose3d& GetExtrinsics() const = 0;
  virtual Status SetIntrinsics(const VectorXd& intrinsics) = 0;
  virtual const VectorXd& GetIntrinsics() const = 0;
  virtual Status SetLatency(double latency) = 0;
  virtual double GetLatency() const = 0;
  virtual void EnableExtrinsicsEstimation(bool enable) = 0;
  virtual void EnableIntrinsicsEstimation(bool enable) = 0;
  virtual void EnableLatencyEstimation(bool enable) = 0;
  virtual Status UpdateResiduals(Problem& problem) = 0;
  virtual void ClearResidualInfo() = 0;
  virtual void SetLossFunction(utils::LossFunctionType loss, double scale = 1.0) = 0;
  virtual StatusOr<int> AddParametersToProblem(Problem& problem) = 0;
  virtual StatusOr<int> AddResidualsToProblem(Problem& problem, Trajectory& sensorrig_trajectory, WorldModel& world_model) = 0;
  virtual Status SetMeasurementNoise(double sigma) = 0;
};

// Shared state/behaviour of the three sensors. The reference leaves the three enable flags and the
// loss type uninitialised (quirk Q1); here they default to false / kNone.
class SensorCommon : public Sensor {
 public:
  void SetName(const std::string& name) final { name_ = name; }
  const std::string& GetName() const final { return name_; }
  void SetExtrinsics(const Pose3d& T) final { T_sensorrig_sensor_ = T; }
  const Pose3d& GetExtrinsics() const final { return T_sensorrig_sensor_; }
  const VectorXd& GetIntrinsics() const final { return intrinsics_; }
  Status SetLatency(double latency) final { latency_ = latency; return OkStatus(); }
  double GetLatency() const final { return latency_; }
  const double* LatencyData() const { return &latency_; }      // (the parameter block's address: Covariance's key)
  void EnableExtrinsicsEstimation(bool e) final { extrinsics_enabled_ = e; }
  void EnableIntrinsicsEstimation(bool e) final { intrinsics_enabled_ = e; }
  void EnableLatencyEstimation(bool e) final { latency_enabled_ = e; }
  void SetLossFunction(utils::LossFunctionType loss, double scale = 1.0) final { loss_function_ = loss; loss_scale_ = scale; }
  Status SetMeasurementNoise(double sigma) final {  // camera.cpp:62-68
    if (sigma <= 0.0) return InvalidArgumentError("Sigma must be greater than 0.");
    sigma_ = sigma; return OkStatus();
  }
  double GetMeasurementNoise() const { return sigma_; }
  /// index of this sensor in the Problem it last added its residuals to (-1: none yet): Covariance::Predictions
  int ProblemSensor() const { return problem_sensor_; }
 protected:
  // camera.cpp:92-113 / gyroscope.cpp:10-31 / accelerometer.cpp:10-33
  StatusOr<int> AddCommonParameters(Problem& problem, bool model_set, const char* what) {
    if (!model_set) return FailedPreconditionError(std::string("Cannot add ") + what + " parameters. Model is not yet defined.");
    int n = 0;
    problem.AddParameterBlock(intrinsics_.data(), int(intrinsics_.size())); n += int(intrinsics_.size());
    n += utils::AddPoseToProblem(problem, T_sensorrig_sensor_);
    problem.AddParameterBlock(&latency_, 1); ++n;
    if (!intrinsics_enabled_) problem.SetParameterBlockConstant(intrinsics_.data());
    if (!extrinsics_enabled_) utils::SetPoseConstantInProblem(problem, T_sensorrig_sensor_);
    if (!latency_enabled_) problem.SetParameterBlockConstant(&latency_);
    return n;
  }
  std::string name_;
  bool intrinsics_enabled_ = false, extrinsics_enabled_ = false, latency_enabled_ = false;
  Pose3d T_sensorrig_sensor_;
  VectorXd intrinsics_;
  double latency_ = 0.0, sigma_ = 1.0;
  utils::LossFunctionType loss_function_ = utils::LossFunctionType::kNone;
  double loss_scale_ = 1.0;
  int problem_sensor_ = -1;
};

/// camera.h:24-58
struct CameraObservationId {
  double stamp; int image_id; int model_id; int feature_id;
  bool operator==(const CameraObservationId& o) const { return stamp == o.stamp && image_id == o.image_id && model_id == o.model_id && feature_id == o.feature_id; }
};
struct CameraObservationIdHash {
  size_t operator()(const CameraObservationId& id) const {
    size_t h = std::hash<double>()(id.stamp);
    for (int v : {id.image_id, id.model_id, id.feature_id}) h = h * 1000003u ^ std::hash<int>()(v);
    return h;
  }
};
struct CameraMeasurement { Vector2d pixel; CameraObservationId id; };

namespace detail {
/// What ResectChart and CalibrateFromChart check and pack alike (px, pt: 2 and 3 doubles per pair; a free_mask has K entries).
inline Status PackChartBatch(const std::string& what, const std::vector<int64_t>& frame_offsets, const std::vector<Vector2d>& pixels,
                             const std::vector<Vector3d>& points, const std::vector<double>* q_init, const std::vector<double>* t_init,
                             size_t mask_size, size_t K, std::vector<double>* px, std::vector<double>* pt) {
  const size_t nf = frame_offsets.size() - 1, n = pixels.size();
  if (frame_offsets.empty() || n != points.size() || frame_offsets.back() != int64_t(n))
    return InvalidArgumentError(what + ": frame_offsets must have n_frames + 1 entries and end at the number of pairs");
  if ((q_init && q_init->size() != 4 * nf) || (t_init && t_init->size() != 3 * nf))
    return InvalidArgumentError(what + ": q_init / t_init must hold 4 / 3 doubles per frame");
  if (mask_size != 0 && mask_size != K) return InvalidArgumentError(what + ": free_mask must have one entry per intrinsic");
  for (size_t i = 0; i < n; ++i) {
    px->insert(px->end(), {pixels[i].x(), pixels[i].y()});
    pt->insert(pt->end(), {points[i][0], points[i][1], points[i][2]});
  }
  return OkStatus();
}
}  // namespace detail

/// What CalibrateRigFromChart and CalibrateRig leave (calico_rig_calibrate): per camera T_rig_camera as q (x, y, z, w) and t with
/// its status (CALICO_RIG_CAMERA_*), per rig frame T_rig_chart with its status (CALICO_RIG_FRAME_*), per view -- in the order
/// the views were given -- the RMS pixel residual, the pairs used and the status (CALICO_RESECT_*), on request the 6 C x 6 C
/// covariance of the extrinsics, and the summary (status: CALICO_RIG_*).
struct RigCalibration {
  std::vector<double> q_rig_camera, t_rig_camera;      // 4 and 3 doubles per camera
  std::vector<uint8_t> camera_status;
  std::vector<double> q_frame, t_frame;                // 4 and 3 doubles per rig frame
  std::vector<uint8_t> frame_status;
  std::vector<double> view_rms, cov;
  std::vector<int32_t> view_n_used;
  std::vector<uint8_t> view_status;
  calico_rig_summary summary{};
  size_t NumCameras() const { return camera_status.size(); }
  size_t NumFrames() const { return frame_status.size(); }
  size_t NumViews() const { return view_status.size(); }
  bool Ok() const { return summary.status == CALICO_RIG_OK; }
  Pose3d CameraPose(size_t c) const {
    return Pose3d(Quaterniond(q_rig_camera[4 * c + 3], q_rig_camera[4 * c], q_rig_camera[4 * c + 1], q_rig_camera[4 * c + 2]),
                  Vector3d(t_rig_camera[3 * c], t_rig_camera[3 * c + 1], t_rig_camera[3 * c + 2]));
  }
  Pose3d FramePose(size_t f) const {
    return Pose3d(Quaterniond(q_frame[4 * f + 3], q_frame[4 * f], q_frame[4 * f + 1], q_frame[4 * f + 2]),
                  Vector3d(t_frame[3 * f], t_frame[3 * f + 1], t_frame[3 * f + 2]));
  }
};

/// sensors::CameraModel (camera_models.h): the inverse model, on the device (calico_camera_unproject). The result is the
/// UNIT-NORM point that projects to the pixel under the library's projection -- the usual bearing for every model but
/// ExtendedUnified, whose projection is not scale invariant (include/calico_hip.h). A model is named by its enum value:
/// there are no model objects here.
class CameraModel {
 public:
  /// UnprojectPixels for n pixels: bearings[i] and valid[i] (0 with a zero vector where the pixel does not unproject)
  static Status UnprojectPixels(CameraIntrinsicsModel model, const VectorXd& intrinsics, const std::vector<Vector2d>& pixels,
                                std::vector<Vector3d>* bearings, std::vector<uint8_t>* valid, int device = 0) {
    const size_t n = pixels.size();
    std::vector<double> px(2 * n), b(3 * n);
    for (size_t i = 0; i < n; ++i) { px[2 * i] = pixels[i].x(); px[2 * i + 1] = pixels[i].y(); }
    std::vector<uint8_t> v(n, 0);
    const int st = calico_camera_unproject(device, int(model), intrinsics.data(), int(intrinsics.size()), int64_t(n), px.data(), b.data(), v.data());
    if (st != CALICO_OK) return Status(static_cast<StatusCode>(st), calico_last_error(nullptr));
    if (bearings) {
      bearings->resize(n);
      for (size_t i = 0; i < n; ++i) (*bearings)[i] = Vector3d(b[3 * i], b[3 * i + 1], b[3 * i + 2]);
    }
    if (valid) valid->swap(v);
    return OkStatus();
  }
  /// CameraModel::UnprojectPixel(intrinsics, pixel): kInvalidArgument for a pixel no point of the model's domain projects to
  static StatusOr<Vector3d> UnprojectPixel(CameraIntrinsicsModel model, const VectorXd& intrinsics, const Vector2d& pixel, int device = 0) {
    std::vector<Vector3d> b;
    std::vector<uint8_t> v;
    if (Status st = UnprojectPixels(model, intrinsics, {pixel}, &b, &v, device); !st.ok()) return st;
    if (!v[0]) return InvalidArgumentError("pixel (" + std::to_string(pixel.x()) + ", " + std::to_string(pixel.y()) + ") does not unproject");
    return b[0];
  }

  /// What ResectChart leaves, frame by frame (calico_camera_resect): T_camera_chart as q (x, y, z, w) and t, the RMS pixel
  /// residual, the pairs used, the steps tried, the status (CALICO_RESECT_*) and, on request, (J^T W J)^-1 in [delta_rot, t].
  struct ChartResection {
    std::vector<double> q, t, rms, cov;      // 4, 3, 1 and (with covariance) 36 doubles per frame
    std::vector<int32_t> n_used, iterations;
    std::vector<uint8_t> status;
    size_t NumFrames() const { return status.size(); }
    bool Ok(size_t frame) const { return status[frame] == CALICO_RESECT_OK; }
  };
  /// Chart resection over arrays, on the device: frame f owns the pairs [frame_offsets[f], frame_offsets[f + 1]) of pixels and
  /// chart points. q_init / t_init (4 and 3 doubles per frame): both or neither (neither: the homography start of a planar
  /// chart). options == nullptr: the library's defaults.
  static Status ResectChart(CameraIntrinsicsModel model, const VectorXd& intrinsics, const std::vector<int64_t>& frame_offsets,
                            const std::vector<Vector2d>& pixels, const std::vector<Vector3d>& points, const calico_resection_options* options,
                            ChartResection* out, bool covariance = false, const std::vector<double>* q_init = nullptr,
                            const std::vector<double>* t_init = nullptr, int device = 0) {
    if (!out) return InvalidArgumentError("ResectChart: null output");
    std::vector<double> px, pt;
    if (Status st = detail::PackChartBatch("ResectChart", frame_offsets, pixels, points, q_init, t_init, 0, 0, &px, &pt); !st.ok()) return st;
    const size_t nf = frame_offsets.size() - 1;
    ChartResection r;
    r.q.assign(4 * nf, 0.0); r.t.assign(3 * nf, 0.0); r.rms.assign(nf, 0.0); r.n_used.assign(nf, 0); r.iterations.assign(nf, 0);
    r.status.assign(nf, 0);
    if (covariance) r.cov.assign(36 * nf, 0.0);
    const int st = calico_camera_resect(device, int(model), intrinsics.data(), int(intrinsics.size()), int64_t(nf), frame_offsets.data(), px.data(),
                                        pt.data(), q_init ? q_init->data() : nullptr, t_init ? t_init->data() : nullptr, options, r.q.data(),
                                        r.t.data(), r.rms.data(), r.n_used.data(), r.iterations.data(), r.status.data(),
                                        covariance ? r.cov.data() : nullptr);
    if (st != CALICO_OK) return Status(static_cast<StatusCode>(st), calico_last_error(nullptr));
    *out = std::move(r);
    return OkStatus();
  }

  /// What CalibrateFromChart leaves (calico_camera_calibrate): the intrinsics, per frame T_camera_chart as q (x, y, z, w) and t,
  /// the RMS pixel residual, the pairs used and the status (CALICO_RESECT_*), on request the K x K covariance of the intrinsics,
  /// and the summary (status: CALICO_CALIB_*).
  struct ChartCalibration {
    VectorXd intrinsics;
    std::vector<double> q, t, rms, cov;      // 4, 3 and 1 doubles per frame; (with covariance) K x K
    std::vector<int32_t> n_used;
    std::vector<uint8_t> status;
    calico_calibration_summary summary{};
    size_t NumFrames() const { return status.size(); }
    bool Ok() const { return summary.status == CALICO_CALIB_OK; }
    bool Used(size_t frame) const { return status[frame] == CALICO_RESECT_OK; }
  };
  /// Intrinsic calibration over arrays, on the device: the intrinsics of `model` from `intrinsics_init`, jointly with the pose of
  /// every frame. Frames as in ResectChart. free_mask (K entries, 0 = constant) may be empty: all free. q_init / t_init: both or
  /// neither (neither: every frame is resected at intrinsics_init). options == nullptr: the library's defaults.
  static Status CalibrateFromChart(CameraIntrinsicsModel model, const VectorXd& intrinsics_init, const std::vector<int64_t>& frame_offsets,
                                   const std::vector<Vector2d>& pixels, const std::vector<Vector3d>& points,
                                   const calico_calibration_options* options, ChartCalibration* out, bool covariance = false,
                                   const std::vector<uint8_t>& free_mask = {}, const std::vector<double>* q_init = nullptr,
                                   const std::vector<double>* t_init = nullptr, int device = 0) {
    if (!out) return InvalidArgumentError("CalibrateFromChart: null output");
    const size_t nf = frame_offsets.size() - 1, K = size_t(intrinsics_init.size());
    std::vector<double> px, pt;
    if (Status st = detail::PackChartBatch("CalibrateFromChart", frame_offsets, pixels, points, q_init, t_init, free_mask.size(), K, &px, &pt); !st.ok())
      return st;
    ChartCalibration r;
    r.intrinsics = intrinsics_init;
    r.q.assign(4 * nf, 0.0); r.t.assign(3 * nf, 0.0); r.rms.assign(nf, 0.0); r.n_used.assign(nf, 0); r.status.assign(nf, 0);
    for (size_t f = 0; f < nf; ++f) r.q[4 * f + 3] = 1.0;
    if (covariance) r.cov.assign(K * K, 0.0);
    const int st = calico_camera_calibrate(device, int(model), intrinsics_init.data(), int(K), free_mask.empty() ? nullptr : free_mask.data(),
                                           int64_t(nf), frame_offsets.data(), px.data(), pt.data(), q_init ? q_init->data() : nullptr,
                                           t_init ? t_init->data() : nullptr, options, r.intrinsics.data(), r.q.data(), r.t.data(),
                                           r.rms.data(), r.n_used.data(), r.status.data(), covariance ? r.cov.data() : nullptr, &r.summary);
    if (st != CALICO_OK) return Status(static_cast<StatusCode>(st), calico_last_error(nullptr));
    *out = std::move(r);
    return OkStatus();
  }

  /// Rig calibration over arrays, on the device (calico_rig_calibrate): the extrinsics T_rig_camera of cameras of the given
  /// models and intrinsics and the pose T_rig_chart of each of n_frames rig frames. View v is camera view_camera[v] in rig frame
  /// view_frame[v] and owns the pairs [view_offsets[v], view_offsets[v + 1]) of pixels and chart points. The starts (4 and 3
  /// doubles per camera / per frame) come in pairs, the frames' only with the cameras'; none: every view is resected and the
  /// cameras are chained through the frames they share. options == nullptr: the library's defaults.
  static Status CalibrateRigFromChart(const std::vector<CameraIntrinsicsModel>& models, const std::vector<VectorXd>& intrinsics, int64_t n_frames,
                                      const std::vector<int32_t>& view_camera, const std::vector<int64_t>& view_frame,
                                      const std::vector<int64_t>& view_offsets, const std::vector<Vector2d>& pixels,
                                      const std::vector<Vector3d>& points, const calico_rig_options* options, RigCalibration* out,
                                      bool covariance = false, const std::vector<double>* q_rig_camera_init = nullptr,
                                      const std::vector<double>* t_rig_camera_init = nullptr, const std::vector<double>* q_frame_init = nullptr,
                                      const std::vector<double>* t_frame_init = nullptr, int device = 0) {
    const std::string what = "CalibrateRigFromChart";
    if (!out) return InvalidArgumentError(what + ": null output");
    const size_t nc = models.size(), nv = view_camera.size(), nf = size_t(std::max<int64_t>(n_frames, 0));
    if (intrinsics.size() != nc) return InvalidArgumentError(what + ": one intrinsics vector per camera");
    if (view_frame.size() != nv || view_offsets.size() != nv + 1)
      return InvalidArgumentError(what + ": view_camera and view_frame have one entry per view, view_offsets one more");
    if ((q_rig_camera_init && q_rig_camera_init->size() != 4 * nc) || (t_rig_camera_init && t_rig_camera_init->size() != 3 * nc))
      return InvalidArgumentError(what + ": q_rig_camera_init / t_rig_camera_init must hold 4 / 3 doubles per camera");
    // (the views' offsets as frame offsets: the same rule, that they end at the number of pairs)
    std::vector<double> px, pt;
    if (Status st = detail::PackChartBatch(what, view_offsets, pixels, points, nullptr, nullptr, 0, 0, &px, &pt); !st.ok()) return st;
    if ((q_frame_init && q_frame_init->size() != 4 * nf) || (t_frame_init && t_frame_init->size() != 3 * nf))
      return InvalidArgumentError(what + ": q_frame_init / t_frame_init must hold 4 / 3 doubles per frame");
    std::vector<int32_t> md(nc);
    std::vector<int64_t> koff(nc + 1, 0);
    std::vector<double> k;
    for (size_t c = 0; c < nc; ++c) {
      md[c] = int32_t(models[c]);
      k.insert(k.end(), intrinsics[c].begin(), intrinsics[c].end());
      koff[c + 1] = int64_t(k.size());
    }
    RigCalibration r;
    r.q_rig_camera.assign(4 * nc, 0.0); r.t_rig_camera.assign(3 * nc, 0.0); r.camera_status.assign(nc, 0);
    r.q_frame.assign(4 * nf, 0.0); r.t_frame.assign(3 * nf, 0.0); r.frame_status.assign(nf, 0);
    r.view_rms.assign(nv, 0.0); r.view_n_used.assign(nv, 0); r.view_status.assign(nv, 0);
    if (covariance) r.cov.assign(36 * nc * nc, 0.0);
    const auto ptr = [](const std::vector<double>* v) { return v ? v->data() : nullptr; };
    const int st = calico_rig_calibrate(device, int32_t(nc), md.data(), koff.data(), k.data(), n_frames, int64_t(nv), view_camera.data(),
                                        view_frame.data(), view_offsets.data(), px.data(), pt.data(), ptr(q_rig_camera_init),
                                        ptr(t_rig_camera_init), ptr(q_frame_init), ptr(t_frame_init), options, r.q_rig_camera.data(),
                                        r.t_rig_camera.data(), r.camera_status.data(), r.q_frame.data(), r.t_frame.data(),
                                        r.frame_status.data(), r.view_rms.data(), r.view_n_used.data(), r.view_status.data(),
                                        covariance ? r.cov.data() : nullptr, &r.summary);
    if (st != CALICO_OK) return Status(static_cast<StatusCode>(st), calico_last_error(nullptr));
    *out = std::move(r);
    return OkStatus();
  }
};

inline bool ProjectPointHost(CameraIntrinsicsModel model, const double* k, const cal::V3& p, double pix[2]) {
  double D[2][3], dK[2][cal::kMaxIntr];
  switch (int(model)) {
    case 1: return cal::project<1, false>(k, p, pix, D, dK);
    case 2: return cal::project<2, false>(k, p, pix, D, dK);
    case 3: return cal::project<3, false>(k, p, pix, D, dK);
    case 4: return cal::project<4, false>(k, p, pix, D, dK);
    case 5: return cal::project<5, false>(k, p, pix, D, dK);
    case 6: return cal::project<6, false>(k, p, pix, D, dK);
    case 7: return cal::project<7, false>(k, p, pix, D, dK);
    default: return false;
  }
}

class Camera : public SensorCommon {
 public:
  Camera() = default;
  Camera(const Camera&) = delete;
  Camera& operator=(const Camera&) = delete;
  Status SetIntrinsics(const VectorXd& intrinsics) final {  // camera.cpp:24-37
    if (model_ == CameraIntrinsicsModel::kNone) return InvalidArgumentError("Camera model has not been set!");
    if (int(intrinsics.size()) != NumberOfParameters(model_))
      return InvalidArgumentError("Tried to set intrinsics of size " + std::to_string(intrinsics.size()) + " for camera " + GetName() +
                                  ". Expected intrinsics size of " + std::to_string(NumberOfParameters(model_)));
    intrinsics_ = intrinsics; return OkStatus();
  }
  Status SetModel(CameraIntrinsicsModel m) {  // camera.cpp:210-219
    if (int(m) < 1 || int(m) > 7) return InvalidArgumentError("Could not create camera model for type " + std::to_string(int(m)) + ". It is likely not yet implemented.");
    model_ = m; intrinsics_.assign(size_t(NumberOfParameters(m)), 0.0); return OkStatus();
  }
  CameraIntrinsicsModel GetModel() const { return model_; }
  /// CameraModel::UnprojectPixels at this camera's current intrinsics (after Optimize: the estimates, written back in place).
  /// The handle-free call with the host's copy of the intrinsics: the facade keeps no handle between calls; a caller that
  /// holds one uses calico_sensor_unproject, which gives the same bits.
  Status UnprojectPixels(const std::vector<Vector2d>& pixels, std::vector<Vector3d>* bearings, std::vector<uint8_t>* valid, int device = 0) const {
    if (model_ == CameraIntrinsicsModel::kNone) return FailedPreconditionError("Camera model has not been set!");
    return CameraModel::UnprojectPixels(model_, intrinsics_, pixels, bearings, valid, device);
  }
  /// Where this camera was when each frame of a chart was detected: CameraModel::ResectChart with this camera's model and
  /// current intrinsics. frames[f] maps a feature id to its pixel, model_definition a feature id to its chart point; the
  /// pairs of a frame are taken in ascending id order. A detected id the model does not define is an argument error.
  Status EstimateChartPoses(const std::vector<std::map<int, Vector2d>>& frames, const std::map<int, Vector3d>& model_definition,
                            const calico_resection_options* options, CameraModel::ChartResection* out, bool covariance = false,
                            int device = 0) const {
    if (model_ == CameraIntrinsicsModel::kNone) return FailedPreconditionError("Camera model has not been set!");
    std::vector<int64_t> offsets(1, 0);
    std::vector<Vector2d> pixels;
    std::vector<Vector3d> points;
    for (const auto& frame : frames) {
      for (const auto& kv : frame) {
        const auto it = model_definition.find(kv.first);
        if (it == model_definition.end()) return InvalidArgumentError("EstimateChartPoses: feature " + std::to_string(kv.first) + " is not in the model definition");
        pixels.push_back(kv.second);
        points.push_back(it->second);
      }
      offsets.push_back(int64_t(pixels.size()));
    }
    return CameraModel::ResectChart(model_, intrinsics_, offsets, pixels, points, options, out, covariance, nullptr, nullptr, device);
  }
  /// Static intrinsic calibration of this camera from chart detections: CameraModel::CalibrateFromChart with this camera's model,
  /// started at its current intrinsics (a rough start: utils.InitialIntrinsics) and, unless q_init / t_init are given, at the
  /// resection of every frame there. Frames and model_definition as in EstimateChartPoses. When the estimation ends with
  /// CALICO_CALIB_OK or CALICO_CALIB_NOT_CONVERGED the camera's intrinsics are set to the estimate; `out` holds the poses and the
  /// per-frame statuses either way.
  Status CalibrateIntrinsics(const std::vector<std::map<int, Vector2d>>& frames, const std::map<int, Vector3d>& model_definition,
                             const calico_calibration_options* options, CameraModel::ChartCalibration* out, bool covariance = false,
                             const std::vector<uint8_t>& free_mask = {}, const std::vector<double>* q_init = nullptr,
                             const std::vector<double>* t_init = nullptr, int device = 0) {
    if (model_ == CameraIntrinsicsModel::kNone) return FailedPreconditionError("Camera model has not been set!");
    if (!out) return InvalidArgumentError("CalibrateIntrinsics: null output");
    std::vector<int64_t> offsets(1, 0);
    std::vector<Vector2d> pixels;
    std::vector<Vector3d> points;
    for (const auto& frame : frames) {
      for (const auto& kv : frame) {
        const auto it = model_definition.find(kv.first);
        if (it == model_definition.end()) return InvalidArgumentError("CalibrateIntrinsics: feature " + std::to_string(kv.first) + " is not in the model definition");
        pixels.push_back(kv.second);
        points.push_back(it->second);
      }
      offsets.push_back(int64_t(pixels.size()));
    }
    if (Status st = CameraModel::CalibrateFromChart(model_, intrinsics_, offsets, pixels, points, options, out, covariance, free_mask, q_init,
                                                    t_init, device); !st.ok()) return st;
    if (!frames.empty() && (out->summary.status == CALICO_CALIB_OK || out->summary.status == CALICO_CALIB_NOT_CONVERGED)) intrinsics_ = out->intrinsics;
    return OkStatus();
  }
  StatusOr<int> AddParametersToProblem(Problem& problem) final {
    return AddCommonParameters(problem, model_ != CameraIntrinsicsModel::kNone, "camera");
  }
  /// camera.cpp:115-153
  StatusOr<int> AddResidualsToProblem(Problem& problem, Trajectory& sensorrig_trajectory, WorldModel& world_model) final {
    (void)sensorrig_trajectory;
    problem_sensor_ = problem.AddSensor(CALICO_SENSOR_CAMERA, int(model_), intrinsics_.data(), T_sensorrig_sensor_.rotation().coeffs().data(),
                                        T_sensorrig_sensor_.translation().data(), &latency_, nullptr, sigma_, int(loss_function_), loss_scale_);
    int added = 0;
    residual_order_.clear();
    for (const auto& [observation_id, measurement] : id_to_measurement_) {
      if (outlier_ids_.count(observation_id)) continue;
      const int rigidbody_id = observation_id.model_id;
      if (!world_model.rigidbodies().count(rigidbody_id))
        return FailedPreconditionError("Attempted to create cost function from an observation for a rigidbody with id " +
                                       std::to_string(rigidbody_id) + " that does not exist in the world model.");
      RigidBody* body = world_model.rigidbodies().at(rigidbody_id);
      Vector3d& t_model_point = body->model_definition.at(observation_id.feature_id);  // throws like the reference (camera.cpp:135)
      problem.AddCameraResidual(problem_sensor_, measurement.pixel, observation_id.stamp, t_model_point.data(),
                                body->T_world_rigidbody.rotation().coeffs().data(), body->T_world_rigidbody.translation().data());
      residual_order_.push_back(observation_id);
      ++added;
    }
    return added;
  }
  Status UpdateResiduals(Problem& problem) final {  // camera.cpp:70-80
    std::vector<double> r; std::vector<uint8_t> valid;
    const Status st = problem.EvaluateResiduals(problem_sensor_, &r, &valid);
    if (!st.ok()) return InternalError("Failed to update residual for camera " + name_);
    for (size_t i = 0; i < residual_order_.size(); ++i) id_to_residual_[residual_order_[i]] = Vector2d(r[2 * i], r[2 * i + 1]);
    return OkStatus();
  }
  void ClearResidualInfo() final { residual_order_.clear(); id_to_residual_.clear(); }
  /// camera.cpp:155-208
  StatusOr<std::vector<CameraMeasurement>> Project(const std::vector<double>& interp_times, const Trajectory& sensorrig_trajectory,
                                                   const WorldModel& world_model) const {
    auto poses = sensorrig_trajectory.Interpolate(interp_times);
    if (!poses.ok()) return poses.status();
    std::vector<CameraMeasurement> out;
    int image_id = 0;
    for (size_t i = 0; i < interp_times.size(); ++i) {
      const Pose3d T_camera_world = ((*poses)[i] * T_sensorrig_sensor_).inverse();
      auto emit = [&](const Vector3d& pc, int model_id, int feature_id) {
        if (pc.z() <= 0) return;
        double pix[2] = {0, 0};
        ProjectPointHost(model_, intrinsics_.data(), cal::mk(pc[0], pc[1], pc[2]), pix);
        out.push_back({Vector2d(pix[0], pix[1]), {interp_times[i] + latency_, image_id, model_id, feature_id}});
      };
      for (const auto& [id, l] : world_model.landmarks()) emit(T_camera_world * l->point, kLandmarkFrameId, id);
      for (const auto& [bid, body] : world_model.rigidbodies()) {
        const Pose3d T_camera_body = T_camera_world * body->T_world_rigidbody;
        std::vector<int> keys;
        for (const auto& kv : body->model_definition) keys.push_back(kv.first);
        std::sort(keys.begin(), keys.end());
        for (int pid : keys) emit(T_camera_body * body->model_definition.at(pid), bid, pid);
      }
      ++image_id;
    }
    return out;
  }
  Status AddMeasurement(const CameraMeasurement& m) {  // camera.cpp:226-236
    if (id_to_measurement_.count(m.id))
      return InvalidArgumentError("Tried to add redundant measurement - Image id: " + std::to_string(m.id.image_id) + ", model id: " +
                                  std::to_string(m.id.model_id) + ", feature id: " + std::to_string(m.id.feature_id));
    id_to_measurement_[m.id] = m; return OkStatus();
  }
  Status AddMeasurements(const std::vector<CameraMeasurement>& ms) {  // camera.cpp:238-251 (Q11: unique ones are still added)
    std::string message;
    for (const auto& m : ms) { const Status st = AddMeasurement(m); if (!st.ok()) message += st.message() + "\n"; }
    return message.empty() ? OkStatus() : InvalidArgumentError(message);
  }
  const std::unordered_map<CameraObservationId, CameraMeasurement, CameraObservationIdHash>& GetMeasurementIdToMeasurement() const { return id_to_measurement_; }
  StatusOr<std::vector<std::pair<CameraMeasurement, Vector2d>>> GetMeasurementResidualPairs() const {  // camera.cpp:258-279
    if (id_to_residual_.size() > id_to_measurement_.size()) return InternalError("There are more residuals than measurements.");
    if (id_to_measurement_.empty()) return FailedPreconditionError("Measurements are empty. Nothing to return.");
    std::vector<std::pair<CameraMeasurement, Vector2d>> pairs;
    for (const auto& [id, r] : id_to_residual_) {
      auto it = id_to_measurement_.find(id);
      if (it == id_to_measurement_.end()) return InternalError("Found a residual that doesn't correspond to any measurement.");
      pairs.push_back({it->second, r});
    }
    return pairs;
  }
  Status MarkOutlierById(const CameraObservationId& id) {  // camera.cpp:281-290
    if (!id_to_measurement_.count(id)) return InvalidArgumentError("Attempted to add id that is not within the measurement set.");
    outlier_ids_.insert(id); return OkStatus();
  }
  Status MarkOutliersById(const std::vector<CameraObservationId>& ids) { for (const auto& id : ids) { const Status st = MarkOutlierById(id); if (!st.ok()) return st; } return OkStatus(); }
  void ClearOutliersList() { outlier_ids_.clear(); }
  bool IsOutlier(const CameraObservationId& id) const { return outlier_ids_.count(id) != 0; }
  void ClearMeasurements() { id_to_measurement_.clear(); residual_order_.clear(); id_to_residual_.clear(); outlier_ids_.clear(); }
  int NumberOfMeasurements() const { return int(id_to_measurement_.size()); }
 private:
  CameraIntrinsicsModel model_ = CameraIntrinsicsModel::kNone;
  std::unordered_map<CameraObservationId, CameraMeasurement, CameraObservationIdHash> id_to_measurement_;
  std::unordered_map<CameraObservationId, Vector2d, CameraObservationIdHash> id_to_residual_;
  std::vector<CameraObservationId> residual_order_;
  std::unordered_set<CameraObservationId, CameraObservationIdHash> outlier_ids_;
};

/// gyroscope.h:20-44 / accelerometer.h (same shape)
struct ImuObservationId {
  double stamp; int sequence;
  bool operator==(const ImuObservationId& o) const { return stamp == o.stamp && sequence == o.sequence; }
};
struct ImuObservationIdHash { size_t operator()(const ImuObservationId& id) const { return std::hash<double>()(id.stamp) * 1000003u ^ std::hash<int>()(id.sequence); } };
struct ImuMeasurement { Vector3d measurement; ImuObservationId id; };
using GyroscopeObservationId = ImuObservationId;
using GyroscopeMeasurement = ImuMeasurement;
using AccelerometerObservationId = ImuObservationId;
using AccelerometerMeasurement = ImuMeasurement;

/// What CharacterizeImuNoise returns: calico_imu_allan's outputs -- the grid of cluster sizes, the Allan variance of the three
/// axes at each of them (avar[j][axis]), the IEEE-952 coefficients per axis, and the summary with the pooled white-noise density.
struct ImuNoise {
  std::vector<int64_t> cluster_sizes;
  std::vector<double> tau, rel_err;
  std::vector<Vector3d> avar;
  std::array<calico_allan_noise, 3> axes{};
  calico_allan_summary summary{};
  /// The sigma SetMeasurementNoise takes for a recording of this sensor at rate_hz: N_pooled sqrt(rate_hz).
  double MeasurementSigma(double rate_hz) const { return summary.N_pooled * std::sqrt(rate_hz); }
};
inline calico_allan_options DefaultAllanOptions() { calico_allan_options o; calico_default_allan_options(&o); return o; }
/// The noise of a gyroscope or an accelerometer from a recording at rest (calico_imu_allan, on the device): stamps (n, evenly
/// spaced: a gap is kInvalidArgument) and samples (n). The fit's status per axis is in axes[i].status (CALICO_ALLAN_*).
inline StatusOr<ImuNoise> CharacterizeImuNoise(const std::vector<double>& stamps, const std::vector<Vector3d>& samples,
                                               const calico_allan_options& options = DefaultAllanOptions(), int device = 0) {
  static_assert(sizeof(Vector3d) == 3 * sizeof(double), "samples travel as n x 3 doubles");
  if (stamps.size() != samples.size()) return InvalidArgumentError("CharacterizeImuNoise: one stamp per sample");
  ImuNoise r;
  int32_t nc = 0;
  r.cluster_sizes.assign(CALICO_ALLAN_MAX_CLUSTERS, 0);
  r.tau.assign(CALICO_ALLAN_MAX_CLUSTERS, 0.0); r.rel_err.assign(CALICO_ALLAN_MAX_CLUSTERS, 0.0);
  r.avar.assign(CALICO_ALLAN_MAX_CLUSTERS, Vector3d());
  const int st = calico_imu_allan(device, int64_t(samples.size()), stamps.empty() ? nullptr : stamps.data(), 0.0,
                                  samples.empty() ? nullptr : samples[0].data(), &options, &nc, r.cluster_sizes.data(), r.tau.data(),
                                  r.avar[0].data(), r.rel_err.data(), r.axes.data(), &r.summary);
  if (st != CALICO_OK) return Status(static_cast<StatusCode>(st), calico_last_error(nullptr));
  r.cluster_sizes.resize(size_t(nc)); r.tau.resize(size_t(nc)); r.rel_err.resize(size_t(nc)); r.avar.resize(size_t(nc));
  return r;
}

template <int KIND>
class ImuSensor : public SensorCommon {
 public:
  Status SetIntrinsics(const VectorXd& intrinsics) final {
    if (model_ == 0) return InvalidArgumentError("Model has not been set!");
    if (int(intrinsics.size()) != NumberOfImuParameters(model_))
      return InvalidArgumentError("Tried to set intrinsics of size " + std::to_string(intrinsics.size()) + " for sensor " + GetName() +
                                  ". Expected intrinsics size of " + std::to_string(NumberOfImuParameters(model_)));
    intrinsics_ = intrinsics; return OkStatus();
  }
  StatusOr<int> AddParametersToProblem(Problem& problem) final { return AddCommonParameters(problem, model_ != 0, KIND == CALICO_SENSOR_GYROSCOPE ? "gyroscope" : "accelerometer"); }
  /// gyroscope.cpp:33-54 / accelerometer.cpp:35-56
  StatusOr<int> AddResidualsToProblem(Problem& problem, Trajectory&, WorldModel& world_model) final {
    problem_sensor_ = problem.AddSensor(KIND, model_, intrinsics_.data(), T_sensorrig_sensor_.rotation().coeffs().data(),
                                        T_sensorrig_sensor_.translation().data(), &latency_,
                                        KIND == CALICO_SENSOR_ACCELEROMETER ? world_model.gravity().data() : nullptr, sigma_,
                                        int(loss_function_), loss_scale_);
    residual_order_.clear();
    for (const auto& [id, m] : id_to_measurement_) { problem.AddImuResidual(problem_sensor_, m.measurement, id.stamp); residual_order_.push_back(id); }
    return int(residual_order_.size());
  }
  Status UpdateResiduals(Problem& problem) final {
    std::vector<double> r; std::vector<uint8_t> valid;
    const Status st = problem.EvaluateResiduals(problem_sensor_, &r, &valid);
    if (!st.ok()) return InternalError("Failed to update residual for sensor " + name_);
    for (size_t i = 0; i < residual_order_.size(); ++i) id_to_residual_[residual_order_[i]] = Vector3d(r[3 * i], r[3 * i + 1], r[3 * i + 2]);
    return OkStatus();
  }
  void ClearResidualInfo() final { residual_order_.clear(); id_to_residual_.clear(); }
  Status AddMeasurement(const ImuMeasurement& m) {
    if (id_to_measurement_.count(m.id))
      return InvalidArgumentError("Tried to add redundant measurement - Sequence: " + std::to_string(m.id.sequence) + ", stamp: " + std::to_string(m.id.stamp));
    id_to_measurement_[m.id] = m; return OkStatus();
  }
  Status AddMeasurements(const std::vector<ImuMeasurement>& ms) {
    std::string message;
    for (const auto& m : ms) { const Status st = AddMeasurement(m); if (!st.ok()) message += st.message() + "\n"; }
    return message.empty() ? OkStatus() : InvalidArgumentError(message);
  }
  void ClearMeasurements() { id_to_measurement_.clear(); }
  int NumberOfMeasurements() const { return int(id_to_measurement_.size()); }
  /// The registered measurements in time order (stamp, then sequence): stamps (n) and values (n x 3).
  void SortedMeasurements(std::vector<double>* stamps, std::vector<double>* values) const {
    std::vector<const ImuMeasurement*> order;
    order.reserve(id_to_measurement_.size());
    for (const auto& kv : id_to_measurement_) order.push_back(&kv.second);
    std::sort(order.begin(), order.end(), [](const ImuMeasurement* a, const ImuMeasurement* b) {
      return a->id.stamp != b->id.stamp ? a->id.stamp < b->id.stamp : a->id.sequence < b->id.sequence;
    });
    stamps->clear(); values->clear();
    for (const ImuMeasurement* m : order) {
      stamps->push_back(m->id.stamp);
      for (int i = 0; i < 3; ++i) values->push_back(m->measurement[i]);
    }
  }
  /// The rate of the registered measurements: (n - 1) / (last stamp - first stamp).
  StatusOr<double> MeasurementRate() const {
    if (id_to_measurement_.size() < 2) return FailedPreconditionError("Sensor " + name_ + " has fewer than two measurements: no rate.");
    double first = id_to_measurement_.begin()->first.stamp, last = first;
    for (const auto& kv : id_to_measurement_) { first = std::min(first, kv.first.stamp); last = std::max(last, kv.first.stamp); }
    if (!(last > first)) return FailedPreconditionError("The measurements of sensor " + name_ + " share one stamp: no rate.");
    return double(id_to_measurement_.size() - 1) / (last - first);
  }
  /// The sensor's sigma from a noise characterisation (CharacterizeImuNoise on a recording at rest) for measurements at rate_hz:
  /// SetMeasurementNoise(noise.MeasurementSigma(rate_hz)). The optimiser's sigma is one scalar per sensor: the pooled density.
  Status ApplyNoise(const ImuNoise& noise, double rate_hz) {
    if (!std::isfinite(rate_hz) || !(rate_hz > 0.0)) return InvalidArgumentError("ApplyNoise: rate_hz must be finite and > 0.");
    if (!(noise.summary.N_pooled > 0.0) || !std::isfinite(noise.summary.N_pooled))
      return InvalidArgumentError("ApplyNoise: the characterisation holds no white-noise density (N_pooled is not > 0).");
    return SetMeasurementNoise(noise.MeasurementSigma(rate_hz));
  }
  const std::unordered_map<ImuObservationId, Vector3d, ImuObservationIdHash>& residuals() const { return id_to_residual_; }
  /// gyroscope.cpp:56-82 / accelerometer.cpp:76-123
  StatusOr<std::vector<ImuMeasurement>> Project(const std::vector<double>& interp_times, const Trajectory& traj, const WorldModel& world_model) const {
    std::vector<ImuMeasurement> out(interp_times.size());
    const Quaterniond& q = T_sensorrig_sensor_.rotation();
    cal::Q4 qs; qs.x = q.x(); qs.y = q.y(); qs.z = q.z(); qs.w = q.w();
    const cal::M3 R_rs = cal::rotmat(cal::normalized(qs));
    for (size_t i = 0; i < interp_times.size(); ++i) {
      double p[6], pd[6], pdd[6];
      Status st = traj.spline().Evaluate(interp_times[i], 0, p); if (!st.ok()) return st;
      st = traj.spline().Evaluate(interp_times[i], 1, pd); if (!st.ok()) return st;
      const cal::V3 phi = cal::mk(-p[0], -p[1], -p[2]), phid = cal::mk(-pd[0], -pd[1], -pd[2]);
      const cal::Rodrigues<double> R = cal::rodrigues<double>(phi.x, phi.y, phi.z, true);
      cal::V3 omega; cal::rod_J_apply<double>(R, phid.x, phid.y, phid.z, &omega.x, &omega.y, &omega.z);
      cal::V3 in;
      if (KIND == CALICO_SENSOR_GYROSCOPE) {
        in = -cal::mulT(R_rs, omega);
      } else {
        st = traj.spline().Evaluate(interp_times[i], 2, pdd); if (!st.ok()) return st;
        const cal::V3 phidd = cal::mk(-pdd[0], -pdd[1], -pdd[2]);
        double jdd[3], Hv[3][3];
        cal::rod_J_apply<double>(R, phidd.x, phidd.y, phidd.z, &jdd[0], &jdd[1], &jdd[2]);
        cal::rod_H_apply<double>(R, phid.x, phid.y, phid.z, Hv);
        const cal::V3 alpha = cal::mk(phid.x * Hv[0][0] + phid.y * Hv[1][0] + phid.z * Hv[2][0] + jdd[0],
                                      phid.x * Hv[0][1] + phid.y * Hv[1][1] + phid.z * Hv[2][1] + jdd[1],
                                      phid.x * Hv[0][2] + phid.y * Hv[1][2] + phid.z * Hv[2][2] + jdd[2]);
        const cal::M3 R_rw = cal::rotmat(cal::angle_axis_to_quat(phi));
        const Vector3d& g = world_model.gravity();
        const Vector3d& tt = T_sensorrig_sensor_.translation();
        const cal::V3 t = cal::mk(tt[0], tt[1], tt[2]);
        const cal::V3 b = cal::mul(R_rw, cal::mk(pdd[3] - g[0], pdd[4] - g[1], pdd[5] - g[2])) + cal::cross(omega, cal::cross(omega, t)) - cal::cross(alpha, t);
        in = cal::mulT(R_rs, b);
      }
      double f[3], Mw[3][3], dK[3][cal::kMaxIntr];
      cal::imu_project<false>(model_, intrinsics_.data(), in, f, Mw, dK);
      out[i] = {Vector3d(f[0], f[1], f[2]), {interp_times[i] + latency_, int(i)}};
    }
    return out;
  }
 protected:
  Status SetModelInt(int m) {
    if (m < 1 || m > 3) return InvalidArgumentError("Could not create model for type " + std::to_string(m) + ". It is likely not yet implemented.");
    model_ = m; intrinsics_.assign(size_t(NumberOfImuParameters(m)), 0.0); return OkStatus();
  }
  int model_ = 0;
  std::unordered_map<ImuObservationId, ImuMeasurement, ImuObservationIdHash> id_to_measurement_;
  std::unordered_map<ImuObservationId, Vector3d, ImuObservationIdHash> id_to_residual_;
  std::vector<ImuObservationId> residual_order_;
};

class Gyroscope : public ImuSensor<CALICO_SENSOR_GYROSCOPE> {
 public:
  Status SetModel(GyroscopeIntrinsicsModel m) { return SetModelInt(int(m)); }
  GyroscopeIntrinsicsModel GetModel() const { return static_cast<GyroscopeIntrinsicsModel>(model_); }
};
class Accelerometer : public ImuSensor<CALICO_SENSOR_ACCELEROMETER> {
 public:
  Status SetModel(AccelerometerIntrinsicsModel m) { return SetModelInt(int(m)); }
  AccelerometerIntrinsicsModel GetModel() const { return static_cast<AccelerometerIntrinsicsModel>(model_); }
};

}  // namespace sensors

using RigCalibration = sensors::RigCalibration;

/// Rig calibration from chart detections (sensors::CameraModel::CalibrateRigFromChart with the cameras' models and current
/// intrinsics, no start given): rig_frames[f] maps a camera's index in `cameras` to its detections in rig frame f (feature id ->
/// pixel), model_definition a feature id to its chart point; the views are taken frame by frame in ascending camera index, a
/// view's pairs in ascending id. The rig's frame is that of the reference camera (options->reference_camera, 0 by default). The
/// extrinsics of every camera whose status is CALICO_RIG_CAMERA_OK are set (SetExtrinsics), and only when the estimation ended
/// with CALICO_RIG_OK; `out` (may be null) holds everything the call left either way. Returns T_rig_chart per rig frame (the
/// identity for a frame whose status is not CALICO_RIG_FRAME_OK).
inline StatusOr<std::vector<Pose3d>> CalibrateRig(const std::vector<sensors::Camera*>& cameras,
                                                  const std::vector<std::map<int, std::map<int, Vector2d>>>& rig_frames,
                                                  const std::map<int, Vector3d>& model_definition, const calico_rig_options* options = nullptr,
                                                  RigCalibration* out = nullptr, bool covariance = false, int device = 0) {
  std::vector<sensors::CameraIntrinsicsModel> models;
  std::vector<VectorXd> intrinsics;
  for (const sensors::Camera* camera : cameras) {
    if (!camera) return InvalidArgumentError("CalibrateRig: null camera");
    if (camera->GetModel() == sensors::CameraIntrinsicsModel::kNone) return FailedPreconditionError("Camera model has not been set!");
    models.push_back(camera->GetModel());
    intrinsics.push_back(camera->GetIntrinsics());
  }
  std::vector<int32_t> view_camera;
  std::vector<int64_t> view_frame, view_offsets(1, 0);
  std::vector<Vector2d> pixels;
  std::vector<Vector3d> points;
  for (size_t f = 0; f < rig_frames.size(); ++f)
    for (const auto& [camera, detections] : rig_frames[f]) {
      if (camera < 0 || size_t(camera) >= cameras.size())
        return InvalidArgumentError("CalibrateRig: rig frame " + std::to_string(f) + " names camera " + std::to_string(camera));
      for (const auto& kv : detections) {
        const auto it = model_definition.find(kv.first);
        if (it == model_definition.end()) return InvalidArgumentError("CalibrateRig: feature " + std::to_string(kv.first) + " is not in the model definition");
        pixels.push_back(kv.second);
        points.push_back(it->second);
      }
      view_camera.push_back(camera); view_frame.push_back(int64_t(f)); view_offsets.push_back(int64_t(pixels.size()));
    }
  RigCalibration r;
  if (Status st = sensors::CameraModel::CalibrateRigFromChart(models, intrinsics, int64_t(rig_frames.size()), view_camera, view_frame, view_offsets,
                                                              pixels, points, options, &r, covariance, nullptr, nullptr, nullptr, nullptr, device);
      !st.ok()) return st;
  if (r.Ok())
    for (size_t c = 0; c < cameras.size(); ++c)
      if (r.camera_status[c] == CALICO_RIG_CAMERA_OK) cameras[c]->SetExtrinsics(r.CameraPose(c));
  std::vector<Pose3d> T_rig_chart(r.NumFrames());
  for (size_t f = 0; f < r.NumFrames(); ++f) T_rig_chart[f] = r.FramePose(f);
  if (out) *out = std::move(r);
  return T_rig_chart;
}

inline StatusOr<Trajectory::ImuAlignment> Trajectory::AlignImu(const sensors::Gyroscope& gyroscope, const sensors::Accelerometer* accelerometer,
                                                               const calico_imu_alignment_options* options, bool covariance, bool curve,
                                                               int device) const {
  std::vector<double> gs, g, as, a, ctrl;
  gyroscope.SortedMeasurements(&gs, &g);
  if (accelerometer) accelerometer->SortedMeasurements(&as, &a);
  for (const auto& c : spline_.control_points()) ctrl.insert(ctrl.end(), c.begin(), c.end());
  double t_ra[3] = {0.0, 0.0, 0.0};
  if (accelerometer)
    for (int i = 0; i < 3; ++i) t_ra[i] = accelerometer->GetExtrinsics().translation()[i];
  ImuAlignment r;
  double q[4] = {0.0, 0.0, 0.0, 1.0};
  if (covariance) r.cov.assign(49, 0.0);
  if (curve) r.curve.assign(CALICO_ALIGN_MAX_LAGS, 0.0);
  const int st = calico_imu_align(device, spline_.GetSplineOrder(), int(spline_.knots().size()), spline_.knots().data(),
                                  spline_.basis_matrices().data(), ctrl.data(), int64_t(gs.size()), gs.data(), g.data(), int64_t(as.size()),
                                  as.data(), a.data(), t_ra, nullptr, nullptr, options, q, r.gyro_bias.data(), &r.latency,
                                  r.gravity_world.data(), r.accel_bias.data(), covariance ? r.cov.data() : nullptr, curve ? r.curve.data() : nullptr, &r.summary);
  if (st != CALICO_OK) return Status(static_cast<StatusCode>(st), calico_last_error(nullptr));
  r.q_rig_gyro = Quaterniond(q[3], q[0], q[1], q[2]);
  if (curve) r.curve.resize(size_t(r.summary.n_lags));
  return r;
}

inline StatusOr<Trajectory::AccelerometerAlignment> Trajectory::AlignAccelerometer(const sensors::Accelerometer& accelerometer,
                                                                                   const calico_accel_alignment_options* options,
                                                                                   bool covariance, int device) const {
  std::vector<double> as, a, ctrl;
  accelerometer.SortedMeasurements(&as, &a);
  for (const auto& c : spline_.control_points()) ctrl.insert(ctrl.end(), c.begin(), c.end());
  const Quaterniond& q0 = accelerometer.GetExtrinsics().rotation();
  const double q_init[4] = {q0.x(), q0.y(), q0.z(), q0.w()}, latency_init = accelerometer.GetLatency();
  AccelerometerAlignment r;
  double q[4] = {0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  if (covariance) r.cov.assign(169, 0.0);
  const int st = calico_accel_align(device, spline_.GetSplineOrder(), int(spline_.knots().size()), spline_.knots().data(),
                                    spline_.basis_matrices().data(), ctrl.data(), int64_t(as.size()), as.data(), a.data(), q_init, &latency_init,
                                    nullptr, nullptr, nullptr, options, q, t, r.bias.data(), r.gravity_world.data(), &r.latency,
                                    covariance ? r.cov.data() : nullptr, &r.summary);
  if (st != CALICO_OK) return Status(static_cast<StatusCode>(st), calico_last_error(nullptr));
  r.T_rig_accel = Pose3d(Quaterniond(q[3], q[0], q[1], q[2]), Vector3d(t[0], t[1], t[2]));
  return r;
}

inline StatusOr<Trajectory::CameraAlignment> Trajectory::AlignCamera(const sensors::Camera& camera, const WorldModel& world_model,
                                                                     const calico_camera_alignment_options* options, int model_id,
                                                                     bool covariance, bool curve, int device) const {
  if (camera.GetModel() == sensors::CameraIntrinsicsModel::kNone) return FailedPreconditionError("Camera model has not been set!");
  const auto body_it = world_model.rigidbodies().find(model_id);
  if (body_it == world_model.rigidbodies().end())
    return InvalidArgumentError("AlignCamera: no rigid body with id " + std::to_string(model_id) + " in the world model");
  const RigidBody& body = *body_it->second;
  // the body's images: (stamp, image id) -> feature id -> pixel, so frames come in stamp order and pairs in id order
  std::map<std::pair<double, int>, std::map<int, Vector2d>> frames;
  for (const auto& [id, m] : camera.GetMeasurementIdToMeasurement()) {
    if (id.model_id != model_id || camera.IsOutlier(id)) continue;
    frames[{id.stamp, id.image_id}][id.feature_id] = m.pixel;
  }
  CameraAlignment r;
  std::vector<int64_t> offsets(1, 0);
  std::vector<Vector2d> pixels;
  std::vector<Vector3d> points;
  for (const auto& [key, frame] : frames) {
    for (const auto& [feature, pixel] : frame) {
      const auto it = body.model_definition.find(feature);
      if (it == body.model_definition.end())
        return InvalidArgumentError("AlignCamera: feature " + std::to_string(feature) + " is not in the model definition");
      pixels.push_back(pixel);
      points.push_back(it->second);
    }
    r.stamps.push_back(key.first); r.image_ids.push_back(key.second);
    offsets.push_back(int64_t(pixels.size()));
  }
  const size_t F = r.stamps.size();
  std::vector<double> ctrl;
  for (const auto& c : spline_.control_points()) ctrl.insert(ctrl.end(), c.begin(), c.end());
  r.frame_rms.assign(F, 0.0); r.frame_n_used.assign(F, 0); r.frame_status.assign(F, 0);
  if (covariance) r.cov.assign(49, 0.0);
  if (curve) r.curve.assign(CALICO_ALIGN_MAX_LAGS, 0.0);
  double q[4] = {0.0, 0.0, 0.0, 1.0}, t[3] = {0.0, 0.0, 0.0};
  static_assert(sizeof(Vector2d) == 2 * sizeof(double) && sizeof(Vector3d) == 3 * sizeof(double), "pixels and points are packed");
  const int st = calico_camera_align(device, spline_.GetSplineOrder(), int(spline_.knots().size()), spline_.knots().data(),
                                     spline_.basis_matrices().data(), ctrl.data(), int(camera.GetModel()), camera.GetIntrinsics().data(),
                                     int(camera.GetIntrinsics().size()), body.T_world_rigidbody.rotation().data(),
                                     body.T_world_rigidbody.translation().data(), int64_t(F), r.stamps.data(), offsets.data(),
                                     pixels.empty() ? nullptr : pixels[0].data(), points.empty() ? nullptr : points[0].data(), nullptr, nullptr,
                                     nullptr, options, q, t, &r.latency, r.frame_rms.data(), r.frame_n_used.data(), r.frame_status.data(),
                                     covariance ? r.cov.data() : nullptr, curve ? r.curve.data() : nullptr, &r.summary);
  if (st != CALICO_OK) return Status(static_cast<StatusCode>(st), calico_last_error(nullptr));
  r.T_rig_camera = Pose3d(Quaterniond(q[3], q[0], q[1], q[2]), Vector3d(t[0], t[1], t[2]));
  if (curve) r.curve.resize(size_t(r.summary.n_lags));
  return r;
}

inline Status Covariance::ProjectionUncertainty(const sensors::Camera& camera, const std::vector<Vector2d>& pixels, double range,
                                                ProjectionFrame frame, std::vector<std::array<double, 3>>* cov,
                                                std::vector<uint8_t>* valid) const {
  return ProjectionUncertainty(camera.ProblemSensor(), pixels, range, frame, cov, valid);
}

// ---------------------------------------------------------------------------
// BatchOptimizer (batch_optimizer.{h,cpp})
// ---------------------------------------------------------------------------
/// Per-sensor blocks of a Covariance: intrinsics (n x n), extrinsics as 6 x 6 [rotation tangent | translation], latency.
inline Status SensorIntrinsicsCovariance(const Covariance& c, const sensors::Sensor& s, std::vector<double>* out) {
  const size_t n = size_t(s.GetIntrinsics().size());
  out->assign(n * n, 0.0);
  return c.Get(s.GetIntrinsics().data(), s.GetIntrinsics().data(), 1, out->data());
}
inline Status SensorExtrinsicsCovariance(const Covariance& c, const sensors::Sensor& s, std::vector<double>* out) {
  const double* q = s.GetExtrinsics().rotation().data();
  const double* t = s.GetExtrinsics().translation().data();
  const double* blk[2] = {q, t};
  out->assign(36, 0.0);
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      double tmp[9];
      if (Status st = c.Get(blk[a], blk[b], 1, tmp); !st.ok()) return st;
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) (*out)[size_t(3 * a + i) * 6 + size_t(3 * b + j)] = tmp[3 * i + j];
    }
  return OkStatus();
}
inline Status SensorLatencyVariance(const Covariance& c, const sensors::Sensor& s, double* out) {
  const auto* sc = dynamic_cast<const sensors::SensorCommon*>(&s);
  if (!sc) return InvalidArgumentError("covariance: not a library sensor");
  return c.Get(sc->LatencyData(), sc->LatencyData(), 1, out);
}

/// Covariance::Predictions for a sensor of the optimizer the covariance came from.
inline Status SensorPredictions(const Covariance& c, const sensors::Sensor& s, bool apply_loss, std::vector<double>* cov,
                                std::vector<double>* leverage, std::vector<uint8_t>* valid) {
  const auto* sc = dynamic_cast<const sensors::SensorCommon*>(&s);
  if (!sc) return InvalidArgumentError("covariance: not a library sensor");
  return c.Predictions(sc->ProblemSensor(), apply_loss, cov, leverage, valid);
}

class BatchOptimizer {
 public:
  ~BatchOptimizer() {  // batch_optimizer.cpp:19-33: un-owned pointers are released, owned ones deleted
    for (size_t i = 0; i < sensors_.size(); ++i) if (own_sensors_[i]) delete sensors_[i];
    if (own_world_model_) delete world_model_;
    if (own_trajectory_) delete trajectory_;
  }
  void AddSensor(sensors::Sensor* sensor, bool take_ownership = true) { sensors_.push_back(sensor); own_sensors_.push_back(take_ownership); }
  void AddWorldModel(WorldModel* world_model, bool take_ownership = true) { world_model_ = world_model; own_world_model_ = take_ownership; }
  void AddTrajectory(Trajectory* trajectory_world_sensorrig, bool take_ownership = true) { trajectory_ = trajectory_world_sensorrig; own_trajectory_ = take_ownership; }
  /// batch_optimizer.cpp:53-81
  /// Covariance of the estimates at the current values (the problem is rebuilt, as Optimize does; the plan cache makes that
  /// cheap). The sensors' residual information is left as it is.
  StatusOr<Covariance> ComputeCovariance(const calico_covariance_options& options = DefaultCovarianceOptions(), int device = 0) {
    if (!world_model_ || !trajectory_) return FailedPreconditionError("world model and trajectory must be added before ComputeCovariance()");
    Problem problem;
    world_model_->AddParametersToProblem(problem);
    trajectory_->AddParametersToProblem(problem);
    for (sensors::Sensor* sensor : sensors_) {
      const auto np = sensor->AddParametersToProblem(problem);
      if (!np.ok()) return np.status();
      const auto nr = sensor->AddResidualsToProblem(problem, *trajectory_, *world_model_);
      if (!nr.ok()) return nr.status();
    }
    Covariance cov;
    const Status st = problem.ComputeCovariance(options, &cov, device);
    if (!st.ok()) return st;
    return cov;
  }
  /// Which directions of the calibration the data determine, at the current values (the problem is rebuilt, as
  /// ComputeCovariance does). Every sensor's blocks are labelled with its name: Describe(i) reads "gyroscope intrinsics 0.52, ...".
  StatusOr<Observability> AnalyzeObservability(const calico_observability_options& options = DefaultObservabilityOptions(), int device = 0) {
    if (!world_model_ || !trajectory_) return FailedPreconditionError("world model and trajectory must be added before AnalyzeObservability()");
    Problem problem;
    world_model_->AddParametersToProblem(problem);
    trajectory_->AddParametersToProblem(problem);
    for (sensors::Sensor* sensor : sensors_) {
      const auto np = sensor->AddParametersToProblem(problem);
      if (!np.ok()) return np.status();
      const auto nr = sensor->AddResidualsToProblem(problem, *trajectory_, *world_model_);
      if (!nr.ok()) return nr.status();
    }
    Observability obs;
    const Status st = problem.AnalyzeObservability(options, &obs, device);
    if (!st.ok()) return st;
    for (size_t i = 0; i < sensors_.size(); ++i) {
      const sensors::Sensor* s = sensors_[i];
      const std::string name = s->GetName().empty() ? "sensor " + std::to_string(i) : s->GetName();
      obs.Label(s->GetIntrinsics().data(), name, "intrinsics");
      obs.Label(s->GetExtrinsics().rotation().data(), name, "rotation");
      obs.Label(s->GetExtrinsics().translation().data(), name, "translation");
      if (const auto* sc = dynamic_cast<const sensors::SensorCommon*>(s)) obs.Label(sc->LatencyData(), name, "latency");
    }
    return obs;
  }
  StatusOr<Summary> Optimize(const SolverOptions& options = DefaultSolverOptions(), int device = 0) {
    if (!world_model_ || !trajectory_) return FailedPreconditionError("world model and trajectory must be added before Optimize()");
    Problem problem;
    world_model_->AddParametersToProblem(problem);
    trajectory_->AddParametersToProblem(problem);
    for (sensors::Sensor* sensor : sensors_) {
      sensor->ClearResidualInfo();
      const auto np = sensor->AddParametersToProblem(problem);
      if (!np.ok()) return np.status();
      const auto nr = sensor->AddResidualsToProblem(problem, *trajectory_, *world_model_);
      if (!nr.ok()) return nr.status();
    }
    Summary summary;
    const Status st = problem.Solve(options, &summary, device);
    if (!st.ok()) return st;
    for (sensors::Sensor* sensor : sensors_) {
      const Status us = sensor->UpdateResiduals(problem);
      if (!us.ok()) return us;
    }
    return summary;
  }
 private:
  std::vector<sensors::Sensor*> sensors_;
  std::vector<bool> own_sensors_;
  WorldModel* world_model_ = nullptr;
  Trajectory* trajectory_ = nullptr;
  bool own_world_model_ = false, own_trajectory_ = false;
};

}  // namespace calico

#endif  // CALICO_CALICO_HPP_
