// pybind_calico.cpp — the Python face of the host-side mirror (include/calico/calico.hpp): the class, method and
// enum names of the reference's `calico` module (calico/calico.cpp:18-437) over the HIP backend, so that the
// notebooks' call sequence (build sensors -> FitSpline -> BatchOptimizer.Optimize -> residual pairs -> outliers)
// runs unchanged with `from calico_amd import calico`. Conventions taken from the reference binding:
//   * Status-returning setters that the reference wraps in lambdas raise RuntimeError("Error: <message>"),
//     the others return the Status object (SetModel, SetLatency, AddMeasurement(s), SetMeasurementNoise),
//   * Pose3d.rotation is [w, x, y, z], vectors travel as numpy arrays,
//   * AddSensor / AddTrajectory / AddWorldModel / AddRigidBody / AddLandmark do not take ownership.
// Not bound: AprilGridDetector (OpenCV image processing, outside the optimisation path).
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <memory>
#include <sstream>
#include <stdexcept>

#include "calico/calico.hpp"

namespace py = pybind11;

namespace pybind11 {
namespace detail {
template <int N, class V>
struct fixed_vector_caster {
  static bool load_into(handle src, V& value) {
    auto arr = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(src);
    if (!arr || arr.size() != N) return false;
    for (int i = 0; i < N; ++i) value.v[i] = arr.data()[i];
    return true;
  }
  static handle to_python(const V& v) {
    py::array_t<double> a(N);
    for (int i = 0; i < N; ++i) a.mutable_data()[i] = v.v[i];
    return a.release();
  }
};
template <>
struct type_caster<calico::Vector3d> {
  PYBIND11_TYPE_CASTER(calico::Vector3d, const_name("numpy.ndarray[float64[3]]"));
  bool load(handle src, bool) { return fixed_vector_caster<3, calico::Vector3d>::load_into(src, value); }
  static handle cast(const calico::Vector3d& v, return_value_policy, handle) { return fixed_vector_caster<3, calico::Vector3d>::to_python(v); }
};
template <>
struct type_caster<calico::Vector2d> {
  PYBIND11_TYPE_CASTER(calico::Vector2d, const_name("numpy.ndarray[float64[2]]"));
  bool load(handle src, bool) { return fixed_vector_caster<2, calico::Vector2d>::load_into(src, value); }
  static handle cast(const calico::Vector2d& v, return_value_policy, handle) { return fixed_vector_caster<2, calico::Vector2d>::to_python(v); }
};
}  // namespace detail
}  // namespace pybind11

namespace {

using namespace calico;           // NOLINT
using namespace calico::sensors;  // NOLINT

void raise_if_error(const Status& st) {
  if (!st.ok()) throw std::runtime_error(std::string("Error: ") + st.message());
}
py::array_t<double> to_array(const VectorXd& v) {
  py::array_t<double> a(py::ssize_t(v.size()));
  std::copy(v.begin(), v.end(), a.mutable_data());
  return a;
}
VectorXd to_vector(const py::object& o) {
  auto arr = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(o);
  if (!arr) throw py::type_error("expected a sequence of floats");
  return VectorXd(arr.data(), arr.data() + arr.size());
}

// (n, 2) pixels of a numpy array
std::vector<Vector2d> to_pixels(const py::object& o) {
  auto arr = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(o);
  if (!arr || !((arr.ndim() == 2 && arr.shape(1) == 2) || (arr.ndim() == 1 && arr.size() == 2)))
    throw py::type_error("expected an (n, 2) array of pixels (or one pixel of length 2)");
  std::vector<Vector2d> px(size_t(arr.size() / 2));
  for (size_t i = 0; i < px.size(); ++i) px[i] = Vector2d(arr.data()[2 * i], arr.data()[2 * i + 1]);
  return px;
}
py::array_t<bool> to_bool_array(const std::vector<uint8_t>& v) {
  py::array_t<bool> ok{py::ssize_t(v.size())};
  for (size_t i = 0; i < v.size(); ++i) ok.mutable_at(py::ssize_t(i)) = v[i] != 0;
  return ok;
}
// (bearings (n, 3), valid (n,) bool)
py::tuple bearings_tuple(const std::vector<Vector3d>& b, const std::vector<uint8_t>& valid) {
  py::array_t<double> a({py::ssize_t(b.size()), py::ssize_t(3)});
  for (size_t i = 0; i < b.size(); ++i)
    for (int c = 0; c < 3; ++c) a.mutable_at(py::ssize_t(i), c) = b[i][c];
  return py::make_tuple(a, to_bool_array(valid));
}

// the part of the sensor interface the three sensors share (calico.cpp:77-103 and its two repetitions)
template <class S, class PyClass>
void bind_sensor_common(PyClass& c) {
  c.def(py::init<>())
      .def("SetName", &S::SetName)
      .def("GetName", &S::GetName)
      .def("SetExtrinsics", &S::SetExtrinsics)
      .def("GetExtrinsics", &S::GetExtrinsics)
      .def("SetIntrinsics", [](S& self, const py::object& intrinsics) { raise_if_error(self.SetIntrinsics(to_vector(intrinsics))); })
      .def("GetIntrinsics", [](const S& self) { return to_array(self.GetIntrinsics()); })
      .def("SetLatency", &S::SetLatency)
      .def("GetLatency", &S::GetLatency)
      .def("EnableExtrinsicsEstimation", &S::EnableExtrinsicsEstimation)
      .def("EnableIntrinsicsEstimation", &S::EnableIntrinsicsEstimation)
      .def("EnableLatencyEstimation", &S::EnableLatencyEstimation)
      .def("SetModel", &S::SetModel)
      .def("GetModel", &S::GetModel)
      .def("SetLossFunction", &S::SetLossFunction, py::arg("loss"), py::arg("scale") = 1.0)
      .def("AddMeasurement", &S::AddMeasurement)
      .def("AddMeasurements", &S::AddMeasurements)
      .def("SetMeasurementNoise", &S::SetMeasurementNoise)
      .def("GetMeasurementNoise", &S::GetMeasurementNoise)
      .def("NumberOfMeasurements", &S::NumberOfMeasurements)
      .def("ClearMeasurements", &S::ClearMeasurements)
      .def("Project",
           [](const S& self, const std::vector<double>& interp_times, const Trajectory& sensorrig_trajectory,
              const WorldModel& world_model) {
             auto vals = self.Project(interp_times, sensorrig_trajectory, world_model);
             raise_if_error(vals.status());
             return vals.value();
           });
}

// ---- IMU noise (calico_imu_allan) ----
// options: None or a dict of calico_allan_options fields; cluster_sizes (a list) travels beside it and is kept alive in `sizes`
calico_allan_options allan_options(const py::object& options, std::vector<int64_t>* sizes) {
  calico_allan_options o = DefaultAllanOptions();
  if (!options.is_none()) {
    for (auto kv : py::cast<py::dict>(options)) {
      const std::string name = py::cast<std::string>(kv.first);
      if (name == "points_per_decade") o.points_per_decade = py::cast<int>(kv.second);
      else if (name == "max_tau_fraction") o.max_tau_fraction = py::cast<double>(kv.second);
      else if (name == "terms") o.terms = py::cast<int>(kv.second);
      else if (name == "cluster_sizes") *sizes = py::cast<std::vector<int64_t>>(kv.second);
      else throw py::type_error("no Allan variance option '" + name + "'");
    }
  }
  if (!sizes->empty()) { o.n_cluster_sizes = int(sizes->size()); o.cluster_sizes = sizes->data(); }
  return o;
}
py::dict imu_noise_dict(const ImuNoise& r) {
  const py::ssize_t nc = py::ssize_t(r.cluster_sizes.size());
  py::array_t<double> avar({nc, py::ssize_t(3)});
  for (py::ssize_t j = 0; j < nc; ++j)
    for (int c = 0; c < 3; ++c) avar.mutable_at(j, c) = r.avar[size_t(j)][c];
  py::list noise;
  for (const calico_allan_noise& a : r.axes) {
    py::dict d;
    d["Q"] = a.Q; d["N"] = a.N; d["B"] = a.B; d["K"] = a.K; d["R"] = a.R; d["objective"] = a.objective;
    d["terms_used"] = a.terms_used; d["n_points"] = a.n_points; d["status"] = int(a.status);
    noise.append(d);
  }
  py::dict sm;
  sm["n"] = r.summary.n; sm["sample_rate_hz"] = r.summary.sample_rate_hz; sm["duration"] = r.summary.duration;
  sm["N_pooled"] = r.summary.N_pooled; sm["sigma_at_rate"] = r.summary.sigma_at_rate;
  sm["bias_drift_over_recording"] = r.summary.bias_drift_over_recording;
  py::dict out;
  out["cluster_sizes"] = py::array_t<int64_t>(nc, r.cluster_sizes.data());
  out["tau"] = py::array_t<double>(nc, r.tau.data());
  out["rel_err"] = py::array_t<double>(nc, r.rel_err.data());
  out["avar"] = avar; out["noise"] = noise; out["summary"] = sm;
  return out;
}
// noise: CharacterizeImuNoise's dict (its summary's N_pooled is what ApplyNoise reads)
template <class S, class PyClass>
void bind_imu_noise(PyClass& c) {
  c.def("MeasurementRate", [](const S& self) { auto r = self.MeasurementRate(); raise_if_error(r.status()); return r.value(); })
      .def("ApplyNoise", [](S& self, const py::dict& noise, double rate_hz) {
        ImuNoise n;
        n.summary.N_pooled = py::cast<double>(py::cast<py::dict>(noise["summary"])["N_pooled"]);
        raise_if_error(self.ApplyNoise(n, rate_hz));
      }, py::arg("noise"), py::arg("rate_hz"));
}

// ---- intrinsic calibration (calico_camera_calibrate): what the two bindings share ----
// options: None or a dict of calico_calibration_options fields
calico_calibration_options calibration_options(const py::object& options) {
  calico_calibration_options o;
  calico_default_calibration_options(&o);
  if (!options.is_none()) {
    for (auto kv : py::cast<py::dict>(options)) {
      const std::string name = py::cast<std::string>(kv.first);
      if (name == "max_iterations") o.max_iterations = py::cast<int>(kv.second);
      else if (name == "step_tolerance") o.step_tolerance = py::cast<double>(kv.second);
      else if (name == "huber_scale") o.huber_scale = py::cast<double>(kv.second);
      else if (name == "min_points") o.min_points = py::cast<int>(kv.second);
      else throw py::type_error("no calibration option '" + name + "'");
    }
  }
  return o;
}
// options: None or a dict of calico_imu_alignment_options fields
calico_imu_alignment_options imu_alignment_options(const py::object& options) {
  calico_imu_alignment_options o;
  calico_default_imu_alignment_options(&o);
  if (!options.is_none()) {
    for (auto kv : py::cast<py::dict>(options)) {
      const std::string name = py::cast<std::string>(kv.first);
      if (name == "max_lag") o.max_lag = py::cast<double>(kv.second);
      else if (name == "lag_step") o.lag_step = py::cast<double>(kv.second);
      else if (name == "max_iterations") o.max_iterations = py::cast<int>(kv.second);
      else if (name == "step_tolerance") o.step_tolerance = py::cast<double>(kv.second);
      else if (name == "estimate_latency") o.estimate_latency = py::cast<int>(kv.second);
      else if (name == "estimate_gyro_bias") o.estimate_gyro_bias = py::cast<int>(kv.second);
      else if (name == "estimate_accel_bias") o.estimate_accel_bias = py::cast<int>(kv.second);
      else if (name == "min_samples") o.min_samples = py::cast<int>(kv.second);
      else if (name == "sigma_gyro") o.sigma_gyro = py::cast<double>(kv.second);
      else throw py::type_error("no IMU alignment option '" + name + "'");
    }
  }
  return o;
}
// options: None or a dict of calico_accel_alignment_options fields
calico_accel_alignment_options accel_alignment_options(const py::object& options) {
  calico_accel_alignment_options o;
  calico_default_accel_alignment_options(&o);
  if (!options.is_none()) {
    for (auto kv : py::cast<py::dict>(options)) {
      const std::string name = py::cast<std::string>(kv.first);
      if (name == "max_iterations") o.max_iterations = py::cast<int>(kv.second);
      else if (name == "step_tolerance") o.step_tolerance = py::cast<double>(kv.second);
      else if (name == "estimate_rotation") o.estimate_rotation = py::cast<int>(kv.second);
      else if (name == "estimate_lever_arm") o.estimate_lever_arm = py::cast<int>(kv.second);
      else if (name == "estimate_bias") o.estimate_bias = py::cast<int>(kv.second);
      else if (name == "estimate_gravity") o.estimate_gravity = py::cast<int>(kv.second);
      else if (name == "estimate_latency") o.estimate_latency = py::cast<int>(kv.second);
      else if (name == "min_samples") o.min_samples = py::cast<int>(kv.second);
      else if (name == "sigma_accel") o.sigma_accel = py::cast<double>(kv.second);
      else throw py::type_error("no accelerometer alignment option '" + name + "'");
    }
  }
  return o;
}
// options: None or a dict of calico_camera_alignment_options fields
calico_camera_alignment_options camera_alignment_options(const py::object& options) {
  calico_camera_alignment_options o;
  calico_default_camera_alignment_options(&o);
  if (!options.is_none()) {
    for (auto kv : py::cast<py::dict>(options)) {
      const std::string name = py::cast<std::string>(kv.first);
      if (name == "max_lag") o.max_lag = py::cast<double>(kv.second);
      else if (name == "lag_step") o.lag_step = py::cast<double>(kv.second);
      else if (name == "max_iterations") o.max_iterations = py::cast<int>(kv.second);
      else if (name == "step_tolerance") o.step_tolerance = py::cast<double>(kv.second);
      else if (name == "estimate_latency") o.estimate_latency = py::cast<int>(kv.second);
      else if (name == "estimate_translation") o.estimate_translation = py::cast<int>(kv.second);
      else if (name == "huber_scale") o.huber_scale = py::cast<double>(kv.second);
      else if (name == "min_points") o.min_points = py::cast<int>(kv.second);
      else if (name == "min_frames") o.min_frames = py::cast<int>(kv.second);
      else if (name == "sigma_pixel") o.sigma_pixel = py::cast<double>(kv.second);
      else throw py::type_error("no camera alignment option '" + name + "'");
    }
  }
  return o;
}
// None, or a dict of calico_spline_fit_options fields; lambda_rot / lambda_pos: a number or a sequence (n_lambda follows its length)
calico_spline_fit_options spline_fit_options(const py::object& options) {
  calico_spline_fit_options o;
  calico_default_spline_fit_options(&o);
  if (options.is_none()) return o;
  bool n_given = false;
  for (auto kv : py::cast<py::dict>(options)) {
    const std::string name = py::cast<std::string>(kv.first);
    if (name == "derivative") o.derivative = py::cast<int>(kv.second);
    else if (name == "relative") o.relative = py::cast<int>(kv.second);
    else if (name == "n_lambda") { o.n_lambda = py::cast<int>(kv.second); n_given = true; }
    else if (name == "target_rms_rot") o.target_rms_rot = py::cast<double>(kv.second);
    else if (name == "target_rms_pos") o.target_rms_pos = py::cast<double>(kv.second);
    else if (name == "lambda_rot" || name == "lambda_pos") {
      std::vector<double> grid;
      if (py::isinstance<py::float_>(kv.second) || py::isinstance<py::int_>(kv.second)) grid.push_back(py::cast<double>(kv.second));
      else for (auto v : py::cast<py::sequence>(kv.second)) grid.push_back(py::cast<double>(v));
      if (grid.empty() || grid.size() > CALICO_FIT_MAX_LAMBDAS) throw py::value_error(name + " must have 1 to 32 entries");
      double* dst = name == "lambda_rot" ? o.lambda_rot : o.lambda_pos;
      for (size_t i = 0; i < CALICO_FIT_MAX_LAMBDAS; ++i) dst[i] = i < grid.size() ? grid[i] : 0.0;
      if (!n_given) o.n_lambda = int(grid.size());
    } else throw py::type_error("no spline fit option '" + name + "'");
  }
  return o;
}
// None, or a dict of calico_spline_robust_options fields; loss: CALICO_ROBUST_HUBER / _TUKEY, or "huber" / "tukey"
calico_spline_robust_options spline_robust_options(const py::object& options) {
  calico_spline_robust_options o;
  calico_default_spline_robust_options(&o);
  if (options.is_none()) return o;
  for (auto kv : py::cast<py::dict>(options)) {
    const std::string name = py::cast<std::string>(kv.first);
    if (name == "loss") {
      if (py::isinstance<py::str>(kv.second)) {
        const std::string loss = py::cast<std::string>(kv.second);
        if (loss != "huber" && loss != "tukey") throw py::value_error("loss must be 'huber' or 'tukey'");
        o.loss = loss == "huber" ? CALICO_ROBUST_HUBER : CALICO_ROBUST_TUKEY;
      } else o.loss = py::cast<int>(kv.second);
    } else if (name == "max_iterations") o.max_iterations = py::cast<int>(kv.second);
    else if (name == "tuning_rot") o.tuning_rot = py::cast<double>(kv.second);
    else if (name == "tuning_pos") o.tuning_pos = py::cast<double>(kv.second);
    else if (name == "scale_rot") o.scale_rot = py::cast<double>(kv.second);
    else if (name == "scale_pos") o.scale_pos = py::cast<double>(kv.second);
    else if (name == "min_scale_rot") o.min_scale_rot = py::cast<double>(kv.second);
    else if (name == "min_scale_pos") o.min_scale_pos = py::cast<double>(kv.second);
    else if (name == "step_tolerance") o.step_tolerance = py::cast<double>(kv.second);
    else throw py::type_error("no robust spline fit option '" + name + "'");
  }
  return o;
}
calico_spline_cv_options spline_cv_options(const py::object& options) {
  calico_spline_cv_options o;
  calico_default_spline_cv_options(&o);
  if (options.is_none()) return o;
  for (auto kv : py::cast<py::dict>(options)) {
    const std::string name = py::cast<std::string>(kv.first);
    if (name == "criterion") {
      if (py::isinstance<py::str>(kv.second)) {
        const std::string criterion = py::cast<std::string>(kv.second);
        if (criterion != "gcv" && criterion != "press") throw py::value_error("criterion must be 'gcv' or 'press'");
        o.criterion = criterion == "gcv" ? CALICO_FIT_CV_GCV : CALICO_FIT_CV_PRESS;
      } else o.criterion = py::cast<int>(kv.second);
    } else throw py::type_error("no cross-validated spline fit option '" + name + "'");
  }
  return o;
}
std::vector<uint8_t> to_mask(const py::object& o) {
  std::vector<uint8_t> mask;
  if (!o.is_none())
    for (auto v : py::cast<py::sequence>(o)) mask.push_back(py::cast<bool>(v) ? 1 : 0);
  return mask;
}
// None, or n doubles per frame as a flat vector
bool to_rows(const py::object& o, std::vector<double>* out) {
  if (o.is_none()) return false;
  const VectorXd v = to_vector(o);
  out->assign(v.begin(), v.end());
  return true;
}
// a dict of arrays, one row per frame, the intrinsics, and the summary's fields
py::dict calibration_dict(const CameraModel::ChartCalibration& r, bool covariance) {
  const py::ssize_t n = py::ssize_t(r.NumFrames()), K = py::ssize_t(r.intrinsics.size());
  py::array_t<double> q({n, py::ssize_t(4)}), t({n, py::ssize_t(3)}), rms(n);
  py::array_t<int32_t> used(n);
  py::array_t<uint8_t> status(n);
  std::copy(r.q.begin(), r.q.end(), q.mutable_data());
  std::copy(r.t.begin(), r.t.end(), t.mutable_data());
  std::copy(r.rms.begin(), r.rms.end(), rms.mutable_data());
  std::copy(r.n_used.begin(), r.n_used.end(), used.mutable_data());
  std::copy(r.status.begin(), r.status.end(), status.mutable_data());
  py::dict out;
  out["intrinsics"] = to_array(r.intrinsics);
  out["q"] = q; out["t"] = t; out["rms"] = rms; out["n_used"] = used; out["frame_status"] = status;
  out["status"] = r.summary.status; out["iterations"] = r.summary.iterations; out["initial_cost"] = r.summary.initial_cost;
  out["final_cost"] = r.summary.final_cost; out["total_rms"] = r.summary.rms; out["frames_used"] = r.summary.frames_used;
  out["pairs_used"] = r.summary.pairs_used; out["lambda"] = r.summary.lambda;
  if (covariance) {
    py::array_t<double> cov({K, K});
    std::copy(r.cov.begin(), r.cov.end(), cov.mutable_data());
    out["cov"] = cov;
  }
  return out;
}

// ---- rig calibration (calico_rig_calibrate): what the two bindings share ----
// options: None or a dict of calico_rig_options fields
calico_rig_options rig_options(const py::object& options) {
  calico_rig_options o;
  calico_default_rig_options(&o);
  if (!options.is_none()) {
    for (auto kv : py::cast<py::dict>(options)) {
      const std::string name = py::cast<std::string>(kv.first);
      if (name == "max_iterations") o.max_iterations = py::cast<int>(kv.second);
      else if (name == "step_tolerance") o.step_tolerance = py::cast<double>(kv.second);
      else if (name == "huber_scale") o.huber_scale = py::cast<double>(kv.second);
      else if (name == "min_points") o.min_points = py::cast<int>(kv.second);
      else if (name == "min_shared_frames") o.min_shared_frames = py::cast<int>(kv.second);
      else if (name == "reference_camera") o.reference_camera = py::cast<int>(kv.second);
      else throw py::type_error("no rig option '" + name + "'");
    }
  }
  return o;
}
template <class T> py::array_t<T> rows_of(const std::vector<T>& v, py::ssize_t rows, py::ssize_t cols) {
  py::array_t<T> a = cols == 1 ? py::array_t<T>(rows) : py::array_t<T>({rows, cols});
  std::copy(v.begin(), v.end(), a.mutable_data());
  return a;
}
// a dict of arrays, one row per camera, per rig frame and per view, and the summary's fields
py::dict rig_dict(const RigCalibration& r, bool covariance) {
  const py::ssize_t nc = py::ssize_t(r.NumCameras()), nf = py::ssize_t(r.NumFrames()), nv = py::ssize_t(r.NumViews());
  py::dict out;
  out["q_rig_camera"] = rows_of(r.q_rig_camera, nc, 4); out["t_rig_camera"] = rows_of(r.t_rig_camera, nc, 3);
  out["camera_status"] = rows_of(r.camera_status, nc, 1);
  out["q_frame"] = rows_of(r.q_frame, nf, 4); out["t_frame"] = rows_of(r.t_frame, nf, 3); out["frame_status"] = rows_of(r.frame_status, nf, 1);
  out["view_rms"] = rows_of(r.view_rms, nv, 1); out["view_n_used"] = rows_of(r.view_n_used, nv, 1); out["view_status"] = rows_of(r.view_status, nv, 1);
  out["status"] = r.summary.status; out["iterations"] = r.summary.iterations; out["initial_cost"] = r.summary.initial_cost;
  out["final_cost"] = r.summary.final_cost; out["total_rms"] = r.summary.rms; out["cameras_used"] = r.summary.cameras_used;
  out["frames_used"] = r.summary.frames_used; out["views_used"] = r.summary.views_used; out["pairs_used"] = r.summary.pairs_used;
  out["lambda"] = r.summary.lambda;
  if (covariance) out["cov"] = rows_of(r.cov, 6 * nc, 6 * nc);
  return out;
}
std::vector<Vector3d> to_points(const py::object& points) {
  const VectorXd flat = to_vector(points);
  if (flat.size() % 3 != 0) throw py::type_error("expected an (n, 3) array of chart points");
  std::vector<Vector3d> pts(flat.size() / 3);
  for (size_t i = 0; i < pts.size(); ++i) pts[i] = Vector3d(flat[3 * i], flat[3 * i + 1], flat[3 * i + 2]);
  return pts;
}
std::map<int, Vector3d> to_model_definition(const py::dict& model_definition) {
  std::map<int, Vector3d> model;
  for (auto kv : model_definition) {
    auto arr = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(kv.second);
    if (!arr || (arr.size() != 2 && arr.size() != 3)) throw py::type_error("a chart point is (x, y) or (x, y, z)");
    model[py::cast<int>(kv.first)] = Vector3d(arr.data()[0], arr.data()[1], arr.size() == 3 ? arr.data()[2] : 0.0);
  }
  return model;
}

}  // namespace

PYBIND11_MODULE(_calico, m) {
  m.doc() = "calico_amd: the reference's `calico` Python API over the MI355X HIP backend (libcalico_hip.so)";

  py::enum_<StatusCode>(m, "StatusCode")
      .value("kOk", StatusCode::kOk)
      .value("kInvalidArgument", StatusCode::kInvalidArgument)
      .value("kFailedPrecondition", StatusCode::kFailedPrecondition)
      .value("kUnimplemented", StatusCode::kUnimplemented)
      .value("kInternal", StatusCode::kInternal);

  py::class_<Status>(m, "Status")
      .def(py::init<>())
      .def("ok", &Status::ok)
      .def("code", &Status::code)
      .def("message", [](const Status& self) { return std::string(self.message()); });

  py::class_<Pose3d>(m, "Pose3d")
      .def(py::init<>())
      .def(py::init<const Pose3d&>())
      .def_property(
          "rotation", [](const Pose3d& self) { const auto q = self.GetRotation(); return to_array(VectorXd(q.begin(), q.end())); },
          [](Pose3d& self, const py::object& wxyz) {
            const VectorXd q = to_vector(wxyz);
            if (q.size() != 4) throw py::value_error("rotation is [w, x, y, z]");
            self.SetRotation({q[0], q[1], q[2], q[3]});
          })
      .def_property("translation", &Pose3d::GetTranslation, &Pose3d::SetTranslation)
      .def("__copy__", [](const Pose3d& self) { return Pose3d(self); })
      .def("__deepcopy__", [](const Pose3d& self, const py::dict&) { return Pose3d(self); });

  py::enum_<utils::LossFunctionType>(m, "LossFunctionType")
      .value("kNone", utils::LossFunctionType::kNone)
      .value("kHuber", utils::LossFunctionType::kHuber)
      .value("kCauchy", utils::LossFunctionType::kCauchy);

  py::class_<Sensor, std::shared_ptr<Sensor>>(m, "Sensor");  // NOLINT

  // ---- IMU: the gyroscope and accelerometer id / measurement types are one C++ type, bound once ----
  py::class_<ImuObservationId>(m, "GyroscopeObservationId")
      .def(py::init<>())
      .def(py::init<const ImuObservationId&>())
      .def_readwrite("stamp", &ImuObservationId::stamp)
      .def_readwrite("sequence", &ImuObservationId::sequence)
      .def("__eq__", [](const ImuObservationId& a, const ImuObservationId& b) { return a == b; })
      .def("__hash__", [](const ImuObservationId& a) { return ImuObservationIdHash()(a); });
  py::class_<ImuMeasurement>(m, "GyroscopeMeasurement")
      .def(py::init<>())
      .def(py::init<const ImuMeasurement&>())
      .def_readwrite("measurement", &ImuMeasurement::measurement)
      .def_readwrite("id", &ImuMeasurement::id);
  m.attr("AccelerometerObservationId") = m.attr("GyroscopeObservationId");
  m.attr("AccelerometerMeasurement") = m.attr("GyroscopeMeasurement");

  py::enum_<AccelerometerIntrinsicsModel>(m, "AccelerometerIntrinsicsModel")
      .value("kNone", AccelerometerIntrinsicsModel::kNone)
      .value("kAccelerometerScaleOnly", AccelerometerIntrinsicsModel::kAccelerometerScaleOnly)
      .value("kAccelerometerScaleAndBias", AccelerometerIntrinsicsModel::kAccelerometerScaleAndBias)
      .value("kAccelerometerVectorNav", AccelerometerIntrinsicsModel::kAccelerometerVectorNav);
  py::class_<Accelerometer, std::shared_ptr<Accelerometer>, Sensor> accelerometer(m, "Accelerometer");
  bind_sensor_common<Accelerometer>(accelerometer);
  bind_imu_noise<Accelerometer>(accelerometer);

  py::enum_<GyroscopeIntrinsicsModel>(m, "GyroscopeIntrinsicsModel")
      .value("kNone", GyroscopeIntrinsicsModel::kNone)
      .value("kGyroscopeScaleOnly", GyroscopeIntrinsicsModel::kGyroscopeScaleOnly)
      .value("kGyroscopeScaleAndBias", GyroscopeIntrinsicsModel::kGyroscopeScaleAndBias)
      .value("kGyroscopeVectorNav", GyroscopeIntrinsicsModel::kGyroscopeVectorNav);
  py::class_<Gyroscope, std::shared_ptr<Gyroscope>, Sensor> gyroscope(m, "Gyroscope");
  bind_sensor_common<Gyroscope>(gyroscope);
  bind_imu_noise<Gyroscope>(gyroscope);

  // ---- camera ----
  py::enum_<CameraIntrinsicsModel>(m, "CameraIntrinsicsModel")
      .value("kNone", CameraIntrinsicsModel::kNone)
      .value("kOpenCv5", CameraIntrinsicsModel::kOpenCv5)
      .value("kOpenCv8", CameraIntrinsicsModel::kOpenCv8)
      .value("kKannalaBrandt", CameraIntrinsicsModel::kKannalaBrandt)
      .value("kDoubleSphere", CameraIntrinsicsModel::kDoubleSphere)
      .value("kFieldOfView", CameraIntrinsicsModel::kFieldOfView)
      .value("kUnifiedCamera", CameraIntrinsicsModel::kUnifiedCamera)
      .value("kExtendedUnifiedCamera", CameraIntrinsicsModel::kExtendedUnifiedCamera);

  // sensors::CameraModel::UnprojectPixel (camera_models.h): not bound by the reference's module; named as the C++. On the
  // device (calico_camera_unproject): the unit-norm point that projects to the pixel.
  py::class_<CameraModel>(m, "CameraModel")
      .def_static("UnprojectPixel",
                  [](CameraIntrinsicsModel model, const py::object& intrinsics, const Vector2d& pixel, int device) {
                    auto b = CameraModel::UnprojectPixel(model, to_vector(intrinsics), pixel, device);
                    raise_if_error(b.status());
                    return b.value();
                  },
                  py::arg("model"), py::arg("intrinsics"), py::arg("pixel"), py::arg("device") = 0)
      .def_static("UnprojectPixels",
                  [](CameraIntrinsicsModel model, const py::object& intrinsics, const py::object& pixels, int device) {
                    std::vector<Vector3d> b;
                    std::vector<uint8_t> valid;
                    raise_if_error(CameraModel::UnprojectPixels(model, to_vector(intrinsics), to_pixels(pixels), &b, &valid, device));
                    return bearings_tuple(b, valid);
                  },
                  py::arg("model"), py::arg("intrinsics"), py::arg("pixels"), py::arg("device") = 0)
      // frame_offsets (n_frames + 1) cuts pixels (N, 2) and points (N, 3) into frames; free_mask: None or K flags; q_init / t_init:
      // None or (n_frames, 4) / (n_frames, 3); options: None or a dict of calico_calibration_options fields
      .def_static("CalibrateFromChart",
                  [](CameraIntrinsicsModel model, const py::object& intrinsics_init, const std::vector<int64_t>& frame_offsets,
                     const py::object& pixels, const py::object& points, const py::object& options, bool covariance,
                     const py::object& free_mask, const py::object& q_init, const py::object& t_init, int device) {
                    const VectorXd flat = to_vector(points);
                    if (flat.size() % 3 != 0) throw py::type_error("expected an (n, 3) array of chart points");
                    std::vector<Vector3d> pts(flat.size() / 3);
                    for (size_t i = 0; i < pts.size(); ++i) pts[i] = Vector3d(flat[3 * i], flat[3 * i + 1], flat[3 * i + 2]);
                    const calico_calibration_options o = calibration_options(options);
                    std::vector<double> q0, t0;
                    const bool hq = to_rows(q_init, &q0), ht = to_rows(t_init, &t0);
                    CameraModel::ChartCalibration r;
                    raise_if_error(CameraModel::CalibrateFromChart(model, to_vector(intrinsics_init), frame_offsets, to_pixels(pixels), pts, &o, &r,
                                                                   covariance, to_mask(free_mask), hq ? &q0 : nullptr, ht ? &t0 : nullptr, device));
                    return calibration_dict(r, covariance);
                  },
                  py::arg("model"), py::arg("intrinsics_init"), py::arg("frame_offsets"), py::arg("pixels"), py::arg("points"),
                  py::arg("options") = py::none(), py::arg("covariance") = false, py::arg("free_mask") = py::none(),
                  py::arg("q_init") = py::none(), py::arg("t_init") = py::none(), py::arg("device") = 0)
      // models and intrinsics: one entry per camera; view v is camera view_camera[v] in rig frame view_frame[v] with the pairs
      // [view_offsets[v], view_offsets[v + 1]) of pixels (N, 2) and points (N, 3); the starts: None or (C, 4) / (C, 3) and
      // (n_frames, 4) / (n_frames, 3); options: None or a dict of calico_rig_options fields
      .def_static("CalibrateRigFromChart",
                  [](const std::vector<CameraIntrinsicsModel>& models, const std::vector<py::object>& intrinsics, int64_t n_frames,
                     const std::vector<int32_t>& view_camera, const std::vector<int64_t>& view_frame, const std::vector<int64_t>& view_offsets,
                     const py::object& pixels, const py::object& points, const py::object& options, bool covariance,
                     const py::object& q_rig_camera_init, const py::object& t_rig_camera_init, const py::object& q_frame_init,
                     const py::object& t_frame_init, int device) {
                    std::vector<VectorXd> ks;
                    for (const py::object& k : intrinsics) ks.push_back(to_vector(k));
                    const calico_rig_options o = rig_options(options);
                    std::vector<double> qc, tc, qf, tf;
                    const bool hqc = to_rows(q_rig_camera_init, &qc), htc = to_rows(t_rig_camera_init, &tc);
                    const bool hqf = to_rows(q_frame_init, &qf), htf = to_rows(t_frame_init, &tf);
                    RigCalibration r;
                    raise_if_error(CameraModel::CalibrateRigFromChart(models, ks, n_frames, view_camera, view_frame, view_offsets, to_pixels(pixels),
                                                                      to_points(points), &o, &r, covariance, hqc ? &qc : nullptr, htc ? &tc : nullptr,
                                                                      hqf ? &qf : nullptr, htf ? &tf : nullptr, device));
                    return rig_dict(r, covariance);
                  },
                  py::arg("models"), py::arg("intrinsics"), py::arg("n_frames"), py::arg("view_camera"), py::arg("view_frame"),
                  py::arg("view_offsets"), py::arg("pixels"), py::arg("points"), py::arg("options") = py::none(), py::arg("covariance") = false,
                  py::arg("q_rig_camera_init") = py::none(), py::arg("t_rig_camera_init") = py::none(), py::arg("q_frame_init") = py::none(),
                  py::arg("t_frame_init") = py::none(), py::arg("device") = 0);
  py::enum_<ProjectionFrame>(m, "ProjectionFrame")
      .value("kCamera", ProjectionFrame::kCamera)
      .value("kRig", ProjectionFrame::kRig);

  py::class_<CameraObservationId>(m, "CameraObservationId")
      .def(py::init([] { return CameraObservationId{0.0, 0, 0, 0}; }))
      .def(py::init<const CameraObservationId&>())
      .def("__hash__", [](const CameraObservationId& id) { return CameraObservationIdHash()(id); })
      .def("__eq__", [](const CameraObservationId& a, const CameraObservationId& b) { return a == b; })
      .def("__str__",
           [](const CameraObservationId& id) {
             std::ostringstream os;
             os << "stamp: " << id.stamp << ", image_id: " << id.image_id << ", model_id: " << id.model_id
                << ", feature_id: " << id.feature_id;
             return os.str();
           })
      .def_readwrite("stamp", &CameraObservationId::stamp)
      .def_readwrite("image_id", &CameraObservationId::image_id)
      .def_readwrite("model_id", &CameraObservationId::model_id)
      .def_readwrite("feature_id", &CameraObservationId::feature_id);

  py::class_<CameraMeasurement>(m, "CameraMeasurement")
      .def(py::init([] { return CameraMeasurement{Vector2d(), CameraObservationId{0.0, 0, 0, 0}}; }))
      .def(py::init<const CameraMeasurement&>())
      .def_readwrite("pixel", &CameraMeasurement::pixel)
      .def_readwrite("id", &CameraMeasurement::id);

  py::class_<Camera, std::shared_ptr<Camera>, Sensor> camera(m, "Camera");
  bind_sensor_common<Camera>(camera);
  camera
      .def("GetMeasurementResidualPairs",
           [](const Camera& self) {
             auto pairs = self.GetMeasurementResidualPairs();
             raise_if_error(pairs.status());
             return pairs.value();
           })
      .def("GetMeasurementIdToMeasurement",
           [](const Camera& self) {
             py::dict out;
             for (const auto& kv : self.GetMeasurementIdToMeasurement()) out[py::cast(kv.first)] = py::cast(kv.second);
             return out;
           })
      .def("MarkOutlierById", [](Camera& self, const CameraObservationId& id) { raise_if_error(self.MarkOutlierById(id)); })
      .def("MarkOutliersById",
           [](Camera& self, const std::vector<CameraObservationId>& ids) { raise_if_error(self.MarkOutliersById(ids)); })
      .def("ClearOutliersList", &Camera::ClearOutliersList)
      .def("UnprojectPixels",
           [](const Camera& self, const py::object& pixels, int device) {
             std::vector<Vector3d> b;
             std::vector<uint8_t> valid;
             raise_if_error(self.UnprojectPixels(to_pixels(pixels), &b, &valid, device));
             return bearings_tuple(b, valid);
           },
           py::arg("pixels"), py::arg("device") = 0)
      // all_detections: a list of {feature id: pixel}; model_definition: {feature id: chart point (x, y[, z])}; options: None or a
      // dict of calico_resection_options fields. Returns a dict of arrays, one row per frame.
      .def("EstimateChartPoses",
           [](const Camera& self, const std::vector<std::map<int, Vector2d>>& all_detections, const py::dict& model_definition,
              const py::object& options, bool covariance, int device) {
             std::map<int, Vector3d> model;
             for (auto kv : model_definition) {
               auto arr = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(kv.second);
               if (!arr || (arr.size() != 2 && arr.size() != 3)) throw py::type_error("a chart point is (x, y) or (x, y, z)");
               model[py::cast<int>(kv.first)] = Vector3d(arr.data()[0], arr.data()[1], arr.size() == 3 ? arr.data()[2] : 0.0);
             }
             calico_resection_options o;
             calico_default_resection_options(&o);
             if (!options.is_none()) {
               for (auto kv : py::cast<py::dict>(options)) {
                 const std::string name = py::cast<std::string>(kv.first);
                 if (name == "max_iterations") o.max_iterations = py::cast<int>(kv.second);
                 else if (name == "step_tolerance") o.step_tolerance = py::cast<double>(kv.second);
                 else if (name == "huber_scale") o.huber_scale = py::cast<double>(kv.second);
                 else if (name == "min_points") o.min_points = py::cast<int>(kv.second);
                 else throw py::type_error("no resection option '" + name + "'");
               }
             }
             CameraModel::ChartResection r;
             raise_if_error(self.EstimateChartPoses(all_detections, model, &o, &r, covariance, device));
             const py::ssize_t n = py::ssize_t(r.NumFrames());
             py::array_t<double> q({n, py::ssize_t(4)}), t({n, py::ssize_t(3)}), rms(n);
             py::array_t<int32_t> used(n), its(n);
             py::array_t<uint8_t> status(n);
             std::copy(r.q.begin(), r.q.end(), q.mutable_data());
             std::copy(r.t.begin(), r.t.end(), t.mutable_data());
             std::copy(r.rms.begin(), r.rms.end(), rms.mutable_data());
             std::copy(r.n_used.begin(), r.n_used.end(), used.mutable_data());
             std::copy(r.iterations.begin(), r.iterations.end(), its.mutable_data());
             std::copy(r.status.begin(), r.status.end(), status.mutable_data());
             py::dict out;
             out["q"] = q; out["t"] = t; out["rms"] = rms; out["n_used"] = used; out["iterations"] = its; out["status"] = status;
             if (covariance) {
               py::array_t<double> cov({n, py::ssize_t(6), py::ssize_t(6)});
               std::copy(r.cov.begin(), r.cov.end(), cov.mutable_data());
               out["cov"] = cov;
             }
             return out;
           },
           py::arg("all_detections"), py::arg("model_definition"), py::arg("options") = py::none(), py::arg("covariance") = false,
           py::arg("device") = 0)
      // all_detections and model_definition as EstimateChartPoses; the camera's intrinsics are the start and, after a run that ends
      // OK or NOT_CONVERGED, the estimate. Returns CalibrateFromChart's dict.
      .def("CalibrateIntrinsics",
           [](Camera& self, const std::vector<std::map<int, Vector2d>>& all_detections, const py::dict& model_definition,
              const py::object& options, bool covariance, const py::object& free_mask, const py::object& q_init, const py::object& t_init,
              int device) {
             std::map<int, Vector3d> model;
             for (auto kv : model_definition) {
               auto arr = py::array_t<double, py::array::c_style | py::array::forcecast>::ensure(kv.second);
               if (!arr || (arr.size() != 2 && arr.size() != 3)) throw py::type_error("a chart point is (x, y) or (x, y, z)");
               model[py::cast<int>(kv.first)] = Vector3d(arr.data()[0], arr.data()[1], arr.size() == 3 ? arr.data()[2] : 0.0);
             }
             const calico_calibration_options o = calibration_options(options);
             std::vector<double> q0, t0;
             const bool hq = to_rows(q_init, &q0), ht = to_rows(t_init, &t0);
             CameraModel::ChartCalibration r;
             raise_if_error(self.CalibrateIntrinsics(all_detections, model, &o, &r, covariance, to_mask(free_mask), hq ? &q0 : nullptr,
                                                     ht ? &t0 : nullptr, device));
             return calibration_dict(r, covariance);
           },
           py::arg("all_detections"), py::arg("model_definition"), py::arg("options") = py::none(), py::arg("covariance") = false,
           py::arg("free_mask") = py::none(), py::arg("q_init") = py::none(), py::arg("t_init") = py::none(), py::arg("device") = 0);

  // ---- trajectory, world model ----
  py::class_<Trajectory, std::shared_ptr<Trajectory>>(m, "Trajectory")
      .def(py::init<>())
      .def(
          "FitSpline",
          [](Trajectory& self, const std::map<double, Pose3d>& poses, double knot_frequency, int spline_order) {
            raise_if_error(self.FitSpline(poses, knot_frequency, spline_order));
          },
          py::arg("poses"), py::arg("knot_frequency") = Trajectory::kDefaultKnotFrequency,
          py::arg("spline_order") = Trajectory::kDefaultSplineOrder)
      // The smoothing fit (calico_fit_spline_smooth). options: None or a dict of calico_spline_fit_options fields; weights: None or
      // one [rotation, position] pair per pose in time order. Returns a dict: status, chosen, n_used (one entry per group) and
      // rows ([group][lambda] dicts: status, replaced_pivots, lambda, rss, penalty, rms).
      .def(
          "FitSplineSmooth",
          [](Trajectory& self, const std::map<double, Pose3d>& poses, double knot_frequency, int spline_order, const py::object& options,
             const py::object& weights) {
            const calico_spline_fit_options o = spline_fit_options(options);
            std::vector<std::array<double, 2>> w;
            if (!weights.is_none())
              for (auto row : py::cast<py::sequence>(weights)) {
                const auto pair = py::cast<std::vector<double>>(row);
                if (pair.size() != 2) throw py::value_error("weights: one [rotation, position] pair per pose");
                w.push_back({pair[0], pair[1]});
              }
            auto res = self.FitSplineSmooth(poses, knot_frequency, spline_order, o, w);
            raise_if_error(res.status());
            const calico_spline_fit_summary& sm = res.value().summary;
            py::dict out;
            out["status"] = py::make_tuple(sm.status[0], sm.status[1]);
            out["chosen"] = py::make_tuple(sm.chosen[0], sm.chosen[1]);
            out["n_used"] = py::make_tuple(sm.n_used[0], sm.n_used[1]);
            py::list groups;
            const size_t nl = res.value().rows.size() / 2;
            for (size_t g = 0; g < 2; ++g) {
              py::list rows;
              for (size_t l = 0; l < nl; ++l) {
                const calico_spline_fit_row& r = res.value().rows[g * nl + l];
                py::dict d;
                d["status"] = r.status; d["replaced_pivots"] = r.replaced_pivots; d["lambda"] = r.lambda; d["rss"] = r.rss;
                d["penalty"] = r.penalty; d["rms"] = r.rms;
                rows.append(d);
              }
              groups.append(rows);
            }
            out["rows"] = groups;
            return out;
          },
          py::arg("poses"), py::arg("knot_frequency") = Trajectory::kDefaultKnotFrequency,
          py::arg("spline_order") = Trajectory::kDefaultSplineOrder, py::arg("options") = py::none(), py::arg("weights") = py::none())
      // The robust fit (calico_fit_spline_robust). options: as FitSplineSmooth's, with one lambda per group; robust: None or a dict of
      // calico_spline_robust_options fields (loss: "huber" or "tukey"); weights: prior weights, as FitSplineSmooth's. Returns a dict: the
      // summary's fields (one entry per group), and robust_weights and residuals, one [rotation, position] pair per pose in time order.
      .def(
          "FitSplineRobust",
          [](Trajectory& self, const std::map<double, Pose3d>& poses, double knot_frequency, int spline_order, const py::object& options,
             const py::object& robust, const py::object& weights) {
            const calico_spline_fit_options o = spline_fit_options(options);
            const calico_spline_robust_options r = spline_robust_options(robust);
            std::vector<std::array<double, 2>> w;
            if (!weights.is_none())
              for (auto row : py::cast<py::sequence>(weights)) {
                const auto pair = py::cast<std::vector<double>>(row);
                if (pair.size() != 2) throw py::value_error("weights: one [rotation, position] pair per pose");
                w.push_back({pair[0], pair[1]});
              }
            auto res = self.FitSplineRobust(poses, knot_frequency, spline_order, o, r, w);
            raise_if_error(res.status());
            const calico_spline_robust_summary& sm = res.value().summary;
            py::dict out;
            out["status"] = py::make_tuple(sm.status[0], sm.status[1]);
            out["iterations"] = py::make_tuple(sm.iterations[0], sm.iterations[1]);
            out["replaced_pivots"] = py::make_tuple(sm.replaced_pivots[0], sm.replaced_pivots[1]);
            out["n_used"] = py::make_tuple(sm.n_used[0], sm.n_used[1]);
            out["n_downweighted"] = py::make_tuple(sm.n_downweighted[0], sm.n_downweighted[1]);
            out["n_rejected"] = py::make_tuple(sm.n_rejected[0], sm.n_rejected[1]);
            out["lambda"] = py::make_tuple(sm.lambda[0], sm.lambda[1]);
            out["scale"] = py::make_tuple(sm.scale[0], sm.scale[1]);
            out["median_residual"] = py::make_tuple(sm.median_residual[0], sm.median_residual[1]);
            out["last_step"] = py::make_tuple(sm.last_step[0], sm.last_step[1]);
            out["rss"] = py::make_tuple(sm.rss[0], sm.rss[1]);
            py::list u, e;
            for (const auto& pair : res.value().robust_weights) u.append(py::make_tuple(pair[0], pair[1]));
            for (const auto& pair : res.value().residuals) e.append(py::make_tuple(pair[0], pair[1]));
            out["robust_weights"] = u;
            out["residuals"] = e;
            return out;
          },
          py::arg("poses"), py::arg("knot_frequency") = Trajectory::kDefaultKnotFrequency,
          py::arg("spline_order") = Trajectory::kDefaultSplineOrder, py::arg("options") = py::none(), py::arg("robust") = py::none(),
          py::arg("weights") = py::none())
      // The cross-validated fit (calico_fit_spline_cv). options: as FitSplineSmooth's, a grid and no target; cv: None or a dict of
      // calico_spline_cv_options fields (criterion: "gcv" or "press"); weights: as FitSplineSmooth's. Returns FitSplineSmooth's dict
      // plus edf and score (one entry per group), cv_rows ([group][lambda] dicts: edf, gcv, press, max_leverage), and leverage and
      // loo_residuals, one [rotation, position] pair per pose in time order.
      .def(
          "FitSplineCV",
          [](Trajectory& self, const std::map<double, Pose3d>& poses, double knot_frequency, int spline_order, const py::object& options,
             const py::object& cv, const py::object& weights) {
            const calico_spline_fit_options o = spline_fit_options(options);
            const calico_spline_cv_options co = spline_cv_options(cv);
            std::vector<std::array<double, 2>> w;
            if (!weights.is_none())
              for (auto row : py::cast<py::sequence>(weights)) {
                const auto pair = py::cast<std::vector<double>>(row);
                if (pair.size() != 2) throw py::value_error("weights: one [rotation, position] pair per pose");
                w.push_back({pair[0], pair[1]});
              }
            auto res = self.FitSplineCV(poses, knot_frequency, spline_order, o, co, w);
            raise_if_error(res.status());
            const calico_spline_cv_summary& sm = res.value().summary;
            py::dict out;
            out["status"] = py::make_tuple(sm.status[0], sm.status[1]);
            out["chosen"] = py::make_tuple(sm.chosen[0], sm.chosen[1]);
            out["n_used"] = py::make_tuple(sm.n_used[0], sm.n_used[1]);
            out["edf"] = py::make_tuple(sm.edf[0], sm.edf[1]);
            out["score"] = py::make_tuple(sm.score[0], sm.score[1]);
            py::list groups, cv_groups;
            const size_t nl = res.value().rows.size() / 2;
            for (size_t g = 0; g < 2; ++g) {
              py::list rows, cv_rows;
              for (size_t l = 0; l < nl; ++l) {
                const calico_spline_fit_row& r = res.value().rows[g * nl + l];
                py::dict d;
                d["status"] = r.status; d["replaced_pivots"] = r.replaced_pivots; d["lambda"] = r.lambda; d["rss"] = r.rss;
                d["penalty"] = r.penalty; d["rms"] = r.rms;
                rows.append(d);
                const calico_spline_cv_row& c = res.value().cv_rows[g * nl + l];
                py::dict e;
                e["edf"] = c.edf; e["gcv"] = c.gcv; e["press"] = c.press; e["max_leverage"] = c.max_leverage;
                cv_rows.append(e);
              }
              groups.append(rows);
              cv_groups.append(cv_rows);
            }
            out["rows"] = groups;
            out["cv_rows"] = cv_groups;
            py::list h, loo;
            for (const auto& pair : res.value().leverage) h.append(py::make_tuple(pair[0], pair[1]));
            for (const auto& pair : res.value().loo_residuals) loo.append(py::make_tuple(pair[0], pair[1]));
            out["leverage"] = h;
            out["loo_residuals"] = loo;
            return out;
          },
          py::arg("poses"), py::arg("knot_frequency") = Trajectory::kDefaultKnotFrequency,
          py::arg("spline_order") = Trajectory::kDefaultSplineOrder, py::arg("options") = py::none(), py::arg("cv") = py::none(),
          py::arg("weights") = py::none())
      .def("Interpolate", [](const Trajectory& self, const std::vector<double>& stamps) {
        auto poses = self.Interpolate(stamps);
        raise_if_error(poses.status());
        return poses.value();
      })
      // Camera-IMU alignment against this trajectory from the sensors' registered measurements (calico_imu_align). options: None
      // or a dict of calico_imu_alignment_options fields. Returns a dict: q_rig_gyro (x, y, z, w), gyro_bias, latency,
      // gravity_world, accel_bias, cov and curve (each on request) and the summary's fields. The sensors are not changed.
      .def("AlignImu",
           [](const Trajectory& self, const Gyroscope& gyroscope, const py::object& accelerometer, const py::object& options,
              bool covariance, bool curve, int device) {
             const calico_imu_alignment_options o = imu_alignment_options(options);
             const Accelerometer* accel = accelerometer.is_none() ? nullptr : py::cast<const Accelerometer*>(accelerometer);
             auto res = self.AlignImu(gyroscope, accel, &o, covariance, curve, device);
             raise_if_error(res.status());
             const Trajectory::ImuAlignment& r = res.value();
             py::dict out;
             out["q_rig_gyro"] = to_array(VectorXd{r.q_rig_gyro.x(), r.q_rig_gyro.y(), r.q_rig_gyro.z(), r.q_rig_gyro.w()});
             out["gyro_bias"] = to_array(VectorXd{r.gyro_bias[0], r.gyro_bias[1], r.gyro_bias[2]});
             out["latency"] = r.latency;
             out["gravity_world"] = to_array(VectorXd{r.gravity_world[0], r.gravity_world[1], r.gravity_world[2]});
             out["accel_bias"] = to_array(VectorXd{r.accel_bias[0], r.accel_bias[1], r.accel_bias[2]});
             if (curve) out["curve"] = to_array(r.curve);
             if (covariance) {
               py::array_t<double> cov({py::ssize_t(7), py::ssize_t(7)});
               std::copy(r.cov.begin(), r.cov.end(), cov.mutable_data());
               out["cov"] = cov;
             }
             const calico_imu_alignment_summary& sm = r.summary;
             out["gyro_status"] = sm.gyro_status; out["accel_status"] = sm.accel_status; out["gyro_samples"] = sm.gyro_samples;
             out["accel_samples"] = sm.accel_samples; out["first_sample"] = sm.first_sample; out["iterations"] = sm.iterations;
             out["n_lags"] = sm.n_lags; out["peak_index"] = sm.peak_index; out["coarse_latency"] = sm.coarse_latency;
             out["peak_correlation"] = sm.peak_correlation; out["gyro_rms"] = sm.gyro_rms; out["accel_rms"] = sm.accel_rms;
             out["gravity_norm"] = sm.gravity_norm; out["scatter_pivot"] = sm.scatter_pivot; out["initial_cost"] = sm.initial_cost;
             out["final_cost"] = sm.final_cost; out["lambda"] = sm.lambda;
             return out;
           },
           py::arg("gyroscope"), py::arg("accelerometer") = py::none(), py::arg("options") = py::none(), py::arg("covariance") = false,
           py::arg("curve") = false, py::arg("device") = 0)
      // Alignment of an accelerometer against this trajectory from its registered measurements, started at its current rotation
      // and latency (calico_accel_align). options: None or a dict of calico_accel_alignment_options fields. Returns a dict:
      // q_rig_accel (x, y, z, w), t_rig_accel, bias, gravity_world, latency, cov (on request) and the summary's fields. The sensor
      // is not changed.
      .def("AlignAccelerometer",
           [](const Trajectory& self, const Accelerometer& accelerometer, const py::object& options, bool covariance, int device) {
             const calico_accel_alignment_options o = accel_alignment_options(options);
             auto res = self.AlignAccelerometer(accelerometer, &o, covariance, device);
             raise_if_error(res.status());
             const Trajectory::AccelerometerAlignment& r = res.value();
             const Quaterniond& q = r.T_rig_accel.rotation();
             const Vector3d& t = r.T_rig_accel.translation();
             py::dict out;
             out["q_rig_accel"] = to_array(VectorXd{q.x(), q.y(), q.z(), q.w()});
             out["t_rig_accel"] = to_array(VectorXd{t[0], t[1], t[2]});
             out["bias"] = to_array(VectorXd{r.bias[0], r.bias[1], r.bias[2]});
             out["gravity_world"] = to_array(VectorXd{r.gravity_world[0], r.gravity_world[1], r.gravity_world[2]});
             out["latency"] = r.latency;
             if (covariance) {
               py::array_t<double> cov({py::ssize_t(13), py::ssize_t(13)});
               std::copy(r.cov.begin(), r.cov.end(), cov.mutable_data());
               out["cov"] = cov;
             }
             const calico_accel_alignment_summary& sm = r.summary;
             out["status"] = sm.status; out["linear_status"] = sm.linear_status; out["samples"] = sm.samples;
             out["first_sample"] = sm.first_sample; out["iterations"] = sm.iterations; out["rms"] = sm.rms; out["linear_rms"] = sm.linear_rms;
             out["gravity_norm"] = sm.gravity_norm; out["initial_cost"] = sm.initial_cost; out["final_cost"] = sm.final_cost;
             out["lambda"] = sm.lambda;
             return out;
           },
           py::arg("accelerometer"), py::arg("options") = py::none(), py::arg("covariance") = false, py::arg("device") = 0)
      // Alignment of a camera that is not synchronised with this trajectory, from its registered measurements of the rigid body
      // model_id (calico_camera_align). options: None or a dict of calico_camera_alignment_options fields. Returns a dict:
      // q_rig_camera (x, y, z, w), t_rig_camera, latency, image_ids, stamps, frame_rms, frame_n_used, frame_status, cov and curve
      // (each on request) and the summary's fields. The camera is not changed.
      .def("AlignCamera",
           [](const Trajectory& self, const Camera& camera, const WorldModel& world_model, const py::object& options, int model_id,
              bool covariance, bool curve, int device) {
             const calico_camera_alignment_options o = camera_alignment_options(options);
             auto res = self.AlignCamera(camera, world_model, &o, model_id, covariance, curve, device);
             raise_if_error(res.status());
             const Trajectory::CameraAlignment& r = res.value();
             const Quaterniond& q = r.T_rig_camera.rotation();
             const Vector3d& t = r.T_rig_camera.translation();
             py::dict out;
             out["q_rig_camera"] = to_array(VectorXd{q.x(), q.y(), q.z(), q.w()});
             out["t_rig_camera"] = to_array(VectorXd{t[0], t[1], t[2]});
             out["latency"] = r.latency;
             out["image_ids"] = r.image_ids; out["stamps"] = to_array(r.stamps); out["frame_rms"] = to_array(r.frame_rms);
             out["frame_n_used"] = std::vector<int>(r.frame_n_used.begin(), r.frame_n_used.end());
             out["frame_status"] = std::vector<int>(r.frame_status.begin(), r.frame_status.end());
             if (curve) out["curve"] = to_array(r.curve);
             if (covariance) {
               py::array_t<double> cov({py::ssize_t(7), py::ssize_t(7)});
               std::copy(r.cov.begin(), r.cov.end(), cov.mutable_data());
               out["cov"] = cov;
             }
             const calico_camera_alignment_summary& sm = r.summary;
             out["status"] = sm.status; out["iterations"] = sm.iterations; out["frames_used"] = sm.frames_used; out["pairs_used"] = sm.pairs_used;
             out["n_lags"] = sm.n_lags; out["peak_index"] = sm.peak_index; out["coarse_latency"] = sm.coarse_latency;
             out["peak_score"] = sm.peak_score; out["rms"] = sm.rms; out["initial_cost"] = sm.initial_cost; out["final_cost"] = sm.final_cost;
             out["lambda"] = sm.lambda;
             return out;
           },
           py::arg("camera"), py::arg("world_model"), py::arg("options") = py::none(), py::arg("model_id") = 0, py::arg("covariance") = false,
           py::arg("curve") = false, py::arg("device") = 0);

  py::class_<Landmark, std::shared_ptr<Landmark>>(m, "Landmark")
      .def(py::init<>())
      .def_readwrite("point", &Landmark::point)
      .def_readwrite("id", &Landmark::id)
      .def_readwrite("point_is_constant", &Landmark::point_is_constant);

  py::class_<RigidBody, std::shared_ptr<RigidBody>>(m, "RigidBody")
      .def(py::init<>())
      .def_readwrite("model_definition", &RigidBody::model_definition)
      .def_readwrite("T_world_rigidbody", &RigidBody::T_world_rigidbody)
      .def_readwrite("id", &RigidBody::id)
      .def_readwrite("world_pose_is_constant", &RigidBody::world_pose_is_constant)
      .def_readwrite("model_definition_is_constant", &RigidBody::model_definition_is_constant);

  py::class_<WorldModel, std::shared_ptr<WorldModel>>(m, "WorldModel")
      .def(py::init<>())
      .def("AddLandmark",
           [](WorldModel& self, std::shared_ptr<Landmark> landmark) {
             raise_if_error(self.AddLandmark(landmark.get(), /*take_ownership=*/false));
           },
           py::keep_alive<1, 2>())
      .def("AddRigidBody",
           [](WorldModel& self, std::shared_ptr<RigidBody> rigidbody) {
             raise_if_error(self.AddRigidBody(rigidbody.get(), /*take_ownership=*/false));
           },
           py::keep_alive<1, 2>())
      .def("SetGravity", &WorldModel::SetGravity)
      .def("GetGravity", [](const WorldModel& self) { return Vector3d(self.GetGravity()); })
      .def("EnableGravityEstimation", &WorldModel::EnableGravityEstimation)
      .def("NumberOfLandmarks", &WorldModel::NumberOfLandmarks)
      .def("NumberOfRigidBodies", &WorldModel::NumberOfRigidBodies);

  // ---- solver options / summary (the fields calico.cpp:352-395 binds, plus the HIP backend's own) ----
  py::class_<Summary>(m, "Summary")
      .def("BriefReport", &Summary::BriefReport)
      .def("FullReport", &Summary::FullReport)
      .def("IsSolutionUsable", &Summary::IsSolutionUsable)
      .def_readonly("initial_cost", &Summary::initial_cost)
      .def_readonly("final_cost", &Summary::final_cost)
      .def_readonly("termination_type", &Summary::termination_type)
      .def_readonly("num_iterations", &Summary::num_iterations)
      .def_readonly("num_successful_steps", &Summary::num_successful_steps)
      .def_readonly("num_unsuccessful_steps", &Summary::num_unsuccessful_steps)
      .def_readonly("num_residual_blocks", &Summary::num_residual_blocks)
      .def_readonly("num_residuals", &Summary::num_residuals)
      .def_readonly("num_parameter_blocks", &Summary::num_parameter_blocks)
      .def_readonly("num_parameters", &Summary::num_parameters)
      .def_readonly("num_parameter_blocks_reduced", &Summary::num_parameter_blocks_reduced)
      .def_readonly("num_parameters_reduced", &Summary::num_parameters_reduced)
      .def_readonly("num_effective_parameters_reduced", &Summary::num_effective_parameters_reduced)
      .def_readonly("num_residual_blocks_reduced", &Summary::num_residual_blocks_reduced)
      .def_readonly("num_residuals_reduced", &Summary::num_residuals_reduced)
      .def_readonly("total_time_in_seconds", &Summary::total_time_in_seconds);

  py::class_<SolverOptions>(m, "SolverOptions")
      .def(py::init([] { return DefaultSolverOptions(); }))
      .def_readwrite("max_num_iterations", &SolverOptions::max_num_iterations)
      .def_readwrite("num_threads", &SolverOptions::num_threads)
      .def_readwrite("function_tolerance", &SolverOptions::function_tolerance)
      .def_readwrite("gradient_tolerance", &SolverOptions::gradient_tolerance)
      .def_readwrite("parameter_tolerance", &SolverOptions::parameter_tolerance)
      .def_property(
          "minimizer_progress_to_stdout", [](const SolverOptions& o) { return o.minimizer_progress_to_stdout != 0; },
          [](SolverOptions& o, bool v) { o.minimizer_progress_to_stdout = v ? 1 : 0; })
      .def_readwrite("jacobi_scaling", &SolverOptions::jacobi_scaling)
      .def_readwrite("sync_every", &SolverOptions::sync_every)
      .def_readwrite("initial_trust_region_radius", &SolverOptions::initial_trust_region_radius)
      .def_readwrite("max_trust_region_radius", &SolverOptions::max_trust_region_radius);
  m.def("DefaultSolverOptions", &DefaultSolverOptions);

  // IMU noise from a recording at rest (calico_imu_allan): stamps (n), samples (n, 3); options: None or a dict of
  // calico_allan_options fields (cluster_sizes: a list). Returns a dict: cluster_sizes, tau, rel_err, avar (c, 3), noise (three
  // dicts: Q, N, B, K, R, objective, terms_used, n_points, status) and summary.
  m.def(
      "CharacterizeImuNoise",
      [](const std::vector<double>& stamps, const py::array_t<double, py::array::c_style | py::array::forcecast>& samples, const py::object& options,
         int device) {
        if (samples.ndim() != 2 || samples.shape(1) != 3) throw py::value_error("samples must be (n, 3)");
        std::vector<Vector3d> y(size_t(samples.shape(0)));
        for (py::ssize_t i = 0; i < samples.shape(0); ++i) y[size_t(i)] = Vector3d(samples.at(i, 0), samples.at(i, 1), samples.at(i, 2));
        std::vector<int64_t> sizes;
        const calico_allan_options o = allan_options(options, &sizes);
        auto r = CharacterizeImuNoise(stamps, y, o, device);
        raise_if_error(r.status());
        return imu_noise_dict(r.value());
      },
      py::arg("stamps"), py::arg("samples"), py::arg("options") = py::none(), py::arg("device") = 0);

  // Rig calibration (calico_rig_calibrate): rig_frames[f] maps a camera's index in `cameras` to its detections {feature id:
  // pixel} in rig frame f; options: None or a dict of calico_rig_options fields. Sets the extrinsics of the cameras whose
  // status is OK when the estimation ends with status OK. Returns CalibrateRigFromChart's dict.
  m.def(
      "CalibrateRig",
      [](const std::vector<std::shared_ptr<Camera>>& cameras, const std::vector<std::map<int, std::map<int, Vector2d>>>& rig_frames,
         const py::dict& model_definition, const py::object& options, bool covariance, int device) {
        std::vector<Camera*> cams;
        for (const auto& c : cameras) cams.push_back(c.get());
        const calico_rig_options o = rig_options(options);
        RigCalibration r;
        raise_if_error(CalibrateRig(cams, rig_frames, to_model_definition(model_definition), &o, &r, covariance, device).status());
        return rig_dict(r, covariance);
      },
      py::arg("cameras"), py::arg("rig_frames"), py::arg("model_definition"), py::arg("options") = py::none(), py::arg("covariance") = false,
      py::arg("device") = 0);

  // the observability report: spectrum, directions and where they live, as numpy arrays / lists of (name, part, share)
  py::class_<Observability>(m, "Observability")
      .def("Dimension", &Observability::Dimension)
      .def("NumUnobserved", &Observability::NumUnobserved)
      .def("NumWeak", &Observability::NumWeak)
      .def("Sweeps", &Observability::Sweeps)
      .def("Eigenvalues",
           [](const Observability& o) {
             const std::vector<double> v = o.Eigenvalues();
             return py::array_t<double>(py::ssize_t(v.size()), v.data());
           })
      .def("Direction",
           [](const Observability& o, int i, bool tangent_units) {
             const std::vector<double> v = o.Direction(i, tangent_units);
             if (v.empty() && o.Dimension() > 0) throw std::out_of_range("observability: direction index out of range");
             return py::array_t<double>(py::ssize_t(v.size()), v.data());
           },
           py::arg("index"), py::arg("tangent_units") = false)
      .def("IntrinsicsShare",
           [](const Observability& o, int i, std::shared_ptr<Sensor> s) {
             auto sh = o.BlockShare(i, s->GetIntrinsics().data());
             raise_if_error(sh.status());
             return sh.value();
           })
      .def("Describe",
           [](const Observability& o, int i) {
             py::list out;
             for (const Observability::Entry& e : o.Describe(i)) out.append(py::make_tuple(e.name, e.part, e.share));
             return out;
           });

  // ceres::Covariance's result: per-sensor blocks as numpy arrays (tangent space: 6 x 6 extrinsics [rotation | translation])
  py::class_<Covariance>(m, "Covariance")
      .def("Dimension", &Covariance::Dimension)
      .def("NumUnobserved", &Covariance::NumUnobserved)
      .def("MinRelativePivot", &Covariance::MinRelativePivot)
      .def("Intrinsics",
           [](const Covariance& c, std::shared_ptr<Sensor> s) {
             std::vector<double> v;
             raise_if_error(SensorIntrinsicsCovariance(c, *s, &v));
             const py::ssize_t n = py::ssize_t(s->GetIntrinsics().size());
             return py::array_t<double>({n, n}, v.data());
           })
      .def("Extrinsics",
           [](const Covariance& c, std::shared_ptr<Sensor> s) {
             std::vector<double> v;
             raise_if_error(SensorExtrinsicsCovariance(c, *s, &v));
             return py::array_t<double>({py::ssize_t(6), py::ssize_t(6)}, v.data());
           })
      .def("Latency", [](const Covariance& c, std::shared_ptr<Sensor> s) {
        double v = 0.0;
        raise_if_error(SensorLatencyVariance(c, *s, &v));
        return v;
      })
      // the trajectory's blocks (ComputeCovariance(control_points=True)): control points i and j by their index in the spline,
      // and the spline's 6-vector at each stamp as an (n, 6, 6) array
      .def("ControlPoints",
           [](const Covariance& c, int i, int j) {
             std::vector<double> v(36);
             raise_if_error(c.ControlPoints(i, j, v.data()));
             return py::array_t<double>({py::ssize_t(6), py::ssize_t(6)}, v.data());
           })
      .def("Trajectory", [](const Covariance& c, const std::vector<double>& stamps) {
        std::vector<double> v;
        raise_if_error(c.TrajectoryCovariance(stamps, &v));
        return py::array_t<double>({py::ssize_t(stamps.size()), py::ssize_t(6), py::ssize_t(6)}, v.data());
      })
      // prediction covariance of a sensor's residual blocks (ComputeCovariance(control_points=True)): (cov (n, d, d),
      // leverage (n,), valid (n,) bool), in the order of the sensor's residual write-back
      .def("Predictions",
           [](const Covariance& c, std::shared_ptr<Sensor> s, bool apply_loss) {
             std::vector<double> cov, lev;
             std::vector<uint8_t> valid;
             raise_if_error(SensorPredictions(c, *s, apply_loss, &cov, &lev, &valid));
             const py::ssize_t n = py::ssize_t(lev.size());
             const py::ssize_t d = n > 0 ? py::ssize_t(std::lround(std::sqrt(double(cov.size() / lev.size())))) :
                                           (dynamic_cast<const sensors::Camera*>(s.get()) ? 2 : 3);
             py::array_t<bool> ok(n);
             for (py::ssize_t i = 0; i < n; ++i) ok.mutable_at(i) = valid[size_t(i)] != 0;
             return py::make_tuple(py::array_t<double>({n, d, d}, cov.data()), py::array_t<double>(n, lev.data()), ok);
           },
           py::arg("sensor"), py::arg("apply_loss") = true)
      // projection uncertainty map of a camera: ([s_uu, s_uv, s_vv] (n, 3) in pixels^2, valid (n,) bool)
      .def("ProjectionUncertainty",
           [](const Covariance& c, std::shared_ptr<Camera> camera, const py::object& pixels, double range, ProjectionFrame frame) {
             std::vector<std::array<double, 3>> cov;
             std::vector<uint8_t> valid;
             raise_if_error(c.ProjectionUncertainty(*camera, to_pixels(pixels), range, frame, &cov, &valid));
             py::array_t<double> a({py::ssize_t(cov.size()), py::ssize_t(3)});
             for (size_t i = 0; i < cov.size(); ++i)
               for (int k = 0; k < 3; ++k) a.mutable_at(py::ssize_t(i), k) = cov[i][size_t(k)];
             return py::make_tuple(a, to_bool_array(valid));
           },
           py::arg("camera"), py::arg("pixels"), py::arg("range") = 1.0, py::arg("frame") = ProjectionFrame::kRig);

  py::class_<BatchOptimizer>(m, "BatchOptimizer")
      .def(py::init<>())
      .def("AddSensor", [](BatchOptimizer& self, std::shared_ptr<Sensor> sensor) { self.AddSensor(sensor.get(), /*take_ownership=*/false); },
           py::keep_alive<1, 2>())
      .def("AddTrajectory",
           [](BatchOptimizer& self, std::shared_ptr<Trajectory> trajectory) { self.AddTrajectory(trajectory.get(), /*take_ownership=*/false); },
           py::keep_alive<1, 2>())
      .def("AddWorldModel",
           [](BatchOptimizer& self, std::shared_ptr<WorldModel> world_model) { self.AddWorldModel(world_model.get(), /*take_ownership=*/false); },
           py::keep_alive<1, 2>())
      .def(
          "Optimize",
          [](BatchOptimizer& self, const SolverOptions& options, int device) {
            auto summary = self.Optimize(options, device);
            raise_if_error(summary.status());
            return summary.value();
          },
          py::arg("options") = DefaultSolverOptions(), py::arg("device") = 0)
      .def(
          "ComputeCovariance",
          [](BatchOptimizer& self, double min_relative_pivot, int device, bool control_points) {
            calico_covariance_options o = DefaultCovarianceOptions();
            if (min_relative_pivot >= 0.0) o.min_relative_pivot = min_relative_pivot;
            o.control_points = control_points ? 1 : 0;
            auto cov = self.ComputeCovariance(o, device);
            raise_if_error(cov.status());
            return cov.value();
          },
          py::arg("min_relative_pivot") = -1.0, py::arg("device") = 0, py::arg("control_points") = false)
      .def(
          "AnalyzeObservability",
          [](BatchOptimizer& self, double weak_threshold, double min_relative_pivot, int device) {
            calico_observability_options o = DefaultObservabilityOptions();
            if (weak_threshold >= 0.0) o.weak_threshold = weak_threshold;
            if (min_relative_pivot >= 0.0) o.min_relative_pivot = min_relative_pivot;
            auto obs = self.AnalyzeObservability(o, device);
            raise_if_error(obs.status());
            return obs.value();
          },
          py::arg("weak_threshold") = -1.0, py::arg("min_relative_pivot") = -1.0, py::arg("device") = 0);
}
