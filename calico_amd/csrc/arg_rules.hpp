// arg_rules.hpp — the argument rules the calls without a problem handle share (chart.cpp, fit.cpp, imu_align.cpp, rig.cpp, camera_align.cpp, accel_align.cpp, allan.cpp), free of HIP:
// the standard library and the C header only, so a plain host program can test them (tests/cpp/arg_rules_check.cpp). A rule
// returns an empty string for "fine", or the message without the call's name (FreeCall, free_call.hpp, puts that in front).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/calico_hip.h"

namespace cal {

// ---- a camera model with its intrinsics (num_params: camera_model_num_params(model), -1: no such model), a count with its buffers ----
inline std::string camera_model_error(int model, int num_params, const double* intrinsics, int n_intrinsics) {
  if (num_params < 0) return "unknown camera model " + std::to_string(model);
  if (n_intrinsics != num_params)
    return "camera model " + std::to_string(model) + " has " + std::to_string(num_params) + " intrinsics, got " + std::to_string(n_intrinsics);
  if (!intrinsics) return "null intrinsics";
  return "";
}
inline std::string count_error(int64_t n, bool pointers_ok) {
  if (n < 0) return "n must be >= 0";
  if (n > 0 && !pointers_ok) return "null input or output buffer";
  return "";
}

// ---- the chart batch of calico_camera_resect / calico_camera_calibrate: what holds whatever n_frames is (Options: either call's) ----
template <class Options>
std::string chart_options_error(int64_t n_frames, const Options& o, const double* q_init, const double* t_init) {
  if (n_frames < 0) return "n_frames must be >= 0";
  if (!std::isfinite(o.step_tolerance) || !(o.step_tolerance > 0.0)) return "step_tolerance must be finite and > 0";
  if (o.max_iterations < 1) return "max_iterations must be >= 1";
  if (!std::isfinite(o.huber_scale) || o.huber_scale < 0.0) return "huber_scale must be finite and >= 0";
  if (o.min_points < 4) return "min_points must be >= 4";
  if ((q_init == nullptr) != (t_init == nullptr)) return "q_init and t_init are given together or not at all";
  return "";
}
// The frames of a batch with n_frames > 0 (n_frames + 1 offsets). outputs: the call has all its output buffers (`null_text` names them).
inline std::string chart_frames_error(int64_t n_frames, const int64_t* offsets, bool outputs, const char* null_text, const double* pixels,
                                      const double* points) {
  if (!offsets || !outputs) return null_text;
  if (offsets[0] != 0) return "frame_offsets must start at 0";
  for (int64_t f = 0; f < n_frames; ++f)
    if (offsets[f + 1] < offsets[f]) return "frame_offsets decrease at frame " + std::to_string(f);
  if (offsets[n_frames] > 0 && (!pixels || !points)) return "null pixels or points";
  return "";
}

// ---- the rig of calico_rig_calibrate: cameras with their models and intrinsics (num_params[c]: camera_model_num_params of
// models[c]), and what its options and starts must satisfy whatever the views are ----
inline std::string rig_cameras_error(int n_cameras, int max_cameras, const int32_t* models, const int* num_params, const int64_t* intrinsics_offsets,
                                     const double* intrinsics) {
  if (n_cameras < 1 || n_cameras > max_cameras) return "n_cameras must be in [1, " + std::to_string(max_cameras) + "]";
  if (!models || !intrinsics_offsets || !intrinsics) return "null models, intrinsics_offsets or intrinsics";
  if (intrinsics_offsets[0] != 0) return "intrinsics_offsets must start at 0";
  for (int c = 0; c < n_cameras; ++c) {
    if (num_params[c] < 0) return "unknown camera model " + std::to_string(models[c]) + " of camera " + std::to_string(c);
    if (intrinsics_offsets[c + 1] - intrinsics_offsets[c] != num_params[c])
      return "camera " + std::to_string(c) + " of model " + std::to_string(models[c]) + " has " + std::to_string(num_params[c]) +
             " intrinsics, its offsets give " + std::to_string(intrinsics_offsets[c + 1] - intrinsics_offsets[c]);
  }
  return "";
}
inline std::string rig_options_error(int n_cameras, int64_t n_frames, int64_t n_views, const calico_rig_options& o, const double* q_camera_init,
                                     const double* t_camera_init, const double* q_frame_init, const double* t_frame_init) {
  if (n_views < 0) return "n_views must be >= 0";
  std::string error = chart_options_error(n_frames, o, q_camera_init, t_camera_init);
  if (!error.empty()) return error;
  if ((q_frame_init == nullptr) != (t_frame_init == nullptr)) return "q_frame_init and t_frame_init are given together or not at all";
  if (q_frame_init && !q_camera_init) return "a start of the frames needs a start of the cameras";
  if (o.reference_camera < 0 || o.reference_camera >= n_cameras) return "reference_camera must be in [0, n_cameras)";
  if (o.min_shared_frames < 1) return "min_shared_frames must be >= 1";
  return "";
}
// The views of a rig with n_views > 0: `order` (n_views) receives them sorted by (frame, camera).
inline std::string rig_views_error(int n_cameras, int64_t n_frames, int64_t n_views, const int32_t* view_camera, const int64_t* view_frame,
                                   const int64_t* view_offsets, const double* pixels, const double* points, int64_t* order) {
  if (!view_camera || !view_frame || !view_offsets) return "null view_camera, view_frame or view_offsets";
  if (view_offsets[0] != 0) return "view_offsets must start at 0";
  for (int64_t v = 0; v < n_views; ++v) {
    if (view_offsets[v + 1] < view_offsets[v]) return "view_offsets decrease at view " + std::to_string(v);
    if (view_camera[v] < 0 || view_camera[v] >= n_cameras) return "view " + std::to_string(v) + " names camera " + std::to_string(view_camera[v]);
    if (view_frame[v] < 0 || view_frame[v] >= n_frames) return "view " + std::to_string(v) + " names frame " + std::to_string(view_frame[v]);
  }
  if (view_offsets[n_views] > 0 && (!pixels || !points)) return "null pixels or points";
  for (int64_t v = 0; v < n_views; ++v) order[v] = v;
  std::sort(order, order + n_views, [&](int64_t x, int64_t y) {
    return view_frame[x] != view_frame[y] ? view_frame[x] < view_frame[y] : view_camera[x] < view_camera[y];
  });
  for (int64_t s = 1; s < n_views; ++s)
    if (view_frame[order[s]] == view_frame[order[s - 1]] && view_camera[order[s]] == view_camera[order[s - 1]])
      return "camera " + std::to_string(view_camera[order[s]]) + " has two views of frame " + std::to_string(view_frame[order[s]]);
  return "";
}

// ---- a spline given as (order, knots) ----
inline int spline_valid_knots(int order, int n_knots) { return n_knots - 2 * (order - 1); }      // segments: one fewer
inline std::string spline_shape_error(int order, int n_knots, int max_order) {
  if (order < 2 || order > max_order) return "order must be in [2, " + std::to_string(max_order) + "]";
  if (n_knots < 2 * order) return "n_knots must be >= 2 order";
  if (spline_valid_knots(order, n_knots) < 2) return "the knots hold no segment";
  return "";
}
// GetSplineIndex (bspline.hpp:138-150): upper_bound(valid_knots, t) - 1, the last valid knot belongs to the last segment.
// -1 where t lies outside the valid knots (or is not a number). valid_knots = knots + order - 1, n_valid of them.
inline int spline_segment(const double* valid_knots, int n_valid, double t) {
  if (!(t >= valid_knots[0]) || !(t <= valid_knots[n_valid - 1])) return -1;
  return std::min(int(std::upper_bound(valid_knots, valid_knots + n_valid, t) - valid_knots) - 1, n_valid - 2);
}

// ---- sample stamps: finite and sorted (equal neighbours are fine) ----
inline std::string stamps_error(const char* name, int64_t n, const double* stamps) {
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(stamps[i])) return std::string(name) + " stamp " + std::to_string(i) + " is not finite";
    if (i > 0 && stamps[i] < stamps[i - 1]) return std::string(name) + " stamps are not sorted: they decrease at sample " + std::to_string(i);
  }
  return "";
}

// ---- the latency grid of calico_camera_align (calico_imu_align's rule): latency0 + l lag_step, |l| <= half ----
// half_out: floor(max_lag / lag_step) with 1e-9 relative slack.
inline std::string lag_grid_error(double max_lag, double lag_step, int max_lags, int* half_out) {
  if (!std::isfinite(lag_step) || !(lag_step > 0.0)) return "lag_step must be finite and > 0";
  if (!std::isfinite(max_lag) || max_lag < 0.0) return "max_lag must be finite and >= 0";
  const double half = std::floor(max_lag / lag_step * (1.0 + 1e-9));
  if (!(2.0 * half + 1.0 <= double(max_lags))) return "max_lag / lag_step gives more than " + std::to_string(max_lags) + " lags";
  *half_out = int(half);
  return "";
}

// ---- calico_camera_align: its options (the chart batch's rules hold too), T_world_chart and its start ----
inline std::string camera_alignment_options_error(const calico_camera_alignment_options& o, int max_lags, int* half_out) {
  const std::string error = lag_grid_error(o.max_lag, o.lag_step, max_lags, half_out);
  if (!error.empty()) return error;
  if (!std::isfinite(o.sigma_pixel) || !(o.sigma_pixel > 0.0)) return "sigma_pixel must be finite and > 0";
  if (o.min_frames < 3) return "min_frames must be >= 3";
  return "";
}
inline double quat_norm(const double* q);
inline std::string camera_alignment_start_error(const double* q_world_chart, const double* t_world_chart, const double* q_init,
                                                const double* t_init, const double* latency_init) {
  if (q_world_chart) {
    const double n = quat_norm(q_world_chart);
    if (!std::isfinite(n) || !(n > 0.0)) return "q_world_chart must be finite and of non-zero length";
  }
  if (t_world_chart && !(std::isfinite(t_world_chart[0]) && std::isfinite(t_world_chart[1]) && std::isfinite(t_world_chart[2])))
    return "t_world_chart must be finite";
  const int given = (q_init ? 1 : 0) + (t_init ? 1 : 0) + (latency_init ? 1 : 0);
  if (given != 0 && given != 3) return "q_init, t_init and latency_init are given together or not at all";
  if (given == 0) return "";
  const double n = quat_norm(q_init);
  if (!std::isfinite(n) || !(n > 0.0)) return "q_init must be finite and of non-zero length";
  if (!(std::isfinite(t_init[0]) && std::isfinite(t_init[1]) && std::isfinite(t_init[2]))) return "t_init must be finite";
  if (!std::isfinite(*latency_init)) return "latency_init must be finite";
  return "";
}

// ---- the smoothing fit of calico_fit_spline_smooth: its options, and the sample weights (n x 2; n_used[g]: weights > 0 of column g) ----
inline std::string spline_fit_options_error(int order, const calico_spline_fit_options& o) {
  const int m_max = std::min(3, order - 1);
  if (o.derivative < 1 || o.derivative > m_max) return "derivative must be in [1, " + std::to_string(m_max) + "] at order " + std::to_string(order);
  if (o.n_lambda < 1 || o.n_lambda > CALICO_FIT_MAX_LAMBDAS) return "n_lambda must be in [1, " + std::to_string(CALICO_FIT_MAX_LAMBDAS) + "]";
  for (int g = 0; g < 2; ++g) {
    const double* grid = g == 0 ? o.lambda_rot : o.lambda_pos;
    const char* name = g == 0 ? "lambda_rot" : "lambda_pos";
    for (int l = 0; l < o.n_lambda; ++l) {
      if (!std::isfinite(grid[l]) || grid[l] < 0.0) return std::string(name) + "[" + std::to_string(l) + "] must be finite and >= 0";
      if (l > 0 && !(grid[l] > grid[l - 1])) return std::string(name) + " must be strictly ascending: entry " + std::to_string(l) + " is not";
    }
    const double target = g == 0 ? o.target_rms_rot : o.target_rms_pos;
    if (!std::isfinite(target) || target < 0.0) return std::string(g == 0 ? "target_rms_rot" : "target_rms_pos") + " must be finite and >= 0";
  }
  return "";
}
// calico_fit_spline_robust: what it asks of the smoothing fit's options (already valid) and of its own
inline std::string spline_robust_options_error(const calico_spline_fit_options& fit, const calico_spline_robust_options& o) {
  if (fit.n_lambda != 1) return "n_lambda must be 1: the robust fit takes one lambda per group";
  if (fit.target_rms_rot != 0.0 || fit.target_rms_pos != 0.0) return "target_rms_rot and target_rms_pos must be 0: the robust fit chooses no lambda";
  if (o.loss != CALICO_ROBUST_HUBER && o.loss != CALICO_ROBUST_TUKEY) return "unknown loss " + std::to_string(o.loss);
  if (o.max_iterations < 0 || o.max_iterations > CALICO_FIT_ROBUST_ITERATION_LIMIT)
    return "max_iterations must be in [0, " + std::to_string(CALICO_FIT_ROBUST_ITERATION_LIMIT) + "]";
  const struct { const char* name; double v; } fields[] = {
      {"tuning_rot", o.tuning_rot}, {"tuning_pos", o.tuning_pos}, {"scale_rot", o.scale_rot}, {"scale_pos", o.scale_pos},
      {"min_scale_rot", o.min_scale_rot}, {"min_scale_pos", o.min_scale_pos}, {"step_tolerance", o.step_tolerance}};
  for (const auto& f : fields)
    if (!std::isfinite(f.v) || f.v < 0.0) return std::string(f.name) + " must be finite and >= 0";
  return "";
}
// calico_fit_spline_cv: what it asks of the smoothing fit's options (already valid) and of its own
inline std::string spline_cv_options_error(const calico_spline_fit_options& fit, const calico_spline_cv_options& o) {
  if (fit.target_rms_rot != 0.0 || fit.target_rms_pos != 0.0) return "target_rms_rot and target_rms_pos must be 0: the cross-validated fit chooses lambda itself";
  if (o.criterion != CALICO_FIT_CV_GCV && o.criterion != CALICO_FIT_CV_PRESS) return "unknown criterion " + std::to_string(o.criterion);
  return "";
}
inline std::string sample_weights_error(int64_t n, const double* weights, int64_t n_used[2]) {
  n_used[0] = n_used[1] = weights ? 0 : n;
  if (!weights) return "";
  for (int64_t j = 0; j < n; ++j)
    for (int g = 0; g < 2; ++g) {
      const double w = weights[j * 2 + g];
      if (!std::isfinite(w) || w < 0.0) return "weight " + std::to_string(g) + " of sample " + std::to_string(j) + " must be finite and >= 0";
      n_used[g] += w > 0.0;
    }
  for (int g = 0; g < 2; ++g)
    if (n_used[g] == 0) return std::string(g == 0 ? "rotation" : "position") + " weights: no sample has a weight > 0";
  return "";
}

// ---- calico_imu_allan: its options, the rate of its log, and its grid of cluster sizes ----
inline std::string allan_options_error(const calico_allan_options& o) {
  constexpr int all_terms = CALICO_ALLAN_TERM_QUANTISATION | CALICO_ALLAN_TERM_WHITE | CALICO_ALLAN_TERM_BIAS_INSTABILITY |
                            CALICO_ALLAN_TERM_RATE_RANDOM_WALK | CALICO_ALLAN_TERM_RAMP;
  if (o.terms == 0 || (o.terms & ~all_terms) != 0) return "terms must be a non-empty mask of CALICO_ALLAN_TERM_* bits";
  if (o.n_cluster_sizes < 0 || o.n_cluster_sizes > CALICO_ALLAN_MAX_CLUSTERS)
    return "n_cluster_sizes must be in [0, " + std::to_string(CALICO_ALLAN_MAX_CLUSTERS) + "]";
  if (o.n_cluster_sizes > 0) return o.cluster_sizes ? "" : "null cluster_sizes";
  if (o.points_per_decade < 1) return "points_per_decade must be >= 1";
  if (!std::isfinite(o.max_tau_fraction) || !(o.max_tau_fraction > 0.0) || o.max_tau_fraction > 0.5) return "max_tau_fraction must be in (0, 0.5]";
  return "";
}
// The rate: from the stamps where they are given ((n - 1) / span; they are finite, strictly increasing, and no step leaves
// [0.5, 1.5] / rate), otherwise the caller's. n >= 3.
inline std::string allan_rate_error(int64_t n, const double* stamps, double sample_rate_hz, double* rate_out) {
  if (!stamps) {
    if (!std::isfinite(sample_rate_hz) || !(sample_rate_hz > 0.0)) return "sample_rate_hz must be finite and > 0 where no stamps are given";
    *rate_out = sample_rate_hz;
    return "";
  }
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(stamps[i])) return "stamp " + std::to_string(i) + " is not finite";
    if (i > 0 && !(stamps[i] > stamps[i - 1])) return "stamps must be strictly increasing: sample " + std::to_string(i) + " is not later than the one before";
  }
  const double rate = double(n - 1) / (stamps[n - 1] - stamps[0]);
  if (!std::isfinite(rate) || !(rate > 0.0)) return "the stamps give no rate";
  for (int64_t i = 1; i < n; ++i) {
    const double steps = (stamps[i] - stamps[i - 1]) * rate;
    if (!(steps >= 0.5 && steps <= 1.5))
      return "the step to sample " + std::to_string(i) + " is " + std::to_string(steps) + " of the mean step (a gap: split the log)";
  }
  *rate_out = rate;
  return "";
}
// m_out (CALICO_ALLAN_MAX_CLUSTERS): the caller's list, or the distinct floor(10^(i / points_per_decade) + 1/2) up to max_tau_fraction n.
inline std::string allan_grid_error(int64_t n, const calico_allan_options& o, int64_t* m_out, int* n_out) {
  int count = 0;
  if (o.n_cluster_sizes > 0) {
    for (int j = 0; j < o.n_cluster_sizes; ++j) {
      const int64_t m = o.cluster_sizes[j];
      if (m < 1 || m >= n || 2 * m >= n) return "cluster size " + std::to_string(j) + " must satisfy 1 <= m and 2 m < n";
      if (j > 0 && m <= o.cluster_sizes[j - 1]) return "cluster_sizes must be strictly increasing: entry " + std::to_string(j) + " is not";
      m_out[count++] = m;
    }
  } else {
    for (int i = 0; count < CALICO_ALLAN_MAX_CLUSTERS; ++i) {
      const double v = std::floor(std::pow(10.0, double(i) / double(o.points_per_decade)) + 0.5);
      if (!(v <= o.max_tau_fraction * double(n)) || !(2.0 * v < double(n))) break;
      const int64_t m = int64_t(v);
      if (count == 0 || m > m_out[count - 1]) m_out[count++] = m;
    }
    if (count == 0) return "the log is too short: no cluster size m has m <= max_tau_fraction n";
  }
  *n_out = count;
  return "";
}

// ---- a caller's quaternion (x, y, z, w) as the unit quaternion with w >= 0; which lengths are an error is the caller's rule ----
inline double quat_norm(const double* q) { return std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]); }
inline void canonical_unit_quat(const double* q, double norm, double* out) {
  const double sg = (q[3] < 0.0 ? -1.0 : 1.0) / norm;
  for (int i = 0; i < 4; ++i) out[i] = sg * q[i];
}

}  // namespace cal
