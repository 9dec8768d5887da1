"""ctypes binding of the C ABI declared in include/calico_hip.h.

`CApi(lib, prefix)` binds one shared library exporting that ABI under a symbol
prefix. The product uses `load_hip()` (libcalico_hip.so, prefix "calico_");
there is no CPU fallback: if the HIP library is missing or no GPU is usable the
call fails loudly. tests/ bind the CPU oracle through the same class with
prefix "oracle_" (see tests/helpers.py) - never the product.
"""
import ctypes as C
import os

import numpy as np

OK, INVALID_ARGUMENT, FAILED_PRECONDITION, UNIMPLEMENTED, INTERNAL = 0, 3, 9, 12, 13
MANIFOLD_EUCLIDEAN, MANIFOLD_EIGEN_QUATERNION = 0, 1
SENSOR_CAMERA, SENSOR_GYROSCOPE, SENSOR_ACCELEROMETER = 0, 1, 2
CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2
FRAME_CAMERA, FRAME_RIG = 0, 1
CAMERA_NUM_PARAMS = {1: 8, 2: 11, 3: 7, 4: 5, 5: 4, 6: 4, 7: 5}      # sensors::CameraIntrinsicsModel -> intrinsics count


class SolverOptions(C.Structure):
    """calico_solver_options (ceres::Solver::Options fields the path uses)."""
    _fields_ = [
        ("max_num_iterations", C.c_int32),
        ("num_threads", C.c_int32),
        ("minimizer_progress_to_stdout", C.c_int32),
        ("jacobi_scaling", C.c_int32),
        ("max_num_consecutive_invalid_steps", C.c_int32),
        ("sync_every", C.c_int32),
        ("function_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double),
        ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double),
        ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double),
        ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double),
    ]


class Summary(C.Structure):
    """calico_summary (ceres::Solver::Summary fields the reference binds)."""
    _fields_ = [
        ("termination_type", C.c_int32),
        ("num_successful_steps", C.c_int32),
        ("num_unsuccessful_steps", C.c_int32),
        ("num_iterations", C.c_int32),
        ("num_jacobian_evaluations", C.c_int32),
        ("num_cost_evaluations", C.c_int32),
        ("num_residual_blocks", C.c_int32),
        ("num_residuals", C.c_int32),
        ("num_parameter_blocks", C.c_int32),
        ("num_parameters", C.c_int32),
        ("num_effective_parameters", C.c_int32),
        ("num_residual_blocks_reduced", C.c_int32),
        ("num_residuals_reduced", C.c_int32),
        ("num_parameter_blocks_reduced", C.c_int32),
        ("num_parameters_reduced", C.c_int32),
        ("num_effective_parameters_reduced", C.c_int32),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("total_time_in_seconds", C.c_double),
        ("solve_time_in_seconds", C.c_double),
        ("message", C.c_char * 256),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["message"] = d["message"].decode()
        return d


class CovarianceOptions(C.Structure):
    """calico_covariance_options."""
    _fields_ = [("min_relative_pivot", C.c_double), ("control_points", C.c_int32), ("reserved", C.c_int32 * 5)]


class ObservabilityOptions(C.Structure):
    """calico_observability_options."""
    _fields_ = [("weak_threshold", C.c_double), ("min_relative_pivot", C.c_double), ("reserved", C.c_int32 * 4)]


class PredictionOptions(C.Structure):
    """calico_prediction_options."""
    _fields_ = [("apply_loss", C.c_int32), ("reserved", C.c_int32 * 7)]


class ResectionOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("step_tolerance", C.c_double), ("huber_scale", C.c_double), ("min_points", C.c_int32)]


RESECT_OK, RESECT_TOO_FEW_POINTS, RESECT_NO_START, RESECT_NOT_CONVERGED, RESECT_DEGENERATE = 0, 1, 2, 3, 4
RESECT_NOT_POSITIVE_DEFINITE = 5      # (calibration only: the frame dropped out)


class CalibrationOptions(C.Structure):
    """calico_calibration_options."""
    _fields_ = [("max_iterations", C.c_int32), ("step_tolerance", C.c_double), ("huber_scale", C.c_double), ("min_points", C.c_int32)]


class CalibrationSummary(C.Structure):
    """calico_calibration_summary."""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("rms", C.c_double), ("frames_used", C.c_int32), ("pairs_used", C.c_int64), ("lambda_", C.c_double)]


CALIB_OK, CALIB_TOO_FEW_FRAMES, CALIB_NOT_CONVERGED, CALIB_DEGENERATE = 0, 1, 2, 3


class RigOptions(C.Structure):
    """calico_rig_options."""
    _fields_ = [("max_iterations", C.c_int32), ("step_tolerance", C.c_double), ("huber_scale", C.c_double), ("min_points", C.c_int32),
                ("min_shared_frames", C.c_int32), ("reference_camera", C.c_int32)]


class RigSummary(C.Structure):
    """calico_rig_summary."""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("rms", C.c_double), ("cameras_used", C.c_int32), ("frames_used", C.c_int32), ("views_used", C.c_int64),
                ("pairs_used", C.c_int64), ("lambda_", C.c_double)]


RIG_MAX_CAMERAS = 8
RIG_OK, RIG_TOO_FEW_VIEWS, RIG_NOT_CONVERGED, RIG_DEGENERATE = 0, 1, 2, 3
RIG_CAMERA_OK, RIG_CAMERA_REFERENCE, RIG_CAMERA_UNCONNECTED = 0, 1, 2
RIG_FRAME_OK, RIG_FRAME_NO_VIEW, RIG_FRAME_NOT_POSITIVE_DEFINITE = 0, 1, 2


class ImuAlignmentOptions(C.Structure):
    """calico_imu_alignment_options."""
    _fields_ = [("max_lag", C.c_double), ("lag_step", C.c_double), ("max_iterations", C.c_int32), ("step_tolerance", C.c_double),
                ("estimate_latency", C.c_int32), ("estimate_gyro_bias", C.c_int32), ("estimate_accel_bias", C.c_int32),
                ("min_samples", C.c_int32), ("sigma_gyro", C.c_double)]


class ImuAlignmentSummary(C.Structure):
    """calico_imu_alignment_summary."""
    _fields_ = [("gyro_status", C.c_int32), ("accel_status", C.c_int32), ("gyro_samples", C.c_int64), ("accel_samples", C.c_int64),
                ("first_sample", C.c_int64), ("iterations", C.c_int32), ("n_lags", C.c_int32), ("peak_index", C.c_int32),
                ("coarse_latency", C.c_double), ("peak_correlation", C.c_double), ("gyro_rms", C.c_double), ("accel_rms", C.c_double),
                ("gravity_norm", C.c_double), ("scatter_pivot", C.c_double), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("lambda_", C.c_double)]


class CameraAlignmentOptions(C.Structure):
    """calico_camera_alignment_options."""
    _fields_ = [("max_lag", C.c_double), ("lag_step", C.c_double), ("max_iterations", C.c_int32), ("step_tolerance", C.c_double),
                ("estimate_latency", C.c_int32), ("estimate_translation", C.c_int32), ("huber_scale", C.c_double),
                ("min_points", C.c_int32), ("min_frames", C.c_int32), ("sigma_pixel", C.c_double)]


class CameraAlignmentSummary(C.Structure):
    """calico_camera_alignment_summary."""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("frames_used", C.c_int64), ("pairs_used", C.c_int64),
                ("n_lags", C.c_int32), ("peak_index", C.c_int32), ("coarse_latency", C.c_double), ("peak_score", C.c_double),
                ("rms", C.c_double), ("initial_cost", C.c_double), ("final_cost", C.c_double), ("lambda_", C.c_double)]


class AccelAlignmentOptions(C.Structure):
    """calico_accel_alignment_options."""
    _fields_ = [("max_iterations", C.c_int32), ("step_tolerance", C.c_double), ("estimate_rotation", C.c_int32),
                ("estimate_lever_arm", C.c_int32), ("estimate_bias", C.c_int32), ("estimate_gravity", C.c_int32),
                ("estimate_latency", C.c_int32), ("min_samples", C.c_int32), ("sigma_accel", C.c_double)]


class AccelAlignmentSummary(C.Structure):
    """calico_accel_alignment_summary."""
    _fields_ = [("status", C.c_int32), ("linear_status", C.c_int32), ("samples", C.c_int64), ("first_sample", C.c_int64),
                ("iterations", C.c_int32), ("rms", C.c_double), ("linear_rms", C.c_double), ("gravity_norm", C.c_double),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("lambda_", C.c_double)]


CAMERA_ALIGN_FRAME_OUTSIDE = 6      # a frame status beside RESECT_*: outside the trajectory
ALIGN_OK, ALIGN_TOO_FEW_SAMPLES, ALIGN_NO_PEAK, ALIGN_DEGENERATE, ALIGN_NOT_CONVERGED, ALIGN_NOT_POSITIVE_DEFINITE = 0, 1, 2, 3, 4, 5
ALIGN_MAX_LAGS = 4096

FIT_MAX_LAMBDAS = 32
FIT_OK, FIT_NOT_POSITIVE_DEFINITE, FIT_TARGET_NOT_MET = 0, 1, 2
FIT_MAX_ITERATIONS, FIT_SCALE_ZERO = 3, 4      # group statuses of the robust fit
ROBUST_HUBER, ROBUST_TUKEY = 1, 2
FIT_ROBUST_ITERATION_LIMIT = 64
FIT_CV_AT_GRID_END = 5                         # group status of the cross-validated fit
FIT_CV_GCV, FIT_CV_PRESS = 0, 1


class SplineFitOptions(C.Structure):
    """calico_spline_fit_options."""
    _fields_ = [("derivative", C.c_int32), ("relative", C.c_int32), ("n_lambda", C.c_int32), ("lambda_rot", C.c_double * FIT_MAX_LAMBDAS),
                ("lambda_pos", C.c_double * FIT_MAX_LAMBDAS), ("target_rms_rot", C.c_double), ("target_rms_pos", C.c_double)]


class SplineFitRow(C.Structure):
    """calico_spline_fit_row."""
    _fields_ = [("status", C.c_int32), ("replaced_pivots", C.c_int32), ("lambda_", C.c_double), ("rss", C.c_double), ("penalty", C.c_double),
                ("rms", C.c_double)]


class SplineFitSummary(C.Structure):
    """calico_spline_fit_summary."""
    _fields_ = [("status", C.c_int32 * 2), ("chosen", C.c_int32 * 2), ("n_used", C.c_int64 * 2)]


class SplineRobustOptions(C.Structure):
    """calico_spline_robust_options."""
    _fields_ = [("loss", C.c_int32), ("max_iterations", C.c_int32), ("tuning_rot", C.c_double), ("tuning_pos", C.c_double),
                ("scale_rot", C.c_double), ("scale_pos", C.c_double), ("min_scale_rot", C.c_double), ("min_scale_pos", C.c_double),
                ("step_tolerance", C.c_double)]


class SplineRobustSummary(C.Structure):
    """calico_spline_robust_summary: one entry per group."""
    _fields_ = [("status", C.c_int32 * 2), ("iterations", C.c_int32 * 2), ("replaced_pivots", C.c_int32 * 2), ("n_used", C.c_int64 * 2),
                ("n_downweighted", C.c_int64 * 2), ("n_rejected", C.c_int64 * 2), ("lambda_", C.c_double * 2), ("scale", C.c_double * 2),
                ("median_residual", C.c_double * 2), ("last_step", C.c_double * 2), ("rss", C.c_double * 2)]


class SplineCvOptions(C.Structure):
    """calico_spline_cv_options."""
    _fields_ = [("criterion", C.c_int32), ("reserved", C.c_int32)]


class SplineCvRow(C.Structure):
    """calico_spline_cv_row."""
    _fields_ = [("edf", C.c_double), ("gcv", C.c_double), ("press", C.c_double), ("max_leverage", C.c_double)]


class SplineCvSummary(C.Structure):
    """calico_spline_cv_summary: one entry per group."""
    _fields_ = [("status", C.c_int32 * 2), ("chosen", C.c_int32 * 2), ("n_used", C.c_int64 * 2), ("edf", C.c_double * 2), ("score", C.c_double * 2)]


class AllanOptions(C.Structure):
    """calico_allan_options."""
    _fields_ = [("points_per_decade", C.c_int32), ("terms", C.c_int32), ("max_tau_fraction", C.c_double), ("n_cluster_sizes", C.c_int32),
                ("reserved", C.c_int32), ("cluster_sizes", C.POINTER(C.c_int64))]


class AllanNoise(C.Structure):
    """calico_allan_noise: one axis."""
    _fields_ = [("Q", C.c_double), ("N", C.c_double), ("B", C.c_double), ("K", C.c_double), ("R", C.c_double), ("objective", C.c_double),
                ("terms_used", C.c_int32), ("n_points", C.c_int32), ("status", C.c_uint8), ("reserved", C.c_uint8 * 7)]


class AllanSummary(C.Structure):
    """calico_allan_summary."""
    _fields_ = [("n", C.c_int64), ("sample_rate_hz", C.c_double), ("duration", C.c_double), ("N_pooled", C.c_double),
                ("sigma_at_rate", C.c_double), ("bias_drift_over_recording", C.c_double)]


ALLAN_MAX_CLUSTERS = 256
ALLAN_TERM_QUANTISATION, ALLAN_TERM_WHITE, ALLAN_TERM_BIAS_INSTABILITY, ALLAN_TERM_RATE_RANDOM_WALK, ALLAN_TERM_RAMP = 1, 2, 4, 8, 16
ALLAN_OK, ALLAN_NO_WHITE_NOISE, ALLAN_TOO_FEW_POINTS, ALLAN_NONFINITE = 0, 1, 2, 3


class Iteration(C.Structure):
    _fields_ = [
        ("iteration", C.c_int32),
        ("step_is_valid", C.c_int32),
        ("step_is_successful", C.c_int32),
        ("reserved", C.c_int32),
        ("cost", C.c_double),
        ("cost_change", C.c_double),
        ("gradient_max_norm", C.c_double),
        ("step_norm", C.c_double),
        ("relative_decrease", C.c_double),
        ("trust_region_radius", C.c_double),
    ]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)


class CalicoError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("Error: %s (status %d)" % (message, code))
        self.code = code
        self.message = message


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


# Every symbol include/calico_hip.h declares (without prefix).
ABI_SYMBOLS = [
    "problem_create", "problem_destroy", "last_error", "default_solver_options",
    "problem_add_param_block", "problem_add_param_blocks", "get_param_block", "set_param_block", "set_param_blocks", "get_param_blocks",
    "problem_set_spline", "problem_add_rigid_body", "problem_add_sensor",
    "problem_add_camera_residuals", "problem_add_imu_residuals", "solve",
    "get_iterations", "get_residuals", "get_inlier_mask",
    "num_effective_parameters", "evaluate", "problem_set_allreduce", "problem_set_shard",
    "problem_set_stream", "get_phase_time", "set_phase_timing", "project",
    "problem_set_outlier_mask", "mark_outliers", "fit_spline", "residual_heatmap",
    "comm_get_unique_id", "comm_init_rccl", "comm_info", "problem_finalize", "plan_cache_stats", "plan_cache_clear",
    "default_covariance_options", "covariance_compute", "covariance_info", "covariance_get_dense", "covariance_get_block",
    "covariance_trajectory", "covariance_trajectory_info",
    "default_prediction_options", "prediction_covariance",
    "default_observability_options", "observability_compute", "observability_info", "observability_get_spectrum",
    "observability_get_directions", "observability_get_block", "observability_get_matrix",
    "camera_unproject", "camera_project_points", "sensor_unproject", "projection_uncertainty",
    "default_resection_options", "camera_resect",
    "default_calibration_options", "camera_calibrate",
    "default_imu_alignment_options", "imu_align",
    "default_camera_alignment_options", "camera_align",
    "default_accel_alignment_options", "accel_align",
    "default_rig_options", "rig_calibrate",
    "default_spline_fit_options", "fit_spline_smooth",
    "default_spline_robust_options", "fit_spline_robust",
    "default_spline_cv_options", "fit_spline_cv",
    "default_allan_options", "imu_allan",
]
# Test hooks (calico_amd/csrc/calico_hip_testing.h): exported, not part of the drop-in surface.
TEST_SYMBOLS = ["debug_lm_control_replay", "debug_plan_info", "debug_roll_table", "debug_last_step", "debug_observability_info",
                "debug_lds_attribute_calls", "debug_camera_unproject_chunked", "debug_panel_product", "debug_block_elim",
                "debug_camera_resect_chunked"]


class CApi:
    """Functions of one shared library exporting the calico C ABI."""

    def __init__(self, lib, prefix, has_device=True):
        self.lib = lib
        self.prefix = prefix
        self.has_device = has_device
        g = self._get
        P, D, I = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
        if has_device:
            g("problem_create", C.c_int32, [C.POINTER(P), C.c_int32])
        else:
            g("problem_create", C.c_int32, [C.POINTER(P)])
        g("problem_destroy", None, [P])
        g("last_error", C.c_char_p, [P])
        g("default_solver_options", None, [C.POINTER(SolverOptions)])
        g("problem_add_param_block", C.c_int32, [P, D, C.c_int32, C.c_int32, C.c_int32, I])
        if has_device:
            g("problem_add_param_blocks", C.c_int32, [P, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), D, I])
        g("get_param_block", C.c_int32, [P, C.c_int32, D])
        g("set_param_block", C.c_int32, [P, C.c_int32, D])
        g("set_param_blocks", C.c_int32, [P, C.c_int32, I, D])
        g("get_param_blocks", C.c_int32, [P, C.c_int32, I, D])
        g("problem_set_spline", C.c_int32, [P, C.c_int32, C.c_int32, D, D, I])
        g("problem_add_rigid_body", C.c_int32, [P, C.c_int32, C.c_int32, I])
        g("problem_add_sensor", C.c_int32,
          [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
           C.c_double, C.c_int32, C.c_double, I])
        g("problem_add_camera_residuals", C.c_int32, [P, C.c_int32, C.c_int64, D, D, I, I])
        g("problem_add_imu_residuals", C.c_int32, [P, C.c_int32, C.c_int64, D, D])
        g("solve", C.c_int32, [P, C.POINTER(SolverOptions), C.POINTER(Summary)])
        g("get_iterations", C.c_int32, [P, C.POINTER(Iteration), C.c_int32, I])
        g("get_residuals", C.c_int32, [P, C.c_int32, D, C.POINTER(C.c_uint8)])
        g("get_inlier_mask", C.c_int32, [P, C.c_int32, C.c_double, C.POINTER(C.c_uint8)])
        g("num_effective_parameters", C.c_int32, [P, I])
        g("evaluate", C.c_int32, [P, D, D, D])
        if has_device:
            g("problem_set_allreduce", C.c_int32, [P, ALLREDUCE_FN, C.c_void_p])
            g("problem_set_shard", C.c_int32, [P, C.c_int32, C.c_int32])
            g("problem_set_stream", C.c_int32, [P, C.c_void_p])
            g("get_phase_time", C.c_int32, [P, C.c_int32, D, C.POINTER(C.c_int64)])
            g("project", C.c_int32, [P, C.c_int32, D, C.POINTER(C.c_uint8)])
            g("problem_set_outlier_mask", C.c_int32, [P, C.c_int32, C.POINTER(C.c_uint8)])
            g("mark_outliers", C.c_int32, [P, C.c_int32, C.c_double, C.POINTER(C.c_int64)])
            g("residual_heatmap", C.c_int32, [P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, D, C.POINTER(C.c_int64)])
            g("fit_spline", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, D, D, C.c_int64, D, D, D])
            g("set_phase_timing", C.c_int32, [P, C.c_int32])
            g("problem_finalize", C.c_int32, [P])
            g("comm_get_unique_id", C.c_int32, [C.POINTER(C.c_uint8)])
            g("comm_init_rccl", C.c_int32, [P, C.POINTER(C.c_uint8), C.c_int32, C.c_int32])
            g("comm_info", C.c_int32, [P, I, I, C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
            g("plan_cache_stats", C.c_int32, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)])
            g("plan_cache_clear", C.c_int32, [])
            g("default_covariance_options", None, [C.POINTER(CovarianceOptions)])
            g("covariance_compute", C.c_int32, [P, C.POINTER(CovarianceOptions)])
            g("covariance_info", C.c_int32, [P, I, I, D])
            g("covariance_get_dense", C.c_int32, [P, D])
            g("covariance_get_block", C.c_int32, [P, C.c_int32, C.c_int32, C.c_int32, D])
            g("covariance_trajectory", C.c_int32, [P, C.c_int64, D, D])
            g("covariance_trajectory_info", C.c_int32, [P, I, I, D])
            g("default_prediction_options", None, [C.POINTER(PredictionOptions)])
            g("prediction_covariance", C.c_int32, [P, C.c_int32, C.POINTER(PredictionOptions), D, D, C.POINTER(C.c_uint8)])
            g("default_observability_options", None, [C.POINTER(ObservabilityOptions)])
            g("observability_compute", C.c_int32, [P, C.POINTER(ObservabilityOptions)])
            g("observability_info", C.c_int32, [P, I, I, I, D, D, I])
            g("observability_get_spectrum", C.c_int32, [P, D])
            g("observability_get_directions", C.c_int32, [P, C.c_int32, C.c_int32, C.c_int32, D])
            g("observability_get_block", C.c_int32, [P, C.c_int32, C.c_int32, C.c_int32, D, D])
            g("observability_get_matrix", C.c_int32, [P, D])
            U8 = C.POINTER(C.c_uint8)
            if hasattr(self.lib, self.prefix + "camera_unproject"):      # (as the debug hooks below: not in a library of an older round)
                g("camera_unproject", C.c_int32, [C.c_int32, C.c_int32, D, C.c_int32, C.c_int64, D, D, U8])
                g("camera_project_points", C.c_int32, [C.c_int32, C.c_int32, D, C.c_int32, C.c_int64, D, D, U8, D, D])
                g("sensor_unproject", C.c_int32, [P, C.c_int32, C.c_int64, D, D, U8])
                g("projection_uncertainty", C.c_int32, [P, C.c_int32, C.c_int32, C.c_double, C.c_int64, D, D, U8])
                g("debug_camera_unproject_chunked", C.c_int32, [C.c_int32, C.c_int32, D, C.c_int32, C.c_int64, D, D, U8, C.c_int64])
            if hasattr(self.lib, self.prefix + "camera_resect"):
                I64, RO = C.POINTER(C.c_int64), C.POINTER(ResectionOptions)
                resect = [C.c_int32, C.c_int32, D, C.c_int32, C.c_int64, I64, D, D, D, D, RO, D, D, D, I, I, U8, D]
                g("default_resection_options", None, [RO])
                g("camera_resect", C.c_int32, resect)
                g("debug_camera_resect_chunked", C.c_int32, resect + [C.c_int64])
            if hasattr(self.lib, self.prefix + "camera_calibrate"):
                I64, CO = C.POINTER(C.c_int64), C.POINTER(CalibrationOptions)
                g("default_calibration_options", None, [CO])
                g("camera_calibrate", C.c_int32, [C.c_int32, C.c_int32, D, C.c_int32, U8, C.c_int64, I64, D, D, D, D, CO, D, D, D, D, I, U8, D,
                                                  C.POINTER(CalibrationSummary)])
            if hasattr(self.lib, self.prefix + "imu_align"):
                AO = C.POINTER(ImuAlignmentOptions)
                g("default_imu_alignment_options", None, [AO])
                g("imu_align", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, D, D, D, C.c_int64, D, D, C.c_int64, D, D, D, D, D, AO,
                                           D, D, D, D, D, D, D, C.POINTER(ImuAlignmentSummary)])
            if hasattr(self.lib, self.prefix + "accel_align"):
                XO = C.POINTER(AccelAlignmentOptions)
                g("default_accel_alignment_options", None, [XO])
                g("accel_align", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, D, D, D, C.c_int64, D, D, D, D, D, D, D, XO,
                                             D, D, D, D, D, D, C.POINTER(AccelAlignmentSummary)])
            if hasattr(self.lib, self.prefix + "camera_align"):
                I64, CAO = C.POINTER(C.c_int64), C.POINTER(CameraAlignmentOptions)
                g("default_camera_alignment_options", None, [CAO])
                g("camera_align", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, D, D, D, C.c_int32, D, C.c_int32, D, D, C.c_int64, D, I64, D, D,
                                              D, D, D, CAO, D, D, D, D, I, U8, D, D, C.POINTER(CameraAlignmentSummary)])
            if hasattr(self.lib, self.prefix + "rig_calibrate"):
                I64, RGO = C.POINTER(C.c_int64), C.POINTER(RigOptions)
                g("default_rig_options", None, [RGO])
                g("rig_calibrate", C.c_int32, [C.c_int32, C.c_int32, I, I64, D, C.c_int64, C.c_int64, I, I64, I64, D, D, D, D, D, D, RGO,
                                               D, D, U8, D, D, U8, D, I, U8, D, C.POINTER(RigSummary)])
            if hasattr(self.lib, self.prefix + "fit_spline_smooth"):
                FO = C.POINTER(SplineFitOptions)
                g("default_spline_fit_options", None, [FO])
                g("fit_spline_smooth", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, D, D, C.c_int64, D, D, D, FO, D, D, C.POINTER(SplineFitRow),
                                                   C.POINTER(SplineFitSummary)])
            if hasattr(self.lib, self.prefix + "fit_spline_robust"):
                FO, RO = C.POINTER(SplineFitOptions), C.POINTER(SplineRobustOptions)
                g("default_spline_robust_options", None, [RO])
                g("fit_spline_robust", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, D, D, C.c_int64, D, D, D, FO, RO, D, D, D,
                                                   C.POINTER(SplineRobustSummary)])
            if hasattr(self.lib, self.prefix + "fit_spline_cv"):
                FO, CO = C.POINTER(SplineFitOptions), C.POINTER(SplineCvOptions)
                g("default_spline_cv_options", None, [CO])
                g("fit_spline_cv", C.c_int32, [C.c_int32, C.c_int32, C.c_int32, D, D, C.c_int64, D, D, D, FO, CO, D, D, C.POINTER(SplineFitRow),
                                               C.POINTER(SplineCvRow), D, D, C.POINTER(SplineCvSummary)])
            if hasattr(self.lib, self.prefix + "imu_allan"):
                I64, NO = C.POINTER(C.c_int64), C.POINTER(AllanOptions)
                g("default_allan_options", None, [NO])
                g("imu_allan", C.c_int32, [C.c_int32, C.c_int64, D, C.c_double, D, NO, I, I64, D, D, D, C.POINTER(AllanNoise),
                                           C.POINTER(AllanSummary)])
            g("debug_observability_info", C.c_int32, [P, D, C.c_int32])
            g("debug_lm_control_replay", C.c_int32,
              [C.c_int32, C.c_int32, D, I, C.POINTER(SolverOptions), D, I, D])
            g("debug_plan_info", C.c_int32, [P, I, C.c_int32])
            if hasattr(self.lib, self.prefix + "debug_roll_table"):      # (a library of an older round, loaded for a same-box A/B, has none)
                g("debug_roll_table", C.c_int32, [C.c_int32, C.c_int32, C.POINTER(C.c_uint32)])
            if hasattr(self.lib, self.prefix + "debug_last_step"):
                g("debug_last_step", C.c_int32, [P, C.c_int32, D, D, D])
            if hasattr(self.lib, self.prefix + "debug_lds_attribute_calls"):
                g("debug_lds_attribute_calls", C.c_int64, [])
            if hasattr(self.lib, self.prefix + "debug_panel_product"):
                g("debug_panel_product", C.c_int32, [C.c_int32, C.c_int32, D, D, D])
                g("debug_block_elim", C.c_int32, [C.c_int32, C.c_int32, D, D, D, D, D])

    def _get(self, name, restype, argtypes):
        fn = getattr(self.lib, self.prefix + name)
        fn.restype = restype
        fn.argtypes = argtypes
        setattr(self, name, fn)

    def default_options(self):
        o = SolverOptions()
        self.default_solver_options(C.byref(o))
        return o


def plan_cache_stats(api):
    """(hits, misses, plans held) of the library's plan cache."""
    h, m, e = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    api.plan_cache_stats(C.byref(h), C.byref(m), C.byref(e))
    return h.value, m.value, e.value


def comm_unique_id(api):
    """128-byte RCCL id drawn by rank 0, to be handed to every rank's Problem.comm_init_rccl."""
    buf = (C.c_uint8 * 128)()
    st = api.comm_get_unique_id(buf)
    if st != OK:
        raise CalicoError(st, "calico_comm_get_unique_id failed")
    return bytes(buf)


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _check_free(api, st):
    """Status of a call without a handle: its message is the calling thread's (calico_last_error(NULL))."""
    if st != OK:
        raise CalicoError(st, api.last_error(None).decode())


def camera_unproject(api, model, intrinsics, pixels, device=0, chunk=None):
    """calico_camera_unproject: pixels (n, 2) -> (unit-norm points (n, 3), valid (n,) bool) under the model's projection at
    `intrinsics`, on the device. Invalid pixels come back as zeros. chunk: test hook (pixels per host-side pass)."""
    k, px = _f64(intrinsics).ravel(), _f64(pixels).reshape(-1, 2)
    n = len(px)
    out, valid = np.zeros((n, 3)), np.zeros(max(n, 1), dtype=np.uint8)
    if chunk is None:
        st = api.camera_unproject(int(device), int(model), _dp(k), k.size, n, _dp(px), _dp(out), _u8p(valid))
    else:
        st = api.debug_camera_unproject_chunked(int(device), int(model), _dp(k), k.size, n, _dp(px), _dp(out), _u8p(valid), int(chunk))
    _check_free(api, st)
    return out, valid[:n].astype(bool)


def camera_project_points(api, model, intrinsics, points, jacobians=False, device=0):
    """calico_camera_project_points: camera-frame points (n, 3) -> (pixels (n, 2), valid (n,) bool), and with jacobians=True
    also d pixel / d point (n, 2, 3) and d pixel / d intrinsics (n, 2, K)."""
    k, pt = _f64(intrinsics).ravel(), _f64(points).reshape(-1, 3)
    n = len(pt)
    px, valid = np.zeros((n, 2)), np.zeros(max(n, 1), dtype=np.uint8)
    dp = np.zeros((n, 2, 3)) if jacobians else None
    dk = np.zeros((n, 2, k.size)) if jacobians else None
    _check_free(api, api.camera_project_points(int(device), int(model), _dp(k), k.size, n, _dp(pt), _dp(px), _u8p(valid),
                                               _dp(dp) if jacobians else None, _dp(dk) if jacobians else None))
    if jacobians:
        return px, valid[:n].astype(bool), dp, dk
    return px, valid[:n].astype(bool)


class Resection:
    """What calico_camera_resect returns: per frame q (x, y, z, w) and t of T_camera_chart, rms (pixels), n_used, iterations,
    status (RESECT_*), and cov (n_frames, 6, 6) or None."""

    def __init__(self, q, t, rms, n_used, iterations, status, cov):
        self.q, self.t, self.rms, self.n_used, self.iterations, self.status, self.cov = q, t, rms, n_used, iterations, status, cov


def _options(struct_cls, default_fn, what, kw):
    """The library's defaults of an options struct with the given fields replaced."""
    o = struct_cls()
    default_fn(C.byref(o))
    for name, v in kw.items():
        if not hasattr(o, name):
            raise TypeError("no %s option %r" % (what, name))
        setattr(o, name, v)
    return o


def resection_options(api, **kw):
    """The library's default calico_resection_options with the given fields replaced."""
    return _options(ResectionOptions, api.default_resection_options, "resection", kw)


class _ChartBatch:
    """The frames of calico_camera_resect / calico_camera_calibrate as contiguous arrays, which it holds for the length of the
    call: nf, and `args`, their pointers in the order the calls take them (q_init and t_init may be None)."""

    def __init__(self, frame_offsets, pixels, points, q_init, t_init):
        off = np.ascontiguousarray(frame_offsets, dtype=np.int64).ravel()
        self.nf = nf = len(off) - 1
        px, pt = _f64(pixels).reshape(-1, 2), _f64(points).reshape(-1, 3)
        if nf < 0 or len(px) != len(pt) or off[-1] != len(px):
            raise ValueError("frame_offsets must have n_frames + 1 entries and end at the number of pairs")
        qi = None if q_init is None else _f64(q_init).reshape(nf, 4)
        ti = None if t_init is None else _f64(t_init).reshape(nf, 3)
        self.arrays = (off, px, pt, qi, ti)
        self.args = [nf, off.ctypes.data_as(C.POINTER(C.c_int64)), _dp(px), _dp(pt), None if qi is None else _dp(qi), None if ti is None else _dp(ti)]


def camera_resect(api, model, intrinsics, frame_offsets, pixels, points, q_init=None, t_init=None, options=None, covariance=False,
                  device=0, chunk=None):
    """calico_camera_resect: the pose T_camera_chart of every frame. frame_offsets (n_frames + 1) cuts pixels (N, 2) and chart
    points (N, 3) into frames; q_init (n_frames, 4) and t_init (n_frames, 3) together, or neither (homography start: planar
    charts). options: a ResectionOptions (resection_options(api, ...)) or None. chunk: test hook (pairs per host-side pass)."""
    k = _f64(intrinsics).ravel()
    batch = _ChartBatch(frame_offsets, pixels, points, q_init, t_init)
    nf = batch.nf
    m = max(nf, 1)
    q, t, rms = np.zeros((m, 4)), np.zeros((m, 3)), np.zeros(m)
    used, its, status = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(m, np.uint8)
    cov = np.zeros((m, 6, 6)) if covariance else None
    args = [int(device), int(model), _dp(k), k.size] + batch.args + [None if options is None else C.byref(options), _dp(q), _dp(t), _dp(rms),
                                                                 _ip(used), _ip(its), _u8p(status), _dp(cov) if covariance else None]
    if chunk is None:
        st = api.camera_resect(*args)
    else:
        st = api.debug_camera_resect_chunked(*(args + [int(chunk)]))
    _check_free(api, st)
    return Resection(q[:nf], t[:nf], rms[:nf], used[:nf], its[:nf], status[:nf], cov[:nf] if covariance else None)


class Calibration:
    """What calico_camera_calibrate returns: intrinsics (K), per frame q (x, y, z, w) and t of T_camera_chart, rms (pixels),
    n_used and status (RESECT_*), cov (K, K) or None, and the summary's fields: status (CALIB_*), iterations, initial_cost,
    final_cost, total_rms, frames_used, pairs_used, lambda_."""

    def __init__(self, intrinsics, q, t, rms, n_used, frame_status, cov, summary):
        self.intrinsics, self.q, self.t, self.rms, self.n_used, self.frame_status, self.cov = intrinsics, q, t, rms, n_used, frame_status, cov
        self.status, self.iterations = summary.status, summary.iterations
        self.initial_cost, self.final_cost, self.total_rms = summary.initial_cost, summary.final_cost, summary.rms
        self.frames_used, self.pairs_used, self.lambda_ = summary.frames_used, summary.pairs_used, summary.lambda_


def calibration_options(api, **kw):
    """The library's default calico_calibration_options with the given fields replaced."""
    return _options(CalibrationOptions, api.default_calibration_options, "calibration", kw)


def camera_calibrate(api, model, intrinsics_init, frame_offsets, pixels, points, q_init=None, t_init=None, free_mask=None, options=None,
                     covariance=False, device=0):
    """calico_camera_calibrate: the intrinsics of `model` jointly with the pose T_camera_chart of every frame. frame_offsets
    (n_frames + 1) cuts pixels (N, 2) and chart points (N, 3) into frames; q_init (n_frames, 4) and t_init (n_frames, 3) together,
    or neither (every frame is resected at intrinsics_init). free_mask: K flags, 0 = the entry is a constant; None = all free.
    options: a CalibrationOptions (calibration_options(api, ...)) or None. Returns a Calibration."""
    k = _f64(intrinsics_init).ravel()
    batch = _ChartBatch(frame_offsets, pixels, points, q_init, t_init)
    nf = batch.nf
    mask = None if free_mask is None else np.ascontiguousarray(np.asarray(free_mask) != 0, dtype=np.uint8).ravel()
    if mask is not None and mask.size != k.size:
        raise ValueError("free_mask must have one entry per intrinsic")
    m = max(nf, 1)
    k_out = k.copy()
    q, t, rms = np.zeros((m, 4)), np.zeros((m, 3)), np.zeros(m)
    q[:, 3] = 1.0
    used, status = np.zeros(m, np.int32), np.zeros(m, np.uint8)
    cov = np.zeros((k.size, k.size)) if covariance else None
    summary = CalibrationSummary()
    st = api.camera_calibrate(*([int(device), int(model), _dp(k), k.size, None if mask is None else _u8p(mask)] + batch.args +
                                [None if options is None else C.byref(options), _dp(k_out), _dp(q), _dp(t), _dp(rms), _ip(used), _u8p(status),
                                 _dp(cov) if covariance else None, C.byref(summary)]))
    _check_free(api, st)
    return Calibration(k_out, q[:nf], t[:nf], rms[:nf], used[:nf], status[:nf], cov, summary)


class RigCalibration:
    """What calico_rig_calibrate returns: per camera q_rig_camera (C, 4; x, y, z, w), t_rig_camera (C, 3) and camera_status
    (RIG_CAMERA_*); per rig frame q_frame, t_frame (T_rig_chart) and frame_status (RIG_FRAME_*); per view, in the caller's order,
    view_rms (pixels), view_n_used and view_status (RESECT_*); cov (6 C, 6 C) or None; and the summary's fields: status (RIG_*),
    iterations, initial_cost, final_cost, total_rms, cameras_used, frames_used, views_used, pairs_used, lambda_."""

    def __init__(self, q_cam, t_cam, camera_status, q_frame, t_frame, frame_status, view_rms, view_n_used, view_status, cov, summary):
        self.q_rig_camera, self.t_rig_camera, self.camera_status = q_cam, t_cam, camera_status
        self.q_frame, self.t_frame, self.frame_status = q_frame, t_frame, frame_status
        self.view_rms, self.view_n_used, self.view_status, self.cov = view_rms, view_n_used, view_status, cov
        self.status, self.iterations = summary.status, summary.iterations
        self.initial_cost, self.final_cost, self.total_rms = summary.initial_cost, summary.final_cost, summary.rms
        self.cameras_used, self.frames_used, self.views_used = summary.cameras_used, summary.frames_used, summary.views_used
        self.pairs_used, self.lambda_ = summary.pairs_used, summary.lambda_


def rig_options(api, **kw):
    """The library's default calico_rig_options with the given fields replaced."""
    return _options(RigOptions, api.default_rig_options, "rig", kw)


def rig_calibrate(api, models, intrinsics, n_frames, view_camera, view_frame, view_offsets, pixels, points, q_rig_camera_init=None,
                  t_rig_camera_init=None, q_frame_init=None, t_frame_init=None, options=None, covariance=False, device=0):
    """calico_rig_calibrate: the extrinsics T_rig_camera of the cameras of a rig and the pose T_rig_chart of every rig frame.
    models: one camera model per camera; intrinsics: one array per camera. View v is camera view_camera[v] in rig frame
    view_frame[v] and owns the pairs [view_offsets[v], view_offsets[v + 1]) of pixels (N, 2) and chart points (N, 3). The
    starts come in pairs (q, t), the frames' only with the cameras'. options: a RigOptions (rig_options(api, ...)) or None.
    Returns a RigCalibration."""
    md = _i32(models).ravel()
    nc = len(md)
    ks = [_f64(k).ravel() for k in intrinsics]
    if len(ks) != nc:
        raise ValueError("one intrinsics array per camera")
    koff = np.zeros(nc + 1, dtype=np.int64)
    koff[1:] = np.cumsum([k.size for k in ks])
    kk = _f64(np.concatenate(ks)) if nc else np.zeros(1)
    vc = _i32(view_camera).ravel()
    vf = np.ascontiguousarray(view_frame, dtype=np.int64).ravel()
    off = np.ascontiguousarray(view_offsets, dtype=np.int64).ravel()
    nv, nf = len(vc), int(n_frames)
    px, pt = _f64(pixels).reshape(-1, 2), _f64(points).reshape(-1, 3)
    if len(vf) != nv or len(off) != nv + 1 or len(px) != len(pt) or off[-1] != len(px):
        raise ValueError("view_camera and view_frame have one entry per view, view_offsets one more, ending at the number of pairs")

    def start(a, rows, cols):
        return None if a is None else _f64(a).reshape(rows, cols)
    qc, tc, qf, tf = start(q_rig_camera_init, nc, 4), start(t_rig_camera_init, nc, 3), start(q_frame_init, nf, 4), start(t_frame_init, nf, 3)
    mc, mf, mv = max(nc, 1), max(nf, 1), max(nv, 1)
    q_cam, t_cam, cam_status = np.zeros((mc, 4)), np.zeros((mc, 3)), np.zeros(mc, np.uint8)
    q_fr, t_fr, fr_status = np.zeros((mf, 4)), np.zeros((mf, 3)), np.zeros(mf, np.uint8)
    v_rms, v_used, v_status = np.zeros(mv), np.zeros(mv, np.int32), np.zeros(mv, np.uint8)
    cov = np.zeros((6 * nc, 6 * nc)) if covariance else None
    summary = RigSummary()
    I64 = C.POINTER(C.c_int64)
    opt = lambda a: None if a is None else _dp(a)      # noqa: E731
    st = api.rig_calibrate(int(device), nc, _ip(md), koff.ctypes.data_as(I64), _dp(kk), nf, nv, _ip(vc), vf.ctypes.data_as(I64),
                           off.ctypes.data_as(I64), _dp(px), _dp(pt), opt(qc), opt(tc), opt(qf), opt(tf),
                           None if options is None else C.byref(options), _dp(q_cam), _dp(t_cam), _u8p(cam_status), _dp(q_fr), _dp(t_fr),
                           _u8p(fr_status), _dp(v_rms), _ip(v_used), _u8p(v_status), _dp(cov) if covariance else None, C.byref(summary))
    _check_free(api, st)
    return RigCalibration(q_cam[:nc], t_cam[:nc], cam_status[:nc], q_fr[:nf], t_fr[:nf], fr_status[:nf], v_rms[:nv], v_used[:nv],
                          v_status[:nv], cov, summary)


def imu_alignment_options(api, **kw):
    """The library's default calico_imu_alignment_options with the given fields replaced."""
    return _options(ImuAlignmentOptions, api.default_imu_alignment_options, "IMU alignment", kw)


def imu_align(api, order, knots, basis, ctrl, gyro_stamps, gyro, accel_stamps=None, accel=None, t_rig_accel=None, q_init=None,
              latency_init=None, options=None, covariance=False, curve=False, device=0):
    """calico_imu_align: the rotation rig <- gyroscope, the gyroscope's bias, the IMU's latency and, with accelerometer samples,
    the world's gravity and the accelerometer's bias, against the spline (order, knots, basis, ctrl (n_knots - order, 6)).
    gyro (n, 3) at gyro_stamps (n, sorted); accel (m, 3) at accel_stamps or neither; q_init (x, y, z, w) and latency_init
    together or neither. options: an ImuAlignmentOptions (imu_alignment_options(api, ...)) or None. Returns a dict: q_rig_gyro,
    gyro_bias, latency, gravity_world and accel_bias (None unless the accelerometer part is ALIGN_OK), cov (7, 7) or None,
    curve (n_lags,) or None, and every field of the summary."""
    knots, basis, ctrl = _f64(knots).ravel(), _f64(basis), _f64(ctrl).reshape(-1, 6)
    order = int(order)
    if len(ctrl) != len(knots) - order or basis.size != (len(knots) - 2 * order + 1) * order * order:
        raise ValueError("ctrl must be (n_knots - order, 6) and basis (n_knots - 2 order + 1, order, order)")
    gs, g = _f64(gyro_stamps).ravel(), _f64(gyro).reshape(-1, 3)
    if len(gs) != len(g):
        raise ValueError("one gyroscope stamp per sample")
    if (accel_stamps is None) != (accel is None):
        raise ValueError("accel_stamps and accel are given together or not at all")
    as_ = np.zeros(0) if accel is None else _f64(accel_stamps).ravel()
    am = np.zeros((0, 3)) if accel is None else _f64(accel).reshape(-1, 3)
    if len(as_) != len(am):
        raise ValueError("one accelerometer stamp per sample")
    tra = None if t_rig_accel is None else _f64(t_rig_accel).reshape(3)
    qi = None if q_init is None else _f64(q_init).reshape(4)
    li = None if latency_init is None else _f64([latency_init]).reshape(1)
    q, bias, lat = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3), np.zeros(1)
    grav, abias = np.full(3, np.nan), np.full(3, np.nan)
    cov = np.zeros((7, 7)) if covariance else None
    cur = np.full(ALIGN_MAX_LAGS, np.nan) if curve else None
    summary = ImuAlignmentSummary()
    st = api.imu_align(int(device), order, len(knots), _dp(knots), _dp(basis), _dp(ctrl), len(g), _dp(gs) if len(g) else None,
                       _dp(g) if len(g) else None, len(am), _dp(as_) if len(am) else None, _dp(am) if len(am) else None,
                       None if tra is None else _dp(tra), None if qi is None else _dp(qi), None if li is None else _dp(li),
                       None if options is None else C.byref(options), _dp(q), _dp(bias), _dp(lat), _dp(grav), _dp(abias),
                       _dp(cov) if covariance else None, _dp(cur) if curve else None, C.byref(summary))
    _check_free(api, st)
    out = {name: getattr(summary, name) for name, _ in ImuAlignmentSummary._fields_}
    solved = len(am) > 0 and summary.accel_status == ALIGN_OK
    out.update(q_rig_gyro=q, gyro_bias=bias, latency=float(lat[0]), gravity_world=grav if solved else None,
               accel_bias=abias if solved else None, cov=cov, curve=cur[:summary.n_lags] if curve else None)
    if curve:
        out["curve_tail"] = cur[summary.n_lags:]      # (never written by the library)
    return out


def accel_alignment_options(api, **kw):
    """The library's default calico_accel_alignment_options with the given fields replaced."""
    return _options(AccelAlignmentOptions, api.default_accel_alignment_options, "accelerometer alignment", kw)


def accel_align(api, order, knots, basis, ctrl, stamps, accel, q_init, latency_init, t_init=None, bias_init=None, gravity_init=None,
                options=None, covariance=False, device=0):
    """calico_accel_align: the rotation rig <- accelerometer, its lever arm, its bias, the world's gravity and its latency against
    the spline (order, knots, basis, ctrl (n_knots - order, 6)). accel (n, 3) at stamps (n, sorted); q_init (x, y, z, w) and
    latency_init are required (calico_imu_align's for the gyroscope); t_init, bias_init and gravity_init all three or none.
    options: an AccelAlignmentOptions (accel_alignment_options(api, ...)) or None. Returns a dict: q_rig_accel, t_rig_accel, bias,
    gravity_world, latency, cov (13, 13) or None, and every field of the summary."""
    knots, basis, ctrl = _f64(knots).ravel(), _f64(basis), _f64(ctrl).reshape(-1, 6)
    order = int(order)
    if len(ctrl) != len(knots) - order or basis.size != (len(knots) - 2 * order + 1) * order * order:
        raise ValueError("ctrl must be (n_knots - order, 6) and basis (n_knots - 2 order + 1, order, order)")
    s, m = _f64(stamps).ravel(), _f64(accel).reshape(-1, 3)
    if len(s) != len(m):
        raise ValueError("one stamp per sample")

    def vec(a, n):
        return None if a is None else _f64(a).reshape(n)
    qi, ti, bi, gi = vec(q_init, 4), vec(t_init, 3), vec(bias_init, 3), vec(gravity_init, 3)
    li = None if latency_init is None else _f64([latency_init]).reshape(1)
    ptr = lambda a: None if a is None else _dp(a)      # noqa: E731
    q, t, bias, grav, lat = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(1)
    cov = np.zeros((13, 13)) if covariance else None
    summary = AccelAlignmentSummary()
    st = api.accel_align(int(device), order, len(knots), _dp(knots), _dp(basis), _dp(ctrl), len(m), _dp(s) if len(m) else None,
                         _dp(m) if len(m) else None, ptr(qi), ptr(li), ptr(ti), ptr(bi), ptr(gi),
                         None if options is None else C.byref(options), _dp(q), _dp(t), _dp(bias), _dp(grav), _dp(lat), ptr(cov),
                         C.byref(summary))
    _check_free(api, st)
    out = {name: getattr(summary, name) for name, _ in AccelAlignmentSummary._fields_}
    out.update(q_rig_accel=q, t_rig_accel=t, bias=bias, gravity_world=grav, latency=float(lat[0]), cov=cov)
    return out


def camera_alignment_options(api, **kw):
    """The library's default calico_camera_alignment_options with the given fields replaced."""
    return _options(CameraAlignmentOptions, api.default_camera_alignment_options, "camera alignment", kw)


def camera_align(api, order, knots, basis, ctrl, model, intrinsics, frame_stamps, frame_offsets, pixels, points, q_world_chart=None,
                 t_world_chart=None, q_init=None, t_init=None, latency_init=None, options=None, covariance=False, curve=False, device=0):
    """calico_camera_align: the extrinsics T_rig_camera and the latency of a camera against the spline (order, knots, basis, ctrl
    (n_knots - order, 6)) from its chart detections at known intrinsics. frame_offsets (n_frames + 1) cuts pixels (N, 2) and chart
    points (N, 3) into frames stamped frame_stamps (n_frames, sorted); (q_world_chart, t_world_chart): the chart's pose, None =
    identity; q_init (x, y, z, w), t_init and latency_init together or none. options: a CameraAlignmentOptions
    (camera_alignment_options(api, ...)) or None. Returns a dict: q_rig_camera, t_rig_camera, latency, frame_rms, frame_n_used,
    frame_status, cov (7, 7) or None, curve (n_lags,) or None, and every field of the summary."""
    knots, basis, ctrl = _f64(knots).ravel(), _f64(basis), _f64(ctrl).reshape(-1, 6)
    order = int(order)
    if len(ctrl) != len(knots) - order or basis.size != (len(knots) - 2 * order + 1) * order * order:
        raise ValueError("ctrl must be (n_knots - order, 6) and basis (n_knots - 2 order + 1, order, order)")
    k = _f64(intrinsics).ravel()
    batch = _ChartBatch(frame_offsets, pixels, points, None, None)
    nf = batch.nf
    fs = _f64(frame_stamps).ravel()
    if len(fs) != nf:
        raise ValueError("one stamp per frame")

    def opt(a, n):
        return None if a is None else _f64(a).reshape(n)
    qw, tw, qi, ti = opt(q_world_chart, 4), opt(t_world_chart, 3), opt(q_init, 4), opt(t_init, 3)
    li = None if latency_init is None else _f64([latency_init]).reshape(1)
    ptr = lambda a: None if a is None else _dp(a)      # noqa: E731
    m = max(nf, 1)
    q, t, lat = np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3), np.zeros(1)
    rms, used, status = np.zeros(m), np.zeros(m, np.int32), np.zeros(m, np.uint8)
    cov = np.zeros((7, 7)) if covariance else None
    cur = np.full(ALIGN_MAX_LAGS, np.nan) if curve else None
    summary = CameraAlignmentSummary()
    off = batch.arrays[0]
    st = api.camera_align(int(device), order, len(knots), _dp(knots), _dp(basis), _dp(ctrl), int(model), _dp(k), k.size, ptr(qw), ptr(tw), nf,
                          _dp(fs) if nf else None, off.ctypes.data_as(C.POINTER(C.c_int64)), batch.args[2], batch.args[3], ptr(qi), ptr(ti),
                          ptr(li), None if options is None else C.byref(options), _dp(q), _dp(t), _dp(lat), _dp(rms), _ip(used),
                          _u8p(status), ptr(cov), ptr(cur), C.byref(summary))
    _check_free(api, st)
    out = {name: getattr(summary, name) for name, _ in CameraAlignmentSummary._fields_}
    out.update(q_rig_camera=q, t_rig_camera=t, latency=float(lat[0]), frame_rms=rms[:nf], frame_n_used=used[:nf], frame_status=status[:nf],
               cov=cov, curve=cur[:summary.n_lags] if curve else None)
    if curve:
        out["curve_tail"] = cur[summary.n_lags:]      # (never written by the library)
    return out


def default_spline_fit_options(api, lambda_rot=None, lambda_pos=None, **kw):
    """The library's default calico_spline_fit_options with the given fields replaced. lambda_rot / lambda_pos: a number or a
    sequence (the grid); n_lambda follows their length unless given."""
    o = _options(SplineFitOptions, api.default_spline_fit_options, "spline fit", kw)
    for name, grid in (("lambda_rot", lambda_rot), ("lambda_pos", lambda_pos)):
        if grid is None:
            continue
        grid = np.atleast_1d(np.asarray(grid, dtype=np.float64))
        if not 1 <= len(grid) <= FIT_MAX_LAMBDAS:
            raise ValueError("%s must have 1 to %d entries" % (name, FIT_MAX_LAMBDAS))
        field = getattr(o, name)
        for i in range(FIT_MAX_LAMBDAS):
            field[i] = grid[i] if i < len(grid) else 0.0
        if "n_lambda" not in kw:
            o.n_lambda = len(grid)
    return o


def fit_spline_smooth(api, order, knots, basis, stamps, data6, weights=None, options=None, device=0):
    """calico_fit_spline_smooth: the penalised spline fit through sorted samples data6 (n, 6) at stamps, per channel group (rotation:
    channels 0..2, position: 3..5) and for every lambda of the options' grid. weights: (n, 2) [rotation, position] or None (all 1).
    options: a SplineFitOptions (default_spline_fit_options(api, ...)) or None. Returns a dict: ctrl (n_ctrl, 6; each group's chosen
    lambda), ctrl_all (n_lambda, n_ctrl, 6), rows ([group][lambda] dicts: status, replaced_pivots, lambda, rss, penalty, rms) and
    summary (status, chosen, n_used: one entry per group)."""
    knots, basis, order = _f64(knots).ravel(), _f64(basis), int(order)
    t, d = _f64(stamps).ravel(), _f64(data6).reshape(-1, 6)
    if len(t) != len(d):
        raise ValueError("one stamp per sample")
    if basis.size != max(len(knots) - 2 * order + 1, 0) * order * order:
        raise ValueError("basis must be (n_knots - 2 order + 1, order, order)")
    w = None if weights is None else _f64(weights).reshape(-1, 2)
    if w is not None and len(w) != len(t):
        raise ValueError("weights must be (n, 2)")
    nl = options.n_lambda if options is not None else 1
    n_ctrl = max(len(knots) - order, 1)
    ctrl = np.full((n_ctrl, 6), np.nan)
    ctrl_all = np.full((max(min(nl, FIT_MAX_LAMBDAS), 1), n_ctrl, 6), np.nan)
    rows = (SplineFitRow * (2 * len(ctrl_all)))()
    summary = SplineFitSummary()
    st = api.fit_spline_smooth(int(device), order, len(knots), _dp(knots), _dp(basis), len(t), _dp(t), _dp(d), None if w is None else _dp(w),
                               None if options is None else C.byref(options), _dp(ctrl), _dp(ctrl_all), rows, C.byref(summary))
    _check_free(api, st)
    names = [("status", "status"), ("replaced_pivots", "replaced_pivots"), ("lambda", "lambda_"), ("rss", "rss"), ("penalty", "penalty"), ("rms", "rms")]
    return dict(ctrl=ctrl, ctrl_all=ctrl_all, rows=[[{k: getattr(rows[g * nl + l], f) for k, f in names} for l in range(nl)] for g in range(2)],
                summary=dict(status=list(summary.status), chosen=list(summary.chosen), n_used=list(summary.n_used)))


def default_spline_robust_options(api, **kw):
    """The library's default calico_spline_robust_options with the given fields replaced."""
    return _options(SplineRobustOptions, api.default_spline_robust_options, "robust spline fit", kw)


def fit_spline_robust(api, order, knots, basis, stamps, data6, weights=None, options=None, robust=None, device=0):
    """calico_fit_spline_robust: iteratively reweighted least squares (Huber or Tukey, scale from the median residual norm) around
    the smoothing fit, per channel group. weights: (n, 2) prior weights or None. options: a SplineFitOptions with one lambda and
    no target, or None; robust: a SplineRobustOptions (default_spline_robust_options(api, ...)) or None. Returns a dict: ctrl
    (n_ctrl, 6), robust_weights (n, 2: u of the last solve, 0 where the prior weight is 0), residuals (n, 2: the residual norms at
    ctrl, NaN where the prior weight is 0) and summary (a dict of two-entry lists, one entry per group)."""
    knots, basis, order = _f64(knots).ravel(), _f64(basis), int(order)
    t, d = _f64(stamps).ravel(), _f64(data6).reshape(-1, 6)
    if len(t) != len(d):
        raise ValueError("one stamp per sample")
    if basis.size != max(len(knots) - 2 * order + 1, 0) * order * order:
        raise ValueError("basis must be (n_knots - 2 order + 1, order, order)")
    w = None if weights is None else _f64(weights).reshape(-1, 2)
    if w is not None and len(w) != len(t):
        raise ValueError("weights must be (n, 2)")
    ctrl = np.full((max(len(knots) - order, 1), 6), np.nan)
    u, e = np.full((len(t), 2), np.nan), np.full((len(t), 2), np.nan)
    summary = SplineRobustSummary()
    st = api.fit_spline_robust(int(device), order, len(knots), _dp(knots), _dp(basis), len(t), _dp(t), _dp(d), None if w is None else _dp(w),
                               None if options is None else C.byref(options), None if robust is None else C.byref(robust), _dp(ctrl), _dp(u),
                               _dp(e), C.byref(summary))
    _check_free(api, st)
    return dict(ctrl=ctrl, robust_weights=u, residuals=e,
                summary={name.rstrip("_"): list(getattr(summary, name)) for name, _ in SplineRobustSummary._fields_})


def default_spline_cv_options(api, **kw):
    """The library's default calico_spline_cv_options with the given fields replaced."""
    return _options(SplineCvOptions, api.default_spline_cv_options, "cross-validated spline fit", kw)


def fit_spline_cv(api, order, knots, basis, stamps, data6, weights=None, options=None, cv=None, device=0):
    """calico_fit_spline_cv: the smoothing fit over the options' lambda grid with each group's lambda chosen by generalised
    cross-validation or the leave-one-out score (cv: a SplineCvOptions, default_spline_cv_options(api, criterion=...), or None).
    options: a SplineFitOptions without targets, or None. Returns fit_spline_smooth's dict (ctrl at the choice) plus cv_rows
    ([group][lambda] dicts: edf, gcv, press, max_leverage), leverage (n, 2: h_j at the chosen lambda, 0 where the weight is 0),
    loo_residuals (n, 2: e_j / (1 - h_j), NaN where the weight is 0), chosen, and a summary with status, chosen, n_used, edf, score."""
    knots, basis, order = _f64(knots).ravel(), _f64(basis), int(order)
    t, d = _f64(stamps).ravel(), _f64(data6).reshape(-1, 6)
    if len(t) != len(d):
        raise ValueError("one stamp per sample")
    if basis.size != max(len(knots) - 2 * order + 1, 0) * order * order:
        raise ValueError("basis must be (n_knots - 2 order + 1, order, order)")
    w = None if weights is None else _f64(weights).reshape(-1, 2)
    if w is not None and len(w) != len(t):
        raise ValueError("weights must be (n, 2)")
    nl = options.n_lambda if options is not None else 1
    n_ctrl = max(len(knots) - order, 1)
    ctrl = np.full((n_ctrl, 6), np.nan)
    ctrl_all = np.full((max(min(nl, FIT_MAX_LAMBDAS), 1), n_ctrl, 6), np.nan)
    rows = (SplineFitRow * (2 * len(ctrl_all)))()
    cv_rows = (SplineCvRow * (2 * len(ctrl_all)))()
    h, loo = np.full((len(t), 2), np.nan), np.full((len(t), 2), np.nan)
    summary = SplineCvSummary()
    st = api.fit_spline_cv(int(device), order, len(knots), _dp(knots), _dp(basis), len(t), _dp(t), _dp(d), None if w is None else _dp(w),
                           None if options is None else C.byref(options), None if cv is None else C.byref(cv), _dp(ctrl), _dp(ctrl_all), rows,
                           cv_rows, _dp(h), _dp(loo), C.byref(summary))
    _check_free(api, st)
    names = [("status", "status"), ("replaced_pivots", "replaced_pivots"), ("lambda", "lambda_"), ("rss", "rss"), ("penalty", "penalty"), ("rms", "rms")]
    cv_names = ("edf", "gcv", "press", "max_leverage")
    return dict(ctrl=ctrl, ctrl_all=ctrl_all, rows=[[{k: getattr(rows[g * nl + l], f) for k, f in names} for l in range(nl)] for g in range(2)],
                cv_rows=[[{k: getattr(cv_rows[g * nl + l], k) for k in cv_names} for l in range(nl)] for g in range(2)],
                leverage=h, loo_residuals=loo, chosen=list(summary.chosen),
                summary={name: list(getattr(summary, name)) for name, _ in SplineCvSummary._fields_})


def default_allan_options(api, cluster_sizes=None, **kw):
    """The library's default calico_allan_options with the given fields replaced. cluster_sizes: an explicit list of cluster
    sizes instead of the logarithmic grid (the returned struct keeps the array alive)."""
    o = _options(AllanOptions, api.default_allan_options, "Allan variance", kw)
    if cluster_sizes is not None:
        m = np.ascontiguousarray(cluster_sizes, dtype=np.int64).ravel()
        o._cluster_sizes = m
        o.n_cluster_sizes = len(m)
        o.cluster_sizes = m.ctypes.data_as(C.POINTER(C.c_int64))
    return o


def imu_allan(api, samples, stamps=None, sample_rate_hz=0.0, options=None, device=0):
    """calico_imu_allan: the overlapping Allan variance of the three axes of a static IMU log (samples (n, 3); stamps (n,) or None
    with sample_rate_hz) over a grid of cluster sizes, and per axis the IEEE-952 noise coefficients. options: an AllanOptions
    (default_allan_options(api, ...)) or None. Returns a dict: cluster_sizes (c,), tau (c,), avar (c, 3), rel_err (c,), noise (three
    dicts: Q, N, B, K, R, objective, terms_used, n_points, status) and summary (n, sample_rate_hz, duration, N_pooled,
    sigma_at_rate, bias_drift_over_recording)."""
    y = _f64(samples).reshape(-1, 3)
    t = None if stamps is None else _f64(stamps).ravel()
    if t is not None and len(t) != len(y):
        raise ValueError("one stamp per sample")
    nc = C.c_int32(0)
    m = np.zeros(ALLAN_MAX_CLUSTERS, dtype=np.int64)
    tau, rel = np.full(ALLAN_MAX_CLUSTERS, np.nan), np.full(ALLAN_MAX_CLUSTERS, np.nan)
    avar = np.full((ALLAN_MAX_CLUSTERS, 3), np.nan)
    noise = (AllanNoise * 3)()
    summary = AllanSummary()
    st = api.imu_allan(int(device), len(y), None if t is None else _dp(t), float(sample_rate_hz), _dp(y) if len(y) else None,
                       None if options is None else C.byref(options), C.byref(nc), m.ctypes.data_as(C.POINTER(C.c_int64)), _dp(tau), _dp(avar),
                       _dp(rel), noise, C.byref(summary))
    _check_free(api, st)
    c = nc.value
    names = ("Q", "N", "B", "K", "R", "objective", "terms_used", "n_points", "status")
    return dict(cluster_sizes=m[:c].copy(), tau=tau[:c].copy(), avar=avar[:c].copy(), rel_err=rel[:c].copy(),
                noise=[{k: getattr(noise[a], k) for k in names} for a in range(3)],
                summary={name: getattr(summary, name) for name, _ in AllanSummary._fields_})


class Problem:
    """Thin object wrapper of a calico_problem handle."""

    def __init__(self, api, device=0):
        self.api = api
        self.h = C.c_void_p()
        if api.has_device:
            st = api.problem_create(C.byref(self.h), int(device))
        else:
            st = api.problem_create(C.byref(self.h))
        if st != OK:
            raise CalicoError(st, "calico_problem_create failed (no usable HIP device?)")
        self._keep = []
        self._sizes = {}      # block id -> ambient size, of the blocks added through this object
        self._manifolds = {}  # block id -> manifold, of the same blocks
        self._sensor_dim = {}  # sensor id -> residual dimension, of the sensors added through this object
        self._sensor_n = {}    # sensor id -> registered observations

    def close(self):
        if self.h:
            self.api.problem_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st):
        if st != OK:
            raise CalicoError(st, self.api.last_error(self.h).decode())

    def add_param_block(self, values, manifold=MANIFOLD_EUCLIDEAN, constant=False):
        v = _f64(values).ravel()
        out = C.c_int32(-1)
        self._check(self.api.problem_add_param_block(self.h, _dp(v), v.size, manifold, int(bool(constant)),
                                                     C.byref(out)))
        self._sizes[out.value] = v.size
        self._manifolds[out.value] = manifold
        return out.value

    def add_param_blocks(self, values, manifold=MANIFOLD_EUCLIDEAN, constant=False):
        """n blocks of one size (rows of `values`); one ABI call where the library has the bulk form. Returns the ids."""
        v = _f64(values)
        if len(v) == 0:
            return np.zeros(0, np.int32)
        v = v.reshape(len(v), -1)
        n, size = v.shape
        const = np.ascontiguousarray(np.broadcast_to(np.asarray(constant, bool), (n,)), dtype=np.uint8)
        if not hasattr(self.api, "problem_add_param_blocks"):
            return np.array([self.add_param_block(v[i], manifold, bool(const[i])) for i in range(n)], np.int32)
        ids = np.zeros(n, np.int32)
        self._check(self.api.problem_add_param_blocks(self.h, n, size, manifold, const.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(v), _ip(ids)))
        for i in ids:
            self._sizes[int(i)] = size
            self._manifolds[int(i)] = manifold
        return ids

    def get_param_block(self, block_id, size):
        out = np.zeros(size)
        self._check(self.api.get_param_block(self.h, block_id, _dp(out)))
        return out

    def get_param_blocks(self, block_ids, sizes):
        """Values of several blocks, concatenated (`sizes`: the blocks' sizes, or one size for all)."""
        ids = _i32(block_ids)
        per = np.broadcast_to(np.asarray(sizes, np.int64), (ids.size,))
        # the C call writes every block's real size and takes no capacity: the caller's sizes must be the blocks' own
        for i, n in zip(ids, per):
            known = self._sizes.get(int(i))
            if known is not None and known != int(n):
                raise ValueError("block %d has %d values, not %d" % (int(i), known, int(n)))
        total = int(per.sum())
        out = np.zeros(total)
        self._check(self.api.get_param_blocks(self.h, ids.size, _ip(ids), _dp(out)))
        return out

    def set_param_block(self, block_id, values):
        v = _f64(values).ravel()
        self._check(self.api.set_param_block(self.h, block_id, _dp(v)))

    def set_param_blocks(self, block_ids, values_concat):
        ids, v = _i32(block_ids), _f64(values_concat)
        self._check(self.api.set_param_blocks(self.h, ids.size, _ip(ids), _dp(v)))

    def set_spline(self, order, knots, basis, ctrl_block_ids):
        k, b, c = _f64(knots), _f64(basis), _i32(ctrl_block_ids)
        assert c.size == k.size - order
        self._check(self.api.problem_set_spline(self.h, order, k.size, _dp(k), _dp(b), _ip(c)))

    def add_rigid_body(self, q_block, t_block):
        out = C.c_int32(-1)
        self._check(self.api.problem_add_rigid_body(self.h, q_block, t_block, C.byref(out)))
        return out.value

    def add_sensor(self, kind, model, intr, q, t, lat, grav=-1, sigma=1.0, loss=0, loss_scale=1.0):
        out = C.c_int32(-1)
        self._check(self.api.problem_add_sensor(self.h, kind, model, intr, q, t, lat, grav, float(sigma), loss,
                                                float(loss_scale), C.byref(out)))
        self._sensor_dim[out.value] = 2 if kind == SENSOR_CAMERA else 3
        self._sensor_n[out.value] = 0
        return out.value

    def add_camera_residuals(self, sensor, pixels, stamps, body_ids, point_blocks):
        px, st, b, p = _f64(pixels), _f64(stamps), _i32(body_ids), _i32(point_blocks)
        self._check(self.api.problem_add_camera_residuals(self.h, sensor, st.size, _dp(px), _dp(st), _ip(b), _ip(p)))
        self._sensor_n[sensor] = self._sensor_n.get(sensor, 0) + st.size

    def add_imu_residuals(self, sensor, meas, stamps):
        m, st = _f64(meas), _f64(stamps)
        self._check(self.api.problem_add_imu_residuals(self.h, sensor, st.size, _dp(m), _dp(st)))
        self._sensor_n[sensor] = self._sensor_n.get(sensor, 0) + st.size

    def solve(self, options=None):
        o = options if options is not None else self.api.default_options()
        s = Summary()
        self._check(self.api.solve(self.h, C.byref(o), C.byref(s)))
        return s

    def iterations(self, max_rows=4096):
        buf = (Iteration * max_rows)()
        n = C.c_int32(0)
        self._check(self.api.get_iterations(self.h, buf, max_rows, C.byref(n)))
        return [buf[i] for i in range(n.value)]

    def residuals(self, sensor, n, dim, check=True):
        out = np.zeros((n, dim))
        valid = np.zeros(n, dtype=np.uint8)
        st = self.api.get_residuals(self.h, sensor, _dp(out), valid.ctypes.data_as(C.POINTER(C.c_uint8)))
        if check:
            self._check(st)
        return out, valid

    def project(self, sensor, n, dim):
        """Sensor::Project for the registered observations: model prediction per observation (device only)."""
        out = np.zeros((n, dim))
        valid = np.zeros(n, dtype=np.uint8)
        self._check(self.api.project(self.h, sensor, _dp(out), valid.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out, valid

    def set_outlier_mask(self, sensor, is_outlier=None):
        """MarkOutliersById / ClearOutliers (device only): one byte per observation, None clears."""
        if is_outlier is None:
            self._check(self.api.problem_set_outlier_mask(self.h, sensor, None))
        else:
            m = np.ascontiguousarray(is_outlier, dtype=np.uint8)
            self._check(self.api.problem_set_outlier_mask(self.h, sensor, m.ctypes.data_as(C.POINTER(C.c_uint8))))

    def mark_outliers(self, sensor, threshold):
        """One tagging pass on the device; returns the number of observations tagged by this call."""
        n = C.c_int64(0)
        self._check(self.api.mark_outliers(self.h, sensor, float(threshold), C.byref(n)))
        return n.value

    def residual_heatmap(self, sensor, image_width, image_height, num_rows=8, num_cols=12):
        """Binned RMSE and feature count of a camera's residuals (utils.py:12-50), reduced on the device."""
        rmse = np.zeros((num_rows, num_cols))
        count = np.zeros((num_rows, num_cols), dtype=np.int64)
        self._check(self.api.residual_heatmap(self.h, sensor, int(image_width), int(image_height), int(num_rows), int(num_cols),
                                              _dp(rmse), count.ctypes.data_as(C.POINTER(C.c_int64))))
        return rmse, count

    def inlier_mask(self, sensor, n, threshold):
        mask = np.zeros(n, dtype=np.uint8)
        self._check(self.api.get_inlier_mask(self.h, sensor, float(threshold),
                                             mask.ctypes.data_as(C.POINTER(C.c_uint8))))
        return mask

    def num_effective_parameters(self):
        n = C.c_int32(0)
        self._check(self.api.num_effective_parameters(self.h, C.byref(n)))
        return n.value

    def evaluate(self, want_jtj=True):
        n = self.num_effective_parameters()
        cost = C.c_double(0)
        g = np.zeros(n)
        H = np.zeros((n, n)) if want_jtj else None
        self._check(self.api.evaluate(self.h, C.byref(cost), _dp(g), _dp(H) if want_jtj else None))
        return cost.value, g, H

    def covariance_compute(self, min_relative_pivot=None, control_points=False):
        """calico_covariance_compute; returns (dim, n_unobserved, min_relative_pivot). Raises CalicoError on failure.
        control_points=True: also the trajectory's blocks (covariance_block of control points, covariance_trajectory)."""
        o = CovarianceOptions()
        self.api.default_covariance_options(C.byref(o))
        if min_relative_pivot is not None:
            o.min_relative_pivot = float(min_relative_pivot)
        o.control_points = int(bool(control_points))
        self._check(self.api.covariance_compute(self.h, C.byref(o)))
        return self.covariance_info()

    def covariance_info(self):
        dim, nu, piv = C.c_int32(0), C.c_int32(0), C.c_double(0)
        self._check(self.api.covariance_info(self.h, C.byref(dim), C.byref(nu), C.byref(piv)))
        return dim.value, nu.value, piv.value

    def covariance_dense(self):
        """Σ of the dense border (dim x dim, border tangent order) of the last successful compute."""
        dim = self.covariance_info()[0]
        out = np.zeros((dim, dim))
        self._check(self.api.covariance_get_dense(self.h, _dp(out)))
        return out

    def covariance(self, blocks, tangent=False, min_relative_pivot=None):
        """Compute Σ and return {(a, b): block} for every pair of the given block ids (a <= b in the list's order), as
        numpy arrays: ambient form (GetCovarianceBlock) or, with tangent=True, tangent form (3 rows per quaternion)."""
        self.covariance_compute(min_relative_pivot)
        res = {}
        for i, a in enumerate(blocks):
            for b in blocks[i:]:
                res[(a, b)] = self.covariance_block(a, b, tangent)
        return res

    def covariance_trajectory_info(self):
        """(n_cp, order, min_relative_pivot_band) of the last compute with control_points=True."""
        n, k, piv = C.c_int32(0), C.c_int32(0), C.c_double(0)
        self._check(self.api.covariance_trajectory_info(self.h, C.byref(n), C.byref(k), C.byref(piv)))
        return n.value, k.value, piv.value

    def covariance_trajectory(self, stamps):
        """Covariance of the spline's 6-vector at each stamp: (n, 6, 6)."""
        t = _f64(np.atleast_1d(stamps)).ravel()
        out = np.zeros((len(t), 6, 6))
        self._check(self.api.covariance_trajectory(self.h, len(t), _dp(t), _dp(out)))
        return out

    def prediction_covariance(self, sensor, apply_loss=True):
        """calico_prediction_covariance for every registered observation of `sensor`, in insertion order: P_i = J_i Σ J_iᵀ
        (n, d, d), the leverages trace(P_i) (n,) and the valid flags (n,) bool. Needs covariance_compute(control_points=True).
        apply_loss=True: diagonal blocks of the hat matrix; False: prediction covariance of the whitened model output."""
        n, d = self._sensor_n.get(sensor, 0), self._sensor_dim.get(sensor, 3)
        o = PredictionOptions()
        self.api.default_prediction_options(C.byref(o))
        o.apply_loss = int(apply_loss)
        cov, lev = np.zeros((n, d, d)), np.zeros(n)
        valid = np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self.api.prediction_covariance(self.h, int(sensor), C.byref(o), _dp(cov), _dp(lev),
                                                   valid.ctypes.data_as(C.POINTER(C.c_uint8))))
        return cov, lev, valid[:n].astype(bool)

    def sensor_unproject(self, sensor, pixels):
        """calico_sensor_unproject: camera_unproject at the camera's current intrinsics, on the handle's stream."""
        px = _f64(pixels).reshape(-1, 2)
        n = len(px)
        out, valid = np.zeros((n, 3)), np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self.api.sensor_unproject(self.h, int(sensor), n, _dp(px), _dp(out), _u8p(valid)))
        return out, valid[:n].astype(bool)

    def projection_uncertainty(self, sensor, pixels, range=1.0, frame=FRAME_RIG):
        """calico_projection_uncertainty: ([s_uu, s_uv, s_vv] (n, 3) in pixels^2, valid (n,) bool) of a point `range` metres
        along each pixel's ray, fixed in the camera frame (FRAME_CAMERA: intrinsics only) or in the sensor-rig frame
        (FRAME_RIG: intrinsics and extrinsics). Needs covariance_compute."""
        px = _f64(pixels).reshape(-1, 2)
        n = len(px)
        out, valid = np.zeros((n, 3)), np.zeros(max(n, 1), dtype=np.uint8)
        self._check(self.api.projection_uncertainty(self.h, int(sensor), int(frame), float(range), n, _dp(px), _dp(out), _u8p(valid)))
        return out, valid[:n].astype(bool)

    def covariance_block(self, block_a, block_b, tangent=False, sizes=None):
        """Block (block_a, block_b) of the last computed Σ. `sizes`: (rows, cols) of the requested form; by default taken
        from the blocks added through this object (ambient size, or 3 for a 4-vector in tangent form; 6 for a control
        point)."""
        if sizes is None:
            def sz(b):
                n = self._sizes[b]
                return 3 if (tangent and n == 4 and self._manifolds.get(b) == MANIFOLD_EIGEN_QUATERNION) else n
            sizes = (sz(block_a), sz(block_b))
        out = np.zeros(sizes)
        self._check(self.api.covariance_get_block(self.h, int(block_a), int(block_b), int(bool(tangent)), _dp(out)))
        return out

    def observability_compute(self, weak_threshold=None, min_relative_pivot=None):
        """calico_observability_compute; returns observability_info(). Raises CalicoError on failure (a trajectory the data
        do not determine); a rank-deficient border is not one: n_weak > 0."""
        o = ObservabilityOptions()
        self.api.default_observability_options(C.byref(o))
        if weak_threshold is not None:
            o.weak_threshold = float(weak_threshold)
        if min_relative_pivot is not None:
            o.min_relative_pivot = float(min_relative_pivot)
        self._check(self.api.observability_compute(self.h, C.byref(o)))
        return self.observability_info()

    def observability_info(self):
        """dict: dim, n_unobserved, n_weak, lambda_min, lambda_max, sweeps of the last successful compute."""
        dim, nu, nw, sw = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
        lo, hi = C.c_double(0), C.c_double(0)
        self._check(self.api.observability_info(self.h, C.byref(dim), C.byref(nu), C.byref(nw), C.byref(lo), C.byref(hi), C.byref(sw)))
        return dict(dim=dim.value, n_unobserved=nu.value, n_weak=nw.value, lambda_min=lo.value, lambda_max=hi.value, sweeps=sw.value)

    def observability_spectrum(self):
        """Eigenvalues of S̃, ascending (dim - n_unobserved of them)."""
        i = self.observability_info()
        out = np.zeros(i["dim"] - i["n_unobserved"])
        self._check(self.api.observability_get_spectrum(self.h, _dp(out) if out.size else _dp(np.zeros(1))))
        return out

    def observability_directions(self, first=0, count=None, tangent_units=False):
        """Rows [first, first + count) of the ascending list, (count, dim): unit eigenvectors v_i, or with tangent_units the
        directions δ_i in the parameters' own units."""
        i = self.observability_info()
        if count is None:
            count = i["dim"] - i["n_unobserved"] - first
        out = np.zeros((max(int(count), 0), i["dim"]))
        self._check(self.api.observability_get_directions(self.h, int(first), int(count), int(bool(tangent_units)),
                                                          _dp(out) if out.size else _dp(np.zeros(1))))
        return out

    def observability_block(self, index, block_id, tangent_units=False, size=None):
        """(entries of direction `index` in the block's tangent rows, the block's share of the unit eigenvector)."""
        if size is None:
            n = self._sizes[block_id]
            size = 3 if (n == 4 and self._manifolds.get(block_id) == MANIFOLD_EIGEN_QUATERNION) else n
        out = np.zeros(size)
        share = C.c_double(0)
        self._check(self.api.observability_get_block(self.h, int(index), int(block_id), int(bool(tangent_units)), _dp(out), C.byref(share)))
        return out, share.value

    def observability_matrix(self):
        """S̃ (dim x dim, zeros in dropped rows and columns)."""
        dim = self.observability_info()["dim"]
        out = np.zeros((dim, dim))
        self._check(self.api.observability_get_matrix(self.h, _dp(out) if out.size else _dp(np.zeros(1))))
        return out

    def observability_debug(self):
        """Test hook (calico_hip_testing.h): what the last observability compute did."""
        out = np.zeros(6)
        self._check(self.api.debug_observability_info(self.h, _dp(out), 6))
        return dict(in_lds=int(out[0]), kept=int(out[1]), reduced_rows=int(out[2]), rotations=int(out[3]),
                    min_relative_pivot_band=out[4], min_relative_pivot_root=out[5])

    def set_allreduce(self, pyfunc):
        cb = ALLREDUCE_FN(pyfunc)
        self._keep.append(cb)
        self._check(self.api.problem_set_allreduce(self.h, cb, None))

    def finalize(self):
        self._check(self.api.problem_finalize(self.h))

    PLAN_INFO_KEYS = ("fuse_expand", "frames", "items", "cells", "max_frames_per_cell", "max_items_per_cell", "tree_solver", "m",
                      "all_control_points_observed",
                      # what a linear solve does (calico_hip_testing.h): tree shape, launch fusions, reduced-solve route
                      "superblocks", "chain", "levels", "root", "schur_rides", "top_seps", "fused_back", "reduced_route",
                      "reduced_in_lds", "schur_slices", "reduced_m", "sep_n",
                      # the rest of the route (LinearRoute): what the solve's switches select, the first back-substitution's table entry
                      "elim", "level0_roll", "dense_mode", "back_pre", "inline_nodes", "first_back_qm", "first_back_mode")
    REDUCED_ROUTES = ("panel", "block", "blocked", "kernel")     # plan_info()["reduced_route"] indexes this

    def plan_info(self):
        """Test hook (calico_hip_testing.h): which evaluation route / solver the plan of this handle takes."""
        n = len(self.PLAN_INFO_KEYS)
        out = np.zeros(n, np.int32)
        self._check(self.api.debug_plan_info(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), n))
        return dict(zip(self.PLAN_INFO_KEYS, (int(v) for v in out)))

    def last_step(self, n=None):
        """Test hook (calico_hip_testing.h): (step, damping, scale) of the last linear solve of the last solve(), in
        calico_evaluate's column order (n=None), or in tangent order over every control point (n = 6 n_cp + m)."""
        n = self.num_effective_parameters() if n is None else int(n)
        step, damping, scale = np.zeros(n), np.zeros(n), np.zeros(n)
        self._check(self.api.debug_last_step(self.h, n, _dp(step), _dp(damping), _dp(scale)))
        return step, damping, scale

    def comm_init_rccl(self, unique_id, rank, world_size):
        """Native exchange: the handle creates its own RCCL communicator from the 128-byte id (see comm_unique_id)."""
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        self._check(self.api.comm_init_rccl(self.h, buf, int(rank), int(world_size)))

    def comm_info(self):
        """(rank, world, local residual blocks, total residual blocks) as the handle's communicator / shard sees them."""
        r, w = C.c_int32(0), C.c_int32(0)
        nl, nt = C.c_int64(0), C.c_int64(0)
        self._check(self.api.comm_info(self.h, C.byref(r), C.byref(w), C.byref(nl), C.byref(nt)))
        return r.value, w.value, nl.value, nt.value

    def set_shard(self, rank, world_size):
        self._check(self.api.problem_set_shard(self.h, int(rank), int(world_size)))

    def set_stream(self, stream_ptr):
        self._check(self.api.problem_set_stream(self.h, C.c_void_p(stream_ptr)))

    def set_phase_timing(self, mask):
        self._check(self.api.set_phase_timing(self.h, int(mask)))

    def phase_time(self, phase):
        ms = C.c_double(0)
        n = C.c_int64(0)
        self._check(self.api.get_phase_time(self.h, phase, C.byref(ms), C.byref(n)))
        return ms.value, n.value


_HIP_LIB_NAME = "libcalico_hip.so"
_hip_api = None


def hip_library_path():
    # CALICO_HIP_LIB (only with CALICO_DEV=1): another build of the same library, for development A/B runs
    # (profiles/dev/ab.sh); the product path is the in-tree one
    other = os.environ.get("CALICO_HIP_LIB") if os.environ.get("CALICO_DEV") == "1" else None
    return other or os.path.join(os.path.dirname(os.path.abspath(__file__)), _HIP_LIB_NAME)


def load_hip():
    """Load libcalico_hip.so (built in-tree by __graft_entry__.build()).

    Raises if it is missing - the product has no other backend."""
    global _hip_api
    if _hip_api is None:
        path = hip_library_path()
        if not os.path.exists(path):
            raise RuntimeError("%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the HIP library is the only backend; there is no CPU fallback)" % path)
        _hip_api = CApi(C.CDLL(path), "calico_", has_device=True)
    return _hip_api
