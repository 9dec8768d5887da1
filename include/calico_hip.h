/*
 * calico_hip.h — C ABI of libcalico_hip.so, the MI355X (gfx950) drop-in for the
 * hot path of yangjames/Calico:  BatchOptimizer::Optimize
 * (reference calico/batch_optimizer.cpp:53-81).
 *
 * The reference builds a ceres::Problem (parameter blocks + one residual block
 * per measurement), calls ceres::Solve, then re-evaluates every residual
 * block.  This header is what a maintainer binds instead of Ceres for that
 * path: every entry point names the reference interface it replaces.  The ABI
 * is plain C: opaque handle, caller-owned host buffers, int32 status codes
 * (absl::StatusCode numbering, as the reference's absl::Status uses), no
 * exceptions, no C++/torch types.
 *
 * Conventions
 *  - all floating point is IEEE-754 double (the reference path is double only);
 *  - quaternion blocks are stored x,y,z,w (Eigen::Quaterniond::coeffs(),
 *    reference optimization_utils.h:51-60);
 *  - host buffers are only read during the call that receives them;
 *  - one handle = one HIP device + one stream; a handle is not thread-safe.
 */
#ifndef CALICO_HIP_H_
#define CALICO_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: absl::StatusCode numbering ------------------------- */
#define CALICO_OK 0
#define CALICO_INVALID_ARGUMENT 3
#define CALICO_FAILED_PRECONDITION 9
#define CALICO_UNIMPLEMENTED 12
#define CALICO_INTERNAL 13

/* ---- enums: integer values identical to the reference ----------------- */
/* ceres manifold kinds used by the reference (optimization_utils.h:51-60) */
#define CALICO_MANIFOLD_EUCLIDEAN 0
#define CALICO_MANIFOLD_EIGEN_QUATERNION 1
/* sensors::CameraIntrinsicsModel (camera_models.h:16-33) */
#define CALICO_CAMERA_NONE 0
#define CALICO_CAMERA_OPENCV5 1
#define CALICO_CAMERA_OPENCV8 2
#define CALICO_CAMERA_KANNALA_BRANDT 3
#define CALICO_CAMERA_DOUBLE_SPHERE 4
#define CALICO_CAMERA_FIELD_OF_VIEW 5
#define CALICO_CAMERA_UNIFIED 6
#define CALICO_CAMERA_EXTENDED_UNIFIED 7
/* sensors::{Gyroscope,Accelerometer}IntrinsicsModel (gyroscope_models.h:16-25) */
#define CALICO_IMU_NONE 0
#define CALICO_IMU_SCALE_ONLY 1
#define CALICO_IMU_SCALE_AND_BIAS 2
#define CALICO_IMU_VECTOR_NAV 3
/* utils::LossFunctionType (optimization_utils.h:15-22) */
#define CALICO_LOSS_NONE 0
#define CALICO_LOSS_HUBER 1
#define CALICO_LOSS_CAUCHY 2
/* ceres::TerminationType */
#define CALICO_CONVERGENCE 0
#define CALICO_NO_CONVERGENCE 1
#define CALICO_FAILURE 2
/* sensor kinds of this ABI */
#define CALICO_SENSOR_CAMERA 0
#define CALICO_SENSOR_GYROSCOPE 1
#define CALICO_SENSOR_ACCELEROMETER 2

typedef struct calico_problem calico_problem;

/* Mirrors the fields of ceres::Solver::Options the reference sets or exposes
 * (batch_optimizer.cpp:10-17, calico.cpp:378-394) plus the Ceres trust-region
 * defaults the path depends on.  calico_default_solver_options() fills it the
 * way DefaultSolverOptions() + Ceres defaults do. */
typedef struct calico_solver_options {
  int32_t max_num_iterations;                /* 50 */
  int32_t num_threads;                       /* 1; honoured by CPU code only */
  int32_t minimizer_progress_to_stdout;      /* reference default: 1 */
  int32_t jacobi_scaling;                    /* 1 */
  int32_t max_num_consecutive_invalid_steps; /* 5 */
  int32_t sync_every; /* HIP: LM iterations enqueued between host syncs (>=1) */
  double function_tolerance;                 /* 1e-8  (batch_optimizer.cpp:14) */
  double gradient_tolerance;                 /* 1e-10 */
  double parameter_tolerance;                /* 1e-10 (batch_optimizer.cpp:15) */
  double initial_trust_region_radius;        /* 1e4 */
  double max_trust_region_radius;            /* 1e16 */
  double min_trust_region_radius;            /* 1e-32 */
  double min_relative_decrease;              /* 1e-3 */
  double min_lm_diagonal;                    /* 1e-6 */
  double max_lm_diagonal;                    /* 1e32 */
} calico_solver_options;

/* The fields of ceres::Solver::Summary the reference reads or binds
 * (calico.cpp:356-375, batch_optimizer_test.cpp:186-187). */
typedef struct calico_summary {
  int32_t termination_type;
  int32_t num_successful_steps;
  int32_t num_unsuccessful_steps;
  int32_t num_iterations; /* LM iterations run, iteration 0 excluded */
  int32_t num_jacobian_evaluations;
  int32_t num_cost_evaluations;
  int32_t num_residual_blocks;
  int32_t num_residuals;
  int32_t num_parameter_blocks;
  int32_t num_parameters;
  int32_t num_effective_parameters;
  int32_t num_residual_blocks_reduced;
  int32_t num_residuals_reduced;
  int32_t num_parameter_blocks_reduced;
  int32_t num_parameters_reduced;
  int32_t num_effective_parameters_reduced;
  double initial_cost;
  double final_cost;
  double total_time_in_seconds;
  double solve_time_in_seconds; /* LM loop only (device-timed on HIP) */
  char message[256];
} calico_summary;

/* One row of Ceres' per-iteration progress table. */
typedef struct calico_iteration {
  int32_t iteration;
  int32_t step_is_valid;
  int32_t step_is_successful;
  int32_t reserved;
  double cost;
  double cost_change;
  double gradient_max_norm;
  double step_norm;
  double relative_decrease;
  double trust_region_radius;
} calico_iteration;

/* ---- lifetime --------------------------------------------------------- */
/* Replaces `ceres::Problem problem;` (batch_optimizer.cpp:57).  device = HIP
 * device ordinal. Fails with CALICO_INTERNAL when no GPU is usable: there is
 * no CPU fallback behind this ABI. */
int32_t calico_problem_create(calico_problem** out, int32_t device);
void calico_problem_destroy(calico_problem* p);
/* Message of the last non-OK status on this handle ("" if none). p == NULL: of the calling thread's last non-OK call that
 * takes no handle or was given none (calico_camera_unproject, calico_camera_project_points, calico_camera_resect,
 * calico_camera_calibrate, calico_rig_calibrate, calico_imu_align, calico_camera_align, calico_accel_align, calico_imu_allan); like a
 * handle's message it is not cleared by a later success. */
const char* calico_last_error(const calico_problem* p);
void calico_default_solver_options(calico_solver_options* o);

/* ---- parameters ------------------------------------------------------- */
/* Replaces ceres::Problem::AddParameterBlock (+ SetParameterBlockConstant,
 * + EigenQuaternionManifold) as used by world_model.cpp:40-77,
 * bspline.hpp:10-17, camera.cpp:92-113, gyroscope.cpp:10-31,
 * accelerometer.cpp:10-33, optimization_utils.h:51-68.  size must be 4 for
 * the quaternion manifold. */
int32_t calico_problem_add_param_block(calico_problem* p, const double* values,
                                       int32_t size, int32_t manifold,
                                       int32_t is_constant,
                                       int32_t* block_id_out);
/* Bulk form for n blocks of one size and manifold (the model points of a chart, the control points of the spline):
 * values n x size row-major, is_constant one byte per block (NULL: none is constant), ids returned in block_ids_out. */
int32_t calico_problem_add_param_blocks(calico_problem* p, int32_t n, int32_t size, int32_t manifold,
                                        const uint8_t* is_constant, const double* values, int32_t* block_ids_out);
/* Read / overwrite the current value of a block (the reference hands Ceres
 * pointers into the user's objects and reads them back in place). */
int32_t calico_get_param_block(calico_problem* p, int32_t block_id,
                               double* out);
int32_t calico_set_param_block(calico_problem* p, int32_t block_id,
                               const double* values);
/* Bulk forms: n blocks, values concatenated in the order of block_ids. Ceres reads and writes through the pointers
 * Trajectory::AddParametersToProblem / WorldModel::AddParametersToProblem hand it (trajectory.cpp:51-60,
 * world_model.cpp:52-61), so after Optimize() (batch_optimizer.cpp:72-78) the control points and model points are
 * simply there; here they are fetched -- in one call instead of one per control point. */
int32_t calico_set_param_blocks(calico_problem* p, int32_t n,
                                const int32_t* block_ids,
                                const double* values);
int32_t calico_get_param_blocks(calico_problem* p, int32_t n,
                                const int32_t* block_ids,
                                double* values_out);

/* Replaces Trajectory::AddParametersToProblem + GetEvaluationParams
 * (trajectory.cpp:51-79, bspline.hpp:138-161): the uniform knot vector
 * (n_knots entries), the per-segment basis matrices (n_segments × order ×
 * order, row-major, n_segments = n_knots - 2*(order-1) - 1) and the block ids
 * of the n_knots - order control points (6-vectors [axis-angle; position]). */
int32_t calico_problem_set_spline(calico_problem* p, int32_t order,
                                  int32_t n_knots, const double* knots,
                                  const double* basis,
                                  const int32_t* ctrl_block_ids);

/* Rigid body (calibration chart) pose blocks, world_model.h:54-69. */
int32_t calico_problem_add_rigid_body(calico_problem* p, int32_t q_block,
                                      int32_t t_block, int32_t* body_id_out);

/* ---- sensors ---------------------------------------------------------- */
/* One call per Sensor object: what AddParametersToProblem registered plus the
 * per-sensor state AddResidualsToProblem reads (model, sigma -> information
 * 1/sigma, loss type + scale).  kind/model per the enums above.
 * gravity_block is used by accelerometers only (pass -1 otherwise). */
int32_t calico_problem_add_sensor(calico_problem* p, int32_t kind,
                                  int32_t model, int32_t intrinsics_block,
                                  int32_t q_block, int32_t t_block,
                                  int32_t latency_block, int32_t gravity_block,
                                  double sigma, int32_t loss,
                                  double loss_scale, int32_t* sensor_id_out);

/* Replaces Camera::AddResidualsToProblem (camera.cpp:115-153) for the
 * non-outlier measurements of one camera: pixels n×2, stamps n, the rigid
 * body and the model-point parameter block of every observation. */
int32_t calico_problem_add_camera_residuals(calico_problem* p,
                                            int32_t sensor_id, int64_t n,
                                            const double* pixels,
                                            const double* stamps,
                                            const int32_t* body_ids,
                                            const int32_t* point_blocks);
/* Replaces Gyroscope/Accelerometer::AddResidualsToProblem
 * (gyroscope.cpp:33-54, accelerometer.cpp:35-56): measurements n×3. */
int32_t calico_problem_add_imu_residuals(calico_problem* p, int32_t sensor_id,
                                         int64_t n, const double* measurements,
                                         const double* stamps);

/* Flatten the recorded blocks into the device-side problem now (cells, work items, gather lists, elimination plan;
 * uploads) instead of inside the first calico_solve / calico_evaluate. What BatchOptimizer::Optimize does before
 * ceres::Solve on every call (batch_optimizer.cpp:57-70: it rebuilds the ceres::Problem each time), made separately
 * callable so that its cost can be measured (bench.py: config.setup_ms). */
int32_t calico_problem_finalize(calico_problem* p);

/* The plan -- everything calico_problem_finalize derives -- depends on the STRUCTURE of the problem only (block sizes,
 * manifolds and constancy; the spline's knots, basis and control-point blocks; every sensor's model, blocks, sigma and
 * loss; per observation its stamp, rigid body and model point), not on parameter values or measurements. The library
 * keeps the plans of the last few structures it has seen (keyed on a 128-bit hash of exactly those inputs, per device)
 * together with the device workspaces of destroyed handles: BatchOptimizer::Optimize rebuilds its problem on every call
 * (batch_optimizer.cpp:57-70), and a rebuilt problem of known structure then only uploads its values. A structure that
 * differs in any of those inputs is planned afresh. CALICO_PLAN_CACHE=0 in the environment switches the cache off.
 * calico_plan_cache_stats: look-ups served from the cache / planned afresh since the process started, plans held.
 * calico_plan_cache_clear: drops the cached plans and workspaces; the device memory of plans no live handle uses, and
 * every allocation slab of the library nothing lives in any more, goes back to the driver (hipFree). Destroying a handle
 * does the same for all idle slabs but one per device. */
int32_t calico_plan_cache_stats(int64_t* hits_out, int64_t* misses_out, int64_t* entries_out);
int32_t calico_plan_cache_clear(void);

/* ---- solve ------------------------------------------------------------ */
/* Replaces ceres::Solve (batch_optimizer.cpp:72-73): Levenberg–Marquardt
 * trust region on the flattened problem, entirely on the device. On return the
 * summary, the iteration table and the parameter values are complete; a few
 * kernels of iterations enqueued ahead of the device (they exit at once) may
 * still be draining on the handle's stream -- later calls on the handle are
 * ordered behind them. */
int32_t calico_solve(calico_problem* p, const calico_solver_options* options,
                     calico_summary* summary);
/* Per-iteration table of the last solve; returns rows written via *n_out. */
int32_t calico_get_iterations(calico_problem* p, calico_iteration* out,
                              int32_t max_rows, int32_t* n_out);

/* Replaces Sensor::UpdateResiduals (camera.cpp:70-80, gyroscope.cpp:171-182,
 * accelerometer.cpp:58-69): sigma-weighted residuals WITHOUT the loss
 * function, in the order the residuals were added. out is n×dim (dim 2 for a
 * camera, 3 for an IMU sensor); valid[i]=0 where the projection failed
 * (the reference returns kInternal in that case; so does this call, after
 * filling both arrays). */
int32_t calico_get_residuals(calico_problem* p, int32_t sensor_id, double* out,
                             uint8_t* valid);
/* Spline initialisation on the device: BSpline::FitToData / FitSpline (bspline.hpp:19-37, 246-297), behind
 * Trajectory::FitSpline (trajectory.cpp:14-49). Least-squares control points (n_knots - order rows of 6) of the
 * spline on the given knot vector / basis matrices (as for calico_problem_set_spline) through n sorted samples
 * `data6` (n x 6: axis-angle, position) at `stamps`. The reference factors the dense normal equations X^T X by
 * column-pivoted QR; here the banded normal equations are assembled in a fixed order (the result is bit-reproducible)
 * and solved by a banded Cholesky with a ridge of 1e-15 mean_diag (mean_diag = trace(X^T X) / n_ctrl).
 * Accuracy (profiles/EXPERIMENTS.md, "spline fit accuracy"): the control points lie within ~1e-15 cond2(X)^2 max|C| of
 * exact least squares -- 2e-9 at order 6 with the last segment covered (cond2 1.8e3), 1e-6 with the last sample half-way
 * into it (cond2 4.3e4) -- and the fitted values at the samples never further, up to 6 decades closer as cond2 grows
 * (4e-11 in the latter case).
 * Control points the samples do not determine are decoupled: a Cholesky pivot <= 1e-13 mean_diag is replaced by
 * mean_diag and the control point comes back ~0 (exactly 0 where no sample touches it; sqrt(pivot / mean_diag) times
 * the samples' noise otherwise). This is a cliff, not a rank test: at order 6 with 100 Hz samples on 10 Hz knots, a
 * last sample 10 % into the last segment leaves the last control point an exact pivot of 3e-16 mean_diag and it is
 * dropped, although X has full rank (cond2 9.4e7); at 30 % the pivot is 1.7e-11 (cond2 4.1e5) and it is kept; at 20 %
 * (3.3e-13) it lies within a decade of the threshold, where roundoff decides. With fewer distinct samples than the
 * control points they touch (one sample per segment, n <= 3) the ridge decides which are kept: the values at the samples
 * are fitted, the largest control point measures 1.2 to 14.5 times the minimum-norm solution's (the latter for a single
 * sample at mid-segment). kInvalidArgument for unsorted stamps, stamps outside the valid
 * knots or bad sizes; kUnimplemented when the band does not fit the on-chip solve (n_ctrl (order + 6) 8 bytes > 156 KiB:
 * more than 1664 control points at order 6, 1426 at order 8; ctrl_out is then left untouched) or n exceeds INT32_MAX.
 * Needs no problem handle: owns its device memory, the argument rules are checked before the device is touched, message in
 * calico_last_error(NULL). */
int32_t calico_fit_spline(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis,
                          int64_t n, const double* stamps, const double* data6, double* ctrl_out);

/* The smoothing (penalised) spline fit: per channel group g (0: axis-angle, channels 0..2; 1: position, channels 3..5)
 *   min_C  sum_j w_jg |X_j C - d_j|^2  +  lambda_g  integral |s^(m)(t)|^2 dt   over the valid knots,
 * for a whole grid of lambda in one launch (one workgroup per group and lambda). The penalty matrix P -- the Gram matrix of the
 * m-th derivatives of the basis functions, closed form per segment -- has the band of X^T W X, so each candidate is the banded
 * Cholesky of calico_fit_spline on A = X^T W X + lambda P, with the same ridge (1e-15 mean_diag of A) and the same pivot rule.
 * What the samples leave open (a gap longer than the spline's support, one sample per segment, a ragged end) the penalty
 * decides: with lambda > 0 and m <= the number of distinct samples, A is positive definite and no pivot is replaced.
 *   weights  n x 2 [rotation, position], >= 0 and finite, or NULL (all 1). A sample of weight 0 in a group is skipped for that
 *            group: its data are not read. Each group needs one sample of positive weight.
 *   lambda   n_lambda values per group, >= 0 and strictly ascending; with `relative` in units of trace(X^T W X) / trace(P) of
 *            the group (taken on the device), so that 1e-3 means the same on every trajectory; otherwise absolute (data
 *            units^2 s^(2m-1)). lambda = 0 is the plain weighted fit; with weights NULL, n_lambda 1 and both lambda 0, ctrl_out
 *            has calico_fit_spline's bits.
 *   choice   target_rms 0: the first lambda of the grid. target_rms > 0: the largest lambda whose weighted RMS is <= the
 *            target (discrepancy principle); if none is, CALICO_FIT_TARGET_NOT_MET and the smallest lambda. A lambda whose
 *            factorisation met a pivot that is not finite is never chosen and its control points are not written (its
 *            row's rss, penalty and rms are NaN); if a group has no other, the call returns kInternal.
 * ctrl_out (n_ctrl x 6) receives each group's chosen lambda; ctrl_all_out (n_lambda x n_ctrl x 6, may be NULL) every lambda's;
 * rows_out (2 x n_lambda, group-major, may be NULL) and summary what was found. Bit-reproducible: fixed-order sums, no atomics.
 * kInvalidArgument as for calico_fit_spline, and for a weight, lambda or target that is negative or not finite, a grid that is
 * not strictly ascending, n_lambda outside [1, CALICO_FIT_MAX_LAMBDAS], derivative outside [1, min(3, order - 1)], a NULL
 * summary or ctrl_out. kUnimplemented, outputs untouched, when one group's [band | 3 rhs] does not fit the on-chip solve
 * (n_ctrl (order + 3) 8 bytes > 156 KiB: more than 2218 control points at order 6) or n exceeds INT32_MAX. Needs no problem handle. */
#define CALICO_FIT_MAX_LAMBDAS 32
#define CALICO_FIT_OK 0
#define CALICO_FIT_NOT_POSITIVE_DEFINITE 1   /* a pivot was not finite: this lambda's control points are not written and never chosen */
#define CALICO_FIT_TARGET_NOT_MET 2          /* group status only: no lambda of the grid reached target_rms; the smallest lambda was taken */
typedef struct {
  int32_t derivative;       /* 2: m, the penalised derivative; 1 <= m <= min(3, order - 1) */
  int32_t relative;         /* 1: lambdas are multiples of trace(X^T W X) / trace(P) of their group; 0: absolute */
  int32_t n_lambda;         /* 1; at most CALICO_FIT_MAX_LAMBDAS */
  double lambda_rot[CALICO_FIT_MAX_LAMBDAS];   /* {1e-3}; >= 0, strictly ascending */
  double lambda_pos[CALICO_FIT_MAX_LAMBDAS];   /* {1e-3} */
  double target_rms_rot;    /* 0: take lambda_rot[0]. > 0: the largest lambda of the grid whose weighted RMS <= target */
  double target_rms_pos;
} calico_spline_fit_options;
typedef struct {            /* one per (group, lambda) */
  int32_t status;           /* CALICO_FIT_OK or CALICO_FIT_NOT_POSITIVE_DEFINITE */
  int32_t replaced_pivots;  /* pivots the 1e-13 rule replaced (0 on a well-posed penalised fit) */
  double lambda;            /* the absolute lambda that was used */
  double rss;               /* sum_j w_j |X_j C - d_j|^2 over the group's three channels */
  double penalty;           /* sum over the channels of c^T P c */
  double rms;               /* sqrt(rss / (3 n_used)), n_used = samples of weight > 0 */
} calico_spline_fit_row;
typedef struct {
  int32_t status[2];        /* per group: CALICO_FIT_OK, CALICO_FIT_NOT_POSITIVE_DEFINITE (no usable lambda) or CALICO_FIT_TARGET_NOT_MET */
  int32_t chosen[2];        /* index into the grid, -1: none */
  int64_t n_used[2];
} calico_spline_fit_summary;
void calico_default_spline_fit_options(calico_spline_fit_options* o);
int32_t calico_fit_spline_smooth(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis,
                                 int64_t n, const double* stamps, const double* data6,
                                 const double* weights /* n x 2: [rotation, position], or NULL = 1 */,
                                 const calico_spline_fit_options* o /* NULL = defaults */,
                                 double* ctrl_out /* n_ctrl x 6: the chosen lambda of each group */,
                                 double* ctrl_all_out /* n_lambda x n_ctrl x 6, may be NULL */,
                                 calico_spline_fit_row* rows_out /* 2 x n_lambda, may be NULL */,
                                 calico_spline_fit_summary* summary);

/* The robust spline fit: iteratively reweighted least squares around calico_fit_spline_smooth, for samples that are wrong and not
 * known to be (a resected pose on the other branch of the planar ambiguity reports a small RMS). One independent loop per channel
 * group g, with prior weights w_j (weights[:, g], NULL = 1); the loop stays on the device, the host reads back once.
 *   iteration 0      calico_fit_spline_smooth with n_lambda 1 (bit for bit). Its absolute lambda is frozen: a relative lambda is not
 *                    re-derived from the reweighted trace, so the objective does not move with the weights.
 *   iteration 1..T   e_j = |X_j C - d_j|_2 (the norm over the group's three channels) over the m samples with w_j > 0;
 *                    med = the element of rank (m - 1) / 2 of the sorted e (the lower median, an exact order statistic);
 *                    sigma = max(med / 1.5381722544550522, min_scale) -- the constant is sqrt(median of chi2_3), so sigma is the
 *                    per-channel standard deviation of Gaussian residuals -- or the caller's scale > 0 (no selection runs then);
 *                    sigma == 0: the group stops with CALICO_FIT_SCALE_ZERO at the previous control points and all u = 1;
 *                    z = e / sigma;  Huber: u = min(1, c / z);  Tukey: u = (1 - (z / c)^2)^2 for z < c, else 0;
 *                    (X^T diag(w u) X + lambda_abs P) C = X^T diag(w u) d with the smoothing fit's sums, ridge and pivot rule (a
 *                    total weight of 0 is skipped like a prior weight of 0);
 *                    step = max|C - C_prev| / max|C| (0 where no control point moved). 0 < step_tolerance and step <= it: the
 *                    group is converged, CALICO_FIT_OK; after T iterations without that CALICO_FIT_MAX_ITERATIONS. A pivot that
 *                    is not finite: CALICO_FIT_NOT_POSITIVE_DEFINITE, the group keeps the previous control points and the call
 *                    returns kInternal (at iteration 0: that group's columns of ctrl_out are not written).
 *   afterwards       one more residual pass gives residuals_out at ctrl_out.
 * On data without noise the median residual is the spline's own approximation error, and Huber at a vanishing scale is an L1 fit
 * that the iteration approaches slowly: give the noise floor as min_scale, or the scale itself.
 * tuning 0 is the loss's default: c = 2.7955 for Huber (sqrt of the 95 % point of chi2_3), twice that for Tukey (conventions).
 * robust_weights_out (n x 2, may be NULL) holds u of the last solve (1 where no reweighting ran), 0 where w = 0; residuals_out
 * (n x 2, may be NULL) e at ctrl_out, NaN where w = 0 (those data are not read). The summary's scale and median_residual are the
 * ones the last reweighting used (NaN: none ran; median_residual NaN with a caller's scale). Bit-reproducible: the selection adds
 * integers only, every floating-point sum has a fixed order.
 * kInvalidArgument for everything calico_fit_spline_smooth refuses, and for fit.n_lambda != 1 or a non-zero target, an unknown
 * loss, max_iterations outside [0, CALICO_FIT_ROBUST_ITERATION_LIMIT], a negative or non-finite tuning, scale, min_scale or
 * step_tolerance, a NULL summary or ctrl_out. kUnimplemented, outputs untouched, at the smoothing fit's LDS ceiling. */
#define CALICO_FIT_MAX_ITERATIONS 3          /* group status: max_iterations reweighted solves without step <= step_tolerance */
#define CALICO_FIT_SCALE_ZERO 4              /* group status: the scale estimate was 0 (set min_scale); previous control points kept */
#define CALICO_ROBUST_HUBER 1
#define CALICO_ROBUST_TUKEY 2
#define CALICO_FIT_ROBUST_ITERATION_LIMIT 64
typedef struct {
  int32_t loss;             /* CALICO_ROBUST_HUBER */
  int32_t max_iterations;   /* 20; 0..CALICO_FIT_ROBUST_ITERATION_LIMIT; 0 = the smoothing fit */
  double tuning_rot;        /* 0 = the loss's default */
  double tuning_pos;
  double scale_rot;         /* 0 = estimate every iteration */
  double scale_pos;
  double min_scale_rot;     /* 0 */
  double min_scale_pos;
  double step_tolerance;    /* 1e-9; 0 = run every iteration */
} calico_spline_robust_options;
typedef struct {            /* per group */
  int32_t status[2];        /* CALICO_FIT_OK, _NOT_POSITIVE_DEFINITE, _MAX_ITERATIONS or _SCALE_ZERO */
  int32_t iterations[2];    /* reweighted solves that produced the control points */
  int32_t replaced_pivots[2];
  int64_t n_used[2];
  int64_t n_downweighted[2];   /* 0 < u < 1 */
  int64_t n_rejected[2];       /* u == 0 */
  double lambda[2];         /* the absolute lambda of every solve */
  double scale[2];
  double median_residual[2];
  double last_step[2];
  double rss[2];            /* sum w u e^2 at the result */
} calico_spline_robust_summary;
void calico_default_spline_robust_options(calico_spline_robust_options* o);
int32_t calico_fit_spline_robust(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis,
                                 int64_t n, const double* stamps, const double* data6,
                                 const double* weights /* n x 2 or NULL */,
                                 const calico_spline_fit_options* fit /* NULL = defaults; n_lambda must be 1, targets 0 */,
                                 const calico_spline_robust_options* robust /* NULL = defaults */,
                                 double* ctrl_out /* n_ctrl x 6 */,
                                 double* robust_weights_out /* n x 2, may be NULL */,
                                 double* residuals_out /* n x 2, may be NULL */,
                                 calico_spline_robust_summary* summary);

/* The smoothing fit with lambda chosen by cross-validation: calico_fit_spline_smooth's grid, and per (group, lambda) what the fit
 * says about its own predictive error, without a noise level from the caller (target_rms needs one, and nobody has it before
 * calibrating). With A = X^T W X + lambda P the hat matrix is H = X A^-1 X^T W; its diagonal and trace need only the entries of
 * A^-1 inside A's band, which Takahashi's selected inversion takes from the banded Cholesky factor the fit already holds on chip
 * (O(n_ctrl order^2), in place). A^-1 is the inverse of the matrix that was factored (A plus the fit's ridge, 1e-15 mean_diag).
 *   h_j      w_j X_j A^-1 X_j^T, the leverage of sample j: the share of its own datum in its fitted value, in [0, 1)
 *   edf      tr(A^-1 X^T W X) = sum_j h_j, the effective degrees of freedom per channel, from the band alone
 *   gcv      (rss / (3 n_used)) / (1 - edf / n_used)^2, n_used = samples of weight > 0; +inf when edf >= n_used
 *   press    sum_j w_j e_j^2 / (1 - h_j)^2 / (3 n_used), e_j = |X_j C - d_j|_2 over the group's three channels: the mean squared
 *            leave-one-out residual, exactly what n_used refits without sample j give AT THE ROW'S ABSOLUTE LAMBDA -- a relative
 *            lambda is converted once, from the full data, and not again for each left-out sample; +inf if any h_j >= 1
 *   choice   per group the smallest score (gcv or press, options.criterion) over the eligible rows; a tie goes to the larger
 *            lambda. A row whose factorisation was not finite, or replaced a pivot (A^-1 is then not the inverse of the fit's
 *            matrix), is never eligible and its cv row is NaN. No eligible row: CALICO_FIT_NOT_POSITIVE_DEFINITE, kInternal, and
 *            that group's columns of ctrl_out, leverage_out and loo_residuals_out are not written. n_lambda >= 2 and the choice
 *            is the first or last entry: CALICO_FIT_CV_AT_GRID_END -- the call succeeds, the minimum may lie outside: extend the grid.
 * ctrl_all_out and rows_out are calico_fit_spline_smooth's for the same inputs bit for bit (the solve, the lambda scaling, rss and
 * penalty are the same code); ctrl_out holds each group's columns of ctrl_all_out at the choice. cv_rows_out (2 x n_lambda,
 * group-major, may be NULL); leverage_out (n x 2, may be NULL) h_j at each group's chosen lambda, 0 where w_j = 0 (those data are
 * not read); loo_residuals_out (n x 2, may be NULL) e_j / (1 - h_j), NaN where w_j = 0 and +inf where h_j >= 1. Bit-reproducible:
 * no atomics, every sum in a fixed order; the choice is made on the device and the host reads back once.
 * Measured (profiles/EXPERIMENTS.md, "Spline fit cross-validation"): h and edf within a few 1e-16 cond2(A) of a long-double inverse.
 * kInvalidArgument for everything calico_fit_spline_smooth refuses, and for a non-zero target_rms (choosing is this call's own
 * job) or an unknown criterion. kUnimplemented, outputs untouched, at the smoothing fit's LDS ceiling. */
#define CALICO_FIT_CV_AT_GRID_END 5          /* group status: the chosen lambda is the grid's first or last entry */
#define CALICO_FIT_CV_GCV 0
#define CALICO_FIT_CV_PRESS 1
typedef struct {
  int32_t criterion;        /* CALICO_FIT_CV_GCV */
  int32_t reserved;         /* 0 */
} calico_spline_cv_options;
typedef struct {            /* one per (group, lambda); all NaN where the row is not eligible */
  double edf;
  double gcv;
  double press;
  double max_leverage;      /* max_j h_j */
} calico_spline_cv_row;
typedef struct {            /* per group */
  int32_t status[2];        /* CALICO_FIT_OK, CALICO_FIT_CV_AT_GRID_END or CALICO_FIT_NOT_POSITIVE_DEFINITE (no eligible lambda) */
  int32_t chosen[2];        /* index into the grid, -1: none */
  int64_t n_used[2];
  double edf[2];            /* at the choice (NaN: none) */
  double score[2];          /* the criterion's value at the choice */
} calico_spline_cv_summary;
void calico_default_spline_cv_options(calico_spline_cv_options* o);
int32_t calico_fit_spline_cv(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis,
                             int64_t n, const double* stamps, const double* data6,
                             const double* weights /* n x 2 or NULL */,
                             const calico_spline_fit_options* fit /* NULL = defaults; targets must be 0 */,
                             const calico_spline_cv_options* cv /* NULL = defaults */,
                             double* ctrl_out /* n_ctrl x 6 */,
                             double* ctrl_all_out /* n_lambda x n_ctrl x 6, may be NULL */,
                             calico_spline_fit_row* rows_out /* 2 x n_lambda, may be NULL */,
                             calico_spline_cv_row* cv_rows_out /* 2 x n_lambda, may be NULL */,
                             double* leverage_out /* n x 2, may be NULL */,
                             double* loo_residuals_out /* n x 2, may be NULL */,
                             calico_spline_cv_summary* summary);

/* Outlier tags (Camera::MarkOutliersById / ClearOutliers, camera.cpp:281-301; outlier_ids_, camera.h:185): tagged
 * observations stay registered but are left out of the problem, as AddResidualsToProblem does (camera.cpp:121-124) --
 * no residual block, no residual, not counted in the summary. `is_outlier` has one byte per observation of the
 * sensor in insertion order; NULL clears all tags. */
int32_t calico_problem_set_outlier_mask(calico_problem* p, int32_t sensor, const uint8_t* is_outlier);
/* One pass of the demos' tagging loop (kalibr_multicam_demo.ipynb:666-674) on the device: residuals at the current
 * estimates without the loss function, every still-untagged observation of `sensor` with ||r|| > threshold (or that
 * cannot be evaluated) is tagged. *n_marked = number of observations tagged by this call. Follow with calico_solve. */
int32_t calico_mark_outliers(calico_problem* p, int32_t sensor, double threshold, int64_t* n_marked);
/* Residual statistics of a camera on the device (utils.py:12-50 ComputeRmseHeatmapAndFeatureCount, the notebooks'
 * per-region RMSE / feature count): the image (image_width x image_height pixels) is divided into num_rows x num_cols
 * bins by the measured pixel; rmse_out[row * num_cols + col] = sqrt(sum ||r||^2 / count) over the untagged
 * observations of the bin (residuals at the current estimates without the loss function, NaN for an empty bin like
 * the reference's 0/0), count_out the number of observations. Fixed-order reductions: results are reproducible. */
int32_t calico_residual_heatmap(calico_problem* p, int32_t sensor, int32_t image_width, int32_t image_height,
                                int32_t num_rows, int32_t num_cols, double* rmse_out, int64_t* count_out);

/* Sensor::Project for the registered observations (camera.cpp:155-208, gyroscope.cpp:56-82,
 * accelerometer.cpp:76-123): the model's prediction -- pixel (2) or IMU reading (3) per observation, in insertion
 * order -- at the current parameter values, i.e. exactly the quantity the residual compares the measurement with
 * (pose at stamp - latency, spline segment of the stamp). Evaluated by the residual kernel in prediction mode, so
 * measurements generated with it give residuals that are exactly zero. Points that do not project (the reference
 * skips them) come back with valid[i] = 0. `valid` may be NULL. */
int32_t calico_project(calico_problem* p, int32_t sensor, double* out, uint8_t* valid);

/* The outlier-tagging step that follows the path in the reference's demos
 * (kalibr_multicam_demo.ipynb:666-674 -> Camera::MarkOutliersById):
 * mask[i] = 1 iff the residual is valid and ||r_i|| <= threshold. */
int32_t calico_get_inlier_mask(calico_problem* p, int32_t sensor_id,
                               double threshold, uint8_t* mask);

/* ---- evaluation entry points (parity tests, benchmarks) --------------- */
/* Number of tangent columns of the reduced problem and their order:
 * [control points (6 each, spline order) | remaining free, used blocks in
 * block-id order]. */
int32_t calico_num_effective_parameters(calico_problem* p, int32_t* n_out);
/* One residual+Jacobian evaluation at the current parameters, as Ceres'
 * Evaluator would do for the LM loop (loss corrected, manifold projected):
 * cost, gradient (n), and the Gauss-Newton matrix JᵀJ expanded to dense
 * row-major n×n.  Any output pointer may be NULL. */
int32_t calico_evaluate(calico_problem* p, double* cost, double* gradient,
                        double* jtj_dense);

/* ---- covariance of the estimates (ceres::Covariance) ------------------ */
/* Σ = (JᵀJ)⁻¹ of the dense border -- every free, used block that is not a spline control point: intrinsics,
 * extrinsics q / t, latencies, gravity, a free chart pose, free model points, rigid bodies -- with all cross-covariances,
 * at the current parameter values. JᵀJ is the Gauss-Newton matrix exactly as the LM loop evaluates it: sigma-weighted
 * residuals, the robust loss applied through the same corrector (Ceres' apply_loss_function = true), quaternion blocks
 * in the EigenQuaternion tangent. No LM damping and no Jacobi scaling enter the result (an internal symmetric
 * equilibration is undone).
 *  - No a-posteriori variance factor is applied. To scale by the estimated residual variance, multiply Σ by
 *    2·cost / (num_residuals - num_effective_parameters) (calico_summary) yourself.
 *  - The control points are eliminated (Schur complement, as in the solver): Σ is their marginal over them. Their own
 *    blocks are computed only on request (control_points = 1, below); otherwise calico_covariance_get_block returns
 *    CALICO_UNIMPLEMENTED for them.
 *  - Constant (and unused) blocks read back as zeros, as in Ceres.
 *  - Deviation from Ceres: a tangent column whose JᵀJ diagonal is exactly 0.0 -- no residual depends on it, e.g. the
 *    gyroscope's translation block -- is left out of the inversion and its rows and columns of Σ are 0 (the
 *    Moore-Penrose result for a zero column). Ceres' default would reject every IMU problem because of it.
 *  - Any other rank deficiency (a gauge freedom, a non-finite value) makes calico_covariance_compute return
 *    CALICO_FAILED_PRECONDITION with a message in calico_last_error. The test is a RELATIVE PIVOT threshold on the
 *    equilibrated reduced system (unit diagonal: a pivot is the fraction of a column's JᵀJ diagonal the other columns do
 *    not explain), not Ceres' min_reciprocal_condition_number on J -- formed from JᵀJ in double precision, a
 *    reciprocal condition number of J below ~1e-8 is out of reach.
 *    Default: see calico_default_covariance_options.
 * The result lives in a buffer of the handle from the first compute to the next compute or calico_problem_destroy; a
 * structural change of the problem (blocks, sensors, observations, shard) makes the readers return
 * CALICO_FAILED_PRECONDITION until the next compute. Ambient blocks are lifted at the values Σ was computed at.
 * calico_covariance_compute leaves the parameters, the LM state, the iteration log and the last summary alone (a solve
 * after it is bit-identical to one without it). On a sharded handle it takes the same exchange as an evaluation (every
 * rank calls it): every rank then holds the same Σ. */
typedef struct calico_covariance_options {
  double min_relative_pivot;   /* smallest relative pivot accepted (>= 0) */
  int32_t control_points;      /* 0 or 1: also compute the trajectory's blocks (below) */
  int32_t reserved[5];
} calico_covariance_options;
/* Defaults. control_points = 0. min_relative_pivot = 1e-12, in the gap measured on the test scenes (tests/test_gpu_covariance.py prints
 * them): the well-posed scenes' minimum relative pivots lie between 3.7e-5 and 8.7e-3 (six camera models, the scale-only
 * and scale-and-bias IMU models robust and not, free model points, spline orders 7 and 8, the banded solver, the configs[3]
 * and configs[4] shapes), the gauge-deficient scene's
 * (camera-only, free chart pose) is 6.4e-16 -- rounding noise of an exactly singular system; an exactly singular
 * column gives a pivot <= 0, reported as 0. */
void calico_default_covariance_options(calico_covariance_options* o);
/* The trajectory's part of Σ (control_points = 1). Tangent order as calico_num_effective_parameters: control points first
 * (6 each, Euclidean: ambient = tangent), then the border. With H = JᵀJ = [[A, E], [Eᵀ, C]], A the control points' block band
 * (block bandwidth order - 1), the compute adds
 *  - every cross block control point x border block, Σ_AE = -A⁻¹ E Σ_EE (exact, dense);
 *  - the control-point pairs (i, j) with |i - j| < order (the spline's support), Σ_AA(i, j) = [A⁻¹]_ij - [Σ_AE (A⁻¹ E)ᵀ]_ij,
 *    from a selected inversion of the band (block band Cholesky of the equilibrated A, Takahashi recurrence), all on the device.
 *    Pairs farther apart are not computed: calico_covariance_get_block returns CALICO_UNIMPLEMENTED for them.
 * An unobserved control point (no residual reaches it) reads back as zeros, as a constant block. A pivot of the equilibrated
 * band below min_relative_pivot fails the whole compute with CALICO_FAILED_PRECONDITION. Spline orders up to 8 (beyond:
 * CALICO_UNIMPLEMENTED). With control_points = 0 nothing of this runs and the compute is the border's alone; on a problem
 * without a spline (no control points) the flag has nothing to compute and is ignored, and the trajectory readers return
 * CALICO_FAILED_PRECONDITION saying so. A border of any width works, none (every calibration block constant) included.
 * On a sharded handle every rank computes the same blocks from the all-reduced normal equations (no further exchange). The control
 * points' blocks are bit-identical from compute to compute; the border's Σ does not depend on control_points. */
/* Compute Σ (finalises the problem if needed). o == NULL: the defaults. A problem refused as rank deficient can be taken to
 * calico_observability_compute (below), which reports which directions of the border are undetermined. */
int32_t calico_covariance_compute(calico_problem* p, const calico_covariance_options* o);
/* Size of Σ (the border's tangent dimension), the number of structurally unobserved columns left out, and the minimum
 * relative pivot of the factorisation. CALICO_FAILED_PRECONDITION without a successful compute. */
int32_t calico_covariance_info(calico_problem* p, int32_t* dim, int32_t* n_unobserved, double* min_relative_pivot);
/* Σ as dim x dim row-major, border tangent order: the free, used non-control-point blocks in block-id order
 * (the tail of calico_num_effective_parameters' order). */
int32_t calico_covariance_get_dense(calico_problem* p, double* out);
/* The (block_a, block_b) block of Σ, row-major. tangent != 0: tangent space (GetCovarianceBlockInTangentSpace, 3 rows per
 * quaternion); tangent == 0: ambient (GetCovarianceBlock), a quaternion block lifted as P Σ Pᵀ with P the
 * EigenQuaternionManifold PlusJacobian at the current value. Control-point blocks (6 rows) after a compute with
 * control_points = 1: with any border block, and with control points less than the spline order apart; CALICO_UNIMPLEMENTED
 * for other control-point pairs and for every control-point block after a compute without it; CALICO_INVALID_ARGUMENT
 * for an unknown id, CALICO_FAILED_PRECONDITION without a successful compute. */
int32_t calico_covariance_get_block(calico_problem* p, int32_t block_a, int32_t block_b, int32_t tangent, double* out);
/* Covariance of the spline's 6-vector (what Interpolate converts to a pose) at each of n stamps, out = n x 36 (row-major
 * 6x6 each): Σ_v(t) = Σ_ij w_i(t) w_j(t) Σ_AA(s + i, s + j) over the order control points of t's segment s, w the spline's
 * weights at t. Symmetric. CALICO_INVALID_ARGUMENT for a stamp outside the valid knots (the rule of Interpolate: the last
 * valid knot belongs to the last segment), CALICO_FAILED_PRECONDITION without a successful compute with control_points = 1
 * or after a structural change. */
int32_t calico_covariance_trajectory(calico_problem* p, int64_t n, const double* stamps, double* out);
/* Number of control points and spline order of the trajectory's blocks, and the minimum relative pivot of the band's
 * factorisation. CALICO_FAILED_PRECONDITION as calico_covariance_trajectory. */
int32_t calico_covariance_trajectory_info(calico_problem* p, int32_t* n_cp, int32_t* order, double* min_relative_pivot_band);

/* ---- prediction covariance and leverage of the observations ------------ */
/* How well the fit determines what the model predicts for each registered observation, and how much each observation
 * carries the fit. For residual block i of a sensor (dimension d = 2 camera, 3 gyroscope / accelerometer), at the CURRENT
 * parameter values:
 *   J_i (d x n_eff): its Jacobian rows exactly as the LM loop and the covariance pass evaluate them -- sigma-weighted,
 *     quaternion blocks in the tangent, tangent order of calico_num_effective_parameters. apply_loss = 1 (default): the
 *     robust loss goes through the corrector as in the solve, so J_i are rows of the very J whose (JᵀJ)⁻¹ Σ is;
 *     apply_loss = 0: the Jacobian of the plain whitened residual (z − f(θ)) / sigma.
 *   P_i = J_i Σ J_iᵀ (d x d, symmetric, row-major), Σ the full covariance [control points | border] of the last successful
 *     calico_covariance_compute with control_points = 1 (structurally unobserved columns are zero in Σ, as there). A
 *     residual block touches the `order` control points of its segment and a few border blocks: exactly the part of Σ that
 *     compute produced. leverage_i = trace(P_i).
 *       apply_loss = 1: P_i is the i-th diagonal block of the hat matrix J (JᵀJ)⁻¹ Jᵀ: 0 <= P_i <= I, and the leverages of all
 *         blocks of all sensors that are in the fit add up to 6 n_cp + dim − n_unobserved (observed control points).
 *       apply_loss = 0: sigma² P_i is the covariance of the model's prediction for observation i in measurement units.
 * Every registered observation of the sensor is evaluated, observations tagged as outliers included (the residual of a
 * held-out point has variance I + P_i, of one in the fit I − P_i; the caller has the mask). An observation that does not
 * evaluate (the projection fails) gets valid = 0 and zeros. Order: insertion order, as calico_get_residuals.
 * J_i is taken at the current values and Σ at the values of its compute: a caller who moved the parameters (a solve, a
 * set_param_block) calls calico_covariance_compute again first. The call leaves the parameters, the LM state, the iteration
 * log, the last summary, the stored covariance and observability report and the phase timers alone. On a sharded handle it
 * evaluates all blocks on every rank without an exchange (every rank holds the same Σ); results are bit-identical from
 * call to call and between ranks. */
typedef struct calico_prediction_options {
  int32_t apply_loss;   /* default 1 */
  int32_t reserved[7];
} calico_prediction_options;
void calico_default_prediction_options(calico_prediction_options* o);
/* cov_out: n x d x d, leverage_out: n, valid: n (n = the sensor's registered observations); any of them may be NULL, not
 * all three (CALICO_INVALID_ARGUMENT). o == NULL: the defaults. CALICO_FAILED_PRECONDITION without a successful
 * calico_covariance_compute with control_points = 1, after a structural change, or on a problem without a spline;
 * CALICO_INVALID_ARGUMENT for an unknown sensor or apply_loss outside {0, 1}; CALICO_UNIMPLEMENTED for a layout whose
 * columns do not fit the kernel's staging area. */
int32_t calico_prediction_covariance(calico_problem* p, int32_t sensor, const calico_prediction_options* o, double* cov_out,
                                     double* leverage_out, uint8_t* valid);

/* ---- observability of the calibration ---------------------------------- */
/* Which directions of the dense border the data determine, and how well: the answer calico_covariance_compute cannot give
 * when it refuses a problem as rank deficient (it works on the well-posed ones too). Definition, at the current values,
 * with H = JᵀJ = [[A, E], [Eᵀ, C]] (A: control points, C: the dense border in the tangent order of
 * calico_num_effective_parameters; the Gauss-Newton matrix exactly as the covariance pass evaluates it: sigma-weighted,
 * robust loss through the corrector, quaternion tangent, no LM damping, no Jacobi scaling):
 *  - S = C - Eᵀ A⁻¹ E, the Schur complement onto the border (dim x dim): the information on the calibration that is left
 *    when the trajectory is free to follow.
 *  - Border columns whose C diagonal is exactly 0.0 (no residual depends on them) are left out, as in the covariance:
 *    n_unobserved of them, dim_kept = dim - n_unobserved.
 *  - S̃ = D⁻¹ S D⁻¹ on the kept columns, D = sqrt(diag C): the column norms of J, NOT diag S (a column the trajectory
 *    explains entirely has diag S ~ 0). Eigenvalues of S̃ lie in [0, dim_kept]; an eigenvalue is the share of a
 *    direction's information that neither the trajectory nor the other directions explain.
 *  - The report is S̃ = V Λ Vᵀ, eigenvalues ascending, each eigenvector's largest-magnitude entry positive (lowest index on
 *    a tie), computed on the device by a cyclic Jacobi method with a fixed order of operations: repeated computes, and the
 *    ranks of a sharded handle, hold bit-identical reports.
 *  - Direction i in TANGENT UNITS: δ_i = D⁻¹ v_i / |D⁻¹ v_i|, zero in the dropped columns. For a null direction S δ_i = 0:
 *    moving the calibration along δ_i (the trajectory following by -A⁻¹ E δ_i) leaves the cost unchanged to second order.
 *  - n_weak = number of eigenvalues below weak_threshold.
 * A rank-deficient border is NOT an error: the compute returns CALICO_OK and n_weak > 0. A itself must be invertible for S
 * to exist: a pivot of the trajectory's equilibrated block band (natural order), or of the root / separator rows of the
 * elimination, that is not positive or below min_relative_pivot makes the compute return CALICO_FAILED_PRECONDITION with a
 * message that names the trajectory as the deficient part (the covariance's border message does not) and both pivots.
 * Borders of up to 256 columns (beyond: CALICO_UNIMPLEMENTED with the two numbers); CALICO_INTERNAL if the eigensolver
 * does not converge in 30 sweeps.
 * Contracts as the covariance's: the result lives on the handle until the next calico_observability_compute or
 * calico_problem_destroy; a structural change (blocks, sensors, observations, shard) makes the readers return
 * CALICO_FAILED_PRECONDITION until the next compute, a change of values does not; the compute leaves the parameters, the LM
 * state, the iteration log, the last summary and a stored covariance alone (a solve after it is bit-identical to one
 * without it); on a sharded handle it takes the same exchange as an evaluation (every rank calls it) and every rank holds
 * the same report. */
typedef struct calico_observability_options {
  double weak_threshold;        /* eigenvalues of S̃ below this count as weak (>= 0) */
  double min_relative_pivot;    /* for the trajectory's band and the root rows (>= 0) */
  int32_t reserved[4];
} calico_observability_options;
/* Defaults. min_relative_pivot = 1e-12 (as calico_default_covariance_options). weak_threshold = 1e-10, inside the gap the test
 * scenes show (tests/test_gpu_observability.py prints the spectra): exact deficiencies -- OpenCV8 at zero distortion, VectorNav
 * IMUs with a free rotation, a free chart pose, configs[3] and configs[4] of BASELINE.json as they are -- come out of the device
 * at |λ| <= 7.3e-16 (the CPU reference built from the oracle: <= 5.8e-15), the smallest eigenvalue of a well-posed or merely weak
 * direction is 8.1e-7 (the free-chart-pose scene): four decades on either side. That scene's three directions near 1e-6 are
 * deliberately NOT counted by the default: at the start values they are weak, not null, and the spectrum shows them. */
void calico_default_observability_options(calico_observability_options* o);
/* Compute the report (finalises the problem if needed). o == NULL: the defaults. */
int32_t calico_observability_compute(calico_problem* p, const calico_observability_options* o);
/* dim (the border's tangent dimension), the structurally unobserved columns left out, the eigenvalues below weak_threshold,
 * the smallest and the largest eigenvalue, the Jacobi sweeps taken. Any output pointer may be NULL.
 * CALICO_FAILED_PRECONDITION without a successful compute. */
int32_t calico_observability_info(calico_problem* p, int32_t* dim, int32_t* n_unobserved, int32_t* n_weak, double* lambda_min,
                                  double* lambda_max, int32_t* sweeps);
/* The dim_kept = dim - n_unobserved eigenvalues of S̃, ascending. */
int32_t calico_observability_get_spectrum(calico_problem* p, double* eigenvalues /* dim_kept */);
/* Rows [first, first + count) of the ascending list; out = count x dim (border tangent order, zeros in dropped columns);
 * tangent_units = 0: v_i (orthonormal), 1: δ_i. CALICO_INVALID_ARGUMENT for a range outside [0, dim_kept]. */
int32_t calico_observability_get_directions(calico_problem* p, int32_t first, int32_t count, int32_t tangent_units, double* out);
/* The entries of direction `index` that belong to one parameter block (tangent size: 3 for a quaternion), and the block's
 * share Σ v_i[rows of block]² of the unit eigenvector (the shares of all blocks add up to 1). out or share may be NULL (not
 * both). A constant or unused block reads back zeros; CALICO_INVALID_ARGUMENT for an unknown id, a control point (the
 * trajectory is eliminated: not part of the report) or an index outside [0, dim_kept). */
int32_t calico_observability_get_block(calico_problem* p, int32_t index, int32_t block_id, int32_t tangent_units, double* out,
                                       double* share);
/* S̃ itself, dim x dim row-major, zeros in dropped rows / columns. */
int32_t calico_observability_get_matrix(calico_problem* p, double* out);

/* ---- camera model maps: unprojection, free points, projection uncertainty ---- */
/* The camera model over arbitrary pixels and points -- no residual blocks, no trajectory, no latency: what a user does
 * with a calibration once it is solved (rays for triangulation and PnP, rectification look-ups) and the map a person reads
 * to judge it (how uncertain the projection is across the image, corners included).
 *
 * calico_camera_unproject replaces sensors::CameraModel::UnprojectPixel (camera_models.h: Newton for OpenCv5/8 and
 * KannalaBrandt, closed forms for the rest) for n pixels at once, on the device. bearings_out[i] (n x 3) is the UNIT-NORM
 * point b with project(intrinsics, b) == pixels[i] under this library's projection (calico_project, the residuals). For six
 * models that is the usual bearing. For ExtendedUnified the projection the reference and this library evaluate is not scale
 * invariant (beta * |p_xy|, not its square), so "unit-norm point" is the definition; the reference's own closed form (which its
 * header calls rather imprecise) is not reproduced. DoubleSphere, FieldOfView, Unified: closed forms; OpenCv5/8: Newton on
 * the normalised point, at most 30 steps; KannalaBrandt, ExtendedUnified: Newton on the polar angle, at most 100 steps; stop
 * rule 1e-14 in normalised units. valid_out[i] = 0 and bearings_out[i] = 0 where Newton did not reach the stop rule, a closed
 * form's radicand is negative, the result is not finite, the projection rejects the point or does not return the pixel.
 * Needs no problem handle (like calico_fit_spline): allocates and frees its own device memory, n is processed in chunks.
 * CALICO_INVALID_ARGUMENT -- checked before the device is touched, message in calico_last_error(NULL), which is kept per
 * thread for the calls without a handle -- for an unknown model, n_intrinsics other than the model's count, n < 0, a NULL
 * pointer with n > 0; n == 0 is CALICO_OK and touches nothing. */
int32_t calico_camera_unproject(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n,
                                const double* pixels, double* bearings_out, uint8_t* valid_out);
/* The forward model for n free camera-frame points (n x 3): pixels_out n x 2, valid_out n (0 and zeros where the model
 * rejects the point, e.g. z <= 0 for the pinhole-type models), d_point_out n x 2 x 3 = d pixel / d point, d_intrinsics_out
 * n x 2 x n_intrinsics = d pixel / d intrinsics. The last three pointers may be NULL. It is the projection of the residuals
 * itself: ideal pixel -> calico_camera_unproject -> rotate -> this call is a rectification look-up table. Errors as above. */
int32_t calico_camera_project_points(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n,
                                     const double* points, double* pixels_out, uint8_t* valid_out, double* d_point_out,
                                     double* d_intrinsics_out);
/* calico_camera_unproject at the CURRENT intrinsics of a camera of the problem, read on the device from the handle's
 * parameter vector, on the handle's stream (ordered behind a solve). Bit-identical to calico_camera_unproject at the values
 * calico_get_param_block returns. CALICO_INVALID_ARGUMENT for an unknown sensor or one that is not a camera. */
int32_t calico_sensor_unproject(calico_problem* p, int32_t sensor, int64_t n, const double* pixels, double* bearings_out,
                                uint8_t* valid_out);
/* Projection uncertainty map: for each of n pixels the covariance of the pixel a fixed 3-D point projects to, under the
 * covariance of the camera's estimates: the pixel is unprojected at the current intrinsics, the ray scaled to `range`
 * metres, and S_pix = G S_tt G^T with G = d pixel / d theta there; cov_out is n x 3 = [s_uu, s_uv, s_vv], in pixels^2
 * (no a-posteriori variance factor, as the covariance).
 *   CALICO_FRAME_CAMERA: the point is fixed in the camera frame; theta = the intrinsics block, G = d pixel / d intrinsics
 *     (`range` only matters for ExtendedUnified, whose projection is not scale invariant).
 *   CALICO_FRAME_RIG: the point is fixed in the sensor-rig frame, p_c = R_rc^T (p_r - t_rc); theta = intrinsics, q_rc and
 *     t_rc with all cross-covariances, the quaternion in the EigenQuaternion tangent the covariance uses.
 * Constant blocks contribute nothing. Latency and the trajectory do NOT enter: the map is about the camera, not about
 * where the rig was. Needs a successful calico_covariance_compute on the handle (either value of control_points: only the
 * border is read); otherwise, and after a structural change, CALICO_FAILED_PRECONDITION. S_tt is taken at the values of
 * that compute, G at the current values. CALICO_INVALID_ARGUMENT for an unknown or non-camera sensor, frame outside {0, 1},
 * range not finite or <= 0, n < 0, a NULL pointer with n > 0. valid_out[i] = 0 with zeros as for the unprojection.
 * Leaves the parameters, the LM state, the iteration log and the stored covariance alone. */
#define CALICO_FRAME_CAMERA 0
#define CALICO_FRAME_RIG 1
int32_t calico_projection_uncertainty(calico_problem* p, int32_t sensor, int32_t frame, double range, int64_t n,
                                      const double* pixels, double* cov_out, uint8_t* valid_out);

/* ---- chart resection: per-frame camera poses at given intrinsics, for every camera model ---- */
/* Where the camera was when each image of a planar chart was taken: for each of n_frames frames -- frame f owns the pairs
 * [frame_offsets[f], frame_offsets[f + 1]) of pixels (N x 2) and points (N x 3, chart frame) -- the pose T_camera_chart,
 * p_camera = R(q) p_chart + t, that minimises  Sum rho(|pixel - project(intrinsics, R p + t)|^2)  in pixels, under this
 * library's own projection (calico_project, the residuals), on the device. It is the step between a detector's output and
 * calico_fit_spline, for all seven models and at KNOWN intrinsics (a previous calibration, a data sheet, a first pinhole pass);
 * calico_camera_calibrate (below) estimates the intrinsics of any model together with these poses, from a rough start such as
 * Zhang's closed form for the pinhole part (utils.InitializePinholeAndPoses, on the host) mapped by utils.InitialIntrinsics.
 *   start  q_init == t_init == NULL: the pixels are unprojected (calico_camera_unproject's map), the pairs with a valid unit
 *          bearing of z > 0.1 give the plane-to-normalised-image homography (Hartley normalisation, normal equations), which
 *          is split into a rotation (its nearest orthonormal matrix of determinant +1) and a translation with the chart in
 *          front. Needs the frame's points in their z = 0 plane (|z| <= 1e-9 x the extent of the frame's points) and at
 *          least 4 usable pairs: otherwise CALICO_RESECT_NO_START. Pixels without a valid unprojection are left out of the
 *          start only. Otherwise q_init (n_frames x 4; x, y, z, w; normalised here) and t_init (n_frames x 3) start every
 *          frame, and the points need not be planar.
 *   refine Levenberg-Marquardt on [delta_rot, t] with the left perturbation R <- exp([delta_rot]x) R, over every pair the model
 *          accepts at the current pose; rho = identity (huber_scale == 0) or Huber with huber_scale in pixels, weights rho',
 *          no second-order term. A candidate at which the model rejects a pair that is valid at the current pose is a rejected
 *          step; a candidate whose cost is within the cost's own rounding error of the current one is accepted. Stops after
 *          an accepted step with |delta_rot|_inf < step_tolerance and |delta_t|_inf < step_tolerance max(1, |t|) taken at a
 *          damping at or below its initial value (1e-4 of the diagonal: the step is the Gauss-Newton step to 1e-4) -- or a
 *          rejected step that small: the pose is kept --, and after max_iterations steps (CALICO_RESECT_NOT_CONVERGED: the
 *          last accepted pose).
 * Outputs per frame: q_out (n_frames x 4, unit, w >= 0), t_out (x 3), rms_out = sqrt(Sum |residual|^2 / n_used) in pixels (no
 * loss applied), n_used_out = the pairs the model accepts at the result, iterations_out = steps tried,
 * status_out, and cov_out (may be NULL) = n_frames x 6 x 6 (J^T W J)^-1 at the result, order [delta_rot, t], pixel^2 units (no
 * variance factor, as the covariance). CALICO_RESECT_TOO_FEW_POINTS: fewer than min_points pairs in the frame;
 * CALICO_RESECT_DEGENERATE: J^T W J not positive definite (at the largest damping, or undamped at the result), no pair valid at
 * the start, or a non-finite result. Every frame whose status is not OK or NOT_CONVERGED has q = (0, 0, 0, 1), t = 0, rms = 0,
 * n_used = 0 and a zero cov. Frames are independent: a frame's result depends neither on the other frames of the call nor on
 * its position, and repeated calls are bit-identical.
 * Needs no problem handle (like calico_camera_unproject): owns its device memory, processes the frames in chunks, message in
 * calico_last_error(NULL). CALICO_INVALID_ARGUMENT, before the device is touched: unknown model, n_intrinsics other than the
 * model's count, n_frames < 0, offsets that do not start at 0 or decrease, a NULL required pointer with n_frames > 0, exactly one
 * of q_init / t_init, step_tolerance not finite or <= 0, max_iterations < 1, huber_scale < 0 or not finite, min_points < 4.
 * n_frames == 0 is CALICO_OK and touches nothing. */
#define CALICO_RESECT_OK 0
#define CALICO_RESECT_TOO_FEW_POINTS 1
#define CALICO_RESECT_NO_START 2
#define CALICO_RESECT_NOT_CONVERGED 3
#define CALICO_RESECT_DEGENERATE 4
typedef struct {
  int32_t max_iterations;   /* 30 */
  double step_tolerance;    /* 1e-11 */
  double huber_scale;       /* 0 = no loss; pixels */
  int32_t min_points;       /* 4; values below 4 are an argument error */
} calico_resection_options;
void calico_default_resection_options(calico_resection_options* o);
int32_t calico_camera_resect(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n_frames,
                             const int64_t* frame_offsets /* n_frames + 1 */, const double* pixels /* N x 2 */,
                             const double* points /* N x 3, chart frame */, const double* q_init,
                             const double* t_init /* both NULL, or n_frames x 4 / x 3 */,
                             const calico_resection_options* o /* NULL = defaults */, double* q_out, double* t_out,
                             double* rms_out, int32_t* n_used_out, int32_t* iterations_out, uint8_t* status_out,
                             double* cov_out /* may be NULL */);

/* ---- intrinsic calibration: the intrinsics of any camera model jointly with the pose of every frame ---- */
/* Static calibration from the same ragged batch of (pixel, chart point) pairs calico_camera_resect takes: the K intrinsics of
 * `model` and the pose T_camera_chart of every usable frame that minimise  Sum rho(|pixel - project(k, R_f p + t_f)|^2)  over the
 * usable frames, under this library's own projection, on the device -- so that calico_solve starts at a minimum of its own
 * camera term. rho = identity or Huber (huber_scale in pixels, weights rho', no second-order term).
 *   unknowns  the pose of a frame moves as in the resection, R <- exp([delta_rot]x) R and t <- t + delta_t; the intrinsics move
 *          additively. free_mask (K bytes; NULL = all free): an entry with free_mask[i] == 0 is a constant, copied bit for bit to
 *          intrinsics_out, with zero rows and columns in intrinsics_cov_out.
 *   start  intrinsics_init, and per frame q_init / t_init (n_frames x 4 / x 3) for every frame with at least min_points pairs
 *          (the others: CALICO_RESECT_TOO_FEW_POINTS). With q_init == t_init == NULL every frame is resected at intrinsics_init
 *          (calico_camera_resect's kernel, the same huber_scale and min_points, its defaults otherwise); a frame whose resection
 *          is not CALICO_RESECT_OK is left out and carries the resection's status. Fewer than 3 usable frames:
 *          CALICO_CALIB_TOO_FEW_FRAMES.
 *   refine Levenberg-Marquardt on the arrowhead system (6 x 6 pose blocks A_f, couplings B_f, one K x K block C) with Marquardt
 *          damping lambda diag on the pose blocks and on C, lambda from 1e-4 within [1e-12, 1e12]: each frame eliminates its
 *          pose, the reduced K x K system gives the step of the intrinsics, the frames back-substitute. The decision is one for
 *          all frames. A candidate at which the model rejects a pair that is valid at the current point is rejected; one whose
 *          cost is within the cost's own rounding error of the current one is accepted. Step size
 *          s = max(|dk_i| / max(1, |k_i|), |delta_rot|_inf, |delta_t|_inf / max(1, |t|)) over all unknowns. Stops after an
 *          accepted step with s < step_tolerance taken at lambda <= 1e-4 -- or a rejected step that small: the point is kept --
 *          (CALICO_CALIB_OK), after max_iterations steps (CALICO_CALIB_NOT_CONVERGED: the last accepted point), and when the
 *          reduced system is not positive definite at the largest damping or the result is not finite
 *          (CALICO_CALIB_DEGENERATE). A frame whose damped 6 x 6 block is not positive definite drops out for good
 *          (CALICO_RESECT_NOT_POSITIVE_DEFINITE).
 * Outputs: intrinsics_out (K), per frame q_out (unit, w >= 0), t_out, rms_out (pixels, no loss), n_used_out, status_out
 * (CALICO_RESECT_*: OK for a frame that took part to the end); a frame that did not has q = (0, 0, 0, 1), t = 0, rms = 0,
 * n_used = 0. intrinsics_cov_out (K x K, may be NULL) = (C - Sum_f B_f^T A_f^-1 B_f)^-1, undamped, at the result, in pixel^2
 * units (no variance factor, as every covariance here). With CALICO_CALIB_TOO_FEW_FRAMES or CALICO_CALIB_DEGENERATE the outputs
 * are the inputs: intrinsics_init, the start poses of the usable frames, zero rms, n_used and covariance.
 * The call returns CALICO_OK whenever `summary` is meaningful; how the estimation ended is summary->status. Repeated calls
 * are bit-identical. Needs no problem handle: owns its device memory, message in calico_last_error(NULL).
 * CALICO_INVALID_ARGUMENT, before the device is touched: calico_camera_resect's list, a free_mask without a free entry, a NULL
 * intrinsics_out or summary, step_tolerance not finite or <= 0, max_iterations < 1, min_points < 4. n_frames == 0 is CALICO_OK
 * and touches nothing. */
#define CALICO_RESECT_NOT_POSITIVE_DEFINITE 5
#define CALICO_CALIB_OK 0
#define CALICO_CALIB_TOO_FEW_FRAMES 1
#define CALICO_CALIB_NOT_CONVERGED 2
#define CALICO_CALIB_DEGENERATE 3
typedef struct {
  int32_t max_iterations;   /* 50 */
  double step_tolerance;    /* 1e-10 */
  double huber_scale;       /* 0 = no loss; pixels */
  int32_t min_points;       /* 4; values below 4 are an argument error */
} calico_calibration_options;
typedef struct {
  int32_t status;           /* CALICO_CALIB_* */
  int32_t iterations;       /* steps tried */
  double initial_cost;      /* Sum rho at the start, over the usable frames */
  double final_cost;        /* == initial_cost, bit for bit, where no step was accepted (the start is returned) */
  double rms;               /* sqrt(Sum |residual|^2 / pairs_used) in pixels, no loss applied */
  int32_t frames_used;
  int64_t pairs_used;
  double lambda;            /* the damping at the end */
} calico_calibration_summary;
void calico_default_calibration_options(calico_calibration_options* o);
int32_t calico_camera_calibrate(int32_t device, int32_t model, const double* intrinsics_init, int32_t n_intrinsics,
                                const uint8_t* free_mask /* K, or NULL */, int64_t n_frames,
                                const int64_t* frame_offsets /* n_frames + 1 */, const double* pixels /* N x 2 */,
                                const double* points /* N x 3, chart frame */, const double* q_init,
                                const double* t_init /* both NULL, or n_frames x 4 / x 3 */,
                                const calico_calibration_options* o /* NULL = defaults */, double* intrinsics_out, double* q_out,
                                double* t_out, double* rms_out, int32_t* n_used_out, uint8_t* status_out,
                                double* intrinsics_cov_out /* K x K, may be NULL */, calico_calibration_summary* summary);

/* ---- rig calibration: camera-to-camera extrinsics and the pose of every rig frame from shared chart views ---- */
/* The second and every further camera of a rig: from the chart detections of n_cameras <= CALICO_RIG_MAX_CAMERAS cameras at
 * KNOWN intrinsics (each camera its own model: models[c], intrinsics[intrinsics_offsets[c] .. intrinsics_offsets[c + 1])), grouped
 * into rig frames -- instants at which the rig stood still relative to the chart --, the extrinsics T_rig_camera_c of every
 * camera but the reference camera and the pose T_rig_chart_f of every rig frame that minimise
 *   Sum_views rho(|pixel - project(k_c, R_c^T (R_f p_chart + t_f - t_c))|^2)
 * in pixels, on the device: a minimum of calico_solve's own camera term restricted to a static chart. T_rig_camera is the
 * library's extrinsics convention, p_rig = R_c p_camera + t_c. Quaternions are x, y, z, w; outputs are unit with w >= 0.
 *   views  a view is the ragged set of (pixel, chart point) pairs of one camera in one rig frame: view v of camera
 *          view_camera[v] in frame view_frame[v] owns the pairs [view_offsets[v], view_offsets[v + 1]) of pixels (N x 2) and
 *          points (N x 3, chart frame). Views may come in any order; a (camera, frame) pair may appear at most once. Every sum
 *          the call forms is ordered by (frame, then camera): the result is bit-identical under any permutation of the views,
 *          and repeated calls are bit-identical.
 *   gauge  the reference camera (options: reference_camera) is held at its start, bit for bit -- the identity when no start
 *          is given --; its status is CALICO_RIG_CAMERA_REFERENCE.
 *   start  (q_rig_camera_init == NULL) every view is resected (calico_camera_resect's kernel at its camera's model and
 *          intrinsics, the same huber_scale and min_points, its defaults otherwise); a view that is not CALICO_RESECT_OK is left
 *          out and keeps that status. Two cameras are connected when at least min_shared_frames frames hold an OK view of both;
 *          a breadth-first tree from the reference camera visits neighbours in index order; each tree edge gives
 *          T_a_b = T_a_chart,f T_b_chart,f^-1 per shared frame, whose rotations are averaged by the chordal mean (the dominant
 *          eigenvector of Sum q q^T after sign alignment, in frame order) and whose translations by the mean. A camera the
 *          tree does not reach is CALICO_RIG_CAMERA_UNCONNECTED: its views are left out, its output is its start or the
 *          identity. A frame starts at T_rig_camera_c T_camera_c_chart,f of its usable view of lowest camera index; a frame
 *          without a usable view is CALICO_RIG_FRAME_NO_VIEW. No camera other than the reference connected:
 *          CALICO_RIG_TOO_FEW_VIEWS, the outputs are the starts. The tree and the averages run on the host, the resections
 *          and everything after them on the device. With q_rig_camera_init / t_rig_camera_init (n_cameras x 4 / x 3, normalised
 *          here) the cameras start there; the same connection rule decides which cameras take part. With q_frame_init /
 *          t_frame_init (n_frames x 4 / x 3; only together with the camera start) nothing is resected: a view with at least
 *          min_points pairs is usable, the others are CALICO_RESECT_TOO_FEW_POINTS.
 *   refine Levenberg-Marquardt on the arrowhead system (6 x 6 frame blocks, one 6 x 6 coupling per view, the 6 C x 6 C block of
 *          the extrinsics) with R_f <- exp([d]x) R_f, t_f <- t_f + dt for a frame and R_c <- exp([d]x) R_c, t_c <- t_c + dt for
 *          a camera; rho = identity or Huber (huber_scale in pixels, weights rho', no second-order term); Marquardt damping
 *          lambda diag on the frame blocks and on the extrinsics block, lambda from 1e-4 within [1e-12, 1e12]; the decision is
 *          one for all frames and cameras; a candidate at which the model rejects a pair that is valid at the current point is
 *          rejected, one whose cost is within the cost's own rounding error of the current one is accepted. Step size
 *          s = max(|d_rot|_inf, |dt|_inf / max(1, |t|_2)) over frames and cameras. Stops after a step with s < step_tolerance
 *          taken at lambda <= 1e-4 (CALICO_RIG_OK), after max_iterations steps (CALICO_RIG_NOT_CONVERGED: the last accepted
 *          point), and when the reduced system is not positive definite at the largest damping or the result is not finite
 *          (CALICO_RIG_DEGENERATE: the outputs are the starts). A frame whose damped 6 x 6 block is not positive definite drops
 *          out for good, with its views (CALICO_RIG_FRAME_NOT_POSITIVE_DEFINITE).
 * Outputs: q_rig_camera_out / t_rig_camera_out (n_cameras x 4 / x 3) and camera_status_out (CALICO_RIG_CAMERA_*); q_frame_out /
 * t_frame_out (n_frames x 4 / x 3: T_rig_chart; the identity for a frame that took no part) and frame_status_out
 * (CALICO_RIG_FRAME_*); per view, in the caller's order, view_rms_out (pixels, no loss), view_n_used_out and view_status_out
 * (CALICO_RESECT_*; a view that took no part has rms = 0 and n_used = 0). extrinsics_cov_out (6 C x 6 C, may be NULL) is the
 * undamped inverse reduced system (C - Sum_f B_f^T A_f^-1 B_f)^-1 at the result, in camera order, 6 entries [d_rot, dt] per
 * camera, zero rows and columns for the reference and unconnected cameras, in pixel^2 units (no variance factor, as every
 * covariance here).
 * The call returns CALICO_OK whenever `summary` is meaningful; how the estimation ended is summary->status. Needs no problem
 * handle: owns its device memory, message in calico_last_error(NULL). CALICO_INVALID_ARGUMENT, before the device is touched:
 * n_cameras outside [1, 8], an unknown model, intrinsics offsets that do not match the models' counts, negative counts, a view's
 * camera or frame out of range, a duplicate (camera, frame) pair, offsets that do not start at 0 or decrease, a NULL required
 * pointer, exactly one of a q / t pair, a frame start without a camera start, reference_camera out of range,
 * min_shared_frames < 1, min_points < 4, step_tolerance not finite or <= 0, max_iterations < 1, huber_scale < 0 or not finite.
 * n_views == 0 is CALICO_OK with CALICO_RIG_TOO_FEW_VIEWS and touches no device. */
#define CALICO_RIG_MAX_CAMERAS 8
#define CALICO_RIG_OK 0
#define CALICO_RIG_TOO_FEW_VIEWS 1
#define CALICO_RIG_NOT_CONVERGED 2
#define CALICO_RIG_DEGENERATE 3
#define CALICO_RIG_CAMERA_OK 0
#define CALICO_RIG_CAMERA_REFERENCE 1
#define CALICO_RIG_CAMERA_UNCONNECTED 2
#define CALICO_RIG_FRAME_OK 0
#define CALICO_RIG_FRAME_NO_VIEW 1
#define CALICO_RIG_FRAME_NOT_POSITIVE_DEFINITE 2
typedef struct {
  int32_t max_iterations;     /* 50 */
  double step_tolerance;      /* 1e-10 */
  double huber_scale;         /* 0 = no loss; pixels */
  int32_t min_points;         /* 4; values below 4 are an argument error */
  int32_t min_shared_frames;  /* 3 */
  int32_t reference_camera;   /* 0 */
} calico_rig_options;
typedef struct {
  int32_t status;             /* CALICO_RIG_* */
  int32_t iterations;         /* steps tried */
  double initial_cost;        /* Sum rho at the start, over the views that take part */
  double final_cost;          /* == initial_cost, bit for bit, where no step was accepted (the start is returned) */
  double rms;                 /* sqrt(Sum |residual|^2 / pairs_used) in pixels, no loss applied */
  int32_t cameras_used;       /* the reference camera and the cameras connected to it */
  int32_t frames_used;
  int64_t views_used;
  int64_t pairs_used;
  double lambda;              /* the damping at the end */
} calico_rig_summary;
void calico_default_rig_options(calico_rig_options* o);
int32_t calico_rig_calibrate(int32_t device, int32_t n_cameras, const int32_t* models /* C */,
                             const int64_t* intrinsics_offsets /* C + 1 */, const double* intrinsics, int64_t n_frames,
                             int64_t n_views, const int32_t* view_camera, const int64_t* view_frame,
                             const int64_t* view_offsets /* n_views + 1 */, const double* pixels /* N x 2 */,
                             const double* points /* N x 3, chart frame */, const double* q_rig_camera_init,
                             const double* t_rig_camera_init /* both NULL, or C x 4 / C x 3 */, const double* q_frame_init,
                             const double* t_frame_init /* both NULL, or n_frames x 4 / x 3; only with the camera start */,
                             const calico_rig_options* o /* NULL = defaults */, double* q_rig_camera_out, double* t_rig_camera_out,
                             uint8_t* camera_status_out, double* q_frame_out, double* t_frame_out, uint8_t* frame_status_out,
                             double* view_rms_out, int32_t* view_n_used_out, uint8_t* view_status_out /* CALICO_RESECT_* */,
                             double* extrinsics_cov_out /* 6 C x 6 C, may be NULL */, calico_rig_summary* summary);

/* ---- camera-IMU alignment: rotation, gyroscope bias, latency and gravity from a fitted trajectory ---- */
/* The start calico_solve needs for the IMU side, from the trajectory of the camera side (calico_fit_spline over the poses of
 * calico_camera_resect / calico_camera_calibrate) and the raw IMU samples, on the device. The model is the optimiser's own
 * gyroscope term with the scale-and-bias model at scale 1:
 *   t = stamp - latency,  phi = -pose[0:3](t),  omega_rig = J(phi) phi',  prediction = -R(q_rig_gyro)^T omega_rig + bias,
 *   residual = (measured - prediction) / sigma_gyro,
 * so the result is a minimum of calico_solve's gyroscope cost over (rotation, bias, latency) at the given trajectory, and its
 * numbers are the gyroscope's extrinsic rotation, intrinsics [1, bias] and latency as they stand. As there (and in the
 * reference's Trajectory::GetEvaluationParams) the spline segment of a sample is the STAMP's; its polynomial is evaluated at t,
 * beyond its own knots where the latency carries t there.
 *   spline  order, n_knots, knots, basis as calico_fit_spline / calico_problem_set_spline take them; ctrl ((n_knots - order) x 6).
 *   samples the gyroscope samples that take part are those whose stamp and whose time stamp - latency lie inside the valid knots
 *          for EVERY latency of the grid  latency_init (or 0) + l lag_step, |l lag_step| <= max_lag (1e-9 relative slack on l)
 *          -- when stage A does not run (a start is given, or estimate_latency == 0): at latency_init (or 0) alone. The stamps are sorted, so they are one range
 *          [first_sample, first_sample + gyro_samples). Fewer than min_samples: CALICO_ALIGN_TOO_FEW_SAMPLES.
 *   A      (no start given, estimate_latency != 0) per latency of the grid the normalised, centred cross-correlation of
 *          |omega_rig(stamp - latency)| with |measured| over those samples; the maximum, refined by the parabola through its
 *          two neighbours, is the coarse latency. CALICO_ALIGN_NO_PEAK: the maximum lies on the first or the last latency of the
 *          grid, or a variance is below 1e-12 of its raw second moment (constant measurements, a trajectory at rest).
 *   B      (no start given) at the coarse latency (0 without A) Horn's quaternion of the cross-covariance of -omega_rig and
 *          measured (both centred when estimate_gyro_bias != 0); the bias is the mean residual. CALICO_ALIGN_DEGENERATE: the
 *          second eigenvalue of the (centred) scatter of omega_rig is below 1e-6 of the first -- the rig turned about one axis
 *          only and the rotation about it is undetermined; their ratio is summary->scatter_pivot.
 *   C      Levenberg-Marquardt on (rotation 3: R <- exp([d]x) R, bias 3, latency 1) with analytic Jacobians, Marquardt damping
 *          lambda diag from 1e-4 within [1e-12, 1e12]; what is not estimated is held. calico_camera_calibrate's rules: a
 *          candidate whose cost is within the cost's own rounding error of the current one is accepted, one with a residual
 *          that is not finite is rejected; step size s = max(|d_rot|_inf, |d_bias|_inf / max(1, |bias|_inf),
 *          |d_latency| / max(1, |latency|)); stops after a step with s < step_tolerance taken at lambda <= 1e-4
 *          (CALICO_ALIGN_OK), after max_iterations steps (CALICO_ALIGN_NOT_CONVERGED: the last accepted point), when the
 *          normal matrix is not positive definite at the largest damping or, undamped, at the result
 *          (CALICO_ALIGN_NOT_POSITIVE_DEFINITE), when the start is not finite (CALICO_ALIGN_DEGENERATE).
 *          With q_init and latency_init the loop starts there, at zero bias.
 *   D      (n_accel > 0, gyroscope part OK or NOT_CONVERGED) AccelerometerResidual's kinematics with q_rig_accel = q_rig_gyro,
 *          the gyroscope's latency, the lever arm t_rig_accel (NULL = 0) and scale 1 are linear in (gravity_world, accel_bias):
 *          one pass forms the 6 x 6 normal equations (3 x 3 with estimate_accel_bias == 0) over the samples whose stamp lies
 *          inside the valid knots, a Cholesky solves them and one step of iterative refinement follows. CALICO_ALIGN_NOT_POSITIVE_DEFINITE (a trajectory that does not
 *          turn cannot separate gravity from the bias) leaves gravity_world_out and accel_bias_out untouched, as every other
 *          status but OK does; when the gyroscope part did not get that far, accel_status is its status.
 * Outputs: q_rig_gyro_out (4: x y z w, unit, w >= 0), gyro_bias_out (3), latency_out -- the start (q_init normalised or the
 * identity, zero bias, latency_init or 0) with TOO_FEW_SAMPLES, NO_PEAK and DEGENERATE; cov_out (7 x 7, may be NULL): the
 * undamped inverse normal matrix (J^T J)^-1 of (rotation, bias, latency) at the result, zero rows and columns for what is not
 * estimated, all zero unless the status is OK or NOT_CONVERGED; curve_out (may be NULL): the first summary->n_lags entries
 * are the correlation curve when stage A ran, the others are never written.
 * The call returns CALICO_OK whenever `summary` is meaningful. Repeated calls are bit-identical: every sum has a fixed order.
 * Needs no problem handle: owns its device memory, message in calico_last_error(NULL).
 * CALICO_INVALID_ARGUMENT, before the device is touched: order outside [2, 8], n_knots < 2 order, a NULL knots, basis, ctrl,
 * output or summary, a negative count, NULL samples with a positive count (gravity_world_out and accel_bias_out may be NULL
 * with n_accel == 0), stamps that decrease, lag_step <= 0, max_lag < 0, more than CALICO_ALIGN_MAX_LAGS latencies in the grid, an option that
 * is not finite, step_tolerance <= 0, sigma_gyro <= 0, max_iterations < 1, min_samples < 3, q_init without latency_init or
 * the reverse, a q_init or latency_init that is not finite or a q_init of zero length. n_gyro == 0 is CALICO_OK with
 * CALICO_ALIGN_TOO_FEW_SAMPLES and touches no device. */
#define CALICO_ALIGN_OK 0
#define CALICO_ALIGN_TOO_FEW_SAMPLES 1
#define CALICO_ALIGN_NO_PEAK 2
#define CALICO_ALIGN_DEGENERATE 3
#define CALICO_ALIGN_NOT_CONVERGED 4
#define CALICO_ALIGN_NOT_POSITIVE_DEFINITE 5
#define CALICO_ALIGN_MAX_LAGS 4096      /* the most latencies a grid may hold: what curve_out must have room for */
typedef struct {
  double max_lag;               /* 0.1 s */
  double lag_step;              /* 1e-3 s */
  int32_t max_iterations;       /* 50 */
  double step_tolerance;        /* 1e-10 */
  int32_t estimate_latency;     /* 1 */
  int32_t estimate_gyro_bias;   /* 1 */
  int32_t estimate_accel_bias;  /* 1 */
  int32_t min_samples;          /* 16; values below 3 are an argument error */
  double sigma_gyro;            /* 1: the gyroscope's sigma in calico_problem_add_sensor (scales the covariance and the RMS) */
} calico_imu_alignment_options;
typedef struct {
  int32_t gyro_status;          /* CALICO_ALIGN_* */
  int32_t accel_status;
  int64_t gyro_samples;         /* samples that took part */
  int64_t accel_samples;
  int64_t first_sample;         /* index of the first gyroscope sample that took part */
  int32_t iterations;           /* steps tried */
  int32_t n_lags;               /* latencies of the grid (0: stage A did not run) */
  int32_t peak_index;           /* of the curve's maximum (-1: stage A did not run) */
  double coarse_latency;        /* the parabola's (the start's latency without stage A) */
  double peak_correlation;
  double gyro_rms;              /* sqrt(Sum |residual|^2 / (3 gyro_samples)), residuals divided by sigma_gyro */
  double accel_rms;             /* m/s^2 */
  double gravity_norm;
  double scatter_pivot;         /* stage B: second / first eigenvalue of the scatter of omega_rig (0: stage B did not run) */
  double initial_cost;          /* 1/2 Sum |residual|^2 at the start of stage C and at the result */
  double final_cost;
  double lambda;                /* the damping at the end */
} calico_imu_alignment_summary;
void calico_default_imu_alignment_options(calico_imu_alignment_options* o);
int32_t calico_imu_align(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis,
                         const double* ctrl /* (n_knots - order) x 6 */, int64_t n_gyro, const double* gyro_stamps,
                         const double* gyro /* n_gyro x 3 */, int64_t n_accel, const double* accel_stamps,
                         const double* accel /* n_accel x 3 */, const double* t_rig_accel /* 3, or NULL */,
                         const double* q_init /* 4 */, const double* latency_init /* 1; both NULL or both given */,
                         const calico_imu_alignment_options* o /* NULL = defaults */, double* q_rig_gyro_out, double* gyro_bias_out,
                         double* latency_out, double* gravity_world_out, double* accel_bias_out, double* cov_out /* 49, may be NULL */,
                         double* curve_out /* n_lags, may be NULL */, calico_imu_alignment_summary* summary);

/* ---- camera-to-trajectory alignment: extrinsics and latency of a camera that is not synchronised with the trajectory ---- */
/* The camera-side twin of calico_imu_align: the start calico_solve needs for a camera that shares no instant with the reference
 * camera (calico_rig_calibrate needs rig frames), from the trajectory fitted to the reference camera's poses and this camera's raw
 * chart detections at known intrinsics, on the device. The model is the optimiser's own camera term with the trajectory held:
 *   t = stamp - latency,  p = pose(t),  R_rw = R(quat(-p[0:3])),  t_wr = p[3:6],
 *   x_camera = R_rc^T (R_rw (R_wm x_chart + t_wm - t_wr) - t_rc),  residual = (pixel - project(intrinsics, x_camera)) / sigma_pixel,
 * with (q_rc, t_rc) = T_rig_camera and (q_wm, t_wm) = T_world_chart (q_world_chart, t_world_chart; NULL = identity / 0), so the
 * result is a minimum of calico_solve's camera cost over (extrinsics, latency) at the given trajectory. As there the spline
 * segment of a frame is the STAMP's; its polynomial is evaluated at t, beyond its own knots where the latency carries t there.
 *   spline  as calico_imu_align takes it.  frames  frame_offsets (n_frames + 1) cuts pixels (N x 2) and chart points (N x 3) into
 *          frames, as calico_camera_resect takes them; frame_stamps (n_frames) do not decrease.
 *   frames that take part: at least min_points pairs (the others: CALICO_RESECT_TOO_FEW_POINTS), and the stamp and the time
 *          stamp - latency inside the valid knots for EVERY latency of the grid  latency_init (or 0) + l lag_step,
 *          |l lag_step| <= max_lag (1e-9 relative slack on l) -- when stage A does not run (a start is given, or
 *          estimate_latency == 0): at latency_init (or 0) alone (the others: CALICO_CAMERA_ALIGN_FRAME_OUTSIDE). Fewer than
 *          min_frames: CALICO_ALIGN_TOO_FEW_SAMPLES.
 *   R      (no start given) every frame that takes part is resected at `intrinsics` (calico_camera_resect's kernel with the same
 *          huber_scale and min_points, its defaults otherwise); a frame whose resection is not CALICO_RESECT_OK drops out with
 *          the resection's status. Fewer than min_frames are left: CALICO_ALIGN_TOO_FEW_SAMPLES.
 *   A      (no start given, estimate_latency != 0) per latency tau of the grid and frame i the estimate
 *          E_i(tau) = T_rig_world(stamp_i - tau) T_world_chart T_chart_camera_i of T_rig_camera, and
 *          score(tau) = 4 (1 - lambda_max(Sum q q^T) / n) + (Sum |t|^2 / n - |mean t|^2) / d^2 -- the scatter of the rotations
 *          (rad^2) plus that of the translations under the angle the camera sees it, d^2 the mean of |t_camera_chart_i|^2.
 *          The minimum, refined by the parabola through its two neighbours, is the coarse latency. CALICO_ALIGN_NO_PEAK: the
 *          minimum lies on the first or the last latency of the grid, or the curve's range is below 1e-12 of its maximum (or of
 *          1 rad^2 where the maximum itself is rounding): a rig at rest.
 *   B      (no start given) at the coarse latency (0 without A) q_rig_camera is the principal eigenvector of Sum q q^T (w >= 0),
 *          t_rig_camera the mean translation (0 with estimate_translation == 0).
 *   C      Levenberg-Marquardt on (rotation 3: R <- exp([d]x) R, translation 3, latency 1) with analytic Jacobians -- the
 *          latency column through the first derivative of the stamp's segment --, Huber's loss on the pixel residual
 *          (huber_scale, pixels; 0 = none; weights rho', no second-order term), Marquardt damping lambda diag from 1e-4 within
 *          [1e-12, 1e12]; what is not estimated is held. calico_camera_calibrate's rules: the costs compared are those over
 *          the pairs valid at the current point, a candidate within the cost's own rounding error of the current one is accepted,
 *          one at which the model rejects a pair that is valid at the current point is rejected; step size
 *          s = max(|d_rot|_inf, |d_t|_inf / max(1, |t|_inf), |d_latency| / max(1, |latency|)); endings as calico_imu_align:
 *          CALICO_ALIGN_OK, _NOT_CONVERGED, _NOT_POSITIVE_DEFINITE, and _DEGENERATE for a start that is not finite or has no
 *          valid pair.
 * Outputs: q_rig_camera_out (4: x y z w, unit, w >= 0), t_rig_camera_out (3), latency_out -- the start (q_init normalised or the
 * identity, t_init or 0, latency_init or 0) with TOO_FEW_SAMPLES, NO_PEAK and DEGENERATE; per frame the RMS pixel residual (no
 * loss), the valid pairs and the status (CALICO_RESECT_*, or CALICO_CAMERA_ALIGN_FRAME_OUTSIDE; a frame that took no part, and
 * every frame unless the status is OK or NOT_CONVERGED, has rms = 0 and n_used = 0); cov_out (7 x 7, may be NULL): the undamped
 * (J^T W J)^-1 of (rotation, translation, latency) at the result, zero rows and columns for what is held, all zero unless the
 * status is OK or NOT_CONVERGED; curve_out (may be NULL): the first summary->n_lags entries are the score curve when stage A ran,
 * the others are never written.
 * The call returns CALICO_OK whenever `summary` is meaningful. Repeated calls are bit-identical: every sum has a fixed order.
 * Needs no problem handle: owns its device memory, message in calico_last_error(NULL).
 * CALICO_INVALID_ARGUMENT, before the device is touched: calico_imu_align's rules for the spline and the grid, calico_camera_resect's
 * for the model, the intrinsics and the frames, frame stamps that decrease or are not finite, a start given in part, not finite
 * or with a q_init of zero length, a q_world_chart that is not finite or of zero length, step_tolerance <= 0, sigma_pixel <= 0,
 * huber_scale < 0, max_iterations < 1, min_points < 4, min_frames < 3, a NULL output or summary. n_frames == 0 is CALICO_OK
 * with CALICO_ALIGN_TOO_FEW_SAMPLES and touches no device. */
#define CALICO_CAMERA_ALIGN_FRAME_OUTSIDE 6      /* frame status: the stamp, or stamp - latency for a latency of the grid, lies outside the valid knots */
typedef struct {
  double max_lag;               /* 0.1 s */
  double lag_step;              /* 1e-3 s */
  int32_t max_iterations;       /* 50 */
  double step_tolerance;        /* 1e-10 */
  int32_t estimate_latency;     /* 1 */
  int32_t estimate_translation; /* 1 */
  double huber_scale;           /* 0 = no loss; pixels */
  int32_t min_points;           /* 4 */
  int32_t min_frames;           /* 8; values below 3 are an argument error */
  double sigma_pixel;           /* 1: the camera's sigma in calico_problem_add_sensor (scales the costs and the covariance) */
} calico_camera_alignment_options;
typedef struct {
  int32_t status;               /* CALICO_ALIGN_* */
  int32_t iterations;           /* steps tried */
  int64_t frames_used;          /* frames that took part (after the resection) */
  int64_t pairs_used;           /* pairs valid at the result */
  int32_t n_lags;               /* latencies of the grid (0: stage A did not run) */
  int32_t peak_index;           /* of the curve's minimum (-1: stage A did not run) */
  double coarse_latency;        /* the parabola's (the start's latency without stage A) */
  double peak_score;            /* the curve's minimum */
  double rms;                   /* pixels, no loss: sqrt(Sum |pixel - projection|^2 / pairs_used) */
  double initial_cost;          /* 1/2 Sum rho(|pixel - projection|^2) / sigma_pixel^2 at the start of stage C and at the result */
  double final_cost;
  double lambda;                /* the damping at the end */
} calico_camera_alignment_summary;
void calico_default_camera_alignment_options(calico_camera_alignment_options* o);
int32_t calico_camera_align(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis,
                            const double* ctrl /* (n_knots - order) x 6 */, int32_t model, const double* intrinsics,
                            int32_t n_intrinsics, const double* q_world_chart /* 4 xyzw, NULL = identity */,
                            const double* t_world_chart /* 3, NULL = 0 */, int64_t n_frames,
                            const double* frame_stamps /* n_frames, non-decreasing */, const int64_t* frame_offsets /* n_frames + 1 */,
                            const double* pixels /* N x 2 */, const double* points /* N x 3, chart frame */,
                            const double* q_init /* 4 */, const double* t_init /* 3 */,
                            const double* latency_init /* 1; all three or none */,
                            const calico_camera_alignment_options* o /* NULL = defaults */, double* q_rig_camera_out,
                            double* t_rig_camera_out, double* latency_out, double* frame_rms_out, int32_t* frame_n_used_out,
                            uint8_t* frame_status_out /* CALICO_RESECT_* */, double* cov_out /* 7 x 7, may be NULL */,
                            double* curve_out /* n_lags, may be NULL */, calico_camera_alignment_summary* summary);

/* ---- accelerometer alignment: rotation, lever arm, bias, gravity and latency from a fitted trajectory ---- */
/* The third sibling of calico_imu_align and calico_camera_align: the start calico_solve needs for an accelerometer whose
 * mounting is not known from a data sheet, on the device. calico_imu_align's stage D takes the accelerometer's rotation and
 * latency from the gyroscope and its lever arm as given; this call estimates all of it. The model is the optimiser's own
 * accelerometer term with the scale-and-bias model at scale 1 and the trajectory held, exactly as stage D states it:
 *   t = stamp - latency,  phi = -pose[0:3](t),  omega = J(phi) phi',  alpha = Sum_i (H_i(phi) phi') phi'_i + J(phi) phi''
 *   (ExpSO3Hessian's closed form, which is not d omega / d t),
 *   prediction = R(q_rig_accel)^T (R(phi) (pose''[3:6](t) - gravity) + omega x (omega x t_rig_accel) - alpha x t_rig_accel) + bias,
 *   residual = (measured - prediction) / sigma_accel,
 * so the result is a minimum of calico_solve's accelerometer cost over (rotation, lever arm, bias, gravity, latency) at the given
 * trajectory. As there the spline segment of a sample is the STAMP's; its polynomial is evaluated at t, beyond its own knots
 * where the latency carries t there. The latency column is the derivative of that expression as it stands (through the closed
 * form of alpha and the pose's third derivative).
 *   spline  as calico_imu_align takes it.
 *   samples those whose stamp and whose time stamp - latency_init lie inside the valid knots; the stamps are sorted, so they are
 *          one range [first_sample, first_sample + samples), fixed for the whole call. Fewer than min_samples:
 *          CALICO_ALIGN_TOO_FEW_SAMPLES.
 *   start  q_init and latency_init are required (what calico_imu_align returned for the gyroscope of the same unit). t_init,
 *          bias_init and gravity_init are given all three or none; with none, all three groups must be estimated and
 *   L      the model being linear in (lever arm, bias, gravity) at fixed rotation and latency, one evaluation at zero forms the
 *          Gram matrix whose 9 x 9 block a Cholesky solves, and one step of iterative refinement follows from a second
 *          evaluation. summary->linear_status and linear_rms are the stage's; CALICO_ALIGN_NOT_POSITIVE_DEFINITE (or
 *          CALICO_ALIGN_DEGENERATE for a residual that is not finite) there ends the call with the start in the outputs.
 *   loop   Levenberg-Marquardt on (rotation 3: R <- exp([d]x) R, lever arm 3, bias 3, gravity 3, latency 1) with analytic
 *          Jacobians and calico_imu_align's rules: damping lambda diag from 1e-4 within [1e-12, 1e12], what is not estimated
 *          (estimate_* == 0) is held, a candidate within the cost's own rounding error is accepted, one with a residual that is
 *          not finite is rejected; step size s = the largest over the groups of |d|_inf / max(1, |value|_inf), the rotation
 *          unscaled; endings CALICO_ALIGN_OK, _NOT_CONVERGED (the last accepted point), _NOT_POSITIVE_DEFINITE (at the largest
 *          damping or, undamped, at the result), _DEGENERATE (a start that is not finite).
 * Outputs: q_rig_accel_out (4: x y z w, unit, w >= 0), t_rig_accel_out (3), bias_out (3), gravity_world_out (3), latency_out
 * -- the start (q_init normalised, latency_init, the three given or zero) with TOO_FEW_SAMPLES, DEGENERATE and a stage L that
 * is not OK; cov_out (13 x 13, may be NULL): the undamped (J^T J)^-1 in that order of the parameters at the result, zero rows
 * and columns for what is held, all zero unless the status is OK or NOT_CONVERGED. summary->rms and linear_rms are in m/s^2
 * (sqrt(Sum |measured - prediction|^2 / (3 samples))), the costs 1/2 Sum |residual|^2.
 * The call returns CALICO_OK whenever `summary` is meaningful. Repeated calls are bit-identical: every sum has a fixed order.
 * Needs no problem handle: owns its device memory, message in calico_last_error(NULL).
 * CALICO_INVALID_ARGUMENT, before the device is touched: calico_imu_align's rules for the spline, the count, the stamps and
 * the outputs; a NULL q_init or latency_init, one that is not finite, a q_init of zero length; t_init, bias_init and
 * gravity_init not all three or none, or not finite; none of them with one of their groups held; an option that is not
 * finite, step_tolerance <= 0, sigma_accel <= 0, max_iterations < 1, min_samples < 5. n == 0 is CALICO_OK with
 * CALICO_ALIGN_TOO_FEW_SAMPLES and touches no device.
 * Out of scope: the scale and the misalignment intrinsics of the other IMU models (the scale is 1), a constraint on the norm of
 * gravity (summary->gravity_norm reports it), and a search over the latency (the gyroscope's alignment supplies the start). */
typedef struct {
  int32_t max_iterations;       /* 50 */
  double step_tolerance;        /* 1e-10 */
  int32_t estimate_rotation;    /* 1 */
  int32_t estimate_lever_arm;   /* 1 */
  int32_t estimate_bias;        /* 1 */
  int32_t estimate_gravity;     /* 1 */
  int32_t estimate_latency;     /* 1 */
  int32_t min_samples;          /* 16; values below 5 are an argument error */
  double sigma_accel;           /* 1: the accelerometer's sigma in calico_problem_add_sensor (scales the covariance and the costs) */
} calico_accel_alignment_options;
typedef struct {
  int32_t status;               /* CALICO_ALIGN_* */
  int32_t linear_status;        /* stage L's; -1: it did not run */
  int64_t samples;              /* samples that took part */
  int64_t first_sample;         /* index of the first of them */
  int32_t iterations;           /* steps tried */
  double rms;                   /* m/s^2, at the result */
  double linear_rms;            /* m/s^2, at stage L's solution before its refinement step */
  double gravity_norm;
  double initial_cost;          /* 1/2 Sum |residual|^2 at the start of the loop and at the result */
  double final_cost;
  double lambda;                /* the damping at the end */
} calico_accel_alignment_summary;
void calico_default_accel_alignment_options(calico_accel_alignment_options* o);
int32_t calico_accel_align(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis,
                           const double* ctrl /* (n_knots - order) x 6 */, int64_t n, const double* stamps /* n, non-decreasing */,
                           const double* accel /* n x 3 */, const double* q_init /* 4 xyzw */, const double* latency_init /* 1 */,
                           const double* t_init /* 3 */, const double* bias_init /* 3 */,
                           const double* gravity_init /* 3; all three or none */,
                           const calico_accel_alignment_options* o /* NULL = defaults */, double* q_rig_accel_out,
                           double* t_rig_accel_out, double* bias_out, double* gravity_world_out, double* latency_out,
                           double* cov_out /* 13 x 13, may be NULL */, calico_accel_alignment_summary* summary);

/* ---- IMU noise from a static log: overlapping Allan variance and the IEEE-952 coefficients ---- */
/* The sigma that calico_problem_add_sensor takes for a gyroscope or an accelerometer, from a recording of the sensor at rest,
 * on the device. With dt = 1 / rate, theta_0 = 0, theta_k = dt Sum_{i<k} (y_i - mean(y)) and tau = m dt, per axis
 *   avar(tau) = 1 / (2 tau^2 (n - 2m)) Sum_{k=0}^{n-2m-1} (theta_{k+2m} - 2 theta_{k+m} + theta_k)^2,
 * the overlapping Allan variance (the mean is removed for conditioning only: the second difference does not see it), and
 *   rel_err(m) = 1 / sqrt(2 (n / m - 1)),
 * IEEE-952's relative error of its square root, the same for the three axes; rel_err^-2 is the fit's weight.
 *   grid     options->n_cluster_sizes == 0: m = the distinct values of floor(10^(i / points_per_decade) + 1/2), i = 0, 1, ...,
 *            while m <= max_tau_fraction n and 2m < n. Otherwise the caller's list.
 *   fit      per axis, in the variance domain, over the enabled terms (options->terms, CALICO_ALLAN_TERM_* bits):
 *              avar(tau) ~ 3 Q^2 / tau^2 + N^2 / tau + (2 ln 2 / pi) B^2 + K^2 tau / 3 + R^2 tau^2 / 2,
 *            the non-negative least squares of Sum_i w_i (1 - model_i / avar_i)^2, w_i = 2 (n / m_i - 1), over the squared
 *            coefficients. With at most five unknowns the NNLS is exact: every non-empty subset of the enabled terms is
 *            solved (Householder QR of the column-normalised design), and of the subsets whose coefficients are all >= 0 the
 *            least objective wins; ties (objectives within Sum_i w_i (64 eps)^2, the rounding of their residuals) go to the
 *            fewer terms, then to the lower mask. Cluster sizes whose variance is 0 or not finite are left out.
 *   summary  N_pooled = sqrt((N_x^2 + N_y^2 + N_z^2) / 3): the optimiser's sigma is one scalar per sensor; sigma_at_rate =
 *            N_pooled sqrt(sample_rate_hz). For a calibration recording at another rate, sigma is N_pooled sqrt(that rate).
 *            duration = n / sample_rate_hz; bias_drift_over_recording = max over the axes of K sqrt(duration): what the rate
 *            random walk moves the bias by over a recording of that length, to hold against the optimiser's constant bias.
 * Outputs: n_clusters_out (1), cluster_sizes_out, tau_out and rel_err_out (CALICO_ALLAN_MAX_CLUSTERS each), avar_out
 * (CALICO_ALLAN_MAX_CLUSTERS x 3; row j holds the three axes at cluster size j, n_clusters rows are written), noise_out (3).
 * The kernels (allan_kernels.hip) sum in FP64 in orders that n and m alone fix -- a three-phase prefix sum over blocks of
 * kAllanScanBlock = 2048 samples, then per (cluster size, axis) partial sums over chunks of kAllanTermChunk = 4096 terms -- so
 * repeated calls are bit-identical, the axes do not see each other, and an explicit list gives what the same grid gives.
 * Needs no problem handle: owns its device memory, message in calico_last_error(NULL).
 * CALICO_INVALID_ARGUMENT, before the device is touched: n < 3; a NULL samples or output; stamps that are not finite and
 * strictly increasing, or with a step outside [0.5, 1.5] / rate, rate = (n - 1) / (t_last - t_first) -- the message names
 * the first such sample ("a gap: split the log"); without stamps a sample_rate_hz that is not finite and > 0 (with stamps it
 * is not read); points_per_decade < 1, max_tau_fraction outside (0, 0.5], terms 0 or with unknown bits; a list that is NULL,
 * longer than CALICO_ALLAN_MAX_CLUSTERS, not strictly increasing, or with an m < 1 or 2m >= n. n > 2^31 - 1: CALICO_UNIMPLEMENTED.
 * Out of scope: non-uniform sampling and gap filling, the modified, Hadamard and total variances, confidence intervals
 * beyond rel_err, and a sigma per axis inside the optimiser. */
#define CALICO_ALLAN_MAX_CLUSTERS 256
#define CALICO_ALLAN_TERM_QUANTISATION 1          /* Q: 3 Q^2 / tau^2 */
#define CALICO_ALLAN_TERM_WHITE 2                 /* N: N^2 / tau (angle / velocity random walk) */
#define CALICO_ALLAN_TERM_BIAS_INSTABILITY 4      /* B: (2 ln 2 / pi) B^2 */
#define CALICO_ALLAN_TERM_RATE_RANDOM_WALK 8      /* K: K^2 tau / 3 */
#define CALICO_ALLAN_TERM_RAMP 16                 /* R: R^2 tau^2 / 2 */
#define CALICO_ALLAN_OK 0
#define CALICO_ALLAN_NO_WHITE_NOISE 1             /* N came back 0 */
#define CALICO_ALLAN_TOO_FEW_POINTS 2             /* fewer usable cluster sizes than enabled terms: the coefficients are 0 */
#define CALICO_ALLAN_NONFINITE 3                  /* the axis holds a NaN or Inf: its variances are NaN, the other axes are unaffected */
typedef struct {
  int32_t points_per_decade;      /* 10 */
  int32_t terms;                  /* WHITE | BIAS_INSTABILITY | RATE_RANDOM_WALK */
  double max_tau_fraction;        /* 0.1; at most 0.5 */
  int32_t n_cluster_sizes;        /* 0: the grid above */
  int32_t reserved;               /* 0 */
  const int64_t* cluster_sizes;   /* n_cluster_sizes of them, strictly increasing */
} calico_allan_options;
typedef struct {                  /* one axis */
  double Q, N, B, K, R;           /* 0 where the term is not enabled or not in terms_used */
  double objective;               /* Sum_i w_i (1 - model_i / avar_i)^2 at the result */
  int32_t terms_used;             /* the winning subset */
  int32_t n_points;               /* cluster sizes that took part */
  uint8_t status;                 /* CALICO_ALLAN_* */
  uint8_t reserved[7];
} calico_allan_noise;
typedef struct {
  int64_t n;
  double sample_rate_hz;          /* the rate used: from the stamps where they are given */
  double duration;                /* n / sample_rate_hz */
  double N_pooled;
  double sigma_at_rate;
  double bias_drift_over_recording;
} calico_allan_summary;
void calico_default_allan_options(calico_allan_options* o);
int32_t calico_imu_allan(int32_t device, int64_t n, const double* stamps /* n, or NULL */, double sample_rate_hz,
                         const double* samples /* n x 3, as calico_problem_add_imu_residuals takes them */,
                         const calico_allan_options* options /* NULL: defaults */,
                         int32_t* n_clusters_out, int64_t* cluster_sizes_out, double* tau_out,
                         double* avar_out /* n_clusters x 3 */, double* rel_err_out /* n_clusters */,
                         calico_allan_noise* noise_out /* 3, one per axis */, calico_allan_summary* summary);

/* ---- multi-GPU -------------------------------------------------------- */
/* Observations shard across ranks; the only exchange is the sum of the
 * packed normal-equation buffer (and of the candidate cost).  The host owns
 * the communicator: it registers a callback that must all-reduce (sum)
 * n doubles in place at device address buf, ordered on HIP stream `stream`
 * (e.g. torch.distributed.all_reduce over RCCL). Without a callback the
 * handle is single-rank. */
/* Native exchange (the production path): the handle owns an RCCL communicator and issues ncclAllReduce itself, on its
 * own stream, between the kernels of an iteration -- no host code in the loop. Rank 0 draws the 128-byte id with
 * calico_comm_get_unique_id and hands it to every rank by whatever means the application has (MPI, a file, a
 * torch.distributed broadcast); every rank then calls calico_comm_init_rccl, which also selects its shard (like
 * calico_problem_set_shard). One process per GPU; the communicator lives until the handle is destroyed.
 * LOAD ORDER: librccl is dlopen()ed by the first calico_comm_* call -- an RCCL the process already holds is adopted
 * (RTLD_NOLOAD by soname), otherwise a private copy is loaded (RTLD_LOCAL; CALICO_RCCL_LIB names a particular file).
 * An application that brings its own RCCL (PyTorch does) must therefore load it BEFORE the first calico_comm_* call:
 * two RCCL images in one process have ended in a double free at exit. calico_comm_init_rccl warns on stderr when it
 * finds two.
 * Replaces nothing in the reference (it is single-process); SURVEY.md 8(b),(e). */
#define CALICO_COMM_ID_BYTES 128
int32_t calico_comm_get_unique_id(uint8_t* id_out /* CALICO_COMM_ID_BYTES */);
int32_t calico_comm_init_rccl(calico_problem* p, const uint8_t* id, int32_t rank, int32_t world_size);
/* What the handle's exchange really spans: rank and rank count as the RCCL communicator reports them (ncclCommCount; the
 * shard set by calico_problem_set_shard when there is no communicator) and the number of residual blocks this rank
 * evaluates out of the problem's total (finalises the problem). Any output pointer may be NULL. */
int32_t calico_comm_info(calico_problem* p, int32_t* rank_out, int32_t* world_out, int64_t* local_blocks_out,
                         int64_t* total_blocks_out);
/* Host-side exchange (tests, exotic transports): a callback instead of the communicator. */
typedef int32_t (*calico_allreduce_fn)(void* ctx, void* buf, int64_t n,
                                       void* stream);
int32_t calico_problem_set_allreduce(calico_problem* p, calico_allreduce_fn fn,
                                     void* ctx);
/* Every rank receives the WHOLE problem through the add_* calls above and
 * keeps only its shard on the device: rank r of world_size evaluates the
 * residual blocks whose spline segment lies in its time window (contiguous
 * windows balanced by block count). All ranks solve the same reduced system
 * after the all-reduce, so their parameter estimates stay identical. */
int32_t calico_problem_set_shard(calico_problem* p, int32_t rank,
                                 int32_t world_size);
/* Use an externally owned HIP stream (hipStream_t) for all work of this
 * handle, e.g. torch's current stream so the callback above is ordered. */
int32_t calico_problem_set_stream(calico_problem* p, void* stream);

/* ---- timing ----------------------------------------------------------- */
/* HIP-event timings accumulated since the last calico_set_phase_timing call (over
 * as many solves as followed it), milliseconds summed over launches, and launch
 * counts, for the named phase (the call waits for the stream when brackets are
 * still pending: calico_solve itself returns as soon as the device reports the
 * end of the solve): 0 jacobian evaluation (residual +
 * Jacobian + JᵀJ partials), 1 reduction of partials, 2 linear solve,
 * 3 cost-only evaluation, 4 LM control + update, 5 calibration: the same
 * event bracket around a trivial (~2 us) kernel, i.e. the overhead contained
 * in every per-launch figure of the other phases, 6 the launch inside phase 2
 * that solves the reduced system (dense reduced solve + first back-substitution
 * where they share a launch; not recorded while phase 2's bracket is open). `phase | 0x100` restricts the
 * sums to working launches: kernels of iterations enqueued ahead return at once
 * when the solve has terminated, and brackets shorter than a quarter of the
 * phase's longest one are left out. */
int32_t calico_get_phase_time(calico_problem* p, int32_t phase, double* ms,
                              int64_t* launches);
/* Which phases are bracketed by HIP events (bits 0..6: bit i = phase i; default: none) and, in bits 8..15, a sampling
 * interval N: only every N-th launch of a phase is bracketed (0 or 1: every launch). An event pair costs about 6 us of
 * stream time, so a throughput measurement brackets a sample of the launches, not all of them. The call resets the
 * accumulated times. */
int32_t calico_set_phase_timing(calico_problem* p, int32_t mask);

#ifdef __cplusplus
}
#endif
#endif /* CALICO_HIP_H_ */
