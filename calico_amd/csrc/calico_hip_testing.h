/*
 * calico_hip_testing.h — test hooks of libcalico_hip.so. NOT part of the drop-in surface (include/calico_hip.h): nothing a
 * maintainer binds; tests/ reach these symbols through ctypes.
 */
#ifndef CALICO_HIP_TESTING_H_
#define CALICO_HIP_TESTING_H_

#include "../../include/calico_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The device's trust-region control stage (the accept / reject decision, the
 * radius schedule and the iteration log of ceres::TrustRegionMinimizer as restated in solve_kernels.hip) driven by a
 * given sequence of step qualities rho[i] (infinite[i] != 0: the candidate's cost could not be evaluated). Row i runs
 * the same control kernel a solve runs, seeded with x_cost = model_cost_change = 1 and candidate cost 1 - rho[i];
 * radius, decrease factor and counters carry over. Out: radius after the row, accepted flag, and the cost column the
 * row shows. tests/test_ceres_log.py replays the iteration table the reference ships
 * (demos/imu_camera_calibration.ipynb) through it. */
int32_t calico_debug_lm_control_replay(int32_t device, int32_t n, const double* rho, const int32_t* infinite,
                                       const calico_solver_options* options, double* radius_out, int32_t* accepted_out,
                                       double* cost_column_out);

/* What calico_problem_finalize decided for the handle's structure (finalizes the handle if it has not been yet), so
 * that a test can assert WHICH evaluation route it is comparing with the oracle. out[0..n) (n <= 28) receives:
 *   [0] fuse_expand (1: eval_cells_kernel -- cell workgroups; 0: eval_jacobian_kernel + expand_cells_kernel + row cells),
 *   [1] camera frames on the frame path, [2] work items of the generic / IMU path, [3] cells,
 *   [4] most frames in one camera cell, [5] most work items in one (layout, segment) of the item path,
 *   [6] 1: tree solver, 0: sequential banded solver, [7] m (tangent size of the calibration blocks). */
int32_t calico_debug_plan_info(calico_problem* problem, int32_t* out, int32_t n);
/* (out[8], n = 9: 1 if every control point is observed.)
 * What a linear solve of the plan does (n up to 28; the solve's switches -- SolveSwitches, problem_host.hpp -- as set at the call):
 *   [9] superblocks N of the tree solver (0: banded solver), [10] level 0's chain length q, [11] levels, [12] 1: a root exists,
 *   [13] 1: the Schur complement rides in the last level's launch, [14] top separators back-substituted in the level below,
 *   [15] 1: the dense solve is fused with the first back-substitution,
 *   [16] reduced-solve route (0: 16-column panel kernel, 1: in-LDS block solve, 2: blocked panels, 3: reduced_solve_kernel),
 *   [17] 1: reduced_solve_kernel works in LDS (0: in its global workspace), [18] K-slices of the Schur complement,
 *   [19] width of the reduced system a.m (calibration + root or separator rows), [20] sep_n (separator control points of the
 *   banded solver's split),
 *   [21] 1: elimination by blocks (0: the panel factorisation), [22] 1: level 0's chains with the rolling chief,
 *   [23] the dense reduced solve's mode (0: panel form, 1: blocks with barriers, 2: rolling owners),
 *   [24] 1: the fused launch's nodes in affine form (PRE), [25] 1: node descriptors in the launch arguments,
 *   [26], [27] (QM, MODE) of the table entry of the first back-substitution behind the reduced solve (dense_back_kernel
 *   where [15] is 1, else bcr_back_kernel; 0, 0: banded solver). */

/* The last linear solve of the last calico_solve: step delta (what the candidate update applied to the parameters), the
 * damping d added to the diagonal of J^T J, and the Jacobi scale in use. n: calico_num_effective_parameters (calico_evaluate's
 * column order) or 6 n_cp + m (every control point's rows, observed or not, then the calibration blocks'). Any output may
 * be NULL. Synchronises the handle's stream. CALICO_FAILED_PRECONDITION if no linear solve has run since the plan or the
 * parameters last changed. The radius the damping was formed with is the one the log row before the step's shows. */
int32_t calico_debug_last_step(calico_problem* problem, int32_t n, double* step, double* damping, double* scale);

/* Host only (no device needed): the 48 words of the rolling chief's per-lane offset table (bcr_kernels.hip, g_roll_tab) for a spline
 * order 1..6 and a lane 0..63 -- byte offsets of the lane's tile entries in the band's storage and which of them exist. */
int32_t calico_debug_roll_table(int32_t spline_order, int32_t lane, uint32_t* out48);

/* What the last calico_observability_compute did. out[0..n) (n <= 6) receives: [0] 1: the eigensolver's matrices lived in
 * LDS, 0: in the global workspace, [1] kept columns, [2] rows of the compact reduced system (root / separator rows + kept
 * columns), [3] rotations applied, [4] minimum relative pivot of the trajectory's band, [5] of the root rows.
 * CALICO_FAILED_PRECONDITION without a successful compute. */
int32_t calico_debug_observability_info(calico_problem* problem, double* out, int32_t n);

/* hipFuncSetAttribute calls the library's registry of dynamic-LDS limits has made in this process (raise_lds_limit, plan.cpp):
 * grows only when a handle or an analysis needs more than its device already allows some kernel. */
int64_t calico_debug_lds_attribute_calls(void);

/* calico_camera_unproject with the host-side chunk -- pixels uploaded, unprojected and downloaded per pass -- given by the
 * caller (chunk >= 1) instead of the library's default, so that a test reaches the chunk boundary with a few hundred pixels. */
int32_t calico_debug_camera_unproject_chunked(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics, int64_t n,
                                              const double* pixels, double* bearings_out, uint8_t* valid_out, int64_t chunk);

/* One panel product of the block elimination (block_elim.hpp) on one wave: w, x, out hold one double per lane (64). x: register u
 * of a tile -- lane (l16 = lane & 15, lk = lane >> 4) = entry (row l16, column lk) of a 16x4 tile; w: entry (l16 & 3, lk) of a 4x4
 * factor W in every lane; out: lane (l16, lk) = (x Wᵀ)(l16, lk). form 0: register 0 of the 16x16x4 product, form 1: CAL_PANEL (the
 * 4x4x4 form the kernels use). */
int32_t calico_debug_panel_product(int32_t device, int32_t form, const double* w, const double* x, double* out);

/* One 32x32 block eliminated by the header's own code in a workgroup of its own: elim_chief<1> on wave 0, elim_follow with the
 * identity tiles on wave 1 and with the n_row_tiles (1..3) loaded tiles of X on wave 2. D: [32][32] symmetric positive definite
 * (the lower triangle is read), X: [16 n_row_tiles][32]; L_out: the Cholesky factor (zeros above the diagonal), Z_out = X L⁻ᵀ,
 * Minv_out = L⁻ᵀ, all row-major. A bad pivot is not patched: NaN from its column on, and the call returns CALICO_OK. */
int32_t calico_debug_block_elim(int32_t device, int32_t n_row_tiles, const double* D, const double* X, double* L_out, double* Z_out,
                                double* Minv_out);

/* calico_camera_resect with the host-side chunk -- the most pairs uploaded, resected and downloaded per pass; a frame is never
 * split, one larger than the chunk travels alone -- given by the caller (chunk_pairs >= 1) instead of the library's default. */
int32_t calico_debug_camera_resect_chunked(int32_t device, int32_t model, const double* intrinsics, int32_t n_intrinsics,
                                           int64_t n_frames, const int64_t* frame_offsets, const double* pixels, const double* points,
                                           const double* q_init, const double* t_init, const calico_resection_options* o,
                                           double* q_out, double* t_out, double* rms_out, int32_t* n_used_out, int32_t* iterations_out,
                                           uint8_t* status_out, double* cov_out, int64_t chunk_pairs);

#ifdef __cplusplus
}
#endif
#endif /* CALICO_HIP_TESTING_H_ */
