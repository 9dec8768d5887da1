// kernels.hpp — host interfaces of the kernels: every launch_*, configure_* and size query a .hip file defines, declared once.
// Included by the host translation units that call them and by the .hip file that defines each: callers and definitions are
// compiled against the same declarations (and the same default arguments).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../../include/calico_hip.h"
#include "problem_dev.hpp"

namespace cal {

// ---- launch contract ---------------------------------------------------------
// A kernel family whose instantiation is picked from sizes (bcr_back_kernel, dense_back_kernel, band_backsolve_kernel) keeps
// ONE variant table next to its kernels ({template parameters, function}): its configure_* walks the table, its launch_* picks
// the entry through the family's selection function, so a variant that is launched is one that is configured, and a combination
// without an entry is an assert. The dynamic-LDS limits live in one registry (plan.cpp): `device` allows `fn` at least `bytes` afterwards.
// Limits are only ever raised (handles of different shapes share a device), hipFuncSetAttribute is called only when `bytes`
// exceeds what the registry has set for `fn` there; `device` is the calling thread's current device.
hipError_t raise_lds_limit(int device, const void* fn, size_t bytes);
template <class... A>
hipError_t raise_lds_limit(int device, void (*kernel)(A...), size_t bytes) {
  return raise_lds_limit(device, reinterpret_cast<const void*>(kernel), bytes);
}
hipError_t ensure_roll_table(int device);     // upload_roll_table() once per device (the same per-device record)
long long lds_attribute_calls();              // hipFuncSetAttribute calls of the registry in this process (test hook)

// ---- kernels (eval_kernels.hip / solve_kernels.hip) -------------------------
void launch_eval(const EvalArgs& a, bool jac, hipStream_t stream);
void launch_eval_jacobian(const EvalArgs& a, hipStream_t stream);
void launch_expand_cells(const EvalArgs& a, hipStream_t stream);
void launch_residual_heatmap(const double* res, const uint8_t* valid, const uint8_t* active, const double* px, const double* py,
                             int begin, int end, int width, int height, int num_rows, int num_cols, double* rmse, long long* count,
                             hipStream_t s);
void launch_inlier_mask(const double* res, uint8_t* valid_then_mask, const uint8_t* active, int begin, int end, int dim, double threshold,
                        hipStream_t s);
void launch_mark_outliers(const double* res, const uint8_t* valid, uint8_t* active, int begin, int end, int dim,
                          double threshold, int* n_marked, hipStream_t s);
hipError_t configure_eval_kernels(int device, size_t max_lds_bytes);
hipError_t configure_prediction_kernels(int device);
hipError_t launch_prediction(const PredArgs& pa, size_t lds_bytes, hipStream_t stream);

void launch_gather(double* R, const double* src, const int* out_idx_thin, const int64_t* ptr_thin, const int* idx_thin,
                   int n_thin, int n_thin8, int n_thin4, int thin_per_lane, const int* out_idx_fat, const int64_t* ptr_fat, const int* idx_fat, int n_fat,
                   const double* cost_src, int n_cost, const LmState* st, int need_flag, size_t other_stride, hipStream_t s, const ControlTail* tail = nullptr);
void launch_gather_lists(const GatherStruct& gs, int n_out, int* cnt, int* out_idx, int64_t* ptr, int* idx, int zero_slot, long long* scratch,
                         hipStream_t s);
size_t gather_fixed_entries(int n_thin, int n_thin8, int n_thin4, int thin_per_lane);
void launch_gather_pack_fixed(const int64_t* ptr, const int* idx, int n_thin, int n_thin8, int n_thin4, int thin_per_lane, int zero_slot, int* out,
                              hipStream_t s);
void launch_post_eval(const SolveArgs& a, const double* x, const BlockDev* blocks, int n_blocks, const LmOptionsDev& o,
                      IterLog* log, int log_cap, int first, int jacobi, hipStream_t s);
size_t band_cholesky_lds_bytes(const SolveArgs& a);
size_t reduced_solve_lds_bytes(const SolveArgs& a);
size_t frame_lds_doubles(int Ps, int P1e, int n1);
size_t band_backsolve_lds_bytes(const SolveArgs& a);
hipError_t configure_solve_kernels(int device, size_t band_lds, size_t reduced_lds, size_t back_lds);
void launch_solve(const SolveArgs& a, const LmOptionsDev& o, const double* x, double* x_cand, const BlockDev* blocks,
                  int n_blocks, bool dense_in_lds, hipStream_t s, bool with_post_eval, IterLog* log, int log_cap, int jacobi, int dense_mode);
void launch_cost_reduce(const double* item_cost, int n_items, double* R2, const LmState* st, hipStream_t s);
void launch_control(LmState* st, const LmOptionsDev& o, double* R2, double* x, const double* x_cand, int n_amb,
                    IterLog* log, int log_cap, const double* item_cost, int n_items, const double* Rbase, size_t r_stride,
                    hipStream_t s, bool commit_by_copy = false);
void launch_init_state(LmState* st, double radius, double x_norm, hipStream_t s, const double* upd_ext = nullptr, int upd_ext_n = 0);
void launch_begin_solve(LmState* st, double radius, double x_norm, const double* upd_ext, int upd_ext_n, const ResultSink& sink, double* x,
                        double* x_cand, const double* h_x, int n_amb, hipStream_t s);
void launch_publish_results(const LmState* st, const IterLog* log, int log_rows, const double* x, int n_amb, LmState* h_state,
                            IterLog* h_log, double* h_x, hipStream_t s);
void launch_seed_x(double* x, const double* h_x, int n_amb, hipStream_t s);
void launch_debug_control_replay(LmState* st, const LmOptionsDev& o, const double* rho, const int* infinite, int n, double* R2,
                                 double* radius_out, int* accepted_out, double* cost_out, IterLog* log, int log_cap, hipStream_t s);
size_t bcr_level_lds_bytes();
size_t bcr_back_lds_bytes(int q_max, int m1p);
hipError_t configure_bcr_kernels(int device, int q_max, int m1p);
hipError_t upload_roll_table();                            // (ensure_roll_table calls it, under the registry's lock)
void roll_table_row(int k, int lane, unsigned* out);      // (host only: test hook)
hipError_t configure_dense_block_solve(int device);
hipError_t configure_reduced_block_step(int device);
size_t dense_block_solve_lds_bytes();
void launch_bcr_level(const SolveArgs& a, const BcrArgs& b, int node0, int n_nodes, int level, int keep0, int n_keep, const LmOptionsDev& o,
                      const double* x, const BlockDev* blocks, int n_blocks, int with_post_eval, IterLog* log, int log_cap, int jacobi,
                      hipStream_t s, int schur_ks, int* fan_word, const BcrInlineNodes& inl, bool elim, bool roll);
// test hooks (calico_hip_testing.h): one panel product of block_elim.hpp (form 0: register 0 of the 16x16x4 product, 1: CAL_PANEL), and
// one 32x32 block eliminated by its chief and followers in a workgroup of their own (n_row_tiles <= debug_block_elim_max_tiles())
hipError_t launch_debug_panel_product(int form, const double* w, const double* x, double* out, hipStream_t s);
int debug_block_elim_max_tiles();
hipError_t launch_debug_block_elim(int n_row_tiles, const double* D, const double* X, double* L, double* Z, double* Minv, hipStream_t s);
void launch_bcr_schur(const SolveArgs& a, const BcrArgs& b, int ks, const LmOptionsDev& o, hipStream_t s);
void launch_bcr_back(const SolveArgs& a, const BcrArgs& b, int node0, int n_nodes, bool top, bool extras, bool border_rows, int q_max,
                     const double* x, double* x_cand, const BlockDev* blocks, int n_blocks, const BcrTopSeps& ts, hipStream_t s);

void launch_reduced_solve(const SolveArgs& a, bool reduced_in_lds, int ks, int dense_mode, hipStream_t s);
int reduced_solve_route(const SolveArgs& a);
// shape rules of the tree solver's routes (pure functions of their arguments; the switches are linear_route's, solve.cpp)
bool dense_back_fusable(const SolveArgs& a, int ks, int q_max, bool border_rows);
bool dense_back_pre_fits(const SolveArgs& a);
bool dense_back_pre_pays(const SolveArgs& a);
bool level0_roll_fits(const SolveArgs& a);
int chain_variant(int q_max);      // QM of the back-substitution kernels' table entry for chains of up to q_max
bool dense_back_fits(int q_max, int m1p);
hipError_t configure_dense_back(int device, int q_max, int m1p);
void launch_dense_back(const SolveArgs& a, const BcrArgs& b, int ks, int node0, int n_nodes, int q_max, const double* x, double* x_cand,
                       const BlockDev* blocks, int n_blocks, const BcrTopSeps& ts, int* word, int seq, hipStream_t s, bool pre, int dense_mode);
int reduced_schur_slices(const SolveArgs& a);
void launch_band_reduction(const SolveArgs& a, const LmOptionsDev& o, const double* x, const BlockDev* blocks, int n_blocks, hipStream_t s,
                           bool with_post_eval, IterLog* log, int log_cap, int jacobi);
int covariance_max_dim();
int covariance_ld(int n);
bool covariance_in_lds(int n);
void launch_covariance(const double* Spart, int ks, int m, int mc, const double* Cdiag, const LmState* st, double* work, double* out,
                       double* info, hipStream_t s);
hipError_t configure_covariance_kernel(int device);
int cp_covariance_max_order();
void launch_cp_covariance_band(const CpCovArgs& a, hipStream_t s);
void launch_cp_covariance_finish(const CpCovArgs& a, hipStream_t s);
void launch_cp_band_factor(const CpCovArgs& a, hipStream_t s);
int observability_max_border();
int observability_max_dim();
bool observability_in_lds(int m, int mc);
size_t observability_work_doubles(int m, int mc);
void launch_observability(const double* Spart, int ks, int m, int mc, const double* Cdiag, const LmState* st, double* work, double* lam,
                          double* vec, double* mat, double* d, double* info, hipStream_t s);
hipError_t configure_observability_kernel(int device);
void launch_cp_stamps(int n, int k, const double* stamps, const int* seg, const double* knots, const double* basis, const double* band,
                      double* out, hipStream_t s);

// ---- spline fit (fit_kernels.hip; device pointers: seg_ptr is the CSR of the sorted samples over the segments) ----------------
struct FitArgs {
  int n, k, n_ctrl, n_seg;
  const double* stamps; const int* seg; const int* seg_ptr; const double* knots; const double* basis; const double* data;
  double* W; double* band; double* rhs; double* ctrl; int* status;
};
size_t fit_solve_lds_bytes(int n_ctrl, int k);      // the solve works in LDS: the caller refuses what does not fit
hipError_t launch_fit_spline(int device, const FitArgs& a, hipStream_t s);
// The smoothing fit: two channel groups (0: axis-angle, 1: position), each with its own weights column, normal matrix and
// lambda grid; P is the roughness penalty's band (shared). band [2][n_ctrl][k], rhs [2][n_ctrl][3], ctrl_all [n_lambda][n_ctrl][6],
// rows [2][n_lambda] (the layout of calico_spline_fit_row). weights: [n][2] or null (all 1).
constexpr int kFitMaxLambdas = 32;
struct FitSmoothRow { int status, replaced_pivots; double lambda, rss, penalty, rms; };
struct FitSmoothArgs {
  int n, k, n_ctrl, n_seg, derivative, relative, n_lambda, n_used_rot, n_used_pos;
  double lambda_rot[kFitMaxLambdas], lambda_pos[kFitMaxLambdas];
  const double* stamps; const int* seg; const int* seg_ptr; const double* knots; const double* basis; const double* data; const double* weights;
  double* W; double* P; double* band; double* rhs; double* ctrl_all; FitSmoothRow* rows;
};
size_t fit_solve_smooth_lds_bytes(int n_ctrl, int k);      // [band | 3 rhs] of one group
hipError_t launch_fit_spline_smooth(int device, const FitSmoothArgs& a, hipStream_t s);
void launch_fit_smooth_prepare(const FitSmoothArgs& a, hipStream_t s);      // its launches before the solve: W, P, [band | 3 rhs]
// The cross-validated fit (fit_cv_kernels.hip): the smoothing fit's grid, then per (group, lambda) the band of Z = A^-1 by selected
// inversion of the factor in LDS, edf = sum Z o N, the leverages h_j and the PRESS sum over the samples, and the choice on the
// device. zband [2][n_lambda][n_ctrl][k] (the band's layout); edf [2][n_lambda] (NaN: the row is not eligible); partial
// [2][n_lambda][n_blocks][2]: per block of 256 samples the PRESS terms' sum and the largest h; cv_rows [2][n_lambda] (the layout of
// calico_spline_cv_row); leverage, loo [n][2] at each group's chosen lambda.
struct FitCvRow { double edf, gcv, press, max_leverage; };
struct FitCvSummary { int status[2], chosen[2]; double edf[2], score[2]; };
struct FitCvArgs {
  int criterion, n_blocks;
  double* zband; double* edf; double* partial; FitCvRow* cv_rows; FitCvSummary* summary; double* leverage; double* loo;
};
hipError_t launch_fit_spline_cv(int device, const FitSmoothArgs& a, const FitCvArgs& c, hipStream_t s);
// The robust fit (fit_robust_kernels.hip): iteratively reweighted least squares around the smoothing fit with n_lambda 1, one loop
// per group, controlled on the device. state [2]: done_iter is the control word (0: running; 1 + the iteration that finished the
// group), read first by every kernel of a later iteration. e, u, wu [n][2]: residual norms, robust weights (uploaded as 1, 0 where
// the prior weight is 0) and prior x robust weights; hist [2][8][256]: the digit counts of the selection.
struct FitRobustState { int done_iter, status, iterations, replaced_pivots, n_downweighted, n_rejected; double lambda, scale, median, last_step, rss; };
struct FitRobustArgs {
  int loss, max_iterations, rank[2];      // rank: (m - 1) / 2 of the m samples of weight > 0
  double tuning[2], fixed_scale[2], min_scale[2], step_tolerance;
  double* e; double* u; double* wu; int* hist; FitRobustState* state;
};
hipError_t launch_fit_spline_robust(int device, const FitSmoothArgs& a, const FitRobustArgs& r, hipStream_t s);

// ---- camera model maps (camera_kernels.hip): free pixels and points, no residual blocks -----------------------------------
// All pointers are device memory; `k` (the intrinsics) and, in the rig frame, q_rc are read through wave-uniform addresses. The
// launches return the launch's own status; n == 0 launches nothing.
int camera_model_num_params(int model);      // -1: no such model
// The one dispatch on the camera model: f(std::integral_constant<int, MODEL>{}) launches; hipErrorInvalidValue: no such model
template <class F>
hipError_t with_camera_model(int model, F&& f) {
  using std::integral_constant;
  switch (model) {
    case 1: f(integral_constant<int, 1>{}); break; case 2: f(integral_constant<int, 2>{}); break; case 3: f(integral_constant<int, 3>{}); break;
    case 4: f(integral_constant<int, 4>{}); break; case 5: f(integral_constant<int, 5>{}); break; case 6: f(integral_constant<int, 6>{}); break;
    case 7: f(integral_constant<int, 7>{}); break; default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_camera_unproject(int model, const double* k, long long n, const double* pixels /* n x 2 */, double* bearings /* n x 3 */,
                                   uint8_t* valid, hipStream_t s);
// d_point (n x 2 x 3) and d_intr (n x 2 x K) may be nullptr (both: the instantiation without derivatives); valid may be nullptr
hipError_t launch_camera_project_points(int model, const double* k, long long n, const double* points /* n x 3 */, double* pixels /* n x 2 */,
                                        uint8_t* valid, double* d_point, double* d_intr, hipStream_t s);
// projection_uncertainty_kernel: theta = [intrinsics K | q 3 | t 3] of one camera, sigma its (K + 6) x (K + 6) covariance
// (row-major, tangent form, zero rows and columns for what is constant or does not enter the frame)
struct UncertaintyArgs {
  const double* k; const double* q;                       // the camera's intrinsics and q_rc (x, y, z, w); t_rc does not enter: p_r - t_rc = R_rc p_c
  const double* sigma;
  const double* pixels;                                   // n x 2
  double* cov;                                            // n x 3: s_uu, s_uv, s_vv
  uint8_t* valid;
  long long n;
  double range;
  int frame;
};
hipError_t launch_projection_uncertainty(int model, const UncertaintyArgs& a, hipStream_t s);

// ---- chart resection (resect_kernels.hip): one wave per frame of a ragged batch of (pixel, chart point) pairs ----------------
// All pointers are device memory. offsets (n_frames + 1) start at 0 and index pixels / points / ws / flags; q_init and t_init are
// both nullptr (the kernel makes its own start) or n_frames x 4 / x 3; cov_out may be nullptr.
struct ResectArgs {
  const double* k;                                        // intrinsics, read through wave-uniform addresses
  int64_t n_frames;
  const int64_t* offsets;
  const double* pixels;                                   // N x 2
  const double* points;                                   // N x 3, chart frame
  const double* q_init; const double* t_init;
  double* ws;                                             // N x 2: the start's normalised image points
  uint8_t* flags;                                         // N: usable for the start, valid at the current / candidate pose
  int max_iterations; double step_tolerance; double huber_scale; int min_points;
  double* q_out; double* t_out; double* rms_out; int* n_used_out; int* iterations_out; uint8_t* status_out; double* cov_out;
};
hipError_t launch_camera_resect(int model, const ResectArgs& a, hipStream_t s);

// ---- intrinsic calibration (calib_kernels.hip): K intrinsics and the 6-DOF pose of every frame, an arrowhead system ----------
// The control word of the device's LM loop: every kernel of an iteration reads it, the two single-workgroup kernels write it.
// Its head is the same for every arrowhead estimator (arrowhead_dev.hpp writes it; lm_host.hpp polls its first field):
struct LmControl {
  int done;                     // != 0: every later launch returns at once
  int status;                   // the estimator's own codes (CALICO_CALIB_*, CALICO_RIG_*)
  int cur;                      // the slot (border unknowns, poses, Gram matrices, validity bit) of the current point
  int first;                    // the start has not been evaluated yet
  int redo;                     // the reduced system was not positive definite: eliminate and reduce again at the larger lambda
  int iterations;
  int accepted;                 // a step has been accepted: the point kept is not the start
  int final_ok;                 // the undamped reduced system at the result was positive definite (covariance written)
  int frames_used;
  long long pairs_used;
  double lambda, step;          // step: the size of the border's step the candidate was made with
  double initial_cost, final_cost, rms;
};
struct CalibControl {
  LmControl lm;                 // lm.step: max |dk_i| / max(1, |k_i|)
  double k[2][12];              // the intrinsics of the two slots
  double dk[12];
};
static_assert(offsetof(CalibControl, lm.done) == 0, "the host polls the control word's first field");
// Per frame, kCalibFrameDoubles doubles: two slots of kCalibSlot ([0, 4) q, [4, 7) t, [7] Sum rho, [8] Sum |e|^2, [9] valid
// pairs, [10] the cost's rounding scale), [24] Sum rho over the pairs valid at both points, [25] pairs lost, [26] the pose step's
// size, and from [32] Y = A^-1 [B g], column j at 32 + 6 j.
constexpr int kCalibShare = 128;                         // doubles per frame of `share` (at most 66 + 11 + 11 + 4 are used)
constexpr int kCalibSlot = 12, kCalibCommon = 24, kCalibLost = 25, kCalibStep = 26, kCalibY = 32, kCalibFrameDoubles = 112;
struct CalibArgs {
  CalibControl* ctrl;
  int K;                                                  // the model's intrinsics; the Gram matrix has N = K + 7 columns
  unsigned free_bits;                                     // bit i: intrinsic i is estimated
  int64_t n_frames;
  const int64_t* offsets;
  const double* pixels; const double* points;
  uint8_t* flags;                                         // N pairs: valid at slot 0 / 1 (pose_bit)
  uint8_t* active;                                        // n_frames: the frame takes part
  uint8_t* status;                                        // n_frames: CALICO_RESECT_*
  double* frames;                                         // n_frames x kCalibFrameDoubles
  double* gram;                                           // n_frames x 2 x N x N: [J_pose J_k e]^T W [J_pose J_k e] at the two slots
  double* share;                                          // n_frames x kCalibShare: the frame's entries of the reduced system
  int max_iterations; double step_tolerance; double huber_scale;
  double* q_out; double* t_out; double* rms_out; int* n_used_out; double* cov_out /* K x K */;
};
hipError_t launch_calib_evaluate(int model, const CalibArgs& a, hipStream_t s);      // candidate: back-substitution + one pass over the pairs
hipError_t launch_calib_decide(const CalibArgs& a, hipStream_t s);                   // accept / reject, the next lambda, termination
hipError_t launch_calib_eliminate(const CalibArgs& a, bool final, hipStream_t s);    // per frame: Cholesky, Y, B^T Y (final: undamped, outputs)
hipError_t launch_calib_reduce(const CalibArgs& a, bool final, hipStream_t s);       // fixed-order sum over the frames, the K x K solve, dk

// ---- rig calibration (rig_kernels.hip): the extrinsics of C <= 8 cameras and the pose T_rig_chart of every rig frame ----------
// An arrowhead system again: 6 x 6 frame blocks, bordered by the M x M block of the extrinsics (M = 6 C). A view is one camera's
// pairs in one rig frame; the views are sorted by (frame, camera) -- frame_views (n_frames + 1) cuts them into frames -- and so
// are their pairs. The control word of the device's LM loop, as CalibControl:
constexpr int kRigMaxCameras = 8;                        // CALICO_RIG_MAX_CAMERAS (rig.cpp asserts it)
constexpr int kRigMaxDim = 6 * kRigMaxCameras;
constexpr int kRigN = 13;                                // columns of a view's rows: [J_frame 6 | J_extrinsics 6 | e]
struct RigControl {
  LmControl lm;
  long long views_used;
  double cam[2][kRigMaxCameras][8];      // T_rig_camera of the two slots: [0, 4) q, [4, 7) t
  double dx[kRigMaxDim];
};
static_assert(offsetof(RigControl, lm.done) == 0, "the host polls the control word's first field");
// Per frame, kRigFrameDoubles doubles: two slots of 8 ([0, 4) q, [4, 7) t of T_rig_chart), [16] the pose step's size, and from
// [24] Y = A^-1 [B g], column j (the M columns of the extrinsics, then g) at 24 + 6 j; a camera without a view in the frame
// has zero columns. Per view, kRigViewDoubles: two slots of 4 (Sum rho, Sum |e|^2, valid pairs, the cost's rounding scale),
// [8] Sum rho over the pairs valid at both points, [9] pairs lost.
constexpr int kRigStep = 16, kRigY = 24, kRigFrameDoubles = kRigY + 6 * (kRigMaxDim + 1) + 2;
constexpr int kRigViewDoubles = 16, kRigCommon = 8, kRigLost = 9;
constexpr int kRigShare = kRigMaxDim * kRigMaxDim + 2 * kRigMaxDim + 8;      // doubles per frame of `share`: M M + 2 M + 5 are used
struct RigArgs {
  RigControl* ctrl;
  int n_cameras;
  unsigned held_bits;                                     // bit c: camera c is held (the reference, an unconnected camera)
  int intr_at[kRigMaxCameras];                            // where camera c's intrinsics start in `intrinsics`
  const double* intrinsics;
  int64_t n_frames, n_views;
  const int* view_camera; const int64_t* view_frame;      // n_views
  const int64_t* view_offsets;                            // n_views + 1: the view's pairs
  const int64_t* frame_views;                             // n_frames + 1: the frame's views, in camera order
  const double* pixels; const double* points;
  uint8_t* flags;                                         // N pairs: valid at slot 0 / 1 (pose_bit)
  const uint8_t* view_active;                             // n_views: usable, of a connected camera
  const uint8_t* view_writer;                             // n_views: the frame's first active view writes the frame's candidate pose
  uint8_t* frame_active;                                  // n_frames: the frame takes part
  uint8_t* frame_status;                                  // n_frames: CALICO_RIG_FRAME_*
  double* frames;                                         // n_frames x kRigFrameDoubles
  double* views;                                          // n_views x kRigViewDoubles
  double* gram;                                           // n_views x 2 x 13 x 13: [J_f J_x e]^T W [J_f J_x e] at the two slots
  double* share;                                          // n_frames x kRigShare: the frame's entries of the reduced system
  int max_iterations; double step_tolerance; double huber_scale;
  double* q_frame_out; double* t_frame_out; double* view_rms_out; int* view_n_used_out; double* cov_out /* M x M */;
};
// list: the views (indices) of cameras of `model`, in order
hipError_t launch_rig_evaluate(int model, const RigArgs& a, const int* list, int n_list, hipStream_t s);
hipError_t launch_rig_decide(const RigArgs& a, hipStream_t s);                     // accept / reject, the next lambda, termination
hipError_t launch_rig_eliminate(const RigArgs& a, bool final, hipStream_t s);      // per frame: Cholesky, Y, its share (final: undamped, outputs)
hipError_t launch_rig_reduce(const RigArgs& a, bool final, hipStream_t s);         // fixed-order sum over the frames, the M x M solve, the step

// ---- the alignment family (align_kernels.hip, camalign_kernels.hip, accalign_kernels.hip) ---------------------------------------
// Each runs a Levenberg-Marquardt loop over ONE point with a dense normal matrix (7 or 13 unknowns), two slots (current point and
// candidate), and its control word in device memory. The head of that word is the same for the three (point_lm_dev.hpp decides
// and writes it, align_host.hpp sets it up and reads it back), as LmControl is for the arrowhead estimators:
struct PointLmControl {
  int done;                     // != 0: every later launch of the loop returns at once
  int status;                   // CALICO_ALIGN_*
  int cur;                      // the slot of the current point
  int first;                    // the start has not been evaluated yet
  int iterations;
  int cov_ok;                   // the undamped normal matrix at the result was positive definite (covariance written)
  double lambda, step;          // step: the size of the step the candidate was made with
  double initial_cost, final_cost;
};
static_assert(offsetof(PointLmControl, done) == 0, "done is the head's first field");
// the loop ran to a point that is a result
__host__ __device__ inline bool point_lm_ran(int status) { return status == CALICO_ALIGN_OK || status == CALICO_ALIGN_NOT_CONVERGED; }
// The fitted trajectory the three align against: a spline that is not part of a problem (imu_align_dev.hpp evaluates it).
struct AlignSpline {
  int k;                      // order
  int n_valid;                // valid knots: n_knots - 2 (k - 1); segments: n_valid - 1
  const double* knots;        // n_knots
  const double* basis;        // (n_valid - 1) x k x k
  const double* ctrl;         // (n_knots - k) x 6
};

// ---- camera-IMU alignment (align_kernels.hip): rotation, gyroscope bias, latency, gravity from a fitted trajectory ------------
// The control word of the whole call: every kernel reads it, the single-workgroup kernels write it. The stages follow one
// another on the stream without the host reading anything back; a stage that ends the call sets `done`.
constexpr int kAlignGram = 36;                           // the upper triangle of the 8 x 8 Gram matrix of [J r], row-major
constexpr int kAlignCostAt = kAlignGram - 1;             // its last entry, (7, 7): Sum |r|^2
constexpr int kAlignBadAt = kAlignGram;                  // residuals that are not finite
constexpr int kAlignNoiseAt = kAlignGram + 1;            // the cost's rounding scale
constexpr int kAlignSums = kAlignGram + 2;               // what a workgroup of the evaluation sums
constexpr int kAlignPart = 40;                           // doubles per workgroup of a stage's partials (>= kAlignSums, the largest)
constexpr int kAlignThreads = 256;                       // samples per workgroup of every per-sample kernel
constexpr int kAlignLagTile = 8;                         // lags per workgroup of the correlation
constexpr int kAlignMaxLags = 4096;                      // CALICO_ALIGN_MAX_LAGS (imu_align.cpp asserts it)
constexpr int kAlignHornSums = 21;                       // Sum u (3), Sum v (3), Sum v u^T (9), Sum u u^T (6): u = -omega_rig, v = measured
constexpr int kAlignAccelSums = 16;                      // samples (1), Sum M (9), Sum M^T y (3), Sum y (3)
constexpr int kAlignAccelResidual = 8;                   // Sum |r|^2, samples, A^T r (6)
struct AlignControl {
  PointLmControl lm;            // lm.status: the gyroscope part's; lm.done: every later launch of the gyroscope part returns at once
  int accel_status;             // CALICO_ALIGN_*
  int peak_index;               // of the correlation curve (-1: no search)
  long long accel_samples;
  double coarse_latency, peak_correlation, scatter_pivot, gyro_rms, accel_rms;
  double q[2][4], bias[2][3], latency[2];      // the two slots
  double G[2][kAlignPart];      // the summed partials of the two slots
  double cov[49];
  double gravity[3], accel_bias[3];
  double accel_sums[kAlignAccelSums];
};
static_assert(offsetof(AlignControl, lm) == 0, "every launch reads the control word's first field");
struct AlignArgs {
  AlignControl* ctrl;
  AlignSpline spline;
  const double* stamps; const double* meas;               // the gyroscope samples that take part: n of them (the host's range)
  int n;
  const double* lags; int n_lags; double lag_step;        // the latencies of the grid
  double* corr_part;                                      // chunks x n_lags x 3: Sum a, Sum a^2, Sum a m per (chunk, lag)
  double* corr_m;                                         // chunks x 2: Sum m, Sum m^2
  double* curve;                                          // n_lags
  double* part;                                           // chunks x kAlignPart: the partials of the stage that runs
  unsigned free_bits;                                     // bit i: parameter i of (rotation 3, bias 3, latency 1) is estimated
  int max_iterations; double step_tolerance; double inv_sigma;
  const double* accel_stamps; const double* accel; int n_accel;
  double t_ra[3]; int estimate_accel_bias; int min_samples;
};
int align_chunks(int n);                                                            // workgroups of a per-sample kernel
hipError_t launch_align_correlate(const AlignArgs& a, hipStream_t s);              // stage A: partial sums, then the curve and its peak
hipError_t launch_align_horn(const AlignArgs& a, hipStream_t s);                   // stage B: the sums, then rotation and bias into slot 1
hipError_t launch_align_iteration(const AlignArgs& a, hipStream_t s);              // stage C: evaluate the candidate, decide and step
hipError_t launch_align_finish(const AlignArgs& a, hipStream_t s);                 // the covariance and the RMS at the result
hipError_t launch_align_gravity(const AlignArgs& a, hipStream_t s);                // stage D: the sums, the solve, the residual pass

// ---- camera-to-trajectory alignment (camalign_kernels.hip): T_rig_camera and the camera's latency from a fitted trajectory -----
// The frames are those that take part (the host packs them, in stamp order). The control word of the whole call, as AlignControl:
// every kernel reads it, the single-workgroup kernels write it, no host read between the stages.
constexpr int kCamAlignGram = 36;                        // the upper triangle of the 8 x 8 Gram matrix of sqrt(w) [J r], row-major
constexpr int kCamAlignCostAt = 36;                      // Sum rho / sigma^2 over the valid pairs
constexpr int kCamAlignSsAt = 37;                        // Sum |e|^2 over them, pixels^2, no loss
constexpr int kCamAlignValidAt = 38;                     // their number
constexpr int kCamAlignNoiseAt = 39;                     // the cost's rounding scale
constexpr int kCamAlignSums = 40;                        // what a frame's slot holds
constexpr int kCamAlignCommonAt = 2 * kCamAlignSums;     // Sum rho / sigma^2 of the candidate over the pairs valid at the current point
constexpr int kCamAlignLostAt = kCamAlignCommonAt + 1;   // pairs valid at the current point that the candidate lost
constexpr int kCamAlignFrameDoubles = 88;                // per frame: two slots, common, lost
constexpr int kCamAlignPoseSums = 14;                    // Sum q q^T (10: xx xy xz xw yy yz yw zz zw ww), Sum t (3), Sum |t|^2
constexpr int kCamAlignThreads = 256;                    // frames per workgroup of the pose sums
constexpr int kCamAlignLagTile = 8;                      // lags per workgroup of the pose sums
struct CamAlignControl {
  PointLmControl lm;            // lm.done: every later launch of the loop returns at once
  int peak_index;               // of the score curve (-1: no search)
  int frames_used;              // frames that take part after the resection
  long long pairs_used;
  double rms;
  double coarse_latency, peak_score;
  double d2;                    // the mean of |t_camera_chart|^2 over the frames that take part
  double q[2][4], t[2][3], latency[2];      // the two slots
  double G[2][kCamAlignSums];   // the summed frames of the two slots
  double cov[49];
};
static_assert(offsetof(CamAlignControl, lm) == 0, "every launch reads the control word's first field");
struct CamAlignArgs {
  CamAlignControl* ctrl;
  AlignSpline spline;
  const double* k;                                        // the camera's intrinsics
  double q_wm[4], t_wm[3];                                // T_world_chart
  int n_frames;                                           // frames that take part
  const double* stamps;                                   // n_frames
  const int64_t* offsets;                                 // n_frames + 1
  const double* pixels; const double* points;
  uint8_t* flags;                                         // N pairs: valid at slot 0 / 1 (pose_bit)
  uint8_t* active;                                        // n_frames: the frame still takes part (the resection was OK)
  uint8_t* frame_status;                                  // n_frames: CALICO_RESECT_*
  const double* q_cm; const double* t_cm;                 // n_frames x 4 / x 3: T_camera_chart of the resection
  const uint8_t* resect_status;                           // n_frames
  const double* lags; int n_lags; double lag_step;        // the latencies of the grid
  double* pose_part;                                      // chunks x n_lags x kCamAlignPoseSums
  double* curve;                                          // n_lags
  double* frames;                                         // n_frames x kCamAlignFrameDoubles
  unsigned free_bits;                                     // bit i: parameter i of (rotation 3, translation 3, latency 1) is estimated
  int max_iterations; double step_tolerance; double inv_sigma; double huber_scale; int min_frames;
  double* frame_rms_out; int* frame_n_used_out;           // n_frames
};
int camalign_chunks(int n);                                                          // workgroups of the pose sums
hipError_t launch_camalign_gate(const CamAlignArgs& a, hipStream_t s);               // after the resection: who takes part, d^2
hipError_t launch_camalign_search(const CamAlignArgs& a, hipStream_t s);             // stage A: the pose sums per lag, the curve, its minimum
hipError_t launch_camalign_mean(const CamAlignArgs& a, hipStream_t s);               // stage B: the mean pose at the coarse latency into slot 1
hipError_t launch_camalign_iteration(int model, const CamAlignArgs& a, hipStream_t s);      // stage C: evaluate the candidate, decide and step
hipError_t launch_camalign_finish(const CamAlignArgs& a, hipStream_t s);             // covariance, RMS, per-frame outputs

// ---- accelerometer alignment (accalign_kernels.hip): rotation, lever arm, bias, gravity and latency from a fitted trajectory ----
// The samples are those that take part (the host's range). The control word of the whole call, as AlignControl: every kernel
// reads it, the single-wave kernels write it, no host read between the stages.
constexpr int kAccAlignParams = 13;                      // rotation 3, lever arm 3, bias 3, gravity 3, latency 1
constexpr int kAccAlignCols = 14;                        // [J | r]: the columns of the Gram matrix (one 16 x 16 accumulator tile)
constexpr int kAccAlignGram = kAccAlignCols * kAccAlignCols;      // full and symmetric, row-major
constexpr int kAccAlignCostAt = kAccAlignGram - 1;       // its last entry, (13, 13): Sum |r|^2
constexpr int kAccAlignBadAt = kAccAlignGram;            // residuals that are not finite
constexpr int kAccAlignNoiseAt = kAccAlignGram + 1;      // the cost's rounding scale
constexpr int kAccAlignCountAt = kAccAlignGram + 2;      // samples evaluated
constexpr int kAccAlignSums = kAccAlignGram + 3;         // what a workgroup of the evaluation sums
constexpr int kAccAlignPart = 200;                       // doubles per workgroup of the partials (>= kAccAlignSums)
constexpr int kAccAlignThreads = 256;                    // samples per workgroup of the evaluation
constexpr int kAccAlignLinear = 9;                       // stage L: lever arm, bias, gravity (parameters 3 .. 11)
constexpr int kAccAlignStageLinear = 0, kAccAlignStageRefine = 1, kAccAlignStageLoop = 2;
struct AccAlignControl {
  PointLmControl lm;            // lm.first: the LOOP's start has not been evaluated yet
  int linear_status;            // CALICO_ALIGN_* (-1: stage L did not run)
  int stage;                    // kAccAlignStage*
  double rms, linear_rms;
  double q[2][4], t[2][3], bias[2][3], gravity[2][3], latency[2];      // the two slots
  double G[2][kAccAlignPart];   // the summed partials of the two slots
  double cov[kAccAlignParams * kAccAlignParams];
};
static_assert(offsetof(AccAlignControl, lm) == 0, "every launch reads the control word's first field");
struct AccAlignArgs {
  AccAlignControl* ctrl;
  AlignSpline spline;
  const double* stamps; const double* meas;               // the samples that take part: n of them
  int n;
  double* part;                                           // chunks x kAccAlignPart
  unsigned free_bits;                                     // bit i: parameter i is estimated
  int max_iterations; double step_tolerance; double inv_sigma;
};
int accalign_chunks(int n);                                                          // workgroups of the evaluation
hipError_t launch_accalign_iteration(const AccAlignArgs& a, hipStream_t s);          // evaluate the candidate; stage L's solve, or decide and step
hipError_t launch_accalign_finish(const AccAlignArgs& a, hipStream_t s);             // the covariance and the RMS at the result

// ---- IMU noise (allan_kernels.hip): the overlapping Allan variance of the three axes of a static log ----
// samples [n][3]; theta [3][plane], plane >= n + 1 and even (each axis' plane starts on 16 bytes); block_sum, offsets [3][n_blocks];
// partial [3][n_clusters][n_chunks]; out [n_clusters][3] variances, then the three axes' flags as doubles: the call's one readback.
constexpr int kAllanScanBlock = 2048;      // samples per workgroup of the prefix sum
constexpr int kAllanTermChunk = 4096;      // terms of the variance's sum per workgroup
constexpr int kAllanMaxClusters = 256;
struct AllanArgs {
  int n, n_blocks, n_clusters, n_chunks;
  double dt;
  size_t plane;
  const double* samples;
  double* block_sum; double* offsets; double* mean; double* theta; double* partial; double* out;
  int* flags;                              // [3], zero before the launch: the axis holds a sample that is not finite
  int m[kAllanMaxClusters];                // the cluster sizes, ascending: 1 <= m, 2 m < n
};
inline int allan_blocks(int n) { return int((static_cast<long long>(n) + kAllanScanBlock - 1) / kAllanScanBlock); }
__host__ __device__ inline int allan_chunks(int n, int m) { return int((static_cast<long long>(n) - 2 * m + kAllanTermChunk - 1) / kAllanTermChunk); }      // of n - 2m terms
hipError_t launch_imu_allan(const AllanArgs& a, hipStream_t s);

}  // namespace cal
