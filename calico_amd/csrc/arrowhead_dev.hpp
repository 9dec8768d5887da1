// arrowhead_dev.hpp — the Levenberg-Marquardt loop on an arrowhead system, as calib_kernels.hip (border: the K intrinsics of a
// camera) and rig_kernels.hip (border: the M = 6 C extrinsics of a rig's cameras) run it: independent 6x6 blocks A_f of frame
// poses, bordered by one dense block C through the couplings B_f. Unknowns of a pose: [delta_rot, delta_t] with
// R <- exp([delta_rot]x) R (the resection's). Marquardt damping lambda diag on the pose blocks and on C. One LM iteration is four
// launches, enqueued without the host reading anything back (the control word begins with kernels.hpp's LmControl and lives in
// device memory):
//   evaluate  (one wave per block of pairs) makes the frame's candidate pose by back-substitution (delta_f = -(Y_g + Y_B d),
//             Y_f = (A_f + lambda diag A_f)^-1 [B_f g_f]; retract_pose) and evaluates the candidate in ONE pass over the pairs:
//             costs and counts as wave sums of per-lane partial sums, and the Gram matrix of the rows sqrt(w) [J_pose (6) |
//             J_border | e] -- N columns, two rows per pair -- on the matrix cores: the 64 lanes stage 64 rows (first the u rows,
//             then the v rows) in the wave's LDS area, and sixteen v_mfma_f64_16x16x4_f64 steps per tile add them to the 16 x 16
//             accumulator tiles (gram_store writes them out). The Gram matrix holds A_f, B_f, g_f and the block's share of C and
//             of the border's gradient. The order of accumulation is fixed: pairs in trips of 64, rows in groups of four. The
//             pass itself is written out in each kernel file: see DESIGN.md (the rig's section) for what moves when it is not.
//   decide    (one wave) sums the costs in a fixed order (lane l takes l, l + 64, ...; then the wave sum), accepts or rejects the
//             candidate FOR ALL frames (the border is shared), sets the next lambda and ends the loop (lm_control_decide).
//   eliminate (one wave per frame) Cholesky of A_f + lambda diag A_f in LDS and Y_f (eliminate_frame_block), and the frame's share
//             of the reduced system (bty: the entries of B_f^T Y_f), entry by entry in the order the reduction reads. A frame
//             whose damped block is not positive definite drops out for good.
//   reduce    (one workgroup) sums the shares over the frames (sum_shares: thread (part, entry) adds the frames part,
//             part + PARTS, ... in order, the parts are added in order -- nothing depends on a grid size, and there are no
//             atomics), gives what is held an identity row, solves the damped system by Cholesky in LDS and writes the border's
//             step and candidate; a system that is not positive definite raises lambda instead (lm_control_not_pd).
// Launches behind the end of the loop return at once. The same eliminate and reduce kernels, undamped at the result, give the
// outputs, the summary's sums (lm_control_finish) and the covariance of the border (C - Sum B_f^T A_f^-1 B_f)^-1
// (chol_inverse_gram). Device code only.
#pragma once
#include "kernels.hpp"
#include "resect_dev.hpp"

namespace cal {

namespace {

// ---- a pose in 7 doubles: [0, 4) q, [4, 7) t -----------------------------------------------------------------------------------
DEV Q4 slot_q(const double* st) { Q4 q; q.x = st[0]; q.y = st[1]; q.z = st[2]; q.w = st[3]; return q; }
DEV V3 slot_t(const double* st) { return mk(st[4], st[5], st[6]); }
DEV void put_slot_pose(double* st, Q4 q, V3 t) { st[0] = q.x; st[1] = q.y; st[2] = q.z; st[3] = q.w; st[4] = t.x; st[5] = t.y; st[6] = t.z; }
// a frame's pose outputs: the pose of `st`, or the identity for a frame that takes no part
DEV void put_pose_out(double* q_out, double* t_out, const double* st, bool active) {
  q_out[0] = active ? st[0] : 0.0; q_out[1] = active ? st[1] : 0.0; q_out[2] = active ? st[2] : 0.0; q_out[3] = active ? st[3] : 1.0;
  t_out[0] = active ? st[4] : 0.0; t_out[1] = active ? st[5] : 0.0; t_out[2] = active ? st[6] : 0.0;
}
DEV double max3(V3 v) { return fmax(fmax(dabs(v.x), dabs(v.y)), dabs(v.z)); }

// (q, t) <- (exp([dr]x) q0, t0 + dt). Returns the step's size, max |dr_i| and max |dt_i| / max(1, |t0|); a step that is not
// finite is a large one.
DEV double retract_pose(Q4 q0, V3 t0, V3 dr, V3 dt, Q4* q, V3* t) {
  *q = canonical(quat_mul(angle_axis_to_quat(dr), q0));
  *t = t0 + dt;
  double step = fmax(max3(dr), max3(dt) / fmax(1.0, sqrt(dot(t0, t0))));
  if (!__builtin_isfinite(step)) step = 1e300;
  return step;
}

// Huber's loss of the squared residual sq at scale hs (hs2 = hs^2; hs <= 0: none): the weight rho' and rho
DEV void huber(double sq, double hs, double hs2, double* w, double* rho) {
  *w = 1.0; *rho = sq;
  if (hs > 0.0 && sq > hs2) { const double r = sqrt(sq); *w = hs / r; *rho = 2.0 * hs * r - hs2; }
}

// ---- the Gram matrix of a block's rows, accumulated on the matrix cores ------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));
// The accumulator tiles (0, 0) and, for N > 16, (1, 0) and (1, 1) of the lower triangle to G (N x N), full and symmetric (C/D
// layout: col = lane & 15, row = (lane >> 4) + 4 reg)
template <int N>
DEV void gram_store(double* G, int lane, f64x4 t00, f64x4 t10 = {0, 0, 0, 0}, f64x4 t11 = {0, 0, 0, 0}) {
  const int lc = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = lk + 4 * r;
    if (row < N && lc < N) G[row * N + lc] = t00[r];
    if (N > 16) {
      if (16 + row < N && lc < N) { G[(16 + row) * N + lc] = t10[r]; G[lc * N + 16 + row] = t10[r]; }
      if (16 + row < N && 16 + lc < N) G[(16 + row) * N + 16 + lc] = t11[r];
    }
  }
}

// ---- a frame's 6x6 block ------------------------------------------------------------------------------------------------------------
// W (LDS): the damped block; Y (LDS): n_cols columns of 6 (the couplings, then the gradient), column j at 6 j. Y <- W^-1 Y.
// false: W is not positive definite (Y is as it was).
DEV bool eliminate_frame_block(double* W, double* Y, int n_cols, int lane) {
  if (!lds_chol(W, 6, lane)) return false;
  if (lane < n_cols) {      // lane j solves column j: nobody else reads or writes it
    double* const b = Y + 6 * lane;
    for (int i = 0; i < 6; ++i) {
      double v = b[i];
      for (int kk = 0; kk < i; ++kk) v -= W[6 * i + kk] * b[kk];
      b[i] = v / W[6 * i + i];
    }
    for (int i = 5; i >= 0; --i) {
      double v = b[i];
      for (int kk = i + 1; kk < 6; ++kk) v -= W[6 * kk + i] * b[kk];
      b[i] = v / W[6 * i + i];
    }
  }
  wave_fence();
  return true;
}
// an entry of B^T Y: the column of B in a Gram matrix of N columns (from its row 0), the column of Y
DEV double bty(const double* b_col, int N, const double* y_col) {
  double by = 0.0;
  for (int r = 0; r < 6; ++r) by += b_col[r * N] * y_col[r];
  return by;
}

// ---- the reduced system ----------------------------------------------------------------------------------------------------------------
// One workgroup of PARTS x CHUNK threads. s_tot[el] (el < n_el, wanted(el)) <- the sum over the frames that take part of
// share[f * stride + el], CHUNK entries at a time: thread (part, entry) adds the frames part, part + PARTS, ... in order (the
// loads of UNROLL frames in flight at once), then the parts are added in order. An entry that is not wanted is zero.
template <int PARTS, int CHUNK, int UNROLL, class Wanted>
DEV void sum_shares(const double* share, int stride, const uint8_t* active, int64_t n_frames, int n_el, Wanted wanted,
                    double (*s_part)[CHUNK], double* s_tot) {
  const int part = threadIdx.x / CHUNK, slot = threadIdx.x % CHUNK;
  for (int e0 = 0; e0 < n_el; e0 += CHUNK) {      // (uniform bounds: every thread reaches the barriers)
    const int el = e0 + slot;
    double sum = 0.0;
    if (el < n_el && wanted(el)) {
      // (no branch on the frame's flag: a frame that takes no part adds zero; a wave reads 64 consecutive entries of a share)
#pragma unroll UNROLL
      for (int64_t f = part; f < n_frames; f += PARTS) {
        const bool act = active[f] != 0;
        const double v = share[f * stride + el];
        sum += act ? v : 0.0;
      }
    }
    s_part[part][slot] = sum;
    __syncthreads();
    if (part == 0 && el < n_el) {
      double v = 0.0;
#pragma unroll
      for (int p = 0; p < PARTS; ++p) v += s_part[p][slot];
      s_tot[el] = v;
    }
    __syncthreads();
  }
}

// In-place Cholesky of the lower triangle of A (N x N <= 64 x 64, row-major, LDS), lane i owns row i. false: a pivot was not
// positive. (It divides by the pivot's root where lds_chol multiplies by its reciprocal: the two give different bits.)
DEV bool lds_chol_rows(double* A, int N, int lane) {
  bool ok = true;
  const bool mine = lane < N;
#pragma unroll 1
  for (int j = 0; j < N; ++j) {
    double v = 0.0;
    if (mine && lane >= j) {
      v = A[lane * N + j];
#pragma unroll 1
      for (int k = 0; k < j; ++k) v -= A[lane * N + k] * A[j * N + k];
    }
    const double d = __shfl(v, j, 64);
    ok = ok && d > 0.0 && __builtin_isfinite(d);
    const double l = sqrt(ok ? d : 1.0);
    if (mine && lane >= j) A[lane * N + j] = lane == j ? l : v / l;
    wave_fence();
  }
  return uniform_flag(ok);
}

// (L L^T)^-1 = L^-T L^-1 of the factor L (n x n <= 64 x 64, LDS): Li <- L^-1 column by column (lane col < n owns column col),
// then each(e, r, col, v) for every entry e = n r + col, lane l taking l, l + 64, ... The sum of an entry starts at max(r, col):
// the terms before it multiply entries of Li above the diagonal, stored as exact zeros, and would add 0.0 to 0.0 -- unless the
// factor is not finite, and then the caller reports DEGENERATE and no covariance whichever way the sum runs.
template <class Each>
DEV void chol_inverse_gram(const double* L, double* Li, int n, int lane, Each each) {
  if (lane < n) {
    for (int r = 0; r < n; ++r) {
      double v = r == lane ? 1.0 : 0.0;
      for (int kk = lane; kk < r; ++kk) v -= L[n * r + kk] * Li[n * kk + lane];
      Li[n * r + lane] = r < lane ? 0.0 : v / L[n * r + r];
    }
  }
  wave_fence();
  for (int e = lane; e < n * n; e += 64) {
    const int r = e / n, col = e - n * r;
    double v = 0.0;
    for (int kk = (r > col ? r : col); kk < n; ++kk) v += Li[n * kk + r] * Li[n * kk + col];
    each(e, r, col, v);
  }
}

// ---- the control word's head (kernels.hpp: LmControl); lane 0 of one wave writes it ------------------------------------------------------
struct LmStatusCodes { int converged, bad_start, out_of_iterations; };

// The decision on the candidate (lm_rule.hpp: lm_loop_decision). kept: it is finite and lost no pair; any_valid: it has a valid
// pair; small: the step that made it was below the tolerance.
DEV void lm_control_decide(LmControl* head, int lane, bool kept, bool any_valid, double cand, double common, double current, double noise,
                           bool small, int max_iterations, LmStatusCodes status_of) {
  const bool first = head->first != 0;
  const LmLoopStep s = lm_loop_decision(first, kept, any_valid, common, current, noise, small, head->lambda, head->iterations, max_iterations);
  int status = head->status;
  if (s.outcome == kLmConverged) status = status_of.converged;
  else if (s.outcome == kLmBadStart) status = status_of.bad_start;
  else if (s.outcome == kLmOutOfIterations) status = status_of.out_of_iterations;
  if (lane == 0) {
    head->done = s.outcome != kLmRunning ? 1 : 0; head->status = status; if (s.accept) head->cur ^= 1; head->first = 0;
    head->iterations = s.iterations; head->lambda = s.lambda;
    if (first) head->initial_cost = cand;
    else if (s.accept) head->accepted = 1;
  }
}
// The damped reduced system was not positive definite: eliminate and reduce again at ten times the damping, while there is any.
DEV void lm_control_not_pd(LmControl* head, int lane, double lambda, int degenerate_status) {
  if (lane != 0) return;
  if (lambda >= kLmLambdaMax) { head->status = degenerate_status; head->done = 1; }
  else { head->lambda = fmin(lambda * 10.0, kLmLambdaMax); head->redo = 1; }
}
// The sums at the result; ok: the undamped reduced system was positive definite and everything is finite.
DEV void lm_control_finish(LmControl* head, int lane, bool ok, double cost, double rms, double frames, double pairs) {
  if (lane != 0) return;
  head->final_ok = ok ? 1 : 0; head->final_cost = cost; head->rms = rms; head->frames_used = int(frames); head->pairs_used = (long long)pairs;
  // no step was accepted: the point kept is the start, and its cost is ONE number -- this sum, not the decision's sum of the
  // same terms in another order, which can differ from it in the last bit and would read as a decrease
  if (head->accepted == 0) head->initial_cost = cost;
}

}  // namespace
}  // namespace cal
