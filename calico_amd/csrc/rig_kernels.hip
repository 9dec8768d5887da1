// rig_kernels.hip — rig calibration (calico_rig_calibrate): the extrinsics T_rig_camera of the C <= 8 cameras of a rig (all but
// the held ones: the reference camera, cameras the start could not connect) jointly with the pose T_rig_chart of every rig
// frame, from the chart detections of every camera at known intrinsics, by Levenberg-Marquardt on the device.
//
// A view is one camera's (pixel, chart point) pairs in one rig frame; p_camera = R_c^T (R_f p_chart + t_f - t_c). The normal
// equations are an arrowhead: n_frames independent 6x6 blocks A_f (the sum of the frame's views), bordered by the M x M block of
// the extrinsics (M = 6 C; block diagonal before the elimination, one 6x6 block per camera) through one 6x6 coupling per view of
// a camera that is not held. Unknowns: [delta_rot, delta_t] of a frame with R_f <- exp([delta_rot]x) R_f (the resection's) and
// of a camera with R_c <- exp([delta_rot]x) R_c. Marquardt damping lambda diag on both. One LM iteration is four kinds of
// launches, enqueued without the host reading anything back (the control word, RigControl, lives in device memory):
//   evaluate  (one wave per view, kRigWaves views per workgroup; one instantiation per camera model over that model's views)
//             makes the frame's candidate pose (back-substitution delta_f = -(Y_g + Y_B dx)), takes the camera's candidate from
//             the control word, and evaluates the view in ONE pass over its pairs: costs and counts as wave sums of per-lane
//             partial sums, and the Gram matrix of the rows sqrt(w) [J_frame 6 | J_extrinsics 6 | e] -- 13 columns, two rows per
//             pair -- on the matrix cores: the 64 lanes stage 64 rows (first the u rows, then the v rows) in the wave's LDS
//             area, and sixteen v_mfma_f64_16x16x4_f64 steps add them to ONE 16 x 16 accumulator tile. The order of accumulation
//             is fixed: pairs in trips of 64, rows in groups of four. A view of a held camera has zero extrinsic columns.
//   decide    (one wave) sums the views' costs in a fixed order (lane l takes views l, l + 64, ...; then the wave sum), accepts
//             or rejects the candidate FOR ALL frames and cameras, sets the next lambda and ends the loop (lm_rule.hpp).
//   eliminate (one wave per frame) A_f = the sum of its views' frame blocks in camera order, Cholesky of A_f + lambda diag A_f in
//             LDS, Y_f = A_f^-1 [B_f g_f], and the frame's share of the reduced system, entry by entry in the order the
//             reduction reads: C_v - B_v^T Y_v on the diagonal blocks, the fill -B_v^T Y_w between every two of its cameras, its
//             share of the gradient. A frame whose damped block is not positive definite drops out for good, with its views.
//   reduce    (one workgroup) sums the shares over the frames: thread (part, entry) adds the frames part, part + 4, ... in
//             order, the four parts are added in order -- nothing depends on a grid size, and there are no atomics --, gives
//             held cameras unit diagonals, solves the damped M x M system by Cholesky in LDS and writes the step, the
//             candidate extrinsics and their step size.
// Launches behind the end of the loop return at once. The same eliminate and reduce kernels, undamped at the result, give the
// outputs, the summary's sums and the covariance of the extrinsics (C - Sum B_f^T A_f^-1 B_f)^-1.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/calico_hip.h"
#include "kernels.hpp"
#include "resect_dev.hpp"

namespace cal {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kRigWaves = 4;
constexpr int kRigThreads = 64 * kRigWaves;
constexpr int kRigWavesPerSimd = 2;         // the register budget asked of the compiler: 256 VGPRs
constexpr int kRigParts = 4;                // reduce: partial sums over the frames f = part (mod 4), added in order
constexpr int kRigChunk = 256;              // reduce: entries summed at a time
constexpr int kRigCost = 0, kRigSs = 1, kRigValid = 2, kRigNoise = 3;      // a view's slot

namespace {

DEV Q4 pose_q(const double* st) { Q4 q; q.x = st[0]; q.y = st[1]; q.z = st[2]; q.w = st[3]; return q; }
DEV V3 pose_t(const double* st) { return mk(st[4], st[5], st[6]); }
DEV double max3(V3 v) { return fmax(fmax(dabs(v.x), dabs(v.y)), dabs(v.z)); }
DEV int wave_index() { return __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)); }
DEV bool held(const RigArgs& a, int c) { return ((a.held_bits >> c) & 1u) != 0; }

// In-place Cholesky of the lower triangle of A (N x N <= 64 x 64, row-major, LDS), lane i owns row i. false: a pivot was not
// positive.
DEV bool rig_chol(double* A, int N, int lane) {
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

}  // namespace

template <int MODEL>
__global__ __launch_bounds__(kRigThreads, kRigWavesPerSimd) void rig_evaluate_kernel(RigArgs a, const int* list, int n_list) {
  constexpr int N = kRigN;
  __shared__ double s_x[kRigWaves][64 * N];      // the wave's staging area: 64 rows of N columns
  const int lane = threadIdx.x & 63, wave = wave_index();
  const int at = int(blockIdx.x) * kRigWaves + wave;
  if (at >= n_list) return;      // (the whole wave: no barrier follows)
  const RigControl* const c = a.ctrl;
  if (c->done != 0 || c->redo != 0) return;
  const int v = list[at];
  const int cam = a.view_camera[v];
  const int64_t f = a.view_frame[v];
  if (a.view_active[v] == 0 || a.frame_active[f] == 0) return;
  const int cur = c->cur, nxt = cur ^ 1, M = 6 * a.n_cameras;
  const bool first = c->first != 0;
  double* const fr = a.frames + f * kRigFrameDoubles;
  double* const fns = fr + 8 * nxt;
  double* const vw = a.views + int64_t(v) * kRigViewDoubles;
  const double* const k = a.intrinsics + a.intr_at[cam];
  // the candidate pose of the frame: wave-uniform, in registers (every view of the frame computes the same bits)
  Q4 q;
  V3 t;
  double step = 0.0;
  if (first) {
    q = pose_q(fns); t = pose_t(fns);
  } else {
    const double* const fcs = fr + 8 * cur;
    const double* const Y = fr + kRigY;
    double d[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) d[r] = Y[6 * M + r];
#pragma unroll 1
    for (int j = 0; j < M; ++j) {
      const double dxj = c->dx[j];
#pragma unroll
      for (int r = 0; r < 6; ++r) d[r] += Y[6 * j + r] * dxj;
    }
    const V3 dr = mk(-d[0], -d[1], -d[2]), dt = mk(-d[3], -d[4], -d[5]), t0 = pose_t(fcs);
    q = canonical(quat_mul(angle_axis_to_quat(dr), pose_q(fcs)));
    t = t0 + dt;
    step = fmax(max3(dr), max3(dt) / fmax(1.0, sqrt(dot(t0, t0))));
    if (!__builtin_isfinite(step)) step = 1e300;
  }
  const double* const cs = c->cam[nxt][cam];
  const bool is_held = held(a, cam);
  const M3 Rf = rotmat(q), Rc = rotmat(pose_q(cs));
  const V3 tfc = t - pose_t(cs);
  const int64_t base = a.view_offsets[v], n = a.view_offsets[v + 1] - base;
  const double hs = a.huber_scale, hs2 = hs * hs;
  double* const X = s_x[wave];
  const int lc = lane & 15, lk = lane >> 4;
  // the operand column of this lane (a column past N reads column 0 and is replaced by zero)
  const double* const op0 = X + lk * N + (lc < N ? lc : 0);
  f64x4 acc = {0, 0, 0, 0};
  double s_cost = 0.0, s_common = 0.0, s_ss = 0.0, s_noise = 0.0;
  int n_valid = 0, lost = 0;      // wave-uniform counts (ballots)
  for (int64_t i0 = 0; i0 < n; i0 += 64) {
    const int64_t i = base + i0 + lane;
    double x[2][N];
#pragma unroll
    for (int col = 0; col < N; ++col) { x[0][col] = 0.0; x[1][col] = 0.0; }
    bool ok = false, was = false;
    if (i0 + lane < n) {
      const V3 P = mk(a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]);
      const double u = a.pixels[2 * i], w_ = a.pixels[2 * i + 1];
      const uint8_t fl = a.flags[i];
      was = !first && (fl & pose_bit(cur)) != 0;
      const V3 RP = mul(Rf, P), y = RP + tfc, Pc = mulT(Rc, y);
      double pix[2] = {0.0, 0.0}, D[2][3], dK[2][kMaxIntr];
      ok = project<MODEL, true>(k, Pc, pix, D, dK);
      ok = ok && __builtin_isfinite(pix[0]) && __builtin_isfinite(pix[1]);
      a.flags[i] = uint8_t((fl & ~pose_bit(nxt)) | (ok ? pose_bit(nxt) : 0));
      if (ok) {
        const double e[2] = {pix[0] - u, pix[1] - w_}, sq = e[0] * e[0] + e[1] * e[1];
        double w = 1.0, rho = sq;
        if (hs > 0.0 && sq > hs2) { const double r = sqrt(sq); w = hs / r; rho = 2.0 * hs * r - hs2; }
        const double sw = sqrt(w);
        // d p_camera = R_c^T (-[R_f P]x d_frame + dt_frame + [y]x d_camera - dt_camera): with dd = R_c D_r^T, row r is
        // [(R_f P) x dd, dd | -(y x dd), -dd]
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const V3 dd = mul(Rc, mk(D[r][0], D[r][1], D[r][2])), cf = cross(RP, dd), cx = cross(y, dd);
          x[r][0] = sw * cf.x; x[r][1] = sw * cf.y; x[r][2] = sw * cf.z; x[r][3] = sw * dd.x; x[r][4] = sw * dd.y; x[r][5] = sw * dd.z;
          if (!is_held) {
            x[r][6] = -(sw * cx.x); x[r][7] = -(sw * cx.y); x[r][8] = -(sw * cx.z);
            x[r][9] = -(sw * dd.x); x[r][10] = -(sw * dd.y); x[r][11] = -(sw * dd.z);
          }
          x[r][12] = sw * e[r];
        }
        s_cost += rho; s_ss += sq; s_noise += dabs(e[0] * pix[0]) + dabs(e[1] * pix[1]);
        if (was) s_common += rho;
      }
    }
    n_valid += __popcll(__ballot(ok)); lost += __popcll(__ballot(was && !ok));
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      wave_fence();      // (the products of the previous rows have read the area)
#pragma unroll
      for (int col = 0; col < N; ++col) X[lane * N + col] = x[r][col];
      wave_fence();
#pragma unroll
      for (int g = 0; g < 2; ++g) {      // eight steps (32 rows) of operands at a time
        double v0[8];
#pragma unroll
        for (int s = 0; s < 8; ++s) v0[s] = op0[(32 * g + 4 * s) * N];
        if (lc >= N) {
#pragma unroll
          for (int s = 0; s < 8; ++s) v0[s] = 0.0;
        }
#pragma unroll
        for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v0[s], v0[s], acc, 0, 0, 0);
      }
    }
  }
  // the Gram matrix, full and symmetric (C/D layout: col = lane & 15, row = (lane >> 4) + 4 reg)
  double* const G = a.gram + (int64_t(v) * 2 + nxt) * (N * N);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = lk + 4 * r;
    if (row < N && lc < N) G[row * N + lc] = acc[r];
  }
  s_cost = wave_sum(s_cost); s_common = wave_sum(s_common); s_ss = wave_sum(s_ss); s_noise = wave_sum(s_noise);
  if (lane == 0) {
    double* const ns = vw + 4 * nxt;
    ns[kRigCost] = s_cost; ns[kRigSs] = s_ss; ns[kRigValid] = double(n_valid); ns[kRigNoise] = s_noise;
    vw[kRigCommon] = s_common; vw[kRigLost] = double(lost);
    if (a.view_writer[v] != 0) {
      fns[0] = q.x; fns[1] = q.y; fns[2] = q.z; fns[3] = q.w; fns[4] = t.x; fns[5] = t.y; fns[6] = t.z;
      fr[kRigStep] = step;
    }
  }
}

// One wave. The sums run over the views that take part, lane l over l, l + 64, ..., then the wave sum: a fixed order.
__global__ __launch_bounds__(64) void rig_decide_kernel(RigArgs a) {
  RigControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  if (c->done != 0) return;
  if (c->redo != 0) { if (lane == 0) c->redo = 0; return; }
  const int cur = c->cur, nxt = cur ^ 1;
  double cand = 0.0, common = 0.0, current = 0.0, noise = 0.0, lost = 0.0, valid = 0.0, step = 0.0;
  bool finite = true;
  // (a view that takes no part adds zero; its slots are finite, the host cleared them)
#pragma unroll 2
  for (int64_t v = lane; v < a.n_views; v += 64) {
    const bool act = a.view_active[v] != 0 && a.frame_active[a.view_frame[v]] != 0;
    const double* const vw = a.views + v * kRigViewDoubles;
    const double* const cs = vw + 4 * cur;
    const double* const ns = vw + 4 * nxt;
    cand += act ? ns[kRigCost] : 0.0; valid += act ? ns[kRigValid] : 0.0; common += act ? vw[kRigCommon] : 0.0;
    lost += act ? vw[kRigLost] : 0.0; current += act ? cs[kRigCost] : 0.0; noise += act ? cs[kRigNoise] : 0.0;
  }
#pragma unroll 2
  for (int64_t f = lane; f < a.n_frames; f += 64) {
    const bool act = a.frame_active[f] != 0;
    const double* const fr = a.frames + f * kRigFrameDoubles;
    const double* const ns = fr + 8 * nxt;
    const bool v_finite = finite_pose(pose_q(ns), pose_t(ns));
    step = fmax(step, act ? fr[kRigStep] : 0.0);
    finite = finite && (v_finite || !act);
  }
  if (lane < a.n_cameras) finite = finite && finite_pose(pose_q(c->cam[nxt][lane]), pose_t(c->cam[nxt][lane]));
  cand = wave_sum(cand); common = wave_sum(common); current = wave_sum(current); noise = wave_sum(noise); lost = wave_sum(lost);
  valid = wave_sum(valid); step = wave_max(step);
  finite = __all(finite) != 0;
  const bool kept = lost == 0.0 && finite && __builtin_isfinite(cand);
  const bool first = c->first != 0, small = fmax(step, c->step_x) < a.step_tolerance;
  const LmLoopStep s = lm_loop_decision(first, kept, valid >= 1.0, common, current, noise, small, c->lambda, c->iterations, a.max_iterations);
  int status = c->status;
  if (s.outcome == kLmConverged) status = CALICO_RIG_OK;
  else if (s.outcome == kLmBadStart) status = CALICO_RIG_DEGENERATE;
  else if (s.outcome == kLmOutOfIterations) status = CALICO_RIG_NOT_CONVERGED;
  if (lane == 0) {
    c->done = s.outcome != kLmRunning ? 1 : 0; c->status = status; c->cur = s.accept ? nxt : cur; c->first = 0;
    c->iterations = s.iterations; c->lambda = s.lambda;
    if (first) c->initial_cost = cand;
    else if (s.accept) c->accepted = 1;
  }
}

// final: undamped, at the result, for every frame (the loop is over): the outputs of the frame and of its views, Y and the
// share for the covariance.
__global__ __launch_bounds__(kRigThreads) void rig_eliminate_kernel(RigArgs a, int final) {
  constexpr int N = kRigN;
  __shared__ double s_w[kRigWaves][36 + 6 * (kRigMaxDim + 1)];
  __shared__ int s_av[kRigWaves][2 * kRigMaxCameras];
  const int lane = threadIdx.x & 63, wave = wave_index();
  const int64_t f = int64_t(blockIdx.x) * kRigWaves + wave;
  if (f >= a.n_frames) return;
  const RigControl* const c = a.ctrl;
  if (!final && c->done != 0) return;
  const int C = a.n_cameras, M = 6 * C, cur = c->cur;
  double* const fr = a.frames + f * kRigFrameDoubles;
  const double* const fcs = fr + 8 * cur;
  const int64_t v0 = a.frame_views[f], v1 = a.frame_views[f + 1];
  bool active = a.frame_active[f] != 0;
  if (active) {
    const double lambda = final ? 0.0 : c->lambda;
    const double* const gram = a.gram + cur * (N * N);      // view v's Gram matrix at gram + v * 2 N N
    double* const W = s_w[wave];
    double* const Y = W + 36;      // column j (M columns of B, then g) at 6 j
    int* const av = s_av[wave];    // av[c]: camera c's view in this frame that takes part, or -1; xv[c]: the same, -1 where c is held
    int* const xv = av + kRigMaxCameras;
    if (lane < 2 * kRigMaxCameras) av[lane] = -1;
    wave_fence();
    if (v0 + lane < v1 && a.view_active[v0 + lane] != 0) {      // (a camera has at most one view in a frame)
      const int cam = a.view_camera[v0 + lane];
      av[cam] = int(v0 + lane);
      if (!held(a, cam)) xv[cam] = int(v0 + lane);
    }
    wave_fence();
    if (lane < 36) {
      const int r = lane / 6, col = lane - 6 * r;
      double s = 0.0;
      for (int cam = 0; cam < C; ++cam)
        if (av[cam] >= 0) s += gram[int64_t(av[cam]) * (2 * N * N) + r * N + col];
      W[lane] = s * (r == col ? 1.0 + lambda : 1.0);
    }
    for (int e = lane; e < 6 * (M + 1); e += 64) {
      const int j = e / 6, r = e - 6 * j;
      double s = 0.0;
      if (j < M) {
        const int cam = j / 6;
        if (xv[cam] >= 0) s = gram[int64_t(xv[cam]) * (2 * N * N) + r * N + 6 + (j - 6 * cam)];
      } else {
        for (int cam = 0; cam < C; ++cam)
          if (av[cam] >= 0) s += gram[int64_t(av[cam]) * (2 * N * N) + r * N + 12];
      }
      Y[e] = s;
    }
    wave_fence();
    const bool pd = lds_chol(W, 6, lane);
    if (!pd) {
      active = false;
      if (lane == 0) { a.frame_active[f] = 0; a.frame_status[f] = uint8_t(CALICO_RIG_FRAME_NOT_POSITIVE_DEFINITE); }
    } else {
      if (lane <= M) {      // lane j solves column j: nobody else reads or writes it
        double* const b = Y + 6 * lane;
        for (int i = 0; i < 6; ++i) {
          double s = b[i];
          for (int kk = 0; kk < i; ++kk) s -= W[6 * i + kk] * b[kk];
          b[i] = s / W[6 * i + i];
        }
        for (int i = 5; i >= 0; --i) {
          double s = b[i];
          for (int kk = i + 1; kk < 6; ++kk) s -= W[6 * kk + i] * b[kk];
          b[i] = s / W[6 * i + i];
        }
      }
      wave_fence();
      for (int e = lane; e < 6 * (M + 1); e += 64) fr[kRigY + e] = Y[e];
      // the frame's share, entry by entry in the reduction's order: the lower triangle of the M x M system by rows (row-major,
      // the upper entries are never read), the gradient (M), the diagonal of C (M: the damping's scale), then Sum rho,
      // Sum |e|^2, the valid pairs, a one (the frames are counted) and the frame's views
      double* const sh = a.share + f * kRigShare;
      const int n_el = M * M + 2 * M + 5;
      for (int e = lane; e < n_el; e += 64) {
        double s = 0.0;
        if (e < M * M + M) {
          const int i = e < M * M ? e / M : e - M * M, j = e < M * M ? e - M * i : M;
          const int ci = i / 6, ii = i - 6 * ci, cj = j < M ? j / 6 : ci, jj = j < M ? j - 6 * cj : 6;
          if (j > i && j < M) continue;
          const int vi = xv[ci], vj = xv[cj];
          if (vi >= 0 && vj >= 0) {
            const double* const Gi = gram + int64_t(vi) * (2 * N * N);
            if (ci == cj) s = Gi[(6 + ii) * N + 6 + jj];
            double by = 0.0;
            for (int r = 0; r < 6; ++r) by += Gi[r * N + 6 + ii] * Y[6 * j + r];
            s -= by;
          }
        } else if (e < M * M + 2 * M) {
          const int i = e - M * M - M, ci = i / 6, ii = i - 6 * ci;
          if (xv[ci] >= 0) s = gram[int64_t(xv[ci]) * (2 * N * N) + (6 + ii) * N + 6 + ii];
        } else {
          const int which = e - M * M - 2 * M;
          for (int cam = 0; cam < C; ++cam) {
            if (av[cam] < 0) continue;
            const double* const vs = a.views + int64_t(av[cam]) * kRigViewDoubles + 4 * cur;
            s += which < 3 ? vs[which] : which == 3 ? 0.0 : 1.0;
          }
          if (which == 3) s = 1.0;
        }
        sh[e] = s;
      }
    }
  }
  if (final) {
    if (lane == 0) {
      a.q_frame_out[4 * f] = active ? fcs[0] : 0.0; a.q_frame_out[4 * f + 1] = active ? fcs[1] : 0.0;
      a.q_frame_out[4 * f + 2] = active ? fcs[2] : 0.0; a.q_frame_out[4 * f + 3] = active ? fcs[3] : 1.0;
      a.t_frame_out[3 * f] = active ? fcs[4] : 0.0; a.t_frame_out[3 * f + 1] = active ? fcs[5] : 0.0; a.t_frame_out[3 * f + 2] = active ? fcs[6] : 0.0;
    }
    if (v0 + lane < v1) {
      const int64_t v = v0 + lane;
      const bool act = active && a.view_active[v] != 0;
      const double* const vs = a.views + v * kRigViewDoubles + 4 * cur;
      a.view_rms_out[v] = act ? sqrt(vs[kRigSs] / vs[kRigValid]) : 0.0;
      a.view_n_used_out[v] = act ? int(vs[kRigValid]) : 0;
    }
  }
}

// One workgroup of kRigParts x kRigChunk threads: thread (part, entry) adds the entry of the frames' shares, kRigChunk entries
// at a time.
__global__ __launch_bounds__(kRigParts * kRigChunk) void rig_reduce_kernel(RigArgs a, int final) {
  __shared__ double s_part[kRigParts][kRigChunk];
  __shared__ double s_tot[kRigShare];      // first the M x M system (in place: it becomes its Cholesky factor)
  __shared__ double s_Li[kRigMaxDim * kRigMaxDim], s_rhs[kRigMaxDim];
  RigControl* const c = a.ctrl;
  if (!final && c->done != 0) return;      // (the whole workgroup)
  const int C = a.n_cameras, M = 6 * C, cur = c->cur, nxt = cur ^ 1;
  const int part = threadIdx.x / kRigChunk, slot = threadIdx.x % kRigChunk;
  const int n_el = M * M + 2 * M + 5;
  for (int e0 = 0; e0 < n_el; e0 += kRigChunk) {      // (uniform bounds: every thread reaches the barriers)
    const int el = e0 + slot;
    bool wanted = el < n_el;
    if (wanted && el < M * M) { const int i = el / M; wanted = el - M * i <= i; }
    double sum = 0.0;
    if (wanted) {
      // (no branch on the frame's flag: a frame that takes no part adds zero; a wave reads 64 consecutive entries of a share)
#pragma unroll 4
      for (int64_t f = part; f < a.n_frames; f += kRigParts) {
        const bool act = a.frame_active[f] != 0;
        const double v = a.share[f * kRigShare + el];
        sum += act ? v : 0.0;
      }
    }
    s_part[part][slot] = sum;
    __syncthreads();
    if (part == 0 && el < n_el) {
      double v = 0.0;
#pragma unroll
      for (int p = 0; p < kRigParts; ++p) v += s_part[p][slot];
      s_tot[el] = v;
    }
    __syncthreads();
  }
  if (threadIdx.x >= 64) return;      // the small system: wave 0
  const int lane = threadIdx.x;
  const double lambda = final ? 0.0 : c->lambda;
  double* const S = s_tot;
  const double* const grad = s_tot + M * M;
  const double* const diag = grad + M;
  const double* const sums = diag + M;
  for (int e = lane; e < M * M; e += 64) {
    const int i = e / M, j = e - M * i;
    if (j > i) continue;
    const bool free_ij = !held(a, i / 6) && !held(a, j / 6);
    double v = S[e];
    if (i == j) v += lambda * diag[i];
    S[e] = free_ij ? v : (i == j ? 1.0 : 0.0);      // a held camera: identity rows, a zero right-hand side
  }
  if (lane < M) s_rhs[lane] = held(a, lane / 6) ? 0.0 : -grad[lane];
  wave_fence();
  const bool pd = rig_chol(S, M, lane);
  if (!final) {
    if (!pd) {
      if (lane == 0) {
        if (lambda >= kLmLambdaMax) { c->status = CALICO_RIG_DEGENERATE; c->done = 1; }
        else { c->lambda = fmin(lambda * 10.0, kLmLambdaMax); c->redo = 1; }
      }
      return;
    }
    lds_chol_solve(S, s_rhs, M, lane);
    double step = 0.0;
    if (lane < M) c->dx[lane] = s_rhs[lane];
    if (lane < C) {      // lane c: camera c's candidate
      const double* const cs = c->cam[cur][lane];
      double* const ns = c->cam[nxt][lane];
      Q4 q = pose_q(cs);
      V3 t = pose_t(cs);
      if (!held(a, lane)) {
        const V3 dr = mk(s_rhs[6 * lane], s_rhs[6 * lane + 1], s_rhs[6 * lane + 2]);
        const V3 dt = mk(s_rhs[6 * lane + 3], s_rhs[6 * lane + 4], s_rhs[6 * lane + 5]);
        step = fmax(max3(dr), max3(dt) / fmax(1.0, sqrt(dot(t, t))));
        if (!__builtin_isfinite(step)) step = 1e300;
        q = canonical(quat_mul(angle_axis_to_quat(dr), q));
        t = t + dt;
      }
      ns[0] = q.x; ns[1] = q.y; ns[2] = q.z; ns[3] = q.w; ns[4] = t.x; ns[5] = t.y; ns[6] = t.z;
    }
    step = wave_max(step);
    if (lane == 0) c->step_x = step;
    return;
  }
  // the result: sums for the summary, and the covariance of the extrinsics, the inverse of the undamped reduced system
  const double cost = sums[0], ss = sums[1], valid = sums[2], frames = sums[3], views = sums[4];
  const double rms = sqrt(ss / valid);
  bool ok = pd && __builtin_isfinite(cost) && __builtin_isfinite(rms);
  if (lane < C) ok = ok && finite_pose(pose_q(c->cam[cur][lane]), pose_t(c->cam[cur][lane]));
  // L^-1 column by column (lane col < M owns column col), then L^-T L^-1
  if (lane < M) {
    for (int r = 0; r < M; ++r) {
      double v = r == lane ? 1.0 : 0.0;
      for (int kk = lane; kk < r; ++kk) v -= S[M * r + kk] * s_Li[M * kk + lane];
      s_Li[M * r + lane] = r < lane ? 0.0 : v / S[M * r + r];
    }
  }
  wave_fence();
  for (int e = lane; e < M * M; e += 64) {
    const int r = e / M, col = e - M * r;
    double v = 0.0;
    for (int kk = (r > col ? r : col); kk < M; ++kk) v += s_Li[M * kk + r] * s_Li[M * kk + col];
    v = (!held(a, r / 6) && !held(a, col / 6)) ? v : 0.0;
    ok = ok && __builtin_isfinite(v);
    if (a.cov_out) a.cov_out[e] = pd ? v : 0.0;
  }
  ok = __all(ok) != 0;
  if (lane == 0) {
    c->final_ok = ok ? 1 : 0; c->final_cost = cost; c->rms = rms; c->frames_used = int(frames); c->views_used = (long long)views;
    c->pairs_used = (long long)valid;
    // no step was accepted: the point kept is the start, and its cost is ONE number -- this sum, not the decision's sum of the
    // same terms in another order, which can differ from it in the last bit and would read as a decrease
    if (c->accepted == 0) c->initial_cost = cost;
  }
}

hipError_t launch_rig_evaluate(int model, const RigArgs& a, const int* list, int n_list, hipStream_t s) {
  if (n_list <= 0) return hipSuccess;
  const dim3 grid(unsigned((n_list + kRigWaves - 1) / kRigWaves)), block(kRigThreads);
  return with_camera_model(model, [&](auto m) { hipLaunchKernelGGL(rig_evaluate_kernel<decltype(m)::value>, grid, block, 0, s, a, list, n_list); });
}
hipError_t launch_rig_decide(const RigArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(rig_decide_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}
hipError_t launch_rig_eliminate(const RigArgs& a, bool final, hipStream_t s) {
  if (a.n_frames <= 0) return hipSuccess;
  const dim3 grid(unsigned((a.n_frames + kRigWaves - 1) / kRigWaves)), block(kRigThreads);
  hipLaunchKernelGGL(rig_eliminate_kernel, grid, block, 0, s, a, final ? 1 : 0);
  return hipGetLastError();
}
hipError_t launch_rig_reduce(const RigArgs& a, bool final, hipStream_t s) {
  hipLaunchKernelGGL(rig_reduce_kernel, dim3(1), dim3(kRigParts * kRigChunk), 0, s, a, final ? 1 : 0);
  return hipGetLastError();
}

}  // namespace cal
