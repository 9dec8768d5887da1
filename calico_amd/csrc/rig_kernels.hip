// rig_kernels.hip — rig calibration (calico_rig_calibrate): the extrinsics T_rig_camera of the C <= 8 cameras of a rig (all but
// the held ones: the reference camera, cameras the start could not connect) jointly with the pose T_rig_chart of every rig
// frame, from the chart detections of every camera at known intrinsics, by Levenberg-Marquardt on the device.
//
// The arrowhead loop of arrowhead_dev.hpp, which describes the four launches of an iteration. What is this file's own: a view is
// one camera's (pixel, chart point) pairs in one rig frame, p_camera = R_c^T (R_f p_chart + t_f - t_c), and it is the block of
// pairs of the evaluation: one wave per view, kRigWaves views per workgroup, one instantiation per camera model over that model's
// views (every view of a frame computes the frame's candidate pose, the same bits; the frame's writer stores it). The border is
// the M x M block of the extrinsics (M = 6 C; block diagonal before the elimination, one 6x6 block per camera; a held camera has
// identity rows), and a camera moves as a frame does, R_c <- exp([delta_rot]x) R_c. The rows are sqrt(w) [J_frame 6 |
// J_extrinsics 6 | e], 13 columns, ONE accumulator tile; a view of a held camera has zero extrinsic columns. A frame's block A_f
// is the sum of its views' frame blocks in camera order, and its share of the reduced system is C_v - B_v^T Y_v on the diagonal
// blocks, the fill -B_v^T Y_w between every two of its cameras, and its share of the gradient, summed in four parts, 256 entries
// at a time. A frame that drops out takes its views with it. The control word is RigControl.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/calico_hip.h"
#include "arrowhead_dev.hpp"
#include "kernels.hpp"

namespace cal {

constexpr int kRigWaves = 4;
constexpr int kRigThreads = 64 * kRigWaves;
constexpr int kRigWavesPerSimd = 2;         // the register budget asked of the compiler: 256 VGPRs
constexpr int kRigParts = 4;                // reduce: partial sums over the frames f = part (mod 4), added in order
constexpr int kRigChunk = 256;              // reduce: entries summed at a time
constexpr int kRigCost = 0, kRigSs = 1, kRigValid = 2, kRigNoise = 3;      // a view's slot

namespace {

constexpr LmStatusCodes kRigStatus = {CALICO_RIG_OK, CALICO_RIG_DEGENERATE, CALICO_RIG_NOT_CONVERGED};

DEV int wave_index() { return __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6)); }
DEV bool held(const RigArgs& a, int c) { return ((a.held_bits >> c) & 1u) != 0; }

}  // namespace

template <int MODEL>
__global__ __launch_bounds__(kRigThreads, kRigWavesPerSimd) void rig_evaluate_kernel(RigArgs a, const int* list, int n_list) {
  constexpr int N = kRigN;
  __shared__ double s_x[kRigWaves][64 * N];      // the wave's staging area: 64 rows of N columns
  const int lane = threadIdx.x & 63, wave = wave_index();
  const int at = int(blockIdx.x) * kRigWaves + wave;
  if (at >= n_list) return;      // (the whole wave: no barrier follows)
  const RigControl* const c = a.ctrl;
  if (c->lm.done != 0 || c->lm.redo != 0) return;
  const int v = list[at];
  const int cam = a.view_camera[v];
  const int64_t f = a.view_frame[v];
  if (a.view_active[v] == 0 || a.frame_active[f] == 0) return;
  const int cur = c->lm.cur, nxt = cur ^ 1, M = 6 * a.n_cameras;
  const bool first = c->lm.first != 0;
  double* const fr = a.frames + f * kRigFrameDoubles;
  double* const fns = fr + 8 * nxt;
  double* const vw = a.views + int64_t(v) * kRigViewDoubles;
  const double* const k = a.intrinsics + a.intr_at[cam];
  // the candidate pose of the frame: wave-uniform, in registers (every view of the frame computes the same bits)
  Q4 q;
  V3 t;
  double step = 0.0;
  if (first) {
    q = slot_q(fns); t = slot_t(fns);
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
    step = retract_pose(slot_q(fcs), slot_t(fcs), mk(-d[0], -d[1], -d[2]), mk(-d[3], -d[4], -d[5]), &q, &t);
  }
  const double* const cs = c->cam[nxt][cam];
  const bool is_held = held(a, cam);
  const M3 Rf = rotmat(q), Rc = rotmat(slot_q(cs));
  const V3 tfc = t - slot_t(cs);
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
        double w, rho;
        huber(sq, hs, hs2, &w, &rho);
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
  gram_store<N>(a.gram + (int64_t(v) * 2 + nxt) * (N * N), lane, acc);
  s_cost = wave_sum(s_cost); s_common = wave_sum(s_common); s_ss = wave_sum(s_ss); s_noise = wave_sum(s_noise);
  if (lane == 0) {
    double* const ns = vw + 4 * nxt;
    ns[kRigCost] = s_cost; ns[kRigSs] = s_ss; ns[kRigValid] = double(n_valid); ns[kRigNoise] = s_noise;
    vw[kRigCommon] = s_common; vw[kRigLost] = double(lost);
    if (a.view_writer[v] != 0) {
      put_slot_pose(fns, q, t);
      fr[kRigStep] = step;
    }
  }
}

// One wave. The sums run over the views that take part, lane l over l, l + 64, ..., then the wave sum: a fixed order.
__global__ __launch_bounds__(64) void rig_decide_kernel(RigArgs a) {
  RigControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  if (c->lm.done != 0) return;
  if (c->lm.redo != 0) { if (lane == 0) c->lm.redo = 0; return; }
  const int cur = c->lm.cur, nxt = cur ^ 1;
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
    const bool v_finite = finite_pose(slot_q(ns), slot_t(ns));
    step = fmax(step, act ? fr[kRigStep] : 0.0);
    finite = finite && (v_finite || !act);
  }
  if (lane < a.n_cameras) finite = finite && finite_pose(slot_q(c->cam[nxt][lane]), slot_t(c->cam[nxt][lane]));
  cand = wave_sum(cand); common = wave_sum(common); current = wave_sum(current); noise = wave_sum(noise); lost = wave_sum(lost);
  valid = wave_sum(valid); step = wave_max(step);
  finite = __all(finite) != 0;
  const bool kept = lost == 0.0 && finite && __builtin_isfinite(cand);
  const bool small = fmax(step, c->lm.step) < a.step_tolerance;
  lm_control_decide(&c->lm, lane, kept, valid >= 1.0, cand, common, current, noise, small, a.max_iterations, kRigStatus);
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
  if (!final && c->lm.done != 0) return;
  const int C = a.n_cameras, M = 6 * C, cur = c->lm.cur;
  double* const fr = a.frames + f * kRigFrameDoubles;
  const double* const fcs = fr + 8 * cur;
  const int64_t v0 = a.frame_views[f], v1 = a.frame_views[f + 1];
  bool active = a.frame_active[f] != 0;
  if (active) {
    const double lambda = final ? 0.0 : c->lm.lambda;
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
    if (!eliminate_frame_block(W, Y, M + 1, lane)) {
      active = false;
      if (lane == 0) { a.frame_active[f] = 0; a.frame_status[f] = uint8_t(CALICO_RIG_FRAME_NOT_POSITIVE_DEFINITE); }
    } else {
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
            s -= bty(Gi + 6 + ii, N, Y + 6 * j);
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
    if (lane == 0) put_pose_out(a.q_frame_out + 4 * f, a.t_frame_out + 3 * f, fcs, active);
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
// at a time; of the M x M system only the lower triangle.
__global__ __launch_bounds__(kRigParts * kRigChunk) void rig_reduce_kernel(RigArgs a, int final) {
  __shared__ double s_part[kRigParts][kRigChunk];
  __shared__ double s_tot[kRigShare];      // first the M x M system (in place: it becomes its Cholesky factor)
  __shared__ double s_Li[kRigMaxDim * kRigMaxDim], s_rhs[kRigMaxDim];
  RigControl* const c = a.ctrl;
  if (!final && c->lm.done != 0) return;      // (the whole workgroup)
  const int C = a.n_cameras, M = 6 * C, cur = c->lm.cur, nxt = cur ^ 1;
  const auto lower = [M](int el) { return el >= M * M || el - M * (el / M) <= el / M; };
  sum_shares<kRigParts, kRigChunk, 4>(a.share, kRigShare, a.frame_active, a.n_frames, M * M + 2 * M + 5, lower, s_part, s_tot);
  if (threadIdx.x >= 64) return;      // the small system: wave 0
  const int lane = threadIdx.x;
  const double lambda = final ? 0.0 : c->lm.lambda;
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
  const bool pd = lds_chol_rows(S, M, lane);
  if (!final) {
    if (!pd) { lm_control_not_pd(&c->lm, lane, lambda, CALICO_RIG_DEGENERATE); return; }
    lds_chol_solve(S, s_rhs, M, lane);
    double step = 0.0;
    if (lane < M) c->dx[lane] = s_rhs[lane];
    if (lane < C) {      // lane c: camera c's candidate
      const double* const cs = c->cam[cur][lane];
      Q4 q = slot_q(cs);
      V3 t = slot_t(cs);
      if (!held(a, lane)) {
        const V3 dr = mk(s_rhs[6 * lane], s_rhs[6 * lane + 1], s_rhs[6 * lane + 2]);
        const V3 dt = mk(s_rhs[6 * lane + 3], s_rhs[6 * lane + 4], s_rhs[6 * lane + 5]);
        step = retract_pose(q, t, dr, dt, &q, &t);
      }
      put_slot_pose(c->cam[nxt][lane], q, t);
    }
    step = wave_max(step);
    if (lane == 0) c->lm.step = step;
    return;
  }
  // the result: sums for the summary, and the covariance of the extrinsics, the inverse of the undamped reduced system
  const double cost = sums[0], ss = sums[1], valid = sums[2], frames = sums[3], views = sums[4];
  const double rms = sqrt(ss / valid);
  bool ok = pd && __builtin_isfinite(cost) && __builtin_isfinite(rms);
  if (lane < C) ok = ok && finite_pose(slot_q(c->cam[cur][lane]), slot_t(c->cam[cur][lane]));
  chol_inverse_gram(S, s_Li, M, lane, [&](int e, int r, int col, double v) {
    v = (!held(a, r / 6) && !held(a, col / 6)) ? v : 0.0;
    ok = ok && __builtin_isfinite(v);
    if (a.cov_out) a.cov_out[e] = pd ? v : 0.0;
  });
  ok = __all(ok) != 0;
  lm_control_finish(&c->lm, lane, ok, cost, rms, frames, valid);
  if (lane == 0) c->views_used = (long long)views;
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
