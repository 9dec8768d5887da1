// camalign_kernels.hip — camera-to-trajectory alignment on the device (calico_camera_align): the extrinsics
// T_rig_camera and the latency of a camera that shares no instant with the reference camera, from the fitted trajectory and the
// camera's raw chart detections at known intrinsics, as a start for the batch solve. The camera-side twin of align_kernels.hip.
// The model is the optimiser's own camera term (frame_camera_block, eval_kernels.hip) with the trajectory held:
//   t = stamp - latency (the spline segment is the STAMP's),  p = spline(t),  R_rw = R(quat(-p[0:3])),  t_wr = p[3:6],
//   y = R_rw (R_wm x + t_wm - t_wr),  x_c = R_rc^T (y - t_rc),  residual = (pixel - project(k, x_c)) / sigma_pixel;
// the latency column is exact: d y / d t = omega x y - R_rw t_wr' with omega = J(phi) phi', through the segment's first derivative.
// Stages, one after the other on the stream, steered by the control word (CamAlignControl, kernels.hpp) without a host read:
//   R  (resect_kernels.hip)      T_camera_chart of every frame; camalign_gate_kernel: the frames whose resection is OK go on,
//                                their number and d^2, the mean of |t_camera_chart|^2
//   A  camalign_pose_kernel      frame chunks x lag tiles: E_i(tau) = T_rig_world(stamp_i - tau) T_world_chart T_chart_camera_i
//                                and its 14 sums Sum q q^T, Sum t, Sum |t|^2 per (chunk, lag)
//      camalign_peak_kernel      one workgroup: the chunks added in order, score(tau) = 4 (1 - lambda_max / n) + var(t) / d^2, its
//                                minimum and the parabola through the three points around it
//   B  camalign_pose_kernel      once more at the coarse latency; camalign_mean_kernel: one wave, the principal eigenvector of
//                                Sum q q^T by cyclic Jacobi (w >= 0) and the mean translation, into slot 1
//   C  camalign_eval_kernel      one wave per frame, four frames per workgroup, per camera model: the frame's pose and its time
//                                derivative once, the pairs in trips of 64, the 8-column Gram matrix of sqrt(w) [J | r] in one
//                                16 x 16 FP64 MFMA accumulator tile (as rig_kernels.hip forms its 13 columns)
//      camalign_decide_kernel    one wave: the frames added in order, accept / reject, the damped 7 x 7 step, the next candidate
//      camalign_final_kernel     one wave: the undamped inverse normal matrix, the RMS, the per-frame outputs
// Every sum has a fixed order: two calls give the same bits. FP64 throughout; nothing is indexed at run time in registers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/calico_hip.h"
#include "arrowhead_dev.hpp"
#include "imu_align_dev.hpp"
#include "kernels.hpp"
#include "point_lm_dev.hpp"

namespace cal {

constexpr int kCamAlignWaves = 4;                // frames per workgroup of the evaluation
constexpr int kCamAlignEvalThreads = 64 * kCamAlignWaves;
constexpr int kCamAlignWavesPerSimd = 2;         // the register budget asked of the compiler: 256 VGPRs
constexpr int kCamAlignPoseWaves = kCamAlignThreads / 64;
// a score curve whose range is below this fraction of its maximum -- or of 1, the score's unit (rad^2), where the maximum itself
// is rounding -- is flat: a rig at rest
constexpr double kCamAlignFlat = 1e-12;

namespace {

DEV Q4 quat_conj(Q4 q) { q.x = -q.x; q.y = -q.y; q.z = -q.z; return q; }

// The rig's pose at the time t in the segment seg (the STAMP's, align_segment: t = stamp - latency may lie beyond its knots):
// R_rw, t_wr and, with RATE, omega = J(phi) phi' and t_wr'.
template <bool RATE>
DEV void rig_pose(const AlignSpline& sp, int seg, double t, Q4* q_rw, V3* t_wr, V3* omega, V3* t_wr_dot) {
  double p[RATE ? 2 : 1][6];
  align_pose<RATE ? 2 : 1, 6>(sp, seg, t, p);
  *q_rw = angle_axis_to_quat(mk(-p[0][0], -p[0][1], -p[0][2]));
  *t_wr = mk(p[0][3], p[0][4], p[0][5]);
  if constexpr (RATE) {
    V3 unused;
    align_rates<false>(mk(p[0][0], p[0][1], p[0][2]), mk(p[RATE ? 1 : 0][0], p[RATE ? 1 : 0][1], p[RATE ? 1 : 0][2]), mk(0.0, 0.0, 0.0), omega, &unused);
    *t_wr_dot = mk(p[RATE ? 1 : 0][3], p[RATE ? 1 : 0][4], p[RATE ? 1 : 0][5]);
  }
}

// the 14 sums as a symmetric 4 x 4 matrix in (x, y, z, w)
DEV void qq_matrix(const double* g, double (&A)[4][4]) {
  A[0][0] = g[0]; A[0][1] = g[1]; A[0][2] = g[2]; A[0][3] = g[3];
  A[1][1] = g[4]; A[1][2] = g[5]; A[1][3] = g[6];
  A[2][2] = g[7]; A[2][3] = g[8];
  A[3][3] = g[9];
#pragma unroll
  for (int r = 1; r < 4; ++r)
#pragma unroll
    for (int col = 0; col < r; ++col) A[r][col] = A[col][r];
}

}  // namespace

// ---- after the resection -------------------------------------------------------------------------------------------------------
// One wave: lane l takes the frames l, l + 64, ...; then the wave sum.
__global__ __launch_bounds__(64) void camalign_gate_kernel(CamAlignArgs a) {
  CamAlignControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  double d2 = 0.0;
  int n = 0;
  for (int f = lane; f < a.n_frames; f += 64) {
    const uint8_t st = a.resect_status[f];
    const bool ok = st == CALICO_RESECT_OK;
    const double x = a.t_cm[3 * size_t(f)], y = a.t_cm[3 * size_t(f) + 1], z = a.t_cm[3 * size_t(f) + 2];
    a.active[f] = ok ? 1 : 0;
    a.frame_status[f] = st;
    d2 += ok ? x * x + y * y + z * z : 0.0;
    n += ok ? 1 : 0;
  }
  d2 = wave_sum(d2);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
  if (lane == 0) {
    c->frames_used = n;
    c->d2 = n > 0 ? d2 / double(n) : 0.0;
    if (n < a.min_frames) { c->lm.status = CALICO_ALIGN_TOO_FEW_SAMPLES; c->lm.done = 1; }
    else if (!(c->d2 > 0.0) || !__builtin_isfinite(c->d2)) { c->lm.status = CALICO_ALIGN_DEGENERATE; c->lm.done = 1; }
  }
}

// ---- stages A and B: the pose sums ---------------------------------------------------------------------------------------------
// single: one latency, the candidate's (slot 1: the coarse latency, or the start's), instead of the grid.
__global__ __launch_bounds__(kCamAlignThreads) void camalign_pose_kernel(CamAlignArgs a, int single) {
  __shared__ double s_part[kCamAlignPoseWaves][kCamAlignLagTile][kCamAlignPoseSums];
  const CamAlignControl* const c = a.ctrl;
  if (c->lm.done != 0) return;      // (the whole workgroup)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * kCamAlignThreads + threadIdx.x;
  const bool in = i < a.n_frames && a.active[i < a.n_frames ? i : 0] != 0;
  const AlignSpline& sp = a.spline;
  const int n_lags = single ? 1 : a.n_lags;
  const double stamp = in ? a.stamps[i] : 0.0;
  const int seg = in ? align_segment(sp, stamp) : -1;      // (>= 0: the host let no other frame in)
  // T_world_camera of the frame: q_wc = q_wm conj(q_cm), c_w = R_wm (-R_cm^T t_cm) + t_wm
  Q4 q_wc; q_wc.x = q_wc.y = q_wc.z = 0.0; q_wc.w = 1.0;
  V3 c_w = mk(0.0, 0.0, 0.0);
  if (in) {
    const Q4 q_cm = normalized(quat_at(a.q_cm + 4 * size_t(i))), q_wm = quat_at(a.q_wm);
    const V3 t_cm = mk(a.t_cm[3 * size_t(i)], a.t_cm[3 * size_t(i) + 1], a.t_cm[3 * size_t(i) + 2]);
    q_wc = quat_mul(q_wm, quat_conj(q_cm));
    c_w = mul(rotmat(q_wm), -mulT(rotmat(q_cm), t_cm)) + mk(a.t_wm[0], a.t_wm[1], a.t_wm[2]);
  }
  const int l0 = blockIdx.y * kCamAlignLagTile;
#pragma unroll 1
  for (int j = 0; j < kCamAlignLagTile; ++j) {
    const int l = l0 + j;
    double v[kCamAlignPoseSums];
#pragma unroll
    for (int e = 0; e < kCamAlignPoseSums; ++e) v[e] = 0.0;
    if (seg >= 0 && l < n_lags) {
      const double tau = single ? c->latency[1] : a.lags[l];
      Q4 q_rw;
      V3 t_wr, unused0, unused1;
      rig_pose<false>(sp, seg, stamp - tau, &q_rw, &t_wr, &unused0, &unused1);
      const Q4 q = normalized(quat_mul(q_rw, q_wc));
      const V3 t = mul(rotmat(q_rw), c_w - t_wr);
      v[0] = q.x * q.x; v[1] = q.x * q.y; v[2] = q.x * q.z; v[3] = q.x * q.w; v[4] = q.y * q.y; v[5] = q.y * q.z; v[6] = q.y * q.w;
      v[7] = q.z * q.z; v[8] = q.z * q.w; v[9] = q.w * q.w;
      v[10] = t.x; v[11] = t.y; v[12] = t.z; v[13] = dot(t, t);
    }
#pragma unroll
    for (int e = 0; e < kCamAlignPoseSums; ++e) {
      const double t = align_wave_sum(v[e]);
      if (lane == 0) s_part[wave][j][e] = t;
    }
  }
  __syncthreads();
  if (threadIdx.x < kCamAlignLagTile * kCamAlignPoseSums) {
    const int j = threadIdx.x / kCamAlignPoseSums, e = threadIdx.x - kCamAlignPoseSums * j, l = l0 + j;
    if (l < n_lags) {
      double t = s_part[0][j][e];
#pragma unroll
      for (int w = 1; w < kCamAlignPoseWaves; ++w) t += s_part[w][j][e];
      a.pose_part[(size_t(blockIdx.x) * n_lags + l) * kCamAlignPoseSums + e] = t;
    }
  }
}

__global__ __launch_bounds__(kCamAlignThreads) void camalign_peak_kernel(CamAlignArgs a, int n_chunks) {
  __shared__ double s_curve[kAlignMaxLags];
  CamAlignControl* const c = a.ctrl;
  if (c->lm.done != 0) return;
  const double n = double(c->frames_used), d2 = c->d2;
  for (int l = threadIdx.x; l < a.n_lags; l += kCamAlignThreads) {
    double g[kCamAlignPoseSums];
#pragma unroll
    for (int e = 0; e < kCamAlignPoseSums; ++e) g[e] = 0.0;
    for (int ch = 0; ch < n_chunks; ++ch) {
      const double* const p = a.pose_part + (size_t(ch) * a.n_lags + l) * kCamAlignPoseSums;
#pragma unroll
      for (int e = 0; e < kCamAlignPoseSums; ++e) g[e] += p[e];
    }
    double A[4][4], V[4][4];
    qq_matrix(g, A);
    align_jacobi<4>(A, V);
    const double top = fmax(fmax(A[0][0], A[1][1]), fmax(A[2][2], A[3][3]));
    const double mx = g[10] / n, my = g[11] / n, mz = g[12] / n;
    const double score = 4.0 * (1.0 - top / n) + (g[13] / n - (mx * mx + my * my + mz * mz)) / d2;
    s_curve[l] = score;
    a.curve[l] = score;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int peak = 0;
  double best = s_curve[0], worst = s_curve[0];
  bool finite = __builtin_isfinite(s_curve[0]);
  for (int l = 1; l < a.n_lags; ++l) {
    const double r = s_curve[l];
    finite = finite && __builtin_isfinite(r);
    if (r < best) { best = r; peak = l; }
    worst = fmax(worst, r);
  }
  c->peak_index = peak;
  c->peak_score = best;
  const bool flat = !finite || !(worst - best > kCamAlignFlat * fmax(worst, 1.0));
  if (flat || peak == 0 || peak == a.n_lags - 1) {
    c->coarse_latency = a.lags[peak];
    c->lm.status = CALICO_ALIGN_NO_PEAK;
    c->lm.done = 1;
    return;
  }
  const double ym = s_curve[peak - 1], yp = s_curve[peak + 1], den = ym - 2.0 * best + yp;
  const double off = den > 0.0 ? 0.5 * (ym - yp) / den : 0.0;
  const double coarse = a.lags[peak] + off * a.lag_step;
  c->coarse_latency = coarse;
  c->latency[0] = coarse; c->latency[1] = coarse;
}

__global__ __launch_bounds__(64) void camalign_mean_kernel(CamAlignArgs a, int n_chunks) {
  __shared__ double s_g[16];
  CamAlignControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  if (c->lm.done != 0) return;
  if (lane < kCamAlignPoseSums) {
    double s = 0.0;
    for (int ch = 0; ch < n_chunks; ++ch) s += a.pose_part[size_t(ch) * kCamAlignPoseSums + lane];
    s_g[lane] = s;
  }
  wave_fence();
  double g[kCamAlignPoseSums];
#pragma unroll
  for (int e = 0; e < kCamAlignPoseSums; ++e) g[e] = s_g[e];
  double A[4][4], V[4][4];
  qq_matrix(g, A);
  align_jacobi<4>(A, V);
  double best = A[0][0];
  Q4 q; q.x = V[0][0]; q.y = V[1][0]; q.z = V[2][0]; q.w = V[3][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    const bool take = A[j][j] > best;
    best = take ? A[j][j] : best;
    q.x = take ? V[0][j] : q.x; q.y = take ? V[1][j] : q.y; q.z = take ? V[2][j] : q.z; q.w = take ? V[3][j] : q.w;
  }
  q = canonical(q);
  const double n = double(c->frames_used);
  const V3 t = mk(g[10] / n, g[11] / n, g[12] / n);
  if (lane == 0) {
    c->q[1][0] = q.x; c->q[1][1] = q.y; c->q[1][2] = q.z; c->q[1][3] = q.w;
    if ((a.free_bits & 0x38u) != 0u) { c->t[1][0] = t.x; c->t[1][1] = t.y; c->t[1][2] = t.z; }
    if (!finite_pose(q, t)) { c->lm.status = CALICO_ALIGN_DEGENERATE; c->lm.done = 1; }
  }
}

// ---- stage C -------------------------------------------------------------------------------------------------------------------
// The candidate (the slot that is not the current one) over the pairs of one frame per wave: the upper triangle of the Gram
// matrix of the rows sqrt(w) [J | r] / sigma (rotation 3, translation 3, latency 1, residual), the cost, Sum |e|^2, the valid
// pairs, the cost's rounding scale Sum |e_u| |u| + |e_v| |v|, the cost over the pairs valid at the current point and the pairs
// that the candidate lost, into the frame's own record.
template <int MODEL>
__global__ __launch_bounds__(kCamAlignEvalThreads, kCamAlignWavesPerSimd) void camalign_eval_kernel(CamAlignArgs a) {
  constexpr int N = 8;
  __shared__ double s_x[kCamAlignWaves][64 * N];      // the wave's staging area: 64 rows of N columns
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(int(threadIdx.x >> 6));
  const int f = int(blockIdx.x) * kCamAlignWaves + wave;
  if (f >= a.n_frames) return;      // (the whole wave: no barrier follows)
  const CamAlignControl* const c = a.ctrl;
  if (c->lm.done != 0 || a.active[f] == 0) return;
  const int cur = c->lm.cur, nxt = cur ^ 1;
  const bool first = c->lm.first != 0;
  const AlignSpline& sp = a.spline;
  // the frame's pose and its time derivative: wave-uniform
  Q4 q_rw;
  V3 t_wr, omega, t_wr_dot;
  const double stamp = a.stamps[f];
  const int seg = align_segment(sp, stamp);
  if (seg < 0) return;      // (the host let no such frame in)
  rig_pose<true>(sp, seg, stamp - c->latency[nxt], &q_rw, &t_wr, &omega, &t_wr_dot);
  const M3 R_rw = rotmat(q_rw), Rc = rotmat(quat_at(c->q[nxt]));
  const M3 R_rm = mul(R_rw, rotmat(quat_at(a.q_wm)));
  const V3 t_rm = mul(R_rw, mk(a.t_wm[0], a.t_wm[1], a.t_wm[2]) - t_wr), vel = mul(R_rw, t_wr_dot);
  const V3 t_rc = mk(c->t[nxt][0], c->t[nxt][1], c->t[nxt][2]);
  const int64_t base = a.offsets[f], n = a.offsets[f + 1] - base;
  const double hs = a.huber_scale, hs2 = hs * hs, is = a.inv_sigma;
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
      const V3 y = mul(R_rm, P) + t_rm, z = y - t_rc, Pc = mulT(Rc, z);
      const V3 ydot = cross(omega, y) - vel;
      double pix[2] = {0.0, 0.0}, D[2][3], dK[2][kMaxIntr];
      ok = project<MODEL, true>(a.k, Pc, pix, D, dK);
      ok = ok && __builtin_isfinite(pix[0]) && __builtin_isfinite(pix[1]);
      a.flags[i] = uint8_t((fl & ~pose_bit(nxt)) | (ok ? pose_bit(nxt) : 0));
      if (ok) {
        const double e[2] = {u - pix[0], w_ - pix[1]}, sq = e[0] * e[0] + e[1] * e[1];
        double w, rho;
        huber(sq, hs, hs2, &w, &rho);
        const double sw = sqrt(w) * is;
        // r = e / sigma; for R_rc <- exp([d]x) R_rc: d x_c = R_rc^T ([z]x d - dt), and d y / d latency = -(omega x y - R_rw t_wr'):
        // with dd = R_rc D_r^T, row r is [z x dd, dd, dd . (omega x y - R_rw t_wr'), e_r]
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const V3 dd = mul(Rc, mk(D[r][0], D[r][1], D[r][2])), cz = cross(z, dd);
          x[r][0] = sw * cz.x; x[r][1] = sw * cz.y; x[r][2] = sw * cz.z; x[r][3] = sw * dd.x; x[r][4] = sw * dd.y; x[r][5] = sw * dd.z;
          x[r][6] = sw * dot(dd, ydot);
          x[r][7] = sw * e[r];
        }
        const double is2 = is * is;
        s_cost += rho * is2; s_ss += sq; s_noise += (dabs(e[0] * pix[0]) + dabs(e[1] * pix[1])) * is2;
        if (was) s_common += rho * is2;
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
  double* const fr = a.frames + size_t(f) * kCamAlignFrameDoubles;
  double* const ns = fr + kCamAlignSums * nxt;
  // the accumulator tile's upper triangle (C/D layout: col = lane & 15, row = (lane >> 4) + 4 reg)
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int row = lk + 4 * r;
    if (lc < N && row <= lc) ns[GramTriangle8::at(row, lc)] = acc[r];
  }
  s_cost = wave_sum(s_cost); s_common = wave_sum(s_common); s_ss = wave_sum(s_ss); s_noise = wave_sum(s_noise);
  if (lane == 0) {
    ns[kCamAlignCostAt] = s_cost; ns[kCamAlignSsAt] = s_ss; ns[kCamAlignValidAt] = double(n_valid); ns[kCamAlignNoiseAt] = s_noise;
    fr[kCamAlignCommonAt] = s_common; fr[kCamAlignLostAt] = double(lost);
  }
}

// One wave: the candidate's records added in frame order (lane e adds entry e), then point_lm_dev.hpp's iteration: the decision
// (lm_rule.hpp's lm_loop_decision; the camera's own: the cost over the pairs valid at both points is what is compared, a start
// without a valid pair is a bad one, and the cost is a sum of rho, not half of it), the damped 7 x 7 step from the point that is
// current afterwards, and the next candidate.
__global__ __launch_bounds__(64) void camalign_decide_kernel(CamAlignArgs a) {
  __shared__ double s_g[kCamAlignSums + 2];
  __shared__ double s_h[49];
  __shared__ double s_b[8];
  CamAlignControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  if (c->lm.done != 0) return;
  const int cur = c->lm.cur, nxt = cur ^ 1;
  if (lane < kCamAlignSums + 2) {
    const int at = lane < kCamAlignSums ? kCamAlignSums * nxt + lane : kCamAlignCommonAt + (lane - kCamAlignSums);
    double s = 0.0;
    for (int f = 0; f < a.n_frames; ++f) {
      const double v = a.frames[size_t(f) * kCamAlignFrameDoubles + at];
      s += a.active[f] != 0 ? v : 0.0;
    }
    s_g[lane] = s;
    if (lane < kCamAlignSums) c->G[nxt][lane] = s;
  }
  wave_fence();
  const double cand = s_g[kCamAlignCostAt], common = s_g[kCamAlignSums], lost = s_g[kCamAlignSums + 1];
  const double current = c->G[cur][kCamAlignCostAt], noise = c->G[cur][kCamAlignNoiseAt];
  const bool kept = lost == 0.0 && __builtin_isfinite(cand) && point_lm_finite(c->q[nxt], 4) && point_lm_finite(c->t[nxt], 3) && point_lm_finite(&c->latency[nxt], 1);
  PointLmState st = point_lm_state(c->lm, lm_loop_decision(c->lm.first != 0, kept, s_g[kCamAlignValidAt] >= 1.0, common, current, noise,
                                                           c->lm.step < a.step_tolerance, c->lm.lambda, c->lm.iterations, a.max_iterations), 0.5 * cand);
  double step = 0.0;
  if (st.done == 0) {
    point_lm_restore(s_g, c->G[cur], kCamAlignSums, st.cur != nxt, lane);
    if (point_lm_damped_step(GramTriangle8{s_g}, 7, a.free_bits, &st, s_h, s_b, lane)) {
      const int at = st.cur, to = at ^ 1;
      step = point_lm_step_size(point_lm_rotate(c->q[at], s_b, false, c->q[to], lane), point_lm_add3(c->t[at], s_b + 3, c->t[to], lane),
                                point_lm_add1(c->latency[at], s_b[6], &c->latency[to], lane));
    }
  }
  point_lm_write(&c->lm, lane, st, step);
}

// One wave: the undamped inverse normal matrix at the result (zero rows and columns for what is not estimated), the RMS, and
// every frame's RMS and valid pairs.
__global__ __launch_bounds__(64) void camalign_final_kernel(CamAlignArgs a) {
  __shared__ double s_g[kCamAlignSums];
  __shared__ double s_h[49];
  __shared__ double s_b[8];
  CamAlignControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  const bool ran = point_lm_ran(c->lm.status) && c->lm.first == 0;
  const int cur = c->lm.cur;
  for (int f = lane; f < a.n_frames; f += 64) {
    const double* const cs = a.frames + size_t(f) * kCamAlignFrameDoubles + kCamAlignSums * cur;
    const bool act = ran && a.active[f] != 0 && cs[kCamAlignValidAt] >= 1.0;
    a.frame_rms_out[f] = act ? sqrt(cs[kCamAlignSsAt] / cs[kCamAlignValidAt]) : 0.0;
    a.frame_n_used_out[f] = act ? int(cs[kCamAlignValidAt]) : 0;
  }
  if (!ran) return;
  if (lane < kCamAlignSums) s_g[lane] = c->G[cur][lane];
  wave_fence();
  point_lm_finish(&c->lm, GramTriangle8{s_g}, 7, a.free_bits, 0.5 * s_g[kCamAlignCostAt], s_h, s_b, c->cov, lane);
  if (lane == 0) {
    c->rms = sqrt(s_g[kCamAlignSsAt] / s_g[kCamAlignValidAt]);
    c->pairs_used = (long long)s_g[kCamAlignValidAt];
  }
}

// ---- launches ------------------------------------------------------------------------------------------------------------------
int camalign_chunks(int n) { return n > 0 ? (n + kCamAlignThreads - 1) / kCamAlignThreads : 0; }

hipError_t launch_camalign_gate(const CamAlignArgs& a, hipStream_t s) {
  if (a.n_frames <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(camalign_gate_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_camalign_search(const CamAlignArgs& a, hipStream_t s) {
  const int chunks = camalign_chunks(a.n_frames);
  if (chunks == 0 || a.n_lags <= 0 || a.n_lags > kAlignMaxLags) return hipErrorInvalidValue;
  hipLaunchKernelGGL(camalign_pose_kernel, dim3(unsigned(chunks), unsigned((a.n_lags + kCamAlignLagTile - 1) / kCamAlignLagTile)),
                     dim3(kCamAlignThreads), 0, s, a, 0);
  hipLaunchKernelGGL(camalign_peak_kernel, dim3(1), dim3(kCamAlignThreads), 0, s, a, chunks);
  return hipGetLastError();
}

hipError_t launch_camalign_mean(const CamAlignArgs& a, hipStream_t s) {
  const int chunks = camalign_chunks(a.n_frames);
  if (chunks == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(camalign_pose_kernel, dim3(unsigned(chunks), 1u), dim3(kCamAlignThreads), 0, s, a, 1);
  hipLaunchKernelGGL(camalign_mean_kernel, dim3(1), dim3(64), 0, s, a, chunks);
  return hipGetLastError();
}

hipError_t launch_camalign_iteration(int model, const CamAlignArgs& a, hipStream_t s) {
  if (a.n_frames <= 0) return hipErrorInvalidValue;
  const dim3 grid(unsigned((a.n_frames + kCamAlignWaves - 1) / kCamAlignWaves)), block(kCamAlignEvalThreads);
  const hipError_t e = with_camera_model(model, [&](auto m) { hipLaunchKernelGGL(camalign_eval_kernel<decltype(m)::value>, grid, block, 0, s, a); });
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(camalign_decide_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_camalign_finish(const CamAlignArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(camalign_final_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace cal
