// align_kernels.hip — camera-IMU alignment on the device: the rotation rig <- gyroscope, the gyroscope's bias,
// the IMU's latency and the world's gravity from a fitted trajectory and the raw IMU samples, as a start for the batch solve.
// The model is the optimiser's own (GyroscopeResidual / AccelerometerResidual with the scale-and-bias model at scale 1):
//   t = stamp - latency,  phi = -pose[0:3](t),  omega = J(phi) phi',  prediction = -R(q_rig_gyro)^T omega + bias;
// the latency column is the exact d omega / d t (align_omega_dot), as the optimiser has it.
// Stages, one after the other on the stream, steered by the control word (AlignControl, kernels.hpp) without a host read:
//   A  align_corr_kernel        sample chunks x lag tiles: Sum a, Sum a^2, Sum a m per (chunk, lag), a = |omega(stamp - lag)|, m = |measured|
//      align_corr_peak_kernel   one workgroup: the chunks added in order, the normalised centred correlation per lag, its peak
//                               and the parabola through the three points around it
//   B  align_horn_sums_kernel   per workgroup the 21 sums of u = -omega and v = measured
//      align_horn_kernel        one wave: Horn's quaternion from the (centred) cross-covariance by cyclic Jacobi, the bias
//   C  align_eval_kernel        one lane per sample: the 8-column Gram matrix of [J r] per workgroup (rotation 3, bias 3, latency 1)
//      align_decide_kernel      one wave: the workgroups added in order, accept / reject, the damped 7 x 7 step, the next candidate
//      align_final_kernel       one wave: the undamped inverse normal matrix and the RMS at the result
//   D  align_accel_kernel       per workgroup the sums of the normal equations in (gravity, bias), then of the residual and A^T residual
//      align_accel_solve_kernel one wave: the 6 x 6 (3 x 3) Cholesky solve, one step of iterative refinement, the RMS
// Every sum has a fixed order (a butterfly inside the wave, the waves of a workgroup in order, the workgroups in order): two
// calls give the same bits. FP64 throughout; nothing is indexed at run time in registers (no scratch).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/calico_hip.h"
#include "imu_align_dev.hpp"
#include "kernels.hpp"
#include "point_lm_dev.hpp"
#include "resect_dev.hpp"

namespace cal {

namespace {

constexpr int kAlignWaves = kAlignThreads / 64;
// a variance below this fraction of the raw second moment is rounding: the signal is constant
constexpr double kAlignZeroVariance = 1e-12;
// rotation about one axis only: the second eigenvalue of the scatter of omega_rig against the first
constexpr double kAlignMinPivot = 1e-6;

// The workgroup's sums of v[0 .. NV) to out[0 .. NV): the wave's butterfly, then the waves in order. Every thread of the
// workgroup calls it.
template <int NV>
DEV void align_block_sum(const double (&v)[NV], double (*s_w)[kAlignPart], double* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < NV; ++e) {
    const double t = align_wave_sum(v[e]);
    if (lane == 0) s_w[wave][e] = t;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = s_w[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kAlignWaves; ++w) t += s_w[w][threadIdx.x];
    out[threadIdx.x] = t;
  }
}

// omega_rig of a sample at the latency tau and, with DOT, its exact time derivative. As in the optimiser the segment is the
// STAMP's (Trajectory::GetEvaluationParams looks it up before the latency is taken off): its polynomial is evaluated at
// stamp - tau, beyond its own knots where the latency carries the time there. false: the stamp lies outside the valid knots.
template <bool DOT>
DEV bool gyro_rates(const AlignSpline& sp, double stamp, double tau, V3* omega, V3* omega_dot) {
  const double t = stamp - tau;
  const int seg = align_segment(sp, stamp);
  if (seg < 0) return false;
  double p[DOT ? 3 : 2][3];
  align_pose<DOT ? 3 : 2, 3>(sp, seg, t, p);
  const V3 p0 = mk(p[0][0], p[0][1], p[0][2]), p1 = mk(p[1][0], p[1][1], p[1][2]);
  V3 unused;
  align_rates<false>(p0, p1, mk(0.0, 0.0, 0.0), omega, &unused);
  if constexpr (DOT) *omega_dot = align_omega_dot(p0, p1, mk(p[DOT ? 2 : 0][0], p[DOT ? 2 : 0][1], p[DOT ? 2 : 0][2]));
  return true;
}

}  // namespace

// ---- stage A -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAlignThreads) void align_corr_kernel(AlignArgs a) {
  __shared__ double s_part[kAlignWaves][kAlignLagTile][3];
  __shared__ double s_m[kAlignWaves][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * kAlignThreads + threadIdx.x;
  const bool in = i < a.n;
  const AlignSpline& sp = a.spline;
  const double stamp = in ? a.stamps[i] : 0.0;
  double m = 0.0;
  if (in) { const double x = a.meas[3 * size_t(i)], y = a.meas[3 * size_t(i) + 1], z = a.meas[3 * size_t(i) + 2]; m = sqrt(x * x + y * y + z * z); }
  const int l0 = blockIdx.y * kAlignLagTile;
#pragma unroll 1
  for (int j = 0; j < kAlignLagTile; ++j) {
    const int l = l0 + j;
    double w = 0.0;
    if (in && l < a.n_lags) {
      V3 omega, alpha;
      if (gyro_rates<false>(sp, stamp, a.lags[l], &omega, &alpha)) w = sqrt(dot(omega, omega));
    }
    const double sa = align_wave_sum(w), saa = align_wave_sum(w * w), sam = align_wave_sum(w * m);
    if (lane == 0) { s_part[wave][j][0] = sa; s_part[wave][j][1] = saa; s_part[wave][j][2] = sam; }
  }
  {
    const double sm = align_wave_sum(m), smm = align_wave_sum(m * m);
    if (lane == 0) { s_m[wave][0] = sm; s_m[wave][1] = smm; }
  }
  __syncthreads();
  if (threadIdx.x < kAlignLagTile * 3) {
    const int j = threadIdx.x / 3, e = threadIdx.x - 3 * j, l = l0 + j;
    if (l < a.n_lags) {
      double t = s_part[0][j][e];
#pragma unroll
      for (int w = 1; w < kAlignWaves; ++w) t += s_part[w][j][e];
      a.corr_part[(size_t(blockIdx.x) * a.n_lags + l) * 3 + e] = t;
    }
  }
  if (blockIdx.y == 0 && threadIdx.x < 2) {
    double t = s_m[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kAlignWaves; ++w) t += s_m[w][threadIdx.x];
    a.corr_m[size_t(blockIdx.x) * 2 + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(kAlignThreads) void align_corr_peak_kernel(AlignArgs a, int n_chunks) {
  __shared__ double s_curve[kAlignMaxLags];
  AlignControl* const c = a.ctrl;
  const double n = double(a.n);
  double sm = 0.0, smm = 0.0;
  for (int ch = 0; ch < n_chunks; ++ch) { sm += a.corr_m[size_t(ch) * 2]; smm += a.corr_m[size_t(ch) * 2 + 1]; }
  const double vm = smm - sm * sm / n;
  int flat = !(vm > kAlignZeroVariance * smm);
  for (int l = threadIdx.x; l < a.n_lags; l += kAlignThreads) {
    double sa = 0.0, saa = 0.0, sam = 0.0;
    for (int ch = 0; ch < n_chunks; ++ch) {
      const double* const p = a.corr_part + (size_t(ch) * a.n_lags + l) * 3;
      sa += p[0]; saa += p[1]; sam += p[2];
    }
    const double va = saa - sa * sa / n;
    const bool zero = !(va > kAlignZeroVariance * saa) || !(vm > kAlignZeroVariance * smm);
    const double r = zero ? 0.0 : (sam - sa * sm / n) / sqrt(va * vm);
    flat |= zero ? 1 : 0;
    s_curve[l] = r;
    a.curve[l] = r;
  }
  flat = __syncthreads_or(flat);
  if (threadIdx.x != 0) return;
  int peak = 0;
  double best = s_curve[0];
  for (int l = 1; l < a.n_lags; ++l) { const double r = s_curve[l]; if (r > best) { best = r; peak = l; } }
  c->peak_index = peak;
  c->peak_correlation = best;
  if (flat || peak == 0 || peak == a.n_lags - 1) {
    c->coarse_latency = a.lags[peak];
    c->lm.status = CALICO_ALIGN_NO_PEAK;
    c->lm.done = 1;
    return;
  }
  const double ym = s_curve[peak - 1], yp = s_curve[peak + 1], den = ym - 2.0 * best + yp;
  const double off = den < 0.0 ? 0.5 * (ym - yp) / den : 0.0;
  const double coarse = a.lags[peak] + off * a.lag_step;
  c->coarse_latency = coarse;
  c->latency[0] = coarse; c->latency[1] = coarse;
}

// ---- stage B -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kAlignThreads) void align_horn_sums_kernel(AlignArgs a) {
  __shared__ double s_w[kAlignWaves][kAlignPart];
  const AlignControl* const c = a.ctrl;
  if (c->lm.done != 0) return;
  const double tau = c->latency[1];
  const int i = blockIdx.x * kAlignThreads + threadIdx.x;
  const AlignSpline& sp = a.spline;
  double v[kAlignHornSums];
#pragma unroll
  for (int e = 0; e < kAlignHornSums; ++e) v[e] = 0.0;
  if (i < a.n) {
    V3 omega, alpha;
    if (gyro_rates<false>(sp, a.stamps[i], tau, &omega, &alpha)) {
      const double u[3] = {-omega.x, -omega.y, -omega.z};
      const double m[3] = {a.meas[3 * size_t(i)], a.meas[3 * size_t(i) + 1], a.meas[3 * size_t(i) + 2]};
#pragma unroll
      for (int j = 0; j < 3; ++j) { v[j] = u[j]; v[3 + j] = m[j]; }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int col = 0; col < 3; ++col) v[6 + 3 * r + col] = m[r] * u[col];
      v[15] = u[0] * u[0]; v[16] = u[0] * u[1]; v[17] = u[0] * u[2]; v[18] = u[1] * u[1]; v[19] = u[1] * u[2]; v[20] = u[2] * u[2];
    }
  }
  align_block_sum<kAlignHornSums>(v, s_w, a.part + size_t(blockIdx.x) * kAlignPart);
}

__global__ __launch_bounds__(64) void align_horn_kernel(AlignArgs a, int n_chunks) {
  __shared__ double s_g[kAlignPart];
  AlignControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  if (c->lm.done != 0) return;
  if (lane < kAlignHornSums) {
    double s = 0.0;
    for (int ch = 0; ch < n_chunks; ++ch) s += a.part[size_t(ch) * kAlignPart + lane];
    s_g[lane] = s;
  }
  wave_fence();
  const bool centre = ((a.free_bits >> 3) & 7u) != 0u;
  const double n = double(a.n), in = centre ? 1.0 / n : 0.0;
  const double su[3] = {s_g[0], s_g[1], s_g[2]}, sv[3] = {s_g[3], s_g[4], s_g[5]};
  double S[3][3];      // Sum v u^T: S[r][c] = v_r u_c
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int col = 0; col < 3; ++col) S[r][col] = s_g[6 + 3 * r + col] - sv[r] * su[col] * in;
  double U[3][3], UV[3][3];
  U[0][0] = s_g[15] - su[0] * su[0] * in; U[0][1] = s_g[16] - su[0] * su[1] * in; U[0][2] = s_g[17] - su[0] * su[2] * in;
  U[1][1] = s_g[18] - su[1] * su[1] * in; U[1][2] = s_g[19] - su[1] * su[2] * in; U[2][2] = s_g[20] - su[2] * su[2] * in;
  U[1][0] = U[0][1]; U[2][0] = U[0][2]; U[2][1] = U[1][2];
  align_jacobi<3>(U, UV);
  const double e0 = U[0][0], e1 = U[1][1], e2 = U[2][2];
  const double emax = fmax(e0, fmax(e1, e2)), emin = fmin(e0, fmin(e1, e2)), emid = (e0 + e1 + e2) - emax - emin;
  const double pivot = emax > 0.0 ? emid / emax : 0.0;
  if (!(pivot >= kAlignMinPivot)) {
    if (lane == 0) { c->scatter_pivot = __builtin_isfinite(pivot) ? pivot : 0.0; c->lm.status = CALICO_ALIGN_DEGENERATE; c->lm.done = 1; }
    return;
  }
  // Horn: the unit quaternion (w, x, y, z) that maximises Sum u . R v is the eigenvector of the largest eigenvalue of N
  double N[4][4], NV[4][4];
  N[0][0] = S[0][0] + S[1][1] + S[2][2]; N[0][1] = S[1][2] - S[2][1]; N[0][2] = S[2][0] - S[0][2]; N[0][3] = S[0][1] - S[1][0];
  N[1][1] = S[0][0] - S[1][1] - S[2][2]; N[1][2] = S[0][1] + S[1][0]; N[1][3] = S[2][0] + S[0][2];
  N[2][2] = -S[0][0] + S[1][1] - S[2][2]; N[2][3] = S[1][2] + S[2][1];
  N[3][3] = -S[0][0] - S[1][1] + S[2][2];
#pragma unroll
  for (int r = 1; r < 4; ++r)
#pragma unroll
    for (int col = 0; col < r; ++col) N[r][col] = N[col][r];
  align_jacobi<4>(N, NV);
  double best = N[0][0];
  double qw = NV[0][0], qx = NV[1][0], qy = NV[2][0], qz = NV[3][0];
#pragma unroll
  for (int j = 1; j < 4; ++j) {
    const bool take = N[j][j] > best;
    best = take ? N[j][j] : best;
    qw = take ? NV[0][j] : qw; qx = take ? NV[1][j] : qx; qy = take ? NV[2][j] : qy; qz = take ? NV[3][j] : qz;
  }
  Q4 q; q.x = qx; q.y = qy; q.z = qz; q.w = qw;
  q = canonical(q);
  const M3 R = rotmat(q);
  const V3 mu = mulT(R, mk(su[0] / n, su[1] / n, su[2] / n));
  const double b[3] = {centre ? sv[0] / n - mu.x : 0.0, centre ? sv[1] / n - mu.y : 0.0, centre ? sv[2] / n - mu.z : 0.0};
  if (lane == 0) {
    c->scatter_pivot = pivot;
    c->q[1][0] = q.x; c->q[1][1] = q.y; c->q[1][2] = q.z; c->q[1][3] = q.w;
    c->bias[1][0] = b[0]; c->bias[1][1] = b[1]; c->bias[1][2] = b[2];
    if (!(__builtin_isfinite(q.x) && __builtin_isfinite(q.y) && __builtin_isfinite(q.z) && __builtin_isfinite(q.w))) {
      c->lm.status = CALICO_ALIGN_DEGENERATE; c->lm.done = 1;
    }
  }
}

// ---- stage C -------------------------------------------------------------------------------------------------------------------
// The candidate (the slot that is not the current one) over all samples: per workgroup the upper triangle of [J r]^T [J r], the
// samples whose residual is not finite, and the cost's rounding scale Sum |r| (|measured| + |prediction|) / sigma.
__global__ __launch_bounds__(kAlignThreads) void align_eval_kernel(AlignArgs a) {
  __shared__ double s_w[kAlignWaves][kAlignPart];
  const AlignControl* const c = a.ctrl;
  if (c->lm.done != 0) return;
  const int slot = c->lm.cur ^ 1;
  Q4 q; q.x = c->q[slot][0]; q.y = c->q[slot][1]; q.z = c->q[slot][2]; q.w = c->q[slot][3];
  const double b[3] = {c->bias[slot][0], c->bias[slot][1], c->bias[slot][2]};
  const double tau = c->latency[slot], is = a.inv_sigma;
  const M3 R = rotmat(q);
  const int i = blockIdx.x * kAlignThreads + threadIdx.x;
  const AlignSpline& sp = a.spline;
  double v[kAlignSums];
#pragma unroll
  for (int e = 0; e < kAlignSums; ++e) v[e] = 0.0;
  if (i < a.n) {
    V3 omega, alpha;
    if (gyro_rates<true>(sp, a.stamps[i], tau, &omega, &alpha)) {
      const V3 w = mulT(R, omega), wa = mulT(R, alpha);
      const double m[3] = {a.meas[3 * size_t(i)], a.meas[3 * size_t(i) + 1], a.meas[3 * size_t(i) + 2]};
      const double pred[3] = {b[0] - w.x, b[1] - w.y, b[2] - w.z};
      // d (R^T omega) / d delta_j = R^T (omega x e_j) for R <- exp([delta]x) R
      const V3 c0 = mulT(R, mk(0.0, omega.z, -omega.y)), c1 = mulT(R, mk(-omega.z, 0.0, omega.x)), c2 = mulT(R, mk(omega.y, -omega.x, 0.0));
      double J[3][8];
      J[0][0] = c0.x * is; J[1][0] = c0.y * is; J[2][0] = c0.z * is;
      J[0][1] = c1.x * is; J[1][1] = c1.y * is; J[2][1] = c1.z * is;
      J[0][2] = c2.x * is; J[1][2] = c2.y * is; J[2][2] = c2.z * is;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int col = 0; col < 3; ++col) J[r][3 + col] = r == col ? -is : 0.0;
      J[0][6] = -wa.x * is; J[1][6] = -wa.y * is; J[2][6] = -wa.z * is;      // d r / d latency = + d prediction / d t
      double noise = 0.0;
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        J[r][7] = (m[r] - pred[r]) * is;
        noise += fabs(J[r][7]) * (fabs(m[r]) + fabs(pred[r])) * is;
      }
      v[kAlignBadAt] = __builtin_isfinite(noise) ? 0.0 : 1.0;
      int e = 0;
#pragma unroll
      for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int col = r; col < 8; ++col) { v[e] = J[0][r] * J[0][col] + J[1][r] * J[1][col] + J[2][r] * J[2][col]; ++e; }
      v[kAlignNoiseAt] = noise;
    }
  }
  align_block_sum<kAlignSums>(v, s_w, a.part + size_t(blockIdx.x) * kAlignPart);
}

// One wave: the candidate's partials added in workgroup order, then point_lm_dev.hpp's iteration: the decision (lm_rule.hpp: a
// candidate within the cost's rounding error is accepted, a small step ends the loop only at low damping), the damped 7 x 7 step
// from the point that is current afterwards, and the next candidate.
__global__ __launch_bounds__(64) void align_decide_kernel(AlignArgs a, int n_chunks) {
  __shared__ double s_g[kAlignPart];
  __shared__ double s_h[49];
  __shared__ double s_b[8];
  AlignControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  if (c->lm.done != 0) return;
  const int cur = c->lm.cur, nxt = cur ^ 1;
  if (lane < kAlignSums) {
    double s = 0.0;
    for (int ch = 0; ch < n_chunks; ++ch) s += a.part[size_t(ch) * kAlignPart + lane];
    s_g[lane] = s;
    c->G[nxt][lane] = s;
  }
  wave_fence();
  const double cand = 0.5 * s_g[kAlignCostAt], lost = s_g[kAlignBadAt];
  const double current = 0.5 * c->G[cur][kAlignCostAt], noise = c->G[cur][kAlignNoiseAt];
  const bool kept = lost == 0.0 && __builtin_isfinite(cand) && point_lm_finite(c->q[nxt], 4) && point_lm_finite(c->bias[nxt], 3) && point_lm_finite(&c->latency[nxt], 1);
  PointLmState st = point_lm_state(c->lm, lm_point_decision(c->lm.first != 0, kept, cand, current, noise, c->lm.step < a.step_tolerance, c->lm.lambda,
                                                            c->lm.iterations, a.max_iterations), cand);
  double step = 0.0;
  if (st.done == 0) {
    point_lm_restore(s_g, c->G[cur], kAlignSums, st.cur != nxt, lane);
    if (point_lm_damped_step(GramTriangle8{s_g}, 7, a.free_bits, &st, s_h, s_b, lane)) {
      const int at = st.cur, to = at ^ 1;
      step = point_lm_step_size(point_lm_rotate(c->q[at], s_b, false, c->q[to], lane), point_lm_add3(c->bias[at], s_b + 3, c->bias[to], lane),
                                point_lm_add1(c->latency[at], s_b[6], &c->latency[to], lane));
    }
  }
  point_lm_write(&c->lm, lane, st, step);
}

// The undamped inverse normal matrix at the result (zero rows and columns for what is not estimated) and the RMS.
__global__ __launch_bounds__(64) void align_final_kernel(AlignArgs a) {
  __shared__ double s_g[kAlignPart];
  __shared__ double s_h[49];
  __shared__ double s_b[8];
  AlignControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  if (!point_lm_ran(c->lm.status) || c->lm.first != 0) return;
  const int cur = c->lm.cur;
  if (lane < kAlignSums) s_g[lane] = c->G[cur][lane];
  wave_fence();
  point_lm_finish(&c->lm, GramTriangle8{s_g}, 7, a.free_bits, 0.5 * s_g[kAlignCostAt], s_h, s_b, c->cov, lane);
  if (lane == 0) c->gyro_rms = sqrt(s_g[kAlignCostAt] / (3.0 * double(a.n)));
}

// ---- stage D -------------------------------------------------------------------------------------------------------------------
// measured = R_a^T (R_rw (a_w - g) + lever) + bias with R_a = R(q_rig_gyro), R_rw = R(phi), lever = (Omega Omega + Alpha) t_ra:
// y = measured - R_a^T (R_rw a_w + lever) = -M g + bias, M = R_a^T R_rw. RESIDUAL = false: the sums of the normal equations;
// true: the residual r = y + M g - bias at the solution: Sum |r|^2, the samples, A^T r.
template <bool RESIDUAL>
__global__ __launch_bounds__(kAlignThreads) void align_accel_kernel(AlignArgs a) {
  __shared__ double s_w[kAlignWaves][kAlignPart];
  const AlignControl* const c = a.ctrl;
  if (!point_lm_ran(c->lm.status)) return;
  if (RESIDUAL && c->accel_status != CALICO_ALIGN_OK) return;
  const int cur = c->lm.cur;
  Q4 q; q.x = c->q[cur][0]; q.y = c->q[cur][1]; q.z = c->q[cur][2]; q.w = c->q[cur][3];
  const double tau = c->latency[cur];
  const M3 Ra = rotmat(q);
  const int i = blockIdx.x * kAlignThreads + threadIdx.x;
  const AlignSpline& sp = a.spline;
  constexpr int NV = RESIDUAL ? kAlignAccelResidual : kAlignAccelSums;
  double v[NV];
#pragma unroll
  for (int e = 0; e < NV; ++e) v[e] = 0.0;
  if (i < a.n_accel) {
    const double t = a.accel_stamps[i] - tau;
    const int seg = align_segment(sp, a.accel_stamps[i]);      // (the stamp's segment, as in the optimiser)
    if (seg >= 0) {
      double p[3][6];
      align_pose<3, 6>(sp, seg, t, p);
      V3 omega, alpha;
      align_rates<true>(mk(p[0][0], p[0][1], p[0][2]), mk(p[1][0], p[1][1], p[1][2]), mk(p[2][0], p[2][1], p[2][2]), &omega, &alpha);
      const M3 Rrw = rotmat(angle_axis_to_quat(mk(-p[0][0], -p[0][1], -p[0][2])));
      const V3 tra = mk(a.t_ra[0], a.t_ra[1], a.t_ra[2]);
      const V3 lever = cross(omega, cross(omega, tra)) - cross(alpha, tra);
      const V3 f0 = mulT(Ra, mul(Rrw, mk(p[2][3], p[2][4], p[2][5])) + lever);
      const M3 M = mul(transpose(Ra), Rrw);
      const V3 y = mk(a.accel[3 * size_t(i)] - f0.x, a.accel[3 * size_t(i) + 1] - f0.y, a.accel[3 * size_t(i) + 2] - f0.z);
      if constexpr (RESIDUAL) {
        const V3 g = mk(c->gravity[0], c->gravity[1], c->gravity[2]);
        const V3 r = y + mul(M, g) - mk(c->accel_bias[0], c->accel_bias[1], c->accel_bias[2]);
        const V3 mtr = mulT(M, r);
        v[0] = dot(r, r); v[1] = 1.0;
        v[2] = -mtr.x; v[3] = -mtr.y; v[4] = -mtr.z; v[5] = r.x; v[6] = r.y; v[7] = r.z;      // A^T r, A = [-M I]
      } else {
        v[0] = 1.0;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int col = 0; col < 3; ++col) v[1 + 3 * r + col] = M.m[r][col];
        const V3 mty = mulT(M, y);
        v[10] = mty.x; v[11] = mty.y; v[12] = mty.z; v[13] = y.x; v[14] = y.y; v[15] = y.z;
      }
    }
  }
  align_block_sum<NV>(v, s_w, a.part + size_t(blockIdx.x) * kAlignPart);
}

namespace {
// the normal matrix of (gravity, bias) (N = 6) or of gravity alone (N = 3) from the sums, factored in place; false: not positive definite
DEV bool accel_factor(const double* sums, int N, double* H, int lane) {
  const double n = sums[0];
  if (lane < N * N) {
    const int i = lane / N, j = lane - N * i;
    double h = i == j ? n : 0.0;
    if (i >= 3 && j < 3) h = -sums[1 + 3 * (i - 3) + j];      // A = [-M I]: the block of (bias_i, g_j) is -M[i][j]
    if (i < 3 && j >= 3) h = -sums[1 + 3 * (j - 3) + i];
    H[lane] = h;
  }
  wave_fence();
  return lds_chol(H, N, lane);
}
}  // namespace

// One wave. mode 0: the sums of the normal equations added in workgroup order, the Cholesky solve. mode 1: one step of iterative
// refinement with A^T (y - A x) summed residual by residual (the normal equations square the condition number; the residual
// pass gives the solve the accuracy of a least-squares solve on A itself). mode 2: the RMS at the refined solution.
__global__ __launch_bounds__(64) void align_accel_solve_kernel(AlignArgs a, int n_chunks, int mode) {
  __shared__ double s_g[kAlignPart];
  __shared__ double s_h[36];
  __shared__ double s_b[8];
  AlignControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  if (!point_lm_ran(c->lm.status)) return;
  if (mode != 0 && c->accel_status != CALICO_ALIGN_OK) return;
  const int NV = mode == 0 ? kAlignAccelSums : kAlignAccelResidual;
  if (lane < NV) {
    double s = 0.0;
    for (int ch = 0; ch < n_chunks; ++ch) s += a.part[size_t(ch) * kAlignPart + lane];
    s_g[lane] = s;
  }
  wave_fence();
  const int N = a.estimate_accel_bias != 0 ? 6 : 3;
  if (mode == 2) {
    if (lane == 0) c->accel_rms = sqrt(s_g[0] / (3.0 * s_g[1]));
  } else if (mode == 1) {
    if (lane < kAlignAccelSums) s_g[8 + lane] = c->accel_sums[lane];
    wave_fence();
    if (!accel_factor(s_g + 8, N, s_h, lane)) return;      // (it was positive definite in mode 0: the same bits)
    if (lane < N) s_b[lane] = s_g[2 + lane];
    wave_fence();
    lds_chol_solve(s_h, s_b, N, lane);
    const bool finite = __builtin_isfinite(s_b[0]) && __builtin_isfinite(s_b[1]) && __builtin_isfinite(s_b[2]);
    if (lane == 0 && finite) {
      c->gravity[0] += s_b[0]; c->gravity[1] += s_b[1]; c->gravity[2] += s_b[2];
      if (N == 6) { c->accel_bias[0] += s_b[3]; c->accel_bias[1] += s_b[4]; c->accel_bias[2] += s_b[5]; }
    }
  } else {
    const double n = s_g[0];
    if (lane == 0) c->accel_samples = (long long)n;
    if (lane < kAlignAccelSums) c->accel_sums[lane] = s_g[lane];
    if (n < double(a.min_samples)) {
      if (lane == 0) c->accel_status = CALICO_ALIGN_TOO_FEW_SAMPLES;
      return;
    }
    const bool pd = accel_factor(s_g, N, s_h, lane);
    if (!pd) {
      if (lane == 0) c->accel_status = CALICO_ALIGN_NOT_POSITIVE_DEFINITE;
      return;
    }
    if (lane < N) s_b[lane] = lane < 3 ? -s_g[10 + lane] : s_g[13 + (lane - 3)];
    wave_fence();
    lds_chol_solve(s_h, s_b, N, lane);
    const bool finite = __builtin_isfinite(s_b[0]) && __builtin_isfinite(s_b[1]) && __builtin_isfinite(s_b[2]);
    if (lane == 0) {
      c->gravity[0] = s_b[0]; c->gravity[1] = s_b[1]; c->gravity[2] = s_b[2];
      c->accel_bias[0] = N == 6 ? s_b[3] : 0.0; c->accel_bias[1] = N == 6 ? s_b[4] : 0.0; c->accel_bias[2] = N == 6 ? s_b[5] : 0.0;
      c->accel_status = finite ? CALICO_ALIGN_OK : CALICO_ALIGN_NOT_POSITIVE_DEFINITE;
    }
  }
}

// ---- launches ------------------------------------------------------------------------------------------------------------------
int align_chunks(int n) { return n > 0 ? (n + kAlignThreads - 1) / kAlignThreads : 0; }

hipError_t launch_align_correlate(const AlignArgs& a, hipStream_t s) {
  const int chunks = align_chunks(a.n);
  if (chunks == 0 || a.n_lags <= 0 || a.n_lags > kAlignMaxLags) return hipErrorInvalidValue;
  hipLaunchKernelGGL(align_corr_kernel, dim3(unsigned(chunks), unsigned((a.n_lags + kAlignLagTile - 1) / kAlignLagTile)), dim3(kAlignThreads), 0, s, a);
  hipLaunchKernelGGL(align_corr_peak_kernel, dim3(1), dim3(kAlignThreads), 0, s, a, chunks);
  return hipGetLastError();
}

hipError_t launch_align_horn(const AlignArgs& a, hipStream_t s) {
  const int chunks = align_chunks(a.n);
  if (chunks == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(align_horn_sums_kernel, dim3(unsigned(chunks)), dim3(kAlignThreads), 0, s, a);
  hipLaunchKernelGGL(align_horn_kernel, dim3(1), dim3(64), 0, s, a, chunks);
  return hipGetLastError();
}

hipError_t launch_align_iteration(const AlignArgs& a, hipStream_t s) {
  const int chunks = align_chunks(a.n);
  if (chunks == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(align_eval_kernel, dim3(unsigned(chunks)), dim3(kAlignThreads), 0, s, a);
  hipLaunchKernelGGL(align_decide_kernel, dim3(1), dim3(64), 0, s, a, chunks);
  return hipGetLastError();
}

hipError_t launch_align_finish(const AlignArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(align_final_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_align_gravity(const AlignArgs& a, hipStream_t s) {
  const int chunks = align_chunks(a.n_accel);
  if (chunks == 0) return hipSuccess;
  hipLaunchKernelGGL(align_accel_kernel<false>, dim3(unsigned(chunks)), dim3(kAlignThreads), 0, s, a);
  hipLaunchKernelGGL(align_accel_solve_kernel, dim3(1), dim3(64), 0, s, a, chunks, 0);
  for (int mode = 1; mode <= 2; ++mode) {
    hipLaunchKernelGGL(align_accel_kernel<true>, dim3(unsigned(chunks)), dim3(kAlignThreads), 0, s, a);
    hipLaunchKernelGGL(align_accel_solve_kernel, dim3(1), dim3(64), 0, s, a, chunks, mode);
  }
  return hipGetLastError();
}

}  // namespace cal
