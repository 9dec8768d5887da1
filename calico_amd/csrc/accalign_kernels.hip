// accalign_kernels.hip — accelerometer alignment on the device: the rotation rig <- accelerometer, its
// lever arm, its bias, the world's gravity and its latency from a fitted trajectory and the raw samples, as a start for the batch
// solve. The model is the optimiser's own AccelerometerResidual with the scale-and-bias model at scale 1 and the trajectory held:
//   t = stamp - latency,  phi = -pose[0:3](t),  omega = J(phi) phi',  alpha = Sum_i (H_i phi') phi'_i + J phi''  (ExpSO3Hessian's
//   closed form, align_rates<true>),  inner = R(phi) (pose''[3:6](t) - g) + omega x (omega x t_ra) - alpha x t_ra,
//   prediction = R_a^T inner + bias,  residual = (measured - prediction) / sigma.
// Parameters: rotation 3 (R_a <- exp([d]x) R_a), lever arm 3, bias 3, gravity 3, latency 1. The latency column is the time
// derivative of that expression as it stands: omega and alpha carry their derivative along t in forward mode (D1) through the
// Rodrigues coefficients, with pose''' from the fourth row of the spline weights; d/dt R(phi) v = omega x R(phi) v + R(phi) v'.
//   accalign_eval_kernel    one lane per sample: the 3 x 14 rows [J | r] of the candidate; the wave stages 64 rows of 16 doubles
//                           (first the x rows, then y, then z) in its LDS area and adds their Gram matrix to one 16 x 16
//                           accumulator tile with v_mfma_f64_16x16x4_f64, 48 steps for a full wave; the waves are added in order
//                           into the workgroup's partial
//   accalign_decide_kernel  one wave: the partials added in workgroup order; stage L (no start of lever arm, bias and gravity):
//                           the 9 x 9 Cholesky solve of their block -- the model is linear in them --, then one refinement step
//                           from a second evaluation; the loop: accept / reject (lm_rule.hpp's lm_point_decision), the damped 13 x 13 step, the
//                           next candidate
//   accalign_final_kernel   one wave: the undamped inverse normal matrix and the RMS at the result
// Every sum has a fixed order (rows in groups of four inside the wave, the waves of a workgroup in order, the workgroups in
// order): two calls give the same bits. FP64 throughout; nothing is indexed at run time in registers (no scratch).
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

constexpr int kAccAlignWaves = kAccAlignThreads / 64;
constexpr int kAccAlignRow = 16;                          // doubles of a staged row: 14 columns and two zeros
constexpr int kAccAlignArea = 64 * kAccAlignRow;          // a wave's staging area: 8 KB
typedef double acc_f64x4 __attribute__((ext_vector_type(4)));

DEV D1 pick(bool c, D1 a, D1 b) { D1 r; r.v = c ? a.v : b.v; r.d = c ? a.d : b.d; return r; }
DEV D1 dual(double v, double d) { D1 r; r.v = v; r.d = d; return r; }

// align_rodrigues<true> (imu_align_dev.hpp: rodrigues' coefficients, every field one select) carrying the derivative along t
DEV Rodrigues<D1> accalign_rodrigues(D1 px, D1 py, D1 pz) {
  Rodrigues<D1> R;
  const D1 t2 = px * px + py * py + pz * pz;
  const bool zero = t2.v == 0.0;
  const D1 th = dsqrt(pick(zero, mk1(1.0), t2));
  D1 st, ct;
  dsincos(th, &st, &ct);
  const bool tiny = th.v < 1e-7;
  st = pick(tiny, small_sin(th), st);
  ct = pick(tiny, small_cos(th), ct);
  const D1 one = mk1(1.0), none = mk1(0.0), it = one / th, it2 = it * it;
  R.zero = zero;
  R.hx = pick(zero, none, it * px); R.hy = pick(zero, none, it * py); R.hz = pick(zero, none, it * pz);
  R.a = pick(zero, none, it * (one - ct));
  R.b = pick(zero, none, it * (th - st));
  R.c0 = pick(zero, none, ct - st * it);
  R.c1 = pick(zero, none, (one - ct) * it2);
  R.c2 = pick(zero, none, mk1(3.0) * it2 * st - it * (ct - mk1(2.0)));
  R.c3 = pick(zero, none, it2 * (th - st));
  return R;
}

// The 16 x 16 tile += X^T X of the 64 staged rows X (row-major, kAccAlignRow doubles each): step u takes the rows 4 u .. 4 u + 3,
// lane (l16, lk) supplies X[4 u + lk][l16] as both operands. All sixteen operands are read before the first product is issued.
DEV acc_f64x4 gram_rows(const double* area, int lane, acc_f64x4 acc) {
  const double* const p = area + (lane >> 4) * kAccAlignRow + (lane & 15);
  double v[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) v[u] = p[4 * u * kAccAlignRow];
#pragma unroll
  for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(v[u], v[u], acc, 0, 0, 0);
  return acc;
}

}  // namespace

// The candidate (the slot that is not the current one) over all samples: per workgroup the Gram matrix of [J r], the samples
// whose residual is not finite, the cost's rounding scale Sum |r| (|measured| + |prediction|) / sigma, and the samples.
__global__ __launch_bounds__(kAccAlignThreads) void accalign_eval_kernel(AccAlignArgs a) {
  __shared__ double s_x[kAccAlignWaves * kAccAlignArea];
  __shared__ double s_w[kAccAlignWaves][4];
  const AccAlignControl* const c = a.ctrl;
  if (c->lm.done != 0) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int slot = c->lm.cur ^ 1;
  Q4 q; q.x = c->q[slot][0]; q.y = c->q[slot][1]; q.z = c->q[slot][2]; q.w = c->q[slot][3];
  const V3 tra = mk(c->t[slot][0], c->t[slot][1], c->t[slot][2]);
  const V3 b = mk(c->bias[slot][0], c->bias[slot][1], c->bias[slot][2]);
  const V3 g = mk(c->gravity[slot][0], c->gravity[slot][1], c->gravity[slot][2]);
  const double tau = c->latency[slot], is = a.inv_sigma;
  const M3 Ra = rotmat(q);
  const int i = blockIdx.x * kAccAlignThreads + threadIdx.x;
  const AlignSpline& sp = a.spline;
  double* const area = s_x + wave * kAccAlignArea;
  double* const row = area + lane * kAccAlignRow;

  // the rows' entries that differ between x, y and z: rotation, lever arm, gravity (3 x 3 each), latency and residual (3 each)
  V3 jr[3], jt[3], jg[3], jl = mk(0.0, 0.0, 0.0), res = mk(0.0, 0.0, 0.0);
#pragma unroll
  for (int j = 0; j < 3; ++j) jr[j] = jt[j] = jg[j] = mk(0.0, 0.0, 0.0);
  double used = 0.0, noise = 0.0, bad = 0.0;
  const int seg = i < a.n ? align_segment(sp, a.stamps[i]) : -1;      // (the stamp's segment, as in the optimiser)
  if (seg >= 0) {
    const double t = a.stamps[i] - tau;
    double p[4][6];
    align_pose<4, 6>(sp, seg, t, p);
    // phi = -p, phi' = -p', phi'' = -p'', each with its derivative along t
    const Rodrigues<D1> R = accalign_rodrigues(dual(-p[0][0], -p[1][0]), dual(-p[0][1], -p[1][1]), dual(-p[0][2], -p[1][2]));
    const D1 fx = dual(-p[1][0], -p[2][0]), fy = dual(-p[1][1], -p[2][1]), fz = dual(-p[1][2], -p[2][2]);
    D1 ox, oy, oz, ax, ay, az;
    rod_J_apply<D1>(R, fx, fy, fz, &ox, &oy, &oz);
    rod_J_apply<D1>(R, dual(-p[2][0], -p[3][0]), dual(-p[2][1], -p[3][1]), dual(-p[2][2], -p[3][2]), &ax, &ay, &az);
    D1 H[3][3];
    rod_H_apply<D1>(R, fx, fy, fz, H);      // H[i] = H_i phi'
    ax = ax + H[0][0] * fx + H[1][0] * fy + H[2][0] * fz;
    ay = ay + H[0][1] * fx + H[1][1] * fy + H[2][1] * fz;
    az = az + H[0][2] * fx + H[1][2] * fy + H[2][2] * fz;
    const V3 omega = mk(ox.v, oy.v, oz.v), omega_d = mk(ox.d, oy.d, oz.d), alpha = mk(ax.v, ay.v, az.v), alpha_d = mk(ax.d, ay.d, az.d);
    const M3 Rrw = rotmat(angle_axis_to_quat(mk(-p[0][0], -p[0][1], -p[0][2])));
    const V3 rv = mul(Rrw, mk(p[2][3] - g.x, p[2][4] - g.y, p[2][5] - g.z));
    const V3 inner = rv + cross(omega, cross(omega, tra)) - cross(alpha, tra);
    const V3 inner_d = cross(omega, rv) + mul(Rrw, mk(p[3][3], p[3][4], p[3][5])) + cross(omega_d, cross(omega, tra)) +
                       cross(omega, cross(omega_d, tra)) - cross(alpha_d, tra);
    const V3 f0 = mulT(Ra, inner);
    const double m[3] = {a.meas[3 * size_t(i)], a.meas[3 * size_t(i) + 1], a.meas[3 * size_t(i) + 2]};
    const double pred[3] = {f0.x + b.x, f0.y + b.y, f0.z + b.z};
    res = mk((m[0] - pred[0]) * is, (m[1] - pred[1]) * is, (m[2] - pred[2]) * is);
    // d (R_a^T inner) / d delta_j = R_a^T (inner x e_j) for R_a <- exp([delta]x) R_a
    jr[0] = (-is) * mulT(Ra, mk(0.0, inner.z, -inner.y)); jr[1] = (-is) * mulT(Ra, mk(-inner.z, 0.0, inner.x)); jr[2] = (-is) * mulT(Ra, mk(inner.y, -inner.x, 0.0));
    // d inner / d t_ra_j = omega x (omega x e_j) - alpha x e_j
    jt[0] = (-is) * mulT(Ra, cross(omega, mk(0.0, omega.z, -omega.y)) - mk(0.0, alpha.z, -alpha.y));
    jt[1] = (-is) * mulT(Ra, cross(omega, mk(-omega.z, 0.0, omega.x)) - mk(-alpha.z, 0.0, alpha.x));
    jt[2] = (-is) * mulT(Ra, cross(omega, mk(omega.y, -omega.x, 0.0)) - mk(alpha.y, -alpha.x, 0.0));
    // d inner / d g_j = -R(phi) e_j
    jg[0] = is * mulT(Ra, mk(Rrw.m[0][0], Rrw.m[1][0], Rrw.m[2][0])); jg[1] = is * mulT(Ra, mk(Rrw.m[0][1], Rrw.m[1][1], Rrw.m[2][1]));
    jg[2] = is * mulT(Ra, mk(Rrw.m[0][2], Rrw.m[1][2], Rrw.m[2][2]));
    jl = is * mulT(Ra, inner_d);      // d r / d latency = + d prediction / d t
    noise = (fabs(res.x) * (fabs(m[0]) + fabs(pred[0])) + fabs(res.y) * (fabs(m[1]) + fabs(pred[1])) + fabs(res.z) * (fabs(m[2]) + fabs(pred[2]))) * is;
    bad = __builtin_isfinite(noise) ? 0.0 : 1.0;
    used = 1.0;
  }

  acc_f64x4 acc = {0.0, 0.0, 0.0, 0.0};
  const double nb = used != 0.0 ? -is : 0.0;
  // x rows
  row[0] = jr[0].x; row[1] = jr[1].x; row[2] = jr[2].x; row[3] = jt[0].x; row[4] = jt[1].x; row[5] = jt[2].x;
  row[6] = nb; row[7] = 0.0; row[8] = 0.0; row[9] = jg[0].x; row[10] = jg[1].x; row[11] = jg[2].x; row[12] = jl.x; row[13] = res.x;
  row[14] = 0.0; row[15] = 0.0;
  wave_fence();
  acc = gram_rows(area, lane, acc);
  wave_fence();
  // y rows
  row[0] = jr[0].y; row[1] = jr[1].y; row[2] = jr[2].y; row[3] = jt[0].y; row[4] = jt[1].y; row[5] = jt[2].y;
  row[6] = 0.0; row[7] = nb; row[9] = jg[0].y; row[10] = jg[1].y; row[11] = jg[2].y; row[12] = jl.y; row[13] = res.y;
  wave_fence();
  acc = gram_rows(area, lane, acc);
  wave_fence();
  // z rows
  row[0] = jr[0].z; row[1] = jr[1].z; row[2] = jr[2].z; row[3] = jt[0].z; row[4] = jt[1].z; row[5] = jt[2].z;
  row[7] = 0.0; row[8] = nb; row[9] = jg[0].z; row[10] = jg[1].z; row[11] = jg[2].z; row[12] = jl.z; row[13] = res.z;
  wave_fence();
  acc = gram_rows(area, lane, acc);
  wave_fence();

  // the wave's tile to its own area (col = lane & 15, row = (lane >> 4) + 4 reg), the wave sums, then the waves in order
#pragma unroll
  for (int r = 0; r < 4; ++r) area[((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[r];
  const double s_bad = align_wave_sum(bad), s_noise = align_wave_sum(noise), s_used = align_wave_sum(used);
  if (lane == 0) { s_w[wave][0] = s_bad; s_w[wave][1] = s_noise; s_w[wave][2] = s_used; }
  __syncthreads();
  double* const out = a.part + size_t(blockIdx.x) * kAccAlignPart;
  {
    const int r = threadIdx.x >> 4, col = threadIdx.x & 15;
    double v = s_x[threadIdx.x];
#pragma unroll
    for (int w = 1; w < kAccAlignWaves; ++w) v += s_x[w * kAccAlignArea + threadIdx.x];
    if (r < kAccAlignCols && col < kAccAlignCols) out[r * kAccAlignCols + col] = v;
  }
  if (threadIdx.x < 3) {
    double v = s_w[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kAccAlignWaves; ++w) v += s_w[w][threadIdx.x];
    out[kAccAlignGram + threadIdx.x] = v;
  }
}

// One wave: the candidate's partials added in workgroup order, then what the stage asks for. Stage L: the model is linear in
// (lever arm, bias, gravity) at the given rotation and latency, so the 9 x 9 block of the Gram matrix evaluated at zero solves
// for them; the normal equations square the condition number, so a second evaluation at that solution gives one step of
// iterative refinement (align_accel_solve_kernel's reason) before the loop starts there. The loop is point_lm_dev.hpp's: the decision
// (lm_rule.hpp: lm_point_decision), the damped 13 x 13 step from the point that is current afterwards, and the next candidate.
__global__ __launch_bounds__(64) void accalign_decide_kernel(AccAlignArgs a, int n_chunks) {
  __shared__ double s_g[kAccAlignPart];
  __shared__ double s_h[kAccAlignParams * kAccAlignParams];
  __shared__ double s_b[16];
  AccAlignControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  if (c->lm.done != 0) return;
  const int cur = c->lm.cur, nxt = cur ^ 1, stage = c->stage;
  for (int e = lane; e < kAccAlignSums; e += 64) {
    double s = 0.0;
    for (int ch = 0; ch < n_chunks; ++ch) s += a.part[size_t(ch) * kAccAlignPart + e];
    s_g[e] = s;
    if (stage == kAccAlignStageLoop) c->G[nxt][e] = s;
  }
  wave_fence();
  const double cand = 0.5 * s_g[kAccAlignCostAt], lost = s_g[kAccAlignBadAt];
  const bool kept = lost == 0.0 && __builtin_isfinite(cand) && point_lm_finite(c->q[nxt], 4) && point_lm_finite(c->t[nxt], 3) && point_lm_finite(c->bias[nxt], 3) &&
                    point_lm_finite(c->gravity[nxt], 3) && point_lm_finite(&c->latency[nxt], 1);

  if (stage != kAccAlignStageLoop) {
    int linear = CALICO_ALIGN_OK;
    if (!kept) {
      linear = CALICO_ALIGN_DEGENERATE;
    } else {
      point_lm_normal(GramFull14{s_g}, 3, kAccAlignLinear, ~0u, 1.0, s_h, s_b, lane);
      if (!lds_chol(s_h, kAccAlignLinear, lane)) {
        linear = CALICO_ALIGN_NOT_POSITIVE_DEFINITE;
      } else {
        lds_chol_solve(s_h, s_b, kAccAlignLinear, lane);
        if (!point_lm_finite(s_b, kAccAlignLinear)) linear = CALICO_ALIGN_NOT_POSITIVE_DEFINITE;
        else if (lane == 0) {
#pragma unroll
          for (int j = 0; j < 3; ++j) { c->t[nxt][j] += s_b[j]; c->bias[nxt][j] += s_b[3 + j]; c->gravity[nxt][j] += s_b[6 + j]; }
        }
      }
    }
    if (lane == 0) {
      c->linear_status = linear;
      if (linear != CALICO_ALIGN_OK) { c->lm.status = linear; c->lm.done = 1; }
      if (stage == kAccAlignStageRefine) c->linear_rms = sqrt(s_g[kAccAlignCostAt] / (3.0 * s_g[kAccAlignCountAt])) / a.inv_sigma;
      c->stage = stage + 1;
    }
    return;
  }

  const double current = 0.5 * c->G[cur][kAccAlignCostAt], noise = c->G[cur][kAccAlignNoiseAt];
  PointLmState st = point_lm_state(c->lm, lm_point_decision(c->lm.first != 0, kept, cand, current, noise, c->lm.step < a.step_tolerance, c->lm.lambda,
                                                            c->lm.iterations, a.max_iterations), cand);
  double step = 0.0;
  if (st.done == 0) {
    point_lm_restore(s_g, c->G[cur], kAccAlignSums, st.cur != nxt, lane);
    if (point_lm_damped_step(GramFull14{s_g}, kAccAlignParams, a.free_bits, &st, s_h, s_b, lane)) {
      const int at = st.cur, to = at ^ 1;
      const double rot = point_lm_rotate(c->q[at], s_b, (a.free_bits & 7u) == 0u, c->q[to], lane), lever = point_lm_add3(c->t[at], s_b + 3, c->t[to], lane);
      const double bias = point_lm_add3(c->bias[at], s_b + 6, c->bias[to], lane), grav = point_lm_add3(c->gravity[at], s_b + 9, c->gravity[to], lane);
      step = point_lm_step_size(fmax(rot, lever), fmax(bias, grav), point_lm_add1(c->latency[at], s_b[12], &c->latency[to], lane));
    }
  }
  point_lm_write(&c->lm, lane, st, step);
}

// The undamped inverse normal matrix at the result (zero rows and columns for what is not estimated) and the RMS in m/s^2.
__global__ __launch_bounds__(64) void accalign_final_kernel(AccAlignArgs a) {
  __shared__ double s_g[kAccAlignPart];
  __shared__ double s_h[kAccAlignParams * kAccAlignParams];
  __shared__ double s_b[16];
  AccAlignControl* const c = a.ctrl;
  const int lane = threadIdx.x;
  if (!point_lm_ran(c->lm.status) || c->lm.first != 0) return;
  const int cur = c->lm.cur;
  for (int e = lane; e < kAccAlignSums; e += 64) s_g[e] = c->G[cur][e];
  wave_fence();
  point_lm_finish(&c->lm, GramFull14{s_g}, kAccAlignParams, a.free_bits, 0.5 * s_g[kAccAlignCostAt], s_h, s_b, c->cov, lane);
  if (lane == 0) c->rms = sqrt(s_g[kAccAlignCostAt] / (3.0 * double(a.n))) / a.inv_sigma;
}

// ---- launches ------------------------------------------------------------------------------------------------------------------
int accalign_chunks(int n) { return n > 0 ? (n + kAccAlignThreads - 1) / kAccAlignThreads : 0; }

hipError_t launch_accalign_iteration(const AccAlignArgs& a, hipStream_t s) {
  const int chunks = accalign_chunks(a.n);
  if (chunks == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(accalign_eval_kernel, dim3(unsigned(chunks)), dim3(kAccAlignThreads), 0, s, a);
  hipLaunchKernelGGL(accalign_decide_kernel, dim3(1), dim3(64), 0, s, a, chunks);
  return hipGetLastError();
}

hipError_t launch_accalign_finish(const AccAlignArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(accalign_final_kernel, dim3(1), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace cal
