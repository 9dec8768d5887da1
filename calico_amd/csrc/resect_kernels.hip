// resect_kernels.hip — chart resection (calico_camera_resect): the pose T_camera_chart of every frame of a ragged batch of
// (pixel, chart point) pairs, for any camera model at given intrinsics.
//
// Layout: one wave per frame, kResectWaves frames per workgroup, no barrier (a wave never waits for another). Lane l takes
// pairs l, l + 64, ... of its frame; every loop over the pairs runs ceil(n / 64) trips with ALL lanes in it (a lane past the end
// is `live = false`), so that the DPP sums below and unproject<>'s wave votes always see a whole wave.
//   start (no initial pose): unproject<MODEL> every pixel, keep the pairs with a valid unit bearing of z > 0.1, estimate the
//     homography (x/z, y/z) ~ H (X, Y, 1) with Hartley normalisation on both sides (centroid, mean distance sqrt 2) from the
//     8x8 normal equations of the inhomogeneous form (h22 = 1 in normalised coordinates: the centroid of points in front of
//     the camera is in front of it, so h22 != 0), split H = s [r1 r2 t] with the sign that puts the centroid in front, and take
//     the orthogonal polar factor of [r1 r2 r1 x r2] (Newton's iteration X <- (X + X^-T) / 2; det > 0 by construction).
//     Three passes over the pairs (sums for the centroids, for the scales, for the normal equations); the normalised image
//     points of pass 1 are kept in a workspace (2 doubles per pair), the unprojection is not repeated.
//   refinement: Levenberg-Marquardt on [delta_rot, t], R <- exp([delta]x) R, over Sum rho(|project(k, R p + t) - pixel|^2)
//     with project<MODEL, true> and its d pixel / d point; rho = identity or Huber, weights rho', no second-order term.
//     One pass over the pairs per step evaluates the candidate: costs, J^T W J (21), J^T W e (6), counts. Every sum is
//     wave_sum (problem_dev.hpp) of per-lane partial sums: a fixed order, the same bits in every lane, so every decision
//     below is wave-uniform. Everything wave-uniform lives in the wave's LDS area, not in registers: two state slots (the
//     current pose and the candidate: system, costs, q, t; acceptance swaps their roles) and the work matrix of the 6x6
//     (8x8 for the start) Cholesky, which runs as loops with run-time bounds over LDS (J^T W J + lambda diag). Registers hold
//     the per-lane sums and the projection; nothing is indexed at run time in registers (no scratch).
//     A byte per pair holds "valid at the current pose" / "valid at the candidate" in two bits that swap roles on acceptance.
//     A candidate at which a pair that is valid at the current pose is rejected by the model is a rejected step; the costs
//     compared are those over the pairs valid at the current pose, a pair that became valid joins after acceptance.
//     A candidate is accepted when its cost does not exceed the current one by more than the cost's own rounding error
//     (kCostSlack): near the minimum a step of 1e-11 changes a cost of order 1 in its 16th digit.
//   stop: a step with |delta_rot|_inf < tol and |delta_t|_inf < tol max(1, |t|) taken at lambda <= its initial value 1e-4 (the
//     damped step is then the Gauss-Newton step to 1e-4) -- accepted (OK, at the new pose) or rejected (OK, the pose is kept);
//     max_iterations steps tried (NOT_CONVERGED).
// A frame reads and writes nothing but its own slices: its result does not depend on the other frames or its position.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/calico_hip.h"
#include "arrowhead_dev.hpp"
#include "kernels.hpp"

namespace cal {

constexpr int kResectWaves = 4;
constexpr int kResectThreads = 64 * kResectWaves;
constexpr int kResectPolarSteps = 16;
constexpr int kResectWavesPerSimd = 2;      // the register budget asked of the compiler: 256 VGPRs

namespace {

// A pose's state in the wave's LDS area (two slots: the current pose and the candidate; acceptance swaps their roles):
//   [0, 21) J^T W J, lower triangle by rows, order [delta_rot, t];  [21, 27) J^T W e, e = projection - pixel;
//   [27] Sum rho over the pairs valid at the pose;  [28] Sum |e|^2 over them (no loss);  [29] their number;
//   [30] Sum |e_u| |u| + |e_v| |v|: the scale of the cost's rounding error;  [31, 35) q;  [35, 38) t
constexpr int kSlot = 40, kCost = 27, kSs = 28, kValid = 29, kNoise = 30, kPose = 31;
DEV void put_pose(double* st, Q4 q, V3 t, int lane) {
  if (lane == 0) { st[kPose] = q.x; st[kPose + 1] = q.y; st[kPose + 2] = q.z; st[kPose + 3] = q.w; st[kPose + 4] = t.x; st[kPose + 5] = t.y; st[kPose + 6] = t.z; }
}
DEV Q4 pose_q(const double* st) { Q4 q; q.x = st[kPose]; q.y = st[kPose + 1]; q.z = st[kPose + 2]; q.w = st[kPose + 3]; return q; }
DEV V3 pose_t(const double* st) { return mk(st[kPose + 4], st[kPose + 5], st[kPose + 6]); }

constexpr uint8_t kFlagStart = 1;      // usable for the start

// The pass at the pose of slot `st`, which receives the sums. cur < 0: there is no current pose yet (first evaluation); else bit
// `cur` of a pair's flags says whether it was valid at the current pose. Bit `nxt` receives its validity at this pose.
// *cost_common: Sum rho over the pairs valid at both poses; *n_lost: pairs valid at the current pose that this one loses.
template <int MODEL>
DEV void resect_evaluate(const ResectArgs& a, int64_t base, int64_t n, int lane, int cur, int nxt, double* st, double* cost_common, double* n_lost) {
  const double hs = a.huber_scale, hs2 = hs * hs;
  struct { double cost, cost_common, ss, noise; } s;
  int n_valid = 0, lost = 0;      // wave-uniform counts (ballots)
  double H[21], g[6];
#pragma unroll
  for (int i = 0; i < 21; ++i) H[i] = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) g[i] = 0.0;
  s.cost = s.cost_common = s.ss = s.noise = 0.0;
  for (int64_t i0 = 0; i0 < n; i0 += 64) {
    const int64_t i = base + i0 + lane;
    // the pose is read again in every trip (broadcast reads behind a fence): 24 registers that are not held across the body
    wave_fence();
    const M3 R = rotmat(pose_q(st));
    const V3 t = pose_t(st);
    bool ok = false, was = false;
    if (i0 + lane < n) {
      const V3 P = mk(a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]);
      const double u = a.pixels[2 * i], v = a.pixels[2 * i + 1];
      const uint8_t fl = a.flags[i];
      was = cur >= 0 && (fl & pose_bit(cur)) != 0;
      const V3 RP = mul(R, P), Pc = RP + t;
      double pix[2] = {0.0, 0.0}, D[2][3], dK[2][kMaxIntr];
      ok = project<MODEL, true>(a.k, Pc, pix, D, dK);
      ok = ok && __builtin_isfinite(pix[0]) && __builtin_isfinite(pix[1]);
      a.flags[i] = uint8_t((fl & ~pose_bit(nxt)) | (ok ? pose_bit(nxt) : 0));
      if (ok) {
        const double e0 = pix[0] - u, e1 = pix[1] - v, sq = e0 * e0 + e1 * e1;
        double w, rho;
        huber(sq, hs, hs2, &w, &rho);
        // d Pc / d delta = -[R P]x: row r of J is [(R P) x D_r, D_r]
        double J[2][6];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const V3 d = mk(D[r][0], D[r][1], D[r][2]), c = cross(RP, d);
          J[r][0] = c.x; J[r][1] = c.y; J[r][2] = c.z; J[r][3] = d.x; J[r][4] = d.y; J[r][5] = d.z;
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
          for (int c = 0; c <= r; ++c) H[r * (r + 1) / 2 + c] += w * (J[0][r] * J[0][c] + J[1][r] * J[1][c]);
          g[r] += w * (J[0][r] * e0 + J[1][r] * e1);
        }
        s.cost += rho; s.ss += sq; s.noise += dabs(e0 * pix[0]) + dabs(e1 * pix[1]);
        if (was) s.cost_common += rho;
      }
    }
    n_valid += __popcll(__ballot(ok)); lost += __popcll(__ballot(was && !ok));
  }
#pragma unroll
  for (int i = 0; i < 21; ++i) put(&st[i], wave_sum(H[i]), lane);
#pragma unroll
  for (int i = 0; i < 6; ++i) put(&st[21 + i], wave_sum(g[i]), lane);
  put(&st[kCost], wave_sum(s.cost), lane); put(&st[kSs], wave_sum(s.ss), lane); put(&st[kValid], double(n_valid), lane);
  put(&st[kNoise], wave_sum(s.noise), lane);
  *cost_common = wave_sum(s.cost_common); *n_lost = double(lost);
  wave_fence();
}

// The homography start. false: the frame has none (points off their z = 0 plane, fewer than 4 usable pairs, a singular system).
template <int MODEL>
DEV bool resect_start(const ResectArgs& a, int64_t base, int64_t n, int lane, double* A /* LDS, 8 x 8 */, double* h /* LDS, 8 */, Q4* q_out, V3* t_out) {
  // pass 1: unprojection, centroids, the points' extent
  double cnt = 0.0, sX = 0.0, sY = 0.0, sx = 0.0, sy = 0.0;
  double hiX = -1e300, loX = -1e300, hiY = -1e300, loY = -1e300, hiZ = 0.0;      // lo*: of the negated coordinate
  for (int64_t i0 = 0; i0 < n; i0 += 64) {
    const int64_t i = base + i0 + lane;
    const bool live = i0 + lane < n;
    double u = 0.0, v = 0.0;
    V3 P = mk(0.0, 0.0, 0.0);
    if (live) { u = a.pixels[2 * i]; v = a.pixels[2 * i + 1]; P = mk(a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]); }
    V3 b;
    const bool ok = unproject<MODEL>(a.k, u, v, live, &b);
    if (live) {
      const bool use = ok && b.z > 0.1;
      const double x = use ? b.x / b.z : 0.0, y = use ? b.y / b.z : 0.0;
      a.ws[2 * i] = x; a.ws[2 * i + 1] = y;
      a.flags[i] = use ? kFlagStart : 0;
      if (use) { cnt += 1.0; sX += P.x; sY += P.y; sx += x; sy += y; }
      hiX = fmax(hiX, P.x); loX = fmax(loX, -P.x); hiY = fmax(hiY, P.y); loY = fmax(loY, -P.y); hiZ = fmax(hiZ, dabs(P.z));
      if (!(dabs(P.z) <= 1e300)) hiZ = 1e300;      // a non-finite z is off the plane
    }
  }
  cnt = wave_sum(cnt); sX = wave_sum(sX); sY = wave_sum(sY); sx = wave_sum(sx); sy = wave_sum(sy);
  hiX = wave_max(hiX); loX = wave_max(loX); hiY = wave_max(hiY); loY = wave_max(loY); hiZ = wave_max(hiZ);
  const double extent = fmax(fmax(hiX + loX, hiY + loY), hiZ);
  if (uniform_flag(!(hiZ <= 1e-9 * extent) || cnt < 4.0)) return false;
  const double mX = sX / cnt, mY = sY / cnt, mx = sx / cnt, my = sy / cnt;
  // pass 2: mean distances from the centroids
  double dP = 0.0, dI = 0.0;
  for (int64_t i0 = 0; i0 < n; i0 += 64) {
    const int64_t i = base + i0 + lane;
    if (i0 + lane < n && (a.flags[i] & kFlagStart)) {
      const double X = a.points[3 * i] - mX, Y = a.points[3 * i + 1] - mY, x = a.ws[2 * i] - mx, y = a.ws[2 * i + 1] - my;
      dP += sqrt(X * X + Y * Y); dI += sqrt(x * x + y * y);
    }
  }
  dP = wave_sum(dP); dI = wave_sum(dI);
  if (uniform_flag(!(dP > 0.0) || !(dI > 0.0) || !__builtin_isfinite(dP) || !__builtin_isfinite(dI))) return false;
  const double sP = 1.4142135623730951 * cnt / dP, sI = 1.4142135623730951 * cnt / dI;
  // pass 3: the normal equations of  [X Y 1 0 0 0 -xX -xY] h = x,  [0 0 0 X Y 1 -yX -yY] h = y
  double S0[6], Sx[6], Sy[6], Sr[5];      // sums of {XX, XY, YY, X, Y, 1} times 1, x, y, x^2 + y^2
#pragma unroll
  for (int j = 0; j < 6; ++j) { S0[j] = 0.0; Sx[j] = 0.0; Sy[j] = 0.0; }
#pragma unroll
  for (int j = 0; j < 5; ++j) Sr[j] = 0.0;
  for (int64_t i0 = 0; i0 < n; i0 += 64) {
    const int64_t i = base + i0 + lane;
    if (i0 + lane < n && (a.flags[i] & kFlagStart)) {
      const double X = sP * (a.points[3 * i] - mX), Y = sP * (a.points[3 * i + 1] - mY);
      const double x = sI * (a.ws[2 * i] - mx), y = sI * (a.ws[2 * i + 1] - my), r = x * x + y * y;
      const double m6[6] = {X * X, X * Y, Y * Y, X, Y, 1.0};
#pragma unroll
      for (int j = 0; j < 6; ++j) { S0[j] += m6[j]; Sx[j] += x * m6[j]; Sy[j] += y * m6[j]; }
#pragma unroll
      for (int j = 0; j < 5; ++j) Sr[j] += r * m6[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) { S0[j] = wave_sum(S0[j]); Sx[j] = wave_sum(Sx[j]); Sy[j] = wave_sum(Sy[j]); }
#pragma unroll
  for (int j = 0; j < 5; ++j) Sr[j] = wave_sum(Sr[j]);
  if (lane == 0) {
    for (int e = 0; e < 64; ++e) A[e] = 0.0;
    A[0] = S0[0]; A[8] = S0[1]; A[9] = S0[2]; A[16] = S0[3]; A[17] = S0[4]; A[18] = S0[5];
    A[27] = S0[0]; A[35] = S0[1]; A[36] = S0[2]; A[43] = S0[3]; A[44] = S0[4]; A[45] = S0[5];
    A[48] = -Sx[0]; A[49] = -Sx[1]; A[50] = -Sx[3]; A[56] = -Sx[1]; A[57] = -Sx[2]; A[58] = -Sx[4];
    A[51] = -Sy[0]; A[52] = -Sy[1]; A[53] = -Sy[3]; A[59] = -Sy[1]; A[60] = -Sy[2]; A[61] = -Sy[4];
    A[54] = Sr[0]; A[62] = Sr[1]; A[63] = Sr[2];
    h[0] = Sx[3]; h[1] = Sx[4]; h[2] = Sx[5]; h[3] = Sy[3]; h[4] = Sy[4]; h[5] = Sy[5]; h[6] = -Sr[3]; h[7] = -Sr[4];
  }
  wave_fence();
  if (!lds_chol(A, 8, lane)) return false;
  lds_chol_solve(A, h, 8, lane);
  // H = Ti^-1 Hn Tp,  Tp = [sP 0 -sP mX; 0 sP -sP mY; 0 0 1],  Ti^-1 = [1/sI 0 mx; 0 1/sI my; 0 0 1]
  M3 Hn, G;
  Hn.m[0][0] = h[0]; Hn.m[0][1] = h[1]; Hn.m[0][2] = h[2]; Hn.m[1][0] = h[3]; Hn.m[1][1] = h[4]; Hn.m[1][2] = h[5];
  Hn.m[2][0] = h[6]; Hn.m[2][1] = h[7]; Hn.m[2][2] = 1.0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {      // G = Hn Tp
    G.m[r][0] = Hn.m[r][0] * sP; G.m[r][1] = Hn.m[r][1] * sP;
    G.m[r][2] = Hn.m[r][2] - sP * (Hn.m[r][0] * mX + Hn.m[r][1] * mY);
  }
  const double iI = 1.0 / sI;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    G.m[0][c] = G.m[0][c] * iI + mx * G.m[2][c];
    G.m[1][c] = G.m[1][c] * iI + my * G.m[2][c];
  }
  // the chart in front: the depth of the centroid of the usable points is positive
  const double zc = G.m[2][0] * mX + G.m[2][1] * mY + G.m[2][2];
  V3 h1 = mk(G.m[0][0], G.m[1][0], G.m[2][0]), h2 = mk(G.m[0][1], G.m[1][1], G.m[2][1]), h3 = mk(G.m[0][2], G.m[1][2], G.m[2][2]);
  const double n1 = sqrt(dot(h1, h1)), n2 = sqrt(dot(h2, h2));
  const double sc = (zc < 0.0 ? -2.0 : 2.0) / (n1 + n2);
  h1 = sc * h1; h2 = sc * h2; h3 = sc * h3;
  const V3 r3 = cross(h1, h2);
  M3 X;
  X.m[0][0] = h1.x; X.m[1][0] = h1.y; X.m[2][0] = h1.z; X.m[0][1] = h2.x; X.m[1][1] = h2.y; X.m[2][1] = h2.z;
  X.m[0][2] = r3.x; X.m[1][2] = r3.y; X.m[2][2] = r3.z;
  bool ok = __builtin_isfinite(sc) && dot(r3, r3) > 1e-12;
  // nearest rotation: X <- (X + X^-T) / 2, X^-T = cofactors / det
#pragma unroll 1
  for (int it = 0; it < kResectPolarSteps; ++it) {
    const V3 c0 = mk(X.m[0][0], X.m[1][0], X.m[2][0]), c1 = mk(X.m[0][1], X.m[1][1], X.m[2][1]), c2 = mk(X.m[0][2], X.m[1][2], X.m[2][2]);
    const V3 k0 = cross(c1, c2), k1 = cross(c2, c0), k2 = cross(c0, c1);
    const double idet = 1.0 / dot(c0, k0);
    X.m[0][0] = 0.5 * (c0.x + idet * k0.x); X.m[1][0] = 0.5 * (c0.y + idet * k0.y); X.m[2][0] = 0.5 * (c0.z + idet * k0.z);
    X.m[0][1] = 0.5 * (c1.x + idet * k1.x); X.m[1][1] = 0.5 * (c1.y + idet * k1.y); X.m[2][1] = 0.5 * (c1.z + idet * k1.z);
    X.m[0][2] = 0.5 * (c2.x + idet * k2.x); X.m[1][2] = 0.5 * (c2.y + idet * k2.y); X.m[2][2] = 0.5 * (c2.z + idet * k2.z);
  }
  const Q4 q = canonical(quat_of(X));
  ok = ok && finite_pose(q, h3);
  *q_out = q; *t_out = h3;
  return uniform_flag(ok);
}

}  // namespace

constexpr int kResectLdsDoubles = 2 * kSlot + 72 + 8;      // two pose slots, the work area (8 x 8, or a 6 x 6 factor and its inverse), a right-hand side

template <int MODEL>
__global__ __launch_bounds__(kResectThreads, kResectWavesPerSimd) void resect_kernel(ResectArgs a) {
  __shared__ double s_lds[kResectWaves][kResectLdsDoubles];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t f = int64_t(blockIdx.x) * kResectWaves + wave;
  if (f >= a.n_frames) return;      // (the whole wave: no barrier follows)
  const int64_t base = a.offsets[f], n = a.offsets[f + 1] - base;
  double* const slots = s_lds[wave];
  double* const W = slots + 2 * kSlot;
  double* const rhs = W + 72;

  int status = CALICO_RESECT_NOT_CONVERGED, iterations = 0;
  int cur = 0;      // the slot, and the validity bit, of the current pose
  bool run = true;
  if (n < a.min_points) { status = CALICO_RESECT_TOO_FEW_POINTS; run = false; }
  if (run) {
    Q4 q;
    V3 t;
    if (a.q_init) {
      q.x = a.q_init[4 * f]; q.y = a.q_init[4 * f + 1]; q.z = a.q_init[4 * f + 2]; q.w = a.q_init[4 * f + 3];
      q = canonical(q);
      t = mk(a.t_init[3 * f], a.t_init[3 * f + 1], a.t_init[3 * f + 2]);
    } else if (!resect_start<MODEL>(a, base, n, lane, W, rhs, &q, &t)) {
      status = CALICO_RESECT_NO_START; run = false;
    }
    if (run) put_pose(slots + kSlot * (cur ^ 1), q, t, lane);
    wave_fence();
  }
  if (run) {
    double lambda = kLmLambda0;
    bool first = true, small = false;
#pragma unroll 1
    for (;;) {
      double* const cand = slots + kSlot * (cur ^ 1);
      double cost_common, n_lost;
      resect_evaluate<MODEL>(a, base, n, lane, first ? -1 : cur, cur ^ 1, cand, &cost_common, &n_lost);
      const bool kept = uniform_flag(n_lost == 0.0 && __builtin_isfinite(cand[kCost]) && finite_pose(pose_q(cand), pose_t(cand)));
      if (first) {
        if (!kept || uniform_flag(cand[kValid] < 1.0)) { status = CALICO_RESECT_DEGENERATE; break; }
        cur ^= 1;
        first = false;
      } else {
        const LmVerdict v = lm_rule(kept, cost_common, slots[kSlot * cur + kCost], slots[kSlot * cur + kNoise], small, lambda);
        if (uniform_flag(v.accept)) cur ^= 1;
        lambda = uniform_value(v.lambda);      // (the verdict is wave-uniform; said so, lambda stays in scalar registers)
        if (uniform_flag(v.converged)) { status = CALICO_RESECT_OK; break; }
      }
      if (iterations >= a.max_iterations) break;
      ++iterations;
      // the damped step at the current pose: (J^T W J + lambda diag) d = -J^T W e; more damping while it is not positive definite
      const double* const cs = slots + kSlot * cur;
      bool pd = false;
#pragma unroll 1
      for (;;) {
        if (lane == 0) {
          for (int r = 0; r < 6; ++r) {
            for (int c = 0; c <= r; ++c) W[6 * r + c] = cs[r * (r + 1) / 2 + c] * (c == r ? 1.0 + lambda : 1.0);
            rhs[r] = -cs[21 + r];
          }
        }
        wave_fence();
        pd = lds_chol(W, 6, lane);
        if (pd || lambda >= kLmLambdaMax) break;
        lambda = fmin(lambda * 10.0, kLmLambdaMax);
      }
      if (!pd) { status = CALICO_RESECT_DEGENERATE; break; }
      lds_chol_solve(W, rhs, 6, lane);
      const V3 dr = mk(rhs[0], rhs[1], rhs[2]), dt = mk(rhs[3], rhs[4], rhs[5]), t = pose_t(cs);
      const double tol = a.step_tolerance;
      small = uniform_flag(fmax(fmax(dabs(dr.x), dabs(dr.y)), dabs(dr.z)) < tol &&
                           fmax(fmax(dabs(dt.x), dabs(dt.y)), dabs(dt.z)) < tol * fmax(1.0, sqrt(dot(t, t))));
      Q4 qn;
      V3 tn;
      (void)retract_pose(pose_q(cs), t, dr, dt, &qn, &tn);      // (this kernel's test of the step is the two comparisons above)
      put_pose(slots + kSlot * (cur ^ 1), qn, tn, lane);
      wave_fence();
    }
  }
  // the covariance of the result, (J^T W J)^-1: the undamped system must be positive definite (the pose is locally unique)
  bool has_pose = status == CALICO_RESECT_OK || status == CALICO_RESECT_NOT_CONVERGED;
  double cov = 0.0;      // lane 6 r + c: entry (r, c)
  const double* const cs = slots + kSlot * cur;
  if (has_pose) {
    double* const Li = W + 36;
    if (lane == 0)
      for (int r = 0; r < 6; ++r)
        for (int c = 0; c <= r; ++c) W[6 * r + c] = cs[r * (r + 1) / 2 + c];
    wave_fence();
    bool ok = lds_chol(W, 6, lane);
    chol_inverse_gram(W, Li, 6, lane, [&](int, int, int, double v) { cov = v; });      // (36 entries: one per lane)
    ok = ok && __all(__builtin_isfinite(cov)) && __builtin_isfinite(sqrt(cs[kSs] / cs[kValid]));
    if (uniform_flag(!ok)) { status = CALICO_RESECT_DEGENERATE; has_pose = false; }
  }
  if (lane == 0) {
    Q4 q; q.x = q.y = q.z = 0.0; q.w = 1.0;
    V3 t = mk(0.0, 0.0, 0.0);
    double ss = 0.0, n_valid = 0.0;
    if (has_pose) { q = pose_q(cs); t = pose_t(cs); ss = cs[kSs]; n_valid = cs[kValid]; }
    a.q_out[4 * f] = has_pose ? q.x : 0.0; a.q_out[4 * f + 1] = has_pose ? q.y : 0.0; a.q_out[4 * f + 2] = has_pose ? q.z : 0.0;
    a.q_out[4 * f + 3] = has_pose ? q.w : 1.0;
    a.t_out[3 * f] = has_pose ? t.x : 0.0; a.t_out[3 * f + 1] = has_pose ? t.y : 0.0; a.t_out[3 * f + 2] = has_pose ? t.z : 0.0;
    a.rms_out[f] = has_pose ? sqrt(ss / n_valid) : 0.0;
    a.n_used_out[f] = has_pose ? int(n_valid) : 0;
    a.iterations_out[f] = iterations;
    a.status_out[f] = uint8_t(status);
  }
  if (a.cov_out && lane < 36) a.cov_out[36 * f + lane] = has_pose ? cov : 0.0;
}

hipError_t launch_camera_resect(int model, const ResectArgs& a, hipStream_t s) {
  if (a.n_frames <= 0) return hipSuccess;
  const dim3 grid(unsigned((a.n_frames + kResectWaves - 1) / kResectWaves)), block(kResectThreads);
  return with_camera_model(model, [&](auto m) { hipLaunchKernelGGL(resect_kernel<decltype(m)::value>, grid, block, 0, s, a); });
}

}  // namespace cal
