// imu_align_dev.hpp — what the alignment kernels (align_kernels.hip; camalign_kernels.hip takes the spline, the sums and the Jacobi
// eigen-solver) need of the IMU items' kinematics, on a spline
// that is not part of a problem: the segment of a time, the pose's derivatives there, and the rig's angular velocity and
// acceleration as GyroscopeResidual / AccelerometerResidual form them (phi = -pose[0:3], omega = J(phi) phi', alpha = J' phi' +
// J phi'', gyroscope_cost_functor.h / accelerometer_cost_functor.h through device_math.hpp's Rodrigues pieces). Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "device_math.hpp"
#include "kernels.hpp"      // AlignSpline

namespace cal {

// GetSplineIndex (bspline.hpp:138-150): upper_bound(valid_knots, t) - 1, the last valid knot belongs to the last segment.
// -1 where t lies outside the valid knots (or is not a number).
DEV int align_segment(const AlignSpline& s, double t) {
  const double* const vk = s.knots + (s.k - 1);
  const int nv = s.n_valid;
  if (!(t >= vk[0]) || !(t <= vk[nv - 1])) return -1;
  int lo = 0, hi = nv;      // the first index whose knot is > t lies in [lo, hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (vk[mid] > t) hi = mid; else lo = mid + 1;
  }
  const int seg = lo - 1;      // (>= 0: vk[0] <= t)
  return seg > nv - 2 ? nv - 2 : seg;
}

// out[d][c]: derivative d of component c < NC of the pose at t (NC = 3: the rotation part alone). seg is align_segment's: the
// control points read are seg .. seg + k - 1 <= n_knots - k - 1.
template <int ND, int NC>
DEV void align_pose(const AlignSpline& s, int seg, double t, double out[ND][NC]) {
  const int k = s.k, ki = seg + k - 1;
  double W[ND][kMaxOrder];
  spline_weights<ND>(k, s.knots[ki], s.knots[ki + 1], s.basis + size_t(seg) * k * k, t, W);
#pragma unroll
  for (int d = 0; d < ND; ++d)
#pragma unroll
    for (int c = 0; c < NC; ++c) out[d][c] = 0.0;
#pragma unroll
  for (int a = 0; a < kMaxOrder; ++a) {
    if (a < k) {
      const double* const cp = s.ctrl + size_t(seg + a) * 6;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const double v = cp[c];
#pragma unroll
        for (int d = 0; d < ND; ++d) out[d][c] += W[d][a] * v;
      }
    }
  }
}

// rodrigues<double>'s coefficients (device_math.hpp, the same expressions) without its early return: with the two exits the
// compiler keeps two fields of the returned struct in scratch memory in these kernels; here every field is one select.
template <bool HESSIAN>
DEV Rodrigues<double> align_rodrigues(double px, double py, double pz) {
  Rodrigues<double> R;
  const double t2 = px * px + py * py + pz * pz;
  const bool zero = t2 == 0.0;
  const double th = sqrt(zero ? 1.0 : t2);
  double st, ct;
  dsincos(th, &st, &ct);
  const bool tiny = th < 1e-7;
  st = tiny ? small_sin(th) : st;
  ct = tiny ? small_cos(th) : ct;
  const double it = 1.0 / th;
  R.zero = zero;
  R.hx = zero ? 0.0 : it * px; R.hy = zero ? 0.0 : it * py; R.hz = zero ? 0.0 : it * pz;
  R.a = zero ? 0.0 : it * (1.0 - ct);
  R.b = zero ? 0.0 : it * (th - st);
  R.c0 = R.c1 = R.c2 = R.c3 = 0.0;
  if constexpr (HESSIAN) {
    const double it2 = it * it;
    R.c0 = zero ? 0.0 : ct - st * it;
    R.c1 = zero ? 0.0 : (1.0 - ct) * it2;
    R.c2 = zero ? 0.0 : 3.0 * it2 * st - it * (ct - 2.0);
    R.c3 = zero ? 0.0 : it2 * (th - st);
  }
  return R;
}

// omega = J(phi) phi' and, with ALPHA, alpha = Sum_i (H_i phi') phi'_i + J phi'' at phi = -p, phi' = -pd, phi'' = -pdd
template <bool ALPHA>
DEV void align_rates(V3 p, V3 pd, V3 pdd, V3* omega, V3* alpha) {
  const Rodrigues<double> R = align_rodrigues<ALPHA>(-p.x, -p.y, -p.z);
  double ox, oy, oz;
  rod_J_apply<double>(R, -pd.x, -pd.y, -pd.z, &ox, &oy, &oz);
  *omega = mk(ox, oy, oz);
  if constexpr (ALPHA) {
    double H[3][3];
    rod_H_apply<double>(R, -pd.x, -pd.y, -pd.z, H);      // H[i] = H_i phi'
    double jx, jy, jz;
    rod_J_apply<double>(R, -pdd.x, -pdd.y, -pdd.z, &jx, &jy, &jz);
    *alpha = mk(jx - (H[0][0] * pd.x + H[1][0] * pd.y + H[2][0] * pd.z), jy - (H[0][1] * pd.x + H[1][1] * pd.y + H[2][1] * pd.z),
                jz - (H[0][2] * pd.x + H[1][2] * pd.y + H[2][2] * pd.z));
  }
}

// d omega / d t = J' phi' + J phi'' at phi = -p, phi' = -pd, phi'' = -pdd, EXACTLY: what the optimiser's gyroscope term has for
// its latency column (it differentiates J(phi) phi' itself). ExpSO3Hessian's closed form, which align_rates' alpha follows as the
// accelerometer term does, is not the derivative of ExpSO3Jacobian, so alpha is not d omega / d t. With
//   J = I + A [phi]x + B [phi]x^2,  A = (1 - cos th) / th^2,  B = (th - sin th) / th^3,
//   J' = A' [phi]x + A [phi']x + B' [phi]x^2 + B ([phi']x [phi]x + [phi]x [phi']x),  A' = (dA/dth / th) phi . phi'.
// Below th = 0.25 the two derivative coefficients are their series (the closed forms cancel like eps / th^2).
DEV V3 align_omega_dot(V3 p, V3 pd, V3 pdd) {
  const V3 phi = -p, f = -pd, ff = -pdd;
  const double t2 = dot(phi, phi), th = sqrt(t2);
  double A, B, dA, dB;      // dA = dA/dth / th, dB = dB/dth / th
  if (th < 0.25) {
    A = 0.5 - t2 * (1.0 / 24.0 - t2 * (1.0 / 720.0 - t2 * (1.0 / 40320.0 - t2 * (1.0 / 3628800.0))));
    B = 1.0 / 6.0 - t2 * (1.0 / 120.0 - t2 * (1.0 / 5040.0 - t2 * (1.0 / 362880.0 - t2 * (1.0 / 39916800.0))));
    dA = -1.0 / 12.0 + t2 * (1.0 / 180.0 - t2 * (1.0 / 6720.0 - t2 * (1.0 / 453600.0 - t2 * (1.0 / 47900160.0))));
    dB = -1.0 / 60.0 + t2 * (1.0 / 1260.0 - t2 * (1.0 / 60480.0 - t2 * (1.0 / 4989600.0 - t2 * (1.0 / 622702080.0))));
  } else {
    double s, c;
    dsincos(th, &s, &c);
    const double i2 = 1.0 / t2, i4 = i2 * i2, it = 1.0 / th;
    A = (1.0 - c) * i2;
    B = (th - s) * i2 * it;
    dA = (th * s - 2.0 * (1.0 - c)) * i4;
    dB = ((1.0 - c) * th - 3.0 * (th - s)) * i4 * it;
  }
  const double pf = dot(phi, f);
  const V3 xf = cross(phi, f), xxf = cross(phi, xf), xff = cross(phi, ff), xxff = cross(phi, xff);
  return ff + A * xff + B * xxff + (dA * pf) * xf + (dB * pf) * xxf + B * cross(f, xf);
}

// the sum of v over the wave by a butterfly: the same order on every run, the same bits in every lane
DEV double align_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

constexpr int kAlignJacobiSweeps = 12;
// Eigenvalues (the diagonal of A afterwards) and eigenvectors (the columns of V) of a symmetric matrix by cyclic Jacobi; every
// index is a compile-time constant.
template <int N>
DEV void align_jacobi(double (&A)[N][N], double (&V)[N][N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int j = 0; j < N; ++j) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < kAlignJacobiSweeps; ++sweep) {
#pragma unroll
    for (int p = 0; p < N - 1; ++p) {
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double apq = A[p][q], app = A[p][p], aqq = A[q][q];
        const bool turn = fabs(apq) > 1e-300;
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
        double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        if (!turn || !__builtin_isfinite(s) || !__builtin_isfinite(c)) { c = 1.0; s = 0.0; }
#pragma unroll
        for (int k = 0; k < N; ++k) { const double x = A[k][p], y = A[k][q]; A[k][p] = c * x - s * y; A[k][q] = s * x + c * y; }
#pragma unroll
        for (int k = 0; k < N; ++k) { const double x = A[p][k], y = A[q][k]; A[p][k] = c * x - s * y; A[q][k] = s * x + c * y; }
#pragma unroll
        for (int k = 0; k < N; ++k) { const double x = V[k][p], y = V[k][q]; V[k][p] = c * x - s * y; V[k][q] = s * x + c * y; }
      }
    }
  }
}

}  // namespace cal
