// resect_dev.hpp — what the per-frame Levenberg-Marquardt kernels share (resect_kernels.hip: the pose of a frame at given
// intrinsics; calib_kernels.hip: the intrinsics and the poses of all frames; rig_kernels.hip: a rig: views and rig frames; all
// three through arrowhead_dev.hpp): one wave per frame, wave-uniform small dense systems in the wave's LDS area, quaternion
// helpers. The step rule itself is lm_rule.hpp's. Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "camera_inverse.hpp"
#include "lm_rule.hpp"
#include "problem_dev.hpp"

namespace cal {

namespace {

DEV bool uniform_flag(bool v) { return __builtin_amdgcn_readfirstlane(int(v)) != 0; }
DEV double uniform_value(double v) { return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v))); }

DEV double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// The small dense systems (8x8 of the start, 6x6 of a step) are wave-uniform: they live in the wave's LDS area and are worked on
// by loops with run-time bounds -- every lane reads the same addresses (broadcast) and computes the same bits, lane 0 stores. A
// wave's LDS operations execute in program order, so a later read sees the store; wave_fence keeps the compiler from moving one
// across the other. Registers stay free for the per-lane sums, and nothing is indexed at run time in registers (no scratch).
DEV void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
DEV void put(double* p, double v, int lane) { if (lane == 0) *p = v; }

// In-place Cholesky of the lower triangle of A (N x N, row-major, LDS). false: a pivot was not positive.
DEV bool lds_chol(double* A, int N, int lane) {
  bool ok = true;
#pragma unroll 1
  for (int j = 0; j < N; ++j) {
    double d = A[j * N + j];
#pragma unroll 1
    for (int k = 0; k < j; ++k) d -= A[j * N + k] * A[j * N + k];
    ok = ok && d > 0.0 && __builtin_isfinite(d);
    const double l = sqrt(ok ? d : 1.0), il = 1.0 / l;
    put(&A[j * N + j], l, lane);
#pragma unroll 1
    for (int i = j + 1; i < N; ++i) {
      double v = A[i * N + j];
#pragma unroll 1
      for (int k = 0; k < j; ++k) v -= A[i * N + k] * A[j * N + k];
      put(&A[i * N + j], v * il, lane);
    }
    wave_fence();
  }
  return uniform_flag(ok);
}
// b <- (L L^T)^-1 b
DEV void lds_chol_solve(const double* L, double* b, int N, int lane) {
#pragma unroll 1
  for (int i = 0; i < N; ++i) {
    double v = b[i];
#pragma unroll 1
    for (int k = 0; k < i; ++k) v -= L[i * N + k] * b[k];
    put(&b[i], v / L[i * N + i], lane);
    wave_fence();
  }
#pragma unroll 1
  for (int i = N - 1; i >= 0; --i) {
    double v = b[i];
#pragma unroll 1
    for (int k = i + 1; k < N; ++k) v -= L[k * N + i] * b[k];
    put(&b[i], v / L[i * N + i], lane);
    wave_fence();
  }
}

DEV Q4 quat_at(const double* p) { Q4 q; q.x = p[0]; q.y = p[1]; q.z = p[2]; q.w = p[3]; return q; }      // (x, y, z, w) in memory
DEV Q4 quat_mul(Q4 a, Q4 b) {      // R(a b) = R(a) R(b)
  Q4 r;
  r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  r.x = a.w * b.x + b.w * a.x + a.y * b.z - a.z * b.y;
  r.y = a.w * b.y + b.w * a.y + a.z * b.x - a.x * b.z;
  r.z = a.w * b.z + b.w * a.z + a.x * b.y - a.y * b.x;
  return r;
}
DEV Q4 quat_of(const M3& R) {      // Shepperd: the largest of w, x, y, z is the divisor
  const double tr = R.m[0][0] + R.m[1][1] + R.m[2][2];
  Q4 q;
  if (tr > 0.0) {
    const double s = 2.0 * sqrt(1.0 + tr);
    q.w = 0.25 * s; q.x = (R.m[2][1] - R.m[1][2]) / s; q.y = (R.m[0][2] - R.m[2][0]) / s; q.z = (R.m[1][0] - R.m[0][1]) / s;
  } else if (R.m[0][0] > R.m[1][1] && R.m[0][0] > R.m[2][2]) {
    const double s = 2.0 * sqrt(1.0 + R.m[0][0] - R.m[1][1] - R.m[2][2]);
    q.w = (R.m[2][1] - R.m[1][2]) / s; q.x = 0.25 * s; q.y = (R.m[0][1] + R.m[1][0]) / s; q.z = (R.m[0][2] + R.m[2][0]) / s;
  } else if (R.m[1][1] > R.m[2][2]) {
    const double s = 2.0 * sqrt(1.0 + R.m[1][1] - R.m[0][0] - R.m[2][2]);
    q.w = (R.m[0][2] - R.m[2][0]) / s; q.x = (R.m[0][1] + R.m[1][0]) / s; q.y = 0.25 * s; q.z = (R.m[1][2] + R.m[2][1]) / s;
  } else {
    const double s = 2.0 * sqrt(1.0 + R.m[2][2] - R.m[0][0] - R.m[1][1]);
    q.w = (R.m[1][0] - R.m[0][1]) / s; q.x = (R.m[0][2] + R.m[2][0]) / s; q.y = (R.m[1][2] + R.m[2][1]) / s; q.z = 0.25 * s;
  }
  return q;
}
DEV Q4 canonical(Q4 q) {      // unit, w >= 0
  q = normalized(q);
  if (q.w < 0.0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
  return q;
}
DEV bool finite_pose(Q4 q, V3 t) {
  return __builtin_isfinite(q.x) && __builtin_isfinite(q.y) && __builtin_isfinite(q.z) && __builtin_isfinite(q.w) && finite3(t);
}

// the two validity bits of a pair's flag byte (bit 0: usable for the resection's start): valid at pose slot 0 / 1
DEV uint8_t pose_bit(int which) { return uint8_t(2u << which); }

}  // namespace
}  // namespace cal
