// camera_kernels.hip — the camera model as a map over free pixels and points (no residual blocks, no trajectory):
//   camera_unproject_kernel<MODEL>            pixel -> unit-norm point (camera_inverse.hpp), one lane per pixel
//   camera_project_points_kernel<MODEL, JAC>  camera-frame point -> pixel: project<> itself, with d pix / d point and
//                                             d pix / d intrinsics on request, one lane per point
//   projection_uncertainty_kernel<MODEL>      pixel -> [s_uu, s_uv, s_vv] of S_pix = G S_tt G^T, one lane per pixel
// Throughput kernels over up to millions of elements, unlike the rest of the library: FP64 VALU, no LDS staging of per-lane
// data, no scratch, many waves per SIMD. The intrinsics (and the extrinsics of the uncertainty map) are read through
// wave-uniform addresses, i.e. by scalar loads into SGPRs; S_tt (at most 17 x 17) sits in LDS, loaded once per workgroup and
// read with same-address (broadcast) reads. Tail lanes of the last wave read and write nothing.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/calico_hip.h"
#include "camera_inverse.hpp"
#include "kernels.hpp"

namespace cal {

constexpr int kCameraThreads = 256;

template <int MODEL>
__global__ __launch_bounds__(kCameraThreads) void camera_unproject_kernel(const double* __restrict__ k, long long n,
                                                                          const double* __restrict__ pixels,
                                                                          double* __restrict__ bearings, uint8_t* __restrict__ valid) {
  const long long i = static_cast<long long>(blockIdx.x) * kCameraThreads + threadIdx.x;
  const bool live = i < n;
  double u = 0.0, v = 0.0;
  if (live) { u = pixels[2 * i]; v = pixels[2 * i + 1]; }
  V3 b;
  const bool ok = unproject<MODEL>(k, u, v, live, &b);
  if (live) {
    bearings[3 * i] = b.x; bearings[3 * i + 1] = b.y; bearings[3 * i + 2] = b.z;
    valid[i] = ok ? 1 : 0;
  }
}

template <int MODEL, bool JAC>
__global__ __launch_bounds__(kCameraThreads) void camera_project_points_kernel(const double* __restrict__ k, long long n,
                                                                               const double* __restrict__ points,
                                                                               double* __restrict__ pixels, uint8_t* __restrict__ valid,
                                                                               double* __restrict__ d_point, double* __restrict__ d_intr) {
  constexpr int K = CamK<MODEL>::K;
  const long long i = static_cast<long long>(blockIdx.x) * kCameraThreads + threadIdx.x;
  if (i >= n) return;
  const V3 P = mk(points[3 * i], points[3 * i + 1], points[3 * i + 2]);
  double pix[2] = {0.0, 0.0}, D[2][3], dK[2][kMaxIntr];
  bool ok = project<MODEL, JAC>(k, P, pix, D, dK);
  ok = ok && __builtin_isfinite(pix[0]) && __builtin_isfinite(pix[1]);
  pixels[2 * i] = ok ? pix[0] : 0.0; pixels[2 * i + 1] = ok ? pix[1] : 0.0;
  if (valid) valid[i] = ok ? 1 : 0;
  if constexpr (JAC) {
    if (d_point) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) d_point[6 * i + 3 * r + c] = ok ? D[r][c] : 0.0;
    }
    if (d_intr) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int c = 0; c < K; ++c) d_intr[2 * K * i + K * r + c] = ok ? dK[r][c] : 0.0;
    }
  }
}

// theta = [intrinsics K | q 3 | t 3]; sigma is (K + 6) x (K + 6) row-major, the rows and columns of a constant block (and, in
// the camera frame, of q and t) zero. Rig frame: the point is fixed in the sensor-rig frame at p_r = R_rc p_c + t_rc, so
// p_c = R_rc^T (p_r - t_rc) moves with the extrinsics: d p_c / d t = -R_rc^T, d p_c / d delta = 2 R_rc^T [p_r - t_rc]x in the
// EigenQuaternion tangent (q (+) delta = [sin|delta| delta / |delta|, cos|delta|] * q), as the residual kernels' columns.
template <int MODEL>
__global__ __launch_bounds__(kCameraThreads) void projection_uncertainty_kernel(UncertaintyArgs a) {
  constexpr int K = CamK<MODEL>::K, NT = K + 6;
  __shared__ double S[NT * NT];
  for (int e = threadIdx.x; e < NT * NT; e += kCameraThreads) S[e] = a.sigma[e];
  __syncthreads();
  const long long i = static_cast<long long>(blockIdx.x) * kCameraThreads + threadIdx.x;
  const bool live = i < a.n;
  double u = 0.0, v = 0.0;
  if (live) { u = a.pixels[2 * i]; v = a.pixels[2 * i + 1]; }
  V3 b;
  bool ok = unproject<MODEL>(a.k, u, v, live, &b);
  if (!live) return;
  const V3 pc = a.range * b;
  double pix[2], D[2][3], dK[2][kMaxIntr];
  ok = ok && project<MODEL, true>(a.k, pc, pix, D, dK);
  double g[2][NT];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
#pragma unroll
    for (int c = 0; c < K; ++c) g[r][c] = dK[r][c];
#pragma unroll
    for (int c = K; c < NT; ++c) g[r][c] = 0.0;
  }
  if (a.frame == CALICO_FRAME_RIG) {
    Q4 q; q.x = a.q[0]; q.y = a.q[1]; q.z = a.q[2]; q.w = a.q[3];
    const M3 R = rotmat(normalized(q));
    const V3 y = mul(R, pc);      // p_r - t_rc
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      double T[3];                // D R_rc^T
#pragma unroll
      for (int j = 0; j < 3; ++j) T[j] = D[r][0] * R.m[j][0] + D[r][1] * R.m[j][1] + D[r][2] * R.m[j][2];
      g[r][K] = 2.0 * (T[1] * y.z - T[2] * y.y); g[r][K + 1] = 2.0 * (T[2] * y.x - T[0] * y.z); g[r][K + 2] = 2.0 * (T[0] * y.y - T[1] * y.x);
      g[r][K + 3] = -T[0]; g[r][K + 4] = -T[1]; g[r][K + 5] = -T[2];
    }
  }
  double suu = 0.0, suv = 0.0, svv = 0.0;
#pragma unroll
  for (int r = 0; r < NT; ++r) {
    double w0 = 0.0, w1 = 0.0;
#pragma unroll
    for (int c = 0; c < NT; ++c) { const double s = S[r * NT + c]; w0 += s * g[0][c]; w1 += s * g[1][c]; }
    suu += g[0][r] * w0; suv += g[0][r] * w1; svv += g[1][r] * w1;
  }
  ok = ok && __builtin_isfinite(suu) && __builtin_isfinite(suv) && __builtin_isfinite(svv);
  a.cov[3 * i] = ok ? suu : 0.0; a.cov[3 * i + 1] = ok ? suv : 0.0; a.cov[3 * i + 2] = ok ? svv : 0.0;
  a.valid[i] = ok ? 1 : 0;
}

namespace {
unsigned camera_grid(long long n) { return unsigned((n + kCameraThreads - 1) / kCameraThreads); }
}  // namespace

int camera_model_num_params(int model) {
  switch (model) {
    case 1: return CamK<1>::K; case 2: return CamK<2>::K; case 3: return CamK<3>::K; case 4: return CamK<4>::K;
    case 5: return CamK<5>::K; case 6: return CamK<6>::K; case 7: return CamK<7>::K; default: return -1;
  }
}

hipError_t launch_camera_unproject(int model, const double* k, long long n, const double* pixels, double* bearings, uint8_t* valid,
                                   hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const dim3 grid(camera_grid(n)), block(kCameraThreads);
  return with_camera_model(model, [&](auto m) { hipLaunchKernelGGL(camera_unproject_kernel<decltype(m)::value>, grid, block, 0, s, k, n, pixels, bearings, valid); });
}

hipError_t launch_camera_project_points(int model, const double* k, long long n, const double* points, double* pixels, uint8_t* valid,
                                        double* d_point, double* d_intr, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const dim3 grid(camera_grid(n)), block(kCameraThreads);
  return with_camera_model(model, [&](auto m) {
    constexpr int M = decltype(m)::value;
    if (d_point || d_intr) hipLaunchKernelGGL((camera_project_points_kernel<M, true>), grid, block, 0, s, k, n, points, pixels, valid, d_point, d_intr);
    else hipLaunchKernelGGL((camera_project_points_kernel<M, false>), grid, block, 0, s, k, n, points, pixels, valid, d_point, d_intr);
  });
}

hipError_t launch_projection_uncertainty(int model, const UncertaintyArgs& a, hipStream_t s) {
  if (a.n <= 0) return hipSuccess;
  const dim3 grid(camera_grid(a.n)), block(kCameraThreads);
  return with_camera_model(model, [&](auto m) { hipLaunchKernelGGL(projection_uncertainty_kernel<decltype(m)::value>, grid, block, 0, s, a); });
}

}  // namespace cal
