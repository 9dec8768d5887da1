// fit_kernels.hip — spline initialisation on the device: the kernels of calico_fit_spline (host: fit.cpp).
//
// BSpline::FitToData / FitSpline (bspline.hpp:19-37, 246-297) solves the least-squares problem
//   min_C || X C - data ||²,  X(j, si_j + a) = w_a(t_j)  (k non-zeros per row, si = GetSplineIndex(t)),
// with a dense column-pivoted QR of the normal equations XᵀX -- cubic in the trajectory length (the reference's own
// TODO, bspline.hpp:287-289, notes that the system is banded). Here: the normal equations XᵀX C = Xᵀdata are banded
// SPD with half bandwidth k-1, assembled without atomics and solved by a banded Cholesky in LDS.
//   fit_weights_kernel   one thread per sample: spline weights (bspline.hpp:39-72, derivative 0) -> W[n][k]
//   fit_normal_kernel    one thread per entry of [band(n_ctrl, k) | rhs(n_ctrl, 6)]: fixed-order sum over the samples
//                        of the segments that touch the control point (samples are sorted, seg_ptr is a CSR)
//   fit_solve_kernel     one wave: banded Cholesky (tiny ridge; pivots the samples do not determine -- the trajectory end
//                        can have fewer samples than control points, where the reference's QR result is
//                        roundoff-defined -- are decoupled),
//                        forward and backward substitution of the six right-hand sides, all in LDS (fit_band_solve, shared
//                        with the smoothing fit below: calico_fit_spline_smooth, its kernels after fit_solve_kernel)
// Accuracy (profiles/EXPERIMENTS.md, "spline fit accuracy"; tests/fit_ref.py is the reference): backward error of the normal
// equations ~5e-16 on every shape; control points within 0.2-0.7 x 1e-15 cond₂² max|C| of exact least squares on the kept
// columns (cond₂ theirs), fitted values never further and up to 6 decades closer as cond₂ grows. The pivot rule is a cliff: a control point whose pivot is <= 1e-13 mean_diag comes back ~0 even where
// X has full rank (order 6, 100 Hz samples on 10 Hz knots, last sample 10 % into the last segment: exact pivot 3.2e-16
// mean_diag, cond₂(X) 9.4e7, dropped; 20 %: 3.3e-13, roundoff decides; 30 %: 1.7e-11, cond₂ 4.1e5, kept).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_math.hpp"
#include "fit_dev.hpp"
#include "kernels.hpp"

namespace cal {

__global__ void fit_weights_kernel(int n, int k, const double* __restrict__ stamps, const int* __restrict__ seg,
                                   const double* __restrict__ knots, const double* __restrict__ basis, double* __restrict__ W) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int s = seg[j], ki = s + k - 1;
  double w[1][kMaxOrder];
  spline_weights<1, 0>(k, knots[ki], knots[ki + 1], basis + size_t(s) * k * k, stamps[j], w);
#pragma unroll
  for (int a = 0; a < kMaxOrder; ++a) if (a < k) W[size_t(j) * k + a] = w[0][a];
}

// entry e of row a: e < k -> N(a, a - e) (lower band), e >= k -> rhs(a, e - k)
__global__ void fit_normal_kernel(int n_ctrl, int n_seg, int k, const double* __restrict__ W, const double* __restrict__ data,
                                  const int* __restrict__ seg_ptr, double* __restrict__ band, double* __restrict__ rhs) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int per = k + 6;
  if (t >= n_ctrl * per) return;
  const int a = t / per, e = t - a * per;
  double acc = 0.0;
  const int s_lo = max(0, a - (k - 1)), s_hi = min(a, n_seg - 1);
  for (int s = s_lo; s <= s_hi; ++s) {
    const int ia = a - s;                       // local index of control point a in segment s
    const int ib = e < k ? ia - e : 0;          // local index of control point a - e
    if (e < k && ib < 0) continue;
    for (int q = seg_ptr[s]; q < seg_ptr[s + 1]; ++q) {
      const double wa = W[size_t(q) * k + ia];
      acc += e < k ? wa * W[size_t(q) * k + ib] : wa * data[size_t(q) * 6 + (e - k)];
    }
  }
  if (e < k) band[size_t(a) * k + e] = acc; else rhs[size_t(a) * 6 + (e - k)] = acc;
}

// (fit_band_solve, the solve every fit shares, one wave on [B | Y] in LDS: fit_dev.hpp)
__global__ __launch_bounds__(64) void fit_solve_kernel(int n, int k, const double* __restrict__ band_g, const double* __restrict__ rhs_g,
                                                       double* __restrict__ ctrl, int* status) {
  extern __shared__ double lds[];
  double* B = lds;                   // [n][k]
  double* Y = lds + size_t(n) * k;   // [n][6]
  const int lane = threadIdx.x;
  for (int i = lane; i < n * k; i += 64) B[i] = band_g[i];
  for (int i = lane; i < n * 6; i += 64) Y[i] = rhs_g[i];
  __syncthreads();
  bool bad;
  int replaced;
  fit_band_solve<6>(n, k, B, Y, lane, &bad, &replaced);
  for (int i = lane; i < n * 6; i += 64) ctrl[i] = Y[i];
  if (lane == 0) *status = bad ? 1 : 0;
}

// ---- the smoothing fit (calico_fit_spline_smooth):  min_C sum_j w_j |X_j C - d_j|² + lambda ∫ |s^(m)(t)|² dt  per channel group
// (0: axis-angle, channels 0..2; 1: position, channels 3..5), for a whole grid of lambda in one launch.
//   fit_penalty_kernel          one thread per band entry of P (n_ctrl x k), the Gram matrix of the m-th derivatives of the basis
//                               functions: per segment of length D with basis matrix M (row = power of u),
//                               P_seg = D^(1-2m) Mᵀ H M,  H_ij = c_i c_j / (i + j - 2m + 1),  c_i = i! / (i - m)!  (i, j >= m)
//   fit_normal_weighted_kernel  one thread per entry of [band | 3 rhs] per group: fit_normal_kernel's sum with w_{j,g} applied; a
//                               sample of weight 0 is skipped (its data are not read). Without weights the sum is fit_normal_kernel's.
//   fit_solve_smooth_kernel     one wave per (group, lambda): A = N_g + lambda P in LDS, fit_band_solve, c'Pc, the weighted rss, the row

// entry e of row a: P(a, a - e), summed over the segments that hold both control points, in segment order
__global__ void fit_penalty_kernel(int n_ctrl, int n_seg, int k, int m, const double* __restrict__ knots, const double* __restrict__ basis,
                                   double* __restrict__ P) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_ctrl * k) return;
  const int a = t / k, e = t - a * k;
  double acc = 0.0;
  const int s_lo = max(0, a - (k - 1)), s_hi = min(a, n_seg - 1);
  for (int s = s_lo; s <= s_hi; ++s) {
    const int ia = a - s, ib = ia - e;
    if (ib < 0) continue;
    const double* M = basis + size_t(s) * k * k;
    const double delta = knots[s + k] - knots[s + k - 1];
    double scale = delta;                                     // D^(1 - 2m)
    for (int q = 0; q < 2 * m; ++q) scale /= delta;
    double seg = 0.0;
    for (int i = m; i < k; ++i) {
      double ci = 1.0;
      for (int q = 0; q < m; ++q) ci *= double(i - q);
      double row = 0.0;
      for (int j = m; j < k; ++j) {
        double cj = 1.0;
        for (int q = 0; q < m; ++q) cj *= double(j - q);
        row += (ci * cj / double(i + j - 2 * m + 1)) * M[j * k + ib];
      }
      seg += M[i * k + ia] * row;
    }
    acc += scale * seg;
  }
  P[size_t(a) * k + e] = acc;
}

// entry e of row a of group g: e < k -> N_g(a, a - e), e >= k -> rhs_g(a, e - k); weights [n][2] (WEIGHTED) or none
template <bool WEIGHTED>
__global__ void fit_normal_weighted_kernel(int n_ctrl, int n_seg, int k, const double* __restrict__ W, const double* __restrict__ data,
                                           const double* __restrict__ weights, const int* __restrict__ seg_ptr, double* __restrict__ band,
                                           double* __restrict__ rhs) {
  fit_normal_weighted_entry<WEIGHTED>(blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y, n_ctrl, n_seg, k, W, data, weights, seg_ptr, band, rhs);      // fit_dev.hpp
}

// (fit_smooth_solve_wave, one (group, lambda) of the grid from A = N + lambda P to its row: fit_dev.hpp, shared with the
// cross-validated fit, fit_cv_kernels.hip)
__global__ __launch_bounds__(64) void fit_solve_smooth_kernel(FitSmoothArgs a) {
  extern __shared__ double lds[];
  fit_smooth_solve_wave(a, blockIdx.x, blockIdx.y, threadIdx.x, lds);
}

size_t fit_solve_lds_bytes(int n_ctrl, int k) { return (size_t(n_ctrl) * k + size_t(n_ctrl) * 6) * sizeof(double); }

hipError_t launch_fit_spline(int device, const FitArgs& a, hipStream_t s) {
  const hipError_t e = raise_lds_limit(device, fit_solve_kernel, fit_solve_lds_bytes(a.n_ctrl, a.k));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fit_weights_kernel, dim3(unsigned((a.n + 255) / 256)), dim3(256), 0, s, a.n, a.k, a.stamps, a.seg, a.knots, a.basis, a.W);
  const int n_entries = a.n_ctrl * (a.k + 6);
  hipLaunchKernelGGL(fit_normal_kernel, dim3((n_entries + 255) / 256), dim3(256), 0, s, a.n_ctrl, a.n_seg, a.k, a.W, a.data, a.seg_ptr, a.band,
                     a.rhs);
  hipLaunchKernelGGL(fit_solve_kernel, dim3(1), dim3(64), fit_solve_lds_bytes(a.n_ctrl, a.k), s, a.n_ctrl, a.k, a.band, a.rhs, a.ctrl, a.status);
  return hipGetLastError();
}

size_t fit_solve_smooth_lds_bytes(int n_ctrl, int k) { return (size_t(n_ctrl) * k + size_t(n_ctrl) * 3) * sizeof(double); }

// what every (group, lambda) solve reads: the spline weights W, the penalty band P, and [band | 3 rhs] of both groups
void launch_fit_smooth_prepare(const FitSmoothArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(fit_weights_kernel, dim3(unsigned((a.n + 255) / 256)), dim3(256), 0, s, a.n, a.k, a.stamps, a.seg, a.knots, a.basis, a.W);
  hipLaunchKernelGGL(fit_penalty_kernel, dim3((a.n_ctrl * a.k + 255) / 256), dim3(256), 0, s, a.n_ctrl, a.n_seg, a.k, a.derivative, a.knots, a.basis,
                     a.P);
  const dim3 grid((a.n_ctrl * (a.k + 3) + 255) / 256, 2);
  if (a.weights)
    hipLaunchKernelGGL(fit_normal_weighted_kernel<true>, grid, dim3(256), 0, s, a.n_ctrl, a.n_seg, a.k, a.W, a.data, a.weights, a.seg_ptr, a.band, a.rhs);
  else
    hipLaunchKernelGGL(fit_normal_weighted_kernel<false>, grid, dim3(256), 0, s, a.n_ctrl, a.n_seg, a.k, a.W, a.data, a.weights, a.seg_ptr, a.band, a.rhs);
}

hipError_t launch_fit_spline_smooth(int device, const FitSmoothArgs& a, hipStream_t s) {
  const size_t lds = fit_solve_smooth_lds_bytes(a.n_ctrl, a.k);
  const hipError_t e = raise_lds_limit(device, fit_solve_smooth_kernel, lds);
  if (e != hipSuccess) return e;
  launch_fit_smooth_prepare(a, s);
  hipLaunchKernelGGL(fit_solve_smooth_kernel, dim3(2, a.n_lambda), dim3(64), lds, s, a);
  return hipGetLastError();
}

}  // namespace cal
