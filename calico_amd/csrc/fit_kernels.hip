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
//                        forward and backward substitution of the six right-hand sides, all in LDS
// Accuracy (profiles/EXPERIMENTS.md, "spline fit accuracy"; tests/fit_ref.py is the reference): backward error of the normal
// equations ~5e-16 on every shape; control points within 0.2-0.7 x 1e-15 cond₂² max|C| of exact least squares on the kept
// columns (cond₂ theirs), fitted values never further and up to 6 decades closer as cond₂ grows. The pivot rule is a cliff: a control point whose pivot is <= 1e-13 mean_diag comes back ~0 even where
// X has full rank (order 6, 100 Hz samples on 10 Hz knots, last sample 10 % into the last segment: exact pivot 3.2e-16
// mean_diag, cond₂(X) 9.4e7, dropped; 20 %: 3.3e-13, roundoff decides; 30 %: 1.7e-11, cond₂ 4.1e5, kept).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_math.hpp"
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

__global__ __launch_bounds__(64) void fit_solve_kernel(int n, int k, const double* __restrict__ band_g, const double* __restrict__ rhs_g,
                                                       double* __restrict__ ctrl, int* status) {
  extern __shared__ double lds[];
  double* B = lds;                   // [n][k]  B[a][d] = L(a, a - d) after the factorisation
  double* Y = lds + size_t(n) * k;   // [n][6]
  const int lane = threadIdx.x;
  for (int i = lane; i < n * k; i += 64) B[i] = band_g[i];
  for (int i = lane; i < n * 6; i += 64) Y[i] = rhs_g[i];
  __syncthreads();
  double tr = 0.0;
  for (int i = lane; i < n; i += 64) tr += B[i * k];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) tr += __shfl_xor(tr, off, 64);
  const double mean_diag = tr / n;
  // keeps exact zeros away. It moves the control points by up to 1e-15 cond₂(X)² max|C| (measured with the Cholesky's own
  // error: 0.2-0.7 of that): 2e-9 at order 6 with the last segment covered (cond₂ 1.8e3), 1e-6 with it half covered
  // (cond₂ 4.3e4; the fitted values there move 4e-11), 1e-5 at order 8 with it covered (cond₂ 1.6e5)
  const double ridge = 1e-15 * mean_diag;
  for (int i = lane; i < n; i += 64) B[i * k] += ridge;
  __syncthreads();
  // right-looking banded Cholesky: lane (i, c), 1 <= c <= i < k, owns the update of entry (j+i, j+c)
  int ui = 0, uc = 0;
  {
    int t = lane, i = 1;
    while (i < k && t >= i) { t -= i; ++i; }
    if (i < k) { ui = i; uc = t + 1; }
  }
  bool bad = false;
  for (int j = 0; j < n; ++j) {
    double d = B[j * k];
    bad = bad || !isfinite(d);
    // a control point the samples do not determine (fewer samples than control points at the trajectory end: the
    // reference's pivoted QR returns roundoff there) is decoupled instead of dividing by noise
    if (!(d > 1e-13 * mean_diag)) d = mean_diag;
    const double inv = 1.0 / sqrt(d);
    __syncthreads();
    if (lane == 0) B[j * k] = d * inv;
    if (lane >= 1 && lane < k && j + lane < n) B[(j + lane) * k + lane] *= inv;      // L(j+i, j)
    __syncthreads();
    if (ui > 0 && j + ui < n) B[(j + ui) * k + (ui - uc)] -= B[(j + ui) * k + ui] * B[(j + uc) * k + uc];
    __syncthreads();
  }
  // forward then backward substitution, lane c < 6 per right-hand side
  if (lane < 6) {
    for (int a = 0; a < n; ++a) {
      double s = Y[a * 6 + lane];
      for (int d = 1; d < k && d <= a; ++d) s -= B[a * k + d] * Y[(a - d) * 6 + lane];
      Y[a * 6 + lane] = s / B[a * k];
    }
    for (int a = n - 1; a >= 0; --a) {
      double s = Y[a * 6 + lane];
      for (int d = 1; d < k && a + d < n; ++d) s -= B[(a + d) * k + d] * Y[(a + d) * 6 + lane];
      s /= B[a * k];
      Y[a * 6 + lane] = s;
      ctrl[size_t(a) * 6 + lane] = s;
    }
  }
  if (lane == 0) *status = bad ? 1 : 0;
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

}  // namespace cal
