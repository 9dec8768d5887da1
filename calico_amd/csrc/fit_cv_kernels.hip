// fit_cv_kernels.hip — the smoothing fit's lambda chosen by cross-validation on the device: the kernels of calico_fit_spline_cv
// (host: fit.cpp).
//
// Per channel group g and grid entry l the smoothing fit (fit_kernels.hip) solves A C = X^T W d, A = N + lambda P, N = X^T W X, and
// leaves the banded Cholesky factor of A in LDS. The hat matrix of that fit is H = X A^-1 X^T W: its diagonal h_j = w_j X_j A^-1 X_j^T
// gives the leave-one-out residuals e_j / (1 - h_j) without a refit, its trace tr(A^-1 N) the effective degrees of freedom. Both
// need only the entries of Z = A^-1 inside A's band, which Takahashi's recursion takes from the factor, last column first.
//   fit_cv_solve_kernel    one wave per (group, lambda): fit_smooth_solve_wave (fit_dev.hpp: the smoothing fit's own kernel body, so
//                          control points and row have its bits), then the selected inversion in place over L,
//                            Z(j+i, j) = - sum_c l_c Z(j+i, j+c),  Z(j, j) = 1 / L(j, j)^2 - sum_c l_c Z(j+c, j),  l_c = L(j+c, j) / L(j, j)
//                          (one reciprocal of L(j, j) a column, then products),
//                          lane (i, c) of the (k-1)^2 holding one product, lane (i, 1) summing its row in the order of c, lane 0 the
//                          diagonal in the order of i; one barrier per column. edf = sum over the band of Z o N; Z's band to global.
//                          A row whose factorisation was not finite or replaced a pivot gets no Z (edf NaN): its factor is not A's.
//   fit_cv_score_kernel    one lane per (sample, lambda, group): h_j from the k x k window of Z's band and the sample's k spline
//                          weights, e_j^2 from the lambda's control points, the PRESS term w e^2 / (1 - h)^2 (+inf at h >= 1); per
//                          block of 256 the sum (shuffle tree per wave, then the four waves in order) and the largest h.
//   fit_cv_choose_kernel   one wave, lane per (group, lambda): the partials summed in block order, gcv and press, the cv row; then
//                          per group the smallest score among the eligible rows (a tie goes to the larger lambda), the summary.
//   fit_cv_sample_kernel   one lane per (sample, group): h_j and e_j / (1 - h_j) at the group's chosen lambda.
// Z is the inverse of the matrix that was factored, A + 1e-15 mean_diag I (fit_band_solve's ridge). FP64 throughout, no atomics,
// every sum in a fixed order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_math.hpp"
#include "fit_dev.hpp"
#include "kernels.hpp"

namespace cal {

DEV double fit_cv_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
DEV double fit_cv_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// The band of Z = (L L^T)^-1 in place over L, one wave: B [n][k], B[a][d] = L(a, a - d) before and Z(a, a - d) afterwards. Column j
// reads column j of L and the entries of Z in rows and columns j+1 .. j+k-1 (row j+i holds them at d < i, column j of L at d = i).
DEV void fit_band_selected_inverse(int n, int k, double* B, int lane) {
  const int h = k - 1;
  int i = 0, c = 0;      // lane (i, c), 1 <= i, c <= k-1: the product l_c Z(j+i, j+c)
  if (lane < h * h) { i = lane / h + 1; c = lane - (i - 1) * h + 1; }
  for (int j = n - 1; j >= 0; --j) {
    const double inv = 1.0 / B[j * k];      // one division a column: l_c = L(j+c, j) inv, 1 / L(j, j)^2 = inv inv
    double p = 0.0, li = 0.0;
    if (i > 0 && j + i < n) {
      li = B[(j + i) * k + i] * inv;
      if (j + c < n) {
        const double lc = B[(j + c) * k + c] * inv;
        const double z = i >= c ? B[(j + i) * k + (i - c)] : B[(j + c) * k + (c - i)];
        p = lc * z;
      }
    }
    double s = p;      // lanes (i, 1): the row's products in the order of c
    for (int q = 1; q < h; ++q) s += __shfl_down(p, q, 64);
    const double zi = -s;
    const double t = li * zi;
    double acc = 0.0;      // every lane: sum_i l_i Z(j+i, j) in the order of i
    for (int q = 0; q < h; ++q) acc += __shfl(t, q * h, 64);
    if (c == 1 && j + i < n) B[(j + i) * k + i] = zi;
    if (lane == 0) B[j * k] = inv * inv - acc;
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void fit_cv_solve_kernel(FitSmoothArgs a, FitCvArgs c) {
  extern __shared__ double lds[];
  const int n = a.n_ctrl, k = a.k, g = blockIdx.x, l = blockIdx.y, lane = threadIdx.x;
  const FitSmoothRow row = fit_smooth_solve_wave(a, g, l, lane, lds);
  const size_t at = size_t(g) * a.n_lambda + l;
  if (row.status != 0 || row.replaced_pivots != 0) {
    if (lane == 0) c.edf[at] = fit_cv_nan();
    return;
  }
  double* B = lds;      // [n][k]: L
  fit_band_selected_inverse(n, k, B, lane);
  const double* N = a.band + size_t(g) * n * k;
  double e = 0.0;
  for (int r = lane; r < n; r += 64) {
    double off = 0.0;
    for (int d = 1; d < k && d <= r; ++d) off += B[r * k + d] * N[r * k + d];
    e += B[r * k] * N[r * k] + 2.0 * off;
  }
  e = fit_wave_sum(e);
  if (lane == 0) c.edf[at] = e;
  double* Z = c.zband + at * size_t(n) * k;
  for (int i = lane; i < n * k; i += 64) Z[i] = B[i];
}

// h_j = w X_j Z X_j^T over the window of segment s: rows s .. s+k-1 of Z's band, the sample's spline weights Wj [k]. Without
// contraction, here and in fit_cv_residual2: the score and the sample kernel then compute the same bits, so that a leave-one-out
// residual is +inf exactly where its row's PRESS saw h >= 1.
DEV double fit_cv_leverage(const double* __restrict__ Z, int k, int s, const double* __restrict__ Wj, double w) {
#pragma clang fp contract(off)
  double diag = 0.0, off = 0.0;
  for (int a = 0; a < k; ++a) {
    const double wa = Wj[a];
    const double* z = Z + size_t(s + a) * k;
    diag += wa * wa * z[0];
    double r = 0.0;
    for (int b = 0; b < a; ++b) r += Wj[b] * z[a - b];
    off += wa * r;
  }
  return w * (diag + 2.0 * off);
}

// |X_j C - d_j|^2 over the group's three channels; C: the lambda's control points at the sample's segment, stride 6
DEV double fit_cv_residual2(const double* __restrict__ C, int k, const double* __restrict__ Wj, const double* __restrict__ d) {
#pragma clang fp contract(off)
  double r0 = 0.0, r1 = 0.0, r2 = 0.0;
  for (int i = 0; i < k; ++i) {
    const double wi = Wj[i];
    r0 += wi * C[i * 6]; r1 += wi * C[i * 6 + 1]; r2 += wi * C[i * 6 + 2];
  }
  r0 -= d[0]; r1 -= d[1]; r2 -= d[2];
  return r0 * r0 + r1 * r1 + r2 * r2;
}

__global__ __launch_bounds__(256) void fit_cv_score_kernel(FitSmoothArgs a, FitCvArgs c) {
  extern __shared__ double part[];      // [4 waves][sum, max]
  const int l = blockIdx.y, g = blockIdx.z, k = a.k, n = a.n_ctrl;
  const size_t at = size_t(g) * a.n_lambda + l;
  const FitSmoothRow row = a.rows[at];
  if (row.status != 0 || row.replaced_pivots != 0) return;      // not eligible: fit_cv_choose_kernel does not read its partials
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  double term = 0.0, hmax = 0.0;
  if (j < a.n) {
    const double w = a.weights ? a.weights[size_t(j) * 2 + g] : 1.0;
    if (w != 0.0) {
      const int s = a.seg[j];
      const double* Wj = a.W + size_t(j) * k;
      const double h = fit_cv_leverage(c.zband + at * size_t(n) * k, k, s, Wj, w);
      const double e2 = fit_cv_residual2(a.ctrl_all + (size_t(l) * n + s) * 6 + 3 * g, k, Wj, a.data + size_t(j) * 6 + 3 * g);
      const double q = 1.0 - h;
      term = h < 1.0 ? w * e2 / (q * q) : fit_cv_inf();
      hmax = h;
    }
  }
  term = fit_wave_sum(term);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) hmax = fmax(hmax, __shfl_xor(hmax, off, 64));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { part[wave * 2] = term; part[wave * 2 + 1] = hmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* out = c.partial + (at * size_t(c.n_blocks) + blockIdx.x) * 2;
    out[0] = (part[0] + part[2]) + (part[4] + part[6]);
    out[1] = fmax(fmax(part[1], part[3]), fmax(part[5], part[7]));
  }
}

__global__ __launch_bounds__(64) void fit_cv_choose_kernel(FitSmoothArgs a, FitCvArgs c) {
  const int lane = threadIdx.x, nl = a.n_lambda;
  double edf = fit_cv_nan(), gcv = fit_cv_nan(), press = fit_cv_nan(), hmax = fit_cv_nan();
  int eligible = 0;
  if (lane < 2 * nl) {
    const int g = lane / nl;
    const FitSmoothRow row = a.rows[lane];
    eligible = row.status == 0 && row.replaced_pivots == 0;
    if (eligible) {
      const double nu = double(g == 0 ? a.n_used_rot : a.n_used_pos);
      edf = c.edf[lane];
      double sum = 0.0;
      hmax = 0.0;
      const double* p = c.partial + size_t(lane) * c.n_blocks * 2;
      for (int b = 0; b < c.n_blocks; ++b) { sum += p[size_t(b) * 2]; hmax = fmax(hmax, p[size_t(b) * 2 + 1]); }
      press = sum / (3.0 * nu);
      const double q = 1.0 - edf / nu;
      gcv = edf < nu ? (row.rss / (3.0 * nu)) / (q * q) : fit_cv_inf();
    }
    FitCvRow out;
    out.edf = edf; out.gcv = gcv; out.press = press; out.max_leverage = hmax;
    c.cv_rows[lane] = out;
  }
  const double score = c.criterion == CALICO_FIT_CV_PRESS ? press : gcv;
  if (score != score) eligible = 0;
  for (int g = 0; g < 2; ++g) {
    int best = -1;
    double best_score = 0.0;
    for (int l = 0; l < nl; ++l) {      // the grid ascends: of equal scores the later entry has the larger lambda
      const double s = __shfl(score, g * nl + l, 64);
      const int e = __shfl(eligible, g * nl + l, 64);
      if (e && (best < 0 || s <= best_score)) { best = l; best_score = s; }
    }
    const double best_edf = __shfl(edf, g * nl + (best < 0 ? 0 : best), 64);
    if (lane == 0) {
      FitCvSummary* sm = c.summary;
      sm->chosen[g] = best;
      sm->status[g] = best < 0 ? CALICO_FIT_NOT_POSITIVE_DEFINITE : nl >= 2 && (best == 0 || best == nl - 1) ? CALICO_FIT_CV_AT_GRID_END : CALICO_FIT_OK;
      sm->edf[g] = best < 0 ? fit_cv_nan() : best_edf;
      sm->score[g] = best < 0 ? fit_cv_nan() : best_score;
    }
  }
}

__global__ __launch_bounds__(256) void fit_cv_sample_kernel(FitSmoothArgs a, FitCvArgs c) {
  const int g = blockIdx.y, k = a.k, n = a.n_ctrl;
  const int l = c.summary->chosen[g];
  if (l < 0) return;      // no eligible row: the host leaves the group's outputs alone
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.n) return;
  const size_t out = size_t(j) * 2 + g;
  const double w = a.weights ? a.weights[out] : 1.0;
  if (w == 0.0) { c.leverage[out] = 0.0; c.loo[out] = fit_cv_nan(); return; }
  const size_t at = size_t(g) * a.n_lambda + l;
  const int s = a.seg[j];
  const double* Wj = a.W + size_t(j) * k;
  const double h = fit_cv_leverage(c.zband + at * size_t(n) * k, k, s, Wj, w);
  const double e2 = fit_cv_residual2(a.ctrl_all + (size_t(l) * n + s) * 6 + 3 * g, k, Wj, a.data + size_t(j) * 6 + 3 * g);
  c.leverage[out] = h;
  c.loo[out] = h < 1.0 ? sqrt(e2) / (1.0 - h) : fit_cv_inf();
}

hipError_t launch_fit_spline_cv(int device, const FitSmoothArgs& a, const FitCvArgs& c, hipStream_t s) {
  const size_t lds = fit_solve_smooth_lds_bytes(a.n_ctrl, a.k);
  const hipError_t e = raise_lds_limit(device, fit_cv_solve_kernel, lds);
  if (e != hipSuccess) return e;
  launch_fit_smooth_prepare(a, s);
  hipLaunchKernelGGL(fit_cv_solve_kernel, dim3(2, a.n_lambda), dim3(64), lds, s, a, c);
  hipLaunchKernelGGL(fit_cv_score_kernel, dim3(unsigned(c.n_blocks), a.n_lambda, 2), dim3(256), 8 * sizeof(double), s, a, c);
  hipLaunchKernelGGL(fit_cv_choose_kernel, dim3(1), dim3(64), 0, s, a, c);
  hipLaunchKernelGGL(fit_cv_sample_kernel, dim3(unsigned(c.n_blocks), 2), dim3(256), 0, s, a, c);
  return hipGetLastError();
}

}  // namespace cal
