// fit_dev.hpp — the device code the spline fits share (fit_kernels.hip: calico_fit_spline and calico_fit_spline_smooth;
// fit_robust_kernels.hip: calico_fit_spline_robust): the banded Cholesky solve in LDS, the wave sum, and one entry of the weighted
// normal equations. One definition each, so that a fit that repeats another's step repeats its bits.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.hpp"

namespace cal {

// The solve every fit shares, one wave on [B | Y] in LDS: B [n][k] is the lower band of the matrix (B[a][d] = A(a, a - d); L(a, a - d)
// afterwards), Y [n][NRHS] the right-hand sides (the solution afterwards). Ridge of 1e-15 mean_diag of B, right-looking banded
// Cholesky with the pivot rule, forward and backward substitution. Returns through `bad` whether a pivot was not finite and
// through `replaced` how many pivots the rule replaced (both wave-uniform). The caller has synchronised after filling B and Y.
template <int NRHS>
DEV void fit_band_solve(int n, int k, double* B, double* Y, int lane, bool* bad_out, int* replaced_out) {
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
  int replaced = 0;
  for (int j = 0; j < n; ++j) {
    double d = B[j * k];
    bad = bad || !isfinite(d);
    // a control point the samples do not determine (fewer samples than control points at the trajectory end: the
    // reference's pivoted QR returns roundoff there) is decoupled instead of dividing by noise
    if (!(d > 1e-13 * mean_diag)) { d = mean_diag; ++replaced; }
    const double inv = 1.0 / sqrt(d);
    __syncthreads();
    if (lane == 0) B[j * k] = d * inv;
    if (lane >= 1 && lane < k && j + lane < n) B[(j + lane) * k + lane] *= inv;      // L(j+i, j)
    __syncthreads();
    if (ui > 0 && j + ui < n) B[(j + ui) * k + (ui - uc)] -= B[(j + ui) * k + ui] * B[(j + uc) * k + uc];
    __syncthreads();
  }
  // forward then backward substitution, lane c < NRHS per right-hand side
  if (lane < NRHS) {
    for (int a = 0; a < n; ++a) {
      double s = Y[a * NRHS + lane];
      for (int d = 1; d < k && d <= a; ++d) s -= B[a * k + d] * Y[(a - d) * NRHS + lane];
      Y[a * NRHS + lane] = s / B[a * k];
    }
    for (int a = n - 1; a >= 0; --a) {
      double s = Y[a * NRHS + lane];
      for (int d = 1; d < k && a + d < n; ++d) s -= B[(a + d) * k + d] * Y[(a + d) * NRHS + lane];
      s /= B[a * k];
      Y[a * NRHS + lane] = s;
    }
  }
  __syncthreads();
  *bad_out = bad;
  *replaced_out = replaced;
}

DEV double fit_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// Entry t = (a, e) of [band | 3 rhs] of group g: e < k -> N_g(a, a - e), e >= k -> rhs_g(a, e - k); weights [n][2] (WEIGHTED) or none.
// A fixed-order sum over the samples of the segments that touch control point a; a sample of weight 0 is skipped, its data not read.
template <bool WEIGHTED>
DEV void fit_normal_weighted_entry(int t, int g, int n_ctrl, int n_seg, int k, const double* __restrict__ W, const double* __restrict__ data,
                                   const double* __restrict__ weights, const int* __restrict__ seg_ptr, double* __restrict__ band,
                                   double* __restrict__ rhs) {
  const int per = k + 3;
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
      if (WEIGHTED) {
        const double w = weights[size_t(q) * 2 + g];
        if (w == 0.0) continue;
        acc += e < k ? wa * (W[size_t(q) * k + ib] * w) : wa * (data[size_t(q) * 6 + 3 * g + (e - k)] * w);
      } else {
        acc += e < k ? wa * W[size_t(q) * k + ib] : wa * data[size_t(q) * 6 + 3 * g + (e - k)];
      }
    }
  }
  if (e < k) band[(size_t(g) * n_ctrl + a) * k + e] = acc; else rhs[(size_t(g) * n_ctrl + a) * 3 + (e - k)] = acc;
}

}  // namespace cal
