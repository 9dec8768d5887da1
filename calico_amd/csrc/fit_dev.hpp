// fit_dev.hpp — the device code the spline fits share (fit_kernels.hip: calico_fit_spline and calico_fit_spline_smooth;
// fit_robust_kernels.hip: calico_fit_spline_robust; fit_cv_kernels.hip: calico_fit_spline_cv): the banded Cholesky solve in LDS, the
// wave sum, one entry of the weighted normal equations, and one (group, lambda) of the smoothing fit's grid. One definition each,
// so that a fit that repeats another's step repeats its bits.
#pragma once
#include <hip/hip_runtime.h>

#include "device_math.hpp"
#include "kernels.hpp"

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

// One (group g, grid entry l) of the smoothing fit, one wave: A = N_g + lambda P in LDS ([n_ctrl][k] band | [n_ctrl][3] rhs, the
// caller's dynamic LDS), fit_band_solve, the control points into ctrl_all, c'Pc, the weighted rss, the row (written to a.rows and
// returned, wave-uniform). Afterwards the band in LDS holds the Cholesky factor L (of A + ridge) and the rhs the control points.
DEV FitSmoothRow fit_smooth_solve_wave(const FitSmoothArgs& a, int g, int l, int lane, double* lds) {
  const int n = a.n_ctrl, k = a.k;
  double* B = lds;                   // [n][k]
  double* Y = lds + size_t(n) * k;   // [n][3]
  const double* N = a.band + size_t(g) * n * k;
  const double* rhs = a.rhs + size_t(g) * n * 3;
  double lambda = g == 0 ? a.lambda_rot[l] : a.lambda_pos[l];
  if (a.relative) {      // in units of trace(N_g) / trace(P)
    double tn = 0.0, tp = 0.0;
    for (int i = lane; i < n; i += 64) { tn += N[i * k]; tp += a.P[i * k]; }
    lambda *= fit_wave_sum(tn) / fit_wave_sum(tp);
  }
  if (lambda == 0.0) {
    for (int i = lane; i < n * k; i += 64) B[i] = N[i];
  } else {
    for (int i = lane; i < n * k; i += 64) B[i] = N[i] + lambda * a.P[i];
  }
  for (int i = lane; i < n * 3; i += 64) Y[i] = rhs[i];
  __syncthreads();
  bool bad;
  int replaced;
  fit_band_solve<3>(n, k, B, Y, lane, &bad, &replaced);
  FitSmoothRow row;
  row.status = bad ? 1 : 0; row.replaced_pivots = replaced; row.lambda = lambda;
  if (bad) {      // this lambda's control points are not written; its sums are not numbers
    row.rss = row.penalty = row.rms = __longlong_as_double(0x7ff8000000000000ll);
  } else {
    double* out = a.ctrl_all + size_t(l) * n * 6 + 3 * g;
    for (int i = lane; i < n * 3; i += 64) out[(i / 3) * 6 + i % 3] = Y[i];
    // c' P c over the three channels: row a of P times c, then c_a times that
    double pen = 0.0;
    for (int r = lane; r < n; r += 64) {
      double p0 = 0.0, p1 = 0.0, p2 = 0.0;
      for (int b = max(0, r - (k - 1)); b <= min(n - 1, r + (k - 1)); ++b) {
        const double p = b <= r ? a.P[size_t(r) * k + (r - b)] : a.P[size_t(b) * k + (b - r)];
        p0 += p * Y[b * 3]; p1 += p * Y[b * 3 + 1]; p2 += p * Y[b * 3 + 2];
      }
      pen += Y[r * 3] * p0 + Y[r * 3 + 1] * p1 + Y[r * 3 + 2] * p2;
    }
    row.penalty = fit_wave_sum(pen);
    // the weighted residual sum of squares: lanes stride over the samples, then one fixed shuffle tree
    double rss = 0.0;
    for (int j = lane; j < a.n; j += 64) {
      const double w = a.weights ? a.weights[size_t(j) * 2 + g] : 1.0;
      if (w == 0.0) continue;
      const int s = a.seg[j];
      double r0 = 0.0, r1 = 0.0, r2 = 0.0;
      for (int i = 0; i < k; ++i) {
        const double wi = a.W[size_t(j) * k + i];
        r0 += wi * Y[(s + i) * 3]; r1 += wi * Y[(s + i) * 3 + 1]; r2 += wi * Y[(s + i) * 3 + 2];
      }
      const double* d = a.data + size_t(j) * 6 + 3 * g;
      r0 -= d[0]; r1 -= d[1]; r2 -= d[2];
      rss += w * (r0 * r0 + r1 * r1 + r2 * r2);
    }
    row.rss = fit_wave_sum(rss);
    row.rms = sqrt(row.rss / (3.0 * double(g == 0 ? a.n_used_rot : a.n_used_pos)));
  }
  if (lane == 0) a.rows[size_t(g) * a.n_lambda + l] = row;
  return row;
}

}  // namespace cal
