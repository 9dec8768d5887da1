// fit_robust_kernels.hip — the robust spline fit on the device: the kernels of calico_fit_spline_robust (host: fit.cpp).
//
// Iteratively reweighted least squares around the smoothing fit (fit_kernels.hip), one independent loop per channel group g
// (0: axis-angle, channels 0..2; 1: position, channels 3..5). Iteration 0 is launch_fit_spline_smooth itself with one lambda; its
// absolute lambda is frozen. Iteration t = 1..T of a group, every kernel reading the group's control word first:
//   fit_robust_residual_kernel  one lane per (sample, group): e_j = |X_j C - d_j|_2 from W[n][k] and the control points; NaN where
//                               the prior weight is 0 (data not read). Block 0 clears the iteration's digit counts and counters.
//   fit_robust_select_kernel    x 8: the exact lower median of e over the samples of weight > 0, by radix selection on the bit
//                               patterns (non-negative doubles are monotone as unsigned integers), 8 bits a pass from the top.
//                               Every wave re-derives the digits chosen so far from the earlier passes' counts (a wave scan of
//                               256 integers), counts its samples that share them in LDS, and adds the block's counts to the
//                               pass's 256 global integers. Integer additions only: any order gives the same counts.
//   fit_robust_weight_kernel    the eighth digit, sigma = max(median / sqrt(median chi2_3), min_scale) or the caller's scale,
//                               u = psi(e / sigma), w u into the [n][2] buffer of the normal equations; counts 0 < u < 1 and u == 0.
//                               sigma == 0: the group stops (CALICO_FIT_SCALE_ZERO), all u = 1.
//   fit_robust_normal_kernel    fit_normal_weighted_kernel's sum (fit_dev.hpp) with w u for weights
//   fit_robust_solve_kernel     one wave per group: A = N + lambda_abs P in LDS, fit_band_solve, the step
//                               max|C - C_prev| / max|C| (0 where nothing moved), the control word
// and after the last iteration one more residual pass at the final control points (unconditional) and
//   fit_robust_rss_kernel       one wave per group: sum w u e^2, lanes striding over the samples, one shuffle tree.
// No floating-point atomics; every floating-point sum in a fixed order; psi is evaluated without contraction, so that it is the
// float64 expression bit for bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_math.hpp"
#include "fit_dev.hpp"
#include "kernels.hpp"

namespace cal {

namespace {
constexpr double kChi3MedianRoot = 1.5381722544550522;      // sqrt(median of chi2 with 3 degrees of freedom)
constexpr int kDigits = 8, kBins = 256;
}  // namespace

DEV double fit_robust_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// The bin that holds rank *r of 256 counts, and the rank inside that bin: every lane of the wave gets both.
DEV void fit_robust_digit(const int* h, int lane, int* r, int* digit) {
  const int c0 = h[lane * 4], c1 = h[lane * 4 + 1], c2 = h[lane * 4 + 2], c3 = h[lane * 4 + 3];
  const int s = c0 + c1 + c2 + c3;
  int incl = s;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  const int excl = incl - s;
  const unsigned long long mine = __ballot(excl <= *r && *r < incl);
  const int src = mine ? __ffsll(mine) - 1 : 0;
  int rr = *r - excl, d = 0;
  if (rr >= c0) { rr -= c0; d = 1; if (rr >= c1) { rr -= c1; d = 2; if (rr >= c2) { rr -= c2; d = 3; } } }
  *digit = __shfl(lane * 4 + d, src, 64);
  *r = __shfl(rr, src, 64);
}

// psi(e / sigma) as the float64 expression, operation by operation
DEV double fit_robust_psi(int loss, double e, double sigma, double c) {
#pragma clang fp contract(off)
  const double z = e / sigma;
  if (loss == CALICO_ROBUST_HUBER) {
    const double q = c / z;
    return q < 1.0 ? q : 1.0;
  }
  if (!(z < c)) return 0.0;
  const double s = z / c;
  const double a = 1.0 - s * s;
  return a * a;
}

// lanes 0, 1: the state of a group after iteration 0, from the smoothing fit's row
__global__ void fit_robust_begin_kernel(FitSmoothArgs a, FitRobustArgs r) {
  const int g = threadIdx.x;
  if (g >= 2) return;
  const FitSmoothRow row = a.rows[g];
  FitRobustState st;
  st.status = row.status != 0 ? CALICO_FIT_NOT_POSITIVE_DEFINITE : CALICO_FIT_OK;
  st.done_iter = row.status != 0 || r.max_iterations == 0 ? 1 : 0;
  st.iterations = 0; st.replaced_pivots = row.replaced_pivots; st.n_downweighted = 0; st.n_rejected = 0;
  st.lambda = row.lambda;
  st.scale = st.median = st.last_step = st.rss = fit_robust_nan();
  r.state[g] = st;
}

__global__ void fit_robust_residual_kernel(FitSmoothArgs a, FitRobustArgs r, int final_pass) {
  const int g = blockIdx.y, k = a.k;
  if (!final_pass && r.state[g].done_iter != 0) return;
  if (!final_pass && blockIdx.x == 0) {
    for (int i = threadIdx.x; i < kDigits * kBins; i += blockDim.x) r.hist[g * kDigits * kBins + i] = 0;
    if (threadIdx.x == 0) { r.state[g].n_downweighted = 0; r.state[g].n_rejected = 0; }
  }
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.n) return;
  const double w = a.weights ? a.weights[size_t(j) * 2 + g] : 1.0;
  if (w == 0.0) { r.e[size_t(j) * 2 + g] = fit_robust_nan(); return; }
  const double* C = a.ctrl_all + size_t(a.seg[j]) * 6 + 3 * g;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0;
  for (int i = 0; i < k; ++i) {
    const double wi = a.W[size_t(j) * k + i];
    r0 += wi * C[i * 6]; r1 += wi * C[i * 6 + 1]; r2 += wi * C[i * 6 + 2];
  }
  const double* d = a.data + size_t(j) * 6 + 3 * g;
  r0 -= d[0]; r1 -= d[1]; r2 -= d[2];
  r.e[size_t(j) * 2 + g] = sqrt(r0 * r0 + r1 * r1 + r2 * r2);
}

__global__ void fit_robust_select_kernel(FitSmoothArgs a, FitRobustArgs r, int pass) {
  extern __shared__ int block_hist[];      // [256]
  const int g = blockIdx.y, lane = threadIdx.x & 63;
  if (r.state[g].done_iter != 0 || r.fixed_scale[g] > 0.0) return;
  unsigned long long prefix = 0;
  int rank = r.rank[g];
  for (int q = 0; q < pass; ++q) {
    int d;
    fit_robust_digit(r.hist + (g * kDigits + q) * kBins, lane, &rank, &d);
    prefix = (prefix << 8) | (unsigned long long)d;
  }
  for (int i = threadIdx.x; i < kBins; i += blockDim.x) block_hist[i] = 0;
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x; j < a.n; j += stride) {
    const double w = a.weights ? a.weights[size_t(j) * 2 + g] : 1.0;
    if (w == 0.0) continue;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(r.e[size_t(j) * 2 + g]);
    if (pass == 0 || (bits >> (shift + 8)) == prefix) atomicAdd(&block_hist[int((bits >> shift) & 255ull)], 1);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kBins; i += blockDim.x)
    if (block_hist[i] != 0) atomicAdd(&r.hist[(g * kDigits + pass) * kBins + i], block_hist[i]);
}

__global__ void fit_robust_weight_kernel(FitSmoothArgs a, FitRobustArgs r, int t) {
  const int g = blockIdx.y, lane = threadIdx.x & 63;
  const int done = r.state[g].done_iter;
  if (done != 0 && done != t + 1) return;      // (t + 1: this launch's own block 0 has just stopped the group at sigma == 0)
  double med = fit_robust_nan(), sigma = r.fixed_scale[g];
  if (!(sigma > 0.0)) {
    unsigned long long bits = 0;
    int rank = r.rank[g];
    for (int q = 0; q < kDigits; ++q) {
      int d;
      fit_robust_digit(r.hist + (g * kDigits + q) * kBins, lane, &rank, &d);
      bits = (bits << 8) | (unsigned long long)d;
    }
    med = __longlong_as_double((long long)bits);
    sigma = fmax(med / kChi3MedianRoot, r.min_scale[g]);
  }
  const bool zero = !(sigma > 0.0);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    r.state[g].scale = sigma; r.state[g].median = med;
    if (zero) { r.state[g].status = CALICO_FIT_SCALE_ZERO; r.state[g].done_iter = t + 1; }
  }
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.n) return;
  const size_t at = size_t(j) * 2 + g;
  const double w = a.weights ? a.weights[at] : 1.0;
  if (w == 0.0) { r.u[at] = 0.0; r.wu[at] = 0.0; return; }
  if (zero) { r.u[at] = 1.0; r.wu[at] = w; return; }
  const double u = fit_robust_psi(r.loss, r.e[at], sigma, r.tuning[g]);
  r.u[at] = u; r.wu[at] = w * u;
  const unsigned long long active = __ballot(1), down = __ballot(u > 0.0 && u < 1.0), rejected = __ballot(u == 0.0);
  if (lane == __ffsll(active) - 1) {
    if (down) atomicAdd(&r.state[g].n_downweighted, __popcll(down));
    if (rejected) atomicAdd(&r.state[g].n_rejected, __popcll(rejected));
  }
}

__global__ void fit_robust_normal_kernel(FitSmoothArgs a, FitRobustArgs r) {
  if (r.state[blockIdx.y].done_iter != 0) return;
  fit_normal_weighted_entry<true>(blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y, a.n_ctrl, a.n_seg, a.k, a.W, a.data, r.wu, a.seg_ptr, a.band,
                                  a.rhs);
}

__global__ __launch_bounds__(64) void fit_robust_solve_kernel(FitSmoothArgs a, FitRobustArgs r, int t) {
  extern __shared__ double lds[];
  const int n = a.n_ctrl, k = a.k, g = blockIdx.x, lane = threadIdx.x;
  FitRobustState* st = r.state + g;
  if (st->done_iter != 0) return;
  double* B = lds;                   // [n][k]
  double* Y = lds + size_t(n) * k;   // [n][3]
  const double* N = a.band + size_t(g) * n * k;
  const double* rhs = a.rhs + size_t(g) * n * 3;
  const double lambda = st->lambda;      // iteration 0's absolute lambda: the objective does not move with the weights
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
  if (bad) {      // the group keeps the previous control points
    if (lane == 0) { st->status = CALICO_FIT_NOT_POSITIVE_DEFINITE; st->done_iter = t + 1; }
    return;
  }
  double* C = a.ctrl_all + 3 * g;
  double moved = 0.0, size = 0.0;
  for (int i = lane; i < n * 3; i += 64) {
    double* c = C + (i / 3) * 6 + i % 3;
    moved = fmax(moved, fabs(Y[i] - *c));
    size = fmax(size, fabs(Y[i]));
    *c = Y[i];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    moved = fmax(moved, __shfl_xor(moved, off, 64));
    size = fmax(size, __shfl_xor(size, off, 64));
  }
  const double step = moved == 0.0 ? 0.0 : moved / size;
  if (lane == 0) {
    st->iterations = t; st->last_step = step; st->replaced_pivots = replaced;
    if (r.step_tolerance > 0.0 && step <= r.step_tolerance) { st->status = CALICO_FIT_OK; st->done_iter = t + 1; }
    else if (t == r.max_iterations) { st->status = CALICO_FIT_MAX_ITERATIONS; st->done_iter = t + 1; }
  }
}

__global__ __launch_bounds__(64) void fit_robust_rss_kernel(FitSmoothArgs a, FitRobustArgs r) {
  const int g = blockIdx.x, lane = threadIdx.x;
  double rss = 0.0;
  for (long long j = lane; j < a.n; j += 64) {
    const size_t at = size_t(j) * 2 + g;
    const double w = a.weights ? a.weights[at] : 1.0;
    if (w == 0.0) continue;
    const double e = r.e[at];
    rss += (w * r.u[at]) * (e * e);
  }
  rss = fit_wave_sum(rss);
  if (lane == 0) r.state[g].rss = rss;
}

hipError_t launch_fit_spline_robust(int device, const FitSmoothArgs& a, const FitRobustArgs& r, hipStream_t s) {
  const size_t lds = fit_solve_smooth_lds_bytes(a.n_ctrl, a.k);
  hipError_t e = raise_lds_limit(device, fit_robust_solve_kernel, lds);
  if (e != hipSuccess) return e;
  if ((e = launch_fit_spline_smooth(device, a, s)) != hipSuccess) return e;      // iteration 0
  hipLaunchKernelGGL(fit_robust_begin_kernel, dim3(1), dim3(64), 0, s, a, r);
  const unsigned sample_blocks = unsigned((a.n + 255) / 256);
  const dim3 samples(sample_blocks, 2), chosen(sample_blocks < 1024u ? sample_blocks : 1024u, 2);
  const dim3 entries((a.n_ctrl * (a.k + 3) + 255) / 256, 2);
  const bool select = !(r.fixed_scale[0] > 0.0 && r.fixed_scale[1] > 0.0);
  for (int t = 1; t <= r.max_iterations; ++t) {
    hipLaunchKernelGGL(fit_robust_residual_kernel, samples, dim3(256), 0, s, a, r, 0);
    if (select)
      for (int pass = 0; pass < kDigits; ++pass)
        hipLaunchKernelGGL(fit_robust_select_kernel, chosen, dim3(256), kBins * sizeof(int), s, a, r, pass);
    hipLaunchKernelGGL(fit_robust_weight_kernel, samples, dim3(256), 0, s, a, r, t);
    hipLaunchKernelGGL(fit_robust_normal_kernel, entries, dim3(256), 0, s, a, r);
    hipLaunchKernelGGL(fit_robust_solve_kernel, dim3(2), dim3(64), lds, s, a, r, t);
  }
  hipLaunchKernelGGL(fit_robust_residual_kernel, samples, dim3(256), 0, s, a, r, 1);
  hipLaunchKernelGGL(fit_robust_rss_kernel, dim3(2), dim3(64), 0, s, a, r);
  return hipGetLastError();
}

}  // namespace cal
