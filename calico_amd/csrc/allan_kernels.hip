// allan_kernels.hip — the overlapping Allan variance of the three axes of a static IMU log: the kernels of calico_imu_allan
// (host: allan.cpp; the coefficient fit is the host's, allan_fit.hpp).
//
// Per axis, with dt = 1 / rate: theta_0 = 0, theta_k = dt Sum_{i<k} (y_i - mean), and for a cluster size m, tau = m dt,
//   avar(m) = Sum_{k=0}^{n-2m-1} (theta_{k+2m} - 2 theta_{k+m} + theta_k)^2 / (2 tau^2 (n - 2m)).
// The prefix sum has three phases over blocks of kAllanScanBlock samples, a thread holding kAllanScanBlock / 256 consecutive ones:
//   allan_block_sum_kernel   per block and axis the sum of y: a thread's samples in order, the wave sum, the four waves in order. A
//                            sample that is not finite sets the axis' flag word: a plain store of 1 from every lane that sees one.
//   allan_offsets_kernel     one workgroup, wave c for axis c: the block sums in lane stride and the wave sum give the mean; then
//                            the exclusive scan of block_sum_b - count_b mean, 64 blocks a step (a shuffle scan and a carry).
//   allan_theta_kernel       every block again: y - mean summed along a thread's samples, a shuffle scan of the threads' totals,
//                            the waves before it in order, the block's offset; theta, planar (n + 1 per axis), times dt.
// Then the sums, three loads a term, the planes unit-stride:
//   allan_variance_kernel    grid (chunk, cluster size, axis): a workgroup sums the kAllanTermChunk terms of its chunk, a thread
//                            the pairs (k, k + 1), k = chunk start + 512 q + 2 thread, q ascending; theta_k and theta_{k+2m} come
//                            as one 16-byte load each, theta_{k+m} too where m is even. The wave sum (fit_dev.hpp), the four waves
//                            in order, one partial. The second difference is formed as (theta_{k+2m} - theta_{k+m}) -
//                            (theta_{k+m} - theta_k): neighbours' differences first. Chunks past n - 2m exit at once.
//   allan_finish_kernel      one wave per (cluster size, axis): its partials in lane stride, index ascending, the wave sum, the
//                            scale; NaN for an axis whose flag is set. The flags follow the variances in the same buffer.
// FP64 throughout, no read-modify-write of memory that another thread writes, and every sum in an order that n and m alone fix:
// the variance of an axis does not depend on the other axes or on which other cluster sizes the grid holds.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_math.hpp"
#include "fit_dev.hpp"
#include "kernels.hpp"

namespace cal {

constexpr int kAllanThreads = 256;
constexpr int kAllanPerThread = kAllanScanBlock / kAllanThreads;
constexpr int kAllanPairSteps = kAllanTermChunk / (2 * kAllanThreads);
static_assert(kAllanPerThread * kAllanThreads == kAllanScanBlock && kAllanPairSteps * 2 * kAllanThreads == kAllanTermChunk,
              "a workgroup of 256 covers a block and a chunk in whole steps");

// The inclusive sum over the lanes of a wave, lane order.
DEV double allan_wave_scan(double v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  return v;
}

__global__ __launch_bounds__(256) void allan_block_sum_kernel(AllanArgs a) {
  __shared__ double part[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i0 = (long long)blockIdx.x * kAllanScanBlock + (long long)threadIdx.x * kAllanPerThread;
  double s[3] = {0.0, 0.0, 0.0};
  bool bad[3] = {false, false, false};
#pragma unroll
  for (int q = 0; q < kAllanPerThread; ++q) {
    const long long i = i0 + q;
    if (i < a.n) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double y = a.samples[size_t(i) * 3 + c];
        s[c] += y;
        bad[c] = bad[c] || !isfinite(y);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (bad[c]) a.flags[c] = 1;
    s[c] = fit_wave_sum(s[c]);
    if (lane == 0) part[wave][c] = s[c];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    a.block_sum[size_t(c) * a.n_blocks + blockIdx.x] = (part[0][c] + part[1][c]) + (part[2][c] + part[3][c]);
  }
}

__global__ __launch_bounds__(256) void allan_offsets_kernel(AllanArgs a) {
  const int lane = threadIdx.x & 63, c = threadIdx.x >> 6, nb = a.n_blocks;
  if (c >= 3) return;
  const double* sums = a.block_sum + size_t(c) * nb;
  double* offsets = a.offsets + size_t(c) * nb;
  double total = 0.0;
  for (int b = lane; b < nb; b += 64) total += sums[b];
  const double mean = fit_wave_sum(total) / double(a.n);
  if (lane == 0) a.mean[c] = mean;
  double carry = 0.0;
  for (int b0 = 0; b0 < nb; b0 += 64) {
    const int b = b0 + lane;
    double d = 0.0;
    if (b < nb) d = fma(-double(min(kAllanScanBlock, a.n - b * kAllanScanBlock)), mean, sums[b]);
    const double inclusive = allan_wave_scan(d, lane);
    const double before = __shfl_up(inclusive, 1, 64);
    if (b < nb) offsets[b] = lane == 0 ? carry : carry + before;
    carry += __shfl(inclusive, 63, 64);
  }
}

__global__ __launch_bounds__(256) void allan_theta_kernel(AllanArgs a) {
  __shared__ double wave_total[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i0 = (long long)blockIdx.x * kAllanScanBlock + (long long)threadIdx.x * kAllanPerThread;
  const double mean[3] = {a.mean[0], a.mean[1], a.mean[2]};
  double run[kAllanPerThread][3];      // the thread's inclusive sums
  double s[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < kAllanPerThread; ++q) {
    const long long i = i0 + q;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (i < a.n) s[c] += a.samples[size_t(i) * 3 + c] - mean[c];
      run[q][c] = s[c];
    }
  }
  double base[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double inclusive = allan_wave_scan(s[c], lane);
    const double before = __shfl_up(inclusive, 1, 64);
    base[c] = lane == 0 ? 0.0 : before;
    if (lane == 63) wave_total[wave][c] = inclusive;
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double start = a.offsets[size_t(c) * a.n_blocks + blockIdx.x];
    for (int w = 0; w < wave; ++w) start += wave_total[w][c];
    base[c] += start;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0)
    for (int c = 0; c < 3; ++c) a.theta[size_t(c) * a.plane] = 0.0;
#pragma unroll
  for (int q = 0; q < kAllanPerThread; ++q) {
    const long long i = i0 + q;
    if (i < a.n) {
#pragma unroll
      for (int c = 0; c < 3; ++c) a.theta[size_t(c) * a.plane + size_t(i) + 1] = a.dt * (base[c] + run[q][c]);
    }
  }
}

DEV double allan_term(double lo, double mid, double hi) {
  const double d = (hi - mid) - (mid - lo);
  return d * d;
}

__global__ __launch_bounds__(256) void allan_variance_kernel(AllanArgs a) {
  __shared__ double part[4];
  const int j = blockIdx.y, c = blockIdx.z, m = a.m[j];
  const int terms = a.n - 2 * m;
  const long long first = (long long)blockIdx.x * kAllanTermChunk;
  if (first >= terms) return;
  const double* th = a.theta + size_t(c) * a.plane;
  const bool mid_aligned = (m & 1) == 0;
  double acc = 0.0;
#pragma unroll
  for (int q = 0; q < kAllanPairSteps; ++q) {
    const int k = int(first) + q * (2 * kAllanThreads) + 2 * int(threadIdx.x);      // even: th + k and th + k + 2m lie on 16 bytes
    if (k + 1 < terms) {
      const double2 lo = *reinterpret_cast<const double2*>(th + k);
      const double2 hi = *reinterpret_cast<const double2*>(th + k + 2 * m);
      double2 mid;
      if (mid_aligned) {
        mid = *reinterpret_cast<const double2*>(th + k + m);
      } else {
        mid.x = th[k + m]; mid.y = th[k + m + 1];
      }
      acc += allan_term(lo.x, mid.x, hi.x);
      acc += allan_term(lo.y, mid.y, hi.y);
    } else if (k < terms) {
      acc += allan_term(th[k], th[k + m], th[k + 2 * m]);
    }
  }
  acc = fit_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) a.partial[(size_t(c) * a.n_clusters + j) * a.n_chunks + blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

__global__ __launch_bounds__(64) void allan_finish_kernel(AllanArgs a) {
  const int j = blockIdx.x, c = blockIdx.y, lane = threadIdx.x, m = a.m[j];
  const int terms = a.n - 2 * m, chunks = allan_chunks(a.n, m);
  const double* p = a.partial + (size_t(c) * a.n_clusters + j) * a.n_chunks;
  double s = 0.0;
  for (int b = lane; b < chunks; b += 64) s += p[b];
  s = fit_wave_sum(s);
  const int flag = a.flags[c];
  if (lane == 0) {
    const double tau = double(m) * a.dt;
    a.out[size_t(j) * 3 + c] = flag ? __longlong_as_double(0x7ff8000000000000ll) : s / (2.0 * tau * tau * double(terms));
    if (j == 0) a.out[size_t(a.n_clusters) * 3 + c] = double(flag);
  }
}

hipError_t launch_imu_allan(const AllanArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(allan_block_sum_kernel, dim3(unsigned(a.n_blocks)), dim3(kAllanThreads), 0, s, a);
  hipLaunchKernelGGL(allan_offsets_kernel, dim3(1), dim3(kAllanThreads), 0, s, a);
  hipLaunchKernelGGL(allan_theta_kernel, dim3(unsigned(a.n_blocks)), dim3(kAllanThreads), 0, s, a);
  hipLaunchKernelGGL(allan_variance_kernel, dim3(unsigned(a.n_chunks), unsigned(a.n_clusters), 3), dim3(kAllanThreads), 0, s, a);
  hipLaunchKernelGGL(allan_finish_kernel, dim3(unsigned(a.n_clusters), 3), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace cal
