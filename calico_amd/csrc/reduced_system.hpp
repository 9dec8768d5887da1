// reduced_system.hpp — how covariance_kernel (cov_kernels.hip) and observability_kernel (obs_kernels.hip) take in the reduced
// system the linear solve leaves behind: Spart = [ks K-slices][(m+1)²], lower triangle, rows [calibration (mc) | extra rows
// (m - mc)]. Both kernels drop the same columns and add the slices in the same order, so Σ and the observability report describe
// the same matrix, bit for bit. Nothing here is accumulated atomically.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace cal {

// Compact order, by wave 0 (lane: the caller's lane in it): the extra rows FIRST, then the calibration columns whose JᵀJ
// diagonal (Cdiag: the border's block of the reduce buffer) is not exactly 0.0 -- a ballot per 64 columns. s_idx: compact row
// -> row of Spart. Returns the number of calibration columns kept.
__device__ __forceinline__ int reduced_compact_order(int* s_idx, const double* __restrict__ Cdiag, int m, int mc, int lane) {
  const int nr = m - mc;
  int cnt = 0;
  for (int b0 = 0; b0 < mc; b0 += 64) {
    const int j = b0 + lane;
    const bool keep = j < mc && Cdiag[size_t(min(j, mc - 1)) * (mc + 1)] != 0.0;
    const unsigned long long bal = __ballot(keep);
    const int pos = cnt + __popcll(bal & ((1ull << lane) - 1ull));
    if (keep) s_idx[nr + pos] = j;
    cnt += __popcll(bal);
  }
  for (int r = lane; r < nr; r += 64) s_idx[r] = mc + r;
  return cnt;
}

// The lower triangle of the compact system (n rows, through s_idx) into A (row stride LD), by the whole workgroup of THREADS
// threads: slice 0, then slices 1 .. ks - 1 added in slice order (fixed order: repeated computes and the two kernels are
// bit-consistent). Returns whether this thread met a non-finite sum; merging that over the workgroup is the caller's.
template <int THREADS>
__device__ __forceinline__ int reduced_load_lower(double* A, int LD, int n, const int* s_idx, const double* __restrict__ Spart, int ks, int m,
                                                  int tid) {
  const int m1 = m + 1;
  const size_t msq = size_t(m1) * m1;
  int bad = 0;
  for (int e = tid; e < n * n; e += THREADS) {
    const int p = e / n, q = e - p * n;
    if (q > p) continue;
    const int oi = s_idx[p], oj = s_idx[q];
    const size_t o = size_t(max(oi, oj)) * m1 + min(oi, oj);
    double v = Spart[o];
    for (int k = 1; k < ks; ++k) v += Spart[size_t(k) * msq + o];
    bad |= !isfinite(v);
    A[p * LD + q] = v;
  }
  return bad;
}

}  // namespace cal
