// cov_kernels.hip — marginal covariance of the calibration blocks on gfx950 (calico_covariance_compute).
//
// Input: the reduced system the linear solve leaves behind, Spart = [ks K-slices][(m+1)²], lower triangle, rows
// [calibration (mc) | extra rows (m - mc): the tree solver's root superblock or the banded solver's separator] and the
// right-hand side in row m (ignored here) -- formed UNDAMPED and unscaled by the covariance pass (calico_hip.cpp). It is
// the Schur complement of JᵀJ onto those rows, so the calibration block of its inverse is the marginal covariance
//   Σ_cc = (S_cc - S_cx S_xx⁻¹ S_xc)⁻¹.
// One workgroup:
//   1. calibration columns whose JᵀJ diagonal is exactly 0.0 (no residual reaches them) are dropped; the compact order
//      puts the extra rows FIRST, so that after they are eliminated what is left of the factor is L_c, the Cholesky
//      factor of the calibration block's Schur complement;
//   2. the K-slices are added up in slice order (fixed order: repeated computes are bit-identical), the matrix is
//      equilibrated symmetrically to a unit diagonal (D A D, D = diag(1/sqrt(A_ii)));
//   3. right-looking FP64 Cholesky, one column per step. The calibration columns carry identity rows along (rows of
//      X = [0 | I] riding as extra rows of the elimination: they come out as X L⁻ᵀ = [0 | L_c⁻ᵀ]), stored in the unused
//      upper triangle of the calibration block, their diagonal in LDS. A pivot is the relative pivot: the equilibrated
//      diagonal is 1;
//   4. Σ_eq = L_c⁻ᵀ L_c⁻¹ = Z Zᵀ (Z = L_c⁻ᵀ, upper triangular), Σ = D Σ_eq D into the mc×mc result, zero rows and columns
//      for the dropped columns.
// The matrix lives in LDS when it fits (configs[3]: 121 rows), in a global workspace otherwise (L2-resident: 0.5 MB at
// configs[4]). No private arrays: nothing is indexed at run time outside LDS / global memory (scratch 0 B).
#include <hip/hip_runtime.h>

#include <cmath>

#include "problem_dev.hpp"
#include "solve_dev.hpp"

namespace cal {

namespace {
constexpr int kCovThreads = 1024;
constexpr int kCovMaxDim = 1024;        // rows of the reduced system the kernel takes (static LDS below: 28 KB)
constexpr size_t kCovLdsBudget = 160 * 1024;
constexpr size_t kCovStaticLds = kCovMaxDim * (sizeof(int) + 3 * sizeof(double)) + 64;
}  // namespace

int covariance_max_dim() { return kCovMaxDim; }
int covariance_ld(int n) { return n | 1; }       // odd row stride: the column walks of LDS hit distinct banks
bool covariance_in_lds(int n) { return size_t(n) * covariance_ld(n) * sizeof(double) + kCovStaticLds + 1024 <= kCovLdsBudget; }

// info[0]: minimum relative pivot, info[1]: flags (1 non-finite input, 2 pivot not positive, 4 the reduction's own factorisation
// failed, 8 non-finite result), info[2]: dropped
// (structurally unobserved) calibration columns, info[3]: rows factored
template <bool IN_LDS>
__global__ __launch_bounds__(kCovThreads) void covariance_kernel(const double* __restrict__ Spart, int ks, int m, int mc,
                                                                 const double* __restrict__ Cdiag, const LmState* __restrict__ st,
                                                                 double* __restrict__ work, double* __restrict__ out, double* __restrict__ info) {
  extern __shared__ double lds_dyn[];
  __shared__ int s_idx[kCovMaxDim];          // compact row -> row of Spart
  __shared__ double s_d[kCovMaxDim];         // equilibration D
  __shared__ double s_col[kCovMaxDim];       // column j of the factor (rows > j)
  __shared__ double s_z[kCovMaxDim];         // the carried rows' multipliers of step j
  __shared__ int s_nkeep, s_flags;
  __shared__ double s_minpiv;
  double* const A = IN_LDS ? lds_dyn : work;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nr = m - mc, m1 = m + 1;
  const size_t msq = size_t(m1) * m1;
  // ---- 1. compact order: extra rows, then the observed calibration columns (a ballot per 64 columns) ----
  if (wave == 0) {
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
    if (lane == 0) { s_nkeep = cnt; s_flags = (st->chol_failed ? 4 : 0); s_minpiv = 1.0; }
  }
  for (size_t e = tid; e < size_t(mc) * mc; e += kCovThreads) out[e] = 0.0;
  __syncthreads();
  const int nc = s_nkeep, n = nr + nc, LD = n | 1;
  // ---- 2. load (slices added in order), equilibrate ----
  int bad = 0;
  for (int e = tid; e < n * n; e += kCovThreads) {
    const int p = e / n, q = e - p * n;
    if (q > p) continue;
    const int oi = s_idx[p], oj = s_idx[q];
    const size_t o = size_t(max(oi, oj)) * m1 + min(oi, oj);
    double v = Spart[o];
    for (int k = 1; k < ks; ++k) v += Spart[size_t(k) * msq + o];
    bad |= !isfinite(v);
    A[p * LD + q] = v;
  }
  if (bad) atomicOr(&s_flags, 1);
  __syncthreads();
  for (int p = tid; p < n; p += kCovThreads) {
    const double v = A[p * LD + p];
    const bool ok = v > 0.0 && isfinite(v);
    if (!ok) atomicOr(&s_flags, 2);
    s_d[p] = ok ? 1.0 / sqrt(v) : 1.0;
  }
  __syncthreads();
  for (int e = tid; e < n * n; e += kCovThreads) {
    const int p = e / n, q = e - p * n;
    if (q <= p) A[p * LD + q] *= s_d[p] * s_d[q];
    else if (p >= nr) A[p * LD + q] = 0.0;        // carried rows of the calibration columns start as [0 | I] (their 1 is implied at its step)
  }
  __syncthreads();
  // ---- 3. Cholesky, root / separator rows first; the identity rows of the calibration columns ride along ----
  // Carried row c (calibration column nr + c): entry (c, j) sits at A[(nr + c) * LD + j] for j > nr + c, its diagonal
  // entry (j = nr + c) is 1 until its step. Rows c with nr + c > j are still zero at step j and take no part.
  const int ti = tid >> 5, tc = tid & 31;
  for (int j = 0; j < n; ++j) {
    const double piv = A[j * LD + j];
    if (!(piv > 0.0) || !isfinite(piv)) {       // (uniform: every thread reads the same entry)
      if (tid == 0) { s_flags |= 2; s_minpiv = fmin(s_minpiv, piv > 0.0 ? piv : 0.0); }
      break;
    }
    const double rs = 1.0 / sqrt(piv);
    for (int i = j + 1 + tid; i < n; i += kCovThreads) { const double l = A[i * LD + j] * rs; A[i * LD + j] = l; s_col[i] = l; }
    if (tid == 0) s_minpiv = fmin(s_minpiv, piv);
    // multipliers of the carried rows: Z(c, j) /= L_jj (c <= j - nr); the diagonal one is the identity's 1. The factor's
    // own diagonal is never read again, so the diagonal slot (j, j) takes Z(j - nr, j) = 1 / L_jj -- but only behind the
    // step's barrier: every thread reads the pivot from that slot at the top of the step.
    const int nz = j >= nr ? j - nr + 1 : 0;
    for (int c = tid; c < nz; c += kCovThreads) {
      const bool diag = nr + c == j;
      const double z = (diag ? 1.0 : A[(nr + c) * LD + j]) * rs;
      if (!diag) A[(nr + c) * LD + j] = z;      // (an entry above the diagonal: nobody else reads it in this step)
      s_z[c] = z;
    }
    __syncthreads();
    if (j >= nr && tid == 0) A[j * LD + j] = s_z[j - nr];
    // trailing update of the lower triangle and of the carried rows
    for (int i = j + 1 + ti; i < n; i += 32) {
      const double li = s_col[i];
      for (int c = j + 1 + tc; c <= i; c += 32) A[i * LD + c] -= li * s_col[c];
    }
    for (int c = ti; c < nz; c += 32) {
      const double zc = s_z[c];
      for (int q = j + 1 + tc; q < n; q += 32) A[(nr + c) * LD + q] -= zc * s_col[q];
    }
    __syncthreads();
  }
  __syncthreads();      // (a failed pivot leaves the loop with thread 0's flag just written)
  // ---- 4. Σ = D Z Zᵀ D, Z(a, q) for q >= nr + a ----
  const bool failed = s_flags != 0;
  if (!failed) {
    const int npair = nc * (nc + 1) / 2;
    for (int e = tid; e < npair; e += kCovThreads) {
      int a = int((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
      while (a * (a + 1) / 2 > e) --a;
      while ((a + 1) * (a + 2) / 2 <= e) ++a;
      const int b = e - a * (a + 1) / 2;       // b <= a
      const double* za = A + size_t(nr + a) * LD;
      const double* zb = A + size_t(nr + b) * LD;
      double s = 0.0;
      for (int q = nr + a; q < n; ++q) s += za[q] * zb[q];
      const double v = s * s_d[nr + a] * s_d[nr + b];
      const int ia = s_idx[nr + a], ib = s_idx[nr + b];
      out[size_t(ia) * mc + ib] = v;
      out[size_t(ib) * mc + ia] = v;
      if (!isfinite(v)) atomicOr(&s_flags, 8);
    }
  }
  __syncthreads();
  if (tid == 0) { info[0] = s_minpiv; info[1] = double(s_flags); info[2] = double(mc - nc); info[3] = double(n); }
}

// (n = rows of the compact system is only known on the device; the host sizes for the worst case n = m)
void launch_covariance(const double* Spart, int ks, int m, int mc, const double* Cdiag, const LmState* st, double* work, double* out,
                       double* info, hipStream_t s) {
  if (covariance_in_lds(m))
    hipLaunchKernelGGL(covariance_kernel<true>, dim3(1), dim3(kCovThreads), size_t(m) * covariance_ld(m) * sizeof(double), s, Spart, ks, m,
                       mc, Cdiag, st, work, out, info);
  else
    hipLaunchKernelGGL(covariance_kernel<false>, dim3(1), dim3(kCovThreads), 0, s, Spart, ks, m, mc, Cdiag, st, work, out, info);
}

hipError_t configure_covariance_kernel() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(covariance_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             int(kCovLdsBudget - kCovStaticLds - 1024));
}

}  // namespace cal
