// obs_kernels.hip — observability report of the calibration blocks on gfx950 (calico_observability_compute).
//
// Input: the reduced system the linear solve leaves behind, as covariance_kernel receives it (cov_kernels.hip): Spart =
// [ks K-slices][(m+1)²], lower triangle, rows [calibration (mc) | extra rows (m - mc): the tree solver's root superblock or
// the banded solver's separator], formed UNDAMPED and unscaled; the diagonal of C (the border's block of JᵀJ) from the
// reduce buffer. With H = JᵀJ = [[A, E], [Eᵀ, C]] the kernel forms
//   S̃ = D⁻¹ (C - Eᵀ A⁻¹ E) D⁻¹,  D = sqrt(diag C)  (the column norms of J, not diag S: a column the trajectory explains
//                                                   entirely has diag S ~ 0)
// on the calibration columns whose C diagonal is not exactly 0.0, and its eigendecomposition S̃ = V Λ Vᵀ. One workgroup:
//   1. the compact order covariance_kernel uses (reduced_system.hpp): the extra rows FIRST, then the kept calibration columns;
//   2. the K-slices are added up in slice order (the same load); calibration rows are scaled by 1 / sqrt(C_ii), extra rows by their own
//      diagonal (unit diagonal: their pivots are relative pivots);
//   3. right-looking FP64 Cholesky over the extra rows only; what is left in the trailing block is S̃ (lower triangle). It
//      is compacted to the front of the matrix area row by row (a row's target never reaches a row not yet read), mirrored
//      to a full symmetric matrix and copied out; V = I goes behind it;
//   4. cyclic two-sided Jacobi with the round-robin ordering: a sweep is nn - 1 steps of nn / 2 disjoint rotations (nn: the
//      dimension rounded up to even; the padding index has a zero row and is never rotated). A step computes its rotations
//      from the matrix as the step found it, then every 2x2 block (row pair, column pair) of the lower block triangle is
//      updated by one thread as J₁ᵀ B J₂ and written to both triangles (the matrix stays exactly symmetric), the rotated
//      diagonal is set from the stable formulas (a_pp - t a_pq, a_qq + t a_pq, a_pq = 0), and V's column pairs are rotated.
//      A pair is rotated when |a_pq| > eps · max(sqrt|a_pp a_qq|, d_max / (4 nn)), d_max the largest diagonal entry of S̃:
//      the first term is the relative criterion, the second stops the method from chasing entries of the exactly
//      deficient directions that are rounding noise of S̃ itself (leaving them moves an eigenvalue by at most
//      eps d_max / 4). A sweep without a rotation ends the method; kObsMaxSweeps sweeps that did not are reported (kInfoSweepLimit);
//   5. eigenvalues sorted ascending by rank counting (ties: lower index first), each eigenvector's sign fixed (its
//      largest-magnitude entry positive, the lowest index on a tie), scattered to the border's tangent order.
// Every sum and every rotation runs in a fixed order and nothing is accumulated atomically: repeated computes are
// bit-identical. Size classes: matrix area in LDS (the reduced system, later S̃ and V side by side; odd row strides, so
// that the column walks of the mirrored writes and of V hit distinct banks), or in a global workspace (L2-resident). No
// private arrays (scratch 0 B).
#include <hip/hip_runtime.h>

#include <cmath>

#include "device_math.hpp"
#include "kernels.hpp"
#include "problem_dev.hpp"
#include "reduced_system.hpp"
#include "solve_dev.hpp"

namespace cal {

namespace {
constexpr int kObsThreads = 1024;
constexpr int kObsWaves = kObsThreads / 64;
constexpr int kObsMaxBorder = 256;      // calibration columns (mc) the eigensolver takes
constexpr int kObsMaxDim = 1024;        // rows of the reduced system (as covariance_kernel)
constexpr int kObsMaxPairs = kObsMaxBorder / 2;
constexpr int kObsMaxSweeps = 30;
// static LDS: six arrays per pair slot, the sort's order, the wave flags, scalars
constexpr size_t kObsStaticLds = kObsMaxPairs * (4 * sizeof(double) + 3 * sizeof(int)) + kObsMaxBorder * sizeof(int) + kObsWaves * sizeof(int) + 64;

__host__ __device__ inline int obs_even(int n) { return n + (n & 1); }
__host__ __device__ inline int obs_ld_reduced(int n) { return (n + 1) | 1; }      // odd, and never below the stride of S̃ (the in-place compaction moves entries towards the front only)
__host__ __device__ inline int obs_ld(int nn) { return nn | 1; }                   // nn even: nn + 1
// doubles of the matrix area when it is shared (LDS): the reduced system, then S̃ and V
__host__ __device__ inline size_t obs_shared_doubles(int m, int mc) {
  const size_t a = size_t(m) * obs_ld_reduced(m), b = 2 * size_t(obs_even(mc)) * obs_ld(obs_even(mc));
  return a > b ? a : b;
}
inline size_t obs_small_bytes(int m) { return size_t(m) * (2 * sizeof(double) + sizeof(int)) + 16; }
}  // namespace

int observability_max_border() { return kObsMaxBorder; }
int observability_max_dim() { return kObsMaxDim; }
bool observability_in_lds(int m, int mc) {
  return obs_shared_doubles(m, mc) * sizeof(double) + obs_small_bytes(m) + kObsStaticLds + kLdsSlack <= kLdsBudget;
}
// doubles of the global workspace (the other size class): the reduced system, S̃ and V apart
size_t observability_work_doubles(int m, int mc) {
  return size_t(m) * obs_ld_reduced(m) + 2 * size_t(obs_even(mc)) * obs_ld(obs_even(mc));
}

namespace {
// OR over the workgroup without an atomic: a ballot per wave, one word per wave, read by everybody (two barriers)
__device__ __forceinline__ int obs_block_any(int v, int* s_w) {
  const int w = __ballot(v) != 0ull;
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = w;
  __syncthreads();
  int r = 0;
  for (int i = 0; i < kObsWaves; ++i) r |= s_w[i];
  __syncthreads();
  return r;
}
}  // namespace

// info[0]: minimum relative pivot of the extra rows, info[1]: flags (ReducedInfoFlag, problem_dev.hpp; the pivots are the
// extra rows'), info[2]: dropped
// (structurally unobserved) calibration columns, info[3]: kept columns, info[4]: sweeps, info[5]: rotations applied,
// info[6]: 1 in LDS / 0 global workspace, info[7]: rows of the compact reduced system
template <bool IN_LDS>
__global__ __launch_bounds__(kObsThreads) void observability_kernel(const double* __restrict__ Spart, int ks, int m, int mc,
                                                                    const double* __restrict__ Cdiag, const LmState* __restrict__ st,
                                                                    double* work, double* __restrict__ lam_out, double* __restrict__ vec_out,
                                                                    double* __restrict__ mat_out, double* __restrict__ d_out,
                                                                    double* __restrict__ info) {
  extern __shared__ double lds_dyn[];
  __shared__ double s_c[kObsMaxPairs], s_s[kObsMaxPairs], s_app[kObsMaxPairs], s_aqq[kObsMaxPairs];
  __shared__ int s_p[kObsMaxPairs], s_q[kObsMaxPairs], s_rot[kObsMaxPairs];
  __shared__ int s_ord[kObsMaxBorder];
  __shared__ int s_w[kObsWaves];
  __shared__ int s_nkeep, s_flags;
  __shared__ double s_minpiv, s_dmax;
  double* const s_d = lds_dyn;                  // scale of compact row p
  double* const s_col = s_d + m;                // column j of the factor (rows > j)
  double* const mat = s_col + m;                // the shared matrix area (LDS class)
  int* const s_idx = reinterpret_cast<int*>(mat + (IN_LDS ? obs_shared_doubles(m, mc) : 0));      // compact row -> row of Spart
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nr = m - mc;
  // ---- 1. compact order: extra rows, then the observed calibration columns (reduced_system.hpp) ----
  if (wave == 0) {
    const int cnt = reduced_compact_order(s_idx, Cdiag, m, mc, lane);
    if (lane == 0) { s_nkeep = cnt; s_flags = (st->chol_failed ? kInfoEliminationFailed : 0); s_minpiv = 1.0; s_dmax = 0.0; }
  }
  for (size_t e = tid; e < size_t(mc) * mc; e += kObsThreads) { vec_out[e] = 0.0; mat_out[e] = 0.0; }
  for (int e = tid; e < mc; e += kObsThreads) { lam_out[e] = 0.0; d_out[e] = 0.0; }
  __syncthreads();
  const int nc = s_nkeep, n = nr + nc, LD = obs_ld_reduced(n);
  const int nn = obs_even(nc), LDn = obs_ld(nn), np = nn / 2;
  double* const A = IN_LDS ? mat : work;                                            // the reduced system
  double* const S = IN_LDS ? mat : work + size_t(m) * obs_ld_reduced(m);            // S̃, full symmetric nn x nn
  double* const V = S + size_t(nn) * LDn;
  // ---- 2. load (slices added in order), scale ----
  int bad = reduced_load_lower<kObsThreads>(A, LD, n, s_idx, Spart, ks, m, tid);
  __syncthreads();
  int badpiv = 0;
  for (int p = tid; p < n; p += kObsThreads) {
    const double v = p < nr ? A[p * LD + p] : Cdiag[size_t(s_idx[p]) * (mc + 1)];
    const bool ok = v > 0.0 && isfinite(v);
    if (!ok) { if (p < nr) badpiv = 1; else bad = 1; }
    s_d[p] = ok ? 1.0 / sqrt(v) : 1.0;
  }
  bad = obs_block_any(bad, s_w);
  badpiv = obs_block_any(badpiv, s_w);
  if (tid == 0) s_flags |= (bad ? kInfoNonFiniteInput : 0) | (badpiv ? kInfoPivotNotPositive : 0);
  for (int e = tid; e < n * n; e += kObsThreads) {
    const int p = e / n, q = e - p * n;
    if (q <= p) A[p * LD + q] *= s_d[p] * s_d[q];
  }
  __syncthreads();
  // ---- 3. Cholesky over the extra rows (root superblock / separator): the trailing block becomes S̃ ----
  const int ti = tid >> 5, tc = tid & 31;
  if (s_flags == 0) {
    for (int j = 0; j < nr; ++j) {
      const double piv = A[j * LD + j];
      if (!(piv > 0.0) || !isfinite(piv)) {       // (uniform: every thread reads the same entry)
        if (tid == 0) { s_flags |= kInfoPivotNotPositive; s_minpiv = fmin(s_minpiv, piv > 0.0 ? piv : 0.0); }
        break;
      }
      const double rs = 1.0 / sqrt(piv);
      for (int i = j + 1 + tid; i < n; i += kObsThreads) s_col[i] = A[i * LD + j] * rs;
      if (tid == 0) s_minpiv = fmin(s_minpiv, piv);
      __syncthreads();
      for (int i = j + 1 + ti; i < n; i += 32) {
        const double li = s_col[i];
        for (int c = j + 1 + tc; c <= i; c += 32) A[i * LD + c] -= li * s_col[c];
      }
      __syncthreads();
    }
  }
  __syncthreads();      // (a failed pivot leaves the loop with thread 0's flag just written)
  int sweeps = 0, rotations = 0;
  if (s_flags == 0 && nc > 0) {
    // compaction, row by row: row p of the trailing block to S's row p (at or in front of where it was; a barrier between
    // the read and the write, the next row's source lies behind this row's target)
    for (int p = 0; p < nc; ++p) {
      const double v = tid <= p ? A[size_t(nr + p) * LD + nr + tid] : 0.0;
      __syncthreads();
      if (tid <= p) S[p * LDn + tid] = v;
    }
    __syncthreads();
    for (int e = tid; e < nn * nn; e += kObsThreads) {
      const int p = e / nn, q = e - p * nn;
      if (p >= nc) S[p * LDn + q] = 0.0;                                    // the padding index: a zero row and column
      else if (q > p) S[p * LDn + q] = q < nc ? S[q * LDn + p] : 0.0;
      V[p * LDn + q] = p == q ? 1.0 : 0.0;
    }
    __syncthreads();
    double dm = 0.0;
    for (int e = tid; e < nc * nc; e += kObsThreads) {
      const int p = e / nc, q = e - p * nc;
      mat_out[size_t(s_idx[nr + p]) * mc + s_idx[nr + q]] = S[p * LDn + q];
    }
    if (tid == 0) {
      for (int p = 0; p < nc; ++p) dm = fmax(dm, fabs(S[p * LDn + p]));
      s_dmax = dm;
    }
    __syncthreads();
    // ---- 4. Jacobi sweeps ----
    const double eps = 2.220446049250313e-16;
    const double floor_abs = s_dmax / (4.0 * nn);
    const int ring = nn - 1;
    for (; sweeps < kObsMaxSweeps;) {
      int nrot = 0;
      for (int step = 0; step < ring; ++step) {
        if (tid < np) {
          // round-robin pairing: index nn - 1 stays, the others move round a ring of nn - 1
          const int a = (step + tid) % ring, b = tid == 0 ? ring : (step - tid + ring) % ring;
          const int p = min(a, b), q = max(a, b);
          const double app = S[p * LDn + p], aqq = S[q * LDn + q], apq = S[q * LDn + p];
          double c = 1.0, s = 0.0, napp = app, naqq = aqq;
          const bool rot = fabs(apq) > eps * fmax(sqrt(fabs(app * aqq)), floor_abs);
          if (rot) {
            const double theta = (aqq - app) / (2.0 * apq);
            const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            c = 1.0 / sqrt(t * t + 1.0);
            s = t * c;
            napp = app - t * apq;
            naqq = aqq + t * apq;
            ++nrot;
          }
          s_p[tid] = p; s_q[tid] = q; s_c[tid] = c; s_s[tid] = s; s_app[tid] = napp; s_aqq[tid] = naqq;
        }
        __syncthreads();
        // S <- Jᵀ S J: block (row pair k1, column pair k2 <= k1), both triangles written by the same thread
        for (int k1 = ti; k1 < np; k1 += 32) {
          const double c1 = s_c[k1], s1 = s_s[k1];
          const int p1 = s_p[k1], q1 = s_q[k1];
          for (int k2 = tc; k2 <= k1; k2 += 32) {
            const double c2 = s_c[k2], s2 = s_s[k2];
            if (s1 == 0.0 && s2 == 0.0) continue;
            if (k1 == k2) {
              S[p1 * LDn + p1] = s_app[k1]; S[q1 * LDn + q1] = s_aqq[k1];
              S[p1 * LDn + q1] = 0.0; S[q1 * LDn + p1] = 0.0;
              continue;
            }
            const int p2 = s_p[k2], q2 = s_q[k2];
            const double b00 = S[p1 * LDn + p2], b01 = S[p1 * LDn + q2], b10 = S[q1 * LDn + p2], b11 = S[q1 * LDn + q2];
            const double t00 = c2 * b00 - s2 * b01, t01 = s2 * b00 + c2 * b01;
            const double t10 = c2 * b10 - s2 * b11, t11 = s2 * b10 + c2 * b11;
            const double r00 = c1 * t00 - s1 * t10, r10 = s1 * t00 + c1 * t10;
            const double r01 = c1 * t01 - s1 * t11, r11 = s1 * t01 + c1 * t11;
            S[p1 * LDn + p2] = r00; S[p2 * LDn + p1] = r00;
            S[p1 * LDn + q2] = r01; S[q2 * LDn + p1] = r01;
            S[q1 * LDn + p2] = r10; S[p2 * LDn + q1] = r10;
            S[q1 * LDn + q2] = r11; S[q2 * LDn + q1] = r11;
          }
        }
        // V <- V J: row i, pair k
        for (int e = tid; e < nn * np; e += kObsThreads) {
          const int i = e / np, k = e - i * np;
          const double s = s_s[k];
          if (s == 0.0) continue;
          const double c = s_c[k];
          const int p = s_p[k], q = s_q[k];
          const double vp = V[i * LDn + p], vq = V[i * LDn + q];
          V[i * LDn + p] = c * vp - s * vq;
          V[i * LDn + q] = s * vp + c * vq;
        }
        __syncthreads();
      }
      ++sweeps;
      if (tid < np) s_rot[tid] = nrot;
      __syncthreads();
      int total = 0;
      for (int k = 0; k < np; ++k) total += s_rot[k];
      __syncthreads();
      rotations += total;
      if (total == 0) break;
      if (sweeps == kObsMaxSweeps && tid == 0) s_flags |= kInfoSweepLimit;
    }
    // ---- 5. sort ascending, fix the signs, scatter ----
    if (tid < nc) {
      const double li = S[tid * LDn + tid];
      int rank = 0;
      for (int j = 0; j < nc; ++j) {
        const double lj = S[j * LDn + j];
        rank += (lj < li || (lj == li && j < tid)) ? 1 : 0;
      }
      s_ord[min(rank, nc - 1)] = tid;
    }
    __syncthreads();
    int nonfinite = 0;
    if (tid < nc) {
      const int i = s_ord[tid];
      const double l = S[i * LDn + i];
      lam_out[tid] = l;
      nonfinite = !isfinite(l);
      double best = -1.0, sg = 1.0;
      for (int a = 0; a < nc; ++a) {
        const double v = V[a * LDn + i];
        nonfinite |= !isfinite(v);
        if (fabs(v) > best) { best = fabs(v); sg = v < 0.0 ? -1.0 : 1.0; }
      }
      for (int a = 0; a < nc; ++a) vec_out[size_t(tid) * mc + s_idx[nr + a]] = sg * V[a * LDn + i];
      d_out[s_idx[nr + tid]] = 1.0 / s_d[nr + tid];
    }
    nonfinite = obs_block_any(nonfinite, s_w);
    if (tid == 0 && nonfinite) s_flags |= kInfoNonFiniteResult;
  }
  __syncthreads();
  if (tid == 0) {
    info[0] = s_minpiv; info[1] = double(s_flags); info[2] = double(mc - nc); info[3] = double(nc);
    info[4] = double(sweeps); info[5] = double(rotations); info[6] = IN_LDS ? 1.0 : 0.0; info[7] = double(n);
  }
}

// (the kept columns are only known on the device; the host sizes for the worst case: all of them)
void launch_observability(const double* Spart, int ks, int m, int mc, const double* Cdiag, const LmState* st, double* work, double* lam,
                          double* vec, double* mat, double* d, double* info, hipStream_t s) {
  if (observability_in_lds(m, mc))
    hipLaunchKernelGGL(observability_kernel<true>, dim3(1), dim3(kObsThreads), obs_shared_doubles(m, mc) * sizeof(double) + obs_small_bytes(m),
                       s, Spart, ks, m, mc, Cdiag, st, work, lam, vec, mat, d, info);
  else
    hipLaunchKernelGGL(observability_kernel<false>, dim3(1), dim3(kObsThreads), obs_small_bytes(m), s, Spart, ks, m, mc, Cdiag, st, work, lam,
                       vec, mat, d, info);
}

// (the largest size observability_in_lds admits)
hipError_t configure_observability_kernel(int device) {
  return raise_lds_limit(device, observability_kernel<true>, kLdsBudget - kObsStaticLds - kLdsSlack);
}

}  // namespace cal
