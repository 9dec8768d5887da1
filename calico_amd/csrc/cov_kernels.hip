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

#include "device_math.hpp"
#include "kernels.hpp"
#include "problem_dev.hpp"
#include "reduced_system.hpp"
#include "solve_dev.hpp"

namespace cal {

namespace {
constexpr int kCovThreads = 1024;
constexpr int kCovMaxDim = 1024;        // rows of the reduced system the kernel takes (static LDS below: 28 KB)
constexpr size_t kCovStaticLds = kCovMaxDim * (sizeof(int) + 3 * sizeof(double)) + 64;
}  // namespace

int covariance_max_dim() { return kCovMaxDim; }
int covariance_ld(int n) { return n | 1; }       // odd row stride: the column walks of LDS hit distinct banks
bool covariance_in_lds(int n) { return size_t(n) * covariance_ld(n) * sizeof(double) + kCovStaticLds + kLdsSlack <= kLdsBudget; }

// info[0]: minimum relative pivot, info[1]: flags (ReducedInfoFlag, problem_dev.hpp), info[2]: dropped
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
  const int nr = m - mc;
  // ---- 1. compact order: extra rows, then the observed calibration columns (reduced_system.hpp) ----
  if (wave == 0) {
    const int cnt = reduced_compact_order(s_idx, Cdiag, m, mc, lane);
    if (lane == 0) { s_nkeep = cnt; s_flags = (st->chol_failed ? kInfoEliminationFailed : 0); s_minpiv = 1.0; }
  }
  for (size_t e = tid; e < size_t(mc) * mc; e += kCovThreads) out[e] = 0.0;
  __syncthreads();
  const int nc = s_nkeep, n = nr + nc, LD = n | 1;
  // ---- 2. load (slices added in order), equilibrate ----
  if (reduced_load_lower<kCovThreads>(A, LD, n, s_idx, Spart, ks, m, tid)) atomicOr(&s_flags, kInfoNonFiniteInput);
  __syncthreads();
  for (int p = tid; p < n; p += kCovThreads) {
    const double v = A[p * LD + p];
    const bool ok = v > 0.0 && isfinite(v);
    if (!ok) atomicOr(&s_flags, kInfoPivotNotPositive);
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
      if (tid == 0) { s_flags |= kInfoPivotNotPositive; s_minpiv = fmin(s_minpiv, piv > 0.0 ? piv : 0.0); }
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
      if (!isfinite(v)) atomicOr(&s_flags, kInfoNonFiniteResult);
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

// (the largest size covariance_in_lds admits)
hipError_t configure_covariance_kernel(int device) { return raise_lds_limit(device, covariance_kernel<true>, kLdsBudget - kCovStaticLds - kLdsSlack); }

// ---------------------------------------------------------------------------
// Control-point blocks (calico_covariance_options.control_points). With H = JᵀJ = [[A, E], [Eᵀ, C]], A the block band of the
// control points (6 n_cp rows, k blocks wide, k the spline order) and Σ_EE the border's Σ from covariance_kernel:
//   Σ_AE = -W Σ_EE,  W = A⁻¹ E;      Σ_AA(i, j) = [A⁻¹]_ij - [Σ_AE Wᵀ]_ij  for |i - j| < k only (the band).
// A is read from the reduce buffer R (band and E as the evaluation leaves them: these kernels run before the reduction and read
// no solver workspace, so the tree and the banded solver are served alike), equilibrated as D A D (unit diagonal; a column no
// residual reaches gets D = 1 and a diagonal of 1, and zero rows and columns in the result) and factored as a block band L Lᵀ,
// which keeps its band. The band of Z = (D A D)⁻¹ follows from L by the Takahashi recurrence, run backwards:
//   Z_{J+d,J} = -Σ_e Z_{J+d,J+e} M_{J,e},   Z_JJ = L_JJ⁻ᵀ L_JJ⁻¹ - Σ_e Z_{J+e,J}ᵀ M_{J,e},   M_{J,e} = L_{J+e,J} L_JJ⁻¹ (e = 1..k-1),
// and A⁻¹'s band is D Z D. The factor and the Takahashi sweep are one-workgroup walks over the control points (an LDS window of
// k block columns, the next step's global loads in flight during the current one); W's two substitutions spread the columns
// of E over workgroups; the products and the stamps are one thread per result. Every sum runs in a fixed order and nothing is
// accumulated atomically: repeated computes are bit-identical. Block storage: [n_cp][k][36], block (J + d, J) row-major at
// (J k + d) 36.
// ---------------------------------------------------------------------------
namespace {
constexpr int kCpThreads = 256;       // the one-workgroup walks
constexpr int kCpMaxK = kMaxOrder;    // spline orders 2..8
constexpr int kCpCols = 32;           // columns of E per workgroup of the substitutions (6 rows x 32 columns = 192 threads)
constexpr int kCpPf = (kCpMaxK * 36 + kCpThreads - 1) / kCpThreads;      // entries of a block column per thread
}  // namespace

int cp_covariance_max_order() { return kCpMaxK; }

namespace {
__device__ __forceinline__ bool cp_dropped(const CpCovArgs& a, int row) {      // no residual reaches tangent row `row`
  return a.R[a.off_B + size_t(row / 6) * a.k * 36 + (row % 6) * 7] == 0.0;
}
// entry e = d·36 + r·6 + c of the equilibrated block column c0: (D A D)(6 (c0 + d) + r, 6 c0 + c)
__device__ __forceinline__ double cp_fetch(const CpCovArgs& a, int c0, int e) {
  const int d = e / 36, q = e - d * 36, r = q / 6, c = q - r * 6;
  if (c0 + d >= a.n_cp) return 0.0;
  const int lo = d == 0 ? min(r, c) : c, hi = d == 0 ? max(r, c) : r;      // (a diagonal block: its stored triangle)
  const double v = a.R[a.off_B + (size_t(c0) * a.k + d) * 36 + lo * 6 + hi];
  if (d == 0 && r == c && v == 0.0) return 1.0;
  return v * a.dq[6 * (c0 + d) + r] * a.dq[6 * c0 + c];
}
}  // namespace

// Block band Cholesky of D A D, one workgroup. Window slot c % k holds block column c (blocks (c + d, c), d < k) of the
// partially updated matrix. Step J factors the pivot block (one thread: 6x6 Cholesky and its inverse), forms the panel, updates
// the k - 1 trailing block columns and moves block column J + k (loaded during step J - 1) into the freed slot.
__global__ __launch_bounds__(kCpThreads) void cp_band_factor_kernel(CpCovArgs a) {
  __shared__ double win[kCpMaxK][kCpMaxK * 36];
  __shared__ double pan[kCpMaxK][36];
  __shared__ double li[36];
  __shared__ int s_flags;
  __shared__ double s_minpiv;
  const int tid = threadIdx.x, k = a.k, n_cp = a.n_cp, n = 6 * n_cp, kk36 = k * 36;
  int bad = 0;
  for (int i = tid; i < n; i += kCpThreads) {
    const double v = a.R[a.off_B + size_t(i / 6) * k * 36 + (i % 6) * 7];
    bad |= !(v >= 0.0) || !isfinite(v);
    a.dq[i] = v > 0.0 && isfinite(v) ? 1.0 / sqrt(v) : 1.0;
  }
  if (tid == 0) { s_flags = 0; s_minpiv = 1.0; }
  __syncthreads();
  if (bad) atomicOr(&s_flags, 1);
  for (int c = 0; c < min(k, n_cp); ++c)
    for (int e = tid; e < kk36; e += kCpThreads) win[c][e] = cp_fetch(a, c, e);
  double pf[kCpPf];
#pragma unroll
  for (int u = 0; u < kCpPf; ++u) pf[u] = k < n_cp && tid + u * kCpThreads < kk36 ? cp_fetch(a, k, tid + u * kCpThreads) : 0.0;
  __syncthreads();
  for (int J = 0; J < n_cp; ++J) {
    double* wj = win[J % k];
    if (tid == 0) {
      double l[6][6], iv[6][6];
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) { l[i][j] = j <= i ? wj[i * 6 + j] : 0.0; iv[i][j] = 0.0; }
      double mp = s_minpiv;
      int fl = 0;
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        double p = l[j][j];
#pragma unroll
        for (int q = 0; q < j; ++q) p -= l[j][q] * l[j][q];
        mp = fmin(mp, p > 0.0 ? p : 0.0);
        if (!(p > 0.0) || !isfinite(p)) fl = 2;
        const double ljj = sqrt(p), inv = 1.0 / ljj;
        l[j][j] = ljj;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
          double v = l[i][j];
#pragma unroll
          for (int q = 0; q < j; ++q) v -= l[i][q] * l[j][q];
          l[i][j] = v * inv;
        }
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        iv[j][j] = 1.0 / l[j][j];
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
          double v = 0.0;
#pragma unroll
          for (int q = j; q < i; ++q) v += l[i][q] * iv[q][j];
          iv[i][j] = -v / l[i][i];
        }
      }
#pragma unroll
      for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
          wj[i * 6 + j] = l[i][j]; li[i * 6 + j] = iv[i][j];
          a.L[size_t(J) * kk36 + i * 6 + j] = l[i][j]; a.Li[size_t(J) * 36 + i * 6 + j] = iv[i][j];
        }
      s_minpiv = mp;
      if (fl) s_flags |= fl;
    }
    lds_barrier();
    // panel L_{J+d,J} = A_{J+d,J} L_JJ⁻ᵀ
    const int np = min(k - 1, n_cp - 1 - J);
    for (int e = tid; e < np * 36; e += kCpThreads) {
      const int d = 1 + e / 36, q = e % 36, r = q / 6, c = q % 6;
      const double* A = wj + d * 36 + r * 6;
      double v = 0.0;
      for (int s = 0; s <= c; ++s) v += A[s] * li[c * 6 + s];
      pan[d][q] = v;
    }
    lds_barrier();
    // trailing update of block (J + d, J + e2), 1 <= e2 <= d <= np: -= L_{J+d,J} L_{J+e2,J}ᵀ
    const int npair = np * (np + 1) / 2;
    for (int e = tid; e < npair * 36; e += kCpThreads) {
      const int pq = e / 36, q = e % 36, r = q / 6, c = q % 6;
      int d = 1;
      while (d * (d + 1) / 2 <= pq) ++d;
      const int e2 = pq - d * (d - 1) / 2 + 1;
      double v = 0.0;
#pragma unroll
      for (int s = 0; s < 6; ++s) v += pan[d][r * 6 + s] * pan[e2][c * 6 + s];
      win[(J + e2) % k][(d - e2) * 36 + q] -= v;
    }
    for (int e = tid; e < np * 36; e += kCpThreads) a.L[size_t(J) * kk36 + 36 + e] = pan[1 + e / 36][e % 36];
    if (J + k < n_cp) {
#pragma unroll
      for (int u = 0; u < kCpPf; ++u)
        if (tid + u * kCpThreads < kk36) wj[tid + u * kCpThreads] = pf[u];
    }
#pragma unroll
    for (int u = 0; u < kCpPf; ++u)
      pf[u] = J + k + 1 < n_cp && tid + u * kCpThreads < kk36 ? cp_fetch(a, J + k + 1, tid + u * kCpThreads) : 0.0;
    lds_barrier();
  }
  __syncthreads();
  if (tid == 0) { a.info[0] = s_minpiv; a.info[1] = double(s_flags); }
}

// M_{J,d} = L_{J+d,J} L_JJ⁻¹ (d >= 1) and L_JJ⁻ᵀ L_JJ⁻¹ (d = 0), one thread per entry
__global__ __launch_bounds__(256) void cp_prep_kernel(CpCovArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x, k = a.k;
  if (t >= a.n_cp * k * 36) return;
  const int J = t / (k * 36), e = t - J * k * 36, d = e / 36, q = e % 36, r = q / 6, c = q % 6;
  const double* li = a.Li + size_t(J) * 36;
  double v = 0.0;
  if (d == 0) {
    for (int s = max(r, c); s < 6; ++s) v += li[s * 6 + r] * li[s * 6 + c];
  } else if (J + d < a.n_cp) {
    const double* lb = a.L + size_t(J) * k * 36 + d * 36 + r * 6;
    for (int s = c; s < 6; ++s) v += lb[s] * li[s * 6 + c];
  }
  a.M[t] = v;
}

namespace {
struct CpRow { double l[kCpMaxK - 1][6]; double li[6]; double rhs; };
}  // namespace

// W = A⁻¹ E = D (L Lᵀ)⁻¹ D E: forward, then backward substitution over the control points, kCpCols columns of E per
// workgroup; thread (r, c) owns row 6 J + r of its column at step J. The next step's operands are loaded one step ahead.
__global__ __launch_bounds__(6 * kCpCols) void cp_solve_kernel(CpCovArgs a) {
  __shared__ double xw[kCpMaxK][6][kCpCols];
  __shared__ double sy[6][kCpCols];
  const int tid = threadIdx.x, r = tid / kCpCols, c = tid % kCpCols;
  const int k = a.k, n_cp = a.n_cp, mc = a.mc;
  const int col = blockIdx.x * kCpCols + c;
  const bool on = col < mc;
  const int colc = min(col, mc - 1);
  // forward, row 6 J + r: L_{J,J-d}(r, ·) for d = 1..k-1, L_JJ⁻¹(r, ·), (D E)(6 J + r, col)
  auto load_fwd = [&](int J, CpRow& f) {
    const int row = 6 * J + r;
#pragma unroll
    for (int d = 1; d < kCpMaxK; ++d)
#pragma unroll
      for (int s = 0; s < 6; ++s) f.l[d - 1][s] = d < k && d <= J ? a.L[(size_t(J - d) * k + d) * 36 + r * 6 + s] : 0.0;
#pragma unroll
    for (int s = 0; s < 6; ++s) f.li[s] = a.Li[size_t(J) * 36 + r * 6 + s];
    f.rhs = a.dq[row] * a.R[a.off_E + size_t(row) * mc + colc];
  };
  CpRow cur{}, nxt{};
  load_fwd(0, cur);
  for (int J = 0; J < n_cp; ++J) {
    if (J + 1 < n_cp) load_fwd(J + 1, nxt);
    double y = cur.rhs;
#pragma unroll
    for (int d = 1; d < kCpMaxK; ++d) {
      if (d < k && d <= J) {
        const int sl = (J - d) % k;
#pragma unroll
        for (int s = 0; s < 6; ++s) y -= cur.l[d - 1][s] * xw[sl][s][c];
      }
    }
    sy[r][c] = y;
    lds_barrier();
    double x = 0.0;
#pragma unroll
    for (int s = 0; s < 6; ++s) x += cur.li[s] * sy[s][c];      // (L_JJ⁻¹ is lower triangular: its zeros add nothing)
    xw[J % k][r][c] = x;
    if (on) a.X[size_t(6 * J + r) * mc + col] = x;
    lds_barrier();
    cur = nxt;
  }
  // backward, row 6 J + r: L_{J+d,J}(·, r), L_JJ⁻ᵀ(r, ·) = L_JJ⁻¹(·, r), the forward result (written by this thread)
  auto load_bwd = [&](int J, CpRow& f) {
#pragma unroll
    for (int d = 1; d < kCpMaxK; ++d)
#pragma unroll
      for (int s = 0; s < 6; ++s) f.l[d - 1][s] = d < k && J + d < n_cp ? a.L[(size_t(J) * k + d) * 36 + s * 6 + r] : 0.0;
#pragma unroll
    for (int s = 0; s < 6; ++s) f.li[s] = a.Li[size_t(J) * 36 + s * 6 + r];
    f.rhs = on ? a.X[size_t(6 * J + r) * mc + col] : 0.0;
  };
  load_bwd(n_cp - 1, cur);
  for (int J = n_cp - 1; J >= 0; --J) {
    if (J > 0) load_bwd(J - 1, nxt);
    double y = cur.rhs;
#pragma unroll
    for (int d = 1; d < kCpMaxK; ++d) {
      if (d < k && J + d < n_cp) {
        const int sl = (J + d) % k;
#pragma unroll
        for (int s = 0; s < 6; ++s) y -= cur.l[d - 1][s] * xw[sl][s][c];
      }
    }
    sy[r][c] = y;
    lds_barrier();
    double x = 0.0;
#pragma unroll
    for (int s = 0; s < 6; ++s) x += cur.li[s] * sy[s][c];
    xw[J % k][r][c] = x;
    if (on) a.W[size_t(6 * J + r) * mc + col] = a.dq[6 * J + r] * x;
    lds_barrier();
    cur = nxt;
  }
}

// Σ_AE = -W Σ_EE, one thread per entry
__global__ __launch_bounds__(256) void cp_cross_kernel(CpCovArgs a) {
  const size_t t = size_t(blockIdx.x) * 256 + threadIdx.x;
  const int mc = a.mc;
  if (t >= size_t(6) * a.n_cp * mc) return;
  const size_t i = t / mc;
  const int j = int(t - i * mc);
  const double* w = a.W + i * mc;
  double v = 0.0;
  for (int l = 0; l < mc; ++l) v += w[l] * a.sigma[size_t(l) * mc + j];
  a.sae[t] = -v;
}

// Takahashi's selected inversion of D A D = L Lᵀ, one workgroup, from the last control point backwards. Window slot c % k holds
// block column c of Z (blocks (c + d, c)); the step's M blocks sit in a two-deep LDS buffer filled one step ahead.
__global__ __launch_bounds__(kCpThreads) void cp_takahashi_kernel(CpCovArgs a) {
  __shared__ double zw[kCpMaxK][kCpMaxK * 36];
  __shared__ double mm[2][kCpMaxK * 36];
  const int tid = threadIdx.x, k = a.k, n_cp = a.n_cp, kk36 = k * 36;
  double pf[kCpPf];
  for (int e = tid; e < kk36; e += kCpThreads) mm[(n_cp - 1) & 1][e] = a.M[size_t(n_cp - 1) * kk36 + e];
#pragma unroll
  for (int u = 0; u < kCpPf; ++u)
    pf[u] = n_cp >= 2 && tid + u * kCpThreads < kk36 ? a.M[size_t(n_cp - 2) * kk36 + tid + u * kCpThreads] : 0.0;
  __syncthreads();
  // entry (r, s) of block (hi, lo) of Z, from the window
  auto zb = [&](int hi, int lo, int r, int s) -> double {
    return hi >= lo ? zw[lo % k][(hi - lo) * 36 + r * 6 + s] : zw[hi % k][(lo - hi) * 36 + s * 6 + r];
  };
  for (int J = n_cp - 1; J >= 0; --J) {
    const double* mj = mm[J & 1];
    double* zj = zw[J % k];
    const int np = min(k - 1, n_cp - 1 - J);
    for (int e = tid; e < np * 36; e += kCpThreads) {
      const int d = 1 + e / 36, q = e % 36, r = q / 6, c = q % 6;
      double v = 0.0;
      for (int e2 = 1; e2 <= np; ++e2)
#pragma unroll
        for (int s = 0; s < 6; ++s) v += zb(J + d, J + e2, r, s) * mj[e2 * 36 + s * 6 + c];
      zj[d * 36 + q] = -v;
      a.Z[size_t(J) * kk36 + d * 36 + q] = -v;
    }
    lds_barrier();
    if (tid < 36) {
      const int r = max(tid / 6, tid % 6), c = min(tid / 6, tid % 6);     // the lower triangle, mirrored
      double v = mj[r * 6 + c];
      for (int e2 = 1; e2 <= np; ++e2)
#pragma unroll
        for (int s = 0; s < 6; ++s) v -= zj[e2 * 36 + s * 6 + r] * mj[e2 * 36 + s * 6 + c];
      zj[tid] = v;
      a.Z[size_t(J) * kk36 + tid] = v;
    }
    if (J >= 1) {
#pragma unroll
      for (int u = 0; u < kCpPf; ++u)
        if (tid + u * kCpThreads < kk36) mm[(J - 1) & 1][tid + u * kCpThreads] = pf[u];
    }
#pragma unroll
    for (int u = 0; u < kCpPf; ++u)
      pf[u] = J >= 2 && tid + u * kCpThreads < kk36 ? a.M[size_t(J - 2) * kk36 + tid + u * kCpThreads] : 0.0;
    lds_barrier();
  }
}

// Σ_AA's band: D Z D - Σ_AE Wᵀ, one thread per entry; a diagonal block from its lower triangle (exactly symmetric); zero rows
// and columns for the dropped columns
__global__ __launch_bounds__(256) void cp_band_kernel(CpCovArgs a) {
  const int t = blockIdx.x * 256 + threadIdx.x, k = a.k, mc = a.mc;
  if (t >= a.n_cp * k * 36) return;
  const int J = t / (k * 36), e = t - J * k * 36, d = e / 36, q = e % 36, r0 = q / 6, c0 = q % 6;
  const int r = d == 0 ? max(r0, c0) : r0, c = d == 0 ? min(r0, c0) : c0;
  double v = 0.0;
  if (J + d < a.n_cp) {
    const int row = 6 * (J + d) + r, col = 6 * J + c;
    if (!cp_dropped(a, row) && !cp_dropped(a, col)) {
      const double* s1 = a.sae + size_t(row) * mc;
      const double* w = a.W + size_t(col) * mc;
      double u = 0.0;
      for (int l = 0; l < mc; ++l) u += s1[l] * w[l];
      v = a.dq[row] * a.Z[size_t(J) * k * 36 + d * 36 + r * 6 + c] * a.dq[col] - u;
    }
  }
  a.band[t] = v;
}

// Σ_v(t) = Σ_ij w_i(t) w_j(t) Σ_AA(s + i, s + j) at a stamp t of segment s, one thread per entry (lower triangle, mirrored)
__global__ __launch_bounds__(256) void cp_stamp_kernel(int n, int k, const double* __restrict__ stamps, const int* __restrict__ seg,
                                                       const double* __restrict__ knots, const double* __restrict__ basis,
                                                       const double* __restrict__ band, double* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n * 36) return;
  const int i = t / 36, q = t % 36, r = max(q / 6, q % 6), c = min(q / 6, q % 6);
  const int s = seg[i], ki = s + k - 1;
  double w[1][kMaxOrder];
  spline_weights<1, 0>(k, knots[ki], knots[ki + 1], basis + size_t(s) * k * k, stamps[i], w);
  double v = 0.0;
#pragma unroll
  for (int x = 0; x < kMaxOrder; ++x) {
#pragma unroll
    for (int y = 0; y < kMaxOrder; ++y) {
      if (x < k && y < k) {
        const int hi = max(x, y), lo = min(x, y);
        const double* b = band + (size_t(s + lo) * k + (hi - lo)) * 36;
        v += w[0][x] * w[0][y] * (x >= y ? b[r * 6 + c] : b[c * 6 + r]);
      }
    }
  }
  out[t] = v;
}

void launch_cp_covariance_band(const CpCovArgs& a, hipStream_t s) {      // reads R only: enqueued ahead of the reduction
  hipLaunchKernelGGL(cp_band_factor_kernel, dim3(1), dim3(kCpThreads), 0, s, a);
  const int nb = a.n_cp * a.k * 36;
  hipLaunchKernelGGL(cp_prep_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, a);
  if (a.mc > 0) hipLaunchKernelGGL(cp_solve_kernel, dim3((a.mc + kCpCols - 1) / kCpCols), dim3(6 * kCpCols), 0, s, a);
  hipLaunchKernelGGL(cp_takahashi_kernel, dim3(1), dim3(kCpThreads), 0, s, a);
}
// the band's factorisation alone (dq, L, Li, info of `a`): the observability pass wants its minimum relative pivot
void launch_cp_band_factor(const CpCovArgs& a, hipStream_t s) { hipLaunchKernelGGL(cp_band_factor_kernel, dim3(1), dim3(kCpThreads), 0, s, a); }
void launch_cp_covariance_finish(const CpCovArgs& a, hipStream_t s) {    // behind covariance_kernel (Σ_EE)
  const size_t ne = size_t(6) * a.n_cp * a.mc;
  if (ne > 0) hipLaunchKernelGGL(cp_cross_kernel, dim3(unsigned((ne + 255) / 256)), dim3(256), 0, s, a);
  const int nb = a.n_cp * a.k * 36;
  hipLaunchKernelGGL(cp_band_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, a);
}
void launch_cp_stamps(int n, int k, const double* stamps, const int* seg, const double* knots, const double* basis, const double* band,
                      double* out, hipStream_t s) {
  if (n > 0)
    hipLaunchKernelGGL(cp_stamp_kernel, dim3(unsigned((size_t(n) * 36 + 255) / 256)), dim3(256), 0, s, n, k, stamps, seg, knots, basis, band,
                       out);
}

}  // namespace cal
