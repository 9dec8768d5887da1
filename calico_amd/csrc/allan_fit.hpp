// allan_fit.hpp — the IEEE-952 noise coefficients of one axis from its Allan variances (calico_imu_allan's host part, allan.cpp),
// free of HIP: the standard library and the C header only, so a plain host program can test it (tests/cpp/allan_fit_check.cpp).
//
// In the variance domain the model is linear in the squared coefficients a_t >= 0,
//   avar(tau) ~ a_Q 3 / tau^2 + a_N / tau + a_B 2 ln 2 / pi + a_K tau / 3 + a_R tau^2 / 2,
// and the fit is the non-negative least squares of Sum_i w_i (1 - model_i / avar_i)^2. With at most five unknowns the NNLS is
// solved exactly: every non-empty subset of the enabled terms by Householder QR of its column-normalised design
// (rows sqrt(w_i) phi_t(tau_i) / avar_i, right-hand side sqrt(w_i)), and among the subsets whose solution is >= 0 everywhere the
// least objective wins; ties go to the fewer terms, then to the lower mask. A subset whose design loses rank takes no part.
// Objectives closer than the rounding of their residuals, Sum_i w_i (64 eps)^2, are tied: on a curve that one term describes
// exactly, a second term with a coefficient of rounding size does not win by the last bits of the objective.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/calico_hip.h"

namespace cal {

constexpr int kAllanTerms = 5;      // bit t of a mask: Q, N, B, K, R (CALICO_ALLAN_TERM_*)
constexpr double kAllanTieEps = 64.0 * 2.220446049250313e-16;      // a residual's rounding, generously

// phi_t(tau): the variance a unit coefficient of term t contributes
inline double allan_term_shape(int t, double tau) {
  switch (t) {
    case 0: return 3.0 / (tau * tau);
    case 1: return 1.0 / tau;
    case 2: return 2.0 * 0.69314718055994530942 / 3.14159265358979323846;
    case 3: return tau / 3.0;
    default: return tau * tau / 2.0;
  }
}

// Least squares of |A z - b| by Householder QR, A [cols][rows] column by column (overwritten, as b). false: a column of the
// triangle is zero or not finite.
inline bool allan_householder_solve(int rows, int cols, double (*A)[CALICO_ALLAN_MAX_CLUSTERS], double* b, double* z) {
  double diag[kAllanTerms];
  for (int j = 0; j < cols; ++j) {
    double norm2 = 0.0;
    for (int i = j; i < rows; ++i) norm2 += A[j][i] * A[j][i];
    const double norm = std::sqrt(norm2);
    if (!std::isfinite(norm) || !(norm > 0.0)) return false;
    const double alpha = A[j][j] > 0.0 ? -norm : norm;
    A[j][j] -= alpha;      // v = x - alpha e_1, in place; v'v = 2 (norm2 - alpha x_1) = -2 alpha v_1
    const double vtv = -2.0 * alpha * A[j][j];
    if (!(vtv > 0.0)) return false;
    for (int c = j + 1; c <= cols; ++c) {
      double* col = c < cols ? A[c] : b;
      double dot = 0.0;
      for (int i = j; i < rows; ++i) dot += A[j][i] * col[i];
      const double f = 2.0 * dot / vtv;
      for (int i = j; i < rows; ++i) col[i] -= f * A[j][i];
    }
    diag[j] = alpha;
  }
  for (int j = cols - 1; j >= 0; --j) {
    double s = b[j];
    for (int c = j + 1; c < cols; ++c) s -= A[c][j] * z[c];
    z[j] = s / diag[j];
    if (!std::isfinite(z[j])) return false;
  }
  return true;
}

// One axis: tau and weight (w_i = 2 (n / m_i - 1)) per cluster size, avar[i * stride] its variances. Fills every field of *out
// (status OK, NO_WHITE_NOISE or TOO_FEW_POINTS; an axis that is not finite is the caller's to mark).
inline void allan_fit_axis(int n_clusters, const double* tau, const double* weight, const double* avar, int stride, int terms,
                           calico_allan_noise* out) {
  *out = calico_allan_noise{};
  static_assert(CALICO_ALLAN_TERM_QUANTISATION == 1 && CALICO_ALLAN_TERM_RAMP == 1 << (kAllanTerms - 1), "bit t is term t");
  double G[kAllanTerms][CALICO_ALLAN_MAX_CLUSTERS];      // phi_t(tau_i) / avar_i of the points that take part
  double sw[CALICO_ALLAN_MAX_CLUSTERS];
  int p = 0, enabled = 0;
  for (int t = 0; t < kAllanTerms; ++t) enabled += (terms >> t) & 1;
  for (int i = 0; i < n_clusters && i < CALICO_ALLAN_MAX_CLUSTERS; ++i) {
    const double v = avar[size_t(i) * stride];
    if (!std::isfinite(v) || !(v > 0.0) || !(weight[i] > 0.0)) continue;
    for (int t = 0; t < kAllanTerms; ++t) G[t][p] = allan_term_shape(t, tau[i]) / v;
    sw[p] = std::sqrt(weight[i]);
    ++p;
  }
  out->n_points = p;
  if (enabled == 0 || p < enabled) { out->status = CALICO_ALLAN_TOO_FEW_POINTS; return; }
  double best[kAllanTerms] = {0.0, 0.0, 0.0, 0.0, 0.0}, best_objective = 0.0;
  double tie = 0.0;
  for (int i = 0; i < p; ++i) tie += sw[i] * sw[i];
  tie *= kAllanTieEps * kAllanTieEps;
  int best_mask = 0;
  for (int size = 1; size <= enabled; ++size) {          // fewer terms first, then the lower mask: a later subset must be strictly better
    for (int mask = 1; mask < (1 << kAllanTerms); ++mask) {
      if ((mask & ~terms) != 0) continue;
      int which[kAllanTerms], cols = 0;
      for (int t = 0; t < kAllanTerms; ++t) if ((mask >> t) & 1) which[cols++] = t;
      if (cols != size) continue;
      double A[kAllanTerms][CALICO_ALLAN_MAX_CLUSTERS], b[CALICO_ALLAN_MAX_CLUSTERS], scale[kAllanTerms], z[kAllanTerms];
      bool usable = true;
      for (int c = 0; c < cols; ++c) {
        double norm2 = 0.0;
        for (int i = 0; i < p; ++i) { A[c][i] = sw[i] * G[which[c]][i]; norm2 += A[c][i] * A[c][i]; }
        scale[c] = std::sqrt(norm2);
        if (!std::isfinite(scale[c]) || !(scale[c] > 0.0)) { usable = false; break; }
        for (int i = 0; i < p; ++i) A[c][i] /= scale[c];
      }
      if (!usable) continue;
      for (int i = 0; i < p; ++i) b[i] = sw[i];
      if (!allan_householder_solve(p, cols, A, b, z)) continue;
      double a[kAllanTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
      for (int c = 0; c < cols; ++c) { a[which[c]] = z[c] / scale[c]; usable = usable && a[which[c]] >= 0.0 && std::isfinite(a[which[c]]); }
      if (!usable) continue;
      double objective = 0.0;
      for (int i = 0; i < p; ++i) {
        double model = 0.0;
        for (int c = 0; c < cols; ++c) model += a[which[c]] * G[which[c]][i];
        const double r = sw[i] * (1.0 - model);
        objective += r * r;
      }
      if (!std::isfinite(objective)) continue;
      if (best_mask == 0 || objective < best_objective - tie) {
        best_mask = mask; best_objective = objective;
        for (int t = 0; t < kAllanTerms; ++t) best[t] = a[t];
      }
    }
  }
  if (best_mask == 0) { out->status = CALICO_ALLAN_TOO_FEW_POINTS; return; }      // (no subset had a usable design)
  const auto root = [](double a) { return a > 0.0 ? std::sqrt(a) : 0.0; };
  out->Q = root(best[0]); out->N = root(best[1]); out->B = root(best[2]); out->K = root(best[3]); out->R = root(best[4]);
  out->objective = best_objective; out->terms_used = best_mask;
  out->status = out->N > 0.0 ? CALICO_ALLAN_OK : CALICO_ALLAN_NO_WHITE_NOISE;
}

}  // namespace cal
