// allan_fit_check.cpp — calico_amd/csrc/allan_fit.hpp on its own (a plain host program, no HIP, no library of the project): each
// single-term curve returns its own coefficient and mask, a curve built from two terms returns both, a curve that would need a
// negative coefficient returns the feasible subset, variances that are all zero or all NaN give TOO_FEW_POINTS, fewer usable
// points than enabled terms too, points that are not usable are left out, and a curve without white noise says so.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../calico_amd/csrc/allan_fit.hpp"

static int checks = 0;
#define CHECK(x) do { ++checks; if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static bool near(double value, double exact, double rel) { return std::fabs(value - exact) <= rel * std::fabs(exact); }

int main() {
  using namespace cal;
  // the default grid of n = 2^16 at 200 Hz
  const int64_t n = 1 << 16;
  const double dt = 1.0 / 200.0;
  std::vector<double> tau, weight;
  int64_t last = 0;
  for (int i = 0;; ++i) {
    const double v = std::floor(std::pow(10.0, i / 10.0) + 0.5);
    if (!(v <= 0.1 * double(n))) break;
    if (int64_t(v) > last) { last = int64_t(v); tau.push_back(double(last) * dt); weight.push_back(2.0 * (double(n) / double(last) - 1.0)); }
  }
  const int nc = int(tau.size());
  CHECK(nc == 36);
  const int all = 31;
  const double coefficient[kAllanTerms] = {2e-4, 1e-3, 3e-4, 2e-4, 5e-5};
  std::vector<double> v(size_t(nc) * 3, 0.0);      // strided as the call's avar_out: the checks use column 1
  calico_allan_noise out;
  const auto value = [](const calico_allan_noise& r, int t) { return t == 0 ? r.Q : t == 1 ? r.N : t == 2 ? r.B : t == 3 ? r.K : r.R; };

  // each single term, every term enabled: its own coefficient and mask, the others exactly 0
  for (int t = 0; t < kAllanTerms; ++t) {
    for (int i = 0; i < nc; ++i) v[size_t(i) * 3 + 1] = coefficient[t] * coefficient[t] * allan_term_shape(t, tau[size_t(i)]);
    allan_fit_axis(nc, tau.data(), weight.data(), v.data() + 1, 3, all, &out);
    CHECK(out.terms_used == 1 << t && out.n_points == nc && out.objective <= 1e-24);
    CHECK(out.status == (t == 1 ? CALICO_ALLAN_OK : CALICO_ALLAN_NO_WHITE_NOISE));
    for (int u = 0; u < kAllanTerms; ++u) CHECK(u == t ? near(value(out, u), coefficient[t], 1e-14) : value(out, u) == 0.0);
  }
  // two terms (white noise and rate random walk) under the default mask: both, and no bias instability
  const int defaults = CALICO_ALLAN_TERM_WHITE | CALICO_ALLAN_TERM_BIAS_INSTABILITY | CALICO_ALLAN_TERM_RATE_RANDOM_WALK;
  for (int i = 0; i < nc; ++i) v[size_t(i) * 3 + 1] = 1e-6 * allan_term_shape(1, tau[size_t(i)]) + 4e-8 * allan_term_shape(3, tau[size_t(i)]);
  allan_fit_axis(nc, tau.data(), weight.data(), v.data() + 1, 3, defaults, &out);
  CHECK(out.terms_used == (CALICO_ALLAN_TERM_WHITE | CALICO_ALLAN_TERM_RATE_RANDOM_WALK) && out.status == CALICO_ALLAN_OK);
  CHECK(near(out.N, 1e-3, 1e-13) && near(out.K, 2e-4, 1e-13) && out.B == 0.0 && out.Q == 0.0 && out.R == 0.0);
  // three terms: all three
  for (int i = 0; i < nc; ++i) v[size_t(i) * 3 + 1] += 9e-8 * allan_term_shape(2, tau[size_t(i)]);
  allan_fit_axis(nc, tau.data(), weight.data(), v.data() + 1, 3, defaults, &out);
  CHECK(out.terms_used == defaults && near(out.N, 1e-3, 1e-12) && near(out.B, 3e-4, 1e-12) && near(out.K, 2e-4, 1e-12));
  // a curve that needs K^2 < 0: the feasible subset is the white noise alone, with a positive objective
  for (int i = 0; i < nc; ++i) v[size_t(i) * 3 + 1] = 1e-6 * allan_term_shape(1, tau[size_t(i)]) - 1e-9 * allan_term_shape(3, tau[size_t(i)]);
  allan_fit_axis(nc, tau.data(), weight.data(), v.data() + 1, 3, CALICO_ALLAN_TERM_WHITE | CALICO_ALLAN_TERM_RATE_RANDOM_WALK, &out);
  CHECK(out.terms_used == CALICO_ALLAN_TERM_WHITE && out.K == 0.0 && out.N > 0.0 && out.objective > 0.0 && out.status == CALICO_ALLAN_OK);
  // points that are not usable are left out: a zero, a NaN and an infinity among the white noise's
  for (int i = 0; i < nc; ++i) v[size_t(i) * 3 + 1] = 1e-6 * allan_term_shape(1, tau[size_t(i)]);
  v[1] = 0.0; v[3 * 5 + 1] = std::numeric_limits<double>::quiet_NaN(); v[3 * 9 + 1] = std::numeric_limits<double>::infinity();
  allan_fit_axis(nc, tau.data(), weight.data(), v.data() + 1, 3, defaults, &out);
  CHECK(out.n_points == nc - 3 && out.terms_used == CALICO_ALLAN_TERM_WHITE && near(out.N, 1e-3, 1e-14));
  // nothing usable, and fewer usable points than enabled terms: TOO_FEW_POINTS with zero coefficients
  for (int pass = 0; pass < 3; ++pass) {
    for (int i = 0; i < nc; ++i) v[size_t(i) * 3 + 1] = pass == 1 ? std::numeric_limits<double>::quiet_NaN() : 0.0;
    if (pass == 2) { v[1] = 1e-6; v[4] = 5e-7; }
    allan_fit_axis(nc, tau.data(), weight.data(), v.data() + 1, 3, defaults, &out);
    CHECK(out.status == CALICO_ALLAN_TOO_FEW_POINTS && out.n_points == (pass == 2 ? 2 : 0) && out.terms_used == 0);
    CHECK(out.Q == 0.0 && out.N == 0.0 && out.B == 0.0 && out.K == 0.0 && out.R == 0.0 && out.objective == 0.0);
  }
  // as many points as terms: an exact interpolation
  v[1] = 1e-6 * allan_term_shape(1, tau[0]) + 4e-8 * allan_term_shape(3, tau[0]);
  v[4] = 1e-6 * allan_term_shape(1, tau[1]) + 4e-8 * allan_term_shape(3, tau[1]);
  allan_fit_axis(2, tau.data(), weight.data(), v.data() + 1, 3, CALICO_ALLAN_TERM_WHITE | CALICO_ALLAN_TERM_RATE_RANDOM_WALK, &out);
  CHECK(out.status == CALICO_ALLAN_OK && out.n_points == 2 && near(out.N, 1e-3, 1e-10) && near(out.K, 2e-4, 1e-6));
  std::printf("OK %d\n", checks);
  return 0;
}
