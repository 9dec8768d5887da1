// Checks of calico_amd/csrc/arg_rules.hpp (the argument rules of the calls without a problem handle) and lm_rule.hpp (the
// Levenberg-Marquardt step rule of the device loops, compiled here for the host), as a stand-alone host program: no HIP, no
// library of the project. Every array is a heap allocation of exactly the size the rule may read, so a read past the end
// (offsets[n_frames + 1], stamps[n]) is a sanitizer report.
//
// lm_rule over the grid kept x small x lambda in {1e-12, 1e-5, 1e-4, 1e-3, 1e12} x candidate in {below the current cost, equal to
// it, exactly current + kCostSlack noise, one ulp above that, NaN} x three (current, noise) pairs:
//  1. accept iff kept and candidate <= current + kCostSlack noise (a NaN is never accepted);
//  2. the new lambda lies in [1e-12, 1e12];
//  3. converged iff small and kept and lambda <= 1e-4 before the change (accepted or not);
//  4. on accept the new lambda is max(0.1 lambda, 1e-12);
//  5. on reject the new lambda is lambda if converged, else min(10 lambda, 1e12) -- so it is unchanged iff converged, except at
//     the upper clamp itself (lambda = 1e12 is never converged and cannot grow).
// lm_point_decision (the decision of a loop over one point: the alignments') against the IMU alignment's decision as its kernel
// once spelt it out: see check_point_decision.
// Exits 0 and prints "OK <checks>" when all hold; prints the first violation and exits 1 otherwise.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>

#include "../../calico_amd/csrc/arg_rules.hpp"
#include "../../calico_amd/csrc/lm_rule.hpp"

namespace {

long g_checks = 0;

void expect(bool ok, const char* what, const std::string& got = "") {
  ++g_checks;
  if (ok) return;
  std::printf("FAILED: %s%s%s\n", what, got.empty() ? "" : ": ", got.c_str());
  std::exit(1);
}
bool has(const std::string& s, const char* word) { return s.find(word) != std::string::npos; }

template <class T> std::unique_ptr<T[]> heap(std::initializer_list<T> v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  size_t i = 0;
  for (T x : v) p[i++] = x;
  return p;
}

template <class Options> void check_chart_options(const char* name) {
  const double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
  Options o;
  o.max_iterations = 30; o.step_tolerance = 1e-11; o.huber_scale = 0.0; o.min_points = 4;
  for (int64_t nf : {0, 1, 3}) expect(cal::chart_options_error(nf, o, nullptr, nullptr).empty(), name, "defaults");
  expect(cal::chart_options_error(3, o, q, t).empty(), name, "both starts");
  expect(has(cal::chart_options_error(-1, o, nullptr, nullptr), "n_frames must be >= 0"), name, "n_frames -1");
  expect(has(cal::chart_options_error(3, o, q, nullptr), "q_init and t_init are given together"), name, "q_init alone");
  expect(has(cal::chart_options_error(3, o, nullptr, t), "q_init and t_init are given together"), name, "t_init alone");
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (double v : {0.0, -1e-11, inf, nan}) {
    Options b = o;
    b.step_tolerance = v;
    expect(has(cal::chart_options_error(1, b, nullptr, nullptr), "step_tolerance must be finite and > 0"), name, "step_tolerance");
  }
  for (int v : {0, -3}) {
    Options b = o;
    b.max_iterations = v;
    expect(has(cal::chart_options_error(1, b, nullptr, nullptr), "max_iterations must be >= 1"), name, "max_iterations");
  }
  for (double v : {-1.0, inf, nan}) {
    Options b = o;
    b.huber_scale = v;
    expect(has(cal::chart_options_error(1, b, nullptr, nullptr), "huber_scale must be finite and >= 0"), name, "huber_scale");
  }
  for (int v : {3, 0, -1}) {
    Options b = o;
    b.min_points = v;
    expect(has(cal::chart_options_error(1, b, nullptr, nullptr), "min_points must be >= 4"), name, "min_points");
  }
  // the order of the parent's checks: n_frames, step_tolerance, max_iterations, huber_scale, min_points, the starts
  Options all = o;
  all.step_tolerance = 0.0; all.max_iterations = 0; all.huber_scale = -1.0; all.min_points = 0;
  expect(has(cal::chart_options_error(-1, all, q, nullptr), "n_frames"), name, "order: n_frames first");
  expect(has(cal::chart_options_error(1, all, q, nullptr), "step_tolerance"), name, "order: step_tolerance second");
  all.step_tolerance = 1e-11;
  expect(has(cal::chart_options_error(1, all, q, nullptr), "max_iterations"), name, "order: max_iterations third");
}

void check_chart_frames() {
  const char* const null_text = "null frame offsets or output buffer";
  const auto px = heap<double>({1, 2, 3, 4, 5, 6, 7, 8}), pt = heap<double>({1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12});
  {      // n_frames 0, 1, 3 on exact-size offsets
    const auto o0 = heap<int64_t>({0}), o1 = heap<int64_t>({0, 4}), o3 = heap<int64_t>({0, 1, 3, 4});
    expect(cal::chart_frames_error(0, o0.get(), true, null_text, nullptr, nullptr).empty(), "frames", "n_frames 0");
    expect(cal::chart_frames_error(1, o1.get(), true, null_text, px.get(), pt.get()).empty(), "frames", "n_frames 1");
    expect(cal::chart_frames_error(3, o3.get(), true, null_text, px.get(), pt.get()).empty(), "frames", "n_frames 3");
    expect(cal::chart_frames_error(3, nullptr, true, null_text, px.get(), pt.get()) == null_text, "frames", "null offsets");
    expect(cal::chart_frames_error(3, o3.get(), false, null_text, px.get(), pt.get()) == null_text, "frames", "null output");
    expect(has(cal::chart_frames_error(3, o3.get(), true, null_text, nullptr, pt.get()), "null pixels or points"), "frames", "null pixels, N > 0");
    expect(has(cal::chart_frames_error(3, o3.get(), true, null_text, px.get(), nullptr), "null pixels or points"), "frames", "null points, N > 0");
  }
  {
    const auto o = heap<int64_t>({1, 4, 4});
    expect(has(cal::chart_frames_error(2, o.get(), true, null_text, px.get(), pt.get()), "frame_offsets must start at 0"), "frames", "start at 1");
  }
  {
    const auto mid = heap<int64_t>({0, 5, 4, 12}), last = heap<int64_t>({0, 2, 4, 3});
    expect(has(cal::chart_frames_error(3, mid.get(), true, null_text, px.get(), pt.get()), "frame_offsets decrease at frame 1"), "frames", "decrease");
    expect(has(cal::chart_frames_error(3, last.get(), true, null_text, px.get(), pt.get()), "frame_offsets decrease at frame 2"), "frames",
           "decrease at the last frame");
  }
  {      // empty frames, and a batch without any pair: no pixels needed
    const auto some = heap<int64_t>({0, 0, 4, 4}), none = heap<int64_t>({0, 0, 0, 0});
    expect(cal::chart_frames_error(3, some.get(), true, null_text, px.get(), pt.get()).empty(), "frames", "empty frames");
    expect(cal::chart_frames_error(3, none.get(), true, null_text, nullptr, nullptr).empty(), "frames", "null pixels, N = 0");
  }
}

void check_models_and_counts() {
  const double k[8] = {};
  expect(cal::camera_model_error(1, 8, k, 8).empty(), "model", "fine");
  expect(has(cal::camera_model_error(0, -1, k, 8), "unknown camera model 0"), "model", "unknown");
  expect(has(cal::camera_model_error(1, 8, k, 7), "camera model 1 has 8 intrinsics, got 7"), "model", "count");
  expect(has(cal::camera_model_error(1, 8, nullptr, 8), "null intrinsics"), "model", "null");
  expect(cal::count_error(0, false).empty() && cal::count_error(5, true).empty(), "count", "fine");
  expect(has(cal::count_error(-1, true), "n must be >= 0") && has(cal::count_error(1, false), "null input or output buffer"), "count", "bad");
}

void check_spline() {
  expect(cal::spline_shape_error(4, 8, 8).empty() && cal::spline_shape_error(2, 4, 8).empty() && cal::spline_shape_error(8, 16, 8).empty(), "spline", "fine");
  expect(has(cal::spline_shape_error(1, 20, 8), "order must be in [2, 8]") && has(cal::spline_shape_error(9, 20, 8), "order must be in [2, 8]"), "spline", "order");
  expect(has(cal::spline_shape_error(4, 7, 8), "n_knots must be >= 2 order"), "spline", "n_knots");
  expect(cal::spline_valid_knots(4, 12) == 6, "spline", "valid knots");
  const auto vk = heap<double>({0.0, 1.0, 2.0, 2.5, 4.0});      // 4 segments
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  expect(cal::spline_segment(vk.get(), 5, 0.0) == 0 && cal::spline_segment(vk.get(), 5, 0.999) == 0, "segment", "first");
  expect(cal::spline_segment(vk.get(), 5, 1.0) == 1 && cal::spline_segment(vk.get(), 5, 2.5) == 3, "segment", "a knot belongs to the segment it opens");
  expect(cal::spline_segment(vk.get(), 5, 4.0) == 3 && cal::spline_segment(vk.get(), 5, 3.0) == 3, "segment", "the last knot belongs to the last segment");
  expect(cal::spline_segment(vk.get(), 5, std::nextafter(0.0, -1.0)) == -1 && cal::spline_segment(vk.get(), 5, std::nextafter(4.0, 5.0)) == -1, "segment", "outside");
  expect(cal::spline_segment(vk.get(), 5, nan) == -1 && cal::spline_segment(vk.get(), 5, inf) == -1 && cal::spline_segment(vk.get(), 5, -inf) == -1, "segment", "not a number");
  const auto two = heap<double>({1.0, 2.0});
  expect(cal::spline_segment(two.get(), 2, 1.0) == 0 && cal::spline_segment(two.get(), 2, 2.0) == 0, "segment", "one segment");
}

void check_stamps() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  expect(cal::stamps_error("gyro", 0, nullptr).empty(), "stamps", "n = 0");
  const auto one = heap<double>({3.0});
  expect(cal::stamps_error("gyro", 1, one.get()).empty(), "stamps", "n = 1");
  const auto equal = heap<double>({1.0, 2.0, 2.0, 3.0});
  expect(cal::stamps_error("gyro", 4, equal.get()).empty(), "stamps", "equal neighbours");
  const auto last = heap<double>({1.0, 2.0, 3.0, 2.5});
  expect(cal::stamps_error("accel", 4, last.get()) == "accel stamps are not sorted: they decrease at sample 3", "stamps", "decrease at the last sample");
  const auto bad = heap<double>({1.0, nan, 3.0});
  expect(cal::stamps_error("gyro", 3, bad.get()) == "gyro stamp 1 is not finite", "stamps", "NaN");
  const auto end = heap<double>({1.0, 2.0, std::numeric_limits<double>::infinity()});
  expect(cal::stamps_error("gyro", 3, end.get()) == "gyro stamp 2 is not finite", "stamps", "infinity at the last sample");
}

void check_quaternion() {
  const double q[4] = {0.0, 0.0, 0.0, -2.0}, r[4] = {1.0, 2.0, 2.0, 4.0};
  double out[4];
  expect(cal::quat_norm(q) == 2.0 && cal::quat_norm(r) == 5.0, "quaternion", "norm");
  cal::canonical_unit_quat(q, cal::quat_norm(q), out);
  expect(out[0] == 0.0 && out[1] == 0.0 && out[2] == 0.0 && out[3] == 1.0, "quaternion", "w >= 0");
  cal::canonical_unit_quat(r, 5.0, out);
  expect(out[0] == 0.2 && out[1] == 0.4 && out[2] == 0.4 && out[3] == 0.8, "quaternion", "unit length");
}

void check_lm_rule() {
  using cal::kCostSlack;
  using cal::kLmLambda0;
  using cal::kLmLambdaMax;
  using cal::kLmLambdaMin;
  expect(kLmLambda0 == 1e-4 && kLmLambdaMin == 1e-12 && kLmLambdaMax == 1e12 && kCostSlack == 8.0 * 2.220446049250313e-16, "lm_rule", "constants");
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double points[3][2] = {{1.0, 3.0}, {0.37, 0.0}, {12345.678, 9.0e5}};      // (current, noise)
  for (const auto& pt : points) {
    const double current = pt[0], noise = pt[1], bound = current + kCostSlack * noise;
    const double candidates[5] = {0.5 * current, current, bound, std::nextafter(bound, std::numeric_limits<double>::infinity()), nan};
    for (double lambda : {1e-12, 1e-5, 1e-4, 1e-3, 1e12})
      for (int kept = 0; kept < 2; ++kept)
        for (int small = 0; small < 2; ++small)
          for (int ci = 0; ci < 5; ++ci) {
            const double cand = candidates[ci];
            const cal::LmVerdict v = cal::lm_rule(kept != 0, cand, current, noise, small != 0, lambda);
            const std::string at = "kept " + std::to_string(kept) + " small " + std::to_string(small) + " lambda " + std::to_string(lambda) +
                                   " candidate " + std::to_string(ci) + " current " + std::to_string(current);
            const bool within = ci <= 2;      // below, equal, exactly at the bound; one ulp above and NaN are not
            expect(v.accept == (kept != 0 && within), "lm_rule: accept iff kept and within the slack", at);
            expect(v.lambda >= 1e-12 && v.lambda <= 1e12, "lm_rule: lambda stays in [1e-12, 1e12]", at);
            expect(v.converged == (small != 0 && kept != 0 && lambda <= 1e-4), "lm_rule: converged iff small, kept and lambda <= 1e-4", at);
            if (v.accept) {
              expect(v.lambda == std::fmax(0.1 * lambda, 1e-12), "lm_rule: on accept lambda = max(0.1 lambda, 1e-12)", at);
            } else {
              expect(v.lambda == (v.converged ? lambda : std::fmin(10.0 * lambda, 1e12)), "lm_rule: on reject lambda stays iff converged, else grows", at);
              if (lambda < 1e12) expect((v.lambda == lambda) == v.converged, "lm_rule: on reject lambda is unchanged iff converged", at);
            }
          }
  }
}

// The decision of the IMU alignment's loop as align_decide_kernel spelt it out before it went through lm_point_decision: the
// first evaluation installs the start (a start that is not kept ends the loop), every later one asks lm_rule, the iteration cap
// ends the loop at the point kept, and only a loop that goes on counts the iteration.
cal::LmLoopStep written_out_decision(bool first, bool kept, double cand, double current, double noise, bool small, double lambda, int iterations,
                                     int max_iterations) {
  cal::LmLoopStep s;
  s.accept = false; s.outcome = cal::kLmRunning; s.lambda = lambda; s.iterations = iterations;
  if (first) {
    if (!kept) s.outcome = cal::kLmBadStart;      // (DEGENERATE)
    s.accept = true;
  } else {
    const cal::LmVerdict v = cal::lm_rule(kept, cand, current, noise, small, lambda);
    if (v.accept) s.accept = true;
    s.lambda = v.lambda;
    if (v.converged) s.outcome = cal::kLmConverged;      // (OK)
  }
  if (s.outcome == cal::kLmRunning && iterations >= max_iterations) s.outcome = cal::kLmOutOfIterations;      // (NOT_CONVERGED)
  if (s.outcome == cal::kLmRunning) ++s.iterations;
  return s;
}

// lm_point_decision against it over first x kept x small x candidate in {below the current cost, within its noise, above} x
// lambda in {kLmLambdaMin, kLmLambda0, kLmLambdaMax} x iterations in {below, at, above the cap}: the same accept, outcome,
// lambda (bit for bit) and iteration count everywhere.
void check_point_decision() {
  const double current = 12345.678, noise = 9.0e5, bound = current + cal::kCostSlack * noise;
  const double candidates[3] = {0.5 * current, 0.5 * (current + bound), 2.0 * current};
  expect(candidates[1] > current && candidates[1] < bound, "lm_point_decision", "the middle candidate lies within the noise");
  const int cap = 7;
  for (int first = 0; first < 2; ++first)
    for (int kept = 0; kept < 2; ++kept)
      for (int small = 0; small < 2; ++small)
        for (double cand : candidates)
          for (double lambda : {cal::kLmLambdaMin, cal::kLmLambda0, cal::kLmLambdaMax})
            for (int iterations : {cap - 1, cap, cap + 1}) {
              const cal::LmLoopStep a = written_out_decision(first != 0, kept != 0, cand, current, noise, small != 0, lambda, iterations, cap);
              const cal::LmLoopStep b = cal::lm_point_decision(first != 0, kept != 0, cand, current, noise, small != 0, lambda, iterations, cap);
              const std::string at = "first " + std::to_string(first) + " kept " + std::to_string(kept) + " small " + std::to_string(small) +
                                     " candidate " + std::to_string(cand) + " lambda " + std::to_string(lambda) + " iterations " + std::to_string(iterations);
              expect(a.accept == b.accept, "lm_point_decision: accept", at);
              expect(a.outcome == b.outcome, "lm_point_decision: outcome", at);
              expect(std::memcmp(&a.lambda, &b.lambda, sizeof(double)) == 0, "lm_point_decision: lambda's bits", at);
              expect(a.iterations == b.iterations, "lm_point_decision: iterations", at);
            }
}

}  // namespace

int main() {
  check_chart_options<calico_resection_options>("resection options");
  check_chart_options<calico_calibration_options>("calibration options");
  check_chart_frames();
  check_models_and_counts();
  check_spline();
  check_stamps();
  check_quaternion();
  check_lm_rule();
  check_point_decision();
  std::printf("OK %ld\n", g_checks);
  return 0;
}
