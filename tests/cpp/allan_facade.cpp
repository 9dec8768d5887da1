// allan_facade.cpp — sensors::CharacterizeImuNoise and ImuSensor::ApplyNoise (include/calico/calico.hpp) from C++: a static log of
// 2^16 samples at 256 Hz, white noise of density 1e-3 plus a rate random walk of 2e-4 per axis from a fixed linear congruential
// generator. --host-only: what needs no device (the library's argument errors with their messages, ApplyNoise's arithmetic and
// its refusals). Otherwise, on the device: the facade's numbers against a direct call of calico_imu_allan with the same arrays,
// bit for bit, the white noise against the truth, and the sigma ApplyNoise leaves in a gyroscope and an accelerometer.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "calico/calico.hpp"

using namespace calico;           // NOLINT
using namespace calico::sensors;  // NOLINT

#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

// standard normal numbers from a 64-bit linear congruential generator (Box-Muller): the same on every machine
struct Normal {
  uint64_t s = 0x9e3779b97f4a7c15ull;
  double uniform() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double(s >> 11) + 0.5) / 9007199254740992.0; }
  double operator()() { return std::sqrt(-2.0 * std::log(uniform())) * std::cos(2.0 * M_PI * uniform()); }
};

int main(int argc, char** argv) {
  const bool host_only = argc > 1 && std::strcmp(argv[1], "--host-only") == 0;
  const double rate = 256.0, N0 = 1e-3, K0 = 2e-4;
  const int n = 1 << 16;
  std::vector<double> stamps(n);
  std::vector<Vector3d> samples(n);
  Normal normal;
  Vector3d walk;
  for (int i = 0; i < n; ++i) {
    stamps[size_t(i)] = 2.0 + double(i) / rate;
    for (int c = 0; c < 3; ++c) {
      walk[c] += K0 / std::sqrt(rate) * normal();
      samples[size_t(i)][c] = N0 * std::sqrt(rate) * normal() + walk[c];
    }
  }

  // argument errors reach the caller as kInvalidArgument with the library's message; no device is touched
  {
    std::vector<double> gap = stamps;
    for (int i = 500; i < n; ++i) gap[size_t(i)] += 0.01;
    auto r = CharacterizeImuNoise(gap, samples);
    CHECK(!r.ok() && r.status().code() == StatusCode::kInvalidArgument);
    CHECK(r.status().message().find("calico_imu_allan: the step to sample 500") != std::string::npos);
    CHECK(r.status().message().find("a gap: split the log") != std::string::npos);
    calico_allan_options o = DefaultAllanOptions();
    CHECK(o.points_per_decade == 10 && o.max_tau_fraction == 0.1 && o.n_cluster_sizes == 0);
    o.terms = 0;
    r = CharacterizeImuNoise(stamps, samples, o);
    CHECK(!r.ok() && r.status().code() == StatusCode::kInvalidArgument && r.status().message().find("terms") != std::string::npos);
    r = CharacterizeImuNoise(std::vector<double>(5, 0.0), samples);
    CHECK(!r.ok() && r.status().message().find("one stamp per sample") != std::string::npos);
    r = CharacterizeImuNoise({}, {});
    CHECK(!r.ok() && r.status().message().find("n must be >= 3") != std::string::npos);
  }
  // ApplyNoise: N_pooled sqrt(rate) through the sensor's own SetMeasurementNoise
  {
    ImuNoise noise;
    noise.summary.N_pooled = 1.7e-4;
    CHECK(noise.MeasurementSigma(200.0) == 1.7e-4 * std::sqrt(200.0));
    Gyroscope g;
    Accelerometer a;
    CHECK(g.GetMeasurementNoise() == 1.0);
    CHECK(g.ApplyNoise(noise, 200.0).ok() && g.GetMeasurementNoise() == 1.7e-4 * std::sqrt(200.0));
    CHECK(a.ApplyNoise(noise, 100.0).ok() && a.GetMeasurementNoise() == 1.7e-4 * 10.0);
    CHECK(!a.ApplyNoise(noise, 0.0).ok() && !a.ApplyNoise(noise, -1.0).ok() && a.GetMeasurementNoise() == 1.7e-4 * 10.0);
    noise.summary.N_pooled = 0.0;
    const Status st = a.ApplyNoise(noise, 100.0);
    CHECK(!st.ok() && st.code() == StatusCode::kInvalidArgument && st.message().find("no white-noise density") != std::string::npos);
    CHECK(!g.MeasurementRate().ok());
    CHECK(g.AddMeasurements({{Vector3d(), {1.0, 0}}, {Vector3d(), {1.5, 1}}, {Vector3d(), {1.25, 2}}}).ok());
    auto r = g.MeasurementRate();
    CHECK(r.ok() && r.value() == 4.0);
  }
  if (host_only) { std::printf("OK\n"); return 0; }

  auto res = CharacterizeImuNoise(stamps, samples);
  CHECK(res.ok());
  const ImuNoise& r = res.value();
  std::printf("%zu cluster sizes, N %.6e %.6e %.6e (pooled %.6e), K %.3e %.3e %.3e, drift over %.0f s: %.3e\n", r.tau.size(), r.axes[0].N,
              r.axes[1].N, r.axes[2].N, r.summary.N_pooled, r.axes[0].K, r.axes[1].K, r.axes[2].K, r.summary.duration,
              r.summary.bias_drift_over_recording);
  CHECK(r.cluster_sizes.size() == 36 && r.tau.size() == 36 && r.rel_err.size() == 36 && r.avar.size() == 36);
  CHECK(r.summary.n == n && r.summary.sample_rate_hz == rate && r.summary.duration == double(n) / rate);
  for (int c = 0; c < 3; ++c) CHECK(r.axes[size_t(c)].status == CALICO_ALLAN_OK && std::fabs(r.axes[size_t(c)].N / N0 - 1.0) <= 0.02);
  CHECK(r.summary.sigma_at_rate == r.MeasurementSigma(rate));

  // the same arrays through the C ABI: the same bits
  int32_t nc = 0;
  int64_t m[CALICO_ALLAN_MAX_CLUSTERS];
  double tau[CALICO_ALLAN_MAX_CLUSTERS], rel[CALICO_ALLAN_MAX_CLUSTERS], avar[CALICO_ALLAN_MAX_CLUSTERS * 3];
  calico_allan_noise axes[3];
  calico_allan_summary sm;
  CHECK(calico_imu_allan(0, n, stamps.data(), 0.0, samples[0].data(), nullptr, &nc, m, tau, avar, rel, axes, &sm) == CALICO_OK);
  CHECK(nc == 36 && std::memcmp(m, r.cluster_sizes.data(), 36 * sizeof(int64_t)) == 0 && std::memcmp(tau, r.tau.data(), 36 * sizeof(double)) == 0);
  CHECK(std::memcmp(rel, r.rel_err.data(), 36 * sizeof(double)) == 0 && std::memcmp(avar, r.avar[0].data(), 36 * 3 * sizeof(double)) == 0);
  CHECK(std::memcmp(axes, r.axes.data(), sizeof(axes)) == 0 && std::memcmp(&sm, &r.summary, sizeof(sm)) == 0);

  // an explicit list
  const int64_t sizes[4] = {1, 10, 100, 1000};
  calico_allan_options o = DefaultAllanOptions();
  o.n_cluster_sizes = 4; o.cluster_sizes = sizes;
  auto listed = CharacterizeImuNoise(stamps, samples, o);
  CHECK(listed.ok() && listed.value().cluster_sizes == std::vector<int64_t>(sizes, sizes + 4));
  for (int j = 0; j < 4; ++j)
    for (size_t q = 0; q < r.cluster_sizes.size(); ++q)
      if (r.cluster_sizes[q] == sizes[j]) CHECK(std::memcmp(listed.value().avar[size_t(j)].data(), r.avar[q].data(), 3 * sizeof(double)) == 0);

  // into the sensors, for a calibration recording at 200 Hz
  Gyroscope gyro;
  CHECK(gyro.ApplyNoise(r, 200.0).ok() && gyro.GetMeasurementNoise() == r.summary.N_pooled * std::sqrt(200.0));
  std::printf("OK\n");
  return 0;
}
