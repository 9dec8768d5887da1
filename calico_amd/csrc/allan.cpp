// allan.cpp — calico_imu_allan (this part of the C ABI of include/calico_hip.h): the overlapping Allan variance of the three axes of
// a static IMU log over a grid of cluster sizes (kernels: allan_kernels.hip) and per axis the IEEE-952 noise coefficients
// (allan_fit.hpp). Everything that can be checked without a device is checked before the first HIP call (arg_rules.hpp). The host
// builds the grid, uploads the samples, enqueues the five launches and reads back once: the variances and the axes' flags in
// one buffer. The fit, the pooled density and the summary are the host's: 3 x 256 numbers.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/calico_hip.h"
#include "allan_fit.hpp"
#include "arg_rules.hpp"
#include "free_call.hpp"
#include "kernels.hpp"

static_assert(cal::kAllanMaxClusters == CALICO_ALLAN_MAX_CLUSTERS, "the launch arguments hold the header's grid");

extern "C" void calico_default_allan_options(calico_allan_options* o) {
  if (!o) return;
  *o = calico_allan_options{};
  o->points_per_decade = 10;
  o->terms = CALICO_ALLAN_TERM_WHITE | CALICO_ALLAN_TERM_BIAS_INSTABILITY | CALICO_ALLAN_TERM_RATE_RANDOM_WALK;
  o->max_tau_fraction = 0.1;
}

extern "C" int32_t calico_imu_allan(int32_t device, int64_t n, const double* stamps, double sample_rate_hz, const double* samples,
                                    const calico_allan_options* options, int32_t* n_clusters_out, int64_t* cluster_sizes_out,
                                    double* tau_out, double* avar_out, double* rel_err_out, calico_allan_noise* noise_out,
                                    calico_allan_summary* summary) {
  using namespace cal;
  const FreeCall call{"calico_imu_allan"};
  calico_allan_options o;
  if (options) o = *options; else calico_default_allan_options(&o);
  std::string error;
  if (n < 3) error = "n must be >= 3";
  if (error.empty() && (!samples || !n_clusters_out || !cluster_sizes_out || !tau_out || !avar_out || !rel_err_out || !noise_out || !summary))
    error = "null samples or output buffer";
  if (error.empty()) error = allan_options_error(o);
  if (!error.empty()) return call.invalid(error);
  if (n > INT32_MAX) return call.fail(CALICO_UNIMPLEMENTED, "more than 2^31 - 1 samples");      // the kernels index the samples with int
  double rate = 0.0;
  if (!(error = allan_rate_error(n, stamps, sample_rate_hz, &rate)).empty()) return call.invalid(error);
  int64_t grid[CALICO_ALLAN_MAX_CLUSTERS];
  int nc = 0;
  if (!(error = allan_grid_error(n, o, grid, &nc)).empty()) return call.invalid(error);
  if (int rc = call.select_device(device)) return rc;

  AllanArgs a = {};
  a.n = int(n); a.n_blocks = allan_blocks(a.n); a.n_clusters = nc; a.n_chunks = allan_chunks(a.n, int(grid[0]));
  a.dt = 1.0 / rate;
  a.plane = (size_t(n) + 2) & ~size_t(1);
  for (int j = 0; j < nc; ++j) a.m[j] = int(grid[j]);
  FreeBuf<double> d_samples, d_block_sum, d_offsets, d_mean, d_theta, d_partial, d_out;
  FreeBuf<int> d_flags;
  FREE_TRY(call, d_samples.upload(samples, size_t(n) * 3));
  FREE_TRY(call, d_block_sum.alloc(size_t(3) * a.n_blocks)); FREE_TRY(call, d_offsets.alloc(size_t(3) * a.n_blocks)); FREE_TRY(call, d_mean.alloc(3));
  FREE_TRY(call, d_theta.alloc(3 * a.plane)); FREE_TRY(call, d_partial.alloc(size_t(3) * nc * a.n_chunks));
  FREE_TRY(call, d_out.alloc(size_t(nc) * 3 + 3)); FREE_TRY(call, d_flags.alloc(3)); FREE_TRY(call, d_flags.zero(3));
  a.samples = d_samples.p; a.block_sum = d_block_sum.p; a.offsets = d_offsets.p; a.mean = d_mean.p; a.theta = d_theta.p;
  a.partial = d_partial.p; a.out = d_out.p; a.flags = d_flags.p;
  FREE_TRY(call, launch_imu_allan(a, nullptr));
  std::vector<double> out(size_t(nc) * 3 + 3);
  FREE_TRY(call, d_out.download(out.data(), out.size()));

  // the host's part: the grid's columns, the fit per axis, the pooled values
  double weight[CALICO_ALLAN_MAX_CLUSTERS];
  *n_clusters_out = nc;
  for (int j = 0; j < nc; ++j) {
    cluster_sizes_out[j] = grid[j];
    tau_out[j] = double(grid[j]) * a.dt;
    weight[j] = 2.0 * (double(n) / double(grid[j]) - 1.0);
    rel_err_out[j] = 1.0 / std::sqrt(weight[j]);
    for (int c = 0; c < 3; ++c) avar_out[size_t(j) * 3 + c] = out[size_t(j) * 3 + c];
  }
  const double duration = double(n) / rate;
  double n2 = 0.0, drift = 0.0;
  for (int c = 0; c < 3; ++c) {
    if (out[size_t(nc) * 3 + c] != 0.0) {
      noise_out[c] = calico_allan_noise{};
      noise_out[c].status = CALICO_ALLAN_NONFINITE;
    } else {
      allan_fit_axis(nc, tau_out, weight, avar_out + c, 3, o.terms, &noise_out[c]);
    }
    n2 += noise_out[c].N * noise_out[c].N;
    drift = std::fmax(drift, noise_out[c].K * std::sqrt(duration));
  }
  summary->n = n; summary->sample_rate_hz = rate; summary->duration = duration;
  summary->N_pooled = std::sqrt(n2 / 3.0);
  summary->sigma_at_rate = summary->N_pooled * std::sqrt(rate);
  summary->bias_drift_over_recording = drift;
  return CALICO_OK;
}
