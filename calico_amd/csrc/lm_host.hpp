// lm_host.hpp — the host's side of the estimators whose LM loop runs on the device (chart.cpp, rig.cpp): the poll loop over a
// control word that begins with LmControl, and the resection that gives them their start (and is calico_camera_resect itself).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/calico_hip.h"
#include "free_call.hpp"
#include "kernels.hpp"

namespace cal {

// Runs the device's loop to its end. enqueue_cycle() enqueues one LM cycle -- evaluate, decide, eliminate, reduce -- and returns
// a hipError_t. The cycles are enqueued six at a time; between the groups the host reads the control word's first field (`done`),
// only to stop enqueuing: launches behind the end return at once. Every cycle tries a step or raises lambda tenfold after a
// reduced system that was not positive definite (at most 24 times in a row): the loop ends on its own; the bound only guards the
// host against a control word that never moves. Returns CALICO_OK or the call's failure.
template <class EnqueueCycle>
int run_device_lm(const FreeCall& call, const int* done_ptr, int max_iterations, EnqueueCycle&& enqueue_cycle) {
  constexpr int kPollCycles = 6;
  const int64_t max_cycles = 26 * (int64_t(max_iterations) + 2);
  int done = 0;
  for (int64_t cycle = 0; !done; cycle += kPollCycles) {
    if (cycle > max_cycles) return call.fail(CALICO_INTERNAL, "the device loop did not end");
    for (int i = 0; i < kPollCycles; ++i) FREE_TRY(call, enqueue_cycle());
    FREE_TRY(call, hipMemcpy(&done, done_ptr, sizeof(int), hipMemcpyDeviceToHost));
  }
  return CALICO_OK;
}

// The workspace and the outputs of a resection (resect_kernels.hip) of up to `frames` frames and `pairs` pairs that live on the
// device already.
struct ResectRun {
  FreeBuf<double> ws, q, t, rms, cov;
  FreeBuf<int32_t> used, iterations;
  FreeBuf<uint8_t> status;
  hipError_t alloc(size_t frames, size_t pairs, bool with_cov) {
    const hipError_t es[] = {ws.alloc(pairs * 2), q.alloc(frames * 4), t.alloc(frames * 3), rms.alloc(frames), used.alloc(frames),
                             iterations.alloc(frames), status.alloc(frames), with_cov ? cov.alloc(frames * 36) : hipSuccess};
    for (const hipError_t e : es)      // (what was allocated is freed with the call)
      if (e != hipSuccess) return e;
    return hipSuccess;
  }
  // flags: one zeroed byte per pair; q_init and t_init: both null (the kernel makes its own start) or device memory
  ResectArgs args(const calico_resection_options& o, const double* k, int64_t n_frames, const int64_t* offsets, const double* pixels,
                  const double* points, uint8_t* flags, const double* q_init, const double* t_init) const {
    ResectArgs a = {};
    a.k = k; a.n_frames = n_frames; a.offsets = offsets; a.pixels = pixels; a.points = points; a.q_init = q_init; a.t_init = t_init;
    a.ws = ws.p; a.flags = flags;
    a.max_iterations = o.max_iterations; a.step_tolerance = o.step_tolerance; a.huber_scale = o.huber_scale; a.min_points = o.min_points;
    a.q_out = q.p; a.t_out = t.p; a.rms_out = rms.p; a.n_used_out = used.p; a.iterations_out = iterations.p; a.status_out = status.p;
    a.cov_out = cov.p;
    return a;
  }
  // the resection from the kernel's own start, and what a caller that only wants a start reads of it
  hipError_t start(int model, const calico_resection_options& o, const double* k, size_t n_frames, const int64_t* offsets, const double* pixels,
                   const double* points, uint8_t* flags, double* q_host, double* t_host, uint8_t* status_host) {
    hipError_t e = launch_camera_resect(model, args(o, k, int64_t(n_frames), offsets, pixels, points, flags, nullptr, nullptr), nullptr);
    if (e == hipSuccess) e = q.download(q_host, n_frames * 4);
    if (e == hipSuccess) e = t.download(t_host, n_frames * 3);
    if (e == hipSuccess) e = status.download(status_host, n_frames);
    return e;
  }
};

}  // namespace cal
