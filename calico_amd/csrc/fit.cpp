// fit.cpp — calico_fit_spline (this part of the C ABI of include/calico_hip.h): the control points of a spline from sorted samples
// (kernels: fit_kernels.hip). Everything that can be checked without a device is checked before the first HIP call. The host
// finds the segment of every sample (the samples are sorted: a CSR over the segments), uploads, launches and reads back.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/calico_hip.h"
#include "arg_rules.hpp"
#include "device_math.hpp"
#include "free_call.hpp"
#include "kernels.hpp"

extern "C" int32_t calico_fit_spline(int32_t device, int32_t order, int32_t n_knots, const double* knots, const double* basis,
                                     int64_t n, const double* stamps, const double* data6, double* ctrl_out) {
  using namespace cal;
  const FreeCall call{"calico_fit_spline"};
  std::string error = spline_shape_error(order, n_knots, kMaxOrder);
  if (error.empty() && (!knots || !basis || !stamps || !data6 || !ctrl_out)) error = "null knots, basis, stamps, data or ctrl_out";
  if (error.empty() && n <= 0) error = "n must be > 0";
  if (!error.empty()) return call.invalid(error);
  if (n > INT32_MAX) return call.fail(CALICO_UNIMPLEMENTED, "more than 2^31 - 1 samples");      // the kernels and seg_ptr index the samples with int
  if (!(error = stamps_error("sample", n, stamps)).empty()) return call.invalid(error);      // samples must be sorted (trajectory.cpp:24)
  const int k = order, n_ctrl = n_knots - k, n_valid = spline_valid_knots(k, n_knots), n_seg = n_valid - 1;
  std::vector<int> seg(static_cast<size_t>(n)), seg_ptr(static_cast<size_t>(n_seg) + 1, 0);
  for (int64_t j = 0; j < n; ++j) {
    const int s = spline_segment(knots + (k - 1), n_valid, stamps[j]);
    if (s < 0) return call.invalid("sample stamp " + std::to_string(j) + " lies off the valid knots");
    seg[size_t(j)] = s;
    seg_ptr[size_t(s) + 1] += 1;
  }
  for (int s = 0; s < n_seg; ++s) seg_ptr[size_t(s) + 1] += seg_ptr[size_t(s)];
  if (fit_solve_lds_bytes(n_ctrl, k) > 156 * 1024) return call.fail(CALICO_UNIMPLEMENTED, "the trajectory is too long for the banded solve in LDS");
  if (int rc = call.select_device(device)) return rc;
  FreeBuf<double> d_stamps, d_data, d_knots, d_basis, d_W, d_band, d_rhs, d_ctrl;
  FreeBuf<int> d_seg, d_ptr, d_status;
  FREE_TRY(call, d_stamps.upload(stamps, size_t(n))); FREE_TRY(call, d_data.upload(data6, size_t(n) * 6));
  FREE_TRY(call, d_knots.upload(knots, size_t(n_knots))); FREE_TRY(call, d_basis.upload(basis, size_t(n_seg) * k * k));
  FREE_TRY(call, d_seg.upload(seg.data(), seg.size())); FREE_TRY(call, d_ptr.upload(seg_ptr.data(), seg_ptr.size()));
  FREE_TRY(call, d_W.alloc(size_t(n) * k)); FREE_TRY(call, d_band.alloc(size_t(n_ctrl) * k)); FREE_TRY(call, d_rhs.alloc(size_t(n_ctrl) * 6));
  FREE_TRY(call, d_ctrl.alloc(size_t(n_ctrl) * 6)); FREE_TRY(call, d_status.alloc(1));
  FitArgs a = {};
  a.n = int(n); a.k = k; a.n_ctrl = n_ctrl; a.n_seg = n_seg;
  a.stamps = d_stamps.p; a.seg = d_seg.p; a.seg_ptr = d_ptr.p; a.knots = d_knots.p; a.basis = d_basis.p; a.data = d_data.p;
  a.W = d_W.p; a.band = d_band.p; a.rhs = d_rhs.p; a.ctrl = d_ctrl.p; a.status = d_status.p;
  FREE_TRY(call, launch_fit_spline(device, a, nullptr));
  int status = 0;
  FREE_TRY(call, d_status.download(&status, 1)); FREE_TRY(call, d_ctrl.download(ctrl_out, size_t(n_ctrl) * 6));
  return status == 0 ? CALICO_OK : call.fail(CALICO_INTERNAL, "a pivot of the normal equations was not finite");
}
