// analysis.cpp — what is read from a solved problem: the covariance of the calibration estimates and of the trajectory, the
// prediction covariance with leverage, and the observability report (this part of the C ABI of include/calico_hip.h).
// Describing a problem is calico_hip.cpp, planning it plan.cpp, solving it solve.cpp; the kernels are cov_kernels.hip,
// obs_kernels.hip and prediction_items_kernel (eval_kernels.hip). The covariance and the observability pass open the same way
// (ReducedPass).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/calico_hip.h"
#include "calico_hip_testing.h"
#include "kernels.hpp"
#include "problem_dev.hpp"
#include "problem_host.hpp"

namespace {

// The undamped pass of the covariance and of the observability compute, up to the reduced system: one evaluation (as the LM
// loop's, exchange included; the phase timer records nothing of it) and the linear solve's reduction WITHOUT damping and
// Jacobi scaling -- the pass's own LM state (an infinite radius), a Jacobi scale of ones, damping and solution buffers
// (calico_problem::pass): nothing of the LM's is touched.
struct ReducedPass {
  SolveArgs sa;
  LinearRoute rt;             // of the pass's one linear solve (the solve's switches as set when the pass opens)
  LmOptionsDev o = {};
  int m = 0, mc = 0;          // rows of the reduced system, calibration columns among them
  CpCovArgs ca = {};          // the control points' band (filled by begin_reduced_pass(band = true))
  double R01[2] = {0.0, 0.0}; // [cost, evaluation-failed flag] of the pass's evaluation
};

// the shared preconditions, the plan, the device, the sizes
int open_reduced_pass(calico_problem* p, ReducedPass& rp) {
  if (int rc = require_exchange(p)) return rc;
  const int rc = finalize(p);
  if (rc != CALICO_OK) return rc;
  HIP_TRY(p, hipSetDevice(p->device));
  rp.sa = make_solve_args(p);
  rp.rt = linear_route(p, rp.sa, SolveSwitches{});
  rp.mc = p->m; rp.m = rp.sa.m;
  return CALICO_OK;
}

// The pass's buffers, the parameter upload and the evaluation. band: the buffers of the control points' band factor and what
// CpCovArgs takes from the solve's arguments. On return rp.sa points at the pass's buffers and rp.o holds the damping bounds:
// reduce_pass() then leaves the undamped, unscaled reduced system in rp.sa.Spart.
int begin_reduced_pass(calico_problem* p, ReducedPass& rp, bool band) {
  calico_problem::PassBuffers& b = p->pass;
  SolveArgs& sa = rp.sa;
  if (band) {
    const int n_cp = p->n_cp, k = p->order;
    HIP_TRY(p, b.cp_dq.alloc(6 * size_t(n_cp))); HIP_TRY(p, b.cp_L.alloc(size_t(n_cp) * k * 36)); HIP_TRY(p, b.cp_Li.alloc(size_t(n_cp) * 36));
    HIP_TRY(p, b.cp_info.alloc(2));
    rp.ca.R = sa.R; rp.ca.off_B = sa.off_B(); rp.ca.off_E = sa.off_E(); rp.ca.n_cp = n_cp; rp.ca.k = k; rp.ca.mc = rp.mc;
    rp.ca.dq = b.cp_dq.p; rp.ca.L = b.cp_L.p; rp.ca.Li = b.cp_Li.p; rp.ca.info = b.cp_info.p;
  }
  const int NT = sa.NT(), ny = NT + p->border_extra();
  // (the same sizes as the workspace's buffers they stand in for: prepare_workspace)
  HIP_TRY(p, b.st.alloc(1)); HIP_TRY(p, b.scale.alloc(2 * size_t(NT))); HIP_TRY(p, b.dadd.alloc(size_t(NT)));
  HIP_TRY(p, b.y.alloc(size_t(ny) + 64)); HIP_TRY(p, b.zbuf.alloc(size_t(sa.n_s()) + 64));
  hipStream_t s = p->stream;
  {
    const std::vector<double> ones(2 * size_t(NT), 1.0);      // [Jacobi scale s | 1 / s^2]: no scaling
    HIP_TRY(p, hipMemcpyAsync(b.scale.p, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(p, hipStreamSynchronize(s));      // (`ones` is a local)
  }
  int rc = upload_x(p);
  if (rc != CALICO_OK) return rc;
  {
    // (the phase timer measures the LM loop: the pass records nothing into it)
    const int mask = p->timer.mask;
    p->timer.mask = 0;
    rc = enqueue_jacobian_eval(p, nullptr, 0);      // R(x) into reduce buffer 0, all ranks' sum
    p->timer.mask = mask;
  }
  if (rc != CALICO_OK) return rc;
  // damping = clamp(v s², min, max) / (radius s²) = 0 with s = 1 and an infinite radius (FromR::damping, prepare_kernel)
  launch_init_state(b.st.p, std::numeric_limits<double>::infinity(), 0.0, s);
  sa.st = b.st.p; sa.scale = b.scale.p; sa.dadd = b.dadd.p; sa.y = b.y.p; sa.zbuf = b.zbuf.p; sa.progress = nullptr;
  rp.o = {};
  rp.o.min_lm_diagonal = 1e-6; rp.o.max_lm_diagonal = 1e32;
  (void)hipGetLastError();
  return CALICO_OK;
}

// the reduction, stopped once the reduced system is formed (nothing to reduce onto without calibration columns)
int reduce_pass(calico_problem* p, const ReducedPass& rp) {
  if (rp.mc == 0) return CALICO_OK;
  enqueue_linear_solve(p, rp.sa, rp.rt, rp.o, /*with_post_eval=*/0, /*jacobi=*/0, /*reduce_only=*/true);
  HIP_TRY(p, hipGetLastError());
  return CALICO_OK;
}

// the evaluation's status (rp.R01: read back by the caller behind its launches), looked at once the stream is through
int evaluation_failed(calico_problem* p, const ReducedPass& rp, const char* what) {
  if (rp.R01[1] > 0.0) return p->set_error(CALICO_FAILED_PRECONDITION, std::string(what) + ": the residual evaluation failed at the current parameter values");
  return CALICO_OK;
}

// the blocks' layout as a compute leaves it for the readers of its result
std::vector<calico_problem::BlockSnapshot> snapshot_blocks(const calico_problem* p) {
  std::vector<calico_problem::BlockSnapshot> out(p->blocks.size());
  for (size_t i = 0; i < p->blocks.size(); ++i) {
    const HBlock& h = p->blocks[i];
    const bool in = !h.constant && h.used;
    const bool is_cp = h.tan >= 0 && h.tan < 6 * p->n_cp;
    out[i] = {in ? (is_cp ? calico_problem::kBlockControlPoint : h.tan - 6 * p->n_cp) : calico_problem::kBlockAbsent, h.size, h.tangent_size(),
              h.manifold, h.v, is_cp ? h.tan / 6 : -1};
  }
  return out;
}

// One rule per family for every reader: does the stored result describe the problem as it stands? (p->dirty: the structure
// changed since the compute -- blocks, sensors, observations --; the next finalisation drops the result)
const char* const kNoCovariance = "no covariance of this problem: call calico_covariance_compute (again, if the problem changed) and check its status";
bool covariance_ready(const calico_problem* p) { return p->cov.valid && !p->dirty; }
const char* const kNoObservability = "no observability report of this problem: call calico_observability_compute (again, if the problem "
                                     "changed) and check its status";
bool observability_ready(const calico_problem* p) { return p->obs.valid && !p->dirty; }

}  // namespace

extern "C" {

void calico_default_covariance_options(calico_covariance_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->min_relative_pivot = 1e-12;
}

// Σ = (JᵀJ)⁻¹ of the calibration blocks at the current values: one evaluation (as the LM loop's, exchange included), the
// linear solve's reduction WITHOUT damping and Jacobi scaling -- a state of its own with an infinite radius, a scale of
// ones --, stopped once the reduced system is formed, then covariance_kernel (cov_kernels.hip). The LM state, the
// parameter buffers, the iteration log and the plan / workspace sizes are left alone.
int32_t calico_covariance_compute(calico_problem* p, const calico_covariance_options* opt) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  calico_covariance_options def;
  calico_default_covariance_options(&def);
  if (!opt) opt = &def;
  if (!(opt->min_relative_pivot >= 0.0)) return p->set_error(CALICO_INVALID_ARGUMENT, "min_relative_pivot must be >= 0");
  ReducedPass rp;
  int rc = open_reduced_pass(p, rp);
  if (rc != CALICO_OK) return rc;
  calico_problem::Covariance& cv = p->cov;
  cv.valid = false;
  cv.has_cp = false;
  cv.cp_requested = opt->control_points != 0;
  const SolveArgs& sa = rp.sa;
  const int mc = rp.mc, m = rp.m;
  if (m > covariance_max_dim())
    return p->set_error(CALICO_UNIMPLEMENTED, "covariance: reduced system of " + std::to_string(m) + " rows (at most " +
                                                  std::to_string(covariance_max_dim()) + ")");
  const bool want_cp = opt->control_points != 0 && p->n_cp > 0;
  if (want_cp && p->order > cp_covariance_max_order())
    return p->set_error(CALICO_UNIMPLEMENTED, "covariance: the trajectory's control-point blocks are computed for spline orders up to " +
                                                  std::to_string(cp_covariance_max_order()));
  if (want_cp) {
    const size_t nb = size_t(p->n_cp) * p->order * 36, ne = size_t(6) * p->n_cp * mc;
    HIP_TRY(p, cv.cp_M.alloc(nb)); HIP_TRY(p, cv.cp_X.alloc(ne)); HIP_TRY(p, cv.cp_W.alloc(ne)); HIP_TRY(p, cv.cp_Z.alloc(nb));
    HIP_TRY(p, cv.cp_sae.alloc(ne)); HIP_TRY(p, cv.cp_band.alloc(nb));
  }
  HIP_TRY(p, cv.out.alloc(size_t(mc) * mc)); HIP_TRY(p, cv.info.alloc(4));
  if (!covariance_in_lds(m)) HIP_TRY(p, cv.work.alloc(size_t(m) * covariance_ld(m)));
  HIP_TRY(p, configure_covariance_kernel(p->device));
  hipStream_t s = p->stream;
  rc = begin_reduced_pass(p, rp, want_cp);
  if (rc != CALICO_OK) return rc;
  CpCovArgs& ca = rp.ca;
  if (want_cp) {      // (reads the band and E of R as the evaluation left them: ahead of the reduction)
    ca.M = cv.cp_M.p; ca.X = cv.cp_X.p; ca.W = cv.cp_W.p; ca.Z = cv.cp_Z.p; ca.sae = cv.cp_sae.p; ca.band = cv.cp_band.p;
    launch_cp_covariance_band(ca, s);
    HIP_TRY(p, hipGetLastError());
  }
  rc = reduce_pass(p, rp);
  if (rc != CALICO_OK) return rc;
  if (mc > 0) {
    launch_covariance(sa.Spart, reduced_schur_slices(sa), m, mc, sa.R + sa.off_C(), sa.st, cv.work.p, cv.out.p, cv.info.p, s);
    HIP_TRY(p, hipGetLastError());
  }
  if (want_cp) {
    ca.sigma = cv.out.p;
    launch_cp_covariance_finish(ca, s);
    HIP_TRY(p, hipGetLastError());
  }
  double info[4] = {1.0, 0.0, 0.0, 0.0};
  HIP_TRY(p, hipMemcpyAsync(rp.R01, p->d_R.p, sizeof(rp.R01), hipMemcpyDeviceToHost, s));
  cv.sigma.assign(size_t(mc) * mc, 0.0);
  if (mc > 0) {
    HIP_TRY(p, hipMemcpyAsync(info, cv.info.p, sizeof(info), hipMemcpyDeviceToHost, s));
    HIP_TRY(p, hipMemcpyAsync(cv.sigma.data(), cv.out.p, cv.sigma.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  double cp_info[2] = {1.0, 0.0};
  cv.sae.clear(); cv.band.clear();
  if (want_cp) {
    cv.sae.resize(size_t(6) * p->n_cp * mc); cv.band.resize(size_t(p->n_cp) * p->order * 36);
    HIP_TRY(p, hipMemcpyAsync(cp_info, ca.info, sizeof(cp_info), hipMemcpyDeviceToHost, s));
    if (!cv.sae.empty()) HIP_TRY(p, hipMemcpyAsync(cv.sae.data(), cv.cp_sae.p, cv.sae.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(p, hipMemcpyAsync(cv.band.data(), cv.cp_band.p, cv.band.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(p, hipStreamSynchronize(s));
  if (int failed = evaluation_failed(p, rp, "covariance")) return failed;
  cv.dim = mc; cv.min_relative_pivot = info[0]; cv.n_unobserved = int(info[2]);
  const int flags = int(info[1]);
  if (flags & (kInfoNonFiniteInput | kInfoEliminationFailed | kInfoNonFiniteResult))
    return p->set_error(CALICO_FAILED_PRECONDITION, std::string("covariance: JᵀJ is rank deficient or not finite (") +
                                                        ((flags & kInfoEliminationFailed) ? "a block of the control points' elimination is not positive definite"
                                                         : (flags & kInfoNonFiniteInput) ? "non-finite value in the reduced system" : "non-finite value in the result") + ")");
  if ((flags & kInfoPivotNotPositive) || info[0] < opt->min_relative_pivot) {
    char msg[256];
    std::snprintf(msg, sizeof(msg), "covariance: JᵀJ is rank deficient (minimum relative pivot %.3e, threshold %.3e): a gauge freedom "
                  "or a parameter the data do not determine", info[0], opt->min_relative_pivot);
    return p->set_error(CALICO_FAILED_PRECONDITION, msg);
  }
  if (want_cp) {
    const int cpf = int(cp_info[1]);
    bool finite = true;
    for (double v : cv.sae) finite = finite && std::isfinite(v);
    for (double v : cv.band) finite = finite && std::isfinite(v);
    if ((cpf & 1) || !finite)
      return p->set_error(CALICO_FAILED_PRECONDITION, "covariance: the trajectory's control-point block of JᵀJ is not finite");
    if ((cpf & 2) || cp_info[0] < opt->min_relative_pivot) {
      char msg[256];
      std::snprintf(msg, sizeof(msg), "covariance: the trajectory's control-point band of JᵀJ is rank deficient (minimum relative pivot %.3e, "
                    "threshold %.3e): the data do not determine the trajectory", cp_info[0], opt->min_relative_pivot);
      return p->set_error(CALICO_FAILED_PRECONDITION, msg);
    }
    cv.n_cp = p->n_cp; cv.order = p->order; cv.min_relative_pivot_band = cp_info[0];
  }
  cv.blocks = snapshot_blocks(p);
  cv.has_cp = want_cp;
  cv.valid = true;
  return CALICO_OK;
}

int32_t calico_covariance_info(calico_problem* p, int32_t* dim, int32_t* n_unobserved, double* min_relative_pivot) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (!covariance_ready(p)) return p->set_error(CALICO_FAILED_PRECONDITION, kNoCovariance);
  if (dim) *dim = p->cov.dim;
  if (n_unobserved) *n_unobserved = p->cov.n_unobserved;
  if (min_relative_pivot) *min_relative_pivot = p->cov.min_relative_pivot;
  return CALICO_OK;
}

int32_t calico_covariance_get_dense(calico_problem* p, double* out) {
  if (!p || !out) return CALICO_INVALID_ARGUMENT;
  if (!covariance_ready(p)) return p->set_error(CALICO_FAILED_PRECONDITION, kNoCovariance);
  std::copy(p->cov.sigma.begin(), p->cov.sigma.end(), out);
  return CALICO_OK;
}

namespace {
// EigenQuaternionManifold::PlusJacobian at x (storage x, y, z, w): 4x3 row-major
void quat_plus_jacobian(const double* x, double J[12]) {
  const double X = x[0], Y = x[1], Z = x[2], W = x[3];
  const double j[12] = {W, Z, -Y, -Z, W, X, Y, -X, W, -X, -Y, -Z};
  std::copy(j, j + 12, J);
}
}  // namespace

int32_t calico_covariance_get_block(calico_problem* p, int32_t block_a, int32_t block_b, int32_t tangent, double* out) {
  if (!p || !out) return CALICO_INVALID_ARGUMENT;
  const int nb = int(p->blocks.size());
  if (block_a < 0 || block_a >= nb || block_b < 0 || block_b >= nb) return p->set_error(CALICO_INVALID_ARGUMENT, "covariance: unknown parameter block id");
  if (!covariance_ready(p) || size_t(nb) != p->cov.blocks.size()) return p->set_error(CALICO_FAILED_PRECONDITION, kNoCovariance);
  const calico_problem::BlockSnapshot& A = p->cov.blocks[size_t(block_a)];
  const calico_problem::BlockSnapshot& B = p->cov.blocks[size_t(block_b)];
  const calico_problem::Covariance& cv = p->cov;
  constexpr int kAbsent = calico_problem::kBlockAbsent, kCp = calico_problem::kBlockControlPoint;
  if ((A.off == kCp || B.off == kCp) && !cv.has_cp)
    return p->set_error(CALICO_UNIMPLEMENTED, "covariance: control-point blocks are not computed (calico_covariance_options.control_points = 0)");
  if (A.off == kCp && B.off == kCp && std::abs(A.cp - B.cp) >= cv.order)
    return p->set_error(CALICO_UNIMPLEMENTED, "covariance: control-point pairs are computed only within the spline's support (control "
                                              "points less than the spline order apart)");
  const bool qa = A.manifold == CALICO_MANIFOLD_EIGEN_QUATERNION, qb = B.manifold == CALICO_MANIFOLD_EIGEN_QUATERNION;
  const int ta = A.tsize, tb = B.tsize;
  const int ra = tangent ? ta : A.size, rb = tangent ? tb : B.size;
  std::fill(out, out + size_t(ra) * rb, 0.0);
  if (A.off == kAbsent || B.off == kAbsent) return CALICO_OK;      // constant / unused blocks: zeros (Ceres: constant)
  const int oa = A.off, ob = B.off, dim = cv.dim;
  // (a border offset must leave room for its block; a control point must be one of the computed ones)
  const auto in_range = [&](const calico_problem::BlockSnapshot& X, int tx) {
    return X.off >= 0 ? X.off + tx <= dim : X.cp >= 0 && X.cp < cv.n_cp && tx == 6;
  };
  if (!in_range(A, ta) || !in_range(B, tb)) return p->set_error(CALICO_INTERNAL, "covariance: block layout out of range");
  std::vector<double> t(size_t(ta) * tb);
  for (int i = 0; i < ta; ++i)
    for (int j = 0; j < tb; ++j) {
      double v;
      if (oa >= 0 && ob >= 0) v = cv.sigma[size_t(oa + i) * dim + (ob + j)];
      else if (oa == kCp && ob >= 0) v = cv.sae[size_t(6 * A.cp + i) * dim + (ob + j)];       // Σ_AE
      else if (ob == kCp && oa >= 0) v = cv.sae[size_t(6 * B.cp + j) * dim + (oa + i)];
      else {                                                                                  // Σ_AA's band
        const int hi = std::max(A.cp, B.cp), lo = std::min(A.cp, B.cp);
        const double* b = cv.band.data() + (size_t(lo) * cv.order + (hi - lo)) * 36;
        v = A.cp >= B.cp ? b[i * 6 + j] : b[j * 6 + i];
      }
      t[size_t(i) * tb + j] = v;
    }
  if (tangent) { std::copy(t.begin(), t.end(), out); return CALICO_OK; }
  // ambient: P_a Σ P_bᵀ, P the manifold's PlusJacobian at the value Σ was computed at (identity for Euclidean blocks)
  double Pa[12], Pb[12];
  if (qa) quat_plus_jacobian(A.v.data(), Pa);
  if (qb) quat_plus_jacobian(B.v.data(), Pb);
  std::vector<double> u(size_t(ra) * tb);       // P_a t
  for (int i = 0; i < ra; ++i)
    for (int j = 0; j < tb; ++j) {
      double v = 0.0;
      if (qa) { for (int k = 0; k < 3; ++k) v += Pa[i * 3 + k] * t[size_t(k) * tb + j]; }
      else v = t[size_t(i) * tb + j];
      u[size_t(i) * tb + j] = v;
    }
  for (int i = 0; i < ra; ++i)
    for (int j = 0; j < rb; ++j) {
      double v = 0.0;
      if (qb) { for (int k = 0; k < 3; ++k) v += u[size_t(i) * tb + k] * Pb[j * 3 + k]; }
      else v = u[size_t(i) * tb + j];
      out[size_t(i) * rb + j] = v;
    }
  return CALICO_OK;
}

namespace {
// the readers of the trajectory's blocks: CALICO_OK when the last compute produced them for the problem as it stands
int trajectory_result_ready(calico_problem* p) {
  const calico_problem::Covariance& cv = p->cov;
  if (covariance_ready(p) && !cv.has_cp && cv.cp_requested)
    return p->set_error(CALICO_FAILED_PRECONDITION, "no covariance of the trajectory: the problem has no spline control points "
                                                    "(calico_problem_set_spline)");
  if (!covariance_ready(p) || !cv.has_cp)
    return p->set_error(CALICO_FAILED_PRECONDITION, "no covariance of the trajectory: call calico_covariance_compute with control_points = 1 "
                                                    "(again, if the problem changed) and check its status");
  return CALICO_OK;
}
}  // namespace

int32_t calico_covariance_trajectory_info(calico_problem* p, int32_t* n_cp, int32_t* order, double* min_relative_pivot_band) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (int rc = trajectory_result_ready(p)) return rc;
  if (n_cp) *n_cp = p->cov.n_cp;
  if (order) *order = p->cov.order;
  if (min_relative_pivot_band) *min_relative_pivot_band = p->cov.min_relative_pivot_band;
  return CALICO_OK;
}

// Σ_v(t) at each stamp from Σ_AA's band on the device (cp_stamp_kernel); the segment of a stamp is Interpolate's
int32_t calico_covariance_trajectory(calico_problem* p, int64_t n, const double* stamps, double* out) {
  if (!p || n < 0 || (n > 0 && (!stamps || !out))) return CALICO_INVALID_ARGUMENT;
  if (int rc = trajectory_result_ready(p)) return rc;
  if (n == 0) return CALICO_OK;
  if (n > int64_t((INT32_MAX - 255) / 36)) return p->set_error(CALICO_INVALID_ARGUMENT, "covariance: too many stamps in one call");
  calico_problem::Covariance& cv = p->cov;
  std::vector<int> seg(static_cast<size_t>(n));
  std::vector<double> t(stamps, stamps + n);
  for (int64_t i = 0; i < n; ++i) {
    seg[size_t(i)] = spline_index(p, stamps[i]);
    if (seg[size_t(i)] < 0) {
      char msg[160];
      std::snprintf(msg, sizeof(msg), "covariance: stamp %lld (%.17g) is outside the trajectory's valid knots [%.17g, %.17g]", (long long)i,
                    stamps[i], p->valid_knots.front(), p->valid_knots.back());
      return p->set_error(CALICO_INVALID_ARGUMENT, msg);
    }
  }
  HIP_TRY(p, hipSetDevice(p->device));
  hipStream_t s = p->stream;
  HIP_TRY(p, cv.st_t.upload(t, s));
  HIP_TRY(p, cv.st_seg.upload(seg, s));
  HIP_TRY(p, cv.st_out.alloc(size_t(n) * 36));
  (void)hipGetLastError();
  launch_cp_stamps(int(n), cv.order, cv.st_t.p, cv.st_seg.p, p->d_knots.p, p->d_basis.p, cv.cp_band.p, cv.st_out.p, s);
  HIP_TRY(p, hipGetLastError());
  HIP_TRY(p, hipMemcpyAsync(out, cv.st_out.p, size_t(n) * 36 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(p, hipStreamSynchronize(s));
  return CALICO_OK;
}

void calico_default_prediction_options(calico_prediction_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->apply_loss = 1;
}

// P_i = J_i Σ J_iᵀ of every registered observation of a sensor (prediction_items_kernel): J_i at the current values, Σ the
// device copies the last compute with control_points = 1 left (Σ_EE in cov.out, Σ_AE in cov.cp_sae, Σ_AA's band in
// cov.cp_band). Output buffers of its own; nothing of the LM's, of the residual cache or of the stored reports is touched.
int32_t calico_prediction_covariance(calico_problem* p, int32_t sid, const calico_prediction_options* opt, double* cov_out,
                                     double* leverage_out, uint8_t* valid) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  calico_prediction_options def;
  calico_default_prediction_options(&def);
  if (!opt) opt = &def;
  if (sid < 0 || sid >= int(p->sensors.size())) return p->set_error(CALICO_INVALID_ARGUMENT, "prediction covariance: unknown sensor id");
  if (opt->apply_loss != 0 && opt->apply_loss != 1) return p->set_error(CALICO_INVALID_ARGUMENT, "prediction covariance: apply_loss must be 0 or 1");
  if (!cov_out && !leverage_out && !valid) return p->set_error(CALICO_INVALID_ARGUMENT, "prediction covariance: no output buffer");
  if (int rc = trajectory_result_ready(p)) return rc;
  calico_problem::Covariance& cv = p->cov;
  if (cv.n_cp != p->n_cp || cv.order != p->order || cv.dim != p->m) return p->set_error(CALICO_INTERNAL, "prediction covariance: stored covariance does not match the plan");
  const HSensor& hs = p->sensors[size_t(sid)];
  const int64_t n = hs.n();
  if (n == 0) return CALICO_OK;
  const size_t lds_bytes = pred_lds_doubles(p->pred_cols, p->pred_row_pad) * sizeof(double);
  if (lds_bytes > kLdsBudget) {
    char msg[200];
    std::snprintf(msg, sizeof(msg), "prediction covariance: a residual block of %d Jacobian columns needs %zu bytes of LDS staging (at most %zu)",
                  p->pred_cols, lds_bytes, kLdsBudget);
    return p->set_error(CALICO_UNIMPLEMENTED, msg);
  }
  HIP_TRY(p, hipSetDevice(p->device));
  int rc = upload_x(p);
  if (rc != CALICO_OK) return rc;
  const int dim = hs.dim(), dd = dim * dim;
  const int64_t nrange = hs.sorted_end - hs.sorted_begin;      // (layouts are per sensor: the sensor's observations are contiguous)
  if (nrange != n) return p->set_error(CALICO_INTERNAL, "prediction covariance: the sensor's observations are not contiguous");
  hipStream_t s = p->stream;
  DevBuf<double> d_cov, d_lev;
  DevBuf<uint8_t> d_val;
  HIP_TRY(p, d_cov.alloc(size_t(n) * dd)); HIP_TRY(p, d_lev.alloc(size_t(n))); HIP_TRY(p, d_val.alloc(size_t(n)));
  PredArgs pa = {};
  pa.e = make_eval_args(p, p->d_x.p, opt->apply_loss, false);
  pa.e.items = p->d_items_all.p; pa.e.n_items = p->n_items_all;      // every rank evaluates all blocks
  pa.e.active = nullptr;                                             // tagged observations included
  pa.e.row_pad = p->pred_row_pad; pa.e.lds_cols = (p->pred_cols + 15) & ~15;
  pa.sensor = sid; pa.obs_begin = int(hs.sorted_begin); pa.n_cp = p->n_cp; pa.mc = p->m;
  pa.colmap = p->d_pred_map.p; pa.map_stride = p->pred_map_stride;
  pa.sigma = cv.out.p; pa.sae = cv.cp_sae.p; pa.band = cv.cp_band.p;
  pa.cov = d_cov.p; pa.leverage = d_lev.p; pa.valid = d_val.p;
  (void)hipGetLastError();
  HIP_TRY(p, configure_prediction_kernels(p->device));
  HIP_TRY(p, launch_prediction(pa, lds_bytes, s));
  std::vector<double> hc(size_t(n) * dd), hl(static_cast<size_t>(n));
  std::vector<uint8_t> hv(static_cast<size_t>(n));
  HIP_TRY(p, hipMemcpyAsync(hc.data(), d_cov.p, hc.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(p, hipMemcpyAsync(hl.data(), d_lev.p, hl.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(p, hipMemcpyAsync(hv.data(), d_val.p, hv.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(p, hipStreamSynchronize(s));
  for (int64_t i = 0; i < n; ++i) {
    const size_t q = size_t(hs.sorted_pos[size_t(i)] - hs.sorted_begin);
    if (cov_out) std::copy(hc.begin() + q * dd, hc.begin() + (q + 1) * dd, cov_out + i * dd);
    if (leverage_out) leverage_out[i] = hl[q];
    if (valid) valid[i] = hv[q];
  }
  return CALICO_OK;
}

void calico_default_observability_options(calico_observability_options* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->weak_threshold = 1e-10;
  o->min_relative_pivot = 1e-12;
}

// The spectrum of S̃ = D⁻¹ (C - Eᵀ A⁻¹ E) D⁻¹ at the current values: the covariance pass's evaluation and undamped reduction
// (ReducedPass), the band's own factorisation for its minimum relative pivot (cp_band_factor_kernel, natural order:
// is A invertible at all?), then observability_kernel (obs_kernels.hip). Leaves alone what the covariance pass leaves alone,
// and the stored covariance.
int32_t calico_observability_compute(calico_problem* p, const calico_observability_options* opt) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  calico_observability_options def;
  calico_default_observability_options(&def);
  if (!opt) opt = &def;
  if (!(opt->min_relative_pivot >= 0.0)) return p->set_error(CALICO_INVALID_ARGUMENT, "min_relative_pivot must be >= 0");
  if (!(opt->weak_threshold >= 0.0)) return p->set_error(CALICO_INVALID_ARGUMENT, "weak_threshold must be >= 0");
  ReducedPass rp;
  int rc = open_reduced_pass(p, rp);
  if (rc != CALICO_OK) return rc;
  calico_problem::Observability& ob = p->obs;
  ob.valid = false;
  const SolveArgs& sa = rp.sa;
  const int mc = rp.mc, m = rp.m;
  if (mc > observability_max_border())
    return p->set_error(CALICO_UNIMPLEMENTED, "observability: border of " + std::to_string(mc) + " columns (at most " +
                                                  std::to_string(observability_max_border()) + ")");
  if (m > observability_max_dim())
    return p->set_error(CALICO_UNIMPLEMENTED, "observability: reduced system of " + std::to_string(m) + " rows (at most " +
                                                  std::to_string(observability_max_dim()) + ")");
  const bool have_band = p->n_cp > 0 && p->order <= cp_covariance_max_order();
  const bool in_lds = observability_in_lds(m, mc);
  const size_t n2 = size_t(mc) * mc;
  HIP_TRY(p, ob.lam.alloc(size_t(mc) + 1)); HIP_TRY(p, ob.vec.alloc(n2 + 1)); HIP_TRY(p, ob.mat.alloc(n2 + 1));
  HIP_TRY(p, ob.dvec.alloc(size_t(mc) + 1)); HIP_TRY(p, ob.info.alloc(8));
  if (!in_lds) HIP_TRY(p, ob.work.alloc(observability_work_doubles(m, mc)));
  HIP_TRY(p, configure_observability_kernel(p->device));
  hipStream_t s = p->stream;
  rc = begin_reduced_pass(p, rp, have_band);
  if (rc != CALICO_OK) return rc;
  if (have_band) {      // (reads the band of R as the evaluation left it: ahead of the reduction)
    launch_cp_band_factor(rp.ca, s);
    HIP_TRY(p, hipGetLastError());
  }
  rc = reduce_pass(p, rp);
  if (rc != CALICO_OK) return rc;
  if (mc > 0) {
    launch_observability(sa.Spart, reduced_schur_slices(sa), m, mc, sa.R + sa.off_C(), sa.st, ob.work.p, ob.lam.p, ob.vec.p, ob.mat.p,
                         ob.dvec.p, ob.info.p, s);
    HIP_TRY(p, hipGetLastError());
  }
  double info[8] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0, in_lds ? 1.0 : 0.0, 0.0};
  double cp_info[2] = {1.0, 0.0};
  std::vector<double> lam(size_t(mc), 0.0);
  HIP_TRY(p, hipMemcpyAsync(rp.R01, p->d_R.p, sizeof(rp.R01), hipMemcpyDeviceToHost, s));
  ob.vectors.assign(n2, 0.0); ob.matrix.assign(n2, 0.0); ob.d.assign(size_t(mc), 0.0);
  if (have_band) HIP_TRY(p, hipMemcpyAsync(cp_info, rp.ca.info, sizeof(cp_info), hipMemcpyDeviceToHost, s));
  if (mc > 0) {
    HIP_TRY(p, hipMemcpyAsync(info, ob.info.p, sizeof(info), hipMemcpyDeviceToHost, s));
    HIP_TRY(p, hipMemcpyAsync(lam.data(), ob.lam.p, lam.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(p, hipMemcpyAsync(ob.vectors.data(), ob.vec.p, n2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(p, hipMemcpyAsync(ob.matrix.data(), ob.mat.p, n2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(p, hipMemcpyAsync(ob.d.data(), ob.dvec.p, size_t(mc) * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(p, hipStreamSynchronize(s));
  if (int failed = evaluation_failed(p, rp, "observability")) return failed;
  const int flags = int(info[1]), cpf = int(cp_info[1]);
  ob.min_relative_pivot_band = cp_info[0]; ob.min_relative_pivot_root = info[0];
  if (cpf & 1) return p->set_error(CALICO_FAILED_PRECONDITION, "observability: the trajectory's control-point block of JᵀJ is not finite");
  // A itself is singular: S does not exist. The band's own pivot (natural order), the tree levels' flag, the root rows' pivot
  // (checked ahead of the reduced system's values: an elimination that failed leaves non-finite ones behind).
  if ((cpf & 2) || cp_info[0] < opt->min_relative_pivot || (flags & (kInfoPivotNotPositive | kInfoEliminationFailed)) || info[0] < opt->min_relative_pivot) {
    char msg[512];
    std::snprintf(msg, sizeof(msg), "observability: the trajectory's control-point band of JᵀJ is rank deficient (minimum relative pivot %.3e of "
                  "the band, %.3e of the root rows, threshold %.3e%s): the data do not determine the trajectory, so the calibration's Schur "
                  "complement does not exist", cp_info[0], info[0], opt->min_relative_pivot,
                  (flags & kInfoEliminationFailed) ? "; a block of the control points' elimination is not positive definite" : "");
    return p->set_error(CALICO_FAILED_PRECONDITION, msg);
  }
  if (flags & kInfoNonFiniteInput) return p->set_error(CALICO_FAILED_PRECONDITION, "observability: non-finite value in the reduced system");
  if (flags & kInfoSweepLimit)
    return p->set_error(CALICO_INTERNAL, "observability: the Jacobi eigensolver did not converge in " + std::to_string(int(info[4])) + " sweeps");
  if (flags & kInfoNonFiniteResult) return p->set_error(CALICO_FAILED_PRECONDITION, "observability: non-finite value in the result");
  ob.dim = mc; ob.n_unobserved = int(info[2]); ob.kept = mc > 0 ? int(info[3]) : 0; ob.sweeps = int(info[4]); ob.rotations = int(info[5]);
  ob.in_lds = int(info[6]); ob.reduced_rows = int(info[7]);
  if (ob.kept < 0 || ob.kept > mc) return p->set_error(CALICO_INTERNAL, "observability: kept columns out of range");
  ob.eigenvalues.assign(lam.begin(), lam.begin() + ob.kept);
  ob.n_weak = 0;
  for (double v : ob.eigenvalues) ob.n_weak += v < opt->weak_threshold ? 1 : 0;
  ob.blocks = snapshot_blocks(p);
  ob.valid = true;
  return CALICO_OK;
}

namespace {
// row i of the report in the requested units: v_i, or δ_i = D⁻¹ v_i / |D⁻¹ v_i|
void observability_direction(const calico_problem::Observability& ob, int i, int tangent_units, double* out) {
  const double* v = ob.vectors.data() + size_t(i) * ob.dim;
  if (!tangent_units) { std::copy(v, v + ob.dim, out); return; }
  double nrm = 0.0;
  for (int j = 0; j < ob.dim; ++j) { out[j] = ob.d[size_t(j)] > 0.0 ? v[j] / ob.d[size_t(j)] : 0.0; nrm += out[j] * out[j]; }
  nrm = std::sqrt(nrm);
  if (nrm > 0.0) for (int j = 0; j < ob.dim; ++j) out[j] /= nrm;
}
}  // namespace

int32_t calico_observability_info(calico_problem* p, int32_t* dim, int32_t* n_unobserved, int32_t* n_weak, double* lambda_min,
                                  double* lambda_max, int32_t* sweeps) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (!observability_ready(p)) return p->set_error(CALICO_FAILED_PRECONDITION, kNoObservability);
  const calico_problem::Observability& ob = p->obs;
  if (dim) *dim = ob.dim;
  if (n_unobserved) *n_unobserved = ob.n_unobserved;
  if (n_weak) *n_weak = ob.n_weak;
  if (lambda_min) *lambda_min = ob.eigenvalues.empty() ? 0.0 : ob.eigenvalues.front();
  if (lambda_max) *lambda_max = ob.eigenvalues.empty() ? 0.0 : ob.eigenvalues.back();
  if (sweeps) *sweeps = ob.sweeps;
  return CALICO_OK;
}

int32_t calico_observability_get_spectrum(calico_problem* p, double* eigenvalues) {
  if (!p || !eigenvalues) return CALICO_INVALID_ARGUMENT;
  if (!observability_ready(p)) return p->set_error(CALICO_FAILED_PRECONDITION, kNoObservability);
  std::copy(p->obs.eigenvalues.begin(), p->obs.eigenvalues.end(), eigenvalues);
  return CALICO_OK;
}

int32_t calico_observability_get_directions(calico_problem* p, int32_t first, int32_t count, int32_t tangent_units, double* out) {
  if (!p || !out) return CALICO_INVALID_ARGUMENT;
  if (!observability_ready(p)) return p->set_error(CALICO_FAILED_PRECONDITION, kNoObservability);
  const calico_problem::Observability& ob = p->obs;
  if (first < 0 || count < 0 || first > ob.kept || count > ob.kept - first)
    return p->set_error(CALICO_INVALID_ARGUMENT, "observability: directions [" + std::to_string(first) + ", " + std::to_string(int64_t(first) + count) +
                                                     ") out of range (" + std::to_string(ob.kept) + " directions)");
  for (int i = 0; i < count; ++i) observability_direction(ob, first + i, tangent_units, out + size_t(i) * ob.dim);
  return CALICO_OK;
}

int32_t calico_observability_get_block(calico_problem* p, int32_t index, int32_t block_id, int32_t tangent_units, double* out, double* share) {
  if (!p || (!out && !share)) return CALICO_INVALID_ARGUMENT;
  const int nb = int(p->blocks.size());
  if (block_id < 0 || block_id >= nb) return p->set_error(CALICO_INVALID_ARGUMENT, "observability: unknown parameter block id");
  if (!observability_ready(p) || size_t(nb) != p->obs.blocks.size()) return p->set_error(CALICO_FAILED_PRECONDITION, kNoObservability);
  const calico_problem::Observability& ob = p->obs;
  if (index < 0 || index >= ob.kept) return p->set_error(CALICO_INVALID_ARGUMENT, "observability: direction index out of range");
  const calico_problem::BlockSnapshot& B = ob.blocks[size_t(block_id)];
  if (B.off == calico_problem::kBlockControlPoint)
    return p->set_error(CALICO_INVALID_ARGUMENT, "observability: a control point is not part of the report (the trajectory is eliminated)");
  if (out) std::fill(out, out + B.tsize, 0.0);
  if (share) *share = 0.0;
  if (B.off == calico_problem::kBlockAbsent) return CALICO_OK;      // constant / unused blocks: zeros
  if (B.off < 0 || B.off + B.tsize > ob.dim) return p->set_error(CALICO_INTERNAL, "observability: block layout out of range");
  if (out) {
    std::vector<double> dir(size_t(ob.dim));
    observability_direction(ob, index, tangent_units, dir.data());
    std::copy(dir.begin() + B.off, dir.begin() + B.off + B.tsize, out);
  }
  if (share) {
    const double* v = ob.vectors.data() + size_t(index) * ob.dim + B.off;
    double sh = 0.0;
    for (int j = 0; j < B.tsize; ++j) sh += v[j] * v[j];
    *share = sh;
  }
  return CALICO_OK;
}

int32_t calico_observability_get_matrix(calico_problem* p, double* out) {
  if (!p || !out) return CALICO_INVALID_ARGUMENT;
  if (!observability_ready(p)) return p->set_error(CALICO_FAILED_PRECONDITION, kNoObservability);
  std::copy(p->obs.matrix.begin(), p->obs.matrix.end(), out);
  return CALICO_OK;
}

// test hook (calico_hip_testing.h)
int32_t calico_debug_observability_info(calico_problem* p, double* out, int32_t n) {
  if (!p || !out || n < 0) return CALICO_INVALID_ARGUMENT;
  if (!observability_ready(p)) return p->set_error(CALICO_FAILED_PRECONDITION, kNoObservability);
  const calico_problem::Observability& ob = p->obs;
  const double v[6] = {double(ob.in_lds), double(ob.kept), double(ob.reduced_rows), double(ob.rotations), ob.min_relative_pivot_band,
                       ob.min_relative_pivot_root};
  for (int i = 0; i < n && i < 6; ++i) out[i] = v[i];
  return CALICO_OK;
}


}  // extern "C"
