// calico_hip.cpp — the C ABI of include/calico_hip.h apart from the solve and the analyses: handle lifetime, the description
// of a problem (parameter blocks, spline, rigid bodies, sensors, observations), residuals / projection, inlier mask, outlier
// tagging and heat map, communicator, shard, stream and phase timing; and the loader of RCCL.
//
// What the reference does per Optimize() call (batch_optimizer.cpp:53-81) —
// build a ceres::Problem from the sensors / world model / trajectory, run
// ceres::Solve, re-evaluate the residual blocks — maps here to:
//   add_* calls  -> host-side block / observation tables (this file),
//   finalize()   -> cells, work items, gather lists, device upload (plan.cpp),
//   calico_solve -> device-resident LM (solve.cpp; kernels in eval_kernels.hip, solve_kernels.hip and bcr_kernels.hip),
//   calico_get_residuals -> cost-only kernel without the loss function (this file).
// What is read from a solved problem (covariance, prediction covariance, observability) is analysis.cpp; the handle and
// what the host files share is problem_host.hpp.
// There is no CPU compute path in this library.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>     // types only: the library itself is loaded on first use (rccl() below)
#include <dlfcn.h>
#include <link.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/calico_hip.h"
#include "calico_hip_testing.h"
#include "kernels.hpp"
#include "problem_dev.hpp"
#include "problem_host.hpp"

namespace {

int camera_num_params(int model) {
  switch (model) { case 1: return 8; case 2: return 11; case 3: return 7; case 4: return 5; case 5: return 4; case 6: return 4;
    case 7: return 5; default: return -1; }
}
int imu_num_params(int model) { return model == 1 ? 1 : (model == 2 ? 4 : (model == 3 ? 12 : -1)); }

struct StreamPool {
  std::mutex mu;
  std::map<int, std::vector<hipStream_t>> idle;     // per device: streams of destroyed handles
  static constexpr size_t kMaxIdle = 4;
};
StreamPool& stream_pool() { static StreamPool* sp = new StreamPool(); return *sp; }     // (never destroyed: the streams outlive static destruction)

// Residuals of ALL residual blocks at d_x, without the loss function (camera.cpp:70-80), into d_res / d_valid: every rank
// re-evaluates all blocks here. `predict`: the predictions instead (calico_project).
void launch_all_blocks(calico_problem* p, bool predict) {
  EvalArgs ea = make_eval_args(p, p->d_x.p, 0, true);
  ea.items = p->d_items_all.p; ea.n_items = p->n_items_all;
  ea.project = predict ? 1 : 0;
  launch_eval(ea, false, p->stream);
}
// ... at the handle's current parameter values: plan, device, values, launch. (A caller that returns between the upload and the
// launch, or that needs the plan before it knows whether to evaluate, spells the first three out.)
int evaluate_all_blocks(calico_problem* p, bool predict) {
  if (int rc = finalize(p)) return rc;
  HIP_TRY(p, hipSetDevice(p->device));
  if (int rc = upload_x(p)) return rc;
  launch_all_blocks(p, predict);
  return CALICO_OK;
}

}  // namespace

// ---- what the other host files call as well (declared in problem_host.hpp) ----
namespace cal {

// RCCL is loaded when the first communicator is asked for (calico_comm_get_unique_id / calico_comm_init_rccl), not at
// link time: a single-GPU user needs no librccl on the machine. An already loaded librccl (e.g. the one torch ships) is
// found by its soname; otherwise $ROCM_PATH/lib, then the loader's search path.
RcclApi& rccl() {
  static RcclApi api = [] {
    RcclApi a;
    std::vector<std::string> names;
    if (const char* one = std::getenv("CALICO_RCCL_LIB")) names.push_back(one);      // this library and no other (a particular RCCL build)
    else {
      names = {"librccl.so.1", "librccl.so"};
      for (const char* env : {"ROCM_PATH", "ROCM_HOME"})
        if (const char* r = std::getenv(env)) { names.push_back(std::string(r) + "/lib/librccl.so.1"); names.push_back(std::string(r) + "/lib/librccl.so"); }
      names.push_back("/opt/rocm/lib/librccl.so.1"); names.push_back("/opt/rocm/lib/librccl.so");
    }
    std::string why;
    // An RCCL the process already holds (PyTorch brings its own librccl.so) is the one to use: two copies in one process
    // end in a double free at exit. And a copy this library loads stays private to it (RTLD_LOCAL: the entry points are
    // taken with dlsym) -- loaded globally before PyTorch, its symbols would interpose on the ones PyTorch's own copy
    // expects to bind.
    for (const std::string& n : names) {
      a.lib = dlopen(n.c_str(), RTLD_NOW | RTLD_NOLOAD);
      if (a.lib) break;
    }
    for (const std::string& n : names) {
      if (a.lib) break;
      a.lib = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
      if (a.lib) break;
      const char* e = dlerror();         // (dlerror() clears its state: one call per failure)
      if (e) why = e;
    }
    if (!a.lib) { a.error = "librccl not found: " + why; return a; }
    auto sym = [&](const char* n) { void* f = dlsym(a.lib, n); if (!f && a.error.empty()) a.error = std::string("librccl lacks ") + n; return f; };
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(sym("ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(sym("ncclCommInitRank"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(sym("ncclCommDestroy"));
    a.CommCount = reinterpret_cast<decltype(a.CommCount)>(sym("ncclCommCount"));
    a.AllReduce = reinterpret_cast<decltype(a.AllReduce)>(sym("ncclAllReduce"));
    a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(sym("ncclGetErrorString"));
    if (!a.error.empty()) { dlclose(a.lib); a.lib = nullptr; }
    return a;
  }();
  return api;
}

int require_exchange(calico_problem* p) {
  if (p->world > 1 && !p->has_exchange())
    return p->set_error(CALICO_FAILED_PRECONDITION, "calico_problem_set_shard(world > 1) needs an exchange: calico_comm_init_rccl or calico_problem_set_allreduce");
  return CALICO_OK;
}

// bspline.hpp:138-150
int spline_index(const calico_problem* p, double t) {
  const std::vector<double>& vk = p->valid_knots;
  if (t == vk.back()) return int(vk.size()) - 2;
  if (!(t < vk.back())) return -1;
  // upper_bound(vk, t) - 1, found from a guess on the (uniform) knot spacing and corrected by comparisons with the knots
  // themselves, so the result is the binary search's for any knot vector
  const int n = int(vk.size());
  if (t < vk.front()) return -1;
  const double dt = (vk.back() - vk.front()) / double(n - 1);
  int i = dt > 0.0 ? int((t - vk.front()) / dt) : 0;
  i = std::max(0, std::min(n - 2, i));
  while (i > 0 && t < vk[size_t(i)]) --i;
  while (i + 1 < n && !(t < vk[size_t(i) + 1])) ++i;
  return i;
}
std::string& handle_free_error() { static thread_local std::string e; return e; }      // (free_call.hpp: its writers)

}  // namespace cal

extern "C" {

int32_t calico_problem_create(calico_problem** out, int32_t device) {
  if (!out) return CALICO_INVALID_ARGUMENT;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return CALICO_INTERNAL;
  if (hipSetDevice(device) != hipSuccess) return CALICO_INTERNAL;
  calico_problem* p = new calico_problem();
  p->device = device;
  // (a stream costs a few hundred microseconds to create: the handles of a create-solve-destroy loop pass theirs on)
  {
    StreamPool& sp = stream_pool();
    std::lock_guard<std::mutex> lock(sp.mu);
    std::vector<hipStream_t>& v = sp.idle[device];
    if (!v.empty()) { p->stream = v.back(); v.pop_back(); }
  }
  if (!p->stream && hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess) { delete p; return CALICO_INTERNAL; }
  p->own_stream = true;
  *out = p;
  return CALICO_OK;
}

void calico_problem_destroy(calico_problem* p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  // first drain the stream -- the iterations enqueued ahead of a terminated multi-rank solve each still carry an
  // all-reduce --, then give the communicator back
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  if (p->comm) { (void)rccl().CommDestroy(p->comm); p->comm = nullptr; }
  // the workspace stays with the cached plan: the next handle of this structure takes it over instead of allocating
  return_workspace(p);
  release_measurement_staging(p);      // (only set if a finalize failed half-way)
  if (p->own_stream && p->stream) {      // (drained above)
    StreamPool& sp = stream_pool();
    std::lock_guard<std::mutex> lock(sp.mu);
    std::vector<hipStream_t>& v = sp.idle[p->device];
    if (v.size() < StreamPool::kMaxIdle) v.push_back(p->stream); else (void)hipStreamDestroy(p->stream);
  }
  {
    DeviceArena::Batch batch(p->device);     // what the handle owns goes back to the arena behind ONE wait for its device
    delete p;
  }
  // Idle slabs beyond a few go back to the driver -- lazily: hipFree waits for the whole device (other handles' streams,
  // PyTorch's), and a create / solve / destroy loop over a problem of several slabs would hipMalloc them again every cycle.
  // CALICO_ARENA_KEEP_SLABS (default 4 = 256 MB per device) idle slabs stay; calico_plan_cache_clear() frees them all.
  static const int keep_slabs = env_int("CALICO_ARENA_KEEP_SLABS", 4, 0);
  DeviceArena::get().trim(keep_slabs);
}

int32_t calico_plan_cache_stats(int64_t* hits, int64_t* misses, int64_t* entries) { plan_cache_stats(hits, misses, entries); return CALICO_OK; }
int32_t calico_plan_cache_clear(void) { plan_cache_clear(); return CALICO_OK; }

const char* calico_last_error(const calico_problem* p) {
  if (p) return p->error.c_str();
  return handle_free_error().empty() ? "null problem" : handle_free_error().c_str();
}

void calico_default_solver_options(calico_solver_options* o) {
  // DefaultSolverOptions() (batch_optimizer.cpp:10-17) over Ceres' Solver::Options defaults.
  o->max_num_iterations = 50; o->num_threads = 1; o->minimizer_progress_to_stdout = 1; o->jacobi_scaling = 1;
  o->max_num_consecutive_invalid_steps = 5; o->sync_every = 1;
  o->function_tolerance = 1e-8; o->gradient_tolerance = 1e-10; o->parameter_tolerance = 1e-10;
  o->initial_trust_region_radius = 1e4; o->max_trust_region_radius = 1e16; o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3; o->min_lm_diagonal = 1e-6; o->max_lm_diagonal = 1e32;
}

int32_t calico_problem_add_param_block(calico_problem* p, const double* values, int32_t size, int32_t manifold,
                                       int32_t is_constant, int32_t* block_id_out) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (size <= 0 || !values) return p->set_error(CALICO_INVALID_ARGUMENT, "bad parameter block");
  if (manifold == CALICO_MANIFOLD_EIGEN_QUATERNION && size != 4)
    return p->set_error(CALICO_INVALID_ARGUMENT, "quaternion manifold needs size 4");
  if (manifold != CALICO_MANIFOLD_EUCLIDEAN && manifold != CALICO_MANIFOLD_EIGEN_QUATERNION)
    return p->set_error(CALICO_INVALID_ARGUMENT, "unknown manifold");
  HBlock b; b.v.assign(values, values + size); b.size = size; b.manifold = manifold; b.constant = is_constant != 0;
  p->blocks.push_back(b);
  p->dirty = true;
  if (block_id_out) *block_id_out = int32_t(p->blocks.size()) - 1;
  return CALICO_OK;
}

int32_t calico_problem_add_param_blocks(calico_problem* p, int32_t n, int32_t size, int32_t manifold, const uint8_t* is_constant,
                                        const double* values, int32_t* block_ids_out) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (n < 0 || size <= 0 || (n > 0 && !values)) return p->set_error(CALICO_INVALID_ARGUMENT, "bad parameter blocks");
  if (manifold == CALICO_MANIFOLD_EIGEN_QUATERNION && size != 4)
    return p->set_error(CALICO_INVALID_ARGUMENT, "quaternion manifold needs size 4");
  if (manifold != CALICO_MANIFOLD_EUCLIDEAN && manifold != CALICO_MANIFOLD_EIGEN_QUATERNION)
    return p->set_error(CALICO_INVALID_ARGUMENT, "unknown manifold");
  p->blocks.reserve(p->blocks.size() + size_t(n));
  for (int i = 0; i < n; ++i) {
    HBlock b; b.v.assign(values + size_t(i) * size, values + size_t(i + 1) * size); b.size = size; b.manifold = manifold;
    b.constant = is_constant && is_constant[i] != 0;
    p->blocks.push_back(std::move(b));
    if (block_ids_out) block_ids_out[i] = int32_t(p->blocks.size()) - 1;
  }
  p->dirty = true;
  return CALICO_OK;
}

int32_t calico_get_param_block(calico_problem* p, int32_t id, double* out) {
  if (!p || id < 0 || id >= int(p->blocks.size()) || !out) return p ? p->set_error(CALICO_INVALID_ARGUMENT, "bad block id") : CALICO_INVALID_ARGUMENT;
  std::copy(p->blocks[id].v.begin(), p->blocks[id].v.end(), out);
  return CALICO_OK;
}

int32_t calico_set_param_block(calico_problem* p, int32_t id, const double* v) {
  if (!p || id < 0 || id >= int(p->blocks.size()) || !v) return p ? p->set_error(CALICO_INVALID_ARGUMENT, "bad block id") : CALICO_INVALID_ARGUMENT;
  std::copy(v, v + p->blocks[id].size, p->blocks[id].v.begin());
  if (p->blocks[id].constant || !p->blocks[id].used) p->xc_stale = true;   // the update kernel never rewrites these
  p->step_ready = false;
  return CALICO_OK;
}

int32_t calico_get_param_blocks(calico_problem* p, int32_t n, const int32_t* ids, double* out) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (n < 0 || (n > 0 && (!ids || !out))) return p->set_error(CALICO_INVALID_ARGUMENT, "bad block list");
  for (int32_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= int(p->blocks.size())) return p->set_error(CALICO_INVALID_ARGUMENT, "bad block id");
  for (int32_t i = 0; i < n; ++i) {
    const HBlock& b = p->blocks[size_t(ids[i])];
    std::copy(b.v.begin(), b.v.end(), out);
    out += b.size;
  }
  return CALICO_OK;
}

int32_t calico_set_param_blocks(calico_problem* p, int32_t n, const int32_t* ids, const double* v) {
  if (!p || n < 0 || (n > 0 && (!ids || !v))) return p ? p->set_error(CALICO_INVALID_ARGUMENT, "bad arguments") : CALICO_INVALID_ARGUMENT;
  for (int i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= int(p->blocks.size())) return p->set_error(CALICO_INVALID_ARGUMENT, "bad block id");
  for (int i = 0; i < n; ++i) {
    HBlock& b = p->blocks[ids[i]];
    std::copy(v, v + b.size, b.v.begin());
    v += b.size;
    if (b.constant || !b.used) p->xc_stale = true;
  }
  if (n > 0) p->step_ready = false;
  return CALICO_OK;
}

int32_t calico_problem_set_spline(calico_problem* p, int32_t order, int32_t n_knots, const double* knots,
                                  const double* basis, const int32_t* ctrl) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (order < 2 || order > 16 || n_knots < 2 * order || !knots || !basis || !ctrl)
    return p->set_error(CALICO_INVALID_ARGUMENT, "bad spline");
  const int deg = order - 1;
  for (int i = 0; i < n_knots - order; ++i)
    if (ctrl[i] < 0 || ctrl[i] >= int(p->blocks.size()) || p->blocks[ctrl[i]].size != 6)
      return p->set_error(CALICO_INVALID_ARGUMENT, "control point blocks must be 6-vectors");
  p->order = order;
  p->knots.assign(knots, knots + n_knots);
  p->valid_knots.assign(knots + deg, knots + n_knots - deg);
  const int nseg = int(p->valid_knots.size()) - 1;
  p->basis.assign(basis, basis + size_t(nseg) * order * order);
  p->ctrl.assign(ctrl, ctrl + (n_knots - order));
  p->dirty = true;
  return CALICO_OK;
}

int32_t calico_problem_add_rigid_body(calico_problem* p, int32_t q, int32_t t, int32_t* id_out) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  const int nb = int(p->blocks.size());
  if (q < 0 || q >= nb || t < 0 || t >= nb || p->blocks[q].size != 4 || p->blocks[t].size != 3)
    return p->set_error(CALICO_INVALID_ARGUMENT, "rigid body pose blocks must be a quaternion and a 3-vector");
  p->bodies.push_back({q, t});
  p->dirty = true;
  if (id_out) *id_out = int32_t(p->bodies.size()) - 1;
  return CALICO_OK;
}

int32_t calico_problem_add_sensor(calico_problem* p, int32_t kind, int32_t model, int32_t intr, int32_t q, int32_t t,
                                  int32_t lat, int32_t grav, double sigma, int32_t loss, double loss_scale,
                                  int32_t* id_out) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (kind < 0 || kind > 2) return p->set_error(CALICO_INVALID_ARGUMENT, "unknown sensor kind");
  const int K = kind == CALICO_SENSOR_CAMERA ? camera_num_params(model) : imu_num_params(model);
  // camera.cpp:94-97 / gyroscope.cpp:12-15: model not set -> FailedPrecondition
  if (K < 0) return p->set_error(CALICO_FAILED_PRECONDITION, "Cannot add sensor parameters. Sensor model is not yet defined.");
  const int nb = int(p->blocks.size());
  auto ok = [&](int id, int size) { return id >= 0 && id < nb && p->blocks[id].size == size; };
  if (!ok(intr, K)) return p->set_error(CALICO_INVALID_ARGUMENT, "intrinsics block size does not match the model");
  if (!ok(q, 4) || !ok(t, 3) || !ok(lat, 1)) return p->set_error(CALICO_INVALID_ARGUMENT, "bad extrinsics / latency blocks");
  if (kind == CALICO_SENSOR_ACCELEROMETER && !ok(grav, 3)) return p->set_error(CALICO_INVALID_ARGUMENT, "bad gravity block");
  if (loss < 0 || loss > 2) return p->set_error(CALICO_INVALID_ARGUMENT, "unknown loss function");
  HSensor s; s.kind = kind; s.model = model; s.K = K; s.intr = intr; s.q = q; s.t = t; s.lat = lat;
  s.grav = kind == CALICO_SENSOR_ACCELEROMETER ? grav : -1;
  s.sigma = sigma; s.info = sigma > 0.0 ? 1.0 / sigma : 1.0;  // camera_cost_functor.cpp:15 (Q9)
  s.loss = loss; s.loss_scale = loss_scale;
  p->sensors.push_back(s);
  p->dirty = true;
  if (id_out) *id_out = int32_t(p->sensors.size()) - 1;
  return CALICO_OK;
}

static int32_t add_obs(calico_problem* p, int32_t sid, int64_t n, const double* meas, const double* stamps,
                       const int32_t* body, const int32_t* point) {
  if (sid < 0 || sid >= int(p->sensors.size())) return p->set_error(CALICO_INVALID_ARGUMENT, "bad sensor id");
  if (p->order <= 0) return p->set_error(CALICO_FAILED_PRECONDITION, "spline must be set before residuals");
  if (n < 0 || (n > 0 && (!meas || !stamps))) return p->set_error(CALICO_INVALID_ARGUMENT, "bad observation arrays");
  HSensor& s = p->sensors[sid];
  const int dim = s.dim();
  // validate first so a failing call adds nothing
  std::vector<int> segs(static_cast<size_t>(n));
  double last_t = 0.0;
  int last_sg = -2;       // (the blocks of a camera frame share their stamp: one knot search per frame)
  for (int64_t i = 0; i < n; ++i) {
    const int sg = (last_sg != -2 && stamps[i] == last_t) ? last_sg : spline_index(p, stamps[i]);
    last_t = stamps[i]; last_sg = sg;
    if (sg < 0)
      return p->set_error(CALICO_INVALID_ARGUMENT, "measurement stamp is outside the spline's valid knots");
    segs[size_t(i)] = sg;
    if (body) {
      // camera.cpp:126-131
      if (body[i] < 0 || body[i] >= int(p->bodies.size()))
        return p->set_error(CALICO_FAILED_PRECONDITION,
                            "Attempted to create cost function from an observation for a rigidbody that does not exist in the world model.");
      if (point[i] < 0 || point[i] >= int(p->blocks.size()) || p->blocks[point[i]].size != 3)
        return p->set_error(CALICO_INVALID_ARGUMENT, "model point block must be a 3-vector");
    }
  }
  s.seg.insert(s.seg.end(), segs.begin(), segs.end());
  s.stamps.insert(s.stamps.end(), stamps, stamps + n);
  if (body) { s.body.insert(s.body.end(), body, body + n); s.point.insert(s.point.end(), point, point + n); }
  s.meas.insert(s.meas.end(), meas, meas + n * dim);
  s.active.insert(s.active.end(), size_t(n), uint8_t(1));
  s.n_active = -1;
  p->dirty = true;
  return CALICO_OK;
}

int32_t calico_problem_add_camera_residuals(calico_problem* p, int32_t sid, int64_t n, const double* px, const double* st,
                                            const int32_t* body, const int32_t* point) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (sid >= 0 && sid < int(p->sensors.size()) && p->sensors[sid].kind != CALICO_SENSOR_CAMERA)
    return p->set_error(CALICO_INVALID_ARGUMENT, "sensor is not a camera");
  if (n > 0 && (!body || !point)) return p->set_error(CALICO_INVALID_ARGUMENT, "bad observation arrays");
  return add_obs(p, sid, n, px, st, body, point);
}

int32_t calico_problem_add_imu_residuals(calico_problem* p, int32_t sid, int64_t n, const double* m, const double* st) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (sid >= 0 && sid < int(p->sensors.size()) && p->sensors[sid].kind == CALICO_SENSOR_CAMERA)
    return p->set_error(CALICO_INVALID_ARGUMENT, "sensor is not an IMU sensor");
  return add_obs(p, sid, n, m, st, nullptr, nullptr);
}

int32_t calico_debug_roll_table(int32_t spline_order, int32_t lane, uint32_t* out48) {
  if (!out48 || spline_order < 1 || spline_order > 6 || lane < 0 || lane > 63) return CALICO_INVALID_ARGUMENT;
  cal::roll_table_row(spline_order, lane, out48);
  return CALICO_OK;
}

int64_t calico_debug_lds_attribute_calls(void) { return cal::lds_attribute_calls(); }

int32_t calico_debug_panel_product(int32_t device, int32_t form, const double* w, const double* x, double* out) {
  if ((form != 0 && form != 1) || !w || !x || !out) return CALICO_INVALID_ARGUMENT;
  if (hipSetDevice(device) != hipSuccess) return CALICO_INTERNAL;
  cal::DevBuf<double> d_w, d_x, d_out;
  if (d_w.upload(std::vector<double>(w, w + 64), nullptr) != hipSuccess || d_x.upload(std::vector<double>(x, x + 64), nullptr) != hipSuccess ||
      d_out.alloc(64) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)      // (the uploads' sources are temporaries)
    return CALICO_INTERNAL;
  if (cal::launch_debug_panel_product(form, d_w.p, d_x.p, d_out.p, nullptr) != hipSuccess ||
      hipMemcpy(out, d_out.p, 64 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return CALICO_INTERNAL;
  return CALICO_OK;
}

int32_t calico_debug_block_elim(int32_t device, int32_t n_row_tiles, const double* D, const double* X, double* L_out, double* Z_out,
                                double* Minv_out) {
  if (n_row_tiles < 1 || n_row_tiles > cal::debug_block_elim_max_tiles() || !D || !X || !L_out || !Z_out || !Minv_out) return CALICO_INVALID_ARGUMENT;
  if (hipSetDevice(device) != hipSuccess) return CALICO_INTERNAL;
  const size_t nx = size_t(16) * size_t(n_row_tiles) * 32;
  cal::DevBuf<double> d_D, d_X, d_L, d_Z, d_M;
  if (d_D.upload(std::vector<double>(D, D + 1024), nullptr) != hipSuccess || d_X.upload(std::vector<double>(X, X + nx), nullptr) != hipSuccess ||
      d_L.alloc(1024) != hipSuccess || d_Z.alloc(nx) != hipSuccess || d_M.alloc(1024) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess)
    return CALICO_INTERNAL;
  if (cal::launch_debug_block_elim(n_row_tiles, d_D.p, d_X.p, d_L.p, d_Z.p, d_M.p, nullptr) != hipSuccess ||
      hipMemcpy(L_out, d_L.p, 1024 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(Z_out, d_Z.p, nx * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(Minv_out, d_M.p, 1024 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return CALICO_INTERNAL;
  return CALICO_OK;
}

int32_t calico_get_iterations(calico_problem* p, calico_iteration* out, int32_t max_rows, int32_t* n_out) {
  if (!p || !out || !n_out) return CALICO_INVALID_ARGUMENT;
  const int n = std::min<int>(max_rows, int(p->iterations.size()));
  for (int i = 0; i < n; ++i) out[i] = p->iterations[size_t(i)];
  *n_out = n;
  return CALICO_OK;
}

static int32_t residuals_or_prediction(calico_problem* p, int32_t sid, double* out, uint8_t* valid, bool predict) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (sid < 0 || sid >= int(p->sensors.size())) return p->set_error(CALICO_INVALID_ARGUMENT, "bad sensor id");
  if (p->sensors[size_t(sid)].n() == 0) return CALICO_OK;   // a sensor without measurements has nothing to report
  if (!out) return p->set_error(CALICO_INVALID_ARGUMENT, "null output buffer");
  int rc = finalize(p);
  if (rc != CALICO_OK) return rc;
  HIP_TRY(p, hipSetDevice(p->device));
  // one evaluation and one download serve every sensor as long as no parameter value, measurement or tag has changed
  calico_problem::ResCache& rc_ = p->res_cache;
  std::vector<double> xnow(size_t(p->n_amb), 0.0);
  for (const HBlock& b : p->blocks) std::copy(b.v.begin(), b.v.end(), xnow.begin() + b.amb_off);
  if (!(rc_.valid && rc_.predict == predict && !p->active_dirty && rc_.x == xnow)) {
    rc_.valid = false;
    rc = upload_x(p);
    if (rc != CALICO_OK) return rc;
    launch_all_blocks(p, predict);
    rc_.r.resize(size_t(p->n_obs) * 3);
    rc_.v.resize(size_t(p->n_obs));
    HIP_TRY(p, hipMemcpyAsync(rc_.r.data(), p->d_res.p, rc_.r.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(p, hipMemcpyAsync(rc_.v.data(), p->d_valid.p, rc_.v.size(), hipMemcpyDeviceToHost, p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    rc_.x.swap(xnow); rc_.predict = predict; rc_.valid = true;
  }
  const std::vector<double>& r = rc_.r;
  const std::vector<uint8_t>& v = rc_.v;
  const HSensor& s = p->sensors[sid];
  const int dim = s.dim();
  bool all = true;
  for (int64_t i = 0; i < s.n(); ++i) {
    const int64_t q = s.sorted_pos[size_t(i)];
    for (int c = 0; c < dim; ++c) out[i * dim + c] = v[size_t(q)] ? r[size_t(q) * 3 + c] : 0.0;
    if (valid) valid[i] = v[size_t(q)];
    if (!v[size_t(q)] && s.active[size_t(i)]) all = false;     // tagged outliers have no residual and are no failure
  }
  // camera.cpp:73-76: a failing block makes UpdateResiduals return kInternal; Project just skips such points
  // (camera.cpp:172-174), here they come back with valid = 0
  if (predict) return CALICO_OK;
  return all ? CALICO_OK : p->set_error(CALICO_INTERNAL, "Failed to update residual");
}

int32_t calico_get_residuals(calico_problem* p, int32_t sid, double* out, uint8_t* valid) {
  return residuals_or_prediction(p, sid, out, valid, false);
}

int32_t calico_project(calico_problem* p, int32_t sid, double* out, uint8_t* valid) {
  return residuals_or_prediction(p, sid, out, valid, true);
}

int32_t calico_get_inlier_mask(calico_problem* p, int32_t sid, double threshold, uint8_t* mask) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (sid < 0 || sid >= int(p->sensors.size()) || !mask) return p->set_error(CALICO_INVALID_ARGUMENT, "bad sensor id");
  if (int rc = finalize(p)) return rc;
  HIP_TRY(p, hipSetDevice(p->device));
  if (int rc = upload_x(p)) return rc;
  const HSensor& s = p->sensors[sid];
  if (s.n() == 0) return CALICO_OK;
  launch_all_blocks(p, false);
  // the test runs on the device; one byte per observation comes back (a block that failed to evaluate, or one tagged
  // as an outlier, is no inlier)
  launch_inlier_mask(p->d_res.p, p->d_valid.p, p->d_active.p, int(s.sorted_begin), int(s.sorted_end), s.dim(), threshold, p->stream);
  const int64_t nrange = std::max<int64_t>(0, s.sorted_end - s.sorted_begin);
  std::vector<uint8_t> m(size_t(std::max<int64_t>(nrange, 1)));
  if (nrange > 0) HIP_TRY(p, hipMemcpyAsync(m.data(), p->d_valid.p + s.sorted_begin, size_t(nrange), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(p, hipStreamSynchronize(p->stream));
  for (int64_t i = 0; i < s.n(); ++i) mask[i] = m[size_t(s.sorted_pos[size_t(i)] - s.sorted_begin)];
  return CALICO_OK;
}

int32_t calico_problem_set_outlier_mask(calico_problem* p, int32_t sid, const uint8_t* is_outlier) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (sid < 0 || sid >= int(p->sensors.size())) return p->set_error(CALICO_INVALID_ARGUMENT, "bad sensor id");
  HSensor& s = p->sensors[sid];
  for (int64_t i = 0; i < s.n(); ++i) s.active[size_t(i)] = (is_outlier && is_outlier[i]) ? 0 : 1;
  s.n_active = -1;
  p->active_dirty = true;
  p->res_cache.valid = false;
  return CALICO_OK;
}

int32_t calico_mark_outliers(calico_problem* p, int32_t sid, double threshold, int64_t* n_marked) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (sid < 0 || sid >= int(p->sensors.size())) return p->set_error(CALICO_INVALID_ARGUMENT, "bad sensor id");
  if (int rc = evaluate_all_blocks(p, false)) return rc;
  HSensor& s = p->sensors[sid];
  HIP_TRY(p, hipMemsetAsync(p->d_counter.p, 0, sizeof(int), p->stream));
  launch_mark_outliers(p->d_res.p, p->d_valid.p, p->d_active.p, int(s.sorted_begin), int(s.sorted_end), s.dim(), threshold,
                       p->d_counter.p, p->stream);
  // mirror the tags on the host (they decide counts and survive a re-finalisation)
  const int64_t nrange = std::max<int64_t>(0, s.sorted_end - s.sorted_begin);
  std::vector<uint8_t> act(size_t(std::max<int64_t>(nrange, 1)));
  int marked = 0;
  if (nrange > 0) HIP_TRY(p, hipMemcpyAsync(act.data(), p->d_active.p + s.sorted_begin, size_t(nrange), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(p, hipMemcpyAsync(&marked, p->d_counter.p, sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(p, hipStreamSynchronize(p->stream));
  for (int64_t i = 0; i < s.n(); ++i) s.active[size_t(i)] = act[size_t(s.sorted_pos[size_t(i)] - s.sorted_begin)];
  s.n_active = -1;
  p->res_cache.valid = false;
  if (marked > 0) p->any_tagged = true;
  if (n_marked) *n_marked = marked;
  return CALICO_OK;
}

int32_t calico_residual_heatmap(calico_problem* p, int32_t sid, int32_t image_width, int32_t image_height, int32_t num_rows,
                                int32_t num_cols, double* rmse_out, int64_t* count_out) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (sid < 0 || sid >= int(p->sensors.size())) return p->set_error(CALICO_INVALID_ARGUMENT, "bad sensor id");
  if (p->sensors[size_t(sid)].kind != CALICO_SENSOR_CAMERA) return p->set_error(CALICO_INVALID_ARGUMENT, "not a camera");
  if (image_width <= 0 || image_height <= 0 || num_rows <= 0 || num_cols <= 0 || !rmse_out || !count_out)
    return p->set_error(CALICO_INVALID_ARGUMENT, "bad heat-map dimensions");
  if (int rc = evaluate_all_blocks(p, false)) return rc;
  const HSensor& s = p->sensors[size_t(sid)];
  const size_t nb = size_t(num_rows) * num_cols;
  DevBuf<double> d_rmse; DevBuf<long long> d_cnt;
  HIP_TRY(p, d_rmse.alloc(nb)); HIP_TRY(p, d_cnt.alloc(nb));
  launch_residual_heatmap(p->d_res.p, p->d_valid.p, p->d_active.p, p->d_m0.p, p->d_m1.p, int(std::min(s.sorted_begin, s.sorted_end)),
                          int(s.sorted_end), image_width, image_height, num_rows, num_cols, d_rmse.p, d_cnt.p, p->stream);
  std::vector<long long> cnt(nb);
  HIP_TRY(p, hipMemcpyAsync(rmse_out, d_rmse.p, nb * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(p, hipMemcpyAsync(cnt.data(), d_cnt.p, nb * sizeof(long long), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(p, hipStreamSynchronize(p->stream));
  for (size_t i = 0; i < nb; ++i) count_out[i] = int64_t(cnt[i]);
  return CALICO_OK;
}

int32_t calico_num_effective_parameters(calico_problem* p, int32_t* n_out) {
  if (!p || !n_out) return CALICO_INVALID_ARGUMENT;
  const int rc = finalize(p);
  if (rc != CALICO_OK) return rc;
  *n_out = p->n_eff;
  return CALICO_OK;
}

int32_t calico_problem_set_allreduce(calico_problem* p, calico_allreduce_fn fn, void* ctx) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  p->allreduce = fn; p->allreduce_ctx = ctx;
  return CALICO_OK;
}

int32_t calico_problem_finalize(calico_problem* p) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  const int rc = finalize(p);
  if (rc != CALICO_OK) return rc;
  return upload_x(p) == CALICO_OK && hipStreamSynchronize(p->stream) == hipSuccess ? CALICO_OK : CALICO_INTERNAL;
}

int32_t calico_comm_get_unique_id(uint8_t* id_out) {
  if (!id_out) return CALICO_INVALID_ARGUMENT;
  static_assert(sizeof(ncclUniqueId) == CALICO_COMM_ID_BYTES, "RCCL unique id size");
  ncclUniqueId id;
  if (!rccl().ok() || rccl().GetUniqueId(&id) != ncclSuccess) return CALICO_INTERNAL;
  std::memcpy(id_out, &id, sizeof(id));
  return CALICO_OK;
}

// How many distinct librccl images the process holds. More than one means this library loaded its private copy BEFORE the
// application brought its own (PyTorch imported after the first communicator call): both copies work, but two RCCLs in one
// process have ended in a double free at exit. The load order that avoids it -- the application's RCCL first -- is documented
// in include/calico_hip.h; here the situation is detected and said out loud, once.
static int rccl_images_loaded() {
  std::vector<std::string> seen;
  dl_iterate_phdr([](struct dl_phdr_info* info, size_t, void* data) {
    auto* v = static_cast<std::vector<std::string>*>(data);
    const std::string n = info->dlpi_name ? info->dlpi_name : "";
    const size_t slash = n.rfind('/');
    if (n.compare(slash == std::string::npos ? 0 : slash + 1, 7, "librccl") == 0 && std::find(v->begin(), v->end(), n) == v->end()) v->push_back(n);
    return 0;
  }, &seen);
  return int(seen.size());
}

int32_t calico_comm_init_rccl(calico_problem* p, const uint8_t* id, int32_t rank, int32_t world_size) {
  if (!p || !id) return CALICO_INVALID_ARGUMENT;
  if (world_size < 1 || rank < 0 || rank >= world_size) return p->set_error(CALICO_INVALID_ARGUMENT, "bad rank / world size");
  if (!rccl().ok()) return p->set_error(CALICO_INTERNAL, rccl().error);
  if (rccl_images_loaded() > 1) {
    static std::atomic<bool> said{false};
    if (!said.exchange(true))
      std::fprintf(stderr, "[calico] warning: two librccl images are loaded in this process (this library loaded its own before the "
                           "application's -- e.g. torch was imported after the first calico_comm_* call). Load the application's RCCL "
                           "first, or point CALICO_RCCL_LIB at the same file.\n");
  }
  HIP_TRY(p, hipSetDevice(p->device));
  if (p->comm) { if (p->stream) (void)hipStreamSynchronize(p->stream); (void)rccl().CommDestroy(p->comm); p->comm = nullptr; }
  ncclUniqueId uid;
  std::memcpy(&uid, id, sizeof(uid));
  const ncclResult_t r = rccl().CommInitRank(&p->comm, world_size, uid, rank);
  if (r != ncclSuccess) { p->comm = nullptr; return p->set_error(CALICO_INTERNAL, std::string("ncclCommInitRank: ") + rccl().GetErrorString(r)); }
  p->rank = rank; p->world = world_size; p->dirty = true;
  return CALICO_OK;
}

int32_t calico_comm_info(calico_problem* p, int32_t* rank_out, int32_t* world_out, int64_t* local_blocks_out, int64_t* total_blocks_out) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  int world = p->world;
  if (p->comm) {      // what the communicator itself says, not what the caller asked for
    if (rccl().CommCount(p->comm, &world) != ncclSuccess) return p->set_error(CALICO_INTERNAL, "ncclCommCount failed");
  }
  const int rc = finalize(p);
  if (rc != CALICO_OK) return rc;
  if (rank_out) *rank_out = p->rank;
  if (world_out) *world_out = world;
  if (local_blocks_out) *local_blocks_out = p->n_obs_local;
  if (total_blocks_out) *total_blocks_out = p->n_obs;       // (the work items of all ranks cover every residual block once)
  return CALICO_OK;
}

int32_t calico_problem_set_shard(calico_problem* p, int32_t rank, int32_t world_size) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (world_size < 1 || rank < 0 || rank >= world_size) return p->set_error(CALICO_INVALID_ARGUMENT, "bad rank / world size");
  p->rank = rank; p->world = world_size; p->dirty = true;
  return CALICO_OK;
}

int32_t calico_problem_set_stream(calico_problem* p, void* stream) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (p->stream) (void)hipStreamSynchronize(p->stream);
  if (p->own_stream && p->stream) (void)hipStreamDestroy(p->stream);
  p->stream = reinterpret_cast<hipStream_t>(stream);
  p->own_stream = false;
  return CALICO_OK;
}

int32_t calico_set_phase_timing(calico_problem* p, int32_t mask) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  // the phase times accumulate from this call on, over as many solves as follow
  if (!p->timer.pending.empty()) { (void)hipSetDevice(p->device); (void)hipStreamSynchronize(p->stream); p->timer.resolve(); }
  p->timer.reset();
  p->timer.mask = mask & 0xff;
  p->timer.every = std::max(1, (mask >> 8) & 0xff);
  return CALICO_OK;
}

int32_t calico_get_phase_time(calico_problem* p, int32_t phase, double* ms, int64_t* launches) {
  const bool working = (phase & 0x100) != 0;
  phase &= 0xff;
  if (!p || phase < 0 || phase >= kNumPhases) return CALICO_INVALID_ARGUMENT;
  if (!p->timer.pending.empty()) {   // brackets still on the stream (a solve returns without waiting for it to drain)
    HIP_TRY(p, hipSetDevice(p->device));
    HIP_TRY(p, hipStreamSynchronize(p->stream));
    p->timer.resolve();
  }
  if (ms) *ms = working ? p->timer.ms_working[phase] : p->timer.ms[phase];
  if (launches) *launches = working ? p->timer.count_working[phase] : p->timer.count[phase];
  return CALICO_OK;
}

}  // extern "C"
