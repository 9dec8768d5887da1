// problem_host.hpp — what the host translation units of libcalico_hip.so share: the handle (calico_problem) with its plan,
// device structure and workspace, the device-memory arena, and the functions calico_hip.cpp, plan.cpp, solve.cpp and
// analysis.cpp call of one another (declared once, at the end).
// Internal: nothing declared here is part of the C ABI (include/calico_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>     // types only: the library itself is loaded on first use (rccl(), calico_hip.cpp)

#include <algorithm>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/calico_hip.h"
#include "kernels.hpp"
#include "problem_dev.hpp"

#pragma GCC visibility push(hidden)
namespace cal {

constexpr int kLogCap = 4096;
constexpr int kPlanInfoWords = 28;    // words calico_debug_plan_info reports (calico_hip_testing.h)
constexpr int kNumPhases = 7;   // 5 = calibration: the same event bracket around a trivial kernel; 6 = the reduced-system launch inside phase 2

struct HBlock {
  std::vector<double> v;
  int size = 0, manifold = 0;
  bool constant = false, used = false;
  int amb_off = 0;
  int tan = -1;      // solver tangent index (6·cp for control points, 6·n_cp + c for calibration blocks)
  int eff = -1;      // tangent index in the reduced-problem order exported by calico_evaluate
  int tangent_size() const { return manifold == CALICO_MANIFOLD_EIGEN_QUATERNION ? 3 : size; }
};
struct HBody { int q, t; };
struct HSensor {
  int kind, model, K;
  int intr, q, t, lat, grav;
  double sigma, info;
  int loss; double loss_scale;
  std::vector<double> meas, stamps;
  std::vector<int> body, point, seg;
  std::vector<int64_t> sorted_pos;  // original observation -> position in the sorted device arrays
  std::vector<uint8_t> active;      // 0 = tagged as outlier (outlier_ids_, camera.h:185): left out of the problem
  int64_t n_active = -1;            // cached count of the blocks that are in the problem (-1: recount)
  int64_t sorted_begin = 0, sorted_end = 0;   // this sensor's contiguous range in the sorted arrays
  int dim() const { return kind == CALICO_SENSOR_CAMERA ? 2 : 3; }
  int64_t n() const { return int64_t(stamps.size()); }
};

// Device memory of plans and workspaces comes out of a few large slabs instead of one hipMalloc per buffer: a handle
// has some forty buffers, most of them a few KB, and a buffer of its own sits on pages of its own -- every kernel's
// first touch of each (state, descriptors, index lists, ...) then costs an address translation of its own behind the
// kernel boundary. One slab is one allocation of 64 MB: contiguous, mapped with the largest fragments the driver
// has. First fit over a free list ordered by address, neighbours merged on release; a request no slab can serve opens
// a new slab, and if that fails the request goes to hipMalloc as before. A request larger than a slab is an allocation
// of its own (hipMalloc / hipFree: it has large fragments anyway and must not pin memory for good).
// Slabs go back to the driver: trim() frees every slab that is one free extent -- calico_plan_cache_clear() frees all of
// them, calico_problem_destroy() all but CALICO_ARENA_KEEP_SLABS idle ones per device (default 4) -- so a process that once solved a large
// problem, or that shares the GPU with PyTorch / RCCL, does not keep that memory. (No HIP calls during static
// destruction: what is still held at exit is the driver's to reclaim.) CALICO_ARENA=0: hipMalloc per buffer (rounds 1-4).
class DeviceArena {
 public:
  static DeviceArena& get() { static DeviceArena* a = new DeviceArena; return *a; }
  hipError_t alloc(void** out, size_t bytes) {
    if (!enabled_ || bytes > kSlab) return hipMalloc(out, bytes);
    bytes = (bytes + kAlign - 1) / kAlign * kAlign;
    std::lock_guard<std::mutex> g(mu_);
    int dev = 0; (void)hipGetDevice(&dev);
    for (int pass = 0; pass < 2; ++pass) {
      for (Slab& sl : slabs_) {
        if (sl.device != dev) continue;
        for (auto it = sl.free.begin(); it != sl.free.end(); ++it) {
          if (it->second < bytes) continue;
          const size_t off = it->first, len = it->second;
          sl.free.erase(it);
          if (len > bytes) sl.free.emplace(off + bytes, len - bytes);
          *out = sl.base + off;
          used_[*out] = bytes;
          return hipSuccess;
        }
      }
      if (pass == 1) break;
      void* base = nullptr;
      if (hipMalloc(&base, kSlab) != hipSuccess) { (void)hipGetLastError(); break; }
      Slab sl; sl.base = static_cast<char*>(base); sl.size = kSlab; sl.device = dev; sl.free.emplace(0, kSlab);
      slabs_.push_back(std::move(sl));
    }
    return hipMalloc(out, bytes);      // (not in used_: release() hands it to hipFree)
  }
  void release(void* p) {
    if (!p) return;
    int owner = -1;
    {
      std::lock_guard<std::mutex> g(mu_);
      if (used_.count(p))
        for (const Slab& sl : slabs_)
          if (static_cast<char*>(p) >= sl.base && static_cast<char*>(p) < sl.base + sl.size) { owner = sl.device; break; }
    }
    if (owner < 0) { (void)hipFree(p); return; }
    // hipFree waits for the device; a block that goes back to the free list must do the same (a solve returns while the
    // early-exit kernels of the iterations enqueued ahead are still on its stream) -- for the device that OWNS the slab,
    // and once per batch of releases (Batch below), not once per buffer
    if (batch_device() != owner) sync_device(owner);
    std::lock_guard<std::mutex> g(mu_);
    auto u = used_.find(p);
    if (u == used_.end()) return;
    const size_t bytes = u->second;
    used_.erase(u);
    for (Slab& sl : slabs_) {
      char* c = static_cast<char*>(p);
      if (c < sl.base || c >= sl.base + sl.size) continue;
      size_t off = size_t(c - sl.base), len = bytes;
      auto next = sl.free.lower_bound(off);
      if (next != sl.free.end() && next->first == off + len) { len += next->second; next = sl.free.erase(next); }
      if (next != sl.free.begin()) {
        auto prev = std::prev(next);
        if (prev->first + prev->second == off) { off = prev->first; len += prev->second; sl.free.erase(prev); }
      }
      sl.free.emplace(off, len);
      return;
    }
  }
  // Everything a handle or a plan gives back at once (some forty buffers): ONE wait for the owning device, up front.
  struct Batch {
    explicit Batch(int device) : prev_(batch_device()) { if (DeviceArena::get().enabled_) { sync_device(device); batch_device() = device; } }
    ~Batch() { batch_device() = prev_; }
    Batch(const Batch&) = delete;
    Batch& operator=(const Batch&) = delete;
   private:
    int prev_;
  };
  // Frees the slabs nothing lives in; `keep_per_device` of them stay per device for the next handle. Returns the bytes freed.
  size_t trim(int keep_per_device) {
    std::vector<Slab> drop;
    {
      std::lock_guard<std::mutex> g(mu_);
      std::map<int, int> kept;
      for (size_t i = 0; i < slabs_.size();) {
        Slab& sl = slabs_[i];
        const bool idle = sl.free.size() == 1 && sl.free.begin()->first == 0 && sl.free.begin()->second == sl.size;
        if (idle && kept[sl.device]++ >= keep_per_device) { drop.push_back(std::move(sl)); slabs_.erase(slabs_.begin() + long(i)); }
        else ++i;
      }
    }
    size_t bytes = 0;
    for (Slab& sl : drop) { (void)hipFree(sl.base); bytes += sl.size; }     // (hipFree waits for the device itself)
    return bytes;
  }
  size_t slab_bytes() { std::lock_guard<std::mutex> g(mu_); size_t b = 0; for (const Slab& sl : slabs_) b += sl.size; return b; }
 private:
  static constexpr size_t kAlign = 4096, kSlab = size_t(64) << 20;
  struct Slab { char* base = nullptr; size_t size = 0; int device = 0; std::map<size_t, size_t> free; };
  DeviceArena() { enabled_ = env_flag("CALICO_ARENA", true); }
  static int& batch_device() { static thread_local int d = -1; return d; }
  static void sync_device(int device) {
    int cur = device;
    (void)hipGetDevice(&cur);
    if (cur != device) (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
    if (cur != device) (void)hipSetDevice(cur);
  }
  std::mutex mu_;
  std::vector<Slab> slabs_;
  std::unordered_map<void*, size_t> used_;
  bool enabled_ = true;
};

template <class T> struct DevBuf {
  T* p = nullptr; size_t n = 0;
  bool owner = true;        // false: a view of a buffer the plan cache owns (structure shared between handles)
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() { if (p && owner) DeviceArena::get().release(p); p = nullptr; n = 0; owner = true; }
  void alias(const DevBuf& o) { release(); p = o.p; n = o.n; owner = false; }
  void take(DevBuf& o) { release(); p = o.p; n = o.n; owner = o.owner; o.p = nullptr; o.n = 0; o.owner = true; }
  void swap(DevBuf& o) { std::swap(p, o.p); std::swap(n, o.n); std::swap(owner, o.owner); }
  hipError_t alloc(size_t count) {
    if (count == 0) count = 1;
    if (count == n && p && owner) return hipSuccess;
    release();        // (a view is dropped, never written through)
    hipError_t e = DeviceArena::get().alloc(reinterpret_cast<void**>(&p), count * sizeof(T));
    if (e == hipSuccess) n = count;
    return e;
  }
  hipError_t upload(const std::vector<T>& h, hipStream_t s) {
    hipError_t e = alloc(h.size());
    if (e != hipSuccess || h.empty()) return e;
    return hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s);
  }
};

struct PhaseTimer {
  std::vector<hipEvent_t> pool;
  struct Rec { int phase; hipEvent_t a, b; };
  std::vector<Rec> pending;
  size_t next = 0;
  double ms[kNumPhases] = {0, 0, 0, 0, 0, 0};
  int64_t count[kNumPhases] = {0, 0, 0, 0, 0, 0};
  // the same restricted to "working" launches: kernels of iterations enqueued ahead return at once when the solve has
  // terminated (or the step was rejected), and such brackets (shorter than a quarter of the phase's longest) are left out
  double ms_working[kNumPhases] = {0, 0, 0, 0, 0, 0};
  int64_t count_working[kNumPhases] = {0, 0, 0, 0, 0, 0};
  std::vector<float> samples[kNumPhases];
  hipEvent_t get() {
    if (next == pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); pool.push_back(e); }
    return pool[next++];
  }
  int mask = 0;              // no event brackets unless asked for (calico_set_phase_timing): each pair costs ~6 us of stream time
  int every = 1;            // bracket only every `every`-th launch of a phase (an event pair costs ~6 us of stream time)
  int64_t seen[kNumPhases] = {0, 0, 0, 0, 0, 0};
  bool open_rec = false;
  int nested = 0;           // phase 6 sits inside phase 2: a bracket inside an open bracket is not recorded
  void begin(int phase, hipStream_t s) {
    if (open_rec) { ++nested; return; }
    open_rec = (mask >> phase) & 1;
    if (open_rec && phase != 5 && every > 1) open_rec = (seen[phase]++ % every) == 0;
    if (!open_rec) return;
    Rec r; r.phase = phase; r.a = get(); r.b = nullptr; (void)hipEventRecord(r.a, s); pending.push_back(r);
  }
  void end(hipStream_t s) { if (nested) { --nested; return; } if (!open_rec) return; Rec& r = pending.back(); r.b = get(); (void)hipEventRecord(r.b, s); open_rec = false; }
  void resolve() {  // call after a stream sync
    for (const Rec& r : pending) {
      float t = 0;
      if (r.b && hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) { ms[r.phase] += t; count[r.phase]++; samples[r.phase].push_back(t); }
    }
    pending.clear(); next = 0;
    for (int ph = 0; ph < kNumPhases; ++ph) {
      float mx = 0; for (float t : samples[ph]) mx = std::max(mx, t);
      ms_working[ph] = 0; count_working[ph] = 0;
      for (float t : samples[ph]) if (t >= 0.25f * mx) { ms_working[ph] += t; count_working[ph]++; }
    }
  }
  void reset() { for (int i = 0; i < kNumPhases; ++i) { ms[i] = 0; count[i] = 0; seen[i] = 0; ms_working[i] = 0; count_working[i] = 0; samples[i].clear(); } }
  ~PhaseTimer() { for (hipEvent_t e : pool) (void)hipEventDestroy(e); }
};

}  // namespace cal
#pragma GCC visibility pop

using namespace cal;      // (the handle and its parts are global: calico_problem is the C ABI's opaque type)

// ---- what calico_problem_finalize derives from the STRUCTURE of a problem (not from any value): shared between handles
//      of identical structure through the plan cache -------------------------------------------------------------------
struct BcrLevel { int node0, n_nodes, keep0, n_keep, q_max; };
struct PlanHost {
  bool speculative = true;    // evaluate cost AND Jacobian at the candidate point in one pass (two reduce buffers)
  size_t r_size = 0;
  int sep_s = 0, sep_n = 0;   // separator control points of the nested-dissection split (sep_n = 0: none)
  // tree solver (bcr_kernels.hip): elimination plan, level after level
  bool use_bcr = false, bcr_all_active = false;
  int bcr_N = 0, bcr_m1p = 16, bcr_root = -1, bcr_root_pend = 0, bcr_root_par = 0, bcr_br = 0, bcr_q_max = 1, bcr_slots = 1, bcr_q0 = 1;
  std::vector<BcrLevel> bcr_levels;
  std::vector<BcrNodeDev> h_bcr_nodes;
  int border_extra() const { return use_bcr ? bcr_br : 6 * sep_n; }   // rows the band hands to the dense reduced solve
  int n_cp = 0, m = 0, n_amb = 0, n_eff = 0, n_items = 0, n_items_all = 0, lds_cols = 0, row_pad = kRowPad;
  int64_t n_obs = 0, n_obs_local = 0;   // residual blocks: all, this rank's shard (calico_comm_info)
  size_t partial_doubles = 0, partials_alloc = 0;
  std::vector<int> eff_to_tan;
  std::vector<BlockDev> h_blocks;
  int n_cells = 0, cell_chunk = 1, cell_rec_max = 1, row_cell_chunk = 1;
  int frame_lds_doubles = 0;
  int n_fitems = 0, n_jac_items = 0;
  int max_cell_frames = 0, max_item_run = 0;   // frames of the fullest camera cell, longest run of one cell's work items (calico_debug_plan_info)
  bool fuse_expand = false;    // cell workgroups (EvalArgs.pair_mode): camera cells expanded inside the Jacobian launch, IMU items form their own blocks
  int pair_wave_lds_doubles = 0;
  int n_thin = 0, n_fat = 0;
  int n_thin8 = 0, n_thin4 = 0;  // thin outputs [0, n_thin8) take eight lanes, [n_thin8, n_thin4) four (<= 24 sources), [n_thin4, n_thin) one (<= 8)
  int thin_per_lane = 6;       // sources per lane of a thin output's eight lanes (6: up to 48 sources, 12: up to 96)
  bool gather_fixed = false;   // the thin lists at a fixed stride (d_idx_fixed) instead of CSR
  bool dense_in_lds = true;
  // calico_prediction_covariance: widest layout (columns) and longest work item (row stride) of the list of ALL work items,
  // row length of the column map (d_pred_map)
  int pred_cols = 0, pred_row_pad = 3, pred_map_stride = 1;
};
struct PlanDev {      // structure on the device: immutable once uploaded
  DevBuf<double> d_knots, d_basis, d_stamp;
  DevBuf<int> d_ctrl_off, d_point_off, d_out_thin, d_idx_thin, d_idx_fixed, d_out_fat, d_idx_fat, d_prim_tab, d_bkeep, d_cp_block, d_gs_tab, d_pred_map;
  DevBuf<int64_t> d_ptr_thin, d_ptr_fat;
  DevBuf<uint8_t> d_cp_active;
  DevBuf<SensorDev> d_sensors;
  DevBuf<LayoutDev> d_layouts;
  DevBuf<ItemDev> d_items, d_items_all, d_jac_items;
  DevBuf<FrameItemDev> d_fitems;
  DevBuf<CellDev> d_cells;
  DevBuf<BlockDev> d_blocks;
  DevBuf<BcrNodeDev> d_bnodes;
#define PLAN_DEV_BUFS(X) X(d_knots) X(d_basis) X(d_stamp) X(d_ctrl_off) X(d_point_off) X(d_out_thin) X(d_idx_thin) X(d_idx_fixed) X(d_out_fat) X(d_idx_fat) \
  X(d_prim_tab) X(d_bkeep) X(d_cp_block) X(d_gs_tab) X(d_ptr_thin) X(d_ptr_fat) X(d_cp_active) X(d_sensors) X(d_layouts) X(d_items) X(d_items_all)     \
  X(d_jac_items) X(d_fitems) X(d_cells) X(d_blocks) X(d_bnodes) X(d_pred_map)
  void take_from(PlanDev& o) {
#define X(n) n.take(o.n);
    PLAN_DEV_BUFS(X)
#undef X
  }
  void alias_from(const PlanDev& o) {
#define X(n) n.alias(o.n);
    PLAN_DEV_BUFS(X)
#undef X
  }
};
// ---- what a handle works in: values, normal equations, solver workspaces, result staging. Recycled between handles of
//      identical structure (a destroyed handle leaves its workspace with the cached plan) ----------------------------------
struct Workspace {
  DevBuf<unsigned long long> d_wave_log;   // CALICO_KERNEL_TIMING=3
  DevBuf<double> d_x, d_xc, d_m0, d_m1, d_m2, d_partials, d_R, d_R2, d_Lb, d_Linv, d_Y, d_S, d_Spart, d_Swork, d_zbuf, d_y, d_dadd, d_scale, d_res;
  DevBuf<double> d_bD, d_bG, d_bF, d_bpD, d_bpF, d_bM, d_bZA, d_bZB, d_bY, d_bysol, d_bzb, d_bupd;
  DevBuf<uint8_t> d_valid, d_active;
  DevBuf<int> d_counter;
  DevBuf<int> d_handoff;         // hand-off word of the fused dense-solve + back-substitution launch
  DevBuf<LmState> d_state;
  DevBuf<IterLog> d_log;
  int handoff_seq = 0;           // number of the last such launch (the word carries it when the solve part is through)
  LmState* h_state = nullptr;  // pinned
  int* h_progress = nullptr;   // pinned, device-visible: [epoch << 20 | iterations the control kernel is through with, epoch of the terminated solve]
  int solve_epoch = 0;         // number of the streaming solve under way (1 .. 2047, wraps)
  int* d_progress = nullptr;
  double* h_xpin = nullptr;    // pinned staging for the parameter vector (upload at the start of a call, download at its end)
  size_t h_xpin_n = 0;
  IterLog* h_log = nullptr;    // pinned
  bool ws_ready = false;       // allocated and initialised for the plan at hand
#define WS_BUFS(X) X(d_wave_log) X(d_x) X(d_xc) X(d_m0) X(d_m1) X(d_m2) X(d_partials) X(d_R) X(d_R2) X(d_Lb) X(d_Linv) X(d_Y) X(d_S) X(d_Spart)      \
  X(d_Swork) X(d_zbuf) X(d_y) X(d_dadd) X(d_scale) X(d_res) X(d_bD) X(d_bG) X(d_bF) X(d_bpD) X(d_bpF) X(d_bM) X(d_bZA) X(d_bZB) X(d_bY) X(d_bysol) \
  X(d_bzb) X(d_bupd) X(d_valid) X(d_active) X(d_counter) X(d_handoff) X(d_state) X(d_log)
  void swap_ws(Workspace& o) {
#define X(n) n.swap(o.n);
    WS_BUFS(X)
#undef X
    std::swap(handoff_seq, o.handoff_seq); std::swap(h_state, o.h_state); std::swap(h_progress, o.h_progress);
    std::swap(solve_epoch, o.solve_epoch); std::swap(d_progress, o.d_progress); std::swap(h_xpin, o.h_xpin);
    std::swap(h_xpin_n, o.h_xpin_n); std::swap(h_log, o.h_log); std::swap(ws_ready, o.ws_ready);
  }
  void free_pinned() {
    if (h_state) (void)hipHostFree(h_state);
    if (h_progress) (void)hipHostFree(h_progress);
    if (h_xpin) (void)hipHostFree(h_xpin);
    if (h_log) (void)hipHostFree(h_log);
    h_state = nullptr; h_progress = nullptr; d_progress = nullptr; h_xpin = nullptr; h_xpin_n = 0; h_log = nullptr;
  }
  Workspace() = default;
  Workspace(const Workspace&) = delete;
  Workspace& operator=(const Workspace&) = delete;
  ~Workspace() { free_pinned(); }
};

struct PlanEntry;      // plan cache entry (plan.cpp)

struct calico_problem : PlanHost, PlanDev, Workspace {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string error;
  std::vector<HBlock> blocks;
  std::vector<HBody> bodies;
  std::vector<HSensor> sensors;
  int order = 0;
  std::vector<double> knots, valid_knots, basis;
  std::vector<int> ctrl;
  bool dirty = true;
  calico_allreduce_fn allreduce = nullptr;
  void* allreduce_ctx = nullptr;
  ncclComm_t comm = nullptr;      // native exchange: RCCL communicator owned by the handle (calico_comm_init_rccl)
  bool has_exchange() const { return allreduce != nullptr || comm != nullptr; }
  int rank = 0, world = 1;
  std::shared_ptr<PlanEntry> plan;    // the cached plan this handle's structure buffers are views of (null: it owns them)

  std::vector<double> h_x;     // staging of the parameter values (alive until the upload is through)
  double* h_mpin = nullptr;    // pinned staging of the measurements in device order [m0 | m1 | m2], borrowed from the process-wide pool for the duration of finalize
  size_t h_mpin_n = 0;
  bool active_dirty = true;
  bool any_tagged = false;       // some observation is tagged as an outlier: the kernels look at the tags only then
  bool xc_stale = true;       // the candidate buffer must be re-seeded with the constant blocks' values
  bool step_ready = false;    // d_y / d_dadd / d_scale hold a linear solve of the current plan and values (calico_debug_last_step)
  // residuals of ALL sensors at the parameter values `x` (calico_get_residuals / calico_project are per sensor, as
  // Sensor::UpdateResiduals is: the second to last sensor of a write-back are served from here)
  struct ResCache { bool valid = false, predict = false; std::vector<double> x, r; std::vector<uint8_t> v; } res_cache;
  std::vector<calico_iteration> iterations;
  PhaseTimer timer;
  // The post-solve analyses (analysis.cpp). Owned by the handle, not by the workspace the plan cache recycles.
  // What the covariance and the observability pass work in and nothing reads once a compute has returned: the pass's own LM
  // state, scale, damping and solution buffers (the pass never touches the LM's) and the factor of the control points' band.
  // One set: the two passes share it.
  struct PassBuffers {
    DevBuf<LmState> st;
    DevBuf<double> scale, dadd, y, zbuf, cp_dq, cp_L, cp_Li, cp_info;
  } pass;
  // A parameter block as a compute found it: offset of its tangent rows in the border (kBlockAbsent: not in it -- constant or
  // unused --, kBlockControlPoint: a control point), ambient size, tangent size, manifold, value (the quaternion lift is taken
  // at the values the result was computed at), the control point's index (-1: not one)
  static constexpr int kBlockAbsent = -1, kBlockControlPoint = -2;
  struct BlockSnapshot { int off, size, tsize, manifold; std::vector<double> v; int cp; };
  // calico_covariance_compute: the factorisation's workspace and the result
  struct Covariance {
    DevBuf<double> work, out, info;
    bool valid = false;
    int dim = 0, n_unobserved = 0;
    double min_relative_pivot = 0.0;
    std::vector<double> sigma;       // dim x dim, border tangent order
    std::vector<BlockSnapshot> blocks;      // per block id at the time of the compute
    // control_points: the control points' blocks (cov_kernels.hip, CpCovArgs), their host copies and the stamp buffers
    DevBuf<double> cp_M, cp_X, cp_W, cp_Z, cp_sae, cp_band, st_t, st_out;
    DevBuf<int> st_seg;
    bool has_cp = false, cp_requested = false;     // (requested: control_points = 1, whether or not the problem has a spline)
    int n_cp = 0, order = 0;
    double min_relative_pivot_band = 0.0;
    std::vector<double> sae, band;     // Σ_AE (6 n_cp x dim), Σ_AA's band ([n_cp][order][36], block (J + d, J) row-major)
  } cov;
  // calico_observability_compute: the eigensolver's workspace and the report (obs_kernels.hip)
  struct Observability {
    DevBuf<double> work, lam, vec, mat, dvec, info;
    bool valid = false;
    int dim = 0, kept = 0, n_unobserved = 0, n_weak = 0, sweeps = 0, rotations = 0, in_lds = 0, reduced_rows = 0;
    double min_relative_pivot_root = 0.0, min_relative_pivot_band = 0.0;
    std::vector<double> eigenvalues;     // kept, ascending
    std::vector<double> vectors;         // kept x dim: row i the unit eigenvector v_i, border tangent order, zeros in dropped columns
    std::vector<double> d;               // dim: D = sqrt(diag C), 0 in dropped columns
    std::vector<double> matrix;          // dim x dim: S̃, zeros in dropped rows and columns
    std::vector<BlockSnapshot> blocks;   // per block id at the time of the compute
  } obs;

  int set_error(int code, const std::string& msg) { error = msg; return code; }
  int hip_error(hipError_t e, const char* what) {
    return set_error(CALICO_INTERNAL, std::string(what) + ": " + hipGetErrorString(e));
  }
};

#define HIP_TRY(p, expr)                                    \
  do {                                                      \
    hipError_t _e = (expr);                                 \
    if (_e != hipSuccess) return (p)->hip_error(_e, #expr); \
  } while (0)


// ---- what the host files call of one another --------------------------------------------------------------------------------
#pragma GCC visibility push(hidden)
namespace cal {
// calico_hip.cpp
struct RcclApi {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string error;
  bool ok() const { return lib != nullptr; }
};
RcclApi& rccl();
int spline_index(const calico_problem* p, double t);
// a sharded handle (calico_problem_set_shard, world > 1) evaluates only with an exchange: CALICO_OK, or the error set
int require_exchange(calico_problem* p);
// plan.cpp
int finalize(calico_problem* p);
void return_workspace(calico_problem* p);
void release_measurement_staging(calico_problem* p);
void plan_cache_stats(int64_t* hits, int64_t* misses, int64_t* entries);
void plan_cache_clear();
// solve.cpp
// The switches that shape a solve, read when one is constructed -- at the start of a solve (SolveRun::begin), of
// the analyses' reduce-only pass and of calico_debug_plan_info -- and handed down: the per-solve counterpart of plan.cpp's
// PlanSwitches. Each is an A/B switch whose other value is the reference of a test.
struct SolveSwitches {
  int stream_depth = env_int("CALICO_STREAM_DEPTH", 2, 0);          // iterations the polled loop keeps ahead of the device (0: the batched loop)
  bool predict_end = env_flag("CALICO_PREDICT_END", true);          // 0: always one iteration ahead, no end hint (rounds 2-3)
  bool multirank_async = env_flag("CALICO_MULTIRANK_ASYNC", true);  // 0: one host round trip per iteration with several ranks
  bool inline_nodes = env_flag("CALICO_INLINE_NODES", true);        // 0: every level reads its node descriptors from the table
  bool fuse_back = env_flag("CALICO_FUSE_BACK", true);              // 0: the dense solve and the first back-substitution in two launches
  // the fused launch's nodes in affine form (PRE): unset (-1) where the reduced solve is long enough to hide it behind
  // (dense_back_pre_pays), 0 never, any other value (1) wherever the columns fit
  int back_pre = env_flag("CALICO_BACK_PRE", true) ? (env_flag("CALICO_BACK_PRE", false) ? 1 : -1) : 0;
  bool block_elim = !env_is("CALICO_ELIM", "panel");                // panel: the block factorisation of rounds 1-3 (two in-wave panels + tile update + Z phase)
  bool dense_roll = env_flag("CALICO_DENSE_ROLL", true);            // 0: the dense reduced solve's barrier form instead of rolling owners
  bool level_roll = env_flag("CALICO_ROLL", true);                  // 0: level 0's chains in the barrier form instead of the rolling chief
};
// What one linear solve does, from the plan and the solve's switches: decided once per solve (linear_route), followed by
// enqueue_linear_solve and the launch helpers it hands the fields to, reported by calico_debug_plan_info (one decision, so
// the hook cannot drift from what runs).
struct LinearRoute {
  int ks = 1;                 // K-slices of the Schur complement (reduced_schur_slices)
  int reduced = 0;            // ReducedRoute of the reduced solve
  bool reduced_in_lds = true; // kReducedKernel: works in LDS (else in Swork)
  bool elim = true;           // the elimination by blocks (else the panel factorisation), in the tree's levels and the dense solve
  int dense_mode = 2;         // dense_block_solve_body's `elim`: 0 the panel form, 1 blocks with barriers, 2 rolling owners
  // tree solver only:
  bool schur_rides = false;   // the Schur complement rides in the last level's launch
  BcrTopSeps ts = {};         // top separators back-substituted in the launch of the level below (ts.n of them)
  int l_first = 0;            // level of the first back-substitution launch behind the reduced solve
  bool fused = false;         // the dense solve and that back-substitution share one launch (dense_back_kernel)
  bool back_pre = false;      // ... whose nodes form their solution as an affine map while they wait (dense_back_kernel<.., PRE>)
  bool level0_roll = false;   // level 0's chains with the rolling chief (bcr_level_kernel<true, true, true>)
  bool inline_nodes = false;  // the levels' node descriptors travel in the launch arguments
};
LinearRoute linear_route(const calico_problem* p, const SolveArgs& sa, const SolveSwitches& sw);
int kernel_timing_level();    // CALICO_KERNEL_TIMING, read once per process (development diagnostics of a CALICO_DEV_TIMING build)
SolveArgs make_solve_args(calico_problem* p);
EvalArgs make_eval_args(calico_problem* p, const double* x, int apply_loss, bool want_res);
int upload_x(calico_problem* p, bool seed = true);
int enqueue_jacobian_eval(calico_problem* p, const LmState* st, int need_flag, const double* x_at = nullptr, bool spec = false,
                          const ControlTail* tail = nullptr, bool end_hint = false);
void enqueue_linear_solve(calico_problem* p, const SolveArgs& sa, const LinearRoute& rt, const LmOptionsDev& o, int with_post_eval, int jacobi,
                          bool reduce_only = false);
}  // namespace cal
#pragma GCC visibility pop
