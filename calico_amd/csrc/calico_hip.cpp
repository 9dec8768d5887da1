// calico_hip.cpp — host side of libcalico_hip.so: the C ABI of
// include/calico_hip.h, problem flattening, and the LM driver loop.
//
// What the reference does per Optimize() call (batch_optimizer.cpp:53-81) —
// build a ceres::Problem from the sensors / world model / trajectory, run
// ceres::Solve, re-evaluate the residual blocks — maps here to:
//   add_* calls  -> host-side block / observation tables,
//   finalize()   -> cells, work items, gather lists, device upload,
//   calico_solve -> device-resident LM (kernels in eval_kernels.hip and
//                   solve_kernels.hip; this file only enqueues them and reads
//                   back one small state struct per iteration),
//   calico_get_residuals -> cost-only kernel without the loss function.
// What is read from a solved problem (covariance, prediction covariance, observability) is analysis.cpp; the handle and
// what the two files share is problem_host.hpp.
// There is no CPU compute path in this library.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>     // types only: the library itself is loaded on first use (RcclApi below)
#include <dlfcn.h>
#include <link.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <array>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/calico_hip.h"
#include "calico_hip_testing.h"
#include "kernels.hpp"
#include "problem_dev.hpp"
#include "problem_host.hpp"
#include "shard.hpp"

namespace {

// RCCL is loaded when the first communicator is asked for (calico_comm_get_unique_id / calico_comm_init_rccl), not at
// link time: a single-GPU user needs no librccl on the machine. An already loaded librccl (e.g. the one torch ships) is
// found by its soname; otherwise $ROCM_PATH/lib, then the loader's search path.
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

int camera_num_params(int model) {
  switch (model) { case 1: return 8; case 2: return 11; case 3: return 7; case 4: return 5; case 5: return 4; case 6: return 4;
    case 7: return 5; default: return -1; }
}
int imu_num_params(int model) { return model == 1 ? 1 : (model == 2 ? 4 : (model == 3 ? 12 : -1)); }

// The switches that shape a plan, read when one is constructed -- once per finalize: build_plan takes them from
// here and the plan cache's key hashes them, so a plan built under other settings is never adopted.
struct PlanSwitches {
  bool band_solver = env_is("CALICO_SOLVER", "band");            // the sequential banded factorisation for every spline order
  bool speculative = env_flag("CALICO_SPECULATIVE", true);
  bool band_split = env_flag("CALICO_BAND_SPLIT", true);          // the banded factorisation's separator
  bool fuse_expand = env_flag("CALICO_FUSE_EXPAND", true);        // cell workgroups
  bool gather_struct = env_flag("CALICO_GATHER_STRUCT", true);    // the gather's lists built on the device
  int bcr_leaf = env_int("CALICO_BCR_LEAF", 0, 1, kBcrMaxChain);  // level 0's chain length (0: chosen by the plan)
};

BcrArgs make_bcr_args(calico_problem* p) {
  BcrArgs b;
  b.D = p->d_bD.p; b.G = p->d_bG.p; b.F = p->d_bF.p; b.pendD = p->d_bpD.p; b.pendF = p->d_bpF.p; b.M = p->d_bM.p; b.ZA = p->d_bZA.p;
  b.ZB = p->d_bZB.p; b.Y = p->d_bY.p; b.ysol = p->d_bysol.p; b.zb = p->d_bzb.p; b.upd = p->d_bupd.p; b.nodes = p->d_bnodes.p; b.keep = p->d_bkeep.p;
  b.cp_block = p->d_cp_block.p; b.ctrl_off = p->d_ctrl_off.p; b.all_active = p->bcr_all_active ? 1 : 0; b.pad0 = 0; b.N = p->bcr_N; b.m1p = p->bcr_m1p; b.root = p->bcr_root; b.root_pend = p->bcr_root_pend;
  b.root_par = p->bcr_root_par; b.n_slots = p->bcr_slots;
  return b;
}

// Elimination plan of the tree solver: level 0 eliminates chains of q consecutive superblocks between kept
// separators, every further level every other survivor; the last survivor is the root (joins the dense solve).
// q minimises (levels · launch + chain steps · factorisation) for the trajectory length at hand.
void build_bcr_plan(calico_problem* p, const PlanSwitches& sw, std::vector<int>& keep) {
  const int N = (p->n_cp + kBcrCps - 1) / kBcrCps;
  p->bcr_N = N;
  auto levels_after = [](int n_sep) { int l = 0; while (n_sep > 1) { n_sep /= 2; ++l; } return l; };
  int q = 1;
  {
    double best = 1e300;
    for (int c = 1; c <= kBcrMaxChain; ++c) {
      const int n_sep = N > c ? N / (c + 1) : 0;
      const int L = 1 + levels_after(n_sep);
      double cost = 6.0 * L + 4.0 * (c + L - 1);
      // One workgroup of a level launch fills a CU and the part has 256: a level 0 whose (node, role) workgroups (laid out by XCD:
      // nodes padded to a multiple of eight), eight separators' workgroups and the bookkeeping one do not fit runs its tail in a
      // second dispatch round (1453 control points, chains of four: 256 + 64 + 1 workgroups, level 0 34.7 us; chains of five: +2.9 % it/s)
      const int per = 1 + p->bcr_m1p / 16, nodes = n_sep + 1;
      if (8 * ((nodes + 7) / 8) * per + 9 > 256) cost += 5.0;
      if (cost < best) { best = cost; q = c; }
    }
    if (sw.bcr_leaf > 0) q = sw.bcr_leaf;
  }
  p->bcr_levels.clear(); p->h_bcr_nodes.clear(); keep.clear();
  std::vector<int> alive(static_cast<size_t>(N), 0), mask(static_cast<size_t>(N), 0);
  for (int i = 0; i < N; ++i) alive[size_t(i)] = i;
  int level = 0, q_max_all = 1;
  while (!alive.empty() && (level == 0 || alive.size() > 1)) {
    const int chain = level == 0 ? q : 1;
    BcrLevel L;
    L.node0 = int(p->h_bcr_nodes.size()); L.keep0 = int(keep.size() / 2); L.q_max = 1;
    std::vector<int> kept, new_mask(size_t(N), 0);
    const size_t n = alive.size();
    size_t pos = 0;
    // level 0 with N <= q: one chain, no separator. Otherwise: [chain of `chain`] [keep] [chain] [keep] ...
    while (pos < n) {
      BcrNodeDev nd = {};
      nd.left = kept.empty() ? -1 : kept.back();
      nd.q = 0;
      nd.blk0 = alive[pos]; nd.pend = mask[size_t(alive[pos])];     // chains longer than one block only exist at level 0 (consecutive, no pending)
      while (pos < n && nd.q < chain) { ++nd.q; ++pos; }
      nd.right = pos < n ? alive[pos] : -1;
      nd.slot = int(p->h_bcr_nodes.size());
      L.q_max = std::max(L.q_max, nd.q);
      if (nd.left >= 0) new_mask[size_t(nd.left)] |= 2;
      if (nd.right >= 0) new_mask[size_t(nd.right)] |= 1;
      p->h_bcr_nodes.push_back(nd);
      if (pos < n) { kept.push_back(alive[pos]); ++pos; }
    }
    // separators that survive this level: level 0 initialises them from R(x), later levels add last level's pending updates
    for (int kb : kept)
      if (level == 0 || mask[size_t(kb)]) { keep.push_back(kb); keep.push_back(mask[size_t(kb)]); }
    L.n_nodes = int(p->h_bcr_nodes.size()) - L.node0;
    L.n_keep = int(keep.size() / 2) - L.keep0;
    q_max_all = std::max(q_max_all, L.q_max);
    p->bcr_levels.push_back(L);
    alive = kept; mask = new_mask;
    ++level;
  }
  p->bcr_root = alive.empty() ? -1 : alive[0];
  p->bcr_root_pend = alive.empty() ? 0 : mask[size_t(alive[0])];
  p->bcr_root_par = (level - 1) & 1;
  p->bcr_br = alive.empty() ? 0 : 6 * kBcrCps;
  p->bcr_q_max = q_max_all;
  p->bcr_q0 = q;       // level 0's chain length: its node table is arithmetic on the node's number (BcrInlineNodes)
  p->bcr_slots = int(p->h_bcr_nodes.size()) + 1;
}

constexpr int kImuChunkItems = 21;     // IMU blocks per work item (the Jacobian kernel gives an IMU block three lanes)

// CALICO_SETUP_TIMING=1: wall time of the sections of finalize, plan building included (development aid)
struct SetupTimer {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  void section(const char* name) {
    static const bool on = env_flag("CALICO_SETUP_TIMING", false);
    if (!on) return;
    const auto now = std::chrono::steady_clock::now();
    std::fprintf(stderr, "[calico] finalize %-28s %8.3f ms\n", name, std::chrono::duration<double, std::milli>(now - t).count());
    t = now;
  }
};

// Flatten the host tables into cells / work items / gather lists, plan the elimination, upload the STRUCTURE (everything
// here depends on what the problem looks like, nothing on a value: the result is what the plan cache shares).
// The stages below hand their tables on in PlanTables; only the last one, upload_plan, talks to the device.
struct ObsKey { int layout, seg, sensor; int64_t idx; double stamp; };
struct PlanTables {
  std::vector<uint8_t> cp_active;               // per control point: observed
  std::vector<int> ctrl_off;                    // per control point: ambient offset
  std::vector<int> bcr_keep, cp_block;          // tree solver: kept separators (build_bcr_plan), block of every control point
  std::vector<SensorDev> sd;
  std::vector<LayoutDev> layouts;
  std::vector<std::vector<int>> layout_gmap;    // local calibration column -> solver tangent index
  std::map<std::array<int, 3>, int> layout_of;  // layout_key -> layout id
  std::vector<ObsKey> keys;                     // the observations in device order
  std::vector<double> st; std::vector<int> point_off;   // ... their stamps, their model points' ambient offsets
  int seg_lo = 0, seg_hi = 0;                   // this rank's shard: spline segments [seg_lo, seg_hi)
  std::vector<ItemDev> items, items_all, jac_items;
  std::vector<FrameItemDev> fitems;
  std::vector<CellDev> cells;
  std::vector<int> prim_tab;
  std::vector<int> pred_map;                    // [layout][pred_map_stride]: border offset of every calibration column (prediction covariance)
  size_t partials_end = 0;                      // end of [expanded blocks | item costs | compact frame records | row store]
  // gather lists: host-built CSR (thin / fat), or the table the device builds the thin ones from (gs_ok)
  bool gs_ok = false; int64_t gs_n_out = 0;
  std::vector<int> gs_tab;
  GatherStruct gsd = {};
  std::vector<int> out_thin, idx_thin, out_fat, idx_fat;
  std::vector<int64_t> ptr_thin{0}, ptr_fat{0};
};

// (sensor, body, free model point or -1) of observation i: what its layout is per. A free model point is one more
// calibration block of the residual blocks that observe it, so those blocks get a layout (and cells) of their own per point.
std::array<int, 3> layout_key(const calico_problem* p, size_t si, const HSensor& s, int64_t i) {
  if (s.kind != CALICO_SENSOR_CAMERA) return {int(si), -1, -1};
  return {int(si), s.body[i], p->blocks[s.point[i]].constant ? -1 : s.point[i]};
}

// ---- ambient offsets, used flags, tangent order, the band's separator / the tree solver's plan ----
int plan_blocks(calico_problem* p, const PlanSwitches& sw, PlanTables& t) {
  const int k = p->order;
  const int n_cp = int(p->ctrl.size());
  p->n_cp = n_cp;
  p->speculative = sw.speculative;
  int off = 0;
  for (HBlock& b : p->blocks) { b.amb_off = off; off += b.size; b.used = false; b.tan = -1; b.eff = -1; }
  p->n_amb = off;
  std::vector<char> is_ctrl(p->blocks.size(), 0);
  for (int id : p->ctrl) is_ctrl[id] = 1;
  std::vector<uint8_t>& cp_active = t.cp_active = std::vector<uint8_t>(size_t(n_cp), 0);
  for (HSensor& s : p->sensors) {
    if (s.n() == 0) continue;
    p->blocks[s.intr].used = p->blocks[s.q].used = p->blocks[s.t].used = p->blocks[s.lat].used = true;
    if (s.kind == CALICO_SENSOR_ACCELEROMETER) p->blocks[s.grav].used = true;
    for (int64_t i = 0; i < s.n(); ++i) {
      for (int j = 0; j < k; ++j) cp_active[s.seg[i] + j] = 1;
      if (s.kind == CALICO_SENSOR_CAMERA) {
        p->blocks[s.point[i]].used = true;
        p->blocks[p->bodies[s.body[i]].q].used = p->blocks[p->bodies[s.body[i]].t].used = true;
      }
    }
  }
  for (int i = 0; i < n_cp; ++i) {
    HBlock& b = p->blocks[p->ctrl[i]];
    b.used = cp_active[i] != 0;
    if (b.constant && b.used) return p->set_error(CALICO_UNIMPLEMENTED, "constant control points are not supported");
    b.tan = 6 * i;
    t.ctrl_off.push_back(b.amb_off);
  }
  // ---- tangent order ----
  p->h_blocks.clear(); p->eff_to_tan.clear();
  int eff = 0;
  for (int i = 0; i < n_cp; ++i) {
    if (!cp_active[i]) continue;
    HBlock& b = p->blocks[p->ctrl[i]];
    b.eff = eff; eff += 6;
    for (int c = 0; c < 6; ++c) p->eff_to_tan.push_back(6 * i + c);
    p->h_blocks.push_back({b.amb_off, 6, 0, 6 * i});
  }
  int m = 0;
  for (size_t id = 0; id < p->blocks.size(); ++id) {
    HBlock& b = p->blocks[id];
    if (is_ctrl[id] || b.constant || !b.used) continue;
    b.tan = 6 * n_cp + m; b.eff = eff;
    for (int c = 0; c < b.tangent_size(); ++c) p->eff_to_tan.push_back(b.tan + c);
    p->h_blocks.push_back({b.amb_off, b.size, b.manifold, b.tan});
    m += b.tangent_size(); eff += b.tangent_size();
  }
  p->m = m; p->n_eff = eff;
  bool all_active = true;
  for (int i = 0; i < n_cp; ++i) all_active = all_active && cp_active[size_t(i)] != 0;
  // Nested dissection with one separator (k-1 control points in the middle of the trajectory): the two halves of
  // the band are then factored and back-substituted side by side, the separator joins the dense border. Used when
  // the enlarged border still fits the in-LDS reduced solve and every control point is observed.
  p->sep_s = 0; p->sep_n = 0;
  if (sw.band_split && all_active && n_cp >= 6 * k && m + 6 * (k - 1) + 1 <= 1024) {
    p->sep_n = k - 1;
    p->sep_s = (n_cp - p->sep_n) / 2;
  }
  // Tree solver for spline orders up to 6 (superblocks of five control points are then block tridiagonal); it takes
  // over the split of the band, so the single-separator variant above is switched off. CALICO_SOLVER=band keeps the
  // sequential banded factorisation (A/B switch, and the path of higher spline orders).
  p->use_bcr = k <= 6 && !sw.band_solver;
  if (p->use_bcr) {
    p->sep_s = 0; p->sep_n = 0;
    p->bcr_all_active = all_active;
    p->bcr_m1p = 16 * ((m + 1 + 15) / 16);
    build_bcr_plan(p, sw, t.bcr_keep);
    t.cp_block.assign(size_t(n_cp), -1);
    for (size_t bi = 0; bi < p->h_blocks.size(); ++bi)
      if (p->h_blocks[bi].tan_off < 6 * n_cp) t.cp_block[size_t(p->h_blocks[bi].tan_off / 6)] = int(bi);
  }
  return CALICO_OK;
}

// ---- layouts ----
void plan_layouts(calico_problem* p, PlanTables& t) {
  const int k = p->order;
  t.sd.resize(p->sensors.size());
  auto is_free = [&](int id) { return id >= 0 && !p->blocks[id].constant; };
  for (size_t si = 0; si < p->sensors.size(); ++si) {
    const HSensor& s = p->sensors[si];
    SensorDev& d = t.sd[si];
    d.kind = s.kind; d.model = s.model; d.K = s.K; d.loss = s.loss;
    d.intr_off = p->blocks[s.intr].amb_off; d.q_off = p->blocks[s.q].amb_off; d.t_off = p->blocks[s.t].amb_off;
    d.lat_off = p->blocks[s.lat].amb_off; d.grav_off = s.grav >= 0 ? p->blocks[s.grav].amb_off : 0; d.pad0 = 0;
    d.info = s.info; d.loss_scale = s.loss_scale;
    std::array<int, 3> seen = {-2, -2, -2};       // (consecutive observations mostly share their layout: one compare instead of a map look-up)
    for (int64_t i = 0; i < s.n(); ++i) {
      const int body = s.kind == CALICO_SENSOR_CAMERA ? s.body[i] : -1;
      const std::array<int, 3> lkey = layout_key(p, si, s, i);
      if (lkey == seen) continue;
      seen = lkey;
      if (t.layout_of.count(lkey)) continue;
      LayoutDev L;
      L.sensor = int(si); L.c_pt = -1;
      std::vector<int> gmap;
      int c = 6 * k;
      auto add = [&](int id, int* slot) {
        if (is_free(id)) { *slot = c; for (int q = 0; q < p->blocks[id].tangent_size(); ++q) gmap.push_back(p->blocks[id].tan + q); c += p->blocks[id].tangent_size(); }
        else *slot = -1;
      };
      add(s.intr, &L.c_intr); add(s.q, &L.c_q);
      if (s.kind == CALICO_SENSOR_GYROSCOPE) L.c_t = -1; else add(s.t, &L.c_t);
      add(s.lat, &L.c_lat);
      L.c_bq = L.c_bt = L.c_grav = -1; L.bq_off = L.bt_off = 0;
      if (s.kind == CALICO_SENSOR_CAMERA) {
        add(p->bodies[body].q, &L.c_bq); add(p->bodies[body].t, &L.c_bt);
        L.bq_off = p->blocks[p->bodies[body].q].amb_off; L.bt_off = p->blocks[p->bodies[body].t].amb_off;
        if (lkey[2] >= 0) add(lkey[2], &L.c_pt);
      } else if (s.kind == CALICO_SENSOR_ACCELEROMETER) {
        add(s.grav, &L.c_grav);
      }
      L.ncols = c;
      t.layout_of[lkey] = int(t.layouts.size());
      t.layouts.push_back(L); t.layout_gmap.push_back(gmap);
    }
  }
}

// ---- sort observations by (layout, segment), cut work items, this rank's shard ----
void plan_items(calico_problem* p, PlanTables& t) {
  std::vector<ObsKey>& keys = t.keys;
  int64_t n_obs = 0;
  for (const HSensor& s : p->sensors) n_obs += s.n();
  keys.reserve(size_t(n_obs));
  for (size_t si = 0; si < p->sensors.size(); ++si) {
    HSensor& s = p->sensors[si];
    s.sorted_pos.assign(size_t(s.n()), 0);
    std::array<int, 3> seen = {-2, -2, -2};
    int seen_layout = -1;
    for (int64_t i = 0; i < s.n(); ++i) {
      const std::array<int, 3> lkey = layout_key(p, si, s, i);
      if (!(lkey == seen)) { seen = lkey; seen_layout = t.layout_of[lkey]; }
      keys.push_back({seen_layout, s.seg[i], int(si), i, s.stamps[size_t(i)]});
    }
  }
  {
    // order: (layout, segment, stamp), ties in insertion order. A stable counting sort over the cells (layout, segment)
    // does almost all of it -- measurements arrive in time order, sensor by sensor --; a cell whose stamps are not in
    // order gets a stable comparison sort of its own. (One comparison sort over all keys was 1.5 ms of the set-up.)
    const int nseg_all = std::max(1, int(p->valid_knots.size()) - 1);
    const size_t n_cell_ids = t.layouts.size() * size_t(nseg_all);
    std::vector<int64_t> cstart(n_cell_ids + 1, 0);
    auto cell_of = [&](const ObsKey& kq) { return size_t(kq.layout) * size_t(nseg_all) + size_t(std::max(0, std::min(nseg_all - 1, kq.seg))); };
    for (const ObsKey& kq : keys) ++cstart[cell_of(kq) + 1];
    for (size_t c = 0; c < n_cell_ids; ++c) cstart[c + 1] += cstart[c];
    std::vector<ObsKey> sorted(keys.size());
    {
      std::vector<int64_t> fill(cstart.begin(), cstart.end() - 1);
      for (const ObsKey& kq : keys) sorted[size_t(fill[cell_of(kq)]++)] = kq;
    }
    for (size_t c = 0; c < n_cell_ids; ++c) {
      const int64_t q0 = cstart[c], q1 = cstart[c + 1];
      bool ordered = true;
      for (int64_t q = q0 + 1; q < q1 && ordered; ++q) ordered = !(sorted[size_t(q)].stamp < sorted[size_t(q - 1)].stamp);
      if (!ordered)
        std::stable_sort(sorted.begin() + q0, sorted.begin() + q1, [](const ObsKey& a, const ObsKey& b) { return a.stamp < b.stamp; });
    }
    keys.swap(sorted);
  }
  p->n_obs = n_obs;
  t.st.assign(size_t(n_obs), 0.0);
  t.point_off.assign(size_t(n_obs), 0);
  for (HSensor& s : p->sensors) { s.sorted_begin = n_obs; s.sorted_end = 0; }
  for (int64_t q = 0; q < n_obs; ++q) {
    HSensor& s = p->sensors[keys[q].sensor];
    const int64_t i = keys[q].idx;
    s.sorted_pos[size_t(i)] = q;
    s.sorted_begin = std::min(s.sorted_begin, q); s.sorted_end = std::max(s.sorted_end, q + 1);   // layouts are per sensor: contiguous
    t.st[q] = s.stamps[i];
    if (s.kind == CALICO_SENSOR_CAMERA) t.point_off[q] = p->blocks[s.point[i]].amb_off;
  }
  for (int64_t q = 0; q < n_obs;) {
    int64_t e = q;
    while (e < n_obs && keys[e].layout == keys[q].layout && keys[e].seg == keys[q].seg) ++e;
    const LayoutDev& L = t.layouts[keys[q].layout];
    const int dim = p->sensors[L.sensor].dim();
    // cameras fill the 128 staged rows; an IMU block is a long single-lane computation and there are few of them, so
    // they are cut finer: more waves in flight, shorter JᵀJ stage, smaller LDS footprint next to the camera frames
    const int chunk = dim == 2 ? kRowsPerItem / 2 : kImuChunkItems;
    for (int64_t b = q; b < e; b += chunk) {
      ItemDev it;
      it.layout = keys[q].layout; it.seg = keys[q].seg; it.obs_begin = int(b); it.obs_count = int(std::min<int64_t>(chunk, e - b));
      it.partial_off = 0; it.rows_off = -1;
      t.items_all.push_back(it);
    }
    q = e;
  }
  // this rank's shard: a contiguous window of spline segments (shard.hpp)
  const int nseg = int(p->valid_knots.size()) - 1;
  std::vector<int64_t> per_seg(size_t(nseg), 0);
  for (const ItemDev& it : t.items_all) per_seg[size_t(it.seg)] += it.obs_count;
  const std::vector<int> win = shard_windows(per_seg, p->world);
  t.seg_lo = win[size_t(p->rank)]; t.seg_hi = win[size_t(p->rank) + 1];
  p->n_obs_local = 0;
  for (const ItemDev& it : t.items_all)
    if (it.seg >= t.seg_lo && it.seg < t.seg_hi) { t.items.push_back(it); p->n_obs_local += it.obs_count; }
  p->n_items = int(t.items.size());
  p->n_items_all = int(t.items_all.size());
  // prediction covariance (prediction_items_kernel walks items_all): its staging area's sizes, and per layout the border
  // offset -- row of Σ_EE, column of Σ_AE -- of every calibration column
  {
    int pc = 4, pr = 2, stride = 1;
    for (const ItemDev& it : t.items_all) {
      const LayoutDev& L = t.layouts[size_t(it.layout)];
      pc = std::max(pc, L.ncols);
      pr = std::max(pr, p->sensors[size_t(L.sensor)].dim() * it.obs_count);
    }
    for (const std::vector<int>& g : t.layout_gmap) stride = std::max(stride, int(g.size()));
    p->pred_cols = pc; p->pred_row_pad = (((pr + 3) & ~3) + 1) | 1; p->pred_map_stride = stride;
    t.pred_map.assign(std::max<size_t>(1, t.layouts.size()) * size_t(stride), 0);
    for (size_t l = 0; l < t.layouts.size(); ++l)
      for (size_t j = 0; j < t.layout_gmap[l].size(); ++j) t.pred_map[l * size_t(stride) + j] = t.layout_gmap[l][j] - 6 * p->n_cp;
  }
}

// ---- the evaluation route: frames, cells, cell workgroups, generic and IMU items, the row store ----
int plan_route(calico_problem* p, const PlanSwitches& sw, PlanTables& t) {
  const int k = p->order;
  const int64_t n_obs = p->n_obs;
  const std::vector<ObsKey>& keys = t.keys; const std::vector<LayoutDev>& layouts = t.layouts;
  std::vector<FrameItemDev>& fitems = t.fitems; std::vector<ItemDev>& jac_items = t.jac_items; std::vector<CellDev>& cells = t.cells;
  // Jacobian pass: camera cells are cut into FRAMES (blocks sharing the stamp) for the frame path (eval_frames_body)
  // when the spline order is 6 and frames are reasonably full; everything else goes to the generic kernel.
  size_t poff = 0, comp_off = 0;
  // compact record of a camera frame: M_ext (PE×PE) + expansion coefficients (ncols + 1); see eval_kernels.hip
  auto frame_rec = [&](const LayoutDev& L) -> size_t {
    const int PE = prim_map(L, t.sd[size_t(L.sensor)]).PE;
    return size_t(PE) * PE + size_t(L.ncols + 1);
  };
  // LDS of a frame workgroup of the layout (eval_kernels.hip, frame_lds_doubles)
  auto frame_lds = [&](const LayoutDev& L) -> size_t {
    const SensorDev& S = t.sd[size_t(L.sensor)];
    return frame_lds_doubles(small_map(L, S).P, prim_map(L, S).P1, L.ncols + 1);
  };
  std::vector<char> layout_uses_frames(layouts.size(), 0);
  if (k == 6) {
    std::vector<int64_t> n_obs_l(layouts.size(), 0), n_frames_l(layouts.size(), 0);
    for (int64_t q = 0; q < n_obs;) {
      int64_t e = q;
      while (e < n_obs && keys[e].layout == keys[q].layout && keys[e].seg == keys[q].seg && keys[e].stamp == keys[q].stamp) ++e;
      n_obs_l[size_t(keys[q].layout)] += e - q; n_frames_l[size_t(keys[q].layout)] += 1;
      q = e;
    }
    for (size_t l = 0; l < layouts.size(); ++l)
      layout_uses_frames[l] = p->sensors[size_t(layouts[l].sensor)].kind == CALICO_SENSOR_CAMERA && n_frames_l[l] > 0 &&
                              n_obs_l[l] >= 16 * n_frames_l[l] && layouts[l].ncols + 1 - 36 + 6 <= 30 && layouts[l].c_pt < 0;
  }
  for (int64_t q = 0; q < n_obs;) {
    const ObsKey& kq = keys[q];
    int64_t e = q;
    if (layout_uses_frames[size_t(kq.layout)]) {
      while (e < n_obs && keys[e].layout == kq.layout && keys[e].seg == kq.seg && keys[e].stamp == kq.stamp) ++e;
      if (kq.seg >= t.seg_lo && kq.seg < t.seg_hi) {
        FrameItemDev f;
        f.layout = kq.layout; f.seg = kq.seg; f.obs_begin = int(q); f.obs_count = int(e - q); f.stamp = kq.stamp;
        f.partial_off = int64_t(comp_off);                  // compact record, rebased below
        comp_off += frame_rec(layouts[size_t(kq.layout)]);
        // frames arrive sorted by (layout, segment, stamp): consecutive frames of one cell share one expanded block
        if (cells.empty() || cells.back().layout != kq.layout || cells.back().seg != kq.seg) {
          CellDev c;
          c.layout = kq.layout; c.seg = kq.seg; c.frame_begin = int(fitems.size()); c.frame_count = 0;
          c.partial_off = int64_t(poff); c.prim_off = 0;
          poff += size_t(tri_size(layouts[size_t(kq.layout)].ncols + 1));      // (the block's upper triangle, packed: problem_dev.hpp)
          cells.push_back(c);
        }
        cells.back().frame_count += 1;
        f.cell = int(cells.size()) - 1; f.cell_frames = 0; f.cell_prim_off = 0; f.cell_pad = 0; f.cell_partial_off = 0; f.cell_src_off = 0;   // (filled below)
        fitems.push_back(f);
      }
    } else {
      while (e < n_obs && keys[e].layout == kq.layout) ++e;
    }
    q = e;
  }
  // IMU work items hand their staged rows to the cell kernel ("row cells": one expanded block per (layout, segment)
  // instead of one per item); everything else forms its own block
  // fuse_expand (CALICO_FUSE_EXPAND=0: off): no launch for the cell expansion -- a camera cell is expanded by the last of its
  // frames inside the Jacobian launch (eval_kernels.hip), and the other work items form their blocks themselves, each
  // registered as a cell of its own so that the gather's device-built lists see it. Needs every such (layout, segment) to
  // be ONE work item (an IMU cell of at most kImuChunkItems blocks: the usual case).
  bool fuse = !fitems.empty() && sw.fuse_expand;
  for (const CellDev& c : cells) if (c.frame_count > 2) fuse = false;       // (a workgroup is two waves: one frame each)
  {
    // ... and two waves' staging areas must fit the CU's LDS
    size_t need = 0;
    for (size_t l = 0; l < layouts.size(); ++l) {
      const LayoutDev& L = layouts[l];
      if (layout_uses_frames[l]) need = std::max(need, frame_lds(L));
      else need = std::max(need, size_t((L.ncols + 1 + 15) & ~15) * size_t((((3 * kImuChunkItems + 3) & ~3) + 1) | 1));      // (as lds_cols x row_pad below)
    }
    need = (need + 1) & ~size_t(1);
    if (cells_launch_lds_bytes(need) > kCellsMaxLds) fuse = false;     // (the same bound the kernel's attribute is set to)
    p->pair_wave_lds_doubles = int(need);
  }
  {
    int prev_layout = -1, prev_seg = -1;
    for (const ItemDev& it : t.items) {
      if (layout_uses_frames[size_t(it.layout)]) continue;
      if (it.layout == prev_layout && it.seg == prev_seg) fuse = false;
      if (p->sensors[size_t(layouts[size_t(it.layout)].sensor)].kind == CALICO_SENSOR_CAMERA) fuse = false;     // (camera blocks outside the frame path)
      prev_layout = it.layout; prev_seg = it.seg;
    }
  }
  p->fuse_expand = fuse;
  if (fuse) {
    // two frame entries per workgroup, so that wave w of workgroup g finds its frame at 2 g + w without reading a descriptor
    // first: the two frames of a cell (they expand the cell's block together), or two one-frame cells (`cell_pad` = 1, "solo":
    // each wave expands its own cell alone, no barrier), or a solo frame and an empty entry (obs_count = 0)
    std::vector<FrameItemDev> packed;
    packed.reserve(2 * cells.size());
    std::vector<FrameItemDev> solos;
    for (CellDev& c : cells) {
      if (c.frame_count > 1) {
        FrameItemDev f0 = fitems[size_t(c.frame_begin)], f1 = fitems[size_t(c.frame_begin) + 1];
        f0.cell_pad = f1.cell_pad = 0;
        packed.push_back(f0); packed.push_back(f1);
      } else {
        FrameItemDev f0 = fitems[size_t(c.frame_begin)];
        f0.cell_pad = 1;
        solos.push_back(f0);
      }
    }
    for (size_t i = 0; i < solos.size(); i += 2) {
      packed.push_back(solos[i]);
      FrameItemDev f1 = solos[i];
      if (i + 1 < solos.size()) f1 = solos[i + 1]; else f1.obs_count = 0;
      packed.push_back(f1);
    }
    fitems.swap(packed);
    for (CellDev& c : cells) c.frame_begin = -1;      // (the frames are no longer contiguous by cell: FrameItemDev.cell says whose they are)
  }
  int run = 0;      // (consecutive work items of one cell; the longest run: calico_debug_plan_info)
  p->max_item_run = 0;
  for (ItemDev it : t.items) {
    if (layout_uses_frames[size_t(it.layout)]) continue;
    const LayoutDev& L = layouts[size_t(it.layout)];
    const HSensor& hs = p->sensors[size_t(L.sensor)];
    const int n1 = L.ncols + 1;
    if (fuse) {
      // a cell of one work item that writes the cell's block itself (prim_off = -2: nothing for expand_cells_kernel to do)
      CellDev c;
      c.layout = it.layout; c.seg = it.seg; c.frame_begin = int(jac_items.size()); c.frame_count = 1;
      c.partial_off = int64_t(poff); c.src_off = 0; c.n1 = n1; c.PE = 0; c.prim_off = -2; c.pad0 = 0;
      cells.push_back(c);
      it.rows_off = -2;            // (< 0: the item forms its own block; -2: that block is listed as a cell's)
      it.partial_off = int64_t(poff);
      poff += size_t(tri_size(n1));
    } else if (hs.kind != CALICO_SENSOR_CAMERA && n1 <= 112) {
      it.partial_off = 0; it.rows_off = 0;   // row store offset assigned below, once the staging dimensions are known
      if (cells.empty() || cells.back().prim_off >= 0 || cells.back().layout != it.layout || cells.back().seg != it.seg) {
        CellDev c;
        c.layout = it.layout; c.seg = it.seg; c.frame_begin = int(jac_items.size()); c.frame_count = 0;
        c.partial_off = int64_t(poff); c.src_off = 0; c.n1 = n1; c.PE = hs.dim() * kImuChunkItems; c.prim_off = -1; c.pad0 = 0;
        poff += size_t(tri_size(n1));
        cells.push_back(c);
      }
      cells.back().frame_count += 1;
      cells.back().pad0 += hs.dim() * it.obs_count;
    } else {
      it.rows_off = -1;
      it.partial_off = int64_t(poff);
      poff += size_t(tri_size(n1));
    }
    run = !jac_items.empty() && jac_items.back().layout == it.layout && jac_items.back().seg == it.seg ? run + 1 : 1;
    p->max_item_run = std::max(p->max_item_run, run);
    jac_items.push_back(it);
  }
  p->n_fitems = int(fitems.size());
  p->n_jac_items = int(jac_items.size());
  p->n_cells = int(cells.size());
  // buffer layout: [expanded partial blocks: cells, generic items | item costs (2 per item) | compact frame records]
  const size_t n_cost_slots = 2 * size_t(std::max(std::max(p->n_items, p->n_items_all), p->n_fitems + p->n_jac_items));
  const size_t comp_base = poff + n_cost_slots;
  p->cell_rec_max = 1;
  p->frame_lds_doubles = 0;
  for (FrameItemDev& f : fitems) {
    p->frame_lds_doubles = std::max(p->frame_lds_doubles, int(frame_lds(layouts[size_t(f.layout)])));
    f.partial_off += int64_t(comp_base);
    p->cell_rec_max = std::max(p->cell_rec_max, int(frame_rec(layouts[size_t(f.layout)])));
  }
  p->cell_chunk = std::max(1, int((56 * 1024 / sizeof(double)) / size_t(p->cell_rec_max)));
  // no more LDS than the fullest cell needs: the cell kernel's workgroups should all be resident at once
  p->max_cell_frames = 0;
  for (const CellDev& c : cells) if (c.prim_off >= 0) p->max_cell_frames = std::max(p->max_cell_frames, c.frame_count);   // (camera cells; < 0: IMU cells)
  p->cell_chunk = std::min(p->cell_chunk, std::max(1, p->max_cell_frames));
  // per-layout pair table of the cell kernel: row-major upper triangle of the (c+1)×(c+1) block, each entry with the
  // M_ext element it expands from (prim_of_col: the frame's column order)
  {
    std::vector<int> tab_off(layouts.size(), -1);
    for (CellDev& c : cells) {
      if (c.prim_off < 0) continue;   // row cell
      const LayoutDev& L = layouts[size_t(c.layout)];
      const SensorDev& S = t.sd[size_t(L.sensor)];
      const PrimMap pm = prim_map(L, S);
      const int n1 = L.ncols + 1;
      if (tab_off[size_t(c.layout)] < 0) {
        tab_off[size_t(c.layout)] = int(t.prim_tab.size());
        for (int i = 0; i < n1; ++i)
          for (int j = i; j < n1; ++j)
            t.prim_tab.push_back(i | (j << 8) | ((prim_of_col(L, S, pm, i) * pm.PE + prim_of_col(L, S, pm, j)) << 16));
      }
      c.prim_off = tab_off[size_t(c.layout)]; c.pad0 = 0;
      c.n1 = n1; c.PE = pm.PE;
      c.src_off = c.frame_begin >= 0 ? fitems[size_t(c.frame_begin)].partial_off : 0;      // (no compact records with cell workgroups)
    }
    for (FrameItemDev& fi : fitems) {      // (copies of the cell's fields for the cell's workgroup: fuse_expand)
      const CellDev& c = cells[size_t(fi.cell)];
      fi.cell_frames = c.frame_count; fi.cell_prim_off = c.prim_off; fi.cell_partial_off = c.partial_off; fi.cell_src_off = c.src_off;
    }
  }
  p->partial_doubles = poff;
  if (poff + 2 * size_t(std::max(p->n_items, p->n_fitems + p->n_jac_items)) >= size_t(0x7fffffff))
    return p->set_error(CALICO_UNIMPLEMENTED, "problem too large for 32-bit gather indices");
  {
    // LDS staging of the generic Jacobian kernel: sized by the items that actually go through it
    int jc = 4, jr = 2;
    for (const ItemDev& it : jac_items) {
      const LayoutDev& L = layouts[size_t(it.layout)];
      jc = std::max(jc, L.ncols + 1);
      jr = std::max(jr, p->sensors[size_t(L.sensor)].dim() * it.obs_count);
    }
    // whole groups of sixteen columns and of four rows: stage B reads them without masks (eval_kernels.hip, stage_b_mfma;
    // the padding is cleared by the work item)
    p->lds_cols = (jc + 15) & ~15;
    p->row_pad = (((jr + 3) & ~3) + 1) | 1;
  }
  if (size_t(p->lds_cols) * p->row_pad * sizeof(double) > kMaxLds)
    return p->set_error(CALICO_UNIMPLEMENTED, "too many Jacobian columns per residual block for the LDS staging area");
  // row store of the items that leave [J r]ᵀ[J r] to the cell kernel: behind the compact frame records
  size_t row_store = 0;
  {
    const size_t stride = (size_t(p->lds_cols) * p->row_pad + 1) & ~size_t(1);   // even: the rows travel as 16-byte words
    row_store = (comp_base + comp_off) & 1;                                      // ... from an even offset
    for (ItemDev& it : jac_items) {
      if (it.rows_off < 0) continue;
      it.rows_off = int64_t(comp_base + comp_off + row_store);
      row_store += stride;
    }
    for (CellDev& c : cells)
      if (c.prim_off == -1) c.src_off = jac_items[size_t(c.frame_begin)].rows_off;
    p->row_cell_chunk = std::max(1, int((56 * 1024 / sizeof(double)) / std::max<size_t>(1, stride)));
    int most = 1;
    for (const CellDev& c : cells) if (c.prim_off == -1) most = std::max(most, c.frame_count);
    p->row_cell_chunk = std::min(p->row_cell_chunk, most);
  }
  t.partials_end = comp_base + comp_off + row_store;
  // every work item / frame carries copies of its layout, its sensor and the offsets of its control points
  auto fill = [&](auto& it) {
    it.L = layouts[size_t(it.layout)];
    it.S = t.sd[size_t(it.L.sensor)];
    for (int i = 0; i < 8; ++i) it.ctrl_off[i] = (i < k && it.seg + i < p->n_cp) ? t.ctrl_off[size_t(it.seg + i)] : 0;
  };
  for (ItemDev& it : t.items) fill(it);
  for (ItemDev& it : t.items_all) fill(it);
  for (ItemDev& it : jac_items) fill(it);
  for (FrameItemDev& it : fitems) fill(it);
  return CALICO_OK;
}

// ---- gather lists ----
int plan_gather(calico_problem* p, const PlanSwitches& sw, PlanTables& t) {
  const int k = p->order, n_cp = p->n_cp, m = p->m, NS = 6 * n_cp;
  const std::vector<CellDev>& cells = t.cells; const std::vector<ItemDev>& jac_items = t.jac_items;
  SolveArgs sa; sa.n_cp = n_cp; sa.k = k; sa.mc = m; sa.sep_s = p->sep_s; sa.sep_n = p->sep_n; sa.m = m + p->border_extra(); sa.debug = 0; sa.progress = nullptr;
  const size_t r_size = sa.r_size();
  if (r_size >= size_t(0x7fffffff)) return p->set_error(CALICO_UNIMPLEMENTED, "normal-equation buffer too large");
  p->r_size = r_size;
  struct Pair { int dst, src; };
  std::vector<Pair> pairs;
  const int n_cells = int(cells.size());
  const int n_part = n_cells + p->n_jac_items;     // producers of expanded partial blocks
  // Lists built on the device: when every producer is a cell (camera frames' cells, IMU row cells) and the layouts are
  // few, the sources of the band, the border and the spline part of the right-hand side follow from the outputs' indices
  // (the band is uniform in time): the host uploads three small tables and the device builds those lists itself
  // (launch_gather_lists: count, scan, fill -- the same CSR form the per-iteration gather reads). Only the corner and the
  // calibration part of the right-hand side (2 % of the outputs, sources in every segment) are listed here.
  // CALICO_GATHER_STRUCT=0: everything listed by the host (A/B switch, and the path of problems with free model points or
  // other spline orders' generic items).
  bool gs_ok = sw.gather_struct && int(t.layouts.size()) * k <= 96 && int(t.layouts.size()) >= 1 && m >= 1 && n_cells > 0;
  for (int itn = n_cells; gs_ok && itn < n_part; ++itn) {   // no block of its own, or one that is listed as a cell's (fuse_expand)
    const int64_t ro = jac_items[size_t(itn - n_cells)].rows_off;
    gs_ok = ro >= 0 || ro == -2;
  }
  const int64_t gs_n_out = int64_t(NS) * m + int64_t(n_cp) * k * 36 + NS;
  gs_ok = gs_ok && gs_n_out * 96 < int64_t(0x7fffffff);
  t.gs_ok = gs_ok; t.gs_n_out = gs_n_out;
  std::vector<int>& gs_tab = t.gs_tab; GatherStruct& gsd = t.gsd;
  if (gs_ok) {
    const int n_lay = int(t.layouts.size()), nsg = int(p->valid_knots.size()) - 1;
    gs_tab.assign(size_t(n_lay) * nsg + size_t(n_lay) * m + size_t(n_lay), -1);
    for (const CellDev& c : cells) gs_tab[size_t(c.layout) * nsg + size_t(c.seg)] = int(c.partial_off);
    for (int l = 0; l < n_lay; ++l) {
      const std::vector<int>& gmap = t.layout_gmap[size_t(l)];
      for (size_t q = 0; q < gmap.size(); ++q) gs_tab[size_t(n_lay) * nsg + size_t(l) * m + size_t(gmap[q] - NS)] = 6 * k + int(q);
      gs_tab[size_t(n_lay) * nsg + size_t(n_lay) * m + size_t(l)] = t.layouts[size_t(l)].ncols + 1;
    }
    gsd.n_lay = n_lay; gsd.nseg = nsg; gsd.n_cp = n_cp; gsd.k = k; gsd.m = m;
    {   // band blocks at distance d from the diagonal have (k - d) segments per layout: four lanes in the gather where that is <= 24 sources
      int d4 = k;
      while (d4 > 0 && (k - (d4 - 1)) * n_lay <= 24) --d4;
      gsd.d_split = d4;
    }
    gsd.off_g = sa.off_g(); gsd.off_B = sa.off_B(); gsd.off_E = sa.off_E();
  }
  pairs.reserve(gs_ok ? size_t(n_part) * 256 : p->partial_doubles / 2 + 4 * size_t(p->n_items));
  for (int itn = 0; itn < n_part; ++itn) {
    const bool is_cell = itn < n_cells;
    if (!is_cell && (jac_items[size_t(itn - n_cells)].rows_off >= 0 || jac_items[size_t(itn - n_cells)].rows_off == -2)) continue;   // its block is a cell's
    const int it_layout = is_cell ? cells[size_t(itn)].layout : jac_items[size_t(itn - n_cells)].layout;
    const int it_seg = is_cell ? cells[size_t(itn)].seg : jac_items[size_t(itn - n_cells)].seg;
    const int64_t it_poff = is_cell ? cells[size_t(itn)].partial_off : jac_items[size_t(itn - n_cells)].partial_off;
    const LayoutDev& L = t.layouts[size_t(it_layout)];
    const std::vector<int>& gmap = t.layout_gmap[size_t(it_layout)];
    const int nc = L.ncols, n1 = nc + 1;
    auto tan_of = [&](int c) { return c < 6 * k ? 6 * (it_seg + c / 6) + c % 6 : gmap[size_t(c - 6 * k)]; };
    for (int i = gs_ok ? 6 * k : 0; i < nc; ++i) {      // (structured gather: the spline rows have no lists)
      const int ti = tan_of(i);
      pairs.push_back({int(sa.off_g()) + ti, int(it_poff) + tri_off(i, nc, n1)});
      for (int j = i; j < nc; ++j) {
        const int tj = tan_of(j);
        const int src = int(it_poff) + tri_off(i, j, n1);
        if (ti < NS && tj < NS) {
          const int a = ti / 6, b = tj / 6;  // a <= b
          pairs.push_back({int(sa.off_B()) + (a * k + (b - a)) * 36 + (ti % 6) * 6 + (tj % 6), src});
          if (a == b && ti != tj) pairs.push_back({int(sa.off_B()) + (a * k) * 36 + (tj % 6) * 6 + (ti % 6), src});
        } else if (ti < NS) {
          pairs.push_back({int(sa.off_E() + size_t(ti) * m + (tj - NS)), src});
        } else {
          const int a = ti - NS, b = tj - NS;
          pairs.push_back({int(sa.off_C() + size_t(a) * m + b), src});
          if (a != b) pairs.push_back({int(sa.off_C() + size_t(b) * m + a), src});
        }
      }
    }
  }
  // (outputs 0 and 1 -- cost and invalid count -- are summed by the gather's first workgroup straight from the slot pairs
  //  of the frames and work items behind the partial blocks: no index list)
  // Group the pairs by output, keeping the order in which they were generated inside every group (the summation
  // order of the device's gather, hence its rounding): a counting sort over the outputs -- linear, where a comparison
  // sort of the ~10^6 pairs took most of the set-up time.
  {
    std::vector<int64_t> start(r_size + 1, 0);
    for (const Pair& pr : pairs) ++start[size_t(pr.dst) + 1];
    for (size_t d = 0; d < r_size; ++d) start[d + 1] += start[d];
    std::vector<int> sorted_src(pairs.size());
    {
      std::vector<int64_t> fill(start.begin(), start.end() - 1);
      for (const Pair& pr : pairs) sorted_src[size_t(fill[size_t(pr.dst)]++)] = pr.src;
    }
    // thin outputs: eight lanes, 6 sources per lane -- or 12 when the problem has outputs of 49..96 sources (many
    // layouts: their band and right-hand-side entries would each take a whole wave otherwise)
    int thin_cap = 48;
    if (gs_ok) thin_cap = int(t.layouts.size()) * k <= 48 ? 48 : 96;
    else {
      size_t n_mid = 0;
      for (size_t d = 0; d < r_size; ++d) { const int64_t c = start[d + 1] - start[d]; if (c > 48 && c <= 96) ++n_mid; }
      if (n_mid > 0) thin_cap = 96;
    }
    p->thin_per_lane = thin_cap / 8;
    size_t n_thin_src = 0, n_fat_src = 0;
    for (size_t d = 0; d < r_size; ++d) {
      const int64_t c = start[d + 1] - start[d];
      if (gs_ok || c > thin_cap) n_fat_src += size_t(c); else n_thin_src += size_t(c);
    }
    t.idx_thin.reserve(n_thin_src); t.idx_fat.reserve(n_fat_src);
    for (size_t d = 0; d < r_size; ++d) {
      const int64_t q0 = start[d], q1 = start[d + 1];
      if (q1 == q0) continue;
      const bool fat = gs_ok || (q1 - q0) > thin_cap;        // (the device's lists are the thin ones: what the host lists goes to the waves)
      std::vector<int>& out = fat ? t.out_fat : t.out_thin;
      std::vector<int>& idx = fat ? t.idx_fat : t.idx_thin;
      std::vector<int64_t>& ptr = fat ? t.ptr_fat : t.ptr_thin;
      out.push_back(int(d));
      idx.insert(idx.end(), sorted_src.begin() + q0, sorted_src.begin() + q1);
      ptr.push_back(int64_t(idx.size()));
    }
  }
  p->n_thin = int(t.out_thin.size()); p->n_fat = int(t.out_fat.size());
  p->n_thin8 = p->n_thin; p->n_thin4 = p->n_thin;
  if (gs_ok) {
    p->n_thin = int(gs_n_out);      // (the device's lists: one per output of the band, the border and the spline right-hand side)
    // the border's outputs (behind the right-hand side and the band) have one source per segment and layout that holds
    // their calibration column: at most k where every column belongs to ONE layout -- one lane each in the gather
    bool one_layout = k <= 8;
    for (int tc = 0; one_layout && tc < m; ++tc) {
      int holders = 0;
      for (int l = 0; l < gsd.n_lay; ++l) holders += gs_tab[size_t(gsd.n_lay) * gsd.nseg + size_t(l) * m + size_t(tc)] >= 0 ? 1 : 0;
      one_layout = holders <= 1;
    }
    const int n_border0 = NS + n_cp * k * 36;          // first border output
    p->n_thin4 = one_layout ? n_border0 : p->n_thin;
    // band blocks at distance d from the diagonal have (k - d) segments per layout: four lanes where that is <= 24 sources
    const int d4 = gsd.d_split;
    p->n_thin8 = one_layout ? std::min(n_border0, NS + d4 * n_cp * 36) : p->n_thin;     // (the classes are ranges: [8 | 4 | 1])
  }
  // the thin outputs' lists at a fixed stride per lane class: the gather then needs no pointer load in front of its index
  // loads
  // Only for the device-built lists: their lengths are bounded by the structure (layouts x k <= thin_per_lane x 8 per output),
  // which is what the fixed stride relies on; host-built lists (plans the table cannot describe) keep the CSR form -- padding
  // each of their short lists to 48 / 96 slots would multiply the index memory, and nothing bounds their length.
  p->gather_fixed = p->n_thin > 0 && gs_ok;
  // a word of the partials nobody writes (allocated and cleared with them): what padded list entries point to. The lists
  // hold 32-bit positions, so the whole partials buffer must be addressable by one -- checked for every kind of list
  if (t.partials_end + 2 >= size_t(0x7fffffff)) return p->set_error(CALICO_UNIMPLEMENTED, "problem too large for 32-bit gather indices");
  p->partials_alloc = t.partials_end + 2;      // (+ the word that is always zero: the lists' zero_slot)
  return CALICO_OK;
}

// ---- upload of the structure: the only stage that talks to the device ----
int upload_plan(calico_problem* p, PlanTables& t) {
  hipStream_t s = p->stream;
  HIP_TRY(p, p->d_knots.upload(p->knots, s)); HIP_TRY(p, p->d_basis.upload(p->basis, s));
  HIP_TRY(p, p->d_ctrl_off.upload(t.ctrl_off, s));
  HIP_TRY(p, p->d_stamp.upload(t.st, s)); HIP_TRY(p, p->d_point_off.upload(t.point_off, s));
  HIP_TRY(p, p->d_sensors.upload(t.sd, s)); HIP_TRY(p, p->d_layouts.upload(t.layouts, s));
  HIP_TRY(p, p->d_items.upload(t.items, s)); HIP_TRY(p, p->d_items_all.upload(t.items_all, s));
  HIP_TRY(p, p->d_jac_items.upload(t.jac_items, s)); HIP_TRY(p, p->d_fitems.upload(t.fitems, s));
  HIP_TRY(p, p->d_blocks.upload(p->h_blocks, s));
  HIP_TRY(p, p->d_cp_active.upload(t.cp_active, s));
  DevBuf<int> d_cnt;                    // (scratch of the device's list build; freed behind the synchronisation below)
  DevBuf<long long> d_scan;
  const int zero_slot = int(t.partials_end);
  if (t.gs_ok) {
    HIP_TRY(p, p->d_gs_tab.upload(t.gs_tab, s));
    t.gsd.tab = p->d_gs_tab.p;
    const size_t n_out = size_t(t.gs_n_out), per_out = t.layouts.size() * size_t(p->order);      // (<= 96)
    HIP_TRY(p, p->d_out_thin.alloc(n_out)); HIP_TRY(p, p->d_ptr_thin.alloc(n_out + 1));
    HIP_TRY(p, p->d_idx_thin.alloc(n_out * per_out)); HIP_TRY(p, d_cnt.alloc(n_out));
    HIP_TRY(p, d_scan.alloc(n_out / 1024 + 2));      // block sums of the lists' prefix scan
    launch_gather_lists(t.gsd, int(n_out), d_cnt.p, p->d_out_thin.p, p->d_ptr_thin.p, p->d_idx_thin.p, zero_slot, d_scan.p, s);
  } else {
    HIP_TRY(p, p->d_out_thin.upload(t.out_thin, s)); HIP_TRY(p, p->d_idx_thin.upload(t.idx_thin, s));
    HIP_TRY(p, p->d_ptr_thin.upload(t.ptr_thin, s));
  }
  HIP_TRY(p, p->d_out_fat.upload(t.out_fat, s)); HIP_TRY(p, p->d_idx_fat.upload(t.idx_fat, s));
  HIP_TRY(p, p->d_ptr_fat.upload(t.ptr_fat, s));
  if (p->gather_fixed) {
    HIP_TRY(p, p->d_idx_fixed.alloc(gather_fixed_entries(p->n_thin, p->n_thin8, p->n_thin4, p->thin_per_lane) + 8));
    launch_gather_pack_fixed(p->d_ptr_thin.p, p->d_idx_thin.p, p->n_thin, p->n_thin8, p->n_thin4, p->thin_per_lane, zero_slot, p->d_idx_fixed.p, s);
  }
  HIP_TRY(p, p->d_cells.upload(t.cells, s)); HIP_TRY(p, p->d_prim_tab.upload(t.prim_tab, s));
  HIP_TRY(p, p->d_pred_map.upload(t.pred_map, s));
  if (p->use_bcr) {
    HIP_TRY(p, p->d_bnodes.upload(p->h_bcr_nodes, s)); HIP_TRY(p, p->d_bkeep.upload(t.bcr_keep, s));
    HIP_TRY(p, p->d_cp_block.upload(t.cp_block, s));
  }
  HIP_TRY(p, hipStreamSynchronize(s));      // the uploads read the caller's PlanTables
  return CALICO_OK;
}

int build_plan(calico_problem* p, const PlanSwitches& sw, SetupTimer& setup) {
  PlanTables t;
  int rc = plan_blocks(p, sw, t);
  if (rc != CALICO_OK) return rc;
  setup.section("blocks / tangent order");
  plan_layouts(p, t);
  setup.section("layouts");
  plan_items(p, t);
  setup.section("sort + work items");
  rc = plan_route(p, sw, t);
  if (rc != CALICO_OK) return rc;
  setup.section("evaluation route");
  rc = plan_gather(p, sw, t);
  if (rc != CALICO_OK) return rc;
  setup.section("gather lists");
  const SolveArgs sa = make_solve_args(p);       // (the solvers' LDS windows)
  if (band_cholesky_lds_bytes(sa) > kMaxLds) return p->set_error(CALICO_UNIMPLEMENTED, "spline order too high for the banded factorisation window");
  p->dense_in_lds = reduced_solve_lds_bytes(sa) <= kMaxLds - 1024;
  if (band_backsolve_lds_bytes(sa) > kMaxLds) return p->set_error(CALICO_UNIMPLEMENTED, "trajectory too long for the back-substitution window");
  if (p->use_bcr && (bcr_level_lds_bytes() > kMaxLds || bcr_back_lds_bytes(p->bcr_q_max, p->bcr_m1p) > kMaxLds))
    return p->set_error(CALICO_UNIMPLEMENTED, "tree solver workspace exceeds the LDS");
  rc = upload_plan(p, t);
  if (rc != CALICO_OK) return rc;
  setup.section("structure uploads");
  return CALICO_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Plan cache. The reference rebuilds its ceres::Problem on every Optimize() (batch_optimizer.cpp:57-70); rebuilt here,
// the flattening would cost more than the solve it feeds. What finalize derives depends on the STRUCTURE of the problem
// only -- block sizes / manifolds / constancy, the spline's knots and basis, the sensors' models, blocks, noise and loss
// settings, and per observation its stamp, rigid body and model point -- so it is keyed on a 128-bit hash of exactly
// that and shared: a handle whose structure has been seen before adopts the cached plan (views of its device buffers)
// and a pooled workspace, and only uploads its values. A changed structure hashes differently and is planned afresh.
// CALICO_PLAN_CACHE=0 switches the cache off; calico_plan_cache_clear() empties it.
// ---------------------------------------------------------------------------------------------------------------------
struct PlanKey {
  uint64_t h1 = 0, h2 = 0; size_t n_blocks = 0, n_obs = 0; int device = 0;
  bool operator==(const PlanKey& o) const { return h1 == o.h1 && h2 == o.h2 && n_blocks == o.n_blocks && n_obs == o.n_obs && device == o.device; }
};
}  // namespace
struct PlanEntry {
  PlanKey key;
  PlanHost host;
  PlanDev dev;
  // per parameter block / per sensor: what finalize writes into the handle's own tables
  struct BlockMeta { int amb_off, tan, eff; bool used; };
  std::vector<BlockMeta> block_meta;
  struct SensorMeta { std::vector<int64_t> sorted_pos; int64_t sorted_begin, sorted_end; };
  std::vector<SensorMeta> sensor_meta;
  std::vector<std::unique_ptr<Workspace>> pool;     // workspaces of destroyed handles, ready for the next one
  uint64_t last_use = 0;
};
namespace {
struct PlanCache {
  std::mutex mu;
  std::vector<std::shared_ptr<PlanEntry>> entries;
  uint64_t tick = 0;
  int64_t hits = 0, misses = 0;
  static constexpr size_t kMaxEntries = 8, kMaxPool = 2;
};
// (never destroyed, like the stream and pinned pools: its buffers would be freed after the HIP runtime is gone)
PlanCache& plan_cache() { static PlanCache* c = new PlanCache; return *c; }
bool plan_cache_enabled() {
  static const bool on = env_flag("CALICO_PLAN_CACHE", true);
  return on;
}
struct Hasher {
  uint64_t a = 0x9E3779B97F4A7C15ull, b = 0xC2B2AE3D27D4EB4Full;
  void word(uint64_t w) {
    a = (a ^ w) * 0xff51afd7ed558ccdull; a ^= a >> 32;
    b = (b + w) * 0xc4ceb9fe1a85ec53ull; b ^= b >> 29;
  }
  void bytes(const void* p, size_t n) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    size_t i = 0;
    if (n >= 256) {
      // long arrays (stamps, ids): four independent lanes of 64-bit words, folded into the two running mixes -- the
      // single multiply chain above hashes at the latency of its multiplications, not at memory speed
      uint64_t l0 = 0x243F6A8885A308D3ull, l1 = 0x13198A2E03707344ull, l2 = 0xA4093822299F31D0ull, l3 = 0x082EFA98EC4E6C89ull;
      for (; i + 32 <= n; i += 32) {
        uint64_t w[4];
        std::memcpy(w, c + i, 32);
        l0 = (l0 ^ w[0]) * 0xff51afd7ed558ccdull; l0 ^= l0 >> 32;
        l1 = (l1 ^ w[1]) * 0xc4ceb9fe1a85ec53ull; l1 ^= l1 >> 29;
        l2 = (l2 ^ w[2]) * 0x9E3779B97F4A7C15ull; l2 ^= l2 >> 31;
        l3 = (l3 ^ w[3]) * 0xD6E8FEB86659FD93ull; l3 ^= l3 >> 30;
      }
      word(l0); word(l1); word(l2); word(l3);
    }
    for (; i + 8 <= n; i += 8) { uint64_t w; std::memcpy(&w, c + i, 8); word(w); }
    if (i < n) { uint64_t w = 0; std::memcpy(&w, c + i, n - i); word(w ^ (uint64_t(n - i) << 56)); }
  }
  template <class T> void vec(const std::vector<T>& v) { word(v.size()); bytes(v.data(), v.size() * sizeof(T)); }
  void dbl(double d) { uint64_t w; std::memcpy(&w, &d, 8); word(w); }
};
PlanKey structure_key(const calico_problem* p, const PlanSwitches& sw) {
  Hasher h;
  h.word(uint64_t(p->order)); h.vec(p->knots); h.vec(p->basis); h.vec(p->ctrl);
  h.word(uint64_t(p->rank)); h.word(uint64_t(p->world));
  h.word(p->blocks.size());
  for (const HBlock& b : p->blocks) h.word(uint64_t(b.size) | (uint64_t(b.manifold) << 32) | (uint64_t(b.constant) << 40));
  h.word(p->bodies.size());
  for (const HBody& b : p->bodies) h.word(uint64_t(uint32_t(b.q)) | (uint64_t(uint32_t(b.t)) << 32));
  h.word(p->sensors.size());
  size_t n_obs = 0;
  for (const HSensor& s : p->sensors) {
    h.word(uint64_t(s.kind) | (uint64_t(s.model) << 8) | (uint64_t(s.K) << 16) | (uint64_t(s.loss) << 32));
    h.word(uint64_t(uint32_t(s.intr)) | (uint64_t(uint32_t(s.q)) << 32)); h.word(uint64_t(uint32_t(s.t)) | (uint64_t(uint32_t(s.lat)) << 32));
    h.word(uint64_t(uint32_t(s.grav)));
    h.dbl(s.sigma); h.dbl(s.info); h.dbl(s.loss_scale);
    h.vec(s.stamps); h.vec(s.body); h.vec(s.point);
    n_obs += s.stamps.size();
  }
  h.word(uint64_t(sw.band_solver) | (uint64_t(sw.speculative) << 1) | (uint64_t(sw.band_split) << 2) | (uint64_t(sw.fuse_expand) << 3) |
         (uint64_t(sw.gather_struct) << 4) | (uint64_t(sw.bcr_leaf) << 8));
  PlanKey k; k.h1 = h.a; k.h2 = h.b; k.n_blocks = p->blocks.size(); k.n_obs = n_obs; k.device = p->device;
  return k;
}

// A handle adopts a cached plan: copies of the host-side plan, views of the device-side structure.
void adopt_plan(calico_problem* p, const std::shared_ptr<PlanEntry>& e) {
  static_cast<PlanHost&>(*p) = e->host;
  static_cast<PlanDev&>(*p).alias_from(e->dev);
  for (size_t i = 0; i < p->blocks.size(); ++i) {
    const PlanEntry::BlockMeta& bm = e->block_meta[i];
    p->blocks[i].amb_off = bm.amb_off; p->blocks[i].tan = bm.tan; p->blocks[i].eff = bm.eff; p->blocks[i].used = bm.used;
  }
  for (size_t i = 0; i < p->sensors.size(); ++i) {
    p->sensors[i].sorted_pos = e->sensor_meta[i].sorted_pos;
    p->sensors[i].sorted_begin = e->sensor_meta[i].sorted_begin; p->sensors[i].sorted_end = e->sensor_meta[i].sorted_end;
  }
  p->plan = e;
}

// Everything a handle works in, sized by the plan: a pooled workspace of the same plan if there is one, else allocated
// (and the parts the kernels expect zero-filled cleared) here.
int prepare_workspace(calico_problem* p) {
  hipStream_t s = p->stream;
  if (p->plan) {
    std::unique_ptr<Workspace> w;
    {
      std::lock_guard<std::mutex> lock(plan_cache().mu);
      if (!p->plan->pool.empty()) { w = std::move(p->plan->pool.back()); p->plan->pool.pop_back(); }
    }
    if (w) { static_cast<Workspace&>(*p).swap_ws(*w); p->active_dirty = true; p->xc_stale = true; return CALICO_OK; }   // (w takes the handle's old one along)
  }
  const int n_cp = p->n_cp, m = p->m, k = p->order, NS = 6 * n_cp;
  const int64_t n_obs = p->n_obs;
  const size_t r_size = p->r_size;
  HIP_TRY(p, p->d_x.alloc(size_t(p->n_amb))); HIP_TRY(p, p->d_xc.alloc(size_t(p->n_amb)));
  HIP_TRY(p, p->d_m0.alloc(size_t(n_obs))); HIP_TRY(p, p->d_m1.alloc(size_t(n_obs))); HIP_TRY(p, p->d_m2.alloc(size_t(n_obs)));
  HIP_TRY(p, p->d_partials.alloc(p->partials_alloc));
  HIP_TRY(p, hipMemsetAsync(p->d_partials.p + (p->partials_alloc - 2), 0, 2 * sizeof(double), s));      // the word the lists point to for "nothing"
  if (env_int("CALICO_KERNEL_TIMING", 0, 0) >= 3) HIP_TRY(p, p->d_wave_log.alloc(2 * size_t(p->n_jac_items + p->n_fitems) + 8));
  // Behind the second reduce buffer: what the tree solver's rolling chief (bcr_level_kernel, ROLL) reads and masks past the
  // band of the last superblock I = N - 1. Its lanes load at I·strideB + (g_roll_tab offset) and select afterwards; the offsets
  // reach (6k - 1)·36 + 11 doubles into a superblock's storage (rows 30 and 31 of the 32-row tiles count as control point 5,
  // the Bᵀ rows' column at most 31), i.e. (5N + 1 - n_cp)·k·36 - 24 <= 5·k·36 - 24 doubles past the band's end (5N - n_cp
  // <= 4). In buffer 0 that lands in E / C / buffer 1; in buffer 1 it lands here when E and C are short (mc == 0).
  const size_t r_pad = p->use_bcr ? size_t(kBcrCps) * size_t(k) * 36 : 0;
  HIP_TRY(p, p->d_R.alloc(2 * r_size + r_pad)); HIP_TRY(p, hipMemsetAsync(p->d_R.p, 0, (2 * r_size + r_pad) * sizeof(double), s));
  HIP_TRY(p, p->d_R2.alloc(2));
  const int NT = 6 * n_cp + m;
  const int mw = m + p->border_extra();     // border width the solver kernels work with
  HIP_TRY(p, p->d_Lb.alloc(size_t(NS) * 6 * k)); HIP_TRY(p, p->d_Linv.alloc(size_t(n_cp) * 36));
  HIP_TRY(p, p->d_Y.alloc(size_t(NS) * (mw + 1)));
  HIP_TRY(p, p->d_S.alloc(size_t(mw + 1) * (mw + 1)));
  HIP_TRY(p, p->d_y.alloc(size_t(NT) + p->border_extra() + 64)); HIP_TRY(p, p->d_zbuf.alloc(size_t(NS) + 64)); HIP_TRY(p, p->d_dadd.alloc(NT)); HIP_TRY(p, p->d_scale.alloc(2 * size_t(NT)));      // [Jacobi scale s | 1 / s^2]
  HIP_TRY(p, p->d_res.alloc(size_t(n_obs) * 3)); HIP_TRY(p, p->d_valid.alloc(size_t(n_obs)));
  HIP_TRY(p, p->d_active.alloc(size_t(n_obs))); HIP_TRY(p, p->d_counter.alloc(1));
  p->active_dirty = true; p->xc_stale = true;
  HIP_TRY(p, p->d_state.alloc(1)); HIP_TRY(p, p->d_log.alloc(kLogCap));
  // fine-grained (coherent): the terminating stage of a solve writes its results here and the host reads them while
  // later kernels are still on the stream
  if (!p->h_state) {
    HIP_TRY(p, hipHostMalloc(reinterpret_cast<void**>(&p->h_state), sizeof(LmState), hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(p->h_state, 0, sizeof(LmState));
  }
  if (!p->h_log) HIP_TRY(p, hipHostMalloc(reinterpret_cast<void**>(&p->h_log), size_t(kLogCap) * sizeof(IterLog), hipHostMallocMapped | hipHostMallocCoherent));
  if (p->h_xpin_n < size_t(p->n_amb)) {
    if (p->h_xpin) (void)hipHostFree(p->h_xpin);
    p->h_xpin = nullptr; p->h_xpin_n = 0;
    HIP_TRY(p, hipHostMalloc(reinterpret_cast<void**>(&p->h_xpin), std::max<size_t>(1, size_t(p->n_amb)) * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    p->h_xpin_n = size_t(p->n_amb);
  }
  if (!p->h_progress) {
    HIP_TRY(p, hipHostMalloc(reinterpret_cast<void**>(&p->h_progress), 64, hipHostMallocMapped | hipHostMallocCoherent));   // fine-grained: the host polls it while kernels run
    HIP_TRY(p, hipHostGetDevicePointer(reinterpret_cast<void**>(&p->d_progress), p->h_progress, 0));
    std::memset(p->h_progress, 0, 64);     // epoch 0 is never used: words of "no solve yet"
  }
  const SolveArgs sa = make_solve_args(p);
  const size_t reduced_lds = reduced_solve_lds_bytes(sa);
  HIP_TRY(p, p->d_Spart.alloc(size_t(mw + 1 <= 128 ? 8 : 4) * size_t(mw + 1) * (mw + 1) + 64));   // up to eight K-slices of the Schur complement (long trajectories; four for the blocked path) (+ slack: the blocked factorisation reads whole 32-column panels)
  HIP_TRY(p, p->d_Swork.alloc(std::max<size_t>(reduced_lds / sizeof(double) + 8, size_t(mw + 1) * 16 * 13 + 8)));
  if (p->use_bcr) {
    const size_t N = size_t(p->bcr_N), bb = size_t(kBcrBP) * kBcrBP, fb = size_t(kBcrBP) * p->bcr_m1p;
    HIP_TRY(p, p->d_bD.alloc(N * bb)); HIP_TRY(p, p->d_bG.alloc(2 * N * bb)); HIP_TRY(p, p->d_bF.alloc(N * fb));
    HIP_TRY(p, p->d_bpD.alloc(4 * N * bb)); HIP_TRY(p, p->d_bpF.alloc(4 * N * fb));
    HIP_TRY(p, p->d_bM.alloc(N * bb)); HIP_TRY(p, p->d_bZA.alloc(N * bb)); HIP_TRY(p, p->d_bZB.alloc(N * bb));
    HIP_TRY(p, p->d_bY.alloc(N * fb)); HIP_TRY(p, p->d_bysol.alloc(N * kBcrBP)); HIP_TRY(p, p->d_bzb.alloc(N * kBcrBP)); HIP_TRY(p, p->d_bupd.alloc(size_t(p->bcr_slots) * 4));
    HIP_TRY(p, hipMemsetAsync(p->d_bY.p, 0, N * fb * sizeof(double), s));       // rows of the root are never written
    HIP_TRY(p, hipMemsetAsync(p->d_bG.p, 0, 2 * N * bb * sizeof(double), s));
    HIP_TRY(p, hipMemsetAsync(p->d_bpD.p, 0, 4 * N * bb * sizeof(double), s)); HIP_TRY(p, hipMemsetAsync(p->d_bpF.p, 0, 4 * N * fb * sizeof(double), s));
    HIP_TRY(p, hipMemsetAsync(p->d_bupd.p, 0, size_t(p->bcr_slots) * 4 * sizeof(double), s));
    HIP_TRY(p, p->d_handoff.alloc(8)); HIP_TRY(p, hipMemsetAsync(p->d_handoff.p, 0, 8 * sizeof(int), s));
    p->handoff_seq = 0;
  }
  p->ws_ready = true;
  return CALICO_OK;
}

// Pinned staging buffers for the measurement upload, shared by all handles of the process: a handle holds one from
// upload_values to the synchronisation at the end of finalize (hipHostMalloc costs more than the upload it speeds up).
struct PinnedPool {
  std::mutex mu;
  std::vector<std::pair<double*, size_t>> idle;
  double* acquire(size_t n, size_t* cap) {
    {
      std::lock_guard<std::mutex> lock(mu);
      for (size_t i = 0; i < idle.size(); ++i)
        if (idle[i].second >= n) { double* q = idle[i].first; *cap = idle[i].second; idle.erase(idle.begin() + long(i)); return q; }
    }
    double* q = nullptr;
    const size_t c = n + n / 4;       // (some slack: the next structure is often a little larger)
    if (hipHostMalloc(reinterpret_cast<void**>(&q), c * sizeof(double), hipHostMallocDefault) != hipSuccess) return nullptr;
    *cap = c;
    return q;
  }
  void release(double* q, size_t cap) {
    if (!q) return;
    std::lock_guard<std::mutex> lock(mu);
    if (idle.size() < 2) { idle.emplace_back(q, cap); return; }
    size_t small = 0;
    for (size_t i = 1; i < idle.size(); ++i) if (idle[i].second < idle[small].second) small = i;
    if (idle[small].second < cap) { (void)hipHostFree(idle[small].first); idle[small] = {q, cap}; }
    else (void)hipHostFree(q);
  }
};
PinnedPool& pinned_pool() { static PinnedPool* pp = new PinnedPool(); return *pp; }

// The values: measurements in the device's (sorted) order, parameter vector.
int upload_values(calico_problem* p) {
  hipStream_t s = p->stream;
  const size_t n = size_t(std::max<int64_t>(p->n_obs, 1));
  // pinned staging (part of the workspace, so a pooled one brings it along): the three copies below are DMA transfers
  // that return at once, where pageable vectors went through the runtime's bounce buffers synchronously
  if (p->h_mpin && p->h_mpin_n < 3 * n) { pinned_pool().release(p->h_mpin, p->h_mpin_n); p->h_mpin = nullptr; p->h_mpin_n = 0; }
  if (!p->h_mpin) {
    p->h_mpin = pinned_pool().acquire(3 * n, &p->h_mpin_n);
    if (!p->h_mpin) return p->set_error(CALICO_INTERNAL, "hipHostMalloc (measurement staging) failed");
  }
  double* m0 = p->h_mpin; double* m1 = m0 + n; double* m2 = m1 + n;
  for (const HSensor& sn : p->sensors) {
    const int dim = sn.dim();
    const int64_t ns = sn.n();
    const double* me = sn.meas.data();
    const int64_t* sp = sn.sorted_pos.data();
    if (dim == 2) for (int64_t i = 0; i < ns; ++i) { const size_t q = size_t(sp[i]); m0[q] = me[2 * i]; m1[q] = me[2 * i + 1]; m2[q] = 0.0; }
    else for (int64_t i = 0; i < ns; ++i) { const size_t q = size_t(sp[i]); m0[q] = me[3 * i]; m1[q] = me[3 * i + 1]; m2[q] = me[3 * i + 2]; }
  }
  if (p->n_obs > 0) {
    HIP_TRY(p, hipMemcpyAsync(p->d_m0.p, m0, size_t(p->n_obs) * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(p, hipMemcpyAsync(p->d_m1.p, m1, size_t(p->n_obs) * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(p, hipMemcpyAsync(p->d_m2.p, m2, size_t(p->n_obs) * sizeof(double), hipMemcpyHostToDevice, s));
  }
  p->h_x.assign(size_t(p->n_amb), 0.0);
  for (const HBlock& b : p->blocks) std::copy(b.v.begin(), b.v.end(), p->h_x.begin() + b.amb_off);
  if (p->n_amb > 0) {
    HIP_TRY(p, hipMemcpyAsync(p->d_x.p, p->h_x.data(), p->h_x.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(p, hipMemcpyAsync(p->d_xc.p, p->h_x.data(), p->h_x.size() * sizeof(double), hipMemcpyHostToDevice, s));
  }
  return CALICO_OK;
}

int configure_kernels(calico_problem* p) {
  const SolveArgs sa = make_solve_args(p);
  const size_t reduced_lds = reduced_solve_lds_bytes(sa);
  // The kernels' dynamic-LDS limits depend on a handful of sizes. They are only ever RAISED on a device (two live handles
  // of different shapes must not lower each other's limits), and the forty-odd hipFuncSetAttribute calls (0.3 ms) are
  // skipped when the device already allows what this handle needs -- every handle of a known structure, and most others.
  const bool db_fits = p->use_bcr && std::max(dense_block_solve_lds_bytes(), bcr_back_lds_bytes(std::min(p->bcr_q_max, 4), p->bcr_m1p)) + 1024 <= kMaxLds;
  const std::array<size_t, 8> want = {size_t(p->lds_cols) * p->row_pad * sizeof(double), band_cholesky_lds_bytes(sa),
                                      p->dense_in_lds ? reduced_lds : 0, band_backsolve_lds_bytes(sa), size_t(p->use_bcr ? 1 : 0),
                                      size_t(p->use_bcr ? p->bcr_q_max : 0), size_t(p->use_bcr ? p->bcr_m1p : 0),
                                      db_fits ? dense_back_lds_bytes(std::min(p->bcr_q_max, 4), p->bcr_m1p) : 0};
  static std::mutex mu;
  static std::map<int, std::array<size_t, 8>> allowed;
  std::lock_guard<std::mutex> lock(mu);
  std::array<size_t, 8>& cur = allowed[p->device];       // (zeros for a device seen for the first time)
  std::array<size_t, 8> nw;
  for (size_t i = 0; i < nw.size(); ++i) nw[i] = std::max(cur[i], want[i]);
  if (nw == cur) return CALICO_OK;
  HIP_TRY(p, configure_eval_kernels(nw[0]));
  HIP_TRY(p, configure_solve_kernels(nw[1], nw[2], nw[3]));
  HIP_TRY(p, configure_dense_block_solve());
  HIP_TRY(p, configure_reduced_block_step());
  if (nw[4]) HIP_TRY(p, configure_bcr_kernels(int(nw[5]), int(nw[6])));
  if (nw[7]) HIP_TRY(p, configure_dense_back_bytes(nw[7]));
  cur = nw;
  return CALICO_OK;
}

int do_allreduce(calico_problem* p, double* buf, int64_t n) {
  if (p->comm) {     // native: one in-place RCCL all-reduce on the handle's stream, no host code in between
    const ncclResult_t r = rccl().AllReduce(buf, buf, size_t(n), ncclDouble, ncclSum, p->comm, p->stream);
    if (r != ncclSuccess) return p->set_error(CALICO_INTERNAL, std::string("ncclAllReduce: ") + rccl().GetErrorString(r));
    return CALICO_OK;
  }
  if (!p->allreduce) return CALICO_OK;
  const int st = p->allreduce(p->allreduce_ctx, buf, n, p->stream);
  if (st != 0) return p->set_error(CALICO_INTERNAL, "all-reduce callback failed");
  return CALICO_OK;
}

static bool end_hint_available(const calico_problem* p) { return p->order == 6 && p->n_fitems > 0; }

// What one linear solve does, from the plan and the switches read per solve: enqueue_linear_solve follows it,
// calico_debug_plan_info reports it (one decision, so the hook cannot drift from what runs).
struct LinearRoute {
  int ks = 1;                 // K-slices of the Schur complement (reduced_schur_slices)
  int reduced = 0;            // ReducedRoute of the reduced solve
  bool reduced_in_lds = true; // kReducedKernel: works in LDS (else in Swork)
  // tree solver only:
  bool schur_rides = false;   // the Schur complement rides in the last level's launch
  BcrTopSeps ts = {};         // top separators back-substituted in the launch of the level below (ts.n of them)
  int l_first = 0;            // level of the first back-substitution launch behind the reduced solve
  bool fused = false;         // the dense solve and that back-substitution share one launch (dense_back_kernel)
};
LinearRoute linear_route(const calico_problem* p, const SolveArgs& sa) {
  LinearRoute r;
  r.ks = reduced_schur_slices(sa);
  r.reduced = reduced_solve_route(sa);
  r.reduced_in_lds = p->dense_in_lds;
  if (!p->use_bcr || p->bcr_levels.empty()) return r;
  const int L = int(p->bcr_levels.size());
  // The Schur complement rides in the last level's launch (its tiles over the rows eliminated below that level run beside
  // the level's chains; the level's own rows and the root's rows follow an in-launch fan-in): one launch less. Trees of at
  // least two levels, whose last level has one or two single-superblock nodes by construction of the plan; one-level trees
  // launch bcr_schur_kernel on its own.
  const BcrLevel& last = p->bcr_levels[size_t(L - 1)];
  r.schur_rides = L >= 2 && last.n_nodes >= 1 && last.n_nodes <= 2 && p->bcr_root >= 0;
  for (int i = 0; r.schur_rides && i < last.n_nodes; ++i) r.schur_rides = p->h_bcr_nodes[size_t(last.node0 + i)].q == 1;
  // The top level of the tree is one or two single superblocks next to the root: their back-substitution rides in the
  // launch of the level below (every node there solves the top separators beside it itself -- a few more loads next to
  // the ones it waits for anyway) instead of costing a launch of its own.
  if (L >= 2) {
    const BcrLevel& tl = p->bcr_levels[size_t(L - 1)];
    bool ok = tl.n_nodes <= 2 && p->bcr_levels[size_t(L - 2)].q_max <= 4;
    for (int i = 0; ok && i < tl.n_nodes; ++i) {
      const BcrNodeDev& nd = p->h_bcr_nodes[size_t(tl.node0 + i)];
      ok = nd.q == 1 && (nd.left < 0 || nd.left == p->bcr_root) && (nd.right < 0 || nd.right == p->bcr_root);
      r.ts.blk[i] = nd.blk0; r.ts.left[i] = nd.left; r.ts.right[i] = nd.right;
    }
    r.ts.n = ok ? tl.n_nodes : 0;
  }
  // The first back-substitution launch rides in the launch of the dense reduced solve where the shapes allow it (the
  // nodes fetch what they need while the solve runs and take its solution over a hand-off word: dense_back_kernel).
  r.l_first = r.ts.n > 0 ? L - 2 : L - 1;
  const BcrLevel& lf = p->bcr_levels[size_t(r.l_first)];
  r.fused = r.l_first == 0 && dense_back_fusable(sa, r.ks, lf.q_max, /*border_rows=*/r.l_first > 0) &&
            std::max(dense_block_solve_lds_bytes(), bcr_back_lds_bytes(lf.q_max, p->bcr_m1p)) + 1024 <= kMaxLds;
  return r;
}

int read_state(calico_problem* p) {
  HIP_TRY(p, hipMemcpyAsync(p->h_state, p->d_state.p, sizeof(LmState), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(p, hipStreamSynchronize(p->stream));
  p->timer.resolve();
  return CALICO_OK;
}

void fill_counts(calico_problem* p, calico_summary* sm) {
  int nrb = 0, nr = 0;
  for (HSensor& s : p->sensors) {   // tagged outliers are not part of the problem (camera.cpp:121-124)
    if (s.n_active < 0) { int64_t c = 0; for (uint8_t a : s.active) c += a ? 1 : 0; s.n_active = c; }   // per solve otherwise: 100k bytes
    const int64_t na = s.n_active;
    nrb += int(na); nr += int(na) * s.dim();
  }
  sm->num_residual_blocks = nrb; sm->num_residuals = nr;
  sm->num_residual_blocks_reduced = nrb; sm->num_residuals_reduced = nr;
  sm->num_parameter_blocks = int(p->blocks.size());
  int np = 0, ne = 0, npr = 0;
  for (const HBlock& b : p->blocks) { np += b.size; ne += b.tangent_size(); }
  sm->num_parameters = np; sm->num_effective_parameters = ne;
  sm->num_parameter_blocks_reduced = int(p->h_blocks.size());
  for (const BlockDev& b : p->h_blocks) npr += b.size;
  sm->num_parameters_reduced = npr;
  sm->num_effective_parameters_reduced = p->n_eff;
}

const char* reason_message(int reason) {
  switch (reason) {
    case 1: return "Maximum number of iterations reached.";
    case 2: return "Gradient tolerance reached.";
    case 3: return "Minimum trust region radius reached.";
    case 4: return "Parameter tolerance reached.";
    case 5: return "Function tolerance reached.";
    case 10: return "Initial residual and Jacobian evaluation failed.";
    case 11: return "Residual and Jacobian evaluation failed.";
    case 12: return "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps.";
    default: return "";
  }
}

}  // namespace

// ---- what analysis.cpp calls as well (declared in problem_host.hpp) ----
namespace cal {

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

SolveArgs make_solve_args(calico_problem* p) {
  SolveArgs a;
  a.R = p->d_R.p; a.r_stride = p->speculative ? p->r_size : 0; a.Lb = p->d_Lb.p; a.Linv = p->d_Linv.p; a.Y = p->d_Y.p; a.S = p->d_S.p; a.Spart = p->d_Spart.p;
  a.Swork = p->d_Swork.p; a.y = p->d_y.p; a.zbuf = p->d_zbuf.p; a.dadd = p->d_dadd.p;
  a.scale = p->d_scale.p; a.cp_active = p->d_cp_active.p; a.st = p->d_state.p; a.n_cp = p->n_cp; a.k = p->order; a.mc = p->m; a.sep_s = p->sep_s; a.sep_n = p->sep_n; a.m = p->m + p->border_extra();
  static const int dbg = [] {
    const int v = env_int("CALICO_KERNEL_TIMING", 0, 0);
#ifndef CALICO_DEV_TIMING
    if (v) std::fprintf(stderr, "[calico] CALICO_KERNEL_TIMING is set, but this library was built without the kernels' development "
                                "instrumentation (rebuild with CALICO_DEV_TIMING=1 in the environment of __graft_entry__.build())\n");
#endif
    return v;
  }();
  a.debug = dbg;
  a.progress = nullptr;
  return a;
}

EvalArgs make_eval_args(calico_problem* p, const double* x, int apply_loss, bool want_res) {
  EvalArgs a;
  static const int dbg = env_int("CALICO_KERNEL_TIMING", 0, 0);
  a.debug = dbg;
  a.x = x; a.sensors = p->d_sensors.p; a.layouts = p->d_layouts.p; a.items = p->d_items.p;
  a.knots = p->d_knots.p; a.basis = p->d_basis.p; a.ctrl_off = p->d_ctrl_off.p;
  a.m0 = p->d_m0.p; a.m1 = p->d_m1.p; a.m2 = p->d_m2.p; a.stamp = p->d_stamp.p; a.point_off = p->d_point_off.p;
  a.partials = p->d_partials.p; a.item_cost = p->d_partials.p + p->partial_doubles;
  a.res_out = want_res ? p->d_res.p : nullptr; a.valid_out = want_res ? p->d_valid.p : nullptr;
  a.order = p->order; a.n_items = p->n_items; a.lds_cols = p->lds_cols; a.row_pad = p->row_pad; a.n_cells = p->n_cells; a.cells = p->d_cells.p; a.prim_tab = p->d_prim_tab.p;
  a.cell_chunk = p->cell_chunk; a.cell_rec_max = p->cell_rec_max; a.project = 0; a.row_cell_chunk = p->row_cell_chunk; a.frame_lds_doubles = p->frame_lds_doubles; a.pad5 = 0; a.wave_log = p->d_wave_log.p; a.active = p->any_tagged ? p->d_active.p : nullptr; a.apply_loss = apply_loss;
  a.st = nullptr; a.need_flag = 0; a.cost_index_base = 0;
  a.fitems = p->d_fitems.p; a.n_fitems = p->n_fitems;
  a.hint_progress = nullptr; a.hint_seq = 0; a.hint_ftol = a.hint_ptol = 0.0;
  a.pair_mode = 0; a.wave_lds_doubles = 0;
  return a;
}

// Plan (cached or built), workspace (pooled or allocated), values.
int finalize(calico_problem* p) {
  if (!p->dirty) return CALICO_OK;
  p->res_cache.valid = false;
  p->step_ready = false;
  p->cov.valid = false;      // (a covariance of the structure before is gone: its layout is not this plan's)
  p->obs.valid = false;      // (and so is an observability report)
  if (p->order <= 0) return p->set_error(CALICO_FAILED_PRECONDITION, "spline not set");
  if (p->order > 8) return p->set_error(CALICO_UNIMPLEMENTED, "spline order > 8 is not supported by the HIP kernels");
  HIP_TRY(p, hipSetDevice(p->device));
  const PlanSwitches sw{};
  SetupTimer setup;
  // a workspace that belongs to the plan the handle is leaving goes back to that plan's pool
  const bool use_cache = plan_cache_enabled();
  PlanKey key;
  std::shared_ptr<PlanEntry> hit;
  if (use_cache) {
    key = structure_key(p, sw);
    PlanCache& c = plan_cache();
    std::lock_guard<std::mutex> lock(c.mu);
    for (const std::shared_ptr<PlanEntry>& e : c.entries) if (e->key == key) { hit = e; break; }
    if (hit) { hit->last_use = ++c.tick; ++c.hits; } else ++c.misses;
  }
  setup.section("structure key + look-up");
  if (hit && p->plan == hit && p->ws_ready) {
    // same structure as before on the same handle (values re-registered): nothing to rebuild
  } else {
    if (p->plan && p->ws_ready) {        // leaving another plan: its workspace stays with it
      HIP_TRY(p, hipStreamSynchronize(p->stream));
      auto w = std::make_unique<Workspace>();
      w->swap_ws(static_cast<Workspace&>(*p));
      std::lock_guard<std::mutex> lock(plan_cache().mu);
      if (p->plan->pool.size() < PlanCache::kMaxPool) p->plan->pool.push_back(std::move(w));
    }
    p->plan.reset();
    p->ws_ready = false;
    if (hit) adopt_plan(p, hit);
    else {
      const int rc = build_plan(p, sw, setup);
      if (rc != CALICO_OK) return rc;
      if (use_cache) {
        auto e = std::make_shared<PlanEntry>();
        e->key = key;
        e->host = static_cast<const PlanHost&>(*p);
        e->block_meta.resize(p->blocks.size());
        for (size_t i = 0; i < p->blocks.size(); ++i) e->block_meta[i] = {p->blocks[i].amb_off, p->blocks[i].tan, p->blocks[i].eff, p->blocks[i].used};
        e->sensor_meta.resize(p->sensors.size());
        for (size_t i = 0; i < p->sensors.size(); ++i)
          e->sensor_meta[i] = {p->sensors[i].sorted_pos, p->sensors[i].sorted_begin, p->sensors[i].sorted_end};
        e->dev.take_from(static_cast<PlanDev&>(*p));
        static_cast<PlanDev&>(*p).alias_from(e->dev);
        p->plan = e;
        PlanCache& c = plan_cache();
        std::shared_ptr<PlanEntry> evicted;
        {
          std::lock_guard<std::mutex> lock(c.mu);
          e->last_use = ++c.tick;
          if (c.entries.size() >= PlanCache::kMaxEntries) {
            size_t old = 0;
            for (size_t i = 1; i < c.entries.size(); ++i) if (c.entries[i]->last_use < c.entries[old]->last_use) old = i;
            evicted = std::move(c.entries[old]);
            c.entries.erase(c.entries.begin() + long(old));      // (handles that still use it keep it alive)
          }
          c.entries.push_back(e);
        }
        if (evicted && evicted.use_count() == 1) {       // its buffers go back now: one wait for ITS device, outside the cache's lock
          DeviceArena::Batch batch(evicted->key.device);
          evicted.reset();
        }
      }
    }
    setup.section(hit ? "plan adopted" : "plan cached");
    const int rc = prepare_workspace(p);
    if (rc != CALICO_OK) return rc;
    setup.section("workspace");
  }
  int rc = upload_values(p);
  if (rc != CALICO_OK) return rc;
  rc = configure_kernels(p);
  if (rc != CALICO_OK) return rc;
  HIP_TRY(p, hipStreamSynchronize(p->stream));
  pinned_pool().release(p->h_mpin, p->h_mpin_n); p->h_mpin = nullptr; p->h_mpin_n = 0;     // (the uploads are through)
  setup.section("values + kernel attributes");
  p->dirty = false;
  return CALICO_OK;
}

int upload_x(calico_problem* p, bool seed) {
  if (p->active_dirty) {   // outlier tags, in the sorted order of the device arrays
    std::vector<uint8_t> act(size_t(std::max<int64_t>(p->n_obs, 1)), 1);
    bool tagged = false;
    for (const HSensor& s : p->sensors)
      for (int64_t i = 0; i < s.n(); ++i) { act[size_t(s.sorted_pos[size_t(i)])] = s.active[size_t(i)]; tagged = tagged || !s.active[size_t(i)]; }
    p->any_tagged = tagged;
    HIP_TRY(p, hipMemcpyAsync(p->d_active.p, act.data(), size_t(p->n_obs), hipMemcpyHostToDevice, p->stream));
    HIP_TRY(p, hipStreamSynchronize(p->stream));   // `act` is a local
    p->active_dirty = false;
  }
  for (const HBlock& b : p->blocks) std::copy(b.v.begin(), b.v.end(), p->h_x.begin() + b.amb_off);
  // through the pinned staging buffer: a true asynchronous DMA (every API call ends with a stream synchronisation, so
  // the buffer is never rewritten while a transfer is pending)
  std::copy(p->h_x.begin(), p->h_x.end(), p->h_xpin);
  if (!seed) return CALICO_OK;   // calico_solve: the kernel that resets the LM state reads the staging buffer
  launch_seed_x(p->d_x.p, p->h_xpin, int(p->h_x.size()), p->stream);      // the kernel reads the pinned buffer: no DMA copy (~13 us) on the stream
  // d_xc needs no upload: every parameter block, constant ones included, is rewritten by the update kernel... except
  // the constant blocks, which the update never touches -- so it is seeded once per finalisation (below) and whenever
  // a constant block may have changed
  if (p->xc_stale) {
    HIP_TRY(p, hipMemcpyAsync(p->d_xc.p, p->h_xpin, p->h_x.size() * sizeof(double), hipMemcpyHostToDevice, p->stream));
    p->xc_stale = false;
  }
  return CALICO_OK;
}

// residual + Jacobian evaluation at d_x into the reduce buffer R. With st != nullptr the
// kernels skip themselves on the device when the solve has terminated or (need_flag) when
// the last step was rejected, so whole iterations can be enqueued without a host round trip.
// `spec`: evaluation at the candidate point x_at = x_cand into the reduce buffer that does NOT hold R(x) (chosen on
// the device from LmState.rcur); otherwise evaluation at x into buffer 0.
// `end_hint` (streaming solve loop, fused Jacobian launch only: end_hint_available): the launch tells the host whether the
// control stage behind it is about to end the solve (eval_kernels.hip, end_hint_body).
int enqueue_jacobian_eval(calico_problem* p, const LmState* st, int need_flag, const double* x_at, bool spec, const ControlTail* tail,
                          bool end_hint) {
  p->timer.begin(0, p->stream);
  EvalArgs ea = make_eval_args(p, x_at ? x_at : p->d_x.p, 1, false);
  ea.st = st; ea.need_flag = need_flag;
  if (end_hint && tail && st && end_hint_available(p)) {
    ea.hint_progress = tail->progress; ea.hint_seq = tail->seq;
    ea.hint_ftol = tail->o.function_tolerance; ea.hint_ptol = tail->o.parameter_tolerance;
  }
  ea.items = p->d_jac_items.p; ea.n_items = p->n_jac_items; ea.cost_index_base = p->n_fitems;
  if (p->fuse_expand) { ea.pair_mode = 1; ea.wave_lds_doubles = p->pair_wave_lds_doubles; }      // (the plan has frames and order 6 then)
  // a launch the runtime refuses (too much LDS for the kernel's attribute, a bad grid) would leave last iteration's blocks
  // in place and the solve would go wrong silently on stale partials: ask behind EVERY launch (a thread-local read, no
  // synchronisation). The thread's error word is cleared first -- a benign error some other code on this thread left behind
  // (a PyTorch probe, a hipMalloc fallback) is not this solve's --, and asked per launch: hipGetLastError() reports the last
  // call only on some runtimes, so a refused first launch must not hide behind a second one that went through.
  (void)hipGetLastError();
  if (end_hint_available(p)) launch_eval_jacobian(ea, p->stream);   // camera frames (item-cost slots [0, n_fitems)) + everything else
  else launch_eval(ea, true, p->stream);                             // (no frames: they exist for spline order 6 only)
  HIP_TRY(p, hipGetLastError());
  p->timer.end(p->stream);
  p->timer.begin(1, p->stream);
  // the host knows which buffer is filled: multi-rank runs either read the state back every iteration or (batched)
  // always evaluate the candidate into buffer 1
  double* target = p->d_R.p + ((spec && p->h_state && !p->h_state->rcur) ? p->r_size : 0);
  if (p->has_exchange() && p->world > 1) {
    // a rank's gather only writes the entries its own residual blocks contribute to; the others must enter the sum
    // as zeros, not as what the previous reduction left there
    HIP_TRY(p, hipMemsetAsync(target, 0, p->r_size * sizeof(double), p->stream));
  }
  if (!p->fuse_expand) launch_expand_cells(ea, p->stream);   // compact frame records -> one expanded block per cell
  launch_gather(p->d_R.p, p->d_partials.p, p->d_out_thin.p, p->gather_fixed ? nullptr : p->d_ptr_thin.p, p->gather_fixed ? p->d_idx_fixed.p : p->d_idx_thin.p, p->n_thin, p->n_thin8, p->n_thin4, p->thin_per_lane, p->d_out_fat.p,
                p->d_ptr_fat.p, p->d_idx_fat.p, p->n_fat, p->d_partials.p + p->partial_doubles, p->n_fitems + p->n_jac_items, st, need_flag,
                spec ? p->r_size : 0, p->stream, tail);
  p->timer.end(p->stream);
  if (!p->has_exchange()) return CALICO_OK;  // single rank: no exchange
  return do_allreduce(p, target, int64_t(p->r_size));
}

// One linear solve + update of the candidate point: tree solver or sequential banded factorisation.
// with_post_eval: 0 none, 1 the bookkeeping of the step just accepted rides in the first launch, 2 the bookkeeping of the
// solve's FIRST evaluation does (tree solver only: level 0 then forms the Jacobi scale of its diagonal entries itself)
// reduce_only (the covariance pass): stop once the reduced system is in sa.Spart -- no reduced solve, no back-substitution.
void enqueue_linear_solve(calico_problem* p, const SolveArgs& sa, const LmOptionsDev& o, int with_post_eval, int jacobi, bool reduce_only) {
  hipStream_t s = p->stream;
  const int n_blocks = int(p->h_blocks.size());
  if (reduce_only && !p->use_bcr) {
    launch_band_reduction(sa, o, p->d_x.p, p->d_blocks.p, n_blocks, s, with_post_eval == 1, p->d_log.p, kLogCap, jacobi);
    return;
  }
  if (!p->use_bcr) {
    launch_solve(sa, o, p->d_x.p, p->d_xc.p, p->d_blocks.p, n_blocks, p->dense_in_lds, s, with_post_eval == 1, p->d_log.p, kLogCap, jacobi);
    return;
  }
  const BcrArgs b = make_bcr_args(p);
  const int L = int(p->bcr_levels.size());
  const LinearRoute rt = linear_route(p, sa);
  const int ks = rt.ks;
  const bool schur_rides = rt.schur_rides;
  int* const fan_word = p->d_handoff.p + 4;
  // (A/B switch, read per solve: 0 = every level reads its node descriptors from the table)
  const bool inline_nodes = env_flag("CALICO_INLINE_NODES", true);
  for (int l = 0; l < L; ++l) {
    const BcrLevel& lv = p->bcr_levels[size_t(l)];
    BcrInlineNodes inl = {};
    if (inline_nodes) {
      if (l == 0) inl.q_regular = p->bcr_q0;
      else if (lv.n_nodes <= 4) { inl.n = lv.n_nodes; for (int i = 0; i < lv.n_nodes; ++i) inl.nd[i] = p->h_bcr_nodes[size_t(lv.node0 + i)]; }
    }
    launch_bcr_level(sa, b, lv.node0, lv.n_nodes, l, lv.keep0, lv.n_keep, o, p->d_x.p, p->d_blocks.p, n_blocks, l == 0 ? with_post_eval : 0,
                     p->d_log.p, kLogCap, jacobi, s, schur_rides && l == L - 1 ? ks : 0, schur_rides ? fan_word : nullptr, inl);
  }
  if (!schur_rides) launch_bcr_schur(sa, b, ks, o, s);
  if (reduce_only) return;
  const BcrTopSeps& ts = rt.ts;
  const BcrLevel& lf = p->bcr_levels[size_t(rt.l_first)];
  const bool fused = rt.fused;
  p->timer.begin(6, s);       // the launch that solves the reduced system: the longest kernel of an iteration at configs[3]
  if (fused) {
    p->handoff_seq = p->handoff_seq % 0x3fffffff + 1;
    launch_dense_back(sa, b, ks, lf.node0, lf.n_nodes, lf.q_max, p->d_x.p, p->d_xc.p, p->d_blocks.p, n_blocks, ts, p->d_handoff.p, p->handoff_seq, s);
  } else {
    launch_reduced_solve(sa, p->dense_in_lds, ks, s);
  }
  p->timer.end(s);
  for (int l = L - 1; l >= 0; --l) {
    const BcrLevel& lv = p->bcr_levels[size_t(l)];
    if (ts.n > 0 && l == L - 1) continue;
    const bool first = l == L - 1 || (ts.n > 0 && l == L - 2);     // the first launch behind the reduced solve
    if (first && fused) continue;
    const BcrTopSeps none = {};
    launch_bcr_back(sa, b, lv.node0, lv.n_nodes, first, first, /*border_rows=*/l > 0, lv.q_max, p->d_x.p, p->d_xc.p, p->d_blocks.p, n_blocks,
                    first ? ts : none, s);
  }
  // development aid (CALICO_CHECK_FINITE=1): where does the first non-finite value of a solve sit?
  static const bool check = env_flag("CALICO_CHECK_FINITE", false);
  if (check) {
    (void)hipStreamSynchronize(s);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) std::fprintf(stderr, "[calico] launch error after the tree solve: %s\n", hipGetErrorString(le));
    auto scan = [&](const char* name, const double* d, size_t n) {
      std::vector<double> h(n);
      (void)hipMemcpy(h.data(), d, n * sizeof(double), hipMemcpyDeviceToHost);
      size_t bad = 0, first = 0;
      for (size_t i = 0; i < n; ++i) if (!std::isfinite(h[i])) { if (!bad) first = i; ++bad; }
      if (bad) std::fprintf(stderr, "[calico] %s: %zu of %zu non-finite, first at %zu\n", name, bad, n, first);
    };
    const size_t N = size_t(p->bcr_N), bb = size_t(kBcrBP) * kBcrBP, fb = size_t(kBcrBP) * p->bcr_m1p, m1 = size_t(sa.m) + 1;
    scan("R", p->d_R.p, 2 * p->r_size); scan("D", b.D, N * bb); scan("F", b.F, N * fb); scan("M", b.M, N * bb); scan("ZA", b.ZA, N * bb);
    scan("ZB", b.ZB, N * bb); scan("Y", b.Y, N * fb); scan("Spart", sa.Spart, size_t(ks) * m1 * m1); scan("y", sa.y, size_t(sa.NT()) + p->border_extra());
    scan("dadd", sa.dadd, size_t(sa.NT())); scan("scale", sa.scale, size_t(sa.NT()));
    scan("zb", b.zb, N * kBcrBP); scan("ysol", b.ysol, N * kBcrBP); scan("x", p->d_x.p, size_t(p->n_amb)); scan("x_cand", p->d_xc.p, size_t(p->n_amb));
    {
      std::vector<double> h(N * kBcrBP);
      (void)hipMemcpy(h.data(), b.ysol, h.size() * sizeof(double), hipMemcpyDeviceToHost);
      std::string okb;
      for (size_t I = 0; I < N; ++I) { bool ok = true; for (int r = 0; r < kBcrBP; ++r) ok = ok && std::isfinite(h[I * kBcrBP + r]); okb += ok ? '.' : 'X'; }
      std::fprintf(stderr, "[calico] ysol by superblock (X = non-finite): %s  root %d levels %zu\n", okb.c_str(), p->bcr_root, p->bcr_levels.size());
    }
  }
}

}  // namespace cal

namespace {
struct StreamPool {
  std::mutex mu;
  std::map<int, std::vector<hipStream_t>> idle;     // per device: streams of destroyed handles
  static constexpr size_t kMaxIdle = 4;
};
StreamPool& stream_pool() { static StreamPool* sp = new StreamPool(); return *sp; }     // (never destroyed: the streams outlive static destruction)
}  // namespace

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
  if (p->plan && p->ws_ready) {
    auto w = std::make_unique<Workspace>();
    w->swap_ws(static_cast<Workspace&>(*p));
    std::lock_guard<std::mutex> lock(plan_cache().mu);
    if (p->plan->pool.size() < PlanCache::kMaxPool) p->plan->pool.push_back(std::move(w));
  }
  pinned_pool().release(p->h_mpin, p->h_mpin_n); p->h_mpin = nullptr;      // (only set if a finalize failed half-way)
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

int32_t calico_plan_cache_stats(int64_t* hits, int64_t* misses, int64_t* entries) {
  PlanCache& c = plan_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  if (hits) *hits = c.hits;
  if (misses) *misses = c.misses;
  if (entries) *entries = int64_t(c.entries.size());
  return CALICO_OK;
}

int32_t calico_plan_cache_clear(void) {
  PlanCache& c = plan_cache();
  std::vector<std::shared_ptr<PlanEntry>> drop;
  {
    std::lock_guard<std::mutex> lock(c.mu);
    drop.swap(c.entries);      // (entries that live handles still refer to are freed with the last of them)
  }
  for (std::shared_ptr<PlanEntry>& e : drop) {
    DeviceArena::Batch batch(e->key.device);
    {
      std::lock_guard<std::mutex> lock(c.mu);      // (a live handle of this plan may be taking a workspace from the pool)
      e->pool.clear();
    }
    e.reset();
  }
  DeviceArena::get().trim(0);   // every slab no live handle has a buffer in goes back to the driver
  return CALICO_OK;
}

const char* calico_last_error(const calico_problem* p) { return p ? p->error.c_str() : "null problem"; }

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

int32_t calico_solve(calico_problem* p, const calico_solver_options* opt, calico_summary* sm) {
  if (!p || !opt || !sm) return CALICO_INVALID_ARGUMENT;
  const auto t_start = std::chrono::steady_clock::now();
  // CALICO_SOLVE_TIMING=1: host time of the sections of this call and since the previous call returned (development aid)
  static const bool solve_timing = env_flag("CALICO_SOLVE_TIMING", false);
  static std::chrono::steady_clock::time_point t_last_return = t_start;
  double t_mark[6] = {0, 0, 0, 0, 0, 0};
  auto mark = [&](int i) { if (solve_timing) t_mark[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count(); };
  std::memset(sm, 0, sizeof(*sm));
  if (int rc = require_exchange(p)) return rc;
  int rc = finalize(p);
  if (rc != CALICO_OK) return rc;
  HIP_TRY(p, hipSetDevice(p->device));
  rc = upload_x(p, /*seed=*/false);
  if (rc != CALICO_OK) return rc;
  fill_counts(p, sm);
  p->iterations.clear();
  p->step_ready = false;
  // event brackets nobody has asked about yet: resolved here once they pile up (a solve returns without draining them)
  if (p->timer.pending.size() > 8192) { HIP_TRY(p, hipStreamSynchronize(p->stream)); p->timer.resolve(); }
  LmOptionsDev o;
  o.max_num_iterations = opt->max_num_iterations; o.max_num_consecutive_invalid_steps = opt->max_num_consecutive_invalid_steps;
  o.function_tolerance = opt->function_tolerance; o.gradient_tolerance = opt->gradient_tolerance;
  o.parameter_tolerance = opt->parameter_tolerance; o.max_radius = opt->max_trust_region_radius;
  o.min_radius = opt->min_trust_region_radius; o.min_relative_decrease = opt->min_relative_decrease;
  o.min_lm_diagonal = opt->min_lm_diagonal; o.max_lm_diagonal = opt->max_lm_diagonal;
  double xn = 0.0;
  for (const BlockDev& b : p->h_blocks) for (int i = 0; i < b.size; ++i) xn += p->h_x[b.amb_off + i] * p->h_x[b.amb_off + i];
  hipStream_t s = p->stream;
  const auto t_loop = std::chrono::steady_clock::now();
  const double* upd_ext = p->use_bcr ? p->d_bupd.p : nullptr;
  const int upd_ext_n = p->use_bcr ? p->bcr_slots : 0;
  // Single rank, speculative evaluation: the host never blocks inside the solve. The control kernel publishes the
  // number of the iteration it has finished with (and post_eval / control the termination flag) in host-mapped
  // memory; the host keeps `depth` iterations enqueued ahead of that and stops when the flag goes up. Compared with
  // batches of `sync_every` iterations and a blocking read-back per batch this takes the read-back gaps out of the
  // stream and leaves at most `depth` iterations of early-exit kernels behind a terminated solve. The stage that
  // terminates the solve writes the results (state, log, parameters) into pinned host memory itself, so the call
  // returns as soon as the flag is up: the early-exit kernels drain while the caller prepares its next call.
  const int stream_depth = env_int("CALICO_STREAM_DEPTH", 2, 0);
  // (the progress word carries the iteration count in 20 bits: budgets beyond that take the batched loop)
  const bool streaming = p->speculative && !p->has_exchange() && stream_depth > 0 && p->h_progress != nullptr &&
                         opt->max_num_iterations <= 0xfffff;
  const int log_rows = std::min(kLogCap, std::max(0, opt->max_num_iterations) + 2);
  ResultSink sink = {};
  if (streaming) {
    p->solve_epoch = p->solve_epoch % 2047 + 1;
    sink.state = p->h_state; sink.log = p->h_log; sink.x = p->h_xpin; sink.src_log = p->d_log.p; sink.src_x = p->d_x.p;
    sink.rows = log_rows; sink.n_amb = int(p->h_x.size()); sink.epoch = p->solve_epoch;
  }
  // what a hipEventRecord pair costs around a ~2 us kernel on this stream: lets the caller take the bracket
  // overhead out of the per-launch phase times (phase 5)
  if ((p->timer.mask >> 5) & 1) {
    for (int r = 0; r < 4; ++r) {
      p->timer.begin(5, s);
      launch_init_state(p->d_state.p, opt->initial_trust_region_radius, std::sqrt(xn), s, upd_ext, upd_ext_n);
      p->timer.end(s);
    }
  }
  mark(0);
  launch_begin_solve(p->d_state.p, opt->initial_trust_region_radius, std::sqrt(xn), upd_ext, upd_ext_n, sink, p->d_x.p,
                     p->xc_stale ? p->d_xc.p : nullptr, p->h_xpin, int(p->h_x.size()), s);
  p->xc_stale = false;
  mark(1);
  SolveArgs sa = make_solve_args(p);
  const int n_blocks = int(p->h_blocks.size());
  if (streaming) sa.progress = p->d_progress;
  const int epoch = p->solve_epoch;
  // iteration 0
  rc = enqueue_jacobian_eval(p, nullptr, 0);
  if (rc != CALICO_OK) return rc;
  // The bookkeeping of the first evaluation (initial cost, gradient norms, Jacobi scaling, log row 0) rides in the first
  // linear solve's level-0 launch where the streaming loop and the tree solver run
  const bool fold_first = streaming && p->use_bcr && !p->has_exchange() && opt->max_num_iterations > 0;
  if (!fold_first) {
    p->timer.begin(4, s);
    launch_post_eval(sa, p->d_x.p, p->d_blocks.p, int(p->h_blocks.size()), o, p->d_log.p, kLogCap, 1, opt->jacobi_scaling, s);
    p->timer.end(s);
  }
  // The iteration enqueued ahead of the device is wasted when the one in front of it ends the solve (six early-exit kernels,
  // 40 us at configs[3], in front of the caller's next solve). With the end hint the Jacobian launch of iteration i says, from
  // what the linear solve left, whether iteration i's control stage will end the solve; iteration i + 1 is enqueued on its
  // "go" (progress word 2) -- the evaluation chain is still running then, so the device does not wait -- or, without one,
  // once iteration i has ended without terminating (CALICO_PREDICT_END=0: always one iteration ahead, rounds 2-3).
  const bool predict_end = streaming && end_hint_available(p) && env_flag("CALICO_PREDICT_END", true);
  mark(2);
  int dbg_enq = 0, dbg_go = 0, dbg_wait = 0;      // CALICO_SOLVE_TIMING: iterations enqueued, on a go word, behind a finished iteration
  if (streaming) {
    __atomic_store_n(p->h_progress + 2, 0, __ATOMIC_RELEASE);     // (a go word of the same epoch, 2047 solves ago)
    int enq = 0;
    auto t_progress = std::chrono::steady_clock::now();     // when the device last reported a finished iteration
    int last_seen = 0;
    int64_t spins = 0;
    bool budget_spent = false;
    for (;;) {
      bool done = false;
      for (;;) {
        if (__atomic_load_n(p->h_progress + 1, __ATOMIC_ACQUIRE) == epoch) { done = true; break; }
        const int word = __atomic_load_n(p->h_progress, __ATOMIC_ACQUIRE);
        const int seen = (word >> 20) == epoch ? (word & 0xfffff) : 0;    // words of another epoch: early-exit kernels of the previous solve
        if (seen != last_seen) { last_seen = seen; t_progress = std::chrono::steady_clock::now(); spins = 0; }
        const bool room = predict_end
                              ? (seen >= enq || __atomic_load_n(p->h_progress + 2, __ATOMIC_ACQUIRE) == ((epoch << 20) | enq))
                              : enq - seen < stream_depth;
        if (!budget_spent && room) {
          if (solve_timing) { ++dbg_enq; if (seen >= enq) ++dbg_wait; else ++dbg_go; }
          // the device raises the termination word BEFORE the iteration count: having seen the count move, look at the
          // flag once more, or one solve in two enqueues a whole iteration of early-exit kernels for nothing
          if (__atomic_load_n(p->h_progress + 1, __ATOMIC_ACQUIRE) == epoch) done = true;
          break;
        }
        __builtin_ia32_pause();
        if ((++spins & 0xfffff) == 0) {   // a device fault must not leave the host spinning
          const hipError_t qe = hipStreamQuery(s);
          if (qe != hipSuccess && qe != hipErrorNotReady) return p->set_error(CALICO_INTERNAL, hipGetErrorString(qe));
          if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_progress).count() > 600.0) {
            (void)hipStreamSynchronize(s);     // nothing of this solve stays behind on the stream
            return p->set_error(CALICO_INTERNAL, "solve loop: no progress from the device");
          }
        }
      }
      if (done) break;
      if (enq >= std::max(0, opt->max_num_iterations)) {
        // the iteration budget is enqueued: all that can still be due is the bookkeeping of the last step, should it be
        // accepted (it ends the solve by the iteration count) -- one kernel instead of an iteration of early exits
        launch_post_eval(sa, p->d_x.p, p->d_blocks.p, n_blocks, o, p->d_log.p, kLogCap, 0, opt->jacobi_scaling, s);
        budget_spent = true;
        continue;
      }
      p->timer.begin(2, s);
      enqueue_linear_solve(p, sa, o, /*with_post_eval=*/enq > 0 ? 1 : (fold_first ? 2 : 0), opt->jacobi_scaling);
      p->timer.end(s);
      // the control stage rides in the last workgroup of the gather kernel
      ControlTail tail;
      tail.enabled = 1; tail.n_amb = p->n_amb; tail.log_cap = kLogCap; tail.seq = ++enq; tail.o = o; tail.x = p->d_x.p;
      tail.x_cand = p->d_xc.p; tail.log = p->d_log.p; tail.Rbase = p->d_R.p; tail.r_stride = p->r_size;
      tail.progress = p->d_progress;
      rc = enqueue_jacobian_eval(p, p->d_state.p, 0, p->d_xc.p, true, &tail, predict_end);
      if (rc != CALICO_OK) return rc;
    }
  } else {
    rc = read_state(p);
    if (rc != CALICO_OK) return rc;
  }
  // One LM iteration = linear solve + candidate cost + control (+ Jacobian evaluation if the
  // step was accepted). `sync_every` complete iterations are enqueued per host round trip, every kernel deciding on
  // the device whether it still has work. With several ranks this needs the speculative evaluation: the candidate is
  // then always evaluated into reduce buffer 1, so the collective gets a fixed address and runs in every enqueued
  // iteration on every rank (re-reducing a stale buffer 1 behind a terminated solve is harmless), and an accepted
  // candidate is committed by a copy (commit_kernel) instead of the pointer swap. Without the speculative evaluation
  // a multi-rank run needs the host between the phases (the all-reduce must not run when the evaluation was skipped).
  const bool spec = p->speculative;
  const bool multi = p->has_exchange();
  const bool async = !multi || (spec && env_flag("CALICO_MULTIRANK_ASYNC", true));
  const int batch = async ? std::max(1, opt->sync_every) : 1;
  int batch_now = batch;
  while (!streaming && !p->h_state->terminated) {
    // The iterations enqueued behind a terminated solve are wasted (with several ranks each still carries a real
    // all-reduce), so the batch shrinks when the cost changes of the last two successful steps predict convergence
    // by the function tolerance within fewer iterations: linear convergence, ratio r -> log(tol / change) / log(r).
    batch_now = batch;
    {
      const LmState& hs = *p->h_state;
      const double tol = opt->function_tolerance * hs.x_cost;
      if (batch > 1 && hs.last_cost_change > 0.0 && hs.prev_cost_change > hs.last_cost_change && tol > 0.0) {
        const double r = hs.last_cost_change / hs.prev_cost_change;
        const double left = hs.last_cost_change <= tol ? 0.0 : std::ceil(std::log(tol / hs.last_cost_change) / std::log(r));
        batch_now = int(std::max(1.0, std::min(double(batch), left + 1.0)));
      }
    }
    for (int b = 0; b < batch_now; ++b) {
      // (speculative, single rank) the bookkeeping of the step accepted in the previous iteration of this batch rides
      // in the prepare kernel of this one; the last iteration of a batch gets a stand-alone post_eval below
      const bool ride = spec && async && b > 0;
      p->timer.begin(2, s);
      enqueue_linear_solve(p, sa, o, ride, opt->jacobi_scaling);
      p->timer.end(s);
      if (spec) {
        // Speculative evaluation: cost AND Jacobian at the candidate point in one pass, into the reduce buffer that
        // does not hold R(x). Its first two entries are the candidate's [cost, invalid]; when the step is accepted the
        // control kernel swaps the buffers and the next linear solve starts at once -- no separate cost-only pass,
        // and with several ranks a single all-reduce per iteration. A rejected step wastes the Jacobian work.
        rc = enqueue_jacobian_eval(p, p->d_state.p, 0, p->d_xc.p, true);
        if (rc != CALICO_OK) return rc;
        p->timer.begin(4, s);
        launch_control(p->d_state.p, o, p->d_R2.p, p->d_x.p, p->d_xc.p, p->n_amb, p->d_log.p, kLogCap, nullptr, 0, p->d_R.p,
                       p->r_size, s, /*commit_by_copy=*/multi && async);
        if (!async || b == batch_now - 1)
          launch_post_eval(sa, p->d_x.p, p->d_blocks.p, n_blocks, o, p->d_log.p, kLogCap, 0, opt->jacobi_scaling, s);
        p->timer.end(s);
        if (!async) {
          rc = read_state(p);
          if (rc != CALICO_OK) return rc;
          if (p->h_state->terminated) break;
        }
        continue;
      }
      p->timer.begin(3, s);
      {
        EvalArgs ea = make_eval_args(p, p->d_xc.p, 1, false);
        ea.st = p->d_state.p;
        launch_eval(ea, false, s);
      }
      const bool fuse_cost = !p->has_exchange();    // single rank: the cost sum rides in the control kernel
      if (!fuse_cost) launch_cost_reduce(p->d_partials.p + p->partial_doubles, p->n_items, p->d_R2.p, p->d_state.p, s);
      p->timer.end(s);
      rc = do_allreduce(p, p->d_R2.p, 2);
      if (rc != CALICO_OK) return rc;
      p->timer.begin(4, s);
      launch_control(p->d_state.p, o, p->d_R2.p, p->d_x.p, p->d_xc.p, p->n_amb, p->d_log.p, kLogCap,
                     fuse_cost ? p->d_partials.p + p->partial_doubles : nullptr, p->n_items, nullptr, 0, s);
      p->timer.end(s);
      if (!async) {
        rc = read_state(p);
        if (rc != CALICO_OK) return rc;
        if (p->h_state->terminated || !p->h_state->need_jacobian) continue;
      }
      rc = enqueue_jacobian_eval(p, p->d_state.p, async ? 1 : 0);
      if (rc != CALICO_OK) return rc;
      p->timer.begin(4, s);
      launch_post_eval(sa, p->d_x.p, p->d_blocks.p, n_blocks, o, p->d_log.p, kLogCap, 0, opt->jacobi_scaling, s);
      p->timer.end(s);
    }
    rc = read_state(p);
    if (rc != CALICO_OK) return rc;
  }
  // results: final state, iteration log and parameters come back in one go (pinned buffers, one synchronisation)
  // one small kernel writes them into the pinned host buffers (three DMA copies cost ~13 us of stream time each). R(x)
  // may sit in either reduce buffer afterwards: nobody reads it (every entry point that needs it evaluates first).
  // (streaming loop: the terminating stage has written them already, and nothing is waited for; event brackets of the
  //  phase timer are resolved when somebody asks for the times)
  mark(3);
  if (!streaming) launch_publish_results(p->d_state.p, p->d_log.p, log_rows, p->d_x.p, int(p->h_x.size()), p->h_state, p->h_log, p->h_xpin, s);
  if (!streaming) HIP_TRY(p, hipStreamSynchronize(s));
  sm->num_jacobian_evaluations = p->h_state->n_jac_evals;
  sm->num_cost_evaluations = p->h_state->n_cost_evals;
  const double t_solve = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_loop).count();
  const LmState st = *p->h_state;
  std::copy(p->h_xpin, p->h_xpin + p->h_x.size(), p->h_x.begin());
  for (HBlock& b : p->blocks) std::copy(p->h_x.begin() + b.amb_off, p->h_x.begin() + b.amb_off + b.size, b.v.begin());
  const std::vector<IterLog> log(p->h_log, p->h_log + std::max(0, std::min(st.n_log, log_rows)));
  for (const IterLog& r : log) {
    calico_iteration it;
    it.iteration = r.iteration; it.step_is_valid = r.step_is_valid; it.step_is_successful = r.step_is_successful; it.reserved = 0;
    it.cost = r.cost; it.cost_change = r.cost_change; it.gradient_max_norm = r.gradient_max_norm; it.step_norm = r.step_norm;
    it.relative_decrease = r.relative_decrease; it.trust_region_radius = r.trust_region_radius;
    p->iterations.push_back(it);
    if (opt->minimizer_progress_to_stdout) {
      if (r.iteration == 0) std::printf("iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius\n");
      std::printf("%4d % 8e   % 3.2e   % 3.2e  % 3.2e  % 3.2e % 3.2e\n", r.iteration, r.cost, r.cost_change, r.gradient_max_norm,
                  r.step_norm, r.relative_decrease, r.trust_region_radius);
    }
  }
  if (p->d_wave_log.p && p->d_wave_log.n > 1) {   // development aid: the last Jacobian launch of the solve, workgroup by workgroup
    std::vector<unsigned long long> wl(p->d_wave_log.n);
    HIP_TRY(p, hipMemcpy(wl.data(), p->d_wave_log.p, wl.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (size_t i = 0; i + 1 < wl.size(); i += 2)
      std::fprintf(stderr, "WAVE %zu %s t0 %llu t1 %llu\n", i / 2, int(i / 2) < ((p->n_jac_items + 1) & ~1) ? "item" : "frame", wl[i], wl[i + 1]);
  }
  sm->termination_type = st.termination_type;
  sm->num_successful_steps = st.num_successful; sm->num_unsuccessful_steps = st.num_unsuccessful;
  sm->num_iterations = st.last_logged_iteration;      // Summary::iterations.size() - 1; not read from the log buffer, which is capped at kLogCap rows
  p->step_ready = st.last_logged_iteration >= 1;      // (every logged iteration after the 0th ran a linear solve)
  sm->initial_cost = st.initial_cost;
  sm->final_cost = st.termination_type == CALICO_FAILURE ? 0.0 : std::min(st.initial_cost, st.min_cost);
  std::snprintf(sm->message, sizeof(sm->message), "%s", reason_message(st.termination_reason));
  sm->solve_time_in_seconds = t_solve;
  sm->total_time_in_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  if (solve_timing) {
    mark(4);
    std::fprintf(stderr, "solve host us: since last return %.1f | prep %.1f | begin launch %.1f | first evaluation enqueued %.1f | loop %.1f | results %.1f"
                 " | iterations: device %d, enqueued %d (ahead of the device %d, behind a finished iteration %d), reason %d\n",
                 std::chrono::duration<double, std::micro>(t_start - t_last_return).count(), t_mark[0], t_mark[1] - t_mark[0],
                 t_mark[2] - t_mark[1], t_mark[3] - t_mark[2], t_mark[4] - t_mark[3], st.iteration, dbg_enq, dbg_go, dbg_wait,
                 st.termination_reason);
    t_last_return = std::chrono::steady_clock::now();
  }
  return CALICO_OK;
}

int32_t calico_debug_lm_control_replay(int32_t device, int32_t n, const double* rho, const int32_t* infinite,
                                       const calico_solver_options* opt, double* radius_out, int32_t* accepted_out,
                                       double* cost_column_out) {
  if (n <= 0 || n > kLogCap - 2 || !rho || !infinite || !opt || !radius_out || !accepted_out || !cost_column_out)
    return CALICO_INVALID_ARGUMENT;
  if (hipSetDevice(device) != hipSuccess) return CALICO_INTERNAL;
  DevBuf<double> d_rho, d_R2, d_rad, d_cost;
  DevBuf<int> d_inf, d_acc;
  DevBuf<LmState> d_st;
  DevBuf<IterLog> d_log;
  std::vector<double> h_rho(rho, rho + n);
  std::vector<int> h_inf(infinite, infinite + n);
  if (d_rho.upload(h_rho, nullptr) != hipSuccess || d_inf.upload(h_inf, nullptr) != hipSuccess || d_R2.alloc(2) != hipSuccess ||
      d_rad.alloc(size_t(n)) != hipSuccess || d_cost.alloc(size_t(n)) != hipSuccess || d_acc.alloc(size_t(n)) != hipSuccess ||
      d_st.alloc(1) != hipSuccess || d_log.alloc(kLogCap) != hipSuccess)
    return CALICO_INTERNAL;
  LmOptionsDev o;
  o.max_num_iterations = 1 << 30; o.max_num_consecutive_invalid_steps = opt->max_num_consecutive_invalid_steps;
  o.function_tolerance = 0.0; o.gradient_tolerance = 0.0; o.parameter_tolerance = 0.0;     // the replay never converges
  o.max_radius = opt->max_trust_region_radius; o.min_radius = opt->min_trust_region_radius;
  o.min_relative_decrease = opt->min_relative_decrease; o.min_lm_diagonal = opt->min_lm_diagonal; o.max_lm_diagonal = opt->max_lm_diagonal;
  launch_init_state(d_st.p, opt->initial_trust_region_radius, 1.0, nullptr);
  launch_debug_control_replay(d_st.p, o, d_rho.p, d_inf.p, n, d_R2.p, d_rad.p, d_acc.p, d_cost.p, d_log.p, kLogCap, nullptr);
  if (hipMemcpy(radius_out, d_rad.p, size_t(n) * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(accepted_out, d_acc.p, size_t(n) * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(cost_column_out, d_cost.p, size_t(n) * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
    return CALICO_INTERNAL;
  return CALICO_OK;
}

int32_t calico_debug_roll_table(int32_t spline_order, int32_t lane, uint32_t* out48) {
  if (!out48 || spline_order < 1 || spline_order > 6 || lane < 0 || lane > 63) return CALICO_INVALID_ARGUMENT;
  cal::roll_table_row(spline_order, lane, out48);
  return CALICO_OK;
}

int32_t calico_debug_plan_info(calico_problem* p, int32_t* out, int32_t n) {
  if (!p || !out || n < 0 || n > kPlanInfoWords) return CALICO_INVALID_ARGUMENT;
  int rc = finalize(p);
  if (rc != CALICO_OK) return rc;
  const SolveArgs sa = make_solve_args(p);
  const LinearRoute rt = linear_route(p, sa);
  const bool tree = p->use_bcr;
  const int v[kPlanInfoWords] = {p->fuse_expand ? 1 : 0, p->n_fitems, p->n_jac_items, p->n_cells, p->max_cell_frames, p->max_item_run,
                                 tree ? 1 : 0, p->m, p->bcr_all_active ? 1 : 0,
                                 tree ? p->bcr_N : 0, tree ? p->bcr_q0 : 0, tree ? int(p->bcr_levels.size()) : 0,
                                 tree && p->bcr_root >= 0 ? 1 : 0, rt.schur_rides ? 1 : 0, rt.ts.n, rt.fused ? 1 : 0,
                                 rt.reduced, rt.reduced_in_lds ? 1 : 0, rt.ks, sa.m, p->sep_n};
  for (int i = 0; i < n; ++i) out[i] = v[i];
  return CALICO_OK;
}

int32_t calico_debug_last_step(calico_problem* p, int32_t n, double* step, double* damping, double* scale) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (p->dirty || !p->step_ready)
    return p->set_error(CALICO_FAILED_PRECONDITION, "no linear solve since the plan or the parameters last changed");
  const int NS = 6 * p->n_cp, NT = NS + p->m;
  if (n != p->n_eff && n != NT) return p->set_error(CALICO_INVALID_ARGUMENT, "n must be the effective parameter count or 6 n_cp + m");
  HIP_TRY(p, hipSetDevice(p->device));
  HIP_TRY(p, hipStreamSynchronize(p->stream));
  const SolveArgs sa = make_solve_args(p);
  std::vector<double> y(size_t(NT) + size_t(p->border_extra())), d(static_cast<size_t>(NT)), sc(static_cast<size_t>(NT));
  HIP_TRY(p, hipMemcpy(y.data(), p->d_y.p, y.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(p, hipMemcpy(d.data(), p->d_dadd.p, d.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIP_TRY(p, hipMemcpy(sc.data(), p->d_scale.p, sc.size() * sizeof(double), hipMemcpyDeviceToHost));
  // where the candidate update reads the solution of tangent row t (delta = -y): banded solver, y_index (the separator's rows
  // behind the calibration part); tree solver, the root's rows behind the calibration part, every other row at its own index
  constexpr int RB = 6 * kBcrCps;
  auto y_of = [&](int t) -> double {
    if (!p->use_bcr) return y[size_t(sa.y_index(t))];
    if (t < NS && p->bcr_root >= 0 && t / RB == p->bcr_root) return y[size_t(NS + p->m + (t - RB * p->bcr_root))];
    return y[size_t(t)];
  };
  for (int i = 0; i < n; ++i) {
    const int t = n == NT ? i : p->eff_to_tan[size_t(i)];
    if (step) step[i] = -y_of(t);
    if (damping) damping[i] = d[size_t(t)];
    if (scale) scale[i] = sc[size_t(t)];
  }
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
    {
      EvalArgs ea = make_eval_args(p, p->d_x.p, 0, true);
      ea.items = p->d_items_all.p; ea.n_items = p->n_items_all;  // every rank re-evaluates all blocks here
      ea.project = predict ? 1 : 0;
      launch_eval(ea, false, p->stream);
    }
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
  int rc = finalize(p);
  if (rc != CALICO_OK) return rc;
  HIP_TRY(p, hipSetDevice(p->device));
  rc = upload_x(p);
  if (rc != CALICO_OK) return rc;
  const HSensor& s = p->sensors[sid];
  if (s.n() == 0) return CALICO_OK;
  {
    EvalArgs ea = make_eval_args(p, p->d_x.p, 0, true);   // residuals without the loss function (camera.cpp:70-80)
    ea.items = p->d_items_all.p; ea.n_items = p->n_items_all;
    launch_eval(ea, false, p->stream);
  }
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
  int rc = finalize(p);
  if (rc != CALICO_OK) return rc;
  HIP_TRY(p, hipSetDevice(p->device));
  rc = upload_x(p);
  if (rc != CALICO_OK) return rc;
  HSensor& s = p->sensors[sid];
  {
    EvalArgs ea = make_eval_args(p, p->d_x.p, 0, true);   // residuals without the loss function (camera.cpp:70-80)
    ea.items = p->d_items_all.p; ea.n_items = p->n_items_all;
    launch_eval(ea, false, p->stream);
  }
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
  int rc = finalize(p);
  if (rc != CALICO_OK) return rc;
  HIP_TRY(p, hipSetDevice(p->device));
  rc = upload_x(p);
  if (rc != CALICO_OK) return rc;
  const HSensor& s = p->sensors[size_t(sid)];
  {
    EvalArgs ea = make_eval_args(p, p->d_x.p, 0, true);   // residuals without the loss function (camera.cpp:70-80)
    ea.items = p->d_items_all.p; ea.n_items = p->n_items_all;
    launch_eval(ea, false, p->stream);
  }
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

int32_t calico_evaluate(calico_problem* p, double* cost, double* gradient, double* jtj) {
  if (!p) return CALICO_INVALID_ARGUMENT;
  if (int rc = require_exchange(p)) return rc;
  int rc = finalize(p);
  if (rc != CALICO_OK) return rc;
  HIP_TRY(p, hipSetDevice(p->device));
  rc = upload_x(p);
  if (rc != CALICO_OK) return rc;
  rc = enqueue_jacobian_eval(p, nullptr, 0);
  if (rc != CALICO_OK) return rc;
  SolveArgs sa = make_solve_args(p);
  std::vector<double> R(sa.r_size());
  HIP_TRY(p, hipMemcpyAsync(R.data(), p->d_R.p, R.size() * sizeof(double), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(p, hipStreamSynchronize(p->stream));
  p->timer.resolve();
  if (R[1] > 0.0) return p->set_error(CALICO_INTERNAL, "residual evaluation failed");
  if (cost) *cost = R[0];
  const int n = p->n_eff, NS = 6 * p->n_cp, m = p->m, k = p->order;
  auto H = [&](int ta, int tb) -> double {  // solver tangent indices
    if (ta > tb) std::swap(ta, tb);
    if (tb < NS) {
      const int a = ta / 6, b = tb / 6;
      if (b - a >= k) return 0.0;
      return R[sa.off_B() + (size_t(a) * k + (b - a)) * 36 + (ta % 6) * 6 + (tb % 6)];
    }
    if (ta < NS) return R[sa.off_E() + size_t(ta) * m + (tb - NS)];
    return R[sa.off_C() + size_t(ta - NS) * m + (tb - NS)];
  };
  if (gradient) for (int i = 0; i < n; ++i) gradient[i] = R[sa.off_g() + p->eff_to_tan[size_t(i)]];
  if (jtj)
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) jtj[size_t(i) * n + j] = H(p->eff_to_tan[size_t(i)], p->eff_to_tan[size_t(j)]);
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
