// plan.cpp — what calico_problem_finalize derives from the STRUCTURE of a problem, and the cache that shares it: the plan's
// stages (blocks and tangent order, layouts, work items, the evaluation route, gather lists, the upload), the plan cache with
// its pooled workspaces, the workspace, the upload of the values and the kernels' LDS limits. finalize() at the end puts them
// together. One LM iteration and the solve loop are solve.cpp; the C entry points that describe a problem are calico_hip.cpp;
// what the host files share is problem_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/calico_hip.h"
#include "kernels.hpp"
#include "problem_dev.hpp"
#include "problem_host.hpp"
#include "shard.hpp"

namespace {

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
      if (bcr_level_main_span(nodes, per) + 9 > kNumCUs) cost += 5.0;
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
  if (size_t(p->lds_cols) * p->row_pad * sizeof(double) > kLdsBudget)
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
  if (band_cholesky_lds_bytes(sa) > kLdsBudget) return p->set_error(CALICO_UNIMPLEMENTED, "spline order too high for the banded factorisation window");
  p->dense_in_lds = reduced_solve_lds_bytes(sa) <= kLdsBudget - kLdsSlack;
  if (band_backsolve_lds_bytes(sa) > kLdsBudget) return p->set_error(CALICO_UNIMPLEMENTED, "trajectory too long for the back-substitution window");
  if (p->use_bcr && (bcr_level_lds_bytes() > kLdsBudget || bcr_back_lds_bytes(p->bcr_q_max, p->bcr_m1p) > kLdsBudget))
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

// ---- the cache's operations: look-up and insertion here, a workspace's way back, stats and clear in cal:: below ----
// Look-up by key; counts the hit or the miss.
std::shared_ptr<PlanEntry> cache_lookup(const PlanKey& key) {
  PlanCache& c = plan_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  for (const std::shared_ptr<PlanEntry>& e : c.entries) if (e->key == key) { e->last_use = ++c.tick; ++c.hits; return e; }
  ++c.misses;
  return nullptr;
}

// The plan the handle has just built becomes an entry (the handle keeps views of its buffers); the least recently used one makes room.
void cache_insert(calico_problem* p, const PlanKey& key) {
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
  if (kernel_timing_level() >= 3) HIP_TRY(p, p->d_wave_log.alloc(2 * size_t(p->n_jac_items + p->n_fitems) + 8));
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

// The dynamic-LDS limits this handle's launches need, raised at finalize (raise_lds_limit: a device that already allows them
// -- every handle of a known structure, and most others -- costs a few dozen look-ups and no hipFuncSetAttribute call).
int configure_kernels(calico_problem* p) {
  const SolveArgs sa = make_solve_args(p);
  const int dev = p->device;
  HIP_TRY(p, configure_eval_kernels(dev, size_t(p->lds_cols) * p->row_pad * sizeof(double)));
  HIP_TRY(p, configure_solve_kernels(dev, band_cholesky_lds_bytes(sa), p->dense_in_lds ? reduced_solve_lds_bytes(sa) : 0, band_backsolve_lds_bytes(sa)));
  HIP_TRY(p, configure_dense_block_solve(dev));
  HIP_TRY(p, configure_reduced_block_step(dev));
  if (!p->use_bcr) return CALICO_OK;
  HIP_TRY(p, configure_bcr_kernels(dev, p->bcr_q_max, p->bcr_m1p));
  const int q_fused = std::min(p->bcr_q_max, 4);      // (longer chains never take the fused launch: dense_back_fusable)
  if (dense_back_fits(q_fused, p->bcr_m1p)) HIP_TRY(p, configure_dense_back(dev, q_fused, p->bcr_m1p));
  return CALICO_OK;
}

}  // namespace

// ---- what the other host files call (declared in problem_host.hpp) ----
namespace cal {

// ---- the launch registry (declared in kernels.hpp): what is done once per device and process ----
namespace {
struct DeviceLaunchState {
  std::map<const void*, size_t> lds_limit;      // dynamic LDS each kernel may ask for here (absent: nothing set yet)
  bool roll_table = false;                      // g_roll_tab (bcr_kernels.hip) is uploaded
};
std::mutex g_launch_mu;
std::map<int, DeviceLaunchState> g_launch_state;
long long g_attribute_calls = 0;
}  // namespace

hipError_t raise_lds_limit(int device, const void* fn, size_t bytes) {
  std::lock_guard<std::mutex> lock(g_launch_mu);
  size_t& cur = g_launch_state[device].lds_limit[fn];
  if (bytes <= cur) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
  if (e == hipSuccess) { cur = bytes; ++g_attribute_calls; }
  return e;
}
hipError_t ensure_roll_table(int device) {
  std::lock_guard<std::mutex> lock(g_launch_mu);
  DeviceLaunchState& d = g_launch_state[device];
  if (d.roll_table) return hipSuccess;
  const hipError_t e = upload_roll_table();
  d.roll_table = e == hipSuccess;
  return e;
}
long long lds_attribute_calls() {
  std::lock_guard<std::mutex> lock(g_launch_mu);
  return g_attribute_calls;
}

// A handle's workspace goes back to the pool of the cached plan it belongs to (the handle leaves the plan, or is destroyed):
// the next handle of this structure takes it over instead of allocating. The caller has drained the handle's stream.
void return_workspace(calico_problem* p) {
  if (!p->plan || !p->ws_ready) return;
  auto w = std::make_unique<Workspace>();
  w->swap_ws(static_cast<Workspace&>(*p));
  std::lock_guard<std::mutex> lock(plan_cache().mu);
  if (p->plan->pool.size() < PlanCache::kMaxPool) p->plan->pool.push_back(std::move(w));
}

void release_measurement_staging(calico_problem* p) { pinned_pool().release(p->h_mpin, p->h_mpin_n); p->h_mpin = nullptr; p->h_mpin_n = 0; }

void plan_cache_stats(int64_t* hits, int64_t* misses, int64_t* entries) {
  PlanCache& c = plan_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  if (hits) *hits = c.hits;
  if (misses) *misses = c.misses;
  if (entries) *entries = int64_t(c.entries.size());
}

void plan_cache_clear() {
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
  if (use_cache) { key = structure_key(p, sw); hit = cache_lookup(key); }
  setup.section("structure key + look-up");
  if (hit && p->plan == hit && p->ws_ready) {
    // same structure as before on the same handle (values re-registered): nothing to rebuild
  } else {
    if (p->plan && p->ws_ready) HIP_TRY(p, hipStreamSynchronize(p->stream));     // leaving another plan: its workspace stays with it
    return_workspace(p);
    p->plan.reset();
    p->ws_ready = false;
    if (hit) adopt_plan(p, hit);
    else {
      const int rc = build_plan(p, sw, setup);
      if (rc != CALICO_OK) return rc;
      if (use_cache) cache_insert(p, key);
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
  release_measurement_staging(p);     // (the uploads are through)
  setup.section("values + kernel attributes");
  p->dirty = false;
  return CALICO_OK;
}

}  // namespace cal
