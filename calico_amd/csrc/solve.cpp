// solve.cpp — one LM iteration and the loop around it: what an iteration enqueues (the evaluation with its gather and exchange,
// the linear solve by the tree solver or the banded factorisation), calico_solve as a sequence of stages (begin; the polled or
// the batched loop; collect), and the hooks that report on or replay that machinery (calico_debug_plan_info,
// calico_debug_last_step, calico_debug_lm_control_replay, calico_evaluate). This file only enqueues kernels
// (eval_kernels.hip, solve_kernels.hip, bcr_kernels.hip) and reads back one small state struct; the plan they follow is
// plan.cpp, the handle and what the host files share is problem_host.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/calico_hip.h"
#include "calico_hip_testing.h"
#include "kernels.hpp"
#include "problem_dev.hpp"
#include "problem_host.hpp"

namespace {

BcrArgs make_bcr_args(calico_problem* p) {
  BcrArgs b;
  b.D = p->d_bD.p; b.G = p->d_bG.p; b.F = p->d_bF.p; b.pendD = p->d_bpD.p; b.pendF = p->d_bpF.p; b.M = p->d_bM.p; b.ZA = p->d_bZA.p;
  b.ZB = p->d_bZB.p; b.Y = p->d_bY.p; b.ysol = p->d_bysol.p; b.zb = p->d_bzb.p; b.upd = p->d_bupd.p; b.nodes = p->d_bnodes.p; b.keep = p->d_bkeep.p;
  b.cp_block = p->d_cp_block.p; b.ctrl_off = p->d_ctrl_off.p; b.all_active = p->bcr_all_active ? 1 : 0; b.pad0 = 0; b.N = p->bcr_N; b.m1p = p->bcr_m1p; b.root = p->bcr_root; b.root_pend = p->bcr_root_pend;
  b.root_par = p->bcr_root_par; b.n_slots = p->bcr_slots;
  return b;
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

// development aid (CALICO_CHECK_FINITE=1): where does the first non-finite value of a solve sit?
void check_finite_after_tree_solve(calico_problem* p, const SolveArgs& sa, const BcrArgs& b, int ks) {
  (void)hipStreamSynchronize(p->stream);
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

}  // namespace

// ---- one LM iteration (declared in problem_host.hpp: analysis.cpp and plan.cpp call these as well) ----
namespace cal {

// The route of a solve's linear solves: the plan's shapes, the kernels' shape rules (kernels.hpp) and the solve's switches.
LinearRoute linear_route(const calico_problem* p, const SolveArgs& sa, const SolveSwitches& sw) {
  LinearRoute r;
  r.ks = reduced_schur_slices(sa);
  r.reduced = reduced_solve_route(sa);
  r.reduced_in_lds = p->dense_in_lds;
  r.elim = sw.block_elim;
  r.dense_mode = !r.elim ? 0 : (sw.dense_roll ? 2 : 1);
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
  r.fused = sw.fuse_back && r.l_first == 0 && dense_back_fusable(sa, r.ks, lf.q_max, /*border_rows=*/r.l_first > 0) && dense_back_fits(lf.q_max, p->bcr_m1p);
  r.back_pre = r.fused && dense_back_pre_fits(sa) && (sw.back_pre < 0 ? dense_back_pre_pays(sa) : sw.back_pre != 0);
  r.level0_roll = sw.level_roll && r.elim && level0_roll_fits(sa);
  r.inline_nodes = sw.inline_nodes;
  return r;
}

int kernel_timing_level() {
  static const int level = [] {
    const int v = env_int("CALICO_KERNEL_TIMING", 0, 0);
#ifndef CALICO_DEV_TIMING
    if (v) std::fprintf(stderr, "[calico] CALICO_KERNEL_TIMING is set, but this library was built without the kernels' development "
                                "instrumentation (rebuild with CALICO_DEV_TIMING=1 in the environment of __graft_entry__.build())\n");
#endif
    return v;
  }();
  return level;
}

SolveArgs make_solve_args(calico_problem* p) {
  SolveArgs a;
  a.R = p->d_R.p; a.r_stride = p->speculative ? p->r_size : 0; a.Lb = p->d_Lb.p; a.Linv = p->d_Linv.p; a.Y = p->d_Y.p; a.S = p->d_S.p; a.Spart = p->d_Spart.p;
  a.Swork = p->d_Swork.p; a.y = p->d_y.p; a.zbuf = p->d_zbuf.p; a.dadd = p->d_dadd.p;
  a.scale = p->d_scale.p; a.cp_active = p->d_cp_active.p; a.st = p->d_state.p; a.n_cp = p->n_cp; a.k = p->order; a.mc = p->m; a.sep_s = p->sep_s; a.sep_n = p->sep_n; a.m = p->m + p->border_extra();
  a.debug = kernel_timing_level();
  a.progress = nullptr;
  return a;
}

EvalArgs make_eval_args(calico_problem* p, const double* x, int apply_loss, bool want_res) {
  EvalArgs a;
  a.debug = kernel_timing_level();
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
void enqueue_linear_solve(calico_problem* p, const SolveArgs& sa, const LinearRoute& rt, const LmOptionsDev& o, int with_post_eval, int jacobi,
                          bool reduce_only) {
  hipStream_t s = p->stream;
  const int n_blocks = int(p->h_blocks.size());
  if (reduce_only && !p->use_bcr) {
    launch_band_reduction(sa, o, p->d_x.p, p->d_blocks.p, n_blocks, s, with_post_eval == 1, p->d_log.p, kLogCap, jacobi);
    return;
  }
  if (!p->use_bcr) {
    launch_solve(sa, o, p->d_x.p, p->d_xc.p, p->d_blocks.p, n_blocks, p->dense_in_lds, s, with_post_eval == 1, p->d_log.p, kLogCap, jacobi, rt.dense_mode);
    return;
  }
  const BcrArgs b = make_bcr_args(p);
  const int L = int(p->bcr_levels.size());
  const int ks = rt.ks;
  const bool schur_rides = rt.schur_rides;
  int* const fan_word = p->d_handoff.p + 4;
  for (int l = 0; l < L; ++l) {
    const BcrLevel& lv = p->bcr_levels[size_t(l)];
    BcrInlineNodes inl = {};
    if (rt.inline_nodes) {
      if (l == 0) inl.q_regular = p->bcr_q0;
      else if (lv.n_nodes <= 4) { inl.n = lv.n_nodes; for (int i = 0; i < lv.n_nodes; ++i) inl.nd[i] = p->h_bcr_nodes[size_t(lv.node0 + i)]; }
    }
    launch_bcr_level(sa, b, lv.node0, lv.n_nodes, l, lv.keep0, lv.n_keep, o, p->d_x.p, p->d_blocks.p, n_blocks, l == 0 ? with_post_eval : 0,
                     p->d_log.p, kLogCap, jacobi, s, schur_rides && l == L - 1 ? ks : 0, schur_rides ? fan_word : nullptr, inl, rt.elim, l == 0 && rt.level0_roll);
  }
  if (!schur_rides) launch_bcr_schur(sa, b, ks, o, s);
  if (reduce_only) return;
  const BcrTopSeps& ts = rt.ts;
  const BcrLevel& lf = p->bcr_levels[size_t(rt.l_first)];
  const bool fused = rt.fused;
  p->timer.begin(6, s);       // the launch that solves the reduced system: the longest kernel of an iteration at configs[3]
  if (fused) {
    p->handoff_seq = p->handoff_seq % 0x3fffffff + 1;
    launch_dense_back(sa, b, ks, lf.node0, lf.n_nodes, lf.q_max, p->d_x.p, p->d_xc.p, p->d_blocks.p, n_blocks, ts, p->d_handoff.p, p->handoff_seq, s,
                      rt.back_pre, rt.dense_mode);
  } else {
    launch_reduced_solve(sa, p->dense_in_lds, ks, rt.dense_mode, s);
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
  static const bool check = env_flag("CALICO_CHECK_FINITE", false);
  if (check) check_finite_after_tree_solve(p, sa, b, ks);
}

}  // namespace cal

namespace {

// One calico_solve call as a sequence of stages: begin; the polled or the batched loop; collect.
struct SolveRun {
  calico_problem* p;
  const calico_solver_options* opt;
  calico_summary* sm;
  const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
  std::chrono::steady_clock::time_point t_loop;
  LmOptionsDev o;
  SolveArgs sa;
  LinearRoute rt;      // what every linear solve of this call does
  hipStream_t s = nullptr;
  int n_blocks = 0, log_rows = 0;
  ResultSink sink = {};
  // the mode, decided once in begin(): the polled ("streaming") loop with its options, or the batched one
  bool streaming = false, fold_first = false, predict_end = false, multirank_async = true;
  int stream_depth = 0;
  // CALICO_SOLVE_TIMING=1: host time of the sections of this call and since the previous call returned (development aid)
  bool timing = false;
  double t_mark[6] = {0, 0, 0, 0, 0, 0};
  int dbg_enq = 0, dbg_go = 0, dbg_wait = 0;      // iterations enqueued, on a go word, behind a finished iteration
  void mark(int i) { if (timing) t_mark[i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_start).count(); }

  int begin(), polled_loop(), batched_loop(), collect();
  int speculative_iteration(bool async, bool ride, bool last), cost_first_iteration(bool async);     // the batched loop's two bodies
  void post_eval(int first) { launch_post_eval(sa, p->d_x.p, p->d_blocks.p, n_blocks, o, p->d_log.p, kLogCap, first, opt->jacobi_scaling, s); }
  void control(const double* item_cost, int n_items, const double* Rbase, size_t r_stride, bool commit_by_copy = false) {
    launch_control(p->d_state.p, o, p->d_R2.p, p->d_x.p, p->d_xc.p, p->n_amb, p->d_log.p, kLogCap, item_cost, n_items, Rbase, r_stride, s, commit_by_copy);
  }
};

// Plan and values, the options, the mode; then the solve's first launches: the state reset, the first evaluation, its bookkeeping.
int SolveRun::begin() {
  static const bool solve_timing = env_flag("CALICO_SOLVE_TIMING", false);
  timing = solve_timing;
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
  o.max_num_iterations = opt->max_num_iterations; o.max_num_consecutive_invalid_steps = opt->max_num_consecutive_invalid_steps;
  o.function_tolerance = opt->function_tolerance; o.gradient_tolerance = opt->gradient_tolerance;
  o.parameter_tolerance = opt->parameter_tolerance; o.max_radius = opt->max_trust_region_radius;
  o.min_radius = opt->min_trust_region_radius; o.min_relative_decrease = opt->min_relative_decrease;
  o.min_lm_diagonal = opt->min_lm_diagonal; o.max_lm_diagonal = opt->max_lm_diagonal;
  double xn = 0.0;
  for (const BlockDev& b : p->h_blocks) for (int i = 0; i < b.size; ++i) xn += p->h_x[b.amb_off + i] * p->h_x[b.amb_off + i];
  s = p->stream;
  t_loop = std::chrono::steady_clock::now();
  const double* upd_ext = p->use_bcr ? p->d_bupd.p : nullptr;
  const int upd_ext_n = p->use_bcr ? p->bcr_slots : 0;
  // Single rank, speculative evaluation: the host never blocks inside the solve. The control kernel publishes the
  // number of the iteration it has finished with (and post_eval / control the termination flag) in host-mapped
  // memory; the host keeps `depth` iterations enqueued ahead of that and stops when the flag goes up. Compared with
  // batches of `sync_every` iterations and a blocking read-back per batch this takes the read-back gaps out of the
  // stream and leaves at most `depth` iterations of early-exit kernels behind a terminated solve. The stage that
  // terminates the solve writes the results (state, log, parameters) into pinned host memory itself, so the call
  // returns as soon as the flag is up: the early-exit kernels drain while the caller prepares its next call.
  const SolveSwitches sw;
  stream_depth = sw.stream_depth; multirank_async = sw.multirank_async;
  // (the progress word carries the iteration count in 20 bits: budgets beyond that take the batched loop)
  streaming = p->speculative && !p->has_exchange() && stream_depth > 0 && p->h_progress != nullptr && opt->max_num_iterations <= 0xfffff;
  log_rows = std::min(kLogCap, std::max(0, opt->max_num_iterations) + 2);
  if (streaming) {
    p->solve_epoch = p->solve_epoch % 2047 + 1;
    sink.state = p->h_state; sink.log = p->h_log; sink.x = p->h_xpin; sink.src_log = p->d_log.p; sink.src_x = p->d_x.p;
    sink.rows = log_rows; sink.n_amb = int(p->h_x.size()); sink.epoch = p->solve_epoch;
  }
  // what a hipEventRecord pair costs around a ~2 us kernel on this stream: lets the caller take the bracket
  // overhead out of the per-launch phase times (phase 5)
  if ((p->timer.mask >> 5) & 1) {
    for (int i = 0; i < 4; ++i) {
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
  sa = make_solve_args(p);
  rt = linear_route(p, sa, sw);
  n_blocks = int(p->h_blocks.size());
  if (streaming) sa.progress = p->d_progress;
  // iteration 0
  rc = enqueue_jacobian_eval(p, nullptr, 0);
  if (rc != CALICO_OK) return rc;
  // The bookkeeping of the first evaluation (initial cost, gradient norms, Jacobi scaling, log row 0) rides in the first
  // linear solve's level-0 launch where the streaming loop and the tree solver run
  fold_first = streaming && p->use_bcr && !p->has_exchange() && opt->max_num_iterations > 0;
  if (!fold_first) {
    p->timer.begin(4, s);
    post_eval(1);
    p->timer.end(s);
  }
  // The iteration enqueued ahead of the device is wasted when the one in front of it ends the solve (six early-exit kernels,
  // 40 us at configs[3], in front of the caller's next solve). With the end hint the Jacobian launch of iteration i says, from
  // what the linear solve left, whether iteration i's control stage will end the solve; iteration i + 1 is enqueued on its
  // "go" (progress word 2) -- the evaluation chain is still running then, so the device does not wait -- or, without one,
  // once iteration i has ended without terminating (SolveSwitches::predict_end off: always one iteration ahead).
  predict_end = streaming && end_hint_available(p) && sw.predict_end;
  mark(2);
  return CALICO_OK;
}

// The polled ("streaming") loop: iterations are enqueued as the device reports progress, until this epoch's termination word is up.
int SolveRun::polled_loop() {
  const int epoch = p->solve_epoch;
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
        if (timing) { ++dbg_enq; if (seen >= enq) ++dbg_wait; else ++dbg_go; }
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
      post_eval(0);
      budget_spent = true;
      continue;
    }
    p->timer.begin(2, s);
    enqueue_linear_solve(p, sa, rt, o, /*with_post_eval=*/enq > 0 ? 1 : (fold_first ? 2 : 0), opt->jacobi_scaling);
    p->timer.end(s);
    // the control stage rides in the last workgroup of the gather kernel
    ControlTail tail;
    tail.enabled = 1; tail.n_amb = p->n_amb; tail.log_cap = kLogCap; tail.seq = ++enq; tail.o = o; tail.x = p->d_x.p;
    tail.x_cand = p->d_xc.p; tail.log = p->d_log.p; tail.Rbase = p->d_R.p; tail.r_stride = p->r_size;
    tail.progress = p->d_progress;
    if (int rc = enqueue_jacobian_eval(p, p->d_state.p, 0, p->d_xc.p, true, &tail, predict_end)) return rc;
  }
  return CALICO_OK;
}

// One batched iteration, speculative evaluation: cost AND Jacobian at the candidate point in one pass, into the reduce buffer
// that does not hold R(x). Its first two entries are the candidate's [cost, invalid]; when the step is accepted the
// control kernel swaps the buffers and the next linear solve starts at once -- no separate cost-only pass,
// and with several ranks a single all-reduce per iteration. A rejected step wastes the Jacobian work.
// `ride` (single rank, not the first of its batch): the bookkeeping of the step accepted in the previous iteration of the
// batch rides in the prepare kernel of this one; `last` of a batch: it gets a stand-alone post_eval.
int SolveRun::speculative_iteration(bool async, bool ride, bool last) {
  p->timer.begin(2, s);
  enqueue_linear_solve(p, sa, rt, o, ride, opt->jacobi_scaling);
  p->timer.end(s);
  if (int rc = enqueue_jacobian_eval(p, p->d_state.p, 0, p->d_xc.p, true)) return rc;
  p->timer.begin(4, s);
  control(nullptr, 0, p->d_R.p, p->r_size, /*commit_by_copy=*/p->has_exchange() && async);
  if (!async || last) post_eval(0);
  p->timer.end(s);
  return async ? CALICO_OK : read_state(p);      // (not async: a batch is this one iteration, the loop reads the state once more)
}

// One batched iteration, cost first: the candidate's cost, the control stage, and the Jacobian only where the step was accepted
// (not async: the host reads the state back in between and decides; else the kernels do).
int SolveRun::cost_first_iteration(bool async) {
  p->timer.begin(2, s);
  enqueue_linear_solve(p, sa, rt, o, 0, opt->jacobi_scaling);
  p->timer.end(s);
  p->timer.begin(3, s);
  EvalArgs ea = make_eval_args(p, p->d_xc.p, 1, false);
  ea.st = p->d_state.p;
  launch_eval(ea, false, s);
  const bool fuse_cost = !p->has_exchange();    // single rank: the cost sum rides in the control kernel
  if (!fuse_cost) launch_cost_reduce(p->d_partials.p + p->partial_doubles, p->n_items, p->d_R2.p, p->d_state.p, s);
  p->timer.end(s);
  if (int rc = do_allreduce(p, p->d_R2.p, 2)) return rc;
  p->timer.begin(4, s);
  control(fuse_cost ? p->d_partials.p + p->partial_doubles : nullptr, p->n_items, nullptr, 0);
  p->timer.end(s);
  if (!async) {
    if (int rc = read_state(p)) return rc;
    if (p->h_state->terminated || !p->h_state->need_jacobian) return CALICO_OK;
  }
  if (int rc = enqueue_jacobian_eval(p, p->d_state.p, async ? 1 : 0)) return rc;
  p->timer.begin(4, s);
  post_eval(0);
  p->timer.end(s);
  return CALICO_OK;
}

// The batched loop. One LM iteration = linear solve + candidate cost + control (+ Jacobian evaluation if the
// step was accepted). `sync_every` complete iterations are enqueued per host round trip, every kernel deciding on
// the device whether it still has work. With several ranks this needs the speculative evaluation: the candidate is
// then always evaluated into reduce buffer 1, so the collective gets a fixed address and runs in every enqueued
// iteration on every rank (re-reducing a stale buffer 1 behind a terminated solve is harmless), and an accepted
// candidate is committed by a copy (commit_kernel) instead of the pointer swap. Without the speculative evaluation
// a multi-rank run needs the host between the phases (the all-reduce must not run when the evaluation was skipped).
int SolveRun::batched_loop() {
  if (int rc = read_state(p)) return rc;
  const bool spec = p->speculative;
  const bool async = !p->has_exchange() || (spec && multirank_async);
  const int batch = async ? std::max(1, opt->sync_every) : 1;
  while (!p->h_state->terminated) {
    // The iterations enqueued behind a terminated solve are wasted (with several ranks each still carries a real
    // all-reduce), so the batch shrinks when the cost changes of the last two successful steps predict convergence
    // by the function tolerance within fewer iterations: linear convergence, ratio r -> log(tol / change) / log(r).
    int batch_now = batch;
    const LmState& hs = *p->h_state;
    const double tol = opt->function_tolerance * hs.x_cost;
    if (batch > 1 && hs.last_cost_change > 0.0 && hs.prev_cost_change > hs.last_cost_change && tol > 0.0) {
      const double ratio = hs.last_cost_change / hs.prev_cost_change;
      const double left = hs.last_cost_change <= tol ? 0.0 : std::ceil(std::log(tol / hs.last_cost_change) / std::log(ratio));
      batch_now = int(std::max(1.0, std::min(double(batch), left + 1.0)));
    }
    for (int b = 0; b < batch_now; ++b) {
      if (int rc = spec ? speculative_iteration(async, /*ride=*/async && b > 0, /*last=*/b == batch_now - 1) : cost_first_iteration(async)) return rc;
    }
    if (int rc = read_state(p)) return rc;
  }
  return CALICO_OK;
}

// Results: final state, iteration log and parameters come back in one go (pinned buffers, one synchronisation):
// one small kernel writes them into the pinned host buffers (three DMA copies cost ~13 us of stream time each). R(x)
// may sit in either reduce buffer afterwards: nobody reads it (every entry point that needs it evaluates first).
// (streaming loop: the terminating stage has written them already, and nothing is waited for; event brackets of the
//  phase timer are resolved when somebody asks for the times)
int SolveRun::collect() {
  static std::chrono::steady_clock::time_point t_last_return = t_start;
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
  for (const IterLog& row : log) {
    calico_iteration it;
    it.iteration = row.iteration; it.step_is_valid = row.step_is_valid; it.step_is_successful = row.step_is_successful; it.reserved = 0;
    it.cost = row.cost; it.cost_change = row.cost_change; it.gradient_max_norm = row.gradient_max_norm; it.step_norm = row.step_norm;
    it.relative_decrease = row.relative_decrease; it.trust_region_radius = row.trust_region_radius;
    p->iterations.push_back(it);
    if (opt->minimizer_progress_to_stdout) {
      if (row.iteration == 0) std::printf("iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius\n");
      std::printf("%4d % 8e   % 3.2e   % 3.2e  % 3.2e  % 3.2e % 3.2e\n", row.iteration, row.cost, row.cost_change, row.gradient_max_norm,
                  row.step_norm, row.relative_decrease, row.trust_region_radius);
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
  if (timing) {
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

}  // namespace

extern "C" {

int32_t calico_solve(calico_problem* p, const calico_solver_options* opt, calico_summary* sm) {
  if (!p || !opt || !sm) return CALICO_INVALID_ARGUMENT;
  SolveRun r{p, opt, sm};
  if (int rc = r.begin()) return rc;
  if (int rc = r.streaming ? r.polled_loop() : r.batched_loop()) return rc;
  return r.collect();
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

int32_t calico_debug_plan_info(calico_problem* p, int32_t* out, int32_t n) {
  if (!p || !out || n < 0 || n > kPlanInfoWords) return CALICO_INVALID_ARGUMENT;
  int rc = finalize(p);
  if (rc != CALICO_OK) return rc;
  const SolveArgs sa = make_solve_args(p);
  const LinearRoute rt = linear_route(p, sa, SolveSwitches{});
  const bool tree = p->use_bcr;
  // the table entry of the first back-substitution behind the reduced solve, from what select_back / select_dense_back get
  const bool back = tree && !p->bcr_levels.empty();
  const int first_back_qm = back ? chain_variant(p->bcr_levels[size_t(rt.l_first)].q_max) : 0;
  const int v[kPlanInfoWords] = {p->fuse_expand ? 1 : 0, p->n_fitems, p->n_jac_items, p->n_cells, p->max_cell_frames, p->max_item_run,
                                 tree ? 1 : 0, p->m, p->bcr_all_active ? 1 : 0,
                                 tree ? p->bcr_N : 0, tree ? p->bcr_q0 : 0, tree ? int(p->bcr_levels.size()) : 0,
                                 tree && p->bcr_root >= 0 ? 1 : 0, rt.schur_rides ? 1 : 0, rt.ts.n, rt.fused ? 1 : 0,
                                 rt.reduced, rt.reduced_in_lds ? 1 : 0, rt.ks, sa.m, p->sep_n,
                                 rt.elim ? 1 : 0, rt.level0_roll ? 1 : 0, rt.dense_mode, rt.back_pre ? 1 : 0, rt.inline_nodes ? 1 : 0,
                                 first_back_qm, back ? (rt.ts.n > 0 ? 2 : 1) : 0};
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

}  // extern "C"
