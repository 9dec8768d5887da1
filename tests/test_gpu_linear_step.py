"""The LM step of the linear solvers against a dense solve of the system it claims to solve.

Every case builds a scene whose shape sends the solve down one route (tree solver: superblocks, chain length, levels, root,
where the Schur complement and the top separators' back-substitution ride, the fused dense solve; banded solver with or
without its separator; the reduced solve's kernel; Schur K-slices; ragged last superblocks; unobserved control points),
asserts through plan_info() that it does (the whole route: LinearRoute as calico_debug_plan_info reports it, down to the
(QM, MODE, PRE) of the back-substitution's table entry and the forms the solve's switches select), runs one LM iteration (or k of them) and holds the step the candidate update applied
(calico_debug_last_step) against tests/lm_step.py:

- the Jacobi scale and the damping, restated from Ceres, to 1e-13;
- the normwise backward error of the step for H + diag(d), <= 1e-11 (a backward-stable FP64 solve of a few thousand unknowns
  lands near 1e-15; a dropped or stale tile at 1e-6 and above -- tests/test_lm_step_reference.py);
- the forward error against a refined dense solve, <= 1e-11 kappa_2 where that is below 1e-3;
- the parameters after the solve = Plus(x, delta), the log's step_norm and relative_decrease.
"""
import numpy as np
import pytest

import lm_step
from calico_amd import _capi, synthetic as syn

pytestmark = pytest.mark.gpu

ETA_BOUND = 1e-11
# the scene's sensors: camera 0 (pinhole + radial-tangential, 8 intrinsics), gyroscope and accelerometer (IMU model 2)
CAM, GYRO, ACCEL = 0, 1, 2
# free calibration blocks -> tangent width mc: (intrinsics, extrinsics, latency) per sensor and the number of free model points
_MC = {
    "all": (((True, False, False), (True, True, True), (True, True, True)), 0),      # 8 + 11 + 11 = 30
    0: (((False, False, False),) * 3, 0),
    1: (((False, False, False), (False, False, True), (False, False, False)), 0),
    15: (((True, False, False), (False, True, True), (False, False, False)), 0),
    16: (((True, False, False), (True, False, False), (True, False, False)), 0),
    17: (((True, False, False), (True, False, True), (True, False, False)), 0),
    97: (((True, False, False), (False, False, False), (True, True, True)), 26),      # 8 + 11 + 3 * 26: a.m + 1 = 128 with the root
    98: (((True, False, False), (False, False, False), (False, False, False)), 30),    # 8 + 3 * 30: a.m + 1 = 129 (blocked)
    428: (((True, False, False), (False, False, False), (False, False, False)), 140),  # 8 + 3 * 140: blocked, several panels
}


def make_case_scene(n_cp=57, order=6, mc="all", unobserved=None, perturb_ctrl=0.0, seed=5):
    """One camera and an IMU over a trajectory of exactly n_cp control points (10 Hz knots)."""
    T = (n_cp - order + 0.5) / 10.0
    short = n_cp < 12
    chart = "april" if _MC[mc][1] > 30 else "plane"
    scene = syn.make_scene(1, 1, True, 2, cam_rate=20.0 if short else 4.0, imu_rate=200.0 if short else 40.0,
                           duration=T * 5.0 / 8.7 if unobserved == "tail" else T, segment_duration=T / 23.9, order=order,
                           chart=chart, pixel_noise=0.1, gyro_noise=1e-3, accel_noise=1e-2, seed=seed)
    assert len(scene.ctrl) == n_cp
    flags, n_points = _MC[mc]
    for s, (fi, fe, fl) in zip(scene.sensors, flags):
        s.enable_intrinsics, s.enable_extrinsics, s.enable_latency = fi, fe, fl
    if unobserved == "middle":
        # no observation over 1.2 s (12 segments, more than k) in the middle of the trajectory
        t0 = 0.4 * T
        for s in scene.sensors:
            keep = (s.stamps < t0) | (s.stamps > t0 + 1.2)
            s.meas, s.stamps = s.meas[keep], s.stamps[keep]
            if s.point_idx is not None:
                s.point_idx, s.is_outlier = s.point_idx[keep], s.is_outlier[keep]
    if n_points:
        seen = np.unique(scene.sensors[CAM].point_idx)
        assert len(seen) >= n_points + 3
        pc = np.ones(len(scene.points), bool)
        pc[seen[:n_points]] = False
        scene.points_constant = pc
    if perturb_ctrl:
        scene.ctrl = scene.ctrl + perturb_ctrl * np.random.default_rng(1).standard_normal(scene.ctrl.shape)
    return scene


def _options(api, budget, mu, jacobi, lm_diag):
    o = api.default_options()
    o.minimizer_progress_to_stdout = 0
    o.max_num_iterations = budget
    o.initial_trust_region_radius = mu
    o.jacobi_scaling = int(jacobi)
    if lm_diag is not None:
        o.min_lm_diagonal, o.max_lm_diagonal = lm_diag
    return o


def check_steps(hip, scene, expect, mu=1.0, jacobi=True, iters=(1,), lm_diag=None, label="", rejected_before=None, keep=None):
    """Build, assert the route, and check the step of every iteration in `iters` (see the module's docstring). `keep`: a
    list that takes the built problem, for a caller that wants the handle to outlive the call."""
    built = syn.build_problem(hip, scene)
    if keep is not None:
        keep.append(built)
    P = built.problem
    info = P.plan_info()
    route = {k: info[k] for k in ("tree_solver", "m", "superblocks", "chain", "levels", "root", "schur_rides", "top_seps",
                                  "fused_back", "reduced_route", "reduced_in_lds", "schur_slices", "reduced_m", "sep_n",
                                  "all_control_points_observed", "elim", "level0_roll", "dense_mode", "back_pre", "inline_nodes",
                                  "first_back_qm", "first_back_mode")}
    for k, v in expect.items():
        assert info[k] == v, (label, k, info[k], v, route)
    cols = lm_step.column_blocks(built, scene)
    all_ids = np.array(sorted(P._sizes), np.int32)
    all_sizes = [P._sizes[int(i)] for i in all_ids]
    x_all0 = P.get_param_blocks(all_ids, all_sizes)
    x0 = lm_step.block_values(P, cols)
    c0, g0, H0 = P.evaluate()
    n = len(g0)
    assert sum(3 if m == lm_step.MANIFOLD_EIGEN_QUATERNION else v.size for v, m in x0) == n
    s_ref = lm_step.jacobi_scale(H0, jacobi)
    active = lm_step.control_points_observed(scene)
    NT = 6 * len(scene.ctrl) + info["m"]
    worst = 0.0
    for it in iters:
        if it > 1:
            P.set_param_blocks(all_ids, x_all0)
            P.solve(_options(hip, it - 1, mu, jacobi, lm_diag))
            xs = lm_step.block_values(P, cols)
            cost, g, H = P.evaluate()
        else:
            xs, cost, g, H = x0, c0, g0, H0
        P.set_param_blocks(all_ids, x_all0)
        o = _options(hip, it, mu, jacobi, lm_diag)
        P.solve(o)
        log = P.iterations()
        assert len(log) == it + 1, (label, it, len(log))
        row, radius = log[it], log[it - 1].trust_region_radius
        if rejected_before is not None and it == rejected_before + 1:
            assert not log[rejected_before].step_is_successful, label
        step, damp, scale = P.last_step()
        # the Jacobi scale of the solve's start, the damping of this iteration's radius
        assert np.all(np.abs(scale - s_ref) <= 1e-13 * s_ref), label
        d_ref = lm_step.damping(H, s_ref, radius, o.min_lm_diagonal, o.max_lm_diagonal)
        assert np.all(np.abs(damp - d_ref) <= 1e-13 * d_ref), (label, np.abs(damp - d_ref).max())
        if lm_diag is not None:
            # (at the start both sides bind; later iterations' smaller J^T J may sit below the lower bound everywhere)
            binds = lm_step.clamp_binds(H, s_ref, *lm_diag)
            assert 0 < binds.sum() and (it > 1 or binds.sum() < n), label
        full_step, full_damp, _ = P.last_step(NT)
        inactive = np.repeat(~active, 6)
        assert np.all(full_step[:inactive.size][inactive] == 0.0) and np.all(full_damp[:inactive.size][inactive] == 0.0), label
        # the step against the dense solve
        long = n > 4200
        eta = (lm_step.backward_error_f64 if long else lm_step.backward_error)(H, g, damp, step)
        A = H + np.diag(damp)
        eta_np = (lm_step.backward_error_f64 if long else lm_step.backward_error)(H, g, damp, np.linalg.solve(A, -g))
        msg = "%s it %d: n %d mu %.1e" % (label, it, n, radius)
        if not long:
            kappa = lm_step.kappa2(H, damp)
            delta_ref = lm_step.reference_step(H, g, damp)
            fe = lm_step.forward_error(H, damp, step, delta_ref)
            msg += " kappa %.2e eta %.2e (numpy float64 %.2e) forward %.2e" % (kappa, eta, eta_np, fe)
        else:
            msg += " eta(f64 residual) %.2e (numpy %.2e)" % (eta, eta_np)
        print(msg, "route", route)
        assert eta <= ETA_BOUND, msg
        if not long and ETA_BOUND * kappa < 1e-3:
            assert fe <= ETA_BOUND * kappa, msg
        worst = max(worst, eta)
        # the step that was used
        new = lm_step.plus(xs, step)
        after = lm_step.block_values(P, cols)
        if row.step_is_successful:
            for (v1, _), w, (v0, _) in zip(after, new, xs):
                assert np.all(np.abs(v1 - w) <= 1e-14 * np.maximum(1.0, np.abs(v0))), (label, v1, w)
        else:
            for (v1, _), (v0, _) in zip(after, xs):
                assert np.array_equal(v1, v0), label
        sn = lm_step.step_norm(xs, new)
        assert abs(row.step_norm - sn) <= 1e-10 * sn, (msg, row.step_norm, sn)
        mcc = lm_step.model_cost_change(H, g, step)
        if row.step_is_valid and np.isfinite(row.relative_decrease) and abs(row.cost_change) < 1e300 and mcc > 1e-6 * cost:
            assert abs(row.relative_decrease - row.cost_change / mcc) <= 1e-8 * abs(row.relative_decrease), msg
    return info, worst


# ---- the sweep: one axis at a time around a base case (order 6, 57 control points, 30 calibration columns, mu = 1) ----
CASES = {
    # tree structure
    "N=1 (order 4, 5 control points)": dict(scene=dict(n_cp=5, order=4), expect=dict(superblocks=1, root=0, levels=1)),
    "one chain, no root (leaf 8)": dict(env=dict(CALICO_BCR_LEAF="8"), scene=dict(n_cp=40), expect=dict(superblocks=8, chain=8, root=0, levels=1)),
    "N = q + 1 (one level, own Schur launch)": dict(env=dict(CALICO_BCR_LEAF="4"), scene=dict(n_cp=25),
                                                    expect=dict(superblocks=5, levels=1, root=1, schur_rides=0)),
    "two levels (Schur rides, top separators, fused)": dict(env=dict(CALICO_BCR_LEAF="4"), scene=dict(n_cp=70),
                                                            expect=dict(levels=2, root=1, schur_rides=1, top_seps=1, fused_back=1)),
    "three levels, last of two nodes": dict(env=dict(CALICO_BCR_LEAF="1"), scene=dict(n_cp=75),
                                            expect=dict(levels=3, root=1, schur_rides=1, top_seps=2, fused_back=0)),
    "level L-2 with chains of 5 (top separators not folded)": dict(env=dict(CALICO_BCR_LEAF="5"), scene=dict(n_cp=85),
                                                                   expect=dict(levels=2, chain=5, top_seps=0, fused_back=0)),
    # unobserved control points
    "unobserved tail": dict(scene=dict(n_cp=92, unobserved="tail"), expect=dict(all_control_points_observed=0)),
    "unobserved middle": dict(scene=dict(n_cp=92, unobserved="middle"), expect=dict(all_control_points_observed=0)),
    "unobserved middle, banded": dict(env=dict(CALICO_SOLVER="band"), scene=dict(n_cp=92, unobserved="middle"),
                                      expect=dict(tree_solver=0, all_control_points_observed=0, sep_n=0)),
    # calibration width
    "mc 0 with a root (block solve)": dict(scene=dict(n_cp=40, mc=0), expect=dict(m=0, root=1, reduced_route=1, reduced_m=30)),
    "mc 0 without a root (panel kernel)": dict(env=dict(CALICO_BCR_LEAF="8"), scene=dict(n_cp=40, mc=0),
                                               expect=dict(m=0, root=0, reduced_route=0, reduced_m=0)),
    "mc 0 ragged, speculative (buffer 1 over-read)": dict(scene=dict(n_cp=41, mc=0), iters=(1, 2, 3), expect=dict(m=0, superblocks=9)),
    "mc 0 banded, no split (panel kernel)": dict(env=dict(CALICO_SOLVER="band", CALICO_BAND_SPLIT="0"), scene=dict(n_cp=40, mc=0),
                                                 expect=dict(tree_solver=0, m=0, sep_n=0, reduced_route=0)),
    "mc 1": dict(scene=dict(mc=1), expect=dict(m=1)),
    "mc 15": dict(scene=dict(mc=15), expect=dict(m=15)),
    "mc 16": dict(scene=dict(mc=16), expect=dict(m=16)),
    "mc 17": dict(scene=dict(mc=17), expect=dict(m=17)),
    "mc 97 (128 reduced unknowns)": dict(scene=dict(mc=97), expect=dict(m=97, root=1, reduced_m=127, reduced_route=1)),
    "mc 98 (129: blocked)": dict(scene=dict(mc=98), expect=dict(m=98, root=1, reduced_m=128, reduced_route=2)),
    "mc 428 (blocked, several panels)": dict(scene=dict(mc=428), expect=dict(m=428, reduced_route=2)),
    # spline orders
    "order 2": dict(scene=dict(order=2), expect=dict(tree_solver=1)),
    "order 3": dict(scene=dict(order=3), expect=dict(tree_solver=1)),
    "order 4": dict(scene=dict(order=4), expect=dict(tree_solver=1)),
    "order 5": dict(scene=dict(order=5), expect=dict(tree_solver=1)),
    "order 7 (banded, split)": dict(scene=dict(n_cp=60, order=7), expect=dict(tree_solver=0, sep_n=6, level0_roll=0)),
    "order 8 (banded, split)": dict(scene=dict(n_cp=60, order=8), expect=dict(tree_solver=0, sep_n=7, level0_roll=0)),
    "order 7 (banded, no split)": dict(env=dict(CALICO_BAND_SPLIT="0"), scene=dict(n_cp=60, order=7),
                                       expect=dict(tree_solver=0, sep_n=0, level0_roll=0)),
    "order 6 banded, split": dict(env=dict(CALICO_SOLVER="band", CALICO_BAND_SPLIT="1"), scene=dict(), expect=dict(tree_solver=0, sep_n=5)),
    "order 6 banded, no split": dict(env=dict(CALICO_SOLVER="band", CALICO_BAND_SPLIT="0"), scene=dict(), expect=dict(tree_solver=0, sep_n=0)),
    # length: Schur K-slices
    "160 control points": dict(scene=dict(n_cp=160), expect=dict(schur_slices=1)),
    "320 control points": dict(scene=dict(n_cp=320), expect=dict(schur_slices=2)),
    "640 control points": dict(scene=dict(n_cp=640), expect=dict(schur_slices=4)),
    # LM settings
    "mu 1e-3": dict(mu=1e-3),
    "mu 1e4": dict(mu=1e4),
    "mu 1e10": dict(mu=1e10),
    "no Jacobi scaling": dict(jacobi=False),
    "iterations 1, 2, 3": dict(iters=(1, 2, 3)),
    "after a rejected step": dict(scene=dict(n_cp=40, perturb_ctrl=0.5), mu=1e16, iters=(2, 3), rejected_before=2),
}
for _n in range(40, 45):       # ragged ends: n_cp mod 5 = 0 .. 4, orders 6 and 4, the plan's chain length and chains of one
    for _k in (6, 4):
        CASES["ragged n_cp %d order %d" % (_n, _k)] = dict(scene=dict(n_cp=_n, order=_k), expect=dict(superblocks=(_n + 4) // 5))
        CASES["ragged n_cp %d order %d q 1" % (_n, _k)] = dict(env=dict(CALICO_BCR_LEAF="1"), scene=dict(n_cp=_n, order=_k),
                                                             expect=dict(superblocks=(_n + 4) // 5, chain=1))
for _q in range(1, 9):         # chain lengths on 185 control points
    CASES["185 control points, chains of %d" % _q] = dict(env=dict(CALICO_BCR_LEAF=str(_q)), scene=dict(n_cp=185),
                                                          expect=dict(superblocks=37, chain=_q))
# A/B switches of the tree solver on one two-level scene (14 superblocks = 3 * 4 + 2: chains of four, the top separator folded into
# level 0's back-substitution, 61 reduced unknowns -- too few for the affine form to pay), each with the route words that prove its form
for (_name, _v), _route in {
        ("CALICO_ROLL", "0"): dict(level0_roll=0, elim=1, dense_mode=2),                      # bcr_level_kernel<true, true>
        ("CALICO_DENSE_ROLL", "0"): dict(dense_mode=1, elim=1, level0_roll=1),
        ("CALICO_FUSE_BACK", "0"): dict(fused_back=0, back_pre=0, first_back_qm=4, first_back_mode=2),      # bcr_back_kernel<4, 2>
        ("CALICO_BACK_PRE", "0"): dict(fused_back=1, back_pre=0, first_back_qm=4, first_back_mode=2),       # dense_back_kernel<4, 2, false>
        ("CALICO_BACK_PRE", "1"): dict(fused_back=1, back_pre=1, first_back_qm=4, first_back_mode=2),       # dense_back_kernel<4, 2, true>
        ("CALICO_ELIM", "panel"): dict(elim=0, dense_mode=0, level0_roll=0),                  # bcr_level_kernel<.., false>
        ("CALICO_SPECULATIVE", "0"): dict(elim=1, level0_roll=1, dense_mode=2, back_pre=0),
        ("CALICO_INLINE_NODES", "0"): dict(inline_nodes=0)}.items():
    CASES["two levels, %s=%s" % (_name, _v)] = dict(env={"CALICO_BCR_LEAF": "4", _name: _v}, scene=dict(n_cp=70), iters=(1, 2),
                                                    expect=dict(dict(levels=2, top_seps=1, fused_back=1), **_route))

# Every entry of the kernels' variant tables (dense_back_kernel<QM, MODE, PRE>, bcr_back_kernel<QM, MODE>, band_backsolve_kernel<K>)
# that no case above reaches. A one-level tree of chains of q has q + 1 superblocks; a two-level one whose top separator is
# back-substituted in level 0's launch (MODE 2) has 3 q + 2; five control points to a superblock.
for _q, _n_cp, _levels, _switch in (
        (1, 10, 1, "CALICO_BACK_PRE=1"), (2, 15, 1, "CALICO_BACK_PRE=1"), (4, 25, 1, "CALICO_BACK_PRE=1"),      # dense_back_kernel<QM, 1, true>
        (1, 25, 2, "CALICO_BACK_PRE=1"), (2, 40, 2, "CALICO_BACK_PRE=1"),                                        # <QM, 2, true>
        (2, 15, 1, None), (1, 25, 2, None), (2, 40, 2, None),                                                    # <2, 1, false>, <QM, 2, false>
        (2, 15, 1, "CALICO_FUSE_BACK=0"), (4, 25, 1, "CALICO_FUSE_BACK=0"), (2, 40, 2, "CALICO_FUSE_BACK=0")):   # bcr_back_kernel<QM, 1>, <2, 2>
    CASES["chains of %d, %d level(s), %s" % (_q, _levels, _switch or "fused")] = dict(
        env=dict([("CALICO_BCR_LEAF", str(_q))] + ([_switch.split("=")] if _switch else [])), scene=dict(n_cp=_n_cp),
        expect=dict(levels=_levels, chain=_q, root=1, top_seps=_levels - 1, fused_back=0 if _switch == "CALICO_FUSE_BACK=0" else 1,
                    back_pre=1 if _switch == "CALICO_BACK_PRE=1" else 0, first_back_qm=_q, first_back_mode=_levels))
for _k in (2, 3, 4, 5):
    CASES["order %d banded" % _k] = dict(env=dict(CALICO_SOLVER="band"), scene=dict(n_cp=25, order=_k), expect=dict(tree_solver=0))


@pytest.mark.parametrize("name", list(CASES))
def test_linear_step_matches_dense_solve(name, hip, monkeypatch):
    c = CASES[name]
    for k, v in c.get("env", {}).items():
        monkeypatch.setenv(k, v)
    scene = make_case_scene(**c.get("scene", {}))
    # what a case does not say otherwise is the default route: elimination by blocks, rolling owners in the dense solve, and on
    # the tree solver (every case that does not expect the banded one) level 0's rolling chief and inline node descriptors
    expect = dict(c.get("expect", {}))
    tree = expect.get("tree_solver", 1)
    for k, v in dict(tree_solver=tree, elim=1, dense_mode=2, level0_roll=tree, inline_nodes=tree).items():
        expect.setdefault(k, v)
    check_steps(hip, scene, expect, mu=c.get("mu", 1.0), jacobi=c.get("jacobi", True), iters=c.get("iters", (1,)),
                label=name, rejected_before=c.get("rejected_before"))


def test_linear_step_with_a_binding_damping_clamp(hip):
    """min_lm_diagonal / max_lm_diagonal at the quartiles of the scaled diagonal: the clamp binds on both sides."""
    scene = make_case_scene()
    built = syn.build_problem(hip, scene)
    _, _, H0 = built.problem.evaluate()
    v = np.diag(H0) * lm_step.jacobi_scale(H0) ** 2
    check_steps(hip, scene, {}, lm_diag=(float(np.quantile(v, 0.25)), float(np.quantile(v, 0.75))), iters=(1, 2), label="clamp")


def test_last_step_needs_a_solve(hip):
    """The hook refuses to report a step of other values than the ones the last solve started from."""
    scene = make_case_scene(n_cp=25)
    built = syn.build_problem(hip, scene)
    P = built.problem
    with pytest.raises(_capi.CalicoError) as e:
        P.last_step()
    assert e.value.code == _capi.FAILED_PRECONDITION
    P.solve(_options(hip, 1, 1.0, True, None))
    P.last_step()
    P.set_param_block(int(built.ctrl_blocks[0]), scene.ctrl[0])
    with pytest.raises(_capi.CalicoError) as e:
        P.last_step()
    assert e.value.code == _capi.FAILED_PRECONDITION
