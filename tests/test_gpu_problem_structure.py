"""Problem structures the other GPU tests hold fixed, against the CPU oracle: several rigid bodies (constant, free, sparse,
partly seen, unseen, with free model points, interleaved inside a frame), rigs that mix camera models (and layouts on both
sides of the frame path's limits), and observations registered in another order than time order (permuted, reversed, in
several calls interleaved across the sensors). Scenes: structure_scenes.py; that their converged solves mean something:
test_problem_structure_oracle.py.

Unless a test says otherwise it compares as test_gpu_parity.assert_eval_close does -- cost, gradient and JᵀJ to 1e-9 --,
every sensor's residuals to 1e-9 max(1, |r|) with equal valid flags and the tau = 3 inlier masks bit for bit, residuals and
masks in REGISTRATION order, and asserts through plan_info() that the scene takes the route it was built for.

Measured (MI355X), worst over the cases of this file: cost 3.3e-15, gradient 1.7e-11, JᵀJ 5.6e-11, residuals 3.8e-12 -- all of
them the mixed rig (1, 3, 7) after five LM iterations; at the start values no case is above 6.1e-13 (JᵀJ). Residuals and
project() of a permuted build equal the sorted build's bit for bit. Converged solves: same iterations, cost per iteration
within 3.6e-12 of the oracle's. Covariance with a free body 2.3e-8 of the 1e-7 bound's measure, prediction covariance 3.9e-10.
Plan cache, a sorted build followed by a permuted build of the same observations: a miss (the key covers the registration
order); both evaluate to their oracle.
What a mutated library shows (one build each): body 0's bq_off / bt_off for every layout -- every test with a second body
fails; no per-cell stable_sort -- passes every 10 Hz case (a camera cell is then one frame, and IMU blocks do not care about
their order), which is what the 30 Hz registration cases were added for; residual read-back without
sorted_pos -- the registration, interleaved, free-point and plan-cache cases fail."""
import copy

import numpy as np
import pytest

import lm_step
import prediction_ref as pr
import structure_scenes as ss
import test_gpu_covariance as cov_tests
import test_gpu_linear_step as step_tests
import test_gpu_prediction_covariance as pred_tests
from calico_amd import _capi, synthetic as syn
from helpers import border_layout, run_two_ranks, solve
from test_gpu_parity import assert_estimates_close, solve_both

pytestmark = pytest.mark.gpu

TAU = 3.0


def both(sc, hip, oracle):
    return syn.build_problem(hip, sc), syn.build_problem(oracle, sc)


def eval_errors(gpu, ref):
    """(cost, gradient, JᵀJ) errors in assert_eval_close's measures."""
    cg, gg, Hg = gpu.problem.evaluate()
    cr, gr, Hr = ref.problem.evaluate()
    assert Hg.shape == Hr.shape
    sg = np.sqrt(np.diag(Hr))
    sg = np.where(sg > 0, sg, 1.0)
    return abs(cg - cr) / abs(cr), np.abs(gg - gr).max() / np.abs(gr).max(), (np.abs(Hg - Hr) / np.outer(sg, sg)).max()


def check_parity(gpu, ref, sc, what, masks=True):
    """The module's comparison; prints the figures before it asserts them."""
    ec, eg, eH = eval_errors(gpu, ref)
    er = 0.0
    rows = []
    for i, s in enumerate(sc.sensors):
        rg, vg = gpu.problem.residuals(gpu.sensor_ids[i], s.n, s.dim)
        rr, vr = ref.problem.residuals(ref.sensor_ids[i], s.n, s.dim)
        rows.append((rg, vg, rr, vr))
        if s.n:
            er = max(er, np.abs(rg - rr).max() / max(1.0, np.abs(rr).max()))
    print("evaluation parity %s: cost %.2e gradient %.2e JtJ %.2e residuals %.2e" % (what, ec, eg, eH, er))
    assert ec <= 1e-9 and eg <= 1e-9 and eH <= 1e-9, (what, ec, eg, eH)
    for i, (s, (rg, vg, rr, vr)) in enumerate(zip(sc.sensors, rows)):
        assert np.array_equal(vg, vr), (what, i)
        if s.n:
            assert np.abs(rg - rr).max() <= 1e-9 * max(1.0, np.abs(rr).max()), (what, i)
        if masks:
            assert np.array_equal(gpu.problem.inlier_mask(gpu.sensor_ids[i], s.n, TAU),
                                  ref.problem.inlier_mask(ref.sensor_ids[i], s.n, TAU)), (what, i)
    return max(ec, eg, eH, er)


def free_point(sc, body, point):
    return not np.broadcast_to(np.asarray(sc.bodies[body].points_constant, bool), (len(sc.bodies[body].points),))[point]


def expected_plan(sc, frame_path):
    """ss.expected_plan plus the work items of everything off the frame path: an IMU cell (sensor, segment) in chunks of 21
    blocks, a camera's other observations per (body, free model point or none, segment) in chunks of 64."""
    exp = ss.expected_plan(sc, frame_path)
    items = 0
    for c, s in enumerate(sc.sensors):
        seg = syn.spline_index(sc.knots, sc.order, s.stamps)
        if s.kind != _capi.SENSOR_CAMERA:
            items += sum(-(-n // 21) for n in np.unique(seg, return_counts=True)[1])
            continue
        body = syn.body_indices(s)
        groups = {}
        for b, pt, sg in zip(body, s.point_idx, seg):
            if not frame_path(c, int(b)):
                key = (int(b), int(pt) if free_point(sc, int(b), int(pt)) else -1, int(sg))
                groups[key] = groups.get(key, 0) + 1
        items += sum(-(-n // 64) for n in groups.values())
    exp["items"] = items
    return exp


def assert_plan(gpu, sc, frame_path, fused):
    """The route: fuse_expand as given; a cell per (camera, body, segment) on the frame path and per (IMU sensor, segment);
    the work items off the frame path; and, without cell workgroups (whose frame table is padded), the frames."""
    info = gpu.problem.plan_info()
    exp = expected_plan(sc, frame_path)
    assert info["fuse_expand"] == int(fused), info
    assert info["tree_solver"] == 1 and info["frames"] > 0, info
    assert info["cells"] == exp["cam_cells"] + exp["imu_cells"], (info, exp)
    assert info["items"] == exp["items"], (info, exp)
    if not fused:
        assert info["frames"] == exp["frames"], (info, exp)
    return info, exp


# ---------------------------------------------------------------- several bodies
@pytest.mark.parametrize("cam_rate", [10.0, 30.0])
def test_two_constant_charts(cam_rate, hip, oracle):
    sc = ss.scene(1, [ss.chart1()], cam_rate=cam_rate)
    gpu, ref = both(sc, hip, oracle)
    info, exp = assert_plan(gpu, sc, lambda c, b: True, fused=cam_rate == 10.0)
    one = ss.expected_plan(ss.scene(1, [], cam_rate=cam_rate), lambda c, b: True)
    assert exp["cam_cells"] == 2 * one["cam_cells"]          # both bodies in every (camera, segment)
    if cam_rate == 30.0:
        assert info["max_frames_per_cell"] >= 3, info
    check_parity(gpu, ref, sc, "two constant charts, %g Hz" % cam_rate)


@pytest.mark.parametrize("model", [1, 3, 6])
def test_second_chart_free(model, hip, oracle):
    """Staged width P = 7 + K + 3 for the free body: 18 (model 1), 17 (model 3: one past the pad of 16), 14 (model 6)."""
    sc = ss.second_chart_free(model)
    gpu, ref = both(sc, hip, oracle)
    assert_plan(gpu, sc, lambda c, b: True, fused=True)      # both bodies on the frame path, no camera work item
    assert gpu.problem.num_effective_parameters() == ref.problem.num_effective_parameters()
    check_parity(gpu, ref, sc, "second chart free, model %d" % model)


def test_opencv8_with_a_free_body(hip, oracle):
    """Model 2 against a free body: P = 21 for camera 0 (11 + 6 = 17 calibration columns, on the frame path). Camera 1 adds
    its extrinsics and latency: 24 columns, one more than the frame path takes -- its body-1 layout becomes work items."""
    sc = ss.second_chart_free(2)
    gpu, ref = both(sc, hip, oracle)
    assert_plan(gpu, sc, lambda c, b: not (c == 1 and b == 1), fused=False)
    check_parity(gpu, ref, sc, "second chart free, model 2")


def test_sparse_second_chart(hip, oracle):
    """Six points a frame: body 1's layouts leave the frame path, body 0's stay -- frames, camera work items and IMU row
    cells in one problem."""
    sc = ss.scene(1, [ss.sparse_chart(free_pose=True)])
    gpu, ref = both(sc, hip, oracle)
    info, exp = assert_plan(gpu, sc, lambda c, b: b == 0, fused=False)
    assert info["items"] > exp["imu_cells"]          # camera work items next to the IMU's
    check_parity(gpu, ref, sc, "sparse second chart")


def test_partly_seen_and_unseen_bodies(hip, oracle):
    """Body 1: only camera 1, only the middle third. Body 2: registered, free, never observed."""
    unseen = syn.rigid_body(syn.planar_points(0.5, 0.5, 0.25), t=(-0.5, 0.2, 0.1), free_pose=True, seen_by=[])
    sc = ss.scene(1, [ss.chart1(free_pose=True, seen_by=[1], window=(1.0, 2.0)), unseen])
    assert [int((syn.body_indices(s) == 1).sum()) > 0 for s in sc.sensors[:2]] == [False, True]
    assert all(int((syn.body_indices(s) == 2).sum()) == 0 for s in sc.sensors[:2])
    gpu, ref = both(sc, hip, oracle)
    assert gpu.problem.num_effective_parameters() == ref.problem.num_effective_parameters()
    check_parity(gpu, ref, sc, "partly seen, unseen")
    before = syn.read_back_bodies(gpu, sc)[2]
    gpu, ref, sg, sr = solve_both(sc, hip, oracle, max_iter=5)
    for key in ("num_residual_blocks", "num_residuals", "num_parameter_blocks", "num_parameters", "num_effective_parameters",
                "num_residual_blocks_reduced", "num_residuals_reduced", "num_parameter_blocks_reduced", "num_parameters_reduced",
                "num_effective_parameters_reduced"):
        assert getattr(sg, key) == getattr(sr, key), key
    after = syn.read_back_bodies(gpu, sc)
    assert np.array_equal(after[2]["q"], before["q"]) and np.array_equal(after[2]["t"], before["t"])
    assert np.abs(after[1]["t"] - sc.extra_bodies[0].t).max() > 0      # the seen one did move
    assert_estimates_close(gpu, ref, sc)


def test_free_points_on_the_second_chart(hip, oracle):
    """Layouts per (sensor, body, point) for body 1's 17 free points: those leave the frame path, body 0 stays."""
    sc = ss.scene(1, [ss.chart1(free_pose=True, free_points=True)])
    assert int((~sc.extra_bodies[0].points_constant).sum()) == 17
    gpu, ref = both(sc, hip, oracle)
    assert_plan(gpu, sc, lambda c, b: b == 0, fused=False)
    check_parity(gpu, ref, sc, "free points on the second chart")


def test_bodies_interleaved_inside_the_frame(hip, oracle):
    """b0, b1, b0, b1, ... inside every frame: the layout changes with every observation. The device order (layout, segment,
    stamp, ties in insertion order) is that of the body-by-body registration, so the evaluation is the same, bit for bit."""
    sc = ss.second_chart_free(1)
    mixed = syn.reorder(sc, ss.interleave_bodies(sc))
    assert np.any(np.diff(syn.body_indices(mixed.sensors[0])[:40]) != 0)
    gpu, ref = both(sc, hip, oracle)
    gpu2, ref2 = both(mixed, hip, oracle)
    assert_plan(gpu2, mixed, lambda c, b: True, fused=True)
    check_parity(gpu, ref, sc, "body by body")
    check_parity(gpu2, ref2, mixed, "interleaved in the frame")
    a, b = gpu.problem.evaluate(), gpu2.problem.evaluate()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---------------------------------------------------------------- mixed rigs
@pytest.mark.parametrize("models", ss.MIXED_RIGS)
def test_mixed_rig(models, hip, oracle):
    sc = ss.mixed_rig(models)
    gpu, ref = both(sc, hip, oracle)
    assert_plan(gpu, sc, lambda c, b: True, fused=True)
    check_parity(gpu, ref, sc, "mixed rig %s, start" % (models,))
    if models == (1, 3, 7):
        solve(gpu.problem, hip, 5)
        pr.copy_values(gpu, ref)
        check_parity(gpu, ref, sc, "mixed rig %s, after five iterations" % (models,))


def test_rig_across_the_frame_paths_column_limit(hip, oracle):
    """Every camera estimates intrinsics, extrinsics and latency against a free second body. Calibration columns per
    layout: model 1 -- 8 + 6 + 1 = 15 on body 0, 21 with body 1's pose; model 2 -- 11 + 6 + 1 = 18 on body 0, 24 with body 1's
    pose. The frame path takes at most 23: three layouts stay on it, (camera 1, body 1) becomes work items."""
    sc = ss.column_limit_rig((1, 2))
    gpu, ref = both(sc, hip, oracle)
    info, exp = assert_plan(gpu, sc, lambda c, b: not (c == 1 and b == 1), fused=False)
    cam1 = sc.sensors[1]
    seg = syn.spline_index(sc.knots, sc.order, cam1.stamps[syn.body_indices(cam1) == 1])
    assert exp["items"] - exp["imu_cells"] == len(np.unique(seg)) > 0      # 20 points a frame, one or two frames: one item
    assert info["m"] == (8 + 6 + 1) + (11 + 6 + 1) + 6 + 2 * (4 + 6 + 1)      # cameras, body 1's pose, gyroscope and accelerometer
    check_parity(gpu, ref, sc, "rig across the column limit")


# ---------------------------------------------------------------- registration order
def _order_scene(cam_rate):
    return ss.scene(1, [ss.chart1(free_pose=True)], outlier_fraction=0.03, seed=9, cam_rate=cam_rate)


@pytest.mark.parametrize("cam_rate", [10.0, 30.0])
@pytest.mark.parametrize("name", ["random", "reverse", "three calls"])
def test_registration_order(name, cam_rate, hip, oracle):
    """At 10 Hz a camera cell (layout, segment) is one frame: the counting sort over the cells orders everything. At 30 Hz a
    cell holds three frames, and a cell registered out of time order needs its stamps sorted before frames can be cut."""
    sc = _order_scene(cam_rate)
    variants, perms = ss.registration_variants(sc)
    v, perm = variants[name], perms[name]
    base = syn.build_problem(hip, sc)
    gpu, ref = both(v, hip, oracle)
    info, _ = assert_plan(gpu, v, lambda c, b: True, fused=cam_rate == 10.0)
    assert info["max_frames_per_cell"] >= (3 if cam_rate == 30.0 else 1), info
    check_parity(gpu, ref, v, "registration order: %s, %g Hz" % (name, cam_rate))
    P, B = gpu.problem, base.problem
    # the sorted build, row for row through the permutation: neither the arithmetic nor its inputs depend on where an
    # observation was registered
    for i, s in enumerate(v.sensors):
        r0, v0 = B.residuals(base.sensor_ids[i], s.n, s.dim)
        r1, v1 = P.residuals(gpu.sensor_ids[i], s.n, s.dim)
        assert np.array_equal(r1, r0[perm[i]]) and np.array_equal(v1, v0[perm[i]]), i
        p0, w0 = B.project(base.sensor_ids[i], s.n, s.dim)
        p1, w1 = P.project(gpu.sensor_ids[i], s.n, s.dim)
        assert np.array_equal(p1, p0[perm[i]]) and np.array_equal(w1, w0[perm[i]]), i
    cams = [i for i, s in enumerate(v.sensors) if s.kind == _capi.SENSOR_CAMERA]
    # heat map: integer feature counts per bin
    for i in cams:
        assert np.array_equal(P.residual_heatmap(gpu.sensor_ids[i], 1280, 800)[1], B.residual_heatmap(base.sensor_ids[i], 1280, 800)[1])
    # one tagging pass against the oracle's inlier mask
    n_marked = 0
    for i in cams:
        s = v.sensors[i]
        inl = ref.problem.inlier_mask(ref.sensor_ids[i], s.n, TAU).astype(bool)
        assert not np.any(inl & ~ref.problem.residuals(ref.sensor_ids[i], s.n, 2)[1].astype(bool))
        marked = P.mark_outliers(gpu.sensor_ids[i], TAU)
        assert marked == int((~inl).sum())
        n_marked += marked
        _, valid = P.residuals(gpu.sensor_ids[i], s.n, 2, check=False)
        assert np.array_equal(valid.astype(bool), inl)
        assert (~inl)[s.is_outlier].mean() > 0.9
    assert n_marked > 0
    # a fixed subset, given in registration order, against an oracle built without it
    less = copy.deepcopy(v)
    less.calls = None
    n_less = 0
    for i in cams:
        s, s2 = v.sensors[i], less.sensors[i]
        drop = np.arange(s.n) % 7 == 3
        P.set_outlier_mask(gpu.sensor_ids[i], drop.astype(np.uint8))
        for key in ("meas", "stamps", "point_idx", "body_idx", "is_outlier"):
            setattr(s2, key, getattr(s, key)[~drop])
        n_less += int(drop.sum())
    ref2 = syn.build_problem(oracle, less)
    cg, cr = P.evaluate()[0], ref2.problem.evaluate()[0]
    print("registration order %s: cost without the subset, relative difference %.2e" % (name, abs(cg - cr) / cr))
    assert abs(cg - cr) <= 1e-9 * cr
    og, orr = hip.default_options(), oracle.default_options()
    for o in (og, orr):
        o.minimizer_progress_to_stdout, o.max_num_iterations = 0, 1
    sg, sr = P.solve(og), ref2.problem.solve(orr)
    assert sg.num_residual_blocks == sr.num_residual_blocks == v.num_blocks - n_less
    for i in cams:
        P.set_outlier_mask(gpu.sensor_ids[i], None)
    assert P.solve(og).num_residual_blocks == v.num_blocks


# ---------------------------------------------------------------- solves
def _converged_pair(name, hip, oracle):
    sc = ss.SOLVE_SCENES[name]()
    gpu, ref, sg, sr = solve_both(sc, hip, oracle, max_iter=50)
    return sc, gpu, ref, sg, sr


@pytest.mark.parametrize("name", list(ss.SOLVE_SCENES))
def test_converged_solve_matches_oracle(name, hip, oracle):
    """The bar of test_unfused_route_converged_solve_matches_oracle; every body's pose among the estimates."""
    sc, gpu, ref, sg, sr = _converged_pair(name, hip, oracle)
    assert_plan(gpu, sc, lambda c, b: True, fused=True)
    assert sg.termination_type == sr.termination_type == _capi.CONVERGENCE
    assert sg.num_iterations == sr.num_iterations
    ig, ir = gpu.problem.iterations(), ref.problem.iterations()
    assert [i.step_is_successful for i in ig] == [i.step_is_successful for i in ir]
    worst = max(abs(a.cost - b.cost) / abs(b.cost) for a, b in zip(ig, ir))
    print("converged solve %s: %d iterations, worst cost per iteration %.2e, final cost %.2e" % (
        name, sg.num_iterations, worst, abs(sg.final_cost - sr.final_cost) / sr.final_cost))
    assert worst <= 1e-6
    assert abs(sg.final_cost - sr.final_cost) <= 1e-8 * sr.final_cost
    assert_estimates_close(gpu, ref, sc)
    for a, b in zip(syn.read_back_bodies(gpu, sc), syn.read_back_bodies(ref, sc)):
        for key in ("q", "t"):
            assert np.abs(a[key] - b[key]).max() <= 1e-6 * max(1e-3, np.abs(b[key]).max()), key
    for i, s in enumerate(sc.sensors):
        if s.kind == _capi.SENSOR_CAMERA:
            assert np.array_equal(gpu.problem.inlier_mask(gpu.sensor_ids[i], s.n, TAU), ref.problem.inlier_mask(ref.sensor_ids[i], s.n, TAU))


def test_lm_steps_with_a_body_pose_in_the_border(hip):
    sc = ss.SOLVE_SCENES["second chart free, model 1"]()
    keep = []
    step_tests.check_steps(hip, sc, {"tree_solver": 1}, iters=(1, 2, 3), mu=hip.default_options().initial_trust_region_radius,
                           label="second chart free", keep=keep)
    cols = [b for b, _ in lm_step.column_blocks(keep[0], sc)]
    assert keep[0].bodies[1]["t"] in cols and keep[0].bodies[1]["q"] in cols and keep[0].bodies[0]["q"] not in cols


# ---------------------------------------------------------------- analyses
def test_covariance_with_a_free_body(hip, oracle):
    sc = ss.SOLVE_SCENES["second chart free, model 1"]()
    gpu, ref = both(sc, hip, oracle)
    solve(gpu.problem, hip)
    Sg, Sr, _ = cov_tests.check_parity(gpu, ref, 1e-7, "second chart free")
    order, dim = border_layout(gpu, sc)
    assert dim == gpu.problem.covariance_info()[0]
    b1 = gpu.bodies[1]
    (oq, nq), (ot, nt) = order[b1["q"]], order[b1["t"]]
    assert (nq, nt) == (3, 3)
    P = gpu.problem
    assert np.array_equal(P.covariance_block(b1["t"], b1["t"]), Sg[ot:ot + 3, ot:ot + 3])
    assert np.array_equal(P.covariance_block(b1["q"], b1["q"], tangent=True), Sg[oq:oq + 3, oq:oq + 3])
    assert np.array_equal(P.covariance_block(b1["q"], b1["t"], tangent=True), Sg[oq:oq + 3, ot:ot + 3])
    assert np.all(np.diag(Sg[ot:ot + 3, ot:ot + 3]) > 0) and np.all(np.diag(Sg[oq:oq + 3, oq:oq + 3]) > 0)
    assert gpu.bodies[0]["q"] not in order


def test_covariance_refuses_two_free_bodies(hip, oracle):
    """Both charts free: the world frame is no longer fixed (a shift of both charts and the trajectory changes nothing)."""
    sc = ss.scene(1, [ss.chart1(free_pose=True)], free_chart_pose=True)
    gpu, ref = both(sc, hip, oracle)
    cov_tests.check_parity(gpu, ref, 1e-7, "both charts free", singular=True)
    check_parity(gpu, ref, sc, "both charts free")          # (the handle stays usable)


def test_prediction_covariance_in_registration_order(hip, oracle):
    """The rows of every sensor come back through sorted_pos."""
    sc = ss.SOLVE_SCENES["second chart free, model 1"]()
    rng = np.random.default_rng(5)
    v = syn.reorder(sc, [rng.permutation(s.n) for s in sc.sensors])
    gpu, R, Js = pred_tests.prepared(hip, oracle, v, 50)
    pred_tests.check_parity(gpu, v, R, Js, "permuted registration", tol=1e-7)
    pred_tests.check_trace_identity(gpu, v, R, Js, "permuted registration")


# ---------------------------------------------------------------- plan cache
def test_plan_cache_tells_bodies_apart(hip, oracle):
    hip.plan_cache_clear()
    sc = ss.second_chart_free(1)
    other = copy.deepcopy(sc)
    cam = other.sensors[0]
    # one frame's observations of body 1 now belong to body 0 (the same point numbers: both charts have twenty)
    body = syn.body_indices(cam)
    stamp = cam.stamps[body == 1][len(cam.stamps[body == 1]) // 2]
    swap = (cam.stamps == stamp) & (body == 1)
    assert swap.sum() >= 16 and cam.point_idx[swap].max() < len(other.points)
    cam.body_idx = np.where(swap, 0, body).astype(np.int32)
    h0, m0, _ = _capi.plan_cache_stats(hip)
    a = syn.build_problem(hip, sc)
    ea = eval_errors(a, syn.build_problem(oracle, sc))
    h1, m1, _ = _capi.plan_cache_stats(hip)
    b = syn.build_problem(hip, other)
    eb = eval_errors(b, syn.build_problem(oracle, other))
    h2, m2, _ = _capi.plan_cache_stats(hip)
    c = syn.build_problem(hip, sc)
    ec = eval_errors(c, syn.build_problem(oracle, sc))
    h3, m3, _ = _capi.plan_cache_stats(hip)
    assert (h1 - h0, m1 - m0) == (0, 1) and (h2 - h1, m2 - m1) == (0, 1) and (h3 - h2, m3 - m2) == (1, 0)
    assert max(ea + eb + ec) <= 1e-9, (ea, eb, ec)
    assert a.problem.evaluate()[0] != b.problem.evaluate()[0]
    # a sorted build, then the same observations permuted: hit or miss is the library's business, both must be right
    rng = np.random.default_rng(1)
    v = syn.reorder(sc, [rng.permutation(s.n) for s in sc.sensors])
    d = syn.build_problem(hip, v)
    worst = check_parity(d, syn.build_problem(oracle, v), v, "permuted build behind a sorted one")
    h4, m4, _ = _capi.plan_cache_stats(hip)
    print("plan cache, sorted then permuted: %s (worst error %.2e)" % ("hit" if h4 > h3 else "miss", worst))
    assert (h4 - h3) + (m4 - m3) == 1
    check_parity(c, syn.build_problem(oracle, sc), sc, "sorted build, after the permuted one")


# ---------------------------------------------------------------- two ranks
def test_two_ranks_on_a_permuted_two_body_scene(hip):
    """Two sharded handles with a host exchange against the single handle, to test_gpu_multirank.py's 1e-9: the evaluation,
    and the estimates of ten iterations."""
    sc = ss.second_chart_free(1)
    rng = np.random.default_rng(2)
    v = syn.reorder(sc, [rng.permutation(s.n) for s in sc.sensors])
    single = syn.build_problem(hip, v)
    vals = {b: single.problem.get_param_block(b, n) for b, n in dict(single.problem._sizes).items()}
    c1, g1, H1 = single.problem.evaluate()

    def options():
        o = hip.default_options()
        o.minimizer_progress_to_stdout, o.max_num_iterations, o.sync_every = 0, 10, 4
        return o
    s1 = single.problem.solve(options())
    e1, ctrl1 = syn.read_back(single, v)
    b1 = syn.read_back_bodies(single, v)

    def per_rank(b):
        ev = b.problem.evaluate()
        s = b.problem.solve(options())
        return ev, s, syn.read_back(b, v), syn.read_back_bodies(b, v), b.problem.comm_info()
    results = run_two_ranks(hip, v, vals, per_rank)
    assert sum(r[4][2] for r in results) == v.num_blocks
    sd = np.sqrt(np.diag(H1))
    sd = np.where(sd > 0, sd, 1.0)
    for (c, g, H), s, (est, ctrl), bodies, info in results:
        assert abs(c - c1) <= 1e-9 * c1 and np.abs(g - g1).max() <= 1e-9 * np.abs(g1).max()
        assert (np.abs(H - H1) / np.outer(sd, sd)).max() <= 1e-9
        assert s.termination_type == s1.termination_type and s.num_iterations == s1.num_iterations
        assert abs(s.final_cost - s1.final_cost) <= 1e-9 * s1.final_cost
        assert np.abs(ctrl - ctrl1).max() <= 1e-9 * np.abs(ctrl1).max()
        for a, b in zip(est, e1):
            assert np.abs(a["intrinsics"] - b["intrinsics"]).max() <= 1e-9 * np.abs(b["intrinsics"]).max()
        for key in ("q", "t"):
            assert np.abs(bodies[1][key] - b1[1][key]).max() <= 1e-9 * np.abs(b1[1][key]).max()
    assert np.array_equal(results[0][2][1], results[1][2][1])      # replicated solve of one deterministic sum
