"""The generator's new axes (several rigid bodies, a camera model per camera, a registration order) on the CPU oracle alone.

1. Defaults are unchanged: a scene built through the new code path with its defaults spelled out -- an empty list of
   further bodies, a model per camera, an all-zero body index, the identity permutation and one call per sensor -- is
   the scene of the plain call, bit for bit: observation arrays, block ids and sizes, cost, gradient and JᵀJ.
2. The scenes of the converged-solve comparisons of test_gpu_problem_structure.py determine their estimates: the oracle
   with default tolerances ends within 1e-7 (relative, floor 1e-3; control points relative to their largest) of the oracle
   with tolerances 1e-12 / 1e-14 / 1e-16. That is what gives the device's 1e-6 bound its meaning.
   At small_scene's noise (0.1 px, 1e-3 rad/s, 1e-2 m/s²) these rigs do NOT: over forty seeds the accelerometer's lever arm
   and the later cameras' extrinsics ended 4e-7 .. 1e-5 apart (the default function tolerance stops within a fraction of
   an estimate's standard deviation of the minimum, and that deviation is 1e-5 of a 5 cm lever arm); at a hundredth of the
   noise the median over forty seeds was still 3e-7. The solve scenes therefore carry a thousandth of it (what is left in
   their residuals is the model's own error, the segment a latency straddles), with seeds from a scan of forty; measured:
   2.0e-8 (second chart free, seed 11), 4.0e-8 (mixed rig, seed 33).
3. A permutation of the observations is the same problem for the oracle (cost to 1e-14, JᵀJ to 1e-12 of its largest entry)."""
import numpy as np
import pytest

import structure_scenes as ss
from calico_amd import _capi, synthetic as syn
from helpers import small_scene

_SMALL = dict(cam_rate=10.0, imu_rate=50.0, duration=3.0, segment_duration=3.0 / 23.9, pixel_noise=0.1, gyro_noise=1e-3,
              accel_noise=1e-2)
DEFAULTS = {
    "two cameras + imu, robust": dict(n_cameras=2, camera_model=1, imu=True, robust=True, seed=7, **_SMALL),
    "free chart pose and model points": dict(n_cameras=2, camera_model=3, imu=True, free_points=True, free_chart_pose=True,
                                             seed=5, **_SMALL),
    "outliers, april grid, capped": dict(n_cameras=1, camera_model=1, imu=False, cam_rate=4.0, duration=1.0, chart="april",
                                         seed=0xCA11C0, max_cam_obs=500, pixel_noise=0.1, segment_duration=1.0 / 23.9,
                                         outlier_fraction=0.05, robust=True),
}


@pytest.mark.parametrize("name", list(DEFAULTS))
def test_spelled_out_defaults_build_the_same_problem(name, oracle):
    kw = DEFAULTS[name]
    plain = syn.make_scene(**kw)
    spelled = syn.make_scene(**dict(kw, camera_model=[kw["camera_model"]] * kw["n_cameras"], extra_bodies=[]))
    assert spelled.extra_bodies == [] and spelled.calls is None
    for a, b in zip(plain.sensors, spelled.sensors):
        assert a.model == b.model and a.body_idx is None and b.body_idx is None
        for key in ("meas", "stamps", "point_idx", "is_outlier", "intrinsics", "q", "t"):
            x, y = getattr(a, key), getattr(b, key)
            assert (x is None and y is None) or np.array_equal(x, y), key
    assert np.array_equal(plain.points, spelled.points) and np.array_equal(plain.ctrl, spelled.ctrl)
    for s in spelled.sensors:
        if s.kind == _capi.SENSOR_CAMERA:
            s.body_idx = np.zeros(s.n, np.int32)
    spelled = syn.reorder(spelled, [np.arange(s.n) for s in spelled.sensors], calls=[(i, 0, s.n) for i, s in enumerate(spelled.sensors)])
    a, b = syn.build_problem(oracle, plain), syn.build_problem(oracle, spelled)
    assert a.problem._sizes == b.problem._sizes and list(a.problem._sizes) == list(b.problem._sizes)
    assert a.problem._manifolds == b.problem._manifolds
    assert np.array_equal(a.point_blocks, b.point_blocks) and np.array_equal(a.ctrl_blocks, b.ctrl_blocks)
    assert (a.body_q_block, a.body_t_block, a.gravity_block) == (b.body_q_block, b.body_t_block, b.gravity_block)
    assert a.sensor_ids == b.sensor_ids and a.sensor_blocks == b.sensor_blocks
    assert len(a.bodies) == 1 and a.bodies[0]["q"] == a.body_q_block and a.bodies[0]["t"] == a.body_t_block
    ca, ga, Ha = a.problem.evaluate()
    cb, gb, Hb = b.problem.evaluate()
    assert ca == cb and np.array_equal(ga, gb) and np.array_equal(Ha, Hb)
    for i, s in enumerate(plain.sensors):
        ra, va = a.problem.residuals(a.sensor_ids[i], s.n, s.dim)
        rb, vb = b.problem.residuals(b.sensor_ids[i], s.n, s.dim)
        assert np.array_equal(ra, rb) and np.array_equal(va, vb)


def test_small_scene_is_the_scene_it_was():
    """helpers.small_scene (every GPU test's scene) through the list form and the body-less form."""
    a = small_scene(camera_model=1, n_cameras=2, imu=True, robust=True)
    b = small_scene(camera_model=[1, 1], n_cameras=2, imu=True, robust=True, extra_bodies=None)
    for x, y in zip(a.sensors, b.sensors):
        assert np.array_equal(x.meas, y.meas) and np.array_equal(x.stamps, y.stamps) and np.array_equal(x.intrinsics, y.intrinsics)
    # further bodies leave body 0's observations, and every other sensor, as they are
    c = ss.scene(1, [ss.chart1(free_pose=True)], seed=7)
    for x, z in zip(a.sensors, c.sensors):
        assert np.array_equal(x.meas, z.meas[:x.n]) and np.array_equal(x.stamps, z.stamps[:x.n])
        if x.kind == _capi.SENSOR_CAMERA:
            assert z.n > x.n and np.all(z.body_idx[:x.n] == 0) and np.all(z.body_idx[x.n:] == 1)
        else:
            assert z.n == x.n


def test_blocks_follow_the_reference_order(oracle):
    """WorldModel::AddParametersToProblem: per body its points, then its pose (t, q); gravity after the last body."""
    sc = ss.scene(1, [ss.chart1(free_pose=True), ss.sparse_chart()])
    b = syn.build_problem(oracle, sc)
    want = 0
    for spec, body in zip(sc.bodies, b.bodies):
        assert list(body["point_blocks"]) == list(range(want, want + len(spec.points)))
        want += len(spec.points)
        assert (body["t"], body["q"]) == (want, want + 1)
        want += 2
    assert b.gravity_block == want and b.ctrl_blocks[0] == want + 1
    assert [body["id"] for body in b.bodies] == [0, 1, 2]


def _estimates(built, sc):
    est, ctrl = syn.read_back(built, sc)
    return est, ctrl, syn.read_back_bodies(built, sc)


def worst_difference(a, b):
    """Largest difference of two sets of estimates: relative to each block's largest entry (floor 1e-3), the control points
    relative to theirs (floor 1), every body's pose included."""
    w = 0.0
    for x, y in zip(a[0], b[0]):
        for key in ("intrinsics", "t", "q"):
            w = max(w, np.abs(x[key] - y[key]).max() / max(1e-3, np.abs(y[key]).max()))
        w = max(w, abs(x["latency"] - y["latency"]) / max(1e-3, abs(y["latency"])))
    w = max(w, np.abs(a[1] - b[1]).max() / max(1.0, np.abs(b[1]).max()))
    for x, y in zip(a[2], b[2]):
        for key in ("q", "t"):
            w = max(w, np.abs(x[key] - y[key]).max() / max(1e-3, np.abs(y[key]).max()))
    return w


@pytest.mark.parametrize("name", list(ss.SOLVE_SCENES))
def test_solve_scenes_determine_their_estimates(name, oracle):
    sc = ss.SOLVE_SCENES[name]()
    ends = []
    for tight in (False, True):
        built = syn.build_problem(oracle, sc)
        o = oracle.default_options()
        o.minimizer_progress_to_stdout = 0
        o.max_num_iterations = 200
        o.num_threads = 8
        if tight:
            o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance = 1e-12, 1e-14, 1e-16
        s = built.problem.solve(o)
        assert s.termination_type == _capi.CONVERGENCE
        ends.append(_estimates(built, sc))
    w = worst_difference(*ends)
    print("%s: default tolerances end %.2e from 1e-12 / 1e-14 / 1e-16" % (name, w))
    assert w <= 1e-7, w
    # ... and the free body moved from its start to where it is
    if sc.extra_bodies[0].pose_constant is False:
        assert np.abs(ends[1][2][1]["t"] - sc.extra_bodies[0].t_true).max() < 1e-3


def test_oracle_does_not_care_about_registration_order(oracle):
    sc = ss.scene(1, [ss.chart1(free_pose=True)], seed=7)
    base = syn.build_problem(oracle, sc)
    c0, g0, H0 = base.problem.evaluate()
    variants, perms = ss.registration_variants(sc)
    for name, v in variants.items():
        b = syn.build_problem(oracle, v)
        c, g, H = b.problem.evaluate()
        assert abs(c - c0) <= 1e-14 * c0 and np.abs(H - H0).max() <= 1e-12 * np.abs(H0).max(), name
        for i, s in enumerate(sc.sensors):      # residuals come back in registration order
            r0, v0 = base.problem.residuals(base.sensor_ids[i], s.n, s.dim)
            r, vv = b.problem.residuals(b.sensor_ids[i], s.n, s.dim)
            assert np.array_equal(r, r0[perms[name][i]]) and np.array_equal(vv, v0[perms[name][i]]), (name, i)
