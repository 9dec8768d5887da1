"""Covariance of the calibration estimates (calico_covariance_compute) against a dense reference built from the oracle.

Reference: the same seeded scene in the oracle with the GPU's parameter values copied in, the oracle's dense JᵀJ from
evaluate(), exactly-zero diagonal columns dropped, inverted with numpy, the border rows cut out (tangent order
[control points | free used blocks in block-id order]). Entries are compared relative to sqrt(Σ_ii Σ_jj)."""
import ctypes as C

import numpy as np
import pytest

from calico_amd import _capi, synthetic as syn
from helpers import _state, border_layout, full_size_scene, run_two_ranks, small_scene, solve

pytestmark = pytest.mark.gpu


def _sizes(P):
    return dict(P._sizes)


def reference_sigma(gpu, ref, mc):
    """Dense Σ of the border from the oracle at the GPU's current values."""
    for b, n in _sizes(gpu.problem).items():
        ref.problem.set_param_block(b, gpu.problem.get_param_block(b, n))
    _, _, H = ref.problem.evaluate()
    n = H.shape[0]
    keep = np.diag(H) != 0.0
    S = np.zeros_like(H)
    idx = np.nonzero(keep)[0]
    S[np.ix_(idx, idx)] = np.linalg.inv(H[np.ix_(idx, idx)])
    return S[n - mc:, n - mc:], keep[n - mc:]


def rel_err(a, b):
    d = np.sqrt(np.abs(np.diag(b)))
    d = np.where(d > 0, d, 1.0)
    return (np.abs(a - b) / np.outer(d, d)).max()


def oracle_min_eig(gpu, ref):
    """Smallest eigenvalue of the oracle's equilibrated JᵀJ (zero columns left out) at the GPU's values."""
    for b, n in _sizes(gpu.problem).items():
        ref.problem.set_param_block(b, gpu.problem.get_param_block(b, n))
    _, _, H = ref.problem.evaluate()
    d = np.sqrt(np.diag(H))
    k = d > 0
    return np.linalg.eigvalsh(H[np.ix_(k, k)] / np.outer(d[k], d[k]))[0]


def check_parity(gpu, ref, tol, what="", singular=False):
    """singular=True: the scene is known to be rank deficient (the oracle must agree) and compute must refuse it;
    otherwise the oracle must find it well-posed and Σ is compared entry by entry."""
    ev = oracle_min_eig(gpu, ref)
    assert (ev < 1e-12) == singular, (what, ev)
    if singular:
        with pytest.raises(_capi.CalicoError) as e:
            gpu.problem.covariance_compute()
        assert e.value.code == _capi.FAILED_PRECONDITION and "rank deficient" in e.value.message
        print("covariance %s: singular (oracle's equilibrated min eigenvalue %.2e): refused" % (what, ev))
        return None, None, None
    dim, n_unobs, piv = gpu.problem.covariance_compute()
    Sg = gpu.problem.covariance_dense()
    Sr, keep = reference_sigma(gpu, ref, dim)
    assert n_unobs == int((~keep).sum())
    assert np.all(Sg[~keep] == 0.0) and np.all(Sg[:, ~keep] == 0.0)
    err = rel_err(Sg, Sr)
    print("covariance parity %s: dim %d, unobserved %d, min relative pivot %.3e, max rel err %.2e" % (what, dim, n_unobs, piv, err))
    assert err <= tol, err
    return Sg, Sr, piv


# OpenCV8 (model 2) at the synthetic start values is exactly singular: its distortion starts at 0 (synthetic.py,
# _initial_intrinsics), where the numerator and denominator terms of the same radial power have opposite Jacobian columns
# (d/dk4 = -d/dk1, d/dk5 = -d/dk2, d/dk6 = -d/dk3 at k = 0; the oracle's equilibrated JᵀJ has eigenvalues ~1e-16).
# Compute refuses it; every other model compares numerically.
@pytest.mark.parametrize("model,singular", [(1, False), (2, True), (3, False), (4, False), (5, False), (6, False), (7, False)])
def test_camera_models_parity(model, singular, hip, oracle):
    scene = small_scene(camera_model=model, imu=False)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    # measured max 3.6e-10 over the six compared models (minimum relative pivots 3.2e-4 .. 8.7e-3). At the start values: the
    # camera-only scenes run to convergence end singular (test_camera_only_scene_singular_when_solved); the converged
    # comparisons use scenes with an IMU.
    check_parity(gpu, ref, 1e-7, "camera %d, start" % model, singular=singular)


def test_camera_only_scene_singular_when_solved(hip, oracle):
    """The camera-only small scene, solved to the iteration limit, ends where the oracle's equilibrated JᵀJ is singular
    (eigenvalues ~1e-16; it is well-posed at its start values): compute refuses it there, as it must."""
    scene = small_scene(camera_model=1, imu=False)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip)
    check_parity(gpu, ref, 1e-7, "camera 1, solved", singular=True)


@pytest.mark.parametrize("model", [2, 3, 7])
def test_camera_models_with_imu_converged_parity(model, hip, oracle):
    scene = small_scene(camera_model=model, imu=True)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip)
    check_parity(gpu, ref, 1e-7, "camera %d + imu, converged" % model)


# VectorNav (model 3): its full 3x3 gyroscope matrix and the free gyroscope rotation describe the same rotation of the
# measurement (a rotation of the matrix's rows is absorbed by q_rg): exactly singular, refused, in both loss settings.
@pytest.mark.parametrize("imu_model,singular", [(1, False), (2, False), (3, True)])
@pytest.mark.parametrize("robust", [False, True])
def test_imu_models_parity_and_unobserved_columns(imu_model, singular, robust, hip, oracle):
    scene = small_scene(camera_model=1, imu=True, imu_model=imu_model, robust=robust)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip)
    Sg, _, _ = check_parity(gpu, ref, 1e-7, "imu %d robust %d" % (imu_model, robust), singular=singular)      # measured max 7.3e-11
    if singular:
        return
    dim, n_unobs, _ = gpu.problem.covariance_info()
    assert n_unobs >= 3          # the gyroscope's translation block: registered, used by no residual
    gyro = [b for s, b in zip(scene.sensors, gpu.sensor_blocks) if s.kind == _capi.SENSOR_GYROSCOPE][0]
    assert np.all(gpu.problem.covariance_block(gyro["t"], gyro["t"]) == 0.0)
    assert np.all(gpu.problem.covariance_block(gyro["intrinsics"], gyro["intrinsics"]).diagonal() > 0.0)


def test_quaternion_block_tangent_and_ambient(hip, oracle):
    scene = small_scene(camera_model=1, n_cameras=2, imu=True)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip)
    Sg, Sr, _ = check_parity(gpu, ref, 1e-7, "quaternion")
    P = gpu.problem
    order, dim = border_layout(gpu, scene)
    assert dim == P.covariance_info()[0]
    cam1 = gpu.sensor_blocks[1]
    for b, (o, t) in order.items():      # every block of the border reads back its rows of the dense Σ
        assert np.array_equal(P.covariance_block(b, b, tangent=True), Sg[o:o + t, o:o + t])
    oq, _ = order[cam1["q"]]
    ot, _ = order[cam1["t"]]
    tan = P.covariance_block(cam1["q"], cam1["t"], tangent=True)
    assert np.array_equal(tan, Sg[oq:oq + 3, ot:ot + 3])
    x, y, z, w = P.get_param_block(cam1["q"], 4)
    Pj = np.array([[w, z, -y], [-z, w, x], [y, -x, w], [-x, -y, -z]])
    amb = P.covariance_block(cam1["q"], cam1["q"])
    ref_amb = Pj @ Sr[oq:oq + 3, oq:oq + 3] @ Pj.T
    s = np.sqrt(np.abs(np.diag(Sr[oq:oq + 3, oq:oq + 3]))).max()
    assert np.abs(amb - ref_amb).max() <= 1e-7 * s * s
    assert amb.shape == (4, 4) and tan.shape == (3, 3)


def test_free_model_points_parity(hip, oracle):
    scene = small_scene(camera_model=1, n_cameras=2, imu=True, free_points=True, seed=5)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip, 25)
    check_parity(gpu, ref, 1e-7, "free model points")        # measured 8.1e-11
    assert gpu.problem.covariance_info()[0] > 128      # the reduced system leaves LDS: the global-memory variant


@pytest.mark.parametrize("order", [7, 8])
def test_banded_path_parity_high_order(order, hip, oracle):
    scene = small_scene(camera_model=1, imu=True, order=order)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip)
    check_parity(gpu, ref, 1e-7, "order %d" % order)        # measured 4.5e-11 / 6.7e-11


def test_banded_path_parity_forced(hip, oracle, monkeypatch):
    monkeypatch.setenv("CALICO_SOLVER", "band")
    scene = small_scene(camera_model=3, imu=True)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    assert gpu.problem.plan_info()["tree_solver"] == 0
    solve(gpu.problem, hip)
    check_parity(gpu, ref, 1e-7, "CALICO_SOLVER=band")       # measured 4.4e-11


def test_gauge_deficiency_is_refused(hip, oracle):
    scene = small_scene(camera_model=1, imu=False, free_chart_pose=True)
    gpu = syn.build_problem(hip, scene)
    with pytest.raises(_capi.CalicoError) as e:
        gpu.problem.covariance_compute()
    assert e.value.code == _capi.FAILED_PRECONDITION and "rank deficient" in e.value.message
    print("gauge-deficient scene:", e.value.message)
    # the threshold sits between the well-posed scenes' minimum relative pivots (printed by the parity tests) and this one
    with pytest.raises(_capi.CalicoError) as e:
        gpu.problem.covariance_dense()
    assert e.value.code == _capi.FAILED_PRECONDITION
    s = solve(gpu.problem, hip, 20)
    assert s.final_cost < s.initial_cost


def test_no_side_effects(hip):
    scene = small_scene(camera_model=1, imu=True)
    a, b = syn.build_problem(hip, scene), syn.build_problem(hip, scene)
    for x in (a, b):
        x.problem.set_phase_timing(0x7f)
    sa1 = solve(a.problem, hip, 5)
    sb1 = solve(b.problem, hip, 5)
    na = [a.problem.phase_time(k)[1] for k in range(7)]
    before = _state(b, scene)
    b.problem.covariance_compute()
    after = _state(b, scene)
    for k in before[0]:
        assert np.array_equal(before[0][k], after[0][k])
    for (rx, vx), (ry, vy) in zip(before[1], after[1]):
        assert np.array_equal(rx, ry) and np.array_equal(vx, vy)
    its_b_first = [(r.iteration, r.cost) for r in b.problem.iterations()]
    assert its_b_first == [(r.iteration, r.cost) for r in a.problem.iterations()]
    assert b.problem.plan_info() == a.problem.plan_info()
    assert [b.problem.phase_time(k)[1] for k in range(7)] == na      # the pass records no launches into the phase timer
    sa2 = solve(a.problem, hip, 30)
    sb2 = solve(b.problem, hip, 30)
    keys = [k for k, _ in _capi.Summary._fields_ if "time" not in k]
    d1a, d1b, d2a, d2b = (x.as_dict() for x in (sa1, sb1, sa2, sb2))
    assert [d1a[k] for k in keys] == [d1b[k] for k in keys]
    assert [d2a[k] for k in keys] == [d2b[k] for k in keys]
    ia = [(r.iteration, r.step_is_successful, r.cost, r.cost_change, r.trust_region_radius) for r in a.problem.iterations()]
    ib = [(r.iteration, r.step_is_successful, r.cost, r.cost_change, r.trust_region_radius) for r in b.problem.iterations()]
    assert ia == ib
    va, _ = _state(a, scene)
    vb, _ = _state(b, scene)
    for k in va:
        assert np.array_equal(va[k], vb[k])


def test_determinism(hip):
    scene = small_scene(camera_model=1, imu=True)
    g = syn.build_problem(hip, scene)
    solve(g.problem, hip)
    g.problem.covariance_compute()
    s1 = g.problem.covariance_dense()
    g.problem.covariance_compute()
    s2 = g.problem.covariance_dense()
    assert np.array_equal(s1, s2)


def test_errors(hip):
    scene = small_scene(camera_model=1, imu=True)
    g = syn.build_problem(hip, scene)
    P = g.problem
    with pytest.raises(_capi.CalicoError) as e:
        P.covariance_dense()
    assert e.value.code == _capi.FAILED_PRECONDITION
    with pytest.raises(_capi.CalicoError) as e:
        P.covariance_block(g.sensor_blocks[0]["intrinsics"], g.sensor_blocks[0]["intrinsics"])
    assert e.value.code == _capi.FAILED_PRECONDITION
    P.covariance_compute()
    with pytest.raises(_capi.CalicoError) as e:
        P.covariance_block(int(g.ctrl_blocks[3]), g.sensor_blocks[0]["intrinsics"], sizes=(6, 8))
    assert e.value.code == _capi.UNIMPLEMENTED
    out = np.zeros(9)
    assert hip.covariance_get_block(P.h, 10 ** 6, 0, 1, out.ctypes.data_as(C.POINTER(C.c_double))) == _capi.INVALID_ARGUMENT
    assert hip.covariance_get_block(P.h, -1, 0, 1, out.ctypes.data_as(C.POINTER(C.c_double))) == _capi.INVALID_ARGUMENT
    # constant blocks (the chart pose, gravity, camera 0's extrinsics): zeros, in either form
    assert np.all(P.covariance_block(g.gravity_block, g.gravity_block) == 0.0)
    assert np.all(P.covariance_block(g.body_q_block, g.sensor_blocks[0]["intrinsics"]) == 0.0)
    assert P.covariance_block(g.body_q_block, g.body_q_block, tangent=True).shape == (3, 3)


def test_stale_result_is_refused_after_the_problem_changes(hip):
    scene = small_scene(camera_model=1, imu=True)
    g = syn.build_problem(hip, scene)
    P = g.problem
    intr = g.sensor_blocks[0]["intrinsics"]
    P.covariance_compute()
    before = P.covariance_block(intr, intr)
    solve(P, hip, 3)                       # values change, the structure does not: the result stays readable
    assert np.array_equal(P.covariance_block(intr, intr), before)
    new = P.add_param_block(np.ones(3))    # a structural change: Σ no longer describes this problem
    for call in (lambda: P.covariance_block(intr, intr), P.covariance_dense, P.covariance_info):
        with pytest.raises(_capi.CalicoError) as e:
            call()
        assert e.value.code == _capi.FAILED_PRECONDITION
    solve(P, hip, 3)                       # re-finalised: still refused until computed again
    with pytest.raises(_capi.CalicoError) as e:
        P.covariance_block(new, new)
    assert e.value.code == _capi.FAILED_PRECONDITION
    P.covariance_compute()
    assert np.all(P.covariance_block(new, new) == 0.0)      # (unused by any residual)
    assert P.covariance_block(intr, intr).shape == before.shape


@pytest.mark.parametrize("index", [3, 4])
def test_full_size_parity_and_wall_time(index, hip, oracle):
    import time
    scene = full_size_scene(index)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip, 10)
    Sg, _, _ = check_parity(gpu, ref, 1e-7, "configs[%d] shape" % index)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        gpu.problem.covariance_compute()
        ts.append(time.perf_counter() - t0)
    assert np.array_equal(gpu.problem.covariance_dense(), Sg)
    print("configs[%d] shape: covariance_compute wall time %.3f ms (median of 5 after a warm-up), plan %s" % (
        index, 1e3 * np.median(ts), gpu.problem.plan_info()))


def test_multirank_two_handles_agree(hip):
    """Two ranks on one device, each a handle sharded to its time window (calico_problem_set_shard) with a host exchange
    (sum in rank order): both
    hold the same Σ bit for bit, equal to the single-rank Σ to rounding."""
    scene = small_scene(camera_model=1, imu=True, robust=True, seed=3)
    single = syn.build_problem(hip, scene)
    solve(single.problem, hip)
    vals = {b: single.problem.get_param_block(b, n) for b, n in _sizes(single.problem).items()}
    single.problem.covariance_compute()
    S1 = single.problem.covariance_dense()

    def per_rank(b):
        b.problem.covariance_compute()
        return b.problem.covariance_dense()
    results = run_two_ranks(hip, scene, vals, per_rank)
    assert np.array_equal(results[0], results[1])
    assert rel_err(results[0], S1) <= 1e-9, rel_err(results[0], S1)


def test_python_facade_covariance(hip):
    """BatchOptimizer.ComputeCovariance() of the pybind module (the C++ facade underneath) on a stereo rig: the per-sensor
    blocks have Ceres' shapes, are symmetric positive definite where estimated, and agree with the facade's own dense
    layout; a sensor whose blocks are constant reads back zeros."""
    from calico_amd import calico
    import test_python_api as tpa
    stamps, poses = tpa._poses()
    times = [float(t) for t in stamps]
    trajectory = calico.Trajectory()
    trajectory.FitSpline(poses)
    chart = calico.RigidBody()
    chart.model_definition = {i: p for i, p in enumerate(syn.planar_points())}
    chart.world_pose_is_constant = True
    chart.model_definition_is_constant = True
    world = calico.WorldModel()
    world.AddRigidBody(chart)
    true_cam = np.array([785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2])
    optimizer = calico.BatchOptimizer()
    sensors = []
    for k in range(2):
        truth = calico.Camera()
        assert truth.SetModel(calico.CameraIntrinsicsModel.kOpenCv5).ok()
        truth.SetIntrinsics(true_cam)
        ex = calico.Pose3d()
        if k:
            ex.translation = np.array([0.05, -0.02, 0.01])
        truth.SetExtrinsics(ex)
        meas = truth.Project(times, trajectory, world)
        cam = calico.Camera()
        assert cam.SetModel(calico.CameraIntrinsicsModel.kOpenCv5).ok()
        cam.SetIntrinsics(true_cam)
        cam.SetExtrinsics(ex)
        cam.EnableIntrinsicsEstimation(True)
        cam.EnableExtrinsicsEstimation(k == 1)
        cam.EnableLatencyEstimation(k == 1)
        assert cam.AddMeasurements(meas).ok()
        optimizer.AddSensor(cam)
        sensors.append(cam)
    optimizer.AddTrajectory(trajectory)
    optimizer.AddWorldModel(world)
    cov = optimizer.ComputeCovariance()      # at the true values (perfect measurements): Σ of a well-posed rig
    assert cov.Dimension() == 8 + 8 + 6 + 1
    for cam in sensors:
        I = cov.Intrinsics(cam)
        assert I.shape == (8, 8) and np.allclose(I, I.T, rtol=0, atol=1e-12 * np.abs(I).max())
        assert np.linalg.eigvalsh(I).min() > 0
    E0, E1 = cov.Extrinsics(sensors[0]), cov.Extrinsics(sensors[1])
    assert E0.shape == (6, 6) and np.all(E0 == 0.0) and cov.Latency(sensors[0]) == 0.0
    assert np.linalg.eigvalsh(E1).min() > 0 and cov.Latency(sensors[1]) > 0
    print("facade: camera 1 latency sd %.3e s, lever arm sd %s m" % (np.sqrt(cov.Latency(sensors[1])), np.sqrt(np.diag(E1)[3:])))
