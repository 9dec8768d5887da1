"""Prediction covariance and leverage of every observation (calico_prediction_covariance) against the dense reference of
prediction_ref.py: P_i = J_i S J_iᵀ from the oracle's Jacobian at the GPU's values.

Parity bound, per entry (a, b) of P_i: |P − P_ref| <= 1e-7 β_a β_b with β_a = Σ_j |J_aj| sqrt(S_jj) -- the guarantee of
test_gpu_trajectory_covariance.py for every entry of Σ (1e-7 relative to sqrt(Σ_ii Σ_jj)) pushed through the bilinear form.
The tighter figure max |ΔP_ab| / sqrt(P_aa P_bb) is printed per scene (cancellation in J Σ Jᵀ is real: it is not asserted).

Measured (MI355X): see DESIGN.md section 4, prediction_covariance_kernel."""
import copy
import time

import numpy as np
import pytest

import prediction_ref as pr
from calico_amd import _capi, synthetic as syn
from helpers import full_size_scene, run_two_ranks, small_scene, solve

pytestmark = pytest.mark.gpu

TOL = 1e-7


def prepared(hip, oracle, scene, iters):
    """The scene on the GPU (solved for `iters` iterations, Σ with control points computed) and its reference at the same
    values: (gpu, Reference, {apply_loss: dense J})."""
    gpu = syn.build_problem(hip, scene)
    if iters:
        solve(gpu.problem, hip, iters)
    gpu.problem.covariance_compute(control_points=True)
    ref, ref0 = pr.build_pair(oracle, scene)
    pr.copy_values(gpu, ref)
    pr.copy_values(gpu, ref0)
    R = pr.Reference(ref)
    return gpu, R, {1: R.J_fit, 0: pr.dense_jacobian(ref0)}


def compare(cov, lev, Pref, beta, tol):
    """Worst |ΔP| / (β_a β_b) and the tight figure max |ΔP_ab| / sqrt(P_aa P_bb); asserts the bound entry by entry."""
    bound = tol * beta[:, :, None] * beta[:, None, :]
    err = np.abs(cov - Pref)
    dg = np.sqrt(np.abs(np.einsum("nii->ni", Pref)))
    tight = (err / np.maximum(dg[:, :, None] * dg[:, None, :], 1e-300)).max() if len(cov) else 0.0
    ratio = (err / np.maximum(bound, 1e-300)).max() * tol if len(cov) else 0.0
    assert np.all(err <= bound), (ratio, tight)
    assert np.array_equal(lev, np.einsum("nii->n", cov))
    return ratio, tight


def check_parity(gpu, scene, R, Js, what, tol=TOL):
    P = gpu.problem
    worst = {}
    for apply_loss in (1, 0):
        ratio = tight = 0.0
        for sid, s, (first, n, d) in zip(gpu.sensor_ids, scene.sensors, pr.sensor_rows(scene)):
            cov, lev, valid = P.prediction_covariance(sid, apply_loss=bool(apply_loss))
            assert cov.shape == (n, d, d) and lev.shape == (n,) and valid.shape == (n,) and valid.all()
            assert np.array_equal(cov, cov.transpose(0, 2, 1))
            Pref, beta = R.blocks(Js[apply_loss], first, n, d)
            a, b = compare(cov, lev, Pref, beta, tol)
            ratio, tight = max(ratio, a), max(tight, b)
        worst[apply_loss] = (ratio, tight)
    print("prediction covariance %s: %d blocks, %d columns; apply_loss=1: max |dP| / (beta_a beta_b) %.2e, max |dP_ab| / "
          "sqrt(P_aa P_bb) %.2e; apply_loss=0: %.2e, %.2e" % (what, scene.num_blocks, R.S.shape[0], worst[1][0], worst[1][1],
                                                             worst[0][0], worst[0][1]))
    return worst


def expected_trace(P):
    dim, n_unobs, _ = P.covariance_info()
    n_cp = P.covariance_trajectory_info()[0]
    return 6 * n_cp + dim - n_unobs


def check_trace_identity(gpu, scene, R, Js, what):
    """apply_loss = 1: Σ leverage = 6 n_cp + dim − n_unobserved within 1e-7 (Σ_j sqrt(S_jj H_jj))²; every P_i symmetric bit for
    bit with eigenvalues in [0, 1] widened by 1e-7 Σ_a β_a² (where the dense Jacobian gives β: Js is not None)."""
    P = gpu.problem
    total, lo, hi = 0.0, 0.0, 0.0
    for sid, s, (first, n, d) in zip(gpu.sensor_ids, scene.sensors, pr.sensor_rows(scene)):
        cov, lev, valid = P.prediction_covariance(sid)
        assert valid.all() and np.array_equal(cov, cov.transpose(0, 2, 1))
        total += float(np.sum(lev))
        if n == 0:
            continue
        ev = np.linalg.eigvalsh(cov)
        if Js is not None:
            _, beta = R.blocks(Js[1], first, n, d)
            widen = TOL * np.sum(beta ** 2, axis=1)
            assert np.all(ev[:, 0] >= -widen) and np.all(ev[:, -1] <= 1.0 + widen), (ev[:, 0].min(), ev[:, -1].max())
        lo, hi = min(lo, ev[:, 0].min()), max(hi, ev[:, -1].max())
    want = expected_trace(P)
    assert want == R.n_kept      # (every control point of these scenes is observed)
    bound = R.trace_bound(TOL)
    print("trace identity %s: sum of leverages %.10f, expected %d, deviation %.3e (relative %.1e), bound %.3e; eigenvalues of "
          "P_i in [%.3e, %.6f]" % (what, total, want, total - want, abs(total - want) / want, bound, lo, hi))
    assert abs(total - want) <= bound
    return total - want


SMALL = {
    "camera 1, imu 1": (dict(camera_model=1, imu_model=1), 50),
    "camera 1, imu 2": (dict(camera_model=1, imu_model=2), 50),
    "camera 3, imu 1": (dict(camera_model=3, imu_model=1), 50),
    "camera 3, imu 2": (dict(camera_model=3, imu_model=2), 50),
    "camera 4, imu 1": (dict(camera_model=4, imu_model=1), 50),
    "camera 4, imu 2": (dict(camera_model=4, imu_model=2), 50),
    "camera 7, imu 1": (dict(camera_model=7, imu_model=1), 50),
    "camera 7, imu 2": (dict(camera_model=7, imu_model=2), 50),
    "robust": (dict(camera_model=1, imu_model=2, robust=True), 50),
    "order 4": (dict(camera_model=1, order=4), 50),
    "order 7": (dict(camera_model=1, order=7), 50),
    "order 8": (dict(camera_model=1, order=8), 50),
    "free model points": (dict(camera_model=1, n_cameras=2, free_points=True, seed=5), 25),
}


@pytest.mark.parametrize("name", list(SMALL))
def test_parity_and_trace_small_scenes(name, hip, oracle):
    """Parity of both apply_loss values for every sensor (cameras 1 and later estimate their latency, as do the IMUs), and
    the trace identity on the device's own numbers."""
    kw, iters = SMALL[name]
    scene = small_scene(**kw)
    gpu, R, Js = prepared(hip, oracle, scene, iters)
    check_parity(gpu, scene, R, Js, name)
    check_trace_identity(gpu, scene, R, Js, name)


def test_parity_long_trajectory(hip, oracle):
    scene = syn.make_scene(2, 1, True, 2, seed=4)      # 185 control points
    gpu, R, Js = prepared(hip, oracle, scene, 10)
    check_parity(gpu, scene, R, Js, "185 control points")
    check_trace_identity(gpu, scene, R, Js, "185 control points")


def test_parity_configs3_shape(hip, oracle):
    scene = full_size_scene(3)
    gpu, R, Js = prepared(hip, oracle, scene, 10)
    check_parity(gpu, scene, R, Js, "configs[3] shape")
    check_trace_identity(gpu, scene, R, Js, "configs[3] shape")


def test_trace_identity_configs4_shape(hip, oracle):
    """The configs[4] shape: S and H of the bound from the oracle's dense JᵀJ (its dense Jacobian is not formed)."""
    scene = full_size_scene(4)
    gpu = syn.build_problem(hip, scene)
    solve(gpu.problem, hip, 10)
    gpu.problem.covariance_compute(control_points=True)
    ref = syn.build_problem(oracle, scene)
    pr.copy_values(gpu, ref)
    R = pr.Reference.from_normal_matrix(ref.problem.evaluate()[2])
    check_trace_identity(gpu, scene, R, None, "configs[4] shape")


def test_tagged_observations_are_returned(hip, oracle):
    """After calico_mark_outliers the tagged observations still come back, valid, with P_i = J_i S J_iᵀ for an S that does
    not see them: rows from the oracle problem with them, S from the one without."""
    tau = 3.0
    scene = syn.make_scene(2, 1, True, 2, cam_rate=10.0, imu_rate=50.0, duration=3.0, segment_duration=3.0 / 23.9,
                           pixel_noise=0.1, gyro_noise=1e-3, accel_noise=1e-2, seed=21, outlier_fraction=0.04, robust=True)
    gpu = syn.build_problem(hip, scene)
    P = gpu.problem
    solve(P, hip, 40)
    scene2 = copy.deepcopy(scene)
    n_tagged = 0
    tags = {}
    for i, s in enumerate(scene.sensors):
        if s.kind != _capi.SENSOR_CAMERA:
            continue
        inl = P.inlier_mask(gpu.sensor_ids[i], s.n, tau).astype(bool)
        assert P.mark_outliers(gpu.sensor_ids[i], tau) == int((~inl).sum())
        tags[i] = ~inl
        n_tagged += int((~inl).sum())
        s2 = scene2.sensors[i]
        s2.meas, s2.stamps, s2.point_idx, s2.is_outlier = s.meas[inl], s.stamps[inl], s.point_idx[inl], s.is_outlier[inl]
    assert n_tagged > 0
    P.covariance_compute(control_points=True)
    ref_all, ref_all0 = pr.build_pair(oracle, scene)
    ref_fit = syn.build_problem(oracle, scene2)
    for r in (ref_all, ref_all0, ref_fit):
        pr.copy_values(gpu, r)
    R = pr.Reference(ref_fit)
    Js = {1: pr.dense_jacobian(ref_all), 0: pr.dense_jacobian(ref_all0)}
    assert Js[1].shape[1] == R.S.shape[0]
    check_parity(gpu, scene, R, Js, "%d tagged" % n_tagged)
    # the leverages of the untagged observations add up to the number of parameters; a tagged one may exceed 1
    total = 0.0
    for i, (sid, s) in enumerate(zip(gpu.sensor_ids, scene.sensors)):
        lev = P.prediction_covariance(sid)[1]
        total += float(lev[~tags[i]].sum()) if i in tags else float(lev.sum())
    want = expected_trace(P)
    print("tagged: sum of the untagged leverages %.10f, expected %d, deviation %.3e, bound %.3e" % (total, want, total - want, R.trace_bound(TOL)))
    assert abs(total - want) <= R.trace_bound(TOL)


def test_observation_that_cannot_be_evaluated(hip, oracle):
    """A chart point far behind the cameras, its observations tagged so that the fit does not see them: exactly those come
    back with valid = 0 and zeros, all others valid and in parity."""
    scene = copy.deepcopy(small_scene(camera_model=1, imu=True, seed=3))
    scene.points[5] = scene.points[5] + np.array([0.0, 0.0, 50.0])
    gpu = syn.build_problem(hip, scene)
    P = gpu.problem
    scene2 = copy.deepcopy(scene)
    bad = {}
    for i, s in enumerate(scene.sensors):
        if s.kind != _capi.SENSOR_CAMERA:
            continue
        bad[i] = s.point_idx == 5
        assert bad[i].any()
        P.set_outlier_mask(gpu.sensor_ids[i], bad[i].astype(np.uint8))
        s2 = scene2.sensors[i]
        keep = ~bad[i]
        s2.meas, s2.stamps, s2.point_idx = s.meas[keep], s.stamps[keep], s.point_idx[keep]
        if s.is_outlier is not None:
            s2.is_outlier = s.is_outlier[keep]
    P.covariance_compute(control_points=True)
    ref, ref0 = pr.build_pair(oracle, scene2)
    pr.copy_values(gpu, ref)
    pr.copy_values(gpu, ref0)
    R = pr.Reference(ref)
    Js = {1: R.J_fit, 0: pr.dense_jacobian(ref0)}
    for apply_loss in (1, 0):
        for i, (sid, s, (first, n2, d)) in enumerate(zip(gpu.sensor_ids, scene.sensors, pr.sensor_rows(scene2))):
            cov, lev, valid = P.prediction_covariance(sid, apply_loss=bool(apply_loss))
            keep = ~bad[i] if i in bad else np.ones(s.n, bool)
            assert np.array_equal(valid, keep)
            assert np.all(cov[~keep] == 0.0) and np.all(lev[~keep] == 0.0)
            Pref, beta = R.blocks(Js[apply_loss], first, n2, d)
            compare(cov[keep], lev[keep], Pref, beta, TOL)


def test_contracts(hip):
    scene = small_scene(camera_model=1, imu=True)
    g, h = syn.build_problem(hip, scene), syn.build_problem(hip, scene)
    P, Q = g.problem, h.problem
    sid = g.sensor_ids[0]

    def refused(call, code):
        with pytest.raises(_capi.CalicoError) as e:
            call()
        assert e.value.code == code, e.value
        return e.value.message

    assert "calico_covariance_compute" in refused(lambda: P.prediction_covariance(sid), _capi.FAILED_PRECONDITION)
    solve(P, hip, 5)
    solve(Q, hip, 5)
    P.covariance_compute()
    assert "control_points" in refused(lambda: P.prediction_covariance(sid), _capi.FAILED_PRECONDITION)
    P.covariance_compute(control_points=True)
    P.observability_compute()
    refused(lambda: P.prediction_covariance(-1), _capi.INVALID_ARGUMENT)
    refused(lambda: P.prediction_covariance(len(g.sensor_ids)), _capi.INVALID_ARGUMENT)
    refused(lambda: P.prediction_covariance(sid, apply_loss=2), _capi.INVALID_ARGUMENT)
    o = _capi.PredictionOptions()
    assert hip.prediction_covariance(P.h, sid, o, None, None, None) == _capi.INVALID_ARGUMENT
    sigma, spectrum, obs_matrix = P.covariance_dense(), P.observability_spectrum(), P.observability_matrix()
    runs = [[P.prediction_covariance(s, apply_loss=a) for s in g.sensor_ids for a in (True, False)] for _ in range(3)]
    for r in runs[1:]:
        for x, y in zip(r, runs[0]):
            assert all(np.array_equal(u, v) for u, v in zip(x, y))
    # NULL outputs: any subset
    n = scene.sensors[0].n
    lev = np.zeros(n)
    assert hip.prediction_covariance(P.h, sid, None, None, _capi._dp(lev), None) == _capi.OK
    assert np.array_equal(lev, runs[0][0][1])
    assert np.array_equal(P.covariance_dense(), sigma) and np.array_equal(P.observability_spectrum(), spectrum)
    assert np.array_equal(P.observability_matrix(), obs_matrix)
    # a solve after the call equals a solve without it
    sa, sb = solve(P, hip, 20), solve(Q, hip, 20)
    keys = [k for k, _ in _capi.Summary._fields_ if "time" not in k]
    assert [sa.as_dict()[k] for k in keys] == [sb.as_dict()[k] for k in keys]
    for blk, nb in dict(P._sizes).items():
        assert np.array_equal(P.get_param_block(blk, nb), Q.get_param_block(blk, nb))
    P.covariance_compute(control_points=True)
    assert P.prediction_covariance(sid)[0].shape == (n, 2, 2)
    P.add_param_block(np.ones(3))      # a structural change
    refused(lambda: P.prediction_covariance(sid), _capi.FAILED_PRECONDITION)


def test_multirank_two_handles_agree(hip, oracle):
    """Two ranks on one device with a host exchange: both ranks' outputs are bit-identical and within the parity bound of
    the single rank's with 1e-9 in place of 1e-7."""
    scene = small_scene(camera_model=1, imu=True, robust=True, seed=3)
    single, R, Js = prepared(hip, oracle, scene, 50)
    vals = {b: single.problem.get_param_block(b, n) for b, n in dict(single.problem._sizes).items()}
    one = {(s, a): single.problem.prediction_covariance(s, apply_loss=a) for s in single.sensor_ids for a in (True, False)}

    def per_rank(b):
        b.problem.covariance_compute(control_points=True)
        return {(s, a): b.problem.prediction_covariance(s, apply_loss=a) for s in b.sensor_ids for a in (True, False)}
    results = run_two_ranks(hip, scene, vals, per_rank)
    rows = dict(zip(single.sensor_ids, pr.sensor_rows(scene)))
    worst = 0.0
    for key, (cov, lev, valid) in results[0].items():
        c1, l1, v1 = results[1][key]
        assert np.array_equal(cov, c1) and np.array_equal(lev, l1) and np.array_equal(valid, v1)
        first, n, d = rows[key[0]]
        _, beta = R.blocks(Js[int(key[1])], first, n, d)
        err = np.abs(cov - one[key][0])
        bound = 1e-9 * beta[:, :, None] * beta[:, None, :]
        worst = max(worst, (err / bound).max() * 1e-9)
        assert np.all(err <= bound)
    print("two ranks against one: max |dP| / (beta_a beta_b) %.2e" % worst)


def _facade_rig():
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
    true_imu = np.array([1.3, 0.01, -0.01, 0.01])
    optimizer = calico.BatchOptimizer()
    specs = [(calico.Camera, calico.CameraIntrinsicsModel.kOpenCv5, true_cam, [0, 0, 0]),
             (calico.Camera, calico.CameraIntrinsicsModel.kOpenCv5, true_cam, [0.05, -0.02, 0.01]),
             (calico.Gyroscope, calico.GyroscopeIntrinsicsModel.kGyroscopeScaleAndBias, true_imu, [0, 0, 0]),
             (calico.Accelerometer, calico.AccelerometerIntrinsicsModel.kAccelerometerScaleAndBias, true_imu, [0.01, 0.02, 0.0])]
    sensors = []
    for n, (cls, model, intr, t) in enumerate(specs):
        truth = cls()
        assert truth.SetModel(model).ok()
        truth.SetIntrinsics(intr)
        ex = calico.Pose3d()
        ex.translation = np.array(t, float)
        truth.SetExtrinsics(ex)
        meas = truth.Project(times, trajectory, world)
        s = cls()
        assert s.SetModel(model).ok()
        s.SetIntrinsics(intr)
        s.SetExtrinsics(ex)
        s.EnableIntrinsicsEstimation(True)
        s.EnableExtrinsicsEstimation(n > 0)
        assert s.AddMeasurements(meas).ok()
        optimizer.AddSensor(s)
        sensors.append((s, len(meas)))
    optimizer.AddTrajectory(trajectory)
    optimizer.AddWorldModel(world)
    return optimizer, sensors


def test_python_facade_predictions(hip):
    """BatchOptimizer.ComputeCovariance(control_points=True).Predictions(sensor) on the stereo + IMU rig of the trajectory
    covariance's facade test."""
    from calico_amd import calico
    optimizer, sensors = _facade_rig()
    cov = optimizer.ComputeCovariance(control_points=True)
    total = 0.0
    for s, n in sensors:
        d = 2 if isinstance(s, calico.Camera) else 3
        P, lev, valid = cov.Predictions(s)
        assert P.shape == (n, d, d) and lev.shape == (n,) and valid.shape == (n,) and valid.dtype == bool and valid.all()
        assert np.array_equal(lev, np.einsum("nii->n", P))
        for v in P:
            assert np.array_equal(v, v.T)
            ev = np.linalg.eigvalsh(v)
            assert ev.min() >= -1e-12 * ev.max()
        P0, _, _ = cov.Predictions(s, apply_loss=False)
        assert P0.shape == P.shape
        total += float(lev.sum())
    n_cp = 0
    while True:
        try:
            cov.ControlPoints(n_cp, n_cp)
        except Exception:      # noqa: BLE001  (an index past the last control point)
            break
        n_cp += 1
    want = 6 * n_cp + cov.Dimension() - cov.NumUnobserved()
    print("facade: sum of the four sensors' leverages %.10f, 6 n_cp + Dimension() - NumUnobserved() = %d, deviation %.3e"
          % (total, want, total - want))
    cov0 = optimizer.ComputeCovariance()
    with pytest.raises(Exception):
        cov0.Predictions(sensors[0][0])


@pytest.mark.parametrize("shape", ["configs3", "configs4"])
def test_wall_time(shape, hip):
    """Wall time of a synchronised call per sensor kind and in total, after a warm-up, next to covariance_compute with control
    points on the same handle (median of 5; the kernel's own time: rocprofv3 --kernel-trace --stats)."""
    scene = full_size_scene(3 if shape == "configs3" else 4)
    gpu = syn.build_problem(hip, scene)
    P = gpu.problem
    solve(P, hip, 10)
    P.covariance_compute(control_points=True)
    t_cov, t_pred = [], []
    for sid in gpu.sensor_ids:
        P.prediction_covariance(sid)
    for _ in range(5):
        t0 = time.perf_counter()
        P.covariance_compute(control_points=True)
        t1 = time.perf_counter()
        for sid in gpu.sensor_ids:
            P.prediction_covariance(sid)
        t_cov.append(t1 - t0)
        t_pred.append(time.perf_counter() - t1)
    print("%s: %d blocks, %d sensors: prediction_covariance of all sensors %.3f ms, covariance_compute(control_points=True) "
          "%.3f ms (median of 5)" % (shape, scene.num_blocks, len(gpu.sensor_ids), 1e3 * np.median(t_pred), 1e3 * np.median(t_cov)))
