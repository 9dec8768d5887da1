"""The trajectory's part of Σ (calico_covariance_compute with control_points = 1): the control points' band blocks, their
cross blocks with the border, and the covariance of the spline's 6-vector at stamps, against a dense reference built from
the oracle.

Reference: the oracle's dense JᵀJ at the GPU's parameter values, exactly-zero diagonal columns dropped, inverted with numpy;
tangent order [control points | border]. Entries are compared relative to sqrt(Σ_ii Σ_jj), the bound of the border's tests."""
import time

import numpy as np
import pytest

from calico_amd import _capi, synthetic as syn
from helpers import border_layout, full_size_scene, run_two_ranks, small_scene, solve

pytestmark = pytest.mark.gpu

TOL = 1e-7


def reference_full(gpu, ref):
    for b, n in dict(gpu.problem._sizes).items():
        ref.problem.set_param_block(b, gpu.problem.get_param_block(b, n))
    _, _, H = ref.problem.evaluate()
    keep = np.diag(H) != 0.0
    idx = np.nonzero(keep)[0]
    S = np.zeros_like(H)
    S[np.ix_(idx, idx)] = np.linalg.inv(H[np.ix_(idx, idx)])
    return S


def gpu_blocks(gpu, scene):
    """The GPU's Σ in the reference's order, filled where it is computed (band, cross blocks, border), and that mask."""
    P = gpu.problem
    dim = P.covariance_info()[0]
    n_cp, k, _ = P.covariance_trajectory_info()
    ctrl = [int(c) for c in gpu.ctrl_blocks]
    assert n_cp == len(ctrl) and k == scene.order
    layout, d2 = border_layout(gpu, scene)
    assert d2 == dim
    nc = 6 * n_cp
    G = np.zeros((nc + dim, nc + dim))
    mask = np.zeros(G.shape, bool)
    G[nc:, nc:] = P.covariance_dense()
    mask[nc:, nc:] = True
    for i in range(n_cp):
        for j in range(max(0, i - k + 1), min(n_cp, i + k)):
            G[6 * i:6 * i + 6, 6 * j:6 * j + 6] = P.covariance_block(ctrl[i], ctrl[j], tangent=True)
            mask[6 * i:6 * i + 6, 6 * j:6 * j + 6] = True
        for b, (o, t) in layout.items():
            blk = P.covariance_block(ctrl[i], b, tangent=True)
            assert blk.shape == (6, t)
            G[6 * i:6 * i + 6, nc + o:nc + o + t] = blk
            G[nc + o:nc + o + t, 6 * i:6 * i + 6] = blk.T
            mask[6 * i:6 * i + 6, nc + o:nc + o + t] = mask[nc + o:nc + o + t, 6 * i:6 * i + 6] = True
    for b0 in list(layout)[:1]:
        assert np.array_equal(P.covariance_block(b0, ctrl[0], tangent=True), P.covariance_block(ctrl[0], b0, tangent=True).T)
    return G, mask


def masked_err(G, S, mask):
    d = np.sqrt(np.abs(np.diag(S)))
    d = np.where(d > 0, d, 1.0)
    return (np.abs(G - S) / np.outer(d, d))[mask].max()


def check_trajectory_parity(gpu, ref, scene, what):
    P = gpu.problem
    dim, _, piv = P.covariance_compute(control_points=True)
    n_cp, k, piv_band = P.covariance_trajectory_info()
    S = reference_full(gpu, ref)
    assert S.shape[0] == 6 * n_cp + dim      # (every control point of these scenes is observed)
    G, mask = gpu_blocks(gpu, scene)
    nc = 6 * n_cp
    err_band = masked_err(G[:nc, :nc], S[:nc, :nc], mask[:nc, :nc])
    d = np.sqrt(np.abs(np.diag(S)))
    d = np.where(d > 0, d, 1.0)
    err_cross = (np.abs(G[:nc, nc:] - S[:nc, nc:]) / np.outer(d[:nc], d[nc:])).max() if dim else 0.0
    print("trajectory covariance %s: %d control points, order %d, border %d, min relative pivot band %.3e / border %.3e, "
          "max rel err band %.2e, cross %.2e" % (what, n_cp, k, dim, piv_band, piv, err_band, err_cross))
    assert err_band <= TOL and err_cross <= TOL
    return S, G


def reference_stamps(S_cp, scene, stamps):
    W, seg = syn.spline_weights(np.asarray(scene.knots), np.asarray(scene.basis), scene.order, np.asarray(stamps), 0)
    k = scene.order
    out, scale = [], []
    sd = np.sqrt(np.abs(np.diag(S_cp)))
    for w, s in zip(W, seg):
        V = np.zeros((6, 6))
        B = np.zeros((6, 6))
        for i in range(k):
            for j in range(k):
                a, b = 6 * (s + i), 6 * (s + j)
                V += w[i] * w[j] * S_cp[a:a + 6, b:b + 6]
                B += abs(w[i] * w[j]) * np.outer(sd[a:a + 6], sd[b:b + 6])
        out.append(V)
        scale.append(B)
    return np.array(out), np.array(scale)


def valid_range(scene):
    deg = scene.order - 1
    return np.asarray(scene.knots)[deg:len(scene.knots) - deg]


def stamp_grid(scene):
    vk = valid_range(scene)
    return np.concatenate([np.linspace(vk[0], vk[-1], 41), vk, [vk[-1]]])


def check_stamps(gpu, scene, S):
    P = gpu.problem
    n_cp = P.covariance_trajectory_info()[0]
    t = stamp_grid(scene)
    V = P.covariance_trajectory(t)
    assert V.shape == (len(t), 6, 6)
    R, B = reference_stamps(S[:6 * n_cp, :6 * n_cp], scene, t)
    err = (np.abs(V - R) / B).max()
    for v in V:
        assert np.array_equal(v, v.T)
        ev = np.linalg.eigvalsh(v)
        assert ev.min() >= -1e-12 * ev.max()
    print("stamps: %d, max rel err %.2e" % (len(t), err))
    assert err <= TOL
    return V


@pytest.mark.parametrize("order", [4, 6, 7, 8])
def test_orders_parity(order, hip, oracle):
    """Orders 4 and 6: the tree solver's plan; 7 and 8: the banded solver's. The new kernels read neither's workspace."""
    scene = small_scene(camera_model=1, imu=True, order=order)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip)
    S, _ = check_trajectory_parity(gpu, ref, scene, "order %d" % order)
    check_stamps(gpu, scene, S)


def test_robust_loss_and_unobserved_gyroscope_lever_arm(hip, oracle):
    scene = small_scene(camera_model=1, imu=True, imu_model=2, robust=True)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip)
    S, _ = check_trajectory_parity(gpu, ref, scene, "robust, imu 2")
    assert gpu.problem.covariance_info()[1] >= 3
    gyro = [b for s, b in zip(scene.sensors, gpu.sensor_blocks) if s.kind == _capi.SENSOR_GYROSCOPE][0]
    assert np.all(gpu.problem.covariance_block(int(gpu.ctrl_blocks[2]), gyro["t"]) == 0.0)


def test_free_model_points_parity(hip, oracle):
    scene = small_scene(camera_model=1, n_cameras=2, imu=True, free_points=True, seed=5)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip, 25)
    check_trajectory_parity(gpu, ref, scene, "free model points")


@pytest.mark.parametrize("border", ["none", "latency"])
def test_narrow_border_parity(border, hip, oracle):
    """Borders narrower than a control point: every calibration block constant (border of 0 columns: the trajectory alone,
    how well the data pin the motion with calibrated sensors), or only camera 1's latency free (1 column)."""
    scene = small_scene(camera_model=1, n_cameras=2, imu=True)
    for i, s in enumerate(scene.sensors):
        s.enable_intrinsics = s.enable_extrinsics = False
        s.enable_latency = border == "latency" and i == 1
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    S, _ = check_trajectory_parity(gpu, ref, scene, "border %s" % border)
    assert gpu.problem.covariance_info()[0] == (0 if border == "none" else 1)
    check_stamps(gpu, scene, S)


def test_configs3_shape_parity(hip, oracle):
    scene = full_size_scene(3)
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip, 10)
    S, _ = check_trajectory_parity(gpu, ref, scene, "configs[3] shape")
    check_stamps(gpu, scene, S)


def test_long_trajectory_parity(hip, oracle):
    scene = syn.make_scene(2, 1, True, 2, seed=4)      # 185 control points: a tree of several levels
    gpu, ref = syn.build_problem(hip, scene), syn.build_problem(oracle, scene)
    solve(gpu.problem, hip, 10)
    S, _ = check_trajectory_parity(gpu, ref, scene, "185 control points")
    check_stamps(gpu, scene, S)


def long_scene():
    """The configs[3] shape with knots at 50 Hz: 440 control points."""
    return syn.make_scene(4, 1, True, 2, cam_rate=20.0, imu_rate=200.0, duration=8.7, chart="april", seed=0xCA11C0 + 3,
                          pixel_noise=0.1, gyro_noise=1.7e-4 * np.sqrt(200.0), accel_noise=2e-3 * np.sqrt(200.0),
                          robust=True, segment_duration=8.7 / 23.9, knot_frequency=50.0)


@pytest.mark.parametrize("shape", ["configs3", "configs4", "long"])
def test_wall_time(shape, hip):
    """Wall time of a compute with and without the control points' blocks (the kernels' own times: rocprofv3)."""
    scene = {"configs3": lambda: full_size_scene(3), "configs4": lambda: full_size_scene(4),
             "long": long_scene}[shape]()
    gpu = syn.build_problem(hip, scene)
    solve(gpu.problem, hip, 10)
    P = gpu.problem
    med = {}
    for cp in (False, True):
        P.covariance_compute(control_points=cp)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            P.covariance_compute(control_points=cp)
            ts.append(time.perf_counter() - t0)
        med[cp] = 1e3 * np.median(ts)
    n_cp, k, piv = P.covariance_trajectory_info()
    V = P.covariance_trajectory(stamp_grid(scene))
    assert np.all(np.linalg.eigvalsh(V).min(axis=1) >= -1e-12 * np.abs(V).max())
    print("%s: %d control points, order %d, border %d, band pivot %.2e: covariance_compute %.3f ms, with control points %.3f ms "
          "(median of 5)" % (shape, n_cp, k, P.covariance_info()[0], piv, med[False], med[True]))


def test_no_change_to_existing_behaviour(hip):
    scene = small_scene(camera_model=1, imu=True)
    a, b = syn.build_problem(hip, scene), syn.build_problem(hip, scene)
    solve(a.problem, hip, 5)
    solve(b.problem, hip, 5)
    a.problem.covariance_compute()
    b.problem.covariance_compute(control_points=True)
    assert np.array_equal(a.problem.covariance_dense(), b.problem.covariance_dense())
    assert a.problem.covariance_info() == b.problem.covariance_info()
    # without the flag the control points' blocks stay unimplemented, and there is no trajectory result
    c0, intr = int(a.ctrl_blocks[3]), a.sensor_blocks[0]["intrinsics"]
    for x, y in ((c0, intr), (c0, c0)):
        with pytest.raises(_capi.CalicoError) as e:
            a.problem.covariance_block(x, y)
        assert e.value.code == _capi.UNIMPLEMENTED
    for call in (lambda: a.problem.covariance_trajectory([valid_range(scene)[0]]), a.problem.covariance_trajectory_info):
        with pytest.raises(_capi.CalicoError) as e:
            call()
        assert e.value.code == _capi.FAILED_PRECONDITION
    # a solve after the compute is bit-identical to one without it
    sa, sb = solve(a.problem, hip, 20), solve(b.problem, hip, 20)
    keys = [k for k, _ in _capi.Summary._fields_ if "time" not in k]
    assert [sa.as_dict()[k] for k in keys] == [sb.as_dict()[k] for k in keys]
    for blk, n in dict(a.problem._sizes).items():
        assert np.array_equal(a.problem.get_param_block(blk, n), b.problem.get_param_block(blk, n))


def test_errors_and_staleness(hip):
    scene = small_scene(camera_model=1, imu=True)
    g = syn.build_problem(hip, scene)
    P = g.problem
    solve(P, hip, 10)
    P.covariance_compute(control_points=True)
    n_cp, k, _ = P.covariance_trajectory_info()
    ctrl = [int(c) for c in g.ctrl_blocks]
    assert P.covariance_block(ctrl[0], ctrl[k - 1]).shape == (6, 6)
    with pytest.raises(_capi.CalicoError) as e:
        P.covariance_block(ctrl[0], ctrl[k])
    assert e.value.code == _capi.UNIMPLEMENTED and "support" in e.value.message
    vk = valid_range(scene)
    for t in (vk[0] - 1e-3, vk[-1] + 1e-3, np.nan):
        with pytest.raises(_capi.CalicoError) as e:
            P.covariance_trajectory([vk[0], t])
        assert e.value.code == _capi.INVALID_ARGUMENT
    assert P.covariance_trajectory([]).shape == (0, 6, 6)
    P.add_param_block(np.ones(3))      # a structural change
    for call in (lambda: P.covariance_trajectory([vk[0]]), P.covariance_trajectory_info,
                 lambda: P.covariance_block(ctrl[0], ctrl[1])):
        with pytest.raises(_capi.CalicoError) as e:
            call()
        assert e.value.code == _capi.FAILED_PRECONDITION
    P.covariance_compute()
    with pytest.raises(_capi.CalicoError) as e:
        P.covariance_trajectory([vk[0]])
    assert e.value.code == _capi.FAILED_PRECONDITION


def test_gauge_deficiency_is_refused_with_control_points(hip):
    scene = small_scene(camera_model=1, imu=False, free_chart_pose=True)
    gpu = syn.build_problem(hip, scene)
    with pytest.raises(_capi.CalicoError) as e:
        gpu.problem.covariance_compute(control_points=True)
    assert e.value.code == _capi.FAILED_PRECONDITION and "rank deficient" in e.value.message
    with pytest.raises(_capi.CalicoError) as e:
        gpu.problem.covariance_trajectory_info()
    assert e.value.code == _capi.FAILED_PRECONDITION


def test_determinism(hip):
    scene = small_scene(camera_model=1, imu=True, order=6)
    g = syn.build_problem(hip, scene)
    solve(g.problem, hip)
    t = stamp_grid(scene)
    res = []
    for _ in range(3):
        g.problem.covariance_compute(control_points=True)
        G, _ = gpu_blocks(g, scene)
        res.append((G, g.problem.covariance_trajectory(t)))
    for G, V in res[1:]:
        assert np.array_equal(G, res[0][0]) and np.array_equal(V, res[0][1])


def test_multirank_two_handles_agree(hip):
    """Two ranks on one device with a host exchange (the pattern of test_gpu_covariance): the trajectory blocks of both
    ranks are bit-identical and within 1e-9 of the single rank's."""
    scene = small_scene(camera_model=1, imu=True, robust=True, seed=3)
    single = syn.build_problem(hip, scene)
    solve(single.problem, hip)
    vals = {b: single.problem.get_param_block(b, n) for b, n in dict(single.problem._sizes).items()}
    single.problem.covariance_compute(control_points=True)
    G1, mask = gpu_blocks(single, scene)
    t = stamp_grid(scene)
    V1 = single.problem.covariance_trajectory(t)

    def per_rank(b):
        b.problem.covariance_compute(control_points=True)
        return b, b.problem.covariance_trajectory(t)
    both = run_two_ranks(hip, scene, vals, per_rank)
    ranks, results = [x[0] for x in both], [x[1] for x in both]
    Gs = [gpu_blocks(b, scene)[0] for b in ranks]
    assert np.array_equal(Gs[0], Gs[1]) and np.array_equal(results[0], results[1])
    err = masked_err(Gs[0], G1, mask)
    assert err <= 1e-9, err
    d = np.sqrt(np.abs(np.einsum("nii->ni", V1)))
    assert (np.abs(results[0] - V1) / np.einsum("ni,nj->nij", d, d)).max() <= 1e-9


def test_python_facade_trajectory_covariance(hip):
    """BatchOptimizer.ComputeCovariance(control_points=True) on a stereo + IMU rig at its true values: Trajectory(stamps) is
    (n, 6, 6), symmetric positive semidefinite and the weighted sum of the ControlPoints(i, j) blocks it is made of; the
    border's Σ does not change with the keyword."""
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
    optimizer.AddTrajectory(trajectory)
    optimizer.AddWorldModel(world)
    cov0 = optimizer.ComputeCovariance()
    cov = optimizer.ComputeCovariance(control_points=True)
    assert cov.Dimension() == cov0.Dimension()
    t = np.linspace(times[0] + 0.1, times[-1] - 0.1, 17)
    V = cov.Trajectory(list(t))
    assert V.shape == (len(t), 6, 6)
    for v in V:
        assert np.array_equal(v, v.T)
        ev = np.linalg.eigvalsh(v)
        assert ev.max() > 0 and ev.min() >= -1e-12 * ev.max()
    C00, C01 = cov.ControlPoints(5, 5), cov.ControlPoints(5, 6)
    assert C00.shape == (6, 6) and np.array_equal(C00, C00.T) and np.linalg.eigvalsh(C00).min() > 0
    assert np.array_equal(cov.ControlPoints(6, 5), C01.T)
    # Trajectory(t) = Σ_ij w_i(t) w_j(t) ControlPoints(s + i, s + j): the facade's index mapping of the control points
    # against the library's own (the knots and basis of Trajectory::FitSpline, restated: the poses' first stamp, 10 Hz
    # knots, order 6)
    order, kf = 6, 10.0
    deg = order - 1
    t0 = min(times)
    nvalid = 1 + int(np.ceil((max(times) - t0) * kf))
    knots = np.array([t0 + (1.0 / kf) * i for i in range(-deg, nvalid + deg)])
    basis = syn.basis_matrices(knots, order)
    W, seg = syn.spline_weights(knots, basis, order, t, 0)
    n_cp = len(knots) - order
    for v, w, s in zip(V, W, seg):
        assert s + order <= n_cp
        R, B = np.zeros((6, 6)), np.zeros((6, 6))
        for i in range(order):
            for j in range(order):
                blk = cov.ControlPoints(int(s + i), int(s + j))
                R += w[i] * w[j] * blk
                B += abs(w[i] * w[j]) * np.sqrt(np.outer(np.diag(cov.ControlPoints(int(s + i), int(s + i))),
                                                         np.diag(cov.ControlPoints(int(s + j), int(s + j)))))
        assert (np.abs(v - R) / B).max() <= 1e-10
    with pytest.raises(Exception):
        cov.ControlPoints(0, n_cp)          # (an index past the last control point)
    with pytest.raises(Exception):
        cov.ControlPoints(0, order)         # (outside the spline's support: not computed)
    with pytest.raises(Exception):
        cov0.Trajectory([float(t[0])])
    print("facade: %d control points, pose sd at t = %.2f: %s" % (n_cp, t[8], np.sqrt(np.diag(V[8]))))


def test_covariance_trajectory_of_the_ctypes_problem_matches_blocks(hip):
    """covariance_trajectory equals the weighted sum of the control points' band blocks read back through covariance_block
    (w(t)ᵀ Σ w(t) in numpy, to rounding)."""
    scene = small_scene(camera_model=1, imu=True)
    g = syn.build_problem(hip, scene)
    solve(g.problem, hip)
    g.problem.covariance_compute(control_points=True)
    G, _ = gpu_blocks(g, scene)
    n_cp = g.problem.covariance_trajectory_info()[0]
    t = stamp_grid(scene)
    V = g.problem.covariance_trajectory(t)
    R, B = reference_stamps(G[:6 * n_cp, :6 * n_cp], scene, t)
    assert (np.abs(V - R) / B).max() <= 1e-13
