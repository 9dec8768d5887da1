"""The notebook flow for a camera that is not a pinhole: detect -> utils.InitializePoses -> Trajectory.FitSpline -> Optimize.
A KannalaBrandt camera with a gyroscope and an accelerometer over a six-second excitation; the solve whose spline was fitted
from the resected poses ends in the minimum of the solve whose spline was fitted from the true poses."""
import numpy as np
import pytest

import __graft_entry__ as _entry

_entry.build_hip()
_entry.build_python_module()   # no-ops when the in-tree libraries are up to date

from calico_amd import calico, synthetic as syn  # noqa: E402

KB = np.array([785.0, 640, 400, -1.3e-2, 2.1e-3, -8.0e-4, 1.0e-4])
IMU = np.array([1.3, 0.01, -0.01, 0.01])


def _pose(q_xyzw, t):
    p = calico.Pose3d()
    p.rotation = [q_xyzw[3], q_xyzw[0], q_xyzw[1], q_xyzw[2]]
    p.translation = t
    return p


def _quat_of(R):
    """(x, y, z, w), stable at every angle."""
    d = [R[0, 0], R[1, 1], R[2, 2], np.trace(R)]
    i = int(np.argmax(d))
    if i == 3:
        s = 2 * np.sqrt(1 + d[3])
        return np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s])
    j, k = (i + 1) % 3, (i + 2) % 3
    s = 2 * np.sqrt(1 + R[i, i] - R[j, j] - R[k, k])
    q = np.zeros(4)
    q[i], q[j], q[k], q[3] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    return q


@pytest.mark.gpu
def test_resected_poses_start_a_calibration_that_ends_where_the_true_poses_do():
    stamps, quats, trans = syn.default_synthetic_poses(segment_duration=0.25)
    true_poses = {float(t): _pose(q, p) for t, q, p in zip(stamps, quats, trans)}
    truth = calico.Trajectory()
    truth.FitSpline(true_poses)
    chart = calico.RigidBody()
    model_definition = {i: p for i, p in enumerate(syn.planar_points())}
    chart.model_definition = model_definition
    chart.world_pose_is_constant = True
    chart.model_definition_is_constant = True
    world = calico.WorldModel()
    world.AddRigidBody(chart)
    rng = np.random.default_rng(11)
    specs = [("camera", calico.Camera, calico.CameraIntrinsicsModel.kKannalaBrandt, KB, 0.1),
             ("gyro", calico.Gyroscope, calico.GyroscopeIntrinsicsModel.kGyroscopeScaleAndBias, IMU, 1e-3),
             ("acc", calico.Accelerometer, calico.AccelerometerIntrinsicsModel.kAccelerometerScaleAndBias, IMU, 1e-2)]
    times = [float(t) for t in stamps]
    measurements = {}
    for name, cls, model, intrinsics, noise in specs:
        s = cls()
        assert s.SetModel(model).ok()
        s.SetIntrinsics(intrinsics)
        ms = s.Project(times if name == "camera" else list(np.arange(times[0], times[-1], 0.01)), truth, world)
        for m in ms:
            if name == "camera":
                m.pixel = m.pixel + noise * rng.standard_normal(2)
            else:
                m.measurement = m.measurement + noise * rng.standard_normal(3)
        measurements[name] = ms

    # the detector's output, frame by frame: {feature id: pixel}
    frames = {}
    for m in measurements["camera"]:
        frames.setdefault(m.id.stamp, {})[m.id.feature_id] = np.asarray(m.pixel)
    frame_stamps = sorted(frames)
    assert len(frame_stamps) == len(times) and all(len(frames[t]) == 36 for t in frame_stamps)

    def solve(poses):
        trajectory = calico.Trajectory()
        trajectory.FitSpline(poses)
        optimizer = calico.BatchOptimizer()
        sensors = {}
        for name, cls, model, intrinsics, _ in specs:
            s = cls()
            s.SetName(name)
            assert s.SetModel(model).ok()
            s.SetIntrinsics(intrinsics)
            s.EnableIntrinsicsEstimation(True)
            s.EnableExtrinsicsEstimation(False)
            s.EnableLatencyEstimation(False)
            assert s.AddMeasurements(measurements[name]).ok()
            optimizer.AddSensor(s)
            sensors[name] = s
        optimizer.AddTrajectory(trajectory)
        optimizer.AddWorldModel(world)
        options = calico.DefaultSolverOptions()
        options.minimizer_progress_to_stdout = False
        options.max_num_iterations = 100
        options.function_tolerance = 1e-12
        return optimizer.Optimize(options), sensors

    camera = calico.Camera()
    camera.SetModel(calico.CameraIntrinsicsModel.kKannalaBrandt)
    camera.SetIntrinsics(KB)
    R_wc, t_wc, ok = calico.InitializePoses(camera, [frames[t] for t in frame_stamps], model_definition)
    assert ok.all() and len(R_wc) == len(frame_stamps)
    # the pixels were made on the fitted spline, not at the poses it was fitted to
    worst = max(np.abs(t - p.translation).max() for t, p in zip(t_wc, truth.Interpolate(frame_stamps)))
    print("resected camera positions against the truth:", worst)
    assert worst < 1e-3      # (0.1 px of noise on 36 points at a metre and f = 785: some 1e-4 m)
    resected = {t: _pose(_quat_of(R), p) for t, R, p in zip(frame_stamps, R_wc, t_wc)}

    from_truth, _ = solve(true_poses)
    from_resection, sensors = solve(resected)
    print(from_truth.BriefReport())
    print(from_resection.BriefReport())
    assert from_truth.termination_type == 0 and from_resection.termination_type == 0      # CALICO_CONVERGENCE
    assert abs(from_resection.final_cost - from_truth.final_cost) <= 1e-6 * from_truth.final_cost
    np.testing.assert_allclose(sensors["camera"].GetIntrinsics()[:3], KB[:3], rtol=1e-3)
