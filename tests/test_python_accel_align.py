"""Trajectory.AlignAccelerometer and utils.InitializeAccelerometer through the Python surface. Without a GPU: the names, the option
dict, the library's argument errors as they reach Python, and what the numpy reference reaches on Project()-style data. On the GPU
(Trajectory.FitSpline runs there): a gyroscope and an accelerometer of one unit, mounted at 40 degrees with a latency of 13.7 ms
and biases, the accelerometer 0.1 m off the rig's origin, all of it UNKNOWN at the start -- InitializeImu sets rotation and latency
(and leaves the translation alone), InitializeAccelerometer then sets rotation, TRANSLATION, latency, bias and the world's gravity.

Project() takes the spline segment of the true time, so its data lie outside the model the alignment shares with the optimiser.
REF_PROJECT is what the numpy reference reaches on the same data in numpy (synthetic.default_synthetic_poses fitted by
synthetic.fit_trajectory, synthetic.project_accelerometer at the poses' stamps): here no sample's latency carries it across a knot
and the figure is rounding. The device is held to ten times that."""
import numpy as np
import pytest

import accel_align_ref as ar
from calico_amd import calico, synthetic as syn

REF_PROJECT = 1.4e-14      # 2026-10-20: the largest difference (rad, m, m/s^2, s) of the reference's result to the truth, 240 samples
LEVER = np.array(ar.LEVER)
BIAS = np.array([0.05, -0.03, 0.02])
GRAVITY = np.array([0.3, -9.7, 0.9])
LATENCY = 0.0137


def _pose(axis, angle_deg, t=(0.0, 0.0, 0.0)):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    half = 0.5 * np.deg2rad(angle_deg)
    p = calico.Pose3d()
    p.rotation = [np.cos(half), *(np.sin(half) * axis)]
    p.translation = np.asarray(t, float)
    return p


def _trajectory():
    stamps, quats, trans = syn.default_synthetic_poses()
    poses = {}
    for t, q, p in zip(stamps, quats, trans):
        T = calico.Pose3d()
        T.rotation = [q[3], q[0], q[1], q[2]]
        T.translation = p
        poses[float(t)] = T
    trajectory = calico.Trajectory()
    trajectory.FitSpline(poses)
    return [float(t) for t in stamps], trajectory


def test_python_surfaces_expose_the_new_names():
    assert hasattr(calico.Trajectory, "AlignAccelerometer") and callable(calico.InitializeAccelerometer)
    trajectory, acc = calico.Trajectory(), calico.Accelerometer()
    with pytest.raises(RuntimeError, match="calico_accel_align: order"):      # (no spline yet: the library's own argument rule)
        trajectory.AlignAccelerometer(acc)
    with pytest.raises(TypeError, match="no accelerometer alignment option"):
        trajectory.AlignAccelerometer(acc, options={"no_such_option": 1})
    with pytest.raises(RuntimeError, match="IMU model 0"):      # (no model set: refused before anything is changed)
        calico.InitializeAccelerometer(trajectory, acc)
    assert acc.SetModel(calico.AccelerometerIntrinsicsModel.kAccelerometerScaleAndBias).ok()
    with pytest.raises(RuntimeError, match="Error: calico_accel_align"):
        calico.InitializeAccelerometer(trajectory, acc)


def test_the_reference_on_project_style_data():
    stamps, quats, trans = syn.default_synthetic_poses()
    knots, basis, ctrl = syn.fit_trajectory(stamps, quats, trans, 10.0, 6)
    spl = (knots, basis, ctrl, 6)
    truth = dict(q=ar.ir.TRUTH["q"], t_rig_accel=LEVER, accel_bias=BIAS, gravity=GRAVITY, latency=LATENCY)
    meas, st = syn.project_accelerometer(spl, 2, np.concatenate([[1.0], BIAS]), truth["q"], LEVER, LATENCY, GRAVITY, np.asarray(stamps, float))
    r = ar.align(spl, st, meas, *ar.imu_start(truth, 1e-8, 1e-8))
    dist = ar.distance_to_truth(ar.estimate(r), truth)
    print("reference on Project()-style data: distance to the truth", dist, "rms", r["rms"], "samples", r["samples"], "iterations", r["iterations"])
    assert r["status"] == ar.OK and r["samples"] == len(stamps) - 1 == 239      # (the last stamp lies behind the knots)
    assert dist <= 2 * REF_PROJECT


@pytest.mark.gpu
def test_too_few_samples_raise_and_change_nothing():
    times, trajectory = _trajectory()      # (FitSpline runs on the device)
    acc = calico.Accelerometer()
    assert acc.SetModel(calico.AccelerometerIntrinsicsModel.kAccelerometerScaleAndBias).ok()
    acc.SetIntrinsics([1.0, 7.0, 8.0, 9.0])
    acc.SetExtrinsics(_pose([0.0, 0.0, 1.0], 10.0, (1.0, 2.0, 3.0)))
    assert acc.SetLatency(0.004).ok()
    world = calico.WorldModel()
    world.SetGravity([1.0, 2.0, 3.0])
    with pytest.raises(RuntimeError, match="must all be estimated"):
        trajectory.AlignAccelerometer(acc, options={"estimate_gravity": 0})
    r = trajectory.AlignAccelerometer(acc, covariance=True)      # no measurements: OK with TOO_FEW_SAMPLES, the start in the outputs
    assert r["status"] == 1 and r["linear_status"] == -1 and r["samples"] == 0 and r["cov"].shape == (13, 13) and not r["cov"].any()
    assert r["latency"] == 0.004 and r["t_rig_accel"].tolist() == [0, 0, 0]
    with pytest.raises(RuntimeError, match="Error: the accelerometer alignment ended with status 1"):
        calico.InitializeAccelerometer(trajectory, acc, world)
    assert np.array_equal(acc.GetIntrinsics(), [1.0, 7.0, 8.0, 9.0]) and acc.GetLatency() == 0.004
    assert np.array_equal(acc.GetExtrinsics().translation, [1.0, 2.0, 3.0]) and np.array_equal(np.asarray(world.GetGravity()), [1.0, 2.0, 3.0])


@pytest.mark.gpu
def test_initialize_accelerometer_sets_the_mounting():
    times, trajectory = _trajectory()
    world_true, world = calico.WorldModel(), calico.WorldModel()
    world_true.SetGravity(list(GRAVITY))
    specs = [("gyro", calico.Gyroscope, calico.GyroscopeIntrinsicsModel.kGyroscopeScaleAndBias, np.array([1.0, 0.01, -0.02, 0.015]),
              _pose([1.0, -2.0, 2.0], 40.0)),
             ("acc", calico.Accelerometer, calico.AccelerometerIntrinsicsModel.kAccelerometerScaleAndBias, np.concatenate([[1.0], BIAS]),
              _pose([1.0, -2.0, 2.0], 40.0, LEVER))]
    sensors = {}
    for name, cls, model, intrinsics, extrinsics in specs:
        true_sensor = cls()
        assert true_sensor.SetModel(model).ok()
        true_sensor.SetIntrinsics(intrinsics)
        true_sensor.SetExtrinsics(extrinsics)
        assert true_sensor.SetLatency(LATENCY).ok()
        sensor = cls()
        assert sensor.SetModel(model).ok()
        sensor.SetIntrinsics([1.0, 0.0, 0.0, 0.0])      # nothing known about the IMU but its unit scale
        measurements = true_sensor.Project(times, trajectory, world_true)
        assert sensor.AddMeasurements(measurements).ok()
        sensors[name] = sensor
    gyro, acc = sensors["gyro"], sensors["acc"]
    mount = specs[1][4]
    ri = calico.InitializeImu(trajectory, gyro, acc, world, options={"max_lag": 0.05, "lag_step": 0.0025})
    # InitializeImu copies the gyroscope's rotation and latency and never touches the translation; with the lever arm taken as
    # zero its gravity and bias carry the lever-arm terms
    assert np.array_equal(acc.GetExtrinsics().translation, [0.0, 0.0, 0.0]) and acc.GetLatency() == ri["latency"]
    print("after InitializeImu: gravity off by", np.abs(ri["gravity_world"] - GRAVITY).max(), "bias off by", np.abs(ri["accel_bias"] - BIAS).max())
    r = calico.InitializeAccelerometer(trajectory, acc, world)
    assert r["status"] == 0 and r["linear_status"] == 0 and r["samples"] == len(times) - 1 == 239
    # the sensor and the world model carry the estimates
    x, y, z, w = r["q_rig_accel"]
    assert np.allclose(acc.GetExtrinsics().rotation, [w, x, y, z], rtol=0, atol=1e-15) and acc.GetLatency() == r["latency"]
    assert np.array_equal(acc.GetExtrinsics().translation, r["t_rig_accel"])
    assert np.array_equal(acc.GetIntrinsics(), np.concatenate([[1.0], r["bias"]]))
    assert np.array_equal(np.asarray(world.GetGravity()), r["gravity_world"])
    # they are the truth: ten times what the numpy reference reaches on the same data (REF_PROJECT, measured by the host half)
    got = np.asarray(acc.GetExtrinsics().rotation)
    sign = 1.0 if got @ np.asarray(mount.rotation) >= 0 else -1.0
    dist = max(2.0 * np.abs(sign * got - mount.rotation).max(), np.abs(r["t_rig_accel"] - LEVER).max(), np.abs(r["bias"] - BIAS).max(),
               np.abs(r["gravity_world"] - GRAVITY).max(), abs(r["latency"] - LATENCY))
    print("distance to the truth", dist, "bound", 10 * REF_PROJECT, "rms", r["rms"], "iterations", r["iterations"], "lever arm", r["t_rig_accel"])
    assert dist <= 10 * REF_PROJECT
    # the bias goes where the sensor's model keeps it: VectorNav [scale 3, misalignment 6, bias 3]
    other = calico.Accelerometer()
    assert other.SetModel(calico.AccelerometerIntrinsicsModel.kAccelerometerVectorNav).ok()
    start = [1.0, 1, 1, 0, 0, 0, 0, 0, 0, 7, 7, 7]
    other.SetIntrinsics(start)
    T = calico.Pose3d()
    T.rotation = gyro.GetExtrinsics().rotation
    other.SetExtrinsics(T)
    assert other.SetLatency(gyro.GetLatency()).ok()
    assert other.AddMeasurements([m for m in measurements]).ok()      # (the accelerometer's: the loop's last)
    ro = calico.InitializeAccelerometer(trajectory, other)
    k = np.asarray(other.GetIntrinsics())
    assert np.array_equal(k[:9], start[:9]) and np.array_equal(k[9:], ro["bias"]) and np.abs(ro["bias"] - BIAS).max() <= 10 * REF_PROJECT
    assert np.array_equal(other.GetExtrinsics().translation, ro["t_rig_accel"])
