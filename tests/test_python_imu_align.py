"""Trajectory.AlignImu and utils.InitializeImu through the Python surface. Without a GPU: the names, the option dict, the library's
argument errors as they reach Python. On the GPU (Trajectory.FitSpline runs there): the toy stereo-camera-and-IMU problem of test_python_api.py with both IMU sensors mounted at 40 degrees,
a latency of 13.7 ms and biases, all of it UNKNOWN at the start (identity, zero latency, zero bias) -- InitializeImu sets the
sensors and the world's gravity (the bias where the sensor's model keeps it: ScaleAndBias, VectorNav, none for ScaleOnly), and
Optimize from there recovers every parameter. This problem lies inside the alignment's model, so Optimize starts at its minimum:
the test is about the facade and the setters. The solve from an aligned start that has work left to do --
helpers.small_scene(imu=True), IMU scale 1.3, the accelerometer rotated against the gyroscope, noise -- is
test_gpu_imu_align.py::test_optimize_from_the_aligned_start_reaches_the_small_scenes_minimum."""
import numpy as np
import pytest

from calico_amd import calico, synthetic as syn


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
    assert hasattr(calico.Trajectory, "AlignImu") and callable(calico.InitializeImu)
    trajectory, gyro = calico.Trajectory(), calico.Gyroscope()
    with pytest.raises(RuntimeError, match="calico_imu_align: order"):      # (no spline yet: the library's own argument rule)
        trajectory.AlignImu(gyro)
    with pytest.raises(TypeError, match="no IMU alignment option"):
        trajectory.AlignImu(gyro, options={"no_such_option": 1})
    with pytest.raises(RuntimeError, match="IMU model 0"):      # (no model set: refused before anything is changed)
        calico.InitializeImu(trajectory, gyro)
    assert gyro.SetModel(calico.GyroscopeIntrinsicsModel.kGyroscopeScaleAndBias).ok()
    with pytest.raises(RuntimeError, match="Error: calico_imu_align"):
        calico.InitializeImu(trajectory, gyro)


@pytest.mark.gpu
def test_too_few_samples_and_option_errors_on_a_fitted_trajectory():
    times, trajectory = _trajectory()      # (FitSpline runs on the device)
    gyro = calico.Gyroscope()
    assert gyro.SetModel(calico.GyroscopeIntrinsicsModel.kGyroscopeScaleAndBias).ok()
    with pytest.raises(RuntimeError, match="lag_step"):
        trajectory.AlignImu(gyro, options={"lag_step": 0.0})
    r = trajectory.AlignImu(gyro, covariance=True, curve=True)      # no measurements: OK with TOO_FEW_SAMPLES
    assert r["gyro_status"] == 1 and r["gyro_samples"] == 0 and r["cov"].shape == (7, 7) and r["curve"].shape == (0,)
    assert r["q_rig_gyro"].tolist() == [0, 0, 0, 1]
    with pytest.raises(RuntimeError, match="Error: the gyroscope alignment ended with status 1"):
        calico.InitializeImu(trajectory, gyro)


@pytest.mark.gpu
def test_initialize_imu_sets_the_sensors_and_optimize_converges_from_there():
    times, trajectory = _trajectory()
    chart = calico.RigidBody()
    chart.model_definition = {i: p for i, p in enumerate(syn.planar_points())}
    chart.world_pose_is_constant = True
    chart.model_definition_is_constant = True
    world_true, world = calico.WorldModel(), calico.WorldModel()
    world.AddRigidBody(chart)
    world_true.AddRigidBody(chart)
    gravity = np.array([0.3, -9.7, 0.9])
    world_true.SetGravity(list(gravity))
    mount = _pose([1.0, -2.0, 2.0], 40.0)
    true_cam = np.array([785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2])
    specs = [("left", calico.Camera, calico.CameraIntrinsicsModel.kOpenCv5, true_cam, calico.Pose3d(), 0.0),
             ("gyro", calico.Gyroscope, calico.GyroscopeIntrinsicsModel.kGyroscopeScaleAndBias, np.array([1.0, 0.01, -0.02, 0.015]), mount, 0.0137),
             ("acc", calico.Accelerometer, calico.AccelerometerIntrinsicsModel.kAccelerometerScaleAndBias, np.array([1.0, 0.05, -0.03, 0.02]), mount, 0.0137)]
    optimizer, sensors = calico.BatchOptimizer(), {}
    for name, cls, model, intrinsics, extrinsics, latency in specs:
        true_sensor = cls()
        assert true_sensor.SetModel(model).ok()
        true_sensor.SetIntrinsics(intrinsics)
        true_sensor.SetExtrinsics(extrinsics)
        assert true_sensor.SetLatency(latency).ok()
        measurements = true_sensor.Project(times, trajectory, world_true)
        sensor = cls()
        sensor.SetName(name)
        assert sensor.SetModel(model).ok()
        if cls is calico.Camera:
            sensor.SetIntrinsics(intrinsics)
        else:
            sensor.SetIntrinsics([1.0, 0.0, 0.0, 0.0])      # nothing known about the IMU but its unit scale
            sensor.EnableIntrinsicsEstimation(True)
            sensor.EnableExtrinsicsEstimation(True)
            sensor.EnableLatencyEstimation(True)
        assert sensor.AddMeasurements(measurements).ok()
        if name == "gyro":
            gyro_measurements = measurements
        optimizer.AddSensor(sensor)
        sensors[name] = sensor
    gyro, acc = sensors["gyro"], sensors["acc"]
    r = calico.InitializeImu(trajectory, gyro, acc, world, options={"max_lag": 0.05, "lag_step": 0.0025})
    assert r["gyro_status"] == 0 and r["accel_status"] == 0 and r["gyro_samples"] > 200
    print("aligned: latency", r["latency"], "rotation", r["q_rig_gyro"], "gravity", r["gravity_world"], "rms", r["gyro_rms"], r["accel_rms"])
    # the sensors and the world model carry the estimates
    x, y, z, w = r["q_rig_gyro"]
    for sensor, bias in ((gyro, r["gyro_bias"]), (acc, r["accel_bias"])):
        assert np.allclose(sensor.GetExtrinsics().rotation, [w, x, y, z], rtol=0, atol=1e-15) and sensor.GetLatency() == r["latency"]
        assert np.array_equal(sensor.GetIntrinsics(), np.concatenate([[1.0], bias]))
    assert np.array_equal(np.asarray(world.GetGravity()), r["gravity_world"])
    # they are the truth (measured: the latency to 3e-16 s, gyroscope rms 4e-15; Project()'s data are the model's to rounding here)
    assert np.abs(gyro.GetExtrinsics().rotation - mount.rotation).max() < 1e-8 and abs(r["latency"] - 0.0137) < 1e-8
    assert np.abs(r["gravity_world"] - gravity).max() < 1e-7
    # the bias goes where the sensor's model keeps it: VectorNav [scale 3, misalignment 6, bias 3]; ScaleOnly has none
    measurements = [m for m in gyro_measurements]
    for model, start in ((calico.GyroscopeIntrinsicsModel.kGyroscopeVectorNav, [1.0, 1, 1, 0, 0, 0, 0, 0, 0, 7, 7, 7]),
                         (calico.GyroscopeIntrinsicsModel.kGyroscopeScaleOnly, [1.0])):
        other = calico.Gyroscope()
        assert other.SetModel(model).ok()
        other.SetIntrinsics(start)
        assert other.AddMeasurements(measurements).ok()
        ro = calico.InitializeImu(trajectory, other, options={"max_lag": 0.05, "lag_step": 0.0025})
        k = np.asarray(other.GetIntrinsics())
        assert np.array_equal(ro["gyro_bias"], r["gyro_bias"]) and other.GetLatency() == r["latency"]
        assert np.array_equal(k[:9], start[:9]) and (len(k) == 1 or np.array_equal(k[9:], r["gyro_bias"]))
    optimizer.AddTrajectory(trajectory)
    optimizer.AddWorldModel(world)
    options = calico.DefaultSolverOptions()
    options.minimizer_progress_to_stdout = False
    options.max_num_iterations = 100
    summary = optimizer.Optimize(options)
    print("final cost", summary.final_cost)
    assert summary.IsSolutionUsable() and summary.final_cost < 1e-7      # (measured 5.6e-20)
    for sensor, k in ((gyro, specs[1][3]), (acc, specs[2][3])):
        got = sensor.GetExtrinsics().rotation
        assert min(np.abs(got - mount.rotation).max(), np.abs(got + mount.rotation).max()) < 1e-7
        assert abs(sensor.GetLatency() - 0.0137) < 1e-7
        np.testing.assert_allclose(sensor.GetIntrinsics(), k, rtol=0, atol=1e-7)
