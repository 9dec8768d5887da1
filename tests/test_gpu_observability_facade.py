"""BatchOptimizer.AnalyzeObservability() of the pybind module (the C++ facade's calico::Observability underneath) on a stereo
rig with VectorNav IMUs: the full 3x3 matrix of each IMU and its free mounting rotation describe the same rotation of the
measurement, so three directions per IMU are undetermined -- the problem ComputeCovariance refuses. The report counts
them and names the blocks they live in."""
import numpy as np
import pytest

from calico_amd import synthetic as syn

pytestmark = pytest.mark.gpu


def test_python_facade_observability(hip):
    # (imported here, behind the `hip` fixture: PyTorch's HIP runtime is loaded before the module's, as conftest.py arranges)
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

    def pose(axis, angle_deg, t):
        axis = np.asarray(axis, float) / np.linalg.norm(axis)
        half = 0.5 * np.deg2rad(angle_deg)
        p = calico.Pose3d()
        p.rotation = [np.cos(half), *(np.sin(half) * axis)]
        p.translation = t
        return p

    true_cam = np.array([785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2])
    true_imu = np.array([1.01, 0.99, 1.02, 1e-3, -2e-3, 1.5e-3, -1e-3, 2e-3, 1e-3, 0.01, -0.01, 0.01])
    specs = [("left", calico.Camera, calico.CameraIntrinsicsModel.kOpenCv5, true_cam, calico.Pose3d(), 0.0),
             ("right", calico.Camera, calico.CameraIntrinsicsModel.kOpenCv5, true_cam,
              pose([0.68, -0.21, 0.57], 2.0, 0.05 * np.array([0.6, -0.33, 0.54])), 0.01),
             ("gyro", calico.Gyroscope, calico.GyroscopeIntrinsicsModel.kGyroscopeVectorNav, true_imu, pose([-0.44, 0.11, -0.05], 2.0, [0, 0, 0]), 0.02),
             ("acc", calico.Accelerometer, calico.AccelerometerIntrinsicsModel.kAccelerometerVectorNav, true_imu,
              pose([0.26, -0.27, 0.9], 2.0, [0.01, -0.02, 0.03]), 0.02)]
    optimizer = calico.BatchOptimizer()
    sensors = {}
    for name, cls, model, intrinsics, extrinsics, latency in specs:
        sensor = cls()
        sensor.SetName(name)
        assert sensor.SetModel(model).ok()
        sensor.SetIntrinsics(intrinsics)
        sensor.SetExtrinsics(extrinsics)
        assert sensor.SetLatency(latency).ok()
        measurements = sensor.Project(times, trajectory, world)
        assert len(measurements) > 0
        sensor.EnableIntrinsicsEstimation(True)
        sensor.EnableExtrinsicsEstimation(name != "left")
        sensor.EnableLatencyEstimation(name != "left")
        assert sensor.AddMeasurements(measurements).ok()
        optimizer.AddSensor(sensor)
        sensors[name] = sensor
    optimizer.AddTrajectory(trajectory)
    optimizer.AddWorldModel(world)
    with pytest.raises(RuntimeError, match="rank deficient"):      # the covariance cannot serve this rig
        optimizer.ComputeCovariance()
    obs = optimizer.AnalyzeObservability()
    lam = obs.Eigenvalues()
    assert obs.Dimension() == 8 + (8 + 6 + 1) + 2 * (12 + 6 + 1)
    assert obs.NumUnobserved() == 3                      # the gyroscope's lever arm
    assert len(lam) == obs.Dimension() - obs.NumUnobserved() and np.all(np.diff(lam) >= 0)
    print("facade: lowest eigenvalues", lam[:8], "sweeps", obs.Sweeps())
    assert obs.NumWeak() == 6
    assert lam[5] < 1e-10 < 1e-7 < lam[6]
    for i in range(6):
        d = obs.Describe(i)
        print("facade: direction %d: %s" % (i, ", ".join("%s %s %.3f" % e for e in d)))
        big = [e for e in d if e[2] > 1e-8]
        assert big and all(name in ("gyro", "acc") and part in ("intrinsics", "rotation") for name, part, _ in big)
        assert [e[2] for e in d] == sorted((e[2] for e in d), reverse=True)
        assert abs(sum(e[2] for e in d) - 1.0) <= 1e-8
        v, t = obs.Direction(i), obs.Direction(i, tangent_units=True)
        assert v.shape == t.shape == (obs.Dimension(),)
        assert abs(np.linalg.norm(v) - 1.0) <= 1e-12 and abs(np.linalg.norm(t) - 1.0) <= 1e-12
    assert obs.IntrinsicsShare(0, sensors["left"]) <= 1e-8
    with pytest.raises(Exception):
        obs.Direction(len(lam))
