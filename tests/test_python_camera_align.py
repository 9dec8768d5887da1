"""Trajectory.AlignCamera and utils.InitializeCamera through the Python surface. Without a GPU: the names, the option dict, the
library's argument errors as they reach Python. On the GPU (Trajectory.FitSpline runs there): a second camera mounted at 12
degrees, 13.7 ms late, all of it UNKNOWN at the start (identity, zero latency), sees a small chart; its measurements are the
facade's own Project() (the spline segment of the true time, where the alignment, as the optimiser, takes the stamp's).
InitializeCamera sets extrinsics and latency to the mounting within the distance of the two segment polynomials, which the test
computes on the same spline fitted in numpy; on NO_PEAK it raises and leaves the camera as it was."""
import numpy as np
import pytest

from calico_amd import calico, synthetic as syn

TRUE_CAM = np.array([785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2])
LATENCY = 0.0137
OPTIONS = {"max_lag": 0.05, "lag_step": 0.0025}


def _pose(axis, angle_deg, t=(0.0, 0.0, 0.0)):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    half = 0.5 * np.deg2rad(angle_deg)
    p = calico.Pose3d()
    p.rotation = [np.cos(half), *(np.sin(half) * axis)]
    p.translation = np.asarray(t, float)
    return p


def _poses(at_rest=False):
    """Gentle turns about all three axes (every 0.05 s over 7 s), looking along +z at a chart 2.2 m away."""
    t = 0.05 * np.arange(141)
    s = 0.0 if at_rest else 1.0
    phi = s * np.stack([0.2 * np.sin(1.3 * t), 0.15 * np.sin(0.9 * t + 1.0), 0.25 * np.sin(1.7 * t + 2.0)], 1)
    pos = s * np.stack([0.2 * np.sin(0.7 * t), 0.15 * np.cos(0.5 * t), 0.1 * np.sin(1.1 * t)], 1)
    return t, syn.quat_from_axis_angle(phi), pos


def _trajectory(at_rest=False):
    t, quats, pos = _poses(at_rest)
    poses = {}
    for ti, q, p in zip(t, quats, pos):
        T = calico.Pose3d()
        T.rotation = [q[3], q[0], q[1], q[2]]
        T.translation = p
        poses[float(ti)] = T
    trajectory = calico.Trajectory()
    trajectory.FitSpline(poses)
    return trajectory


def _world():
    chart = calico.RigidBody()
    g = 0.1 * (np.arange(5) - 2)
    chart.model_definition = {5 * i + j: [g[i], g[j], 0.0] for i in range(5) for j in range(5)}
    chart.T_world_rigidbody = _pose([0.6, 0.8, 0.0], np.rad2deg(0.1), [0.05, -0.1, 2.2])
    chart.world_pose_is_constant = True
    chart.model_definition_is_constant = True
    world = calico.WorldModel()
    world.AddRigidBody(chart)
    return world


def _camera(extrinsics=None, latency=0.0):
    cam = calico.Camera()
    assert cam.SetModel(calico.CameraIntrinsicsModel.kOpenCv5).ok()
    cam.SetIntrinsics(TRUE_CAM)
    if extrinsics is not None:
        cam.SetExtrinsics(extrinsics)
    assert cam.SetLatency(latency).ok()
    return cam


def test_python_surfaces_expose_the_new_names():
    assert hasattr(calico.Trajectory, "AlignCamera") and callable(calico.InitializeCamera)
    trajectory, world = calico.Trajectory(), _world()
    with pytest.raises(RuntimeError, match="model has not been set"):
        trajectory.AlignCamera(calico.Camera(), world)
    cam = _camera()
    with pytest.raises(RuntimeError, match="calico_camera_align: order"):      # (no spline yet: the library's own argument rule)
        trajectory.AlignCamera(cam, world)
    with pytest.raises(TypeError, match="no camera alignment option"):
        trajectory.AlignCamera(cam, world, options={"no_such_option": 1})
    with pytest.raises(RuntimeError, match="no rigid body with id 5"):
        trajectory.AlignCamera(cam, world, model_id=5)
    with pytest.raises(RuntimeError, match="Error: calico_camera_align"):
        calico.InitializeCamera(trajectory, cam, world)


def _segment_distance(times):
    """The largest distance of the polynomials of the true time's and of the stamp's segment, at the true time, over the frames
    whose latency crosses a knot (the spline of the facade's fit, fitted here in numpy)."""
    t, quats, pos = _poses()
    knots, basis, ctrl = syn.fit_trajectory(t, quats, pos, 10.0, 6)
    a, b = syn.spline_index(knots, 6, times), syn.spline_index(knots, 6, times + LATENCY)
    cross = a != b
    assert cross.any()
    pa = syn.spline_eval(knots, basis, ctrl, 6, times[cross], 0, a[cross])
    pb = syn.spline_eval(knots, basis, ctrl, 6, times[cross], 0, b[cross])
    return float(np.abs(pa - pb).max())


@pytest.mark.gpu
def test_initialize_camera_sets_extrinsics_and_latency():
    trajectory, world = _trajectory(), _world()
    mount = _pose([2.0, -1.0, 2.0], 12.0, [0.08, -0.05, 0.03])
    times = 0.3 + 0.0517 * np.arange(128) + 0.0071      # (none of them a stamp of the poses; some of them 14 ms before a knot)
    measurements = _camera(mount, LATENCY).Project([float(t) for t in times], trajectory, world)
    assert len(measurements) == 128 * 25
    cam = _camera()
    assert cam.AddMeasurements(measurements).ok()
    with pytest.raises(RuntimeError, match="sigma_pixel"):
        trajectory.AlignCamera(cam, world, options={"sigma_pixel": 0.0})
    r = calico.InitializeCamera(trajectory, cam, world, options=OPTIONS)
    bound = _segment_distance(times)
    x, y, z, w = r["q_rig_camera"]
    got = cam.GetExtrinsics()
    print("aligned: latency", r["latency"], "rotation", r["q_rig_camera"], "translation", r["t_rig_camera"], "rms", r["rms"], "iterations",
          r["iterations"], "the segment polynomials differ by", bound)
    assert r["status"] == 0 and r["frames_used"] == 128 and r["pairs_used"] == 128 * 25 and r["n_lags"] == 41
    assert list(r["image_ids"]) == list(range(128)) and np.allclose(r["stamps"], times + LATENCY, rtol=0, atol=1e-15)
    # the camera carries the estimates
    assert np.allclose(got.rotation, [w, x, y, z], rtol=0, atol=1e-15) and np.array_equal(got.translation, r["t_rig_camera"])
    assert cam.GetLatency() == r["latency"]
    # they are the mounting, within the distance of the two polynomials (1e-10: the refinement's own tolerance)
    assert 0.0 < bound < 1e-6
    assert np.abs(got.rotation - mount.rotation).max() <= bound + 1e-10 and np.abs(got.translation - mount.translation).max() <= bound + 1e-10
    assert abs(r["latency"] - LATENCY) <= bound + 1e-10
    r2 = trajectory.AlignCamera(cam, world, options=OPTIONS, covariance=True, curve=True)
    assert r2["cov"].shape == (7, 7) and r2["curve"].shape == (41,) and np.array_equal(r2["q_rig_camera"], r["q_rig_camera"])


@pytest.mark.gpu
def test_initialize_camera_raises_on_no_peak_and_leaves_the_camera():
    world = _world()
    trajectory = _trajectory(at_rest=True)
    mount = _pose([2.0, -1.0, 2.0], 12.0, [0.08, -0.05, 0.03])
    measurements = _camera(mount, LATENCY).Project([float(t) for t in 0.3 + 0.05 * np.arange(64)], trajectory, world)
    start = _pose([0.0, 0.0, 1.0], 3.0, [0.01, 0.02, 0.03])
    cam = _camera(start, 0.004)
    assert cam.AddMeasurements(measurements).ok()
    with pytest.raises(RuntimeError, match="Error: the camera alignment ended with status 2"):
        calico.InitializeCamera(trajectory, cam, world, options=OPTIONS)
    got = cam.GetExtrinsics()
    assert np.array_equal(got.rotation, start.rotation) and np.array_equal(got.translation, start.translation) and cam.GetLatency() == 0.004
    few = _camera()
    assert few.AddMeasurements(measurements[:5 * 25]).ok()
    with pytest.raises(RuntimeError, match="Error: the camera alignment ended with status 1"):
        calico.InitializeCamera(trajectory, few, world)
