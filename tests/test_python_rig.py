"""Rig calibration from Python: calico.CalibrateRig, CameraModel.CalibrateRigFromChart and utils.InitializeRig. Without a GPU:
the names are there, the facade's and the library's argument errors reach Python, and a call without views changes nothing. On
the GPU: the standard rig fixture's detections through InitializeRig -- the extrinsics of cameras 1 and 2 are set to what the C
ABI gives for the same views, bit for bit, the reference camera keeps what it had, and the returned chart poses feed
Trajectory.FitSpline."""
import numpy as np
import pytest

import __graft_entry__ as _entry

_entry.build_hip()
_entry.build_python_module()   # no-ops when the in-tree libraries are up to date

import resect_ref as rr  # noqa: E402
import rig_ref as gr  # noqa: E402
from calico_amd import _capi, calico, synthetic as syn  # noqa: E402


def _cameras(rig):
    cams = []
    for model, k in zip(rig.models, rig.ks):
        c = calico.Camera()
        assert c.SetModel(calico.CameraIntrinsicsModel(model)).ok()
        c.SetIntrinsics(k)
        cams.append(c)
    return cams


def _detections(rig):
    """(rig_frames, model_definition) of a fixture whose views all hold the whole planar chart."""
    rig_frames = [{} for _ in range(rig.n_frames)]
    for v, (c, f) in enumerate(zip(rig.view_camera, rig.view_frame)):
        px = rig.pixels[rig.view_offsets[v]:rig.view_offsets[v + 1]]
        rig_frames[f][int(c)] = {i: p for i, p in enumerate(px)}
    return rig_frames, {i: p for i, p in enumerate(syn.planar_points())}


def test_python_surfaces_expose_the_new_names_and_their_errors():
    assert callable(calico.CalibrateRig) and callable(calico.InitializeRig) and hasattr(calico.CameraModel, "CalibrateRigFromChart")
    bare = calico.Camera()
    with pytest.raises(RuntimeError, match="Error: Camera model has not been set"):
        calico.CalibrateRig([bare], [], {})
    rig = gr.standard(0.0)
    cams = _cameras(rig)
    with pytest.raises(RuntimeError, match="names camera 3"):
        calico.CalibrateRig(cams, [{3: {0: np.zeros(2)}}], {0: np.zeros(3)})
    with pytest.raises(RuntimeError, match="not in the model definition"):
        calico.CalibrateRig(cams, [{1: {5: np.zeros(2)}}], {0: np.zeros(3)})
    with pytest.raises(TypeError):
        calico.CalibrateRig(cams, [], {}, options={"no_such_option": 1})
    with pytest.raises(RuntimeError, match="calico_rig_calibrate: min_shared_frames"):      # the library's rule, reached without a device
        calico.CalibrateRig(cams, [], {}, options={"min_shared_frames": 0})
    out = calico.CalibrateRig(cams, [{}, {}], {}, covariance=True)      # no views: OK, TOO_FEW_VIEWS
    assert out["status"] == _capi.RIG_TOO_FEW_VIEWS and out["q_frame"].shape == (2, 4) and out["cov"].shape == (18, 18)
    assert out["camera_status"].tolist() == [1, 2, 2] and out["view_status"].shape == (0,)
    before = [c.GetExtrinsics().translation for c in cams]
    with pytest.raises(RuntimeError, match="the rig calibration ended with status 1"):
        calico.InitializeRig(cams, [{}, {}], {})
    assert all(np.array_equal(c.GetExtrinsics().translation, b) for c, b in zip(cams, before))
    raw = calico.CameraModel.CalibrateRigFromChart([calico.CameraIntrinsicsModel.kOpenCv5], [rig.ks[0]], 0, [], [], [0], np.zeros((0, 2)),
                                                   np.zeros((0, 3)))
    assert raw["status"] == _capi.RIG_TOO_FEW_VIEWS and raw["q_rig_camera"].tolist() == [[0, 0, 0, 1]]


@pytest.mark.gpu
def test_initialize_rig_sets_the_extrinsics_and_its_poses_feed_fit_spline():
    rig = gr.standard(0.1)
    cams = _cameras(rig)
    held = calico.Pose3d()
    held.rotation = [1.0, 0.0, 0.0, 0.0]
    held.translation = [0.0, 0.0, 0.0]
    cams[0].SetExtrinsics(held)
    rig_frames, model_definition = _detections(rig)
    R_chart_rig, t_chart_rig, ok = calico.InitializeRig(cams, rig_frames, model_definition)
    assert ok.all() and len(R_chart_rig) == len(t_chart_rig) == 20
    # the same views as arrays (the pybind module's own call: one HIP runtime in this process)
    direct = calico.CameraModel.CalibrateRigFromChart([calico.CameraIntrinsicsModel(m) for m in rig.models], rig.ks, rig.n_frames,
                                                      rig.view_camera.tolist(), rig.view_frame.tolist(), rig.view_offsets.tolist(),
                                                      rig.pixels, rig.points)
    assert direct["status"] == _capi.RIG_OK and direct["views_used"] == 60 and direct["pairs_used"] == 2160
    for c in (1, 2):
        T = cams[c].GetExtrinsics()
        x, y, z, w = direct["q_rig_camera"][c]
        assert np.array_equal(T.rotation, [w, x, y, z]) and np.array_equal(T.translation, direct["t_rig_camera"][c])
        assert rr.pose_distance(rr.rot([*T.rotation[1:], T.rotation[0]]), np.asarray(T.translation), *rig.cams[c]) < 2e-3      # (0.1 px noise)
    assert np.array_equal(cams[0].GetExtrinsics().translation, [0, 0, 0]) and np.array_equal(cams[0].GetExtrinsics().rotation, [1, 0, 0, 0])
    for f in (0, 7, 19):      # InitializePoses' convention: the inverse of T_rig_chart
        R = rr.rot(direct["q_frame"][f])
        assert np.abs(R_chart_rig[f] - R.T).max() <= 1e-15 and np.abs(t_chart_rig[f] + R.T @ direct["t_frame"][f]).max() <= 1e-14
    stamps, _, _ = syn.default_synthetic_poses()
    poses = {}
    for t, R, p in zip(stamps[::12], R_chart_rig, t_chart_rig):
        T = calico.Pose3d()
        q = rr.quat_of(R)
        T.rotation = [q[3], q[0], q[1], q[2]]
        T.translation = p
        poses[float(t)] = T
    trajectory = calico.Trajectory()
    trajectory.FitSpline(poses, knot_frequency=0.25)      # (raises on error; twenty poses over 18 s: a coarse spline)
    back = trajectory.Interpolate([float(stamps[::12][7])])[0]
    assert np.isfinite(np.asarray(back.translation)).all()
