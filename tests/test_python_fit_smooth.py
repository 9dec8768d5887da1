"""Trajectory.FitSplineSmooth through `from calico_amd import calico`. On the CPU: option and weight errors as they reach Python.
On the GPU: the synthetic fixture's poses with a 1.5 s stretch removed (three times the support of an order-6 spline on 10 Hz
knots) -- Interpolate inside the gap is as close to the true poses as the long-double reference of the same penalised fit
(tests/fit_smooth_ref.py), where FitSpline on the same poses is not."""
from types import SimpleNamespace

import numpy as np
import pytest

import __graft_entry__ as _entry

_entry.build_hip()
_entry.build_python_module()   # no-ops when the in-tree libraries are up to date

import fit_smooth_ref as fs  # noqa: E402
from calico_amd import calico, synthetic as syn  # noqa: E402

GAP = (5.0, 6.5)


def _fixture():
    stamps, quats, trans = syn.default_synthetic_poses()
    poses = {}
    for t, q, p in zip(stamps, quats, trans):
        pose = calico.Pose3d()
        pose.rotation = [q[3], q[0], q[1], q[2]]
        pose.translation = p
        poses[float(t)] = pose
    return stamps, quats, trans, poses


def test_option_and_weight_errors_reach_python():
    _, _, _, poses = _fixture()
    trajectory = calico.Trajectory()
    with pytest.raises(TypeError, match="no spline fit option 'lamda_rot'"):
        trajectory.FitSplineSmooth(poses, options={"lamda_rot": 1e-3})
    with pytest.raises(ValueError, match="1 to 32 entries"):
        trajectory.FitSplineSmooth(poses, options={"lambda_rot": [1e-3] * 33})
    with pytest.raises(ValueError, match="one \\[rotation, position\\] pair per pose"):
        trajectory.FitSplineSmooth(poses, weights=[[1.0, 1.0, 1.0]] * len(poses))
    with pytest.raises(RuntimeError, match="Weights and time vectors are not the same size"):
        trajectory.FitSplineSmooth(poses, weights=[[1.0, 1.0]] * 3)
    # the library's own argument rules come before the device, with their message
    with pytest.raises(RuntimeError, match="calico_fit_spline_smooth: lambda_pos must be strictly ascending"):
        trajectory.FitSplineSmooth(poses, options={"lambda_rot": [1e-3, 1e-2], "lambda_pos": [1e-2, 1e-3]})
    with pytest.raises(RuntimeError, match="calico_fit_spline_smooth: derivative must be in \\[1, 3\\]"):
        trajectory.FitSplineSmooth(poses, options={"derivative": 4})


def _angle(q1, q2):
    return 2.0 * np.arccos(np.clip(np.abs((q1 * q2).sum(-1)), 0.0, 1.0))


@pytest.mark.gpu
def test_smoothing_fit_carries_the_trajectory_across_a_gap():
    stamps, quats, trans, poses = _fixture()
    gap = (stamps >= GAP[0]) & (stamps < GAP[1])
    assert gap.sum() == 20
    kept = {t: p for t, p in poses.items() if not GAP[0] <= t < GAP[1]}
    # the reference: the same penalised fit (defaults: m 2, relative lambda 1e-3, no weights) in long double
    c = SimpleNamespace(name="fixture-gap", order=6, stamps=np.ascontiguousarray(stamps[~gap]))
    c.knots = syn.knot_vector(c.stamps[0], c.stamps[-1], 6, 10.0)
    c.basis = np.ascontiguousarray(syn.basis_matrices(c.knots, 6))
    c.n_ctrl = len(c.knots) - 6
    c.data = np.concatenate([syn.unwrap_phase_log_map(syn.quat_to_axis_angle(quats[~gap])), trans[~gap]], 1)
    p = fs.build(c, np.ones((len(c.stamps), 2)), 2, (1e-3,), (1e-3,))
    C_ref = np.hstack([p.sys[0, 0].C_ref, p.sys[1, 0].C_ref])
    ref = syn.spline_eval(c.knots, c.basis, C_ref, 6, stamps[gap])
    ref_rot = _angle(np.array([syn.quat_from_axis_angle(v) for v in ref[:, :3]]), quats[gap]).max()
    ref_pos = np.abs(ref[:, 3:] - trans[gap]).max()
    # a B-spline's weights are non-negative and sum to 1: a value moves by no more than its control points (rotation: per axis)
    tol = max(fs.forward_bound(p.sys[g, 0].cond, p.sys[g, 0].C_ref, c.data) for g in range(2))

    def distance(trajectory):
        got = trajectory.Interpolate([float(t) for t in stamps[gap]])
        q = np.array([[g.rotation[1], g.rotation[2], g.rotation[3], g.rotation[0]] for g in got])
        return _angle(q, quats[gap]).max(), np.abs(np.array([g.translation for g in got]) - trans[gap]).max()
    smooth = calico.Trajectory()
    found = smooth.FitSplineSmooth(kept)
    assert found["status"] == (0, 0) and found["chosen"] == (0, 0) and found["n_used"] == (220, 220)
    assert [len(rows) for rows in found["rows"]] == [1, 1] and all(rows[0]["replaced_pivots"] == 0 for rows in found["rows"])
    rot, pos = distance(smooth)
    print("in the gap: smoothing fit %.3e rad %.3e m, reference %.3e rad %.3e m (tolerance %.1e)" % (rot, pos, ref_rot, ref_pos, tol))
    assert rot <= ref_rot + 4.0 * tol and pos <= ref_pos + tol
    plain = calico.Trajectory()
    plain.FitSpline(kept)
    rot, pos = distance(plain)
    print("in the gap: plain fit %.3e rad %.3e m" % (rot, pos))
    assert rot > ref_rot + 4.0 * tol and pos > ref_pos + tol and pos > 0.5
    # a grid with a target, through the dict
    found = smooth.FitSplineSmooth(kept, options={"lambda_rot": [1e-6, 1e-3, 1.0], "lambda_pos": [1e-6, 1e-3, 1.0], "target_rms_pos": 1e3})
    assert [len(rows) for rows in found["rows"]] == [3, 3] and found["chosen"] == (0, 2) and found["status"] == (0, 0)
