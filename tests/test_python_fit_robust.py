"""Trajectory.FitSplineRobust through `from calico_amd import calico`. On the CPU: option and weight errors as they reach Python.
On the GPU: the synthetic fixture's poses with seeded noise (0.01 rad per axis, 0.005 m: without noise the median residual, and
with it the scale, is the spline's approximation error, and Huber at a vanishing scale is an L1 fit that IRLS approaches slowly)
and a tenth turned by 0.5 rad -- the per-pose robust weights single out the turned poses, Interpolate stays within a tenth of the turn of the
true rotations where FitSplineSmooth's is off by more than a fifth of it, and with max_iterations 0 the trajectory is
FitSplineSmooth's."""
import numpy as np
import pytest

import __graft_entry__ as _entry

_entry.build_hip()
_entry.build_python_module()   # no-ops when the in-tree libraries are up to date

from calico_amd import calico, synthetic as syn  # noqa: E402


SIGMA_ROT = 0.01      # rad per axis
KNOT_HZ = 3.0         # 4.5 poses per segment: at the default 10 Hz the fixture has 1.3, and a spline that can follow every pose has no outliers


def _quat_mul(a, b):
    """Hamilton product of quaternions (x, y, z, w)."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def _fixture(turned=()):
    stamps, quats, trans = syn.default_synthetic_poses()
    turn = np.array([np.sin(0.25), 0.0, 0.0, np.cos(0.25)])      # 0.5 rad about the sensor rig's x
    rng = np.random.default_rng(17)
    wobble, shift = SIGMA_ROT * rng.standard_normal((len(stamps), 3)), 0.005 * rng.standard_normal((len(stamps), 3))
    poses = {}
    for i, (t, q, p) in enumerate(zip(stamps, quats, trans)):
        if turned:
            q, p = _quat_mul(q, np.append(0.5 * wobble[i], 1.0)), p + shift[i]
            q = q / np.linalg.norm(q)
        if i in turned:
            q = _quat_mul(q, turn)
        pose = calico.Pose3d()
        pose.rotation = [q[3], q[0], q[1], q[2]]
        pose.translation = p
        poses[float(t)] = pose
    return stamps, quats, trans, poses


def test_option_and_weight_errors_reach_python():
    _, _, _, poses = _fixture()
    trajectory = calico.Trajectory()
    with pytest.raises(TypeError, match="no robust spline fit option 'tunning_rot'"):
        trajectory.FitSplineRobust(poses, robust={"tunning_rot": 2.0})
    with pytest.raises(TypeError, match="no spline fit option 'lamda_rot'"):
        trajectory.FitSplineRobust(poses, options={"lamda_rot": 1e-3})
    with pytest.raises(ValueError, match="loss must be 'huber' or 'tukey'"):
        trajectory.FitSplineRobust(poses, robust={"loss": "cauchy"})
    with pytest.raises(ValueError, match="one \\[rotation, position\\] pair per pose"):
        trajectory.FitSplineRobust(poses, weights=[[1.0, 1.0, 1.0]] * len(poses))
    with pytest.raises(RuntimeError, match="Weights and time vectors are not the same size"):
        trajectory.FitSplineRobust(poses, weights=[[1.0, 1.0]] * 3)
    # the library's own argument rules come before the device, with their message
    with pytest.raises(RuntimeError, match="calico_fit_spline_robust: n_lambda must be 1"):
        trajectory.FitSplineRobust(poses, options={"lambda_rot": [1e-3, 1e-2], "lambda_pos": [1e-3, 1e-2]})
    with pytest.raises(RuntimeError, match="calico_fit_spline_robust: max_iterations must be in \\[0, 64\\]"):
        trajectory.FitSplineRobust(poses, robust={"max_iterations": 65})
    with pytest.raises(RuntimeError, match="calico_fit_spline_robust: unknown loss 7"):
        trajectory.FitSplineRobust(poses, robust={"loss": 7})
    with pytest.raises(RuntimeError, match="calico_fit_spline_robust: scale_pos must be finite and >= 0"):
        trajectory.FitSplineRobust(poses, robust={"scale_pos": -1.0})


def _angle(q1, q2):
    return 2.0 * np.arccos(np.clip(np.abs((q1 * q2).sum(-1)), 0.0, 1.0))


@pytest.mark.gpu
@pytest.mark.parametrize("loss", ["huber", "tukey"])
def test_robust_fit_singles_out_the_turned_poses(loss):
    n = len(syn.default_synthetic_poses()[0])
    turned = np.arange(14, n - 10, 10)
    stamps, quats, trans, poses = _fixture(set(turned.tolist()))
    others = np.setdiff1d(np.arange(n), turned)
    robust = calico.Trajectory()
    found = robust.FitSplineRobust(poses, KNOT_HZ, robust={"loss": loss})
    u, e = np.array(found["robust_weights"]), np.array(found["residuals"])
    assert u.shape == (n, 2) and e.shape == (n, 2) and found["n_used"] == (n, n) and found["iterations"][0] > 0
    print("%s: rotation weights of the turned poses <= %.3e, of the others >= %.3e (%d at 0); status %s after %s iterations" % (
        loss, u[turned, 0].max(), u[others, 0].min(), (u[others, 0] == 0).sum(), found["status"], found["iterations"]))
    assert (e[turned, 0] > 0.4).all() and u[turned, 1].min() > u[turned, 0].max()      # (their positions are as good as anyone's)
    if loss == "huber":      # the weight falls with the residual norm: singled out = each below every other pose's, and small
        assert u[turned, 0].max() < u[others, 0].min() and u[turned, 0].max() <= 0.1
    else:                    # rejected, every one; Tukey also rejects a pose or two of the noise's tail (at most one in twenty here)
        assert (u[turned, 0] == 0).all() and len(turned) <= found["n_rejected"][0] <= len(turned) + len(others) // 20

    def distance(trajectory):
        got = trajectory.Interpolate([float(t) for t in stamps])
        q = np.array([[g.rotation[1], g.rotation[2], g.rotation[3], g.rotation[0]] for g in got])
        return _angle(q, quats).max()
    smooth = calico.Trajectory()
    smooth.FitSplineSmooth(poses, KNOT_HZ)
    d_robust, d_smooth = distance(robust), distance(smooth)
    print("%s: largest rotation error along the trajectory %.3e rad, smoothing fit %.3e rad" % (loss, d_robust, d_smooth))
    assert d_robust <= 0.05 and d_smooth > 0.1      # (a tenth of the turn, 5 sigma of the noise; more than a fifth of the turn)
    # max_iterations 0: the smoothing fit's trajectory
    zero = calico.Trajectory()
    none = zero.FitSplineRobust(poses, KNOT_HZ, robust={"loss": loss, "max_iterations": 0})
    assert none["iterations"] == (0, 0) and none["status"] == (0, 0) and (np.array(none["robust_weights"]) == 1).all()
    a, b = zero.Interpolate([float(t) for t in stamps]), smooth.Interpolate([float(t) for t in stamps])
    assert all(list(x.rotation) == list(y.rotation) and list(x.translation) == list(y.translation) for x, y in zip(a, b))
