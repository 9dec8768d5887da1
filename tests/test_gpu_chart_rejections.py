"""Pairs the camera model rejects, on the device (calico_camera_resect, calico_camera_calibrate, calico_rig_calibrate) against the
references' loops (lm_rule_ref.py). One construction for the three estimators, resect_ref.boundary_case: the unified model at
alpha = 0.7, whose pixel stays finite at its validity boundary z = -w d, and ONE extra chart point off the plane near that
boundary in one frame (resection: the frame; calibration: frame 5 of 20, alpha held; rig: camera 0's view of frame 5). The
properties of the cases are asserted from the reference alone in tests/test_resect_host.py, tests/test_calib_host.py and
tests/test_rig_host.py (test_boundary_*).

Which test reaches which code (continues the table of tests/test_gpu_chart_steps.py):

  `lost`: a candidate that loses a pair that was valid is rejected       test_resect_lost, test_calib_lost, test_rig_lost
  for ALL frames; the `ok == false` lane of the candidate's pass;        (max_iterations = 1: the start comes back, lambda = 1e-3;
  pose_bit: the pair's two validity bits swap roles on acceptance        k up to one past the first accepted step: the reference's)
  a pair that is invalid at every point: `ok == false` in every pass,    test_resect_invalid, test_calib_invalid, test_rig_invalid
  n_used = n - 1, rms and costs over the valid pairs
  `common`: the costs compared are over the pairs valid at both          test_resect_joins, test_calib_joins, test_rig_joins
  points; a pair that becomes valid joins after acceptance
  a frame with no valid pair at the start: CALICO_RESECT_DEGENERATE;     test_resect_frame_without_a_valid_pair,
  its 6x6 block is not positive definite and it drops out:               test_calib_frame_without_a_valid_pair,
  CALICO_RESECT_NOT_POSITIVE_DEFINITE,                                   test_rig_frame_without_a_valid_pair
  CALICO_RIG_FRAME_NOT_POSITIVE_DEFINITE; no frame with a valid pair:
  *_DEGENERATE with the outputs equal to the starts

Bounds: as tests/test_gpu_chart_steps.py -- the point kept after k steps within max(10 floors, ROUNDING) of the reference's,
floor = the reference's k-step point from h = 2e-6 against h = 1e-6 differences, lambda exactly, costs to 1e-9 relative; the
optimality criterion of tests/test_gpu_resect.py, test_gpu_calib.py and test_gpu_rig.py where a call runs to convergence.

Measured on an MI355X (floor / the device's distance to the reference's k-step point; every lambda equal to the reference's):
  lost     resect: five rejections (the device's pose 7.9e-18 from the start), step 6 accepted 5.7e-14 / 2.4e-14, step 7 rejected
           calib:  four rejections (lambda 1e-3 .. 1, 6.2e-18 from the start, costs equal), step 5 accepted 1.1e-12 / 8.8e-13
           rig:    five rejections (lambda 1e-3 .. 10, 8.0e-17 from the start), step 6 accepted 2.1e-13 / 1.5e-13. The first run
                   had final_cost = 73242.25082406186 against initial_cost = 73242.25082406188 on the rejected steps: fixed
                   (tests/test_gpu_chart_steps.py says how)
  invalid  the reference's step at the device's estimate: resect 3.7e-14, calib 3.4e-13, rig 3.7e-14; n_used = n - 1
  joins    resect 1.5e-12 / 1.1e-12; calib 5.3e-12 / 4.0e-12, cost 1537.7 -> 10042.8; rig 2.1e-12 / 1.5e-12, cost 72914 -> 90089
  a frame without a valid pair: calib with and without it 8.7e-16 (intrinsics), 1.2e-15 (poses), the reference's step 9.6e-13;
           rig: the reference's step over the views in use 5.7e-14
"""
import numpy as np
import pytest

import calib_ref as cr
import lm_rule_ref as lm
import resect_ref as rr
import rig_ref as gr
from calico_amd import _capi

pytestmark = pytest.mark.gpu

ROUNDING = 1e-14      # (tests/test_gpu_chart_steps.py says why)


@pytest.fixture(scope="module")
def api(hip):
    return hip


def _close(a, b, rel=1e-9):
    return abs(a - b) <= rel * abs(b)


def _quat(R):
    q = rr.quat_of(R)
    return q if q[3] >= 0 else -q


def _is_start(q, t, q0, t0):
    """The pose is the start: the quaternion within 1e-15 of the normalised one, the translation bit for bit."""
    q0 = np.asarray(q0, float)
    return bool(np.abs(q - q0 / np.linalg.norm(q0)).max() <= 1e-15 and np.asarray(t).tobytes() == np.asarray(t0, float).tobytes())


# ---------------------------------------------------------------------------------------------------------------- resection


def _resect(api, c, **kw):
    return _capi.camera_resect(api, 6, c.k, [0, len(c.points)], c.pixels, c.points, q_init=_quat(c.start[0])[None], t_init=c.start[1][None],
                               options=_capi.resection_options(api, **kw) if kw else None)


def test_resect_lost(api):
    c = rr.boundary_case("lost")
    a = lm.resect_loop(6, c.k, *c.start, c.points, c.pixels, 8)
    b = lm.resect_loop(6, c.k, *c.start, c.points, c.pixels, 8, h=2e-6)
    first = a.log.index(True) + 1
    assert a.log == b.log and first >= 4
    q0 = _quat(c.start[0])
    for k in range(1, first + 2):
        r = _resect(api, c, max_iterations=k)
        point = a.trace[k - 1][0]
        floor = rr.pose_distance(*point, *b.trace[k - 1][0])
        dist = rr.pose_distance(rr.rot(r.q[0]), r.t[0], *point)
        print("resect lost k", k, "accepted", a.log[:k], "floor", floor, "device", dist, "rms", r.rms[0])
        assert r.status[0] == _capi.RESECT_NOT_CONVERGED and r.iterations[0] == k and r.n_used[0] == 37
        assert dist <= max(10 * floor, ROUNDING)
        rms, n = rr.rms_at(6, c.k, r.q[0], r.t[0], c.points, c.pixels)
        assert n == 37 and _close(r.rms[0], rms)
        if k < first:
            assert _is_start(r.q[0], r.t[0], q0, c.start[1])


def test_resect_invalid(api):
    c = rr.boundary_case("invalid")
    r = _resect(api, c)
    assert r.status[0] == _capi.RESECT_OK and r.n_used[0] == 36
    step = rr.criterion(6, c.k, r.q[0], r.t[0], c.points, c.pixels)
    rms, n = rr.rms_at(6, c.k, r.q[0], r.t[0], c.points, c.pixels)
    print("resect invalid: reference step", step, "iterations", r.iterations[0], "rms", r.rms[0])
    assert step <= 1e-11 + 10 * rr.FLOOR and n == 36 and _close(r.rms[0], rms)


def test_resect_joins(api):
    c = rr.boundary_case("joins")
    a = lm.resect_loop(6, c.k, *c.start, c.points, c.pixels, 1)
    b = lm.resect_loop(6, c.k, *c.start, c.points, c.pixels, 1, h=2e-6)
    r = _resect(api, c, max_iterations=1)
    floor, dist = rr.pose_distance(*a.point, *b.point), rr.pose_distance(rr.rot(r.q[0]), r.t[0], *a.point)
    print("resect joins: floor", floor, "device", dist, "rms", r.rms[0])
    assert a.log == [True] and r.status[0] == _capi.RESECT_NOT_CONVERGED and r.iterations[0] == 1 and r.n_used[0] == 37
    assert dist <= max(10 * floor, ROUNDING)
    rms, n = rr.rms_at(6, c.k, r.q[0], r.t[0], c.points, c.pixels)
    assert n == 37 and _close(r.rms[0], rms)      # (the pair that joined is in the sums)


def _started(poses, seed, scale=0.02):
    rng = np.random.default_rng(seed)
    q0, t0 = [], []
    for R, t in poses:
        p = scale * rng.standard_normal(6)
        q0.append(_quat(rr.exp_so3(p[:3]) @ R))
        t0.append(t + p[3:])
    return np.array(q0), np.array(t0)


def test_resect_frame_without_a_valid_pair(api):
    k, off, px, pt, poses = rr.fixture(1, 0.1)
    n = 5
    q0, t0 = _started(poses[:n], 11)
    clean = _capi.camera_resect(api, 1, k, off[:n + 1], px[:off[n]], pt[:off[n]], q_init=q0, t_init=t0, covariance=True)
    assert (clean.status == _capi.RESECT_OK).all()
    qb, tb = q0.copy(), t0.copy()
    qb[2], tb[2] = _quat(poses[2][0]), rr.behind(poses[2])[1]
    r = _capi.camera_resect(api, 1, k, off[:n + 1], px[:off[n]], pt[:off[n]], q_init=qb, t_init=tb, covariance=True)
    assert r.status[2] == _capi.RESECT_DEGENERATE and r.iterations[2] == 0
    assert np.array_equal(r.q[2], [0, 0, 0, 1]) and not r.t[2].any() and r.rms[2] == 0 and r.n_used[2] == 0 and not r.cov[2].any()
    others = [0, 1, 3, 4]
    for name in ("q", "t", "rms", "n_used", "iterations", "status", "cov"):
        assert getattr(r, name)[others].tobytes() == getattr(clean, name)[others].tobytes(), name
    tb = np.array([rr.behind(p)[1] for p in poses[:n]])
    r = _capi.camera_resect(api, 1, k, off[:n + 1], px[:off[n]], pt[:off[n]], q_init=q0, t_init=tb)
    assert (r.status == _capi.RESECT_DEGENERATE).all() and not r.t.any() and not r.n_used.any()


# -------------------------------------------------------------------------------------------------------------- calibration

F = cr.BOUNDARY_FRAME


def _calib_distance(k_a, poses_a, k_b, poses_b, free=None):
    return max(cr.intrinsics_distance(k_a, k_b, free), cr.poses_distance(poses_a, poses_b))


def _calibrate(api, fixture, **kw):
    k, off, px, pt, k0, q0, t0 = fixture
    return _capi.camera_calibrate(api, 6, k0, off, px, pt, q_init=q0, t_init=t0, free_mask=cr.BOUNDARY_FREE,
                                  options=_capi.calibration_options(api, **kw) if kw else None)


def test_calib_lost(api):
    fx = cr.boundary_fixture("lost")
    k, off, px, pt, k0, q0, t0 = fx
    start = cr.start_poses(q0, t0)
    a = lm.calib_loop(6, k0, start, off, pt, px, 7, free=cr.BOUNDARY_FREE)
    b = lm.calib_loop(6, k0, start, off, pt, px, 7, free=cr.BOUNDARY_FREE, h=2e-6)
    first = a.log.index(True) + 1
    assert a.log == b.log and 4 <= first <= 6
    used = np.full(20, 36)
    used[F] = 37
    for n in range(1, first + 2):
        r = _calibrate(api, fx, max_iterations=n)
        point, lam = a.trace[n - 1][:2]
        floor = _calib_distance(*point, *b.trace[n - 1][0], cr.BOUNDARY_FREE)
        dist = _calib_distance(r.intrinsics, cr.start_poses(r.q, r.t), *point, cr.BOUNDARY_FREE)
        at = lm.calib_measure(6, r.intrinsics, cr.start_poses(r.q, r.t), off, pt, px)
        print("calib lost k", n, "accepted", a.log[:n], "lambda", r.lambda_, lam, "floor", floor, "device", dist, "costs", r.initial_cost, r.final_cost)
        assert r.status == _capi.CALIB_NOT_CONVERGED and r.iterations == n and r.lambda_ == lam
        assert np.array_equal(r.n_used, used) and r.pairs_used == 721 and r.frames_used == 20
        assert dist <= max(10 * floor, ROUNDING)
        assert _close(r.initial_cost, a.initial.cost) and _close(r.final_cost, at.cost)
        if n < first:      # rejected for ALL frames: the start comes back
            assert r.intrinsics.tobytes() == k0.tobytes() and r.final_cost == r.initial_cost and (n > 1 or r.lambda_ == 1e-3)
            for f in (0, F, 19):
                assert _is_start(r.q[f], r.t[f], q0[f], t0[f]), f
        else:
            assert r.final_cost < r.initial_cost and not _is_start(r.q[0], r.t[0], q0[0], t0[0])


def test_calib_invalid(api):
    fx = cr.boundary_fixture("invalid")
    k, off, px, pt, k0, q0, t0 = fx
    r = _calibrate(api, fx)
    assert r.status == _capi.CALIB_OK and r.frames_used == 20 and r.pairs_used == 720 and r.n_used[F] == 36 and (np.delete(r.n_used, F) == 36).all()
    s = cr.criterion(6, r.intrinsics, r.q, r.t, off, pt, px, free=cr.BOUNDARY_FREE)
    rms, n = cr.rms_at(6, r.intrinsics, r.q, r.t, off, pt, px)
    rf, nf = rr.rms_at(6, r.intrinsics, r.q[F], r.t[F], pt[off[F]:off[F + 1]], px[off[F]:off[F + 1]])
    print("calib invalid: reference step", s, "iterations", r.iterations, "rms", r.total_rms)
    assert s <= 1e-10 + 10 * cr.FLOOR[6]
    assert n == 720 and nf == 36 and _close(r.total_rms, rms) and _close(r.rms[F], rf) and _close(r.final_cost, 720 * rms * rms)
    assert r.intrinsics[3] == k0[3]


def test_calib_joins(api):
    fx = cr.boundary_fixture("joins")
    k, off, px, pt, k0, q0, t0 = fx
    start = cr.start_poses(q0, t0)
    a = lm.calib_loop(6, k0, start, off, pt, px, 1, free=cr.BOUNDARY_FREE)
    b = lm.calib_loop(6, k0, start, off, pt, px, 1, free=cr.BOUNDARY_FREE, h=2e-6)
    r = _calibrate(api, fx, max_iterations=1)
    floor = _calib_distance(*a.point, *b.point, cr.BOUNDARY_FREE)
    dist = _calib_distance(r.intrinsics, cr.start_poses(r.q, r.t), *a.point, cr.BOUNDARY_FREE)
    at = lm.calib_measure(6, r.intrinsics, cr.start_poses(r.q, r.t), off, pt, px)
    print("calib joins: lambda", r.lambda_, "floor", floor, "device", dist, "costs", r.initial_cost, r.final_cost)
    assert a.log == [True] and r.status == _capi.CALIB_NOT_CONVERGED and r.iterations == 1 and r.lambda_ == 1e-5
    assert r.n_used[F] == 37 and r.pairs_used == 721
    assert dist <= max(10 * floor, ROUNDING)
    assert r.final_cost > r.initial_cost      # (the pair that joined: a comparison of the totals would have rejected)
    assert _close(r.initial_cost, a.initial.cost) and _close(r.final_cost, at.cost) and at.ok.all()


def test_calib_frame_without_a_valid_pair(api):
    model, f = 1, 7
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    k0, q0, t0 = cr.standard_start(model, 0.1)
    tb = t0.copy()
    tb[f] = rr.behind((None, t0[f]))[1]
    _, ok = rr.project(model, k0, rr.rot(q0[f]), tb[f], pt[off[f]:off[f + 1]])
    assert not ok.any()
    r = _capi.camera_calibrate(api, model, k0, off, px, pt, q_init=q0, t_init=tb, covariance=True)
    keep = [i for i in range(20) if i != f]
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in keep])
    off19 = np.arange(20, dtype=np.int64) * 36
    clean = _capi.camera_calibrate(api, model, k0, off19, px[rows], pt[rows], q_init=q0[keep], t_init=t0[keep], covariance=True)
    assert r.status == clean.status == _capi.CALIB_OK and r.frames_used == clean.frames_used == 19 and r.pairs_used == 19 * 36
    assert r.frame_status[f] == _capi.RESECT_NOT_POSITIVE_DEFINITE and (r.frame_status[keep] == _capi.RESECT_OK).all()
    assert np.array_equal(r.q[f], [0, 0, 0, 1]) and not r.t[f].any() and r.rms[f] == 0 and r.n_used[f] == 0
    dk = cr.intrinsics_distance(r.intrinsics, clean.intrinsics)
    dp = cr.poses_distance(cr.start_poses(r.q[keep], r.t[keep]), cr.start_poses(clean.q, clean.t))
    s = cr.criterion(model, r.intrinsics, r.q[keep], r.t[keep], off19, pt[rows], px[rows])
    print("calib, a frame behind the camera: with and without it", dk, dp, "reference step", s, "iterations", r.iterations, clean.iterations)
    assert max(dk, dp) <= 10 * cr.FLOOR[model] and s <= 1e-10 + 10 * cr.FLOOR[model]
    # no frame has a valid pair: degenerate, the outputs are the starts as given
    tb = np.array([rr.behind((None, t))[1] for t in t0])
    q_in = q0 * 2.0
    r = _capi.camera_calibrate(api, model, k0, off, px, pt, q_init=q_in, t_init=tb, covariance=True)
    assert r.status == _capi.CALIB_DEGENERATE and r.iterations == 0 and r.lambda_ == 1e-4
    assert r.intrinsics.tobytes() == k0.tobytes() and r.q.tobytes() == q_in.tobytes() and r.t.tobytes() == tb.tobytes()
    assert not r.cov.any() and not r.rms.any() and not r.n_used.any()


# ---------------------------------------------------------------------------------------------------------------------- rig


def _rig_call(api, rig, start, **kw):
    names = ("q_rig_camera_init", "t_rig_camera_init", "q_frame_init", "t_frame_init")
    return _capi.rig_calibrate(api, rig.models, rig.ks, rig.n_frames, rig.view_camera, rig.view_frame, rig.view_offsets, rig.pixels,
                               rig.points, options=_capi.rig_options(api, **kw) if kw else None, covariance=True, **dict(zip(names, start)))


def _rig_point(r):
    return gr.poses_of(r.q_rig_camera, r.t_rig_camera), gr.poses_of(r.q_frame, r.t_frame)


def _rig_distance(a, b):
    return max(rr.pose_distance(*p, *q) for p, q in zip(list(a[0]) + list(a[1]), list(b[0]) + list(b[1])))


def test_rig_lost(api):
    rig, start, v = gr.boundary_rig("lost")
    c0, f0 = gr.poses_of(*start[:2]), gr.poses_of(*start[2:])
    a, b = lm.rig_loop(rig, c0, f0, 7), lm.rig_loop(rig, c0, f0, 7, h=2e-6)
    first = a.log.index(True) + 1
    assert a.log == b.log and 4 <= first <= 6
    used = np.full(60, 36)
    used[v] = 37
    for n in range(1, first + 2):
        r = _rig_call(api, rig, start, max_iterations=n)
        point, lam = a.trace[n - 1][:2]
        floor = _rig_distance(point, b.trace[n - 1][0])
        dist = _rig_distance(_rig_point(r), point)
        at = lm.rig_measure(rig, *_rig_point(r))
        print("rig lost k", n, "accepted", a.log[:n], "lambda", r.lambda_, lam, "floor", floor, "device", dist, "costs", r.initial_cost, r.final_cost)
        assert r.status == _capi.RIG_NOT_CONVERGED and r.iterations == n and r.lambda_ == lam
        assert np.array_equal(r.view_n_used, used) and r.pairs_used == 2161 and r.views_used == 60
        assert dist <= max(10 * floor, ROUNDING)
        assert _close(r.initial_cost, a.initial.cost) and _close(r.final_cost, at.cost)
        if n < first:      # rejected for ALL frames and cameras: the start comes back
            assert r.final_cost == r.initial_cost and (n > 1 or r.lambda_ == 1e-3)
            for f in (0, gr.BOUNDARY_FRAME, 19):
                assert _is_start(r.q_frame[f], r.t_frame[f], start[2][f], start[3][f]), f
            for c in (1, 2):
                assert _is_start(r.q_rig_camera[c], r.t_rig_camera[c], start[0][c], start[1][c]), c
        else:
            assert r.final_cost < r.initial_cost and not _is_start(r.q_frame[0], r.t_frame[0], start[2][0], start[3][0])


def test_rig_invalid(api):
    rig, start, v = gr.boundary_rig("invalid")
    r = _rig_call(api, rig, start)
    used = np.full(60, 36)
    assert r.status == _capi.RIG_OK and np.array_equal(r.view_n_used, used) and r.pairs_used == 2160 and r.views_used == 60
    s = gr.criterion(rig, r.q_rig_camera, r.t_rig_camera, r.q_frame, r.t_frame)
    rms, n, per = gr.rms_at(rig, r.q_rig_camera, r.t_rig_camera, r.q_frame, r.t_frame)
    print("rig invalid: reference step", s, "iterations", r.iterations, "rms", r.total_rms)
    assert s <= 1e-10 + 10 * gr.FLOOR["standard"]
    assert n == 2160 and _close(r.total_rms, rms) and _close(r.view_rms[v], per[v]) and _close(r.final_cost, 2160 * rms * rms)


def test_rig_joins(api):
    rig, start, v = gr.boundary_rig("joins")
    c0, f0 = gr.poses_of(*start[:2]), gr.poses_of(*start[2:])
    a, b = lm.rig_loop(rig, c0, f0, 1), lm.rig_loop(rig, c0, f0, 1, h=2e-6)
    r = _rig_call(api, rig, start, max_iterations=1)
    floor, dist = _rig_distance(a.point, b.point), _rig_distance(_rig_point(r), a.point)
    at = lm.rig_measure(rig, *_rig_point(r))
    print("rig joins: lambda", r.lambda_, "floor", floor, "device", dist, "costs", r.initial_cost, r.final_cost)
    assert a.log == [True] and r.status == _capi.RIG_NOT_CONVERGED and r.iterations == 1 and r.lambda_ == 1e-5
    assert r.view_n_used[v] == 37 and r.pairs_used == 2161
    assert dist <= max(10 * floor, ROUNDING)
    assert r.final_cost > r.initial_cost      # (the pair that joined: a comparison of the totals would have rejected)
    assert _close(r.initial_cost, a.initial.cost) and _close(r.final_cost, at.cost) and at.ok.all()


def test_rig_frame_without_a_valid_pair(api):
    rig, f = gr.standard(0.1, models=(1, 1, 1)), 7
    start = [a.copy() for a in gr.perturbed_start(rig, scale=0.005)]
    start[3][f] = rr.behind((None, start[3][f]))[1]
    cams, frames = gr.poses_of(*start[:2]), gr.poses_of(*start[2:])
    mine = np.flatnonzero(rig.view_frame == f)
    for u in mine:
        assert not gr.project(rig, u, cams[rig.view_camera[u]], frames[f])[1].any()
    r = _rig_call(api, rig, start)
    use = rig.view_frame != f
    assert r.status == _capi.RIG_OK and r.frames_used == 19 and r.views_used == 57 and r.pairs_used == 57 * 36
    assert r.frame_status[f] == _capi.RIG_FRAME_NOT_POSITIVE_DEFINITE and (np.delete(r.frame_status, f) == _capi.RIG_FRAME_OK).all()
    assert not r.view_n_used[mine].any() and not r.view_rms[mine].any() and (r.view_n_used[use] == 36).all()
    assert np.array_equal(r.q_frame[f], [0, 0, 0, 1]) and not r.t_frame[f].any()
    s = gr.criterion(rig, r.q_rig_camera, r.t_rig_camera, r.q_frame, r.t_frame, use=use)
    rms, n, per = gr.rms_at(rig, r.q_rig_camera, r.t_rig_camera, r.q_frame, r.t_frame, use=use)
    print("rig, a frame behind the cameras: reference step over the views in use", s, "iterations", r.iterations)
    assert s <= 1e-10 + 10 * gr.FLOOR["standard"] and n == 57 * 36 and _close(r.total_rms, rms)
    # no frame has a valid pair: degenerate, the outputs are the starts
    for i in range(rig.n_frames):
        start[3][i] = rr.behind((None, start[3][i]))[1]
    r = _rig_call(api, rig, start)
    assert r.status == _capi.RIG_DEGENERATE and r.iterations == 0 and r.lambda_ == 1e-4
    for i in range(rig.n_frames):
        assert _is_start(r.q_frame[i], r.t_frame[i], start[2][i], start[3][i]), i
    for c in range(3):
        assert _is_start(r.q_rig_camera[c], r.t_rig_camera[c], start[0][c], start[1][c]), c
    assert not r.cov.any() and not r.view_rms.any() and not r.view_n_used.any()
