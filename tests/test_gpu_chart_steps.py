"""The chart estimators' LM steps, long batches and redo ladder on the device (calico_camera_resect, calico_camera_calibrate,
calico_rig_calibrate), held to the references' dense damped Levenberg-Marquardt (lm_rule_ref.py over resect_ref.py,
calib_ref.py and rig_ref.py). With max_iterations = k an estimator tries exactly k damped steps from the start it is given and
returns the point it kept, iterations = k and the next lambda: the step tests compare that point with the reference loop's.

Which test reaches which code (tests/test_gpu_chart_rejections.py continues the table for the pairs the camera model rejects):

  Gram blocks A_f, B_f, C, lambda diag, Y_f, the frames' shares,     test_calib_steps, test_rig_steps, test_resect_steps: a wrong
  rig's fill -B_v^T Y_w, the back-substitution                        block moves the k-th point by far more than 10 floors
                                                                      (tests/test_calib_host.py and tests/test_rig_host.py hold
                                                                      the fixtures to that: the mutant steps)
  calib_decide_kernel  f += 64 (second and third trip)                test_calib_long_batch, test_calib_long_batch_step
  calib_reduce_kernel  unrolled body (8 parts x 16 frames)            test_calib_long_batch, test_calib_long_batch_covariance
  rig_decide_kernel    v += 64 (three trips), f += 64 (two)           test_rig_many_views, test_rig_many_views_step
  rig_reduce_kernel    unrolled body (4 parts x 4 frames)             test_rig_many_views, test_rig_many_views_covariance
  a rejected first step (lambda x 10), all frames and cameras stay,   test_rig_steps[standard-*], test_rig_steps[chain-*]
  final_cost == initial_cost bit for bit
  redo: the reduced system is not positive definite, lambda x 10,     test_redo_ladder_ends_degenerate_with_the_inputs
  elimination and reduction again; the top of the ladder,
  CALICO_CALIB_DEGENERATE, give_inputs (chart.cpp)
  Rig has no reachable counterpart of the redo ladder: a camera that is connected has views, every view of a camera that is not
  held adds a positive definite block to the camera's diagonal, and a frame that is not positive definite drops out before the
  reduction; no finite input makes the reduced system of the extrinsics indefinite while every frame's block is definite.

Costs: initial_cost against the reference's cost at the start and final_cost against the reference's cost AT THE DEVICE's kept
point, to 1e-9 relative. (Away from the minimum the cost has a gradient: at its own k-step points from h = 1e-6 and h = 2e-6
the reference's costs differ from each other by up to 5e-9 relative, so they cannot hold anything to 1e-9; the test prints them.)
Bound of the step tests: 10 x the reference's own floor, the distance between its k-step points from difference steps
h = 1e-6 and h = 2e-6, measured inside the test and printed; where every step was rejected the floor is zero and the bound is
ROUNDING = 1e-14, twenty units in the last place of the unit quaternions and of translations of at most 2 m that the start
goes through on its way in and out (normalisation, quaternion to matrix and back). Costs to 1e-9 relative, lambda exactly.

Measured on an MI355X (floor / the device's distance to the reference's k-step point; every lambda equal to the reference's):
  resect, 3 frames     model 1: k=1 4.7e-12 / 4.4e-12, k=3 4.1e-14 / 3.4e-14   3: 5.2e-12 / 4.0e-12, 7.1e-14 / 7.3e-14
                       6: 6.3e-12 / 4.1e-12, 9.4e-14 / 1.1e-13      (every step accepted)
  calib opencv5        k=1 1.1e-11 / 9.9e-12   k=3 1.4e-12 / 1.9e-12      opencv8  4.9e-10 / 1.6e-10   2.5e-9 / 8.3e-10 (third step
  rejected)            division 2.7e-11 / 2.1e-11   6.9e-11 / 3.1e-11      opencv8-free 1.0e-11 / 9.5e-12   3.4e-12 / 1.6e-12
                       opencv5-huber 8.8e-12 / 9.2e-12   2.9e-12 / 4.8e-12      long-1 (k=1) 1.9e-11 / 1.7e-11   long-6 2.4e-11 / 2.6e-11
  rig standard, chain  every step rejected (lambda 1e-3 after one, 0.1 after three): floor 0, the device 6.3e-17 from the start
  rig standard-near    4.1e-12 / 3.2e-12   9.4e-14 / 5.2e-14      chain-near 4.3e-12 / 3.7e-12   1.2e-13 / 9.3e-14
  rig wide             1.7e-11 / 9.7e-12   3.0e-12 / 3.1e-12      standard-huber 1.6e-11 / 1.6e-11   1.3e-12 / 8.1e-13      many (k=1) 1.6e-11 / 1.2e-11
  costs: the device's within 2e-14 relative of the reference's at the start and 4e-12 at the device's point (opencv8, k=3)
  calib, 137 frames    the reference's step at the device's estimate 1.1e-12 (model 1, 8 iterations) and 2.0e-12 (model 6, 6);
                       covariance: the reference agrees with itself to 3.3e-10 and 3.8e-10, the device is within 1.1e-10 and 2.5e-10
  rig, 140 views       the reference's step 1.5e-13 (no start, 15 iterations) and 1.7e-13 (perturbed start, 6); covariance 5.4e-11 / 3.6e-11
  rig covariance       agreement / device: chain with reference camera 1  7.1e-11 / 6.8e-11, wide 7.3e-11 / 9.8e-11, standard with Huber 5.4e-11 / 2.5e-11
  redo ladder          CALICO_CALIB_DEGENERATE, lambda 1e12, iterations 1; with w held: OK in 5 iterations, the reference's step 8.7e-14
The first run of the rejected-step cases showed final_cost one unit in the last place below initial_cost on a rig call that had
kept its start (tests/test_gpu_chart_rejections.py::test_rig_lost): the two were sums of the same terms in two orders. They are
one number now where no step was accepted (rig_kernels.hip, calib_kernels.hip: the final reduction).
"""
import functools

import numpy as np
import pytest

import calib_ref as cr
import lm_rule_ref as lm
import resect_ref as rr
import rig_ref as gr
from calico_amd import _capi

pytestmark = pytest.mark.gpu

TOL = 1e-10
ROUNDING = 1e-14


@pytest.fixture(scope="module")
def api(hip):
    return hip


def _close(a, b, rel=1e-9):
    return abs(a - b) <= rel * abs(b)


# ---------------------------------------------------------------------------------------------------------------- resection


def _resect_start(poses, seed):
    """The truth perturbed by 0.02 N(0, 1), as calib_ref.standard_start and rig_ref.perturbed_start perturb it."""
    rng = np.random.default_rng(seed)
    q0, t0 = [], []
    for R, t in poses:
        p = 0.02 * rng.standard_normal(6)
        q = rr.quat_of(rr.exp_so3(p[:3]) @ R)
        q0.append(q if q[3] >= 0 else -q)
        t0.append(t + p[3:])
    return np.array(q0), np.array(t0)


@pytest.mark.parametrize("k_steps", (1, 3))
@pytest.mark.parametrize("model", (1, 3, 6))
def test_resect_steps(api, model, k_steps):
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    n = 3
    q0, t0 = _resect_start(poses[:n], 4321 + model)
    r = _capi.camera_resect(api, model, k, off[:n + 1], px[:off[n]], pt[:off[n]], q_init=q0, t_init=t0,
                            options=_capi.resection_options(api, max_iterations=k_steps))
    floor = dist = 0.0
    for f in range(n):
        s = slice(off[f], off[f + 1])
        a = lm.resect_loop(model, k, rr.rot(q0[f]), t0[f], pt[s], px[s], k_steps)
        b = lm.resect_loop(model, k, rr.rot(q0[f]), t0[f], pt[s], px[s], k_steps, h=2e-6)
        assert a.log == b.log and a.status == "out_of_iterations"
        assert r.status[f] == _capi.RESECT_NOT_CONVERGED and r.iterations[f] == k_steps and r.n_used[f] == 36
        floor = max(floor, rr.pose_distance(*a.point, *b.point))
        dist = max(dist, rr.pose_distance(rr.rot(r.q[f]), r.t[f], *a.point))
        assert _close(r.rms[f], rr.rms_at(model, k, r.q[f], r.t[f], pt[s], px[s])[0])
    print("resect model", model, "k", k_steps, "floor", floor, "device", dist, "accepted", a.log)
    assert dist <= max(10 * floor, ROUNDING)


@pytest.mark.parametrize("model", (1, 6))
def test_resect_long_batch_is_frame_by_frame_bit_identical(api, model):
    """137 frames of 12 pairs: every frame's outputs are those of the same frame resected alone (the kernel's header: a frame
    reads and writes nothing but its own slices)."""
    k, off, px, pt, poses = rr.long_fixture(model, 0.1)
    whole = _capi.camera_resect(api, model, k, off, px, pt, covariance=True)
    assert (whole.status == _capi.RESECT_OK).all() and (whole.n_used == 12).all()
    for f in range(len(poses)):
        s = slice(off[f], off[f + 1])
        one = _capi.camera_resect(api, model, k, [0, 12], px[s], pt[s], covariance=True)
        for name in ("q", "t", "rms", "n_used", "iterations", "status", "cov"):
            assert getattr(whole, name)[f].tobytes() == getattr(one, name)[0].tobytes(), (f, name)


# -------------------------------------------------------------------------------------------------------------- calibration


def _calib_distance(k_a, poses_a, k_b, poses_b, free=None):
    return max(cr.intrinsics_distance(k_a, k_b, free), cr.poses_distance(poses_a, poses_b))


@functools.lru_cache(maxsize=None)
def _calib_case(name):
    """(model, k0, q0, t0, offsets, pixels, points, huber, free mask or None) of a step case."""
    model = {"opencv5": 1, "opencv8": 2, "division": 4, "opencv8-free": 2, "opencv5-huber": 1, "long-1": 1, "long-6": 6}[name]
    if name.startswith("long"):
        k, off, px, pt, _ = rr.long_fixture(model, 0.1)
        k0, q0, t0 = cr.long_start(model, 0.1)
    else:
        k, off, px, pt, _ = rr.fixture(model, 0.1)
        k0, q0, t0 = cr.standard_start(model, 0.1)
    huber, free = 0.0, None
    if name == "opencv8-free":      # the denominator fixed at the truth (test_gpu_calib.py)
        k0 = k0.copy()
        k0[8:] = k[8:]
        free = (1,) * 8 + (0,) * 3
    if name == "opencv5-huber":      # the displaced pixels of test_gpu_calib.py::test_huber_loss_resists_displaced_pixels
        rng = np.random.default_rng(31 + model)
        bad = rng.choice(len(px), len(px) // 20, replace=False)
        ang = rng.uniform(0, 2 * np.pi, len(bad))
        px = px.copy()
        px[bad] += 30.0 * np.c_[np.cos(ang), np.sin(ang)]
        huber = 1.0
    return model, k0, q0, t0, off, px, pt, huber, free


def _check_calib_steps(api, name, k_steps):
    model, k0, q0, t0, off, px, pt, huber, free = _calib_case(name)
    start = cr.start_poses(q0, t0)
    a = lm.calib_loop(model, k0, start, off, pt, px, k_steps, huber, free)
    b = lm.calib_loop(model, k0, start, off, pt, px, k_steps, huber, free, h=2e-6)
    assert a.log == b.log and a.status == "out_of_iterations" and a.final.ok.all()
    floor = _calib_distance(*b.point, *a.point, free)
    r = _capi.camera_calibrate(api, model, k0, off, px, pt, q_init=q0, t_init=t0, free_mask=free,
                               options=_capi.calibration_options(api, max_iterations=k_steps, huber_scale=huber))
    dist = _calib_distance(r.intrinsics, cr.start_poses(r.q, r.t), *a.point, free)
    print("calib", name, "k", k_steps, "floor", floor, "device", dist, "accepted", a.log, "lambda", r.lambda_, a.lam)
    assert r.status == _capi.CALIB_NOT_CONVERGED and r.iterations == k_steps and r.frames_used == len(q0) and r.pairs_used == len(px)
    assert r.lambda_ == a.lam
    assert dist <= max(10 * floor, ROUNDING)
    at = lm.calib_measure(model, r.intrinsics, cr.start_poses(r.q, r.t), off, pt, px, huber)
    print("    costs: device", r.initial_cost, r.final_cost, "reference at the start", a.initial.cost, "at the device's point", at.cost,
          "at its own points (h = 1e-6, 2e-6)", a.final.cost, b.final.cost)
    assert _close(r.initial_cost, a.initial.cost) and _close(r.final_cost, at.cost)
    assert (r.final_cost == r.initial_cost) if not any(a.log) else (r.final_cost < r.initial_cost)
    if free is not None:
        fixed = ~np.asarray(free, bool)
        assert r.intrinsics[fixed].tobytes() == k0[fixed].tobytes()


@pytest.mark.parametrize("k_steps", (1, 3))
@pytest.mark.parametrize("name", ("opencv5", "opencv8", "division", "opencv8-free", "opencv5-huber"))
def test_calib_steps(api, name, k_steps):
    _check_calib_steps(api, name, k_steps)


@pytest.mark.parametrize("model", (1, 6))
def test_calib_long_batch_step(api, model):
    _check_calib_steps(api, "long-%d" % model, 1)


_LONG = {}


def _long_run(api, model):
    if model not in _LONG:
        _, k0, q0, t0, off, px, pt, _, _ = _calib_case("long-%d" % model)
        _LONG[model] = _capi.camera_calibrate(api, model, k0, off, px, pt, q_init=q0, t_init=t0, covariance=True)
    return _LONG[model]


@pytest.mark.parametrize("model", (1, 6))
def test_calib_long_batch(api, model):
    k, off, px, pt, poses = rr.long_fixture(model, 0.1)
    r = _long_run(api, model)
    assert r.status == _capi.CALIB_OK and r.frames_used == 137 and r.pairs_used == 1644
    assert (r.frame_status == _capi.RESECT_OK).all() and (r.n_used == 12).all()
    s = cr.criterion(model, r.intrinsics, r.q, r.t, off, pt, px)
    limit = TOL + 10 * cr.FLOOR_LONG[model]
    rms, n = cr.rms_at(model, r.intrinsics, r.q, r.t, off, pt, px)
    print("calib long model", model, "reference step at the device's estimate", s, "bound", limit, "iterations", r.iterations)
    assert s <= limit
    assert n == 1644 and _close(r.total_rms, rms) and _close(r.final_cost, 1644 * rms * rms)
    for f in (0, 63, 136):
        rf, _ = rr.rms_at(model, r.intrinsics, r.q[f], r.t[f], pt[off[f]:off[f + 1]], px[off[f]:off[f + 1]])
        assert _close(r.rms[f], rf), f


@pytest.mark.parametrize("model", (1, 6))
def test_calib_long_batch_covariance(api, model):
    k, off, px, pt, poses = rr.long_fixture(model, 0.1)
    r = _long_run(api, model)
    assert r.status == _capi.CALIB_OK
    C1 = cr.reduced_covariance(model, r.intrinsics, r.q, r.t, off, pt, px)
    C2 = cr.reduced_covariance(model, r.intrinsics, r.q, r.t, off, pt, px, h=2e-6)
    agree = np.abs(C1 - C2).max() / np.abs(C1).max()
    err = np.abs(r.cov - C1).max() / np.abs(C1).max()
    print("calib long model", model, "covariance: the reference's own agreement", agree, "device against reference", err)
    assert err <= 10 * agree


def test_redo_ladder_ends_degenerate_with_the_inputs(api):
    """FieldOfView at w = 1e-3 with w free: its column is exactly zero, the reduced system is never positive definite, lambda
    climbs to its cap and the call ends DEGENERATE with the outputs equal to the inputs -- on its own, not at the host's bound
    on the cycles (the call returns CALICO_OK: camera_calibrate raises on anything else)."""
    k, off, px, pt, poses = cr.fov_fixture()
    k0, q0, t0 = cr.fov_start()
    ref = lm.calib_loop(5, k0, cr.start_poses(q0, t0), off, pt, px, 50)
    assert ref.status == "degenerate" and ref.lam == 1e12 and ref.iterations == 1
    q_in = q0 * 2.0      # (not normalised: the inputs come back as given)
    r = _capi.camera_calibrate(api, 5, k0, off, px, pt, q_init=q_in, t_init=t0, covariance=True)
    print("redo ladder: status", r.status, "lambda", r.lambda_, "iterations", r.iterations)
    assert r.status == _capi.CALIB_DEGENERATE and r.lambda_ == 1e12 and r.iterations == ref.iterations
    assert r.intrinsics.tobytes() == k0.tobytes() and r.q.tobytes() == q_in.tobytes() and r.t.tobytes() == t0.tobytes()
    assert not r.cov.any() and not r.rms.any() and not r.n_used.any() and (r.frame_status == _capi.RESECT_OK).all()
    assert r.frames_used == 20 and r.pairs_used == 0 and r.final_cost == 0.0


def test_field_of_view_with_w_held_converges(api):
    k, off, px, pt, poses = cr.fov_fixture()
    k0, q0, t0 = cr.fov_start()
    free = (1, 1, 1, 0)
    r = _capi.camera_calibrate(api, 5, k0, off, px, pt, q_init=q0, t_init=t0, free_mask=free, covariance=True)
    assert r.status == _capi.CALIB_OK and r.frames_used == 20 and r.pairs_used == 720
    assert r.intrinsics[3:].tobytes() == k0[3:].tobytes()
    s = cr.criterion(5, r.intrinsics, r.q, r.t, off, pt, px, free=free)
    print("field of view, w held: reference step over the free set", s, "iterations", r.iterations, "lambda", r.lambda_)
    assert s <= TOL + 10 * cr.FLOOR[5]
    assert not r.cov[3, :].any() and not r.cov[:, 3].any() and (np.diag(r.cov)[:3] > 0).all()


# ---------------------------------------------------------------------------------------------------------------------- rig


def _rig_call(api, rig, start=None, views=None, **kw):
    vc, vf, off, px, pt = (rig.view_camera, rig.view_frame, rig.view_offsets, rig.pixels, rig.points) if views is None else views
    names = ("q_rig_camera_init", "t_rig_camera_init", "q_frame_init", "t_frame_init")
    init = {} if start is None else dict(zip(names, start))
    return _capi.rig_calibrate(api, rig.models, rig.ks, rig.n_frames, vc, vf, off, px, pt,
                               options=_capi.rig_options(api, **kw) if kw else None, covariance=True, **init)


def _rig_distance(a, b):
    return max(rr.pose_distance(*p, *q) for p, q in zip(list(a[0]) + list(a[1]), list(b[0]) + list(b[1])))


def _displaced(rig):
    """The pixels of test_gpu_rig.py::test_huber_loss_resists_displaced_pixels."""
    rng = np.random.default_rng(777)
    px = rig.pixels.copy()
    hit = rng.choice(len(px), len(px) // 20, replace=False)
    ang = rng.uniform(0, 2 * np.pi, len(hit))
    px[hit] += 30.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    return px


@functools.lru_cache(maxsize=None)
def _rig_case(name):
    """(rig, start, huber) of a step case. `near`: from a quarter of the perturbation, where the first step is accepted (from
    the full one the reference -- and the device -- reject the first three steps of the standard and chain fixtures)."""
    rig = gr.FIXTURES[name.split("-")[0]](0.1)
    if name == "standard-huber":
        rig = rig._replace(pixels=_displaced(rig))
    start = gr.perturbed_start(rig, scale=0.005) if name.endswith("near") else gr.perturbed_start(rig)
    return rig, start, 1.0 if name.endswith("huber") else 0.0


def _check_rig_steps(api, name, k_steps):
    rig, start, huber = _rig_case(name)
    c0, f0 = gr.poses_of(*start[:2]), gr.poses_of(*start[2:])
    a = lm.rig_loop(rig, c0, f0, k_steps, huber=huber)
    b = lm.rig_loop(rig, c0, f0, k_steps, huber=huber, h=2e-6)
    assert a.log == b.log and a.status == "out_of_iterations" and a.final.ok.all()
    floor = _rig_distance(a.point, b.point)
    r = _rig_call(api, rig, start, max_iterations=k_steps, huber_scale=huber)
    dist = _rig_distance((gr.poses_of(r.q_rig_camera, r.t_rig_camera), gr.poses_of(r.q_frame, r.t_frame)), a.point)
    print("rig", name, "k", k_steps, "floor", floor, "device", dist, "accepted", a.log, "lambda", r.lambda_, a.lam)
    assert r.status == _capi.RIG_NOT_CONVERGED and r.iterations == k_steps
    assert r.views_used == len(rig.view_camera) and r.pairs_used == len(rig.pixels)
    assert r.lambda_ == a.lam
    assert dist <= max(10 * floor, ROUNDING)
    at = lm.rig_measure(rig, gr.poses_of(r.q_rig_camera, r.t_rig_camera), gr.poses_of(r.q_frame, r.t_frame), huber=huber)
    print("    costs: device", r.initial_cost, r.final_cost, "reference at the start", a.initial.cost, "at the device's point", at.cost,
          "at its own points (h = 1e-6, 2e-6)", a.final.cost, b.final.cost)
    assert _close(r.initial_cost, a.initial.cost) and _close(r.final_cost, at.cost)
    assert (r.final_cost == r.initial_cost) if not any(a.log) else (r.final_cost < r.initial_cost)


@pytest.mark.parametrize("k_steps", (1, 3))
@pytest.mark.parametrize("name", ("standard", "standard-near", "chain", "chain-near", "wide", "standard-huber"))
def test_rig_steps(api, name, k_steps):
    _check_rig_steps(api, name, k_steps)


def test_rig_many_views_step(api):
    _check_rig_steps(api, "many", 1)


_MANY = {}


def _many_run(api, started):
    if started not in _MANY:
        rig = gr.many(0.1)
        _MANY[started] = _rig_call(api, rig, gr.perturbed_start(rig) if started else None)
    return _MANY[started]


@pytest.mark.parametrize("started", (False, True))
def test_rig_many_views(api, started):
    rig = gr.many(0.1)
    r = _many_run(api, started)
    assert r.status == _capi.RIG_OK and (r.frames_used, r.views_used, r.pairs_used, r.cameras_used) == (70, 140, 1680, 2)
    assert (r.frame_status == _capi.RIG_FRAME_OK).all() and (r.view_status == _capi.RESECT_OK).all() and (r.view_n_used == 12).all()
    s = gr.criterion(rig, r.q_rig_camera, r.t_rig_camera, r.q_frame, r.t_frame)
    rms, n, per = gr.rms_at(rig, r.q_rig_camera, r.t_rig_camera, r.q_frame, r.t_frame)
    print("rig many views, start given:", started, "reference step", s, "bound", TOL + 10 * gr.FLOOR["many"], "iterations", r.iterations)
    assert s <= TOL + 10 * gr.FLOOR["many"]
    assert n == 1680 and _close(r.total_rms, rms) and _close(r.final_cost, 1680 * rms * rms)
    for v in (0, 64, 139):
        assert _close(r.view_rms[v], per[v]), v


def test_rig_many_views_covariance(api):
    rig = gr.many(0.1)
    r = _many_run(api, True)
    est = (r.q_rig_camera, r.t_rig_camera, r.q_frame, r.t_frame)
    ref, ref2 = gr.reduced_covariance(rig, *est), gr.reduced_covariance(rig, *est, h=2e-6)
    agree = np.abs(ref - ref2).max() / np.abs(ref).max()
    got = np.abs(r.cov - ref).max() / np.abs(ref).max()
    print("rig many views: covariance: device within", got, "of the reference; the reference agrees with itself to", agree)
    assert got <= 10 * agree


def test_rig_many_views_permuted_are_bit_identical(api):
    rig = gr.many(0.1)
    first = _many_run(api, False)
    perm = np.random.default_rng(6).permutation(len(rig.view_camera))
    off = rig.view_offsets
    counts = (off[1:] - off[:-1])[perm]
    rows = np.concatenate([np.arange(off[v], off[v + 1]) for v in perm])
    views = (rig.view_camera[perm], rig.view_frame[perm], np.concatenate([[0], np.cumsum(counts)]), rig.pixels[rows], rig.points[rows])
    other = _rig_call(api, rig, None, views)
    for name in ("q_rig_camera", "t_rig_camera", "camera_status", "q_frame", "t_frame", "frame_status", "view_rms", "view_n_used", "view_status", "cov"):
        a, b = getattr(first, name), getattr(other, name)
        assert (a[perm] if name.startswith("view_") else a).tobytes() == b.tobytes(), name
    for name in ("status", "iterations", "initial_cost", "final_cost", "total_rms", "cameras_used", "frames_used", "views_used", "pairs_used", "lambda_"):
        assert getattr(first, name) == getattr(other, name), name


@pytest.mark.parametrize("name", ("chain-reference-1", "wide", "standard-huber"))
def test_rig_covariance_beyond_the_standard_fixture(api, name):
    rig, start, huber = _rig_case(name if name != "chain-reference-1" else "chain")
    held = {1} if name == "chain-reference-1" else {0}
    if name == "chain-reference-1":
        r = _rig_call(api, rig, None, reference_camera=1)
    else:
        r = _rig_call(api, rig, start, huber_scale=huber)
    assert r.status == _capi.RIG_OK and r.views_used == len(rig.view_camera)
    est = (r.q_rig_camera, r.t_rig_camera, r.q_frame, r.t_frame)
    ref = gr.reduced_covariance(rig, *est, held=held, huber=huber)
    ref2 = gr.reduced_covariance(rig, *est, held=held, huber=huber, h=2e-6)
    agree = np.abs(ref - ref2).max() / np.abs(ref).max()
    got = np.abs(r.cov - ref).max() / np.abs(ref).max()
    print("rig", name, "covariance: device within", got, "of the reference; the reference agrees with itself to", agree)
    assert got <= 10 * agree
    h = sorted(held)[0]
    assert not r.cov[6 * h:6 * h + 6, :].any() and not r.cov[:, 6 * h:6 * h + 6].any()
