"""Intrinsic calibration on the device (calico_camera_calibrate) against the numpy reference of calib_ref.py.

The optimality criterion: the reference's UNDAMPED Gauss-Newton step at the DEVICE's estimate has
s <= step_tolerance + 10 FLOOR[model] (s: calib_ref.step_size, the library's step size): the device stops after an accepted step
below step_tolerance = 1e-10 taken at low damping, Gauss-Newton contracts from there, and 10 FLOOR covers the reference's own
difference quotients (FLOOR: tests/test_calib_host.py measures it).
Noise-free bound: max(100 x the reference's own distance to the truth from the same start, 1e-9); the reference's distance is at
most 3.6e-15 (REF_FREE, measured in tests/test_calib_host.py), so the bound is 1e-9.
Covariance bound: 10 x the relative agreement of the reference's reduced-system inverse from h = 1e-6 and h = 2e-6 differences
at the device's estimate, computed per model in the test (measured by model: the agreement is 1.9e-9, 2.7e-9, 1.5e-10, 2.2e-9,
7.4e-11, 1.1e-9, 3.0e-9; the device is within 1.4e-9, 3.8e-10, 4.1e-11, 2.4e-9, 8.8e-11, 7.7e-10, 1.7e-9 of the h = 1e-6 inverse).
Measured on an MI355X, standard start, 0.1 px noise: iterations 7, 12, 6, 7, 6, 6, 6 for models 1..7; the reference's s at the
device's estimate 9.0e-13, 5.5e-12, 1.8e-11, 1.8e-10, 4.6e-13, 2.6e-13, 3.2e-11; noise-free distance to the truth at most 5.5e-15."""
import numpy as np
import pytest

import calib_ref as cr
import resect_ref as rr
from calico_amd import _capi, synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-10


def bound(model):
    return TOL + 10 * cr.FLOOR[model]


@pytest.fixture(scope="module")
def api(hip):
    return hip


_RUNS = {}


def _standard(api, model, noise):
    """The call from the standard start with the covariance, once per (model, noise) and module."""
    if (model, noise) not in _RUNS:
        _, off, px, pt, _ = rr.fixture(model, noise)
        k0, q0, t0 = cr.standard_start(model, noise)
        _RUNS[(model, noise)] = _capi.camera_calibrate(api, model, k0, off, px, pt, q_init=q0, t_init=t0, covariance=True)
    return _RUNS[(model, noise)]


def _same(a, b):
    for name in ("intrinsics", "q", "t", "rms", "n_used", "frame_status", "cov"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None and y is None) or x.tobytes() == y.tobytes(), name
    for name in ("status", "iterations", "initial_cost", "final_cost", "total_rms", "frames_used", "pairs_used", "lambda_"):
        assert getattr(a, name) == getattr(b, name), name


@pytest.mark.parametrize("model", cr.MODELS)
def test_noisy_fixture_meets_the_optimality_criterion(api, model):
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    r = _standard(api, model, 0.1)
    assert r.status == _capi.CALIB_OK and r.frames_used == 20 and r.pairs_used == 720, (r.status, r.frames_used, r.pairs_used)
    assert (r.frame_status == _capi.RESECT_OK).all() and (r.n_used == 36).all()
    s = cr.criterion(model, r.intrinsics, r.q, r.t, off, pt, px)
    rms, n = cr.rms_at(model, r.intrinsics, r.q, r.t, off, pt, px)
    print("model", model, "reference step at the device's estimate", s, "bound", bound(model), "iterations", r.iterations, "rms", r.total_rms,
          "lambda", r.lambda_)
    assert s <= bound(model)
    assert n == 720 and abs(r.total_rms - rms) <= 1e-9 * rms, (r.total_rms, rms)
    assert r.final_cost < r.initial_cost and abs(r.final_cost - 720 * rms * rms) <= 1e-9 * r.final_cost
    for f in (0, 11, 19):
        rf, _ = rr.rms_at(model, r.intrinsics, r.q[f], r.t[f], pt[off[f]:off[f + 1]], px[off[f]:off[f + 1]])
        assert abs(r.rms[f] - rf) <= 1e-9 * rf


@pytest.mark.parametrize("model", cr.MODELS)
def test_noise_free_fixture_recovers_the_truth(api, model):
    k, off, px, pt, poses = rr.fixture(model, 0.0)
    r = _standard(api, model, 0.0)
    assert r.status == _capi.CALIB_OK and r.frames_used == 20
    dist = max(cr.intrinsics_distance(r.intrinsics, k), cr.poses_distance(cr.start_poses(r.q, r.t), poses))
    limit = max(100 * cr.REF_FREE[model], 1e-9)
    print("model", model, "distance to the truth", dist, "bound", limit, "iterations", r.iterations, "rms", r.total_rms)
    assert dist <= limit
    assert r.total_rms <= 1e-9


def test_opencv8_with_the_denominator_fixed_at_the_truth(api):
    model = 2
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    k0, q0, t0 = cr.standard_start(model, 0.1)
    k0 = k0.copy()
    k0[8:] = k[8:]
    free = np.array([1] * 8 + [0] * 3)
    r = _capi.camera_calibrate(api, model, k0, off, px, pt, q_init=q0, t_init=t0, free_mask=free, covariance=True)
    assert r.status == _capi.CALIB_OK and r.frames_used == 20
    assert r.intrinsics[8:].tobytes() == k0[8:].tobytes()
    s = cr.criterion(model, r.intrinsics, r.q, r.t, off, pt, px, free=free)
    print("reference step over the free set", s, "iterations", r.iterations)
    assert s <= bound(model)
    assert not r.cov[8:, :].any() and not r.cov[:, 8:].any() and (np.diag(r.cov)[:8] > 0).all()
    ref = cr.reduced_covariance(model, r.intrinsics, r.q, r.t, off, pt, px, free=free)
    ref2 = cr.reduced_covariance(model, r.intrinsics, r.q, r.t, off, pt, px, h=2e-6, free=free)
    agree = np.abs(ref - ref2).max() / np.abs(ref).max()
    assert np.abs(r.cov - ref).max() / np.abs(ref).max() <= 10 * agree


def _ragged(model):
    """The 20 noisy frames of the fixture, interleaved with frames of 0, 3, 65 and 129 pairs: shifted copies of the chart (as the
    resection test builds them) seen from poses of the fixture, 0.1 px noise. Returns (frames as (pixels, points), extra)."""
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    plane = syn.planar_points()
    pool = np.concatenate([plane + [dx, dy, 0.0] for dx, dy in ((0, 0), (0.1, 0.05), (-0.07, 0.11), (0.13, -0.09))])
    rng = np.random.default_rng(99 + model)
    frames = [(px[off[f]:off[f + 1]], pt[off[f]:off[f + 1]]) for f in range(20)]
    extra = {}
    for at, count, pose in ((17, 129, 3), (12, 3, 5), (6, 65, 9), (2, 0, 14)):      # (inserted from the back: positions stay)
        p = {3: pool[[7, 10, 25]], 0: pool[:0]}.get(count, pool[:count])
        pix, ok = rr.project(model, k, *poses[pose], p)
        assert ok.all()
        frames.insert(at, (pix + 0.1 * rng.standard_normal(pix.shape), p))
    for i, (a, _) in enumerate(frames):
        if len(a) != 36:
            extra[len(a)] = i
    return frames, extra


def _batch(frames):
    off = np.concatenate([[0], np.cumsum([len(a) for a, _ in frames])]).astype(np.int64)
    return off, np.concatenate([a for a, _ in frames]).reshape(-1, 2), np.concatenate([b for _, b in frames]).reshape(-1, 3)


@pytest.mark.parametrize("model", (1, 4))
def test_ragged_batch_with_deficient_frames(api, model):
    """Frames of 65 and 129 pairs cross the 64-lane trips; frames of 0 and 3 pairs carry their status and do not take part: the
    estimate agrees with the call without them."""
    frames, extra = _ragged(model)
    k0 = cr.start_intrinsics(model)
    whole = _capi.camera_calibrate(api, model, k0, *_batch(frames))
    deficient = sorted((extra[0], extra[3]))
    clean_frames = [fr for i, fr in enumerate(frames) if i not in deficient]
    clean = _capi.camera_calibrate(api, model, k0, *_batch(clean_frames))
    assert whole.status == clean.status == _capi.CALIB_OK
    assert whole.frames_used == clean.frames_used == 22 and whole.pairs_used == 20 * 36 + 65 + 129
    for i in deficient:
        assert whole.frame_status[i] == _capi.RESECT_TOO_FEW_POINTS
        assert np.array_equal(whole.q[i], [0, 0, 0, 1]) and not whole.t[i].any() and whole.rms[i] == 0 and whole.n_used[i] == 0
    keep = [i for i in range(len(frames)) if i not in deficient]
    assert (whole.frame_status[keep] == _capi.RESECT_OK).all()
    assert whole.n_used[keep].tolist() == [len(a) for a, _ in clean_frames] == clean.n_used.tolist()
    dk = cr.intrinsics_distance(whole.intrinsics, clean.intrinsics)
    dp = cr.poses_distance(cr.start_poses(whole.q[keep], whole.t[keep]), cr.start_poses(clean.q, clean.t))
    off, px, pt = _batch(clean_frames)
    s = cr.criterion(model, whole.intrinsics, whole.q[keep], whole.t[keep], off, pt, px)
    print("model", model, "with and without the deficient frames", dk, dp, "reference step", s, "iterations", whole.iterations)
    assert max(dk, dp) <= 10 * cr.FLOOR[model]
    assert s <= bound(model)


@pytest.mark.parametrize("model", (1, 6))
def test_huber_loss_resists_displaced_pixels(api, model):
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    k0, q0, t0 = cr.standard_start(model, 0.1)
    rng = np.random.default_rng(31 + model)
    bad = rng.choice(len(px), len(px) // 20, replace=False)
    ang = rng.uniform(0, 2 * np.pi, len(bad))
    pix = px.copy()
    pix[bad] += 30.0 * np.c_[np.cos(ang), np.sin(ang)]
    dist = {}
    for scale in (1.0, 0.0):
        r = _capi.camera_calibrate(api, model, k0, off, pix, pt, q_init=q0, t_init=t0, options=_capi.calibration_options(api, huber_scale=scale))
        assert r.status == _capi.CALIB_OK and r.frames_used == 20 and r.pairs_used == 720
        dist[scale] = cr.intrinsics_distance(r.intrinsics, k)
        s = cr.criterion(model, r.intrinsics, r.q, r.t, off, pt, pix, huber=scale)
        print("model", model, "huber", scale, "reference step", s, "intrinsics' distance to the truth", dist[scale], "iterations", r.iterations)
        if scale > 0:      # (without the loss the 30 px residuals lift the reference's own difference error above its FLOOR)
            assert s <= bound(model)
    assert dist[1.0] < dist[0.0]


@pytest.mark.parametrize("model", cr.MODELS)
def test_covariance_is_the_inverse_of_the_reduced_system(api, model):
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    r = _standard(api, model, 0.1)
    assert r.status == _capi.CALIB_OK
    C1 = cr.reduced_covariance(model, r.intrinsics, r.q, r.t, off, pt, px)
    C2 = cr.reduced_covariance(model, r.intrinsics, r.q, r.t, off, pt, px, h=2e-6)
    agree = np.abs(C1 - C2).max() / np.abs(C1).max()
    err = np.abs(r.cov - C1).max() / np.abs(C1).max()
    print("model", model, "reference's own agreement", agree, "device against reference", err)
    assert np.array_equal(r.cov, r.cov.T) or np.abs(r.cov - r.cov.T).max() <= 1e-12 * np.abs(r.cov).max()
    assert (np.diag(r.cov) > 0).all()
    assert err <= 10 * agree


def test_one_iteration_is_not_converged_with_a_finite_point(api):
    model = 3
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    k0, q0, t0 = cr.standard_start(model, 0.1)
    r = _capi.camera_calibrate(api, model, k0, off, px, pt, q_init=q0, t_init=t0, options=_capi.calibration_options(api, max_iterations=1),
                               covariance=True)
    assert r.status == _capi.CALIB_NOT_CONVERGED and r.iterations == 1 and r.frames_used == 20
    assert np.isfinite(r.intrinsics).all() and np.isfinite(r.q).all() and np.isfinite(r.t).all() and np.isfinite(r.cov).all()
    assert r.final_cost < r.initial_cost      # (the one step was accepted: the point moved)
    assert not np.array_equal(r.intrinsics, k0)


def test_two_usable_frames_are_too_few(api):
    model = 1
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    k0, q0, t0 = cr.standard_start(model, 0.1)
    n = off[2]
    off3 = np.array([0, off[1], n, n + 3], np.int64)      # two frames and one of three pairs
    q_in, t_in = np.r_[q0[:2], [[0.0, 0, 0, 1]]], np.r_[t0[:2], [[0.0, 0, 1]]]
    r = _capi.camera_calibrate(api, model, k0, off3, px[:n + 3], pt[:n + 3], q_init=q_in, t_init=t_in, covariance=True)
    assert r.status == _capi.CALIB_TOO_FEW_FRAMES and r.iterations == 0 and r.frames_used == 2
    assert r.intrinsics.tobytes() == k0.tobytes()
    assert r.q[:2].tobytes() == q0[:2].tobytes() and r.t[:2].tobytes() == t0[:2].tobytes()
    assert r.frame_status.tolist() == [_capi.RESECT_OK, _capi.RESECT_OK, _capi.RESECT_TOO_FEW_POINTS]
    assert np.array_equal(r.q[2], [0, 0, 0, 1]) and not r.t[2].any() and not r.cov.any() and not r.rms.any()
    cold = _capi.camera_calibrate(api, model, k0, off3, px[:n + 3], pt[:n + 3])      # the same through the resection
    assert cold.status == _capi.CALIB_TOO_FEW_FRAMES and cold.intrinsics.tobytes() == k0.tobytes()
    assert cold.frame_status.tolist() == [_capi.RESECT_OK, _capi.RESECT_OK, _capi.RESECT_TOO_FEW_POINTS]


def test_two_calls_are_bit_identical(api):
    model = 7
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    k0, q0, t0 = cr.standard_start(model, 0.1)
    o = _capi.calibration_options(api, huber_scale=0.15)
    a = _capi.camera_calibrate(api, model, k0, off, px, pt, q_init=q0, t_init=t0, options=o, covariance=True)
    b = _capi.camera_calibrate(api, model, k0, off, px, pt, q_init=q0, t_init=t0, options=o, covariance=True)
    assert a.status == _capi.CALIB_OK
    _same(a, b)
    c = _capi.camera_calibrate(api, model, k0, off, px, pt, covariance=True)      # and through the resection
    d = _capi.camera_calibrate(api, model, k0, off, px, pt, covariance=True)
    assert c.status == _capi.CALIB_OK
    _same(c, d)


def _detections(off, px, pt):
    model_definition = {i: pt[i] for i in range(off[1])}
    return [{i: px[off[f] + i] for i in range(off[f + 1] - off[f])} for f in range(len(off) - 1)], model_definition


def test_kannala_brandt_from_detections_end_to_end(api):
    """utils.InitializeIntrinsicsAndPoses: Zhang's pinhole, InitialIntrinsics, the resection of every frame and the calibration,
    from nothing but the detections (model 3: the model tests/test_calib_host.py shows the reference converging for)."""
    from calico_amd import calico
    model = 3
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    detections, model_definition = _detections(off, px, pt)
    camera = calico.Camera()
    camera.SetModel(calico.CameraIntrinsicsModel.kKannalaBrandt)
    intrinsics, R_chart_camera, t_chart_camera, ok = calico.InitializeIntrinsicsAndPoses(camera, detections, model_definition)
    assert ok.all() and np.array_equal(intrinsics, camera.GetIntrinsics())
    est = [(R.T, -R.T @ t) for R, t in zip(R_chart_camera, t_chart_camera)]
    s = cr.gn(model, intrinsics, est, off, pt, px)[2]
    print("reference step", s, "intrinsics' distance to the truth", cr.intrinsics_distance(intrinsics, k))
    assert s <= bound(model)
    assert cr.intrinsics_distance(intrinsics, k) < 1e-2 and cr.poses_distance(est, poses) < 1e-2


@pytest.mark.parametrize("model", (1, 4))
def test_camera_calibrate_intrinsics_through_pybind(api, model):
    from calico_amd import calico
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    k0, q0, t0 = cr.standard_start(model, 0.1)
    detections, model_definition = _detections(off, px, pt)
    camera = calico.Camera()
    camera.SetModel(calico.CameraIntrinsicsModel(model))
    camera.SetIntrinsics(k0)
    out = camera.CalibrateIntrinsics(detections, model_definition, covariance=True, q_init=q0, t_init=t0)
    r = _standard(api, model, 0.1)
    assert out["status"] == _capi.CALIB_OK and out["iterations"] == r.iterations
    assert np.array_equal(camera.GetIntrinsics(), out["intrinsics"])
    for name, mine in (("intrinsics", r.intrinsics), ("q", r.q), ("t", r.t), ("rms", r.rms), ("cov", r.cov)):      # the C ABI's bits
        assert out[name].tobytes() == mine.tobytes(), name
    s = cr.criterion(model, out["intrinsics"], out["q"], out["t"], off, pt, px)
    print("model", model, "reference step", s)
    assert s <= bound(model)
