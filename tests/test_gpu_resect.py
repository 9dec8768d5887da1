"""Chart resection on the device (calico_camera_resect) against the numpy reference of resect_ref.py.

The optimality criterion: for a frame with status OK the reference's weighted Gauss-Newton step at the DEVICE's pose satisfies
|step|_inf <= step_tolerance + 10 FLOOR (1e-11 + 1.5e-12): the kernel stops after an accepted step below step_tolerance and
Gauss-Newton contracts from there; 10 FLOOR covers the reference's own difference error (FLOOR: its last step, 1.4e-13 measured
over the seven models and twenty frames, tests/test_resect_host.py).
Noise-free bound: the reference started 1e-3 off the truth ends 6.4e-16 from it on the same data (measured, all models and
frames); 100 times that is below the floor of 1e-12 the bound is given, so the bound is 1e-12.
Covariance bound: 10 times the relative agreement of the reference's (J^T W J)^-1 from h = 1e-6 and h = 2e-6 differences,
computed per frame at the device's pose (measured: up to 4.9e-10, so the bound is a few 1e-9)."""
import os

import numpy as np
import pytest

import helpers
import resect_ref as rr
from calico_amd import _capi, synthetic as syn

pytestmark = pytest.mark.gpu

TOL = 1e-11
BOUND = TOL + 10 * rr.FLOOR
REF_FREE = 6.4e-16
FREE_BOUND = max(100 * REF_FREE, 1e-12)
W = 4      # frames per workgroup (kResectWaves, resect_kernels.hip)


@pytest.fixture(scope="module")
def api(hip):
    return hip


def test_waves_per_workgroup_is_what_the_batch_sizes_assume():
    src = open(os.path.join(helpers.ROOT, "calico_amd", "csrc", "resect_kernels.hip")).read()
    assert "constexpr int kResectWaves = %d;" % W in src


def _same(a, b, frames_a=None, frames_b=None):
    """Bit-identical outputs (of the given frames)."""
    for name in ("q", "t", "rms", "n_used", "iterations", "status", "cov"):
        x, y = getattr(a, name), getattr(b, name)
        if x is None and y is None:
            continue
        x = x if frames_a is None else x[frames_a]
        y = y if frames_b is None else y[frames_b]
        assert x.tobytes() == y.tobytes(), name


def _zeroed(r, f):
    assert np.array_equal(r.q[f], [0, 0, 0, 1]) and not r.t[f].any() and r.rms[f] == 0 and r.n_used[f] == 0
    assert r.cov is None or not r.cov[f].any()


@pytest.mark.parametrize("model", rr.MODELS)
def test_noise_free_recovers_the_true_pose(api, model):
    k, off, px, pt, poses = rr.fixture(model, 0.0)
    r = _capi.camera_resect(api, model, k, off, px, pt)
    assert (r.status == _capi.RESECT_OK).all(), r.status
    dist = [rr.pose_distance(rr.rot(r.q[f]), r.t[f], *poses[f]) for f in range(len(poses))]
    print("model", model, "distance to the truth", max(dist), "rms", r.rms.max(), "iterations", r.iterations.max())
    assert max(dist) <= FREE_BOUND
    assert r.rms.max() <= 1e-9
    assert (r.n_used == 36).all()


@pytest.mark.parametrize("model", rr.MODELS)
def test_noisy_frames_meet_the_optimality_criterion(api, model):
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    r = _capi.camera_resect(api, model, k, off, px, pt)
    assert (r.status == _capi.RESECT_OK).all(), r.status
    assert (r.n_used == 36).all()
    worst = 0.0
    for f in range(len(poses)):
        s = slice(off[f], off[f + 1])
        worst = max(worst, rr.criterion(model, k, r.q[f], r.t[f], pt[s], px[s]))
        rms, n = rr.rms_at(model, k, r.q[f], r.t[f], pt[s], px[s])
        assert n == 36 and abs(r.rms[f] - rms) <= 1e-9 * rms, (f, r.rms[f], rms)
    print("model", model, "reference step at the device's poses", worst, "iterations", r.iterations.max())
    assert worst <= BOUND


def _ragged(model):
    counts = [4, 5, 0, 63, 64, 3, 65, 129, 144]
    k = np.array(syn._TRUE_INTRINSICS[model], float)
    plane = syn.planar_points()
    pool = np.concatenate([plane + [dx, dy, 0.0] for dx, dy in ((0, 0), (0.1, 0.05), (-0.07, 0.11), (0.13, -0.09))])
    poses = rr.true_poses()
    rng = np.random.default_rng(77 + model)
    pts, pix, used = [], [], []
    for i, c in enumerate(counts):
        # (the few-point frames from the middle of the chart: at its corners the tilted OpenCv models have no inverse, and a pixel
        # without a valid unprojection does not count towards the four the start needs)
        p = {4: pool[[7, 10, 25, 28]], 5: pool[[7, 10, 25, 28, 14]], 3: pool[[7, 10, 25]], 144: syn.aprilgrid_points()}.get(c, pool[:c])
        R, t = poses[2 * i + 1]
        px, ok = rr.project(model, k, R, t, p)
        assert ok.all()
        pts.append(p)
        pix.append(px + 0.1 * rng.standard_normal(px.shape))
        used.append((R, t))
    return k, counts, pts, pix


def _batch(pts, pix, frames):
    off = np.concatenate([[0], np.cumsum([len(pts[f]) for f in frames])]).astype(np.int64)
    return off, np.concatenate([pix[f] for f in frames]).reshape(-1, 2), np.concatenate([pts[f] for f in frames]).reshape(-1, 3)


@pytest.mark.parametrize("model", (1, 4))
def test_ragged_batch(api, model):
    k, counts, pts, pix = _ragged(model)
    every = list(range(len(counts)))
    whole = _capi.camera_resect(api, model, k, *_batch(pts, pix, every), covariance=True)
    for f, c in enumerate(counts):
        if c < 4:
            assert whole.status[f] == _capi.RESECT_TOO_FEW_POINTS and whole.iterations[f] == 0
            _zeroed(whole, f)
            continue
        assert whole.status[f] == _capi.RESECT_OK and whole.n_used[f] == c, (f, whole.status[f], whole.n_used[f])
        step = rr.criterion(model, k, whole.q[f], whole.t[f], pts[f], pix[f])
        print("model", model, "pairs", c, "reference step", step, "iterations", whole.iterations[f])
        assert step <= BOUND
    singles = [_capi.camera_resect(api, model, k, *_batch(pts, pix, [f]), covariance=True) for f in every]
    for f in every:      # a frame's result depends neither on the other frames of the call nor on its position
        _same(whole, singles[f], [f], [0])
    order = [8, 0, 2, 3, 6]
    for n in (1, W, W + 1):
        part = _capi.camera_resect(api, model, k, *_batch(pts, pix, order[:n]), covariance=True)
        for i, f in enumerate(order[:n]):
            _same(part, singles[f], [i], [0])
    # the host's passes: chunks of whole frames (at most 100 pairs, a larger frame alone)
    _same(whole, _capi.camera_resect(api, model, k, *_batch(pts, pix, every), covariance=True, chunk=100))


def test_two_calls_are_bit_identical(api):
    k, off, px, pt, _ = rr.fixture(7, 0.1)
    o = _capi.resection_options(api, huber_scale=0.15)
    a = _capi.camera_resect(api, 7, k, off, px, pt, options=o, covariance=True)
    b = _capi.camera_resect(api, 7, k, off, px, pt, options=o, covariance=True)
    assert (a.status == _capi.RESECT_OK).all()
    _same(a, b)


@pytest.mark.parametrize("model", rr.MODELS)
def test_chart_origin_does_not_matter(api, model):
    """Points shifted by (3, -2, 0) with the pose compensated: R p + t = R (p + s) + (t - R s). Catches a start that assumes a
    centred chart."""
    k, off, px, pt, poses = rr.fixture(model, 0.0)
    s = np.array([3.0, -2.0, 0.0])
    r = _capi.camera_resect(api, model, k, off, px, pt + s)
    assert (r.status == _capi.RESECT_OK).all(), r.status
    dist = [rr.pose_distance(rr.rot(r.q[f]), r.t[f] + rr.rot(r.q[f]) @ s, *poses[f]) for f in range(len(poses))]
    print("model", model, "distance to the truth", max(dist))
    assert max(dist) <= FREE_BOUND


@pytest.mark.parametrize("model", (4, 6, 7))
def test_wide_angle_uses_points_behind_the_image_plane(api, model):
    k, px, pts, ok, R, t = rr.wide_angle(model)
    assert ok.sum() == 121 and ((pts @ R.T + t)[:, 2] <= 0).sum() == 44
    pix = px + 0.1 * np.random.default_rng(5).standard_normal(px.shape)
    r = _capi.camera_resect(api, model, k, [0, len(pts)], pix, pts)
    assert r.status[0] == _capi.RESECT_OK, r.status
    Rd = rr.rot(r.q[0])
    behind = ((pts @ Rd.T + r.t[0])[:, 2] <= 0).sum()
    step = rr.criterion(model, k, r.q[0], r.t[0], pts, pix)
    print("model", model, "used", r.n_used[0], "behind the image plane", behind, "reference step", step, "iterations", r.iterations[0])
    assert r.n_used[0] == rr.rms_at(model, k, r.q[0], r.t[0], pts, pix)[1] == 121
    assert behind >= 1
    assert step <= BOUND
    assert rr.pose_distance(Rd, r.t[0], R, t) < 1e-2      # (it is the pose the pixels were made at, not another minimum)


@pytest.mark.parametrize("model", (1, 3, 7))
def test_warm_start_takes_a_chart_that_is_not_planar(api, model):
    k, off, px, pt, poses = rr.fixture(model, 0.0)
    f = 5
    pts = pt[off[f]:off[f + 1]].copy()
    pts[:, 2] = 0.1 * (-1.0) ** np.arange(len(pts))
    R, t = poses[f]
    pix, ok = rr.project(model, k, R, t, pts)
    assert ok.all()
    pix = pix + 0.1 * np.random.default_rng(9).standard_normal(pix.shape)
    cold = _capi.camera_resect(api, model, k, [0, len(pts)], pix, pts, covariance=True)
    assert cold.status[0] == _capi.RESECT_NO_START
    _zeroed(cold, 0)
    q0 = rr.quat_of(rr.exp_so3(np.deg2rad(2.0) * np.array([0.6, -0.64, 0.48])) @ R)
    t0 = t + 0.02 * np.array([0.48, 0.6, -0.64])
    warm = _capi.camera_resect(api, model, k, [0, len(pts)], pix, pts, q_init=q0[None], t_init=t0[None])
    assert warm.status[0] == _capi.RESECT_OK and warm.n_used[0] == len(pts)
    step = rr.criterion(model, k, warm.q[0], warm.t[0], pts, pix)
    print("model", model, "reference step", step, "iterations", warm.iterations[0])
    assert step <= BOUND


@pytest.mark.parametrize("model", (1, 6))
def test_huber_loss_resists_displaced_pixels(api, model):
    k = np.array(syn._TRUE_INTRINSICS[model], float)
    pts = syn.aprilgrid_points()
    R, t = rr.true_poses()[3]
    pix, ok = rr.project(model, k, R, t, pts)
    assert ok.all()
    rng = np.random.default_rng(21)
    pix = pix + 0.1 * rng.standard_normal(pix.shape)
    bad = rng.choice(len(pts), 7, replace=False)
    ang = rng.uniform(0, 2 * np.pi, 7)
    pix[bad] += np.linspace(5.0, 50.0, 7)[:, None] * np.c_[np.cos(ang), np.sin(ang)]
    res = {}
    for scale in (1.0, 0.0):
        r = _capi.camera_resect(api, model, k, [0, len(pts)], pix, pts, options=_capi.resection_options(api, huber_scale=scale))
        assert r.status[0] == _capi.RESECT_OK and r.n_used[0] == 144
        step = rr.criterion(model, k, r.q[0], r.t[0], pts, pix, huber=scale)
        res[scale] = rr.pose_distance(rr.rot(r.q[0]), r.t[0], R, t)
        print("model", model, "huber", scale, "reference step", step, "distance to the truth", res[scale])
        if scale > 0:      # (without the loss the 50 px residuals lift the reference's own difference error above its FLOOR)
            assert step <= BOUND
    assert res[1.0] < res[0.0]


@pytest.mark.parametrize("model", rr.MODELS)
def test_covariance_is_the_inverse_of_the_normal_matrix(api, model):
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    r = _capi.camera_resect(api, model, k, off, px, pt, covariance=True)
    assert (r.status == _capi.RESECT_OK).all()
    worst = 0.0
    for f in (0, 4, 9, 13, 19):
        s = slice(off[f], off[f + 1])
        Rd = rr.rot(r.q[f])
        C1 = np.linalg.inv(rr.system(model, k, Rd, r.t[f], pt[s], px[s])[0])
        C2 = np.linalg.inv(rr.system(model, k, Rd, r.t[f], pt[s], px[s], h=2e-6)[0])
        agree = np.abs(C1 - C2).max() / np.abs(C1).max()
        err = np.abs(r.cov[f] - C1).max() / np.abs(C1).max()
        worst = max(worst, err / agree)
        print("model", model, "frame", f, "reference's own agreement", agree, "device against reference", err)
        assert np.array_equal(r.cov[f], r.cov[f].T)
        assert err <= 10 * agree
