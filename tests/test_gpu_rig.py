"""Rig calibration on the device (calico_rig_calibrate) against the numpy reference of rig_ref.py.

The optimality criterion: the reference's UNDAMPED Gauss-Newton step at the DEVICE's estimate has
s <= step_tolerance + 10 FLOOR[fixture] (s: rig_ref.step_size, the library's step size): the device stops after a step below
step_tolerance = 1e-10 taken at low damping, Gauss-Newton contracts from there, and 10 FLOOR covers the reference's own difference
quotients (FLOOR: tests/test_rig_host.py measures it).
Noise-free bound: max(100 x the reference's own distance to the truth from the same start, 1e-9); the reference's distance is at
most 1.4e-15 (REF_FREE, measured in tests/test_rig_host.py), so the bound is 1e-9.
Covariance bound: 10 x the relative agreement of the reference's reduced-system inverse from h = 1e-6 and h = 2e-6 differences at
the device's estimate, computed in the test.
Measured on an MI355X, 0.1 px noise: the reference's s at the device's estimate 6.0e-14 (standard, 11 iterations from the perturbed
start; 6.0e-14 and 4 iterations with no start given), 1.3e-13 (chain, no start), 6.5e-14 (chain with camera 0 unconnected), 8.5e-14
(wide, 7 iterations), 3.4e-13 (long views); noise-free distance to the truth 5.7e-16, rms 7.5e-13 px; the covariance within 5.9e-11 of
the reference where the reference agrees with itself to 6.5e-11; Huber: the extrinsics 3.9e-5 from the truth against 1.8e-3."""
import numpy as np
import pytest

import resect_ref as rr
import rig_ref as gr
from calico_amd import _capi

pytestmark = pytest.mark.gpu

TOL = 1e-10
ARRAYS = ("q_rig_camera", "t_rig_camera", "camera_status", "q_frame", "t_frame", "frame_status", "view_rms", "view_n_used", "view_status", "cov")
FIELDS = ("status", "iterations", "initial_cost", "final_cost", "total_rms", "cameras_used", "frames_used", "views_used", "pairs_used", "lambda_")


def bound(name):
    return TOL + 10 * gr.FLOOR[name]


@pytest.fixture(scope="module")
def api(hip):
    return hip


def _call(api, rig, start=None, views=None, n_frames=None, **kw):
    """The call on the rig's views (or on `views`: (camera, frame, offsets, pixels, points)), from `start` (q_cam, t_cam, q_frame,
    t_frame) or from none, with the covariance; the remaining keywords are options."""
    vc, vf, off, px, pt = (rig.view_camera, rig.view_frame, rig.view_offsets, rig.pixels, rig.points) if views is None else views
    names = ("q_rig_camera_init", "t_rig_camera_init", "q_frame_init", "t_frame_init")
    init = {} if start is None else dict(zip(names, start))
    return _capi.rig_calibrate(api, rig.models, rig.ks, rig.n_frames if n_frames is None else n_frames, vc, vf, off, px, pt,
                               options=_capi.rig_options(api, **kw) if kw else None, covariance=True, **init)


_RUNS = {}


def _started(api, name, noise):
    """The call from the truth perturbed by 0.02 N(0, 1), once per (fixture, noise) and module."""
    if (name, noise) not in _RUNS:
        rig = gr.FIXTURES[name](noise)
        _RUNS[(name, noise)] = _call(api, rig, gr.perturbed_start(rig))
    return _RUNS[(name, noise)]


def _criterion(rig, r, use=None, held=None, huber=0.0):
    return gr.criterion(rig, r.q_rig_camera, r.t_rig_camera, r.q_frame, r.t_frame, use, held, huber)


def _same(a, b):
    for name in ARRAYS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    for name in FIELDS:
        assert getattr(a, name) == getattr(b, name), name


def test_noisy_standard_fixture_meets_the_optimality_criterion(api):
    rig = gr.standard(0.1)
    r = _started(api, "standard", 0.1)
    assert r.status == _capi.RIG_OK and (r.frames_used, r.views_used, r.pairs_used, r.cameras_used) == (20, 60, 2160, 3)
    assert r.camera_status.tolist() == [_capi.RIG_CAMERA_REFERENCE, _capi.RIG_CAMERA_OK, _capi.RIG_CAMERA_OK]
    assert (r.frame_status == _capi.RIG_FRAME_OK).all() and (r.view_status == _capi.RESECT_OK).all() and (r.view_n_used == 36).all()
    s = _criterion(rig, r)
    rms, n, per = gr.rms_at(rig, r.q_rig_camera, r.t_rig_camera, r.q_frame, r.t_frame)
    print("reference step at the device's estimate", s, "bound", bound("standard"), "iterations", r.iterations, "rms", r.total_rms, "lambda", r.lambda_)
    assert s <= bound("standard")
    assert n == 2160 and abs(r.total_rms - rms) <= 1e-9 * rms, (r.total_rms, rms)
    for v in (0, 31, 59):
        assert abs(r.view_rms[v] - per[v]) <= 1e-9 * per[v], v
    assert r.final_cost < r.initial_cost and abs(r.final_cost - 2160 * rms * rms) <= 1e-9 * r.final_cost
    assert (np.abs(np.linalg.norm(r.q_rig_camera, axis=1) - 1) < 1e-15).all() and (r.q_rig_camera[:, 3] >= 0).all() and (r.q_frame[:, 3] >= 0).all()


def test_noise_free_standard_fixture_recovers_the_truth(api):
    rig = gr.standard(0.0)
    r = _started(api, "standard", 0.0)
    assert r.status == _capi.RIG_OK and r.frames_used == 20
    dist = gr.distance(gr.poses_of(r.q_rig_camera, r.t_rig_camera), gr.poses_of(r.q_frame, r.t_frame), rig)
    limit = max(100 * gr.REF_FREE["standard"], 1e-9)
    print("distance to the truth", dist, "bound", limit, "iterations", r.iterations, "rms", r.total_rms)
    assert dist <= limit and r.total_rms <= 1e-9


def test_no_start_standard_fixture(api):
    rig = gr.standard(0.1)
    r = _call(api, rig)
    assert r.status == _capi.RIG_OK and (r.frames_used, r.views_used, r.pairs_used) == (20, 60, 2160)
    assert np.array_equal(r.q_rig_camera[0], [0, 0, 0, 1]) and not r.t_rig_camera[0].any()
    s = _criterion(rig, r)
    print("no start: reference step", s, "iterations", r.iterations)
    assert s <= bound("standard")


def test_no_start_chain_fixture_reaches_camera_2_through_camera_1(api):
    rig = gr.chain(0.1)
    r = _call(api, rig)
    assert r.status == _capi.RIG_OK and r.views_used == len(rig.view_camera) == 42 and r.frames_used == 20
    assert r.camera_status.tolist() == [_capi.RIG_CAMERA_REFERENCE, _capi.RIG_CAMERA_OK, _capi.RIG_CAMERA_OK]
    assert (r.frame_status == _capi.RIG_FRAME_OK).all()      # (frames 10-19: camera 0 never saw them)
    s = _criterion(rig, r)
    print("chain: reference step", s, "iterations", r.iterations)
    assert s <= bound("chain")


def test_no_start_chain_fixture_with_an_unconnected_camera(api):
    """The chain's cameras share 10 (0 and 1), 12 (1 and 2) and 2 (0 and 2) frames. With min_shared_frames = 13 no pair of cameras
    is connected (cameras 0 and 1 share ten frames only, so camera 1 does not join the reference either): TOO_FEW_VIEWS, the
    outputs are the starts. A camera that is left out while the others go on needs a threshold between two of the counts: with
    camera 1 as the reference and min_shared_frames = 11, camera 2 joins (12 frames) and camera 0 does not (10): it is
    UNCONNECTED, its views are left out, its output is the identity, and the criterion holds on what remains."""
    rig = gr.chain(0.1)
    r = _call(api, rig, min_shared_frames=13)
    assert r.status == _capi.RIG_TOO_FEW_VIEWS and r.iterations == 0 and r.cameras_used == 1
    assert r.camera_status.tolist() == [_capi.RIG_CAMERA_REFERENCE, _capi.RIG_CAMERA_UNCONNECTED, _capi.RIG_CAMERA_UNCONNECTED]
    assert np.array_equal(r.q_rig_camera, np.tile([0.0, 0, 0, 1], (3, 1))) and not r.t_rig_camera.any() and not r.cov.any()
    r = _call(api, rig, min_shared_frames=11, reference_camera=1)
    use = rig.view_camera != 0
    assert r.status == _capi.RIG_OK and r.views_used == use.sum() == 32 and r.cameras_used == 2 and r.frames_used == 20
    assert r.camera_status.tolist() == [_capi.RIG_CAMERA_UNCONNECTED, _capi.RIG_CAMERA_REFERENCE, _capi.RIG_CAMERA_OK]
    for c in (0, 1):
        assert np.array_equal(r.q_rig_camera[c], [0, 0, 0, 1]) and not r.t_rig_camera[c].any()
    assert not r.view_rms[~use].any() and not r.view_n_used[~use].any() and (r.view_n_used[use] == 36).all()
    assert (r.view_status == _capi.RESECT_OK).all()      # (the views that are left out keep their resection's status)
    assert not r.cov[:12, :].any() and not r.cov[:, :12].any() and (np.diag(r.cov)[12:] > 0).all()
    s = _criterion(rig, r, use=use, held={0, 1})
    print("chain without camera 0: reference step", s, "iterations", r.iterations)
    assert s <= bound("chain")


def test_wide_fixture_runs_eight_cameras_of_every_model(api):
    rig = gr.wide(0.1)
    start = [a.copy() for a in gr.perturbed_start(rig)]
    start[0][0] = [0.0, 0.0, 0.0, 2.0]      # the reference camera's start is not normalised: it comes back as given
    r = _call(api, rig, tuple(start))
    assert r.status == _capi.RIG_OK and (r.frames_used, r.views_used, r.pairs_used, r.cameras_used) == (6, 47, 47 * 36, 8)
    assert r.q_rig_camera[0].tobytes() == start[0][0].tobytes() and r.t_rig_camera[0].tobytes() == start[1][0].tobytes()
    s = _criterion(rig, r)
    print("wide: reference step", s, "iterations", r.iterations, "rms", r.total_rms)
    assert s <= bound("wide")
    assert np.array_equal(r.cov, r.cov.T) or np.abs(r.cov - r.cov.T).max() <= 1e-12 * np.abs(r.cov).max()
    assert not r.cov[:6, :].any() and not r.cov[:, :6].any() and (np.diag(r.cov)[6:] > 0).all()


def test_long_views_cross_the_trips_of_64_pairs(api):
    rig = gr.long_views(0.1)
    r = _started(api, "long", 0.1)
    assert r.status == _capi.RIG_OK and (r.views_used, r.pairs_used) == (12, 12 * 144) and (r.view_n_used == 144).all()
    s = _criterion(rig, r)
    print("long views: reference step", s, "iterations", r.iterations)
    assert s <= bound("long")


def test_covariance_of_the_extrinsics(api):
    rig = gr.standard(0.1)
    r = _started(api, "standard", 0.1)
    est = (r.q_rig_camera, r.t_rig_camera, r.q_frame, r.t_frame)
    ref, ref2 = gr.reduced_covariance(rig, *est), gr.reduced_covariance(rig, *est, h=2e-6)
    agree = np.abs(ref - ref2).max() / np.abs(ref).max()
    got = np.abs(r.cov - ref).max() / np.abs(ref).max()
    print("covariance: device within", got, "of the reference; the reference agrees with itself to", agree)
    assert got <= 10 * agree
    assert not r.cov[:6, :].any() and not r.cov[:, :6].any() and (np.diag(r.cov)[6:] > 0).all()


def test_huber_loss_resists_displaced_pixels(api):
    rig = gr.standard(0.1)
    rng = np.random.default_rng(777)
    px = rig.pixels.copy()
    hit = rng.choice(len(px), len(px) // 20, replace=False)
    ang = rng.uniform(0, 2 * np.pi, len(hit))
    px[hit] += 30.0 * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    views = (rig.view_camera, rig.view_frame, rig.view_offsets, px, rig.points)
    start = gr.perturbed_start(rig)
    plain, robust = _call(api, rig, start, views), _call(api, rig, start, views, huber_scale=1.0)
    assert plain.status == robust.status == _capi.RIG_OK

    def dist(r):
        return max(rr.pose_distance(*p, *t) for p, t in zip(gr.poses_of(r.q_rig_camera, r.t_rig_camera)[1:], rig.cams[1:]))
    print("extrinsics' distance to the truth: plain", dist(plain), "huber", dist(robust))
    assert dist(robust) < dist(plain)


def test_permuted_views_and_a_second_call_are_bit_identical(api):
    rig = gr.standard(0.1)
    first = _call(api, rig)
    _same(first, _call(api, rig))
    perm = np.random.default_rng(5).permutation(len(rig.view_camera))
    off = rig.view_offsets
    counts = (off[1:] - off[:-1])[perm]
    rows = np.concatenate([np.arange(off[v], off[v + 1]) for v in perm])
    views = (rig.view_camera[perm], rig.view_frame[perm], np.concatenate([[0], np.cumsum(counts)]), rig.pixels[rows], rig.points[rows])
    other = _call(api, rig, None, views)
    for name in ARRAYS:
        a, b = getattr(first, name), getattr(other, name)
        assert (a[perm] if name.startswith("view_") else a).tobytes() == b.tobytes(), name
    for name in FIELDS:
        assert getattr(first, name) == getattr(other, name), name
    # with a start too
    start = gr.perturbed_start(rig)
    _same(_started(api, "standard", 0.1), _call(api, rig, start))


def test_one_iteration_is_not_converged_with_a_finite_point(api):
    rig = gr.standard(0.1)
    r = _call(api, rig, gr.perturbed_start(rig), max_iterations=1)
    assert r.status == _capi.RIG_NOT_CONVERGED and r.iterations == 1
    for name in ("q_rig_camera", "t_rig_camera", "q_frame", "t_frame", "view_rms", "cov"):
        assert np.isfinite(getattr(r, name)).all(), name
    assert np.isfinite(r.final_cost) and r.final_cost <= r.initial_cost and r.views_used == 60


def test_a_frame_whose_only_view_is_too_small_takes_no_part(api):
    rig = gr.standard(0.1)
    vc = np.concatenate([rig.view_camera, [1]]).astype(np.int32)
    vf = np.concatenate([rig.view_frame, [20]])
    off = np.concatenate([rig.view_offsets, [rig.view_offsets[-1] + 3]])
    px, pt = np.concatenate([rig.pixels, rig.pixels[36:39]]), np.concatenate([rig.points, rig.points[36:39]])
    whole = _call(api, rig, None, (vc, vf, off, px, pt), n_frames=21)
    clean = _call(api, rig)
    assert whole.status == clean.status == _capi.RIG_OK
    assert whole.frame_status[20] == _capi.RIG_FRAME_NO_VIEW and whole.view_status[60] == _capi.RESECT_TOO_FEW_POINTS
    assert whole.view_n_used[60] == 0 and whole.view_rms[60] == 0.0
    assert (whole.frames_used, whole.views_used, whole.pairs_used) == (20, 60, 2160)
    for name in ARRAYS:
        a, b = getattr(whole, name), getattr(clean, name)
        assert a[:len(b)].tobytes() == b.tobytes(), name
    for name in FIELDS:
        assert getattr(whole, name) == getattr(clean, name), name
