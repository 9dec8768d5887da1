"""calico_camera_align on the device against the numpy reference (camera_align_ref.py), the truth, and the optimiser itself.

The yardsticks are the reference's own, measured by test_camera_align_host.py: FLOOR (its criterion -- the scaled size of one
undamped Gauss-Newton step -- at and after its own result on the noisy standard fixture), REF_FREE (its distance to the truth on
noise-free data) and CURVE_LEVEL (what the score curve moves by when the resection starts elsewhere). The house rule of
test_gpu_rig.py: criterion <= step_tolerance + 10 FLOOR, noise-free distance <= max(100 REF_FREE, 1e-9), covariance <= 1e-6
relative against the reference's, the score curve to 10 CURVE_LEVEL.

What the noise-free checks do and do not show: the fixtures' pixels come from the reference's own model (the spline segment of the
STAMP, as the optimiser takes it). "Recovers the truth" is a check of the device against the model it shares with the reference.
What stands outside that model: the reference is pinned on the ORACLE's evaluate (test_camera_align_host.py), the device's result
is checked by the optimiser's own gradient here (calico_evaluate on the device), and the last test runs the optimiser from the
aligned start on a scene whose data are synthetic.project_camera's (the true time's segment).

The grid always has an odd number of latencies (2 half + 1), so 64 cannot occur: 63 and 65 straddle the eight-lag tiles and the
64th lag, 3 is the smallest grid with an interior.

Measured on an MI355X (printed by the tests), first run: noise-free distance to the truth 9.1e-16 after 2 iterations; noisy
standard fixture: criterion 2.2e-15 after 3 iterations, 2.7e-15 from the reference's estimate, covariance 1.2e-11 relative, score
curve 5.8e-15 from the reference's (bound 5.6e-14); by the optimiser's own system (calico_evaluate): step 8.7e-16, cost equal to
1e-13 relative, covariance 1.5e-14; the shape cases: criterion 5.7e-16 to 3.7e-13 (the largest with held parameters), covariance
2.8e-12 to 5.3e-11; every camera model on 9 frames of 16 points: 1.5e-14 to 8.5e-14; Huber with 2 % outliers: 2.9e-15, 1.7e-15
from the reference's estimate; a rig at rest: a curve of 1.0210302284e-07 whose range is 5e-18."""
import dataclasses

import numpy as np
import pytest

import camera_align_ref as cref
import helpers
from calico_amd import _capi, synthetic as syn

pytestmark = pytest.mark.gpu

STEP_TOLERANCE = 1e-10
CRITERION_BOUND = STEP_TOLERANCE + 10 * cref.FLOOR
FREE_BOUND = max(100 * cref.REF_FREE, 1e-9)
CURVE_BOUND = 10 * cref.CURVE_LEVEL


@pytest.fixture(scope="module")
def api():
    return helpers.hip_api()


def device(api, fx, **kw):
    extra = {k: kw.pop(k) for k in ("q_init", "t_init", "latency_init") if k in kw}
    return _capi.camera_align(api, *cref.call_args(fx), options=_capi.camera_alignment_options(api, **kw), covariance=True, curve=True, **extra)


def took_part(r):
    return r["frame_status"] == cref.RESECT_OK


def check_minimum(fx, r, free=np.ones(7, bool), huber=0.0, sigma=1.0, what=""):
    """The device's estimate is a minimum by the reference's criterion over the frames the device used, and its covariance the
    reference's there."""
    frames = took_part(r)
    est = cref.estimate(r)
    crit = cref.criterion(fx, est, free, sigma, huber, frames)
    cov = cref.covariance(fx, est, free, sigma, huber, frames)
    cov_err = np.abs(r["cov"] - cov).max() / np.abs(cov).max()
    print(what, "criterion", crit, "covariance against the reference", cov_err, "iterations", r["iterations"], "frames", int(frames.sum()))
    assert crit <= CRITERION_BOUND, (what, crit)
    assert cov_err <= 1e-6, (what, cov_err)
    return crit


@pytest.fixture(scope="module")
def noisy(api):
    """The noisy standard fixture: the data, the reference's result, the device's."""
    fx = cref.fixture(noise=0.1)
    return fx, cref.align(fx, **cref.OPTIONS), device(api, fx, **cref.OPTIONS)


def test_noise_free_standard_fixture_recovers_the_truth(api):
    fx = cref.fixture(noise=0.0)
    ref = cref.align(fx, **cref.OPTIONS)
    r = device(api, fx, **cref.OPTIONS)
    assert (r["status"], r["frames_used"], r["n_lags"]) == (_capi.ALIGN_OK, 132, 41) and took_part(r).all()
    dist = cref.distance_to_truth(cref.estimate(r), fx["truth"])
    print("device distance to the truth", dist, "iterations", r["iterations"], "rms", r["rms"], "peak", r["peak_index"], "coarse", r["coarse_latency"])
    assert dist <= FREE_BOUND
    assert r["peak_index"] == ref["peak_index"] == 25
    assert r["rms"] <= 1e-9 and r["pairs_used"] == ref["pairs_used"] == fx["offsets"][-1]


def test_noisy_standard_fixture_is_a_minimum_by_the_references_criterion(noisy):
    fx, ref, r = noisy
    assert r["status"] == _capi.ALIGN_OK and ref["status"] == cref.OK
    assert np.array_equal(r["frame_status"], ref["frame_status"]) and r["frames_used"] == ref["frames_used"] == 132
    check_minimum(fx, r, what="noisy standard fixture:")
    ref_est = dict(q=ref["q_rig_camera"], t=ref["t_rig_camera"], latency=ref["latency"])
    print("distance to the reference", cref.distance_to_truth(cref.estimate(r), ref_est), "to the truth", cref.distance_to_truth(cref.estimate(r), fx["truth"]))
    assert cref.distance_to_truth(cref.estimate(r), ref_est) <= 1e-8
    assert r["peak_index"] == ref["peak_index"] == 25
    curve_err = np.abs(r["curve"] - ref["curve"]).max()
    print("curve against the reference", curve_err, "bound", CURVE_BOUND, "coarse latency", r["coarse_latency"], ref["coarse_latency"])
    assert curve_err <= CURVE_BOUND
    assert abs(r["coarse_latency"] - ref["coarse_latency"]) <= 1e-9 and abs(r["peak_score"] - ref["curve"][25]) <= CURVE_BOUND
    assert np.isnan(r["curve_tail"]).all()
    assert abs(r["rms"] - ref["rms"]) <= 1e-9 * ref["rms"] and abs(r["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
    assert np.array_equal(r["frame_n_used"], ref["frame_n_used"]) and np.abs(r["frame_rms"] - ref["frame_rms"]).max() <= 1e-8
    assert r["final_cost"] <= r["initial_cost"] and r["pairs_used"] == ref["pairs_used"]


def test_result_is_a_minimum_of_the_optimisers_own_camera_term(api):
    """The device's estimate loaded into a problem with that camera (calico_evaluate on the device): the optimiser's cost is the
    reported one, and the Gauss-Newton step of ITS gradient and J^T J in (q, t, latency) is within the bound. A slip in a sign or in
    the direction of time shows here: the step would be the size of the estimate."""
    fx = cref.fixture(noise=0.1)
    sigma = 0.1
    r = device(api, fx, sigma_pixel=sigma, **cref.OPTIONS)
    assert r["status"] == _capi.ALIGN_OK
    est = cref.estimate(r)
    P, columns = cref.camera_problem(api, fx, est, sigma, took_part(r), constant_ctrl=False)
    cost, step, H = cref.oracle_step(P, columns, est)
    print("optimiser cost", cost, "final_cost", r["final_cost"], "Gauss-Newton step of the optimiser's own system", step)
    assert abs(cost - r["final_cost"]) <= 1e-12 * cost
    assert step <= CRITERION_BOUND
    cov = np.linalg.inv(H)
    cov_err = np.abs(r["cov"] - cov).max() / np.abs(cov).max()
    print("covariance against the optimiser's (J^T J)^-1", cov_err)
    assert cov_err <= 1e-6


def dense_fixture(counts, noise=0.1, times=None, latency=None, seed=3):
    """Frames with the given numbers of pairs (cycled): a dense small chart (13 x 13 points over 0.48 m, shuffled), of which frame
    f keeps the first counts[f % len(counts)] of the pairs it sees (all of them where it sees fewer: the chart leaves the image
    when the rig turns away); every count occurs."""
    g = np.linspace(-0.24, 0.24, 13)
    pts = np.array([[x, y, 0.0] for x in g for y in g])
    pts = pts[np.random.default_rng(seed).permutation(len(pts))]
    fx = cref.fixture(noise=noise, points=pts, times=times, latency=latency)
    off = fx["offsets"]
    keep, new_off = [], [0]
    for f in range(len(off) - 1):
        n = min(counts[f % len(counts)], off[f + 1] - off[f])
        keep.append(np.arange(off[f], off[f] + n))
        new_off.append(new_off[-1] + n)
    keep = np.concatenate(keep).astype(np.int64)
    fx["offsets"], fx["pixels"], fx["points"] = np.array(new_off, np.int64), fx["pixels"][keep], fx["points"][keep]
    assert set(counts) <= set(np.diff(fx["offsets"]).tolist())
    return fx


def test_pairs_per_frame_across_the_trip_of_64(api):
    """3 pairs (dropped), 4, 63, 64, 65 and 129 pairs per frame, and a frame without pairs in the middle."""
    counts = [3, 4, 63, 64, 65, 129, 0, 16]
    fx = dense_fixture(counts)
    r = device(api, fx, **cref.OPTIONS)
    n = np.diff(fx["offsets"])
    assert r["status"] == _capi.ALIGN_OK
    assert np.array_equal(r["frame_status"][n < 4], np.full(int((n < 4).sum()), cref.RESECT_TOO_FEW_POINTS))
    assert (r["frame_status"][n >= 4] == cref.RESECT_OK).all() and r["frames_used"] == int((n >= 4).sum())
    assert np.array_equal(r["frame_n_used"], np.where(n >= 4, n, 0)) and not r["frame_rms"][n < 4].any() and (r["frame_rms"][n >= 4] > 0).all()
    check_minimum(fx, r, what="pairs per frame %s:" % counts)
    assert cref.distance_to_truth(cref.estimate(r), fx["truth"]) < 1e-3


@pytest.mark.parametrize("n_frames", [7, 8, 9, 257])
def test_frame_counts(api, n_frames):
    fx = dense_fixture([12], times=0.3 + 6.6 * np.arange(n_frames) / n_frames)
    r = device(api, fx, **cref.OPTIONS)
    if n_frames < 8:
        assert r["status"] == _capi.ALIGN_TOO_FEW_SAMPLES and r["frames_used"] == n_frames and r["n_lags"] == 0
        assert np.array_equal(r["q_rig_camera"], [0, 0, 0, 1]) and not r["t_rig_camera"].any() and r["latency"] == 0.0 and not r["cov"].any()
        return
    assert r["status"] == _capi.ALIGN_OK and r["frames_used"] == n_frames
    check_minimum(fx, r, what="%d frames:" % n_frames)


@pytest.mark.parametrize("half,lag_step,latency", [(1, 0.01, 0.002), (31, 0.001, 0.0137), (32, 0.001, 0.0137)])
def test_lag_counts(api, half, lag_step, latency):
    fx = dense_fixture([12], latency=latency)
    opts = dict(max_lag=half * lag_step, lag_step=lag_step)
    ref = cref.align(fx, **opts)
    r = device(api, fx, **opts)
    assert r["n_lags"] == 2 * half + 1 == len(r["curve"]) and r["status"] == _capi.ALIGN_OK == ref["status"]
    assert r["peak_index"] == ref["peak_index"] and np.abs(r["curve"] - ref["curve"]).max() <= CURVE_BOUND
    check_minimum(fx, r, what="%d lags:" % (2 * half + 1))


def test_frames_outside_the_knots_at_each_end(api):
    lo, hi = cref.iref.valid_range(cref.iref.trajectory())
    times = np.concatenate([[lo - 0.2, lo + 0.01], 0.3 + 0.05 * np.arange(100), [hi - 0.03, hi + 0.1]])
    fx = dense_fixture([12], times=np.clip(times, lo, hi - 0.0137))      # (the pixels of the outer frames play no part)
    fx["stamps"] = times + 0.0137
    r = device(api, fx, **cref.OPTIONS)
    ref = cref.align(fx, **cref.OPTIONS)
    outside = [0, 1, len(times) - 2, len(times) - 1]
    assert r["status"] == _capi.ALIGN_OK and np.array_equal(r["frame_status"], ref["frame_status"])
    assert (r["frame_status"][outside] == _capi.CAMERA_ALIGN_FRAME_OUTSIDE).all() and r["frames_used"] == 100
    assert not r["frame_rms"][outside].any() and not r["frame_n_used"][outside].any()
    check_minimum(fx, r, what="frames outside:")


def test_held_parameters(noisy):
    fx, ref, full = noisy
    api = helpers.hip_api()
    tr = fx["truth"]
    start = dict(q_init=-1.7 * cref.apply((tr["q"], tr["t"], 0.0), np.array([0.01, -0.02, 0.01, 0, 0, 0, 0]))[0], t_init=tr["t"] + [0.01, 0.0, -0.01],
                 latency_init=0.01)
    for hold, free in (("estimate_latency", [1, 1, 1, 1, 1, 1, 0]), ("estimate_translation", [1, 1, 1, 0, 0, 0, 1])):
        r = device(api, fx, **{hold: 0}, **start, **cref.OPTIONS)
        free = np.array(free, bool)
        assert r["status"] == _capi.ALIGN_OK and r["n_lags"] == 0 and r["peak_index"] == -1 and r["curve"].size == 0
        assert not r["cov"][~free].any() and not r["cov"][:, ~free].any() and (np.diag(r["cov"])[free] > 0).all()
        if hold == "estimate_latency":
            assert r["latency"] == 0.01 and not np.array_equal(r["t_rig_camera"], start["t_init"])
        else:
            assert np.array_equal(r["t_rig_camera"], start["t_init"]) and r["latency"] != 0.01
        check_minimum(fx, r, free, what="held (%s = 0):" % hold)
    # without a start: the latency is held at 0 and no search runs; the translation is held at 0
    r = device(api, fx, estimate_latency=0, **cref.OPTIONS)
    assert r["status"] == _capi.ALIGN_OK and r["latency"] == 0.0 and r["n_lags"] == 0
    check_minimum(fx, r, np.array([1, 1, 1, 1, 1, 1, 0], bool), what="no search:")
    r = device(api, fx, estimate_translation=0, **cref.OPTIONS)
    assert r["status"] == _capi.ALIGN_OK and not r["t_rig_camera"].any() and r["n_lags"] == 41
    check_minimum(fx, r, np.array([1, 1, 1, 0, 0, 0, 1], bool), what="translation held at 0:")


def test_a_full_start_runs_no_resection_and_a_failed_resection_carries_its_status(api):
    fx = cref.fixture(noise=0.1)
    # frame 40: pixels that no pose explains (every pixel the same): the resection has no start for it
    a, b = fx["offsets"][40], fx["offsets"][41]
    fx["pixels"] = fx["pixels"].copy()
    fx["pixels"][a:b] = [640.0, 400.0]
    r = device(api, fx, **cref.OPTIONS)
    print("status of the frame whose resection fails", r["frame_status"][40], "frames used", r["frames_used"])
    assert r["status"] == _capi.ALIGN_OK and r["frame_status"][40] not in (cref.RESECT_OK, _capi.CAMERA_ALIGN_FRAME_OUTSIDE)
    assert r["frames_used"] == 131 and r["frame_n_used"][40] == 0 and r["frame_rms"][40] == 0.0
    check_minimum(fx, r, what="a frame dropped by the resection:")
    # with a full start no resection runs: the frame takes part, as the status says
    tr = fx["truth"]
    s = device(api, fx, q_init=tr["q"], t_init=tr["t"], latency_init=tr["latency"], huber_scale=1.0, **cref.OPTIONS)
    assert s["status"] == _capi.ALIGN_OK and s["frames_used"] == 132 and took_part(s).all() and s["n_lags"] == 0 and s["frame_n_used"][40] == b - a
    check_minimum(fx, s, huber=1.0, what="a full start:")


@pytest.mark.parametrize("model", range(1, 8))
def test_every_camera_model_on_a_tiny_case(api, model):
    """9 frames of 16 points."""
    g = np.linspace(-0.15, 0.15, 4)
    pts = np.array([[x, y, 0.0] for x in g for y in g])
    fx = cref.fixture(noise=0.1, model=model, points=pts, times=0.5 + 0.7 * np.arange(9))
    assert (np.diff(fx["offsets"]) == 16).all()
    ref = cref.align(fx, **cref.OPTIONS)
    r = device(api, fx, **cref.OPTIONS)
    assert r["status"] == _capi.ALIGN_OK == ref["status"] and r["frames_used"] == 9 and r["pairs_used"] == 144
    assert r["peak_index"] == ref["peak_index"]
    check_minimum(fx, r, what="model %d:" % model)


def test_huber_with_gross_outliers_against_the_reference(api):
    fx = cref.fixture(noise=0.1, outliers=0.02)
    opts = dict(huber_scale=0.5, **cref.OPTIONS)
    ref = cref.align(fx, **opts)
    r = device(api, fx, **opts)
    assert r["status"] == _capi.ALIGN_OK == ref["status"] and np.array_equal(r["frame_status"], ref["frame_status"])
    check_minimum(fx, r, huber=0.5, what="Huber, 2 % outliers:")
    ref_est = dict(q=ref["q_rig_camera"], t=ref["t_rig_camera"], latency=ref["latency"])
    print("distance to the reference", cref.distance_to_truth(cref.estimate(r), ref_est), "to the truth", cref.distance_to_truth(cref.estimate(r), fx["truth"]))
    assert cref.distance_to_truth(cref.estimate(r), ref_est) <= 1e-8 and abs(r["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
    assert cref.distance_to_truth(cref.estimate(r), fx["truth"]) < 1e-3 and r["rms"] > 1.0      # (the RMS carries no loss)


def test_a_rig_at_rest_and_a_latency_outside_the_grid_have_no_peak(api):
    for what, fx, opts in (("at rest", cref.fixture(noise=0.1, at_rest=True), cref.OPTIONS),
                           ("latency outside the grid", cref.fixture(noise=0.1, latency=0.04), dict(max_lag=0.02, lag_step=0.0025))):
        ref = cref.align(fx, **opts)
        r = device(api, fx, **opts)
        print(what, "peak", r["peak_index"], "curve", r["curve"].min(), "to", r["curve"].max())
        assert r["status"] == _capi.ALIGN_NO_PEAK == ref["status"], what
        assert np.array_equal(r["q_rig_camera"], [0, 0, 0, 1]) and not r["t_rig_camera"].any() and r["latency"] == 0.0 and not r["cov"].any()
        assert r["n_lags"] == len(ref["curve"]) and r["iterations"] == 0 and not r["frame_rms"].any() and not r["frame_n_used"].any()
        assert r["frames_used"] == 132
    assert r["peak_index"] == r["n_lags"] - 1


def test_two_calls_are_bit_identical(noisy):
    fx, _, first = noisy
    again = device(helpers.hip_api(), fx, **cref.OPTIONS)
    for key, v in first.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, again[key], equal_nan=True), key
        else:
            assert v == again[key], key


def test_unsynchronised_stamps(api):
    """Frame stamps that coincide with none of the trajectory's input poses (its poses come every 0.03 s from 0)."""
    times = 0.3 + 0.0517 * np.arange(120) + 0.0071
    stamps, _, _ = syn.default_synthetic_poses(segment_duration=0.3)
    assert np.abs((times + 0.0137)[:, None] - stamps[None, :]).min() > 1e-4
    fx = cref.fixture(noise=0.1, times=times)
    r = device(api, fx, **cref.OPTIONS)
    assert r["status"] == _capi.ALIGN_OK and r["frames_used"] == 120
    check_minimum(fx, r, what="unsynchronised:")
    assert cref.distance_to_truth(cref.estimate(r), fx["truth"]) < 1e-3


def _angle(a, b):
    d = syn.quat_mul(a, syn.quat_conj(b))
    return 2.0 * np.arctan2(np.linalg.norm(d[:3]), abs(d[3]))


def two_camera_scene():
    """helpers.small_scene with two cameras and no IMU, the second camera remounted at camera_align_ref.TRUTH (25 degrees from the
    rig frame, 13.7 ms late): its pixels are synthetic.project_camera's (the true time's segment) plus 0.1 pixel of noise, kept where
    a detector would return them. Both cameras' intrinsics are known; the second camera's extrinsics and latency are free."""
    scene = helpers.small_scene(n_cameras=2, imu=False, perturb=False)
    spl = (scene.knots, scene.basis, scene.ctrl_true, scene.order)
    tr = cref.TRUTH
    c0, c1 = scene.sensors[0], scene.sensors[1]
    times = np.unique(c0.stamps)
    times = times[times + 0.05 <= cref.iref.valid_range(spl)[1]]
    px, valid, st, frame, pidx = syn.project_camera(spl, c1.model, c1.intrinsics_true, tr["q"], tr["t"], tr["latency"], times, scene.points,
                                                    scene.body_q, scene.body_t)
    fx = dict(spl=spl, model=c1.model, k=c1.intrinsics_true, q_wm=scene.body_q, t_wm=scene.body_t, stamps=times + tr["latency"],
              offsets=np.arange(len(times) + 1, dtype=np.int64) * len(scene.points), points=np.tile(scene.points, (len(times), 1)))
    with np.errstate(all="ignore"):
        valid = valid & cref.detected(fx, (tr["q"], tr["t"], tr["latency"]), px)
    px = px + 0.1 * np.random.default_rng(17).standard_normal(px.shape)
    cam = dataclasses.replace(c1, intrinsics=c1.intrinsics_true.copy(), q=tr["q"].copy(), t=tr["t"].copy(), latency=tr["latency"], q_true=tr["q"],
                              t_true=tr["t"], latency_true=tr["latency"], enable_intrinsics=False, meas=px[valid], stamps=st[valid],
                              point_idx=pidx[valid].astype(np.int32), is_outlier=np.zeros(int(valid.sum()), bool))
    scene.sensors = [dataclasses.replace(c0, enable_intrinsics=False), cam]
    fx["offsets"] = np.concatenate([[0], np.cumsum(np.bincount(frame[valid], minlength=len(times)))]).astype(np.int64)
    fx["pixels"], fx["points"] = px[valid], fx["points"][valid]
    fx["spl"] = (scene.knots, scene.basis, scene.ctrl, scene.order)
    return scene, fx


def solve_from(api, scene, start, iterations=50):
    built = syn.build_problem(api, scene)
    blk = built.sensor_blocks[1]
    for name, v in zip(("q", "t", "latency"), start):
        built.problem.set_param_block(blk[name], np.atleast_1d(v))
    summary = helpers.solve(built.problem, api, iterations)
    return summary, syn.read_back(built, scene)[0][1]


def test_optimize_from_the_aligned_start_reaches_the_minimum(api):
    """The two-camera scene of two_camera_scene(): the alignment runs on the second camera's pixels and the scene's starting
    spline. Asserted: the solve from the aligned start converges to the ORACLE's estimates -- its solve from the truth, on the CPU
    (the cost to ten times the solver's function tolerance, extrinsics and latency to its square root) -- and starts at a cost
    within 1 % of the truth's, a million times below the uninformed start's (identity, zero latency). From that start the solve
    gets there too on this scene but needs more iterations, measured with the oracle on the CPU: 44 from a cost of 2.2e9 against
    38 from the aligned start's 1690.7 (34 from the truth's 1693.7; the minimum is 1569.37). Most of every count is the tail of the
    free, noisy trajectory, not the extrinsics: on an MI355X the counts were 32 (identity), 37 (aligned) and 33 (truth), so the
    order of the counts is printed, not asserted."""
    scene, fx = two_camera_scene()
    r = device(api, fx, sigma_pixel=0.1, **cref.OPTIONS)
    tr = cref.TRUTH
    print("alignment: rotation off by", _angle(r["q_rig_camera"], tr["q"]), "translation", r["t_rig_camera"] - tr["t"], "latency", r["latency"],
          "frames", r["frames_used"], "rms", r["rms"])
    assert r["status"] == _capi.ALIGN_OK and cref.distance_to_truth(cref.estimate(r), tr) < 2e-3
    o = api.default_options()
    tol = 10 * o.function_tolerance
    ref, ref_est = solve_from(helpers.oracle_api(), scene, (tr["q"], tr["t"], tr["latency"]))
    s, est = solve_from(api, scene, cref.estimate(r))
    u, u_est = solve_from(api, scene, (np.array([0.0, 0, 0, 1]), np.zeros(3), 0.0))
    for name, (sm, e) in (("truth (oracle)", (ref, ref_est)), ("aligned", (s, est)), ("identity", (u, u_est))):
        print(name, "start: iterations", sm.num_iterations, "cost", sm.initial_cost, "->", sm.final_cost, "latency", e["latency"],
              "rotation off by", _angle(e["q"], tr["q"]))
    assert s.termination_type == _capi.CONVERGENCE and abs(s.final_cost - ref.final_cost) <= tol * ref.final_cost
    assert _angle(est["q"], ref_est["q"]) <= np.sqrt(tol) and np.abs(est["t"] - ref_est["t"]).max() <= np.sqrt(tol)
    assert abs(est["latency"] - ref_est["latency"]) <= np.sqrt(tol)
    assert s.initial_cost < 1.01 * ref.initial_cost and u.initial_cost > 1e6 * s.initial_cost
