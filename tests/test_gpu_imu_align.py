"""calico_imu_align on the device against the numpy reference (imu_align_ref.py), the truth, and the optimiser itself.

The yardsticks are the reference's own: FLOOR (the reference's criterion -- the scaled size of one undamped Gauss-Newton step --
at and after its own result on the noisy standard fixture) and REF_FREE / REF_FREE_ACCEL (its distance to the truth on noise-free
data); test_imu_align_host.py measures them. The device is held to 2 x FLOOR at its estimate and to 10 x the reference's own
distance to the truth.

What the noise-free checks do and do not show: the fixtures' data come from the reference's own kinematics (the spline segment of
the STAMP, as the optimiser takes it), not from synthetic.project_gyroscope / project_accelerometer (the segment of the true time).
"Recovers the truth" is therefore a check of the device against the model it shares with the reference, not an independent one.
What stands outside that model: the reference is pinned on the ORACLE's evaluate (test_imu_align_host.py), the device's result is
checked by the optimiser's own gradient here, tests/cpp/imu_align_facade.cpp and test_python_imu_align.py recover mountings
from the facade's Project() (the true time's segment), and the last test here runs the optimiser from the aligned start on
helpers.small_scene, whose data are synthetic.py's.

Bounds set here, with their reasons:
  CURVE_BOUND  the correlation curve against the reference's, rounding only. Measured on the first run on an MI355X:
               maximum 6.7e-16 over the 41 lags of the noisy standard fixture (1.9e-15 with 16 samples); allowed 10 x that.
  SHAPE_BOUND  the shape cases run other sample sets than the one FLOOR was measured on, so they are held to what a backward
               stable least-squares solve guarantees, 100 eps cond(J), with cond(J) the reference's Jacobian's at the device's
               estimate (14 on these fixtures: 3e-13).
Measured on an MI355X (printed by the tests): the device's criterion on the noisy standard fixture, the same through the
optimiser's own normal equations, and its noise-free distances; see the figures beside each assertion."""
import numpy as np
import pytest

import helpers
import imu_align_ref as ar
from calico_amd import _capi, synthetic as syn

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16
CURVE_BOUND = 10 * 6.7e-16


@pytest.fixture(scope="module")
def api():
    return helpers.hip_api()


def device(api, spl, gs, g, as_=None, a=None, **kw):
    knots, basis, ctrl, order = spl
    extra = {k: kw.pop(k) for k in ("t_rig_accel", "q_init", "latency_init") if k in kw}
    return _capi.imu_align(api, order, knots, basis, ctrl, gs, g, as_, a, options=_capi.imu_alignment_options(api, **kw), covariance=True,
                           curve=True, **extra)


def used(r, gs, g):
    s = slice(r["first_sample"], r["first_sample"] + r["gyro_samples"])
    return gs[s], g[s]


def shape_bound(spl, gs, g, est, free=np.ones(7, bool)):
    _, J = ar.gyro_system(spl, gs, g, est)
    return 100 * EPS * np.linalg.cond(J.reshape(-1, 7)[:, np.asarray(free, bool)])


@pytest.fixture(scope="module")
def noisy(api):
    """The noisy standard fixture: the data, the reference's result, the device's."""
    spl, gs, g, as_, a, truth = ar.fixture(1e-3)
    return spl, gs, g, as_, a, truth, ar.align(spl, gs, g, as_, a, **ar.OPTIONS), device(api, spl, gs, g, as_, a, **ar.OPTIONS)


def test_noise_free_standard_fixture_recovers_the_truth(api):
    spl, gs, g, as_, a, truth = ar.fixture(0.0)
    r = device(api, spl, gs, g, as_, a, **ar.OPTIONS)
    assert (r["gyro_status"], r["accel_status"], r["gyro_samples"], r["accel_samples"], r["n_lags"]) == (_capi.ALIGN_OK, _capi.ALIGN_OK, 680, 680, 41)
    dist = ar.distance_to_truth(ar.estimate(r), truth)
    dist_accel = max(np.abs(r["gravity_world"] - truth["gravity"]).max(), np.abs(r["accel_bias"] - truth["accel_bias"]).max())
    print("device distance to the truth", dist, "accelerometer part", dist_accel, "iterations", r["iterations"], "rms", r["gyro_rms"], r["accel_rms"])
    assert dist <= 10 * ar.REF_FREE
    assert dist_accel <= 10 * ar.REF_FREE_ACCEL
    assert abs(r["gravity_norm"] - np.linalg.norm(truth["gravity"])) <= 1e-12 and r["gyro_rms"] <= 1e-13 and r["accel_rms"] <= 1e-12


def test_noisy_standard_fixture_is_a_minimum_by_the_references_criterion(noisy):
    spl, gs, g, as_, a, truth, ref, r = noisy
    assert (r["gyro_status"], r["accel_status"]) == (_capi.ALIGN_OK, _capi.ALIGN_OK) and ref["gyro_status"] == ar.OK
    assert (r["gyro_samples"], r["first_sample"]) == (ref["gyro_samples"], ref["first_sample"])
    s, m = used(r, gs, g)
    crit = ar.criterion(spl, s, m, ar.estimate(r))
    print("device criterion", crit, "FLOOR", ar.FLOOR, "iterations", r["iterations"], "distance to the reference",
          ar.distance_to_truth(ar.estimate(r), dict(q=ref["q_rig_gyro"], bias=ref["gyro_bias"], latency=ref["latency"])))
    assert crit <= 2 * ar.FLOOR
    assert r["peak_index"] == ref["peak_index"] == 25
    curve_err = np.abs(r["curve"] - ref["curve"]).max()
    print("curve against the reference", curve_err, "coarse latency", r["coarse_latency"], ref["coarse_latency"])
    assert curve_err <= CURVE_BOUND
    assert abs(r["coarse_latency"] - ref["coarse_latency"]) <= 1e-9 and abs(r["peak_correlation"] - ref["curve"][25]) <= CURVE_BOUND
    cov = ar.covariance(spl, s, m, ar.estimate(r))
    cov_err = np.abs(r["cov"] - cov).max() / np.abs(cov).max()
    print("covariance against the reference", cov_err)
    assert cov_err <= 1e-6 and np.abs(r["cov"] - r["cov"].T).max() <= 1e-12 * np.abs(cov).max()
    assert abs(r["gyro_rms"] - ref["gyro_rms"]) <= 1e-9 * ref["gyro_rms"] and abs(r["accel_rms"] - ref["accel_rms"]) <= 1e-9 * ref["accel_rms"]
    assert np.abs(r["gravity_world"] - ref["gravity_world"]).max() <= 1e-9 and np.abs(r["accel_bias"] - ref["accel_bias"]).max() <= 1e-9


def test_result_is_a_minimum_of_the_optimisers_own_gyroscope_term(api):
    """The device's estimate loaded into a problem with that gyroscope (calico_evaluate): the optimiser's cost is the reported RMS,
    and the Gauss-Newton step of ITS gradient and J^T J in (q, latency, bias) is within 2 x FLOOR. A slip in a sign or in the
    direction of time shows here: the step would be the size of the estimate."""
    spl, gs, g, as_, a, truth = ar.fixture(1e-3)
    sigma = 1e-3
    r = device(api, spl, gs, g, sigma_gyro=sigma, **ar.OPTIONS)
    assert r["gyro_status"] == _capi.ALIGN_OK
    s, m = used(r, gs, g)
    built, cols = ar.gyro_problem(api, spl, s, m, ar.estimate(r), sigma)
    cost, grad, H = built.problem.evaluate()
    n = len(s)
    print("optimiser cost", cost, "2 cost / 3n", 2 * cost / (3 * n), "reported rms^2", r["gyro_rms"] ** 2, "final_cost", r["final_cost"])
    assert abs(2 * cost / (3 * n) - r["gyro_rms"] ** 2) <= 1e-12 * r["gyro_rms"] ** 2
    assert abs(cost - r["final_cost"]) <= 1e-12 * cost
    d = -np.linalg.solve(H[np.ix_(cols, cols)], grad[cols])
    d[:3] *= 2.0      # (Ceres' quaternion tangent is half the rotation vector)
    step = ar.step_size(ar.estimate(r), d)
    print("Gauss-Newton step of the optimiser's own system", step, "FLOOR", ar.FLOOR)
    assert step <= 2 * ar.FLOOR
    # the covariance is the inverse of that J^T J (tangent scaled)
    scale = np.array([2.0, 2, 2, 1, 1, 1, 1])
    cov = np.linalg.inv(H[np.ix_(cols, cols)] / scale[:, None] / scale[None, :])
    assert np.abs(r["cov"] - cov).max() <= 1e-6 * np.abs(cov).max()


@pytest.mark.parametrize("n", [15, 16, 63, 64, 65, 257])
def test_sample_counts_around_the_wave_and_the_workgroup(api, n):
    spl, gs, g, as_, a, truth = ar.fixture(1e-3, rate=n / 6.8)
    assert len(gs) == n
    ref = ar.align(spl, gs, g, as_, a, **ar.OPTIONS)
    r = device(api, spl, gs, g, as_, a, **ar.OPTIONS)
    assert (r["gyro_status"], r["accel_status"], r["gyro_samples"], r["peak_index"]) == (ref["gyro_status"], ref["accel_status"], n, ref["peak_index"])
    if n == 15:
        assert r["gyro_status"] == _capi.ALIGN_TOO_FEW_SAMPLES and r["q_rig_gyro"].tolist() == [0, 0, 0, 1] and r["gravity_world"] is None
        return
    assert r["gyro_status"] == _capi.ALIGN_OK and r["accel_samples"] == n
    crit, bound = ar.criterion(spl, gs, g, ar.estimate(r)), shape_bound(spl, gs, g, ar.estimate(r))
    print("n", n, "criterion", crit, "bound", bound, "curve", np.abs(r["curve"] - ref["curve"]).max())
    assert crit <= bound and np.abs(r["curve"] - ref["curve"]).max() <= CURVE_BOUND
    assert np.abs(r["gravity_world"] - ref["gravity_world"]).max() <= 1e-9


def test_samples_in_the_first_and_last_segment(api):
    spl, gs, g, as_, a, truth = ar.fixture(1e-3, t0=0.04, t1=7.13)
    r = device(api, spl, gs, g, as_, a, **ar.OPTIONS)
    assert (r["gyro_status"], r["gyro_samples"], r["first_sample"], r["accel_samples"]) == (_capi.ALIGN_OK, len(gs), 0, len(gs))
    assert gs[0] < 0.1 and gs[-1] > 7.1
    crit = ar.criterion(spl, gs, g, ar.estimate(r))
    print("criterion", crit)
    assert crit <= shape_bound(spl, gs, g, ar.estimate(r))


def test_a_wide_lag_grid_pushes_samples_off_the_knots(api):
    spl, gs, g, as_, a, truth = ar.fixture(1e-3, t0=0.0, t1=7.18)
    ref = ar.align(spl, gs, g, as_, a, max_lag=1.0, lag_step=0.025)
    r = device(api, spl, gs, g, as_, a, max_lag=1.0, lag_step=0.025)
    assert 0.25 * len(gs) <= len(gs) - ref["gyro_samples"] <= 0.35 * len(gs)
    assert (r["gyro_samples"], r["first_sample"], r["n_lags"], r["peak_index"]) == (ref["gyro_samples"], ref["first_sample"], 81, ref["peak_index"])
    assert r["gyro_status"] == _capi.ALIGN_OK and r["accel_samples"] == len(as_)
    s, m = used(r, gs, g)
    assert ar.criterion(spl, s, m, ar.estimate(r)) <= shape_bound(spl, s, m, ar.estimate(r))
    assert np.abs(r["curve"] - ref["curve"]).max() <= CURVE_BOUND


@pytest.mark.parametrize("latency", [-0.031, 0.049])
def test_latencies_of_either_sign(api, latency):
    spl, gs, g, as_, a, truth = ar.fixture(1e-3, t0=0.3, t1=6.9, latency=latency)
    ref = ar.align(spl, gs, g, as_, a, max_lag=0.1, lag_step=0.0025)
    r = device(api, spl, gs, g, as_, a, max_lag=0.1, lag_step=0.0025)
    assert (r["gyro_status"], r["peak_index"], r["gyro_samples"]) == (_capi.ALIGN_OK, ref["peak_index"], ref["gyro_samples"])
    assert abs(r["latency"] - latency) <= 1e-4 and abs(r["coarse_latency"] - latency) <= 1e-3
    s, m = used(r, gs, g)
    assert ar.criterion(spl, s, m, ar.estimate(r)) <= shape_bound(spl, s, m, ar.estimate(r))


def test_a_latency_beyond_the_grid_is_no_peak(api):
    spl, gs, g, as_, a, truth = ar.fixture(1e-3, t0=0.3, t1=6.9, latency=0.08)
    r = device(api, spl, gs, g, as_, a, **ar.OPTIONS)
    assert (r["gyro_status"], r["accel_status"], r["peak_index"]) == (_capi.ALIGN_NO_PEAK, _capi.ALIGN_NO_PEAK, 40)
    assert r["q_rig_gyro"].tolist() == [0, 0, 0, 1] and r["latency"] == 0.0 and r["gravity_world"] is None and not r["cov"].any()


def test_constant_measurements_are_no_peak(api):
    spl, gs, g, as_, a, truth = ar.fixture(1e-3)
    r = device(api, spl, gs, np.tile([0.1, 0.2, -0.3], (len(gs), 1)), **ar.OPTIONS)
    assert r["gyro_status"] == _capi.ALIGN_NO_PEAK and not r["curve"].any()


def test_rotation_about_one_axis_is_degenerate(api):
    spl, gs, g, as_, a, truth = ar.fixture(1e-3, one_axis=True)
    ref = ar.align(spl, gs, g, as_, a, **ar.OPTIONS)
    r = device(api, spl, gs, g, as_, a, **ar.OPTIONS)
    assert ref["gyro_status"] == ar.DEGENERATE
    assert (r["gyro_status"], r["accel_status"], r["peak_index"]) == (_capi.ALIGN_DEGENERATE, _capi.ALIGN_DEGENERATE, ref["peak_index"])
    assert r["scatter_pivot"] < 1e-6 and r["q_rig_gyro"].tolist() == [0, 0, 0, 1]


def test_a_given_start_with_the_latency_held(api):
    spl, gs, g, as_, a, truth = ar.fixture(1e-3)
    q0 = ar.apply((truth["q"], truth["bias"], truth["latency"]), np.array([0.05, -0.04, 0.03, 0, 0, 0, 0]))[0]
    r = device(api, spl, gs, g, as_, a, q_init=q0, latency_init=truth["latency"], estimate_latency=0, **ar.OPTIONS)
    assert (r["gyro_status"], r["accel_status"], r["n_lags"], r["peak_index"]) == (_capi.ALIGN_OK, _capi.ALIGN_OK, 0, -1)
    assert r["latency"] == truth["latency"] and r["curve"].shape == (0,) and r["gyro_samples"] == len(gs)
    free = np.array([1, 1, 1, 1, 1, 1, 0], bool)
    crit = ar.criterion(spl, gs, g, ar.estimate(r), free)
    print("criterion with the latency held", crit)
    assert crit <= shape_bound(spl, gs, g, ar.estimate(r), free)
    assert not r["cov"][6].any() and not r["cov"][:, 6].any() and r["cov"][0, 0] > 0
    # with the latency free the same start reaches the same minimum as the search does
    r2 = device(api, spl, gs, g, q_init=q0, latency_init=0.01, **ar.OPTIONS)
    assert r2["gyro_status"] == _capi.ALIGN_OK and ar.criterion(spl, gs, g, ar.estimate(r2)) <= shape_bound(spl, gs, g, ar.estimate(r2))


def test_the_bias_held_at_zero(api):
    spl, gs, g, as_, a, truth = ar.fixture(1e-3)
    ref = ar.align(spl, gs, g, estimate_gyro_bias=0, **ar.OPTIONS)
    r = device(api, spl, gs, g, estimate_gyro_bias=0, **ar.OPTIONS)
    assert (r["gyro_status"], ref["gyro_status"]) == (_capi.ALIGN_OK, ar.OK) and r["gyro_bias"].tolist() == [0, 0, 0]
    free = np.array([1, 1, 1, 0, 0, 0, 1], bool)
    assert ar.criterion(spl, gs, g, ar.estimate(r), free) <= shape_bound(spl, gs, g, ar.estimate(r), free)
    assert not r["cov"][3:6].any() and not r["cov"][:, 3:6].any()


def test_without_an_accelerometer_and_with_a_lever_arm(api):
    spl, gs, g, as_, a, truth = ar.fixture(0.0, lever=(0.1, 0.0, 0.0))
    r = device(api, spl, gs, g, **ar.OPTIONS)
    assert (r["gyro_status"], r["accel_status"], r["accel_samples"]) == (_capi.ALIGN_OK, _capi.ALIGN_TOO_FEW_SAMPLES, 0) and r["gravity_world"] is None
    ref = ar.align(spl, gs, g, as_, a, t_rig_accel=truth["t_rig_accel"], **ar.OPTIONS)
    own = max(np.abs(ref["gravity_world"] - truth["gravity"]).max(), np.abs(ref["accel_bias"] - truth["accel_bias"]).max(), ar.REF_FREE_ACCEL)
    r = device(api, spl, gs, g, as_, a, t_rig_accel=truth["t_rig_accel"], **ar.OPTIONS)
    dist = max(np.abs(r["gravity_world"] - truth["gravity"]).max(), np.abs(r["accel_bias"] - truth["accel_bias"]).max())
    print("lever arm: device", dist, "reference", own)
    assert r["accel_status"] == _capi.ALIGN_OK and dist <= 10 * own
    # the lever arm matters: without it the same data are off by far more
    r0 = device(api, spl, gs, g, as_, a, **ar.OPTIONS)
    assert np.abs(r0["gravity_world"] - truth["gravity"]).max() > 1e-4
    # gravity alone
    r3 = device(api, spl, gs, g, as_, a - truth["accel_bias"], t_rig_accel=truth["t_rig_accel"], estimate_accel_bias=0, **ar.OPTIONS)
    assert r3["accel_status"] == _capi.ALIGN_OK and r3["accel_bias"].tolist() == [0, 0, 0]
    assert np.abs(r3["gravity_world"] - truth["gravity"]).max() <= 10 * own


@pytest.mark.parametrize("order", [4, 8])
def test_spline_orders(api, order):
    spl, gs, g, as_, a, truth = ar.fixture(0.0, order=order)
    ref = ar.align(spl, gs, g, as_, a, **ar.OPTIONS)
    own = max(ar.distance_to_truth(ar.estimate(ref), truth), ar.REF_FREE)
    own_accel = max(np.abs(ref["gravity_world"] - truth["gravity"]).max(), np.abs(ref["accel_bias"] - truth["accel_bias"]).max(), ar.REF_FREE_ACCEL)
    r = device(api, spl, gs, g, as_, a, **ar.OPTIONS)
    dist = ar.distance_to_truth(ar.estimate(r), truth)
    dist_accel = max(np.abs(r["gravity_world"] - truth["gravity"]).max(), np.abs(r["accel_bias"] - truth["accel_bias"]).max())
    print("order", order, "device", dist, dist_accel, "reference", own, own_accel)
    assert (r["gyro_status"], r["accel_status"], r["peak_index"]) == (_capi.ALIGN_OK, _capi.ALIGN_OK, ref["peak_index"])
    assert dist <= 10 * own and dist_accel <= 10 * own_accel


def test_two_calls_are_bit_identical_and_the_curves_tail_is_untouched(api, noisy):
    spl, gs, g, as_, a, truth, ref, r = noisy
    again = device(api, spl, gs, g, as_, a, **ar.OPTIONS)
    for key, v in r.items():
        w = again[key]
        if isinstance(v, np.ndarray):
            assert v.tobytes() == w.tobytes(), key
        else:
            assert v == w, key
    assert r["curve"].shape == (41,) and np.isfinite(r["curve"]).all()
    assert r["curve_tail"].shape == (_capi.ALIGN_MAX_LAGS - 41,) and np.isnan(r["curve_tail"]).all()


def _angle(a, b):
    d = syn.quat_mul(a, syn.quat_conj(b))
    return 2.0 * np.arctan2(np.linalg.norm(d[:3]), abs(d[3]))


def test_optimize_from_the_aligned_start_reaches_the_small_scenes_minimum(api):
    """helpers.small_scene(imu=True): two cameras, a gyroscope and an accelerometer with a scale of 1.3, each rotated by 2 degrees
    about an axis of its own, 20 ms late, noisy -- outside the alignment's model (scale 1, one rotation) in the ways the optimiser
    is left to refine. The alignment runs on the scene's IMU samples and starting spline; rotation and latency go to both
    sensors, the bias to the gyroscope (gravity is a constant of the scene, and the accelerometer's part, run at the wrong scale,
    is not used). Asserted: the alignment is closer to the gyroscope's mounting and latency than the uninformed start (identity,
    zero latency), the optimiser's own gyroscope cost is lower there, and the solve from the aligned start ends at the scene's
    minimum -- the cost of the solve that starts AT the truth to ten times the solver's function tolerance, its IMU parameters to
    the square root of that. Printed: what the same solve does from the uninformed start (on this scene, whose mountings are 2 degrees from the
    identity, it gets there too)."""
    scene = helpers.small_scene(imu=True)
    gy, ac = scene.sensors[2], scene.sensors[3]
    assert (gy.kind, ac.kind, gy.intrinsics_true[0]) == (_capi.SENSOR_GYROSCOPE, _capi.SENSOR_ACCELEROMETER, 1.3)
    spl = (scene.knots, scene.basis, scene.ctrl, scene.order)
    r = device(api, spl, gy.stamps, gy.meas, sigma_gyro=gy.sigma, **ar.OPTIONS)
    assert r["gyro_status"] == _capi.ALIGN_OK
    identity = np.array([0.0, 0.0, 0.0, 1.0])
    print("alignment: rotation off by", _angle(r["q_rig_gyro"], gy.q_true), "(identity:", _angle(identity, gy.q_true), ") latency", r["latency"],
          "bias", r["gyro_bias"], "samples", r["gyro_samples"])
    assert _angle(r["q_rig_gyro"], gy.q_true) < 0.1 * _angle(identity, gy.q_true) and abs(r["latency"] - gy.latency_true) < 0.1 * gy.latency_true

    def truth(b):
        for sp, blk in zip(scene.sensors, b.sensor_blocks):
            for name, v in (("intrinsics", sp.intrinsics_true), ("q", sp.q_true), ("t", sp.t_true), ("latency", [sp.latency_true])):
                b.problem.set_param_block(blk[name], v)

    def uninformed(b):
        for blk in b.sensor_blocks[2:]:
            b.problem.set_param_block(blk["q"], identity)
            b.problem.set_param_block(blk["latency"], [0.0])

    def aligned(b):
        for blk in b.sensor_blocks[2:]:
            b.problem.set_param_block(blk["q"], r["q_rig_gyro"])
            b.problem.set_param_block(blk["latency"], [r["latency"]])
        b.problem.set_param_block(b.sensor_blocks[2]["intrinsics"], np.concatenate([gy.intrinsics[:1], r["gyro_bias"]]))

    o = api.default_options()
    out = {}
    for name, setup in (("truth", truth), ("uninformed", uninformed), ("aligned", aligned)):
        built = syn.build_problem(api, scene)
        setup(built)
        res, _ = built.problem.residuals(built.sensor_ids[2], gy.n, 3)
        summary = helpers.solve(built.problem, api, 50)
        est, _ = syn.read_back(built, scene)
        out[name] = (0.5 * float(np.sum(res * res)), summary, est)
        print(name, "start: gyroscope cost", out[name][0], "iterations", summary.num_iterations, "cost", summary.initial_cost, "->", summary.final_cost,
              "IMU latencies", est[2]["latency"], est[3]["latency"], "rotations off by", _angle(est[2]["q"], gy.q_true), _angle(est[3]["q"], ac.q_true))
    assert out["aligned"][0] < out["uninformed"][0]
    tol = 10 * o.function_tolerance      # the cost; a cost within tol of its minimum leaves the parameters within about sqrt(tol)
    ref_cost, ref_est = out["truth"][1].final_cost, out["truth"][2]
    s, est = out["aligned"][1], out["aligned"][2]
    assert s.termination_type == _capi.CONVERGENCE and abs(s.final_cost - ref_cost) <= tol * ref_cost
    for i in (2, 3):
        assert _angle(est[i]["q"], ref_est[i]["q"]) <= np.sqrt(tol) and abs(est[i]["latency"] - ref_est[i]["latency"]) <= np.sqrt(tol)
        assert np.abs(est[i]["intrinsics"] - ref_est[i]["intrinsics"]).max() <= np.sqrt(tol) * np.abs(ref_est[i]["intrinsics"]).max()
