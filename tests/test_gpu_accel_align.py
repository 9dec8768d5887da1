"""calico_accel_align on the device against the numpy reference (accel_align_ref.py), the truth, and the optimiser itself.

The yardsticks are the reference's own: FLOOR (the reference's criterion -- the scaled size of one undamped Gauss-Newton step --
at and after its own result on the noisy standard fixture with the lever arm LEVER) and REF_FREE (its distance to the truth on
noise-free data); test_accel_align_host.py measures them. The device is held to 2 x FLOOR at its estimate and to 10 x REF_FREE.

As in test_gpu_imu_align.py the fixtures' data come from the reference's own kinematics (the spline segment of the STAMP), so
"recovers the truth" checks the device against the model it shares with the reference. What stands outside that model: the
reference is pinned on the ORACLE's evaluate over all 13 columns (test_accel_align_host.py), the device's result is checked by
the optimiser's own gradient here, and the facade tests recover a mounting from Project()'s data (the true time's segment).

BOUND: everything that is compared with the reference is held to what a backward stable least-squares solve guarantees,
100 eps cond(J), relative, with cond(J) the reference's Jacobian's (free columns) at the device's estimate -- 1.8e3 on the
standard fixture: 4e-11. "Relative" for an estimate is the loop's own step measure (per group |difference|_inf / max(1,
|value|_inf), the rotation unscaled), for the covariance the largest entry's.

Measured on the first MI355X run (printed by the tests): criterion 3.9e-15 on the noisy standard fixture after 5 iterations, the
estimate 3.4e-15 from the reference's, the covariance 1.6e-14; noise-free 5.9e-15 from the truth; over the shapes and masks the
estimate within 3.4e-14 and the covariance within 5.1e-14; the optimiser's gradient 6.4e-10 against 8.8e-8 allowed.

The shapes: n of 16, 63, 64, 65, 256 and 257 (a partial wave, a full wave and one lane more, a full workgroup and one lane more)
and a range that starts mid-array, at orders 4 and 6, each spread over the whole trajectory by lowering the rate. The reference
alone ends OK on every one of them (checked on the CPU; test_accel_align_host.py repeats the check)."""
import math

import numpy as np
import pytest

import accel_align_ref as ar
import helpers
import imu_align_ref as ir
from calico_amd import _capi

pytestmark = pytest.mark.gpu

EPS = ar.EPS
OUTPUTS = ("q_rig_accel", "t_rig_accel", "bias", "gravity_world", "latency", "cov")
SHAPES = (16, 63, 64, 65, 256, 257)


@pytest.fixture(scope="module")
def api():
    return helpers.hip_api()


def device(api, spl, s, a, q_init, latency_init, start=None, device_index=0, **kw):
    knots, basis, ctrl, order = spl
    t, b, g = (None, None, None) if start is None else start
    return _capi.accel_align(api, order, knots, basis, ctrl, s, a, q_init, latency_init, t, b, g,
                             options=_capi.accel_alignment_options(api, **kw), covariance=True, device=device_index)


def used(r, s, a):
    sl = slice(r["first_sample"], r["first_sample"] + r["samples"])
    return s[sl], a[sl]


def bound(spl, s, a, est, free=np.ones(13, bool)):
    return 100 * EPS * ar.cond(spl, s, a, est, free)


def apart(a, b):
    """The loop's step measure of the difference of two estimates."""
    return ar.step_size(b, ar.difference(a, b))


def shaped(n, order, lead=0):
    """n samples spread over the whole trajectory; lead: that many stamps in front of the valid knots, measurements zero."""
    spl, s, a, truth = ar.fixture(1e-3, rate=n / 6.8, order=order)
    assert len(s) == n
    if lead:
        lo = ir.valid_range(spl)[0]
        s = np.concatenate([lo - 1.0 + 0.01 * np.arange(lead), s])
        a = np.concatenate([np.zeros((lead, 3)), a])
    return spl, s, a, truth


@pytest.fixture(scope="module")
def noisy(api):
    """The noisy standard fixture: the data, the start InitializeImu leaves, the reference's result, the device's."""
    spl, s, a, truth = ar.fixture(1e-3)
    q0, l0 = ar.imu_start(truth)
    return spl, s, a, truth, q0, l0, ar.align(spl, s, a, q0, l0), device(api, spl, s, a, q0, l0)


def test_noise_free_standard_fixture_recovers_the_truth(api):
    """680 samples: two full workgroups, then two waves and a 40-lane tail."""
    spl, s, a, truth = ar.fixture(0.0)
    q0, l0 = ar.imu_start(truth)
    ref = ar.align(spl, s, a, q0, l0)
    r = device(api, spl, s, a, q0, l0)
    assert (r["status"], r["linear_status"]) == (_capi.ALIGN_OK, _capi.ALIGN_OK) and (ref["status"], ref["linear_status"]) == (ar.OK, ar.OK)
    assert (r["samples"], r["first_sample"]) == (ref["samples"], ref["first_sample"]) == (680, 0)
    dist = ar.distance_to_truth(ar.estimate(r), truth)
    print("device distance to the truth", dist, "REF_FREE", ar.REF_FREE, "iterations", r["iterations"], ref["iterations"], "rms", r["rms"],
          "linear rms", r["linear_rms"], ref["linear_rms"])
    assert dist <= 10 * ar.REF_FREE
    assert abs(r["gravity_norm"] - np.linalg.norm(truth["gravity"])) <= 1e-11 and r["rms"] <= 1e-12
    assert abs(r["linear_rms"] - ref["linear_rms"]) <= 1e-9 * ref["linear_rms"]


def test_noisy_standard_fixture_is_a_minimum_by_the_references_criterion(noisy):
    spl, s, a, truth, q0, l0, ref, r = noisy
    assert (r["status"], r["linear_status"]) == (_capi.ALIGN_OK, _capi.ALIGN_OK) and ref["status"] == ar.OK
    assert (r["samples"], r["first_sample"]) == (ref["samples"], ref["first_sample"])
    est = ar.estimate(r)
    crit = ar.criterion(spl, s, a, est)
    b = bound(spl, s, a, est)
    print("device criterion", crit, "FLOOR", ar.FLOOR, "iterations", r["iterations"], ref["iterations"], "bound", b)
    assert crit <= 2 * ar.FLOOR
    d = apart(est, ar.estimate(ref))
    cov = ar.covariance(spl, s, a, est)
    cov_err = np.abs(r["cov"] - cov).max() / np.abs(cov).max()
    print("result against the reference", d, "covariance", cov_err, "lever arm error", np.abs(r["t_rig_accel"] - truth["t_rig_accel"]).max())
    assert d <= b and cov_err <= b
    assert np.abs(r["cov"] - r["cov"].T).max() <= 1e-12 * np.abs(cov).max()
    assert abs(r["rms"] - ref["rms"]) <= 1e-9 * ref["rms"] and abs(r["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
    assert abs(r["initial_cost"] - ref["initial_cost"]) <= 1e-6 * ref["initial_cost"]
    assert abs(r["gravity_norm"] - np.linalg.norm(r["gravity_world"])) <= 1e-14
    assert np.abs(r["t_rig_accel"] - truth["t_rig_accel"]).max() <= 5e-4      # (1e-2 m/s^2 of noise on 680 samples: 1e-4 m)


def test_result_is_a_minimum_of_the_optimisers_own_accelerometer_term(api, noisy):
    """The device's estimate loaded into a problem with that accelerometer and free q, t, bias, gravity and latency
    (calico_evaluate): the optimiser's cost is the reported one and its gradient is zero to BOUND x |J^T| |r|. A slip in a sign,
    in the direction of time or in the latency column shows here."""
    spl, s, a, truth, q0, l0, ref, r = noisy
    est = ar.estimate(r)
    P, cols = ar.accel_problem(api, spl, s, a, est, ctrl_constant=False)
    cost, grad, H = P.evaluate()
    res, J, _ = ar.system(spl, s, a, est)
    scale = bound(spl, s, a, est) * np.linalg.norm(J.reshape(-1, 13), 2) * np.linalg.norm(res)
    g = grad[cols] / ar.ROTATION_TANGENT
    print("optimiser cost", cost, "final_cost", r["final_cost"], "gradient", np.abs(g).max(), "allowed", scale)
    assert abs(cost - r["final_cost"]) <= 1e-12 * cost
    assert np.abs(g).max() <= scale


@pytest.mark.parametrize("order", [4, 6])
@pytest.mark.parametrize("n,lead", [(n, 0) for n in SHAPES] + [(100, 37)])
def test_shapes(api, n, lead, order):
    spl, s, a, truth = shaped(n, order, lead)
    q0, l0 = ar.imu_start(truth)
    ref = ar.align(spl, s, a, q0, l0)
    r = device(api, spl, s, a, q0, l0)
    assert ref["status"] == ar.OK and (r["status"], r["linear_status"]) == (_capi.ALIGN_OK, _capi.ALIGN_OK)
    assert (r["samples"], r["first_sample"]) == (ref["samples"], ref["first_sample"]) == (n, lead)
    su, au = used(r, s, a)
    est = ar.estimate(r)
    b = bound(spl, su, au, est)
    d = apart(est, ar.estimate(ref))
    cov = ar.covariance(spl, su, au, est)
    cov_err = np.abs(r["cov"] - cov).max() / np.abs(cov).max()
    print("n", n, "order", order, "result against the reference", d, "covariance", cov_err, "bound", b, "iterations", r["iterations"], ref["iterations"])
    assert d <= b and cov_err <= b
    assert abs(r["rms"] - ref["rms"]) <= 1e-9 * ref["rms"]


def _given(truth):
    return (truth["t_rig_accel"] + [0.01, -0.02, 0.015], truth["accel_bias"] + [0.02, 0.01, -0.01], truth["gravity"] + [0.2, -0.1, 0.3])


@pytest.mark.parametrize("held", ["rotation", "lever_arm", "bias", "gravity", "latency"])
def test_a_held_group_stays_bit_identical(api, noisy, held):
    spl, s, a, truth, q0, l0, _, _ = noisy
    start = _given(truth)
    kw = {"estimate_" + held: 0}
    ref = ar.align(spl, s, a, q0, l0, *start, **kw)
    r = device(api, spl, s, a, q0, l0, start, **kw)
    assert ref["status"] == ar.OK and r["status"] == _capi.ALIGN_OK and r["linear_status"] == -1
    free = ar.free_mask(**{held: 0})
    nrm = math.sqrt(q0[0] * q0[0] + q0[1] * q0[1] + q0[2] * q0[2] + q0[3] * q0[3])
    sg = (-1.0 if q0[3] < 0 else 1.0) / nrm
    expected = dict(rotation=("q_rig_accel", np.array([sg * v for v in q0])), lever_arm=("t_rig_accel", start[0]), bias=("bias", start[1]),
                    gravity=("gravity_world", start[2]), latency=("latency", np.float64(l0)))[held]
    assert np.asarray(r[expected[0]]).tobytes() == np.asarray(expected[1], float).tobytes()
    assert not r["cov"][~free, :].any() and not r["cov"][:, ~free].any() and np.all(np.diag(r["cov"])[free] > 0)
    est = ar.estimate(r)
    b = bound(spl, s, a, est, free)
    cov = ar.covariance(spl, s, a, est, free)
    d, cov_err = apart(est, ar.estimate(ref)), np.abs(r["cov"] - cov).max() / np.abs(cov).max()
    print("held", held, "result against the reference", d, "covariance", cov_err, "bound", b)
    assert d <= b and cov_err <= b


def test_rotation_and_latency_held_is_the_linear_solution(api, noisy):
    spl, s, a, truth, q0, l0, _, _ = noisy
    r = device(api, spl, s, a, q0, l0, estimate_rotation=0, estimate_latency=0)
    t, b_, g, rms, status = ar.linear(spl, s, a, q0 / np.linalg.norm(q0), l0)
    assert status == ar.OK and (r["status"], r["linear_status"]) == (_capi.ALIGN_OK, _capi.ALIGN_OK)
    free = ar.free_mask(rotation=0, latency=0)
    est = ar.estimate(r)
    b = bound(spl, s, a, est, free)
    d = apart(est, (est[0], t, b_, g, est[4]))
    print("device against lstsq", d, "bound", b, "rms", r["rms"], rms, "linear_rms", r["linear_rms"], "iterations", r["iterations"])
    assert d <= b and abs(r["rms"] - rms) <= 1e-9 * rms and abs(r["linear_rms"] - rms) <= 1e-6 * rms


def test_lever_arm_held_agrees_with_the_gyroscope_alignments_stage_d(api):
    """The two paths tied together: calico_imu_align's stage D (gravity and bias at the gyroscope's rotation and latency and a given
    lever arm) and this call with rotation, lever arm and latency held there."""
    spl, gs, g, as_, a, truth = ir.fixture(1e-3, lever=ar.LEVER)
    knots, basis, ctrl, order = spl
    lever = np.asarray(ar.LEVER, float)
    d = _capi.imu_align(api, order, knots, basis, ctrl, gs, g, as_, a, t_rig_accel=lever, options=_capi.imu_alignment_options(api, **ir.OPTIONS))
    assert (d["gyro_status"], d["accel_status"]) == (_capi.ALIGN_OK, _capi.ALIGN_OK)
    r = device(api, spl, as_, a, d["q_rig_gyro"], d["latency"], (lever, np.zeros(3), np.zeros(3)), estimate_rotation=0, estimate_lever_arm=0,
               estimate_latency=0)
    assert r["status"] == _capi.ALIGN_OK and r["samples"] == d["accel_samples"]
    free = ar.free_mask(rotation=0, lever_arm=0, latency=0)
    est = ar.estimate(r)
    b = bound(spl, as_, a, est, free)
    apart_ = apart(est, (est[0], est[1], d["accel_bias"], d["gravity_world"], est[4]))
    print("against stage D", apart_, "bound", b, "rms", r["rms"], d["accel_rms"])
    assert apart_ <= b and abs(r["rms"] - d["accel_rms"]) <= 1e-9 * d["accel_rms"]


def test_stage_l_and_a_given_start_reach_the_same_minimum(api, noisy):
    spl, s, a, truth, q0, l0, _, r = noisy
    g = device(api, spl, s, a, q0, l0, _given(truth))
    assert g["status"] == _capi.ALIGN_OK and g["linear_status"] == -1 and g["linear_rms"] == 0.0 and r["linear_status"] == _capi.ALIGN_OK
    b = bound(spl, s, a, ar.estimate(r))
    d = apart(ar.estimate(g), ar.estimate(r))
    print("given start against stage L's", d, "bound", b, "iterations", g["iterations"], r["iterations"])
    assert d <= b


def _is_start(r, q0, l0, start=None):
    t, b, g = (np.zeros(3),) * 3 if start is None else start
    q = q0 / np.linalg.norm(q0)
    return (np.abs(r["q_rig_accel"] - q).max() <= 1e-15 and r["t_rig_accel"].tolist() == list(t) and r["bias"].tolist() == list(b)
            and r["gravity_world"].tolist() == list(g) and r["latency"] == l0 and not r["cov"].any())


def test_too_few_samples_and_no_samples(api):
    spl, s, a, truth = ar.fixture(1e-3)
    q0, l0 = ar.imu_start(truth)
    r = device(api, spl, s[:15], a[:15], q0, l0)
    assert (r["status"], r["linear_status"], r["samples"], r["iterations"]) == (_capi.ALIGN_TOO_FEW_SAMPLES, -1, 15, 0) and _is_start(r, q0, l0)
    r = device(api, spl, s[:0], a[:0], q0, l0, _given(truth), device_index=10 ** 6)      # n == 0 touches no device
    assert (r["status"], r["samples"]) == (_capi.ALIGN_TOO_FEW_SAMPLES, 0) and _is_start(r, q0, l0, _given(truth))


def test_rotation_about_one_axis_is_not_positive_definite(api):
    """The lever arm along the axis has no effect: its column is zero whatever the damping."""
    spl, s, a, truth = ar.fixture(1e-3, one_axis=True)
    q0, l0 = ar.imu_start(truth)
    ref = ar.align(spl, s, a, q0, l0)
    r = device(api, spl, s, a, q0, l0)
    assert (ref["status"], ref["linear_status"]) == (ar.NOT_POSITIVE_DEFINITE, ar.NOT_POSITIVE_DEFINITE)
    assert (r["status"], r["linear_status"], r["iterations"]) == (_capi.ALIGN_NOT_POSITIVE_DEFINITE, _capi.ALIGN_NOT_POSITIVE_DEFINITE, 0)
    assert _is_start(r, q0, l0)
    start = _given(truth)
    ref = ar.align(spl, s, a, q0, l0, *start)
    r = device(api, spl, s, a, q0, l0, start)
    assert ref["status"] == ar.NOT_POSITIVE_DEFINITE
    assert (r["status"], r["linear_status"], r["lambda_"]) == (_capi.ALIGN_NOT_POSITIVE_DEFINITE, -1, 1e12)
    assert _is_start(r, q0, l0, start)      # (no step was ever made: the current point is the start)


def test_one_iteration_is_not_converged_at_the_last_accepted_point(api, noisy):
    spl, s, a, truth, q0, l0, _, _ = noisy
    ref = ar.align(spl, s, a, q0, l0, max_iterations=1)
    r = device(api, spl, s, a, q0, l0, max_iterations=1)
    assert ref["status"] == ar.NOT_CONVERGED and (r["status"], r["iterations"]) == (_capi.ALIGN_NOT_CONVERGED, 1)
    assert r["final_cost"] <= r["initial_cost"] and r["cov"].any()
    est = ar.estimate(r)
    d = apart(est, ar.estimate(ref))
    print("after one step against the reference", d, "costs", r["initial_cost"], r["final_cost"], ref["initial_cost"], ref["final_cost"])
    assert d <= 1e-9 and abs(ar.cost(spl, s, a, est) - r["final_cost"]) <= 1e-9 * r["final_cost"]


def test_a_measurement_that_is_not_a_number_is_degenerate(api, noisy):
    spl, s, a, truth, q0, l0, _, _ = noisy
    bad = a.copy()
    bad[300, 1] = np.nan
    r = device(api, spl, s, bad, q0, l0)
    assert (r["status"], r["linear_status"]) == (_capi.ALIGN_DEGENERATE, _capi.ALIGN_DEGENERATE) and _is_start(r, q0, l0)
    start = _given(truth)
    r = device(api, spl, s, bad, q0, l0, start)
    assert (r["status"], r["linear_status"], r["iterations"]) == (_capi.ALIGN_DEGENERATE, -1, 0) and _is_start(r, q0, l0, start)


def test_two_calls_give_identical_bytes(api, noisy):
    spl, s, a, truth, q0, l0, _, r = noisy
    again = device(api, spl, s, a, q0, l0)
    for name in OUTPUTS:
        assert np.asarray(r[name]).tobytes() == np.asarray(again[name]).tobytes(), name
    for name, _ in _capi.AccelAlignmentSummary._fields_:
        assert np.float64(r[name]).tobytes() == np.float64(again[name]).tobytes(), name
