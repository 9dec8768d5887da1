"""The robust spline fit on the device (`-m gpu`): calico_fit_spline_robust against tests/fit_robust_ref.py (proved on the CPU in
test_fit_robust_reference.py). Every reweighted iteration is checked from the device's own previous iterate -- the median is an
exact order statistic of the residuals the device reported, psi is the float64 expression, the solve is held to the long-double
system of the device's own weights -- so that no criterion depends on how an IRLS trajectory amplifies roundoff; the scenario
then says what the call is for. Measured (MI355X): the scenario's fitted values lie 0.6e-12 to 2.6e-12 (RMS) from the long-double
IRLS after the same iterations, as far as the float64 restatement on the CPU.

Two things the interface decides: the loss is one field for both groups, so the independence test changes group 1's data, weights,
lambda, tuning, scale and min_scale (not its loss); and max_iterations is one field, so the early-out test repeats each group with
its own iteration count."""
import ctypes as C

import numpy as np
import pytest

import fit_ref
import fit_robust_ref as fr
import fit_smooth_ref as fs
from calico_amd import _capi

pytestmark = pytest.mark.gpu
LD = np.longdouble
LOSSES = [fr.HUBER, fr.TUKEY]


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _robust(hip, c, weights=None, fit=None, **robust):
    o = _capi.default_spline_fit_options(hip, **fit) if fit else None
    return _capi.fit_spline_robust(hip, c.order, c.knots, c.basis, c.stamps, c.data, weights, o, _capi.default_spline_robust_options(hip, **robust))


def _smooth(hip, c, weights=None):
    return _capi.fit_spline_smooth(hip, c.order, c.knots, c.basis, c.stamps, c.data, weights, None)


def _tuning(loss):
    return dict(loss=loss, tuning_rot=fr.SCENARIO_TUNING[loss][0], tuning_pos=fr.SCENARIO_TUNING[loss][1])


def _same_bits(a, b, groups=(0, 1), but=()):
    """Every output of two calls, bit for bit (NaN equal to NaN), in the given groups; `but`: summary fields left out."""
    for g in groups:
        assert np.array_equal(a["ctrl"][:, 3 * g:3 * g + 3], b["ctrl"][:, 3 * g:3 * g + 3]), g
        for key in ("robust_weights", "residuals"):
            assert np.array_equal(a[key][:, g], b[key][:, g], equal_nan=True), (key, g)
        for key, v in a["summary"].items():
            if key not in but:
                assert np.array_equal(v[g], b["summary"][key][g], equal_nan=True), (key, g, v, b["summary"][key])


def _without(c, keep):
    return fr.with_data(c, np.ascontiguousarray(c.data[keep]), np.ascontiguousarray(c.stamps[keep]))


def test_no_iteration_is_the_smoothing_fit(hip):
    """max_iterations 0: ctrl has calico_fit_spline_smooth's bits, u = 1 (0 where the prior weight is 0), and the residual norms lie
    within 64 x 2^-53 x |sum|W||C| + |d||_2 (the norm over the channels of each channel's bound) of the long-double ones at the
    device's own control points."""
    s = fr.scenario()
    p, c = s.dirty, s.dirty.c
    out = _robust(hip, c, s.weights, max_iterations=0)
    assert np.array_equal(out["ctrl"], _smooth(hip, c, s.weights)["ctrl"])
    S = out["summary"]
    assert S["status"] == [0, 0] and S["iterations"] == [0, 0] and S["n_downweighted"] == [0, 0] and S["n_rejected"] == [0, 0]
    assert S["n_used"] == [494, 494] and np.isnan(S["scale"] + S["median_residual"] + S["last_step"]).all()
    idx = p.seg[:, None] + np.arange(c.order)[None, :]
    for g in range(2):
        use = s.weights[:, g] > 0
        assert np.array_equal(out["robust_weights"][:, g], use.astype(float)) and np.isnan(out["residuals"][~use, g]).all()
        Cg = out["ctrl"][:, 3 * g:3 * g + 3]
        mag = np.einsum("nj,njc->nc", np.abs(p.W), np.abs(Cg)[idx]) + np.abs(c.data[:, 3 * g:3 * g + 3])
        err = np.abs(np.asarray(out["residuals"][:, g], LD) - fr.residual_norms(p, g, Cg, LD))[use]
        bound = 64 * 2.0 ** -53 * np.linalg.norm(mag, axis=1)[use]
        print("group %d: residual norms within %.2f of the bound" % (g, float((err / bound).max())))
        assert (err <= bound).all()
        rss = float((np.asarray(s.weights[:, g], LD) * np.asarray(out["residuals"][:, g], LD) ** 2)[use].sum())
        assert abs(S["rss"][g] - rss) <= fs.SUM_BOUND * rss


@pytest.mark.parametrize("weighted", [False, True])
def test_everything_an_inlier_changes_no_bit(weighted, hip):
    """scale 1e300: every u is 1, the reweighted solve repeats iteration 0 bit for bit, the step is 0 and the group has converged."""
    s = fr.scenario()
    w = np.ascontiguousarray(s.weights) if weighted else None
    start = _robust(hip, s.dirty.c, w, max_iterations=0)
    out = _robust(hip, s.dirty.c, w, max_iterations=3, scale_rot=1e300, scale_pos=1e300)
    S = out["summary"]
    assert np.array_equal(out["ctrl"], start["ctrl"]) and np.array_equal(out["residuals"], start["residuals"], equal_nan=True)
    assert S["iterations"] == [1, 1] and S["last_step"] == [0.0, 0.0] and S["status"] == [0, 0] and S["scale"] == [1e300, 1e300]
    assert np.array_equal(out["robust_weights"], start["robust_weights"]) and S["lambda"] == start["summary"]["lambda"]


@pytest.mark.parametrize("loss", LOSSES)
def test_chain_every_iteration_from_the_previous_iterate(loss, hip):
    """The scenario with step_tolerance 0, max_iterations T and T + 1 for T = 0..4: fit_robust_ref.check_step on every pair."""
    s = fr.scenario()
    p = s.dirty
    runs = [_robust(hip, p.c, s.weights, max_iterations=T, step_tolerance=0.0, **_tuning(loss)) for T in range(6)]
    for T in range(5):
        result = fr.check_step(p, runs[T], runs[T + 1], loss, fr.SCENARIO_TUNING[loss], iterations=T + 1)
        print("loss %d T %d -> %d:" % (loss, T, T + 1), {k: "%.3g / %.3g" % v for k, v in result.items()})
        assert not fr.failed(result), (T, result)
    S = runs[5]["summary"]
    assert all(0 < S["n_downweighted"][g] for g in range(2)) and all((S["n_rejected"][g] > 0) == (loss == fr.TUKEY) for g in range(2))


def _check_selection(c, w, start, out, loss=fr.HUBER):
    """The median, the scale, psi and the counts of one reweighting (`out`, max_iterations 1) from iteration 0's residuals."""
    for g in range(2):
        use = np.ones(len(c.stamps), bool) if w is None else w[:, g] > 0
        S, e = out["summary"], start["residuals"][:, g]
        med = np.sort(e[use])[(use.sum() - 1) // 2]
        assert S["median_residual"][g] == med and S["n_used"][g] == use.sum(), (g, S["median_residual"][g], med)
        assert abs(S["scale"][g] - med / fr.CHI3_MEDIAN_ROOT) <= np.spacing(med / fr.CHI3_MEDIAN_ROOT)
        if S["scale"][g] == 0:
            assert S["status"][g] == fr.SCALE_ZERO
            continue
        want, u = fr.psi(loss, e[use], S["scale"][g], fr.DEFAULT_TUNING[loss]), out["robust_weights"][use, g]
        assert (np.abs(u - want) <= 4 * np.spacing(want)).all() and np.array_equal(u[(want == 0) | (want == 1)], want[(want == 0) | (want == 1)])
        assert S["n_downweighted"][g] == ((u > 0) & (u < 1)).sum() and S["n_rejected"][g] == (u == 0).sum()


@pytest.mark.parametrize("name", ["n1", "n2", "n3", "stamp-repeated-4x"])
def test_selection_on_few_samples_and_ties(name, hip):
    c = fit_ref.case(name)
    start, out = [_robust(hip, c, None, max_iterations=T, step_tolerance=0.0) for T in (0, 1)]
    _check_selection(c, None, start, out)
    if name == "stamp-repeated-4x":      # the four samples on one stamp have one residual
        e = start["residuals"][np.flatnonzero(c.stamps == c.stamps[257]), 0]
        assert len(e) == 4 and (e == e[0]).all()


@pytest.mark.parametrize("m", [63, 64, 65, 127, 128, 129])
def test_selection_at_the_wave_sizes(m, hip):
    """m samples of weight > 0: the first m in the rotation group, the last m in the position group, all others at weight 0."""
    c = fit_ref.case("rough-order6-f1")
    n = len(c.stamps)
    w = fs.sample_weights(n, seed=7)
    w[m:, 0] = 0.0
    w[:n - m, 1] = 0.0
    start, out = [_robust(hip, c, w, max_iterations=T, step_tolerance=0.0) for T in (0, 1)]
    assert out["summary"]["n_used"] == [m, m]
    _check_selection(c, w, start, out)


@pytest.mark.parametrize("loss", LOSSES)
def test_selection_over_many_workgroups(loss, hip):
    """109 201 samples on 57 control points: 427 workgroups of residuals, every selection pass over all of them."""
    c = fit_ref.inputs(dict(fit_ref._ragged(6, 1.0, 57, 21000.0), data=fit_ref.rough_data))
    assert 1.0e5 < len(c.stamps) < 1.2e5
    start, out = [_robust(hip, c, None, max_iterations=T, step_tolerance=0.0, loss=loss) for T in (0, 1)]
    _check_selection(c, None, start, out, loss)
    assert out["summary"]["status"] == [fr.MAX_ITERATIONS] * 2 and out["summary"]["n_downweighted"][0] > 0


def test_samples_of_weight_zero_are_not_read(hip):
    """A tenth of the samples per group at weight 0 with NaN data: ctrl, scale, median and u have the bits of the call without those
    samples, the left-out samples report u = 0 and residual NaN, n_used counts the rest."""
    c = fit_ref.case("rough-order6-f1")
    n = len(c.stamps)
    w = fs.sample_weights(n, seed=5)
    rng = np.random.default_rng(6)
    off = [rng.choice(n, n // 10, replace=False) for _ in range(2)]
    data = c.data.copy()
    for g in range(2):
        w[off[g], g] = 0.0
        data[off[g], 3 * g:3 * g + 3] = np.nan
    poisoned = fr.with_data(c, data)
    out = _robust(hip, poisoned, w, max_iterations=3, step_tolerance=0.0)
    assert out["summary"]["n_used"] == [n - n // 10] * 2 and np.isfinite(out["ctrl"]).all()
    for g in range(2):
        keep = np.setdiff1d(np.arange(n), off[g])
        part = _robust(hip, _without(poisoned, keep), np.ascontiguousarray(w[keep]), max_iterations=3, step_tolerance=0.0)
        assert np.array_equal(out["ctrl"][:, 3 * g:3 * g + 3], part["ctrl"][:, 3 * g:3 * g + 3]), g
        assert np.array_equal(out["robust_weights"][keep, g], part["robust_weights"][:, g]) and np.array_equal(out["residuals"][keep, g], part["residuals"][:, g])
        for key in ("scale", "median_residual", "lambda", "last_step", "iterations", "status", "n_downweighted", "n_rejected", "n_used"):
            assert out["summary"][key][g] == part["summary"][key][g], (key, g)
        assert (out["robust_weights"][off[g], g] == 0).all() and np.isnan(out["residuals"][off[g], g]).all()
        assert np.isfinite(out["residuals"][keep, g]).all()


def test_groups_are_independent(hip):
    s = fr.scenario()
    c = s.dirty.c
    a = _robust(hip, c, s.weights, max_iterations=4, step_tolerance=0.0)
    w2, data2 = s.weights.copy(), s.data.copy()
    w2[:, 1] = s.weights[::-1, 1]
    data2[:, 3:] = s.data[::-1, 3:] * 1.5
    b = _robust(hip, fr.with_data(c, data2), w2, fit=dict(lambda_pos=1e-2), max_iterations=4, step_tolerance=0.0, tuning_pos=1.5, scale_pos=0.3,
                min_scale_pos=0.01)
    _same_bits(a, b, groups=(0,))
    assert not np.array_equal(a["ctrl"][:, 3:], b["ctrl"][:, 3:]) and np.isnan(b["summary"]["median_residual"][1])


def test_early_out_stops_where_the_full_chain_would_be(hip):
    """Huber at step_tolerance 1e-9 on the scenario's clean data converges (the float64 restatement takes 14 and 10 iterations); each
    group has the bits of a call that runs exactly its number of iterations without a tolerance (but for the status, which is
    MAX_ITERATIONS there), and the call at the iteration limit has the same bits throughout."""
    s = fr.scenario()
    c = s.clean.c
    out = _robust(hip, c, s.weights)
    S = out["summary"]
    print("converged after", S["iterations"], "last steps", S["last_step"])
    assert S["status"] == [0, 0] and all(0 < it < 20 for it in S["iterations"]) and all(step <= 1e-9 for step in S["last_step"])
    for g in range(2):
        exact = _robust(hip, c, s.weights, max_iterations=S["iterations"][g], step_tolerance=0.0)
        assert exact["summary"]["status"][g] == fr.MAX_ITERATIONS
        _same_bits(out, exact, groups=(g,), but=("status",))
    _same_bits(out, _robust(hip, c, s.weights, max_iterations=64))


def test_other_statuses(hip):
    s = fr.scenario()
    c = s.dirty.c
    out = _robust(hip, c, s.weights, max_iterations=2)
    assert out["summary"]["status"] == [fr.MAX_ITERATIONS] * 2 and out["summary"]["iterations"] == [2, 2]
    # a position group whose data are all exactly 0
    data = s.data.copy()
    data[:, 3:] = 0.0
    flat = fr.with_data(c, data)
    start = _robust(hip, flat, s.weights, max_iterations=0)
    zero = _robust(hip, flat, s.weights, max_iterations=2)
    Z = zero["summary"]
    assert Z["status"] == [fr.MAX_ITERATIONS, fr.SCALE_ZERO] and Z["iterations"] == [2, 0] and Z["scale"][1] == 0.0 and Z["median_residual"][1] == 0.0
    assert np.array_equal(zero["ctrl"][:, 3:], start["ctrl"][:, 3:]) and (zero["ctrl"][:, 3:] == 0).all()
    assert np.array_equal(zero["robust_weights"][:, 1], (s.weights[:, 1] > 0).astype(float)) and Z["n_downweighted"][1] == 0
    _same_bits(zero, out, groups=(0,))
    floor = _robust(hip, flat, s.weights, min_scale_pos=1e-6)
    F = floor["summary"]
    assert F["status"][1] == 0 and F["iterations"][1] == 1 and F["scale"][1] == 1e-6 and F["last_step"][1] == 0.0 and (floor["ctrl"][:, 3:] == 0).all()
    # a caller's scale: nothing is selected
    fixed = _robust(hip, c, s.weights, max_iterations=2, scale_rot=0.1, scale_pos=0.2, step_tolerance=0.0)
    assert np.isnan(fixed["summary"]["median_residual"]).all() and fixed["summary"]["scale"] == [0.1, 0.2]
    start = _robust(hip, c, s.weights, max_iterations=1, scale_rot=0.1, scale_pos=0.2, step_tolerance=0.0)
    result = fr.check_step(s.dirty, start, fixed, fr.HUBER, fixed_scale=True, iterations=2)
    assert not fr.failed(result), result


@pytest.mark.parametrize("loss", LOSSES)
def test_scenario(loss, hip):
    """What the call is for (fit_robust_ref.check_scenario, the conditions the reference meets with a factor 1.5 to spare), with
    the call's defaults; and the distance of the fitted values from the long-double IRLS after the same iterations, held to 10 x
    the distance of the float64 restatement on the CPU (the only error measurement there is without a device; the factor covers
    the device's other summation order).
    Measured on the device (RMS, rotation / position): Huber 1.3e-12 / 2.6e-12, Tukey 6.2e-13 / 1.0e-12; the restatement shows the
    same to three digits (both carry the solve's 1e-15 ridge, which the long-double reference does not)."""
    s = fr.scenario()
    out = _robust(hip, s.dirty.c, s.weights, **_tuning(loss))
    result = fr.check_scenario(out, loss)
    assert not fr.failed(result), result
    T = tuple(out["summary"]["iterations"])
    ref = fr.reference_irls(s.dirty, loss, T, tuning=fr.SCENARIO_TUNING[loss])
    cpu = fr.restated_robust_fit(s.dirty, loss, T, tuning=fr.SCENARIO_TUNING[loss])
    for g in range(2):
        device, proxy = fr.rms_distance(s.dirty, g, out["ctrl"], ref["ctrl_ld"]), fr.rms_distance(s.dirty, g, cpu["ctrl"], ref["ctrl_ld"])
        print("loss %d group %d after %d iterations: device %.3e from the long-double IRLS, float64 restatement %.3e" % (loss, g, T[g], device, proxy))
        assert device <= 10 * proxy


def test_robust_fit_is_bit_reproducible(hip):
    s = fr.scenario()
    a, b = [_robust(hip, s.dirty.c, s.weights, loss=fr.TUKEY) for _ in range(2)]
    _same_bits(a, b)


def test_length_at_the_lds_ceiling(hip):
    """Order 6 at 2218 control points (the ceiling of [band | 3 rhs]): two reweighted iterations, the backward error of the last
    solve against the long-double system of the device's own weights and lambda."""
    c = fit_ref.inputs(dict(fit_ref._ragged(6, 1.0, 2218, 20.0), data=fit_ref.rough_data))
    p = fr.problem(c, fs.sample_weights(len(c.stamps)))
    out = _robust(hip, c, p.weights, max_iterations=2, step_tolerance=0.0)
    assert out["summary"]["status"] == [fr.MAX_ITERATIONS] * 2 and out["summary"]["replaced_pivots"] == [0, 0]
    for g in range(2):
        wu = np.asarray(p.weights[:, g], LD) * np.asarray(out["robust_weights"][:, g], LD)
        N, b = fs.normal_band(p.W, p.seg, wu, c.data[:, 3 * g:3 * g + 3], c.n_ctrl)
        eta = fs.backward_error(N + LD(out["summary"]["lambda"][g]) * p.P, b, out["ctrl"][:, 3 * g:3 * g + 3]).max()
        print("order 6 n_ctrl 2218 group %d eta %.1e, %d downweighted" % (g, eta, out["summary"]["n_downweighted"][g]))
        assert eta <= fit_ref.ETA_BOUND and out["summary"]["n_downweighted"][g] > 0


def test_one_control_point_past_the_ceiling_is_refused(hip):
    c = fit_ref.inputs(fit_ref._ragged(6, 1.0, 2219, 20.0))
    n = len(c.stamps)
    ctrl, u, e, summary = np.full((c.n_ctrl, 6), 7.5), np.full((n, 2), 7.5), np.full((n, 2), 7.5), _capi.SplineRobustSummary()
    rc = hip.fit_spline_robust(0, c.order, len(c.knots), dp(c.knots), dp(c.basis), n, dp(c.stamps), dp(c.data), None, None, None, dp(ctrl),
                               dp(u), dp(e), C.byref(summary))
    assert rc == _capi.UNIMPLEMENTED and (ctrl == 7.5).all() and (u == 7.5).all() and (e == 7.5).all()
    assert hip.last_error(None).decode().startswith("calico_fit_spline_robust: ")
