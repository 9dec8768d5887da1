"""The cross-validated spline fit on the device (`-m gpu`): calico_fit_spline_cv against tests/fit_cv_ref.py (proved on the CPU in
test_fit_cv_reference.py) over the smoothing fit's sweep, one and two segments, and the length at the LDS ceiling; the choice
against the long-double reference's on noisy data; and the contracts of the call: rows, every lambda's control points and the
chosen ones are calico_fit_spline_smooth's bit for bit, the group statuses, rows that replaced a pivot are never chosen, samples of
weight 0 are not read, determinism.

The per-sample outputs belong to the chosen lambda, so the sweep calls once with the entry's grid (scores, bit identity) and once
per lambda with that lambda alone (leverages, leave-one-out residuals); the one-lambda call's cv row has the grid call's bits.

What the ridge does to h = 1: the factor is that of A + 1e-15 mean_diag I, so on an interpolating fit (as many samples as control
points) the device's h is 1 - O(1e-15), not 1, and which side of 1 it rounds to is not the caller's to choose. The +inf branches
are therefore tested for consistency (test_an_interpolating_fit_is_consistent_about_infinity), not forced."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import fit_cv_ref as cv
import fit_ref
import fit_smooth_ref as fs
from calico_amd import _capi, synthetic as syn

pytestmark = pytest.mark.gpu


def dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _options(hip, **options):
    return _capi.default_spline_fit_options(hip, **options) if options else None


def _cv(hip, c, weights=None, criterion=None, **options):
    co = None if criterion is None else _capi.default_spline_cv_options(hip, criterion=criterion)
    return _capi.fit_spline_cv(hip, c.order, c.knots, c.basis, c.stamps, c.data, weights, _options(hip, **options), co)


def _smooth(hip, c, weights=None, **options):
    return _capi.fit_spline_smooth(hip, c.order, c.knots, c.basis, c.stamps, c.data, weights, _options(hip, **options))


def _same_as_the_smoothing_fit(out, smooth):
    """rows, every lambda's control points, and each group's chosen control points: calico_fit_spline_smooth's bits."""
    assert out["rows"] == smooth["rows"] and np.array_equal(out["ctrl_all"], smooth["ctrl_all"], equal_nan=True)
    for g in range(2):
        assert np.array_equal(out["ctrl"][:, 3 * g:3 * g + 3], smooth["ctrl_all"][out["chosen"][g]][:, 3 * g:3 * g + 3])


def _run(hip, p, label=""):
    """The grid call and the one-lambda calls of problem p, held to cv.check and to the smoothing fit's bits. Returns the grid call."""
    c, nl = p.c, len(p.grid[0])
    out = _cv(hip, c, p.weights, derivative=p.m, lambda_rot=p.grid[0], lambda_pos=p.grid[1])
    _same_as_the_smoothing_fit(out, _smooth(hip, c, p.weights, derivative=p.m, lambda_rot=p.grid[0], lambda_pos=p.grid[1]))
    assert out["summary"]["n_used"] == p.n_used and out["chosen"] == out["summary"]["chosen"]
    out["loo"] = [[None] * nl for _ in range(2)]
    out["leverage_at_choice"], out["leverage"] = out["leverage"], [[None] * nl for _ in range(2)]
    for l in range(nl):
        one = _cv(hip, c, p.weights, derivative=p.m, lambda_rot=p.grid[0][l], lambda_pos=p.grid[1][l])
        assert one["chosen"] == [0, 0] and one["summary"]["status"] == [0, 0]      # (one entry is no grid: never AT_GRID_END)
        for g in range(2):
            assert one["cv_rows"][g][0] == out["cv_rows"][g][l] and one["rows"][g][0] == out["rows"][g][l], (g, l)
            assert one["summary"]["edf"][g] == out["cv_rows"][g][l]["edf"]
            out["leverage"][g][l], out["loo"][g][l] = one["leverage"][:, g], one["loo_residuals"][:, g]
            if out["chosen"][g] == l:      # the grid call's per-sample outputs are the chosen lambda's
                assert np.array_equal(out["leverage_at_choice"][:, g], one["leverage"][:, g])
                assert np.array_equal(out["loo_residuals"][:, g], one["loo_residuals"][:, g], equal_nan=True)
    result = cv.check(p, out, label=label)
    assert not cv.failed(result), result
    assert set(result) >= {"finite", "edf", "max_leverage", "gcv", "press", "leverage", "consistency", "zero_weight", "loo", "loo_infinite"}
    return out


@pytest.mark.parametrize("name,m", list(fs.SWEEP))
def test_cv_fit_sweep_against_long_double(name, m, hip):
    """Per (group, lambda) of the entry's grid (fit_cv_ref.check), with hb = 1e-14 cond2(A) + 1e-13: |h - h_ref| <= hb for every
    sample and for the largest; |sum h - edf| <= hb n_used; |edf - edf_ref| <= hb edf_ref; gcv and press within the bounds that rss's
    bound and hb give through their formulas (fit_cv_ref.scores_at), against long double at the device's own control points."""
    _run(hip, fs.problem(name, m))


@pytest.mark.parametrize("name", list(cv.SMALL))
def test_one_and_two_segments(name, hip):
    """n_ctrl = order and order + 1 at orders 2, 6, 8: the recursion's steps all run short of the full band."""
    _run(hip, cv.small_problem(name))


def test_length_at_the_lds_ceiling(hip):
    """Order 6, 2218 control points: the selected inversion over the longest factor the solve accepts, against the long-double
    recursion on the band (cond2 from the eigenvalues of the float64 matrix)."""
    c = fit_ref.inputs(fit_ref._ragged(6, 1.0, 2218, 20.0))
    c.name = "order6-2218"
    p = fs.build(c, fs.sample_weights(len(c.stamps)), 2, (1e-3,), (1e-3,), reference=False)
    for s in p.sys.values():
        ev = np.linalg.eigvalsh(np.asarray(fs.band_to_dense(s.A), float))
        s.cond = float(ev[-1] / ev[0])
        assert ev[0] > 0 and s.cond <= fs.COND_BOUND
    out = _run(hip, p)
    assert all(out["rows"][g][0]["replaced_pivots"] == 0 for g in range(2))


@pytest.mark.parametrize("criterion", cv.CRITERIA)
@pytest.mark.parametrize("sigma,weighted", cv.CHOICE_CASES)
def test_the_choice_is_the_references(sigma, weighted, criterion, hip):
    """smooth_data + sigma N(0, 1) on a 25-point grid: each group's chosen lambda is the long-double reference's (whose best and
    second-best scores differ by >= 1e-4, test_fit_cv_reference.py), interior, and the summary and ctrl_out are that row's."""
    p = cv.choice_problem(sigma, weighted)
    ref = cv.reference_scores(p)
    out = _cv(hip, p.c, p.weights if weighted else None, criterion=_capi.FIT_CV_GCV if criterion == "gcv" else _capi.FIT_CV_PRESS,
              lambda_rot=cv.CHOICE_GRID, lambda_pos=cv.CHOICE_GRID)
    want = [cv.choose(ref[criterion][g]) for g in range(2)]
    print("sigma %g weighted %d %s: chosen %s (lambda %.1e, %.1e), edf %s, rms %s" % (
        sigma, weighted, criterion, out["chosen"], cv.CHOICE_GRID[out["chosen"][0]], cv.CHOICE_GRID[out["chosen"][1]], out["summary"]["edf"],
        [out["rows"][g][out["chosen"][g]]["rms"] for g in range(2)]))
    assert out["chosen"] == want and out["summary"]["status"] == [_capi.FIT_OK] * 2
    for g in range(2):
        row = out["cv_rows"][g][want[g]]
        assert out["summary"]["edf"][g] == row["edf"] and out["summary"]["score"][g] == row[criterion]
        assert row[criterion] == min(r[criterion] for r in out["cv_rows"][g])
        assert np.array_equal(out["ctrl"][:, 3 * g:3 * g + 3], out["ctrl_all"][want[g]][:, 3 * g:3 * g + 3])


def test_a_truncated_grid_ends_at_grid_end(hip):
    """The grid cut off below the minimum ends at its last entry, cut off above it at its first: CALICO_FIT_CV_AT_GRID_END, and the
    call succeeds. One entry alone is no grid and reports CALICO_FIT_OK."""
    p = cv.choice_problem(0.01, False)
    ref = cv.reference_scores(p)["gcv"]
    for lo, hi, end in ((12, 17, 4), (18, 23, 0)):
        assert all(cv.choose(ref[g][lo:hi]) == end for g in range(2))
        out = _cv(hip, p.c, lambda_rot=cv.CHOICE_GRID[lo:hi], lambda_pos=cv.CHOICE_GRID[lo:hi])
        assert out["chosen"] == [end, end] and out["summary"]["status"] == [_capi.FIT_CV_AT_GRID_END] * 2
        assert np.array_equal(out["ctrl"], out["ctrl_all"][end]) and np.isfinite(out["leverage"]).all()
    # the groups end separately: the rotation grid around its minimum, the position grid below it
    out = _cv(hip, p.c, lambda_rot=cv.CHOICE_GRID[15:20], lambda_pos=cv.CHOICE_GRID[10:15])
    assert out["summary"]["status"] == [_capi.FIT_OK, _capi.FIT_CV_AT_GRID_END] and out["chosen"] == [cv.choose(ref[0][15:20]), 4]
    one = _cv(hip, p.c, lambda_rot=cv.CHOICE_GRID[3], lambda_pos=cv.CHOICE_GRID[3])
    assert one["summary"]["status"] == [_capi.FIT_OK] * 2 and one["chosen"] == [0, 0]


def test_rows_that_replaced_a_pivot_are_never_chosen(hip):
    """one-per-segment has fewer samples than control points: at lambda 0 the factorisation replaces pivots, the smoothing fit still
    returns that row's control points, and cross-validation must not use it (the factor is not A's) -- its cv row is NaN and the
    choice is among the others, although its rss is the smallest. With lambda 0 alone no row is eligible: kInternal,
    CALICO_FIT_NOT_POSITIVE_DEFINITE, chosen -1, and ctrl_out, leverage_out and loo_residuals_out are not written."""
    c = fit_ref.case("one-per-segment")
    grid = (0.0, 1e-3, 1.0)
    out = _cv(hip, c, lambda_rot=grid, lambda_pos=grid)
    _same_as_the_smoothing_fit(out, _smooth(hip, c, lambda_rot=grid, lambda_pos=grid))
    for g in range(2):
        rows = out["rows"][g]
        assert rows[0]["status"] == 0 and rows[0]["replaced_pivots"] > 0 and rows[0]["rss"] < min(rows[1]["rss"], rows[2]["rss"])
        assert np.isfinite(out["ctrl_all"][0][:, 3 * g:3 * g + 3]).all()
        assert all(np.isnan(v) for v in out["cv_rows"][g][0].values())
        assert all(np.isfinite(v) for l in (1, 2) for v in out["cv_rows"][g][l].values())
        assert out["chosen"][g] in (1, 2)
    n = len(c.stamps)
    ctrl, h, loo = np.full((c.n_ctrl, 6), 7.5), np.full((n, 2), 7.5), np.full((n, 2), 7.5)
    ctrl_all, rows, cv_rows, summary = np.full((1, c.n_ctrl, 6), 7.5), (_capi.SplineFitRow * 2)(), (_capi.SplineCvRow * 2)(), _capi.SplineCvSummary()
    o = _capi.default_spline_fit_options(hip, lambda_rot=0.0, lambda_pos=0.0)
    rc = hip.fit_spline_cv(0, c.order, len(c.knots), dp(c.knots), dp(c.basis), n, dp(c.stamps), dp(c.data), None, C.byref(o), None, dp(ctrl), dp(ctrl_all),
                           rows, cv_rows, dp(h), dp(loo), C.byref(summary))
    assert rc == _capi.INTERNAL and hip.last_error(None).decode().startswith("calico_fit_spline_cv: no lambda of the rotation grid")
    assert list(summary.status) == [_capi.FIT_NOT_POSITIVE_DEFINITE] * 2 and list(summary.chosen) == [-1, -1] and list(summary.n_used) == [n, n]
    assert np.isnan(list(summary.edf)).all() and np.isnan(list(summary.score)).all()
    assert (ctrl == 7.5).all() and (h == 7.5).all() and (loo == 7.5).all()
    assert np.isfinite(ctrl_all).all() and rows[0].replaced_pivots > 0 and np.isnan(cv_rows[0].edf) and np.isnan(cv_rows[1].press)


def test_an_interpolating_fit_is_consistent_about_infinity(hip):
    """Order 2 with one sample on every knot and lambda 0: X is the identity, every h_j is 1 up to the ridge and rounding
    (>= 1 - 1e-14), edf is n_used up to the same. Whichever side of 1 they fall: loo is +inf exactly where h >= 1, press is +inf
    exactly when some h >= 1, gcv is +inf exactly when edf >= n_used, nothing is NaN, and the call succeeds."""
    knots = fit_ref.uniform_knots(9, 2)
    c = SimpleNamespace(order=2, n_ctrl=9, knots=knots, basis=np.ascontiguousarray(syn.basis_matrices(knots, 2)),
                        stamps=np.ascontiguousarray(knots[1:-1]))
    c.data = np.ascontiguousarray(fit_ref.rough_data(c.stamps))
    assert len(c.stamps) == c.n_ctrl
    for w in (None, fs.sample_weights(9)):
        out = _cv(hip, c, w, derivative=1, lambda_rot=0.0, lambda_pos=0.0)
        for g in range(2):
            h, loo, row = out["leverage"][:, g], out["loo_residuals"][:, g], out["cv_rows"][g][0]
            print("interpolating, group %d: 1 - h in [%.1e, %.1e], edf - n %.1e, gcv %g, press %g" % (g, 1 - h.max(), 1 - h.min(), row["edf"] - 9, row["gcv"], row["press"]))
            assert out["rows"][g][0]["replaced_pivots"] == 0 and (np.abs(h - 1) <= 1e-14).all() and abs(row["edf"] - 9) <= 9e-14
            assert not np.isnan(loo).any() and np.array_equal(np.isinf(loo), h >= 1.0)
            assert row["max_leverage"] == h.max() and not np.isnan([row["gcv"], row["press"]]).any()
            assert (row["press"] == np.inf) == bool((h >= 1.0).any()) and (row["gcv"] == np.inf) == bool(row["edf"] >= 9)
            assert out["chosen"][g] == 0 and out["summary"]["status"][g] == _capi.FIT_OK


def test_samples_of_weight_zero_are_not_read(hip):
    """A tenth of the samples at weight 0 in the rotation column, another tenth in the position column, their channels NaN: leverage
    0 and leave-one-out residual NaN there, every criterion met on the rest, n_used counts the rest."""
    c = fit_ref.case("rough-order6-f1")
    n = len(c.stamps)
    w = fs.sample_weights(n, seed=5)
    rng = np.random.default_rng(6)
    data = c.data.copy()
    for g in range(2):
        off = rng.choice(n, n // 10, replace=False)
        w[off, g] = 0.0
        data[off, 3 * g:3 * g + 3] = np.nan
    poisoned = SimpleNamespace(name="rough-order6-f1 with weights of 0", order=c.order, n_ctrl=c.n_ctrl, knots=c.knots, basis=c.basis, stamps=c.stamps,
                               data=data)
    p = fs.build(poisoned, w, 2, (1e-4, 1e-2), (1e-4, 1e-2))
    out = _run(hip, p)
    assert out["summary"]["n_used"] == [n - n // 10] * 2
    for g in range(2):
        off = w[:, g] == 0
        assert (out["leverage_at_choice"][off, g] == 0).all() and np.isnan(out["loo_residuals"][off, g]).all()
        assert (out["leverage_at_choice"][~off, g] > 0).all() and np.isfinite(out["loo_residuals"][~off, g]).all()


def test_cv_fit_is_bit_reproducible(hip):
    p = cv.choice_problem(0.01, True)
    a, b = [_cv(hip, p.c, p.weights, criterion=_capi.FIT_CV_PRESS, lambda_rot=cv.CHOICE_GRID, lambda_pos=cv.CHOICE_GRID) for _ in range(2)]
    assert a["rows"] == b["rows"] and a["cv_rows"] == b["cv_rows"] and a["summary"] == b["summary"]
    for key in ("ctrl", "ctrl_all", "leverage", "loo_residuals"):
        assert np.array_equal(a[key], b[key]), key
