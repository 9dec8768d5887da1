"""The cross-validated fit's reference and criteria, proved on the CPU (tests/fit_cv_ref.py): the band recursion is the inverse, the
leverages add up to the effective degrees of freedom, PRESS is what leave-one-out refits give, the float64 restatement of the
device's steps passes every criterion the GPU test runs while each of five ways to get them wrong fails the one that is there for
it, and the fixtures of the choice leave the long-double reference an unambiguous, interior minimum at the noise's level."""
import numpy as np
import pytest

import fit_cv_ref as cv
import fit_ref
import fit_smooth_ref as fs

LD = np.longdouble
SMALL_CASES = [("n3", 2), ("one-per-segment", 2), ("order2-f0.1", 1), ("order8-f0.1", 3), ("gap-12-segments", 2)]


@pytest.mark.parametrize("name,m", SMALL_CASES)
def test_band_recursion_is_the_dense_inverse_on_the_band(name, m):
    """Long-double Takahashi on the long-double factor against a Newton-refined dense inverse: every band entry within
    1e-17 cond2(A) of the largest entry of the inverse (long double carries 64 bits: u = 5.4e-20)."""
    p = fs.problem(name, m)
    for (g, l), s in sorted(p.sys.items()):
        Z = cv.reference(p, g, l).Z
        X = cv.dense_inverse(s.A)
        n, k = Z.shape
        err = max(float(np.abs(Z[e:, e] - X[np.arange(e, n), np.arange(e, n) - e]).max()) for e in range(k))
        residual = float(np.abs(fs.band_to_dense(np.asarray(s.A, LD)) @ X - np.eye(n, dtype=LD)).max())
        print(name, m, g, l, "cond2 %.1e  band error %.1e  |A X - I| %.1e" % (s.cond, err, residual))
        assert residual <= 1e-17 * s.cond
        assert err <= 1e-17 * s.cond * float(np.abs(X).max())


@pytest.mark.parametrize("name,m", SMALL_CASES + [("rough-order6-f1", 2)])
def test_leverages_add_up_to_edf_and_lie_in_the_unit_interval(name, m):
    p = fs.problem(name, m)
    for (g, l), s in sorted(p.sys.items()):
        ref = cv.reference(p, g, l)
        assert abs(float(ref.h.sum() - ref.edf)) <= 1e-17 * s.cond * float(ref.edf)
        assert float(ref.h.min()) >= 0.0 and float(ref.h.max()) < 1.0 and 0.0 < float(ref.edf) <= p.c.n_ctrl
        # the smoother's null space is kept whatever lambda: m polynomial degrees of freedom at least
        assert float(ref.edf) >= m - 1e-9


def test_press_is_brute_force_leave_one_out_at_the_absolute_lambda():
    """one-per-segment (52 samples), m = 2, seeded weights: refit without each sample in long double at the row's absolute lambda;
    the left-out sample's residual is e_j / (1 - h_j), so their weighted mean square is PRESS. A refit at the relative lambda
    re-derived from the remaining data is not (the header says so): it differs by orders of magnitude more."""
    p = fs.problem("one-per-segment", 2)
    c, k = p.c, p.c.order
    assert len(c.stamps) <= 80
    for g in range(2):
        l = len(p.grid[g]) - 1
        s, w = p.sys[g, l], p.weights[:, g]
        d = c.data[:, 3 * g:3 * g + 3]
        sc = cv.scores_at(p, g, l, s.C_ref)
        total, total_relative = LD(0), LD(0)
        for j in range(len(c.stamps)):
            wj = w.copy()
            wj[j] = 0.0
            N, b = fs.normal_band(p.W, p.seg, wj, d, c.n_ctrl)
            pred = []
            for lam in (s.lam, LD(p.grid[g][l]) * N[:, 0].sum() / p.P[:, 0].sum()):
                C, _, _ = fs.reference_solve(N + lam * p.P, b)
                pred.append(np.asarray(p.W[j], LD) @ np.asarray(C, LD)[p.seg[j]:p.seg[j] + k] - np.asarray(d[j], LD))
            total += LD(w[j]) * (pred[0] ** 2).sum()
            total_relative += LD(w[j]) * (pred[1] ** 2).sum()
        brute, relative = float(total / (3 * p.n_used[g])), float(total_relative / (3 * p.n_used[g]))
        print("group %d press %.12e brute force %.12e (relative lambda re-derived: %.12e)" % (g, sc.press, brute, relative))
        assert abs(brute - sc.press) <= 1e-12 * sc.press       # (C of reference_solve is rounded to float64: 1e-16 cond of it)
        assert abs(relative - sc.press) > 1e-6 * sc.press


RESTATED = [("rough-order6-f1", 2), ("gap-12-segments", 2), ("one-per-segment", 2), ("order8-f0.1", 3), ("order2-f0.1", 1)]


@pytest.mark.parametrize("name,m", RESTATED)
def test_the_restated_algorithm_passes_every_criterion(name, m):
    p = fs.problem(name, m)
    result = cv.check(p, cv.restated_cv_fit(p))
    assert not cv.failed(result), result
    assert set(result) >= {"finite", "edf", "max_leverage", "gcv", "press", "leverage", "consistency", "zero_weight", "loo", "loo_infinite"}


@pytest.mark.parametrize("name", list(cv.SMALL))
def test_the_restated_algorithm_passes_on_one_and_two_segments(name):
    p = cv.small_problem(name)
    assert p.c.n_ctrl - p.c.order in (0, 1) and max(s.cond for s in p.sys.values()) <= fs.COND_BOUND
    result = cv.check(p, cv.restated_cv_fit(p))
    assert not cv.failed(result), result


# fault -> the criterion that is there for it
EXPECTED = {"offdiagonal_once": "leverage", "edf_from_a": "edf", "weight_missing_in_h": "leverage", "recursion_one_column_short": "leverage",
            "press_not_squared": "press"}


@pytest.mark.parametrize("fault", cv.FAULTS)
def test_every_fault_fails_its_criterion(fault):
    for name, m in (("rough-order6-f1", 2), ("gap-12-segments", 2)):
        p = fs.problem(name, m)
        result = cv.check(p, cv.restated_cv_fit(p, fault=fault), verbose=False)
        assert EXPECTED[fault] in cv.failed(result), (fault, name, result)


def test_the_faults_are_all_there():
    assert set(EXPECTED) == set(cv.FAULTS) and len(cv.FAULTS) == 5


def test_a_weight_of_zero_gives_zero_and_nan():
    c = fit_ref.case("rough-order6-f1")
    w = fs.sample_weights(len(c.stamps), seed=5)
    w[::7, 0] = 0.0
    w[3::11, 1] = 0.0
    p = fs.build(c, w, 2, (1e-3,), (1e-3,))
    out = cv.restated_cv_fit(p)
    for g in range(2):
        off = w[:, g] == 0
        assert off.any() and (out["leverage"][g][0][off] == 0).all() and np.isnan(out["loo"][g][0][off]).all()
    result = cv.check(p, out, verbose=False)
    assert not cv.failed(result), result


@pytest.mark.parametrize("sigma,weighted", cv.CHOICE_CASES)
def test_choice_fixtures_have_an_unambiguous_interior_minimum_at_the_noise_level(sigma, weighted):
    """Per group and criterion, in long double: the best and second-best scores of the 25-point grid differ by >= 1e-4 relative,
    the minimum is not at an end of the grid, and the RMS of the residuals there (unweighted: the noise has one sigma whatever the
    weights) is within 5 % of sigma -- the criterion recovers a noise level it was never told."""
    p = cv.choice_problem(sigma, weighted)
    assert len(cv.CHOICE_GRID) == 25 and cv.CHOICE_GRID[0] == 1e-8 and cv.CHOICE_GRID[-1] == 1e4
    ref = cv.reference_scores(p)
    for g in range(2):
        for name in cv.CRITERIA:
            s = np.array(ref[name][g])
            best = cv.choose(s)
            second = np.sort(s)[1]
            rms = ref["rms"][g][best]
            print("sigma %g weighted %d group %d %s: chosen %d (lambda %.1e), gap %.2e, rms %.5f" % (
                sigma, weighted, g, name, best, cv.CHOICE_GRID[best], (second - s[best]) / s[best], rms))
            assert (second - s[best]) / s[best] >= cv.CHOICE_GAP
            assert 0 < best < len(s) - 1
            assert abs(rms - sigma) <= cv.CHOICE_RMS * sigma
    # the restatement chooses what the reference chooses
    for name in cv.CRITERIA:
        assert cv.restated_cv_fit(p, criterion=name)["chosen"] == [cv.choose(ref[name][g]) for g in range(2)]
