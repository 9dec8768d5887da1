"""The robust fit's reference and criteria, proved on the CPU (tests/fit_robust_ref.py): the float64 restatement of the algorithm
passes every criterion of the chain that the GPU test runs (each iteration checked from the previous iterate), each of seven ways
to get the algorithm wrong fails the criterion that is there for it, and the scenario's inputs leave the long-double reference a
factor 1.5 to spare on what the robust fit is for."""
import numpy as np
import pytest

import fit_robust_ref as fr


@pytest.fixture(scope="module")
def chains():
    """{loss: the unfaulted restatement after T = 0..3 iterations on the scenario}, built once."""
    p = fr.scenario().dirty
    return {loss: [fr.restated_robust_fit(p, loss, T, tuning=fr.SCENARIO_TUNING[loss]) for T in range(4)] for loss in (fr.HUBER, fr.TUKEY)}


@pytest.mark.parametrize("loss", [fr.HUBER, fr.TUKEY])
def test_the_restated_algorithm_passes_the_chain(loss, chains):
    p = fr.scenario().dirty
    for T in range(3):
        result = fr.check_step(p, chains[loss][T], chains[loss][T + 1], loss, fr.SCENARIO_TUNING[loss], iterations=T + 1)
        assert not fr.failed(result), (T, result)
        assert set(result) >= {"median", "scale", "psi", "psi_exact", "lambda", "eta", "replaced_pivots", "rss", "counts", "iterations"}
    # the chain exercises both ends of psi: samples at exactly 1 and downweighted ones; with Tukey rejected ones
    S = chains[loss][3]["summary"]
    assert all(0 < S["n_downweighted"][g] < S["n_used"][g] for g in range(2))
    assert all((S["n_rejected"][g] > 0) == (loss == fr.TUKEY) for g in range(2))
    assert S["n_used"] == [494, 494] and S["median_residual"][0] != S["median_residual"][1]


# fault -> (the loss that shows it, the criterion that is there for it)
EXPECTED = {"upper_median": (fr.HUBER, "median"), "median_over_weight_zero": (fr.HUBER, "median"), "mad_constant": (fr.HUBER, "scale"),
            "lambda_rederived": (fr.HUBER, "lambda"), "prior_weight_dropped": (fr.HUBER, "eta"), "tukey_no_cutoff": (fr.TUKEY, "psi_exact"),
            "huber_squared": (fr.HUBER, "psi")}


@pytest.mark.parametrize("fault", fr.FAULTS)
def test_every_fault_fails_its_criterion(fault):
    loss, criterion = EXPECTED[fault]
    p = fr.scenario().dirty
    for T in (0, 1):
        prev, cur = [fr.restated_robust_fit(p, loss, t, fault=fault, tuning=fr.SCENARIO_TUNING[loss]) for t in (T, T + 1)]
        result = fr.check_step(p, prev, cur, loss, fr.SCENARIO_TUNING[loss], iterations=T + 1)
        assert criterion in fr.failed(result), (fault, T, result)


def test_the_faults_are_all_there():
    assert set(EXPECTED) == set(fr.FAULTS) and len(fr.FAULTS) == 7


@pytest.mark.parametrize("loss", [fr.HUBER, fr.TUKEY])
def test_scenario_leaves_the_reference_a_factor_to_spare(loss):
    """The long-double IRLS with the call's defaults (20 iterations, tolerance 1e-9) and the scenario's tuning meets the scenario's
    conditions with a factor 1.5 to spare; the float64 restatement after the same iterations meets them as they stand and lies
    within 1e-10 (RMS of the fitted values) of the reference."""
    s = fr.scenario()
    assert all(len(s.displaced[g]) == 52 and not np.intersect1d(s.displaced[g], s.off[g]).size for g in range(2))
    ref = fr.reference_irls(s.dirty, loss, 20, tolerance=1e-9, tuning=fr.SCENARIO_TUNING[loss])
    result = fr.check_scenario(ref, loss, spare=1.5)
    assert not fr.failed(result), result
    out = fr.restated_robust_fit(s.dirty, loss, ref["summary"]["iterations"], tuning=fr.SCENARIO_TUNING[loss])
    assert not fr.failed(fr.check_scenario(out, loss, verbose=False))
    for g in range(2):
        d = fr.rms_distance(s.dirty, g, out["ctrl"], ref["ctrl_ld"])
        print("loss %d group %d: float64 restatement %.2e from the long-double reference" % (loss, g, d))
        assert 0 < d <= 1e-10
    # the smoothing fit itself fails what the robust fit is for
    assert "distance_0" in fr.failed(fr.check_scenario(fr.restated_robust_fit(s.dirty, loss, 0), loss, verbose=False))


def test_psi_and_the_median_are_what_the_header_says():
    e = np.array([0.0, 0.1, 0.2, 0.3, 1e300])
    assert np.array_equal(fr.psi(fr.HUBER, e, 0.1, 2.0), [1.0, 1.0, 1.0, 2.0 / (0.3 / 0.1), 2.0 / (1e300 / 0.1)])
    t = fr.psi(fr.TUKEY, e, 0.1, 2.5)
    assert t[0] == 1.0 and t[3] == 0.0 and t[4] == 0.0 and t[1] == (1 - (0.1 / 0.1 / 2.5) ** 2) ** 2
    assert fr.lower_median(np.array([3.0, 1.0])) == 1.0 and fr.lower_median(np.array([3.0, 1.0, 2.0])) == 2.0 and fr.lower_median(np.array([5.0])) == 5.0
    # sqrt(median of chi2_3): the median of chi2_3 solves P(3/2, x/2) = 1/2, x = 2.3659738843753377
    assert abs(fr.CHI3_MEDIAN_ROOT ** 2 - 2.3659738843753377) < 1e-15
    assert abs(fr.DEFAULT_TUNING[fr.HUBER] ** 2 - 7.8147) < 1e-3 and fr.DEFAULT_TUNING[fr.TUKEY] == 2 * fr.DEFAULT_TUNING[fr.HUBER]
