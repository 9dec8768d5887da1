"""tests/fit_ref.py proved on the CPU (no GPU): its reference solves the fit exactly, every case of the GPU sweep meets the
sweep's input condition, the device's algorithm restated in float64 passes every criterion on every case, and the criteria
reject fits that are wrong by a little."""
import numpy as np
import pytest

import fit_ref
from calico_amd import synthetic as syn

SHORT = [n for n, s in fit_ref.CASES.items() if s["n_ctrl"] == 57]      # (the long cases' references take seconds each)


# ---- the input condition of the GPU sweep, for every case ----
@pytest.mark.parametrize("name", list(fit_ref.CASES))
def test_case_meets_the_input_condition(name):
    c = fit_ref.case(name)
    vk = c.knots[c.order - 1:len(c.knots) - (c.order - 1)]
    assert len(c.knots) - c.order == c.n_ctrl and c.X.shape == (len(c.stamps), c.n_ctrl)
    assert (np.diff(c.stamps) >= 0).all() and c.stamps[0] >= vk[0] and c.stamps[-1] <= vk[-1]
    assert c.n_ctrl * (c.order + 6) * 8 <= fit_ref.LDS_CEILING
    near = c.pivots[(c.pivots > 1e-18) & (c.pivots < 1e-10)]
    print("%-22s n %4d pivots within three decades of the rule: %s" % (name, len(c.stamps), near))
    if c.kind == "posed":
        # the decoupling comparison needs every exact pivot a decade away from the rule; the named cases run eta only
        assert c.in_band == (name in fit_ref.BAND_CASES)
    else:
        touched = (c.X != 0.0).any(0).sum()
        assert len(np.unique(c.stamps)) < touched      # fewer distinct samples than the control points they touch


def test_the_sweep_covers_what_it_says():
    ragged = {k: [n for n in fit_ref.CASES if n.startswith("order%d-f0." % k)] for k in range(2, 9)}
    for k, names in ragged.items():
        assert len(names) == 3
        assert sum(n in fit_ref.BAND_CASES for n in names) <= 1             # at most one case per order in the band
        assert any(not fit_ref.case(n).in_band for n in names)             # and a ragged end outside it
    assert fit_ref.BAND_CASES <= set(fit_ref.CASES)
    # the cliff: order 6 with the last sample 10 % into the last segment loses its last control point although the design
    # matrix has full rank; at 50 % nothing is dropped
    c = fit_ref.case("order6-f0.1")
    assert np.linalg.matrix_rank(c.X) == 57 and list(np.flatnonzero(c.pivots <= fit_ref.PIVOT_RULE)) == [56]
    assert (fit_ref.case("order6-f0.5").pivots > fit_ref.PIVOT_RULE).all()
    # the gaps: twelve empty segments leave seven control points untouched, four and a half leave none
    assert list(np.flatnonzero(~(fit_ref.case("gap-12-segments").X != 0).any(0))) == list(range(25, 32))
    assert (fit_ref.case("gap-4.5-segments").X != 0).any(0).all()
    # the LDS sizes: 683 is the first order-6 length above 64 KiB, 1664 and 1426 are the last below the ceiling
    assert 682 * 12 * 8 <= 64 * 1024 < 683 * 12 * 8
    assert 1664 * 12 * 8 == fit_ref.LDS_CEILING < 1665 * 12 * 8
    assert 1426 * 14 * 8 <= fit_ref.LDS_CEILING < 1427 * 14 * 8
    for name, spec in fit_ref.TOO_LONG.items():
        assert spec["n_ctrl"] * (spec["order"] + 6) * 8 > fit_ref.LDS_CEILING
    # stamps on knots are exactly the valid knots; the repeated stamp appears four times
    c = fit_ref.case("stamps-on-knots")
    assert np.array_equal(c.stamps, c.knots[5:-5]) and c.seg[-1] == c.seg[-2] == len(c.stamps) - 2
    c = fit_ref.case("stamp-repeated-4x")
    assert np.unique(c.stamps, return_counts=True)[1].max() == 4
    assert len(np.unique(fit_ref.case("all-in-one-segment").seg)) == 1


@pytest.mark.parametrize("name", fit_ref.ORACLE_CASES)
def test_oracle_cases_have_the_knots_the_oracle_builds(name):
    c = fit_ref.case(name)
    assert np.array_equal(syn.knot_vector(c.stamps[0], c.stamps[-1], c.order, fit_ref.KNOT_HZ), c.knots)
    last = c.knots[-c.order]
    assert last - 2 * np.spacing(last) <= c.stamps[-1] <= last       # the last valid knot: the last segment is fully covered


# ---- the reference itself ----
@pytest.mark.parametrize("name", ["order2-f0.5", "order4-f1", "order6-f0.5", "order6-f0.1", "order8-f0.1", "gap-12-segments",
                                  "two-per-segment", "rough-order6-f1"])
def test_reference_solves_the_normal_equations(name):
    """reference_fit never forms N, yet its control points solve N C = b to the last bits, the dropped rows included (an
    exact pivot of ~0 means the row depends on the rows before it), and match minimum-norm least squares where nothing drops."""
    c, r = fit_ref.case(name), fit_ref.reference(name)
    eta = fit_ref.backward_error(c.X, c.data, r.C_ref).max()
    print("%s: cond2 %.2e dropped %s eta(ref) %.2e" % (name, r.cond, list(np.flatnonzero(~r.kept)), eta))
    assert eta <= 2e-15
    if r.kept.all():
        assert np.abs(fit_ref.minimum_norm_fit(c.X, c.data) - r.C_ref).max() <= 1e-16 * r.cond ** 2 * np.abs(r.C_ref).max() + 1e-13


def test_what_the_rule_costs_where_noise_meets_the_cliff():
    """Order 6, last sample 10 % into the last segment: the last control point's exact pivot is 3e-16 mean_diag, not zero, so
    dropping it leaves a residual in its row of the normal equations. On the smooth channels that residual is lost in the
    roundoff (eta 6e-16, |C_56| 5e-16). With noise of sigma 0.1 on the samples the contract's own answer has eta 9e-12, just
    inside the sweep's 1e-11, and the device's algorithm returns |C_56| = 7e-10: "~ 0" then means sqrt(pivot / mean_diag)
    times the noise, not 1e-12. Least squares on every column would spend that control point (weight u^5 / 120 <= 8e-8 at the
    last ten samples) on their noise: |C_56| 2e6, fitted values 0.05 away, half the noise's sigma. Recorded here, on the CPU, so that a change to the rule or the ridge shows; the device sweep keeps to cases where a dropped
    control point is ~ 0 to 1e-12."""
    c = fit_ref.inputs(fit_ref.NOISY_CLIFF)
    X, _ = fit_ref.design_matrix(c.knots, c.basis, c.order, c.stamps)
    C_ref, kept, cond, piv = fit_ref.reference_fit(X, c.data)
    assert list(np.flatnonzero(~kept)) == [56] and 1e-16 < piv[56] < 1e-15
    eta = fit_ref.backward_error(X, c.data, C_ref).max()
    C = fit_ref.restated_fit(c.knots, c.basis, c.order, c.stamps, c.data)
    full = fit_ref.minimum_norm_fit(X, c.data)
    moved = np.abs(X @ (full - C)).max()
    print("contract: eta %.2e; restated algorithm: eta %.2e |C_56| %.2e; least squares on every column: |C_56| %.2e, fitted values %.2e away"
          % (eta, fit_ref.backward_error(X, c.data, C).max(), np.abs(C[56]).max(), np.abs(full[56]).max(), moved))
    assert 1e-12 < eta <= fit_ref.ETA_BOUND
    assert 1e-10 < np.abs(C[56]).max() < 1e-8
    assert np.abs(C - C_ref)[kept].max() <= fit_ref.forward_bound(cond, C_ref, c.data)
    assert np.abs(full[56]).max() > 1e4 and 1e-3 < moved < 0.1           # (the noise's sigma)


def test_exact_pivots_against_a_dense_long_double_cholesky():
    c = fit_ref.case("order5-f0.5")
    N = np.asarray(c.X, np.longdouble).T @ np.asarray(c.X, np.longdouble)
    assert np.abs(fit_ref.normal_matrix_ld(c.X) - N).max() <= 1e-17 * float(np.abs(N).max())
    mean_diag = np.trace(N) / len(N)
    L = np.zeros_like(N)
    for j in range(len(N)):             # left-looking, dense: another order of the same sums
        L[j, j] = np.sqrt(N[j, j] - (L[j, :j] ** 2).sum())
        L[j + 1:, j] = (N[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    assert np.abs(np.diag(L).astype(float) ** 2 / float(mean_diag) - c.pivots).max() <= 1e-12 * c.pivots.max()


# ---- the device's algorithm in float64 passes every criterion on every case ----
@pytest.mark.parametrize("name", SHORT)
def test_restated_algorithm_passes(name):
    c = fit_ref.case(name)
    result = fit_ref.check(c, fit_ref.restated_fit(c.knots, c.basis, c.order, c.stamps, c.data))
    assert not fit_ref.failed(result), result


# ---- the test of the test: one fault at a time ----
@pytest.mark.parametrize("fault", fit_ref.FAULTS)
@pytest.mark.parametrize("name", ["rough-order6-f1", "rough-order6-f0.5"])
def test_criteria_reject_a_seeded_fault(name, fault):
    """With the last segment covered (cond2 1.8e3) the backward error, the kept columns and the fitted values each reject each
    fault. At the ragged end (cond2 4.3e4, the bound on the forward errors 6e2 times wider) the backward error, which does not
    depend on the conditioning, still rejects each of them."""
    c = fit_ref.case(name)
    clean = fit_ref.check(c, fit_ref.restated_fit(c.knots, c.basis, c.order, c.stamps, c.data), verbose=False)
    assert not fit_ref.failed(clean), clean
    wrong = fit_ref.check(c, fit_ref.restated_fit(c.knots, c.basis, c.order, c.stamps, c.data, fault=fault), verbose=False)
    print("%s %-28s %s" % (name, fault, "  ".join("%s %.1e (bound %.1e)" % (k, v, b) for k, (v, b) in wrong.items())))
    for criterion in ("eta", "kept_columns", "fitted_values") if name == "rough-order6-f1" else ("eta",):
        measured, bound = wrong[criterion]
        assert measured > 10.0 * bound, criterion


def test_dropped_column_criterion_rejects_what_reaches_a_dropped_column():
    """A ridge of 1e-9 keeps the control point that the rule drops at order 6, f = 0.1; a sample binned into the gap's
    first empty segment reaches a control point the gap leaves untouched."""
    c = fit_ref.case("order6-f0.1")
    wrong = fit_ref.check(c, fit_ref.restated_fit(c.knots, c.basis, c.order, c.stamps, c.data, fault="ridge_1e-9"), verbose=False)
    assert wrong["dropped_columns"][0] >= 1e3 * wrong["dropped_columns"][1]
    c = fit_ref.case("gap-12-segments")
    j = len(c.stamps) // 2
    assert c.seg[j] == 32 and c.seg[j - 1] == 19           # the first sample after the gap
    wrong = fit_ref.check(c, fit_ref.restated_fit(c.knots, c.basis, c.order, c.stamps, c.data, fault="sample_in_neighbour_segment"),
                          verbose=False)
    assert wrong["dropped_columns"][0] >= 1e3 * wrong["dropped_columns"][1]


def test_smooth_data_alone_would_not_notice_a_lost_sample():
    """Why the sweep carries the two rough-data cases: the smooth channels are fitted so closely that a fit without one of
    its 500 samples still meets every bound."""
    c = fit_ref.case("order6-f1")
    wrong = fit_ref.check(c, fit_ref.restated_fit(c.knots, c.basis, c.order, c.stamps, c.data, fault="sample_left_out"), verbose=False)
    assert not fit_ref.failed(wrong)


@pytest.mark.parametrize("name", fit_ref.ORACLE_CASES)
def test_oracle_agrees_with_the_reference_where_the_fit_is_well_posed(name, oracle):
    """The oracle factors the normal equations (column-pivoted QR of X^T X, as the reference project does), so its own error
    also grows with cond2^2: measured 1.1e-15 cond2^2 max|C| at the most, inside the bound the device is held to against it."""
    c, r = fit_ref.case(name), fit_ref.reference(name)
    diff = np.abs(fit_ref.oracle_fit(oracle, c) - r.C_ref).max()
    print("%s: cond2 %.2e max|C_oracle - C_ref| %.2e" % (name, r.cond, diff))
    assert r.kept.all()
    assert diff <= 0.5 * fit_ref.forward_bound(r.cond, r.C_ref, c.data)
