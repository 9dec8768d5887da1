"""tests/fit_smooth_ref.py proved on the CPU: the closed-form penalty against quadrature and against what a roughness penalty
must annihilate, the sweep's inputs against the condition the GPU test's bounds assume, and the criteria against the device's
algorithm restated in float64 -- right, and wrong in five small ways."""
import numpy as np
import pytest

import fit_ref
import fit_smooth_ref as fs
from calico_amd import synthetic as syn

ORDERS_M = [(k, m) for k in range(2, 9) for m in range(1, min(3, k - 1) + 1)]


@pytest.mark.parametrize("order,m", ORDERS_M)
def test_closed_form_penalty_matches_quadrature(order, m):
    """P = sum over the segments of D^(1-2m) M^T H M against 12-point Gauss-Legendre quadrature of spline_weights' m-th
    derivative (exact for its polynomial integrand up to roundoff): <= 1e-13 max|P|, on uniform knots and on stretched ones."""
    for knots in (fit_ref.uniform_knots(20, order), np.cumsum(np.linspace(0.05, 0.3, 20 + order))):
        basis = syn.basis_matrices(knots, order)
        P = np.asarray(fs.band_to_dense(fs.penalty_band(knots, basis, order, m)), float)
        Q = fs.penalty_quadrature(knots, basis, order, m)
        assert np.abs(P - Q).max() <= 1e-13 * np.abs(P).max()
        assert (np.linalg.eigvalsh(P) >= -1e-12 * np.abs(P).max()).all()


@pytest.mark.parametrize("order,m", ORDERS_M)
def test_penalty_annihilates_polynomials_below_its_derivative(order, m):
    """On uniform knots the control points of a polynomial of degree < order are a polynomial of that degree in their index:
    P c = 0 for degree < m (to roundoff of P's entries), and c' P c > 0 for degree m."""
    knots = fit_ref.uniform_knots(20, order)
    P = fs.penalty_band(knots, syn.basis_matrices(knots, order), order, m)
    i = np.arange(20, dtype=fs.LD)[:, None] / 20
    scale = fs.band_inf_norm(P)
    for degree in range(m):
        assert np.abs(fs.band_matvec(P, i ** degree)).max() <= 1e-13 * scale, degree
    # degree m: the spline is (t / (20 D))^m + lower terms, its m-th derivative the constant m! / (20 D)^m over n_seg D seconds
    c, n_seg = i ** m, 20 - (order - 1)
    expect = (np.prod(np.arange(1, m + 1)) / 2.0 ** m) ** 2 * n_seg * 0.1
    assert abs(float((c * fs.band_matvec(P, c)).sum()) - expect) <= 1e-10 * expect


@pytest.mark.parametrize("name,m", list(fs.SWEEP))
def test_sweep_inputs_are_well_posed(name, m):
    """The condition the forward bound assumes, on the inputs: no exact pivot the rule would replace, cond2(A) <= 1e10."""
    p = fs.problem(name, m)
    assert len(p.grid[0]) >= 1
    for (g, l), s in p.sys.items():
        assert s.replaced == 0 and s.pivots.min() > 10 * fit_ref.PIVOT_RULE, (g, l, s.pivots.min())
        assert s.cond <= fs.COND_BOUND, (g, l, s.cond)


def test_sweep_covers_the_cases_and_settings():
    assert {n for n, _ in fs.SWEEP} == set(fs.CASE_NAMES) and len(fs.CASE_NAMES) == 15
    for name in fs.CASE_NAMES:
        order = fit_ref.CASES[name]["order"]
        assert {m for n, m in fs.SWEEP if n == name} >= set(range(1, min(2, order - 1) + 1))
    assert all(set(fs.SWEEP[n, m]) <= set(fs.GRID) for n, m in fs.SWEEP)
    assert sum(len(g) for g in fs.SWEEP.values()) >= 90
    w = fs.sample_weights(500)
    assert w.min() >= 0.25 and w.max() <= 4.0 and not np.array_equal(w[:, 0], w[:, 1])


TEST_OF_TEST = [("gap-12-segments", 2), ("one-per-segment", 2), ("rough-order6-f1", 1), ("order4-f0.1", 2), ("order8-f0.1", 3)]


@pytest.mark.parametrize("name,m", TEST_OF_TEST)
def test_restated_algorithm_passes_and_every_fault_fails(name, m):
    p = fs.problem(name, m)
    good = fs.check(p, fs.restated_smooth_fit(p))
    assert not fs.failed(good), good
    for fault in fs.FAULTS:
        if fault == "neighbour_lambda" and len(p.grid[0]) < 2:
            continue
        bad = fs.failed(fs.check(p, fs.restated_smooth_fit(p, fault), verbose=False))
        print(name, m, fault, "->", bad)
        assert bad, fault


def test_gap_is_filled_and_smooth_data_barely_move():
    """What the penalty is for (defaults: m 2, relative lambda 1e-3, no weights): the control points inside gap-12-segments are
    the data's size instead of ~0, and on order6-f1's smooth channels the fitted values move by ~4e-6 rms."""
    c = fit_ref.case("gap-12-segments")
    p = fs.build(c, np.ones((len(c.stamps), 2)), 2, (1e-3,), (1e-3,))
    dropped = ~fit_ref.reference("gap-12-segments").kept
    assert dropped.sum() >= 5
    C = np.hstack([p.sys[0, 0].C_ref, p.sys[1, 0].C_ref])
    assert np.abs(C[dropped]).max(1).min() > 0.1 * np.abs(c.data).max() and np.abs(C).max() < 2.0 * np.abs(c.data).max()
    c = fit_ref.case("order6-f1")
    p = fs.build(c, np.ones((len(c.stamps), 2)), 2, (1e-3,), (1e-3,))
    C = np.hstack([p.sys[0, 0].C_ref, p.sys[1, 0].C_ref])
    moved = c.X @ C - c.X @ fit_ref.reference("order6-f1").C_ref
    assert 1e-7 < np.sqrt((moved ** 2).mean()) < 1e-4
