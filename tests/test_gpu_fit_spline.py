"""Spline initialisation on the device (`-m gpu`): calico_fit_spline against the reference's own known answers
(bspline_test.cpp:19-31, 52-94: fit of (cos t, sin 1.5 t, t cos t) at 10 Hz with 5 Hz knots; derivative tolerances
1e-6 / 1e-5 / 1e-4 / 1e-2), against the oracle's FitToData on the same samples, and, case by case over orders, sampling
patterns and lengths, against exact least squares (tests/fit_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import helpers
from calico_amd import _capi, synthetic as syn

pytestmark = pytest.mark.gpu


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _fit_on_device(hip, t, data, order, knot_frequency):
    knots = syn.knot_vector(t[0], t[-1], order, knot_frequency)
    basis = np.ascontiguousarray(syn.basis_matrices(knots, order))
    ctrl = np.zeros((len(knots) - order, 6))
    rc = hip.fit_spline(0, order, len(knots), dp(knots), dp(basis), len(t), dp(t), dp(np.ascontiguousarray(data)), dp(ctrl))
    return rc, knots, basis, ctrl


def test_fit_reproduces_reference_known_answers(hip):
    t = 0.1 * np.arange(101)
    data = np.zeros((101, 6))
    data[:, 0], data[:, 1], data[:, 2] = np.cos(t), np.sin(1.5 * t), t * np.cos(t)
    rc, knots, basis, ctrl = _fit_on_device(hip, t, data, 6, 5.0)
    assert rc == 0
    ti = (t[-1] - t[0]) / 201 * np.arange(201)
    expect = [
        np.stack([np.cos(ti), np.sin(1.5 * ti), ti * np.cos(ti)], 1),
        np.stack([-np.sin(ti), 1.5 * np.cos(1.5 * ti), np.cos(ti) - ti * np.sin(ti)], 1),
        np.stack([-np.cos(ti), -2.25 * np.sin(1.5 * ti), -2.0 * np.sin(ti) - ti * np.cos(ti)], 1),
        np.stack([np.sin(ti), -3.375 * np.cos(1.5 * ti), ti * np.sin(ti) - 3.0 * np.cos(ti)], 1),
    ]
    for d, tol in enumerate([1e-6, 1e-5, 1e-4, 1e-2]):       # bspline_test.cpp:52-94
        out = syn.spline_eval(knots, basis, ctrl, 6, ti, d)
        assert np.abs(out[:, :3] - expect[d]).max() < tol


@pytest.mark.parametrize("order", [4, 6])
def test_fit_matches_oracle(order, hip, oracle):
    """Well-posed fit (more samples than control points everywhere): same control points as the oracle's FitToData
    (QR of the normal equations) to 1e-8 relative (normal equations square the conditioning of the B-spline basis)."""
    rng = np.random.default_rng(5)
    t = np.sort(rng.uniform(0.0, 12.0, 2000))
    t[0], t[-1] = 0.0, 12.0
    data = np.stack([np.sin(0.7 * t + i) * (1.0 + 0.1 * i) + 0.05 * t for i in range(6)], 1)
    rc, knots, basis, ctrl = _fit_on_device(hip, t, data, order, 10.0)
    assert rc == 0
    lib = oracle.lib
    lib.oracle_spline_create.restype = C.c_void_p
    s = C.c_void_p(lib.oracle_spline_create())
    lib.oracle_spline_fit_vectors.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_int32]
    assert lib.oracle_spline_fit_vectors(s, len(t), dp(t), dp(np.ascontiguousarray(data)), C.c_double(10.0), order) == 0
    ref = np.zeros_like(ctrl)
    lib.oracle_spline_get.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.oracle_spline_get(s, None, None, dp(ref))
    assert np.abs(ctrl - ref).max() <= 1e-8 * np.abs(ref).max()


def test_fit_error_conventions(hip):
    t = 0.1 * np.arange(50)
    data = np.zeros((50, 6))
    knots = syn.knot_vector(t[0], t[-1], 6, 5.0)
    basis = np.ascontiguousarray(syn.basis_matrices(knots, 6))
    ctrl = np.zeros((len(knots) - 6, 6))
    bad = t.copy(); bad[10] = bad[9] - 1.0                      # unsorted
    assert hip.fit_spline(0, 6, len(knots), dp(knots), dp(basis), 50, dp(bad), dp(data), dp(ctrl)) == 3
    far = t.copy(); far[-1] = 100.0                             # outside the valid knots
    assert hip.fit_spline(0, 6, len(knots), dp(knots), dp(basis), 50, dp(far), dp(data), dp(ctrl)) == 3
    assert hip.fit_spline(0, 1, len(knots), dp(knots), dp(basis), 50, dp(t), dp(data), dp(ctrl)) == 3   # order < 2


# ---- the sweep: every case of tests/fit_ref.py against the exact least-squares reference (proved in test_fit_reference.py) ----
import fit_ref  # noqa: E402


def _fit_case(hip, c, fill=np.nan):
    """calico_fit_spline on a case's inputs; ctrl_out starts as `fill`, so a row the device leaves unwritten shows."""
    ctrl = np.full((c.n_ctrl, 6), fill)
    rc = hip.fit_spline(0, c.order, len(c.knots), dp(c.knots), dp(c.basis), len(c.stamps), dp(c.stamps), dp(c.data), dp(ctrl))
    return rc, ctrl


@pytest.mark.parametrize("name", list(fit_ref.CASES))
def test_fit_sweep_against_exact_least_squares(name, hip):
    """Orders 2-8 with covered and ragged ends, gaps, sparse and degenerate sampling, stamps on knots, and the lengths around
    the two LDS limits. Per case (fit_ref.check): backward error of the normal equations <= 1e-11 on every right-hand side;
    where no exact pivot lies within a decade of the rule, the dropped control points <= 1e-12 max|data| and the kept ones and
    the fitted values within 1e-14 cond2(X_kept)^2 max|C_ref| + 1e-13 max|data| of the reference; the rank-deficient cases
    within 1e-9 max|data| of the minimum-norm fit at the samples and no larger than 10 times its control points."""
    c = fit_ref.case(name)
    rc, ctrl = _fit_case(hip, c)
    assert rc == _capi.OK
    result = fit_ref.check(c, ctrl)
    assert not fit_ref.failed(result), result


@pytest.mark.parametrize("name", list(fit_ref.TOO_LONG))
def test_fit_too_long_for_the_on_chip_solve(name, hip):
    """One control point past the 156 KiB ceiling of [band | rhs]: kUnimplemented, ctrl_out left as passed in."""
    c = fit_ref.inputs(fit_ref.TOO_LONG[name])
    rc, ctrl = _fit_case(hip, c, fill=7.5)
    assert rc == _capi.UNIMPLEMENTED
    assert (ctrl == 7.5).all()


def test_fit_sample_count_beyond_int32(hip):
    """The kernels index the samples with int: a count that does not fit is refused before any sample is read."""
    c = fit_ref.case("n3")
    ctrl = np.full((c.n_ctrl, 6), 7.5)
    for n in (2 ** 31, 2 ** 32 + 3):
        assert hip.fit_spline(0, c.order, len(c.knots), dp(c.knots), dp(c.basis), n, dp(c.stamps), dp(c.data), dp(ctrl)) == _capi.UNIMPLEMENTED
    assert (ctrl == 7.5).all()


def test_fit_is_bit_reproducible(hip):
    """Fixed-order sums, no atomics: three fits of one case (above the 64 KiB default of dynamic LDS) give identical bits."""
    c = fit_ref.case(fit_ref.REPEAT_CASE)
    fits = [_fit_case(hip, c) for _ in range(3)]
    assert all(rc == _capi.OK for rc, _ in fits)
    assert np.array_equal(fits[0][1], fits[1][1]) and np.array_equal(fits[0][1], fits[2][1])


@pytest.mark.parametrize("name", fit_ref.ORACLE_CASES)
def test_fit_sweep_matches_oracle(name, hip, oracle):
    """Orders 2-8 with the last segment covered against the oracle's FitToData (column-pivoted QR of the normal equations), held to
    the case's own bound 1e-14 cond2^2 max|C_ref| + 1e-13 max|data| instead of a flat 1e-8."""
    c, r = fit_ref.case(name), fit_ref.reference(name)
    rc, ctrl = _fit_case(hip, c)
    assert rc == _capi.OK
    ref = fit_ref.oracle_fit(oracle, c)
    diff, bound = np.abs(ctrl - ref).max(), fit_ref.forward_bound(r.cond, r.C_ref, c.data)
    print("%s: max|C - C_oracle| %.2e, bound %.2e" % (name, diff, bound))
    assert diff <= bound
