"""calico_imu_allan on the device (`-m gpu`) against tests/allan_ref.py (proved on the CPU in test_allan_reference.py).

Lengths around the kernels' seams (the prefix sum's block of B = kAllanScanBlock samples, the variance's chunk of T =
kAllanTermChunk terms) with explicit lists of cluster sizes, and the default grid on the synthetic log of 2^18 samples. The axes
carry different data: white noise, white noise plus a random walk, a ramp.

Bounds. A variance may differ from the long-double reference by 8 times what the float64 restatement of the reference differs
by on the same case and cluster size (the device's tree sums and the restatement's sequential ones differ in order only), with a
floor of 1e-13 (the restatement is exact by accident on some cases). The fit is compared on identical inputs -- the reference
fits the DEVICE's variances --: the same winning mask, and per squared coefficient a_t, |delta a_t| max_i(phi_t(tau_i) / avar_i)
at most 8 times the same quantity between the float64 and the long-double reference fits, floored at 1e-13. Both errors are
printed per case. Everything else is exact: the pooled values follow from the per-axis numbers by the header's expressions in
double, and repeated calls, permuted axes, an explicit list equal to the grid, and axes beside a NaN give the same bits."""
import functools

import numpy as np
import pytest

import allan_ref as ar
from calico_amd import _capi

pytestmark = pytest.mark.gpu

RATE = 200.0
B, T = ar.SCAN_BLOCK, ar.TERM_CHUNK
SEAM_LENGTHS = (3, B - 1, B, B + 1, 2 * B + 37, T + 3, 2 * T + 2 * 5 + 1)
RAMP = 3.7e-4
FACTOR, FLOOR = 8.0, 1e-13


def seam_cluster_sizes(n):
    """m = 1, both parities, a few in between, the m that leaves one term (2m = n - 1) or two (2m = n - 2), and every m that puts
    n - 2m one above or one below a multiple of T."""
    ms = {1, 2, 7, 64, 100, (n - 1) // 2}
    for q in range(1, n // T + 1):
        for terms in (q * T + 1, q * T - 1):
            if (n - terms) % 2 == 0:
                ms.add((n - terms) // 2)
    return sorted(m for m in ms if m >= 1 and 2 * m < n)


@functools.lru_cache(maxsize=None)
def seam_samples(n):
    rng = np.random.default_rng(1000 + n)
    white = 1e-3 * np.sqrt(RATE) * rng.standard_normal((n, 2))
    walk = np.cumsum(2e-4 / np.sqrt(RATE) * rng.standard_normal(n))
    y = np.stack([white[:, 0], white[:, 1] + walk, RAMP * np.arange(n)], axis=1)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def synthetic():
    y = ar.synthetic_log(0)
    y.setflags(write=False)
    return y


@functools.lru_cache(maxsize=None)
def reference(case):
    """(samples, cluster sizes, long-double variances (c, 3), the float64 restatement's relative error (c, 3)) of a case: a seam
    length, or "grid" for the default grid on the synthetic log."""
    y = synthetic() if case == "grid" else seam_samples(case)
    ms = ar.grid(len(y)) if case == "grid" else seam_cluster_sizes(case)
    exact = np.stack([ar.avar(y[:, c], RATE, ms) for c in range(3)], axis=1)
    f64 = np.stack([ar.avar(y[:, c], RATE, ms, dtype=np.float64) for c in range(3)], axis=1)
    return y, ms, exact, ar.relative_error(f64, exact)


def call(hip, y, ms=None, **options):
    o = _capi.default_allan_options(hip, cluster_sizes=ms, **options) if ms is not None or options else None
    return _capi.imu_allan(hip, y, None, RATE, o)


def check_variances(label, out, ms, exact, err64):
    assert list(out["cluster_sizes"]) == list(ms) and out["avar"].shape == (len(ms), 3)
    assert np.array_equal(out["tau"], np.array(ms) * ar.time_step(RATE))
    assert np.array_equal(out["rel_err"], 1.0 / np.sqrt(ar.weights(out["summary"]["n"], ms)))
    err = ar.relative_error(out["avar"], exact)
    bound = np.maximum(FACTOR * err64, FLOOR)
    ratio = err / bound
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("%s: device error max %.2e, float64 restatement max %.2e, worst error / bound %.3f (m = %d, axis %d: %.2e against %.2e)"
          % (label, err.max(), err64.max(), ratio[at], ms[at[0]], at[1], err[at], err64[at]))
    assert np.all(err <= bound), (label, [(ms[j], c, err[j, c], err64[j, c]) for j, c in zip(*np.nonzero(err > bound))])


def check_fit(label, out, n, terms=ar.DEFAULT_TERMS):
    """The reference fit on the device's own variances against the device's coefficients."""
    ms, tau = list(out["cluster_sizes"]), out["tau"]
    w = ar.weights(n, ms)
    for c in range(3):
        got = out["noise"][c]
        exact = ar.fit(tau, w, out["avar"][:, c], terms)
        f64 = ar.fit(tau, w, out["avar"][:, c], terms, dtype=np.float64)
        assert got["status"] == exact["status"] and got["n_points"] == exact["n_points"], (label, c, got, exact["status"])
        assert got["terms_used"] == exact["mask"], (label, c, got["terms_used"], exact["mask"])
        a = np.array([got[name] for name in ar.NAMES], dtype=ar.LD) ** 2
        scale = exact["shapes_over_avar"]
        err = np.asarray(np.abs(a - exact["a"]) * scale, dtype=np.float64)
        err64 = np.asarray(np.abs(f64["a"].astype(ar.LD) - exact["a"]) * scale, dtype=np.float64) if f64["mask"] == exact["mask"] else np.zeros(5)
        print("%s axis %d: mask %d, coefficient error max %.2e, float64 reference fit max %.2e" % (label, c, exact["mask"], err.max(), err64.max()))
        assert np.all(err <= np.maximum(FACTOR * err64, FLOOR)), (label, c, err, err64)
        if exact["status"] != ar.TOO_FEW_POINTS:
            assert abs(got["objective"] - float(exact["objective"])) <= 1e-9 * max(float(exact["objective"]), 1e-20) + exact["n_points"] * 1e-20


def check_pooled(out):
    """The summary from the per-axis numbers, by the header's expressions in double: exactly."""
    sm, noise = out["summary"], out["noise"]
    assert sm["sample_rate_hz"] == RATE and sm["duration"] == sm["n"] / RATE
    n2 = 0.0
    for a in noise:
        n2 += a["N"] * a["N"]
    assert sm["N_pooled"] == np.sqrt(n2 / 3.0) and sm["sigma_at_rate"] == sm["N_pooled"] * np.sqrt(RATE)
    assert sm["bias_drift_over_recording"] == max(a["K"] * np.sqrt(sm["duration"]) for a in noise)


def same_bits(a, b):
    assert np.array_equal(a["avar"], b["avar"], equal_nan=True) and np.array_equal(a["tau"], b["tau"]) and np.array_equal(a["rel_err"], b["rel_err"])
    assert np.array_equal(a["cluster_sizes"], b["cluster_sizes"]) and a["noise"] == b["noise"] and a["summary"] == b["summary"]


@pytest.mark.parametrize("n", SEAM_LENGTHS)
def test_lengths_around_the_seams(hip, n):
    y, ms, exact, err64 = reference(n)
    assert 1 in ms and (n - 1) // 2 in ms and (n < T + 3 or {(n - T - 1) // 2, (n - T + 1) // 2} <= set(ms))
    out = call(hip, y, ms)
    assert out["summary"]["n"] == n
    check_variances("n = %d" % n, out, ms, exact, err64)
    check_fit("n = %d" % n, out, n)
    check_pooled(out)
    # the known answer: the ramp's variance is (a m)^2 / 2, within the same bound
    ramp = np.array([(ar.LD(RAMP) * m) ** 2 / 2 for m in ms])
    err = ar.relative_error(out["avar"][:, 2], ramp)
    print("n = %d: the ramp against (a m)^2 / 2: %.2e" % (n, err.max()))
    assert np.all(err <= np.maximum(FACTOR * err64[:, 2], FLOOR))
    same_bits(out, call(hip, y, ms))


def test_the_default_grid(hip):
    y, ms, exact, err64 = reference("grid")
    out = call(hip, y)
    assert len(ms) == 42
    check_variances("default grid, n = 2^18", out, ms, exact, err64)
    check_fit("default grid", out, len(y))
    check_pooled(out)
    for a in out["noise"]:      # the log's own truth, loosely: the reference's caps (test_allan_reference.py)
        assert a["status"] == ar.OK and abs(a["N"] / 1e-3 - 1) <= 0.02 and abs(a["K"] / 2e-4 - 1) <= 0.30, a
    # every term enabled: the same variances, a fit over five terms
    full = call(hip, y, terms=31)
    assert np.array_equal(full["avar"], out["avar"])
    check_fit("default grid, five terms", full, len(y), terms=31)


def test_determinism(hip):
    y, ms, _, _ = reference("grid")
    out = call(hip, y)
    same_bits(out, call(hip, y))
    # an explicit list equal to the grid: the grid call's bits
    same_bits(out, call(hip, y, ms))
    # the axes do not see each other: a permutation of the input's columns permutes the outputs
    perm = [2, 0, 1]
    moved = call(hip, np.ascontiguousarray(y[:, perm]))
    assert np.array_equal(moved["avar"], out["avar"][:, perm]) and moved["noise"] == [out["noise"][c] for c in perm]
    assert moved["summary"]["bias_drift_over_recording"] == out["summary"]["bias_drift_over_recording"]
    # a cluster size's variance does not depend on its neighbours in the list
    few = call(hip, y, ms[5:30:3])
    assert np.array_equal(few["avar"], out["avar"][5:30:3])
    # stamps at the same rate: the rate comes from them
    stamped = _capi.imu_allan(hip, y[:5000], 17.0 + np.arange(5000) / 256.0, 0.0, None)
    assert stamped["summary"]["sample_rate_hz"] == 256.0
    same_bits(stamped, _capi.imu_allan(hip, y[:5000], None, 256.0, None))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_an_axis_that_is_not_finite(hip, bad):
    y = seam_samples(2 * B + 37)
    ms = seam_cluster_sizes(len(y))
    clean = call(hip, y, ms)
    dirty = y.copy()
    dirty[B + 5, 1] = bad
    out = call(hip, dirty, ms)
    assert out["noise"][1]["status"] == ar.NONFINITE and np.all(np.isnan(out["avar"][:, 1]))
    assert all(out["noise"][1][k] == 0 for k in ("Q", "N", "B", "K", "R", "objective", "terms_used", "n_points"))
    for c in (0, 2):
        assert np.array_equal(out["avar"][:, c], clean["avar"][:, c]) and out["noise"][c] == clean["noise"][c]
    check_pooled(out)
    # the last sample, in the prefix sum's last and partly filled block
    dirty = y.copy()
    dirty[-1, 2] = bad
    out = call(hip, dirty, ms)
    assert [a["status"] for a in out["noise"]] == [clean["noise"][0]["status"], clean["noise"][1]["status"], ar.NONFINITE]
    assert np.array_equal(out["avar"][:, :2], clean["avar"][:, :2]) and np.all(np.isnan(out["avar"][:, 2]))


def test_statuses_of_short_and_flat_logs(hip):
    # one cluster size, three enabled terms: too few points, coefficients 0, the variance still reported
    y = seam_samples(3)
    out = call(hip, y, [1])
    assert [a["status"] for a in out["noise"]] == [ar.TOO_FEW_POINTS] * 3 and out["summary"]["N_pooled"] == 0.0
    assert out["noise"][0]["n_points"] == 1 and np.all(out["avar"] > 0)
    # a constant axis has no variance: the reference's own cap (test_allan_reference.py); the axes beside it are not touched
    y = seam_samples(B + 1)
    flat = np.array(y)
    flat[:, 0] = 9.80665
    ms = seam_cluster_sizes(B + 1)
    out = call(hip, flat, ms)
    assert np.all(out["avar"][:, 0] <= 1e-25 * 9.80665 ** 2)
    assert np.array_equal(out["avar"][:, 1:], call(hip, y, ms)["avar"][:, 1:])
    check_pooled(out)
