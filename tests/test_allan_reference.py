"""tests/allan_ref.py proved on the CPU (no library of the project is loaded): the long-double Allan variance against the closed
forms of a ramp and a constant, the grid, and variance plus fit on synthetic logs of known white noise and rate random walk.

The caps on the synthetic logs are conditions on the reference, not tolerances of the device: the white noise is read off the
grid's short end (rel_err 1e-3: 2 % is twenty of them), the random walk off its long end, where rel_err = 1 / sqrt(2 (n / m - 1))
is 0.23 at m = 25119 of n = 2^18 and the neighbouring points are strongly correlated (30 % is 1.3 of them)."""
import numpy as np
import pytest

import allan_ref as ar

N0, K0, RATE = 1e-3, 2e-4, 200.0


def test_a_ramp_has_its_closed_form():
    """y_k = a k: theta's second difference is a m^2 dt for every k, so avar(m) = (a m)^2 / 2 exactly."""
    n, a = 20001, 0.37
    ms = [1, 7, 100, 10000]
    v = ar.avar(a * np.arange(n, dtype=ar.LD), RATE, ms)
    exact = np.array([(ar.LD(a) * m) ** 2 / 2 for m in ms])
    err = ar.relative_error(v, exact)
    print("ramp, long double:", err)
    assert err.max() <= 1e-15
    err64 = ar.relative_error(ar.avar(a * np.arange(n), RATE, ms, dtype=np.float64), exact)
    print("ramp, float64:", err64)
    assert err64.max() <= 1e-9      # (the restatement is a sane one; the device tests measure it case by case)


def test_a_constant_has_no_variance():
    c = 9.81
    v = ar.avar(np.full(5000, c, dtype=ar.LD), RATE, ar.grid(5000, max_tau_fraction=0.4))
    assert np.all(v <= 1e-25 * c * c)


def test_the_default_grid():
    ms = ar.grid(2 ** 18)
    assert len(ms) == 42 and ms[:8] == [1, 2, 3, 4, 5, 6, 8, 10] and ms[-1] == 25119
    assert all(b > a for a, b in zip(ms, ms[1:]))
    assert ar.grid(100, points_per_decade=1, max_tau_fraction=0.5) == [1, 10] and ar.grid(3) == [] and ar.grid(3, max_tau_fraction=0.5) == [1]
    w = ar.weights(2 ** 18, ms)
    assert abs(1 / np.sqrt(w[-1]) - 0.2302) < 1e-4


@pytest.mark.parametrize("seed", range(5))
def test_white_noise_and_random_walk_are_recovered(seed):
    y = ar.synthetic_log(seed, N0=N0, K0=K0, rate=RATE)[:, 0]
    ms = ar.grid(len(y))
    tau = np.array(ms) * ar.time_step(RATE)
    v = ar.avar(y, RATE, ms)
    f = ar.fit(tau, ar.weights(len(y), ms), v)
    N, K = f["coefficients"]["N"], f["coefficients"]["K"]
    print("seed %d: N / N0 - 1 = %+.4f, K / K0 - 1 = %+.4f, B = %.3e, mask %d, objective %.3f" % (seed, N / N0 - 1, K / K0 - 1, f["coefficients"]["B"],
                                                                                                f["mask"], float(f["objective"])))
    assert f["status"] == ar.OK and f["n_points"] == 42 and f["mask"] & ar.TERM_N and f["mask"] & ar.TERM_K
    assert abs(N / N0 - 1) <= 0.02 and abs(K / K0 - 1) <= 0.30
    # the float64 restatement of the fit on the same variances chooses the same subset
    f64 = ar.fit(tau, ar.weights(len(y), ms), v.astype(np.float64), dtype=np.float64)
    assert f64["mask"] == f["mask"]


def test_the_fit_on_exact_curves():
    tau = np.array(ar.grid(2 ** 16)) * ar.time_step(RATE)
    w = ar.weights(2 ** 16, ar.grid(2 ** 16))
    shapes = ar.term_shapes(tau)
    for t in range(5):
        f = ar.fit(tau, w, 4e-6 * shapes[t], terms=31)
        assert f["mask"] == 1 << t and abs(f["a"][t] / ar.LD(4e-6) - 1) <= 1e-17 and f["objective"] <= 1e-30, (t, f)
    f = ar.fit(tau, w, 1e-6 * shapes[1] + 4e-8 * shapes[3])
    assert f["mask"] == ar.TERM_N | ar.TERM_K and abs(f["a"][1] / ar.LD(1e-6) - 1) <= 1e-15 and abs(f["a"][3] / ar.LD(4e-8) - 1) <= 1e-15
    # white noise minus a little random walk: the unconstrained fit of N and K has K^2 < 0; the feasible subset is N alone
    f = ar.fit(tau, w, 1e-6 * shapes[1] - 1e-9 * shapes[3], terms=ar.TERM_N | ar.TERM_K)
    assert f["mask"] == ar.TERM_N and f["a"][3] == 0 and f["status"] == ar.OK
    for bad in (np.zeros(len(tau)), np.full(len(tau), np.nan)):
        f = ar.fit(tau, w, bad)
        assert f["status"] == ar.TOO_FEW_POINTS and f["n_points"] == 0 and not f["a"].any()
    f = ar.fit(tau, w, 1e-6 * shapes[3], terms=ar.TERM_K | ar.TERM_B)
    assert f["status"] == ar.NO_WHITE_NOISE and f["mask"] == ar.TERM_K
