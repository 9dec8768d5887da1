"""The robust spline fit restated in numpy: what calico_fit_spline_robust must produce, its scenario, and the criteria of its tests.

A plain module (numpy only) on tests/fit_smooth_ref.py (build, normal_band, band_cholesky_solve, penalty_band), shared by
tests/test_fit_robust_reference.py, which proves on the CPU that the criteria pass the algorithm and fail each of seven ways to get
it wrong, and tests/test_gpu_fit_robust.py.

The algorithm (include/calico_hip.h), per channel group g with prior weights w = weights[:, g]:
  iteration 0     the smoothing fit with one lambda; its absolute lambda is frozen
  iteration t     e_j = |X_j C - d_j|_2 over the m samples with w_j > 0;  med = sorted(e)[(m - 1) // 2];
                  sigma = max(med / CHI3_MEDIAN_ROOT, min_scale), or the caller's scale;  sigma == 0: stop, SCALE_ZERO, u = 1;
                  z = e / sigma;  Huber u = min(1, c / z);  Tukey u = (1 - (z / c)^2)^2 for z < c, else 0;
                  (X^T diag(w u) X + lambda P) C = X^T diag(w u) d;  step = max|C - C_prev| / max|C| (0 where nothing moved);
                  0 < tolerance and step <= tolerance: OK;  after T iterations without that: MAX_ITERATIONS
  afterwards      e at the final control points.
- irls(p, loss, T, ...): the algorithm in long double (reference_irls) or float64 (restated_robust_fit, with one fault switched on).
- scenario(): rough-order6-f1 with seeded prior weights, a tenth of each group displaced by U[1, 3] in a random direction, and a
  twentieth at prior weight 0 with data 10 units off.
- check_step / check_scenario: the criteria, the same functions for the CPU test of the test and the GPU tests.
"""
import functools
from types import SimpleNamespace

import numpy as np

import fit_ref
import fit_smooth_ref as fs

LD = np.longdouble
CHI3_MEDIAN_ROOT = 1.5381722544550522       # sqrt(median of chi2 with 3 degrees of freedom) = sqrt(2.3659738843753377)
HUBER, TUKEY = 1, 2
DEFAULT_TUNING = {HUBER: 2.7955, TUKEY: 2.0 * 2.7955}      # sqrt(7.8147), the 95 % point of chi_3; twice that
OK, NOT_POSITIVE_DEFINITE, MAX_ITERATIONS, SCALE_ZERO = 0, 1, 3, 4
FAULTS = ("upper_median", "median_over_weight_zero", "mad_constant", "lambda_rederived", "prior_weight_dropped", "tukey_no_cutoff",
          "huber_squared")
SEED = 41                                   # the scenario's displaced samples
LAMBDA, DERIVATIVE = 1e-3, 2                # the smoothing fit's defaults
# The scenario's tuning constants. Tukey: the default. Huber: 2.0 -- at the default 2.7955 the long-double reference leaves the
# displaced sample nearest its 1-unit minimum at u = 0.35 and is 0.23 as far from the clean fit as the smoothing fit, which meets
# the scenario's conditions (0.5, 1/3) but not with the factor 1.5 to spare that is asked of the inputs; at 2.0 it has 0.24 and 0.18.
SCENARIO_TUNING = {HUBER: (2.0, 2.0), TUKEY: (0.0, 0.0)}


def psi(loss, e, sigma, c, fault=None):
    """The robust weight of residual norms e, operation by operation in e's dtype: what the device evaluates without contraction."""
    e = np.asarray(e)
    one = e.dtype.type(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        z = e / e.dtype.type(sigma)
        if loss == HUBER:
            q = e.dtype.type(c) / z
            u = np.where(q < one, q, one)
            return u * u if fault == "huber_squared" else u
        s = z / e.dtype.type(c)
        a = one - s * s
        return a * a if fault == "tukey_no_cutoff" else np.where(z < e.dtype.type(c), a * a, 0 * one)


def lower_median(e):
    return np.sort(e)[(len(e) - 1) // 2]


def fitted_values(p, C, dtype=np.float64):
    idx = p.seg[:, None] + np.arange(p.c.order)[None, :]
    return np.einsum("nj,njc->nc", np.asarray(p.W, dtype), np.asarray(C, dtype)[idx])


def residual_norms(p, g, C, dtype=np.float64):
    """|X_j C - d_j|_2 of group g at control points C (n_ctrl, 3), NaN where the prior weight is 0."""
    r = fitted_values(p, C, dtype) - np.asarray(p.c.data[:, 3 * g:3 * g + 3], dtype)
    e = np.sqrt((r * r).sum(1))
    e[p.weights[:, g] == 0] = np.nan
    return e


def _solve(p, g, wu, lam, dtype):
    """(C, replaced pivots) of (X^T diag(wu) X + lam P) C = X^T diag(wu) d: float64 as the device does it (ridge, one Cholesky);
    long double without ridge, refined twice."""
    N, b = fs.normal_band(p.W, p.seg, wu, p.c.data[:, 3 * g:3 * g + 3], p.c.n_ctrl, dtype=dtype)
    if dtype is LD:
        A = N + lam * p.P
        C, _, replaced = fs.band_cholesky_solve(A, b)
        for _ in range(2):
            C = C + fs.band_cholesky_solve(A, b - fs.band_matvec(A, C))[0]
        return C, replaced
    if not hasattr(p, "P64"):
        p.P64 = fs.penalty_band(p.c.knots, p.c.basis, p.c.order, p.m, dtype=np.float64)      # (restated_smooth_fit's)
    P = p.P64
    C, _, replaced = fs.band_cholesky_solve(N + lam * P if lam != 0 else N, b, ridge=fit_ref.RIDGE)
    return C, replaced


def irls(p, loss, T, dtype=np.float64, tuning=(0.0, 0.0), scale=(0.0, 0.0), min_scale=(0.0, 0.0), tolerance=0.0, fault=None):
    """The robust fit on problem p (fit_smooth_ref.build with one lambda per group) with at most T (an int or one per group)
    reweighted iterations. Returns what the call returns: ctrl, robust_weights, residuals, summary (a dict of two-entry lists);
    with dtype long double, ctrl_ld as well."""
    assert fault is None or fault in FAULTS
    c, n = p.c, len(p.c.stamps)
    T = (T, T) if np.isscalar(T) else T
    ctrl = np.zeros((c.n_ctrl, 6), dtype)
    u_out, e_out = np.zeros((n, 2)), np.zeros((n, 2))
    names = ("status", "iterations", "replaced_pivots", "n_used", "n_downweighted", "n_rejected", "lambda", "scale", "median_residual",
             "last_step", "rss")
    summary = {k: [None, None] for k in names}
    start = fs.restated_smooth_fit(p) if dtype is not LD else None
    for g in range(2):
        w = p.weights[:, g]
        use = w > 0
        tune = tuning[g] if tuning[g] > 0 else DEFAULT_TUNING[loss]
        if dtype is LD:
            lam = p.sys[g, 0].lam
            C, replaced = _solve(p, g, w, lam, LD)
        else:
            lam, replaced = start["rows"][g][0]["lambda"], start["rows"][g][0]["replaced_pivots"]
            C = start["ctrl_all"][0][:, 3 * g:3 * g + 3].copy()
        lam0 = lam
        u = np.where(use, 1.0, 0.0).astype(dtype)
        status, iterations, step, sigma, med = OK, 0, np.nan, np.nan, np.nan
        for t in range(1, T[g] + 1):
            e = residual_norms(p, g, C, dtype)
            if scale[g] > 0:
                sigma, med = dtype(scale[g]), np.nan
            else:
                pool = (fitted_values(p, C, dtype) - np.asarray(c.data[:, 3 * g:3 * g + 3], dtype)) if fault == "median_over_weight_zero" else None
                ranked = np.sqrt((pool * pool).sum(1)) if pool is not None else e[use]
                med = np.sort(ranked)[len(ranked) // 2] if fault == "upper_median" else lower_median(ranked)
                sigma = med * dtype(1.4826) if fault == "mad_constant" else med / dtype(CHI3_MEDIAN_ROOT)
                sigma = max(sigma, dtype(min_scale[g]))
            if sigma == 0:
                status, u = SCALE_ZERO, np.where(use, 1.0, 0.0).astype(dtype)
                break
            u = np.where(use, psi(loss, np.where(use, e, 0), sigma, tune, fault), 0).astype(dtype)
            wu = u if fault == "prior_weight_dropped" else np.asarray(w, dtype) * u
            if fault == "lambda_rederived":
                N, _ = fs.normal_band(p.W, p.seg, wu, c.data[:, 3 * g:3 * g + 3], c.n_ctrl, dtype=dtype)
                lam = dtype(p.grid[g][0]) * (N[:, 0].sum() / np.asarray(p.P, dtype)[:, 0].sum())
            C_new, replaced = _solve(p, g, wu, lam, dtype)
            if not np.isfinite(C_new).all():
                status = NOT_POSITIVE_DEFINITE
                break
            moved = np.abs(C_new - C).max()
            step = 0.0 if moved == 0 else float(moved / np.abs(C_new).max())
            C, iterations = C_new, t
            if tolerance > 0 and step <= tolerance:
                status = OK
                break
            if t == T[g]:
                status = MAX_ITERATIONS
        e = residual_norms(p, g, C, dtype)
        ctrl[:, 3 * g:3 * g + 3] = C
        u_out[:, g], e_out[:, g] = np.asarray(u, float), np.asarray(e, float)
        wl, ul = np.asarray(w, LD), np.asarray(u, LD)
        values = dict(status=status, iterations=iterations, replaced_pivots=replaced, n_used=int(use.sum()),
                      n_downweighted=int(((u > 0) & (u < 1) & use).sum()), n_rejected=int(((u == 0) & use).sum()), scale=float(sigma),
                      median_residual=float(med), last_step=float(step), rss=float((wl * ul * np.asarray(e, LD) ** 2)[use].sum()))
        values["lambda"] = float(lam if fault == "lambda_rederived" else lam0)
        for k in names:
            summary[k][g] = values[k]
    out = dict(ctrl=np.asarray(ctrl, float), robust_weights=u_out, residuals=e_out, summary=summary)
    if dtype is LD:
        out["ctrl_ld"] = ctrl
    return out


def reference_irls(p, loss, T, **kw):
    return irls(p, loss, T, dtype=LD, **kw)


def restated_robust_fit(p, loss, T, fault=None, **kw):
    return irls(p, loss, T, dtype=np.float64, fault=fault, **kw)


# ---- the scenario ----
def with_data(c, data=None, stamps=None, name=None):
    return SimpleNamespace(name=name or getattr(c, "name", "case"), order=c.order, n_ctrl=c.n_ctrl, knots=c.knots, basis=c.basis,
                           stamps=c.stamps if stamps is None else stamps, data=c.data if data is None else data)


def problem(c, weights, lam=LAMBDA, m=DERIVATIVE):
    return fs.build(c, weights, m, (lam,), (lam,), reference=False)


@functools.lru_cache(maxsize=None)
def scenario():
    """rough-order6-f1 (521 samples, 57 control points, noise sigma 0.1) with seeded prior weights in [0.25, 4]. Per group, drawn
    separately: a tenth of the samples displaced by U[1, 3] in a uniformly random direction; of the rest, a twentieth at prior
    weight 0 with data 10 units off (finite, so that a median taken over them too can be computed and is wrong). s.clean /
    s.dirty: the problems on the clean and on the displaced data with the same weights; s.displaced[g]: the displaced samples."""
    c = fit_ref.case("rough-order6-f1")
    n = len(c.stamps)
    rng = np.random.default_rng(SEED)
    weights = fs.sample_weights(n)
    data, displaced, off = c.data.copy(), [], []
    for g in range(2):
        order = rng.permutation(n)
        d, z = order[:n // 10], order[n // 10:n // 10 + n // 20 + 1]      # (27 of 521: m = 494 is even, the two medians differ)
        direction = rng.standard_normal((len(d), 3))
        direction /= np.linalg.norm(direction, axis=1)[:, None]
        data[d, 3 * g:3 * g + 3] += rng.uniform(1.0, 3.0, len(d))[:, None] * direction
        data[z, 3 * g:3 * g + 3] += 10.0
        weights[z, g] = 0.0
        displaced.append(np.sort(d))
        off.append(np.sort(z))
    s = SimpleNamespace(c=c, weights=weights, data=data, displaced=displaced, off=off)
    s.clean = problem(with_data(c, name="scenario-clean"), weights)
    s.dirty = problem(with_data(c, data, name="scenario"), weights)
    for a in (weights, data):
        a.setflags(write=False)
    return s


# ---- the criteria ----
def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, float)))


def check_step(p, prev, cur, loss, tuning=(0.0, 0.0), groups=(0, 1), fixed_scale=False, iterations=None):
    """One reweighted iteration checked from the previous iterate: `prev` is the result after T iterations, `cur` after T + 1 (both
    run without early-out; results as calico_fit_spline_robust returns them). Returns {criterion: (measured, bound)}, the worst
    over the groups; a criterion holds when measured <= bound.
      median   cur's median_residual is the lower median of prev's residuals over the samples of weight > 0, bit for bit
      scale    within 1 ulp of median / CHI3_MEDIAN_ROOT
      psi      cur's robust weights within 4 ulp of psi in float64 on prev's residuals and cur's scale; exactly 1 and 0 where psi
               is; 0 where the prior weight is 0
      lambda   the lambda has iteration 0's bits
      eta      backward error of cur's control points against (X^T diag(w u) X + lambda P, X^T diag(w u) d) in long double, built
               from cur's own u and lambda, <= fit_ref.ETA_BOUND; no replaced pivot
      rss, counts, n_used   the summary agrees with the outputs (rss within SUM_BOUND of the sum of its terms)"""
    res = {}

    def worst(key, value, bound):
        ratio = value / bound if bound > 0 else (0.0 if value == 0 else np.inf)
        if key not in res or ratio > res[key][2]:
            res[key] = (value, bound, ratio)
    for g in groups:
        w = p.weights[:, g]
        use = w > 0
        S, e_prev, u = cur["summary"], prev["residuals"][:, g], cur["robust_weights"][:, g]
        sigma = S["scale"][g]
        if not fixed_scale:
            med = lower_median(e_prev[use])
            worst("median", 0.0 if S["median_residual"][g] == med else 1.0, 0.0)
            worst("scale", abs(sigma - med / CHI3_MEDIAN_ROOT), float(_ulp(med / CHI3_MEDIAN_ROOT)))
        tune = tuning[g] if tuning[g] > 0 else DEFAULT_TUNING[loss]
        want = psi(loss, e_prev[use], sigma, tune)
        with np.errstate(over="ignore"):
            worst("psi", float((np.abs(u[use] - want) / _ulp(want)).max()), 4.0)
        worst("psi_exact", float(((u[use] != want) & ((want == 0) | (want == 1))).sum() + (u[~use] != 0).sum()), 0.0)
        worst("lambda", 0.0 if S["lambda"][g] == prev["summary"]["lambda"][g] else 1.0, 0.0)
        N, b = fs.normal_band(p.W, p.seg, np.asarray(w, LD) * np.asarray(u, LD), p.c.data[:, 3 * g:3 * g + 3], p.c.n_ctrl)
        A = N + LD(S["lambda"][g]) * p.P
        worst("eta", float(fs.backward_error(A, b, cur["ctrl"][:, 3 * g:3 * g + 3]).max()), fit_ref.ETA_BOUND)
        worst("replaced_pivots", float(S["replaced_pivots"][g]), 0.0)
        e = np.asarray(cur["residuals"][:, g], LD)
        rss = float((np.asarray(w, LD) * np.asarray(u, LD) * e * e)[use].sum())
        worst("rss", abs(S["rss"][g] - rss), fs.SUM_BOUND * rss)
        counts = (int(((u > 0) & (u < 1) & use).sum()), int(((u == 0) & use).sum()), int(use.sum()))
        worst("counts", 0.0 if (S["n_downweighted"][g], S["n_rejected"][g], S["n_used"][g]) == counts else 1.0, 0.0)
        worst("nan_where_unused", 0.0 if np.isnan(cur["residuals"][~use, g]).all() and np.isfinite(cur["residuals"][use, g]).all() else 1.0, 0.0)
        if iterations is not None:
            worst("iterations", 0.0 if (S["iterations"][g], S["status"][g]) == (iterations, MAX_ITERATIONS) else 1.0, 0.0)
    return {k: v[:2] for k, v in res.items()}


def rms_distance(p, g, C_a, C_b):
    """RMS over the samples and the group's channels of the distance between the fitted values of two sets of control points."""
    d = fitted_values(p, np.asarray(C_a, LD)[:, 3 * g:3 * g + 3] - np.asarray(C_b, LD)[:, 3 * g:3 * g + 3], LD)
    return float(np.sqrt((d * d).mean()))


@functools.lru_cache(maxsize=None)
def scenario_baselines():
    """(the clean-data smoothing fit's control points, the displaced-data smoothing fit's), both in long double: T = 0."""
    s = scenario()
    return reference_irls(s.clean, HUBER, 0)["ctrl_ld"], reference_irls(s.dirty, HUBER, 0)["ctrl_ld"]


def check_scenario(out, loss, spare=1.0, verbose=True):
    """What the robust fit is for, on a result on scenario().dirty: every displaced sample has u <= 0.5 (Huber) or u == 0 (Tukey),
    and the fitted values are at most 1/3 as far (RMS) from the clean-data smoothing fit as the smoothing fit of the displaced data
    is. spare: the factor to spare that is asked (the reference must meet the conditions with 1.5)."""
    s = scenario()
    clean, smooth = scenario_baselines()
    res = {}
    for g in range(2):
        u = out["robust_weights"][s.displaced[g], g]
        res["displaced_weight_%d" % g] = (float(u.max()), 0.0 if loss == TUKEY else 0.5 / spare)
        own, base = rms_distance(s.dirty, g, out["ctrl"], clean), rms_distance(s.dirty, g, smooth, clean)
        res["distance_%d" % g] = (own, base / 3.0 / spare)
        if verbose:
            print("scenario loss %d group %d: max u of the displaced %.3f, rms distance from the clean fit %.4f (smoothing fit %.4f), "
                  "scale %.4f, iterations %d, status %d" % (loss, g, u.max(), own, base, out["summary"]["scale"][g],
                                                            out["summary"]["iterations"][g], out["summary"]["status"][g]))
    return res


def failed(result):
    return sorted(k for k, (v, bound) in result.items() if not v <= bound)
