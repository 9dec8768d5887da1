"""The cross-validated spline fit restated in numpy: what calico_fit_spline_cv must produce beyond the smoothing fit, and the cases
its GPU test runs.

A plain module (numpy only) on tests/fit_smooth_ref.py's problems and band algebra (row a, entry e = (a, a - e)), shared by
tests/test_fit_cv_reference.py, which proves on the CPU that the criteria tell a right result from one that is wrong by a little,
and tests/test_gpu_fit_cv.py.

Per (group g, grid entry l) of a problem p (fit_smooth_ref.build): A = N + lambda P, Z = A^-1 on A's band,
    h_j = w_j X_j Z X_j^T,   edf = sum over the band of Z o N = sum_j h_j,
    gcv = (rss / (3 n_used)) / (1 - edf / n_used)^2,   press = sum_j w_j e_j^2 / (1 - h_j)^2 / (3 n_used),
and per group the smallest score, a tie going to the larger lambda.
- band_cholesky, band_selected_inverse: the factor of a band and Takahashi's recursion over it, in the band's own dtype.
- reference(p, g, l): Z, h and edf in long double from A without the ridge (the exact fit, as fit_smooth_ref.reference_solve).
- scores_at: gcv and press in long double at given control points, with the bounds propagated from the bounds on their inputs.
- restated_cv_fit: the device's steps in float64 after fit_smooth_ref.restated_smooth_fit, one fault switched on at a time.
- check: the criteria, one function for the CPU test of the test and the GPU sweep.
- choice_problem: the fixtures on which the choice itself is held to the reference's.
"""
import functools
from types import SimpleNamespace

import numpy as np

import fit_ref
import fit_smooth_ref as fs

LD = np.longdouble
CRITERIA = ("gcv", "press")
CHOICE_GRID = tuple(float(10.0 ** e) for e in np.arange(-8.0, 4.25, 0.5))      # 25 relative lambdas, 1e-8 .. 1e4
CHOICE_GAP = 1e-4                           # the reference's best and second-best score differ by at least this, relatively
CHOICE_RMS = 0.05                           # the reference's RMS at the minimum is within this of the noise's sigma


# ---- band algebra ----
def band_cholesky(band, ridge=0.0, rule=True):
    """The factor of fit_smooth_ref.band_cholesky_solve (right-looking, ridge in units of mean_diag, the pivot rule) without the
    substitutions: (L's band, replaced)."""
    n, k = band.shape
    B = band.copy()
    mean_diag = B[:, 0].sum() / n
    B[:, 0] += B.dtype.type(ridge) * mean_diag
    replaced = 0
    for j in range(n):
        d = B[j, 0]
        if not d > B.dtype.type(fit_ref.PIVOT_RULE) * mean_diag:
            replaced += 1
            if rule:
                d = mean_diag
        inv = 1 / np.sqrt(d)
        B[j, 0] = d * inv
        h = min(k, n - j)
        col = np.array([B[j + i, i] for i in range(1, h)], B.dtype) * inv
        for i in range(1, h):
            B[j + i, i] = col[i - 1]
            B[j + i, i - 1::-1][:i] -= col[i - 1] * col[:i]
    return B, replaced


def band_selected_inverse(L, short=False):
    """The band of Z = (L L^T)^-1 from the band of L, last column first, in L's dtype and in the device's order of operations:
    Z(j+i, j) = -sum_c l_c Z(j+i, j+c) summed in the order of c, Z(j, j) = 1 / L(j, j)^2 - sum_i l_i Z(j+i, j) in the order of i,
    l_c = L(j+c, j) (1 / L(j, j)), one reciprocal a column. `short` (a fault): the recursion stops one column early."""
    n, k = L.shape
    Z = L.copy()
    for j in range(n - 1, 0 if short else -1, -1):
        inv, h = 1 / Z[j, 0], min(k, n - j)
        ell = [Z[j + c, c] * inv for c in range(1, h)]
        new = []
        for i in range(1, h):
            s = None
            for c in range(1, h):
                prod = ell[c - 1] * (Z[j + i, i - c] if i >= c else Z[j + c, c - i])
                s = prod if s is None else s + prod
            new.append(-s)
        acc = Z.dtype.type(0)
        for i in range(1, h):
            acc = acc + ell[i - 1] * new[i - 1]
        for i in range(1, h):
            Z[j + i, i] = new[i - 1]
        Z[j, 0] = inv * inv - acc
    return Z


def dense_inverse(A_band, steps=3):
    """A^-1 dense in long double: numpy's float64 inverse refined by Newton's iteration X <- X (2 I - A X)."""
    A = fs.band_to_dense(np.asarray(A_band, LD))
    X = np.asarray(np.linalg.inv(np.asarray(A, float)), LD)
    eye2 = 2 * np.eye(len(A), dtype=LD)
    for _ in range(steps):
        X = X @ (eye2 - A @ X)
    return X


def band_dot(Z, N):
    """sum over the symmetric matrices of two bands of Z o N: the diagonal once, the off-diagonal entries twice."""
    return (Z[:, 0] * N[:, 0]).sum() + 2 * (Z[:, 1:] * N[:, 1:]).sum()


def windows(Z, seg, k):
    """Z(s + a, s + b) for every sample's segment s: (n, k, k) from the band."""
    a = np.arange(k)
    hi, lo = np.maximum(a[:, None], a[None, :]), np.abs(a[:, None] - a[None, :])
    return Z[seg[:, None, None] + hi[None], lo[None]]


def leverages(Z, W, seg, w, offdiag_once=False, weight=True):
    """h_j = w_j X_j Z X_j^T in Z's dtype; 0 where w_j = 0. The two flags are faults."""
    k = W.shape[1]
    Wl = np.asarray(W, Z.dtype)
    win = windows(Z, seg, k)
    if offdiag_once:
        win = win * np.tril(np.ones((k, k), Z.dtype))[None]
    h = np.einsum("na,nab,nb->n", Wl, win, Wl)
    if weight:
        h = h * np.asarray(w, Z.dtype)
    return np.where(w > 0, h, Z.dtype.type(0))


# ---- the reference ----
def reference(p, g, l):
    """Z's band, h (n,) and edf of system (g, l) of problem p in long double, from A itself (no ridge); cached on the problem."""
    cache = p.__dict__.setdefault("_cv_reference", {})
    if (g, l) not in cache:
        s = p.sys[g, l]
        L, _ = band_cholesky(np.asarray(s.A, LD), rule=False)
        Z = band_selected_inverse(L)
        cache[g, l] = SimpleNamespace(Z=Z, h=leverages(Z, p.W, p.seg, p.weights[:, g]), edf=band_dot(Z, p.N[g]))
    return cache[g, l]


def leverage_bound(cond):
    """|h - h_ref|: the project's forward-bound convention (fit_smooth_ref.forward_bound) on a quantity of size <= 1."""
    return 1e-14 * cond + 1e-13


def residuals_at(p, g, C):
    """Per sample of group g at control points C, in long double: e_j^2 over the three channels and the square of the sum of the
    magnitudes of its terms (fit_smooth_ref.sums_at's, before the sum over the samples); 0 where the weight is 0."""
    c = p.c
    Cl, Wl, d = np.asarray(C, LD), np.asarray(p.W, LD), np.asarray(c.data[:, 3 * g:3 * g + 3], LD)
    idx = p.seg[:, None] + np.arange(c.order)[None, :]
    use = p.weights[:, g] > 0
    e2, mag2 = np.zeros(len(use), LD), np.zeros(len(use), LD)
    r = np.einsum("nj,njc->nc", Wl[use], Cl[idx[use]]) - d[use]
    mag = np.einsum("nj,njc->nc", np.abs(Wl[use]), np.abs(Cl[idx[use]])) + np.abs(d[use])
    e2[use], mag2[use] = (r * r).sum(1), (mag * mag).sum(1)
    return e2, mag2


def scores_at(p, g, l, C):
    """gcv and press of system (g, l) in long double at control points C with the reference's h and edf, and the bound on each
    that follows from the bounds on what they are made of. With hb = leverage_bound(cond2(A)), n = n_used:
      rss is held to SUM_BOUND of the sum of its terms' magnitudes, edf to hb edf, so to first order
        |d gcv| <= gcv (SUM_BOUND rss_mag / rss + 2 hb edf / (n - edf));
      a PRESS term t_j = w_j e_j^2 / (1 - h_j)^2 has its numerator held as rss's terms are and h_j to hb, so to first order
        |d t_j| <= SUM_BOUND w_j mag_j^2 / (1 - h_j)^2 + t_j 2 hb / (1 - h_j),
      which says nothing once 1 - h_j <= hb (the bound is then infinite)."""
    ref, s, n = reference(p, g, l), p.sys[g, l], p.n_used[g]
    hb = leverage_bound(s.cond)
    w = np.asarray(p.weights[:, g], LD)
    e2, mag2 = residuals_at(p, g, C)
    rss, rss_mag = (w * e2).sum(), (w * mag2).sum()
    out = SimpleNamespace(rss=float(rss), e2=e2, mag2=mag2)
    if ref.edf < n:
        out.gcv = float((rss / (3 * n)) / (1 - ref.edf / n) ** 2)
        rel = fs.SUM_BOUND * rss_mag / rss if rss > 0 else LD(0)
        out.gcv_bound = float(out.gcv * (rel + 2 * hb * ref.edf / (n - ref.edf)))
    else:
        out.gcv, out.gcv_bound = np.inf, 0.0
    q = 1 - ref.h
    if (q[w > 0] <= 0).any():
        out.press, out.press_bound = np.inf, 0.0
    else:
        t = w * e2 / (q * q)
        out.press = float(t.sum() / (3 * n))
        if (q[w > 0] <= hb).any():
            out.press_bound = np.inf
        else:
            out.press_bound = float((fs.SUM_BOUND * w * mag2 / (q * q) + t * 2 * hb / q).sum() / (3 * n))
    return out


def choose(scores, eligible=None):
    """The index of the smallest score among the eligible ones, the last of equal ones (the grid ascends: the larger lambda); -1: none."""
    best = -1
    for l, s in enumerate(scores):
        if (eligible is None or eligible[l]) and not np.isnan(s) and (best < 0 or s <= scores[best]):
            best = l
    return best


def reference_scores(p):
    """{criterion: [group][lambda]} in long double at the reference's own control points (fit_smooth_ref's C_ref), and the RMS of the
    residuals there (unweighted: the noise of the fixtures has one sigma whatever the weights)."""
    out = {"gcv": [[], []], "press": [[], []], "rms": [[], []]}
    for g in range(2):
        for l in range(len(p.grid[g])):
            sc = scores_at(p, g, l, p.sys[g, l].C_ref)
            out["gcv"][g].append(sc.gcv)
            out["press"][g].append(sc.press)
            out["rms"][g].append(float(np.sqrt(sc.e2.sum() / (3 * p.n_used[g]))))      # of the residuals themselves, without the weights
    return out


# ---- the device's algorithm, step by step in float64 (the subject of the test of the test, never a reference) ----
FAULTS = ("offdiagonal_once", "edf_from_a", "weight_missing_in_h", "recursion_one_column_short", "press_not_squared")


def restated_cv_fit(p, criterion="gcv", fault=None):
    """calico_fit_spline_cv in numpy float64 on problem p: the smoothing fit (fit_smooth_ref.restated_smooth_fit), then per (group,
    lambda) the factor of A with the ridge, the selected inversion, edf = sum Z o N, h and e per sample, gcv, press, the largest h;
    the choice per group. Returns the smoothing fit's dict plus cv_rows[g][l], leverage[g][l] and loo[g][l] (per sample, for every
    lambda; the device gives those of the chosen one) and chosen[g]."""
    assert fault is None or fault in FAULTS
    c, nl = p.c, len(p.grid[0])
    out = fs.restated_smooth_fit(p)
    P = fs.penalty_band(c.knots, c.basis, c.order, p.m, dtype=np.float64)
    out.update(cv_rows=[[None] * nl for _ in range(2)], leverage=[[None] * nl for _ in range(2)], loo=[[None] * nl for _ in range(2)], chosen=[-1, -1])
    idx = p.seg[:, None] + np.arange(c.order)[None, :]
    for g in range(2):
        w, n = p.weights[:, g], p.n_used[g]
        use = w > 0
        N, _ = fs.normal_band(p.W, p.seg, w, c.data[:, 3 * g:3 * g + 3], c.n_ctrl, dtype=np.float64)
        for l in range(nl):
            row, lam = out["rows"][g][l], out["rows"][g][l]["lambda"]
            A = N + lam * P if lam != 0 else N
            L, replaced = band_cholesky(A, ridge=fit_ref.RIDGE)
            if replaced:
                out["cv_rows"][g][l] = dict(edf=np.nan, gcv=np.nan, press=np.nan, max_leverage=np.nan)
                continue
            Z = band_selected_inverse(L, short=fault == "recursion_one_column_short")
            edf = float(band_dot(Z, A if fault == "edf_from_a" else N))
            h = leverages(Z, p.W, p.seg, w, offdiag_once=fault == "offdiagonal_once", weight=fault != "weight_missing_in_h")
            r = np.einsum("nj,njc->nc", p.W, out["ctrl_all"][l][:, 3 * g:3 * g + 3][idx]) - c.data[:, 3 * g:3 * g + 3]
            e2 = (r * r).sum(1)
            q = 1.0 - h
            with np.errstate(divide="ignore", invalid="ignore"):
                terms = np.where(h < 1.0, w * e2 / (q if fault == "press_not_squared" else q * q), np.inf)[use]
                loo = np.where(use, np.where(h < 1.0, np.sqrt(e2) / q, np.inf), np.nan)
            out["cv_rows"][g][l] = dict(edf=edf, gcv=(row["rss"] / (3.0 * n)) / (1.0 - edf / n) ** 2 if edf < n else np.inf,
                                        press=float(terms.sum() / (3.0 * n)), max_leverage=float(h[use].max()))
            out["leverage"][g][l], out["loo"][g][l] = h, loo
        out["chosen"][g] = choose([r[criterion] for r in out["cv_rows"][g]])
    return out


# ---- the criteria ----
def check(p, out, verbose=True, label=""):
    """Every criterion of problem p on a result (ctrl_all, cv_rows[g][l], leverage[g][l], loo[g][l]: the per-sample arrays of every
    (group, lambda), None where there is none). Returns {criterion: (measured, bound)}, the worst over groups and lambdas; a
    criterion holds when measured <= bound. Prints one table row per (group, lambda): cond2(A) and the errors of h, edf and of the
    consistency sum over u cond2(A), u = 2^-53."""
    res = {}
    u = 2.0 ** -53

    def worst(key, value, bound):
        ratio = value / bound if bound > 0 else (0.0 if value == 0 else np.inf)
        if key not in res or ratio > res[key][2]:
            res[key] = (value, bound, ratio)
    for (g, l), s in sorted(p.sys.items()):
        ref, row = reference(p, g, l), out["cv_rows"][g][l]
        hb, n = leverage_bound(s.cond), p.n_used[g]
        use = p.weights[:, g] > 0
        worst("finite", 0.0 if np.isfinite(row["edf"]) and np.isfinite(row["max_leverage"]) else 1.0, 0.0)
        if not np.isfinite(row["edf"]):
            continue
        d_edf = abs(float(row["edf"] - ref.edf))
        worst("edf", d_edf, hb * float(ref.edf))
        worst("max_leverage", abs(float(row["max_leverage"] - ref.h[use].max())), hb)
        sc = scores_at(p, g, l, out["ctrl_all"][l][:, 3 * g:3 * g + 3])
        for name in CRITERIA:
            want, bound = getattr(sc, name), getattr(sc, name + "_bound")
            if np.isinf(want):
                worst(name, 0.0 if row[name] == np.inf else 1.0, 0.0)
            elif np.isfinite(bound):
                worst(name, abs(row[name] - want), bound)
        d_h = d_sum = np.nan
        h = out["leverage"][g][l]
        if h is not None:
            d_h = float(np.abs(np.asarray(h, LD) - ref.h).max())
            d_sum = abs(float(np.asarray(h, LD)[use].sum() - LD(row["edf"])))
            worst("leverage", d_h, hb)
            worst("consistency", d_sum, hb * n)
            worst("zero_weight", float(np.abs(h[~use]).sum()) if (~use).any() else 0.0, 0.0)
            loo = out["loo"][g][l]
            worst("zero_weight", 0.0 if np.isnan(loo[~use]).all() and not np.isnan(loo[use]).any() else 1.0, 0.0)
            fin = use & np.isfinite(loo)
            worst("loo_infinite", 0.0 if (h[use & ~fin] >= 1.0).all() else 1.0, 0.0)
            # e_j = loo_j (1 - h_j) with the device's own h, squared, against e_j^2 in long double: held as a term of rss is
            back = (np.asarray(loo[fin], LD) * (1 - np.asarray(h[fin], LD))) ** 2
            excess = np.abs(back - sc.e2[fin]) - fs.SUM_BOUND * sc.mag2[fin]
            worst("loo", float(max(excess.max(), 0)) if fin.any() else 0.0, 0.0)
        if verbose:
            print("%-20s%s order %d m %d group %d lambda %.0e cond2 %.2e  edf %.6g  max h %.3g  |dh| / (u cond2) %.2e  |dedf| / (edf u cond2) %.2e  "
                  "|sum h - edf| / (n u cond2) %.2e  gcv %.4e (err %.1e, bound %.1e)  press %.4e (err %.1e, bound %.1e)" % (
                      p.c.name, label, p.c.order, p.m, g, p.grid[g][l], s.cond, row["edf"], row["max_leverage"], d_h / (u * s.cond),
                      d_edf / (float(ref.edf) * u * s.cond), d_sum / (n * u * s.cond), row["gcv"], abs(row["gcv"] - sc.gcv), sc.gcv_bound,
                      row["press"], abs(row["press"] - sc.press), sc.press_bound))
    return {k: v[:2] for k, v in res.items()}


def failed(result):
    return sorted(k for k, (v, bound) in result.items() if not v <= bound)


# ---- the new small shapes, and the fixtures of the choice ----
def _every_tenth(knots, order, per_segment=7):
    """per_segment samples inside every segment of the valid knots."""
    vk = knots[order - 1:len(knots) - (order - 1)]
    u = (np.arange(per_segment) + 0.5) / per_segment
    return (vk[:-1, None] + u[None, :] * np.diff(vk)[:, None]).ravel()


SMALL = {}      # one and two segments: n_ctrl = order and order + 1
for _k in (2, 6, 8):
    for _extra in (0, 1):
        SMALL["order%d-%d-segments" % (_k, _extra + 1)] = dict(order=_k, n_ctrl=_k + _extra,
                                                               stamps=functools.partial(_every_tenth, order=_k), data=fit_ref.rough_data)
SMALL_GRID = (1e-3, 1.0)      # with m = min(3, order - 1): cond2(A) <= 2.6e9 (m = 1 at order 8 on one segment: 4e13, 1e11)


@functools.lru_cache(maxsize=None)
def small_problem(name):
    c = fit_ref.inputs(SMALL[name])
    c.name = name
    return fs.build(c, fs.sample_weights(len(c.stamps)), min(3, c.order - 1), SMALL_GRID, SMALL_GRID)


CHOICE_CASES = [(0.003, False), (0.01, False), (0.03, False), (0.01, True)]      # (sigma, seeded weights)


@functools.lru_cache(maxsize=None)
def choice_problem(sigma, weighted):
    """smooth_data + sigma N(0, 1) (seed 5) on rough-order6-f1's stamps and knots, m = 2, CHOICE_GRID for both groups, unit or seeded
    weights; built once with its long-double reference."""
    base = fit_ref.case("rough-order6-f1")
    noise = np.random.default_rng(5).standard_normal((len(base.stamps), 6))
    c = SimpleNamespace(name="choice-sigma%g%s" % (sigma, "-weighted" if weighted else ""), order=base.order, n_ctrl=base.n_ctrl, knots=base.knots,
                        basis=base.basis, stamps=base.stamps, data=np.ascontiguousarray(fit_ref.smooth_data(base.stamps) + sigma * noise))
    w = fs.sample_weights(len(c.stamps)) if weighted else np.ones((len(c.stamps), 2))
    p = fs.build(c, w, 2, CHOICE_GRID, CHOICE_GRID)
    p.sigma = sigma
    return p
