"""The smoothing spline fit restated in numpy: what calico_fit_spline_smooth must produce, and the sweep its GPU test runs.

A plain module (numpy only) on tests/fit_ref.py's cases, shared by tests/test_fit_smooth_reference.py, which proves on the CPU
that the criteria tell a right fit from one that is wrong by a little, and tests/test_gpu_fit_smooth.py.

Per channel group g (0: channels 0..2 with weights[:, 0]; 1: channels 3..5 with weights[:, 1]) the device solves
    (X^T W_g X + lambda P) C = X^T W_g d,      P = Gram matrix of the m-th derivatives of the basis functions,
with calico_fit_spline's banded Cholesky (ridge 1e-15 mean_diag of the matrix factored, pivot rule 1e-13 mean_diag). A relative
lambda is in units of trace(X^T W_g X) / trace(P).

Everything here works on the band (row a, entry e = (a, a - e)), so the lengths at the LDS ceiling cost no dense matrix.
- penalty_band: P from the closed form per segment, in long double. penalty_quadrature: the same by Gauss-Legendre quadrature of
  synthetic.spline_weights(..., derivative=m), the independent statement.
- system: A's band and b in long double from the float64 weights of synthetic.spline_weights (never a float64 normal matrix).
- reference_solve: long-double banded Cholesky, refined twice; the exact pivots in units of mean_diag.
- restated_smooth_fit: the device's algorithm step by step in float64, with one fault switched on at a time.
- problem(name, m): a sweep entry built once -- weights, P, and per (group, lambda) A, b, C_ref, cond2(A), replaced pivots.
- check: the criteria, one function for the CPU test of the test and the GPU sweep.
"""
import functools
from types import SimpleNamespace

import numpy as np

import fit_ref
from calico_amd import synthetic as syn

LD = np.longdouble
GRID = (1e-6, 1e-3, 1.0)                    # the sweep's relative lambdas (one call: a three-entry grid)
COND_BOUND = 1e10                           # a condition on the sweep's inputs, not on the device
LAMBDA_BOUND = 1e-12                        # the absolute lambda of a relative one: two sums of n_ctrl positive terms, one division
SUM_BOUND = 1e-12                           # rss and penalty against long double, relative to the sum of their terms' magnitudes


# ---- the penalty ----
def _segment_gram(M, delta, m, exponent_fault=False, denominator_fault=False, dtype=LD):
    """D^(1-2m) M^T H M of one segment: H_ij = c_i c_j / (i + j - 2m + 1), c_i = i! / (i - m)! for i, j >= m."""
    k = len(M)
    H = np.zeros((k, k), dtype)
    for i in range(m, k):
        for j in range(m, k):
            ci = np.prod([dtype(i - q) for q in range(m)])
            cj = np.prod([dtype(j - q) for q in range(m)])
            H[i, j] = ci * cj / dtype(i + j - 2 * m + (2 if denominator_fault else 1))
    Ml = np.asarray(M, dtype)
    return dtype(delta) ** ((2 if exponent_fault else 1) - 2 * m) * (Ml.T @ H @ Ml)


def penalty_band(knots, basis, order, m, dtype=LD, **faults):
    """Band of P (n_ctrl x order): summed in segment order over the segments that hold both control points."""
    k, n_ctrl = order, len(knots) - order
    band = np.zeros((n_ctrl, k), dtype)
    for s in range(len(basis)):
        G = _segment_gram(basis[s], dtype(knots[s + k]) - dtype(knots[s + k - 1]), m, dtype=dtype, **faults)
        for ia in range(k):
            for ib in range(ia + 1):
                band[s + ia, ia - ib] += G[ia, ib]
    return band


def penalty_quadrature(knots, basis, order, m, points=12):
    """Dense P by Gauss-Legendre quadrature (exact for the degree 2 (order - 1 - m) integrand) of spline_weights' m-th derivative."""
    k, n_ctrl = order, len(knots) - order
    x, w = np.polynomial.legendre.leggauss(points)
    P = np.zeros((n_ctrl, n_ctrl))
    for s in range(len(basis)):
        t0, t1 = knots[s + k - 1], knots[s + k]
        t = t0 + (t1 - t0) * (x + 1.0) / 2.0
        D, _ = syn.spline_weights(knots, basis, k, t, m, seg=np.full(points, s))
        P[s:s + k, s:s + k] += (D * (w * (t1 - t0) / 2.0)[:, None]).T @ D
    return P


# ---- band algebra ----
def band_to_dense(band):
    n, k = band.shape
    A = np.zeros((n, n), band.dtype)
    for e in range(k):
        i = np.arange(e, n)
        A[i, i - e] = band[e:, e]
        A[i - e, i] = band[e:, e]
    return A


def band_matvec(band, C):
    """A C for the symmetric matrix of a band."""
    n, k = band.shape
    Y = band[:, :1] * C
    for e in range(1, min(k, n)):
        Y[e:] += band[e:, e:e + 1] * C[:n - e]
        Y[:n - e] += band[e:, e:e + 1] * C[e:]
    return Y


def band_inf_norm(band):
    return float(band_matvec(np.abs(band), np.ones((len(band), 1), band.dtype)).max())


def normal_band(W, seg, w, data, n_ctrl, dtype=LD, rhs_weight=None):
    """(band of X^T diag(w) X, X^T diag(w) data), samples of weight 0 left out. rhs_weight: the weights of the right-hand side
    (a fault's; w by default)."""
    k = W.shape[1]
    use = np.flatnonzero(w > 0)
    Wl, wl, dl, sg = np.asarray(W[use], dtype), np.asarray(w[use], dtype), np.asarray(data[use], dtype), seg[use]
    wr = wl if rhs_weight is None else np.asarray(rhs_weight[use], dtype)
    band, rhs = np.zeros((n_ctrl, k), dtype), np.zeros((n_ctrl, data.shape[1]), dtype)
    for ia in range(k):
        np.add.at(rhs, sg + ia, Wl[:, ia:ia + 1] * (dl * wr[:, None]))
        for ib in range(ia + 1):
            np.add.at(band[:, ia - ib], sg + ia, Wl[:, ia] * (Wl[:, ib] * wl))
    return band, rhs


def band_cholesky_solve(band, rhs, ridge=0.0, rule=True):
    """Right-looking banded Cholesky and the two substitutions in the band's own dtype. Returns (solution, pivots / mean_diag,
    replaced): `replaced` counts the pivots <= 1e-13 mean_diag, which `rule` replaces by mean_diag as the device does."""
    n, k = band.shape
    B, Y = band.copy(), rhs.copy()
    mean_diag = B[:, 0].sum() / n
    B[:, 0] += B.dtype.type(ridge) * mean_diag
    piv, replaced = np.zeros(n), 0
    for j in range(n):
        d = B[j, 0]
        piv[j] = float(d / mean_diag)
        if not d > B.dtype.type(fit_ref.PIVOT_RULE) * mean_diag:
            replaced += 1
            if rule:
                d = mean_diag
        inv = 1 / np.sqrt(d)
        B[j, 0] = d * inv
        h = min(k, n - j)
        col = np.array([B[j + i, i] for i in range(1, h)], B.dtype) * inv        # L(j+i, j)
        for i in range(1, h):
            B[j + i, i] = col[i - 1]
            B[j + i, i - 1::-1][:i] -= col[i - 1] * col[:i]                        # entries (j+i, j+c), c = 1..i
    for a in range(n):
        for d in range(1, min(k - 1, a) + 1):
            Y[a] -= B[a, d] * Y[a - d]
        Y[a] /= B[a, 0]
    for a in range(n - 1, -1, -1):
        for d in range(1, min(k, n - a)):
            Y[a] -= B[a + d, d] * Y[a + d]
        Y[a] /= B[a, 0]
    return Y, piv, replaced


def reference_solve(A_band, b):
    """Long-double Cholesky of A (no ridge), refined twice against the long-double residual. (C_ref float64, exact pivots in
    units of mean_diag, pivots the rule would replace)."""
    C, piv, replaced = band_cholesky_solve(A_band, b)
    for _ in range(2):
        C = C + band_cholesky_solve(A_band, b - band_matvec(A_band, C))[0]
    return np.asarray(C, float), piv, replaced


# ---- the sweep ----
CASE_NAMES = ["gap-12-segments", "gap-4.5-segments", "one-per-segment", "two-per-segment", "n3", "stamps-on-knots",
              "all-in-one-segment", "rough-order6-f1"] + ["order%d-f0.1" % k for k in range(2, 9)]
# The sweep is every case at m = 1, 2 (and 3 at order >= 6) with the lambdas of GRID at which cond2(A) <= COND_BOUND in both
# groups under the seeded weights (test_fit_smooth_reference.py asserts that for every entry). Left out, with their cond2:
# lambda 1e-6 on one-per-segment m 1 (8e10), stamps-on-knots m 1 (9e10), n3 m 1, 2 (7e11, 2e11), all-in-one-segment m 1, 2
# (1e12, 5e12), order7-f0.1 m 1, 2 (2e11, 3e10), order8-f0.1 m 1, 2, 3 (3e13, 2e12, 1e11); lambda 1e-3 on order8-f0.1 m 1 (1e11);
# m = 3 on n3 and all-in-one-segment altogether (2e14, 2e15 at 1e-6: three samples, or samples in one segment, leave the
# penalty's null space of quadratics to a few control points).
_NOT_1E6 = {("one-per-segment", 1), ("stamps-on-knots", 1), ("n3", 1), ("n3", 2), ("all-in-one-segment", 1), ("all-in-one-segment", 2),
            ("order7-f0.1", 1), ("order7-f0.1", 2), ("order8-f0.1", 1), ("order8-f0.1", 2), ("order8-f0.1", 3)}
_NOT_1E3 = {("order8-f0.1", 1)}
_NO_M3 = {"n3", "all-in-one-segment"}
SWEEP = {}
for _name in CASE_NAMES:
    _order = fit_ref.CASES[_name]["order"]
    for _m in (1, 2, 3):
        if _m > _order - 1 or (_m == 3 and (_order < 6 or _name in _NO_M3)):
            continue
        SWEEP[_name, _m] = tuple(lam for lam in GRID if not (lam == 1e-6 and (_name, _m) in _NOT_1E6) and not (lam == 1e-3 and (_name, _m) in _NOT_1E3))


def sample_weights(n, seed=23):
    """Seeded weights in [0.25, 4], log-uniform, the rotation and position columns drawn separately."""
    return np.ascontiguousarray(4.0 ** np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 2)))


def build(c, weights, m, grid_rot, grid_pos, relative=True, reference=True):
    """A problem on case c (fit_ref.case / fit_ref.inputs): P, and per group g and grid index l the absolute lambda, A's band and
    b in long double, and with `reference` C_ref, cond2(A) and the exact replaced pivots."""
    p = SimpleNamespace(c=c, m=m, weights=weights, grid=(tuple(grid_rot), tuple(grid_pos)), relative=relative)
    p.W, p.seg = syn.spline_weights(c.knots, c.basis, c.order, c.stamps, 0)
    p.P = penalty_band(c.knots, c.basis, c.order, m)
    p.n_used = [int((weights[:, g] > 0).sum()) for g in range(2)]
    p.N, p.b, p.sys = [], [], {}
    for g in range(2):
        N, b = normal_band(p.W, p.seg, weights[:, g], c.data[:, 3 * g:3 * g + 3], c.n_ctrl)
        p.N.append(N)
        p.b.append(b)
        unit = N[:, 0].sum() / p.P[:, 0].sum() if relative else LD(1)
        for l, lam in enumerate(p.grid[g]):
            s = SimpleNamespace(lam=LD(lam) * unit)
            s.A = N + s.lam * p.P
            if reference:
                s.C_ref, s.pivots, s.replaced = reference_solve(s.A, b)
                s.cond = float(np.linalg.cond(np.asarray(band_to_dense(s.A), float)))
            p.sys[g, l] = s
    return p


@functools.lru_cache(maxsize=None)
def problem(name, m):
    """A sweep entry, built once and never changed: fit_ref's case, seeded weights, the entry's lambdas for both groups."""
    c = fit_ref.case(name)
    return build(c, sample_weights(len(c.stamps)), m, SWEEP[name, m], SWEEP[name, m])


# ---- the device's algorithm, step by step in float64 (the subject of the test of the test, never a reference) ----
FAULTS = ("delta_exponent", "h_denominator", "weight_not_on_rhs", "rotation_weights_for_position", "neighbour_lambda")


def restated_smooth_fit(p, fault=None):
    """calico_fit_spline_smooth's kernels in numpy float64 on problem p: P per band entry, [band | rhs] per group with the weights,
    lambda from the two traces, A = N + lambda P, ridge, banded Cholesky with the pivot rule, substitutions, c'Pc and the weighted
    rss. Returns what the device returns: ctrl_all (n_lambda, n_ctrl, 6) and rows[g][l]. `fault`: one of FAULTS."""
    assert fault is None or fault in FAULTS
    c, nl = p.c, len(p.grid[0])
    P = penalty_band(c.knots, c.basis, c.order, p.m, dtype=np.float64, exponent_fault=fault == "delta_exponent",
                     denominator_fault=fault == "h_denominator")
    ctrl_all = np.zeros((nl, c.n_ctrl, 6))
    rows = [[None] * nl for _ in range(2)]
    for g in range(2):
        w = p.weights[:, 0 if fault == "rotation_weights_for_position" else g]
        d = c.data[:, 3 * g:3 * g + 3]
        N, rhs = normal_band(p.W, p.seg, w, d, c.n_ctrl, dtype=np.float64, rhs_weight=np.ones_like(w) if fault == "weight_not_on_rhs" else None)
        for l in range(nl):
            grid = p.grid[g]
            lam = grid[l + 1 if l + 1 < nl else l - 1] if fault == "neighbour_lambda" else grid[l]
            if p.relative:
                lam = lam * (N[:, 0].sum() / P[:, 0].sum())
            C, _, replaced = band_cholesky_solve(N + lam * P if lam != 0 else N, rhs, ridge=fit_ref.RIDGE)
            ctrl_all[l, :, 3 * g:3 * g + 3] = C
            r = np.einsum("nj,njc->nc", p.W, C[p.seg[:, None] + np.arange(c.order)[None, :]]) - d
            rss = float((p.weights[:, g][:, None] * r * r)[p.weights[:, g] > 0].sum())
            rows[g][l] = dict(status=0, replaced_pivots=replaced, rss=rss, penalty=float((C * band_matvec(P, C)).sum()),
                              rms=float(np.sqrt(rss / (3 * p.n_used[g]))), **{"lambda": float(lam)})
    return dict(ctrl_all=ctrl_all, rows=rows)


# ---- the criteria ----
def forward_bound(cond, C_ref, data):
    """The bound on max|C - C_ref| and on the fitted values: 1e-14 cond2(A) max|C_ref| + 1e-13 max|data|. The Cholesky solve of A
    contributes a few u cond2(A), the ridge 1e-15 mean_diag at most 1e-15 cond2(A); 1e-14 leaves about a factor 5 over their sum."""
    return 1e-14 * cond * np.abs(C_ref).max() + 1e-13 * np.abs(data).max()


def backward_error(A_band, b, C):
    """Normwise backward error per right-hand side against A and b in long double: max|A C - b| / (||A||_inf max|C| + max|b|)."""
    Cl = np.asarray(C, LD)
    r = np.abs(band_matvec(A_band, Cl) - b).max(0)
    den = band_inf_norm(A_band) * np.abs(Cl).max(0) + np.abs(b).max(0)
    return np.array([float(x / y) if y > 0 else float(x) for x, y in zip(r, den)])


def sums_at(p, g, C):
    """rss and penalty of group g at control points C in long double, and the sums of the magnitudes of their terms (what a
    relative error of a sum that cancels is relative to: rss's terms are w (sum_a X_ja C_a - d_j)^2, the penalty's C_a P_ab C_b)."""
    c, w = p.c, np.asarray(p.weights[:, g], LD)
    Cl, Wl, d = np.asarray(C, LD), np.asarray(p.W, LD), np.asarray(c.data[:, 3 * g:3 * g + 3], LD)
    idx = p.seg[:, None] + np.arange(c.order)[None, :]
    use = np.asarray(p.weights[:, g] > 0)
    r = np.einsum("nj,njc->nc", Wl[use], Cl[idx[use]]) - d[use]
    mag = np.einsum("nj,njc->nc", np.abs(Wl[use]), np.abs(Cl[idx[use]])) + np.abs(d[use])
    rss, rss_mag = (w[use, None] * r * r).sum(), (w[use, None] * mag * mag).sum()
    pen, pen_mag = (Cl * band_matvec(p.P, Cl)).sum(), (np.abs(Cl) * band_matvec(np.abs(p.P), np.abs(Cl))).sum()
    return float(rss), float(rss_mag), float(pen), float(pen_mag)


def check(p, out, verbose=True, label=""):
    """Every criterion of problem p on a result (ctrl_all, rows[g][l]). Returns {criterion: (measured, bound)}, the worst over
    groups and lambdas; a criterion holds when measured <= bound. Prints one table row per (group, lambda): cond2(A), eta, and
    the control-point and fitted-value differences over 1e-15 cond2(A) max|C_ref| (the ridge's own share of the bound)."""
    c = p.c
    res = {}

    def worst(key, value, bound):
        ratio = value / bound if bound > 0 else (0.0 if value == 0 else np.inf)
        if key not in res or ratio > res[key][2]:
            res[key] = (value, bound, ratio)
    idx = p.seg[:, None] + np.arange(c.order)[None, :]
    for (g, l), s in sorted(p.sys.items()):
        C, row = out["ctrl_all"][l][:, 3 * g:3 * g + 3], out["rows"][g][l]
        worst("finite", 0.0 if np.isfinite(C).all() and row["status"] == 0 else 1.0, 0.0)
        if not np.isfinite(C).all():
            continue
        eta = backward_error(s.A, p.b[g], C).max()
        worst("eta", eta, fit_ref.ETA_BOUND)
        bound, unit = forward_bound(s.cond, s.C_ref, c.data), 1e-15 * s.cond * np.abs(s.C_ref).max()
        dc = np.abs(C - s.C_ref).max()
        df = np.abs(np.einsum("nj,njc->nc", p.W, (C - s.C_ref)[idx])).max()
        worst("control_points", dc, bound)
        worst("fitted_values", df, bound)
        worst("replaced_pivots", float(row["replaced_pivots"]), 0.0)
        worst("lambda", abs(row["lambda"] - float(s.lam)), LAMBDA_BOUND * float(s.lam))
        rss, rss_mag, pen, pen_mag = sums_at(p, g, C)
        worst("rss", abs(row["rss"] - rss), SUM_BOUND * rss_mag)
        worst("penalty", abs(row["penalty"] - pen), SUM_BOUND * pen_mag)
        rms = np.sqrt(row["rss"] / (3 * p.n_used[g]))                      # (of the row's own rss: a division and a root)
        worst("rms", abs(row["rms"] - rms), 1e-15 * rms)
        if verbose:
            print("%-20s%s order %d m %d group %d lambda %.0e (abs %.2e) cond2 %.2e  eta %.1e  ctrl ratio %.2e  fit ratio %.2e  "
                  "rss %.3e (err / terms %.1e, / value %.1e)  penalty %.3e (err / terms %.1e, / value %.1e)" % (
                      c.name, label, c.order, p.m, g, p.grid[g][l], float(s.lam), s.cond, eta, dc / unit, df / unit, rss,
                      abs(row["rss"] - rss) / rss_mag, abs(row["rss"] - rss) / rss if rss > 0 else 0.0, pen,
                      abs(row["penalty"] - pen) / pen_mag, abs(row["penalty"] - pen) / pen if pen > 0 else 0.0))
    return {k: v[:2] for k, v in res.items()}


def failed(result):
    return sorted(k for k, (v, bound) in result.items() if not v <= bound)
