"""The spline fit restated in numpy: what calico_fit_spline must produce, and the cases its GPU sweep runs.

A plain module (numpy only), shared by tests/test_fit_reference.py, which proves on the CPU that its criteria tell a right fit
from one that is wrong by a little, and tests/test_gpu_fit_spline.py, which holds the device's control points against it.

The device solves  min_C ||X C - data||^2,  X(j, seg_j + a) = w_a(t_j),  through the banded normal equations N C = b
(N = X^T X, b = X^T data) with a right-looking banded Cholesky. Its documented contract: a ridge of 1e-15 mean_diag on the
diagonal (mean_diag = trace(N) / n_ctrl), and a pivot <= 1e-13 mean_diag is replaced by mean_diag, so that a control point the
samples do not determine drops out (comes back ~ 0).

- design_matrix: X from synthetic.spline_weights, the independent numpy restatement of the weights.
- exact_pivots: the Cholesky pivots of N in long double, divided by mean_diag, under the documented rule.
- reference_fit: the contract's answer -- the columns with an exact pivot <= 1e-13 dropped, least squares on the rest by
  QR/SVD on X itself (never the normal equations), refined twice against a long-double residual.
- backward_error: how close given control points are to solving N C = b.
- restated_fit: the device's algorithm step by step in float64, with one fault switched on at a time (the test of the test).
- CASES / case(name): the sweep. Every case is built once per process and never changed.
"""
import functools
from types import SimpleNamespace

import numpy as np

from calico_amd import synthetic as syn

LD = np.longdouble
RIDGE, PIVOT_RULE = 1e-15, 1e-13            # the device's ridge and pivot threshold, both in units of mean_diag
BAND_LO, BAND_HI = 1e-14, 1e-12             # one decade either side of the rule: float64 may decide either way inside
ETA_BOUND = 1e-11                           # tests/test_gpu_linear_step.py's bound on a backward error
DROPPED_BOUND = 1e-12                       # |C_j| <= DROPPED_BOUND max|data| on a dropped column
KNOT_HZ = 10.0
LDS_CEILING = 156 * 1024                    # bytes of [band | rhs] the on-chip solve accepts: n_ctrl (k + 6) 8


# ---- the reference ----
def uniform_knots(n_ctrl, order, knot_frequency=KNOT_HZ):
    """The knot vector of synthetic.knot_vector(0, n_seg / f, order, f) with n_seg = n_ctrl - (order - 1) segments."""
    deg = order - 1
    dt = 1.0 / knot_frequency
    return np.array([0.0 + dt * i for i in range(-deg, n_ctrl + 1)])


def design_matrix(knots, basis, order, stamps):
    """X (n x n_ctrl) and the samples' segments."""
    W, seg = syn.spline_weights(knots, basis, order, stamps, 0)
    X = np.zeros((len(stamps), len(knots) - order))
    X[np.arange(len(stamps))[:, None], seg[:, None] + np.arange(order)[None, :]] = W
    return X, seg


def _half_bandwidth(X):
    nz = X != 0.0
    first = np.where(nz.any(1), nz.argmax(1), 0)
    last = np.where(nz.any(1), X.shape[1] - 1 - nz[:, ::-1].argmax(1), 0)
    return int((last - first).max()) if len(X) else 0


def normal_matrix_ld(X):
    """N = X^T X in long double (dense; only the band is computed, the rest is exactly zero)."""
    Xl = np.asarray(X, LD)
    m = X.shape[1]
    N = np.zeros((m, m), LD)
    for d in range(min(_half_bandwidth(X), m - 1) + 1):
        v = (Xl[:, :m - d] * Xl[:, d:]).sum(0)
        i = np.arange(m - d)
        N[i + d, i] = v
        N[i, i + d] = v
    return N


def exact_pivots(X):
    """Right-looking Cholesky pivots of N = X^T X in long double, divided by mean_diag = trace(N) / n_ctrl, under the
    documented rule (a pivot <= 1e-13 is replaced by mean_diag before its column is eliminated). No ridge."""
    N = normal_matrix_ld(X)
    m = len(N)
    p = _half_bandwidth(X)
    mean_diag = np.trace(N) / m
    piv = np.zeros(m)
    for j in range(m):
        d = N[j, j]
        piv[j] = float(d / mean_diag)
        if not d > LD(PIVOT_RULE) * mean_diag:
            d = mean_diag
        hi = min(m, j + p + 1)
        col = N[j + 1:hi, j] / d
        N[j + 1:hi, j + 1:hi] -= np.outer(col, N[j + 1:hi, j])
    return piv


def _svd_solver(X):
    """Least squares on X through its thin SVD (full column rank expected), and cond2(X)."""
    U, sv, Vt = np.linalg.svd(X, full_matrices=False)
    cond = float(sv[0] / sv[-1]) if len(sv) and sv[-1] > 0 else np.inf
    return (lambda d: Vt.T @ ((U.T @ d) / sv[:, None])), cond


def reference_fit(X, data, pivots=None, refine=2):
    """(C_ref, kept, cond2(X_kept), exact pivots): the columns whose exact pivot is <= 1e-13 are dropped (C_ref = 0 there),
    the others solve least squares on X's kept columns by SVD, refined twice against a long-double residual."""
    piv = exact_pivots(X) if pivots is None else pivots
    kept = piv > PIVOT_RULE
    Xk = X[:, kept]
    solve, cond = _svd_solver(Xk)
    Ck = solve(data)
    Xl = np.asarray(Xk, LD)
    for _ in range(refine):
        r = np.asarray(data, LD) - Xl @ np.asarray(Ck, LD)
        Ck = Ck + solve(np.asarray(r, float))
    C = np.zeros((X.shape[1], data.shape[1]))
    C[kept] = Ck
    return C, kept, cond, piv


def minimum_norm_fit(X, data):
    """The minimum-norm least-squares control points, as synthetic.spline_fit computes them (rcond 1e-9)."""
    return np.linalg.lstsq(X, data, rcond=1e-9)[0]


def backward_error(X, data, C):
    """Normwise backward error of the normal equations per right-hand side, N and b accumulated in long double:
    eta = max|N C - b| / (||N||_inf max|C| + max|b|)."""
    N = normal_matrix_ld(X)
    b = np.asarray(X, LD).T @ np.asarray(data, LD)
    Cl = np.asarray(C, LD)
    r = np.abs(N @ Cl - b).max(0)
    den = np.abs(N).sum(1).max() * np.abs(Cl).max(0) + np.abs(b).max(0)
    return np.array([float(x / y) if y > 0 else float(x) for x, y in zip(r, den)])


def forward_bound(cond, C_ref, data):
    """The bound on max|C - C_ref| over the kept columns and on max|X C - X C_ref|:
    1e-14 cond2(X_kept)^2 max|C_ref| + 1e-13 max|data|. The ridge r = 1e-15 mean_diag moves the solution by at most
    r / sigma_min^2 ||C|| <= 1e-15 cond2^2 ||C||; the rest of the factor covers the Cholesky's own u cond2^2 term."""
    return 1e-14 * cond ** 2 * np.abs(C_ref).max() + 1e-13 * np.abs(data).max()


# ---- the device's algorithm, step by step in float64 (the subject of the test of the test, never a reference) ----
FAULTS = ("band_entry", "sample_left_out", "sample_in_neighbour_segment", "backsubstitution_short", "ridge_1e-9")


def restated_fit(knots, basis, order, stamps, data, fault=None):
    """calico_fit_spline's three kernels in numpy float64: weights per sample, [band | rhs] summed over the samples in
    order, ridge, right-looking banded Cholesky with the pivot rule, forward and backward substitution. `fault` (one of
    FAULTS) seeds one mistake a kernel of this shape can make."""
    assert fault is None or fault in FAULTS
    k, m, n = order, len(knots) - order, len(stamps)
    W, seg = syn.spline_weights(knots, basis, k, stamps, 0)
    seg = seg.copy()
    use = np.ones(n, bool)
    if fault == "sample_left_out":
        use[n // 2] = False
    if fault == "sample_in_neighbour_segment":        # binned one segment early, its weights unchanged
        j = n // 2
        assert seg[j] > 0
        seg[j] -= 1
    band = np.zeros((m, k))          # band[a][e] = N(a, a - e)
    rhs = np.zeros((m, data.shape[1]))
    for j in np.flatnonzero(use):
        s = seg[j]
        for ia in range(k):
            rhs[s + ia] += W[j, ia] * data[j]
            for ib in range(ia + 1):
                band[s + ia, ia - ib] += W[j, ia] * W[j, ib]
    if fault == "band_entry":
        band[m // 2, 1] = 0.0
    mean_diag = band[:, 0].sum() / m
    B = band.copy()
    B[:, 0] += (1e-9 if fault == "ridge_1e-9" else RIDGE) * mean_diag
    for j in range(m):
        d = B[j, 0]
        if not d > PIVOT_RULE * mean_diag:
            d = mean_diag
        inv = 1.0 / np.sqrt(d)
        B[j, 0] = d * inv
        for i in range(1, k):
            if j + i < m:
                B[j + i, i] *= inv
        for i in range(1, k):
            for c in range(1, i + 1):
                if j + i < m:
                    B[j + i, i - c] -= B[j + i, i] * B[j + c, c]
    Y = rhs.copy()
    for a in range(m):
        for d in range(1, min(k - 1, a) + 1):
            Y[a] -= B[a, d] * Y[a - d]
        Y[a] /= B[a, 0]
    for a in range(m - 1, 0 if fault == "backsubstitution_short" else -1, -1):
        for d in range(1, k):
            if a + d < m:
                Y[a] -= B[a + d, d] * Y[a + d]
        Y[a] /= B[a, 0]
    return Y


# ---- the sweep ----
def smooth_data(t):
    """Six smooth channels of amplitude O(1) (test_fit_matches_oracle's)."""
    return np.stack([np.sin(0.7 * t + i) * (1.0 + 0.1 * i) + 0.05 * t for i in range(6)], 1)


def _grid(t_end, rate):
    """Stamps i / rate up to t_end, and t_end itself as the last one."""
    t = np.arange(int(np.floor(t_end * rate * (1 + 1e-12))) + 1) / rate
    t = t[t < t_end]
    return np.append(t, t_end)


def rough_data(t):
    """smooth_data plus seeded noise of sigma 0.1: data no spline of the sweep represents, so that every sample counts (the
    smooth channels are fitted to ~1e-9, and a fit that loses one of 500 such samples moves by less than the bounds)."""
    return smooth_data(t) + 0.1 * np.random.default_rng(11).standard_normal((len(t), 6))


def _ragged(order, f, n_ctrl=57, rate=100.0):
    """Samples at `rate` whose last one lies at fraction f of the last segment. f = 1: the last valid knot itself, or the
    double below it where knot_vector(t0, t1, ...) would round the duration up to one segment more (0.1 * 56 * 10 > 56)."""
    def make(knots):
        vk = knots[order - 1:len(knots) - (order - 1)]
        end = vk[-1] if f == 1.0 else vk[-2] + f * (vk[-1] - vk[-2])
        while np.ceil((end - vk[0]) * KNOT_HZ) > len(vk) - 1:
            end = np.nextafter(end, vk[0])
        return _grid(end, rate)
    return dict(order=order, n_ctrl=n_ctrl, stamps=make)


def _with_gap(n_segments):
    def make(knots):
        t = _grid(knots[5:-5][-1], 100.0)
        return t[(t < 2.0) | (t >= 2.0 + n_segments / KNOT_HZ)]
    return dict(order=6, n_ctrl=57, stamps=make)


def _per_segment(count):
    def make(knots):
        vk = knots[5:-5]
        u = (np.arange(count) + 0.5) / count if count > 1 else np.array([0.37])
        return (vk[:-1, None] + u[None, :] * np.diff(vk)[:, None]).ravel()
    return dict(order=6, n_ctrl=57, stamps=make)


def _few(n):
    # a sample 34 % into its segment, one on a knot, one 71 % into its segment
    return dict(order=6, n_ctrl=57, stamps=lambda knots: np.array([0.234, 2.5, 4.071])[:n])


def _on_knots(knots):
    return knots[5:-5].copy()


def _repeated(knots):
    t = _grid(knots[5:-5][-1], 100.0)
    return np.sort(np.concatenate([t, np.repeat(t[257], 3)]))


def _one_segment(knots):
    vk = knots[5:-5]
    return vk[20] + (vk[21] - vk[20]) * (np.arange(40) + 0.5) / 40


# kind "posed": held to reference_fit (the decoupling comparison) unless one of its exact pivots lies in the band, which
# only the cases named in BAND_CASES may; kind "deficient": held to the minimum-norm solution.
CASES = {}
for _k in range(2, 9):
    for _f in (1.0, 0.02, 0.1, 0.5):
        CASES["order%d-f%g" % (_k, _f)] = dict(_ragged(_k, _f), kind="posed")
CASES.update({
    "gap-12-segments": dict(_with_gap(12), kind="posed"),
    "gap-4.5-segments": dict(_with_gap(4.5), kind="posed"),
    "two-per-segment": dict(_per_segment(2), kind="posed"),
    "one-per-segment": dict(_per_segment(1), kind="deficient"),
    "n1": dict(_few(1), kind="deficient"),
    "n2": dict(_few(2), kind="deficient"),
    "n3": dict(_few(3), kind="deficient"),
    "stamps-on-knots": dict(order=6, n_ctrl=57, stamps=_on_knots, kind="deficient"),
    "stamp-repeated-4x": dict(order=6, n_ctrl=57, stamps=_repeated, kind="posed"),
    "all-in-one-segment": dict(order=6, n_ctrl=57, stamps=_one_segment, kind="posed"),
    "rough-order6-f1": dict(_ragged(6, 1.0), kind="posed", data=rough_data),
    "rough-order6-f0.5": dict(_ragged(6, 0.5), kind="posed", data=rough_data),
    "order6-683": dict(_ragged(6, 1.0, 683, 20.0), kind="posed"),          # first size above 64 KiB of LDS
    "order6-1664": dict(_ragged(6, 1.0, 1664, 20.0), kind="posed"),        # the ceiling: 1664 (6 + 6) 8 = 156 KiB
    "order8-1426": dict(_ragged(8, 1.0, 1426, 20.0), kind="posed"),        # order 8's ceiling
    "order2-2000": dict(_ragged(2, 1.0, 2000, 20.0), kind="posed"),
})
TOO_LONG = {"order6-1665": dict(_ragged(6, 1.0, 1665, 20.0)), "order8-1427": dict(_ragged(8, 1.0, 1427, 20.0))}
# Not in the device sweep: noise where the rule drops a determined control point (see test_fit_reference.py for what it does)
NOISY_CLIFF = dict(_ragged(6, 0.1), data=rough_data)
ORACLE_CASES = ["order%d-f1" % k for k in range(2, 9)]
BAND_CASES = {"order4-f0.02", "order8-f0.5"}        # exact pivots 2.2e-13 and 2.8e-14: the eta criterion only
REPEAT_CASE = "order6-683"


def inputs(spec):
    """knots, basis, stamps, data of a case's specification."""
    order = spec["order"]
    knots = uniform_knots(spec["n_ctrl"], order)
    basis = np.ascontiguousarray(syn.basis_matrices(knots, order))
    stamps = np.ascontiguousarray(spec["stamps"](knots), dtype=float)
    return SimpleNamespace(order=order, n_ctrl=spec["n_ctrl"], knots=knots, basis=basis, stamps=stamps,
                           data=np.ascontiguousarray(spec.get("data", smooth_data)(stamps)))


@functools.lru_cache(maxsize=None)
def case(name):
    """A case of CASES, built once: its inputs, X, the exact pivots and whether one of them lies in the band."""
    c = inputs(CASES[name])
    c.name, c.kind = name, CASES[name]["kind"]
    c.X, c.seg = design_matrix(c.knots, c.basis, c.order, c.stamps)
    c.pivots = exact_pivots(c.X)
    c.in_band = bool(((c.pivots > BAND_LO) & (c.pivots < BAND_HI)).any())
    for a in (c.knots, c.basis, c.stamps, c.data, c.X, c.pivots):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference of a case, computed once: C_ref, kept, cond (posed) or C_minnorm (deficient)."""
    c = case(name)
    r = SimpleNamespace()
    if c.kind == "deficient":
        r.C_minnorm = minimum_norm_fit(c.X, c.data)
        r.C_minnorm.setflags(write=False)
    else:
        r.C_ref, r.kept, r.cond, _ = reference_fit(c.X, c.data, c.pivots)
        r.C_ref.setflags(write=False)
    return r


def oracle_fit(oracle, c):
    """The CPU oracle's FitToData on a case's samples; it builds the knot vector itself (asserted to be the case's)."""
    import ctypes as C
    D = C.POINTER(C.c_double)
    dp = lambda a: a.ctypes.data_as(D)      # noqa: E731
    lib = oracle.lib
    lib.oracle_spline_create.restype = C.c_void_p
    lib.oracle_spline_destroy.argtypes = [C.c_void_p]
    lib.oracle_spline_fit_vectors.argtypes = [C.c_void_p, C.c_int32, D, D, C.c_double, C.c_int32]
    lib.oracle_spline_get.argtypes = [C.c_void_p, D, D, D]
    s = C.c_void_p(lib.oracle_spline_create())
    try:
        assert lib.oracle_spline_fit_vectors(s, len(c.stamps), dp(c.stamps), dp(c.data), C.c_double(KNOT_HZ), c.order) == 0
        knots, basis, ctrl = np.zeros(len(c.knots) + 8), np.zeros(c.basis.size + 8 * c.order ** 2), np.zeros((c.n_ctrl + 8, 6))
        lib.oracle_spline_get(s, dp(knots), dp(basis), dp(ctrl))
    finally:
        lib.oracle_spline_destroy(s)
    assert np.array_equal(knots[:len(c.knots)], c.knots) and (knots[len(c.knots):] == 0).all() and (ctrl[c.n_ctrl:] == 0).all()
    return ctrl[:c.n_ctrl]


# ---- the criteria, one function for the CPU test of the test and the GPU sweep ----
def check(c, C, verbose=True):
    """Every criterion of case c on control points C. Returns {criterion: (measured, bound)}; a criterion holds when
    measured <= bound. Prints the table row: order, n_ctrl, dropped columns, cond2, eta, control-point and fitted-value ratio
    (measured difference over 1e-15 cond2^2 max|C_ref|, the ridge's own share of the bound)."""
    out = {"finite": (0.0 if np.isfinite(C).all() else 1.0, 0.0)}
    if not np.isfinite(C).all():
        return out
    scale = np.abs(c.data).max()
    eta = backward_error(c.X, c.data, C).max()
    out["eta"] = (eta, ETA_BOUND)
    row = "%-22s order %d n_ctrl %4d" % (c.name, c.order, c.n_ctrl)
    ref = None if c.kind == "posed" and c.in_band else reference(c.name)
    if c.kind == "deficient":
        fit = np.abs(c.X @ C - c.X @ ref.C_minnorm).max()
        out["fitted_values_vs_minimum_norm"] = (fit, 1e-9 * scale)
        out["size_vs_minimum_norm"] = (np.abs(C).max(), 10.0 * np.abs(ref.C_minnorm).max())
        row += " rank-deficient            eta %.1e  |fit - minnorm| %.1e  max|C| / max|C_minnorm| %.2f" % (
            eta, fit, np.abs(C).max() / np.abs(ref.C_minnorm).max())
    elif c.in_band:
        row += " pivot in the band         eta %.1e  (eta only)" % eta
    else:
        dropped = ~ref.kept
        bound = forward_bound(ref.cond, ref.C_ref, c.data)
        unit = 1e-15 * ref.cond ** 2 * np.abs(ref.C_ref).max()
        if dropped.any():
            out["dropped_columns"] = (np.abs(C[dropped]).max(), DROPPED_BOUND * scale)
        dc = np.abs(C - ref.C_ref)[ref.kept].max()
        df = np.abs(c.X @ C - c.X @ ref.C_ref).max()
        out["kept_columns"] = (dc, bound)
        out["fitted_values"] = (df, bound)
        row += " dropped %2d cond2 %.2e  eta %.1e  ctrl ratio %.2e  fit ratio %.2e" % (dropped.sum(), ref.cond, eta, dc / unit, df / unit)
    if verbose:
        print(row)
    return out


def failed(result):
    return sorted(k for k, (v, bound) in result.items() if not v <= bound)
