"""Reference of calico_imu_allan in numpy long double: the overlapping Allan variance as the header writes it (a sequential
cumsum for theta, one vectorised second difference per cluster size), the same grid of cluster sizes, and the same exhaustive
non-negative least squares of the IEEE-952 coefficients (every subset of the enabled terms by Householder QR of the
column-normalised design). Every function takes the dtype: float64 restates both, and is used only to size the tests' bounds."""
import numpy as np

LD = np.longdouble
SCAN_BLOCK = 2048       # kAllanScanBlock (calico_amd/csrc/kernels.hpp)
TERM_CHUNK = 4096       # kAllanTermChunk
MAX_CLUSTERS = 256      # CALICO_ALLAN_MAX_CLUSTERS
TERM_Q, TERM_N, TERM_B, TERM_K, TERM_R = 1, 2, 4, 8, 16
DEFAULT_TERMS = TERM_N | TERM_B | TERM_K
TIE_EPS = 64 * 2.0 ** -52     # kAllanTieEps (calico_amd/csrc/allan_fit.hpp)
OK, NO_WHITE_NOISE, TOO_FEW_POINTS, NONFINITE = 0, 1, 2, 3
NAMES = ("Q", "N", "B", "K", "R")


def grid(n, points_per_decade=10, max_tau_fraction=0.1):
    """The distinct floor(10^(i / ppd) + 1/2), i = 0, 1, ..., with m <= max_tau_fraction n and 2 m < n."""
    out = []
    i = 0
    while len(out) < MAX_CLUSTERS:
        v = np.floor(10.0 ** (i / float(points_per_decade)) + 0.5)
        if not v <= max_tau_fraction * float(n) or not 2.0 * v < float(n):
            break
        if not out or int(v) > out[-1]:
            out.append(int(v))
        i += 1
    return out


def time_step(rate):
    """dt as the library forms it (a double), so that tau = m dt is the same number in every precision."""
    return np.float64(1.0) / np.float64(rate)


def weights(n, ms):
    """w_i = 2 (n / m_i - 1) = rel_err^-2."""
    return np.array([2.0 * (float(n) / float(m) - 1.0) for m in ms])


def avar(y, rate, ms, dtype=LD):
    """One axis: avar(m) = Sum_{k < n - 2m} (theta_{k+2m} - 2 theta_{k+m} + theta_k)^2 / (2 tau^2 (n - 2m)), theta_0 = 0,
    theta_k = dt Sum_{i<k} (y_i - mean)."""
    y = np.asarray(y, dtype=dtype)
    n = len(y)
    dt = dtype(time_step(rate))
    theta = np.concatenate((np.zeros(1, dtype), dt * np.cumsum(y - y.mean(), dtype=dtype)))
    out = np.zeros(len(ms), dtype)
    for j, m in enumerate(ms):
        terms = n - 2 * m
        d = theta[2 * m:2 * m + terms] - dtype(2) * theta[m:m + terms] + theta[:terms]
        tau = dtype(m) * dt
        out[j] = (d * d).sum(dtype=dtype) / (dtype(2) * tau * tau * dtype(terms))
    return out


def term_shapes(tau, dtype=LD):
    """phi_t(tau_i), (5, p): the variance a unit squared coefficient of Q, N, B, K, R contributes."""
    tau = np.asarray(tau, dtype=dtype)
    const = dtype(2) * np.log(dtype(2)) / (dtype(4) * np.arctan(dtype(1)))
    return np.stack([dtype(3) / (tau * tau), dtype(1) / tau, const * np.ones_like(tau), tau / dtype(3), tau * tau / dtype(2)])


def _householder_solve(A, b):
    """min |A z - b| by Householder QR; None where a column of the triangle vanishes."""
    A, b = A.copy(), b.copy()
    rows, cols = A.shape
    diag = np.zeros(cols, A.dtype)
    for j in range(cols):
        x = A[j:, j]
        norm = np.sqrt((x * x).sum())
        if not np.isfinite(norm) or not norm > 0:
            return None
        alpha = -norm if x[0] > 0 else norm
        v = x.copy()
        v[0] -= alpha
        vtv = (v * v).sum()
        if not vtv > 0:
            return None
        A[j:, j + 1:] -= np.outer(v, (2 * (v @ A[j:, j + 1:]) / vtv))
        b[j:] -= v * (2 * (v @ b[j:]) / vtv)
        diag[j] = alpha
    z = np.zeros(cols, A.dtype)
    for j in range(cols - 1, -1, -1):
        z[j] = (b[j] - (A[j, j + 1:] * z[j + 1:]).sum()) / diag[j]
    return z if np.all(np.isfinite(z)) else None


def fit(tau, weight, variances, terms=DEFAULT_TERMS, dtype=LD):
    """The coefficients of one axis. Returns dict(a: the five squared coefficients, coefficients: their roots by name, mask,
    objective, n_points, status, shapes_over_avar: max_i phi_t(tau_i) / avar_i per term over the points used)."""
    v = np.asarray(variances, dtype=dtype)
    use = np.isfinite(v) & (v > 0) & (np.asarray(weight) > 0)
    enabled = [t for t in range(5) if terms >> t & 1]
    out = dict(a=np.zeros(5, dtype), mask=0, objective=dtype(0), n_points=int(use.sum()), status=TOO_FEW_POINTS,
               shapes_over_avar=np.zeros(5, dtype))
    out["coefficients"] = dict.fromkeys(NAMES, 0.0)
    if not enabled or use.sum() < len(enabled):
        return out
    G = term_shapes(np.asarray(tau)[use], dtype) / v[use]
    sw = np.sqrt(np.asarray(weight, dtype=dtype)[use])
    out["shapes_over_avar"] = G.max(axis=1)
    tie = (sw * sw).sum() * dtype(TIE_EPS) ** 2      # objectives closer than the residuals' rounding are tied (in every dtype)
    best = None
    masks = sorted((m for m in range(1, 32) if m & ~terms == 0), key=lambda m: (bin(m).count("1"), m))
    for mask in masks:
        which = [t for t in range(5) if mask >> t & 1]
        A = (G[which] * sw).T
        scale = np.sqrt((A * A).sum(axis=0))
        if not np.all(np.isfinite(scale)) or not np.all(scale > 0):
            continue
        z = _householder_solve(A / scale, sw)
        if z is None:
            continue
        a = z / scale
        if not np.all(a >= 0):
            continue
        r = sw * (dtype(1) - a @ G[which])
        objective = (r * r).sum()
        if np.isfinite(objective) and (best is None or objective < best[0] - tie):
            best = (objective, mask, which, a)
    if best is None:
        return out
    out["objective"], out["mask"] = best[0], best[1]
    out["a"][best[2]] = best[3]
    out["coefficients"] = {name: float(np.sqrt(out["a"][t])) for t, name in enumerate(NAMES)}
    out["status"] = OK if out["a"][1] > 0 else NO_WHITE_NOISE
    return out


def synthetic_log(seed, n=2 ** 18, rate=200.0, N0=1e-3, K0=2e-4):
    """(n, 3) samples at `rate`: white noise of density N0 plus a rate random walk of K0 on every axis."""
    rng = np.random.default_rng(seed)
    white = N0 * np.sqrt(rate) * rng.standard_normal((n, 3))
    walk = np.cumsum(K0 / np.sqrt(rate) * rng.standard_normal((n, 3)), axis=0)
    return white + walk


def relative_error(value, exact):
    """|value - exact| / |exact| element-wise in long double (0 where both are 0)."""
    value, exact = np.asarray(value, dtype=LD), np.asarray(exact, dtype=LD)
    return np.where(exact == 0, np.abs(value), np.abs(value - exact) / np.where(exact == 0, 1, np.abs(exact))).astype(np.float64)
