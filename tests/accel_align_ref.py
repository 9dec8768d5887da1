"""Accelerometer alignment in numpy: the reference of calico_accel_align, written from the header's description and
imu_align_ref.py's kinematics and fixture, with analytic Jacobians.

The model is the optimiser's accelerometer term with the trajectory held and scale 1 (test_accel_align_host.py pins cost and
gradient over all 13 columns on the oracle's evaluate):
  t = stamp - latency, phi = -pose[0:3](t), omega = J(phi) phi', alpha = Sum_i (H_i phi') phi'_i + J phi'' (ExpSO3Hessian's closed form),
  inner = R(phi) (pose''[3:6](t) - g) + omega x (omega x t_ra) - alpha x t_ra, prediction = R_a^T inner + bias,
  r = (measured - prediction) / sigma,
parameters (rotation 3: R_a <- exp([d]x) R_a, lever arm 3, bias 3, gravity 3, latency 1). The latency column differentiates that
expression as it stands: omega and alpha carry their derivative along t through the Rodrigues coefficients as dual numbers
(_Dual), with pose''' behind phi''; d/dt R(phi) v = omega x R(phi) v + R(phi) v'.

Measured by test_accel_align_host.py (its docstring has the figures): FLOOR, the largest criterion over six undamped Gauss-Newton
steps at and after the reference's own result on the noisy standard fixture with the lever arm LEVER, and REF_FREE, its distance
to the truth on noise-free data. Both are rounding: the tests hold re-measured values to twice these."""
import numpy as np

import imu_align_ref as ir
from calico_amd import synthetic as syn

OK, TOO_FEW_SAMPLES, NO_PEAK, DEGENERATE, NOT_CONVERGED, NOT_POSITIVE_DEFINITE = 0, 1, 2, 3, 4, 5
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = ir.LAMBDA0, ir.LAMBDA_MIN, ir.LAMBDA_MAX
COST_SLACK = ir.COST_SLACK
EPS = 2.220446049250313e-16
NP = 13
GROUPS = dict(rotation=slice(0, 3), lever_arm=slice(3, 6), bias=slice(6, 9), gravity=slice(9, 12), latency=slice(12, 13))

LEVER = (0.05, -0.08, 0.03)
# 2026-10-20, fixture(1e-3, lever=LEVER) (accelerometer noise 1e-2 m/s^2, 680 samples, order 6) and fixture(0.0, lever=LEVER)
FLOOR = 3.3e-15          # criterion of the reference at its own result
REF_FREE = 6.0e-15       # distance_to_truth of the reference on noise-free data


def fixture(noise=0.0, lever=LEVER, **kw):
    """imu_align_ref.fixture with a lever arm: (spline, stamps, accel, truth); truth has q, t_rig_accel, accel_bias, gravity, latency."""
    spl, _, _, as_, a, truth = ir.fixture(noise, lever=lever, **kw)
    return spl, as_, a, truth


def truth_estimate(truth):
    return (truth["q"], truth["t_rig_accel"], truth["accel_bias"], truth["gravity"], truth["latency"])


def imu_start(truth, angle=np.deg2rad(1.5), dlat=0.002):
    """What utils.InitializeImu leaves: the gyroscope's rotation (off by `angle`) and latency (off by dlat)."""
    q = syn.quat_mul(syn.quat_from_axis_angle(angle * np.array([0.6, -0.48, 0.64])), truth["q"])
    return q / np.linalg.norm(q), truth["latency"] + dlat


# ---- dual numbers along t ------------------------------------------------------------------------------------------------------------
class _Dual:
    def __init__(self, v, d):
        self.v, self.d = v, d

    @staticmethod
    def of(x):
        return x if isinstance(x, _Dual) else _Dual(x, 0.0)

    def __add__(self, o):
        o = _Dual.of(o)
        return _Dual(self.v + o.v, self.d + o.d)
    __radd__ = __add__

    def __sub__(self, o):
        o = _Dual.of(o)
        return _Dual(self.v - o.v, self.d - o.d)

    def __rsub__(self, o):
        return _Dual.of(o) - self

    def __neg__(self):
        return _Dual(-self.v, -self.d)

    def __mul__(self, o):
        o = _Dual.of(o)
        return _Dual(self.v * o.v, self.v * o.d + self.d * o.v)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _Dual.of(o)
        return _Dual(self.v / o.v, (self.d - self.v / o.v * o.d) / o.v)

    def __rtruediv__(self, o):
        return _Dual.of(o) / self


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _rates_dual(phi, f, ff):
    """omega = J(phi) f and alpha = Sum_i (H_i f) f_i + J ff in the unit-axis form of geometry.h (device_math.hpp's rodrigues,
    rod_J_apply, rod_H_apply), phi, f, ff lists of three _Dual."""
    t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]
    th = _Dual(np.sqrt(t2.v), 0.5 * t2.d / np.sqrt(t2.v))
    st, ct = _Dual(np.sin(th.v), th.d * np.cos(th.v)), _Dual(np.cos(th.v), -th.d * np.sin(th.v))
    it = 1.0 / th
    h = [it * p for p in phi]
    a, b = it * (1.0 - ct), it * (th - st)
    c0, c1, c2, c3 = ct - st * it, (1.0 - ct) * it * it, 3.0 * it * it * st - it * (ct - 2.0), it * it * (th - st)

    def J(v):
        kv = _cross(h, v)
        k2v = _cross(h, kv)
        return [v[i] + a * kv[i] + b * k2v[i] for i in range(3)]

    omega = J(f)
    alpha = J(ff)
    kv = _cross(h, f)
    k2v = _cross(h, kv)
    for i in range(3):
        e = [1.0 if j == i else 0.0 for j in range(3)]
        gv, gkv = _cross(e, f), _cross(e, kv)
        kgv = _cross(h, gv)
        Hi = [c0 * h[i] * kv[j] + c1 * gv[j] + c2 * h[i] * k2v[j] + c3 * (gkv[j] + kgv[j]) for j in range(3)]
        alpha = [alpha[j] + Hi[j] * f[i] for j in range(3)]
    return omega, alpha


def kinematics(spl, stamps, latency):
    """phi, omega, alpha, their derivatives along t, the world acceleration and the jerk of samples stamped `stamps` at `latency`, in
    the stamp's segment (imu_align_ref.kinematics' rule)."""
    knots, basis, ctrl, order = spl
    stamps = np.asarray(stamps, float)
    seg = syn.spline_index(knots, order, stamps)
    p = [syn.spline_eval(knots, basis, ctrl, order, stamps - latency, d, seg) for d in range(4)]
    dual = lambda d: [_Dual(-p[d][:, i], -p[d + 1][:, i]) for i in range(3)]      # noqa: E731
    omega, alpha = _rates_dual(dual(0), dual(1), dual(2))
    stack = lambda x, part: np.stack([getattr(c, part) for c in x], 1)      # noqa: E731
    return dict(phi=-p[0][:, :3], omega=stack(omega, "v"), omega_d=stack(omega, "d"), alpha=stack(alpha, "v"), alpha_d=stack(alpha, "d"),
                acc=p[2][:, 3:], jerk=p[3][:, 3:])


def system(spl, stamps, meas, est, sigma=1.0):
    """Residuals (n, 3), Jacobian (n, 3, 13) and predictions (n, 3) at est = (q, t_ra, bias, gravity, latency)."""
    q, t, b, g, tau = est
    t, b, g = (np.asarray(x, float) for x in (t, b, g))
    k = kinematics(spl, stamps, tau)
    om, al = k["omega"], k["alpha"]
    q_rw = syn.quat_from_axis_angle(k["phi"])
    rv = syn.quat_rotate(q_rw, k["acc"] - g)
    inner = rv + np.cross(om, np.cross(om, t)) - np.cross(al, t)
    inner_d = (np.cross(om, rv) + syn.quat_rotate(q_rw, k["jerk"]) + np.cross(k["omega_d"], np.cross(om, t))
               + np.cross(om, np.cross(k["omega_d"], t)) - np.cross(k["alpha_d"], t))
    pred = ir.rot_t(q, inner) + b
    r = (meas - pred) / sigma
    J = np.zeros((len(stamps), 3, NP))
    for j, e in enumerate(np.eye(3)):
        eb = np.broadcast_to(e, om.shape)
        J[:, :, j] = -ir.rot_t(q, np.cross(inner, eb)) / sigma
        J[:, :, 3 + j] = -ir.rot_t(q, np.cross(om, np.cross(om, eb)) - np.cross(al, eb)) / sigma
        J[:, j, 6 + j] = -1.0 / sigma
        J[:, :, 9 + j] = ir.rot_t(q, syn.quat_rotate(q_rw, eb)) / sigma
    J[:, :, 12] = ir.rot_t(q, inner_d) / sigma
    return r, J, pred


def cost(spl, stamps, meas, est, sigma=1.0):
    r = system(spl, stamps, meas, est, sigma)[0]
    return 0.5 * float(np.sum(r * r))


def apply(est, d):
    q, t, b, g, tau = est
    qn = syn.quat_mul(syn.quat_from_axis_angle(d[:3]), q)
    qn = qn / np.linalg.norm(qn)
    return (qn if qn[3] >= 0 else -qn, t + d[3:6], b + d[6:9], g + d[9:12], tau + d[12])


def step_size(est, d):
    _, t, b, g, tau = est
    scaled = lambda dv, v: np.abs(dv).max() / max(1.0, np.abs(v).max())      # noqa: E731
    return max(np.abs(d[:3]).max(), scaled(d[3:6], t), scaled(d[6:9], b), scaled(d[9:12], g), abs(d[12]) / max(1.0, abs(tau)))


def free_mask(**held):
    """13 booleans; free_mask(rotation=0, latency=0) holds those groups."""
    free = np.ones(NP, bool)
    for name, on in held.items():
        free[GROUPS[name]] = bool(on)
    return free


def gn(spl, stamps, meas, est, free=np.ones(NP, bool), sigma=1.0):
    """The undamped Gauss-Newton step (least squares on J itself, not on the normal equations) and its scaled size."""
    r, J, _ = system(spl, stamps, meas, est, sigma)
    free = np.asarray(free, bool)
    d = np.zeros(NP)
    d[free] = np.linalg.lstsq(J.reshape(-1, NP)[:, free], -r.ravel(), rcond=None)[0]
    return d, step_size(est, d)


def criterion(spl, stamps, meas, est, free=np.ones(NP, bool), sigma=1.0):
    """The scaled size of one undamped Gauss-Newton step at est: zero at a minimum of the accelerometer cost."""
    return gn(spl, stamps, meas, est, free, sigma)[1]


def jacobian(spl, stamps, meas, est, free=np.ones(NP, bool), sigma=1.0):
    return system(spl, stamps, meas, est, sigma)[1].reshape(-1, NP)[:, np.asarray(free, bool)]


def cond(spl, stamps, meas, est, free=np.ones(NP, bool), sigma=1.0):
    """cond(J) of the free columns at est."""
    return float(np.linalg.cond(jacobian(spl, stamps, meas, est, free, sigma)))


def covariance(spl, stamps, meas, est, free=np.ones(NP, bool), sigma=1.0):
    free = np.asarray(free, bool)
    Jf = jacobian(spl, stamps, meas, est, free, sigma)
    cov = np.zeros((NP, NP))
    Rinv = np.linalg.inv(np.linalg.qr(Jf, mode="r"))      # (J = Q R: (J^T J)^-1 = R^-1 R^-T, without squaring the condition number)
    cov[np.ix_(free, free)] = Rinv @ Rinv.T
    return cov


def vector(est):
    """The estimate as 14 numbers (q 4, lever arm, bias, gravity, latency) for comparisons."""
    q, t, b, g, tau = est
    return np.concatenate([q, t, b, g, [tau]])


def difference(a, b):
    """The 13 parameter differences between two estimates: the rotation vector of q_a q_b^-1, then plain differences."""
    dq = syn.quat_mul(a[0], syn.quat_conj(b[0]))
    dq = dq if dq[3] >= 0 else -dq
    return np.concatenate([syn.quat_to_axis_angle(dq), a[1] - b[1], a[2] - b[2], a[3] - b[3], [a[4] - b[4]]])


def distance_to_truth(est, truth):
    """max over (angle rad, lever arm m, bias m/s^2, gravity m/s^2, latency s)."""
    return float(np.abs(difference(est, truth_estimate(truth))).max())


# ---- the stages --------------------------------------------------------------------------------------------------------------------
def sample_range(spl, stamps, latency):
    return ir.sample_range(spl, np.asarray(stamps, float), latency, latency)


def linear(spl, stamps, meas, q, latency, sigma=1.0):
    """Stage L by lstsq: (lever arm, bias, gravity, rms, status) at the given rotation and latency."""
    zero = (q, np.zeros(3), np.zeros(3), np.zeros(3), latency)
    r, J, _ = system(spl, stamps, meas, zero, sigma)
    if not np.all(np.isfinite(r)):
        return np.zeros(3), np.zeros(3), np.zeros(3), 0.0, DEGENERATE
    A = J.reshape(-1, NP)[:, 3:12]
    x, _, rank, _ = np.linalg.lstsq(A, -r.ravel(), rcond=None)
    if rank < 9:
        return np.zeros(3), np.zeros(3), np.zeros(3), 0.0, NOT_POSITIVE_DEFINITE
    res = (r.ravel() + A @ x) * sigma
    return x[0:3], x[3:6], x[6:9], float(np.sqrt(res @ res / len(res))), OK


def refine(spl, stamps, meas, est, free=np.ones(NP, bool), max_iterations=50, step_tolerance=1e-10, sigma=1.0):
    """The loop with the library's rules (imu_align_ref.refine's, 13 parameters). Returns (est, status, iterations, costs)."""
    free = np.asarray(free, bool)

    def evaluate(e):
        if not all(np.all(np.isfinite(x)) for x in e):
            return None
        r, J, pred = system(spl, stamps, meas, e, sigma)
        if not np.all(np.isfinite(r)):
            return None
        noise = float(np.sum(np.abs(r) * (np.abs(meas) + np.abs(pred)))) / sigma
        Jf = J.reshape(-1, NP)
        return 0.5 * float(np.sum(r * r)), Jf.T @ Jf, Jf.T @ r.ravel(), noise

    cur = evaluate(est)
    if cur is None:
        return est, DEGENERATE, 0, (0.0, 0.0)
    initial = cur[0]
    lam, iterations = LAMBDA0, 0
    while True:
        if iterations >= max_iterations:
            return est, NOT_CONVERGED, iterations, (initial, cur[0])
        iterations += 1
        c, H, g, noise = cur
        while True:
            Hm, gm = H.copy(), g.copy()
            Hm[~free, :] = 0.0
            Hm[:, ~free] = 0.0
            Hm[~free, ~free] = 1.0
            gm[~free] = 0.0
            Hm[np.diag_indices(NP)] *= 1.0 + lam
            try:
                if not np.all(np.diag(Hm) > 0):
                    raise np.linalg.LinAlgError
                L = np.linalg.cholesky(Hm)
                break
            except np.linalg.LinAlgError:
                if lam >= LAMBDA_MAX:
                    return est, NOT_POSITIVE_DEFINITE, iterations, (initial, cur[0])
                lam = min(lam * 10.0, LAMBDA_MAX)
        d = -np.linalg.solve(L.T, np.linalg.solve(L, gm))
        s = step_size(est, d)
        cand_est = apply(est, d)
        cand = evaluate(cand_est)
        small, gauss_newton = s < step_tolerance, lam <= LAMBDA0
        if cand is not None and cand[0] <= c + COST_SLACK * noise:
            est, cur = cand_est, cand
            lam = max(lam * 0.1, LAMBDA_MIN)
            if small and gauss_newton:
                return est, OK, iterations, (initial, cur[0])
        else:
            if small and cand is not None and gauss_newton:
                return est, OK, iterations, (initial, cur[0])
            lam = min(lam * 10.0, LAMBDA_MAX)


def align(spl, stamps, accel, q_init, latency_init, t_init=None, bias_init=None, gravity_init=None, max_iterations=50,
          step_tolerance=1e-10, estimate_rotation=1, estimate_lever_arm=1, estimate_bias=1, estimate_gravity=1, estimate_latency=1,
          min_samples=16, sigma_accel=1.0):
    """calico_accel_align, stage by stage. Returns a dict with the device wrapper's keys."""
    stamps, accel = np.asarray(stamps, float), np.asarray(accel, float).reshape(-1, 3)
    q0 = np.asarray(q_init, float) / np.linalg.norm(q_init)
    q0 = q0 if q0[3] >= 0 else -q0
    lat0 = float(latency_init)
    given = t_init is not None
    start = (q0, np.asarray(t_init, float) if given else np.zeros(3), np.asarray(bias_init, float) if given else np.zeros(3),
             np.asarray(gravity_init, float) if given else np.zeros(3), lat0)
    first, end = sample_range(spl, stamps, lat0) if len(stamps) else (0, 0)
    out = dict(status=TOO_FEW_SAMPLES, linear_status=-1, samples=end - first, first_sample=first, iterations=0, rms=0.0, linear_rms=0.0,
               initial_cost=0.0, final_cost=0.0, cov=np.zeros((NP, NP)))

    def give(est):
        out.update(q_rig_accel=est[0], t_rig_accel=est[1], bias=est[2], gravity_world=est[3], latency=est[4],
                   gravity_norm=float(np.linalg.norm(est[3])))
        return out
    if end - first < min_samples:
        return give(start)
    s, m = stamps[first:end], accel[first:end]
    free = free_mask(rotation=estimate_rotation, lever_arm=estimate_lever_arm, bias=estimate_bias, gravity=estimate_gravity,
                     latency=estimate_latency)
    est = start
    if not given:
        t, b, g, rms, status = linear(spl, s, m, q0, lat0, sigma_accel)
        out.update(linear_status=status, linear_rms=rms)
        if status != OK:
            out["status"] = status
            return give(start)
        est = (q0, t, b, g, lat0)
    est, status, iterations, costs = refine(spl, s, m, est, free, max_iterations, step_tolerance, sigma_accel)
    out.update(status=status, iterations=iterations, initial_cost=costs[0], final_cost=costs[1])
    if status == DEGENERATE:
        return give(start)
    if status in (OK, NOT_CONVERGED):
        r = system(spl, s, m, est, sigma_accel)[0]
        out.update(cov=covariance(spl, s, m, est, free, sigma_accel), rms=float(np.sqrt(np.sum(r * r) / r.size)) * sigma_accel)
    return give(est)


def estimate(result):
    return result["q_rig_accel"], result["t_rig_accel"], result["bias"], result["gravity_world"], result["latency"]


# ---- the optimiser's own term (the oracle, or the device's calico_evaluate) -------------------------------------------------------------
def accel_problem(api, spl, stamps, accel, est, sigma=1.0, ctrl_constant=True):
    """A problem with one accelerometer (ScaleAndBias, intrinsics [1, bias]) holding `est` with FREE q, t, intrinsics, gravity and
    latency, the control points constant (imu_align_ref.accel_problem's pattern; ctrl_constant=False for the device's
    calico_evaluate, which does not take constant control points: their columns come first and are skipped). Returns (problem, columns): columns[i] is the
    tangent index of parameter i of (rotation 3, lever arm 3, bias 3, gravity 3, latency 1) in calico_evaluate's gradient. The
    quaternion's tangent is Ceres': its columns are twice the derivative in the rotation vector."""
    from calico_amd import _capi
    knots, basis, ctrl, order = spl
    q, t, b, g, tau = est
    P = _capi.Problem(api, 0)
    grav = P.add_param_block(np.asarray(g, float), constant=False)
    cb = P.add_param_blocks(np.asarray(ctrl, float), constant=ctrl_constant)
    P.set_spline(order, knots, basis, cb)
    bi = P.add_param_block(np.concatenate([[1.0], b]), constant=False)
    bt = P.add_param_block(np.asarray(t, float), constant=False)
    bq = P.add_param_block(np.asarray(q, float), _capi.MANIFOLD_EIGEN_QUATERNION, False)
    bl = P.add_param_block([float(tau)], constant=False)
    sid = P.add_sensor(_capi.SENSOR_ACCELEROMETER, 2, bi, bq, bt, bl, grav, sigma, 0, 1.0)
    P.add_imu_residuals(sid, np.asarray(accel, float), np.asarray(stamps, float))
    # the control points' columns come first; then the blocks in order: gravity 0-2, intrinsics [scale 3, bias 4-6], t 7-9, q 10-12, latency 13
    return P, P.num_effective_parameters() - 14 + np.array([10, 11, 12, 7, 8, 9, 4, 5, 6, 0, 1, 2, 13])


ROTATION_TANGENT = np.array([2.0, 2, 2] + [1.0] * 10)
