"""Camera-to-trajectory alignment in numpy: the reference of calico_camera_align, written from the header's description of the
stages and synthetic.py's kinematics, dense and slow. No code under test in here.

The model is the optimiser's camera term with the trajectory held (test_camera_align_host.py pins cost and Gauss-Newton step on
the oracle's evaluate):
  t = stamp - latency (the segment is the STAMP's), p = spline(t), R_rw = R(quat(-p[0:3])), t_wr = p[3:6],
  y = R_rw (R_wm x + t_wm - t_wr), x_c = R_rc^T (y - t_rc), r = (pixel - project(k, x_c)) / sigma,
parameters (rotation 3: R_rc <- exp([d]x) R_rc, translation 3, latency 1). The point Jacobian of the projection is a central
difference of synthetic.project_point (h = 1e-6 of the point's distance); everything else is analytic.

Measured by test_camera_align_host.py (its docstring says how): FLOOR, REF_FREE and CURVE_LEVEL below."""
import functools

import numpy as np

import imu_align_ref as iref
from calico_amd import synthetic as syn

OK, TOO_FEW_SAMPLES, NO_PEAK, DEGENERATE, NOT_CONVERGED, NOT_POSITIVE_DEFINITE = 0, 1, 2, 3, 4, 5
RESECT_OK, RESECT_TOO_FEW_POINTS, FRAME_OUTSIDE = 0, 1, 6
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-4, 1e-12, 1e12
COST_SLACK = 8.0 * 2.220446049250313e-16
FLAT = 1e-12

FLOOR = 5.1e-15          # criterion (rad, m, s) of the reference at and after its own result, pixel noise 0.1
REF_FREE = 9.4e-16       # distance_to_truth of the reference on noise-free data
CURVE_LEVEL = 5.6e-15    # |score curve over resected poses - the curve over the same frames resected from another start|_inf

TRUTH = dict(q=syn.quat_from_axis_angle(np.deg2rad(25.0) * np.array([2.0, -1.0, 2.0]) / 3.0), t=np.array([0.08, -0.05, 0.03]),
             latency=0.0137)
OPTIONS = dict(max_lag=0.05, lag_step=0.0025)
MODEL = 1      # OpenCv5
# T_world_chart: the chart lies where the true camera looks at the rig's rest pose (0, 0, 1), turned a little out of the plane
CHART_Q = syn.quat_from_axis_angle(np.deg2rad(8.0) * np.array([0.6, 0.8, 0.0]))


def rot(q):
    """R(q), q = (x, y, z, w)."""
    return np.stack([syn.quat_rotate(q, e) for e in np.eye(3)], -1)


@functools.lru_cache(maxsize=None)
def chart_t():
    """The chart's centre: where the camera's optical axis at the rig's rest pose meets the plane z = 0."""
    _, quats, trans = syn.default_synthetic_poses(segment_duration=0.3)
    q_wr, t_wr = quats[0], trans[0]
    axis = syn.quat_rotate(q_wr, syn.quat_rotate(TRUTH["q"], np.array([0.0, 0.0, 1.0])))
    centre = syn.quat_rotate(q_wr, TRUTH["t"]) + t_wr
    return centre - axis * (centre[2] / axis[2])


def intrinsics(model=MODEL):
    return np.array(syn._TRUE_INTRINSICS[model], float)


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def rig_pose(spl, stamps, latency):
    """(q_rw (n, 4), t_wr, omega, t_wr') of frames stamped `stamps` at `latency`: the STAMP's segment, evaluated at stamp - latency."""
    knots, basis, ctrl, order = spl
    stamps = np.asarray(stamps, float)
    seg = syn.spline_index(knots, order, stamps)
    p, pd = (syn.spline_eval(knots, basis, ctrl, order, stamps - latency, d, seg) for d in range(2))
    phi, f = -p[:, :3], -pd[:, :3]
    omega = np.einsum("nij,nj->ni", syn.exp_so3_jacobian(phi), f)
    return syn.quat_from_axis_angle(phi), p[:, 3:], omega, pd[:, 3:]


def project(model, k, xc):
    px, valid = syn.project_point(model, k, xc)
    return px, valid & np.isfinite(px).all(1)


def point_jacobian(model, k, xc):
    """d pixel / d x_c (n, 2, 3) by central differences."""
    D = np.zeros((len(xc), 2, 3))
    h = 1e-6 * np.maximum(1.0, np.linalg.norm(xc, axis=1))
    for j in range(3):
        d = np.zeros_like(xc)
        d[:, j] = h
        with np.errstate(all="ignore"):
            D[:, :, j] = (syn.project_point(model, k, xc + d)[0] - syn.project_point(model, k, xc - d)[0]) / (2.0 * h)[:, None]
    return D


def frame_of_pair(fx):
    return np.repeat(np.arange(len(fx["stamps"])), np.diff(fx["offsets"]))


def system(fx, est, sigma=1.0, huber=0.0, frames=None):
    """(r (N, 2), J (N, 2, 7), w (N,), e (N, 2) pixels, valid (N,), pix (N, 2)) at est = (q, t, latency) over the pairs of the
    frames that take part (frames: a mask, None = all); rows of pairs that are not valid are zero."""
    q, t, tau = est
    fi = frame_of_pair(fx)
    q_rw, t_wr, omega, tdot = rig_pose(fx["spl"], fx["stamps"], tau)
    xw = syn.quat_rotate(fx["q_wm"], fx["points"]) + fx["t_wm"]
    y = syn.quat_rotate(q_rw[fi], xw - t_wr[fi])
    z = y - t
    xc = syn.quat_rotate(syn.quat_conj(q), z)
    pix, valid = project(fx["model"], fx["k"], xc)
    if frames is not None:
        valid = valid & np.asarray(frames, bool)[fi]
    ydot = np.cross(omega[fi], y) - syn.quat_rotate(q_rw[fi], tdot[fi])
    with np.errstate(all="ignore"):
        D = point_jacobian(fx["model"], fx["k"], xc)
    dd = syn.quat_rotate(q, D)      # (N, 2, 3): R_rc D_r^T
    J = np.zeros((len(xc), 2, 7))
    J[:, :, 0:3] = np.cross(z[:, None, :], dd)
    J[:, :, 3:6] = dd
    J[:, :, 6] = np.einsum("nrc,nc->nr", dd, ydot)
    e = fx["pixels"] - pix
    e[~valid] = 0.0
    J[~valid] = 0.0
    w = np.ones(len(xc))
    if huber > 0:
        s = np.sqrt((e * e).sum(1))
        big = s > huber
        w[big] = huber / s[big]
    return e / sigma, J / sigma, w, e, valid, pix


def rho_sum(e, huber):
    sq = (e * e).sum(1)
    if huber > 0:
        big = sq > huber * huber
        return float(np.sum(np.where(big, 2.0 * huber * np.sqrt(sq) - huber * huber, sq)))
    return float(sq.sum())


def cost(fx, est, sigma=1.0, huber=0.0, frames=None):
    """1/2 Sum rho(|e|^2) / sigma^2."""
    _, _, _, e, _, _ = system(fx, est, sigma, huber, frames)
    return 0.5 * rho_sum(e, huber) / sigma ** 2


def apply(est, d):
    q, t, tau = est
    qn = syn.quat_mul(syn.quat_from_axis_angle(d[:3]), q)
    qn = qn / np.linalg.norm(qn)
    return (qn if qn[3] >= 0 else -qn, t + d[3:6], tau + d[6])


def step_size(est, d):
    _, t, tau = est
    return max(np.abs(d[:3]).max(), np.abs(d[3:6]).max() / max(1.0, np.abs(t).max()), abs(d[6]) / max(1.0, abs(tau)))


def gn(fx, est, free=np.ones(7, bool), sigma=1.0, huber=0.0, frames=None):
    """The undamped weighted Gauss-Newton step (least squares on sqrt(w) J itself) and its scaled size."""
    r, J, w, _, _, _ = system(fx, est, sigma, huber, frames)
    free = np.asarray(free, bool)
    sw = np.sqrt(w)[:, None]
    d = np.zeros(7)
    d[free] = np.linalg.lstsq((J * sw[:, :, None]).reshape(-1, 7)[:, free], -(r * sw).ravel(), rcond=None)[0]
    return d, step_size(est, d)


def criterion(fx, est, free=np.ones(7, bool), sigma=1.0, huber=0.0, frames=None):
    """The scaled size of one undamped Gauss-Newton step at est: zero at a minimum of the camera cost."""
    return gn(fx, est, free, sigma, huber, frames)[1]


def covariance(fx, est, free=np.ones(7, bool), sigma=1.0, huber=0.0, frames=None):
    _, J, w, _, _, _ = system(fx, est, sigma, huber, frames)
    free = np.asarray(free, bool)
    Jf = (J * np.sqrt(w)[:, None, None]).reshape(-1, 7)[:, free]
    cov = np.zeros((7, 7))
    cov[np.ix_(free, free)] = np.linalg.inv(Jf.T @ Jf)
    return cov


def distance_to_truth(est, truth):
    q, t, tau = est
    dq = syn.quat_mul(q, syn.quat_conj(truth["q"]))
    angle = 2.0 * np.arctan2(np.linalg.norm(dq[:3]), abs(dq[3]))
    return max(angle, np.abs(t - truth["t"]).max(), abs(tau - truth["latency"]))


def estimate(result):
    return result["q_rig_camera"], result["t_rig_camera"], result["latency"]


# ---- fixtures ----------------------------------------------------------------------------------------------------------------------
def fixture(noise=0.0, model=MODEL, rate=20.0, t0=0.3, t1=6.9, latency=None, points=None, seed=5, outliers=0.0, times=None, order=6,
            one_axis=False, at_rest=False):
    """The standard fixture: the chart seen at `rate` over true times [t0, t1), stamped t + latency, pixels under the optimiser's
    own model (the spline segment of the stamp, for the reason imu_align_ref.fixture states: a frame whose latency crosses a
    knot would otherwise differ by the two polynomials' distance, and the truth would not be the minimum of noise-free data to
    rounding). A pair the model rejects at the truth, or that no detector would return (detected()), is left out: the frames are ragged. outliers: the fraction of pairs displaced
    by 30 to 60 pixels. at_rest: every control point is the first one. Returns a dict."""
    spl = iref.trajectory(order, one_axis)
    if at_rest:
        knots, basis, ctrl, order = spl
        spl = (knots, basis, np.ascontiguousarray(np.tile(ctrl[len(ctrl) // 2], (len(ctrl), 1))), order)
    truth = dict(TRUTH)
    if latency is not None:
        truth["latency"] = latency
    pts = syn.planar_points() if points is None else np.asarray(points, float)
    times = t0 + np.arange(int(round((t1 - t0) * rate))) / rate if times is None else np.asarray(times, float)
    stamps = times + truth["latency"]
    fx = dict(spl=spl, model=model, k=intrinsics(model), q_wm=CHART_Q, t_wm=chart_t(), stamps=stamps, truth=truth,
              offsets=np.arange(len(stamps) + 1, dtype=np.int64) * len(pts), points=np.tile(pts, (len(stamps), 1)))
    fx["pixels"] = np.zeros((len(fx["points"]), 2))
    _, _, _, _, valid, pix = system(fx, (truth["q"], truth["t"], truth["latency"]))
    valid = valid & detected(fx, (truth["q"], truth["t"], truth["latency"]), pix)
    rng = np.random.default_rng(seed)
    if noise:
        pix = pix + noise * rng.standard_normal(pix.shape)
    if outliers:
        bad = rng.random(len(pix)) < outliers
        ang = rng.random(len(pix)) * 2.0 * np.pi
        pix = pix + (bad * (30.0 + 30.0 * rng.random(len(pix))))[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    fi = frame_of_pair(fx)
    fx["offsets"] = np.concatenate([[0], np.cumsum(np.bincount(fi[valid], minlength=len(stamps)))]).astype(np.int64)
    fx["pixels"], fx["points"] = np.ascontiguousarray(pix[valid]), np.ascontiguousarray(fx["points"][valid])
    return fx


IMAGE = (1280.0, 800.0)
MAX_ANGLE = np.deg2rad(50.0)


def detected(fx, est, pix):
    """What a detector can return: the pixel lies inside the image and the point within 50 degrees of the optical axis (the
    distortion polynomial of the reference tests' OpenCv5 intrinsics folds back beyond some 57 degrees: points far outside the
    field of view would land inside the image again)."""
    q, t, tau = est
    fi = frame_of_pair(fx)
    q_rw, t_wr, _, _ = rig_pose(fx["spl"], fx["stamps"], tau)
    y = syn.quat_rotate(q_rw[fi], syn.quat_rotate(fx["q_wm"], fx["points"]) + fx["t_wm"] - t_wr[fi])
    xc = syn.quat_rotate(syn.quat_conj(q), y - t)
    with np.errstate(all="ignore"):
        inside = (pix[:, 0] >= 0) & (pix[:, 0] <= IMAGE[0]) & (pix[:, 1] >= 0) & (pix[:, 1] <= IMAGE[1])
        return inside & (np.arctan2(np.linalg.norm(xc[:, :2], axis=1), xc[:, 2]) < MAX_ANGLE)


def call_args(fx):
    """The arguments of _capi.camera_align, in its order, without the options."""
    knots, basis, ctrl, order = fx["spl"]
    return (order, knots, basis, ctrl, fx["model"], fx["k"], fx["stamps"], fx["offsets"], fx["pixels"], fx["points"], fx["q_wm"], fx["t_wm"])


# ---- the stages --------------------------------------------------------------------------------------------------------------------
def lag_grid(latency0, max_lag, lag_step):
    return iref.lag_grid(latency0, max_lag, lag_step)


def frames_taking_part(fx, lat_lo, lat_hi, min_points=4):
    """Per frame the status (RESECT_OK: it takes part)."""
    lo, hi = iref.valid_range(fx["spl"])
    s = fx["stamps"]
    inside = (s >= lo) & (s <= hi) & (s - lat_hi >= lo) & (s - lat_lo <= hi)
    n = np.diff(fx["offsets"])
    return np.where(n < min_points, RESECT_TOO_FEW_POINTS, np.where(inside, RESECT_OK, FRAME_OUTSIDE)).astype(np.uint8)


def true_camera_pose(fx, f):
    """T_camera_chart (q, t) of frame f at the truth."""
    tr = fx["truth"]
    q_rw, t_wr, _, _ = rig_pose(fx["spl"], fx["stamps"][f:f + 1], tr["latency"])
    q = syn.quat_mul(syn.quat_conj(tr["q"]), syn.quat_mul(q_rw[0], fx["q_wm"]))
    t = syn.quat_rotate(syn.quat_conj(tr["q"]), syn.quat_rotate(q_rw[0], fx["t_wm"] - t_wr[0]) - tr["t"])
    return q / np.linalg.norm(q), t


def resect_frame(fx, f, start, huber=0.0, max_steps=20):
    """Gauss-Newton on T_camera_chart of frame f from `start` (q, t), R <- exp([d]x) R, until the step stops shrinking. Returns
    (q, t, ok)."""
    q, t = np.asarray(start[0], float), np.asarray(start[1], float)
    a, b = fx["offsets"][f], fx["offsets"][f + 1]
    P, px = fx["points"][a:b], fx["pixels"][a:b]
    last = np.inf
    for it in range(max_steps):
        Rp = syn.quat_rotate(q, P)
        xc = Rp + t
        pix, valid = project(fx["model"], fx["k"], xc)
        if valid.sum() < 4:
            return q, t, False
        D = point_jacobian(fx["model"], fx["k"], xc)
        J = np.concatenate([-np.einsum("nrc,ncj->nrj", D, syn.skew(Rp)), D], 2)[valid]
        e = (pix - px)[valid]
        w = np.ones(len(e))
        if huber > 0:
            s = np.sqrt((e * e).sum(1))
            w[s > huber] = huber / s[s > huber]
        sw = np.sqrt(w)[:, None]
        d = np.linalg.lstsq((J * sw[:, :, None]).reshape(-1, 6), -(e * sw).ravel(), rcond=None)[0]
        n = np.abs(d).max()
        if it > 0 and (n >= last or n < 1e-15):
            break
        qn = syn.quat_mul(syn.quat_from_axis_angle(d[:3]), q)
        q, t, last = qn / np.linalg.norm(qn), t + d[3:], n
    return q, t, bool(np.isfinite(last) and last < 1e-6)


def resect(fx, status, huber=0.0, start_offset=None):
    """Stage R: T_camera_chart of every frame that takes part, from the true pose (start_offset: a 6-vector added to that start,
    for the measurement of CURVE_LEVEL). Returns (q (F, 4), t (F, 3), status)."""
    F = len(fx["stamps"])
    q, t, status = np.tile([0.0, 0, 0, 1], (F, 1)), np.zeros((F, 3)), status.copy()
    for f in np.nonzero(status == RESECT_OK)[0]:
        q0, t0 = true_camera_pose(fx, f)
        if start_offset is not None:
            q0 = syn.quat_mul(syn.quat_from_axis_angle(start_offset[:3]), q0)
            t0 = t0 + start_offset[3:]
        q[f], t[f], ok = resect_frame(fx, f, (q0, t0), huber)
        if not ok:
            status[f] = 4      # RESECT_DEGENERATE
    return q, t, status


def pose_samples(fx, poses, use, latency):
    """E_i(latency) = T_rig_world(stamp_i - latency) T_world_chart T_chart_camera_i of the frames `use`: (q (n, 4), t (n, 3))."""
    q_cm, t_cm = poses[0][use], poses[1][use]
    q_rw, t_wr, _, _ = rig_pose(fx["spl"], fx["stamps"][use], latency)
    q_wc = syn.quat_mul(np.broadcast_to(fx["q_wm"], q_cm.shape), syn.quat_conj(q_cm))
    c_w = syn.quat_rotate(fx["q_wm"], -syn.quat_rotate(syn.quat_conj(q_cm), t_cm)) + fx["t_wm"]
    q = syn.quat_mul(q_rw, q_wc)
    return q / np.linalg.norm(q, axis=1)[:, None], syn.quat_rotate(q_rw, c_w - t_wr)


def score(fx, poses, use, latency):
    q, t = pose_samples(fx, poses, use, latency)
    n = len(q)
    d2 = float(np.mean(np.sum(poses[1][use] ** 2, 1)))
    top = np.linalg.eigvalsh(q.T @ q)[-1]
    return 4.0 * (1.0 - top / n) + (np.sum(t * t) / n - np.sum(t.mean(0) ** 2)) / d2


def search(fx, poses, use, lags):
    """Stage A: the curve, the minimum's index, the coarse latency, the status."""
    curve = np.array([score(fx, poses, use, lag) for lag in lags])
    peak = int(np.argmin(curve))
    flat = not np.all(np.isfinite(curve)) or not (curve.max() - curve.min() > FLAT * max(curve.max(), 1.0))
    if flat or peak == 0 or peak == len(lags) - 1:
        return curve, peak, lags[peak], NO_PEAK
    ym, y0, yp = curve[peak - 1], curve[peak], curve[peak + 1]
    den = ym - 2.0 * y0 + yp
    off = 0.5 * (ym - yp) / den if den > 0 else 0.0
    return curve, peak, lags[peak] + off * (lags[1] - lags[0]), OK


def mean_pose(fx, poses, use, latency):
    """Stage B: the principal eigenvector of Sum q q^T (w >= 0) and the mean translation."""
    q, t = pose_samples(fx, poses, use, latency)
    v = np.linalg.eigh(q.T @ q)[1][:, -1]
    v = v / np.linalg.norm(v)
    return (v if v[3] >= 0 else -v), t.mean(0)


def refine(fx, est, free=np.ones(7, bool), max_iterations=50, step_tolerance=1e-10, sigma=1.0, huber=0.0, frames=None):
    """Stage C with the library's rules. Returns (est, status, iterations)."""
    free = np.asarray(free, bool)

    def evaluate(e_):
        if not all(np.all(np.isfinite(x)) for x in e_):
            return None
        r, J, w, e, valid, pix = system(fx, e_, sigma, huber, frames)
        Jw = (J * np.sqrt(w)[:, None, None]).reshape(-1, 7)
        rw = (r * np.sqrt(w)[:, None]).ravel()
        noise = float(np.sum(np.abs(e * pix)[valid])) / sigma ** 2
        return dict(e=e, valid=valid, H=Jw.T @ Jw, g=Jw.T @ rw, noise=noise, cost=rho_sum(e, huber) / sigma ** 2)

    cur = evaluate(est)
    if cur is None or not cur["valid"].any() or not np.isfinite(cur["cost"]):
        return est, DEGENERATE, 0
    lam, iterations = LAMBDA0, 0
    while True:
        if iterations >= max_iterations:
            return est, NOT_CONVERGED, iterations
        iterations += 1
        while True:
            Hm, gm = cur["H"].copy(), cur["g"].copy()
            Hm[~free, :] = 0.0
            Hm[:, ~free] = 0.0
            Hm[~free, ~free] = 1.0
            gm[~free] = 0.0
            Hm[np.diag_indices(7)] *= 1.0 + lam
            try:
                L = np.linalg.cholesky(Hm)
                break
            except np.linalg.LinAlgError:
                if lam >= LAMBDA_MAX:
                    return est, NOT_POSITIVE_DEFINITE, iterations
                lam = min(lam * 10.0, LAMBDA_MAX)
        d = -np.linalg.solve(L.T, np.linalg.solve(L, gm))
        s = step_size(est, d)
        cand_est = apply(est, d)
        cand = evaluate(cand_est)
        kept = cand is not None and np.isfinite(cand["cost"]) and not np.any(cur["valid"] & ~cand["valid"])
        small, gauss_newton = s < step_tolerance, lam <= LAMBDA0
        if kept and rho_sum(cand["e"][cur["valid"]], huber) / sigma ** 2 <= cur["cost"] + COST_SLACK * cur["noise"]:
            est, cur = cand_est, cand
            lam = max(lam * 0.1, LAMBDA_MIN)
            if small and gauss_newton:
                return est, OK, iterations
        else:
            if small and kept and gauss_newton:
                return est, OK, iterations
            lam = min(lam * 10.0, LAMBDA_MAX)


def align(fx, q_init=None, t_init=None, latency_init=None, max_lag=0.1, lag_step=1e-3, max_iterations=50, step_tolerance=1e-10,
          estimate_latency=1, estimate_translation=1, huber_scale=0.0, min_points=4, min_frames=8, sigma_pixel=1.0):
    """calico_camera_align, stage by stage. Returns a dict with the device wrapper's keys (and `frames`: who took part)."""
    given = q_init is not None
    lat0 = float(latency_init) if given else 0.0
    q0 = np.asarray(q_init, float) / np.linalg.norm(q_init) if given else np.array([0.0, 0, 0, 1])
    q0 = q0 if q0[3] >= 0 else -q0
    t0 = np.asarray(t_init, float) if given else np.zeros(3)
    lags = lag_grid(lat0, max_lag, lag_step)
    search_runs = not given and bool(estimate_latency)
    status = frames_taking_part(fx, lags[0], lags[-1], min_points) if search_runs else frames_taking_part(fx, lat0, lat0, min_points)
    out = dict(status=TOO_FEW_SAMPLES, frames_used=int((status == RESECT_OK).sum()), pairs_used=0, iterations=0, n_lags=0, peak_index=-1,
               coarse_latency=lat0, q_rig_camera=q0, t_rig_camera=t0, latency=lat0, cov=np.zeros((7, 7)), curve=None, rms=0.0,
               frame_status=status, frames=status == RESECT_OK)
    if out["frames_used"] < min_frames:
        return out
    free = np.array([1, 1, 1] + [estimate_translation] * 3 + [estimate_latency], bool)
    est = (q0, t0, lat0)
    if not given:
        q_cm, t_cm, status = resect(fx, status, huber_scale)
        use = status == RESECT_OK
        out.update(frame_status=status, frames=use, frames_used=int(use.sum()))
        if use.sum() < min_frames:
            return out
        if estimate_latency:
            curve, peak, coarse, st = search(fx, (q_cm, t_cm), use, lags)
            out.update(curve=curve, n_lags=len(lags), peak_index=peak, coarse_latency=coarse, peak_score=curve[peak])
            if st != OK:
                out["status"] = st
                return out
            est = (q0, t0, coarse)
        q, t = mean_pose(fx, (q_cm, t_cm), use, est[2])
        est = (q, t if estimate_translation else t0, est[2])
    frames = out["frames"]
    est, st, iterations = refine(fx, est, free, max_iterations, step_tolerance, sigma_pixel, huber_scale, frames)
    out.update(status=st, iterations=iterations)
    if st == DEGENERATE:
        return out
    out.update(q_rig_camera=est[0], t_rig_camera=est[1], latency=est[2])
    if st not in (OK, NOT_CONVERGED):
        return out
    _, _, _, e, valid, _ = system(fx, est, sigma_pixel, huber_scale, frames)
    fi = frame_of_pair(fx)
    n_used = np.bincount(fi[valid], minlength=len(frames))
    ss = np.bincount(fi, weights=(e * e).sum(1), minlength=len(frames))
    out.update(cov=covariance(fx, est, free, sigma_pixel, huber_scale, frames), rms=float(np.sqrt((e * e).sum() / valid.sum())),
               pairs_used=int(valid.sum()), final_cost=0.5 * rho_sum(e, huber_scale) / sigma_pixel ** 2, frame_n_used=n_used,
               frame_rms=np.sqrt(ss / np.maximum(n_used, 1)))
    return out


# ---- the optimiser's own camera term (the oracle, or the device's calico_evaluate) ------------------------------------------------------
def camera_problem(api, fx, est, sigma=1.0, frames=None, constant_ctrl=True):
    """A problem with one camera holding `est`, constant control points (the oracle; the device's library has them free, and the
    camera's blocks, registered last, are the last seven columns: constant_ctrl=False), chart and intrinsics; free extrinsics and
    latency. Returns (problem, columns): columns[i] is the index of parameter i of (rotation 3, translation 3, latency 1) in
    calico_evaluate's gradient; the sub-block of J^T J in these columns is the camera term's with the trajectory held. The quaternion's tangent is Ceres': q <- exp(d) q with |d| HALF the rotation angle, so its columns are twice the
    derivative in the rotation vector."""
    from calico_amd import _capi
    knots, basis, ctrl, order = fx["spl"]
    q, t, tau = est
    fi = frame_of_pair(fx)
    keep = np.ones(len(fi), bool) if frames is None else np.asarray(frames, bool)[fi]
    pts, inverse = np.unique(fx["points"][keep], axis=0, return_inverse=True)
    P = _capi.Problem(api, 0)
    pb = P.add_param_blocks(pts, constant=True)
    bt = P.add_param_block(fx["t_wm"], constant=True)
    bq = P.add_param_block(fx["q_wm"], _capi.MANIFOLD_EIGEN_QUATERNION, True)
    P.add_param_block(np.array([0.0, 0.0, -9.80665]), constant=True)
    body = P.add_rigid_body(bq, bt)
    cb = P.add_param_blocks(np.asarray(ctrl, float), constant=constant_ctrl)
    P.set_spline(order, knots, basis, cb)
    bi = P.add_param_block(fx["k"], constant=True)
    bT = P.add_param_block(np.asarray(t, float), constant=False)
    bQ = P.add_param_block(np.asarray(q, float), _capi.MANIFOLD_EIGEN_QUATERNION, False)
    bl = P.add_param_block([float(tau)], constant=False)
    sid = P.add_sensor(_capi.SENSOR_CAMERA, fx["model"], bi, bQ, bT, bl, -1, sigma, 0, 1.0)
    P.add_camera_residuals(sid, fx["pixels"][keep], fx["stamps"][fi][keep], np.full(int(keep.sum()), body, np.int32),
                           np.asarray(pb, np.int32)[np.ravel(inverse)])
    return P, np.array([3, 4, 5, 0, 1, 2, 6]) + (P.num_effective_parameters() - 7)


def oracle_step(P, columns, est, free=np.ones(7, bool)):
    """(cost, scaled Gauss-Newton step) of the problem's own gradient and J^T J in (rotation, translation, latency)."""
    c, g, H = P.evaluate()
    scale = np.array([2.0, 2.0, 2.0, 1, 1, 1, 1])      # Ceres' half-angle tangent
    g = g[columns] / scale
    H = H[np.ix_(columns, columns)] / np.outer(scale, scale)
    free = np.asarray(free, bool)
    d = np.zeros(7)
    d[free] = -np.linalg.solve(H[np.ix_(free, free)], g[free])
    return c, step_size(est, d), H
