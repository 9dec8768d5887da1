"""What the intrinsic-calibration tests share: the standard start and a plain numpy reference. No code under test in here.

The reference estimates the K intrinsics and the pose T_camera_chart of every frame jointly over the ORACLE's forward model
(camera_ref.oracle_project). Derivatives are central differences: h = 1e-6 for the pose (the local left perturbation
R <- exp([d]x) R and t, as resect_ref), h_i = 1e-6 max(1, |k_i|) for intrinsic i. Weights are rho' of Huber's loss, no
second-order term. Every frame eliminates its pose (per-frame Schur complement), the reduced K x K system gives dk, the frames
back-substitute. Marquardt damping lambda diag on the pose blocks and on the intrinsics block.

Step size (the library's definition):  s = max(|dk_i| / max(1, |k_i|), |d_rot|_inf, |d_t|_inf / max(1, |t|_2))  over all
unknowns. The optimality criterion the tests hold the device to: the reference's UNDAMPED Gauss-Newton step at the DEVICE's
estimate has s <= step_tolerance + 10 FLOOR[model].
"""
import functools

import numpy as np

import resect_ref as rr
from calico_amd import synthetic as syn

H = 1e-6
MODELS = rr.MODELS
NUM_PARAMS = {1: 8, 2: 11, 3: 7, 4: 5, 5: 4, 6: 4, 7: 5}
# FLOOR[model]: the reference's smallest repeatable undamped Gauss-Newton s at its own result (0.1 px noise, the standard
# start): the largest s of six undamped Gauss-Newton steps taken at and after the point where refine() stops. The steps do not
# shrink there, they scatter by a factor of up to ten: this is what the difference quotients resolve, amplified by the
# conditioning of the reduced system. tests/test_calib_host.py::test_reference_floor_and_noise_free_distance re-measures it on
# every run. Measured:
#   model 1: 2.4e-12   2: 3.3e-11   3: 1.5e-10   4: 1.9e-10   5: 8.1e-12   6: 2.7e-12   7: 4.9e-10
FLOOR = {1: 2.4e-12, 2: 3.3e-11, 3: 1.5e-10, 4: 1.9e-10, 5: 8.1e-12, 6: 2.7e-12, 7: 4.9e-10}
# REF_FREE[model]: the reference's own distance to the truth on noise-free data from the standard start (same test). Measured:
#   model 1: 3.4e-15   2: 3.2e-15   3: 2.0e-15   4: 3.6e-15   5: 2.4e-15   6: 4.0e-16   7: 1.4e-15
REF_FREE = {1: 3.4e-15, 2: 3.2e-15, 3: 2.0e-15, 4: 3.6e-15, 5: 2.4e-15, 6: 4.0e-16, 7: 1.4e-15}

# FLOOR_LONG[model]: FLOOR, measured the same way on resect_ref.long_fixture (137 frames of 12 pairs, 0.1 px noise) from
# long_start (tests/test_calib_host.py::test_reference_floor_of_the_long_batch re-measures it). Measured:
#   model 1: 6.2e-10   6: 5.9e-12      (6 and 5 accepted steps)
FLOOR_LONG = {1: 6.2e-10, 6: 5.9e-12}


def frame_system(model, k, R, t, pts, pix, huber=0.0, h=H, free=None):
    """(A 6x6, B 6xK, C KxK, g_pose, g_k, e, ok) of one frame: J by central differences in [d_rot, t | k]; the columns of an
    intrinsic that is not free are zero."""
    k = np.asarray(k, float)
    K = len(k)
    px, ok = rr.project(model, k, R, t, pts)
    cols = []
    for i in range(6):
        d = np.zeros(6)
        d[i] = h
        a, oka = rr.project(model, k, rr.exp_so3(d[:3]) @ R, t + d[3:], pts)
        b, okb = rr.project(model, k, rr.exp_so3(-d[:3]) @ R, t - d[3:], pts)
        ok = ok & oka & okb
        cols.append((a - b) / (2 * h))
    for i in range(K):
        if free is not None and not free[i]:
            cols.append(np.zeros_like(px))
            continue
        hi = h * max(1.0, abs(k[i]))
        kp, km = k.copy(), k.copy()
        kp[i] += hi
        km[i] -= hi
        a, oka = rr.project(model, kp, R, t, pts)
        b, okb = rr.project(model, km, R, t, pts)
        ok = ok & oka & okb
        cols.append((a - b) / (2 * hi))
    e = (px - pix)[ok]
    J = np.stack([c[ok] for c in cols], axis=2)      # (n, 2, 6 + K)
    w = rr.weights(e, huber)
    M = np.einsum("n,nri,nrj->ij", w, J, J)
    g = np.einsum("n,nri,nr->i", w, J, e)
    return M[:6, :6], M[:6, 6:], M[6:, 6:], g[:6], g[6:], e, ok


def systems(model, k, poses, off, pts, pix, huber=0.0, h=H, free=None):
    return [frame_system(model, k, R, t, pts[off[f]:off[f + 1]], pix[off[f]:off[f + 1]], huber, h, free)
            for f, (R, t) in enumerate(poses)]


def reduced(sys, lam=0.0, free=None):
    """(S, g_reduced, [(Y_B, Y_g) per frame]): S = C + lam diag C - Sum B^T (A + lam diag A)^-1 B; a constant gets an identity
    row and a zero right-hand side."""
    K = sys[0][1].shape[1]
    C = sum(s[2] for s in sys)
    S = C + lam * np.diag(np.diag(C))
    g = sum(s[4] for s in sys).copy()
    Y = []
    for A, B, _, gp, _, _, _ in sys:
        Ad = A + lam * np.diag(np.diag(A))
        YB, Yg = np.linalg.solve(Ad, B), np.linalg.solve(Ad, gp)
        S = S - B.T @ YB
        g = g - B.T @ Yg
        Y.append((YB, Yg))
    if free is not None:
        for i in range(K):
            if not free[i]:
                S[i, :] = 0.0
                S[:, i] = 0.0
                S[i, i] = 1.0
                g[i] = 0.0
    return S, g, Y


def step(sys, lam=0.0, free=None):
    """(dk, [d_f (6,) per frame]) of the (damped) Gauss-Newton step."""
    S, g, Y = reduced(sys, lam, free)
    dk = -np.linalg.solve(S, g)
    return dk, [-(Yg + YB @ dk) for YB, Yg in Y]


def step_size(k, poses, dk, d):
    s = float(np.max(np.abs(dk) / np.maximum(1.0, np.abs(k))))
    for (R, t), df in zip(poses, d):
        s = max(s, float(np.abs(df[:3]).max()), float(np.abs(df[3:]).max() / max(1.0, np.linalg.norm(t))))
    return s


def apply(k, poses, dk, d):
    return k + dk, [(rr.exp_so3(df[:3]) @ R, t + df[3:]) for (R, t), df in zip(poses, d)]


def cost(sys, huber=0.0):
    c = 0.0
    for s in sys:
        sq = (s[5] ** 2).sum(1)
        if huber > 0:
            r = np.sqrt(sq)
            sq = np.where(r > huber, 2 * huber * r - huber ** 2, sq)
        c += float(sq.sum())
    return c


def gn(model, k, poses, off, pts, pix, huber=0.0, h=H, free=None):
    """The undamped Gauss-Newton step at (k, poses): (dk, d, s)."""
    sys = systems(model, k, poses, off, pts, pix, huber, h, free)
    dk, d = step(sys, 0.0, free)
    return dk, d, step_size(k, poses, dk, d)


def refine(model, k, poses, off, pts, pix, huber=0.0, free=None, max_steps=40):
    """Levenberg-Marquardt (lambda from 1e-4, /10 on an accepted step, x10 on a rejected one) until the step stops shrinking
    at lambda <= 1e-4. Returns (k, poses, s of the last step, accepted steps, converged)."""
    k = np.asarray(k, float).copy()
    poses = [(R.copy(), np.asarray(t, float).copy()) for R, t in poses]
    lam, last, accepted = 1e-4, np.inf, 0
    sys = systems(model, k, poses, off, pts, pix, huber, H, free)
    c0 = cost(sys, huber)
    for _ in range(max_steps):
        dk, d = step(sys, lam, free)
        s = step_size(k, poses, dk, d)
        k1, p1 = apply(k, poses, dk, d)
        sys1 = systems(model, k1, p1, off, pts, pix, huber, H, free)
        c1 = cost(sys1, huber)
        same_pairs = all(a[6].sum() == b[6].sum() for a, b in zip(sys, sys1))
        if same_pairs and np.isfinite(c1) and c1 <= c0 * (1 + 1e-14):
            small = lam <= 1e-4 and last < 1e-7 and (s >= last or s < 1e-15)      # (quadratic convergence has hit the floor)
            if small and s >= last:
                return k, poses, last, accepted, True
            k, poses, sys, c0, last = k1, p1, sys1, c1, s
            accepted += 1
            if small:
                return k, poses, last, accepted, True
            lam = max(lam * 0.1, 1e-12)
        else:
            if lam <= 1e-4 and s < 1e-9:      # below what the cost resolves: the point is kept
                return k, poses, s, accepted, True
            lam = min(lam * 10.0, 1e12)
    return k, poses, last, accepted, False


def criterion(model, k, q, t, off, pts, pix, huber=0.0, free=None):
    """s of the reference's undamped Gauss-Newton step at the device's estimate (frames as (q, t) rows)."""
    poses = [(rr.rot(qf), np.asarray(tf, float)) for qf, tf in zip(q, t)]
    return gn(model, k, poses, off, pts, pix, huber, H, free)[2]


def rms_at(model, k, q, t, off, pts, pix):
    ss, n = 0.0, 0
    for f in range(len(q)):
        s = slice(off[f], off[f + 1])
        px, ok = rr.project(model, k, rr.rot(q[f]), np.asarray(t[f], float), pts[s])
        e = (px - pix[s])[ok]
        ss += float((e * e).sum())
        n += int(ok.sum())
    return float(np.sqrt(ss / n)), n


def reduced_covariance(model, k, q, t, off, pts, pix, huber=0.0, h=H, free=None):
    """(C - Sum B^T A^-1 B)^-1 at the estimate, zero rows and columns for the constants."""
    poses = [(rr.rot(qf), np.asarray(tf, float)) for qf, tf in zip(q, t)]
    S, _, _ = reduced(systems(model, k, poses, off, pts, pix, huber, h, free), 0.0, free)
    cov = np.linalg.inv(S)
    if free is not None:
        for i in range(len(k)):
            if not free[i]:
                cov[i, :] = 0.0
                cov[:, i] = 0.0
    return cov


def intrinsics_distance(k, truth, free=None):
    d = np.abs(np.asarray(k) - truth) / np.maximum(1.0, np.abs(truth))
    return float(d.max() if free is None else d[np.asarray(free, bool)].max())


def poses_distance(poses, truth):
    return max(rr.pose_distance(R, t, Rt, tt) for (R, t), (Rt, tt) in zip(poses, truth))


def start_intrinsics(model):
    """k0 = truth with f x 1.01, cx + 3, cy - 2 and the remaining entries x 0.9."""
    k = np.array(syn._TRUE_INTRINSICS[model], float)
    k0 = k * 0.9
    k0[0], k0[1], k0[2] = k[0] * 1.01, k[1] + 3.0, k[2] - 2.0
    return k0


@functools.lru_cache(maxsize=None)
def standard_start(model, noise):
    """(k0, q0 (20, 4), t0 (20, 3)) of the standard start for resect_ref.fixture(model, noise): k0 as above, the poses from
    resect_ref.refine at k0, started from the truth perturbed by 0.02 N(0, 1). Read-only arrays."""
    return start_of(rr.fixture(model, noise), model)


@functools.lru_cache(maxsize=None)
def long_start(model, noise):
    """The standard start of resect_ref.long_fixture(model, noise): (k0, q0 (137, 4), t0 (137, 3))."""
    return start_of(rr.long_fixture(model, noise), model)


def start_of(fixture, model):
    _, off, px, pt, poses = fixture
    k0 = start_intrinsics(model)
    rng = np.random.default_rng(4321 + model)
    q0, t0 = [], []
    for f, (R, t) in enumerate(poses):
        s = slice(off[f], off[f + 1])
        p = 0.02 * rng.standard_normal(6)
        Rs, ts, _, _ = rr.refine(model, k0, rr.exp_so3(p[:3]) @ R, t + p[3:], pt[s], px[s])
        q = rr.quat_of(Rs)
        q0.append(q if q[3] >= 0 else -q)
        t0.append(ts)
    q0, t0 = np.array(q0), np.array(t0)
    for a in (k0, q0, t0):
        a.setflags(write=False)
    return k0, q0, t0


def start_poses(q0, t0):
    return [(rr.rot(q), np.asarray(t, float)) for q, t in zip(q0, t0)]


FOV_W = 1e-3      # FieldOfView (model 5) below its w^2 < 1e-5 branch: the pixel does not depend on w there


@functools.lru_cache(maxsize=None)
def fov_fixture(noise=0.1):
    """resect_ref.fixture's 20 frames for FieldOfView at w = FOV_W: (intrinsics, offsets, pixels, points, true poses)."""
    model = 5
    k = np.array(syn._TRUE_INTRINSICS[model], float)
    k[3] = FOV_W
    pts = syn.planar_points()
    rng = np.random.default_rng(1234 + 50)
    poses = rr.true_poses()
    pix = []
    for R, t in poses:
        px, ok = rr.project(model, k, R, t, pts)
        assert ok.all()
        pix.append(px + noise * rng.standard_normal(px.shape))
    off = np.arange(len(poses) + 1, dtype=np.int64) * len(pts)
    px, pt = np.concatenate(pix), np.tile(pts, (len(poses), 1))
    for a in (k, off, px, pt):
        a.setflags(write=False)
    return k, off, px, pt, poses


@functools.lru_cache(maxsize=None)
def fov_start():
    """The standard start of fov_fixture() with w left at FOV_W: (k0, q0, t0)."""
    k, off, px, pt, poses = fov_fixture()
    k0 = np.array([k[0] * 1.01, k[1] + 3.0, k[2] - 2.0, FOV_W])
    rng = np.random.default_rng(4321 + 50)
    q0, t0 = [], []
    for f, (R, t) in enumerate(poses):
        s = slice(off[f], off[f + 1])
        p = 0.02 * rng.standard_normal(6)
        Rs, ts, _, _ = rr.refine(5, k0, rr.exp_so3(p[:3]) @ R, t + p[3:], pt[s], px[s])
        q = rr.quat_of(Rs)
        q0.append(q if q[3] >= 0 else -q)
        t0.append(ts)
    q0, t0 = np.array(q0), np.array(t0)
    for a in (k0, q0, t0):
        a.setflags(write=False)
    return k0, q0, t0


BOUNDARY_FRAME = 5
BOUNDARY_FREE = (1, 1, 1, 0)      # alpha is held: the validity boundary z = -w d of the unified model stays where the case put it


@functools.lru_cache(maxsize=None)
def boundary_fixture(kind):
    """resect_ref.fixture's 20 frames under the unified model at alpha = 0.7, frame BOUNDARY_FRAME replaced by
    resect_ref.boundary_case(kind) (37 pairs, the last one near the validity boundary). The start: k0 = the truth with
    f x 1.01, cx + 3, cy - 2 and alpha as it is (constant: BOUNDARY_FREE); the frames as standard_start makes them, the boundary
    frame at the case's start. Returns (k, off, px, pt, k0, q0, t0). Read-only arrays."""
    k = rr.unified_intrinsics()
    k0 = np.array([k[0] * 1.01, k[1] + 3.0, k[2] - 2.0, k[3]])
    case = rr.boundary_case(kind, BOUNDARY_FRAME, 0.1, tuple(k0))
    plane = syn.planar_points()
    rng, rng_start = np.random.default_rng(1234 + 60), np.random.default_rng(4321 + 60)
    px, pt, q0, t0 = [], [], [], []
    for f, (R, t) in enumerate(rr.true_poses()):
        if f == BOUNDARY_FRAME:
            pix, pts, (Rs, ts) = case.pixels, case.points, case.start
        else:
            pix, ok = rr.project(6, k, R, t, plane)
            assert ok.all()
            pix, pts = pix + 0.1 * rng.standard_normal(pix.shape), plane
            p = 0.02 * rng_start.standard_normal(6)
            Rs, ts, _, _ = rr.refine(6, k0, rr.exp_so3(p[:3]) @ R, t + p[3:], pts, pix)
        px.append(pix)
        pt.append(pts)
        q = rr.quat_of(Rs)
        q0.append(q if q[3] >= 0 else -q)
        t0.append(ts)
    off = np.concatenate([[0], np.cumsum([len(a) for a in px])]).astype(np.int64)
    out = (k, off, np.concatenate(px), np.concatenate(pt), k0, np.array(q0), np.array(t0))
    for a in out:
        a.setflags(write=False)
    return out
