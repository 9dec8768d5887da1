"""What the chart-resection tests share: fixtures and a plain numpy reference. No code under test in here.

The reference is a hand-written Gauss-Newton on T_camera_chart over the ORACLE's forward model (camera_ref.oracle_project):
derivatives are central differences with h = 1e-6, the rotation is parametrised by a local left perturbation about the
current pose, R <- exp([d]x) R (a global rotation vector is discontinuous at the angle pi of the reference fixture's
camera-from-chart rotations), weights are rho' of Huber's loss (1, or scale / |e|), and there is no second-order term. Its
own last step -- the FLOOR -- bounds what its difference quotients can resolve; the optimality criterion the tests hold the
device to is that the reference's weighted Gauss-Newton step AT THE DEVICE'S POSE is at most step_tolerance + 10 FLOOR.
"""
import collections
import functools

import numpy as np

import camera_ref
from calico_amd import synthetic as syn

H = 1e-6
# the largest last step of the reference over the seven models and 20 noisy frames (test_resect_host.py re-measures it)
FLOOR = 1.5e-13
MODELS = (1, 2, 3, 4, 5, 6, 7)


def rot(q):
    x, y, z, w = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def exp_so3(d):
    d = np.asarray(d, float)
    th = np.linalg.norm(d)
    K = np.array([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K + 0.5 * K @ K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * K @ K


def log_so3(R):
    """Rotation vector of a rotation near the identity."""
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(w)
    return w if s < 1e-8 else w * (np.arcsin(min(s, 1.0)) / s)


def pose_distance(Ra, ta, Rb, tb):
    """max(|rotation vector of Ra Rb^T|, |ta - tb|)."""
    return max(np.linalg.norm(log_so3(Ra @ Rb.T)), np.linalg.norm(np.asarray(ta) - np.asarray(tb)))


def project(model, k, R, t, pts):
    return camera_ref.oracle_project(model, k, pts @ R.T + t)


def weights(e, huber):
    s = np.sqrt((e * e).sum(1))
    w = np.ones(len(e))
    if huber > 0:
        big = s > huber
        w[big] = huber / s[big]
    return w


def system(model, k, R, t, pts, pix, huber=0.0, h=H):
    """(J^T W J, J^T W e, e, valid) at the pose: e = projection - pixel over the pairs the oracle accepts there (and at the
    twelve perturbed poses), J by central differences in [delta_rot, t]."""
    px, ok = project(model, k, R, t, pts)
    plus, minus = [], []
    for i in range(6):
        d = np.zeros(6)
        d[i] = h
        a, oka = project(model, k, exp_so3(d[:3]) @ R, t + d[3:], pts)
        b, okb = project(model, k, exp_so3(-d[:3]) @ R, t - d[3:], pts)
        ok = ok & oka & okb
        plus.append(a)
        minus.append(b)
    e = (px - pix)[ok]
    J = np.stack([((a - b) / (2 * h))[ok] for a, b in zip(plus, minus)], axis=2)      # (n, 2, 6)
    w = weights(e, huber)
    A = np.einsum("n,nri,nrj->ij", w, J, J)
    g = np.einsum("n,nri,nr->i", w, J, e)
    return A, g, e, ok


def gn_step(model, k, R, t, pts, pix, huber=0.0, h=H):
    A, g, _, _ = system(model, k, R, t, pts, pix, huber, h)
    return -np.linalg.solve(A, g)


def refine(model, k, R, t, pts, pix, huber=0.0, max_steps=25):
    """Gauss-Newton until the step stops shrinking. Returns (R, t, |last step|_inf, steps)."""
    last = np.inf
    for it in range(max_steps):
        d = gn_step(model, k, R, t, pts, pix, huber)
        n = np.abs(d).max()
        if it > 0 and (n >= last or n < 1e-15):
            if n < last:
                R, t, last = exp_so3(d[:3]) @ R, t + d[3:], n
            return R, t, last, it + 1
        R, t, last = exp_so3(d[:3]) @ R, t + d[3:], n
    return R, t, last, max_steps


def criterion(model, k, q, t, pts, pix, huber=0.0):
    """|reference Gauss-Newton step at the device's pose|_inf."""
    return float(np.abs(gn_step(model, k, rot(q), np.asarray(t, float), pts, pix, huber)).max())


def rms_at(model, k, q, t, pts, pix):
    px, ok = project(model, k, rot(q), np.asarray(t, float), pts)
    e = (px - pix)[ok]
    return float(np.sqrt((e * e).sum() / ok.sum())), int(ok.sum())


def true_poses():
    """T_camera_chart (R, t) of every 12th of the 240 default synthetic poses: 20 frames."""
    _, q_wr, t_wr = syn.default_synthetic_poses()
    out = []
    for q, tw in zip(q_wr[::12], t_wr[::12]):
        R = rot(q).T
        out.append((R, -R @ tw))
    return out


@functools.lru_cache(maxsize=None)
def fixture(model, noise, points="planar"):
    """(intrinsics, frame offsets, pixels (N, 2), points (N, 3), true poses) of the 20 frames: every point of the chart in
    every frame, pixels of the oracle's projection plus Gaussian noise of `noise` pixels. Read-only arrays."""
    k = np.array(syn._TRUE_INTRINSICS[model], float)
    pts = syn.planar_points() if points == "planar" else syn.aprilgrid_points()
    rng = np.random.default_rng(1234 + model)
    poses = true_poses()
    pix = []
    for R, t in poses:
        px, ok = project(model, k, R, t, pts)
        assert ok.all()
        pix.append(px + noise * rng.standard_normal(px.shape))
    off = np.arange(len(poses) + 1, dtype=np.int64) * len(pts)
    px, pt = np.concatenate(pix), np.tile(pts, (len(poses), 1))
    for a in (k, off, px, pt):
        a.setflags(write=False)
    return k, off, px, pt, poses


LONG_FRAMES = 137      # more than 8 x 16 (the calibration's unrolled reduction) and 2 x 64 + 9 (its decision's strided sums)


@functools.lru_cache(maxsize=None)
def long_poses(n_frames, seed):
    """n_frames seeded draws around true_poses(): pose f is true_poses()[f % 20] turned by 0.05 N(0, 1) rad and moved by
    0.03 N(0, 1) m."""
    base = true_poses()
    rng = np.random.default_rng(seed)
    out = []
    for f in range(n_frames):
        R, t = base[f % len(base)]
        p = rng.standard_normal(6)
        out.append((exp_so3(0.05 * p[:3]) @ R, t + 0.03 * p[3:]))
    return out


@functools.lru_cache(maxsize=None)
def long_fixture(model, noise, n_frames=LONG_FRAMES):
    """As fixture(), for n_frames poses of long_poses() and the 12 chart points planar_points()[::3] per frame: every pair is
    valid (asserted from the oracle). Read-only arrays."""
    k = np.array(syn._TRUE_INTRINSICS[model], float)
    pts = syn.planar_points()[::3]
    rng = np.random.default_rng(5678 + model)
    poses = long_poses(n_frames, 8765)
    pix = []
    for R, t in poses:
        px, ok = project(model, k, R, t, pts)
        assert ok.all()
        pix.append(px + noise * rng.standard_normal(px.shape))
    off = np.arange(len(poses) + 1, dtype=np.int64) * len(pts)
    px, pt = np.concatenate(pix), np.tile(pts, (len(poses), 1))
    for a in (k, off, px, pt):
        a.setflags(write=False)
    return k, off, px, pt, poses


UNIFIED_ALPHA = 0.7      # the unified model (6) of the boundary cases: valid for z > -w d, w = (1 - alpha) / alpha; the pixel is finite there


def unified_intrinsics():
    k = np.array(syn._TRUE_INTRINSICS[6], float)
    k[3] = UNIFIED_ALPHA
    return k


def axis_angle(P):
    """The angle between a point in the camera frame and the optical axis."""
    P = np.asarray(P, float)
    return float(np.arccos(P[2] / np.linalg.norm(P)))


def unified_boundary_angle():
    return float(np.arccos(-(1 - UNIFIED_ALPHA) / UNIFIED_ALPHA))


BoundaryCase = collections.namedtuple("BoundaryCase", "k points pixels start truth")


@functools.lru_cache(maxsize=None)
def boundary_case(kind, frame=5, noise=0.1, k_start=None, displaced=100.0):
    """One frame of the chart under the unified model at alpha = 0.7 with ONE extra chart point off the plane (the last pair),
    near the model's validity boundary. truth: the pose the 36 planar pixels were made at (0.1 px noise); start: the truth
    turned by 0.02 rad about the camera's y axis, which moves the extra point across the boundary.
      "lost":    valid at the start, 0.3 degrees inside, pixel = its projection at the start; beyond the boundary at the truth
      "invalid": 2 degrees beyond the boundary at the start and farther at the truth; its pixel is never read
      "joins":   0.3 degrees beyond at the start, inside at the truth; pixel = its projection at the truth moved by `displaced` px
    k_start (a tuple): the intrinsics the "lost" pixel is projected with, where the start's are not the truth's (the
    calibration; alpha must be the truth's). Returns BoundaryCase(k, points (37, 3), pixels (37, 2), start (R, t), truth (R, t)).
    Read-only arrays."""
    k = unified_intrinsics()
    Rt, tt = true_poses()[frame]
    plane = syn.planar_points()
    rng = np.random.default_rng(606 + frame)
    px, ok = project(6, k, Rt, tt, plane)
    assert ok.all()
    px = px + noise * rng.standard_normal(px.shape)
    off_deg, sign = {"lost": (-0.3, -1.0), "invalid": (2.0, -1.0), "joins": (0.3, 1.0)}[kind]
    Rs = exp_so3([0.0, sign * 0.02, 0.0]) @ Rt
    th = unified_boundary_angle() + np.deg2rad(off_deg)
    Pc = 1.0 * np.array([np.sin(th), 0.0, np.cos(th)])      # in the camera frame at the start, 1 m away
    extra = Rs.T @ (Pc - tt)
    pts = np.vstack([plane, extra])
    if kind == "joins":
        e_px, e_ok = project(6, k, Rt, tt, extra[None])
        e_px = e_px + [[displaced, 0.0]]
    else:
        e_px, e_ok = project(6, k if k_start is None else np.array(k_start, float), Rs, tt, extra[None])
        if kind == "invalid":
            e_px, e_ok = np.zeros((1, 2)), np.ones(1, bool)
    assert e_ok.all()
    pix = np.vstack([px, e_px])
    for a in (k, pts, pix):
        a.setflags(write=False)
    return BoundaryCase(k, pts, pix, (Rs, np.array(tt, float)), (Rt, np.array(tt, float)))


def behind(pose):
    """The pose moved along the optical axis so that the chart (within 1 m of its origin) is behind the camera: no pair of a
    pinhole model (1) projects from there."""
    R, t = pose
    return R, np.array([t[0], t[1], -abs(t[2]) - 1.0])


def wide_angle(model):
    """An 11 x 11 chart of 0.3 m pitch seen from 0.25 m above its centre, looking down, tilted 35 degrees about x: points behind
    the image plane (camera z <= 0) project under the sphere models. (intrinsics, pixels, points, valid, R, t)."""
    k = np.array(syn._TRUE_INTRINSICS[model], float)
    g = (np.arange(11) - 5) * 0.3
    pts = np.array([[x, y, 0.0] for x in g for y in g])
    R = exp_so3([np.deg2rad(35.0), 0, 0]) @ np.diag([1.0, -1.0, -1.0])
    t = -R @ np.array([0.0, 0.0, 0.25])
    px, ok = project(model, k, R, t, pts)
    return k, px, pts, ok, R, t


def quat_of(R):
    """(x, y, z, w) of a rotation matrix, stable at every angle (the largest of the four components is the divisor)."""
    tr = np.trace(R)
    if tr > 0:
        s = 2 * np.sqrt(1 + tr)
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, 0.25 * s]
    elif R[0, 0] > R[1, 1] and R[0, 0] > R[2, 2]:
        s = 2 * np.sqrt(1 + R[0, 0] - R[1, 1] - R[2, 2])
        q = [0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif R[1, 1] > R[2, 2]:
        s = 2 * np.sqrt(1 + R[1, 1] - R[0, 0] - R[2, 2])
        q = [(R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        s = 2 * np.sqrt(1 + R[2, 2] - R[0, 0] - R[1, 1])
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s, (R[1, 0] - R[0, 1]) / s]
    return np.array(q)
