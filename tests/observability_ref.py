"""CPU reference of the observability report (calico_observability_compute), shared by test_observability_host.py and
test_gpu_observability.py: the scenes, and the numpy recipe that turns the oracle's dense JᵀJ into the spectrum of
S̃ = D⁻¹ (C - Eᵀ A⁻¹ E) D⁻¹ (include/calico_hip.h, "observability of the calibration")."""
import numpy as np

from calico_amd import _capi, synthetic as syn


def small_scene(camera_model=1, n_cameras=2, imu=True, imu_model=2, robust=False, seed=7, **kw):
    """The small scene of the covariance tests (same seeds, same rates)."""
    return syn.make_scene(n_cameras, camera_model, imu, imu_model, cam_rate=10.0, imu_rate=50.0, duration=3.0,
                          segment_duration=3.0 / 23.9, pixel_noise=0.1, gyro_noise=1e-3, accel_noise=1e-2, robust=robust,
                          seed=seed, **kw)


# name -> (scene factory, solver iterations before the pass (0: at the start values), n_weak with the default options)
TABLE_SCENES = {
    "camera 1, start": (lambda: small_scene(camera_model=1, imu=False), 0, 0),
    "camera 2 (OpenCV8), start": (lambda: small_scene(camera_model=2, imu=False), 0, 6),
    "free chart pose (gauge), start": (lambda: small_scene(camera_model=1, imu=False, free_chart_pose=True), 0, 3),
    "scale-and-bias IMU, solved": (lambda: small_scene(camera_model=1, imu=True, imu_model=2), 50, 0),
    "VectorNav IMU, solved": (lambda: small_scene(camera_model=1, imu=True, imu_model=3), 50, 6),
    "VectorNav IMU, solved, robust": (lambda: small_scene(camera_model=1, imu=True, imu_model=3, robust=True), 50, 6),
}
# further well-posed scenes of the spectrum parity: n_weak == 0
MORE_SCENES = {
    "camera 3, start": (lambda: small_scene(camera_model=3, imu=False), 0, 0),
    "camera 4, start": (lambda: small_scene(camera_model=4, imu=False), 0, 0),
    "camera 5, start": (lambda: small_scene(camera_model=5, imu=False), 0, 0),
    "camera 6, start": (lambda: small_scene(camera_model=6, imu=False), 0, 0),
    "camera 7, start": (lambda: small_scene(camera_model=7, imu=False), 0, 0),
    "order 7, solved": (lambda: small_scene(camera_model=1, imu=True, order=7), 50, 0),
    "order 8, solved": (lambda: small_scene(camera_model=1, imu=True, order=8), 50, 0),
    "free model points, solved": (lambda: small_scene(camera_model=1, n_cameras=2, imu=True, free_points=True, seed=5), 25, 0),
}
SINGULAR_SCENES = [k for k, v in TABLE_SCENES.items() if v[2] > 0]
WEAK_THRESHOLD = 1e-10       # calico_default_observability_options
GAP = 1e6                    # the subspace comparison needs λ_ref[n_weak] / max|λ_ref[:n_weak]| at least this


def copy_values(src, dst):
    """Parameter values of one built problem into another built from the same scene."""
    for b, n in dict(src.problem._sizes).items():
        dst.problem.set_param_block(b, src.problem.get_param_block(b, n))


def band_min_pivot(A, bandwidth):
    """Minimum pivot of the natural-order Cholesky of the equilibrated A (unit diagonal), stopping at the first pivot <= 0."""
    A = A.copy()
    n = len(A)
    lo = 1.0
    for j in range(n):
        p = A[j, j]
        lo = min(lo, p)
        if not p > 0.0:
            return lo
        e = min(n, j + bandwidth)
        c = A[j + 1:e, j] / np.sqrt(p)
        A[j + 1:e, j + 1:e] -= np.outer(c, c)
    return lo


def reference(ref, mc, order):
    """From the oracle's evaluate() at its current values. Returns a dict: keep (mask of the border's kept columns), lam, V
    (columns: eigenvectors on the kept columns), S (S̃ on the kept columns), band_pivot, band_cond; lam is None when the
    band is not positive definite."""
    _, _, H = ref.problem.evaluate()
    n = H.shape[0]
    na = n - mc
    A, E, C = H[:na, :na], H[:na, na:], H[na:, na:]
    ka = np.diag(A) != 0.0
    A, E = A[np.ix_(ka, ka)], E[ka]
    da = np.sqrt(np.diag(A))
    Ae = A / np.outer(da, da)
    out = dict(keep=np.diag(C) != 0.0, band_pivot=band_min_pivot(Ae, 6 * order), lam=None)
    if not out["band_pivot"] > 0.0:
        return out
    out["band_cond"] = np.linalg.cond(Ae)
    Es = E / da[:, None]
    S = C - Es.T @ np.linalg.solve(Ae, Es)
    kc = out["keep"]
    D = np.sqrt(np.diag(C)[kc])
    St = S[np.ix_(kc, kc)] / np.outer(D, D)
    St = 0.5 * (St + St.T)
    out["lam"], out["V"] = np.linalg.eigh(St)
    out["S"] = St
    return out


def weak_count(lam):
    return int((lam < WEAK_THRESHOLD).sum())


def projector(V, k):
    return V[:, :k] @ V[:, :k].T


def border_layout(built, scene):
    """{block id: (offset, tangent size)} of the dense border and its dimension, from the scene's structure alone: the free
    blocks a residual uses, control points excluded, in block-id order."""
    free, used = {}, set()
    pc = np.broadcast_to(np.asarray(scene.points_constant, bool), (len(scene.points),))
    for b, c in zip(built.point_blocks, pc):
        free[int(b)] = (not c, 3)
    free[built.body_t_block] = (not scene.body_pose_constant, 3)
    free[built.body_q_block] = (not scene.body_pose_constant, 3)
    free[built.gravity_block] = (False, 3)
    for s, b in zip(scene.sensors, built.sensor_blocks):
        free[b["intrinsics"]] = (s.enable_intrinsics, len(s.intrinsics))
        free[b["t"]] = (s.enable_extrinsics, 3)
        free[b["q"]] = (s.enable_extrinsics, 3)
        free[b["latency"]] = (s.enable_latency, 1)
        if s.n:
            used.update([b["intrinsics"], b["t"], b["q"], b["latency"]])
            if s.kind == _capi.SENSOR_CAMERA:
                used.update(int(built.point_blocks[i]) for i in np.unique(s.point_idx))
                used.update([built.body_t_block, built.body_q_block])
    out, off = {}, 0
    for b in sorted(free):
        if free[b][0] and b in used:
            out[b] = (off, free[b][1])
            off += free[b][1]
    return out, off


def null_space_blocks(name, built, scene):
    """Block ids the null space of a singular table scene lives in (the issue's oracle finding)."""
    if "OpenCV8" in name:
        return [b["intrinsics"] for s, b in zip(scene.sensors, built.sensor_blocks) if s.kind == _capi.SENSOR_CAMERA]
    if "VectorNav" in name:
        return [b[k] for s, b in zip(scene.sensors, built.sensor_blocks) if s.kind != _capi.SENSOR_CAMERA for k in ("intrinsics", "q")]
    if "gauge" in name:
        return [built.body_t_block]
    raise KeyError(name)
