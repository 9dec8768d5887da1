"""CPU reference of the observability report (calico_observability_compute), shared by test_observability_host.py and
test_gpu_observability.py: the scenes, and the numpy recipe that turns the oracle's dense JᵀJ into the spectrum of
S̃ = D⁻¹ (C - Eᵀ A⁻¹ E) D⁻¹ (include/calico_hip.h, "observability of the calibration")."""
import numpy as np

from calico_amd import _capi
from helpers import border_layout, copy_values, small_scene  # noqa: F401  (the tests reach them through this module)


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


def null_space_blocks(name, built, scene):
    """Block ids the null space of a singular table scene lives in (the issue's oracle finding)."""
    if "OpenCV8" in name:
        return [b["intrinsics"] for s, b in zip(scene.sensors, built.sensor_blocks) if s.kind == _capi.SENSOR_CAMERA]
    if "VectorNav" in name:
        return [b[k] for s, b in zip(scene.sensors, built.sensor_blocks) if s.kind != _capi.SENSOR_CAMERA for k in ("intrinsics", "q")]
    if "gauge" in name:
        return [built.body_t_block]
    raise KeyError(name)
