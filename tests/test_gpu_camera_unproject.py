"""Camera model maps on the device: calico_camera_unproject, calico_camera_project_points, calico_sensor_unproject.

References are existing code, never the code under test: the oracle's forward model (oracle_project_point) and numpy.
The grid is the reference's own (camera_models_test.cpp: 61 x 61 points of a 1.5 m plane 1 m in front of the camera), the
intrinsics are its test's, the tolerances on the bearing are its test's too: 1e-10 OpenCv5/8, 1e-9 KannalaBrandt, 1e-12
DoubleSphere / FieldOfView / Unified. ExtendedUnified is held to the definition of this library's inverse (the unit-norm point
that projects to the pixel; quirk Q5b): pixels are the oracle's projection of p / |p|, and the bound is the one the reference
gives its other Newton-based inverses with the same stop rule, 1e-10.
Pixel space, all seven models: oracle_project_point(unproject(px)) == px within 1e-9 px (stop rule 1e-14 normalised x f = 785:
8e-12 px, two orders of margin for conditioning at the grid's edge).
Measured (MI355X), max over the grid, bearing / pixel: OpenCv5 7.7e-15 / 6.8e-12, OpenCv8 8.3e-15 / 6.7e-12, KannalaBrandt
1.0e-14 / 7.4e-12, DoubleSphere 3.3e-16 / 1.1e-13, FieldOfView 3.3e-16 / 3.4e-13, Unified 3.3e-16 / 2.3e-13, ExtendedUnified
6.3e-15 / 7.2e-12."""
import ctypes as C
import functools

import numpy as np
import pytest

from calico_amd import _capi, synthetic as syn
from camera_ref import grid, oracle_project
from helpers import small_scene, solve

pytestmark = pytest.mark.gpu

CASES = {
    1: ([785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2], 1e-10),
    2: ([785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2, 1.225e-1, -5.26e-2, 8.58e-3], 1e-10),
    3: ([785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4], 1e-9),
    4: ([785, 640, 400, 0.5, 0.5], 1e-12),
    5: ([785, 640, 400, 0.05], 1e-12),
    6: ([785, 640, 400, 0.5], 1e-12),
    7: ([785, 640, 400, 0.5, 0.5], 1e-10),
}
PIXEL_TOL = 1e-9
MODELS = sorted(CASES)


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


@functools.lru_cache(maxsize=None)
def grid_pixels(model):
    """The oracle's pixels of the grid (ExtendedUnified: of the grid's unit vectors), computed once per model."""
    pts, unit = grid()
    px, ok = oracle_project(model, CASES[model][0], unit if model == 7 else pts)
    assert ok.all()
    px.setflags(write=False)
    return px


@pytest.mark.parametrize("model", MODELS)
def test_round_trip_on_the_reference_grid(model, hip):
    k, tol = CASES[model]
    _, unit = grid()
    px = grid_pixels(model)
    b, valid = _capi.camera_unproject(hip, model, k, px)
    assert valid.all(), int((~valid).sum())           # the oracle projects all 3,721: the share left out is zero
    assert np.abs(np.linalg.norm(b, axis=1) - 1.0).max() <= 1e-15
    e_bearing = np.abs(b - unit).max()
    back, ok = oracle_project(model, k, b)
    assert ok.all()
    e_pixel = np.abs(back - px).max()
    print("model %d: bearing error %.2e (bound %.0e), pixel error %.2e (bound %.0e)" % (model, e_bearing, tol, e_pixel, PIXEL_TOL))
    assert e_bearing <= tol
    assert e_pixel <= PIXEL_TOL


@pytest.mark.parametrize("n,chunk", [(1, None), (63, None), (64, None), (65, None), (257, None), (257, 100), (257, 256), (130, 64)])
def test_sizes_chunks_and_untouched_tails(n, chunk, hip):
    """Less than a wave, a wave, one lane more, more than one workgroup (256 threads); n over two and three host-side chunks
    (the chunk is a parameter of the internal helper: a few hundred pixels reach its boundary). Whatever lies beyond n in an
    over-allocated buffer keeps its canary."""
    model = 1
    k = np.array(CASES[model][0], float)
    full, _ = _capi.camera_unproject(hip, model, k, grid_pixels(model)[:300])
    px = np.ascontiguousarray(grid_pixels(model)[:n + 40])
    out = np.full((n + 40, 3), -7.25)
    valid = np.full(n + 40, 0xA5, np.uint8)
    if chunk is None:
        st = hip.camera_unproject(0, model, _dp(k), k.size, n, _dp(px), _dp(out), _u8(valid))
    else:
        st = hip.debug_camera_unproject_chunked(0, model, _dp(k), k.size, n, _dp(px), _dp(out), _u8(valid), chunk)
    assert st == _capi.OK, hip.last_error(None)
    assert np.array_equal(out[:n], full[:n]) and np.all(valid[:n] == 1)
    assert np.all(out[n:] == -7.25) and np.all(valid[n:] == 0xA5)


def _numpy_newton_residual(k, px, steps=30):
    """Residual (normalised units) of a plain numpy Newton on the OpenCv5 distortion after `steps` steps from the distorted point."""
    f, cx, cy, k1, k2, p1, p2, k3 = k
    mx, my = (px[:, 0] - cx) / f, (px[:, 1] - cy) / f
    x, y = mx.copy(), my.copy()
    best = np.full(len(px), np.inf)
    with np.errstate(all="ignore"):
        for it in range(steps + 1):
            r2 = x * x + y * y
            s = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
            sp = k1 + r2 * (2 * k2 + 3 * r2 * k3)
            ex = mx - (x * s + 2 * p1 * x * y + p2 * (r2 + 2 * x * x))
            ey = my - (y * s + 2 * p2 * x * y + p1 * (r2 + 2 * y * y))
            res = np.abs(ex) + np.abs(ey)
            best = np.fmin(best, np.where(np.isfinite(res), res, np.inf))
            if it == steps:
                break
            a = s + 2 * x * x * sp + 2 * p1 * y + 6 * p2 * x
            c = 2 * x * y * sp + 2 * p1 * x + 2 * p2 * y
            d = s + 2 * y * y * sp + 2 * p2 * x + 6 * p1 * y
            det = a * d - c * c
            x, y = x + (d * ex - c * ey) / det, y + (a * ey - c * ex) / det
    return best


def test_invalid_pixels_come_back_as_zeros_and_leave_their_wave_alone(hip):
    """A negative radicand (DoubleSphere with alpha = 0.8: 1 - (2 alpha - 1) r^2 < 0; ExtendedUnified with alpha = 0.8: no
    unit-norm point in the projection's domain reaches |m| = 3, where the reference's radicand 1 - (2 alpha - 1) beta r^2 is
    negative too) and an OpenCv5 pixel far outside the image where a numpy Newton never comes within 1e-3 of the stop rule's
    quantity in 30 steps: valid = 0 with zeros, and the other lanes of the same wave are what they are without them."""
    f = 785.0
    far5 = np.array([[640 + f * a, 400 + f * b] for a in np.arange(0.9, 3.05, 0.1) for b in np.arange(0.9, 3.05, 0.1)])
    k5 = np.array(CASES[1][0], float)
    res = _numpy_newton_residual(k5, far5)
    assert (res > 1e-3).any(), "no OpenCv5 pixel of the candidates fails on the CPU"
    bad5 = far5[np.argsort(-res)[:2]]
    print("OpenCv5 pixels the numpy Newton does not invert (best residual %s): %s" % (np.sort(res)[-2:], bad5.tolist()))
    cases = [(1, k5, bad5),
             (4, np.array([785, 640, 400, 0.5, 0.8]), np.array([[640 + 2 * f, 400.0], [640.0, 400 - 1.5 * f]])),
             (7, np.array([785, 640, 400, 0.8, 0.5]), np.array([[640 + 3 * f, 400.0], [640 - 2.5 * f, 400 + 2.5 * f]]))]
    for model, k, bad in cases:
        good = np.array([[640 + 3.0 * i, 400 - 2.0 * i] for i in range(64)])      # one wave of pixels near the image centre
        clean, v_clean = _capi.camera_unproject(hip, model, k, good)
        assert v_clean.all()
        mixed = good.copy()
        mixed[5], mixed[40] = bad[0], bad[1]
        b, v = _capi.camera_unproject(hip, model, k, mixed)
        keep = np.ones(64, bool)
        keep[[5, 40]] = False
        assert not v[5] and not v[40] and np.all(b[[5, 40]] == 0.0), (model, v[[5, 40]], b[[5, 40]])
        assert v[keep].all() and np.array_equal(b[keep], clean[keep]), model


def _central(model, k, pts, h):
    """Central differences of the oracle's forward model: (d pixel / d point (n, 2, 3), d pixel / d intrinsics (n, 2, K))."""
    k = np.array(k, float)
    dP, dK = np.zeros((len(pts), 2, 3)), np.zeros((len(pts), 2, len(k)))
    for c in range(3):
        e = np.zeros(3)
        e[c] = h
        dP[:, :, c] = (oracle_project(model, k, pts + e)[0] - oracle_project(model, k, pts - e)[0]) / (2 * h)
    for c in range(len(k)):
        e = np.zeros(len(k))
        e[c] = h
        dK[:, :, c] = (oracle_project(model, k + e, pts)[0] - oracle_project(model, k - e, pts)[0]) / (2 * h)
    return dP, dK


def _column_error(a, b):
    """Largest difference per column (parameter), relative to the column's largest entry of b."""
    scale = np.abs(b).max(axis=(0, 1))
    return (np.abs(a - b).max(axis=(0, 1)) / np.where(scale > 0, scale, 1.0)).max()


@pytest.mark.parametrize("model", MODELS)
def test_forward_points_kernel(model, hip):
    """camera_project_points on the grid: pixels equal the oracle's within 1e-9 px; d_point and d_intrinsics equal central
    differences of the oracle (step 1e-6) on every fifth grid point in each direction (13 x 13, corners and centre included).
    Tolerance: ten times the finite-difference floor, which is the same central difference at step 1e-5 against itself at 1e-6,
    per column relative to the column's largest entry -- measured by the reference alone, inside the test.
    Measured (MI355X) finite-difference floor / error of the analytic derivatives against step 1e-6, worst column, d_point and
    d_intrinsics together: OpenCv5 1.8e-7 / 1.7e-7, OpenCv8 1.5e-7 / 1.5e-7, KannalaBrandt 1.8e-7 / 1.8e-7, DoubleSphere
    1.3e-7 / 1.3e-7, FieldOfView 1.5e-7 / 1.5e-7, Unified 1.4e-7 / 1.3e-7, ExtendedUnified 1.1e-6 / 1.3e-7 (the worst column
    is a linear one, c_x or c_y: the rounding of a pixel value of ~1e3 over a step of 1e-6); pixels within 2.9e-13 px."""
    k = CASES[model][0]
    pts, _ = grid()
    px, valid = _capi.camera_project_points(hip, model, k, pts)
    assert valid.all()
    ref, ok = oracle_project(model, k, pts)
    assert ok.all()
    print("model %d: pixels against the oracle %.2e" % (model, np.abs(px - ref).max()))
    assert np.abs(px - ref).max() <= PIXEL_TOL
    sub = np.ascontiguousarray(pts.reshape(61, 61, 3)[::5, ::5].reshape(-1, 3))
    px2, v2, dP, dK = _capi.camera_project_points(hip, model, k, sub, jacobians=True)
    assert v2.all() and np.array_equal(px2, px.reshape(61, 61, 2)[::5, ::5].reshape(-1, 2))
    fP, fK = _central(model, k, sub, 1e-6)
    cP, cK = _central(model, k, sub, 1e-5)
    floor = max(_column_error(cP, fP), _column_error(cK, fK))
    err = max(_column_error(dP, fP), _column_error(dK, fK))
    print("model %d: finite-difference floor %.2e, analytic against step 1e-6 %.2e" % (model, floor, err))
    assert err <= 10.0 * floor


def test_points_the_models_reject(hip):
    """z <= 0 is rejected by the pinhole-type models (OpenCv5/8, KannalaBrandt, FieldOfView); the sphere models take a point
    slightly behind the camera plane, Unified and ExtendedUnified reject one on the negative axis. DoubleSphere's rule
    (z^2 <= -w2^2 |p|^2) rejects nothing; at (0, 0, -1) with xi = alpha = 0.5 its denominator is exactly zero and the oracle
    returns a non-finite pixel with an OK status: the device reports such a pixel as valid = 0. valid = 0 comes with zeros
    everywhere."""
    pts = np.array([[0.1, 0.1, 1.0], [0.1, 0.1, -1.0], [0.2, -0.1, 0.0], [1.0, 0.0, -0.1], [0.0, 0.0, -1.0]])
    for model in MODELS:
        k = CASES[model][0]
        px, v, dP, dK = _capi.camera_project_points(hip, model, k, pts, jacobians=True)
        ref, ok = oracle_project(model, k, pts)
        ok = ok & np.isfinite(ref).all(axis=1)
        assert np.array_equal(v, ok), (model, v, ok)
        assert v[0] and not v[4]
        if model in (1, 2, 3, 5):
            assert not v[1] and not v[2] and not v[3]
        assert np.abs(px[v] - ref[v]).max() <= PIXEL_TOL
        assert np.all(px[~v] == 0.0) and np.all(dP[~v] == 0.0) and np.all(dK[~v] == 0.0)


def test_sensor_unproject_is_the_free_call_at_the_current_intrinsics(hip):
    """After a solve of the small camera + IMU scene: the handle's call (intrinsics read on the device from the parameter
    vector, on the handle's stream) equals calico_camera_unproject at the values calico_get_param_block returns, bit for bit.
    The sensor rules need a handle and are held here: an unknown id and a sensor that is not a camera are argument errors."""
    scene = small_scene(camera_model=1, imu=True)
    gpu = syn.build_problem(hip, scene)
    P = gpu.problem
    start = P.get_param_block(gpu.sensor_blocks[1]["intrinsics"], 8)
    solve(P, hip)
    px = np.array([[40.0 * i + 3.5, 25.0 * j + 1.25] for i in range(33) for j in range(33)])      # 1089 pixels over a 1280 x 800 image
    for c in (0, 1):
        k = P.get_param_block(gpu.sensor_blocks[c]["intrinsics"], 8)
        b, v = P.sensor_unproject(gpu.sensor_ids[c], px)
        b0, v0 = _capi.camera_unproject(hip, 1, k, px)
        assert v.sum() > 1000 and np.array_equal(v, v0)
        assert b.tobytes() == b0.tobytes()
    assert not np.array_equal(k, start)        # (the solve moved them: it is the CURRENT values that are read)
    gyro = [sid for sid, s in zip(gpu.sensor_ids, scene.sensors) if s.kind == _capi.SENSOR_GYROSCOPE][0]
    for sid, word in ((len(scene.sensors), "unknown sensor"), (-1, "unknown sensor"), (gyro, "not a camera")):
        with pytest.raises(_capi.CalicoError) as e:
            P.sensor_unproject(sid, px)
        assert e.value.code == _capi.INVALID_ARGUMENT and word in e.value.message
    out, vv = np.zeros((4, 3)), np.zeros(4, np.uint8)
    assert hip.sensor_unproject(P.h, gpu.sensor_ids[0], -1, _dp(px), _dp(out), _u8(vv)) == _capi.INVALID_ARGUMENT
    assert hip.sensor_unproject(P.h, gpu.sensor_ids[0], 4, None, _dp(out), _u8(vv)) == _capi.INVALID_ARGUMENT
    assert hip.sensor_unproject(P.h, gpu.sensor_ids[0], 0, None, None, None) == _capi.OK
