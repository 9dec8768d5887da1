"""What the camera-map tests share: the oracle's forward model over arrays of points and the grid of the reference's own
camera model test. No code under test in here."""
import ctypes as C
import functools

import numpy as np

import helpers


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def oracle_project(model, k, pts):
    """(pixels, valid) of the oracle's forward model, point by point."""
    lib = helpers.oracle_lib()
    k = np.ascontiguousarray(k, float)
    pts = np.ascontiguousarray(pts, float).reshape(-1, 3)
    px, ok = np.zeros((len(pts), 2)), np.zeros(len(pts), bool)
    for i in range(len(pts)):
        ok[i] = lib.oracle_project_point(model, _dp(k), _dp(pts[i]), _dp(px[i])) == 0
    return px, ok


@functools.lru_cache(maxsize=None)
def grid():
    """The 61 x 61 points of camera_models_test.cpp in the camera frame, and their unit vectors."""
    R = np.diag([1.0, -1.0, -1.0])
    tc = np.array([0.75, 0.75, 1.0])
    n = int(1.5 / 0.025) + 1
    pts = np.array([[i * 0.025, j * 0.025, 0.0] for i in range(n) for j in range(n)])
    pts = (pts - tc) @ R
    pts.setflags(write=False)
    unit = pts / np.linalg.norm(pts, axis=1, keepdims=True)
    unit.setflags(write=False)
    return pts, unit
