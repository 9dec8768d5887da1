"""Camera model maps without a GPU: every argument rule of the four entry points is checked before the device is touched (a rule
that reached HIP first would come back as CALICO_INTERNAL on a machine without one), n == 0 is OK, the entry points are
declared, listed and exported, _capi and the pybind module expose the new names, and the new kernels keep their budget: no
scratch, more than one wave per SIMD."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

import helpers
from calico_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

ENTRY_POINTS = ["camera_unproject", "camera_project_points", "sensor_unproject", "projection_uncertainty"]
K5 = np.array([785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2])


@pytest.fixture(scope="module")
def api():
    entry.build_hip()
    return _capi.CApi(C.CDLL(_capi.hip_library_path()), "calico_")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _invalid(api, st, *words):
    assert st == _capi.INVALID_ARGUMENT, st
    msg = api.last_error(None).decode()
    assert msg and msg != "null problem", msg
    for w in words:
        assert w in msg, (w, msg)


def test_entry_points_are_declared_listed_and_exported(api):
    header = open(os.path.join(ROOT, "include", "calico_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bcalico_%s\(" % name, header), name
        assert name in _capi.ABI_SYMBOLS
        assert hasattr(api.lib, "calico_" + name)
        assert hasattr(api, name)
    assert re.search(r"#define CALICO_FRAME_CAMERA 0\b", header) and re.search(r"#define CALICO_FRAME_RIG 1\b", header)
    assert (_capi.FRAME_CAMERA, _capi.FRAME_RIG) == (0, 1)
    assert "camera_kernels.hip" in entry.HIP_SOURCES
    for name in ("camera_unproject", "camera_project_points"):
        assert callable(getattr(_capi, name))
    for name in ("sensor_unproject", "projection_uncertainty"):
        assert callable(getattr(_capi.Problem, name))


def test_unproject_argument_rules_need_no_device(api):
    px, out, v = np.zeros((4, 2)), np.zeros((4, 3)), np.zeros(4, np.uint8)
    call = api.camera_unproject
    _invalid(api, call(0, 0, _dp(K5), 8, 4, _dp(px), _dp(out), _u8(v)), "unknown camera model")
    _invalid(api, call(0, 8, _dp(K5), 8, 4, _dp(px), _dp(out), _u8(v)), "unknown camera model")
    _invalid(api, call(0, 1, _dp(K5), 7, 4, _dp(px), _dp(out), _u8(v)), "8 intrinsics")
    _invalid(api, call(0, 2, _dp(K5), 8, 4, _dp(px), _dp(out), _u8(v)), "11 intrinsics")
    _invalid(api, call(0, 1, None, 8, 4, _dp(px), _dp(out), _u8(v)), "null intrinsics")
    _invalid(api, call(0, 1, _dp(K5), 8, -1, _dp(px), _dp(out), _u8(v)), "n must be >= 0")
    _invalid(api, call(0, 1, _dp(K5), 8, 4, None, _dp(out), _u8(v)), "null")
    _invalid(api, call(0, 1, _dp(K5), 8, 4, _dp(px), None, _u8(v)), "null")
    _invalid(api, call(0, 1, _dp(K5), 8, 4, _dp(px), _dp(out), None), "null")
    # the rules come before the device: a bad argument AND a bad device ordinal is still the argument's error
    _invalid(api, call(10 ** 6, 1, _dp(K5), 7, 4, _dp(px), _dp(out), _u8(v)), "intrinsics")
    assert call(0, 1, _dp(K5), 8, 0, None, None, None) == _capi.OK          # n == 0 touches nothing
    assert call(10 ** 6, 1, _dp(K5), 8, 0, None, None, None) == _capi.OK
    _invalid(api, api.debug_camera_unproject_chunked(0, 1, _dp(K5), 8, 4, _dp(px), _dp(out), _u8(v), 0), "chunk")
    if not helpers.has_gpu():       # a valid call without a device fails loudly, with a message
        assert call(0, 1, _dp(K5), 8, 4, _dp(px), _dp(out), _u8(v)) == _capi.INTERNAL
        assert "device" in api.last_error(None).decode()


def test_project_points_argument_rules_need_no_device(api):
    pt, px, v = np.ones((4, 3)), np.zeros((4, 2)), np.zeros(4, np.uint8)
    call = api.camera_project_points
    _invalid(api, call(0, -3, _dp(K5), 8, 4, _dp(pt), _dp(px), _u8(v), None, None), "unknown camera model")
    _invalid(api, call(0, 4, _dp(K5), 8, 4, _dp(pt), _dp(px), _u8(v), None, None), "5 intrinsics")
    _invalid(api, call(0, 1, None, 8, 4, _dp(pt), _dp(px), _u8(v), None, None), "null intrinsics")
    _invalid(api, call(0, 1, _dp(K5), 8, -2, _dp(pt), _dp(px), _u8(v), None, None), "n must be >= 0")
    _invalid(api, call(0, 1, _dp(K5), 8, 4, None, _dp(px), _u8(v), None, None), "null")
    _invalid(api, call(0, 1, _dp(K5), 8, 4, _dp(pt), None, _u8(v), None, None), "null")
    assert call(0, 1, _dp(K5), 8, 0, None, None, None, None, None) == _capi.OK
    if not helpers.has_gpu():       # valid, d_point and d_intrinsics, even all three optional pointers NULL: past the rules
        assert call(0, 1, _dp(K5), 8, 4, _dp(pt), _dp(px), None, None, None) == _capi.INTERNAL


def test_handle_calls_argument_rules_need_no_device(api):
    """What can be said without a handle (none can be created without a device): the rules on frame, range, n and the buffers
    come first and name themselves; a null handle is an argument error of its own. The sensor rules (unknown id, not a camera)
    need a handle: tests/test_gpu_camera_unproject.py and tests/test_gpu_projection_uncertainty.py hold them."""
    px, out, v = np.zeros((4, 2)), np.zeros((4, 3)), np.zeros(4, np.uint8)
    pu = api.projection_uncertainty
    _invalid(api, pu(None, 0, 2, 1.0, 4, _dp(px), _dp(out), _u8(v)), "frame")
    _invalid(api, pu(None, 0, -1, 1.0, 4, _dp(px), _dp(out), _u8(v)), "frame")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        _invalid(api, pu(None, 0, 1, bad, 4, _dp(px), _dp(out), _u8(v)), "range")
    _invalid(api, pu(None, 0, 1, 1.0, -1, _dp(px), _dp(out), _u8(v)), "n must be >= 0")
    _invalid(api, pu(None, 0, 1, 1.0, 4, None, _dp(out), _u8(v)), "null")
    _invalid(api, pu(None, 0, 1, 1.0, 4, _dp(px), None, _u8(v)), "null")
    _invalid(api, pu(None, 0, 1, 1.0, 4, _dp(px), _dp(out), None), "null")
    _invalid(api, pu(None, 0, 1, 1.0, 4, _dp(px), _dp(out), _u8(v)), "null problem handle")
    su = api.sensor_unproject
    _invalid(api, su(None, 0, 4, _dp(px), _dp(out), _u8(v)), "null problem handle")


def test_python_surfaces_expose_the_new_names():
    entry.build_hip()
    entry.build_python_module()
    from calico_amd import calico
    assert hasattr(calico.CameraModel, "UnprojectPixel") and hasattr(calico.CameraModel, "UnprojectPixels")
    assert hasattr(calico.Camera, "UnprojectPixels")
    assert hasattr(calico.Covariance, "ProjectionUncertainty")
    assert int(calico.ProjectionFrame.kCamera) == 0 and int(calico.ProjectionFrame.kRig) == 1
    # the module's error convention (a failed status raises with the library's message), reached without a device
    with pytest.raises(RuntimeError) as e:
        calico.CameraModel.UnprojectPixel(calico.CameraIntrinsicsModel.kOpenCv5, np.zeros(7), np.zeros(2))
    assert str(e.value).startswith("Error: ") and "8 intrinsics" in str(e.value)
    with pytest.raises(TypeError):      # pixels are (n, 2), or one pixel of length 2: nothing else is reinterpreted
        calico.CameraModel.UnprojectPixels(calico.CameraIntrinsicsModel.kOpenCv5, np.zeros(8), np.zeros((2, 3)))
    with pytest.raises(TypeError):
        calico.CameraModel.UnprojectPixels(calico.CameraIntrinsicsModel.kOpenCv5, np.zeros(8), np.zeros(4))


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_camera_kernels_resource_budget():
    """Throughput kernels: no scratch, no spills, and -- unlike every other kernel of the library -- several waves per SIMD
    (DESIGN.md section 4 states the registers)."""
    res = helpers.kernel_resources("camera_kernels.hip")
    names = {"camera_unproject_kernel": 7, "camera_project_points_kernel": 14, "projection_uncertainty_kernel": 7}
    for stem, count in names.items():
        mine = {k: v for k, v in res.items() if stem in k}
        assert len(mine) == count, sorted(res)
        for k, v in mine.items():
            print(k, v)
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
            assert v["Occupancy"] >= 4, (k, v)
            assert v["AGPRs"] == 0, (k, v)
    assert max(v["LDS Size"] for k, v in res.items() if "projection_uncertainty_kernel" in k) == 17 * 17 * 8
    assert all(v["LDS Size"] == 0 for k, v in res.items() if "projection_uncertainty_kernel" not in k)
