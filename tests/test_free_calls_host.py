"""The calls without a problem handle, without a GPU: every one of them -- calico_camera_unproject, calico_camera_project_points,
calico_camera_resect, calico_camera_calibrate, calico_imu_align and calico_fit_spline -- returns its non-OK code with a message
that starts with its own name in the calling thread's slot (calico_last_error(NULL)); calico_fit_spline's argument rules give
the codes they always gave (INVALID_ARGUMENT, UNIMPLEMENTED) and now a message; an argument's error comes before the device is
touched; a valid call without a device is INTERNAL and says "device". And the layout that keeps it that way: one device buffer,
one error macro, one camera-model dispatch, one step rule (free_call.hpp, kernels.hpp, lm_rule.hpp)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import fit_ref
import helpers
import imu_align_ref as ar
from calico_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

K5 = np.array([500.0, 320.0, 240.0, 0.01, -0.02, 0.001, 0.002, 0.0])      # OpenCv5 (model 1): 8 intrinsics
NO_DEVICE = 10 ** 6


@pytest.fixture(scope="module")
def api():
    entry.build_hip()
    return _capi.CApi(C.CDLL(_capi.hip_library_path()), "calico_")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _message(api, st, code, name, *words):
    assert st == code, (st, code)
    msg = api.last_error(None).decode()
    assert msg.startswith(name + ": "), msg
    for w in words:
        assert w in msg, (w, msg)
    return msg


class _Fit:
    """calico_fit_spline on fifty samples of a 7.2 s trajectory, one argument replaced at a time."""

    NAMES = ("device", "order", "n_knots", "knots", "basis", "n", "stamps", "data", "ctrl")

    def __init__(self, api):
        self.api = api
        self.order = 6
        self.knots = fit_ref.uniform_knots(30, self.order)
        from calico_amd import synthetic as syn
        self.basis = np.ascontiguousarray(syn.basis_matrices(self.knots, self.order))
        vk = self.knots[self.order - 1:len(self.knots) - self.order + 1]
        self.first, self.last = vk[0], vk[-1]
        self.stamps = np.linspace(self.first, self.last, 50)
        self.data = np.zeros((50, 6))
        self.ctrl = np.zeros((30, 6))

    def __call__(self, **kw):
        a = dict(device=0, order=self.order, n_knots=len(self.knots), knots=_dp(self.knots), basis=_dp(self.basis), n=50, stamps=_dp(self.stamps),
                 data=_dp(self.data), ctrl=_dp(self.ctrl))
        a.update(kw)
        return self.api.fit_spline(*[a[n] for n in self.NAMES])


def test_every_free_call_names_itself(api):
    """One argument error per entry point: its code, and a message that starts with the entry's own name."""
    px, b3, v = np.zeros((4, 2)), np.zeros((4, 3)), np.zeros(4, np.uint8)
    _message(api, api.camera_unproject(NO_DEVICE, 1, _dp(K5), 7, 4, _dp(px), _dp(b3), _u8(v)), _capi.INVALID_ARGUMENT,
             "calico_camera_unproject", "8 intrinsics, got 7")
    _message(api, api.camera_unproject(NO_DEVICE, 1, _dp(K5), 8, -1, _dp(px), _dp(b3), _u8(v)), _capi.INVALID_ARGUMENT,
             "calico_camera_unproject", "n must be >= 0")
    _message(api, api.camera_project_points(NO_DEVICE, 9, _dp(K5), 8, 4, _dp(b3), _dp(px), _u8(v), None, None), _capi.INVALID_ARGUMENT,
             "calico_camera_project_points", "unknown camera model 9")
    _message(api, api.camera_project_points(NO_DEVICE, 1, _dp(K5), 8, 4, None, _dp(px), _u8(v), None, None), _capi.INVALID_ARGUMENT,
             "calico_camera_project_points", "null input or output buffer")
    _message(api, api.camera_resect(NO_DEVICE, 1, _dp(K5), 8, -1, None, None, None, None, None, None, None, None, None, None, None, None, None),
             _capi.INVALID_ARGUMENT, "calico_camera_resect", "n_frames must be >= 0")
    _message(api, api.camera_calibrate(NO_DEVICE, 1, _dp(K5), 8, None, -1, None, None, None, None, None, None, None, None, None, None, None, None,
                                       None, None), _capi.INVALID_ARGUMENT, "calico_camera_calibrate", "n_frames must be >= 0")
    knots, basis, ctrl, order = ar.trajectory()
    _message(api, api.imu_align(NO_DEVICE, 1, len(knots), _dp(knots), _dp(basis), _dp(ctrl), 0, None, None, 0, None, None, None, None, None, None,
                                None, None, None, None, None, None, None, None), _capi.INVALID_ARGUMENT, "calico_imu_align", "order must be in [2, 8]")
    _message(api, _Fit(api)(device=NO_DEVICE, order=1), _capi.INVALID_ARGUMENT, "calico_fit_spline", "order must be in [2, 8]")


def test_fit_spline_argument_rules_need_no_device(api):
    call = _Fit(api)

    def invalid(st, *words):
        _message(api, st, _capi.INVALID_ARGUMENT, "calico_fit_spline", *words)
    for v in (1, 9):
        invalid(call(order=v), "order")
    for name in ("knots", "basis", "stamps", "data", "ctrl"):
        invalid(call(**{name: None}), "null")
    for v in (0, -1):
        invalid(call(n=v), "n must be > 0")
    invalid(call(n_knots=2 * call.order - 1), "n_knots must be >= 2 order")
    unsorted = call.stamps.copy()
    unsorted[10] = unsorted[8]
    invalid(call(stamps=_dp(unsorted)), "sample stamps are not sorted", "sample 10")
    nan = call.stamps.copy()
    nan[7] = np.nan
    invalid(call(stamps=_dp(nan)), "not finite")
    for at, value in ((49, call.last + 1e-9), (0, call.first - 1e-9)):
        off = call.stamps.copy()
        off[at] = value
        invalid(call(stamps=_dp(off)), "sample stamp %d lies off the valid knots" % at)
    # a bad argument AND a bad device ordinal is still the argument's error
    invalid(call(device=NO_DEVICE, order=1), "order")
    invalid(call(device=NO_DEVICE, stamps=_dp(unsorted)), "not sorted")
    # the trajectory the banded solve cannot hold in LDS: UNIMPLEMENTED, before the device
    for name, spec in fit_ref.TOO_LONG.items():
        c = fit_ref.inputs(spec)
        ctrl = np.zeros((c.n_ctrl, 6))
        st = api.fit_spline(NO_DEVICE, c.order, len(c.knots), _dp(c.knots), _dp(c.basis), len(c.stamps), _dp(c.stamps), _dp(c.data), _dp(ctrl))
        _message(api, st, _capi.UNIMPLEMENTED, "calico_fit_spline", "too long")
    # a valid call: OK on a device; without one it fails loudly, with a message -- and so does a device ordinal out of range
    st = call()
    if st != _capi.OK:
        assert not helpers.has_gpu()
        _message(api, st, _capi.INTERNAL, "calico_fit_spline", "device")
    _message(api, call(device=NO_DEVICE), _capi.INTERNAL, "calico_fit_spline", "device", str(NO_DEVICE))
    _message(api, call(device=-1), _capi.INTERNAL, "calico_fit_spline", "device")


def test_valid_calls_without_a_device_say_so(api):
    px, b3, v = np.zeros((4, 2)), np.ones((4, 3)), np.zeros(4, np.uint8)
    _message(api, api.camera_unproject(NO_DEVICE, 1, _dp(K5), 8, 4, _dp(px), _dp(b3), _u8(v)), _capi.INTERNAL, "calico_camera_unproject",
             "no usable HIP device")
    _message(api, api.camera_project_points(NO_DEVICE, 1, _dp(K5), 8, 4, _dp(b3), _dp(px), _u8(v), None, None), _capi.INTERNAL,
             "calico_camera_project_points", "no usable HIP device")


def test_the_scaffold_is_defined_once():
    csrc = entry.CSRC
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".cpp", ".hip", ".hpp", ".h"))}
    assert sorted(f for f, src in sources.items() if "hipMalloc(" in src) == ["free_call.hpp", "problem_host.hpp"]
    for word in ("struct Buf", "CAMERA_MODEL_SWITCH", "kResectLambda0", "kCalibLambda0", "kAlignLambda0", "ALIGN_TRY"):
        assert [f for f, src in sources.items() if word in src] == [], word
    assert 'extern "C"' not in sources["fit_kernels.hip"]
    assert [f for f, src in sources.items() if re.search(r"#define\s+FREE_TRY\b", src)] == ["free_call.hpp"]
    assert [f for f, src in sources.items() if "no usable HIP device" in src] == ["free_call.hpp"]
    assert [f for f, src in sources.items() if re.search(r"handle_free_error\(\)\s*\{", src)] == ["calico_hip.cpp"]
    # the step rule and its constants: one definition, one kernel that calls it itself (the resection's in-wave loop); the two
    # arrowhead estimators reach it through the one loop decision that the arrowhead header calls, the three alignments ask it themselves
    # and hand the outcome to the dense one-point header's one mapping to their status codes
    assert [f for f, src in sources.items() if "kCostSlack =" in src] == ["lm_rule.hpp"]
    assert sorted(f for f, src in sources.items() if "lm_rule(" in src and f != "lm_rule.hpp") == ["resect_kernels.hip"]
    assert [f for f, src in sources.items() if "lm_loop_decision(" in src and f != "lm_rule.hpp"] == ["arrowhead_dev.hpp", "camalign_kernels.hip"]
    assert [f for f, src in sources.items() if "lm_point_decision(" in src and f != "lm_rule.hpp"] == ["accalign_kernels.hip", "align_kernels.hip"]
    assert [f for f, src in sources.items() if re.search(r"\blm_decide\(", src)] == []
    assert sorted(f for f, src in sources.items() if "point_lm_state(" in src) == ["accalign_kernels.hip", "align_kernels.hip", "camalign_kernels.hip",
                                                                                  "point_lm_dev.hpp"]
    assert [f for f, src in sources.items() if "CALICO_ALIGN_NOT_CONVERGED" in src and f.endswith((".hip", "_dev.hpp"))] == ["point_lm_dev.hpp"]
    # the dense one-point loop: the normal equations, the damping ladder and the undamped inverse are defined once, and no
    # alignment kernel file spells the ladder out
    for word in ("point_lm_normal(", "point_lm_damped_step(", "point_lm_finish("):
        assert [f for f, src in sources.items() if re.search(r"DEV \w+ " + re.escape(word), src)] == ["point_lm_dev.hpp"], word
    assert [f for f, src in sources.items() if "tries < 26" in src] == ["point_lm_dev.hpp"]
    for f in ("align_kernels.hip", "camalign_kernels.hip", "accalign_kernels.hip"):
        assert "point_lm_damped_step(" in sources[f] and "point_lm_finish(" in sources[f] and "kLmLambdaMax" not in sources[f], f
    assert sorted(f for f, src in sources.items() if "lm_control_decide(" in src) == ["arrowhead_dev.hpp", "calib_kernels.hip", "rig_kernels.hip"]
    # the camera-model dispatch: defined in kernels.hpp, used by the three launch files
    assert "with_camera_model(int model" in sources["kernels.hpp"]
    for f in ("camera_kernels.hip", "resect_kernels.hip", "calib_kernels.hip"):
        assert "with_camera_model(model" in sources[f] and not re.search(r"case 7:\s*hipLaunchKernelGGL", sources[f]), f
    # the files by role
    for f in ("chart.cpp", "fit.cpp", "camera.cpp", "imu_align.cpp"):
        assert f in entry.HIP_SOURCES and "getenv" not in sources[f], f
    assert "calico_camera_resect(" in sources["chart.cpp"] and "calico_camera_calibrate(" in sources["chart.cpp"]
    assert "calico_camera_resect(" not in sources["camera.cpp"] and "calico_fit_spline(" in sources["fit.cpp"]
    assert "launch_fit_spline" in sources["kernels.hpp"] and "raise_lds_limit" in sources["fit_kernels.hip"]
    assert "hipFuncSetAttribute" not in sources["fit_kernels.hip"]
