"""Chart resection without a GPU: the two entry points are declared, listed and exported, the default options are the header's,
every argument rule of calico_camera_resect is checked before the device is touched (a rule that reached HIP first would come
back as CALICO_INTERNAL on a machine without one), n_frames == 0 is OK, _capi and the pybind module expose the new names, the
kernels keep their budget, and the shared numpy reference (resect_ref.py) reaches the floor the GPU tests rely on.

Kernel resources as compiled (resect_kernel<1..7>): ScratchSize 0, no VGPR spills, no AGPRs, 174..243 VGPRs, 5120 B of LDS per
workgroup of four waves, occupancy 2 waves per SIMD (the budget the kernel asks for: kResectWavesPerSimd).

The reference's floor, re-measured with the oracle's projection (seven models x 20 frames, 0.1 px noise, started 1e-3 off the
truth): its last Gauss-Newton step is at most 1.4e-13; resect_ref.FLOOR = 1.5e-13."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

import helpers
import resect_ref as rr
from calico_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

K5 = np.array([785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2])


@pytest.fixture(scope="module")
def api():
    entry.build_hip()
    return _capi.CApi(C.CDLL(_capi.hip_library_path()), "calico_")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class _Call:
    """calico_camera_resect on two frames of four pairs, one argument replaced at a time."""

    def __init__(self, api):
        self.api = api
        self.off = np.array([0, 4, 8], np.int64)
        self.px, self.pt = np.zeros((8, 2)), np.zeros((8, 3))
        self.q, self.t, self.rms = np.zeros((2, 4)), np.zeros((2, 3)), np.zeros(2)
        self.used, self.its, self.status = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(2, np.uint8)
        self.qi, self.ti = np.tile([0.0, 0, 0, 1], (2, 1)), np.zeros((2, 3))

    def __call__(self, **kw):
        a = dict(device=0, model=1, k=_dp(K5), nk=8, nf=2, off=self.off.ctypes.data_as(C.POINTER(C.c_int64)), px=_dp(self.px),
                 pt=_dp(self.pt), qi=None, ti=None, o=None, q=_dp(self.q), t=_dp(self.t), rms=_dp(self.rms),
                 used=self.used.ctypes.data_as(C.POINTER(C.c_int32)), its=self.its.ctypes.data_as(C.POINTER(C.c_int32)),
                 status=self.status.ctypes.data_as(C.POINTER(C.c_uint8)), cov=None)
        a.update(kw)
        return self.api.camera_resect(*[a[n] for n in ("device", "model", "k", "nk", "nf", "off", "px", "pt", "qi", "ti", "o", "q", "t",
                                                        "rms", "used", "its", "status", "cov")])


def _invalid(api, st, *words):
    assert st == _capi.INVALID_ARGUMENT, st
    msg = api.last_error(None).decode()
    assert msg.startswith("calico_camera_resect"), msg
    for w in words:
        assert w in msg, (w, msg)


def test_entry_points_are_declared_listed_and_exported(api):
    header = open(os.path.join(ROOT, "include", "calico_hip.h")).read()
    for name in ("default_resection_options", "camera_resect"):
        assert re.search(r"\bcalico_%s\(" % name, header), name
        assert name in _capi.ABI_SYMBOLS
        assert hasattr(api.lib, "calico_" + name) and hasattr(api, name)
    for i, name in enumerate(("OK", "TOO_FEW_POINTS", "NO_START", "NOT_CONVERGED", "DEGENERATE")):
        assert re.search(r"#define CALICO_RESECT_%s %d\b" % (name, i), header), name
        assert getattr(_capi, "RESECT_" + name) == i
    assert "resect_kernels.hip" in entry.HIP_SOURCES
    assert callable(_capi.camera_resect) and callable(_capi.resection_options)
    assert "debug_camera_resect_chunked" in _capi.TEST_SYMBOLS and hasattr(api.lib, "calico_debug_camera_resect_chunked")
    # no new environment switches
    for f in ("resect_kernels.hip", "chart.cpp", "arg_rules.hpp", "free_call.hpp"):
        assert "getenv" not in open(os.path.join(entry.CSRC, f)).read()


def test_default_options(api):
    o = _capi.ResectionOptions()
    api.default_resection_options(C.byref(o))
    assert (o.max_iterations, o.step_tolerance, o.huber_scale, o.min_points) == (30, 1e-11, 0.0, 4)
    api.default_resection_options(None)      # (a null pointer is ignored)
    assert _capi.resection_options(api, huber_scale=2.0).huber_scale == 2.0
    with pytest.raises(TypeError):
        _capi.resection_options(api, no_such_field=1)


def test_argument_rules_need_no_device(api):
    call = _Call(api)
    _invalid(api, call(model=0), "unknown camera model")
    _invalid(api, call(model=8), "unknown camera model")
    _invalid(api, call(nk=7), "8 intrinsics")
    _invalid(api, call(model=3, nk=8), "7 intrinsics")
    _invalid(api, call(k=None), "null intrinsics")
    _invalid(api, call(nf=-1), "n_frames")
    bad = np.array([1, 4, 8], np.int64)
    _invalid(api, call(off=bad.ctypes.data_as(C.POINTER(C.c_int64))), "start at 0")
    bad2 = np.array([0, 5, 4], np.int64)
    _invalid(api, call(off=bad2.ctypes.data_as(C.POINTER(C.c_int64))), "decrease")
    for name in ("off", "q", "t", "rms", "used", "its", "status", "px", "pt"):
        _invalid(api, call(**{name: None}), "null")
    _invalid(api, call(qi=_dp(call.qi)), "q_init and t_init")
    _invalid(api, call(ti=_dp(call.ti)), "q_init and t_init")

    def opts(**kw):
        return C.byref(_capi.resection_options(api, **kw))
    for v in (0.0, -1e-11, float("inf"), float("nan")):
        _invalid(api, call(o=opts(step_tolerance=v)), "step_tolerance")
    for v in (0, -3):
        _invalid(api, call(o=opts(max_iterations=v)), "max_iterations")
    for v in (-1.0, float("inf"), float("nan")):
        _invalid(api, call(o=opts(huber_scale=v)), "huber_scale")
    for v in (3, 0, -1):
        _invalid(api, call(o=opts(min_points=v)), "min_points")
    # the rules come before the device: a bad argument AND a bad device ordinal is still the argument's error
    _invalid(api, call(device=10 ** 6, nk=7), "intrinsics")
    _invalid(api, api.debug_camera_resect_chunked(0, 1, _dp(K5), 8, 0, None, None, None, None, None, None, None, None, None, None, None,
                                                  None, None, 0), "chunk")
    # n_frames == 0 touches nothing
    assert call(nf=0, off=None, px=None, pt=None, q=None, t=None, rms=None, used=None, its=None, status=None) == _capi.OK
    assert call(device=10 ** 6, nf=0) == _capi.OK
    if not helpers.has_gpu():       # a valid call without a device fails loudly, with a message
        assert call() == _capi.INTERNAL
        assert "device" in api.last_error(None).decode()


def test_wrapper_checks_its_shapes(api):
    with pytest.raises(ValueError):
        _capi.camera_resect(api, 1, K5, [0, 4], np.zeros((5, 2)), np.zeros((5, 3)))
    r = _capi.camera_resect(api, 1, K5, [0], np.zeros((0, 2)), np.zeros((0, 3)), covariance=True)
    assert r.q.shape == (0, 4) and r.cov.shape == (0, 6, 6) and r.status.shape == (0,)


def test_python_surfaces_expose_the_new_names():
    entry.build_hip()
    entry.build_python_module()
    from calico_amd import calico
    assert hasattr(calico.Camera, "EstimateChartPoses") and callable(calico.InitializePoses)
    camera = calico.Camera()
    with pytest.raises(RuntimeError, match="Error: Camera model has not been set"):
        camera.EstimateChartPoses([], {})
    camera.SetModel(calico.CameraIntrinsicsModel.kKannalaBrandt)
    with pytest.raises(RuntimeError, match="not in the model definition"):
        camera.EstimateChartPoses([{3: np.zeros(2)}], {0: np.zeros(3)})
    with pytest.raises(TypeError):
        camera.EstimateChartPoses([], {}, options={"no_such_option": 1})
    with pytest.raises(RuntimeError, match="min_points"):      # the library's argument rules, reached without a device
        camera.EstimateChartPoses([], {}, options={"min_points": 3})
    out = camera.EstimateChartPoses([], {}, covariance=True)      # no frames: OK, empty arrays
    assert out["q"].shape == (0, 4) and out["cov"].shape == (0, 6, 6)
    R, t, ok = calico.InitializePoses(camera, [], {})
    assert R == [] and t == [] and ok.shape == (0,)


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_resect_kernels_resource_budget():
    """No scratch, no spills, more than one wave per SIMD, the small systems in LDS (figures: the module's docstring)."""
    res = helpers.kernel_resources("resect_kernels.hip")
    mine = {k: v for k, v in res.items() if "resect_kernel" in k}
    assert len(mine) == 7 and len(res) == 7, sorted(res)
    for k, v in mine.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        assert v["Occupancy"] >= 2 and v["AGPRs"] == 0, (k, v)
        assert v["LDS Size"] == 4 * 160 * 8, (k, v)


def test_reference_reaches_its_floor():
    """The reference from a start 1e-3 off the truth and from the truth ends at the same pose, and its last step is below FLOOR
    (three frames of every model here; the figure in the docstring is over all twenty)."""
    worst = 0.0
    for model in rr.MODELS:
        k, off, px, pt, poses = rr.fixture(model, 0.1)
        for f in (0, 7, 19):
            s = slice(off[f], off[f + 1])
            R, t = poses[f]
            Ra, ta, last_a, _ = rr.refine(model, k, rr.exp_so3([1e-3, -2e-3, 1e-3]) @ R, t + [1e-3, 2e-3, -1e-3], pt[s], px[s])
            Rb, tb, last_b, _ = rr.refine(model, k, R, t, pt[s], px[s])
            worst = max(worst, last_a, last_b)
            assert rr.pose_distance(Ra, ta, Rb, tb) <= 2e-13, (model, f)
            assert np.abs(rr.gn_step(model, k, Ra, ta, pt[s], px[s])).max() <= rr.FLOOR      # (the criterion at its own pose)
    print("reference floor", worst)
    assert worst <= rr.FLOOR



def test_boundary_cases_have_the_properties_the_gpu_tests_rely_on():
    """resect_ref.boundary_case, from the reference alone (lm_rule_ref's checks say what is held): `lost` is rejected until the
    damping keeps the extra point inside the validity boundary, `invalid` never has it, `joins` gains it at the first candidate,
    which only the comparison over the pairs in common accepts. And a start that puts the chart behind a pinhole camera has no
    valid pair."""
    import lm_rule_ref as lm
    same = lambda p: p      # noqa: E731  (the point of the resection's loop is the frame's pose)
    c = rr.boundary_case("lost")
    first = lm.check_lost(lm.resect_loop(6, c.k, *c.start, c.points, c.pixels, 8), same, c.start, c.points[-1], -1)
    c = rr.boundary_case("joins")
    lm.check_joins(lm.resect_loop(6, c.k, *c.start, c.points, c.pixels, 1), same, c.start, c.points[-1], -1)
    c = rr.boundary_case("invalid")
    lm.check_invalid(lm.resect_loop(6, c.k, *c.start, c.points, c.pixels, 30), same, c.start, c.points[-1], -1)
    print("lost: the first accepted step is step", first)
    k, off, px, pt, poses = rr.fixture(1, 0.1)
    for f in (0, 7, 19):
        _, ok = rr.project(1, k, *rr.behind(poses[f]), pt[off[f]:off[f + 1]])
        assert not ok.any()
