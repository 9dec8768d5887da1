"""Rig calibration without a GPU: the entry points are declared, listed and exported, the default options are the header's,
every argument rule of calico_rig_calibrate is checked before the device is touched, n_views == 0 is OK with
CALICO_RIG_TOO_FEW_VIEWS, and the shared numpy reference (rig_ref.py) is measured on every fixture the GPU tests use: its FLOOR
and its noise-free distance to the truth. The committed figures (rig_ref.FLOOR, rig_ref.REF_FREE) are this machine's; the floor
is rounding noise, so another CPU's libm and BLAS move it: the test holds the re-measured values to twice the committed ones
(calib_ref's rule) and prints them.
Measured: the reference's first LM step from h = 2e-6 against h = 1e-6 differences, and the same step without the fill between
the cameras: standard (a quarter of the perturbation) 4.1e-12 / 3.4e-3, wide 1.7e-11 / 7.5e-2."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import helpers
import rig_ref as gr
from calico_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

K1 = np.array([785, 640, 400, -3.149e-1, 1.069e-1, 1.616e-4, 1.141e-4, -1.853e-2])
K6 = np.array([500.0, 640, 400, 0.6])
I64, I32, U8 = C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def api():
    entry.build_hip()
    return _capi.CApi(C.CDLL(_capi.hip_library_path()), "calico_")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class _Call:
    """calico_rig_calibrate on two cameras (models 1 and 6), three frames and six views of four pairs, one argument replaced
    at a time."""

    ORDER = ("device", "nc", "models", "koff", "k", "nf", "nv", "vc", "vf", "off", "px", "pt", "qci", "tci", "qfi", "tfi", "o", "qc", "tc",
             "cs", "qf", "tf", "fs", "rms", "used", "vs", "cov", "summary")

    def __init__(self, api):
        self.api = api
        self.models = np.array([1, 6], np.int32)
        self.koff = np.array([0, 8, 12], np.int64)
        self.k = np.concatenate([K1, K6])
        self.vc = np.array([0, 1, 0, 1, 0, 1], np.int32)
        self.vf = np.array([0, 0, 1, 1, 2, 2], np.int64)
        self.off = np.arange(7, dtype=np.int64) * 4
        self.px, self.pt = np.zeros((24, 2)), np.zeros((24, 3))
        self.qc, self.tc, self.cs = np.zeros((2, 4)), np.zeros((2, 3)), np.zeros(2, np.uint8)
        self.qf, self.tf, self.fs = np.zeros((3, 4)), np.zeros((3, 3)), np.zeros(3, np.uint8)
        self.rms, self.used, self.vs = np.zeros(6), np.zeros(6, np.int32), np.zeros(6, np.uint8)
        self.qci, self.tci = np.tile([0.0, 0, 0, 1], (2, 1)), np.zeros((2, 3))
        self.qfi, self.tfi = np.tile([0.0, 0, 0, 1], (3, 1)), np.zeros((3, 3))
        self.summary = _capi.RigSummary()

    def __call__(self, **kw):
        a = dict(device=0, nc=2, models=self.models.ctypes.data_as(I32), koff=self.koff.ctypes.data_as(I64), k=_dp(self.k), nf=3, nv=6,
                 vc=self.vc.ctypes.data_as(I32), vf=self.vf.ctypes.data_as(I64), off=self.off.ctypes.data_as(I64), px=_dp(self.px),
                 pt=_dp(self.pt), qci=None, tci=None, qfi=None, tfi=None, o=None, qc=_dp(self.qc), tc=_dp(self.tc),
                 cs=self.cs.ctypes.data_as(U8), qf=_dp(self.qf), tf=_dp(self.tf), fs=self.fs.ctypes.data_as(U8), rms=_dp(self.rms),
                 used=self.used.ctypes.data_as(I32), vs=self.vs.ctypes.data_as(U8), cov=None, summary=C.byref(self.summary))
        a.update(kw)
        return self.api.rig_calibrate(*[a[n] for n in self.ORDER])


def _invalid(api, st, *words):
    assert st == _capi.INVALID_ARGUMENT, st
    msg = api.last_error(None).decode()
    assert msg.startswith("calico_rig_calibrate"), msg
    for w in words:
        assert w in msg, (w, msg)


def test_entry_points_are_declared_listed_and_exported(api):
    header = open(os.path.join(ROOT, "include", "calico_hip.h")).read()
    for name in ("default_rig_options", "rig_calibrate"):
        assert re.search(r"\bcalico_%s\(" % name, header), name
        assert name in _capi.ABI_SYMBOLS
        assert hasattr(api.lib, "calico_" + name) and hasattr(api, name)
    for prefix, names in (("", ("OK", "TOO_FEW_VIEWS", "NOT_CONVERGED", "DEGENERATE")), ("CAMERA_", ("OK", "REFERENCE", "UNCONNECTED")),
                          ("FRAME_", ("OK", "NO_VIEW", "NOT_POSITIVE_DEFINITE"))):
        for i, name in enumerate(names):
            assert re.search(r"#define CALICO_RIG_%s%s %d\b" % (prefix, name, i), header), name
            assert getattr(_capi, "RIG_" + prefix + name) == i
    assert re.search(r"#define CALICO_RIG_MAX_CAMERAS 8\b", header) and _capi.RIG_MAX_CAMERAS == 8
    assert "rig_kernels.hip" in entry.HIP_SOURCES and "rig.cpp" in entry.HIP_SOURCES
    assert callable(_capi.rig_calibrate) and callable(_capi.rig_options)
    for f in ("rig_kernels.hip", "rig.cpp"):      # no environment switches; the shared scaffold, not copies of it
        src = open(os.path.join(entry.CSRC, f)).read()
        assert "getenv" not in src and "hipMalloc(" not in src, f
    src = open(os.path.join(entry.CSRC, "rig_kernels.hip")).read()
    # the step rule is lm_rule.hpp's: the decide kernel asks the arrowhead header's decision, which asks the loop decision, which
    # asks lm_rule; no constants of its own. The shared device code is one header, not a copy.
    rule = open(os.path.join(entry.CSRC, "lm_rule.hpp")).read()
    shared = open(os.path.join(entry.CSRC, "arrowhead_dev.hpp")).read()
    assert '#include "arrowhead_dev.hpp"' in src and '#include "resect_dev.hpp"' in shared
    assert "lds_chol(double*" not in src and "lds_chol(double*" not in shared and "lm_control_decide(" in src
    assert "= lm_loop_decision(" in shared
    assert 0 <= rule.find("LmLoopStep lm_loop_decision(") < rule.rfind("= lm_rule(") and "1e-4" not in src and "kCostSlack" not in src
    assert "1e-4" not in shared and "kCostSlack" not in shared
    assert "mfma_f64_16x16x4f64" in src and not re.search(r"\batomic[A-Z_a-z]*\(", src + shared)


def test_default_options(api):
    o = _capi.RigOptions()
    api.default_rig_options(C.byref(o))
    assert (o.max_iterations, o.step_tolerance, o.huber_scale, o.min_points, o.min_shared_frames, o.reference_camera) == (50, 1e-10, 0.0, 4, 3, 0)
    api.default_rig_options(None)      # (a null pointer is ignored)
    assert _capi.rig_options(api, min_shared_frames=5).min_shared_frames == 5
    with pytest.raises(TypeError):
        _capi.rig_options(api, no_such_field=1)


def test_argument_rules_need_no_device(api):
    call = _Call(api)
    _invalid(api, call(nc=0), "n_cameras")
    _invalid(api, call(nc=9), "n_cameras")
    for bad_model in (0, 8):
        m = np.array([1, bad_model], np.int32)
        _invalid(api, call(models=m.ctypes.data_as(I32)), "unknown camera model")
    koff = np.array([0, 8, 13], np.int64)
    _invalid(api, call(koff=koff.ctypes.data_as(I64)), "4 intrinsics")
    koff = np.array([1, 9, 13], np.int64)
    _invalid(api, call(koff=koff.ctypes.data_as(I64)), "start at 0")
    _invalid(api, call(nf=-1), "n_frames")
    _invalid(api, call(nv=-1), "n_views")
    for cam in (-1, 2):
        vc = np.array([0, 1, 0, 1, 0, cam], np.int32)
        _invalid(api, call(vc=vc.ctypes.data_as(I32)), "names camera")
    for frame in (-1, 3):
        vf = np.array([0, 0, 1, 1, 2, frame], np.int64)
        _invalid(api, call(vf=vf.ctypes.data_as(I64)), "names frame")
    vf = np.array([0, 0, 1, 1, 2, 1], np.int64)      # camera 1 twice in frame 1
    _invalid(api, call(vf=vf.ctypes.data_as(I64)), "two views of frame 1")
    off = np.array([1, 4, 8, 12, 16, 20, 24], np.int64)
    _invalid(api, call(off=off.ctypes.data_as(I64)), "start at 0")
    off = np.array([0, 4, 8, 7, 16, 20, 24], np.int64)
    _invalid(api, call(off=off.ctypes.data_as(I64)), "decrease")
    for name in ("models", "koff", "k", "vc", "vf", "off", "px", "pt", "qc", "tc", "cs", "qf", "tf", "fs", "rms", "used", "vs", "summary"):
        _invalid(api, call(**{name: None}), "null")
    _invalid(api, call(qci=_dp(call.qci)), "q_init and t_init")
    _invalid(api, call(tci=_dp(call.tci)), "q_init and t_init")
    _invalid(api, call(qci=_dp(call.qci), tci=_dp(call.tci), qfi=_dp(call.qfi)), "q_frame_init and t_frame_init")
    _invalid(api, call(qci=_dp(call.qci), tci=_dp(call.tci), tfi=_dp(call.tfi)), "q_frame_init and t_frame_init")
    _invalid(api, call(qfi=_dp(call.qfi), tfi=_dp(call.tfi)), "needs a start of the cameras")

    def opts(**kw):
        return C.byref(_capi.rig_options(api, **kw))
    for v in (-1, 2):
        _invalid(api, call(o=opts(reference_camera=v)), "reference_camera")
    for v in (0, -2):
        _invalid(api, call(o=opts(min_shared_frames=v)), "min_shared_frames")
    for v in (3, 0, -1):
        _invalid(api, call(o=opts(min_points=v)), "min_points")
    for v in (0.0, -1e-11, float("inf"), float("nan")):
        _invalid(api, call(o=opts(step_tolerance=v)), "step_tolerance")
    for v in (0, -3):
        _invalid(api, call(o=opts(max_iterations=v)), "max_iterations")
    for v in (-1.0, float("inf"), float("nan")):
        _invalid(api, call(o=opts(huber_scale=v)), "huber_scale")
    # the rules come before the device: a bad argument AND a bad device ordinal is still the argument's error
    _invalid(api, call(device=10 ** 6, nc=9), "n_cameras")
    if not helpers.has_gpu():       # a valid call without a device fails loudly, with a message
        assert call() == _capi.INTERNAL
        assert "device" in api.last_error(None).decode()


def test_no_views_is_ok_and_touches_no_device(api):
    call = _Call(api)
    call.qc[:], call.qf[:], call.cs[:], call.fs[:] = 7.0, 7.0, 9, 9
    assert call(device=10 ** 6, nv=0, vc=None, vf=None, off=None, px=None, pt=None, rms=None, used=None, vs=None) == _capi.OK
    assert call.summary.status == _capi.RIG_TOO_FEW_VIEWS and call.summary.iterations == 0 and call.summary.views_used == 0
    assert np.array_equal(call.qc, np.tile([0.0, 0, 0, 1], (2, 1))) and np.array_equal(call.qf, np.tile([0.0, 0, 0, 1], (3, 1)))
    assert call.cs.tolist() == [_capi.RIG_CAMERA_REFERENCE, _capi.RIG_CAMERA_UNCONNECTED] and call.fs.tolist() == [_capi.RIG_FRAME_NO_VIEW] * 3
    # the starts come back: the reference camera's bit for bit, as given
    qci = np.array([[0.0, 0, 0, 2.0], [0.0, 0.6, 0, 0.8]])
    tci = np.array([[1.0, 2, 3], [4.0, 5, 6]])
    assert call(nv=0, qci=_dp(qci), tci=_dp(tci)) == _capi.OK
    assert np.array_equal(call.qc, qci) and np.array_equal(call.tc, tci)
    r = _capi.rig_calibrate(api, [1, 6], [K1, K6], 0, [], [], [0], np.zeros((0, 2)), np.zeros((0, 3)), covariance=True)
    assert r.status == _capi.RIG_TOO_FEW_VIEWS and r.q_frame.shape == (0, 4) and r.cov.shape == (12, 12) and r.view_status.shape == (0,)
    with pytest.raises(ValueError):
        _capi.rig_calibrate(api, [1, 6], [K1], 0, [], [], [0], np.zeros((0, 2)), np.zeros((0, 3)))
    with pytest.raises(ValueError):
        _capi.rig_calibrate(api, [1, 6], [K1, K6], 1, [0], [0], [0, 4], np.zeros((5, 2)), np.zeros((5, 3)))


@pytest.mark.parametrize("name", sorted(gr.FIXTURES))
def test_reference_floor_and_noise_free_distance(name):
    """The reference from the truth perturbed by 0.02 N(0, 1): converges, six more undamped Gauss-Newton steps stay within twice
    the committed FLOOR, and on noise-free data it ends within twice REF_FREE of the truth."""
    rig = gr.FIXTURES[name](0.1)
    start = gr.perturbed_start(rig)
    cams, frames, last, accepted, converged = gr.refine(rig, gr.poses_of(*start[:2]), gr.poses_of(*start[2:]))
    assert converged and accepted <= 12, (accepted, last)
    floor = 0.0
    for _ in range(6):
        d, s = gr.gn(rig, cams, frames)
        floor = max(floor, s)
        cams, frames = gr.apply(rig, cams, frames, d)
    print("fixture", name, "FLOOR", floor, "accepted steps", accepted)
    assert floor <= 2 * gr.FLOOR[name]
    rig = gr.FIXTURES[name](0.0)
    start = gr.perturbed_start(rig)
    cams, frames, last, accepted, converged = gr.refine(rig, gr.poses_of(*start[:2]), gr.poses_of(*start[2:]))
    free = gr.distance(cams, frames, rig)
    print("fixture", name, "noise-free distance to the truth", free, "accepted steps", accepted)
    assert converged and free <= 2 * gr.REF_FREE[name]


@pytest.mark.parametrize("name", ("standard", "wide"))
def test_a_step_without_the_fill_between_cameras_is_far_from_the_true_step(name):
    """What keeps the step tests' bound (10 floors, tests/test_gpu_chart_steps.py) from hiding what they are for: the
    reference's first step is accepted, and the same step with the camera-to-camera blocks of the Schur complement zeroed ends at
    least 1000 floors away (floor: the first step from h = 2e-6 against h = 1e-6 differences). From perturbed_start the
    standard fixture's first step is REJECTED (the step tests pin that as well); the condition is held on the start the step
    tests call `standard-near`, a quarter of the perturbation."""
    import lm_rule_ref as lm
    import resect_ref as rr
    rig = gr.FIXTURES[name](0.1)
    if name == "standard":
        far = gr.perturbed_start(rig)
        assert lm.rig_loop(rig, gr.poses_of(*far[:2]), gr.poses_of(*far[2:]), 1).log == [False]
    start = gr.perturbed_start(rig, scale=0.005) if name == "standard" else gr.perturbed_start(rig)
    c0, f0 = gr.poses_of(*start[:2]), gr.poses_of(*start[2:])
    true, other, mutant = lm.rig_loop(rig, c0, f0, 1), lm.rig_loop(rig, c0, f0, 1, h=2e-6), lm.rig_loop(rig, c0, f0, 1, drop_fill=True)

    def dist(a, b):
        return max(rr.pose_distance(*p, *q) for p, q in zip(a.point[0] + a.point[1], b.point[0] + b.point[1]))
    floor, moved = dist(true, other), dist(true, mutant)
    print("fixture", name, "floor", floor, "the mutant's distance", moved, "the mutant's step accepted:", mutant.log)
    assert true.log == other.log == [True] and true.lam == 1e-5
    assert floor > 0 and moved >= 1000 * floor


def test_boundary_rigs_have_the_properties_the_gpu_tests_rely_on():
    """rig_ref.boundary_rig, from the reference alone (lm_rule_ref's checks say what is held). Camera 0 is the reference camera
    at the rig's origin: its T_camera_chart is the rig frame's pose."""
    import lm_rule_ref as lm
    f = gr.BOUNDARY_FRAME
    pose = lambda p: p[1][f]      # noqa: E731
    for kind, check, steps in (("lost", lm.check_lost, 8), ("joins", lm.check_joins, 1), ("invalid", lm.check_invalid, 50)):
        rig, start, v = gr.boundary_rig(kind)
        assert rig.view_camera[v] == 0 and rig.view_frame[v] == f and rig.view_offsets[v + 1] - rig.view_offsets[v] == 37
        assert np.array_equal(rig.cams[0][0], np.eye(3)) and not rig.cams[0][1].any()
        at = rig.view_offsets[v + 1] - 1
        point = (gr.poses_of(*start[:2]), gr.poses_of(*start[2:]))
        loop = lm.rig_loop(rig, *point, steps)
        print(kind, "accepted", loop.log, "lambda", loop.lam, "first accepted step", check(loop, pose, point, rig.points[at], at))
