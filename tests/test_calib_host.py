"""Intrinsic calibration without a GPU: the entry points are declared, listed and exported, the default options are the
header's, every argument rule of calico_camera_calibrate is checked before the device is touched, n_frames == 0 is OK, the
Python surfaces expose the new names, utils.InitialIntrinsics keeps its on-axis rule against the oracle's projection, and the
shared numpy reference (calib_ref.py) is measured: its FLOOR, its noise-free distance to the truth, and its convergence from
InitialIntrinsics.

Measured here (seven models, resect_ref.fixture: 20 frames x 36 points, the standard start):
  FLOOR -- the largest s of six undamped Gauss-Newton steps of the reference at and after its own result, 0.1 px noise --
    model 1: 2.4e-12   2: 3.3e-11   3: 1.5e-10   4: 1.9e-10   5: 8.1e-12   6: 2.7e-12   7: 4.9e-10
  the reference's own distance to the truth on noise-free data (s-scaled for the intrinsics, pose_distance for the poses):
    model 1: 3.4e-15   2: 3.2e-15   3: 2.0e-15   4: 3.6e-15   5: 2.4e-15   6: 4.0e-16   7: 1.4e-15
  accepted steps of the reference from the standard start: 5 to 12; rms at 0.1 px noise 0.132 to 0.138 px.
  FLOOR_LONG (resect_ref.long_fixture: 137 frames x 12 points, long_start) -- model 1: 6.2e-10   6: 5.9e-12
  the reference's first LM step from h = 2e-6 against h = 1e-6 differences, and the same step without lambda diag C:
    model 1: 1.1e-11 / 9.8e-3   2: 4.9e-10 / 5.6e-2   4: 2.7e-11 / 3.2e-2
The committed figures are this machine's. The floor is rounding noise, so another CPU's libm and BLAS move it: the test holds the
re-measured values to twice the committed ones and prints them."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import calib_ref as cr
import camera_ref
import helpers
import resect_ref as rr
from calico_amd import _capi, synthetic as syn

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
    """calico_camera_calibrate on three frames of four pairs, one argument replaced at a time."""

    def __init__(self, api):
        self.api = api
        self.off = np.array([0, 4, 8, 12], np.int64)
        self.px, self.pt = np.zeros((12, 2)), np.zeros((12, 3))
        self.k, self.q, self.t, self.rms = np.zeros(8), np.zeros((3, 4)), np.zeros((3, 3)), np.zeros(3)
        self.used, self.status = np.zeros(3, np.int32), np.zeros(3, np.uint8)
        self.qi, self.ti = np.tile([0.0, 0, 0, 1], (3, 1)), np.zeros((3, 3))
        self.summary = _capi.CalibrationSummary()

    def __call__(self, **kw):
        a = dict(device=0, model=1, k=_dp(K5), nk=8, mask=None, nf=3, off=self.off.ctypes.data_as(C.POINTER(C.c_int64)), px=_dp(self.px),
                 pt=_dp(self.pt), qi=None, ti=None, o=None, ko=_dp(self.k), q=_dp(self.q), t=_dp(self.t), rms=_dp(self.rms),
                 used=self.used.ctypes.data_as(C.POINTER(C.c_int32)), status=self.status.ctypes.data_as(C.POINTER(C.c_uint8)), cov=None,
                 summary=C.byref(self.summary))
        a.update(kw)
        return self.api.camera_calibrate(*[a[n] for n in ("device", "model", "k", "nk", "mask", "nf", "off", "px", "pt", "qi", "ti", "o", "ko",
                                                           "q", "t", "rms", "used", "status", "cov", "summary")])


def _invalid(api, st, *words):
    assert st == _capi.INVALID_ARGUMENT, st
    msg = api.last_error(None).decode()
    assert msg.startswith("calico_camera_calibrate"), msg
    for w in words:
        assert w in msg, (w, msg)


def test_entry_points_are_declared_listed_and_exported(api):
    header = open(os.path.join(ROOT, "include", "calico_hip.h")).read()
    for name in ("default_calibration_options", "camera_calibrate"):
        assert re.search(r"\bcalico_%s\(" % name, header), name
        assert name in _capi.ABI_SYMBOLS
        assert hasattr(api.lib, "calico_" + name) and hasattr(api, name)
    for i, name in enumerate(("OK", "TOO_FEW_FRAMES", "NOT_CONVERGED", "DEGENERATE")):
        assert re.search(r"#define CALICO_CALIB_%s %d\b" % (name, i), header), name
        assert getattr(_capi, "CALIB_" + name) == i
    assert re.search(r"#define CALICO_RESECT_NOT_POSITIVE_DEFINITE 5\b", header) and _capi.RESECT_NOT_POSITIVE_DEFINITE == 5
    assert "calib_kernels.hip" in entry.HIP_SOURCES
    assert callable(_capi.camera_calibrate) and callable(_capi.calibration_options)
    for f in ("calib_kernels.hip", "resect_dev.hpp"):      # no new environment switches
        assert "getenv" not in open(os.path.join(entry.CSRC, f)).read()
    # the helpers the per-frame LM kernels share are in one header, not copied: resect_dev.hpp, which all three include through the
    # arrowhead header
    for f, header in (("calib_kernels.hip", "arrowhead_dev.hpp"), ("resect_kernels.hip", "arrowhead_dev.hpp"), ("arrowhead_dev.hpp", "resect_dev.hpp")):
        src = open(os.path.join(entry.CSRC, f)).read()
        assert '#include "%s"' % header in src and "lds_chol(double*" not in src and "getenv" not in src, f


def test_default_options(api):
    o = _capi.CalibrationOptions()
    api.default_calibration_options(C.byref(o))
    assert (o.max_iterations, o.step_tolerance, o.huber_scale, o.min_points) == (50, 1e-10, 0.0, 4)
    api.default_calibration_options(None)      # (a null pointer is ignored)
    assert _capi.calibration_options(api, huber_scale=2.0).huber_scale == 2.0
    with pytest.raises(TypeError):
        _capi.calibration_options(api, no_such_field=1)


def test_argument_rules_need_no_device(api):
    call = _Call(api)
    _invalid(api, call(model=0), "unknown camera model")
    _invalid(api, call(model=8), "unknown camera model")
    _invalid(api, call(nk=7), "8 intrinsics")
    _invalid(api, call(model=3, nk=8), "7 intrinsics")
    _invalid(api, call(k=None), "null intrinsics")
    _invalid(api, call(nf=-1), "n_frames")
    bad = np.array([1, 4, 8, 12], np.int64)
    _invalid(api, call(off=bad.ctypes.data_as(C.POINTER(C.c_int64))), "start at 0")
    bad2 = np.array([0, 5, 4, 12], np.int64)
    _invalid(api, call(off=bad2.ctypes.data_as(C.POINTER(C.c_int64))), "decrease")
    for name in ("off", "ko", "q", "t", "rms", "used", "status", "px", "pt", "summary"):
        _invalid(api, call(**{name: None}), "null")
    _invalid(api, call(qi=_dp(call.qi)), "q_init and t_init")
    _invalid(api, call(ti=_dp(call.ti)), "q_init and t_init")
    none_free = np.zeros(8, np.uint8)
    _invalid(api, call(mask=none_free.ctypes.data_as(C.POINTER(C.c_uint8))), "free_mask")

    def opts(**kw):
        return C.byref(_capi.calibration_options(api, **kw))
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
    # n_frames == 0 touches nothing
    assert call(nf=0, off=None, px=None, pt=None, ko=None, q=None, t=None, rms=None, used=None, status=None, summary=None) == _capi.OK
    assert call(device=10 ** 6, nf=0) == _capi.OK
    if not helpers.has_gpu():       # a valid call without a device fails loudly, with a message
        assert call() == _capi.INTERNAL
        assert "device" in api.last_error(None).decode()


def test_wrapper_checks_its_shapes(api):
    with pytest.raises(ValueError):
        _capi.camera_calibrate(api, 1, K5, [0, 4], np.zeros((5, 2)), np.zeros((5, 3)))
    with pytest.raises(ValueError):
        _capi.camera_calibrate(api, 1, K5, [0, 4], np.zeros((4, 2)), np.zeros((4, 3)), free_mask=[1, 1])
    r = _capi.camera_calibrate(api, 1, K5, [0], np.zeros((0, 2)), np.zeros((0, 3)), covariance=True)
    assert r.q.shape == (0, 4) and r.cov.shape == (8, 8) and r.frame_status.shape == (0,) and np.array_equal(r.intrinsics, K5)


def test_python_surfaces_expose_the_new_names():
    entry.build_hip()
    entry.build_python_module()
    from calico_amd import calico
    assert hasattr(calico.Camera, "CalibrateIntrinsics") and hasattr(calico.CameraModel, "CalibrateFromChart")
    assert callable(calico.InitialIntrinsics) and callable(calico.InitializeIntrinsicsAndPoses)
    camera = calico.Camera()
    with pytest.raises(RuntimeError, match="Error: Camera model has not been set"):
        camera.CalibrateIntrinsics([], {})
    camera.SetModel(calico.CameraIntrinsicsModel.kKannalaBrandt)
    with pytest.raises(RuntimeError, match="not in the model definition"):
        camera.CalibrateIntrinsics([{3: np.zeros(2)}], {0: np.zeros(3)})
    with pytest.raises(TypeError):
        camera.CalibrateIntrinsics([], {}, options={"no_such_option": 1})
    with pytest.raises(RuntimeError, match="min_points"):      # the library's argument rules, reached without a device
        camera.CalibrateIntrinsics([], {}, options={"min_points": 3})
    with pytest.raises(RuntimeError, match="free_mask"):
        camera.CalibrateIntrinsics([], {}, free_mask=[0] * 7)
    out = camera.CalibrateIntrinsics([], {}, covariance=True)      # no frames: OK, empty arrays
    assert out["q"].shape == (0, 4) and out["cov"].shape == (7, 7) and out["status"] == 0
    out = calico.CameraModel.CalibrateFromChart(calico.CameraIntrinsicsModel.kOpenCv5, K5, [0], np.zeros((0, 2)), np.zeros((0, 3)))
    assert np.array_equal(out["intrinsics"], K5) and out["frame_status"].shape == (0,)
    with pytest.raises(ValueError):
        calico.InitialIntrinsics(0, [500, 500, 0, 640, 400])


@pytest.mark.parametrize("model", cr.MODELS)
def test_initial_intrinsics_agree_with_the_pinhole_on_the_axis(model):
    """The oracle's projection at InitialIntrinsics(model, pinhole): the optical axis lands on the principal point, and the
    derivative of the pixel in x / z and y / z there is the pinhole's focal length (central differences, h = 1e-6: rounding
    1e-10; ExtendedUnifiedCamera's |x| under the root makes its difference quotient first order in h: alpha beta h / 4)."""
    from calico_amd.calico import utils
    fp, cx, cy = 512.5, 631.0, 407.0
    k = utils.InitialIntrinsics(model, [fp, fp, 0.0, cx, cy])
    assert len(k) == cr.NUM_PARAMS[model] and k[1] == cx and k[2] == cy
    h = 1e-6
    pts = np.array([[0, 0, 1.0], [h, 0, 1], [-h, 0, 1], [0, h, 1], [0, -h, 1], [0, 0, 2.5]])
    px, ok = camera_ref.oracle_project(model, k, pts)
    assert ok.all()
    assert np.abs(px[0] - [cx, cy]).max() <= 1e-12 * cx and np.abs(px[5] - [cx, cy]).max() <= 1e-12 * cx
    J = np.array([(px[1] - px[2]) / (2 * h), (px[3] - px[4]) / (2 * h)]).T
    print("model", model, "on-axis derivative", J.tolist())
    assert np.abs(J - fp * np.eye(2)).max() <= 1e-6 * fp
    # the neutral distortion is the pinhole off the axis too
    if model in (1, 2, 4, 6):
        far, ok = camera_ref.oracle_project(model, k, np.array([[0.3, -0.2, 1.0]]))
        assert ok.all() and np.abs(far[0] - [cx + 0.3 * fp, cy - 0.2 * fp]).max() <= 1e-10 * fp


def _as_arrays(poses):
    q = np.array([rr.quat_of(R) for R, _ in poses])
    return q, np.array([t for _, t in poses])


@pytest.mark.parametrize("model", cr.MODELS)
def test_reference_floor_and_noise_free_distance(model):
    """The reference from the standard start: converges within 12 accepted steps, six more undamped Gauss-Newton steps stay within
    twice the committed FLOOR (the figures in this module's docstring and beside calib_ref.FLOOR are this test's), and on
    noise-free data it ends within twice REF_FREE of the truth."""
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    k0, q0, t0 = cr.standard_start(model, 0.1)
    kr, pr, last, accepted, converged = cr.refine(model, k0, cr.start_poses(q0, t0), off, pt, px)
    assert converged and accepted <= 12, (accepted, last)
    floor = 0.0
    for _ in range(6):
        dk, d, s = cr.gn(model, kr, pr, off, pt, px)
        floor = max(floor, s)
        kr, pr = cr.apply(kr, pr, dk, d)
    rms, n = cr.rms_at(model, kr, *_as_arrays(pr), off, pt, px)
    print("model", model, "FLOOR", floor, "accepted steps", accepted, "rms", rms)
    assert n == 720 and 0.12 <= rms <= 0.15
    assert floor <= 2 * cr.FLOOR[model]
    k, off, px, pt, poses = rr.fixture(model, 0.0)
    k0, q0, t0 = cr.standard_start(model, 0.0)
    kr, pr, last, accepted, converged = cr.refine(model, k0, cr.start_poses(q0, t0), off, pt, px)
    free = max(cr.intrinsics_distance(kr, k), cr.poses_distance(pr, poses))
    print("model", model, "noise-free distance to the truth", free, "accepted steps", accepted)
    assert converged and free <= 2 * cr.REF_FREE[model]


def test_reference_converges_from_initial_intrinsics_for_kannala_brandt():
    """Reference only: from InitialIntrinsics of the true pinhole part (zero distortion) and poses resected there, the reference
    reaches the minimum it reaches from the standard start. This is what admits model 3 to the GPU end-to-end test; no other
    model has been shown to converge from there (the OpenCv5 / OpenCv8 fixtures, k1 = -0.31, did not), so no other is in it."""
    from calico_amd.calico import utils
    model = 3
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    k0 = utils.InitialIntrinsics(model, [k[0], k[0], 0.0, k[1], k[2]])
    start = []
    for f, (R, t) in enumerate(poses):
        s = slice(off[f], off[f + 1])
        Rs, ts, _, _ = rr.refine(model, k0, R, t, pt[s], px[s])
        start.append((Rs, ts))
    ka, pa, last, accepted, converged = cr.refine(model, k0, start, off, pt, px)
    ks, q0, t0 = cr.standard_start(model, 0.1)
    kb, pb, _, _, _ = cr.refine(model, ks, cr.start_poses(q0, t0), off, pt, px)
    print("accepted steps", accepted, "last s", last, "distance between the two results", cr.intrinsics_distance(ka, kb), cr.poses_distance(pa, pb))
    assert converged
    assert max(cr.intrinsics_distance(ka, kb), cr.poses_distance(pa, pb)) <= 10 * cr.FLOOR[model]


@pytest.mark.parametrize("model", (1, 6))
def test_reference_floor_of_the_long_batch(model):
    """calib_ref.FLOOR_LONG, re-measured as FLOOR is: the reference converges from long_start on the 137 frames of
    resect_ref.long_fixture (every pair valid: the fixture asserts it) and six more undamped Gauss-Newton steps stay within
    twice the committed figure."""
    k, off, px, pt, poses = rr.long_fixture(model, 0.1)
    assert len(poses) == 137 and len(px) == 1644
    k0, q0, t0 = cr.long_start(model, 0.1)
    kr, pr, last, accepted, converged = cr.refine(model, k0, cr.start_poses(q0, t0), off, pt, px)
    assert converged and accepted <= 12, (accepted, last)
    floor = 0.0
    for _ in range(6):
        dk, d, s = cr.gn(model, kr, pr, off, pt, px)
        floor = max(floor, s)
        kr, pr = cr.apply(kr, pr, dk, d)
    print("model", model, "FLOOR_LONG", floor, "accepted steps", accepted)
    assert floor <= 2 * cr.FLOOR_LONG[model]


@pytest.mark.parametrize("model", (1, 2, 4))
def test_a_step_without_lambda_diag_c_is_far_from_the_true_step(model):
    """What keeps the step tests' bound (10 floors, tests/test_gpu_chart_steps.py) from hiding what they are for: from the
    standard start the reference's first step is accepted, and the same step with the lambda diag C term left out of the reduced
    system ends at least 1000 floors away (floor: the first step from h = 2e-6 against h = 1e-6 differences)."""
    import lm_rule_ref as lm
    k, off, px, pt, poses = rr.fixture(model, 0.1)
    k0, q0, t0 = cr.standard_start(model, 0.1)
    start = cr.start_poses(q0, t0)
    true = lm.calib_loop(model, k0, start, off, pt, px, 1)
    other = lm.calib_loop(model, k0, start, off, pt, px, 1, h=2e-6)
    mutant = lm.calib_loop(model, k0, start, off, pt, px, 1, drop_diag_c=True)

    def dist(a, b):
        return max(cr.intrinsics_distance(a.point[0], b.point[0]), cr.poses_distance(a.point[1], b.point[1]))
    floor, moved = dist(true, other), dist(true, mutant)
    print("model", model, "floor", floor, "the mutant's distance", moved)
    assert true.log == other.log == [True] and true.lam == 1e-5
    assert floor > 0 and moved >= 1000 * floor


def test_field_of_view_column_of_w_is_exactly_zero_below_its_branch():
    """FieldOfView at w = 1e-3 (w^2 < 1e-5): the oracle's pixel does not depend on w, the reference's central difference for that
    column is exactly zero, its reduced system is never positive definite with w free, and its loop climbs the ladder to the
    cap: degenerate at lambda = 1e12 within the first iteration."""
    import lm_rule_ref as lm
    k, off, px, pt, poses = cr.fov_fixture()
    k0, q0, t0 = cr.fov_start()
    assert k0[3] == cr.FOV_W and k[3] == cr.FOV_W and cr.FOV_W ** 2 < 1e-5
    sys = cr.systems(5, k0, cr.start_poses(q0, t0), off, pt, px)
    for A, B, Cm, _, gk, _, ok in sys:
        assert ok.all() and not B[:, 3].any() and not Cm[3, :].any() and not Cm[:, 3].any() and gk[3] == 0.0
        np.linalg.cholesky(A)
    ref = lm.calib_loop(5, k0, cr.start_poses(q0, t0), off, pt, px, 50)
    assert ref.status == "degenerate" and ref.lam == 1e12 and ref.iterations == 1 and ref.log == []
    held = lm.calib_loop(5, k0, cr.start_poses(q0, t0), off, pt, px, 1, free=(1, 1, 1, 0))
    assert held.status == "out_of_iterations" and held.log == [True]


def test_boundary_fixtures_have_the_properties_the_gpu_tests_rely_on():
    """calib_ref.boundary_fixture, from the reference alone (lm_rule_ref's checks say what is held), with alpha held."""
    import lm_rule_ref as lm
    f = cr.BOUNDARY_FRAME
    pose = lambda p: p[1][f]      # noqa: E731
    for kind, check, steps in (("lost", lm.check_lost, 8), ("joins", lm.check_joins, 1), ("invalid", lm.check_invalid, 50)):
        k, off, px, pt, k0, q0, t0 = cr.boundary_fixture(kind)
        assert len(px) == 721 and off[f + 1] - off[f] == 37
        start = (k0, cr.start_poses(q0, t0))
        loop = lm.calib_loop(6, k0, start[1], off, pt, px, steps, free=cr.BOUNDARY_FREE)
        print(kind, "accepted", loop.log, "lambda", loop.lam, "first accepted step", check(loop, pose, start, pt[off[f + 1] - 1], off[f + 1] - 1))
