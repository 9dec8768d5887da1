"""Accelerometer alignment without a GPU: the entry points are declared, listed and exported, the default options and the struct
sizes are the header's, every argument rule of calico_accel_align is checked before the device is touched, n == 0 is OK, and the
shared numpy reference (accel_align_ref.py) is pinned on the optimiser's conventions -- its cost and its gradient over all 13
columns (rotation, lever arm, bias, gravity, latency) equal the ORACLE's evaluate of a problem with that accelerometer and free q,
t, intrinsics, gravity and latency -- and measured.

Measured here (standard fixture: 6.8 s of the 7.2 s trajectory, 100 Hz, 680 samples, order 6, lever arm (0.05, -0.08, 0.03), the
start InitializeImu leaves: the rotation off by 1.5 degrees, the latency by 2 ms):
  FLOOR -- the largest criterion of six undamped Gauss-Newton steps of the reference at and after its own result, accelerometer
    noise 1e-2 m/s^2: 3.2e-15 (five LM steps from stage L's start; rms 9.908e-3; the lever arm comes back to 1.0e-4 m)
  REF_FREE -- the reference's own distance to the truth on noise-free data: 6.0e-15 (rad, m, m/s^2, s)
  cond(J) 1.82e3 at the result.
The committed figures (accel_align_ref.FLOOR, REF_FREE) are this machine's. They are rounding noise, so another CPU's libm and
BLAS move them: the test holds the re-measured values to twice the committed ones and prints them."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import accel_align_ref as ar
import helpers
from calico_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

NEW_SOURCES = ("accalign_kernels.hip", "accel_align.cpp")


@pytest.fixture(scope="module")
def api():
    entry.build_hip()
    return _capi.CApi(C.CDLL(_capi.hip_library_path()), "calico_")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class _Call:
    """calico_accel_align on 32 samples, one argument replaced at a time."""

    NAMES = ("device", "order", "n_knots", "knots", "basis", "ctrl", "n", "s", "a", "qi", "li", "ti", "bi", "gi", "o", "q", "t", "b", "g", "lat",
             "cov", "summary")

    def __init__(self, api):
        self.api = api
        self.knots, self.basis, self.ctrl, self.order = ar.ir.trajectory()
        self.s = 1.0 + 0.01 * np.arange(32)
        self.a = np.zeros((32, 3))
        self.q, self.t, self.b, self.g, self.lat = np.zeros(4), np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(1)
        self.qi, self.li = np.array([0.0, 0, 0, 2.0]), np.array([0.01])
        self.v3 = np.array([0.1, 0.2, 0.3])
        self.summary = _capi.AccelAlignmentSummary()

    def __call__(self, **kw):
        a = dict(device=0, order=self.order, n_knots=len(self.knots), knots=_dp(self.knots), basis=_dp(self.basis), ctrl=_dp(self.ctrl), n=32,
                 s=_dp(self.s), a=_dp(self.a), qi=_dp(self.qi), li=_dp(self.li), ti=None, bi=None, gi=None, o=None, q=_dp(self.q), t=_dp(self.t),
                 b=_dp(self.b), g=_dp(self.g), lat=_dp(self.lat), cov=None, summary=C.byref(self.summary))
        a.update(kw)
        return self.api.accel_align(*[a[n] for n in self.NAMES])


def _invalid(api, st, *words):
    assert st == _capi.INVALID_ARGUMENT, st
    msg = api.last_error(None).decode()
    assert msg.startswith("calico_accel_align"), msg
    for w in words:
        assert w in msg, (w, msg)


def test_entry_points_are_declared_listed_and_exported(api):
    header = open(os.path.join(ROOT, "include", "calico_hip.h")).read()
    for name in ("default_accel_alignment_options", "accel_align"):
        assert re.search(r"\bcalico_%s\(" % name, header), name
        assert name in _capi.ABI_SYMBOLS
        assert hasattr(api.lib, "calico_" + name) and hasattr(api, name)
    assert "accalign_kernels.hip" in entry.HIP_SOURCES and "accel_align.cpp" in entry.HIP_SOURCES
    assert callable(_capi.accel_align) and callable(_capi.accel_alignment_options)
    for f in NEW_SOURCES:      # no environment switches
        assert "getenv" not in open(os.path.join(entry.CSRC, f)).read(), f
    # the small Cholesky and the step rule are the shared ones, not copies; the launches are declared in kernels.hpp
    src = open(os.path.join(entry.CSRC, "accalign_kernels.hip")).read()
    assert '#include "resect_dev.hpp"' in src and "lds_chol(double*" not in src and "lm_point_decision(" in src and "kLmLambda0 =" not in src
    assert "mfma_f64_16x16x4f64" in src and "atomic" not in src
    assert "launch_accalign_iteration" in open(os.path.join(entry.CSRC, "kernels.hpp")).read()
    # the structs mirror the header field by field
    for struct, cls in (("calico_accel_alignment_options", _capi.AccelAlignmentOptions), ("calico_accel_alignment_summary", _capi.AccelAlignmentSummary)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, header).group(1)
        fields = re.findall(r"^\s*(?:int32_t|int64_t|double)\s+(\w+);", body, re.M)
        assert fields == [n.rstrip("_") for n, _ in cls._fields_], struct


def test_default_options_and_struct_sizes(api):
    o = _capi.AccelAlignmentOptions()
    api.default_accel_alignment_options(C.byref(o))
    assert (o.max_iterations, o.step_tolerance, o.min_samples, o.sigma_accel) == (50, 1e-10, 16, 1.0)
    assert (o.estimate_rotation, o.estimate_lever_arm, o.estimate_bias, o.estimate_gravity, o.estimate_latency) == (1, 1, 1, 1, 1)
    api.default_accel_alignment_options(None)      # (a null pointer is ignored)
    assert _capi.accel_alignment_options(api, estimate_bias=0).estimate_bias == 0
    with pytest.raises(TypeError):
        _capi.accel_alignment_options(api, no_such_field=1)
    # 4 (+4) + 8 + 6 x 4 + 8, and 4 + 4 + 8 + 8 + 4 (+4) + 6 x 8: what a C compiler lays out for the header's structs
    assert C.sizeof(_capi.AccelAlignmentOptions) == 48 and C.sizeof(_capi.AccelAlignmentSummary) == 80
    assert _capi.AccelAlignmentOptions.sigma_accel.offset == 40 and _capi.AccelAlignmentSummary.rms.offset == 32


def test_argument_rules_need_no_device(api):
    call = _Call(api)
    for v in (1, 9):
        _invalid(api, call(order=v), "order")
    _invalid(api, call(n_knots=11), "n_knots")
    for name in ("knots", "basis", "ctrl"):
        _invalid(api, call(**{name: None}), "null knots, basis or ctrl")
    _invalid(api, call(n=-1), "n must be >= 0")
    for name in ("s", "a"):
        _invalid(api, call(**{name: None}), "null stamps or accel")
    for name in ("q", "t", "b", "g", "lat", "summary"):
        _invalid(api, call(**{name: None}), "null q_rig_accel_out")
    unsorted = call.s.copy()
    unsorted[5] = unsorted[3]
    _invalid(api, call(s=_dp(unsorted)), "accel stamps are not sorted", "sample 5")
    nan = call.s.copy()
    nan[7] = np.nan
    _invalid(api, call(s=_dp(nan)), "not finite")
    # the start
    _invalid(api, call(qi=None), "q_init and latency_init are required")
    _invalid(api, call(li=None), "q_init and latency_init are required")
    _invalid(api, call(qi=_dp(np.zeros(4))), "q_init", "non-zero length")
    _invalid(api, call(qi=_dp(np.array([0.0, np.nan, 0, 1]))), "q_init")
    _invalid(api, call(li=_dp(np.array([np.inf]))), "latency_init")
    v3 = _dp(call.v3)
    for given in (dict(ti=v3), dict(bi=v3), dict(gi=v3), dict(ti=v3, bi=v3), dict(ti=v3, gi=v3), dict(bi=v3, gi=v3)):
        _invalid(api, call(**given), "given together or not at all")
    bad = _dp(np.array([0.0, np.nan, 0.0]))
    for name in ("ti", "bi", "gi"):
        _invalid(api, call(**dict(dict(ti=v3, bi=v3, gi=v3), **{name: bad})), "must be finite")

    def opts(**kw):
        return C.byref(_capi.accel_alignment_options(api, **kw))
    for name in ("estimate_lever_arm", "estimate_bias", "estimate_gravity"):      # stage L needs all three free
        _invalid(api, call(o=opts(**{name: 0})), "must all be estimated")
        st = call(o=opts(**{name: 0}), ti=v3, bi=v3, gi=v3, device=10 ** 6, n=0, s=None, a=None)
        assert st == _capi.OK
    for v in (0.0, -1e-11, float("inf"), float("nan")):
        _invalid(api, call(o=opts(step_tolerance=v)), "step_tolerance")
        _invalid(api, call(o=opts(sigma_accel=v)), "sigma_accel")
    for v in (0, -3):
        _invalid(api, call(o=opts(max_iterations=v)), "max_iterations")
    for v in (4, 0, -1):
        _invalid(api, call(o=opts(min_samples=v)), "min_samples")
    # the rules come before the device: a bad argument AND a bad device ordinal is still the argument's error
    _invalid(api, call(device=10 ** 6, order=1), "order")
    # no samples, or too few on the knots: OK with TOO_FEW_SAMPLES, no device touched, the outputs are the start
    call.q[:] = 7.0
    call.t[:] = 7.0
    assert call(device=10 ** 6, n=0, s=None, a=None) == _capi.OK
    s = call.summary
    assert (s.status, s.linear_status, s.samples, s.first_sample, s.iterations) == (_capi.ALIGN_TOO_FEW_SAMPLES, -1, 0, 0, 0)
    assert call.q.tolist() == [0.0, 0.0, 0.0, 1.0] and call.t.tolist() == [0.0, 0.0, 0.0] and call.lat[0] == 0.01
    assert call(device=10 ** 6, n=15, ti=v3, bi=v3, gi=v3) == _capi.OK and call.summary.status == _capi.ALIGN_TOO_FEW_SAMPLES
    assert call.summary.samples == 15 and call.t.tolist() == call.v3.tolist() and call.g.tolist() == call.v3.tolist()
    assert abs(call.summary.gravity_norm - np.linalg.norm(call.v3)) <= 1e-15
    far = call.s + 100.0      # (off the knots)
    assert call(device=10 ** 6, s=_dp(far)) == _capi.OK and call.summary.samples == 0
    st = call()                     # a valid call: OK on a device, and without one it fails loudly, with a message
    if st != _capi.OK:
        assert st == _capi.INTERNAL and "device" in api.last_error(None).decode() and not helpers.has_gpu()


def test_the_range_is_the_stamps_and_the_times_on_the_knots(api):
    """Both the stamp and stamp - latency_init inside the valid knots, one range."""
    call = _Call(api)
    lo, hi = ar.ir.valid_range(ar.ir.trajectory())
    call.s = np.concatenate([[lo - 0.5, lo + 0.005], lo + 0.02 + 0.01 * np.arange(28), [hi - 0.001, hi + 0.2]])
    assert len(call.s) == 32
    assert call(device=10 ** 6, o=C.byref(_capi.accel_alignment_options(api, min_samples=10 ** 6))) == _capi.OK
    first, end = ar.sample_range(ar.ir.trajectory(), call.s, 0.01)
    assert (call.summary.first_sample, call.summary.samples) == (first, end - first) == (2, 29)      # (lo + 0.005 - 0.01 is off the knots)


def test_wrapper_checks_its_shapes(api):
    knots, basis, ctrl, order = ar.ir.trajectory()
    q = np.array([0.0, 0, 0, 1])
    with pytest.raises(ValueError):
        _capi.accel_align(api, order, knots, basis, ctrl[:-1], np.zeros(4), np.zeros((4, 3)), q, 0.0)
    with pytest.raises(ValueError):
        _capi.accel_align(api, order, knots, basis, ctrl, np.zeros(5), np.zeros((4, 3)), q, 0.0)
    r = _capi.accel_align(api, order, knots, basis, ctrl, np.zeros(0), np.zeros((0, 3)), q, 0.25, covariance=True)
    assert r["status"] == _capi.ALIGN_TOO_FEW_SAMPLES and r["linear_status"] == -1 and r["cov"].shape == (13, 13) and not r["cov"].any()
    assert r["latency"] == 0.25 and r["q_rig_accel"].tolist() == [0, 0, 0, 1]


def test_reference_accelerometer_term_is_the_optimisers():
    """Cost, gradient and J^T J of the reference over all 13 columns at a random estimate against the oracle's evaluate of a problem
    with that accelerometer: 1e-10 relative. (Ceres' quaternion tangent is half the rotation vector.) The latency column goes
    through the closed form of alpha and the pose's third derivative: the oracle's gradient decides whether it is right."""
    spl, s, a, truth = ar.fixture(1e-3)
    rng = np.random.default_rng(5)
    est = ar.apply(ar.truth_estimate(truth), np.concatenate([0.2 * rng.standard_normal(3), 0.05 * rng.standard_normal(3),
                                                             0.05 * rng.standard_normal(3), 0.3 * rng.standard_normal(3), [0.004]]))
    sigma = 0.7
    P, cols = ar.accel_problem(helpers.oracle_api(), spl, s, a, est, sigma)
    cost, grad, H = P.evaluate()
    r, J, _ = ar.system(spl, s, a, est, sigma)
    Jf = J.reshape(-1, 13)
    scale = ar.ROTATION_TANGENT
    mine_g, mine_H = scale * (Jf.T @ r.ravel()), scale[:, None] * (Jf.T @ Jf) * scale[None, :]
    print("cost", cost, ar.cost(spl, s, a, est, sigma), "gradient", grad[cols], mine_g)
    assert abs(ar.cost(spl, s, a, est, sigma) - cost) <= 1e-10 * cost
    assert np.abs(mine_g - grad[cols]).max() <= 1e-10 * np.abs(grad[cols]).max()
    assert abs(mine_g[12] - grad[cols][12]) <= 1e-10 * abs(grad[cols][12])      # (the latency column on its own scale)
    assert np.abs(mine_H - H[np.ix_(cols, cols)]).max() <= 1e-10 * np.abs(H[np.ix_(cols, cols)]).max()


def test_reference_stage_l_is_the_minimum_at_fixed_rotation_and_latency():
    spl, s, a, truth = ar.fixture(1e-3)
    q0, l0 = ar.imu_start(truth)
    t, b, g, rms, status = ar.linear(spl, s, a, q0, l0)
    free = ar.free_mask(rotation=0, latency=0)
    crit = ar.criterion(spl, s, a, (q0, t, b, g, l0), free)
    print("stage L's criterion", crit, "rms", rms)
    assert status == ar.OK and crit <= 1e-12
    assert ar.linear(*ar.fixture(1e-3, one_axis=True)[:3], q0, l0)[4] == ar.NOT_POSITIVE_DEFINITE


def test_reference_floor_and_noise_free_distance():
    """The reference on the standard fixture. Noise-free it recovers the truth within twice REF_FREE; with 1e-2 m/s^2 of noise six
    more undamped Gauss-Newton steps stay within twice FLOOR, and the lever arm comes back to some 1e-4 m."""
    spl, s, a, truth = ar.fixture(0.0)
    q0, l0 = ar.imu_start(truth)
    r = ar.align(spl, s, a, q0, l0)
    assert (r["status"], r["linear_status"], r["samples"], r["first_sample"]) == (ar.OK, ar.OK, 680, 0)
    free = ar.distance_to_truth(ar.estimate(r), truth)
    print("noise-free distance to the truth", free, "iterations", r["iterations"])
    assert free <= 2 * ar.REF_FREE
    spl, s, a, truth = ar.fixture(1e-3)
    r = ar.align(spl, s, a, q0, l0)
    assert r["status"] == ar.OK and r["iterations"] <= 6
    est, floor = ar.estimate(r), 0.0
    print("cond(J)", ar.cond(spl, s, a, est), "lever arm error", np.abs(est[1] - truth["t_rig_accel"]).max())
    for _ in range(6):
        d, size = ar.gn(spl, s, a, est)
        floor = max(floor, size)
        est = ar.apply(est, d)
    print("FLOOR", floor, "iterations", r["iterations"], "rms", r["rms"], "distance to the truth", ar.distance_to_truth(est, truth))
    assert 0.9e-2 <= r["rms"] <= 1.1e-2
    assert floor <= 2 * ar.FLOOR
    assert np.abs(est[1] - truth["t_rig_accel"]).max() <= 5e-4
    # the noise moves the estimate by far more than the floor: the criterion tells a minimum from the truth
    assert ar.criterion(spl, s, a, ar.truth_estimate(truth)) >= 1e6 * ar.FLOOR


def test_reference_ends_ok_on_every_shape_of_the_device_tests():
    import test_gpu_accel_align as tg
    for order in (4, 6):
        for n, lead in [(n, 0) for n in tg.SHAPES] + [(100, 37)]:
            spl, s, a, truth = tg.shaped(n, order, lead)
            r = ar.align(spl, s, a, *ar.imu_start(truth))
            assert (r["status"], r["samples"], r["first_sample"]) == (ar.OK, n, lead), (order, n, lead)
