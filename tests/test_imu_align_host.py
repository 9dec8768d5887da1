"""Camera-IMU alignment without a GPU: the entry points are declared, listed and exported, the default options are the header's,
every argument rule of calico_imu_align is checked before the device is touched, n_gyro == 0 is OK, and the shared numpy reference
(imu_align_ref.py) is pinned on the optimiser's conventions -- its gyroscope cost and gradient in (rotation, bias, latency) and its
accelerometer term's gradient in (gravity, bias) equal the ORACLE's evaluate -- and measured.

Measured here (standard fixture: 6.8 s of the 7.2 s trajectory, 100 Hz, 680 samples, 41 lags):
  FLOOR -- the largest criterion of six undamped Gauss-Newton steps of the reference at and after its own result, gyroscope noise
    1e-3 rad/s: 1.9e-16 (three LM steps from Horn's start; rms 1.0017e-3)
  the reference's own distance to the truth on noise-free data: 1.9e-16 (rotation rad, bias rad/s, latency s); gravity and
    accelerometer bias 5.6e-15 m/s^2
The committed figures (imu_align_ref.FLOOR, REF_FREE, REF_FREE_ACCEL) are this machine's. They are rounding noise, so another
CPU's libm and BLAS move them: the test holds the re-measured values to twice the committed ones and prints them."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import helpers
import imu_align_ref as ar
from calico_amd import _capi, synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

NEW_SOURCES = ("align_kernels.hip", "imu_align.cpp", "imu_align_dev.hpp")


@pytest.fixture(scope="module")
def api():
    entry.build_hip()
    return _capi.CApi(C.CDLL(_capi.hip_library_path()), "calico_")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class _Call:
    """calico_imu_align on 32 gyroscope and 32 accelerometer samples, one argument replaced at a time."""

    NAMES = ("device", "order", "n_knots", "knots", "basis", "ctrl", "ng", "gs", "g", "na", "as_", "a", "tra", "qi", "li", "o", "q", "b", "lat",
             "grav", "ab", "cov", "curve", "summary")

    def __init__(self, api):
        self.api = api
        self.knots, self.basis, self.ctrl, self.order = ar.trajectory()
        self.gs = 1.0 + 0.01 * np.arange(32)
        self.g, self.a = np.zeros((32, 3)), np.zeros((32, 3))
        self.q, self.b, self.lat, self.grav, self.ab = np.zeros(4), np.zeros(3), np.zeros(1), np.zeros(3), np.zeros(3)
        self.qi, self.li = np.array([0.0, 0, 0, 1]), np.zeros(1)
        self.summary = _capi.ImuAlignmentSummary()

    def __call__(self, **kw):
        a = dict(device=0, order=self.order, n_knots=len(self.knots), knots=_dp(self.knots), basis=_dp(self.basis), ctrl=_dp(self.ctrl), ng=32,
                 gs=_dp(self.gs), g=_dp(self.g), na=32, as_=_dp(self.gs), a=_dp(self.a), tra=None, qi=None, li=None, o=None, q=_dp(self.q),
                 b=_dp(self.b), lat=_dp(self.lat), grav=_dp(self.grav), ab=_dp(self.ab), cov=None, curve=None, summary=C.byref(self.summary))
        a.update(kw)
        return self.api.imu_align(*[a[n] for n in self.NAMES])


def _invalid(api, st, *words):
    assert st == _capi.INVALID_ARGUMENT, st
    msg = api.last_error(None).decode()
    assert msg.startswith("calico_imu_align"), msg
    for w in words:
        assert w in msg, (w, msg)


def test_entry_points_are_declared_listed_and_exported(api):
    header = open(os.path.join(ROOT, "include", "calico_hip.h")).read()
    for name in ("default_imu_alignment_options", "imu_align"):
        assert re.search(r"\bcalico_%s\(" % name, header), name
        assert name in _capi.ABI_SYMBOLS
        assert hasattr(api.lib, "calico_" + name) and hasattr(api, name)
    for i, name in enumerate(("OK", "TOO_FEW_SAMPLES", "NO_PEAK", "DEGENERATE", "NOT_CONVERGED", "NOT_POSITIVE_DEFINITE")):
        assert re.search(r"#define CALICO_ALIGN_%s %d\b" % (name, i), header), name
        assert getattr(_capi, "ALIGN_" + name) == i and getattr(ar, name) == i
    assert re.search(r"#define CALICO_ALIGN_MAX_LAGS %d\b" % _capi.ALIGN_MAX_LAGS, header)
    assert "align_kernels.hip" in entry.HIP_SOURCES and "imu_align.cpp" in entry.HIP_SOURCES
    assert callable(_capi.imu_align) and callable(_capi.imu_alignment_options)
    for f in NEW_SOURCES:      # no environment switches
        assert "getenv" not in open(os.path.join(entry.CSRC, f)).read(), f
    # the small Cholesky is resect_dev.hpp's, not a copy; the launches are declared in kernels.hpp
    src = open(os.path.join(entry.CSRC, "align_kernels.hip")).read()
    assert '#include "resect_dev.hpp"' in src and "lds_chol(double*" not in src
    assert "launch_align_iteration" in open(os.path.join(entry.CSRC, "kernels.hpp")).read()
    # the structs mirror the header field by field
    for struct, cls in (("calico_imu_alignment_options", _capi.ImuAlignmentOptions), ("calico_imu_alignment_summary", _capi.ImuAlignmentSummary)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, header).group(1)
        fields = re.findall(r"^\s*(?:int32_t|int64_t|double)\s+(\w+);", body, re.M)
        assert fields == [n.rstrip("_") for n, _ in cls._fields_], struct


def test_default_options(api):
    o = _capi.ImuAlignmentOptions()
    api.default_imu_alignment_options(C.byref(o))
    assert (o.max_lag, o.lag_step, o.max_iterations, o.step_tolerance) == (0.1, 1e-3, 50, 1e-10)
    assert (o.estimate_latency, o.estimate_gyro_bias, o.estimate_accel_bias, o.min_samples, o.sigma_gyro) == (1, 1, 1, 16, 1.0)
    api.default_imu_alignment_options(None)      # (a null pointer is ignored)
    assert _capi.imu_alignment_options(api, max_lag=0.05).max_lag == 0.05
    with pytest.raises(TypeError):
        _capi.imu_alignment_options(api, no_such_field=1)


def test_argument_rules_need_no_device(api):
    call = _Call(api)
    for v in (1, 9):
        _invalid(api, call(order=v), "order")
    _invalid(api, call(n_knots=11), "n_knots")
    for name in ("knots", "basis", "ctrl"):
        _invalid(api, call(**{name: None}), "null knots, basis or ctrl")
    _invalid(api, call(ng=-1), "n_gyro")
    _invalid(api, call(na=-1), "n_accel")
    for name in ("gs", "g"):
        _invalid(api, call(**{name: None}), "null gyro_stamps or gyro")
    for name in ("as_", "a"):
        _invalid(api, call(**{name: None}), "null accel_stamps or accel")
    for name in ("q", "b", "lat", "summary"):
        _invalid(api, call(**{name: None}), "null q_rig_gyro_out")
    for name in ("grav", "ab"):
        _invalid(api, call(**{name: None}), "null gravity_world_out")
    unsorted = call.gs.copy()
    unsorted[5] = unsorted[3]
    _invalid(api, call(gs=_dp(unsorted)), "gyro stamps are not sorted", "sample 5")
    _invalid(api, call(as_=_dp(unsorted)), "accel stamps are not sorted")
    nan = call.gs.copy()
    nan[7] = np.nan
    _invalid(api, call(gs=_dp(nan)), "not finite")
    _invalid(api, call(qi=_dp(call.qi)), "q_init and latency_init")
    _invalid(api, call(li=_dp(call.li)), "q_init and latency_init")
    _invalid(api, call(qi=_dp(np.zeros(4)), li=_dp(call.li)), "q_init")
    _invalid(api, call(qi=_dp(call.qi), li=_dp(np.array([np.inf]))), "latency_init")

    def opts(**kw):
        return C.byref(_capi.imu_alignment_options(api, **kw))
    for v in (0.0, -1e-3, float("inf"), float("nan")):
        _invalid(api, call(o=opts(lag_step=v)), "lag_step")
    for v in (-0.1, float("inf"), float("nan")):
        _invalid(api, call(o=opts(max_lag=v)), "max_lag")
    _invalid(api, call(o=opts(max_lag=2.048, lag_step=1e-3)), "4096 lags")      # 4,097 latencies
    for v in (0.0, -1e-11, float("inf"), float("nan")):
        _invalid(api, call(o=opts(step_tolerance=v)), "step_tolerance")
        _invalid(api, call(o=opts(sigma_gyro=v)), "sigma_gyro")
    for v in (0, -3):
        _invalid(api, call(o=opts(max_iterations=v)), "max_iterations")
    for v in (2, 0, -1):
        _invalid(api, call(o=opts(min_samples=v)), "min_samples")
    # the rules come before the device: a bad argument AND a bad device ordinal is still the argument's error
    _invalid(api, call(device=10 ** 6, order=1), "order")
    # no gyroscope samples, or too few on the knots: OK with TOO_FEW_SAMPLES, no device touched, the outputs are the start
    call.q[:] = 7.0
    assert call(device=10 ** 6, ng=0, gs=None, g=None, na=0, as_=None, a=None, grav=None, ab=None) == _capi.OK
    s = call.summary
    assert (s.gyro_status, s.accel_status, s.gyro_samples, s.peak_index) == (_capi.ALIGN_TOO_FEW_SAMPLES, _capi.ALIGN_TOO_FEW_SAMPLES, 0, -1)
    assert call.q.tolist() == [0.0, 0.0, 0.0, 1.0]
    assert call(device=10 ** 6, ng=15) == _capi.OK and call.summary.gyro_status == _capi.ALIGN_TOO_FEW_SAMPLES and call.summary.gyro_samples == 15
    far = call.gs + 100.0      # (off the knots)
    assert call(device=10 ** 6, gs=_dp(far)) == _capi.OK and call.summary.gyro_samples == 0
    st = call()                     # a valid call: OK on a device, and without one it fails loudly, with a message
    if st != _capi.OK:
        assert st == _capi.INTERNAL and "device" in api.last_error(None).decode() and not helpers.has_gpu()


def test_wrapper_checks_its_shapes(api):
    knots, basis, ctrl, order = ar.trajectory()
    with pytest.raises(ValueError):
        _capi.imu_align(api, order, knots, basis, ctrl[:-1], np.zeros(4), np.zeros((4, 3)))
    with pytest.raises(ValueError):
        _capi.imu_align(api, order, knots, basis, ctrl, np.zeros(5), np.zeros((4, 3)))
    with pytest.raises(ValueError):
        _capi.imu_align(api, order, knots, basis, ctrl, np.zeros(4), np.zeros((4, 3)), accel=np.zeros((4, 3)))
    r = _capi.imu_align(api, order, knots, basis, ctrl, np.zeros(0), np.zeros((0, 3)), covariance=True, curve=True)
    assert r["gyro_status"] == _capi.ALIGN_TOO_FEW_SAMPLES and r["gravity_world"] is None and r["curve"].shape == (0,)
    assert not r["cov"].any() and r["latency"] == 0.0


def test_reference_gyroscope_term_is_the_optimisers():
    """Cost and gradient of the reference in (rotation, bias, latency) at a random estimate against the oracle's evaluate of a
    problem with that gyroscope: 1e-10 relative. (Ceres' quaternion tangent is half the rotation vector.)"""
    spl, gs, g, _, _, truth = ar.fixture(1e-3)
    rng = np.random.default_rng(5)
    est = ar.apply((truth["q"], truth["bias"], truth["latency"]), np.concatenate([0.2 * rng.standard_normal(3), 0.05 * rng.standard_normal(3), [0.004]]))
    sigma = 0.7
    built, cols = ar.gyro_problem(helpers.oracle_api(), spl, gs, g, est, sigma)
    cost, grad, H = built.problem.evaluate()
    r, J = ar.gyro_system(spl, gs, g, est, sigma)
    Jf = J.reshape(-1, 7)
    scale = np.array([2.0, 2, 2, 1, 1, 1, 1])
    mine_g, mine_H = scale * (Jf.T @ r.ravel()), scale[:, None] * (Jf.T @ Jf) * scale[None, :]
    print("cost", cost, ar.cost(spl, gs, g, est, sigma), "gradient", grad[cols], mine_g)
    assert abs(ar.cost(spl, gs, g, est, sigma) - cost) <= 1e-10 * cost
    assert np.abs(mine_g - grad[cols]).max() <= 1e-10 * np.abs(grad[cols]).max()
    assert np.abs(mine_H - H[np.ix_(cols, cols)]).max() <= 1e-10 * np.abs(H[np.ix_(cols, cols)]).max()


@pytest.mark.parametrize("lever", [None, (0.1, -0.02, 0.03)])
def test_reference_accelerometer_term_is_the_optimisers(lever):
    """The reference's linear system in (gravity, bias): residual y + M g - bias, against the oracle's cost and gradient of a
    problem with that accelerometer and a free gravity block, lever arm included."""
    spl, _, _, as_, a, truth = ar.fixture(1e-3, lever=lever)
    q, tau, tra = truth["q"], truth["latency"] + 0.002, truth["t_rig_accel"]
    g, b = truth["gravity"] + [0.3, -0.2, 0.1], truth["accel_bias"] + [0.01, 0.02, -0.03]
    P, cols = ar.accel_problem(helpers.oracle_api(), spl, as_, a, q, tau, tra, g, b)
    cost, grad, _ = P.evaluate()
    M, y, used = ar.accel_system(spl, as_, a, q, tau, tra)
    assert used.all()
    res = y + M @ g - b      # = measured - prediction
    mine = np.concatenate([np.einsum("nji,nj->i", M, res), -res.sum(0)])
    print("cost", cost, 0.5 * np.sum(res * res), "gradient", grad[cols], mine)
    assert abs(0.5 * np.sum(res * res) - cost) <= 1e-10 * cost
    assert np.abs(mine - grad[cols]).max() <= 1e-10 * np.abs(grad[cols]).max()


def test_reference_floor_and_noise_free_distance():
    """The reference on the standard fixture. Noise-free it recovers the truth within twice REF_FREE (REF_FREE_ACCEL for gravity
    and the accelerometer's bias); with 1e-3 rad/s noise six more undamped Gauss-Newton steps stay within twice FLOOR."""
    spl, gs, g, as_, a, truth = ar.fixture(0.0)
    r = ar.align(spl, gs, g, as_, a, **ar.OPTIONS)
    assert (r["gyro_status"], r["accel_status"], r["gyro_samples"], r["n_lags"]) == (ar.OK, ar.OK, 680, 41)
    free = ar.distance_to_truth(ar.estimate(r), truth)
    free_accel = max(np.abs(r["gravity_world"] - truth["gravity"]).max(), np.abs(r["accel_bias"] - truth["accel_bias"]).max())
    print("noise-free distance to the truth", free, "accelerometer part", free_accel, "iterations", r["iterations"])
    assert free <= 2 * ar.REF_FREE and free_accel <= 2 * ar.REF_FREE_ACCEL
    spl, gs, g, as_, a, truth = ar.fixture(1e-3)
    r = ar.align(spl, gs, g, as_, a, **ar.OPTIONS)
    assert r["gyro_status"] == ar.OK and r["iterations"] <= 6 and r["peak_index"] == 25
    est, floor = ar.estimate(r), 0.0
    for _ in range(6):
        d, s = ar.gn(spl, gs, g, est)
        floor = max(floor, s)
        est = ar.apply(est, d)
    print("FLOOR", floor, "iterations", r["iterations"], "rms", r["gyro_rms"], "distance to the truth", ar.distance_to_truth(est, truth))
    assert 0.9e-3 <= r["gyro_rms"] <= 1.1e-3
    assert floor <= 2 * ar.FLOOR
    # the noise moves the estimate by far more than the floor: the criterion tells a minimum from the truth
    assert ar.criterion(spl, gs, g, (truth["q"], truth["bias"], truth["latency"])) > 1e3 * ar.FLOOR
