"""calico_imu_align, calico_camera_align and calico_accel_align, bit for bit against the commit before their kernels took the dense
one-point Levenberg-Marquardt loop from one header (calico_amd/csrc/point_lm_dev.hpp) and their hosts the family's scaffold from
align_host.hpp: every output array and every field of the summary of every case below has the bytes that
tests/golden/align_parent_bits.npz holds. tests/golden/make_align_parent_bits.py recorded them on an MI355X from a library built
from that commit; the file names the compiler (`hipcc --version`) that built it.

The golden file is re-recorded only by a commit that changes the arithmetic of these calls on purpose -- an order of summation, a
formula, a launch shape that an order depends on -- and says so; a refactor never does. A change of toolchain is the other
legitimate reason: another compiler may contract or schedule floating-point operations differently, and then the parent commit
is to be built with the new one and recorded again. The file holds recorded results only.

The cases are the smallest at which each shared piece can still go wrong:
  IMU            300 gyroscope samples at order 4 (a full workgroup plus 44: a partial wave and a second chunk). Runs: the searched
                 start with accelerometer samples (stage D reads the head's status); a given start with the latency held; the bias
                 held; max_iterations = 1 (NOT_CONVERGED); constant measurements (NO_PEAK ends before the loop); rotation about
                 one axis (DEGENERATE); a given start 2.4 rad and 0.3 s from the truth (ten iterations, the damping falling to
                 its floor); and the measurements times three (a wrong scale factor: the residual at the minimum is large) from
                 a start 0.54 rad and 0.05 s off with max_iterations = 12, where seven of the twelve steps are rejected.
  camera         six frames: four of 20 pairs, one of 70 (a second trip of 64) and one of 3 (below min_points: it takes no part),
                 min_frames = 4, for models 2 (11 intrinsics) and 6 (4). Runs: through the resection and the search; a given
                 start; Huber; the translation held; the latency held; max_iterations = 2; a rig at rest (NO_PEAK); and a given
                 start far from the truth, whose first steps are rejected.
  accelerometer  300 samples at order 4. Runs: stage L's start; a given start; each of the five groups held in turn (the free_bits
                 masks of the 13 x 13 system, and "held keeps its bits"); max_iterations = 1; rotation about one axis (the ladder
                 climbs to lambda = 1e12, NOT_POSITIVE_DEFINITE); one NaN measurement (DEGENERATE); and a given start far from the
                 truth, whose first steps are rejected.
The status every case ends with is stated; for the cases with rejected steps the numpy references (imu_align_ref.py,
camera_align_ref.py, accel_align_ref.py, with lm_rule_ref.py's rule) run the same loop from the same start on the CPU:
test_the_rejected_step_cases_reject_in_the_reference_too holds that they reject at least once (the IMU seven times, the camera twice with model 2
and five times with model 6, the accelerometer three times), and the GPU test that the device ends with the reference's status after the
reference's number of iterations. The starts were picked with the references on the CPU.

The IMU's start alone rejects nothing: imu_align_ref.py's loop rejected no step from some 900 starts on the fixture's own data
(rotations of up to pi, latencies up to 3 s off, the bias or the latency held). Its model has no scale factor, so measurements three
times too large leave a large residual at the minimum, the Gauss-Newton matrix misjudges the curvature there, and the loop rejects
about every other step until the cap ends it."""
import functools
import os

import numpy as np
import pytest

import accel_align_ref as acr
import camera_align_ref as cref
import imu_align_ref as ir
from calico_amd import _capi
from calico_amd import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "align_parent_bits.npz")

IMU_FIELDS = tuple(name for name, _ in _capi.ImuAlignmentSummary._fields_) + ("q_rig_gyro", "gyro_bias", "latency", "gravity_world", "accel_bias", "cov",
                                                                                "curve", "curve_tail")
CAMERA_FIELDS = tuple(name for name, _ in _capi.CameraAlignmentSummary._fields_) + ("q_rig_camera", "t_rig_camera", "latency", "frame_rms", "frame_n_used",
                                                                                      "frame_status", "cov", "curve", "curve_tail")
ACCEL_FIELDS = tuple(name for name, _ in _capi.AccelAlignmentSummary._fields_) + ("q_rig_accel", "t_rig_accel", "bias", "gravity_world", "latency", "cov")


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def imu_data(one_axis=False):
    """imu_align_ref.fixture at 300 samples and order 4: (spline, gyro stamps, gyro, accel stamps, accel, truth)."""
    fx = ir.fixture(1e-3, rate=300 / 6.8, order=4, one_axis=one_axis)
    assert len(fx[1]) == 300
    return fx


def _turned(q, angle, axis):
    q = syn.quat_mul(syn.quat_from_axis_angle(angle * np.asarray(axis, float) / np.linalg.norm(axis)), q)
    return q if q[3] >= 0 else -q


def imu_far_start():
    """(q_init, latency_init): 2.4 rad from the truth about (1, 2, -2), the latency 0.3 s off."""
    truth = imu_data()[5]
    return _turned(truth["q"], 2.4, (1.0, 2.0, -2.0)), truth["latency"] + 0.3


IMU_REJECTED = dict(scale=3.0, angle=0.54, dlat=0.05, max_iterations=12)


def imu_rejected_start():
    """(q_init, latency_init, gyro): IMU_REJECTED's start off the truth about (1, 2, -2), and the measurements times its scale."""
    _, _, g, _, _, truth = imu_data()
    return _turned(truth["q"], IMU_REJECTED["angle"], (1.0, 2.0, -2.0)), truth["latency"] + IMU_REJECTED["dlat"], IMU_REJECTED["scale"] * g


def _imu_rejected(api):
    q0, l0, g = imu_rejected_start()
    return _imu(api, accel=False, gyro=g, q_init=q0, latency_init=l0, max_iterations=IMU_REJECTED["max_iterations"])


def _imu_reference_rejected():
    spl, gs, _, _, _, _ = imu_data()
    q0, l0, g = imu_rejected_start()
    return ir.align(spl, gs, g, q_init=q0, latency_init=l0, max_iterations=IMU_REJECTED["max_iterations"], **ir.OPTIONS)


def _imu(api, one_axis=False, accel=True, gyro=None, **kw):
    spl, gs, g, as_, a, _ = imu_data(one_axis)
    knots, basis, ctrl, order = spl
    extra = {k: kw.pop(k) for k in ("q_init", "latency_init") if k in kw}
    return _capi.imu_align(api, order, knots, basis, ctrl, gs, g if gyro is None else gyro, as_ if accel else None, a if accel else None,
                           options=_capi.imu_alignment_options(api, **dict(ir.OPTIONS, **kw)), covariance=True, curve=True, **extra)


CAMERA_TIMES = (0.6, 1.7, 2.8, 4.2, 5.3, 6.4)


@functools.lru_cache(maxsize=None)
def camera_data(model, at_rest=False):
    """camera_align_ref.fixture's frames at CAMERA_TIMES with 0.1 pixels of noise: frames 0, 1, 3 and 5 see the first 20 points
    of the AprilGrid, frame 2 its first 70, frame 4 its first three (every one of them is in the image at these times)."""
    grid = syn.aprilgrid_points()
    parts = [cref.fixture(noise=0.1, model=model, points=grid[:{2: 70, 4: 3}.get(f, 20)], times=[t], seed=5 + f, at_rest=at_rest)
             for f, t in enumerate(CAMERA_TIMES)]
    fx = dict(parts[0])
    fx["stamps"] = np.concatenate([p["stamps"] for p in parts])
    fx["pixels"] = np.concatenate([p["pixels"] for p in parts])
    fx["points"] = np.concatenate([p["points"] for p in parts])
    fx["offsets"] = np.concatenate([[0], np.cumsum([p["offsets"][1] for p in parts])]).astype(np.int64)
    assert np.diff(fx["offsets"]).tolist() == [20, 20, 70, 20, 3, 20], np.diff(fx["offsets"])
    return fx


CAMERA_OPTIONS = dict(cref.OPTIONS, min_frames=4)


def camera_start(model, angle=0.02, shift=0.01, dlat=0.002):
    """(q_init, t_init, latency_init) off the truth by `angle` about (2, -1, 1), `shift` along (1, -1, 1) and dlat."""
    truth = camera_data(model)["truth"]
    return _turned(truth["q"], angle, (2.0, -1.0, 1.0)), truth["t"] + shift * np.array([1.0, -1.0, 1.0]), truth["latency"] + dlat


CAMERA_FAR = {2: dict(angle=0.6, shift=0.3, dlat=0.02), 6: dict(angle=0.1, shift=0.3, dlat=-0.25)}


def _camera(api, model, start=None, at_rest=False, **kw):
    fx = camera_data(model, at_rest)
    extra = {} if start is None else dict(zip(("q_init", "t_init", "latency_init"), start))
    return _capi.camera_align(api, *cref.call_args(fx), options=_capi.camera_alignment_options(api, **dict(CAMERA_OPTIONS, **kw)), covariance=True,
                              curve=True, **extra)


def _camera_reference_far(model):
    q0, t0, l0 = camera_start(model, **CAMERA_FAR[model])
    return cref.align(camera_data(model), q_init=q0, t_init=t0, latency_init=l0, **CAMERA_OPTIONS)


@functools.lru_cache(maxsize=None)
def accel_data(one_axis=False):
    """accel_align_ref.fixture at 300 samples and order 4: (spline, stamps, accel, truth, q_init, latency_init), the start
    accel_align_ref.imu_start's."""
    spl, s, a, truth = acr.fixture(1e-3, rate=300 / 6.8, order=4, one_axis=one_axis)
    assert len(s) == 300
    return (spl, s, a, truth) + acr.imu_start(truth)


def accel_given(scale=1.0):
    """(t_init, bias_init, gravity_init) off the truth, as test_gpu_accel_align.py's given start is at scale 1."""
    truth = accel_data()[3]
    return (truth["t_rig_accel"] + scale * np.array([0.01, -0.02, 0.015]), truth["accel_bias"] + scale * np.array([0.02, 0.01, -0.01]),
            truth["gravity"] + scale * np.array([0.2, -0.1, 0.3]))


def accel_far_start():
    """(q_init, latency_init, (t_init, bias_init, gravity_init)): 2.43 rad from the truth, the latency 0.4 s off, the rest twenty
    times the given start's offsets."""
    truth = accel_data()[3]
    return _turned(truth["q"], 2.43, (1.0, 2.0, -2.0)), truth["latency"] + 0.4, accel_given(20.0)


def _accel(api, start=None, one_axis=False, meas=None, q_init=None, latency_init=None, **kw):
    spl, s, a, _, q0, l0 = accel_data(one_axis)
    knots, basis, ctrl, order = spl
    t, b, g = (None, None, None) if start is None else start
    return _capi.accel_align(api, order, knots, basis, ctrl, s, a if meas is None else meas, q0 if q_init is None else q_init,
                             l0 if latency_init is None else latency_init, t, b, g, options=_capi.accel_alignment_options(api, **kw), covariance=True)


def _accel_far(api):
    q0, l0, start = accel_far_start()
    return _accel(api, start, q_init=q0, latency_init=l0)


def _accel_reference_far():
    spl, s, a, _, _, _ = accel_data()
    q0, l0, start = accel_far_start()
    return acr.align(spl, s, a, q0, l0, *start)


def _accel_nan():
    a = accel_data()[2].copy()
    a[137, 1] = np.nan
    return a


def _constant_gyro():
    return np.tile([0.1, 0.2, -0.3], (300, 1))


# name: (the call, the fields compared, the summary's status field, the status it ends with)
CASES = {
    "imu-searched": (lambda api: _imu(api), IMU_FIELDS, "gyro_status", _capi.ALIGN_OK),
    "imu-given-latency-held": (lambda api: _imu(api, q_init=_turned(imu_data()[5]["q"], 0.07, (5.0, -4.0, 3.0)), latency_init=imu_data()[5]["latency"],
                                                estimate_latency=0), IMU_FIELDS, "gyro_status", _capi.ALIGN_OK),
    "imu-bias-held": (lambda api: _imu(api, accel=False, estimate_gyro_bias=0), IMU_FIELDS, "gyro_status", _capi.ALIGN_OK),
    "imu-one-iteration": (lambda api: _imu(api, max_iterations=1), IMU_FIELDS, "gyro_status", _capi.ALIGN_NOT_CONVERGED),
    "imu-constant-measurements": (lambda api: _imu(api, accel=False, gyro=_constant_gyro()), IMU_FIELDS, "gyro_status", _capi.ALIGN_NO_PEAK),
    "imu-one-axis": (lambda api: _imu(api, one_axis=True), IMU_FIELDS, "gyro_status", _capi.ALIGN_DEGENERATE),
    "imu-far-start": (lambda api: _imu(api, q_init=imu_far_start()[0], latency_init=imu_far_start()[1]), IMU_FIELDS, "gyro_status", _capi.ALIGN_OK),
    "imu-rejected-steps": (_imu_rejected, IMU_FIELDS, "gyro_status", _capi.ALIGN_NOT_CONVERGED),
    "accel-stage-l": (lambda api: _accel(api), ACCEL_FIELDS, "status", _capi.ALIGN_OK),
    "accel-given": (lambda api: _accel(api, accel_given()), ACCEL_FIELDS, "status", _capi.ALIGN_OK),
    "accel-one-iteration": (lambda api: _accel(api, max_iterations=1), ACCEL_FIELDS, "status", _capi.ALIGN_NOT_CONVERGED),
    "accel-one-axis": (lambda api: _accel(api, accel_given(), one_axis=True), ACCEL_FIELDS, "status", _capi.ALIGN_NOT_POSITIVE_DEFINITE),
    "accel-nan": (lambda api: _accel(api, accel_given(), meas=_accel_nan()), ACCEL_FIELDS, "status", _capi.ALIGN_DEGENERATE),
    "accel-rejected-steps": (_accel_far, ACCEL_FIELDS, "status", _capi.ALIGN_OK),
}
for _held in ("rotation", "lever_arm", "bias", "gravity", "latency"):
    CASES["accel-held-" + _held] = (lambda api, _held=_held: _accel(api, accel_given(), **{"estimate_" + _held: 0}), ACCEL_FIELDS, "status", _capi.ALIGN_OK)
for _m in (2, 6):
    CASES.update({
        "camera-%d-searched" % _m: (lambda api, m=_m: _camera(api, m), CAMERA_FIELDS, "status", _capi.ALIGN_OK),
        "camera-%d-given" % _m: (lambda api, m=_m: _camera(api, m, camera_start(m)), CAMERA_FIELDS, "status", _capi.ALIGN_OK),
        "camera-%d-huber" % _m: (lambda api, m=_m: _camera(api, m, camera_start(m), huber_scale=0.15), CAMERA_FIELDS, "status", _capi.ALIGN_OK),
        "camera-%d-translation-held" % _m: (lambda api, m=_m: _camera(api, m, camera_start(m, shift=0.0), estimate_translation=0), CAMERA_FIELDS, "status",
                                            _capi.ALIGN_OK),
        "camera-%d-latency-held" % _m: (lambda api, m=_m: _camera(api, m, camera_start(m, dlat=0.0), estimate_latency=0), CAMERA_FIELDS, "status",
                                        _capi.ALIGN_OK),
        "camera-%d-two-iterations" % _m: (lambda api, m=_m: _camera(api, m, camera_start(m), max_iterations=2), CAMERA_FIELDS, "status",
                                          _capi.ALIGN_NOT_CONVERGED),
        "camera-%d-at-rest" % _m: (lambda api, m=_m: _camera(api, m, at_rest=True), CAMERA_FIELDS, "status", _capi.ALIGN_NO_PEAK),
        "camera-%d-rejected-steps" % _m: (lambda api, m=_m: _camera(api, m, camera_start(m, **CAMERA_FAR[m])), CAMERA_FIELDS, "status", _capi.ALIGN_OK),
    })

# the cases whose start makes the loop reject: (the reference module whose loop runs it, the reference's run, its status key)
REJECTED = {
    "imu-rejected-steps": (ir, _imu_reference_rejected, "gyro_status"),
    "accel-rejected-steps": (acr, _accel_reference_far, "status"),
    "camera-2-rejected-steps": (cref, lambda: _camera_reference_far(2), "status"),
    "camera-6-rejected-steps": (cref, lambda: _camera_reference_far(6), "status"),
}


@functools.lru_cache(maxsize=None)
def reference_run(name):
    """(the reference's result, the steps its loop rejected). The references' loops make every candidate with their module's
    apply(est, d) from the current point: two candidates in a row from the same point mean the first was rejected."""
    module, run, _ = REJECTED[name]
    made_from, original = [], module.apply

    def apply(est, d):
        made_from.append(est)
        return original(est, d)
    module.apply = apply
    try:
        result = run()
    finally:
        module.apply = original
    return result, sum(1 for a, b in zip(made_from, made_from[1:]) if a is b)


def run_case(api, name):
    """{field: raw bytes} of one case, its status checked."""
    call, fields, status_key, status = CASES[name]
    r = call(api)
    assert r[status_key] == status, (name, r[status_key], r["iterations"])
    if name in REJECTED:
        ref, rejected = reference_run(name)
        assert rejected >= 1 and (r[status_key], r["iterations"]) == (ref[REJECTED[name][2]], ref["iterations"]), (name, rejected, r["iterations"], ref["iterations"])
    return {field: b"" if r[field] is None else np.ascontiguousarray(r[field]).tobytes() for field in fields}


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {key: z[key] for key in z.files}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_are_the_parents(hip, name):
    golden = _golden()
    got = run_case(hip, name)
    for field in CASES[name][1]:
        assert got[field] == golden[name + "/" + field].tobytes(), "%s: %s differs from the parent commit's (%s)" % (name, field, str(golden["hipcc_version"]))


@pytest.mark.parametrize("name", sorted(REJECTED))
def test_the_rejected_step_cases_reject_in_the_reference_too(name):
    ref, rejected = reference_run(name)
    print(name, "rejected steps", rejected, "iterations", ref["iterations"], "status", ref[REJECTED[name][2]])
    assert rejected >= 1 and ref[REJECTED[name][2]] == CASES[name][3]


def test_the_golden_file_holds_every_field_of_every_case():
    golden = _golden()
    assert sorted(golden) == sorted(["hipcc_version"] + [name + "/" + field for name, (_, fields, _, _) in CASES.items() for field in fields])
    assert all(golden[key].dtype == np.uint8 for key in golden if key != "hipcc_version") and "version" in str(golden["hipcc_version"])
