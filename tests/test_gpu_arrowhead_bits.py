"""calico_camera_calibrate, calico_rig_calibrate and calico_camera_resect, bit for bit against the commit before their kernels took
their shared parts from one header (calico_amd/csrc/arrowhead_dev.hpp): every output array and every field of the summary of every case below has the
bytes that tests/golden/arrowhead_parent_bits.npz holds. tests/golden/make_arrowhead_parent_bits.py recorded them on an MI355X
from a library built from that commit; the file names the compiler (`hipcc --version`) that built it.

The golden file is re-recorded only by a commit that changes the arithmetic of these calls on purpose -- an order of summation, a
formula, a launch shape that an order depends on -- and says so; a refactor never does. A change of toolchain is the other
legitimate reason: another compiler may contract or schedule floating-point operations differently, and then the parent commit
is to be built with the new one and recorded again. The file holds recorded results only.

The cases are the smallest at which each shared piece can still go wrong:
  calibration  models 2 (N = 18, three accumulator tiles) and 6 (N = 11, one tile); eleven frames: nine of 20 pairs (the eight
               parts of the reduction wrap once), one of 70 pairs (a second trip of 64) and one of 3 pairs (below min_points: it
               takes no part). Runs: to convergence from given poses; max_iterations = 2; Huber; one intrinsic held; through the
               resection (no poses given); and calib_ref.fov_fixture, whose redo ladder climbs to lambda = 1e12 and DEGENERATE.
  rig          cameras of models 1, 3, 6 (M = 18: n_el = 365, two chunks of the reduction), six frames (the four parts wrap), one
               view of 70 pairs, one frame lacking a camera. Runs: from the resection's start; from a given start (a quarter of the
               standard perturbation: every step is accepted); twice the standard perturbation, seed 3 (the reference loop
               rejects its first three steps and converges in twelve); max_iterations = 2; Huber; and the chain fixture with
               reference camera 1 and min_shared_frames = 11, where camera 0 is held besides the reference.
  resection    models 2 and 5, the first five frames of resect_ref.fixture from the kernel's own start, with the covariance (the
               inverse of the 6x6 system is the shared one), without and with Huber.
The status that every case with a given start ends with is the numpy references' (lm_rule_ref.py), which the step tests hold to
the device's: the calibration of model 2 rejects its fourth step on the way.
"""
import functools
import os

import numpy as np
import pytest

import calib_ref as cr
import resect_ref as rr
import rig_ref as gr
from calico_amd import _capi
from calico_amd import synthetic as syn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arrowhead_parent_bits.npz")

CALIB_FIELDS = ("intrinsics", "q", "t", "rms", "n_used", "frame_status", "cov", "status", "iterations", "initial_cost", "final_cost",
                "total_rms", "frames_used", "pairs_used", "lambda_")
RESECT_FIELDS = ("q", "t", "rms", "n_used", "iterations", "status", "cov")
RIG_FIELDS = ("q_rig_camera", "t_rig_camera", "camera_status", "q_frame", "t_frame", "frame_status", "view_rms", "view_n_used", "view_status",
              "cov", "status", "iterations", "initial_cost", "final_cost", "total_rms", "cameras_used", "frames_used", "views_used",
              "pairs_used", "lambda_")


@functools.lru_cache(maxsize=None)
def calib_batch(model):
    """(k, offsets, pixels, points, poses): frames 0-8 see the first 20 planar points, frame 9 the first 70 points of the
    AprilGrid, frame 10 three points; pixels of the reference's projection plus 0.1 pixels of seeded noise."""
    k = np.array(syn._TRUE_INTRINSICS[model], float)
    poses = rr.true_poses()[:11]
    rng = np.random.default_rng(2718 + model)
    off, pix, pnt = [0], [], []
    for f, (R, t) in enumerate(poses):
        pts = syn.aprilgrid_points()[:70] if f == 9 else syn.planar_points()[:3 if f == 10 else 20]
        px, ok = rr.project(model, k, R, t, pts)
        assert ok.all(), f
        pix.append(px + 0.1 * rng.standard_normal(px.shape))
        pnt.append(pts)
        off.append(off[-1] + len(pts))
    return k, np.array(off, np.int64), np.concatenate(pix), np.concatenate(pnt), poses


@functools.lru_cache(maxsize=None)
def calib_start(model):
    """(k0, q0, t0): calib_ref.start_intrinsics and the truth perturbed by 0.005 N(0, 1)."""
    poses = calib_batch(model)[4]
    rng = np.random.default_rng(4321 + model)
    q0, t0 = [], []
    for R, t in poses:
        p = 0.005 * rng.standard_normal(6)
        q = rr.quat_of(rr.exp_so3(p[:3]) @ R)
        q0.append(q if q[3] >= 0 else -q)
        t0.append(t + p[3:])
    return cr.start_intrinsics(model), np.array(q0), np.array(t0)


def _calib(api, model, given=True, free_mask=None, **options):
    k, off, px, pt, _ = calib_batch(model)
    k0, q0, t0 = calib_start(model)
    return _capi.camera_calibrate(api, model, k0, off, px, pt, q_init=q0 if given else None, t_init=t0 if given else None, free_mask=free_mask,
                                  options=_capi.calibration_options(api, **options), covariance=True)


def _calib_fov(api):
    k, off, px, pt, _ = cr.fov_fixture()
    k0, q0, t0 = cr.fov_start()
    return _capi.camera_calibrate(api, 5, k0, off, px, pt, q_init=q0, t_init=t0, covariance=True)


@functools.lru_cache(maxsize=None)
def small_rig():
    """rig_ref.standard's cameras (models 1, 3, 6) over six frames of 20 planar points; camera 1's view of frame 2 has the first
    70 points of the AprilGrid, and frame 4 has no view of camera 2: 17 views."""
    models = (1, 3, 6)
    ks = [np.array(syn._TRUE_INTRINSICS[m], float) for m in models]
    cams, frames = gr._cams(gr.STANDARD_CAMS), rr.true_poses()[::3][:6]
    rng = np.random.default_rng(3141)
    vc, vf, off, pix, pnt = [], [], [0], [], []
    for f, frame in enumerate(frames):
        for c, cam in enumerate(cams):
            if (c, f) == (2, 4):
                continue
            pts = syn.aprilgrid_points()[:70] if (c, f) == (1, 2) else syn.planar_points()[:20]
            R, t = gr.camera_from_chart(cam, frame)
            px, ok = rr.project(models[c], ks[c], R, t, pts)
            assert ok.all(), (c, f)
            vc.append(c); vf.append(f); off.append(off[-1] + len(pts))
            pix.append(px + 0.1 * rng.standard_normal(px.shape)); pnt.append(pts)
    return gr.Rig(models, ks, len(frames), np.array(vc, np.int32), np.array(vf, np.int64), np.array(off, np.int64), np.concatenate(pix),
                  np.concatenate(pnt), cams, frames)


def _rig(api, rig, start=None, **options):
    s = (None,) * 4 if start is None else start
    return _capi.rig_calibrate(api, rig.models, rig.ks, rig.n_frames, rig.view_camera, rig.view_frame, rig.view_offsets, rig.pixels,
                               rig.points, s[0], s[1], s[2], s[3], options=_capi.rig_options(api, **options), covariance=True)


def _resect(api, model, **options):
    k, off, px, pt, _ = rr.fixture(model, 0.1)
    return _capi.camera_resect(api, model, k, off[:6], px[:off[5]], pt[:off[5]], options=_capi.resection_options(api, **options), covariance=True)


def _near(rig):
    return gr.perturbed_start(rig, scale=0.005)


# name: (the call, the fields compared, the status it ends with)
CASES = {
    "calib-2": (lambda api: _calib(api, 2), CALIB_FIELDS, _capi.CALIB_OK),
    "calib-6": (lambda api: _calib(api, 6), CALIB_FIELDS, _capi.CALIB_OK),
    "calib-2-two-iterations": (lambda api: _calib(api, 2, max_iterations=2), CALIB_FIELDS, _capi.CALIB_NOT_CONVERGED),
    "calib-6-two-iterations": (lambda api: _calib(api, 6, max_iterations=2), CALIB_FIELDS, _capi.CALIB_NOT_CONVERGED),
    "calib-2-huber": (lambda api: _calib(api, 2, huber_scale=0.15), CALIB_FIELDS, _capi.CALIB_OK),
    "calib-6-huber": (lambda api: _calib(api, 6, huber_scale=0.15), CALIB_FIELDS, _capi.CALIB_OK),
    "calib-2-held": (lambda api: _calib(api, 2, free_mask=(1,) * 10 + (0,)), CALIB_FIELDS, _capi.CALIB_OK),
    "calib-6-held": (lambda api: _calib(api, 6, free_mask=(1, 1, 1, 0)), CALIB_FIELDS, _capi.CALIB_OK),
    "calib-2-resected": (lambda api: _calib(api, 2, given=False), CALIB_FIELDS, _capi.CALIB_OK),
    "calib-6-resected": (lambda api: _calib(api, 6, given=False), CALIB_FIELDS, _capi.CALIB_OK),
    "calib-fov-redo-ladder": (_calib_fov, CALIB_FIELDS, _capi.CALIB_DEGENERATE),
    "resect-2": (lambda api: _resect(api, 2), RESECT_FIELDS, _capi.RESECT_OK),
    "resect-5": (lambda api: _resect(api, 5), RESECT_FIELDS, _capi.RESECT_OK),
    "resect-2-huber": (lambda api: _resect(api, 2, huber_scale=0.15), RESECT_FIELDS, _capi.RESECT_OK),
    "resect-5-huber": (lambda api: _resect(api, 5, huber_scale=0.15), RESECT_FIELDS, _capi.RESECT_OK),
    "rig": (lambda api: _rig(api, small_rig()), RIG_FIELDS, _capi.RIG_OK),
    "rig-started": (lambda api: _rig(api, small_rig(), _near(small_rig())), RIG_FIELDS, _capi.RIG_OK),
    "rig-rejected-steps": (lambda api: _rig(api, small_rig(), gr.perturbed_start(small_rig(), seed=3, scale=0.04)), RIG_FIELDS, _capi.RIG_OK),
    "rig-two-iterations": (lambda api: _rig(api, small_rig(), _near(small_rig()), max_iterations=2), RIG_FIELDS, _capi.RIG_NOT_CONVERGED),
    "rig-huber": (lambda api: _rig(api, small_rig(), _near(small_rig()), huber_scale=0.15), RIG_FIELDS, _capi.RIG_OK),
    "rig-chain-held": (lambda api: _rig(api, gr.chain(0.1), min_shared_frames=11, reference_camera=1), RIG_FIELDS, _capi.RIG_OK),
}


def run_case(api, name):
    """{field: raw bytes} of one case, its status checked."""
    call, fields, status = CASES[name]
    r = call(api)
    assert np.all(r.status == status), (name, r.status)      # (the resection's status is one per frame)
    return {field: np.ascontiguousarray(getattr(r, field)).tobytes() for field in fields}


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


def test_the_golden_file_holds_every_field_of_every_case():
    golden = _golden()
    assert sorted(golden) == sorted(["hipcc_version"] + [name + "/" + field for name, (_, fields, _) in CASES.items() for field in fields])
    assert all(golden[key].dtype == np.uint8 for key in golden if key != "hipcc_version") and "version" in str(golden["hipcc_version"])
