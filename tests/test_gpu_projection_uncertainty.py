"""calico_projection_uncertainty against a reference built from the oracle and numpy alone.

Scene: the small two-camera + IMU scene (camera 0: free intrinsics, constant extrinsics -- the rig frame; camera 1: free
intrinsics AND extrinsics), OpenCv5 and DoubleSphere, solved, then calico_covariance_compute.
Reference: Sigma is the oracle's dense inverse (as tests/test_gpu_covariance.py obtains it) restricted to the camera's blocks
and lifted to AMBIENT form (quaternion rows through the manifold's plus Jacobian). The Jacobian is a central difference (step
1e-6) of  oracle_project_point o (p_r -> R(q / |q|)^T (p_r - t))  in ambient k, q, t: the lifted Sigma annihilates the
radial direction of q, so no tangent convention enters the reference. The 3-D point of a pixel is range x the unit vector the
device's unprojection returns, ACCEPTED only after the oracle projects it back onto the pixel within 1e-9 px -- from there on
the reference is the oracle's.
Tolerance: ten times the reference's own finite-difference floor (the same construction at step 1e-5 against step 1e-6),
entries relative to the pixel's larger variance; both are printed per model, camera and frame.
Measured (MI355X), floor / device against step 1e-6, sigma over the image: OpenCv5 camera 0 (both frames) 3.4e-7 / 3.3e-7,
0.017 .. 0.021 px; camera 1 CAMERA 3.3e-7 / 3.3e-7, 0.020 .. 0.029 px; camera 1 RIG 3.8e-7 / 3.8e-7, 0.017 .. 0.021 px;
DoubleSphere camera 0 (both frames) 1.8e-6 / 1.8e-6, 0.040 .. 0.095 px; camera 1 CAMERA 8.5e-7 / 7.5e-7, 0.045 .. 0.115 px;
camera 1 RIG 1.2e-6 / 1.1e-6, 0.037 .. 0.106 px: the device sits at the reference's own floor."""
import functools

import numpy as np
import pytest

from calico_amd import _capi, synthetic as syn
from camera_ref import oracle_project
from helpers import _state, border_layout, small_scene, solve

pytestmark = pytest.mark.gpu

RANGE = 2.5
# 9 x 7 pixels over the 1280 x 800 image, corners included
PIXELS = np.array([[u, v] for v in np.linspace(0.0, 800.0, 7) for u in np.linspace(0.0, 1280.0, 9)])


def _rot(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


class Solved:
    """One solved scene with its covariance on the device and the oracle's Sigma, built once per model."""

    def __init__(self, hip, oracle, model):
        self.scene = small_scene(camera_model=model, n_cameras=2, imu=True)
        self.model = model
        self.gpu, ref = syn.build_problem(hip, self.scene), syn.build_problem(oracle, self.scene)
        P = self.gpu.problem
        solve(P, hip)
        self.dim = P.covariance_compute()[0]
        for b, n in dict(P._sizes).items():
            ref.problem.set_param_block(b, P.get_param_block(b, n))
        _, _, H = ref.problem.evaluate()
        keep = np.nonzero(np.diag(H) != 0.0)[0]
        S = np.zeros_like(H)
        S[np.ix_(keep, keep)] = np.linalg.inv(H[np.ix_(keep, keep)])
        self.sigma = S[H.shape[0] - self.dim:, H.shape[0] - self.dim:]
        self.layout, dim = border_layout(self.gpu, self.scene)
        assert dim == self.dim

    def ambient_sigma(self, cam, with_extrinsics):
        """Sigma of [k | q (4) | t] of camera `cam` in ambient form; blocks that are constant (or left out) are zero."""
        P, blk = self.gpu.problem, self.gpu.sensor_blocks[cam]
        K = len(self.scene.sensors[cam].intrinsics)
        rows, lift = [], np.zeros((K + 7, 0))
        parts = [(blk["intrinsics"], 0, np.eye(K))]
        if with_extrinsics:
            x, y, z, w = P.get_param_block(blk["q"], 4)
            parts += [(blk["q"], K, np.array([[w, z, -y], [-z, w, x], [y, -x, w], [-x, -y, -z]])), (blk["t"], K + 4, np.eye(3))]
        for b, at, L in parts:
            if b not in self.layout:
                continue
            off, size = self.layout[b]
            rows += list(range(off, off + size))
            col = np.zeros((K + 7, size))
            col[at:at + L.shape[0]] = L
            lift = np.hstack([lift, col])
        return lift @ self.sigma[np.ix_(rows, rows)] @ lift.T

    def reference(self, cam, frame, pts_c, h):
        """[s_uu, s_uv, s_vv] of the points (camera frame, at the current extrinsics) from central differences of step h."""
        P, blk, model = self.gpu.problem, self.gpu.sensor_blocks[cam], self.model
        K = len(self.scene.sensors[cam].intrinsics)
        k, q, t = P.get_param_block(blk["intrinsics"], K), P.get_param_block(blk["q"], 4), P.get_param_block(blk["t"], 3)
        p_r = pts_c @ _rot(q).T + t

        def f(theta):
            px, ok = oracle_project(model, theta[:K], (p_r - theta[K + 4:]) @ _rot(theta[K:K + 4]))
            assert ok.all()
            return px
        theta = np.concatenate([k, q, t])
        J = np.zeros((len(pts_c), 2, K + 7))
        for c in range(K + 7 if frame == _capi.FRAME_RIG else K):
            e = np.zeros(K + 7)
            e[c] = h
            J[:, :, c] = (f(theta + e) - f(theta - e)) / (2 * h)
        S = self.ambient_sigma(cam, frame == _capi.FRAME_RIG)
        C = np.einsum("nik,kl,njl->nij", J, S, J)
        return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 1, 1]], 1)


@functools.lru_cache(maxsize=None)
def _solved(hip, oracle, model):
    return Solved(hip, oracle, model)


def _rel(a, b):
    return (np.abs(a - b) / np.maximum(b[:, 0], b[:, 2])[:, None]).max()


@pytest.mark.parametrize("model", [1, 4])
def test_uncertainty_map_against_the_oracle(model, hip, oracle):
    S = _solved(hip, oracle, model)
    P = S.gpu.problem
    for cam in (0, 1):
        sid = S.gpu.sensor_ids[cam]
        K = len(S.scene.sensors[cam].intrinsics)
        b, vb = P.sensor_unproject(sid, PIXELS)
        k = P.get_param_block(S.gpu.sensor_blocks[cam]["intrinsics"], K)
        back, ok = oracle_project(model, k, RANGE * b[vb])
        assert vb.sum() >= 40 and ok.all() and np.abs(back - PIXELS[vb]).max() <= 1e-9      # the points ARE the pixels' (oracle)
        for frame in (_capi.FRAME_CAMERA, _capi.FRAME_RIG):
            cov, v = P.projection_uncertainty(sid, PIXELS, RANGE, frame)
            assert np.array_equal(v, vb) and np.all(cov[~v] == 0.0)
            ref6, ref5 = S.reference(cam, frame, RANGE * b[v], 1e-6), S.reference(cam, frame, RANGE * b[v], 1e-5)
            floor, err = _rel(ref5, ref6), _rel(cov[v], ref6)
            sd = np.sqrt(np.maximum(cov[v][:, 0], cov[v][:, 2]))
            print("model %d camera %d frame %d: %d pixels, sigma %.3f .. %.3f px, finite-difference floor %.2e, device against step 1e-6 %.2e"
                  % (model, cam, frame, v.sum(), sd.min(), sd.max(), floor, err))
            assert err <= 10.0 * floor
            # positive semidefinite, every pixel
            det = cov[v][:, 0] * cov[v][:, 2] - cov[v][:, 1] ** 2
            assert np.all(cov[v][:, 0] >= 0.0) and np.all(cov[v][:, 2] >= 0.0)
            assert np.all(det >= -1e-12 * cov[v][:, 0] * cov[v][:, 2])
        # camera 0's extrinsics are constant: the rig frame adds nothing; camera 1's are free: it must
        cam_map, _ = P.projection_uncertainty(sid, PIXELS, RANGE, _capi.FRAME_CAMERA)
        rig_map, _ = P.projection_uncertainty(sid, PIXELS, RANGE, _capi.FRAME_RIG)
        if cam == 0:
            assert np.array_equal(cam_map, rig_map)
        else:
            assert not np.array_equal(cam_map, rig_map)


def test_preconditions_arguments_and_what_the_call_leaves_alone(hip, oracle):
    scene = small_scene(camera_model=1, n_cameras=2, imu=True)
    a, b = syn.build_problem(hip, scene), syn.build_problem(hip, scene)
    Pa, Pb = a.problem, b.problem
    sid = a.sensor_ids[1]
    with pytest.raises(_capi.CalicoError) as e:
        Pa.projection_uncertainty(sid, PIXELS, RANGE)
    assert e.value.code == _capi.FAILED_PRECONDITION and "calico_covariance_compute" in e.value.message
    assert Pa.projection_uncertainty(sid, np.zeros((0, 2)), RANGE)[0].shape == (0, 3)      # n == 0 is OK and asks for nothing
    o = hip.default_options()
    o.minimizer_progress_to_stdout = 0
    o.max_num_iterations = 3
    Pa.solve(o)
    Pb.solve(o)
    Pa.covariance_compute()
    Pb.covariance_compute()
    dense = Pa.covariance_dense()
    cov, v = Pa.projection_uncertainty(sid, PIXELS, RANGE)
    assert v.sum() >= 40
    assert np.array_equal(Pa.covariance_dense(), dense)
    cov2, _ = Pa.projection_uncertainty(sid, PIXELS, RANGE)
    assert cov.tobytes() == cov2.tobytes()
    # the argument rules that need a handle
    gyro = [s for s, spec in zip(a.sensor_ids, scene.sensors) if spec.kind == _capi.SENSOR_GYROSCOPE][0]
    for args, word in (((len(scene.sensors), PIXELS, RANGE), "unknown sensor"), ((gyro, PIXELS, RANGE), "not a camera"),
                       ((sid, PIXELS, 0.0), "range"), ((sid, PIXELS, float("nan")), "range"), ((sid, PIXELS, RANGE, 2), "frame")):
        with pytest.raises(_capi.CalicoError) as e:
            Pa.projection_uncertainty(*args)
        assert e.value.code == _capi.INVALID_ARGUMENT and word in e.value.message, (word, e.value.message)
    assert Pa.projection_uncertainty(sid, np.zeros((0, 2)), RANGE)[0].shape == (0, 3)
    # a solve after the call is bit-identical to one without it
    o.max_num_iterations = 4
    sa, sb = Pa.solve(o), Pb.solve(o)
    assert sa.final_cost == sb.final_cost and sa.num_iterations == sb.num_iterations
    va, vb = _state(a, scene), _state(b, scene)
    for blk in va[0]:
        assert va[0][blk].tobytes() == vb[0][blk].tobytes(), blk
    # a structural change (one more observation) invalidates the stored covariance for this reader too
    Pa.covariance_compute()
    Pa.projection_uncertainty(sid, PIXELS, RANGE)
    s1 = scene.sensors[1]
    Pa.add_camera_residuals(sid, s1.meas[:1], s1.stamps[:1], np.array([a.bodies[0]["id"]], np.int32), np.array([a.point_blocks[s1.point_idx[0]]], np.int32))
    with pytest.raises(_capi.CalicoError) as e:
        Pa.projection_uncertainty(sid, PIXELS, RANGE)
    assert e.value.code == _capi.FAILED_PRECONDITION
