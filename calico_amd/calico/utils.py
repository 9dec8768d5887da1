"""Host-side helpers with the names and return conventions of the reference's calico/utils.py (numpy only; the
reference leans on OpenCV for the homography and the image resize). Cheap CPU work either side of the optimiser:
they stay on the host by design."""
from typing import Dict, List, Tuple

import numpy as np

from .. import _calico


def ComputeRmseHeatmapAndFeatureCount(measurement_residual_pairs, image_width: int, image_height: int,
                                      num_rows: int = 8, num_cols: int = 12):
    """utils.py:12-50. Bins the residuals of GetMeasurementResidualPairs() over a num_rows x num_cols grid of the
    image. Returns (heatmap stretched to image_height x image_width by nearest neighbour, binned RMSE, counts);
    empty bins are NaN like the reference's 0/0."""
    n = len(measurement_residual_pairs)
    px = np.array([m.pixel for m, _ in measurement_residual_pairs], float).reshape(n, 2)
    sq = np.array([float(np.sum(np.asarray(r) ** 2)) for _, r in measurement_residual_pairs], float)
    col = np.clip(np.floor(px[:, 0] / image_width * num_cols).astype(int), 0, num_cols - 1)
    row = np.clip(np.floor(px[:, 1] / image_height * num_rows).astype(int), 0, num_rows - 1)
    count = np.zeros((num_rows, num_cols))
    total = np.zeros((num_rows, num_cols))
    np.add.at(count, (row, col), 1.0)
    np.add.at(total, (row, col), sq)
    with np.errstate(invalid="ignore", divide="ignore"):
        rmse = np.sqrt(total / count)
    # nearest-neighbour stretch: destination pixel centre -> source bin
    r_idx = np.minimum((np.arange(image_height) * num_rows) // image_height, num_rows - 1)
    c_idx = np.minimum((np.arange(image_width) * num_cols) // image_width, num_cols - 1)
    return rmse[np.ix_(r_idx, c_idx)], rmse, count


def DetectionsToCameraMeasurements(detections: Dict[int, np.ndarray], stamp: float, seq: int):
    """utils.py:81-99: one CameraMeasurement per detected feature; model_id is 0 (single chart)."""
    out = []
    for feature_id, point in detections.items():
        m = _calico.CameraMeasurement()
        m.id.stamp = stamp
        m.id.image_id = seq
        m.id.model_id = 0
        m.id.feature_id = int(feature_id)
        m.pixel = np.asarray(point, float)
        out.append(m)
    return out


def _normalising_transform(p):
    c = p.mean(axis=0)
    d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    s = np.sqrt(2.0) / d if d > 0 else 1.0
    return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])


def _homography(src, dst, refine_iterations=10):
    """dst ~ H [src; 1]: normalised DLT, then a few Gauss-Newton steps on the transfer error (what
    cv2.findHomography does after its linear estimate)."""
    Ts, Td = _normalising_transform(src), _normalising_transform(dst)
    s = (Ts @ np.c_[src, np.ones(len(src))].T).T
    d = (Td @ np.c_[dst, np.ones(len(dst))].T).T
    A = np.zeros((2 * len(src), 9))
    A[0::2, 0:3] = s
    A[0::2, 6:9] = -d[:, :1] * s
    A[1::2, 3:6] = s
    A[1::2, 6:9] = -d[:, 1:2] * s
    h = np.linalg.svd(A)[2][-1]
    H = np.linalg.inv(Td) @ h.reshape(3, 3) @ Ts
    H /= H[2, 2]
    sh = np.c_[src, np.ones(len(src))]
    for _ in range(refine_iterations):
        q = sh @ H.T
        w = q[:, 2]
        r = np.c_[q[:, 0] / w - dst[:, 0], q[:, 1] / w - dst[:, 1]].ravel()
        J = np.zeros((2 * len(src), 8))
        J[0::2, 0:3] = sh / w[:, None]
        J[0::2, 6:8] = -(q[:, 0] / w ** 2)[:, None] * sh[:, :2]
        J[1::2, 3:6] = sh / w[:, None]
        J[1::2, 6:8] = -(q[:, 1] / w ** 2)[:, None] * sh[:, :2]
        step = np.linalg.lstsq(J, -r, rcond=None)[0]
        H = (H.ravel() + np.r_[step, 0.0]).reshape(3, 3)
        if np.abs(step).max() < 1e-14:
            break
    return H


def InitializePinholeAndPoses(all_detections: List[Dict[int, np.ndarray]], model_definition: Dict[int, np.ndarray]
                              ) -> Tuple[list, List[np.ndarray], List[np.ndarray]]:
    """utils.py:102-186: Zhang's closed-form pinhole initialisation from planar-chart detections.
    Returns ([fx, fy, s, cx, cy], [R_chart_camera per frame], [t_chart_camera per frame])."""
    Hs = []
    V = np.zeros((2 * len(all_detections), 6))

    def v(H, i, j):   # Zhang (1998) eq. (7), columns i, j of H
        a, b = H[:, i], H[:, j]
        return np.array([a[0] * b[0], a[0] * b[1] + a[1] * b[0], a[1] * b[1],
                         a[2] * b[0] + a[0] * b[2], a[2] * b[1] + a[1] * b[2], a[2] * b[2]])
    for i, det in enumerate(all_detections):
        ids = list(det.keys())
        pix = np.array([det[k] for k in ids], float).reshape(-1, 2)
        mod = np.array([np.asarray(model_definition[k], float)[:2] for k in ids]).reshape(-1, 2)
        H = _homography(mod, pix)
        Hs.append(H)
        V[2 * i] = v(H, 0, 1)
        V[2 * i + 1] = v(H, 0, 0) - v(H, 1, 1)
    # b = [B11, B12, B22, B13, B23, B33] of B = K^-T K^-1 up to scale: null vector of V
    b = np.linalg.svd(V)[2][-1]
    if b[0] < 0:
        b = -b
    B11, B12, B22, B13, B23, B33 = b
    den = B11 * B22 - B12 ** 2
    v0 = (B12 * B13 - B11 * B23) / den
    lam = B33 - (B13 ** 2 + v0 * (B12 * B13 - B11 * B23)) / B11
    alpha = np.sqrt(lam / B11)
    beta = np.sqrt(lam * B11 / den)
    gamma = -B12 * alpha ** 2 * beta / lam
    u0 = gamma * v0 / beta - B13 * alpha ** 2 / lam
    intrinsics = [alpha, beta, gamma, u0, v0]
    K = np.array([[alpha, gamma, u0], [0, beta, v0], [0, 0, 1.0]])
    K_inv = np.linalg.inv(K)
    R_chart_camera, t_chart_camera = [], []
    for H in Hs:
        Rt = K_inv @ H
        scale = 0.5 * (np.linalg.norm(Rt[:, 0]) + np.linalg.norm(Rt[:, 1]))
        if Rt[2, 2] < 0:          # the chart is in front of the camera
            scale = -scale
        R = np.c_[Rt[:, 0] / scale, Rt[:, 1] / scale, np.cross(Rt[:, 0] / scale, Rt[:, 1] / scale)]
        U, _, Vt = np.linalg.svd(R)
        R = U @ Vt                # nearest rotation
        t = Rt[:, 2] / scale
        R_chart_camera.append(R.T)
        t_chart_camera.append(-R.T @ t)
    return intrinsics, R_chart_camera, t_chart_camera


def InitializePoses(camera, all_detections: List[Dict[int, np.ndarray]], model_definition: Dict[int, np.ndarray]
                    ) -> Tuple[List[np.ndarray], List[np.ndarray], np.ndarray]:
    """The pose half of InitializePinholeAndPoses for ANY camera model, at the camera's own model and current intrinsics, on
    the device (Camera.EstimateChartPoses: homography start from the unprojected pixels, then Levenberg-Marquardt on the
    library's projection). Returns ([R_chart_camera per frame], [t_chart_camera per frame], ok (n_frames,) bool) in the
    conventions of InitializePinholeAndPoses; a frame that is not ok (too few points, no start, not converged, degenerate)
    carries the identity and must not be handed to FitSpline. With the smoothing fit (Trajectory.FitSplineSmooth) such frames
    are simply left out: its roughness penalty carries the spline across the gap they leave, where FitSpline would drop the
    control points of a gap longer than the spline's support to zero (Trajectory.FitSplineCV is the same fit with the penalty's
    weight lambda chosen from a grid by cross-validation: no noise level of the poses is needed). A frame that IS ok can still be wrong (the planar two-fold
    ambiguity, few corners, a mis-decoded tag: a small RMS at a pose tenths of a radian off): for frames not known to be bad use
    the robust fit, Trajectory.FitSplineRobust, whose per-pose weights single them out."""
    r = camera.EstimateChartPoses(all_detections, model_definition)
    R_chart_camera, t_chart_camera = [], []
    for (x, y, z, w), t in zip(r["q"], r["t"]):
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        R_chart_camera.append(R.T)
        t_chart_camera.append(-R.T @ t)
    return R_chart_camera, t_chart_camera, np.asarray(r["status"]) == 0


def _rotation_of(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


# InitialIntrinsics' mid-range values for the parameters that have no neutral value
_FOV_START = 1.0          # FieldOfView's w (radians): w -> 0 is the pinhole, but the model's derivative in w vanishes there
_EUCM_ALPHA_START = 0.5   # ExtendedUnifiedCamera's alpha: at its neutral value 0, beta has no effect on the projection


def InitialIntrinsics(model, pinhole) -> np.ndarray:
    """Starting intrinsics of any camera model from Zhang's pinhole [fx, fy, s, cx, cy] (InitializePinholeAndPoses), in the
    model's own layout [f, cx, cy, distortion...]. The rule: on the optical axis the model's projection agrees with the pinhole
    of focal length (fx + fy) / 2 and principal point (cx, cy) to first order (these models have one focal length and no skew).
    Distortion starts at its neutral value where the model has one -- OpenCv5 / OpenCv8: all zero; KannalaBrandt: all zero
    (equidistant); DoubleSphere: xi = 0, alpha = 0; UnifiedCamera: alpha = 0 -- and at a documented mid-range value otherwise:
    FieldOfView w = 1 rad, with f = f_pinhole w / (2 tan(w / 2)); ExtendedUnifiedCamera alpha = 0.5, beta = 1 (on the axis its
    focal length is the pinhole's for every alpha)."""
    fx, fy, _, cx, cy = [float(v) for v in pinhole]
    f = 0.5 * (fx + fy)
    m = int(model)
    if m == 1:
        return np.array([f, cx, cy, 0, 0, 0, 0, 0], float)
    if m == 2:
        return np.array([f, cx, cy, 0, 0, 0, 0, 0, 0, 0, 0], float)
    if m == 3:
        return np.array([f, cx, cy, 0, 0, 0, 0], float)
    if m == 4:
        return np.array([f, cx, cy, 0.0, 0.0])
    if m == 5:
        w = _FOV_START
        return np.array([f * w / (2.0 * np.tan(0.5 * w)), cx, cy, w])
    if m == 6:
        return np.array([f, cx, cy, 0.0])
    if m == 7:
        return np.array([f, cx, cy, _EUCM_ALPHA_START, 1.0])
    raise ValueError("no camera model %r" % (model,))


def InitializeIntrinsicsAndPoses(camera, all_detections: List[Dict[int, np.ndarray]], model_definition: Dict[int, np.ndarray]
                                 ) -> Tuple[np.ndarray, List[np.ndarray], List[np.ndarray], np.ndarray]:
    """InitializePinholeAndPoses for ANY camera model: Zhang's closed form gives the pinhole part, InitialIntrinsics maps it to
    the camera's model, and Camera.CalibrateIntrinsics (on the device) estimates the model's intrinsics jointly with the pose of
    every frame under the library's own projection, so that Optimize starts at a minimum of its camera term. The camera's
    intrinsics are set to the estimate. Returns (intrinsics, [R_chart_camera per frame], [t_chart_camera per frame],
    ok (n_frames,) bool) in the conventions of InitializePoses; a frame that is not ok carries the identity and must not be handed
    to FitSpline. Raises RuntimeError when the estimation does not end with status OK.

    The start has zero distortion. That does not reach the minimum for strong OpenCV distortion: the numpy reference of the tests,
    started this way, converged for the KannalaBrandt fixture and did not for the OpenCv5 / OpenCv8 fixtures (k1 = -0.31). For
    such a lens start from a data sheet or a previous calibration (Camera.SetIntrinsics, then Camera.CalibrateIntrinsics)."""
    pinhole, _, _ = InitializePinholeAndPoses(all_detections, model_definition)
    camera.SetIntrinsics(InitialIntrinsics(camera.GetModel(), pinhole))
    r = camera.CalibrateIntrinsics(all_detections, model_definition)
    if r["status"] != 0:
        raise RuntimeError("Error: the intrinsic calibration ended with status %d after %d iterations" % (r["status"], r["iterations"]))
    R_chart_camera, t_chart_camera = [], []
    for q, t in zip(r["q"], r["t"]):
        R = _rotation_of(q)
        R_chart_camera.append(R.T)
        t_chart_camera.append(-R.T @ t)
    return r["intrinsics"], R_chart_camera, t_chart_camera, np.asarray(r["frame_status"]) == 0


def InitializeRig(cameras, rig_frames: List[Dict[int, Dict[int, np.ndarray]]], model_definition: Dict[int, np.ndarray], options=None
                  ) -> Tuple[List[np.ndarray], List[np.ndarray], np.ndarray]:
    """The second and every further camera of the start of Optimize: calico.CalibrateRig (on the device) estimates the extrinsics
    of every camera but the reference camera (cameras[0] unless options says otherwise), whose frame is the rig's, jointly with
    the pose of every rig frame, from the chart detections of all cameras at their current intrinsics. rig_frames[f] maps a
    camera's index in `cameras` to its detections {feature id: pixel} at an instant the rig stood still relative to the chart.
    Sets the extrinsics of the cameras that took part. Returns ([R_chart_rig per rig frame], [t_chart_rig per rig frame],
    ok (n_frames,) bool) in the conventions of InitializePoses -- what Trajectory.FitSpline takes, now also for the frames the
    reference camera never saw; a frame that is not ok carries the identity and must not be handed to FitSpline (with
    Trajectory.FitSplineSmooth such frames are simply left out: the penalty carries the spline across the gap, and
    Trajectory.FitSplineCV chooses the penalty's weight by cross-validation; for frames that are
    wrong and not known to be, Trajectory.FitSplineRobust downweights them and says which). options: None or
    a dict of calico_rig_options fields. Raises RuntimeError when the estimation does not end with status OK (before anything is
    changed)."""
    r = _calico.CalibrateRig(list(cameras), rig_frames, model_definition, options)
    if r["status"] != 0:
        raise RuntimeError("Error: the rig calibration ended with status %d after %d iterations (%d cameras, %d views used)"
                           % (r["status"], r["iterations"], r["cameras_used"], r["views_used"]))
    R_chart_rig, t_chart_rig = [], []
    for q, t in zip(r["q_frame"], r["t_frame"]):
        R = _rotation_of(q)
        R_chart_rig.append(R.T)
        t_chart_rig.append(-R.T @ t)
    return R_chart_rig, t_chart_rig, np.asarray(r["frame_status"]) == 0


# where the three bias entries start in the intrinsics of the IMU models (gyroscope and accelerometer models share their layouts):
# ScaleOnly [s]: none; ScaleAndBias [s, b 3]; VectorNav [scale 3, misalignment 6, bias 3]
_IMU_BIAS_AT = {1: None, 2: 1, 3: 9}


def InitializeImu(trajectory, gyroscope, accelerometer=None, world_model=None, options=None) -> dict:
    """The IMU side of the start of Optimize, from the trajectory of the camera side (Trajectory.FitSpline over the poses of
    InitializePoses / InitializeIntrinsicsAndPoses) and the sensors' registered measurements: Trajectory.AlignImu (on the device)
    estimates the rotation rig <- gyroscope, the gyroscope's bias and the IMU's latency as a minimum of Optimize's own gyroscope
    term and, with an accelerometer, the world's gravity and the accelerometer's bias. Sets the rotation of the extrinsics, the
    latency and the bias intrinsics of the gyroscope and of the accelerometer (which shares rotation and latency; the scale and
    every other intrinsic are left as they are, and a scale-only model has no bias to set) and, given a world model and an
    accelerometer, its gravity. options: None or a dict of calico_imu_alignment_options fields. Returns AlignImu's dict.
    Raises RuntimeError when a part does not end with status OK, or for a sensor whose model has not been set (before anything
    is changed)."""
    for sensor in (gyroscope, accelerometer):
        if sensor is not None and int(sensor.GetModel()) not in _IMU_BIAS_AT:
            raise RuntimeError("Error: InitializeImu does not know where IMU model %d keeps its bias" % int(sensor.GetModel()))
    r = trajectory.AlignImu(gyroscope, accelerometer, options)
    if r["gyro_status"] != 0:
        raise RuntimeError("Error: the gyroscope alignment ended with status %d after %d iterations (%d samples)"
                           % (r["gyro_status"], r["iterations"], r["gyro_samples"]))
    if accelerometer is not None and r["accel_status"] != 0:
        raise RuntimeError("Error: the accelerometer alignment ended with status %d (%d samples)" % (r["accel_status"], r["accel_samples"]))
    x, y, z, w = r["q_rig_gyro"]
    for sensor, bias in ((gyroscope, r["gyro_bias"]), (accelerometer, r["accel_bias"])):
        if sensor is None:
            continue
        T = sensor.GetExtrinsics()
        T.rotation = [w, x, y, z]
        sensor.SetExtrinsics(T)
        sensor.SetLatency(float(r["latency"]))
        at = _IMU_BIAS_AT[int(sensor.GetModel())]
        if at is not None:
            k = np.array(sensor.GetIntrinsics(), float)
            k[at:at + 3] = bias
            sensor.SetIntrinsics(k)
    if world_model is not None and accelerometer is not None:
        world_model.SetGravity([float(v) for v in r["gravity_world"]])
    return r


def InitializeAccelerometer(trajectory, accelerometer, world_model=None, options=None) -> dict:
    """The accelerometer's start of Optimize where no data sheet gives its mounting, after InitializeImu (which leaves it the
    gyroscope's rotation and latency and does not touch its translation): Trajectory.AlignAccelerometer (on the device) estimates
    its rotation, its lever arm, its bias, the world's gravity and its latency as a minimum of Optimize's own accelerometer term
    with the trajectory held, started at the sensor's current rotation and latency. Sets the rotation AND the translation of the
    extrinsics, the latency, the bias intrinsics (the scale and every other intrinsic are left as they are, and a scale-only
    model has no bias to set) and, given a world model, its gravity. options: None or a dict of calico_accel_alignment_options
    fields. Returns AlignAccelerometer's dict. Raises RuntimeError when the alignment does not end with status OK, or for a
    sensor whose model has not been set, before anything is changed."""
    if int(accelerometer.GetModel()) not in _IMU_BIAS_AT:
        raise RuntimeError("Error: InitializeAccelerometer does not know where IMU model %d keeps its bias" % int(accelerometer.GetModel()))
    r = trajectory.AlignAccelerometer(accelerometer, options)
    if r["status"] != 0:
        raise RuntimeError("Error: the accelerometer alignment ended with status %d (linear stage %d) after %d iterations (%d samples)"
                           % (r["status"], r["linear_status"], r["iterations"], r["samples"]))
    x, y, z, w = r["q_rig_accel"]
    T = accelerometer.GetExtrinsics()
    T.rotation = [w, x, y, z]
    T.translation = [float(v) for v in r["t_rig_accel"]]
    accelerometer.SetExtrinsics(T)
    accelerometer.SetLatency(float(r["latency"]))
    at = _IMU_BIAS_AT[int(accelerometer.GetModel())]
    if at is not None:
        k = np.array(accelerometer.GetIntrinsics(), float)
        k[at:at + 3] = r["bias"]
        accelerometer.SetIntrinsics(k)
    if world_model is not None:
        world_model.SetGravity([float(v) for v in r["gravity_world"]])
    return r


def InitializeCamera(trajectory, camera, world_model, options=None) -> dict:
    """The start of Optimize for a camera that is not synchronised with the trajectory's camera, from the trajectory
    (Trajectory.FitSpline over the reference camera's poses) and this camera's registered measurements of rigid body 0:
    Trajectory.AlignCamera (on the device) estimates the extrinsics T_rig_camera and the latency at the camera's current
    intrinsics as a minimum of Optimize's own camera term with the trajectory held. Sets the camera's extrinsics and latency.
    options: None or a dict of calico_camera_alignment_options fields. Returns AlignCamera's dict. Raises RuntimeError when the
    alignment does not end with status OK, before anything is changed."""
    r = trajectory.AlignCamera(camera, world_model, options)
    if r["status"] != 0:
        raise RuntimeError("Error: the camera alignment ended with status %d after %d iterations (%d frames)"
                           % (r["status"], r["iterations"], r["frames_used"]))
    x, y, z, w = r["q_rig_camera"]
    T = camera.GetExtrinsics()
    T.rotation = [w, x, y, z]
    T.translation = [float(v) for v in r["t_rig_camera"]]
    camera.SetExtrinsics(T)
    camera.SetLatency(float(r["latency"]))
    return r


def CharacterizeImuNoise(stamps, samples, options=None) -> dict:
    """The noise of a gyroscope or an accelerometer from a recording of the sensor at rest (calico_imu_allan, on the device): the
    overlapping Allan variance of the three axes over a logarithmic grid of cluster sizes and per axis the IEEE-952 coefficients
    (white noise N, bias instability B, rate random walk K; quantisation and ramp through options["terms"]). stamps (n,) evenly
    spaced (a gap raises RuntimeError: split the log), samples (n, 3). options: None or a dict of calico_allan_options fields
    (points_per_decade, max_tau_fraction, terms, cluster_sizes). Returns a dict: cluster_sizes, tau, rel_err, avar (c, 3), noise
    (one dict per axis) and summary (N_pooled, sigma_at_rate, bias_drift_over_recording, ...)."""
    return _calico.CharacterizeImuNoise([float(t) for t in np.asarray(stamps, float).ravel()], np.asarray(samples, float).reshape(-1, 3), options)


def SetImuNoise(sensor, noise, rate_hz=None) -> float:
    """SetMeasurementNoise of a gyroscope or an accelerometer from CharacterizeImuNoise's dict: sigma = N_pooled sqrt(rate_hz), the
    optimiser's one scalar per sensor. rate_hz None: the rate of the sensor's own registered measurements, (n - 1) / (last stamp
    - first stamp). Returns the sigma that was set. Raises RuntimeError where the characterisation holds no white noise or the
    sensor has no rate."""
    rate = float(sensor.MeasurementRate() if rate_hz is None else rate_hz)
    sensor.ApplyNoise(noise, rate)
    return sensor.GetMeasurementNoise()
