"""Scenes with several rigid bodies, mixed camera models and unordered registration, shared by
test_problem_structure_oracle.py (oracle alone) and test_gpu_problem_structure.py (device against oracle).

All of them are the 3 s trajectory of helpers.small_scene (10 Hz knots, 30 segments) with two cameras and an IMU unless a
test says otherwise: body 0 is small_scene's 6 x 6 chart at the origin, body 1 a 5 x 4 chart (20 points a frame: enough
for the frame path's 16) beside and behind it, tilted."""
import numpy as np

from calico_amd import _capi, synthetic as syn

MIXED_RIGS = [(1, 3, 7), (2, 5), (4, 6)]


def chart1(**kw):
    """Body 1: 20 points, 0.6 m beside body 0 and 0.3 m behind it (farther from the cameras, so that
    no model's projection is pushed to the edge of its range when the rig comes close), tilted by about 15 degrees."""
    return syn.rigid_body(syn.planar_points(1.0, 0.75, 0.25), t=(0.6, 0.1, -0.3), rotvec=(0.0, 0.25, 0.05), **kw)


def sparse_chart(**kw):
    """Six points: fewer than the 16 a frame needs for the frame path."""
    return syn.rigid_body(syn.planar_points(0.5, 0.25, 0.25), t=(0.6, 0.1, -0.3), rotvec=(0.0, 0.25, 0.05), **kw)


def scene(models=1, bodies=None, cam_rate=10.0, imu_rate=50.0, robust=True, seed=7, n_cameras=None, pixel_noise=0.1, gyro_noise=1e-3, accel_noise=1e-2, **kw):
    """small_scene's trajectory and noise with a camera model per camera and further bodies."""
    models = list(np.atleast_1d(models))
    n = n_cameras if n_cameras is not None else max(2, len(models))
    if len(models) == 1:
        models = models * n
    return syn.make_scene(n, models, True, 2, cam_rate=cam_rate, imu_rate=imu_rate, duration=3.0, segment_duration=3.0 / 23.9,
                          pixel_noise=pixel_noise, gyro_noise=gyro_noise, accel_noise=accel_noise, robust=robust, seed=seed,
                          extra_bodies=[chart1()] if bodies is None else bodies, **kw)


def second_chart_free(model=1, seed=7, **kw):
    """Body 0 constant, body 1 free: a rig of two cameras of one model plus IMU."""
    return scene(model, [chart1(free_pose=True)], seed=seed, **kw)


def mixed_rig(models, seed=7, **kw):
    """One camera per model against two constant charts."""
    return scene(models, seed=seed, **kw)


# the scenes of the converged-solve comparisons: {name: constructor}. test_problem_structure_oracle.py proves on the oracle
# alone that their minima determine every estimate to 1e-7, which is what gives the 1e-6 device bound its meaning -- and
# says why they carry a thousandth of small_scene's noise.
_QUIET = dict(pixel_noise=1e-4, gyro_noise=1e-6, accel_noise=1e-5)
SOLVE_SCENES = {
    "second chart free, model 1": lambda: second_chart_free(1, seed=11, **_QUIET),
    "mixed rig (1, 3, 7)": lambda: mixed_rig((1, 3, 7), seed=33, **_QUIET),
}


def column_limit_rig(models=(1, 2)):
    """Every camera estimates intrinsics, extrinsics and latency against a free second body: 21 calibration columns for
    model 1 (8 + 6 + 1 + 6: stays on the frame path), 24 for model 2 (11 + 6 + 1 + 6: one more than the path's 23)."""
    sc = scene(models, [chart1(free_pose=True)])
    for s in sc.sensors:
        if s.kind == _capi.SENSOR_CAMERA:
            s.enable_extrinsics = s.enable_latency = True
    return sc


def interleave_bodies(sc):
    """Every camera's observations re-registered frame by frame with the bodies alternating inside each frame
    (b0, b1, b0, b1, ... while both last); returns the permutations for syn.reorder (None for the other sensors)."""
    perms = []
    for s in sc.sensors:
        if s.kind != _capi.SENSOR_CAMERA:
            perms.append(None)
            continue
        body = syn.body_indices(s)
        order = []
        for st in np.unique(s.stamps):
            rows = [list(np.nonzero((s.stamps == st) & (body == b))[0]) for b in np.unique(body)]
            while any(rows):
                for r in rows:
                    if r:
                        order.append(r.pop(0))
        perms.append(np.array(order))
    return perms


def registration_variants(sc, seed=3):
    """{name: scene} of one scene registered in another order: a random permutation of every sensor (IMU included), the
    reverse order, and three calls per sensor interleaved across the sensors (over the random permutation)."""
    rng = np.random.default_rng(seed)
    rand = [rng.permutation(s.n) for s in sc.sensors]
    return {
        "random": syn.reorder(sc, rand),
        "reverse": syn.reorder(sc, [np.arange(s.n)[::-1] for s in sc.sensors]),
        "three calls": syn.reorder(sc, rand, calls=syn.interleaved_calls(sc, 3)),
    }, {"random": rand, "reverse": [np.arange(s.n)[::-1] for s in sc.sensors], "three calls": rand}


def expected_plan(sc, frame_path):
    """What the plan must count for a scene (order 6): `frame_path(camera index, body) -> bool` says which layouts the test
    expects on the frame path. Returns frames (one per camera, body and stamp there), camera cells (one per camera, body and
    segment there) and IMU cells (one per IMU sensor and segment)."""
    frames = cam_cells = imu_cells = 0
    for c, s in enumerate(sc.sensors):
        seg = syn.spline_index(sc.knots, sc.order, s.stamps)
        if s.kind != _capi.SENSOR_CAMERA:
            imu_cells += len(np.unique(seg))
            continue
        body = syn.body_indices(s)
        for b in np.unique(body):
            if frame_path(c, int(b)):
                frames += len(np.unique(s.stamps[body == b]))
                cam_cells += len(np.unique(seg[body == b]))
    return dict(frames=frames, cam_cells=cam_cells, imu_cells=imu_cells)
