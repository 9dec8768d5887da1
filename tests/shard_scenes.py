"""The scenes and worlds of the sharding tests (tests/test_gpu_shard_windows.py on the device, tests/test_host_abi.py on the
CPU oracle), the partition rule of calico_amd/csrc/shard.hpp restated in numpy from a scene's stamps, and the partition every
case is expected to run on -- pinned, so that a changed generator cannot quietly turn an empty-window case into a full one.

A plain module (numpy only). The block counts were computed once with windows() below and checked by hand against the rule
for the short cases (tests/cpp/shard_windows_check.cpp holds two of them)."""
import functools

import numpy as np


def _small():
    import test_gpu_multirank
    return test_gpu_multirank._scene()


def _case_scene(**kw):
    import test_gpu_linear_step
    return test_gpu_linear_step.make_case_scene(**kw)


# mixed_rate: what the scene is cut at (fraction of the 3 s) -- settled so that the ranks of a world of three take different
# evaluation routes: rank 0's window lies before the cut (10 Hz frames, one or two per segment: the fused route), the others'
# behind it (30 Hz, three and more frames per segment: Jacobian launch + cell expansion)
MIXED_RATE_CUT = 0.6
MIXED_RATE_DURATION = 3.0


def _mixed_rate():
    """Two cameras + IMU over 3 s on 10 Hz knots; the cameras run at 30 Hz, and before the cut only every third frame is kept."""
    from calico_amd import synthetic as syn
    scene = syn.make_scene(2, 1, True, 2, cam_rate=30.0, imu_rate=50.0, duration=MIXED_RATE_DURATION,
                           segment_duration=MIXED_RATE_DURATION / 23.9, pixel_noise=0.1, gyro_noise=1e-3, accel_noise=1e-2,
                           robust=True, seed=3)
    cut = MIXED_RATE_CUT * MIXED_RATE_DURATION
    for s in scene.sensors:
        if s.kind != 0:
            continue
        frame = np.rint((s.stamps - s.latency_true) * 30.0).astype(np.int64)
        keep = (s.stamps >= cut) | (frame % 3 == 0)
        s.meas, s.stamps, s.point_idx, s.is_outlier = s.meas[keep], s.stamps[keep], s.point_idx[keep], s.is_outlier[keep]
    return scene


def _small_outliers():
    """`small` with 5 % gross outliers among the camera observations."""
    import test_gpu_multirank
    return test_gpu_multirank._scene(outlier_fraction=0.05)


def _small_scene(**kw):
    import helpers
    return helpers.small_scene(**kw)


_MAKERS = {
    "small": _small,
    "short": lambda: _case_scene(n_cp=10),
    "two_segments": lambda: _case_scene(n_cp=7),
    "gap": lambda: _case_scene(n_cp=92, unobserved="middle"),
    "tail": lambda: _case_scene(n_cp=92, unobserved="tail"),
    "mixed_rate": _mixed_rate,
    "order4": lambda: _small_scene(order=4, robust=True, seed=5),
    "order7": lambda: _small_scene(order=7, robust=True, seed=5),
    "free_points": lambda: _small_scene(camera_model=1, imu=True, free_points=True, seed=5),
    "small_outliers": _small_outliers,
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """The scene of that name; built once, shared, not to be modified."""
    return _MAKERS[name]()


def segments(sc):
    """(number of spline segments, every observation's segment sensor by sensor)."""
    from calico_amd import synthetic as syn
    nseg = len(sc.knots) - 2 * (sc.order - 1) - 1
    return nseg, [syn.spline_index(sc.knots, sc.order, s.stamps) if s.n else np.zeros(0, np.int32) for s in sc.sensors]


def windows(sc, world):
    """shard.hpp restated: (boundaries b[0..world], blocks per rank). Cut r is the first segment boundary at which the running
    block count reaches r / world of the total."""
    nseg, segs = segments(sc)
    per_seg = np.zeros(nseg, np.int64)
    for sg in segs:
        assert sg.size == 0 or (sg.min() >= 0 and sg.max() < nseg)
        per_seg += np.bincount(sg, minlength=nseg)
    prefix = np.concatenate([[0], np.cumsum(per_seg)])
    total = int(prefix[-1])
    bounds = [0] + [int(np.argmax(prefix * world >= total * r)) for r in range(1, world)] + [nseg]
    return bounds, [int(prefix[bounds[r + 1]] - prefix[bounds[r]]) for r in range(world)]


def n_rows(sc):
    """Residual rows of the scene."""
    return sum(s.n * s.dim for s in sc.sensors)


# (scene, world) -> (segments, boundaries, blocks per rank): the partition the case runs on
PARTITIONS = {
    ("small", 3): (30, [0, 11, 21, 30], [900, 820, 740]),
    ("small", 5): (30, [0, 6, 12, 19, 24, 30], [492, 492, 572, 412, 492]),
    ("small", 8): (30, [0, 4, 8, 12, 16, 19, 23, 27, 30], [326, 328, 330, 326, 246, 328, 328, 248]),
    ("short", 3): (5, [0, 2, 4, 5], [218, 222, 102]),
    ("short", 5): (5, [0, 2, 2, 3, 4, 5], [218, 0, 110, 112, 102]),                       # one segment above a fifth of the blocks
    ("short", 8): (5, [0, 1, 2, 2, 3, 4, 4, 5, 5], [104, 114, 0, 110, 112, 0, 102, 0]),   # more ranks than segments
    ("two_segments", 2): (2, [0, 1, 2], [104, 102]),
    ("two_segments", 3): (2, [0, 1, 2, 2], [104, 102, 0]),
    ("two_segments", 5): (2, [0, 1, 1, 2, 2, 2], [104, 0, 102, 0, 0]),
    ("gap", 3): (87, [0, 25, 62, 87], [560, 560, 558]),                                   # rank 1 spans the unobserved stretch
    ("gap", 8): (87, [0, 9, 18, 28, 50, 58, 68, 78, 87], [216, 216, 224, 188, 208, 224, 224, 178]),
    ("tail", 3): (87, [0, 16, 33, 87], [380, 388, 350]),                                  # the last window: mostly unobserved control points
    ("mixed_rate", 3): (30, [0, 17, 24, 30], [1430, 1438, 1320]),                         # the cut lies in segment 18
    ("order4", 3): (30, [0, 11, 21, 30], [900, 820, 740]),
    ("order7", 3): (30, [0, 11, 21, 30], [900, 820, 740]),
    ("free_points", 3): (30, [0, 11, 21, 30], [900, 820, 740]),
    ("small_outliers", 3): (30, [0, 11, 21, 30], [900, 820, 740]),
}

CASES = sorted(k for k in PARTITIONS if k[0] != "small_outliers")      # (the tagging test's scene has a test of its own)


# Whole worlds solving together: (scene, world), and the solver options of a scene where they differ from the two-rank tests'
# (test_gpu_multirank.py: the defaults, 25 iterations, sync_every 4).
#
# The bar of those solves -- every iteration's cost and the estimates to 1e-9 of the single-rank solve's -- is a condition on the
# case as well as on the code: the sharded solve differs from the single-rank one by the association of one sum (1e-16), and
# what an iteration makes of that is the conditioning of its damped system. So a case is admitted only with options under which
# the REFERENCE alone, sharded to the same world (helpers.run_oracle_ranks), stays within 1e-11 of its own single-rank solve,
# a hundredth of the bar (tests/test_host_abi.py::test_oracle_worlds_solve_like_its_single_rank holds every case to that).
# `short` does not with the defaults: it is test_gpu_linear_step's fixture for single LM steps, the whole motion squeezed into
# 0.45 s over ten control points (start cost 4e13, the scaled H numerically singular), and once the trust region has grown
# past 1e3 the oracle's own world of five is 2.6e-7 off its single-rank solve at a rejected candidate (4e-9 at an accepted
# step). It runs from the radius its home module takes its steps at (1.0) with the radius capped at 100, so that the
# damping keeps every iteration's system conditioned: the reference's world of five then agrees with its single-rank solve
# to 4e-14 (worlds of 3 and 8: 4e-13 and 9e-14), through two rejected steps and 23 accepted ones.
# (order7 with a world of three is not among them yet: see test_worlds_solve_like_a_single_rank)
SOLVE_CASES = [("small", 3), ("small", 8), ("short", 5), ("mixed_rate", 3)]
SOLVE_OPTIONS = {"short": dict(initial_trust_region_radius=1.0, max_trust_region_radius=100.0)}
REFERENCE_SOLVE_BAR = 1e-11


def solve_options(api, name):
    o = api.default_options()
    o.minimizer_progress_to_stdout = 0
    o.max_num_iterations = 25
    o.sync_every = 4
    for key, value in SOLVE_OPTIONS.get(name, {}).items():
        setattr(o, key, value)
    return o


def partition(name, world):
    """(boundaries, blocks per rank) of a case, recomputed from the scene's stamps and held against the pinned values."""
    nseg, bounds, counts = PARTITIONS[(name, world)]
    sc = scene(name)
    assert segments(sc)[0] == nseg and sum(counts) == sc.num_blocks, (name, world)
    assert windows(sc, world) == (bounds, counts), (name, world, windows(sc, world))
    return bounds, counts
