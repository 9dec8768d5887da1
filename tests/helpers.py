"""Test helpers: loads the CPU oracle (test infrastructure) and the HIP library."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from calico_amd import _capi  # noqa: E402

ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_LIB = os.path.join(ORACLE_DIR, "libcalico_oracle.so")
_oracle = None


def build_oracle():
    subprocess.check_call(["make", "-s", "-C", ORACLE_DIR])


def oracle_lib():
    if not os.path.exists(ORACLE_LIB):
        build_oracle()
    return C.CDLL(ORACLE_LIB)


def oracle_api():
    """The CPU oracle behind the same ABI shape (prefix oracle_). Checker only."""
    global _oracle
    if _oracle is None:
        _oracle = _capi.CApi(oracle_lib(), "oracle_", has_device=False)
    return _oracle


def hip_api():
    return _capi.load_hip()


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


# ---- what the test files share: scenes, solving, reading a problem's state, the two-rank harness, the compiler's remarks ----

def small_scene(camera_model=1, n_cameras=2, imu=True, imu_model=2, robust=False, seed=7, noise=True, **kw):
    """The small seeded scene of the parity, covariance, observability and prediction tests. noise=False: exact measurements."""
    from calico_amd import synthetic as syn
    return syn.make_scene(n_cameras, camera_model, imu, imu_model, cam_rate=10.0, imu_rate=50.0, duration=3.0,
                          segment_duration=3.0 / 23.9, pixel_noise=0.1 if noise else 0.0,
                          gyro_noise=1e-3 if noise else 0.0, accel_noise=1e-2 if noise else 0.0, robust=robust,
                          seed=seed, **kw)


def full_size_scene(index):
    """The shape of configs[3] / configs[4] with scale-and-bias IMUs: the VectorNav model of the configs themselves is
    singular with a free IMU rotation (see test_imu_models_parity_and_unobserved_columns of test_gpu_covariance.py)."""
    import numpy as np
    from calico_amd import synthetic as syn
    if index == 3:
        return syn.make_scene(4, 1, True, 2, cam_rate=20.0, imu_rate=200.0, duration=8.7, chart="april", seed=0xCA11C0 + 3,
                              pixel_noise=0.1, gyro_noise=1.7e-4 * np.sqrt(200.0), accel_noise=2e-3 * np.sqrt(200.0),
                              robust=True, segment_duration=8.7 / 23.9)
    return syn.make_scene(8, 1, True, 2, cam_rate=20.0, imu_rate=200.0, duration=21.7, chart="april", seed=0xCA11C0 + 4,
                          pixel_noise=0.1, gyro_noise=1.7e-4 * np.sqrt(200.0), accel_noise=2e-3 * np.sqrt(200.0),
                          robust=True, outlier_fraction=0.02, repeats=2, segment_duration=21.7 / 47.9, n_imus=2)


def solve(P, api, iters=50):
    o = api.default_options()
    o.minimizer_progress_to_stdout = 0
    o.max_num_iterations = iters
    return P.solve(o)


def copy_values(src, dst):
    """Parameter values of one built problem into another built from the same scene."""
    for b, n in dict(src.problem._sizes).items():
        dst.problem.set_param_block(b, src.problem.get_param_block(b, n))


def _state(built, scene):
    """({block id: values}, [every sensor's (residuals, valid flags)]) of a built problem."""
    P = built.problem
    vals = {b: P.get_param_block(b, n) for b, n in dict(P._sizes).items()}
    res = [P.residuals(sid, s.n, 2 if s.kind == _capi.SENSOR_CAMERA else 3) for sid, s in zip(built.sensor_ids, scene.sensors)]
    return vals, res


def border_layout(built, scene):
    """{block id: (offset, tangent size)} of the dense border and its dimension, derived from the scene's structure alone: the
    free blocks a residual uses, control points excluded, in block-id order (the order calico_num_effective_parameters
    documents)."""
    import numpy as np
    from calico_amd import synthetic as syn
    free, used = {}, set()
    bodies = built.bodies      # (body 0 first; a scene without further bodies has just that one)
    for spec, b in zip(scene.bodies, bodies):
        pc = np.broadcast_to(np.asarray(spec.points_constant, bool), (len(spec.points),))
        for blk, c in zip(b["point_blocks"], pc):
            free[int(blk)] = (not c, 3)
        free[b["t"]] = (not spec.pose_constant, 3)
        free[b["q"]] = (not spec.pose_constant, 3)
    free[built.gravity_block] = (False, 3)
    for s, b in zip(scene.sensors, built.sensor_blocks):
        free[b["intrinsics"]] = (s.enable_intrinsics, len(s.intrinsics))
        free[b["t"]] = (s.enable_extrinsics, 3)
        free[b["q"]] = (s.enable_extrinsics, 3)
        free[b["latency"]] = (s.enable_latency, 1)
        if s.n:
            used.update([b["intrinsics"], b["t"], b["q"], b["latency"]])
            if s.kind == _capi.SENSOR_CAMERA:
                which = syn.body_indices(s)
                for k in np.unique(which):
                    used.update(int(bodies[k]["point_blocks"][i]) for i in np.unique(s.point_idx[which == k]))
                    used.update([bodies[k]["t"], bodies[k]["q"]])
    out, off = {}, 0
    for b in sorted(free):
        if free[b][0] and b in used:
            out[b] = (off, free[b][1])
            off += free[b][1]
    return out, off


class _DevArray:
    """A device buffer of n doubles at `ptr` for torch.as_tensor."""
    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (ptr, False), "version": 2}


def _run_rank_threads(ranks, per_rank, install, read, write):
    """The harness of run_ranks and run_oracle_ranks: one thread per handle of `ranks` runs per_rank(built); their exchange
    callbacks (made here, installed with install(built, callback)) meet at a barrier, sum what read(*args) gives in rank
    order and hand the total to write(*args, total). Every wait has a limit, and an error in one rank aborts the barrier so
    that the others fail at once. Returns (results rank by rank, exchanges of every rank)."""
    import threading
    world = len(ranks)
    meet = threading.Barrier(world, timeout=120)
    staged = [None] * world
    results, errors = [None] * world, []
    n_calls = [0] * world

    def make_allreduce(rank):
        def allreduce(ctx, *args):
            try:
                n_calls[rank] += 1
                staged[rank] = read(*args)
                meet.wait()
                total = staged[0].copy()
                for k in range(1, world):
                    total += staged[k]
                meet.wait()
                write(*args, total)
                return 0
            except Exception as e:      # noqa: BLE001 (an exception must not unwind through the C frames)
                errors.append(repr(e))
                meet.abort()
                return 1
        return allreduce

    for r, b in enumerate(ranks):
        install(b, make_allreduce(r))

    def run(r):
        try:
            results[r] = per_rank(ranks[r])
        except Exception as e:      # noqa: BLE001
            errors.append(repr(e))
            meet.abort()
    th = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=180)
    assert not errors, errors
    assert not any(t.is_alive() for t in th), "a rank did not finish in time"
    return results, n_calls


def run_ranks_counting(api, scene, values, per_rank, world=2):
    """`world` ranks on one device: each a handle built from `scene` with the parameter values `values` ({block id: values})
    installed, sharded to its time window (calico_problem_set_shard) with a host exchange (sum in rank order).
    per_rank(built) runs in a thread per rank. Returns (its results rank by rank, the number of exchanges of every rank)."""
    import torch
    from calico_amd import synthetic as syn
    ranks = []
    for r in range(world):
        b = syn.build_problem(api, scene)
        for blk, v in values.items():
            b.problem.set_param_block(blk, v)
        b.problem.set_shard(r, world)
        ranks.append(b)

    def read(buf, n, strm):
        torch.cuda.ExternalStream(strm).synchronize()
        return torch.as_tensor(_DevArray(buf, n), device="cuda").cpu().numpy().copy()

    def write(buf, n, strm, total):
        torch.as_tensor(_DevArray(buf, n), device="cuda").copy_(torch.from_numpy(total).cuda())
        torch.cuda.synchronize()
    return _run_rank_threads(ranks, per_rank, lambda b, cb: b.problem.set_allreduce(cb), read, write)


def run_ranks(api, scene, values, per_rank, world=2):
    """run_ranks_counting's results alone."""
    return run_ranks_counting(api, scene, values, per_rank, world)[0]


run_two_ranks = run_ranks      # (the name the two-rank tests use)


def run_oracle_ranks(scene, per_rank, world):
    """run_ranks on the CPU oracle: `world` handles of `scene`, each sharded to its window (oracle_problem_set_shard), with the
    oracle's host all-reduce summing in rank order; per_rank(built) runs in a thread per rank. Returns its results rank by rank."""
    import numpy as np
    from calico_amd import synthetic as syn
    oracle = oracle_api()
    fn_t = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.POINTER(C.c_double), C.c_int64)
    set_allreduce = oracle.lib.oracle_problem_set_allreduce
    set_allreduce.argtypes, set_allreduce.restype = [C.c_void_p, fn_t, C.c_void_p], C.c_int32
    ranks, keep = [], []
    for r in range(world):
        b = syn.build_problem(oracle, scene)
        assert oracle.lib.oracle_problem_set_shard(b.problem.h, r, world) == 0
        ranks.append(b)

    def install(b, callback):
        keep.append(fn_t(callback))
        assert set_allreduce(b.problem.h, keep[-1], None) == 0

    def write(buf, n, total):
        np.ctypeslib.as_array(buf, shape=(n,))[:] = total
    return _run_rank_threads(ranks, per_rank, install, lambda buf, n: np.ctypeslib.as_array(buf, shape=(n,)).copy(), write)[0]


def kernel_resources(source):
    """{kernel's mangled name: {remark: value}} of one file of calico_amd/csrc, from the compiler's own remarks
    (-Rpass-analysis=kernel-resource-usage) of a device-only compile with the build's flags."""
    import re
    import __graft_entry__ as entry
    src = os.path.join(entry.CSRC, source)
    flags = [f for f in entry.HIP_FLAGS if f != "-fPIC"] + entry.HIP_FILE_FLAGS.get(source, [])
    r = subprocess.run([entry.HIPCC] + flags + ["--cuda-device-only", "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    res, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[a-zA-Z/]+\])?: (\d+)", line)
        if m and name:
            res[name][m.group(1).strip()] = int(m.group(2))
    return res
