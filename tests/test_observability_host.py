"""Observability entry points without a GPU: the C ABI declares and exports them, the kernel keeps no scratch and spills
nothing in either size class (from the compiler's own remarks), and the CPU reference recipe the GPU tests compare with
(observability_ref.py) reproduces the spectral gaps and weak counts of their scenes from the oracle alone."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import helpers  # noqa: E402
import observability_ref as R  # noqa: E402
from calico_amd import _capi, synthetic as syn  # noqa: E402

NAMES = ["default_observability_options", "observability_compute", "observability_info", "observability_get_spectrum",
         "observability_get_directions", "observability_get_block", "observability_get_matrix"]


def test_observability_entries_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "calico_hip.h")).read()
    for n in NAMES:
        assert re.search(r"\bcalico_%s\s*\(" % n, header), n
        assert n in _capi.ABI_SYMBOLS
    assert "obs_kernels.hip" in entry.HIP_SOURCES
    entry.build_hip()
    lib = C.CDLL(_capi.hip_library_path())
    for n in NAMES + ["debug_observability_info"]:
        getattr(lib, "calico_" + n)
    m = re.search(r"typedef struct calico_observability_options \{(.*?)\}", header, re.S)
    fields = re.findall(r"\b(double|int32_t)\s+(\w+)(?:\[(\d+)\])?;", m.group(1))
    assert [f[1] for f in fields] == [f[0] for f in _capi.ObservabilityOptions._fields_]
    assert sum((8 if t == "double" else 4) * int(k or 1) for t, _, k in fields) == C.sizeof(_capi.ObservabilityOptions) == 32
    o = _capi.ObservabilityOptions()
    lib.calico_default_observability_options(C.byref(o))
    assert 0.0 < o.weak_threshold < 1e-6 and o.weak_threshold == R.WEAK_THRESHOLD
    assert 0.0 < o.min_relative_pivot < 1e-6
    assert list(o.reserved) == [0, 0, 0, 0]
    lib.calico_observability_compute.restype = C.c_int32
    assert lib.calico_observability_compute(None, None) == _capi.INVALID_ARGUMENT


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_observability_kernel_scratch_free():
    res = helpers.kernel_resources("obs_kernels.hip")
    ks = {k: v for k, v in res.items() if "observability_kernel" in k}
    assert len(ks) == 2, sorted(res)      # the in-LDS and the global-workspace class
    for k, v in ks.items():
        print(k, v)
        assert v["ScratchSize"] == 0, (k, v)
        assert v["VGPRs Spill"] == 0, (k, v)
        assert v["VGPRs"] <= 128, (k, v)      # 1024 threads: four waves per SIMD


def test_no_atomics_in_the_kernel_source():
    for name in ("obs_kernels.hip", "reduced_system.hpp"):      # the kernel and the prologue it shares with covariance_kernel
        src = open(os.path.join(entry.CSRC, name)).read()
        code = "\n".join(line.split("//")[0] for line in src.splitlines())
        assert not re.search(r"\batomic\w*\s*\(", code), name


@pytest.mark.parametrize("name", list(R.TABLE_SCENES))
def test_reference_recipe_reproduces_the_table(name):
    """The scenes of the GPU tests satisfy their own gap condition, from the oracle alone (solved scenes: the oracle's own
    solve; the GPU tests use the device's values, which agree to the solver's tolerance)."""
    oracle = helpers.oracle_api()
    mk, iters, n_weak = R.TABLE_SCENES[name]
    scene = mk()
    ref = syn.build_problem(oracle, scene)
    if iters:
        o = oracle.default_options()
        o.minimizer_progress_to_stdout = 0
        o.max_num_iterations = iters
        ref.problem.solve(o)
    _, mc = R.border_layout(ref, scene)
    r = R.reference(ref, mc, scene.order)
    lam = r["lam"]
    assert lam is not None and r["band_pivot"] > 1e-12
    k = R.weak_count(lam)
    print("%s: border %d kept %d, lowest %s, next %.3e, max %.3f" % (name, mc, int(r["keep"].sum()), lam[:max(k, 3)], lam[k], lam[-1]))
    assert k == n_weak
    expect = {"camera 1, start": (23, 23, 2.21), "camera 2 (OpenCV8), start": (29, 29, 3.53), "free chart pose (gauge), start": (29, 29, 2.21),
              "scale-and-bias IMU, solved": (45, 42, 3.54), "VectorNav IMU, solved": (61, 58, 3.52), "VectorNav IMU, solved, robust": (61, 58, 3.57)}[name]
    assert (mc, int(r["keep"].sum())) == expect[:2] and abs(lam[-1] - expect[2]) < 0.02
    if k:
        assert np.abs(lam[:k]).max() <= 5.8e-15      # exact deficiencies: rounding noise
        assert lam[k] / np.abs(lam[:k]).max() >= R.GAP
        assert lam[k] >= 8.0e-7                      # the smallest eigenvalue of a merely weak direction (the gauge scene's)
        # the null space lives in the named blocks only
        layout, _ = R.border_layout(ref, scene)
        kept_pos = np.cumsum(r["keep"]) - 1
        P = R.projector(r["V"], k)
        named = set(R.null_space_blocks(name, ref, scene))
        outside = 0.0
        for b, (off, t) in layout.items():
            rows = [kept_pos[j] for j in range(off, off + t) if r["keep"][j]]
            if b not in named and rows:
                outside += float(np.trace(P[np.ix_(rows, rows)]))
        assert outside <= 1e-8 * k
    else:
        assert lam[0] >= 8.0e-7


def test_reference_finds_the_solved_camera_scene_trajectory_deficient():
    oracle = helpers.oracle_api()
    scene = R.small_scene(camera_model=1, imu=False)
    ref = syn.build_problem(oracle, scene)
    o = oracle.default_options()
    o.minimizer_progress_to_stdout = 0
    ref.problem.solve(o)
    _, mc = R.border_layout(ref, scene)
    r = R.reference(ref, mc, scene.order)
    print("camera 1, solved: natural-order band pivot %.3e" % r["band_pivot"])
    assert r["band_pivot"] < 1e-12 and r["lam"] is None
