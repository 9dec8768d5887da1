"""Prediction covariance / leverage without a GPU: the reference's own invariants on the small scenes (prediction_ref.py),
the declared and exported entry points, the default options, and the new kernel's scratch / spill budget from the
compiler's remarks."""
import ctypes as C
import os
import re
import shutil
import sys

import numpy as np
import pytest

import helpers
import prediction_ref as pr
from calico_amd import _capi, synthetic as syn
from helpers import small_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

ENTRY_POINTS = ["default_prediction_options", "prediction_covariance"]


@pytest.mark.parametrize("name,kw,kept", [("plain", dict(), 252), ("robust", dict(robust=True), 252), ("order 4", dict(order=4), 240)])
def test_reference_invariants(name, kw, kept):
    """Hat matrix of the small scene at its start values: the traces of all blocks add up to the number of kept columns, every
    row's leverage lies in [0, 1], every block's eigenvalues too."""
    scene = small_scene(camera_model=1, imu=True, **kw)
    ref = syn.build_problem(helpers.oracle_api(), scene)
    R = pr.Reference(ref)
    assert R.n_kept == kept
    total, lo, hi = 0.0, 1.0, 0.0
    for first, n, d in pr.sensor_rows(scene):
        P, beta = R.blocks(R.J_fit, first, n, d)
        total += float(np.einsum("nii->", P))
        h = np.einsum("nii->ni", P)
        lo, hi = min(lo, h.min()), max(hi, h.max())
        ev = np.linalg.eigvalsh(0.5 * (P + P.transpose(0, 2, 1)))
        assert ev.min() >= -1e-12 and ev.max() <= 1.0 + 1e-12
        assert np.all(np.abs(P) <= beta[:, :, None] * beta[:, None, :] * (1 + 1e-12))
    print("%s: sum of traces %d %+.1e, row leverages in [%.1e, %.3f]" % (name, kept, total - kept, lo, hi))
    assert abs(total - kept) <= 1e-9 * kept
    assert 0.0 <= lo and hi <= 1.0


def test_apply_loss_off_uses_the_plain_rows():
    """Without the loss the rows are those of the whitened residual: equal to the corrected ones on a scene without a loss
    function, different on a robust one (same column order)."""
    plain, robust = small_scene(camera_model=1, imu=True), small_scene(camera_model=1, imu=True, robust=True)
    a, a0 = pr.build_pair(helpers.oracle_api(), plain)
    assert np.array_equal(pr.dense_jacobian(a), pr.dense_jacobian(a0))
    b, b0 = pr.build_pair(helpers.oracle_api(), robust)
    J, J0 = pr.dense_jacobian(b), pr.dense_jacobian(b0)
    assert J.shape == J0.shape and not np.array_equal(J, J0)


def test_entry_points_are_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "calico_hip.h")).read()
    entry.build_hip()
    lib = C.CDLL(_capi.hip_library_path())
    for name in ENTRY_POINTS:
        assert re.search(r"\bcalico_%s\(" % name, header), name
        assert name in _capi.ABI_SYMBOLS
        assert hasattr(lib, "calico_" + name)
    assert "typedef struct calico_prediction_options" in header


def test_default_options_and_host_side_argument_checks():
    entry.build_hip()
    lib = C.CDLL(_capi.hip_library_path())
    o = _capi.PredictionOptions()
    o.apply_loss = 7
    o.reserved[3] = 9
    lib.calico_default_prediction_options(C.byref(o))
    assert o.apply_loss == 1 and list(o.reserved) == [0] * 7
    assert C.sizeof(_capi.PredictionOptions) == 32
    lib.calico_prediction_covariance.restype = C.c_int32
    assert lib.calico_prediction_covariance(None, 0, None, None, None, None) == _capi.INVALID_ARGUMENT


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_prediction_kernel_scratch_budget():
    """ScratchSize / VGPRs Spill of prediction_items_kernel stay within what eval_items_kernel<true, 6> has, both read from
    one compile."""
    res = helpers.kernel_resources("eval_kernels.hip")
    base = [v for k, v in res.items() if "eval_items_kernelILb1ELi6E" in k]
    pred = {k: v for k, v in res.items() if "prediction_items_kernel" in k}
    assert len(base) == 1 and len(pred) == 2, sorted(res)
    for k, v in pred.items():
        print(k, v)
        assert v["ScratchSize"] <= base[0]["ScratchSize"], (k, v, base[0])
        assert v["VGPRs Spill"] <= base[0]["VGPRs Spill"], (k, v, base[0])
        assert v["Occupancy"] >= 1
