"""Covariance entry points without a GPU: the C ABI declares and exports them, and the covariance kernel keeps no
scratch (no private arrays indexed at run time), from the compiler's own remarks."""
import ctypes as C
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import helpers  # noqa: E402
from calico_amd import _capi  # noqa: E402

NAMES = ["default_covariance_options", "covariance_compute", "covariance_info", "covariance_get_dense", "covariance_get_block"]


def test_covariance_entries_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "calico_hip.h")).read()
    for n in NAMES:
        assert re.search(r"\bcalico_%s\s*\(" % n, header), n
        assert n in _capi.ABI_SYMBOLS
    entry.build_hip()
    lib = C.CDLL(_capi.hip_library_path())
    for n in NAMES:
        getattr(lib, "calico_" + n)
    o = _capi.CovarianceOptions()
    lib.calico_default_covariance_options(C.byref(o))
    assert 0.0 < o.min_relative_pivot < 1e-6


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_covariance_kernel_scratch_free():
    res = helpers.kernel_resources("cov_kernels.hip")
    ks = {k: v for k, v in res.items() if "covariance_kernel" in k}
    assert len(ks) == 2, sorted(res)      # the in-LDS and the global-memory variant
    for k, v in ks.items():
        assert v["ScratchSize"] == 0, (k, v)
        assert v["VGPRs Spill"] == 0, (k, v)
