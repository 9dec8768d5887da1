"""The robust fit's kernels' resources as compiled for gfx950 (fit_robust_kernels.hip, from the compiler's own remarks): no kernel uses
scratch memory, spills or AGPRs, all LDS is dynamic (the selection's 256 counts, the solve's [band | 3 rhs], both sized by the
launch), the one-wave kernels keep __launch_bounds__(64), and the solve's LDS limit goes through the registry."""
import os
import re
import shutil
import sys

import pytest

import helpers

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

KERNELS = ("fit_robust_begin_kernel", "fit_robust_residual_kernel", "fit_robust_select_kernel", "fit_robust_weight_kernel",
           "fit_robust_normal_kernel", "fit_robust_solve_kernel", "fit_robust_rss_kernel")


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_robust_fit_kernels_use_no_scratch():
    res = helpers.kernel_resources("fit_robust_kernels.hip")
    assert len(res) == len(KERNELS), sorted(res)
    for name, v in res.items():
        print(name, v)
        (kernel,) = [k for k in KERNELS if "%d%sE" % (len(k), k) in name]
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["AGPRs"] == 0, (name, v)
        assert v["LDS Size"] == 0, (name, v)
        assert v["VGPRs"] <= 128, (name, v)


def test_the_new_unit_is_built_and_keeps_its_launch_bounds():
    assert "fit_robust_kernels.hip" in entry.HIP_SOURCES
    src = open(os.path.join(entry.CSRC, "fit_robust_kernels.hip")).read()
    for kernel in ("fit_robust_solve_kernel", "fit_robust_rss_kernel"):
        assert re.search(r"__global__\s+__launch_bounds__\(64\)\s+void\s+%s\(" % kernel, src), kernel
    assert "raise_lds_limit(device, fit_robust_solve_kernel" in src
    # iteration 0 is the smoothing fit's own launch, and the solve and the normal-equation sum are the shared ones
    assert "launch_fit_spline_smooth(device, a, s)" in src and "fit_band_solve<3>(" in src and "fit_normal_weighted_entry<true>(" in src
