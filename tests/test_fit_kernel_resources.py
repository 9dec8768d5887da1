"""The spline-fit kernels' resources as compiled for gfx950 (fit_kernels.hip, from the compiler's own remarks): no kernel uses scratch
memory or spills -- the penalty's loops over powers and the solve's per-lane sums index no per-lane array -- the solves' LDS is all
dynamic ([band | rhs], sized by the launch), and the one-wave solves keep __launch_bounds__(64)."""
import os
import re
import shutil
import sys

import pytest

import helpers

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

KERNELS = ("fit_weights_kernel", "fit_normal_kernel", "fit_solve_kernel", "fit_penalty_kernel", "fit_normal_weighted_kernel",
           "fit_solve_smooth_kernel")


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_fit_kernels_use_no_scratch():
    res = helpers.kernel_resources("fit_kernels.hip")
    assert len(res) == 7, sorted(res)      # (fit_normal_weighted_kernel with and without weights)
    for name, v in res.items():
        print(name, v)
        (kernel,) = [k for k in KERNELS if "%d%sE" % (len(k), k) in name or "%d%sI" % (len(k), k) in name]
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["AGPRs"] == 0, (name, v)
        assert v["LDS Size"] == 0, (name, v)
        # one wave per workgroup and one workgroup per CU at the LDS the long trajectories take: 128 VGPRs cost nothing
        assert v["VGPRs"] <= 128, (name, v)


def test_solve_kernels_keep_their_launch_bounds():
    src = open(os.path.join(entry.CSRC, "fit_kernels.hip")).read()
    for kernel in ("fit_solve_kernel", "fit_solve_smooth_kernel"):
        assert re.search(r"__global__\s+__launch_bounds__\(64\)\s+void\s+%s\(" % kernel, src), kernel
    assert "raise_lds_limit(device, fit_solve_smooth_kernel" in src
