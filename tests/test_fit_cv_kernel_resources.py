"""The cross-validated fit's kernels' resources as compiled for gfx950 (fit_cv_kernels.hip, from the compiler's own remarks): no kernel
uses scratch memory, spills or AGPRs, all LDS is dynamic (the solve's [band | 3 rhs], the score's eight partials, both sized by
the launch), the kernels keep their launch bounds, the solve's LDS limit goes through the registry, and the solve is the smoothing
fit's own body."""
import os
import re
import shutil
import sys

import pytest

import helpers

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

KERNELS = ("fit_cv_solve_kernel", "fit_cv_score_kernel", "fit_cv_choose_kernel", "fit_cv_sample_kernel")


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_cv_fit_kernels_use_no_scratch():
    res = helpers.kernel_resources("fit_cv_kernels.hip")
    assert len(res) == len(KERNELS), sorted(res)
    for name, v in res.items():
        print(name, v)
        (kernel,) = [k for k in KERNELS if "%d%sE" % (len(k), k) in name]
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["AGPRs"] == 0, (name, v)
        assert v["LDS Size"] == 0, (name, v)
        assert v["VGPRs"] <= 128, (name, v)


def test_the_new_unit_is_built_and_keeps_its_launch_bounds():
    assert "fit_cv_kernels.hip" in entry.HIP_SOURCES
    src = open(os.path.join(entry.CSRC, "fit_cv_kernels.hip")).read()
    for kernel, bound in (("fit_cv_solve_kernel", 64), ("fit_cv_choose_kernel", 64), ("fit_cv_score_kernel", 256), ("fit_cv_sample_kernel", 256)):
        assert re.search(r"__global__\s+__launch_bounds__\(%d\)\s+void\s+%s\(" % (bound, kernel), src), kernel
    assert "raise_lds_limit(device, fit_cv_solve_kernel" in src and "hipFuncSetAttribute" not in src
    # the solve is the smoothing fit's own body (fit_dev.hpp), which fit_solve_smooth_kernel calls too, and so are the launches before it
    assert "fit_smooth_solve_wave(a, g, l, lane, lds)" in src and "launch_fit_smooth_prepare(a, s)" in src
    smooth = open(os.path.join(entry.CSRC, "fit_kernels.hip")).read()
    assert "fit_smooth_solve_wave(a, blockIdx.x, blockIdx.y, threadIdx.x, lds)" in smooth and "launch_fit_smooth_prepare(a, s)" in smooth
    assert "atomic" not in re.sub(r"//.*", "", src)
