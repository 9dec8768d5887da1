"""The Allan variance kernels' resources as compiled for gfx950 (allan_kernels.hip, from the compiler's own remarks): no kernel uses
scratch memory, spills or AGPRs, the streaming kernels keep workgroups of 256 and stay far below the register count that would
cost occupancy, every kernel keeps its launch bounds, and the source holds no atomic: the sums are ordered."""
import os
import re
import shutil
import sys

import pytest

import helpers

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

KERNELS = {"allan_block_sum_kernel": 256, "allan_offsets_kernel": 256, "allan_theta_kernel": 256, "allan_variance_kernel": 256,
           "allan_finish_kernel": 64}


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_allan_kernels_use_no_scratch():
    res = helpers.kernel_resources("allan_kernels.hip")
    assert len(res) == len(KERNELS), sorted(res)
    for name, v in res.items():
        print(name, v)
        (kernel,) = [k for k in KERNELS if "%d%sE" % (len(k), k) in name]
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["AGPRs"] == 0, (name, v)
        assert v["VGPRs"] <= 128, (name, v)      # eight waves per SIMD and more
        assert v["LDS Size"] <= 4 * 3 * 8, (name, v)      # at most the four waves' sums of three axes


def test_the_unit_is_built_and_keeps_its_launch_bounds():
    assert "allan_kernels.hip" in entry.HIP_SOURCES and "allan.cpp" in entry.HIP_SOURCES
    src = open(os.path.join(entry.CSRC, "allan_kernels.hip")).read()
    assert sorted(re.findall(r"__global__[^\n]*?void\s+(\w+)\(", src)) == sorted(KERNELS)
    for kernel, bound in KERNELS.items():
        assert re.search(r"__global__\s+__launch_bounds__\(%d\)\s+void\s+%s\(" % (bound, kernel), src), kernel
    code = re.sub(r"//.*", "", src)
    assert "atomic" not in code.lower()
    assert "fit_wave_sum(" in code and '#include "fit_dev.hpp"' in src      # the wave sum is the spline fits'
    assert "hipFuncSetAttribute" not in src and 'extern "C"' not in src
