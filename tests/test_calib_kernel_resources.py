"""The calibration kernels' resources as compiled (calib_kernels.hip, from the compiler's own remarks).

Budget: the per-frame evaluation kernel asks for two waves per SIMD (kCalibWavesPerSimd), that is at most 256 VGPRs, with no
scratch and no spills -- 171 per-lane partial sums in FP64 (342 VGPRs) would not fit, the Gram matrix on the matrix cores does.
As compiled: calib_evaluate_kernel<1..7> 191, 233, 223, 168, 226, 161, 168 VGPRs; LDS per workgroup of four waves
4 x 64 x (K + 7) x 8 bytes = 30720, 36864, 28672, 24576, 22528, 22528, 24576 (9216 per wave at most); calib_eliminate_kernel 73
VGPRs and 3456 bytes; calib_reduce_kernel 59 VGPRs and 11616 bytes; calib_decide_kernel 67 VGPRs, no LDS. ScratchSize 0 in all."""
import os
import shutil

import pytest

import helpers

import sys
sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

VGPR_BUDGET = 256      # two waves per SIMD
K = {1: 8, 2: 11, 3: 7, 4: 5, 5: 4, 6: 4, 7: 5}


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_calib_kernels_resource_budget():
    res = helpers.kernel_resources("calib_kernels.hip")
    assert len(res) == 10, sorted(res)
    for name, v in res.items():
        print(name, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    evaluate = {k: v for k, v in res.items() if "calib_evaluate_kernel" in k}
    assert len(evaluate) == 7
    for model in K:
        (v,) = [v for k, v in evaluate.items() if "ILi%dE" % model in k]
        assert v["VGPRs"] <= VGPR_BUDGET and v["AGPRs"] == 0 and v["Occupancy"] >= 2, (model, v)
        assert v["LDS Size"] == 4 * 64 * (K[model] + 7) * 8, (model, v)
    for part in ("calib_decide_kernel", "calib_eliminate_kernel", "calib_reduce_kernel"):
        (v,) = [v for k, v in res.items() if part in k]
        assert v["VGPRs"] <= 128 and v["LDS Size"] <= 16384, (part, v)
