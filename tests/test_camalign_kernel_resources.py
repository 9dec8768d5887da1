"""The camera-alignment kernels' resources as compiled (camalign_kernels.hip, from the compiler's own remarks).

Budget: the per-frame evaluation kernel asks for two waves per SIMD (kCamAlignWavesPerSimd), that is at most 256 VGPRs, with no
scratch and no spills: the Gram matrix of the 8 columns [rotation 3 | translation 3 | latency | r] lives in ONE 16 x 16
accumulator tile of the FP64 matrix cores (4 registers). LDS is static everywhere (nothing to register with the LDS-limit
registry): the evaluation stages 64 rows of 8 columns per wave, 4 x 64 x 8 x 8 = 16384 bytes per workgroup; the pose sums keep
4 x 8 x 14 partial sums (3584 bytes); the peak kernel keeps the curve (4096 lags, 32768 bytes); the one-wave kernels the 42 sums,
the 7 x 7 system and its right-hand side. All under the 64 KiB a workgroup may have without asking.
As compiled: camalign_eval_kernel<1..7> 164, 166, 232, 164, 230, 164, 164 VGPRs, occupancy 3, 3, 2, 3, 2, 3, 3;
camalign_pose_kernel 142 VGPRs; camalign_peak_kernel 78; camalign_mean_kernel 108; camalign_decide_kernel 52;
camalign_final_kernel 28; camalign_gate_kernel 20, no LDS. ScratchSize 0 and no spills in all."""
import os
import shutil

import pytest

import helpers

import sys
sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

VGPR_BUDGET = 256      # two waves per SIMD
LDS_LIMIT = 64 * 1024
LDS = {"camalign_gate_kernel": 0, "camalign_pose_kernel": 4 * 8 * 14 * 8, "camalign_peak_kernel": 4096 * 8,
       "camalign_mean_kernel": 16 * 8, "camalign_decide_kernel": 800, "camalign_final_kernel": 784}      # (the one-wave kernels: their arrays, each 16-byte aligned)


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_camalign_kernels_resource_budget():
    res = helpers.kernel_resources("camalign_kernels.hip")
    assert len(res) == 7 + len(LDS), sorted(res)
    for name, v in res.items():
        print(name, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["LDS Size"] < LDS_LIMIT, (name, v)
    evaluate = {k: v for k, v in res.items() if "camalign_eval_kernel" in k}
    assert len(evaluate) == 7
    for model in range(1, 8):
        (v,) = [v for k, v in evaluate.items() if "ILi%dE" % model in k]
        assert v["VGPRs"] <= VGPR_BUDGET and v["AGPRs"] == 0 and v["Occupancy"] >= 2, (model, v)
        assert v["LDS Size"] == 4 * 64 * 8 * 8, (model, v)
    for part, lds in LDS.items():
        (v,) = [v for k, v in res.items() if part in k]
        assert v["VGPRs"] <= VGPR_BUDGET and v["LDS Size"] <= lds, (part, v)
