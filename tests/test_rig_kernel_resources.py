"""The rig-calibration kernels' resources as compiled (rig_kernels.hip, from the compiler's own remarks).

Budget: the per-view evaluation kernel asks for two waves per SIMD (kRigWavesPerSimd), that is at most 256 VGPRs, with no scratch
and no spills: the Gram matrix of the 13 columns [J_frame 6 | J_extrinsics 6 | e] lives in ONE 16 x 16 accumulator tile of the
FP64 matrix cores (4 registers), not in 91 per-lane partial sums. LDS is static everywhere (nothing to register with the LDS-limit
registry): the evaluation stages 64 rows of 13 columns per wave, 4 x 64 x 13 x 8 = 26624 bytes per workgroup; the elimination
keeps a 6 x 6 block and the 6 x 49 columns of Y per wave, 4 x ((36 + 294) x 8 + 64) = 10816 bytes; the reduction keeps the
48 x 48 system with its gradient, diagonal and sums (2408 doubles), the inverse factor (2304), the right-hand side (48) and the
4 x 256 partial sums: 46272 bytes, under the 64 KiB a workgroup may have without asking.
As compiled: rig_evaluate_kernel<1..7> 182, 182, 234, 182, 247, 182, 182 VGPRs, occupancy 2; rig_eliminate_kernel 65 VGPRs;
rig_reduce_kernel 56 VGPRs (1024 threads); rig_decide_kernel 58 VGPRs, no LDS. ScratchSize 0 in all."""
import os
import shutil

import pytest

import helpers

import sys
sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

VGPR_BUDGET = 256      # two waves per SIMD
LDS = {"rig_eliminate_kernel": 10816, "rig_reduce_kernel": 46272, "rig_decide_kernel": 0}


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_rig_kernels_resource_budget():
    res = helpers.kernel_resources("rig_kernels.hip")
    assert len(res) == 10, sorted(res)
    for name, v in res.items():
        print(name, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
    evaluate = {k: v for k, v in res.items() if "rig_evaluate_kernel" in k}
    assert len(evaluate) == 7
    for model in range(1, 8):
        (v,) = [v for k, v in evaluate.items() if "ILi%dE" % model in k]
        assert v["VGPRs"] <= VGPR_BUDGET and v["AGPRs"] == 0 and v["Occupancy"] >= 2, (model, v)
        assert v["LDS Size"] == 4 * 64 * 13 * 8, (model, v)
    for part, lds in LDS.items():
        (v,) = [v for k, v in res.items() if part in k]
        assert v["VGPRs"] <= 128 and v["LDS Size"] <= lds, (part, v)
