"""The accelerometer-alignment kernels' resources as compiled (accalign_kernels.hip, from the compiler's own remarks).

Three kernels, no scratch, no spills, no AGPRs (the file is built with the VGPR form of the FP64 MFMA, as eval_kernels.hip is:
the one accumulator tile of the evaluation lives in four VGPRs). LDS is static and asserted exactly: the evaluation stages 64
rows of 16 doubles per wave, 4 x 8 KB, and keeps 4 x 4 wave sums (32896 bytes); the one-wave kernels keep the 200 sums, the
13 x 13 system and its right-hand side of 16 (the decision 3080 bytes, the final kernel 3088 with its alignment padding).

VGPRs: the siblings' bar is four waves per SIMD (128). The one-wave kernels are under it (60 and 20 as compiled). The
evaluation is not: 176 as compiled. One lane carries a sample's whole forward-mode evaluation -- four derivative rows of spline
weights unrolled to order 8, the Rodrigues coefficients with their derivative along t (nine dual numbers), omega and alpha as
duals, and then the 42 entries of its three rows [J | r] live until the last of the three staging passes. Its figure is pinned
with a ceiling of 256 (two waves per SIMD); the kernel's time is the per-sample arithmetic, not latency that more waves
would hide."""
import os
import shutil

import pytest

import helpers

import sys
sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

LDS = {"accalign_eval_kernel": 4 * 64 * 16 * 8 + 4 * 4 * 8, "accalign_decide_kernel": 3080, "accalign_final_kernel": 3088}
VGPRS = {"accalign_eval_kernel": 256, "accalign_decide_kernel": 128, "accalign_final_kernel": 128}
EVAL_VGPRS_AS_COMPILED = 176


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_accalign_kernels_resource_budget():
    res = helpers.kernel_resources("accalign_kernels.hip")
    assert len(res) == 3, sorted(res)
    for part, lds in LDS.items():
        (v,) = [v for k, v in res.items() if part in k]
        print(part, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0 and v["AGPRs"] == 0, (part, v)
        assert v["LDS Size"] == lds, (part, v)
        assert v["VGPRs"] <= VGPRS[part], (part, v)
    (v,) = [v for k, v in res.items() if "accalign_eval_kernel" in k]
    assert v["VGPRs"] <= EVAL_VGPRS_AS_COMPILED + 8 and v["Occupancy"] >= 2, v
