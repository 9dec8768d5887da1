"""The camera-IMU alignment kernels' resources as compiled (align_kernels.hip, from the compiler's own remarks).

No kernel may use scratch memory or spill: every per-lane array (the 38 sums of a sample's Gram matrix, the spline weights, the 4 x 4
Jacobi iteration) is indexed by compile-time constants only. (rodrigues<double>'s early return made the compiler keep two fields
of the returned struct in scratch here -- 24 bytes per lane -- which is why imu_align_dev.hpp has a branch-free align_rodrigues.)
As compiled, VGPRs and LDS bytes per workgroup:
  align_corr_kernel 110 / 832 (4 waves x 8 lags x 3 sums + 4 x 2)      align_corr_peak_kernel 32 / 33024 (the curve: 4096 doubles)
  align_horn_sums_kernel 74 / 1280 (4 waves x 40 doubles)              align_horn_kernel 114 / 320 (the Jacobi iterations live in registers)
  align_eval_kernel 88 / 1280                                          align_decide_kernel 52 / 784 (40 + 49 + 8 doubles + the flag)
  align_final_kernel 20 / 784                                          align_accel_kernel<false / true> 98 / 1280
  align_accel_solve_kernel 14 / 672
The per-sample kernels run 256 threads per workgroup; at most 128 VGPRs keeps four waves per SIMD. The LDS figures are the
kernels' static arrays, asserted exactly: a change there is a change of the reduction's layout."""
import os
import shutil
import sys

import pytest

import helpers

sys.path.insert(0, helpers.ROOT)
import __graft_entry__ as entry  # noqa: E402

LDS = {"align_corr_kernel": 832, "align_corr_peak_kernel": 33024, "align_horn_sums_kernel": 1280, "align_horn_kernel": 320,
       "align_eval_kernel": 1280, "align_decide_kernel": 784, "align_final_kernel": 784, "align_accel_kernel": 1280,
       "align_accel_solve_kernel": 672}


@pytest.mark.skipif(shutil.which(entry.HIPCC) is None and not os.path.exists(entry.HIPCC), reason="no hipcc")
def test_align_kernels_resource_budget():
    res = helpers.kernel_resources("align_kernels.hip")
    assert len(res) == 10, sorted(res)
    for name, v in res.items():
        print(name, v)
        # align_corr_kernel keeps the order's loop-invariant lane masks (i < k, j < k of the spline weights) live across its loop
        # over the lags: 4 SGPRs more than the 102 a wave has go to lanes of a VGPR (v_writelane), not to memory
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == (4 if "17align_corr_kernelE" in name else 0), (name, v)
        assert v["VGPRs"] <= 128 and v["AGPRs"] == 0 and v["Occupancy"] >= 4, (name, v)
        (kernel,) = [k for k in LDS if "%d%sE" % (len(k), k) in name or "%d%sI" % (len(k), k) in name]      # (plain or a template's)
        assert v["LDS Size"] == LDS[kernel], (name, v)
