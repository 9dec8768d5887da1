#!/usr/bin/env python
"""Record what calico_imu_align, calico_camera_align and calico_accel_align made of the cases of tests/test_gpu_align_bits.py
BEFORE their kernels took the dense one-point LM loop from one header: every output array and summary field of every case, as raw
bytes, and the compiler that built the library. Needs a GPU and a library built from the parent commit, named by CALICO_HIP_LIB
(with CALICO_DEV=1):

    CALICO_DEV=1 CALICO_HIP_LIB=<that library> python tests/golden/make_align_parent_bits.py [out.npz]

The file holds recorded results only; the test reads it as the yardstick for the code in the tree. It is recorded again only by a
commit that changes the arithmetic of these calls on purpose, or for another toolchain (from the parent commit built with it)."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import __graft_entry__ as entry  # noqa: E402
import helpers  # noqa: E402
import test_gpu_align_bits as t  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    hip = helpers.hip_api()
    version = [line for line in subprocess.run([entry.HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines() if "version" in line]
    doc = {"hipcc_version": np.array("; ".join(version))}
    for name in sorted(t.CASES):
        for field, raw in t.run_case(hip, name).items():
            doc[name + "/" + field] = np.frombuffer(raw, dtype=np.uint8)
        print(name, "recorded")
    np.savez_compressed(out, **doc)
    print(len(doc) - 1, "fields of", len(t.CASES), "cases to", out)


if __name__ == "__main__":
    main()
