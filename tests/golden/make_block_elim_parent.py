#!/usr/bin/env python
"""Record what the block elimination made of the cases of tests/test_gpu_block_elim_panel.py BEFORE its panel products moved to the
4x4x4 form of the FP64 MFMA: the errors of L, Z and L⁻ᵀ against the long-double reference, per case. Needs a GPU and a library
that has the hook (calico_debug_block_elim) over the header of that commit -- calico_amd/csrc/block_elim.hpp as of the commit
before, with CAL_PANEL defined as register 0 of the 16x16x4 product -- named by CALICO_HIP_LIB (with CALICO_DEV=1):

    CALICO_DEV=1 CALICO_HIP_LIB=<that library> python tests/golden/make_block_elim_parent.py [out.json]

The file holds recorded results only; the test reads it as the yardstick for the form in the tree."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import helpers  # noqa: E402
import test_gpu_block_elim_panel as t  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else t.GOLDEN
    hip = helpers.hip_api()
    doc = {"form": "v_mfma_f64_16x16x4_f64 panel products, result register 0 (the commit before the 4x4x4 form)",
           "measure": "max |got - ref| / max |ref| against Cholesky, L^-T and X L^-T in numpy.longdouble",
           "condition": {name: t.block(name)[1] for name in t.MATRICES}, "errors": {}}
    for name in t.MATRICES:
        for n in t.ROW_TILES:
            doc["errors"][t.case_key(name, n)] = t.block_errors(hip, name, n)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
