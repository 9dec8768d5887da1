"""The registry of dynamic-LDS limits (raise_lds_limit, plan.cpp): a kernel's limit is raised when a handle needs more than its
device allows, and only then.

The limits belong to the process and the device, and the pytest process has raised most of them by the time this test runs,
so the sequence runs in a fresh child: the smallest tree-solver case of test_gpu_linear_step.py, a wide one (428 calibration
columns: wider evaluation rows, a wider back-substitution), then both again with the first two handles still alive.
calico_debug_lds_attribute_calls counts the hipFuncSetAttribute calls in between; every step is held to that module's bounds.
"""
import os
import subprocess
import sys

import pytest

import helpers

pytestmark = pytest.mark.gpu

_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import helpers
from test_gpu_linear_step import check_steps, make_case_scene
hip = helpers.hip_api()
small, wide = make_case_scene(n_cp=12), make_case_scene(mc=428)
keep, counts = [], [int(hip.debug_lds_attribute_calls())]
for i, (scene, expect) in enumerate(((small, dict(tree_solver=1)), (wide, dict(tree_solver=1, m=428, reduced_route=2))) * 2):
    check_steps(hip, scene, expect, label="step %%d" %% (i + 1), keep=keep if i < 2 else None)
    counts.append(int(hip.debug_lds_attribute_calls()))
print("COUNTS", *counts)
"""


def test_limits_are_raised_when_needed_and_only_then():
    r = subprocess.run([sys.executable, "-c", _CHILD % (helpers.ROOT, os.path.join(helpers.ROOT, "tests"))], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    counts = [int(w) for line in r.stdout.splitlines() if line.startswith("COUNTS") for w in line.split()[1:]]
    print(r.stdout)
    assert len(counts) == 5 and counts[0] == 0, counts
    assert counts[1] > 0, counts              # a device seen for the first time
    assert counts[2] > counts[1], counts      # the wide handle needs more than the small one was given
    assert counts[3] == counts[2] and counts[4] == counts[2], counts      # nothing is raised twice, nothing lowered in between
