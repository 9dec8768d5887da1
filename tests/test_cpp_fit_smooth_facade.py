"""Trajectory::FitSplineSmooth (include/calico/calico.hpp) through tests/cpp/fit_smooth_facade.cpp, host only: with the solve replaced
by a recorder (BSpline6::smooth_fit_solver(), -DCALICO_TEST_HOOKS) the facade hands the knots and basis of FitSpline, the unwrapped
axis-angle data, the weights and the options through unchanged, and maps every return code to its Status."""
import os
import subprocess

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "fit_smooth_facade.cpp")
EXE = os.path.join(helpers.ROOT, "tests", "cpp", "build", "fit_smooth_facade")


def test_fit_smooth_facade_hands_everything_through():
    import __graft_entry__ as g
    g.build_hip()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(helpers.ROOT, "calico_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-DCALICO_TEST_HOOKS", "-I", os.path.join(helpers.ROOT, "include"),
                           SRC, "-o", EXE, "-L", libdir, "-lcalico_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
