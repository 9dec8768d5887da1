"""Trajectory::FitSplineCV (include/calico/calico.hpp) through tests/cpp/fit_cv_facade.cpp. Host only: with the solve replaced by a
recorder (BSpline6::cv_fit_solver(), -DCALICO_TEST_HOOKS) the facade hands the knots and basis of FitSpline, the unwrapped
axis-angle data, the weights and both option structs through unchanged, returns both kinds of rows and the per-pose leverages and
leave-one-out residuals in time order, and maps every return code to its Status. On the GPU: the recorder forwards to
calico_fit_spline_cv and the facade returns that call's bits; noisy poses get an interior lambda under both criteria."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "fit_cv_facade.cpp")
EXE = os.path.join(helpers.ROOT, "tests", "cpp", "build", "fit_cv_facade")


def _build():
    import __graft_entry__ as g
    g.build_hip()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(helpers.ROOT, "calico_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-DCALICO_TEST_HOOKS", "-I", os.path.join(helpers.ROOT, "include"),
                           SRC, "-o", EXE, "-L", libdir, "-lcalico_hip", "-Wl,-rpath," + libdir])


def test_fit_cv_facade_hands_everything_through():
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")


@pytest.mark.gpu
def test_fit_cv_facade_returns_the_library_call_bit_for_bit():
    _build()
    out = subprocess.run([EXE, "device"], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
