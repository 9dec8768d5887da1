"""sensors::CameraModel::CalibrateFromChart and Camera::CalibrateIntrinsics (include/calico/calico.hpp) through
tests/cpp/calib_facade.cpp: the argument errors that need no GPU here; on the GPU, models 1 and 4 from the standard start, the
facade's bits against the C ABI, the camera's intrinsics set to the estimate, a constant kept bit for bit."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "calib_facade.cpp")
EXE = os.path.join(helpers.ROOT, "tests", "cpp", "build", "calib_facade")


def _build():
    import __graft_entry__ as g
    g.build_hip()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(helpers.ROOT, "calico_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(helpers.ROOT, "include"),
                           SRC, "-o", EXE, "-L", libdir, "-lcalico_hip", "-Wl,-rpath," + libdir])


def test_calib_facade_compiles_and_reports_argument_errors():
    _build()
    out = subprocess.run([EXE, "--host-only"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")


@pytest.mark.gpu
def test_calib_facade_matches_the_c_abi():
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
