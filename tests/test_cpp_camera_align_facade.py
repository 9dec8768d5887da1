"""Trajectory::AlignCamera (include/calico/calico.hpp) through tests/cpp/camera_align_facade.cpp: what needs no GPU here (the
library's argument errors reach the caller with their message, a body the world model does not have); on the GPU, a camera mounted
at 12 degrees and 13.7 ms late recovered from the facade's own Project() within the distance of the two segment polynomials, too
few frames, and the facade's bits against a direct call of calico_camera_align."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "camera_align_facade.cpp")
EXE = os.path.join(helpers.ROOT, "tests", "cpp", "build", "camera_align_facade")


def _build():
    import __graft_entry__ as g
    g.build_hip()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(helpers.ROOT, "calico_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(helpers.ROOT, "include"),
                           SRC, "-o", EXE, "-L", libdir, "-lcalico_hip", "-Wl,-rpath," + libdir])


def test_camera_align_facade_compiles_and_reports_argument_errors():
    _build()
    out = subprocess.run([EXE, "--host-only"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")


@pytest.mark.gpu
def test_camera_align_facade_matches_the_c_abi():
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
