"""sensors::CharacterizeImuNoise and ImuSensor::ApplyNoise (include/calico/calico.hpp) through tests/cpp/allan_facade.cpp: what needs
no GPU here (the library's argument errors reach the caller as kInvalidArgument with their message -- a gap in the stamps among
them --, ApplyNoise's arithmetic and refusals); on the GPU, the facade's bits against a direct call of calico_imu_allan, the
white noise of the program's log against its truth, and the sigma left in the sensors."""
import os
import subprocess

import pytest

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "allan_facade.cpp")
EXE = os.path.join(helpers.ROOT, "tests", "cpp", "build", "allan_facade")


def _build():
    import __graft_entry__ as g
    g.build_hip()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(helpers.ROOT, "calico_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(helpers.ROOT, "include"),
                           SRC, "-o", EXE, "-L", libdir, "-lcalico_hip", "-Wl,-rpath," + libdir])


def test_allan_facade_compiles_and_reports_argument_errors():
    _build()
    out = subprocess.run([EXE, "--host-only"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")


@pytest.mark.gpu
def test_allan_facade_matches_the_c_abi():
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
