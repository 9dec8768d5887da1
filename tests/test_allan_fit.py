"""The coefficient fit of calico_imu_allan on its own (calico_amd/csrc/allan_fit.hpp): tests/cpp/allan_fit_check.cpp, a stand-alone host
program built with g++ alone under the address and undefined-behaviour sanitizers, checks that each single-term curve returns
its own coefficient and mask, that a curve of two terms returns both, that a curve which would need a negative coefficient
returns the feasible subset, and that variances that are all zero or all NaN give TOO_FEW_POINTS. No GPU, no library of the
project is loaded."""
import os
import subprocess

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "allan_fit_check.cpp")
EXE = os.path.join(helpers.ROOT, "tests", "cpp", "build", "allan_fit_check")


def test_the_fit_header_needs_no_hip():
    path = os.path.join(helpers.ROOT, "calico_amd", "csrc", "allan_fit.hpp")
    includes = [line.split()[1] for line in open(path) if line.startswith("#include")]
    assert all(i.startswith("<") and "hip" not in i for i in includes[:-1]) and includes[-1] == '"../../include/calico_hip.h"', includes


def test_the_fit_on_known_curves_under_sanitizers():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", EXE])
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().startswith("OK ") and int(out.stdout.split()[1]) >= 40, out.stdout
    assert out.stderr.strip() == "", out.stderr       # (a sanitizer report would be here)
