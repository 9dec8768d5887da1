"""The argument rules of the calls without a problem handle (calico_amd/csrc/arg_rules.hpp) and the device loops' step rule
(lm_rule.hpp) on their own: tests/cpp/arg_rules_check.cpp, a stand-alone host program built with the address and
undefined-behaviour sanitizers, checks the chart batch's rules on exact-size heap arrays (n_frames 0, 1 and 3, offsets that start
at 1 or decrease, empty frames, null pixels with and without pairs, every option field at its bad values), the spline's shape and
segment rule, the stamps' rule (n = 0 and 1, equal neighbours, a decrease at the last sample, a NaN), the canonical quaternion, and
lm_rule over the full grid of its arguments. No GPU, no library of the project is loaded."""
import os
import subprocess

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "arg_rules_check.cpp")
EXE = os.path.join(helpers.ROOT, "tests", "cpp", "build", "arg_rules_check")


def test_rules_headers_need_no_hip():
    """arg_rules.hpp includes the standard library and the C header, nothing else; lm_rule.hpp only device_math.hpp."""
    csrc = os.path.join(helpers.ROOT, "calico_amd", "csrc")
    includes = [line.split()[1] for line in open(os.path.join(csrc, "arg_rules.hpp")) if line.startswith("#include")]
    assert all(i.startswith("<") and "hip" not in i for i in includes[:-1]) and includes[-1] == '"../../include/calico_hip.h"', includes
    includes = [line.split()[1] for line in open(os.path.join(csrc, "lm_rule.hpp")) if line.startswith("#include")]
    assert includes == ['"device_math.hpp"'], includes


def test_argument_rules_and_lm_rule_under_sanitizers():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", EXE])
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().startswith("OK ") and int(out.stdout.split()[1]) > 1000, out.stdout
    assert out.stderr.strip() == "", out.stderr       # (a sanitizer report would be here)
