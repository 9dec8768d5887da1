"""cal::shard_windows (calico_amd/csrc/shard.hpp) on its own: tests/cpp/shard_windows_check.cpp, a stand-alone host program
built with the address and undefined-behaviour sanitizers, checks the partition rule's properties -- boundaries from 0 to
nseg, every block owned once, each cut the first boundary that reaches its share, prefixes within one segment of their
share, where windows come out empty -- on random and hand-picked block counts (zeros, one dominant segment, a total of
zero, no segments, worlds up to 2 nseg + 1). No GPU, no library of the project is loaded."""
import os
import subprocess

import helpers

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "shard_windows_check.cpp")
EXE = os.path.join(helpers.ROOT, "tests", "cpp", "build", "shard_windows_check")


def test_shard_windows_properties_under_sanitizers():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", SRC, "-o", EXE])
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().startswith("OK ") and int(out.stdout.split()[1]) > 50000, out.stdout
    assert out.stderr.strip() == "", out.stderr       # (a sanitizer report would be here)
