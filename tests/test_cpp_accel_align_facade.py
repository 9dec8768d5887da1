"""Trajectory::AlignAccelerometer (include/calico/calico.hpp) through tests/cpp/accel_align_facade.cpp: what needs no GPU here (the
library's argument errors reach the caller with their message); on the GPU, an accelerometer mounted at 40 degrees with a lever
arm recovered from the facade's own Project(), and the facade's bits against a direct call of calico_accel_align.

Project() takes the spline segment of the true time, so its data lie outside the model the alignment shares with the optimiser
(the stamp's segment). The host half here measures what the numpy reference reaches on the same data -- the program's poses
fitted and projected in numpy (synthetic.fit_trajectory, synthetic.project_accelerometer) --: REF_PROJECT. The program holds the
device to ten times that."""
import os
import subprocess

import numpy as np
import pytest

import accel_align_ref as ar
import helpers
from calico_amd import synthetic as syn

SRC = os.path.join(helpers.ROOT, "tests", "cpp", "accel_align_facade.cpp")
EXE = os.path.join(helpers.ROOT, "tests", "cpp", "build", "accel_align_facade")
REF_PROJECT = 2.8e-9      # 2026-10-20: the largest difference (rad, m, m/s^2, s) of the reference's result to the truth; data rms 2.3e-9 m/s^2


def _build():
    import __graft_entry__ as g
    g.build_hip()
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    libdir = os.path.join(helpers.ROOT, "calico_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(helpers.ROOT, "include"),
                           SRC, "-o", EXE, "-L", libdir, "-lcalico_hip", "-Wl,-rpath," + libdir])


def test_accel_align_facade_compiles_and_reports_argument_errors():
    _build()
    out = subprocess.run([EXE, "--host-only"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")


def test_the_reference_on_the_programs_data():
    """The program's trajectory and samples in numpy; the bound the program uses is ten times what is measured here."""
    t = 0.05 * np.arange(141)
    phi = np.stack([0.4 * np.sin(1.3 * t), 0.3 * np.sin(0.9 * t + 1.0), 0.5 * np.sin(1.7 * t + 2.0)], 1)
    trans = np.stack([0.3 * np.sin(0.7 * t), 0.2 * np.cos(0.5 * t), 1.0 + 0.1 * np.sin(1.1 * t)], 1)
    knots, basis, ctrl = syn.fit_trajectory(t, syn.quat_from_axis_angle(phi), trans, 10.0, 6)
    spl = (knots, basis, ctrl, 6)
    truth = dict(ar.ir.TRUTH, t_rig_accel=np.array(ar.LEVER))
    meas, stamps = syn.project_accelerometer(spl, 2, np.concatenate([[1.0], truth["accel_bias"]]), truth["q"], truth["t_rig_accel"],
                                             truth["latency"], truth["gravity"], 0.3 + 0.01 * np.arange(640))
    q0, l0 = ar.imu_start(truth, np.deg2rad(1.0), 1e-3)
    r = ar.align(spl, stamps, meas, q0, l0)
    dist = ar.distance_to_truth(ar.estimate(r), truth)
    print("reference on Project()'s data: distance to the truth", dist, "rms", r["rms"], "iterations", r["iterations"])
    assert r["status"] == ar.OK and r["samples"] == 640
    assert 0.5 * REF_PROJECT <= dist <= 2 * REF_PROJECT
    src = open(SRC).read()
    assert "const double bound = 10.0 * 2.8e-9;" in src and REF_PROJECT == 2.8e-9


@pytest.mark.gpu
def test_accel_align_facade_matches_the_c_abi():
    _build()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("OK")
