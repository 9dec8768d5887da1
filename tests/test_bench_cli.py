"""bench.py's launcher contract on a box without (enough) GPUs: `--gpus N` must never silently run on fewer devices;
on a GPU, `--steps` sets the timed iterations and `--dump-outputs` writes the same arrays run after run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers

BENCH = os.path.join(helpers.ROOT, "bench.py")


def _gpus():
    try:
        import torch
        return torch.cuda.device_count() if torch.cuda.is_available() else 0
    except Exception:
        return 0


@pytest.mark.skipif(_gpus() >= 2, reason="needs a box with fewer than two GPUs")
def test_gpus_2_without_two_devices_exits_nonzero():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0
    assert "only %d GPU(s) visible" % _gpus() in r.stderr
    assert r.stdout.strip() == ""           # no JSON line that could be mistaken for a measurement


def test_gpus_flag_must_match_the_launcher():
    env = dict(os.environ, WORLD_SIZE="4", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "does not match" in r.stderr and r.stdout.strip() == ""


@pytest.mark.skipif(_gpus() >= 1, reason="checks the no-GPU behaviour")
def test_single_gpu_run_without_a_gpu_fails_loudly():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode != 0 and "needs a GPU" in r.stderr and r.stdout.strip() == ""


@pytest.mark.gpu
def test_steps_and_dump_outputs(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dirs = [tmp_path / "a", tmp_path / "b"]
    for d in dirs:
        r = subprocess.run([sys.executable, BENCH, "--config", "0", "--steps", "7", "--warmup", "2", "--no-cpu-baseline",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads(r.stdout)
        assert line["steps"] == 7 and line["timed_steps_total"] == 7 and line["repeats"] == 1
        assert line["ms_per_step"] > 0
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert {"summary.npy", "iterations.npy", "control_points.npy", "sensor0_intrinsics.npy", "sensor0_residuals.npy"} <= set(names)
    assert sum(os.path.getsize(dirs[0] / n) for n in names) <= 64 << 20
    for n in names:
        a, b = np.load(dirs[0] / n), np.load(dirs[1] / n)
        assert a.dtype in (np.float32, np.float64), n
        assert np.array_equal(a, b), n
    summary = np.load(dirs[0] / "summary.npy")
    assert 0 < summary[1] <= 7 and summary[7] < summary[6]        # the last timed solve: iterations, final < initial cost
