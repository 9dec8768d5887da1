"""Timing of calico_imu_allan on the synthetic static log (profiles/EXPERIMENTS.md, "IMU noise characterisation"): the wall time of
the whole call (upload, five launches, one readback, the host's fit) as the median over repeated calls after a warm-up, the
bytes the variance kernel asks for (24 Sum_j (n - 2 m_j) per axis), and the numpy float64 restatement's wall time on the same host
as context. The kernels' own times come from running this script under `rocprofv3 --kernel-trace --stats`.

usage: python profiles/allan_timing.py [--n 262144] [--calls 20] [--warmup 3] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2 ** 18)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    import torch      # PyTorch's HIP runtime first, as in bench.py
    torch.zeros(1, device="cuda")
    import allan_ref as ar
    from calico_amd import _capi
    api = _capi.load_hip()
    rate = 200.0
    y = ar.synthetic_log(0, n=args.n, rate=rate)
    ms = ar.grid(args.n)
    for _ in range(args.warmup):
        out = _capi.imu_allan(api, y, None, rate)
    times = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        out = _capi.imu_allan(api, y, None, rate)
        times.append(time.perf_counter() - t0)
    terms = sum(args.n - 2 * m for m in ms)
    result = dict(n=args.n, cluster_sizes=len(ms), calls=args.calls, call_ms_median=1e3 * float(np.median(times)), call_ms_min=1e3 * min(times),
                  variance_bytes=3 * 24 * terms, N=[a["N"] for a in out["noise"]], K=[a["K"] for a in out["noise"]],
                  sigma_at_rate=out["summary"]["sigma_at_rate"])
    if not args.no_numpy:
        t0 = time.perf_counter()
        for c in range(3):
            ar.avar(y[:, c], rate, ms, dtype=np.float64)
        result["numpy_float64_ms"] = 1e3 * (time.perf_counter() - t0)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
