"""Device time of the Riccati feedback policy (include/hsqp_feedback.h) at B x N: k_feedback_gains for the whole policy (N + 1 entries) and for a
5-node window, into device buffers (hsqp_feedback_policy_device), wall clock per call (each call ends with a stream synchronisation, so this
includes the launch); and hsqp_evaluate_feedback_policy with its transfers.
For kernel-only numbers run it under `rocprofv3 --kernel-trace --stats -- python tools/feedback_timing.py`.
    python tools/feedback_timing.py [--batch 256] [--nodes 100] [--reps 50]"""
import argparse
import json
import os
import sys

import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wb_humanoid_mpc_amd import _abi, load_model  # noqa: E402
from wb_humanoid_mpc_amd.reference import make_problem  # noqa: E402
from wb_humanoid_mpc_amd.solver import HipSqpSolver  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from test_gpu_feedback_policy import DeviceBuffer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    B, N = a.batch, a.nodes
    model = load_model()
    x0, x, u, par, dt = make_problem(model, n_nodes=N, batch=B, perturb=True)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    s.upload(x0, x, u, par, dt)
    s.iterate(1, take_step=True)
    K, uff = DeviceBuffer((B, N + 1, _abi.NU, _abi.NX), 0.0), DeviceBuffer((B, N + 1, _abi.NU), 0.0)
    res = {}
    for name, (first, count) in (("full_policy", (0, N + 1)), ("window_5", (N // 2, 5))):
        for _ in range(5):
            s.feedback_policy_device(first, count, K.ptr.value, uff.ptr.value)
        t = time.perf_counter()
        for _ in range(a.reps):
            s.feedback_policy_device(first, count, K.ptr.value, uff.ptr.value)
        ms = 1e3 * (time.perf_counter() - t) / a.reps
        mb = B * count * (NBYTES_NODE) / 1e6
        res[name] = dict(entries=count, ms_per_call=round(ms, 4), approx_MB=round(mb, 1), GBps=round(mb / ms, 1))
    sv, xm = np.full(B, 0.5 * N * dt), x0.copy()
    s.evaluate_feedback_policy(sv, xm)
    t = time.perf_counter()
    for _ in range(a.reps):
        s.evaluate_feedback_policy(sv, xm)
    res["evaluate_feedback_policy_host_ms"] = round(1e3 * (time.perf_counter() - t) / a.reps, 4)
    print(json.dumps(dict(batch=B, nodes=N, **res)))
    K.free(); uff.free()
    s.close()


# per entry: Px (35 x 58), Pu (35 x 23), K~ (23 x 58), x, u read; K and uff written
NBYTES_NODE = 8 * (35 * 58 + 35 * 23 + 23 * 58 + 58 + 35 + 35 * 58 + 35)

if __name__ == "__main__":
    main()
