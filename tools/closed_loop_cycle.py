"""Closed-loop MPC cycle on the device at BASELINE config 4 (whole-body G1, 256 instances x 100 nodes, walk gait): every cycle
hsqp_upload_reference with HSQP_WARM_SHIFT from the rolled-out state (COLD on the first), one SQP iteration with the filter line search,
then hsqp_rollout_policy over the period (1/60 s) with the task.info rollout settings (ODE45, 1e-5 / 1e-3, 0.015 s, 10000 steps/s) — the
plant is the MPC's own flow map under its feed-forward policy, as in the reference's dummy-simulation loop.  The rolled-out state is the next
cycle's measured state.  Prints one JSON line: wall-clock ms per cycle and the rollout's share, accepted / rejected steps per instance
(min / median / max), the statuses, and the base-height range over the run.
    python tools/closed_loop_cycle.py [--cycles 30] [--warmup 3] [--batch 256] [--nodes 100] [--controller feedforward|feedback]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wb_humanoid_mpc_amd import load_model  # noqa: E402
from wb_humanoid_mpc_amd.reference import pack_reference, swing_config, tile_gait, velocity_command_targets  # noqa: E402
from wb_humanoid_mpc_amd.solver import HipSqpSolver  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--period", type=float, default=1.0 / 60.0)
    ap.add_argument("--controller", default="feedforward", choices=("feedforward", "feedback"))
    args = ap.parse_args()
    m = load_model()
    B, N, dt = args.batch, args.nodes, m.sqp["dt"]
    t_final = (args.warmup + args.cycles) * args.period + N * dt + 1.0
    schedules = [tile_gait(m.gaits["walk"], 0.3 + 0.5 * b / B, t_final) for b in range(B)]
    targets = velocity_command_targets(m, (0.3, 0.0, 0.7925, 0.0), 0.0, m.initial_state, t_final)
    ref = pack_reference(schedules, [targets] * B)
    rng = np.random.default_rng(20250808)
    x_init = np.tile(m.initial_state, (B, 1))
    x_init[:, 6:6 + m.nj] += 0.01 * rng.standard_normal((B, m.nj))
    sw = swing_config(m)
    s = HipSqpSolver(m, max_nodes=N, max_batch=B, linesearch=True)
    s.set_scan_backoff_persistent(True)
    t = 0.0
    cycle_ms, rollout_ms, steps, rejected, heights = [], [], [], [], []
    statuses = np.zeros(3, dtype=np.int64)
    try:
        for c in range(args.warmup + args.cycles):
            t_a = time.perf_counter()
            s.upload_reference_warm(x_init, N, dt, t, *ref, sw, mode="cold" if c == 0 else "shift")
            s.iterate(1, take_step=True, linesearch=True)
            t_r = time.perf_counter()
            r = s.rollout_policy(np.zeros(B), x_init, args.period, 1, controller=args.controller)
            t_b = time.perf_counter()
            x_init = r["x"][:, 0]
            heights.append(x_init[:, 2].copy())
            if c >= args.warmup:
                cycle_ms.append(1e3 * (t_b - t_a)); rollout_ms.append(1e3 * (t_b - t_r))
                steps.append(r["steps"].copy()); rejected.append(r["rejected"].copy())
                statuses += np.bincount(r["status"], minlength=3)[:3]
            t += args.period
    finally:
        s.close()
    steps, rejected, heights = np.concatenate(steps), np.concatenate(rejected), np.concatenate(heights)
    mmm = lambda v: {"min": int(np.min(v)), "median": float(np.median(v)), "max": int(np.max(v))}  # noqa: E731
    print(json.dumps({"metric": "closed_loop_cycle", "batch": B, "nodes": N, "dt": dt, "period": args.period, "cycles": args.cycles,
                      "controller": args.controller, "cycle_ms_median": round(float(np.median(cycle_ms)), 3),
                      "cycle_ms_mean": round(float(np.mean(cycle_ms)), 3), "rollout_ms_median": round(float(np.median(rollout_ms)), 3),
                      "rollout_share": round(float(np.median(rollout_ms) / np.median(cycle_ms)), 4),
                      "accepted_steps_per_instance": mmm(steps), "rejected_steps_per_instance": mmm(rejected),
                      "status_counts": {"ok": int(statuses[0]), "max_steps": int(statuses[1]), "nonfinite": int(statuses[2])},
                      "base_height_range": [round(float(heights.min()), 5), round(float(heights.max()), 5)]}))


if __name__ == "__main__":
    main()
