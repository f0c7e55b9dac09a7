"""Closed-loop MPC cycle resident on the device (include/hsqp_loop.h) at BASELINE config 4 (whole-body G1, 256 instances x 100 nodes, walk gait):
the loop of tools/closed_loop_cycle.py — targets, hsqp_upload_reference's work with the device-built warm start, one SQP iteration with the
filter line search, the policy rollout over the period (1/60 s), the rolled-out state as the next measured state — with the targets
regenerated on the device in every cycle from the measured state and each instance's velocity command, and nothing but status words crossing
to the host between cycles.  Every cycle is one hsqp_loop_run(1) call, timed by the wall clock like the other tool's cycle; the last line also
reports one hsqp_loop_run(cycles) call per cycle (`run_ms_per_cycle`), which is how a caller would use it.
Prints one JSON line with the fields of tools/closed_loop_cycle.py (no rollout share and no step counts: the loop does not stop between the
iteration and the rollout, and its rollout keeps no step counters).
    python tools/device_loop_cycle.py [--cycles 30] [--warmup 3] [--batch 256] [--nodes 100] [--controller feedforward|feedback]
                                      [--commands same|spread] [--gait ladder|walk] [--isolate park|reset]
--gait: the loop is started through hsqp_loop_start_gait (include/hsqp_gait.h): every instance starts in stance with the resident gait schedule
and ladder instead of an uploaded walk schedule.  ladder: the scenario of tests/test_gpu_gait.py across the batch (instance b mod 4: zero
command; 0.2 m/s from cycle 10; 0.2 m/s from cycle 10 and zero again from cycle 40; a yaw rate of 0.3 rad/s from cycle 10), and the line
reports the rungs at the end; walk: --commands from the start (feet lift about one second in: choose --warmup 120 to time walking cycles).
--isolate: hsqp_loop_isolate (include/hsqp_episode.h) behind the start, with the bounds off: every cycle also runs the triage (and, with --gait, the
per-instance gait reset); the line reports the episode counters at the end.
--commands same: every instance is commanded (0.3, 0, 0.7925, 0), the other tool's command; spread: vx from 0 to 0.6 m/s and yaw rates from
-0.2 to 0.2 rad/s across the batch.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wb_humanoid_mpc_amd import load_model  # noqa: E402
from wb_humanoid_mpc_amd.reference import gait_settings, pack_reference, tile_gait, velocity_command_targets  # noqa: E402
from wb_humanoid_mpc_amd.solver import HipSqpSolver  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--period", type=float, default=1.0 / 60.0)
    ap.add_argument("--controller", default="feedforward", choices=("feedforward", "feedback"))
    ap.add_argument("--commands", default="same", choices=("same", "spread"))
    ap.add_argument("--filter-alpha", type=float, default=0.8)
    ap.add_argument("--gait", default=None, choices=("ladder", "walk"))
    ap.add_argument("--isolate", default=None, choices=("park", "reset"))
    args = ap.parse_args()
    m = load_model()
    B, N, dt = args.batch, args.nodes, m.sqp["dt"]
    t_final = (2 * args.warmup + 2 * args.cycles) * args.period + N * dt + 1.0
    schedules = [tile_gait(m.gaits["walk"], 0.3 + 0.5 * b / B, t_final) for b in range(B)]
    knots = velocity_command_targets(m, (0.3, 0.0, 0.7925, 0.0), 0.0, m.initial_state, t_final)
    n_events, event_times, mode_sequence = pack_reference(schedules, [knots] * B)[:3]
    rng = np.random.default_rng(20250808)
    x_init = np.tile(m.initial_state, (B, 1))
    x_init[:, 6:6 + m.nj] += 0.01 * rng.standard_normal((B, m.nj))
    cmd = np.tile((0.3, 0.0, 0.7925, 0.0), (B, 1))
    if args.commands == "spread":
        cmd[:, 0] = np.linspace(0.0, 0.6, B)
        cmd[:, 3] = np.linspace(-0.2, 0.2, B)
    s = HipSqpSolver(m, max_nodes=N, max_batch=B, linesearch=True)
    s.set_scan_backoff_persistent(True)
    st = s.loop_settings(N, dt, period=args.period, filter_alpha=args.filter_alpha, iterations=1, take_step=True, linesearch=True,
                         controller=args.controller)
    cycle_ms, heights = [], []
    changes = {}
    if args.gait == "ladder":
        zero = np.tile((0.0, 0.0, 0.7925, 0.0), (B, 1))
        go, k = zero.copy(), np.arange(B) % 4
        go[(k == 1) | (k == 2), 0] = 0.2
        go[k == 3, 3] = 0.3
        stop = go.copy()
        stop[k == 2, 0] = 0.0
        cmd, changes = zero, {10: go, 40: stop}
    try:
        if args.gait:
            s.loop_start(st, 0.0, x_init, cmd, gait=gait_settings(m))
        else:
            s.loop_start(st, 0.0, x_init, cmd, n_events, event_times, mode_sequence)
        if args.isolate:
            s.loop_isolate(s.episode_settings(args.isolate))
        for c in range(args.warmup + args.cycles):
            if c in changes:
                s.loop_command(changes[c])
            t_a = time.perf_counter()
            r = s.loop_run(1)
            t_b = time.perf_counter()
            heights.append(r["x"][0, :, 2].copy())
            if c >= args.warmup:
                cycle_ms.append(1e3 * (t_b - t_a))
        t_a = time.perf_counter()
        r = s.loop_run(args.cycles, log=False)
        run_ms = 1e3 * (time.perf_counter() - t_a) / args.cycles
        t_end, x_end, v_filt = s.loop_state()
        rungs = np.bincount(s.gait_state()["rung"], minlength=7).tolist() if args.gait else None
        ep = s.loop_episodes() if args.isolate else None
        heights.append(x_end[:, 2].copy())
    finally:
        s.close()
    heights = np.concatenate(heights)
    q = np.percentile(cycle_ms, [25, 75])
    print(json.dumps({"metric": "device_loop_cycle", "batch": B, "nodes": N, "dt": dt, "period": args.period, "cycles": args.cycles,
                      "controller": args.controller, "commands": args.commands, "filter_alpha": args.filter_alpha, "gait": args.gait, "instances_per_rung": rungs, "isolate": args.isolate,
                      "episodes": {"failed_now": int((ep["state"] != 0).sum()), "failures": int(ep["n_failures"].sum()), "episodes": int(ep["n_episodes"].sum())} if ep else None,
                      "cycle_ms_median": round(float(np.median(cycle_ms)), 3), "cycle_ms_mean": round(float(np.mean(cycle_ms)), 3),
                      "cycle_ms_quartiles": [round(float(q[0]), 3), round(float(q[1]), 3)], "cycle_ms_min": round(float(np.min(cycle_ms)), 3),
                      "run_ms_per_cycle": round(float(run_ms), 3), "t_end": round(float(t_end), 6),
                      "status_counts": {"ok": int(B * (args.warmup + 2 * args.cycles)), "max_steps": 0, "nonfinite": 0},
                      "forward_speed_range": [round(float(x_end[:, 6 + m.nj].min()), 4), round(float(x_end[:, 6 + m.nj].max()), 4)],
                      "base_height_range": [round(float(heights.min()), 5), round(float(heights.max()), 5)]}))


if __name__ == "__main__":
    main()
