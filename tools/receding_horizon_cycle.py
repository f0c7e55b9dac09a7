"""Receding-horizon MPC cycle at BASELINE config 4 (whole-body G1, 256 instances x 100 nodes, dt = 0.035 s, one SQP iteration with the
filter line search per cycle, t0 advancing by 0.02 s — not a multiple of dt), through two paths measured in the same process, alternated:

  host    the adaptor's host warm start (reference.host_warm_start on the downloaded previous solution), hsqp_upload_reference with the
          trajectories (HSQP_WARM_CALLER), iterate, hsqp_download — what every batch caller had to do before hsqp_reference::warm_start;
  device  hsqp_upload_reference with HSQP_WARM_SHIFT (the warm start built on the device from the resident solution), iterate,
          hsqp_evaluate_policy (the feed-forward sample the controller needs; the trajectories stay in HBM).

Both loops see the same measured state every cycle (the device path's policy sample), so they compute the same numbers: at the end the
device path's resident solution is downloaded once (outside the timed region) and compared with the host path's, bit for bit.  Prints one
JSON line: wall-clock ms per cycle of each path (median, mean), the host path's numpy share, and the bytes crossing PCIe per cycle
computed from the array shapes.
    python tools/receding_horizon_cycle.py [--cycles 30] [--warmup 3] [--batch 256] [--nodes 100]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wb_humanoid_mpc_amd import _abi, load_model  # noqa: E402
from wb_humanoid_mpc_amd.reference import (LF, RF, STANCE, host_warm_start, pack_reference, swing_config, tile_gait,  # noqa: E402
                                           velocity_command_targets)
from wb_humanoid_mpc_amd.solver import HipSqpSolver  # noqa: E402


def host_cycle(host, mass, x_init, stamps, events, modes, prev, dt, t, ref, sw, N):
    """The host path of one cycle: the adaptor's warm start in numpy, trajectories up, one iteration, the solution down."""
    mode = np.stack([md[np.searchsorted(ev, stamps[:N], side="left")] for ev, md in zip(events, modes)])   # ModeSchedule::modeAtTime
    flags = np.stack([(mode == LF) | (mode == STANCE), (mode == RF) | (mode == STANCE)], axis=-1).astype(float)
    x, u = host_warm_start(mass, x_init, stamps, flags, prev)
    t_w = time.perf_counter()
    host.upload_reference(x_init, x, u, dt, t, *ref, sw)
    host.iterate(1, take_step=True, linesearch=True)
    out = host.download()
    out["t_w"] = t_w
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--period", type=float, default=0.02)
    ap.add_argument("--device-only", action="store_true", help="time the device path alone (no alternation, no bit-for-bit check)")
    args = ap.parse_args()
    m = load_model()
    B, N, dt = args.batch, args.nodes, m.sqp["dt"]
    t_final = (args.warmup + args.cycles) * args.period + N * dt + 1.0
    schedules = [tile_gait(m.gaits["walk"], 0.3 + 0.5 * b / B, t_final) for b in range(B)]
    targets = velocity_command_targets(m, (0.3, 0.0, 0.7925, 0.0), 0.0, m.initial_state, t_final)
    ref = pack_reference(schedules, [targets] * B)
    events = [np.asarray(sc.event_times) for sc in schedules]
    modes = [np.asarray(sc.mode_sequence) for sc in schedules]
    rng = np.random.default_rng(20250808)
    x_init = np.tile(m.initial_state, (B, 1))
    x_init[:, 6:6 + m.nj] += 0.01 * rng.standard_normal((B, m.nj))
    mass = 0.0
    for body in m.desc.bodies:   # DevModel::total_mass
        mass += body.mass
    sw = swing_config(m)
    host, dev = (HipSqpSolver(m, max_nodes=N, max_batch=B, linesearch=True) for _ in range(2))
    for s in (host, dev):
        s.set_scan_backoff_persistent(True)   # (host/HipSqpSolver.h does the same for receding-horizon handles)
    prev, t = None, 0.0
    ms = {"host": [], "device": [], "host_warm_start": [], "device_parts": []}
    try:
        for c in range(args.warmup + args.cycles):
            stamps = t + np.arange(N + 1) * dt
            # ---- host path
            t_a = time.perf_counter()
            if args.device_only:
                t_w = t_b = t_a
            else:
                out = host_cycle(host, mass, x_init, stamps, events, modes, prev, dt, t, ref, sw, N)
                t_w, t_b = out.pop("t_w"), time.perf_counter()
                prev = dict(times=stamps, x=out["x"], u=out["u"])
            # ---- device path
            t_c = time.perf_counter()
            dev.upload_reference_warm(x_init, N, dt, t, *ref, sw, mode="cold" if c == 0 else "shift")
            t_u = time.perf_counter()
            dev.iterate(1, take_step=True, linesearch=True)
            t_i = time.perf_counter()
            xs, _, _ = dev.evaluate_policy(np.full(B, args.period))
            t_d = time.perf_counter()
            if c >= args.warmup:
                ms["host"].append(1e3 * (t_b - t_a)); ms["device"].append(1e3 * (t_d - t_c)); ms["host_warm_start"].append(1e3 * (t_w - t_a))
                ms["device_parts"].append([round(1e3 * (t_u - t_c), 3), round(1e3 * (t_i - t_u), 3), round(1e3 * (t_d - t_i), 3)])
            x_init = xs
            t += args.period
        d = dev.download()
        same = None if args.device_only else all(np.array_equal(d[k], out[k]) for k in ("x", "u", "alpha", "step_type")) and d["perf_after"] == out["perf_after"]
    finally:
        host.close(); dev.close()
    E, K = ref[1].shape[1], ref[3].shape[1]
    ref_bytes = B * (4 + E * 8 + (E + 1) * 4 + K * 8 + K * _abi.NX * 8)
    traj = B * ((N + 1) * _abi.NX + N * _abi.NU) * 8
    pcie = {"host_up": B * _abi.NX * 8 + traj + ref_bytes,
            "host_down": 2 * traj + B * (2 * 4 * 8 + 2 * 8 + 8 + 4 + 8 + 8 + 4),   # x u dx du, perf x2, kkt, alpha, step, armijo, grad_inf, status
            "device_up": B * _abi.NX * 8 + ref_bytes + B * 8,                      # x_init, compact reference, policy times
            "device_down": B * (_abi.NX + _abi.NU + _abi.NJ) * 8 + 2 * B * 4}      # policy sample, status read of the SHIFT check and of the upload
    stat = lambda v: {"median_ms": round(float(np.median(v)), 3), "mean_ms": round(float(np.mean(v)), 3), "p90_ms": round(float(np.percentile(v, 90)), 3),  # noqa: E731
                      "max_ms": round(float(np.max(v)), 3)}
    print(json.dumps({"metric": "receding_horizon_cycle", "batch": B, "nodes": N, "dt": dt, "period": args.period, "cycles": args.cycles,
                      "host": stat(ms["host"]), "host_numpy_warm_start": stat(ms["host_warm_start"]), "device": stat(ms["device"]),
                      "speedup_median": None if args.device_only else round(float(np.median(ms["host"]) / np.median(ms["device"])), 3),
                      "pcie_bytes_per_cycle": pcie, "paths_bit_identical": same if same is None else bool(same),
                      "host_ms_per_cycle": [round(v, 3) for v in ms["host"]], "device_ms_per_cycle": [round(v, 3) for v in ms["device"]],
                      "device_upload_iterate_policy_ms": ms["device_parts"]}))


if __name__ == "__main__":
    main()
