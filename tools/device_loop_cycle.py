"""Closed-loop MPC cycle resident on the device (include/hsqp_loop.h) at BASELINE config 4 (whole-body G1, 256 instances x 100 nodes, walk gait):
the loop of tools/closed_loop_cycle.py — targets, hsqp_upload_reference's work with the device-built warm start, one SQP iteration with the
filter line search, the policy rollout over the period (1/60 s), the rolled-out state as the next measured state — with the targets
regenerated on the device in every cycle from the measured state and each instance's velocity command, and nothing but status words crossing
to the host between cycles.  Every cycle is one hsqp_loop_run(1) call, timed by the wall clock like the other tool's cycle; the last line also
reports one hsqp_loop_run(cycles) call per cycle (`run_ms_per_cycle`), which is how a caller would use it.
Prints one JSON line with the fields of tools/closed_loop_cycle.py (no rollout share and no step counts: the loop does not stop between the
iteration and the rollout, and its rollout keeps no step counters).
    python tools/device_loop_cycle.py [--cycles 30] [--warmup 3] [--batch 256] [--nodes 100] [--controller feedforward|feedback]
                                      [--commands same|spread] [--gait ladder|walk] [--isolate park|reset] [--with-push NEWTONS]
                                      [--plant flow|torque] [--kp 100] [--kd 2] [--armature 0.01] [--lookahead 0.005]
                                      [--contact] [--stiffness 5e4] [--damping 10] [--mu MODEL] [--slip-velocity 0.01]
                                      [--actuator] [--command-period 0.002] [--effort-limits FILE] [--joint-damping 0] [--joint-friction 0]
                                      [--inertia] [--mass-spread 0.15] [--payload KG]
                                      [--terrain ramp|ledge|rubble] [--terrain-seed 2026]
                                      [--observe] [--obs-noise 0.005] [--obs-bias 0.02] [--sensor-delay 1] [--compute-delay 1] [--obs-seed 2026]
                                      [--metrics] [--perceive]
    python tools/device_loop_cycle.py --push [--batch 16] [--nodes 40] [--cycles 120] [--push-max 400] [--push-at 0.5] [--push-for 0.2]
                                      [--plant torque [--contact ...] [--actuator ...] [--inertia ...]]
--with-push: the timed run with one push per instance resident (include/hsqp_push.h): a constant lateral force at the pelvis over the whole run.
--plant: the plant of the loop's rollout (include/hsqp_plant.h).  torque: full forward dynamics under the joint PD law with the given gains
(defaults: the gains of the tests); flow: the MPC's own flow map, set explicitly.  With --plant the line also carries `rollout_probe`: after the
timed cycles one more hsqp_rollout_policy call over the period from the loop's last state on the resident policy, timed by the wall clock
(median of five), with its accepted / rejected step counts per instance — the rollout's share of a cycle and what the integrator spends.
--push: a small push-recovery sweep instead of the timing.  Every instance walks under the same command; instance b is pushed sideways at the
pelvis (the base link's origin) with b / (batch - 1) of --push-max newtons from --push-at seconds on for --push-for seconds.  Isolation is on
(park; box: base height above 0.45 m, tilt below 0.7 rad), and the sweep runs once with the feed-forward and once with the feedback controller.
It prints which instances the triage recorded as failed, with which cause and in which cycle.  It reports; it asserts nothing: without --plant the
plant's joints are ideal acceleration sources and its contacts do not slip, and nobody has measured at which magnitude the G1 falls in this model.
With --plant torque --contact the feet stand on the ground of include/hsqp_contact.h, the ground reaction is the contact model's, and the sweep
also prints each instance's peak total normal force and peak tangential / normal ratio, from contact_forces at the logged states.
--contact: the ground under the torque plant (include/hsqp_contact.h; requires --plant torque): penalty contact with Coulomb friction at the eight
sole corners, with the given stiffness [N/m per point], damping [s/m], friction coefficient (default: the model's) and slip velocity [m/s].
--actuator: the actuator model on the torque plant (include/hsqp_actuator.h; requires --plant torque): the joint command sampled every
--command-period seconds and held (0: the continuous controller), the actuator torque clamped to the limits of --effort-limits (a JSON object
joint name -> N m, mapped through the model's joint names, e.g. tests/golden/g1_effort_limits.json; default: no limits), viscous damping
[N m s/rad] and dry friction [N m] at every joint.  The line reports the setting and `saturated_share`: the share of the instances that end the
run with |tau_cmd| above the limit at any joint (hsqp_actuator_last; instances without a record are not counted).
--inertia: per-instance inertial variations of the torque PLANT (include/hsqp_inertia.h; requires --plant torque): instance b has every link's mass and
rotational inertia scaled by 1 + spread (2 b / (B - 1) - 1), spread = --mass-spread (0: no scaling), and with --payload KG carries a point mass of
KG kilograms at the origin of the torso link.  The MPC keeps the nominal model: this is the model mismatch.  The timing mode and the --push sweep
both honour it; either prints, per instance, the plant's total mass (plant_dynamics) and whether the instance finished the run.
--terrain: uneven ground under the torque plant (include/hsqp_terrain.h; requires --plant torque --contact): sixteen height maps of growing difficulty,
built here, instance b on map b mod 16 — ramp: a slope of 0 .. 7.5 degrees (0.5 degree steps) that begins 0.3 m ahead of the start; ledge: a step up of
0 .. 6 cm (4 mm steps) over one 1 cm cell, 0.3 m ahead; rubble: a 64 x 64 grid of 4 cm cells around the start with heights drawn from --terrain-seed,
amplitude 0 .. 3 cm (2 mm steps), the cells under the soles at the start levelled.  The MPC plans on flat ground: this is the mismatch.  Isolation is on (park; box: base
height above 0.45 m, tilt below 0.7 rad, as in --push) unless --isolate says otherwise, and the run prints, per instance, the cycles it survived and its
final base position; the line carries the count of survivors per map.  It reports; it asserts nothing.
--observe: the observation model of the loop (include/hsqp_observe.h): the MPC measures the plant with white noise of standard deviation --obs-noise
on every state entry (rad, m, rad/s, m/s), a bias of --obs-bias metres on the base height, --sensor-delay periods it does not know about and
--compute-delay periods it does.  The timed run has the model on; the same run is then repeated with the model off, and the line carries, side by
side, the tracking of the commanded planar velocity (`tracking_on`, `tracking_off`: the error |v_base - R(yaw) v_cmd| in m/s, mean over the instances
and the timed cycles, and over the instances at the end) and the cycle times of both runs.
It reports; it asserts nothing (profiles/observe_loop_ab.txt: with the feed-forward controller one period of compute delay is enough to lose the walk
on the flow plant, with --controller feedback the defaults walk).
--metrics: the episode metrics of include/hsqp_metrics.h are on for the whole run (warm-up, the single cycles and the one long call): one record per
instance accumulated on the device and read back once, at the end.  The run prints a table of the open record of every instance (and, where an episode was
closed, of the last closed one) and the line carries `metrics`: the summary over the batch (survivors, RMS tracking error, distance, cost of transport) and
the share of torque samples in saturation.  With --terrain the final base position, and with --actuator `saturated_share` (then: the share of the
instances with a saturated sample anywhere in their records), come from the records instead of from logs and the last actuator record.  Opt-in: without
the flag the tool's output is what it was.
--event-grid [EVENT_NODES]: hsqp_loop_event_grid (include/hsqp_grid.h) behind the start: every cycle builds the ocs2 event-node grid of every instance on
the device and solves on nodes + EVENT_NODES intervals (default 32; the handle is created with that many nodes).  The line carries `event_grid`: the
settings and the range of the instances' own interval counts in the last cycle.  --schedule walk | run: the gait of the uploaded schedules (run has
twice the events per second).  Opt-in: without the flags the tool's output is what it was.
--ground-adapt [on | off]: hsqp_loop_ground (include/hsqp_ground.h) behind the start: every cycle estimates the ground height under every instance from its
stance feet, the command's height entry means height above it and step 2 takes it as the instance's terrain height; --box-above-ground puts the
base-height box of the triage on the height above the estimate.  The line carries `ground`: the range of the estimates at the end, the instances alive
and the base height above the LOCAL ground at the end (the height map under the base with --terrain, the plane at 0 without), mean and range over
the instances alive.  off: the same report from a loop that does not follow the ground (the partner of an A/B pair).  Opt-in: without the flag the
tool's output is what it was.
--perceive: hsqp_loop_perceive (include/hsqp_perceive.h) behind the start; requires --terrain.  Every cycle reads, per instance and foot, the lift-off and
touch-down height of every phase of the schedule from the height map — under the foot where it stands, under the foothold the targets carry to the
touch-down time where it will land — and step 2 takes them in place of the one terrain height.  The line carries `perceive`: the range of the last
cycle's lift-off heights over the instances alive and the largest difference between a swing's touch-down and lift-off height (offset removed).
Opt-in: without the flag the tool's output is what it was.
--gait: the loop is started through hsqp_loop_start_gait (include/hsqp_gait.h): every instance starts in stance with the resident gait schedule
and ladder instead of an uploaded walk schedule.  ladder: the scenario of tests/test_gpu_gait.py across the batch (instance b mod 4: zero
command; 0.2 m/s from cycle 10; 0.2 m/s from cycle 10 and zero again from cycle 40; a yaw rate of 0.3 rad/s from cycle 10), and the line
reports the rungs at the end; walk: --commands from the start (feet lift about one second in: choose --warmup 120 to time walking cycles).
--isolate: hsqp_loop_isolate (include/hsqp_episode.h) behind the start, with the bounds off: every cycle also runs the triage (and, with --gait, the
per-instance gait reset); the line reports the episode counters at the end.
--commands same: every instance is commanded (0.3, 0, 0.7925, 0), the other tool's command; spread: vx from 0 to 0.6 m/s and yaw rates from
-0.2 to 0.2 rad/s across the batch; stand: (0, 0, 0.7925, 0), with --schedule stance a standing robot.
--formulation centroidal: the loop of include/hsqp_cent_loop.h on the centroidal model (BASELINE configs 1-2; dt from the model's sqp block, --period as
given).  The line carries the per-cycle time of the resident loop (`cycle_ms_*`: one hsqp_loop_run(1) per cycle; `run_ms_per_cycle`: one call for all) and,
from the same run, of the same cycles driven from the host through the public calls (`driven_ms_*`: hsqp_centroidal_command_targets,
hsqp_upload_reference with the device-built warm start, hsqp_iterate_device, hsqp_rollout_policy).  --isolate, --with-push and --push work; the plant,
contact, actuator, inertia, terrain, gait, event-grid, ground, perceive, observe and metrics options are whole-body only and refused up front.
A cycle the MPC does not survive (HSQP_ERR_NUMERIC) ends the driven or the resident part there; the line says where (`driven_stopped`, `resident_stopped`,
`run_stopped`) and the times are those of the cycles that ran.  profiles/cent_loop.txt: the walk at 0.3 m/s on the 2 s horizon does not survive.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from wb_humanoid_mpc_amd import load_model  # noqa: E402
from wb_humanoid_mpc_amd.reference import (centroidal_velocity_command_targets, gait_settings, pack_reference, pad_targets, swing_config, tile_gait,  # noqa: E402
                                           velocity_command_targets)
from wb_humanoid_mpc_amd.solver import HipSqpSolver  # noqa: E402


def padded_state(m):
    """The model's initial state as a [58] row (centroidal: 35 live entries, zero padding)."""
    x = np.zeros(58)
    x[:len(m.initial_state)] = m.initial_state
    return x


def dummy_knots(m, cent, t_final):
    """Knots for pack_reference (only the schedules are taken from its result)."""
    if cent:
        return pad_targets(centroidal_velocity_command_targets(m, (0.3, 0.0, 0.7925, 0.0), 0.0, m.initial_state, t_final))
    return velocity_command_targets(m, (0.3, 0.0, 0.7925, 0.0), 0.0, m.initial_state, t_final)


def push_sweep(args):
    cent = args.formulation == "centroidal"
    m = load_model(formulation="centroidal") if cent else load_model()
    pose = 6 if cent else 0                                    # where the base pose starts in a state row
    given = {a.split("=")[0] for a in sys.argv[1:]}
    B = args.batch if "--batch" in given else 16
    N = args.nodes if "--nodes" in given else 40
    cycles = args.cycles if "--cycles" in given else 120
    dt = m.sqp["dt"]
    t_final = cycles * args.period + N * dt + 1.0
    schedule = tile_gait(m.gaits["walk"], 0.3, t_final)
    knots = dummy_knots(m, cent, t_final)
    n_events, event_times, mode_sequence = pack_reference([schedule] * B, [knots] * B)[:3]
    x_init = np.tile(padded_state(m), (B, 1))
    cmd = np.tile((0.3, 0.0, 0.7925, 0.0), (B, 1))
    force = args.push_max * np.arange(B) / max(B - 1, 1)
    pushes = [[dict(body=0, t_start=args.push_at, duration=args.push_for, point=(0.0, 0.0, 0.0), force=(0.0, f, 0.0))] for f in force]
    causes = {0: "alive", 1: "numeric", 2: "rollout", 3: "bounds"}
    rows, ground = {}, {}
    s = HipSqpSolver(m, max_nodes=N, max_batch=B, linesearch=True)
    s.set_scan_backoff_persistent(True)
    try:
        s.set_pushes(pushes)
        if args.plant:
            s.set_plant(kind=args.plant, kp=args.kp, kd=args.kd, armature=args.armature, lookahead=args.lookahead)
        if args.contact:
            s.set_contact(**contact_args(args))
        if args.actuator:
            s.set_actuator(**actuator_args(args, m))
        if args.inertia:
            s.set_inertia_instances(*inertia_args(args, B))
            masses = s.plant_dynamics(x_init)[2]
        for controller in ("feedforward", "feedback"):
            st = s.loop_settings(N, dt, period=args.period, filter_alpha=args.filter_alpha, iterations=1, take_step=True, linesearch=True, controller=controller)
            s.loop_start(st, 0.0, x_init, cmd, n_events, event_times, mode_sequence)
            s.loop_isolate(s.episode_settings("park", min_base_height=0.45, max_tilt=0.7))
            r = s.loop_run(cycles)
            ep = s.loop_episodes()
            x = r["x"]                                         # [cycle][instance][58], NaN rows once parked
            sway = np.nanmax(np.abs(x[:, :, pose + 1] - x[:, :1, pose + 1]), axis=0)
            rows[controller] = (ep, sway)
            if args.contact:                                   # ground reaction at every logged state (parked rows: no force)
                fn_peak, ratio_peak = np.zeros(B), np.zeros(B)
                for xc in x:
                    live = np.isfinite(xc).all(axis=1)
                    f, _ = s.contact_forces(np.where(live[:, None], xc, x_init))
                    fn = f[:, :, :, 2].sum(axis=(1, 2))
                    ft = np.linalg.norm(f[:, :, :, :2].sum(axis=(1, 2)), axis=1)
                    fn_peak = np.maximum(fn_peak, np.where(live, fn, 0.0))
                    ratio_peak = np.maximum(ratio_peak, np.where(live & (fn > 0.0), ft / np.maximum(fn, 1e-300), 0.0))
                ground[controller] = (fn_peak, ratio_peak)
    finally:
        s.close()
    print(f"push sweep: {B} instances x {N} nodes, walk at 0.3 m/s, {cycles} cycles of {args.period:.4f} s; lateral push at the pelvis from "
          f"{args.push_at} s for {args.push_for} s (cycles {int(args.push_at / args.period)} .. {int((args.push_at + args.push_for) / args.period)})")
    if args.plant:
        print(f"plant {args.plant}: kp {args.kp} kd {args.kd} armature {args.armature} lookahead {args.lookahead}" + (f"; contact {contact_args(args)}" if args.contact else ""))
    extra = f" {'peak fn [N]':>12} {'peak ft/fn':>10}" if args.contact else ""
    print(f"{'instance':>8} {'force [N]':>10} | " + " | ".join(f"{c + ': state':>20} {'cycle':>6} {'sway [m]':>9}" + extra for c in rows))
    if args.inertia:
        for b in range(B):
            print(f"instance {b}: total mass {masses[b]:.3f} kg, finished " + ", ".join(f"{c}: {'no' if ep['n_failures'][b] else 'yes'}" for c, (ep, _) in rows.items()))
    for b in range(B):
        cells = []
        for c, (ep, sway) in rows.items():
            cells.append(f"{causes.get(int(ep['cause'][b]), '?'):>20} {int(ep['fail_cycle'][b]) if ep['n_failures'][b] else '-':>6} {sway[b]:9.4f}"
                         + (f" {ground[c][0][b]:12.1f} {ground[c][1][b]:10.3f}" if args.contact else ""))
        print(f"{b:8d} {force[b]:10.1f} | " + " | ".join(cells))
    print(json.dumps({"metric": "push_sweep", "batch": B, "nodes": N, "cycles": cycles, "forces": [round(float(f), 2) for f in force],
                      "plant": args.plant, "contact": contact_args(args) if args.contact else None,
                      "inertia": dict(mass_spread=args.mass_spread, payload=args.payload, total_mass=[round(float(v), 3) for v in masses]) if args.inertia else None,
                      **({"peak_normal_force": {c: [round(float(v), 1) for v in g[0]] for c, g in ground.items()},
                          "peak_tangential_ratio": {c: [round(float(v), 3) for v in g[1]] for c, g in ground.items()}} if args.contact else {}),
                      **{c: {"failed": [int(b) for b in np.nonzero(ep["n_failures"])[0]], "fail_cycle": [int(v) for v in ep["fail_cycle"]]} for c, (ep, _) in rows.items()}}))


def contact_args(args):
    """The keywords of HipSqpSolver.set_contact from the command line (mu None: the model's friction_mu)."""
    return dict(stiffness=args.stiffness, damping=args.damping, mu=args.mu, slip_velocity=args.slip_velocity)


def actuator_args(args, m):
    """The keywords of HipSqpSolver.set_actuator from the command line."""
    limits = None
    if args.effort_limits:
        with open(args.effort_limits) as f:
            table = json.load(f)
        limits = [float(table[n]) for n in m.joint_names]
    return dict(command_period=args.command_period, effort_limit=limits, damping=args.joint_damping, friction=args.joint_friction)


TORSO_LINK = 15   # the torso of the G1 tree (data/g1_wb.json)


def inertia_args(args, B):
    """(mass_scale [B], payloads) of HipSqpSolver.set_inertia_instances from the command line."""
    scale = 1.0 + args.mass_spread * (2.0 * np.arange(B) / max(B - 1, 1) - 1.0) if B > 1 else np.ones(1)
    payloads = [[dict(body=TORSO_LINK, mass=args.payload)] for _ in range(B)] if args.payload is not None else None
    return scale, payloads


TERRAIN_MAPS = 16


def terrain_args(args, x_init):
    """(maps, placements, labels) of --terrain: sixteen maps of growing difficulty (label: what grows), instance b on map b mod 16, placed relative to its start."""
    rng = np.random.default_rng(args.terrain_seed)
    maps, labels = [], []
    for k in range(TERRAIN_MAPS):
        if args.terrain == "ramp":
            deg = 0.5 * k
            rise = np.tan(np.radians(deg)) * 8.0
            maps.append((np.array([[0.0, rise], [0.0, rise]]), 8.0))
            labels.append(f"{deg:.1f} deg")
        elif args.terrain == "ledge":
            h = 0.004 * k
            maps.append((np.array([[0.0, 0.0, 0.0, h, h]] * 4), 0.01))
            labels.append(f"{100 * h:.1f} cm")
        else:
            amp = 0.002 * k
            H = amp * rng.uniform(-1.0, 1.0, (64, 64))
            H[27:37, 28:36] = 0.0                          # (level under the start, +-0.14 m ahead and +-0.18 m aside: the feet begin on the plane)
            maps.append((H, 0.04))
            labels.append(f"{100 * amp:.1f} cm")
    place = []
    for b, x in enumerate(x_init):
        k = b % TERRAIN_MAPS
        c, sn = np.cos(x[3]), np.sin(x[3])
        if args.terrain == "rubble":
            off = (-31.5 * 0.04, -31.5 * 0.04)             # the map's centre under the base
        else:
            off = (0.3 - (0.02 if args.terrain == "ledge" else 0.0), -0.015 if args.terrain == "ledge" else -4.0)
        place.append(dict(map=k, origin=(x[0] + c * off[0] - sn * off[1], x[1] + sn * off[0] + c * off[1]), yaw=float(x[3])))
    return maps, place, labels


def saturated_share(s, m, args):
    """The share of the instances whose last record has |tau_cmd| above the limit at any joint."""
    limits = actuator_args(args, m)["effort_limit"]
    cmd = s.actuator_torques()[0]
    live = np.isfinite(cmd).all(axis=1)
    if limits is None or not live.any():
        return 0.0
    return round(float((np.abs(cmd[live]) > np.asarray(limits)).any(axis=1).mean()), 4)


def rollout_probe(s, args, x_end):
    """One rollout over the period from the loop's last state on the resident policy: wall-clock ms (median of five calls) and step counts."""
    from wb_humanoid_mpc_amd.solver import HsqpError
    B = len(x_end)
    ms, r = [], None
    for _ in range(5):
        t_a = time.perf_counter()
        try:
            r = s.rollout_policy(np.zeros(B), x_end, args.period, 1, controller=args.controller)
        except HsqpError as e:
            r = e.result
        ms.append(1e3 * (time.perf_counter() - t_a))
    if r is None:
        return None
    return {"rollout_ms_median": round(float(np.median(ms)), 3), "steps_mean": round(float(r["steps"].mean()), 2), "steps_max": int(r["steps"].max()),
            "rejected_mean": round(float(r["rejected"].mean()), 2), "rejected_max": int(r["rejected"].max()), "status_ok": int((r["status"] == 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--period", type=float, default=1.0 / 60.0)
    ap.add_argument("--controller", default="feedforward", choices=("feedforward", "feedback"))
    ap.add_argument("--commands", default="same", choices=("same", "spread", "stand"))
    ap.add_argument("--filter-alpha", type=float, default=0.8)
    ap.add_argument("--gait", default=None, choices=("ladder", "walk"))
    ap.add_argument("--isolate", default=None, choices=("park", "reset"))
    ap.add_argument("--with-push", type=float, default=None)
    ap.add_argument("--push", action="store_true")
    ap.add_argument("--plant", default=None, choices=("flow", "torque"))
    ap.add_argument("--kp", type=float, default=100.0)
    ap.add_argument("--kd", type=float, default=2.0)
    ap.add_argument("--armature", type=float, default=0.01)
    ap.add_argument("--lookahead", type=float, default=0.005)
    ap.add_argument("--contact", action="store_true")
    ap.add_argument("--stiffness", type=float, default=5e4)
    ap.add_argument("--damping", type=float, default=10.0)
    ap.add_argument("--mu", type=float, default=None)
    ap.add_argument("--slip-velocity", type=float, default=0.01)
    ap.add_argument("--actuator", action="store_true")
    ap.add_argument("--command-period", type=float, default=0.002)
    ap.add_argument("--effort-limits", default=None, metavar="FILE")
    ap.add_argument("--joint-damping", type=float, default=0.0)
    ap.add_argument("--joint-friction", type=float, default=0.0)
    ap.add_argument("--inertia", action="store_true")
    ap.add_argument("--mass-spread", type=float, default=0.15)
    ap.add_argument("--payload", type=float, default=None, metavar="KG")
    ap.add_argument("--terrain", default=None, choices=("ramp", "ledge", "rubble"))
    ap.add_argument("--terrain-seed", type=int, default=2026)
    ap.add_argument("--observe", action="store_true")
    ap.add_argument("--obs-noise", type=float, default=5e-3)
    ap.add_argument("--obs-bias", type=float, default=0.02)
    ap.add_argument("--sensor-delay", type=int, default=1)
    ap.add_argument("--compute-delay", type=int, default=1)
    ap.add_argument("--obs-seed", type=int, default=2026)
    ap.add_argument("--metrics", action="store_true")
    ap.add_argument("--event-grid", type=int, nargs="?", const=32, default=None, metavar="EVENT_NODES")
    ap.add_argument("--schedule", default="walk", choices=("walk", "run", "stance"))
    ap.add_argument("--ground-adapt", nargs="?", const="on", default=None, choices=("on", "off"))
    ap.add_argument("--box-above-ground", action="store_true")
    ap.add_argument("--perceive", action="store_true")
    ap.add_argument("--formulation", default="wb", choices=("wb", "centroidal"))
    ap.add_argument("--push-max", type=float, default=400.0)
    ap.add_argument("--push-at", type=float, default=0.5)
    ap.add_argument("--push-for", type=float, default=0.2)
    args = ap.parse_args()
    if args.contact and args.plant != "torque":
        ap.error("--contact requires --plant torque (the ground acts on the torque plant only)")
    if args.actuator and args.plant != "torque":
        ap.error("--actuator requires --plant torque (the actuator model acts on the torque plant only)")
    given = {a.split("=")[0] for a in sys.argv[1:]}
    if not args.inertia and given & {"--mass-spread", "--payload"}:
        ap.error("--mass-spread and --payload belong to --inertia (without it nothing is varied)")
    if args.inertia and args.plant != "torque":
        ap.error("--inertia requires --plant torque (the inertial variations act on the torque plant only)")
    if args.terrain and not (args.plant == "torque" and args.contact):
        ap.error("--terrain requires --plant torque --contact (the terrain lies under the ground of the torque plant)")
    if not args.observe and given & {"--obs-noise", "--obs-bias", "--sensor-delay", "--compute-delay", "--obs-seed"}:
        ap.error("--obs-noise, --obs-bias, --sensor-delay, --compute-delay and --obs-seed belong to --observe (without it the MPC measures the plant exactly)")
    if args.perceive and not args.terrain:
        ap.error("--perceive requires --terrain (the swing heights are read from the resident height maps)")
    if args.box_above_ground and args.ground_adapt != "on":
        ap.error("--box-above-ground belongs to --ground-adapt (the box stands on the estimated ground)")
    if args.formulation == "centroidal":
        wb_only = [o for o, on in (("--plant", args.plant), ("--contact", args.contact), ("--actuator", args.actuator), ("--inertia", args.inertia), ("--terrain", args.terrain),
                                   ("--gait", args.gait), ("--event-grid", args.event_grid is not None), ("--ground-adapt", args.ground_adapt), ("--perceive", args.perceive),
                                   ("--observe", args.observe), ("--metrics", args.metrics)) if on]
        if wb_only:
            ap.error("--formulation centroidal: " + ", ".join(wb_only) + " act on whole-body handles only (include/hsqp_cent_loop.h lists what the centroidal loop has)")
    if args.push:
        return push_sweep(args)
    if args.formulation == "centroidal":
        print(json.dumps(centroidal_run(args)))
        return
    line = timed_run(args, args.observe)
    if args.observe:
        off = timed_run(args, False)
        line["observe"].update(tracking_off=off["tracking"], cycle_ms_median_off=off["cycle_ms_median"], run_ms_per_cycle_off=off["run_ms_per_cycle"],
                               base_height_range_off=off["base_height_range"])
        line["observe"]["tracking_on"] = line["tracking"]
    del line["tracking"]
    print(json.dumps(line))


def tracking_error(m, x, cmd):
    """|v_base - R(yaw) v_cmd| of the planar base velocity, per instance: x [B][58], cmd [B][4]"""
    c, sn = np.cos(x[:, 3]), np.sin(x[:, 3])
    want = np.column_stack([c * cmd[:, 0] - sn * cmd[:, 1], sn * cmd[:, 0] + c * cmd[:, 1]])
    return np.linalg.norm(x[:, 6 + m.nj:8 + m.nj] - want, axis=1)


def metrics_report(s, args, ep):
    """The records at the end of the run: the per-instance table on stdout, the summary for the JSON line, (current, previous)."""
    cur, prev = s.loop_metrics("current"), s.loop_metrics("previous")
    causes = {-1: "open", 0: "host", 1: "numeric", 2: "rollout", 3: "bounds"}
    print(f"episode metrics: {len(cur['cycles'])} instances, period {args.period:.4f} s (the open record; 'closed': the last closed one)")
    print(f"{'instance':>8} {'record':>7} {'cycles':>6} {'first':>6} {'end':>8} {'track rms':>10} {'track max':>10} {'dist [m]':>9} {'path [m]':>9} {'z min':>7} {'z max':>7} "
          f"{'tilt max':>8} {'sat share':>9} {'tau ratio':>9} {'work+ [J]':>10} {'flight':>6} {'touchdowns':>10} {'load max':>9} {'pen max':>8} {'cost mean':>11} {'steps':>6} {'rej':>5}")
    for b in range(len(cur["cycles"])):
        for label, r in (("open", cur), ("closed", prev)):
            n = int(r["cycles"][b])
            if not n:
                continue
            dist = float(np.linalg.norm(r["end_xy"][b] - r["start_xy"][b]))
            sat = r["saturated_samples"][b] / r["torque_samples"][b] if r["torque_samples"][b] else 0.0
            print(f"{b:8d} {label:>7} {n:6d} {int(r['first_cycle'][b]):6d} {causes.get(int(r['end_cause'][b]), '?'):>8} {np.sqrt(r['vel_err_sq'][b] / n):10.5f} "
                  f"{r['vel_err_max'][b]:10.5f} {dist:9.4f} {r['path_length'][b]:9.4f} {r['height_min'][b]:7.4f} {r['height_max'][b]:7.4f} {r['tilt_max'][b]:8.4f} "
                  f"{sat:9.4f} {r['tau_ratio_max'][b]:9.4f} {r['work_pos'][b]:10.3f} {int(r['flight_samples'][b]):6d} "
                  f"{'%d/%d' % tuple(int(v) for v in r['touchdowns'][b]):>10} {r['load_max'][b]:9.1f} {r['penetration_max'][b]:8.5f} {r['cost_sum'][b] / n:11.4e} "
                  f"{int(r['rollout_steps'][b]):6d} {int(r['rollout_rejected'][b]):5d}")
    sm = s.metrics_summary(cur)
    torque = int(cur["torque_samples"].sum() + prev["torque_samples"].sum())
    sm = {k: (round(v, 6) if isinstance(v, float) else v) for k, v in sm.items()}
    sm["saturated_sample_share"] = round(float((cur["saturated_samples"].sum() + prev["saturated_samples"].sum()) / torque), 4) if torque else None
    sm["closed_records"] = int((prev["cycles"] > 0).sum())
    return sm, cur, prev


def centroidal_run(args):
    """The centroidal loop (include/hsqp_cent_loop.h): resident cycles and, from the same run, the same cycles driven by the public calls."""
    m = load_model(formulation="centroidal")
    B, N, dt = args.batch, args.nodes, m.sqp["dt"]
    total = args.warmup + 2 * args.cycles
    t_final = 2 * total * args.period + N * dt + 1.0
    schedules = [tile_gait(m.gaits[args.schedule], 0.3 + 0.5 * b / B, t_final) for b in range(B)]
    n_events, event_times, mode_sequence = pack_reference(schedules, [dummy_knots(m, True, t_final)] * B)[:3]
    rng = np.random.default_rng(20250808)
    x_init = np.tile(padded_state(m), (B, 1))
    x_init[:, 12:12 + m.nj] += 0.01 * rng.standard_normal((B, m.nj))
    cmd = np.tile((0.3, 0.0, 0.7925, 0.0), (B, 1))
    if args.commands == "spread":
        cmd[:, 0] = np.linspace(0.0, 0.6, B)
        cmd[:, 3] = np.linspace(-0.2, 0.2, B)
    if args.commands == "stand":
        cmd[:, 0] = 0.0
    # (no persistent back-off of the KKT gate: the driven and the resident cycles share this handle and must take the same sweeps)
    s = HipSqpSolver(m, max_nodes=N, max_batch=B, linesearch=True, riccati="serial" if args.isolate else "auto")
    st = s.loop_settings(N, dt, period=args.period, filter_alpha=args.filter_alpha, iterations=1, take_step=True, linesearch=True, controller=args.controller)
    sw = swing_config(m)
    cycle_ms, driven_ms, heights = [], [], []
    try:
        if args.with_push is not None:
            s.set_pushes([[dict(body=0, t_start=0.0, duration=1e6, point=(0.0, 0.0, 0.0), force=(0.0, args.with_push, 0.0))]] * B)
        # the cycles driven from the host through the public calls
        from wb_humanoid_mpc_amd.solver import HsqpError
        x, vf, t = x_init.copy(), cmd.copy(), 0.0
        driven_stopped = resident_stopped = None
        for c in range(args.warmup + args.cycles):
            t_a = time.perf_counter()
            try:
                tt, ts, vf = s.command_targets(cmd, x, t, N * dt, filter_alpha=args.filter_alpha, v_filt=vf)
                s.upload_reference_warm(x, N, dt, t, n_events, event_times, mode_sequence, tt, ts, sw, mode="cold" if c == 0 else "shift")
                s.iterate(1, take_step=True, linesearch=True)
                x = s.rollout_policy(np.zeros(B), x, args.period, 1, controller=args.controller)["x"][:, 0].copy()
            except HsqpError as e:
                driven_stopped = f"cycle {c}: {e}"
                break
            t_b = time.perf_counter()
            t += args.period
            if c >= args.warmup:
                driven_ms.append(1e3 * (t_b - t_a))
        driven_x, driven_cycles = x, c + (driven_stopped is None)
        # the resident loop
        s.loop_start(st, 0.0, x_init, cmd, n_events, event_times, mode_sequence)
        if args.isolate:
            s.loop_isolate(s.episode_settings(args.isolate))
        same = None
        for c in range(args.warmup + args.cycles):
            t_a = time.perf_counter()
            try:
                r = s.loop_run(1)
            except HsqpError as e:
                resident_stopped = f"cycle {c}: {e}"
                break
            t_b = time.perf_counter()
            heights.append(r["x"][0, :, 8].copy())
            if c >= args.warmup:
                cycle_ms.append(1e3 * (t_b - t_a))
            if c + 1 == driven_cycles:                            # the state after as many cycles as the driven part completed
                same = bool(np.array_equal(r["x"][0], driven_x))
        t_a = time.perf_counter()
        done, stopped = 0, None
        try:
            if resident_stopped is None:
                done = s.loop_run(args.cycles, log=False)["cycles_done"]
        except HsqpError as e:
            done, stopped = e.result["cycles_done"], str(e)
        run_ms = 1e3 * (time.perf_counter() - t_a) / max(done, 1)
        t_end, x_end, _ = s.loop_state()
        ep = s.loop_episodes() if args.isolate else None
    finally:
        s.close()
    heights = np.concatenate(heights + [x_end[:, 8]])
    stat = lambda v, f: round(float(f(v)), 3) if len(v) else None  # noqa: E731
    q = [stat(cycle_ms, lambda v: np.percentile(v, 25)), stat(cycle_ms, lambda v: np.percentile(v, 75))]
    qd = [stat(driven_ms, lambda v: np.percentile(v, 25)), stat(driven_ms, lambda v: np.percentile(v, 75))]
    return {"metric": "device_loop_cycle", "formulation": "centroidal", "batch": B, "nodes": N, "dt": dt, "period": args.period, "cycles": args.cycles,
            "controller": args.controller, "commands": args.commands, "filter_alpha": args.filter_alpha, "isolate": args.isolate, "with_push": args.with_push,
            "episodes": {"failed_now": int((ep["state"] != 0).sum()), "failures": int(ep["n_failures"].sum()), "episodes": int(ep["n_episodes"].sum())} if ep else None,
            "schedule": args.schedule,
            "cycle_ms_median": stat(cycle_ms, np.median), "cycle_ms_mean": stat(cycle_ms, np.mean), "cycle_ms_quartiles": q, "cycle_ms_min": stat(cycle_ms, np.min),
            "run_ms_per_cycle": round(float(run_ms), 3) if done else None, "run_cycles_done": int(done), "run_stopped": stopped,
            "driven_ms_median": stat(driven_ms, np.median), "driven_ms_mean": stat(driven_ms, np.mean), "driven_ms_quartiles": qd, "driven_ms_min": stat(driven_ms, np.min),
            "driven_stopped": driven_stopped, "resident_stopped": resident_stopped, "resident_equals_driven": same, "t_end": round(float(t_end), 6), "finite": bool(np.isfinite(x_end).all()),
            "base_height_range": [round(float(np.nanmin(heights)), 5), round(float(np.nanmax(heights)), 5)]}


def timed_run(args, observe):
    """The timed loop (with the observation model of --observe on or off): the fields of the JSON line."""
    m = load_model()
    B, N, dt = args.batch, args.nodes, m.sqp["dt"]
    t_final = (2 * args.warmup + 2 * args.cycles) * args.period + N * dt + 1.0
    schedules = [tile_gait(m.gaits[args.schedule], 0.3 + 0.5 * b / B, t_final) for b in range(B)]
    knots = velocity_command_targets(m, (0.3, 0.0, 0.7925, 0.0), 0.0, m.initial_state, t_final)
    n_events, event_times, mode_sequence = pack_reference(schedules, [knots] * B)[:3]
    rng = np.random.default_rng(20250808)
    x_init = np.tile(m.initial_state, (B, 1))
    x_init[:, 6:6 + m.nj] += 0.01 * rng.standard_normal((B, m.nj))
    cmd = np.tile((0.3, 0.0, 0.7925, 0.0), (B, 1))
    if args.commands == "spread":
        cmd[:, 0] = np.linspace(0.0, 0.6, B)
        cmd[:, 3] = np.linspace(-0.2, 0.2, B)
    if args.commands == "stand":
        cmd[:, 0] = 0.0
    s = HipSqpSolver(m, max_nodes=N + (args.event_grid or 0), max_batch=B, linesearch=True)
    s.set_scan_backoff_persistent(True)
    st = s.loop_settings(N, dt, period=args.period, filter_alpha=args.filter_alpha, iterations=1, take_step=True, linesearch=True,
                         controller=args.controller)
    cycle_ms, heights, track = [], [], []
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
        if observe:                                               # before the start: a started loop holds its delays
            sigma, bias = np.full((B, 58), args.obs_noise), np.zeros((B, 58))
            bias[:, 2] = args.obs_bias
            s.set_observation(sensor_delay=args.sensor_delay, compute_delay=args.compute_delay, seed=args.obs_seed)
            s.set_observation_instances(bias, sigma)
        if args.gait:
            s.loop_start(st, 0.0, x_init, cmd, gait=gait_settings(m))
        else:
            s.loop_start(st, 0.0, x_init, cmd, n_events, event_times, mode_sequence)
        if args.isolate:
            s.loop_isolate(s.episode_settings(args.isolate))
        elif args.terrain:
            s.loop_isolate(s.episode_settings("park", min_base_height=0.45, max_tilt=0.7))
        if args.with_push is not None:
            s.set_pushes([[dict(body=0, t_start=0.0, duration=1e6, point=(0.0, 0.0, 0.0), force=(0.0, args.with_push, 0.0))]] * B)
        if args.plant:
            s.set_plant(kind=args.plant, kp=args.kp, kd=args.kd, armature=args.armature, lookahead=args.lookahead)
        if args.contact:
            s.set_contact(**contact_args(args))
        if args.actuator:
            s.set_actuator(**actuator_args(args, m))
        labels = None
        if args.terrain:
            maps, place, labels = terrain_args(args, x_init)
            s.set_terrain_maps(maps)
            s.set_terrain_instances(place)
        if args.metrics:
            s.loop_metrics_enable()
        if args.event_grid is not None:
            s.loop_event_grid(s.grid_settings(event_nodes=args.event_grid))
        if args.ground_adapt == "on":
            s.loop_ground(s.ground_settings(box_above_ground=args.box_above_ground))
        if args.perceive:
            s.loop_perceive()
        last_pos = x_init[:, :3].copy()
        masses = None
        if args.inertia:
            s.set_inertia_instances(*inertia_args(args, B))
            masses = s.plant_dynamics(x_init)[2]
        for c in range(args.warmup + args.cycles):
            if c in changes:
                s.loop_command(changes[c])
                cmd = changes[c]
            t_a = time.perf_counter()
            r = s.loop_run(1)
            t_b = time.perf_counter()
            heights.append(r["x"][0, :, 2].copy())
            live = np.isfinite(r["x"][0]).all(axis=1)
            last_pos[live] = r["x"][0][live, :3]
            if c >= args.warmup:
                cycle_ms.append(1e3 * (t_b - t_a))
                track.append(np.nanmean(tracking_error(m, r["x"][0], cmd)))
        t_a = time.perf_counter()
        r = s.loop_run(args.cycles, log=False)
        run_ms = 1e3 * (time.perf_counter() - t_a) / args.cycles
        t_end, x_end, v_filt = s.loop_state()
        rungs = np.bincount(s.gait_state()["rung"], minlength=7).tolist() if args.gait else None
        ep = s.loop_episodes() if args.isolate or args.terrain else None
        heights.append(x_end[:, 2].copy())
        saturated = saturated_share(s, m, args) if args.actuator else None
        metrics = None
        if args.metrics:                                          # the records instead of logs and of the last actuator record
            metrics, rec, rec_prev = metrics_report(s, args, ep)
            seen = (rec["torque_samples"] + rec_prev["torque_samples"]) > 0
            if args.actuator:
                saturated = round(float(((rec["saturated_samples"] + rec_prev["saturated_samples"])[seen] > 0).mean()), 4) if seen.any() else 0.0
            for r in (rec_prev, rec):                             # where an instance ended: its open record's last sample, else its last closed record's
                have = r["cycles"] > 0
                last_pos[have, :2] = r["end_xy"][have]
        probe = rollout_probe(s, args, x_end) if args.plant else None
        counts = s.loop_grid()["n_intervals"] if args.event_grid is not None else None
        ground = None
        if args.ground_adapt:
            alive = np.isfinite(x_end).all(axis=1) & ((ep["state"] == 0) if ep else True)
            local = s.terrain_height(np.where(alive[:, None, None], x_end[:, None, :2], 0.0))[0][:, 0] if args.terrain else np.zeros(B)
            above = (x_end[:, 2] - local)[alive]
            est = s.loop_ground_state()[0][alive] if args.ground_adapt == "on" else None
            ground = dict(adapt=args.ground_adapt, box_above_ground=args.box_above_ground, alive=int(alive.sum()),
                          local_ground_range=[round(float(local[alive].min()), 4), round(float(local[alive].max()), 4)] if alive.any() else None,
                          height_above_ground_mean=round(float(above.mean()), 4) if alive.any() else None,
                          height_above_ground_range=[round(float(above.min()), 4), round(float(above.max()), 4)] if alive.any() else None,
                          estimate_range=[round(float(est.min()), 4), round(float(est.max()), 4)] if est is not None and alive.any() else None,
                          estimate_error_max=round(float(np.abs(est - local[alive]).max()), 4) if est is not None and alive.any() else None)
        perceive = None
        if args.perceive:
            alive = np.isfinite(x_end).all(axis=1) & (ep["state"] == 0)
            lift, touch, _ = s.loop_foot_heights()
            step = np.abs(touch - lift - st.swing.touch_down_height_offset)[alive]
            perceive = dict(alive=int(alive.sum()), lift_off_range=[round(float(lift[alive].min()), 4), round(float(lift[alive].max()), 4)] if alive.any() else None,
                            step_max=round(float(step.max()), 4) if alive.any() else None)
    finally:
        s.close()
    heights = np.concatenate(heights)
    terrain = None
    if args.terrain:
        total = args.warmup + 2 * args.cycles
        live = np.isfinite(x_end).all(axis=1)
        if not args.metrics:
            last_pos[live] = x_end[live, :3]
        survived = np.where(ep["n_failures"] > 0, ep["fail_cycle"], total).astype(int)
        where = "x, y from the episode metrics' records" if args.metrics else "the last one logged (the second half of the run keeps no log)"
        print(f"terrain {args.terrain}: {B} instances, {total} cycles of {args.period:.4f} s; final base position: {where}")
        print(f"{'instance':>8} {'map':>4} {'difficulty':>10} {'survived':>9} {'base x':>9} {'base y':>9} {'base z':>9}")
        for b in range(B):
            print(f"{b:8d} {b % TERRAIN_MAPS:4d} {labels[b % TERRAIN_MAPS]:>10} {survived[b]:9d} {last_pos[b, 0]:9.4f} {last_pos[b, 1]:9.4f} {last_pos[b, 2]:9.4f}")
        per_map = [[int((survived[k::TERRAIN_MAPS] == total).sum()), int(len(survived[k::TERRAIN_MAPS]))] for k in range(min(TERRAIN_MAPS, B))]
        terrain = dict(kind=args.terrain, seed=args.terrain_seed, difficulty=labels[:len(per_map)], survivors_per_map=per_map, survivors=int((survived == total).sum()),
                       cycles_survived_mean=round(float(survived.mean()), 2))
    q = np.percentile(cycle_ms, [25, 75])
    finished = np.isfinite(x_end).all(axis=1) & ((ep["state"] == 0) if ep else True)
    if args.inertia:
        for b in range(B):
            print(f"instance {b}: total mass {masses[b]:.3f} kg, finished {'yes' if finished[b] else 'no'}")
    extra = {"metrics": metrics} if args.metrics else {}
    if args.ground_adapt:
        extra["ground"] = ground
    if args.perceive:
        extra["perceive"] = perceive
    if args.event_grid is not None:
        extra["event_grid"] = dict(event_nodes=args.event_grid, schedule=args.schedule, intervals=N + args.event_grid, n_intervals_range=[int(counts.min()), int(counts.max())])
    return dict({"metric": "device_loop_cycle", "batch": B, "nodes": N, "dt": dt, "period": args.period, "cycles": args.cycles,
                      "controller": args.controller, "commands": args.commands, "filter_alpha": args.filter_alpha, "gait": args.gait, "instances_per_rung": rungs, "isolate": args.isolate, "with_push": args.with_push,
                      "plant": dict(kind=args.plant, kp=args.kp, kd=args.kd, armature=args.armature, lookahead=args.lookahead) if args.plant else None,
                      "contact": contact_args(args) if args.contact else None,
                      "actuator": dict(actuator_args(args, m), effort_limits=args.effort_limits, saturated_share=saturated) if args.actuator else None,
                      "inertia": dict(mass_spread=args.mass_spread, payload=args.payload, total_mass_range=[round(float(masses.min()), 3), round(float(masses.max()), 3)],
                                      finished=int(finished.sum())) if args.inertia else None, "terrain": terrain, "rollout_probe": probe,
                      "episodes": {"failed_now": int((ep["state"] != 0).sum()), "failures": int(ep["n_failures"].sum()), "episodes": int(ep["n_episodes"].sum())} if ep else None,
                      "cycle_ms_median": round(float(np.median(cycle_ms)), 3), "cycle_ms_mean": round(float(np.mean(cycle_ms)), 3),
                      "cycle_ms_quartiles": [round(float(q[0]), 3), round(float(q[1]), 3)], "cycle_ms_min": round(float(np.min(cycle_ms)), 3),
                      "run_ms_per_cycle": round(float(run_ms), 3), "t_end": round(float(t_end), 6),
                      "status_counts": {"ok": int(B * (args.warmup + 2 * args.cycles)), "max_steps": 0, "nonfinite": 0},
                      "forward_speed_range": [round(float(x_end[:, 6 + m.nj].min()), 4), round(float(x_end[:, 6 + m.nj].max()), 4)],
                      "base_height_range": [round(float(heights.min()), 5), round(float(heights.max()), 5)],
                      "observe": dict(noise=args.obs_noise, height_bias=args.obs_bias, sensor_delay=args.sensor_delay, compute_delay=args.compute_delay,
                                      seed=args.obs_seed) if observe else None,
                      "tracking": dict(mean=round(float(np.mean(track)), 5), end=round(float(np.nanmean(tracking_error(m, x_end, cmd))), 5))}, **extra)


if __name__ == "__main__":
    main()
