"""TEST HELPER: numpy restatement of the per-foot swing heights read from the height map (include/hsqp_perceive.h), written from the header's text
and from SwingTrajectoryPlanner.cpp:101-191, on the reference module's UNCHANGED body_placements, tests/terrain_ref.py's height_normal and
TargetTrajectories.desired_state.

  sequences        the rule of section 2 for one instance, by contact RUNS: [(first phase, last phase)] of each foot, one foothold and one height per run,
                   then the swing phases from their neighbouring runs
  planner_oracle   the three-argument update composed from the REFERENCE'S OWN compiled SplineCpg (oracle/ref_swing.py, RefSwing.spline_cpg): per foot
                   and phase the nodes and the mid height of lines 130-186, evaluated by the reference's code
  case             the shapes of the tests: B = 3 instances (a ledge, the plane, a ramp), their schedules, states, targets, maps and placements
"""
import bisect
import math

import numpy as np

import terrain_ref as TR
from wb_humanoid_mpc_amd import reference as ref
from wb_humanoid_mpc_amd.reference import FLY, LF, RF, STANCE

NV = 29
B, N, E = 3, 8, 6


# ---------------------------------------------------------------------------------------------- the rule
def contact_xy(model, q, f):
    R, p = ref.body_placements(model, np.asarray(q, dtype=float)[:NV])
    fr = model.raw["frames"]["contact"][f]
    return (p[fr["body"]] + R[fr["body"]] @ np.array(fr["p"], dtype=float))[:2]


def runs(flags):
    """[(a, z)]: the maximal ranges a .. z of consecutive True entries"""
    out, a = [], None
    for p, c in enumerate(list(flags) + [False]):
        if c and a is None:
            a = p
        if not c and a is not None:
            out.append((a, p - 1))
            a = None
    return out


def sequences(model, x, t, n_events, event_times, mode_sequence, target_times, target_states, ground, offset):
    """(lift [2][E + 1], touch [2][E + 1], foothold_xy [2][E + 1][2]) of one instance; ground(X, Y): hsqp_terrain_eval's answer.  Entries of phases past
    n_events are 0; a non-finite state gives NaN in phases 0 .. n_events."""
    E1 = len(mode_sequence)
    n = int(n_events) + 1
    lift, touch, fxy = np.zeros((2, E1)), np.zeros((2, E1)), np.zeros((2, E1, 2))
    x = np.asarray(x, dtype=float)
    if not np.isfinite(x).all():
        lift[:, :n], touch[:, :n], fxy[:, :n] = np.nan, np.nan, np.nan
        return lift, touch, fxy
    ev = [float(v) for v in event_times[:n - 1]]
    p_now = bisect.bisect_left(ev, t)
    targets = ref.TargetTrajectories(target_times, target_states)
    nominal = np.zeros(NV)
    nominal[6:] = model.default_joint_state
    for f in range(2):
        P, o = contact_xy(model, x, f), contact_xy(model, nominal, f)
        c = [ref.mode_to_contact_flags(int(m))[f] for m in mode_sequence[:n]]
        found = []
        for a, z in runs(c):
            if a <= p_now:
                F = P
            else:
                d = targets.desired_state(ev[a - 1])
                cs, sn = math.cos(d[3]), math.sin(d[3])
                F = np.array([d[0] + cs * o[0] - sn * o[1], d[1] + sn * o[0] + cs * o[1]])
            h = ground(F[0], F[1])
            found.append((a, z, F, h))
            lift[f, a:z + 1], touch[f, a:z + 1], fxy[f, a:z + 1] = h, h + offset, F
        for p in range(n):
            if c[p]:
                continue
            before = [r for r in found if r[1] < p]
            after = [r for r in found if r[0] > p]
            lift[f, p] = before[-1][3] if before else ground(P[0], P[1])
            touch[f, p] = (after[0][3] if after else lift[f, p]) + offset
            fxy[f, p] = after[0][2] if after else P
    return lift, touch, fxy


def ground_of(maps, place, ground_height):
    """ground(X, Y) of one instance: its contact ground height plus its map's height (steps 1-8 of include/hsqp_terrain.h)"""
    mp = None if place is None or place["map"] < 0 else maps[place["map"]]
    return lambda X, Y: ground_height + float(TR.height_normal(mp, place, X, Y)[0])


def batch_sequences(model, c, t, x=None):
    """sequences over the instances of a case: (lift [B][2][E + 1], touch, foothold_xy [B][2][E + 1][2])"""
    x = c["x"] if x is None else x
    out = [sequences(model, x[b], t, c["ne"][b], c["ev"][b], c["seq"][b], c["tt"][b], c["ts"][b], ground_of(c["maps"], c["place"][b], c["ground"][b]), c["offset"])
           for b in range(len(x))]
    return tuple(np.array([o[k] for o in out]) for k in range(3))


# ---------------------------------------------------------------------------------------------- the planner, composed from the reference's compiled splines
def planner_oracle(rs, cfg, event_times, mode_sequence, lift, touch, times):
    """[len(times)][2][3] = (z, zdot, zddot) per foot of SwingTrajectoryPlanner::update(modeSchedule, liftOffHeightSequence, touchDownHeightSequence)
    followed by the look-up at each time: lines 107-186 restated, every spline evaluated by the reference's own compiled SplineCpg."""
    ev, seq = [float(v) for v in event_times], [int(m) for m in mode_sequence]
    n = len(seq)
    out = np.zeros((len(times), 2, 3))
    for j in range(2):
        c = [ref.mode_to_contact_flags(m)[j] for m in seq]
        for k, t in enumerate(times):
            p = bisect.bisect_left(ev, t)
            L, T = float(lift[j][p]), float(touch[j][p])
            if c[p]:
                out[k, j] = rs.spline_cpg((0.0, L, 0.0), L, (1.0, L, 0.0), [t])[0]
                continue
            start = max(q for q in range(p) if c[q])                       # the phase the foot left the ground in: the swing starts at its end
            final = min(q for q in range(p + 1, n) if c[q]) - 1            # the last phase in the air: the swing ends at its end
            t0, t1 = ev[start], ev[final]
            scaling = min(1.0, (t1 - t0) / cfg["swingTimeScale"])
            if c[p - 1] and c[p + 1]:
                node0, mid, node1 = (t0, L, scaling * cfg["liftOffVelocity"]), min(L, T) + scaling * cfg["swingHeight"], (t1, T, scaling * cfg["touchDownVelocity"])
            elif c[p - 1]:
                mid = L + cfg["swingHeight"]
                node0, node1 = (t0, L, cfg["liftOffVelocity"]), (t1, mid, 0.0)
            elif c[p + 1]:
                mid = T + cfg["swingHeight"]
                node0, node1 = (t0, mid, 0.0), (t1, T, cfg["touchDownVelocity"])
            else:
                mid = T + cfg["swingHeight"]
                node0, node1 = (t0, mid, 0.0), (t1, mid, 0.0)
            out[k, j] = rs.spline_cpg(node0, mid, node1, [t])[0]
    return out


# ---------------------------------------------------------------------------------------------- the shapes of the tests
EV_SHORT = np.array([0.125, 0.25, 0.375, 0.5, 0.5, 0.5])                   # binary fractions: a node at t0 + k dt with dt = 0.0625 can sit exactly on an event
SEQ_0 = np.array([STANCE, RF, FLY, LF, STANCE, STANCE, STANCE], np.int32)  # either foot: a leaving-only and a landing-only phase
SEQ_1 = np.array([STANCE, RF, FLY, RF, STANCE, STANCE, STANCE], np.int32)  # the left foot in the air for the last, current and next phase; the right: a plain swing
EV_GROUND = np.array([1.0, 2.0, 3.0, 4.0, 4.0, 4.0])                       # EVENTS / SEQ / N_EVENTS of tests/test_ground.py
SEQ_GROUND = np.array([STANCE, LF, RF, FLY, STANCE, STANCE, STANCE], np.int32)
TIMES = (0.0, 0.125, 0.3, 0.45, 1.5, 2.0, 2.5, 3.5, 9.0)                   # 0.125 and 2.0 lie exactly on events; runs that began before now and runs ahead
LEDGE_HEIGHT = 0.03


def case(model, seed=20261020):
    """B = 3: instance 0 on a ledge map whose step lies between the current and the predicted foothold of its left foot (in the air from 0.125 s, landing
    at 0.375 s), instance 1 on the plane (map -1, contact ground height 0.02), instance 2 on a 5 degree ramp placed with yaw 0.3 and origin (-0.5, -0.8)
    under a ground height of -0.01.  Targets: the velocity command's knots over 0.5 s (instances 0, 1) and 4 s (instance 2)."""
    rng = np.random.default_rng(seed)
    x = np.tile(model.initial_state, (B, 1))
    x[:, 6:6 + model.nj] += 0.02 * rng.standard_normal((B, model.nj))
    x[:, 3] = [0.1, -0.4, 0.25]
    x[:, 4:6] += 0.02 * rng.standard_normal((B, 2))
    x[:, 0:2] = [[0.3, -0.2], [-1.0, 0.5], [0.2, 0.1]]
    cmd = [(0.5, 0.0, 0.79, 0.0), (0.3, 0.1, 0.79, 0.2), (0.3, -0.05, 0.79, -0.1)]
    horizon = (0.5, 0.5, 4.0)
    knots = [ref.velocity_command_targets(model, cmd[b], 0.0, x[b], horizon[b]) for b in range(B)]
    tt, ts = np.stack([k.times for k in knots]), np.stack([k.states for k in knots])
    ne = np.array([4, 4, 4], np.int32)
    ev, seq = np.stack([EV_SHORT, EV_SHORT, EV_GROUND]), np.stack([SEQ_0, SEQ_1, SEQ_GROUND])
    # the ledge: its one-cell slope (x in [0.02, 0.03] of the map, along the world x: yaw 0) half-way between where instance 0's left foot stands and where
    # the targets carry its nominal foothold at the touch-down time 0.375
    nominal = np.zeros(NV)
    nominal[6:] = model.default_joint_state
    P, o = contact_xy(model, x[0], 0), contact_xy(model, nominal, 0)
    d = knots[0].desired_state(0.375)
    Fx = d[0] + math.cos(d[3]) * o[0] - math.sin(d[3]) * o[1]
    assert Fx - P[0] > 0.05
    ledge = TR.ledge_map(LEDGE_HEIGHT, 0.01)
    ramp = TR.ramp_map(5.0, 2.0)
    maps = [ledge, ramp]
    place = [TR.placement((0.5 * (P[0] + Fx) - 0.025, P[1] - 0.02), 0.0, 0), dict(map=-1, origin=(0.0, 0.0), yaw=0.0), TR.placement((-0.5, -0.8), 0.3, 1)]
    return dict(x=x, ne=ne, ev=ev, seq=seq, tt=tt, ts=ts, maps=maps, place=place, ground=np.array([0.0, 0.02, -0.01]), offset=model.swing["touchDownHeightOffset"],
                knots=knots, cmd=np.array(cmd))
