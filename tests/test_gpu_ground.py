"""The per-instance ground-height estimate from the stance feet (include/hsqp_ground.h) on the MI355X: k_ground_estimate against the numpy
restatement (tests/ground_ref.py) and its device twin bit for bit, the estimate's feet against the contact flags of the problem, the per-instance
terrain height as the scalar generalised, the resident loop with the setting on against the public calls it replaces bit for bit (two integrators and
controllers, a resident gait, the observation model, isolation), the lift invariance the feature exists for, the absence of it without the setting,
the base-height box above the ground, and the refusals.  Shapes: N = 20 nodes, five cycles, B = 8 with the serial recursion unless noted."""
import ctypes as C
import signal

import numpy as np
import pytest

import ground_ref as G
import observe_ref as O
from test_gpu_feedback_policy import DeviceBuffer
from test_gpu_grid import int_buffer
from test_ground import ATOL_DEVICE, EVENTS, N_EVENTS, SEQ, random_states
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import FLY, LF, RF, STANCE, gait_settings, mode_to_contact_flags, pack_reference, swing_config, tile_gait, velocity_command_targets
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu

NX, NU, NJ, KNOTS = _abi.NX, _abi.NU, _abi.NJ, _abi.CMD_KNOTS
B, N, CYCLES, PERIOD, ALPHA = 8, 20, 5, 1.0 / 60.0, 0.8
LIFT = 0.125
# The lift invariance of the PARENT commit, lifted by hand (terrain_height = 0.125, command height + 0.125, x0 raised, no setting) against its own base
# run over the same five cycles of lift_case(): max |x_B - x_A - 0.125 e_2| over every logged entry, measured on one MI355X (profiles/ground_loop.txt).
# It is NOT a rounding figure: see test_lift_invariance.  The test allows ten times it.
LIFT_PARENT = 9.036939058594532
_ip, _dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)


@pytest.fixture(autouse=True)
def time_limit():
    def expired(signum, frame):
        raise TimeoutError("test_gpu_ground: a test ran past its 120 s limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture
def s(model):
    h = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    yield h
    h.close()


def settings(s, model, integrator="ode45", controller="feedforward", alpha=ALPHA):
    return s.loop_settings(N, model.sqp["dt"], period=PERIOD, filter_alpha=alpha, iterations=1, take_step=True, linesearch=True, integrator=integrator,
                           controller=controller)


def loop_case(model, batch=B, seed=20261019):
    """Walk schedules that start between 0.05 s and 0.3 s, so that the five cycles and the horizon see stance, single support and their switches;
    instance b stands on a ground 2 b cm up (the whole state is raised), commands spread."""
    rng = np.random.default_rng(seed)
    schedules = [tile_gait(model.gaits["walk"], 0.05 + 0.25 * b / batch, 3.0) for b in range(batch)]
    dummy = velocity_command_targets(model, (0.0, 0.0, 0.79, 0.0), 0.0, model.initial_state, 1.0)
    ne, ev, seq = pack_reference(schedules, [dummy] * batch)[:3]
    x0 = np.tile(model.initial_state, (batch, 1))
    x0[:, 6:6 + NJ] += 0.01 * rng.standard_normal((batch, NJ))
    x0[:, 3] += 0.05 * rng.standard_normal(batch)
    x0[:, 2] += 0.02 * np.arange(batch)
    cmd = np.column_stack([rng.uniform(0.0, 0.5, batch), rng.uniform(-0.1, 0.1, batch), rng.uniform(0.77, 0.8, batch), rng.uniform(-0.2, 0.2, batch)])
    return dict(ne=ne, ev=ev, seq=seq, x0=x0, cmd=cmd)


# ---------------------------------------------------------------------------------------------- 1. the kernel against the mirror
def shifted_schedules(rows):
    """test_ground.py's schedule of every mode, instance b's events b mod 4 seconds later: one launch holds several modes"""
    ev = np.array([EVENTS + (b % 4) for b in range(rows)])
    return np.full(rows, N_EVENTS, np.int32), ev, np.tile(SEQ, (rows, 1))


@pytest.mark.parametrize("rows", [1, 33, 64])
def test_estimate_and_its_device_twin_equal_the_mirror(model, rows):
    """rows = 33 is one instance past a workgroup of 32 pairs: the live guard and the pair exchange.  A canary row behind g and foot_z."""
    s = HipSqpSolver(model, max_nodes=4, max_batch=64)
    CANARY = -12345.678
    bufs = []
    try:
        x = random_states(model, rows, seed=100 + rows)
        ne, ev, seq = shifted_schedules(rows)
        want_fz = np.array([G.foot_heights(model, xb) for xb in x])
        g0 = np.linspace(-0.2, 0.3, rows)
        seen = set()
        for t in (0.5, 1.5, 2.5, 3.5, 2.0, 5.0, 9.0):                        # 2.0 and 5.0 lie exactly on event times of some instances
            for alpha in (0.0, 0.8):
                g, fz = s.ground_estimate(x, t, ne, ev, seq, g0, alpha)
                want, _ = G.estimate(model, x, t, ne, ev, seq, g0, alpha, foot_z=want_fz)   # (the mirror's rule on the mirror's own heights)
                assert np.abs(fz - want_fz).max() <= ATOL_DEVICE and np.abs(g - want).max() <= ATOL_DEVICE, (t, alpha)
                exact, _ = G.estimate(model, x, t, ne, ev, seq, g0, alpha, foot_z=fz)     # the rule on the device's own heights: no transcendental, the same bits
                assert np.array_equal(g, exact), (t, alpha)
                modes = [G.mode_at(ne[b], ev[b], seq[b], t) for b in range(rows)]
                seen.update(modes)
                fly = np.array(modes) == FLY
                assert np.array_equal(g[fly], g0[fly])
                # the device twin, in place on g
                bufs = [DeviceBuffer((rows, NX)), int_buffer(ne, rows), DeviceBuffer(ev.shape), int_buffer(seq, rows), DeviceBuffer((rows + 1,), fill=CANARY),
                        DeviceBuffer((rows + 1, 2), fill=CANARY)]
                bufs[0].upload(x); bufs[2].upload(ev); bufs[4].upload(np.concatenate([g0, [CANARY]]))
                s.ground_estimate_device(rows, t, bufs[0].ptr.value, ev.shape[1], bufs[1].ptr.value, bufs[2].ptr.value, bufs[3].ptr.value, bufs[4].ptr.value,
                                         bufs[5].ptr.value, filter_alpha=alpha)
                dg, dfz = bufs[4].numpy(), bufs[5].numpy()
                assert np.array_equal(dg[:rows].view(np.uint64), g.view(np.uint64)) and np.array_equal(dfz[:rows].view(np.uint64), fz.view(np.uint64)), (t, alpha)
                assert dg[rows] == CANARY and (dfz[rows] == CANARY).all()
                for b in bufs:
                    b.free()
                bufs = []
        assert seen == {STANCE, LF, RF, FLY}, seen
    finally:
        for b in bufs:
            b.free()
        s.close()


# ---------------------------------------------------------------------------------------------- 2. agreement with the problem
def reference_args(model, case, t, x=None):
    """What upload_reference* takes behind x_init, n_nodes and dt, for the case's commands at time t"""
    x = case["x0"] if x is None else x
    targets = [velocity_command_targets(model, tuple(case["cmd"][b]), t, x[b], N * model.sqp["dt"]) for b in range(len(x))]
    tt, ts = np.stack([k.times for k in targets]), np.stack([k.states for k in targets])
    return dict(ne=case["ne"], ev=case["ev"], seq=case["seq"], tt=tt, ts=ts)


def test_the_estimate_selects_the_feet_the_problem_flags(s, model):
    case = loop_case(model)
    dt, sw = model.sqp["dt"], swing_config(model)
    patterns = set()
    for t in (0.0, 0.2, 0.45, 0.7, float(case["ev"][3, 2])):                 # the last one: exactly on an event of instance 3
        r = reference_args(model, case, t)
        sentinel = np.full(B, 7.0)
        g, fz = s.ground_estimate(case["x0"], t, r["ne"], r["ev"], r["seq"], sentinel)
        s.upload_reference_ground(case["x0"], N, dt, t, r["ne"], r["ev"], r["seq"], r["tt"], r["ts"], sw, g, mode="cold")
        flags = s.device_params()[:, 0, _abi.P_CONTACT:_abi.P_CONTACT + 2]
        for b in range(B):
            left, right = bool(flags[b, 0]), bool(flags[b, 1])
            want = 0.5 * (fz[b, 0] + fz[b, 1]) if left and right else (fz[b, 0] if left else (fz[b, 1] if right else 7.0))
            assert g[b] == want, (t, b, flags[b])
            patterns.add((left, right))
    assert len(patterns) >= 3, patterns                                      # double support and both single supports were met


# ---------------------------------------------------------------------------------------------- 3. per-instance terrain is the scalar, generalised
def test_per_instance_terrain_heights_generalise_the_scalar(s, model):
    case = loop_case(model)
    dt, sw, t = model.sqp["dt"], swing_config(model), 0.2
    r = reference_args(model, case, t)
    args = (r["ne"], r["ev"], r["seq"], r["tt"], r["ts"], sw)
    s.upload_reference_warm(case["x0"], N, dt, t, *args, terrain_height=0.03, mode="cold")
    want = (s.device_params(), *s.device_trajectory())
    s.upload_reference_ground(case["x0"], N, dt, t, *args, np.full(B, 0.03), mode="cold")
    got = (s.device_params(), *s.device_trajectory())
    for a, b in zip(got, want):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    s.iterate(1, take_step=True, linesearch=True)                                                              # and the shifted warm start
    s.upload_reference_ground(case["x0"], N, dt, t + PERIOD, *args, np.full(B, 0.03), mode="shift")
    got = (s.device_params(), *s.device_trajectory())
    s.upload_reference_warm(case["x0"], N, dt, t, *args, terrain_height=0.03, mode="cold")
    s.iterate(1, take_step=True, linesearch=True)
    s.upload_reference_warm(case["x0"], N, dt, t + PERIOD, *args, terrain_height=0.03, mode="shift")
    for a, b in zip(got, (s.device_params(), *s.device_trajectory())):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    heights = np.linspace(-0.05, 0.17, B)
    s.upload_reference_ground(case["x0"], N, dt, t, *args, heights, mode="cold")
    table = s.device_params()
    swing = table[:, :, _abi.P_SWING:_abi.P_SWING + 6]
    assert not np.array_equal(swing[0], swing[1])
    for b in range(B):
        one = slice(b, b + 1)
        s.upload_reference_warm(case["x0"][one], N, dt, t, r["ne"][one], r["ev"][one], r["seq"][one], r["tt"][one], r["ts"][one], sw, terrain_height=float(heights[b]),
                                mode="cold")
        assert np.array_equal(s.device_params()[0].view(np.uint64), table[b].view(np.uint64)), b


# ---------------------------------------------------------------------------------------------- 4. the loop against the calls it replaces
def by_hand(s, model, case, cycles, integrator="ode45", controller="feedforward", gait=None, delays=None, ground_alpha=0.0, g_init=None):
    """The cycles through the public calls: (hsqp_observe_eval,) hsqp_command_targets, (hsqp_gait_update,) hsqp_ground_estimate, the three adds on the host,
    hsqp_upload_reference_ground, hsqp_iterate_device, hsqp_rollout_policy."""
    dt, sw = model.sqp["dt"], swing_config(model)
    x, cmd = case["x0"].copy(), case["cmd"].copy()
    rows = len(x)
    vf, t = cmd.copy(), 0.0
    k = delays[1] if delays else 0
    ring = O.Ring(rows, sum(delays)) if delays else None
    g = np.zeros(rows) if g_init is None else np.array(g_init, dtype=float)
    ne, ev, seq = case["ne"], case["ev"], case["seq"]
    if gait is not None:
        s.gait_reset(gait, rows, O.problem_time(t, k, PERIOD) if delays else t)
    xs, us, gs, fzs = [], [], [], []
    for c in range(cycles):
        y = s.observe(ring.cycle(c, x, np.full(rows, c == 0)), c) if delays else x
        tp = O.problem_time(t, k, PERIOD) if delays else t
        tt, ts, vf = s.command_targets(cmd, y, tp, N * dt, filter_alpha=ALPHA, v_filt=vf)
        if gait is not None:
            ne, ev, seq = s.gait_update(tp, N * dt, vf, y)
        g, fz = s.ground_estimate(y, tp, ne, ev, seq, g, ground_alpha)
        ts = G.shift_knots(ts, g)
        s.upload_reference_ground(y, N, dt, tp, ne, ev, seq, tt, ts, sw, g, mode="cold" if c == 0 else "shift")
        s.iterate(1, take_step=True, linesearch=True)
        r = s.rollout_policy(np.full(rows, O.policy_time(k, PERIOD) if delays else 0.0), x, PERIOD, 1, integrator=integrator, controller=controller)
        x = r["x"][:, 0].copy()
        xs.append(x); us.append(r["u"][:, 0].copy()); gs.append(g.copy()); fzs.append(fz)
        t += PERIOD
    X, U = s.device_trajectory()
    return dict(x=np.array(xs), u=np.array(us), g=np.array(gs), fz=np.array(fzs), vf=vf, t=t, X=X, U=U, stamps=s.stamps(), par=s.device_params(),
                gait=s.gait_state() if gait is not None else {})


def assert_loop_equals(s, got, want):
    t, x_end, vf = s.loop_state()
    X, U = s.device_trajectory()
    g, fz = s.loop_ground_state()
    assert got["cycles_done"] == len(want["x"]) and np.isfinite(got["x"]).all() and np.isfinite(got["u"]).all()
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])
    assert np.array_equal(vf, want["vf"]) and np.array_equal(x_end, want["x"][-1]) and t == want["t"]
    assert np.array_equal(X, want["X"]) and np.array_equal(U, want["U"]) and np.array_equal(s.stamps(), want["stamps"])
    assert np.array_equal(s.device_params().view(np.uint64), want["par"].view(np.uint64))
    assert np.array_equal(g, want["g"][-1]) and np.array_equal(fz, want["fz"][-1])


@pytest.mark.parametrize("integrator,controller,ground_alpha", [("ode45", "feedforward", 0.0), ("rk4", "feedback", 0.8)])
def test_loop_equals_the_calls_it_replaces(s, model, integrator, controller, ground_alpha):
    case = loop_case(model)
    g_init = np.linspace(-0.01, 0.02, B)
    want = by_hand(s, model, case, CYCLES, integrator, controller, ground_alpha=ground_alpha, g_init=g_init)
    # the test's own preconditions: the estimates move while the feet do, and the unfiltered ones follow the instances' grounds (2 b cm)
    assert np.ptp(want["g"], axis=0).max() > 1e-5 and (ground_alpha != 0.0 or np.abs(want["g"][-1] - 0.02 * np.arange(B)).max() < 0.02)
    s.loop_start(settings(s, model, integrator, controller), 0.0, case["x0"], case["cmd"], case["ne"], case["ev"], case["seq"])
    s.loop_ground(s.ground_settings(filter_alpha=ground_alpha), g_init)
    g, fz = s.loop_ground_state()
    assert np.array_equal(g, g_init) and not fz.any()
    got = s.loop_run(CYCLES)
    assert_loop_equals(s, got, want)
    # the device getter
    bufs = [DeviceBuffer((B,)), DeviceBuffer((B, 2))]
    try:
        s.loop_ground_state_device(bufs[0].ptr.value, bufs[1].ptr.value)
        assert np.array_equal(bufs[0].numpy(), want["g"][-1]) and np.array_equal(bufs[1].numpy(), want["fz"][-1])
    finally:
        for b in bufs:
            b.free()
    # and the setting is felt: the same loop without it is another run
    s.loop_start(settings(s, model, integrator, controller), 0.0, case["x0"], case["cmd"], case["ne"], case["ev"], case["seq"])
    plain = s.loop_run(CYCLES)
    assert np.isfinite(plain["x"]).all() and not np.array_equal(plain["x"], got["x"])
    # initial_height stands in for g_init, a chain of runs is one run
    s.loop_start(settings(s, model, integrator, controller), 0.0, case["x0"], case["cmd"], case["ne"], case["ev"], case["seq"])
    s.loop_ground(s.ground_settings(filter_alpha=ground_alpha, initial_height=0.25))
    assert np.array_equal(s.loop_ground_state()[0], np.full(B, 0.25))


def test_gait_loop_equals_the_calls_it_replaces(s, model):
    case = loop_case(model)
    case["cmd"][:, 0] = np.linspace(0.0, 0.8, B)                             # the ladder's first rung is left by some instances
    gait = gait_settings(model)
    cycles = 16                                                              # (past the ladder's first transition: the schedule that feeds the estimate changes)
    want = by_hand(s, model, case, cycles, gait=gait, ground_alpha=0.5)
    assert (want["gait"]["rung"] > 0).any()
    s.loop_start(settings(s, model), 0.0, case["x0"], case["cmd"], gait=gait)
    s.loop_ground(s.ground_settings(filter_alpha=0.5))
    got = s.loop_run(cycles)
    assert_loop_equals(s, got, want)
    state = s.gait_state()
    for k in state:
        assert np.array_equal(state[k], want["gait"][k]), k


def test_observed_loop_equals_the_calls_it_replaces(s, model):
    """Sensor delay 1, compute delay 1, bias and noise: the estimate reads the observation y at the problem time, not the plant's state."""
    case = loop_case(model)
    rng = np.random.default_rng(5)
    bias, sigma = 0.01 * rng.standard_normal((B, NX)), np.abs(5e-3 * rng.standard_normal((B, NX)))
    bias[:, 2] = -0.02
    s.set_observation(sensor_delay=1, compute_delay=1, seed=2026)
    s.set_observation_instances(bias, sigma)
    want = by_hand(s, model, case, CYCLES, delays=(1, 1))
    s.loop_start(settings(s, model), 0.0, case["x0"], case["cmd"], case["ne"], case["ev"], case["seq"])
    s.loop_ground()
    got = s.loop_run(CYCLES)
    assert_loop_equals(s, got, want)
    y, tp = s.last_observation()
    assert np.array_equal(s.loop_ground_state()[1], s.ground_estimate(y, tp, case["ne"], case["ev"], case["seq"])[1])   # the heights are those of y
    assert np.abs(want["g"][-1] - (0.02 * np.arange(B) - 0.02)).max() < 0.03                                          # the height bias is in the estimate


def test_isolated_loop_restarts_a_failed_latch_and_the_others_go_on(s, model):
    """Instance 1 starts from a NaN state: its cycle 0 fails (its estimate is NaN with it), it is parked at x_reset, and in cycle 1 — the cycle it takes
    HSQP_WARM_COLD in — its latch starts from its g_init, not from the NaN.  The others are the run without a sick instance, bit for bit."""
    case = loop_case(model)
    g_init, ga = np.linspace(0.3, 0.4, B), 0.8
    runs = []
    for sick in (False, True):
        x0 = case["x0"].copy()
        if sick:
            x0[1, 7] = np.nan
        s.loop_start(settings(s, model), 0.0, x0, case["cmd"], case["ne"], case["ev"], case["seq"])
        s.loop_isolate(s.episode_settings("park"), x_reset=case["x0"])
        s.loop_ground(s.ground_settings(filter_alpha=ga), g_init)
        first = s.loop_run(1)
        g1 = s.loop_ground_state()[0]
        second = s.loop_run(1)
        g2, fz2 = s.loop_ground_state()
        rest = s.loop_run(CYCLES - 2)
        runs.append(dict(x=np.concatenate([first["x"], second["x"], rest["x"]]), u=np.concatenate([first["u"], second["u"], rest["u"]]), g1=g1, g2=g2, fz2=fz2,
                         g=s.loop_ground_state()[0], state=s.loop_state(), ep=s.loop_episodes()))
    a, b = runs
    rows = [0] + list(range(2, B))
    assert (a["ep"]["state"] == _abi.EP_ALIVE).all() and b["ep"]["state"][1] != _abi.EP_ALIVE and (b["ep"]["state"][rows] == _abi.EP_ALIVE).all()
    assert np.isfinite(a["x"]).all() and np.isnan(b["x"][:, 1]).all()
    for k in ("x", "u"):
        assert np.array_equal(a[k][:, rows], b[k][:, rows]), k
    for k in ("g1", "g2", "g"):
        assert np.array_equal(a[k][rows], b[k][rows]), k
    assert np.array_equal(a["state"][1][rows], b["state"][1][rows]) and np.array_equal(a["state"][2][rows], b["state"][2][rows])
    assert np.isnan(b["g1"][1])                                              # the failing cycle's estimate
    one = slice(1, 2)                                                        # cycle 1: from g_init, on the parked instance's state x_reset, at t = PERIOD
    want, fz = s.ground_estimate(case["x0"][one], PERIOD, case["ne"][one], case["ev"][one], case["seq"][one], g_init[one], ga)
    assert b["g2"][1] == want[0] and np.array_equal(b["fz2"][1], fz[0]) and np.isfinite(b["g"][1])
    assert a["g2"][1] != b["g2"][1]                                          # (the healthy run's latch had moved on from its first estimate)


# ---------------------------------------------------------------------------------------------- 5. lift invariance
def lift_case(model, batch=B):
    """Flow plant; instances 0 .. 3 stand (stance schedules), 4 .. 7 walk (the walk starts at 0.015 s .. 0.06 s: every one lifts a foot inside the
    five cycles); one command for all but the forward velocity, spread over 0 .. 0.4 m/s on the walkers."""
    rng = np.random.default_rng(20261020)
    schedules = [tile_gait(model.gaits["stance"], -0.1, 3.0) for _ in range(batch // 2)] + \
                [tile_gait(model.gaits["walk"], 0.015 * (b + 1), 3.0) for b in range(batch - batch // 2)]
    dummy = velocity_command_targets(model, (0.0, 0.0, 0.79, 0.0), 0.0, model.initial_state, 1.0)
    ne, ev, seq = pack_reference(schedules, [dummy] * batch)[:3]
    x0 = np.tile(model.initial_state, (batch, 1))
    x0[:, 6:6 + NJ] += 0.01 * rng.standard_normal((batch, NJ))
    cmd = np.tile([0.0, 0.0, 0.7925, 0.0], (batch, 1))
    cmd[batch // 2:, 0] = np.linspace(0.0, 0.4, batch - batch // 2)
    return dict(ne=ne, ev=ev, seq=seq, x0=x0, cmd=cmd)


def test_lift_invariance(s, model):
    """Run A from x0, run B from x0 raised by 0.125 m, the same command, the setting on in both: B's logged states are A's plus 0.125 in entry 2 and
    nothing else, and g_B - g_A = 0.125 in every cycle.

    The bound: the parent commit lifted by hand (terrain_height = 0.125, command height + 0.125, x0 raised, the setting absent) against its own base
    run over the same five cycles of lift_case() differs from the exact lift by LIFT_PARENT (profiles/ground_loop.txt); this test allows ten times it.

    Measured on one MI355X (profiles/ground_loop.txt).  Parent by hand: max |x_B - x_A - lift| 1.051, 2.446, 5.505, 7.998, 9.037 after cycles 1 .. 5
    (the velocity entries), 3.040e-2 in entry 2 alone.  This commit with the setting on: 10.49 over the five cycles, 3.041e-2 in entry 2 alone,
    max |g_B - g_A - lift| 2.133e-2.  Neither is rounding: the whole-body problem is not invariant under a lift, with or without this feature.  The
    stance-foot equality of the reference (EndEffectorDynamicsAccelerationsConstraint, positionErrorGain_z = 100 on the foot's ABSOLUTE height p_z,
    restated in csrc/hsqp_node.h / hsqp_lql.h / hsqp_lqv.h and in the CPU oracle) pulls a foot in contact towards z = 0 whatever the terrain height
    says, which reaches only the swing references and the target knots; on the flow plant, which has no ground, the lifted robot's feet and base
    sink by 3 cm in five cycles, in the parent's hand-lifted run and in this one alike (the entry-2 figures agree to four digits).  So the bound
    the rule above yields is wide, and this test holds the feature to the parent's own behaviour under a lift, no more; what the feature adds is
    pinned exactly by the loop-against-calls tests and by the knots of test_without_the_setting_the_lift_is_not_followed."""
    case = lift_case(model)
    runs = []
    for lift in (0.0, LIFT):
        x0 = case["x0"].copy()
        x0[:, 2] += lift
        s.loop_start(settings(s, model), 0.0, x0, case["cmd"], case["ne"], case["ev"], case["seq"])
        s.loop_ground()
        xs, gs = [], []
        for _ in range(CYCLES):
            r = s.loop_run(1)
            assert r["cycles_done"] == 1
            xs.append(r["x"][0]); gs.append(s.loop_ground_state()[0])
        runs.append((np.array(xs), np.array(gs)))
    (xa, ga), (xb, gb) = runs
    assert np.isfinite(xa).all() and np.isfinite(xb).all()
    d = xb - xa
    d[:, :, 2] -= LIFT
    dg = gb - ga - LIFT
    print(f"lift invariance over {CYCLES} cycles: max |x_B - x_A - lift| {np.abs(d).max():.3e} (entry 2 alone {np.abs(d[:, :, 2]).max():.3e}), "
          f"max |g_B - g_A - lift| {np.abs(dg).max():.3e}; parent by hand {LIFT_PARENT:.3e}, allowed {10 * LIFT_PARENT:.3e}")
    assert np.abs(ga).max() < 0.02 and np.abs(xb[:, :, 2] - xa[:, :, 2]).min() > 0.05
    assert np.abs(d).max() <= 10 * LIFT_PARENT
    assert np.abs(dg).max() <= 10 * LIFT_PARENT


def test_without_the_setting_the_lift_is_not_followed(s, model):
    """The knots are exact: node 0's desired base height is the filtered command's height entry — plus the latch with the setting on, and an absolute
    world height without it, however far the robot has been lifted."""
    case = lift_case(model)
    x0 = case["x0"].copy()
    x0[:, 2] += LIFT
    heights = {}
    for on in (False, True):
        s.loop_start(settings(s, model), 0.0, x0, case["cmd"], case["ne"], case["ev"], case["seq"])
        if on:
            s.loop_ground()
        assert s.loop_run(CYCLES)["cycles_done"] == CYCLES
        vf = s.loop_state()[2]
        par = s.device_params()
        heights[on] = par[:, 0, _abi.P_XDES + 2]                                # node 0 is knot 0 itself: no interpolation
        if on:
            g = s.loop_ground_state()[0]
            assert np.array_equal(heights[on], vf[:, 2] + g) and np.abs(g - LIFT).max() < 0.02
            flags = par[:, 0, _abi.P_CONTACT:_abi.P_CONTACT + 2] == 1.0
            z_ref = par[:, 0, [_abi.P_SWING, _abi.P_SWING + 3]]
            assert flags.any() and np.array_equal(z_ref[flags], np.repeat(g[:, None], 2, axis=1)[flags])                    # the stance feet's z reference
        else:
            assert np.array_equal(heights[on], vf[:, 2])                                                                     # still the absolute command
            assert np.abs(heights[on] - 0.7925).max() < 1e-12
    assert (heights[True] - heights[False]).min() > 0.1


# ---------------------------------------------------------------------------------------------- 6. the box above the ground
def test_box_above_ground(s, model):
    case = lift_case(model)
    x0 = case["x0"].copy()
    x0[:, 2] += 0.5
    for flag, want in ((False, _abi.EP_FAILED_BOUNDS), (True, _abi.EP_ALIVE)):
        s.loop_start(settings(s, model), 0.0, x0, case["cmd"], case["ne"], case["ev"], case["seq"])
        s.loop_isolate(s.episode_settings("park", min_base_height=0.6, max_base_height=1.0), x_reset=x0)
        s.loop_ground(s.ground_settings(box_above_ground=flag), np.full(B, 0.5))
        assert s.loop_run(CYCLES)["cycles_done"] == CYCLES
        ep = s.loop_episodes()
        assert (ep["state"] == want).all(), (flag, ep)
        if not flag:
            assert (ep["cause"] == _abi.EP_FAILED_BOUNDS).all() and (ep["n_failures"] >= 1).all()
        else:
            assert np.abs(s.loop_ground_state()[0] - 0.5).max() < 0.1 and (s.loop_state()[1][:, 2] > 1.0).all()   # (the flow plant has no ground: the feet sink)


# ---------------------------------------------------------------------------------------------- 7. refusals and lifetime
def test_refusals_and_lifetime(s, model, cmodel):
    lib = s.lib
    case = loop_case(model)
    ne, ev, seq, x = case["ne"], case["ev"], case["seq"], case["x0"]
    E = ev.shape[1]
    g, fz = np.zeros(B), np.zeros((B, 2))
    P, I = lambda a: a.ctypes.data_as(_dp), lambda a: a.ctypes.data_as(_ip)  # noqa: E731

    def refused(h, what, name, *args):
        rc = getattr(lib, name)(h.h, *args)
        msg = lib.hsqp_last_error(h.h).decode()
        assert rc == _abi.ERR_BAD_ARG and name in msg and what in msg, (name, what, rc, msg)

    def call(name="hsqp_ground_estimate", batch=B, t=0.1, max_events=E, alpha=0.0, arrays=None):
        a = [P(x), I(ne), P(ev), I(seq), P(g), P(fz)] if arrays is None else arrays
        return (name, batch, t, a[0], max_events, a[1], a[2], a[3], alpha, a[4], a[5])

    for name in ("hsqp_ground_estimate", "hsqp_ground_estimate_device"):
        refused(s, "batch", *call(name, batch=0))
        refused(s, "batch", *call(name, batch=B + 1))
        refused(s, "filter_alpha", *call(name, alpha=1.0))
        refused(s, "filter_alpha", *call(name, alpha=-0.1))
        refused(s, "filter_alpha", *call(name, alpha=float("nan")))
        refused(s, "t not finite", *call(name, t=float("inf")))
        refused(s, "max_events", *call(name, max_events=0))
        for k in range(5):                                                   # foot_z may be NULL, nothing else
            arrays = [P(x), I(ne), P(ev), I(seq), P(g), P(fz)]
            arrays[k] = None
            refused(s, "null array", *call(name, arrays=arrays))
    bad = ne.copy()
    bad[2] = E + 1
    refused(s, "n_events", *call(arrays=[P(x), I(bad), P(ev), I(seq), P(g), P(fz)]))
    bad[2] = 0
    refused(s, "n_events", *call(arrays=[P(x), I(bad), P(ev), I(seq), P(g), P(fz)]))
    bad_g = g.copy()
    bad_g[3] = np.inf
    refused(s, "non-finite g", *call(arrays=[P(x), I(ne), P(ev), I(seq), P(bad_g), P(fz)]))
    assert getattr(lib, "hsqp_ground_estimate")(s.h, *call(arrays=[P(x), I(ne), P(ev), I(seq), P(g), None])[1:]) == 0   # foot_z NULL
    # the upload
    dt, sw = model.sqp["dt"], swing_config(model)
    r = reference_args(model, case, 0.0)
    with pytest.raises(HsqpError) as ei:
        s.upload_reference_ground(x, N, dt, 0.0, r["ne"], r["ev"], r["seq"], r["tt"], r["ts"], sw, np.array([0.0] * (B - 1) + [np.nan]))
    assert ei.value.code == _abi.ERR_BAD_ARG and "hsqp_upload_reference_ground" in str(ei.value) and "terrain_heights" in str(ei.value)
    refused(s, "null", "hsqp_upload_reference_ground", None, None, P(g))
    # the loop entry points without a loop
    ok = s.ground_settings()
    refused(s, "no loop started", "hsqp_loop_ground", C.byref(ok), None)
    refused(s, "no loop started", "hsqp_loop_ground_state", P(g), P(fz))
    refused(s, "no loop started", "hsqp_loop_ground_state_device", None, None)
    # a centroidal handle
    c = HipSqpSolver(cmodel, max_nodes=N, max_batch=B)
    try:
        refused(c, "whole-body handles only", *call("hsqp_ground_estimate"))
        refused(c, "whole-body handles only", *call("hsqp_ground_estimate_device"))
        refused(c, "whole-body handles only", "hsqp_upload_reference_ground", None, None, P(g))
        refused(c, "whole-body handles only", "hsqp_loop_ground", C.byref(ok), None)
        refused(c, "whole-body handles only", "hsqp_loop_ground_state", P(g), P(fz))
        refused(c, "whole-body handles only", "hsqp_loop_ground_state_device", None, None)
    finally:
        c.close()
    # a started loop
    start = lambda: s.loop_start(settings(s, model), 0.0, case["x0"], case["cmd"], case["ne"], case["ev"], case["seq"])  # noqa: E731
    start()
    refused(s, "is off", "hsqp_loop_ground_state", P(g), P(fz))
    s.loop_ground(s.ground_settings(filter_alpha=0.5), np.full(B, 0.1))
    assert s.loop_run(2)["cycles_done"] == 2
    before = s.loop_ground_state()
    refused(s, "filter_alpha", "hsqp_loop_ground", C.byref(s.ground_settings(filter_alpha=1.0)), None)
    refused(s, "initial_height", "hsqp_loop_ground", C.byref(s.ground_settings(initial_height=float("nan"))), None)
    refused(s, "0 or 1", "hsqp_loop_ground", C.byref(_abi.GroundSettings(enabled=2)), None)
    refused(s, "0 or 1", "hsqp_loop_ground", C.byref(_abi.GroundSettings(enabled=1, box_above_ground=-1)), None)
    refused(s, "non-finite g_init", "hsqp_loop_ground", C.byref(ok), P(bad_g))
    after = s.loop_ground_state()                                            # a refused call leaves the previous setting, and the latches, in place
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    on = s.loop_run(1)
    # off again: NULL settings, enabled 0, and every start
    for off in (lambda: s.loop_ground(on=False), lambda: s.loop_ground(s.ground_settings(enabled=False))):
        start()
        s.loop_ground()
        off()
        refused(s, "is off", "hsqp_loop_ground_state", P(g), P(fz))
    start()
    plain = s.loop_run(3)
    refused(s, "is off", "hsqp_loop_ground_state", P(g), P(fz))
    start()
    s.loop_ground()
    assert s.loop_run(1)["cycles_done"] == 1
    start()                                                                  # hsqp_loop_start switches the setting off again
    refused(s, "is off", "hsqp_loop_ground_state", P(g), P(fz))
    again = s.loop_run(3)
    assert np.array_equal(plain["x"], again["x"]) and np.array_equal(plain["u"], again["u"]) and np.isfinite(on["x"]).all()
    assert np.array_equal(s.device_params()[:, 0, _abi.P_XDES + 2], s.loop_state()[2][:, 2])
    s.upload_reference_warm(x, N, dt, 0.0, r["ne"], r["ev"], r["seq"], r["tt"], r["ts"], sw, mode="cold")          # an upload ends the loop
    refused(s, "no loop started", "hsqp_loop_ground", C.byref(ok), None)
