"""The actuator model on the torque plant (include/hsqp_actuator.h) on the MI355X: RK4 against the numpy restatement (tests/actuator_ref.py on
tests/plant_ref.py / tests/contact_ref.py), ODE45 against a tight RK4 solution of that reference, the record of the last torques, the inert settings
bit for bit, chaining, batch independence, the resident loop, the iteration untouched, and the argument errors.  The small handles of
tests/test_gpu_plant.py: 8 nodes, 3 instances (no push, an elbow push, two overlapping pushes), its gains kp 100, kd 2, armature 0.01."""
import ctypes as C
import json
import os
import signal

import numpy as np
import pytest

import actuator_ref as A
import contact_ref as CR
import plant_ref as PL
import rollout_ref as R
from test_contact import RK4_STEP
from test_gpu_contact import X_TOL as X_TOL_GROUND, grounds
from test_gpu_feedback_policy import DeviceBuffer
from test_gpu_loop import loop_case
from test_gpu_plant import GAINS, U_TOL, plant_pushes
from test_gpu_push import B, D, H, KEYS, N, S0, by_hand, loop_start, problem, same, solved, start
from test_gpu_rollout import policies
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu
NX, NU, NV, NJ = _abi.NX, _abi.NU, _abi.NV, _abi.NJ
# x against the reference: ten times the host emulation's error against the same reference (tests/test_actuator.py::test_rk4_rollout_matches_numpy
# prints at most 2.91e-11 over its twelve cases), not below 1e-10
X_TOL = 2.91e-10
# the record: tau_cmd is linear in x with the gains kp + kd = 102: the x bound times that, relative to max(1, |tau|)
REC_TOL = X_TOL * (GAINS["kp"] + GAINS["kd"])
LIMITED = dict(effort_limit=5.0, damping=0.05, friction=0.1)
HOLDS = {"off": 0.0, "2^-8": 2.0 ** -8, "0.003": 0.003}
S0_BINARY = np.array([0.0, 2.0 ** -5, 2.0 ** -4])


@pytest.fixture(autouse=True)
def time_limit():
    def expired(signum, frame):
        raise TimeoutError("test_gpu_actuator: a test ran past its 120 s limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def golden_limits(model):
    """The reference's actuatorfrcrange of the model's 23 joints (tests/golden/g1_effort_limits.json, through model.joint_names)."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g1_effort_limits.json")) as f:
        table = json.load(f)
    return np.array([table[n] for n in model.joint_names])


def closed_loops(model, oracle, s, out, dts, dt, grid, controller, pl, ac, cts=None):
    pols = policies(s, out, dts, dt, grid, False)
    ctl = R.FEEDBACK if controller == "feedback" else R.FEEDFORWARD
    return pols, [A.ClosedLoop(oracle, model, pols[b], out["x"][b], pl, ctl, ac, None if cts is None else cts[b]) for b in range(len(pols))]


def rk4_case(hold, grid):
    """(s0, step): hold 2^-8 from binary start times with the step 2^-8 — the ticks are step boundaries and the first sample a tick."""
    return (S0_BINARY, 2.0 ** -8) if hold == "2^-8" else (S0[grid], H)


def check_against_reference(model, oracle, s, out, dts, dt, x0, grid, controller, hold, x_tol, ground=False, step=None):
    s0, h = rk4_case(hold, grid)
    h = h if step is None else step
    xs = start(x0, False)
    pushes = plant_pushes(s0)
    ac = A.actuator(HOLDS[hold], **LIMITED)
    s.set_plant(**GAINS)
    s.set_pushes(pushes)
    s.set_actuator(command_period=HOLDS[hold], **LIMITED)
    cts = None
    if ground:
        g = grounds(oracle, model, xs)
        s.set_contact()
        s.set_contact_instances(g)
        cts = [CR.with_ground(CR.contact(model), g[b]) for b in range(B)]
    r = s.rollout_policy(s0, xs, D, 2, integrator="rk4", controller=controller, initial_step=h)
    cmd, act, pas = s.actuator_torques()
    assert (r["status"] == 0).all() and (r["rejected"] == 0).all()
    pl = PL.plant(**GAINS)
    pols, cls = closed_loops(model, oracle, s, out, dts, dt, grid, controller, pl, ac, cts)
    st = R.settings(R.RK4, R.FEEDBACK if controller == "feedback" else R.FEEDFORWARD, initial_step=h)
    refs = [A.rollout(cls[b], pols[b], st, s0[b], xs[b], D, 2, pushes[b]) for b in range(B)]
    # the reference first: some joint of some instance is saturated at the end (standing knees carry well above 5 N m)
    assert all(ref[2] == R.OK for ref in refs)
    assert any((np.abs(ref[5][0]) > ac["effort_limit"]).any() for ref in refs)
    for b, (xr, ur, sr, nr, _, rec) in enumerate(refs):
        assert r["steps"][b] == nr, (b, r["steps"][b], nr)
        err = np.abs(r["x"][b] - xr).max() / max(1.0, np.abs(xr).max())
        erru = np.abs(r["u"][b] - ur).max() / max(1.0, np.abs(ur).max())
        got = np.array([cmd[b], act[b], pas[b]])
        errr = np.abs(got - rec).max() / max(1.0, np.abs(rec).max())
        print(f"{grid} {controller} hold {hold} instance {b}: steps {nr}, x error {err:.2e}, u error {erru:.2e}, record error {errr:.2e}, "
              f"saturated joints {int((np.abs(rec[0]) > ac['effort_limit']).sum())}")
        assert err <= x_tol, (b, err)
        assert erru <= U_TOL, (b, erru)
        assert errr <= max(REC_TOL, x_tol * (GAINS["kp"] + GAINS["kd"])), (b, errr)
    assert (np.abs(act) <= ac["effort_limit"]).all()
    return r


# ---------------------------------------------------------------------------------------------- 1, 4. RK4 and the record against actuator_ref
@pytest.mark.parametrize("hold", list(HOLDS))
@pytest.mark.parametrize("grid,controller", [("uniform", "feedforward"), ("events", "feedback")])
def test_rk4_and_the_record_match_the_reference(model, oracle, grid, controller, hold):
    s, out, dts, dt, x0 = solved(model, False, grid)
    try:
        check_against_reference(model, oracle, s, out, dts, dt, x0, grid, controller, hold, X_TOL)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 2. the same on the ground
def test_rk4_on_the_ground_matches_the_reference(model, oracle):
    """The instantiation with the ground and the actuator model, against contact_ref + actuator_ref; the bound and the step of
    tests/test_gpu_contact.py::test_rk4_matches_the_reference (the reference's contact force carries a central-difference Jacobian)."""
    s, out, dts, dt, x0 = solved(model, False, "events")
    try:
        check_against_reference(model, oracle, s, out, dts, dt, x0, "events", "feedback", "0.003", X_TOL_GROUND, ground=True, step=RK4_STEP)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 3. ODE45 against a tight solution
def test_ode45_against_a_tight_solution(model, oracle):
    """Shaped like tests/test_gpu_plant.py::test_ode45_against_a_tight_solution, with its tolerance rule; hold 0.002, the limits of the reference's
    model file, damping 0.05, friction 0.1; the tight solution is RK4 at 2^-15 s on actuator_ref for instance 1.  A policy kink (a node stamp,
    with or without the lookahead, inside the window) or a change of the saturated set (detected at every step of the tight solution) widens the
    ratio's bound from 10 to 50.  Measured on the MI355X: 10 accepted + 3 rejected steps for the checked instance (9 + 1 and 8 + 0 for its
    neighbours: at least one step per hold interval, eight of them), error / tolerance 0.79, tight error 8.1e-8 (133 + 55 steps); no policy kink
    and no change of the saturated set inside the window, so the bound is 10."""
    s, out, dts, dt, x0 = solved(model, False, "uniform")
    try:
        s0 = S0["uniform"]
        xs = start(x0, False, 1)
        T = 2.0 ** -6
        lim = golden_limits(model)
        pl = PL.plant(**GAINS)
        ac = A.actuator(0.002, lim, 0.05, 0.1)
        pols, cls = closed_loops(model, oracle, s, out, dts, dt, "uniform", "feedforward", pl, ac)
        b = 1
        ref, sat = A.tight_solution(cls[b], pols[b], s0[b], xs[b], T)
        assert np.isfinite(ref).all()
        s.set_plant(**GAINS)
        s.set_actuator(command_period=0.002, effort_limit=lim, damping=0.05, friction=0.1)
        r = s.rollout_policy(s0, xs, T, 1)
        assert (r["status"] == 0).all() and (r["steps"] < 10000).all()
        assert (r["steps"] >= 8).all()                                      # a restart at every tick: 8 intervals in 2^-6 s
        r2 = s.rollout_policy(s0, xs, T, 1, abs_tol=1e-10, rel_tol=1e-10)
        assert (r2["status"] == 0).all() and (r2["steps"] > r["steps"]).all() and (r2["steps"] < 10000).all()
        err = float(np.abs(r2["x"][b, 0] - ref).max())
        ratio = float((np.abs(r["x"][b, 0] - ref) / (1e-5 + 1e-3 * np.abs(ref))).max())
        stamps = np.arange(N + 1) * dt
        kink = any(((stamps - la > s0[b]) & (stamps - la < s0[b] + T)).any() for la in (0.0, pl["lookahead"]))
        switched = len(set(sat)) > 1
        print(f"hold 0.002 T {T}: steps {r['steps']} rejected {r['rejected']} error / tolerance {ratio:.2f}; tight steps {r2['steps']} rejected "
              f"{r2['rejected']} tight error {err:.2e}; policy kink {kink}, saturated set changes {switched}")
        assert ratio <= (50.0 if kink or switched else 10.0), (kink, switched, ratio)
        assert err <= 1e-7, err
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 4. the record: the clamp, and NaN rows
def test_the_record_is_clamped_and_nan_for_an_instance_that_hit_the_step_cap(model):
    s, _, _, _, x0 = solved(model, False, "uniform")
    try:
        s0 = S0["uniform"]
        xs = start(x0, False, 3)
        s.set_plant(**GAINS)
        with pytest.raises(HsqpError) as ei:
            s.actuator_torques()
        assert ei.value.code == _abi.ERR_BAD_ARG and "hsqp_actuator_last" in str(ei.value) and "no rollout" in str(ei.value)
        s.set_actuator(command_period=0.002, **LIMITED)
        with pytest.raises(HsqpError) as ei:
            s.actuator_torques()
        assert "no rollout" in str(ei.value)
        s.rollout_policy(s0, xs, D, 2)
        cmd, act, pas = s.actuator_torques()
        assert np.isfinite(cmd).all() and (np.abs(act) <= 5.0).all() and (np.abs(cmd) > 5.0).any()
        over = np.abs(cmd) > 5.0
        assert np.array_equal(act[~over], cmd[~over]) and np.array_equal(np.abs(act[over]), np.full(int(over.sum()), 5.0))
        # the device entry point: the same rows into device memory, and any of them may be NULL
        bufs = [DeviceBuffer((B, NJ)) for _ in range(3)]
        try:
            cast = lambda d: C.cast(d.ptr, C.POINTER(C.c_double))   # noqa: E731
            s._check(s.lib.hsqp_actuator_last_device(s.h, B, cast(bufs[0]), cast(bufs[1]), cast(bufs[2])))
            assert all(np.array_equal(d.numpy(), w) for d, w in zip(bufs, (cmd, act, pas)))
            bufs[1].upload(np.zeros((B, NJ)))
            s._check(s.lib.hsqp_actuator_last_device(s.h, B, None, cast(bufs[1]), None))
            assert np.array_equal(bufs[1].numpy(), act)
        finally:
            for d in bufs:
                d.free()
        with pytest.raises(HsqpError) as ei:
            s.actuator_torques(B - 1)
        assert ei.value.code == _abi.ERR_BAD_ARG and "hsqp_actuator_last" in str(ei.value) and "batch" in str(ei.value)
        # one step per second: 8 tick intervals cannot be done — every instance ends at the cap, and its rows are NaN
        with pytest.raises(HsqpError) as ei:
            s.rollout_policy(s0, xs, D, 2, max_steps_per_second=1.0)
        assert (ei.value.result["status"] == _abi.ROLLOUT_MAX_STEPS).all()
        cmd, act, pas = s.actuator_torques()
        assert np.isnan(cmd).all() and np.isnan(act).all() and np.isnan(pas).all()
        # a new setting forgets the record
        s.set_actuator(command_period=0.002, **LIMITED)
        with pytest.raises(HsqpError):
            s.actuator_torques()
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 5. the inert settings, bit for bit
def test_inert_settings_equal_a_fresh_handle(model):
    s, _, _, _, x0 = solved(model, False, "events")
    fresh, _, _, _, _ = solved(model, False, "events")
    try:
        s0 = S0["events"]
        xs = start(x0, False, 2)
        pushes = plant_pushes(s0)
        for h in (s, fresh):
            h.set_pushes(pushes)
        for controller in ("feedforward", "feedback"):
            for integrator in ("ode45", "rk4"):
                kw = dict(integrator=integrator, controller=controller, initial_step=H if integrator == "rk4" else 0.015)
                fresh.clear_plant()
                flow = fresh.rollout_policy(s0, xs, D, 2, **kw)
                fresh.set_plant(**GAINS)
                want = fresh.rollout_policy(s0, xs, D, 2, **kw)
                s.set_plant(**GAINS)
                s.clear_actuator()
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "unset"
                for ac in (dict(command_period=0.002), dict(command_period=0.0, effort_limit=5.0), dict(command_period=0.0, damping=0.05),
                           dict(command_period=0.0, friction=0.1), dict(command_period=0.003, **LIMITED)):
                    s.set_actuator(**ac)
                    assert not same(s.rollout_policy(s0, xs, D, 2, **kw), want), ac
                s.set_actuator(enabled=False, command_period=0.003, **LIMITED)
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "enabled = 0"
                s.set_actuator(command_period=0.0)
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "neutral"
                cmd, act, pas = s.actuator_torques()
                assert np.array_equal(cmd, act) and (pas == 0.0).all()
                s.set_actuator(command_period=0.003, **LIMITED)
                s.clear_actuator()
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "cleared"
                s.set_actuator(command_period=0.003, **LIMITED)
                s.set_plant(kind="flow", **GAINS)
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), flow), "kind flow"
                s.clear_plant()
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), flow), "no plant"
                assert s.get_actuator()["command_period"] == 0.003                  # ... and the plant calls left the setting alone
    finally:
        s.close()
        fresh.close()


# ---------------------------------------------------------------------------------------------- 6. chained calls
def test_chained_calls_equal_one_call_when_the_split_is_on_a_tick(model):
    s, _, _, _, x0 = solved(model, False, "events")
    try:
        s0 = S0_BINARY
        d = 2.0 ** -7
        xs = start(x0, False, 2)
        s.set_plant(**GAINS)
        s.set_pushes(plant_pushes(s0))
        s.set_actuator(command_period=2.0 ** -9, **LIMITED)
        for controller in ("feedforward", "feedback"):
            for integrator in ("ode45", "rk4"):
                kw = dict(integrator=integrator, controller=controller, initial_step=0.003 if integrator == "rk4" else 0.015)
                r = s.rollout_policy(s0, xs, 2 * d, 2, **kw)
                assert (r["status"] == 0).all()
                last = s.actuator_torques()
                a = s.rollout_policy(s0, xs, d, 1, **kw)
                b = s.rollout_policy(s0 + d, a["x"][:, 0].copy(), d, 1, **kw)
                assert np.array_equal(a["x"][:, 0], r["x"][:, 0]) and np.array_equal(a["u"][:, 0], r["u"][:, 0]), (controller, integrator)
                assert np.array_equal(b["x"][:, 0], r["x"][:, 1]) and np.array_equal(b["u"][:, 0], r["u"][:, 1]), (controller, integrator)
                assert np.array_equal(a["steps"] + b["steps"], r["steps"])
                assert all(np.array_equal(g, w) for g, w in zip(s.actuator_torques(), last))
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 7. batch independence
def test_every_instance_equals_its_solo_rollout(model):
    s, _, _, _, x0 = solved(model, False, "events")
    try:
        s0 = S0["events"]
        xs = start(x0, False, 4)
        pushes = plant_pushes(s0)
        s.set_plant(**GAINS)
        s.set_pushes(pushes)
        s.set_actuator(command_period=0.003, **LIMITED)
        rs, ts = {}, {}
        for c in ("feedforward", "feedback"):
            rs[c] = s.rollout_policy(s0, xs, D, 2, controller=c)
            ts[c] = s.actuator_torques()
    finally:
        s.close()
    for b in range(B):
        solo, _, _, _, _ = solved(model, False, "events", rows=slice(b, b + 1))
        try:
            solo.set_plant(**GAINS)
            solo.set_pushes(pushes[b:b + 1])
            solo.set_actuator(command_period=0.003, **LIMITED)
            for c, r in rs.items():
                r1 = solo.rollout_policy(s0[b:b + 1], xs[b:b + 1], D, 2, controller=c)
                for k in KEYS:
                    assert np.array_equal(r1[k], r[k][b:b + 1]), (b, c, k)
                assert all(np.array_equal(g, w[b:b + 1]) for g, w in zip(solo.actuator_torques(), ts[c])), (b, c)
        finally:
            solo.close()


def test_sixty_four_copies_equal_the_solo_result(model):
    x0, x, u, par, dt = problem(model, False)
    one = slice(1, 2)
    big = HipSqpSolver(model, max_nodes=N, max_batch=64, riccati="serial")
    solo = HipSqpSolver(model, max_nodes=N, max_batch=64, riccati="serial")
    try:
        rep = lambda a: np.ascontiguousarray(np.repeat(a[one], 64, axis=0))   # noqa: E731
        big.run(rep(x0), rep(x), rep(u), rep(par), dt)
        solo.run(x0[one], x[one], u[one], par[one], dt)
        s0 = S0["uniform"][one]
        xs = start(x0, False, 5)[one]
        push = plant_pushes(S0["uniform"])[one]
        for h, n in ((big, 64), (solo, 1)):
            h.set_plant(**GAINS)
            h.set_pushes(push * n)
            h.set_actuator(command_period=0.002, **LIMITED)
        r1 = solo.rollout_policy(s0, xs, D, 2, controller="feedback")
        r = big.rollout_policy(np.repeat(s0, 64), np.repeat(xs, 64, axis=0), D, 2, controller="feedback")
        assert (r1["status"] == 0).all()
        for k in KEYS:
            assert np.array_equal(r[k], np.repeat(r1[k], 64, axis=0)), k
        assert all(np.array_equal(g, np.repeat(w, 64, axis=0)) for g, w in zip(big.actuator_torques(), solo.actuator_torques()))
    finally:
        big.close()
        solo.close()


# ---------------------------------------------------------------------------------------------- 8. the resident loop
def test_the_loop_runs_on_the_actuator_model_and_keeps_it(model):
    case = loop_case(model, batch=B)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        s.set_plant(**GAINS)
        loop_start(s, model, case)
        plain = s.loop_run(2)
        s.set_actuator(command_period=0.002, **LIMITED)
        want = by_hand(s, model, case, 2, "feedforward")         # the setting survives the uploads
        want_last = s.actuator_torques()
        loop_start(s, model, case)                               # ... and the start of a loop
        got = s.loop_run(2)
        got_last = s.actuator_torques()
        s.loop_isolate(s.episode_settings("reset"), x_reset=case["x0"])
        s.loop_reset([1])
        g = s.get_actuator()
        assert g["enabled"] and g["command_period"] == 0.002 and (g["effort_limit"] == 5.0).all() and (g["damping"] == 0.05).all()
        assert (g["friction"] == 0.1).all() and g["friction_velocity"] == 0.01
    finally:
        s.close()
    assert got["cycles_done"] == 2 and np.isfinite(got["x"]).all()
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])
    assert not np.array_equal(got["x"], plain["x"])
    assert np.isfinite(got_last[0]).all() and all(np.array_equal(g, w) for g, w in zip(got_last, want_last))


# ---------------------------------------------------------------------------------------------- 9. the iteration is untouched
def test_run_is_bit_identical_with_and_without_an_actuator(model):
    x0, x, u, par, dt = problem(model, False, 5)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    twin = HipSqpSolver(model, max_nodes=N, max_batch=B)
    try:
        s.set_plant(**GAINS)
        s.set_actuator(command_period=0.002, **LIMITED)
        a, b = s.run(x0, x, u, par, dt), twin.run(x0, x, u, par, dt)
        assert all(np.array_equal(a[k], b[k]) for k in ("x", "u"))
        s.rollout_policy(S0["uniform"], x0, D, 1)
        for h in (s, twin):
            h.iterate(1, take_step=True)
        a, b = s.download(), twin.download()
        assert all(np.array_equal(a[k], b[k]) for k in ("x", "u", "dx", "du"))
    finally:
        s.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 10. errors
def test_errors(model, cmodel):
    c = HipSqpSolver(cmodel, max_nodes=N, max_batch=B)
    try:
        with pytest.raises(HsqpError) as ei:
            c.set_actuator()
        assert ei.value.code == _abi.ERR_BAD_ARG and "hsqp_actuator_set" in str(ei.value) and "whole-body handles only" in str(ei.value)
    finally:
        c.close()
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)

    def refused(what, **kw):
        st = s.actuator_settings(**kw)
        rc = s.lib.hsqp_actuator_set(s.h, C.byref(st))
        msg = s.lib.hsqp_last_error(s.h).decode()
        assert rc == _abi.ERR_BAD_ARG and "hsqp_actuator_set" in msg and what in msg, (what, rc, msg)

    def unchanged(before):
        g = s.get_actuator()
        return all(np.array_equal(g[k], before[k]) for k in before)
    try:
        assert not s.get_actuator()["enabled"]
        s.set_actuator(command_period=0.004, effort_limit=7.0, damping=0.02, friction=0.03, friction_velocity=0.05)
        before = s.get_actuator()
        assert before["enabled"] and before["command_period"] == 0.004 and (before["effort_limit"] == 7.0).all()
        assert s.lib.hsqp_actuator_set(s.h, None) == _abi.ERR_BAD_ARG and "hsqp_actuator_set" in s.lib.hsqp_last_error(s.h).decode()
        assert s.lib.hsqp_actuator_get(s.h, None) == _abi.ERR_BAD_ARG and "hsqp_actuator_get" in s.lib.hsqp_last_error(s.h).decode()
        refused("reserved", reserved=1)
        refused("command_period", command_period=-1e-3)
        refused("command_period", command_period=np.inf)
        refused("command_period", command_period=np.nan)
        bad = np.full(NJ, 1.0)
        for v in (0.0, -1.0, np.nan):
            bad[7] = v
            refused("joint 7: effort_limit", effort_limit=bad)
        for v in (-1.0, np.inf, np.nan):
            bad[7] = v
            refused("joint 7: negative or non-finite damping", damping=bad)
            refused("joint 7: negative or non-finite friction", friction=bad)
        for v in (0.0, -0.01, np.inf, np.nan):
            refused("friction_velocity", friction_velocity=v)
        assert unchanged(before)                                  # no refused call replaced the setting
        lim = np.full(NJ, 5.0)
        lim[7] = np.inf
        s.set_actuator(effort_limit=lim)                          # +inf is a limit
        assert s.get_actuator()["effort_limit"][7] == np.inf
        s.clear_actuator()
        g = s.get_actuator()
        assert not g["enabled"] and g["command_period"] == 0.002 and (g["effort_limit"] == np.inf).all()
    finally:
        s.close()
