"""The torque plant of the rollout (include/hsqp_plant.h) on the MI355X: RK4 against the numpy restatement (tests/plant_ref.py) on the CPU oracle's
unchanged full_dynamics / foot_kinematics / flow_map, ODE45 against a tight RK4 solution of that reference, the flow-map paths bit for bit,
compliance, chaining, batch independence, the resident loop, the iteration untouched, and the argument errors.  Small handles: 8 nodes, 3
instances (no push, an elbow push, two overlapping pushes).  Gains of the tests: kp 100, kd 2, armature 0.01 (kd / (I + armature) <= 200 1/s)."""
import signal

import numpy as np
import pytest

import plant_ref as PL
import push_ref as P
import rollout_ref as R
from test_gpu_loop import loop_case
from test_gpu_push import B, D, H, KEYS, L_ELBOW, N, S0, by_hand, loop_start, problem, pushes_for, same, solved, start
from test_gpu_rollout import policies
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu
NX, NU, NV, NJ = _abi.NX, _abi.NU, _abi.NV, _abi.NJ
GAINS = dict(kp=100.0, kd=2.0, armature=0.01)
ARMS = slice(6 + 15, 6 + 23)     # the arm joints' positions in x (joints 15 .. 22 of the G1 tree: both arms)
# x against the reference: ten times the host emulation's error against the same reference (tests/test_plant.py::test_rk4_rollout_matches_numpy
# prints 2.7e-12 feed-forward, 8.3e-12 feedback), not below 1e-10
X_TOL = 1e-10
U_TOL = 1e-9                     # tests/test_gpu_rollout.py


@pytest.fixture(autouse=True)
def time_limit():
    def expired(signum, frame):
        raise TimeoutError("test_gpu_plant: a test ran past its 120 s limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def plant_pushes(s0):
    """pushes_for of tests/test_gpu_push.py with instance 1's push on the elbow."""
    p = pushes_for(s0)
    p[1] = [dict(p[1][0], body=L_ELBOW, point=[0.1, 0.0, 0.0])]
    return p


def closed_loops(model, oracle, s, out, dts, dt, grid, controller, pl):
    pols = policies(s, out, dts, dt, grid, False)
    ctl = R.FEEDBACK if controller == "feedback" else R.FEEDFORWARD
    return pols, [PL.closed_loop(oracle, model, pols[b], out["x"][b], pl, ctl) for b in range(len(pols))]


# ---------------------------------------------------------------------------------------------- 1. RK4 against plant_ref
@pytest.mark.parametrize("grid,controller", [("uniform", "feedforward"), ("events", "feedback"), ("uniform", "feedback")])
def test_rk4_matches_the_reference(model, oracle, grid, controller):
    s, out, dts, dt, x0 = solved(model, False, grid)
    try:
        s0 = S0[grid]
        xs = start(x0, False)
        pushes = plant_pushes(s0)
        s.set_plant(**GAINS)
        s.set_pushes(pushes)
        r = s.rollout_policy(s0, xs, D, 2, integrator="rk4", controller=controller, initial_step=H)
        assert (r["status"] == 0).all() and (r["rejected"] == 0).all()
        pl = PL.plant(**GAINS)
        pols, cls = closed_loops(model, oracle, s, out, dts, dt, grid, controller, pl)
        st = R.settings(R.RK4, R.FEEDBACK if controller == "feedback" else R.FEEDFORWARD, initial_step=H)
        for b in range(B):
            xr, ur, sr, nr, _ = PL.rollout(cls[b], pols[b], st, s0[b], xs[b], D, 2, pushes[b])
            assert sr == R.OK and r["steps"][b] == nr, (b, r["steps"][b], nr)
            err = np.abs(r["x"][b] - xr).max() / max(1.0, np.abs(xr).max())
            erru = np.abs(r["u"][b] - ur).max() / max(1.0, np.abs(ur).max())
            print(f"{grid} {controller} instance {b}: steps {nr}, x error {err:.2e}, u error {erru:.2e}")
            assert err <= X_TOL, (b, err)
            assert erru <= U_TOL, (b, erru)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 2. ODE45 against a tight solution
@pytest.mark.parametrize("gains,T", [(GAINS, 2.0 ** -6), (dict(kp=1200.0, kd=10.0, armature=0.0), 2.0 ** -8)])
def test_ode45_against_a_tight_solution(model, oracle, gains, T):
    """Shaped like tests/test_gpu_push.py::test_ode45_with_pushes_against_a_tight_solution, with its tolerance rule; the tight solution is RK4 at
    2^-15 s on plant_ref, for ONE instance (instance 1: the numpy reference costs milliseconds per evaluation).  Measured on the MI355X: test
    gains 4 accepted + 1 rejected steps, error / tolerance 0.22, tight error 3.3e-11; reference gains with no armature (rates up to 3.1e4 1/s)
    40 + 12 steps over 2^-8 s, error / tolerance 0.10, tight error 3.9e-9."""
    s, out, dts, dt, x0 = solved(model, False, "uniform")
    try:
        s0 = S0["uniform"]
        xs = start(x0, False, 1)
        pl = PL.plant(**gains)
        pols, cls = closed_loops(model, oracle, s, out, dts, dt, "uniform", "feedforward", pl)
        b = 1
        ref = PL.tight_solution(cls[b], pols[b], s0[b], xs[b], T)
        assert np.isfinite(ref).all()
        s.set_plant(**gains)
        r = s.rollout_policy(s0, xs, T, 1)
        assert (r["status"] == 0).all() and (r["steps"] < 10000).all()
        r2 = s.rollout_policy(s0, xs, T, 1, abs_tol=1e-10, rel_tol=1e-10)
        assert (r2["status"] == 0).all() and (r2["steps"] > r["steps"]).all() and (r2["steps"] < 10000).all()
        err = float(np.abs(r2["x"][b, 0] - ref).max())
        ratio = float((np.abs(r["x"][b, 0] - ref) / (1e-5 + 1e-3 * np.abs(ref))).max())
        print(f"kp {gains['kp']} armature {gains['armature']} T {T}: steps {r['steps']} rejected {r['rejected']} error / tolerance {ratio:.2f}; "
              f"tight steps {r2['steps']} rejected {r2['rejected']} tight error {err:.2e}")
        stamps = np.arange(N + 1) * dt
        kink = any(((stamps - la > s0[b]) & (stamps - la < s0[b] + T)).any() for la in (0.0, pl["lookahead"]))
        assert ratio <= (50.0 if kink else 10.0), (kink, ratio)
        assert err <= 1e-7, err
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 3. the flow-map paths, bit for bit
def test_no_plant_a_cleared_plant_and_kind_flow_equal_a_fresh_handle(model):
    s, _, _, _, x0 = solved(model, False, "events")
    fresh, _, _, _, _ = solved(model, False, "events")
    try:
        s0 = S0["events"]
        xs = start(x0, False, 2)
        for pushes in (None, pushes_for(s0)):
            for h in (s, fresh):
                h.set_pushes(pushes) if pushes else h.clear_pushes()
            for controller in ("feedforward", "feedback"):
                for integrator in ("ode45", "rk4"):
                    kw = dict(integrator=integrator, controller=controller, initial_step=H if integrator == "rk4" else 0.015)
                    want = fresh.rollout_policy(s0, xs, D, 2, **kw)
                    s.clear_plant()
                    assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "no plant"
                    s.set_plant(**GAINS)
                    assert not same(s.rollout_policy(s0, xs, D, 2, **kw), want)
                    s.set_plant(kind="flow", **GAINS)
                    assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "kind flow"
                    s.set_plant(**GAINS)
                    s.clear_plant()
                    assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "cleared plant"
    finally:
        s.close()
        fresh.close()


# ---------------------------------------------------------------------------------------------- 4. compliance
def test_an_elbow_push_moves_the_arm_on_the_torque_plant_only(model):
    """RK4 with a step of 2^-8 s from exact binary start times, the push from one step boundary to another, the feed-forward controller: the
    break points fall on step boundaries, so pushed and unpushed rollouts take the same steps and, on the flow-map plant, the same joint rows."""
    s, _, _, _, x0 = solved(model, False, "uniform")
    try:
        h = 2.0 ** -8
        s0 = np.array([0.0, 2.0 ** -5, 2.0 ** -4])
        xs = start(x0, False, 3)
        elbow = [[P.push(L_ELBOW, s0[b] + h, 2 * h, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0])] for b in range(B)]
        kw = dict(integrator="rk4", initial_step=h)
        for plant in (False, True):
            s.set_plant(**GAINS) if plant else s.clear_plant()
            s.clear_pushes()
            free = s.rollout_policy(s0, xs, D, 2, **kw)
            s.set_pushes(elbow)
            pushed = s.rollout_policy(s0, xs, D, 2, **kw)
            assert (free["status"] == 0).all() and (pushed["status"] == 0).all() and np.array_equal(free["steps"], pushed["steps"])
            d = np.abs(pushed["x"][:, -1, ARMS] - free["x"][:, -1, ARMS])
            if plant:
                assert (d.max(axis=1) > 1e-4).all(), d.max(axis=1)          # the arm gives way (host build of the kernel source: 3e-3 rad)
            else:
                # ideal acceleration sources: today's behaviour
                assert np.array_equal(pushed["x"][:, :, 6:NV], free["x"][:, :, 6:NV]) and np.array_equal(pushed["x"][:, :, NV + 6:], free["x"][:, :, NV + 6:])
                assert not np.array_equal(pushed["x"][:, :, :6], free["x"][:, :, :6])
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 5. chained calls
def test_chained_calls_equal_one_call(model):
    s, _, _, _, x0 = solved(model, False, "events")
    try:
        s0 = np.array([0.0, 2.0 ** -5, 2.0 ** -4])
        d = 2.0 ** -7
        xs = start(x0, False, 2)
        s.set_plant(**GAINS)
        s.set_pushes(plant_pushes(s0))
        for controller in ("feedforward", "feedback"):
            for integrator in ("ode45", "rk4"):
                kw = dict(integrator=integrator, controller=controller, initial_step=0.003 if integrator == "rk4" else 0.015)
                r = s.rollout_policy(s0, xs, 2 * d, 2, **kw)
                assert (r["status"] == 0).all()
                a = s.rollout_policy(s0, xs, d, 1, **kw)
                b = s.rollout_policy(s0 + d, a["x"][:, 0].copy(), d, 1, **kw)
                assert np.array_equal(a["x"][:, 0], r["x"][:, 0]) and np.array_equal(a["u"][:, 0], r["u"][:, 0]), (controller, integrator)
                assert np.array_equal(b["x"][:, 0], r["x"][:, 1]) and np.array_equal(b["u"][:, 0], r["u"][:, 1]), (controller, integrator)
                assert np.array_equal(a["steps"] + b["steps"], r["steps"])
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 6. batch independence
def test_every_instance_equals_its_solo_rollout(model):
    s, _, _, _, x0 = solved(model, False, "events")
    try:
        s0 = S0["events"]
        xs = start(x0, False, 4)
        pushes = plant_pushes(s0)
        s.set_plant(**GAINS)
        s.set_pushes(pushes)
        rs = {c: s.rollout_policy(s0, xs, D, 2, controller=c) for c in ("feedforward", "feedback")}
    finally:
        s.close()
    for b in range(B):
        solo, _, _, _, _ = solved(model, False, "events", rows=slice(b, b + 1))
        try:
            solo.set_plant(**GAINS)
            solo.set_pushes(pushes[b:b + 1])
            for c, r in rs.items():
                r1 = solo.rollout_policy(s0[b:b + 1], xs[b:b + 1], D, 2, controller=c)
                for k in KEYS:
                    assert np.array_equal(r1[k], r[k][b:b + 1]), (b, c, k)
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
        r1 = solo.rollout_policy(s0, xs, D, 2, controller="feedback")
        r = big.rollout_policy(np.repeat(s0, 64), np.repeat(xs, 64, axis=0), D, 2, controller="feedback")
        assert (r1["status"] == 0).all()
        for k in KEYS:
            assert np.array_equal(r[k], np.repeat(r1[k], 64, axis=0)), k
    finally:
        big.close()
        solo.close()


# ---------------------------------------------------------------------------------------------- 7. the resident loop
def test_the_loop_runs_on_the_plant_and_keeps_it(model):
    case = loop_case(model, batch=B)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        loop_start(s, model, case)
        plain = s.loop_run(2)
        s.set_plant(**GAINS)
        want = by_hand(s, model, case, 2, "feedforward")         # the plant survives the uploads
        loop_start(s, model, case)                               # ... and the start of a loop
        got = s.loop_run(2)
        assert s.get_plant()["kind"] == "torque"
        s.loop_isolate(s.episode_settings("reset"), x_reset=case["x0"])
        s.loop_reset([1])
        g = s.get_plant()
        assert g["kind"] == "torque" and (g["kp"] == 100.0).all() and (g["kd"] == 2.0).all() and (g["armature"] == 0.01).all() and g["lookahead"] == 0.005
    finally:
        s.close()
    assert got["cycles_done"] == 2 and np.isfinite(got["x"]).all()
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])
    assert not np.array_equal(got["x"], plain["x"])


# ---------------------------------------------------------------------------------------------- 8. the iteration is untouched
def test_run_is_bit_identical_with_and_without_a_plant(model):
    x0, x, u, par, dt = problem(model, False, 5)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    twin = HipSqpSolver(model, max_nodes=N, max_batch=B)
    try:
        s.set_plant(**GAINS)
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


# ---------------------------------------------------------------------------------------------- 9. errors
def test_errors(model, cmodel):
    import ctypes as C
    c = HipSqpSolver(cmodel, max_nodes=N, max_batch=B)
    try:
        with pytest.raises(HsqpError) as ei:
            c.set_plant(**GAINS)
        assert ei.value.code == _abi.ERR_BAD_ARG and "hsqp_plant_set" in str(ei.value) and "whole-body handles only" in str(ei.value)
    finally:
        c.close()
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)

    def refused(what, **kw):
        st = s.plant_settings(**kw)
        rc = s.lib.hsqp_plant_set(s.h, C.byref(st))
        msg = s.lib.hsqp_last_error(s.h).decode()
        assert rc == _abi.ERR_BAD_ARG and "hsqp_plant_set" in msg and what in msg, (what, rc, msg)
    try:
        assert s.get_plant()["kind"] == "flow"
        assert s.lib.hsqp_plant_set(s.h, None) == _abi.ERR_BAD_ARG and "null" in s.lib.hsqp_last_error(s.h).decode()
        assert s.lib.hsqp_plant_get(s.h, None) == _abi.ERR_BAD_ARG and "null" in s.lib.hsqp_last_error(s.h).decode()
        refused("unknown kind", kind=2)
        refused("unknown kind", kind=-1)
        refused("reserved", reserved=1)
        refused("lookahead", lookahead=-1e-3)
        refused("lookahead", lookahead=np.nan)
        bad = np.full(NJ, 1.0)
        bad[7] = -1.0
        refused("joint 7", kp=bad)
        refused("joint 7", kd=bad)
        refused("joint 7", armature=bad)
        bad[7] = np.inf
        refused("joint 7", kp=bad)
        bad[7] = np.nan
        refused("joint 7", armature=bad)
        assert s.get_plant()["kind"] == "flow"                   # no refused call left a setting behind
        s.set_plant(**GAINS, lookahead=0.0)
        g = s.get_plant()
        assert g["kind"] == "torque" and g["lookahead"] == 0.0 and (g["kp"] == 100.0).all()
        s.clear_plant()
        assert s.get_plant()["kind"] == "flow"
    finally:
        s.close()
