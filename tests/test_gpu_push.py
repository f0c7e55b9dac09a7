"""External pushes on the plant (include/hsqp_push.h) on the MI355X: the pushed rollout against the numpy restatement (tests/push_ref.py) on the CPU
oracle's UNCHANGED flow maps — a push enters the reference as the equivalent change of a foot's contact wrench (E1 / E2 of tests/test_push.py) —
ODE45 against a tight RK4 solution of that reference, the unpushed paths, batch order, chaining and the resident loop bit for bit, the iteration
untouched, and the argument errors.  Small handles: 8 nodes, 3 instances (none, one push, two overlapping pushes on different bodies)."""
import ctypes as C
import signal

import numpy as np
import pytest

import push_ref as P
import rollout_ref as R
from test_gpu_feedback_policy import DeviceBuffer
from test_gpu_loop import loop_case
from test_gpu_rollout import policies
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import make_centroidal_problem, make_problem, swing_config
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu
NX, NU, CNX = _abi.NX, _abi.NU, _abi.CNX
B, N = 3, 8
BASE, L_FOOT, R_FOOT, TORSO, L_ELBOW = 0, 6, 12, 15, 19
D = 2.0 ** -6                # rollout duration: 3.9 RK4 steps of 0.004, two samples
H = 0.004
KEYS = ("x", "u", "status", "steps", "rejected")


@pytest.fixture(autouse=True)
def time_limit():
    def expired(signum, frame):
        raise TimeoutError("test_gpu_push: a test ran past its 120 s limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def problem(m, cent, seed=3):
    return (make_centroidal_problem if cent else make_problem)(m, n_nodes=N, batch=B, perturb=True, seed=seed)


def grid_dts(dt, grid):
    dts = np.full(N, dt)
    if grid == "events":
        dts[2] = 0.0                     # an event at 0.07 (dt = 0.035)
    return dts


def solved(m, cent, grid, rows=slice(None), seed=3):
    """A solver holding one successful iteration of the instances `rows` of the perturbed problem: (solver, solution, dts, dt, x0)."""
    x0, x, u, par, dt = problem(m, cent, seed)
    x0, x, u, par = x0[rows], x[rows], u[rows], par[rows]
    dts = grid_dts(dt, grid)
    s = HipSqpSolver(m, max_nodes=N, max_batch=B, riccati="serial")
    out = s.run(x0, x, u, par, dts if grid == "events" else dt)
    return s, out, dts, dt, x0


def start(x0, cent, seed=0):
    rng = np.random.default_rng(seed)
    x = x0.copy()
    nl = CNX if cent else NX
    x[:, :nl] += 0.01 * rng.standard_normal((len(x), nl))
    if cent:
        x[:, CNX:] = 0.0
    return x


S0 = {"uniform": np.array([0.0, 0.04, 0.075]), "events": np.array([0.0, 0.04, 0.06])}      # events: the last window holds the event stamp 0.07


def pushes_for(s0):
    """Instance 0: none.  Instance 1: one push whose edges fall inside steps, across the first sample time.  Instance 2: two overlapping pushes
    on different bodies, the second one ending between the samples and starting exactly on a step boundary."""
    return [[],
            [P.push(TORSO, s0[1] + 0.003, 0.0065, [0.0, 0.05, 0.2], [70.0, -20.0, 0.0])],
            [P.push(L_ELBOW, s0[2] + 0.0015, 0.009, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0]), P.push(BASE, s0[2] + H, 0.008, [0.0, 0.0, 0.05], [-60.0, 0.0, 20.0])]]


def flow_of(model, cent, oracle, coracle):
    return P.pushed_flow(R.cent_flow(coracle) if cent else R.wb_flow(oracle), model, cent)


# ---------------------------------------------------------------------------------------------- 1. RK4 against push_ref
@pytest.mark.parametrize("formulation,grid,controller", [("wb", "uniform", "feedforward"), ("wb", "events", "feedback"), ("wb", "uniform", "feedback"),
                                                         ("centroidal", "events", "feedforward"), ("centroidal", "uniform", "feedback")])
def test_rk4_with_pushes_matches_the_oracle(model, cmodel, oracle, coracle, formulation, grid, controller):
    cent = formulation == "centroidal"
    s, out, dts, dt, x0 = solved(cmodel if cent else model, cent, grid)
    try:
        s0 = S0[grid]
        xs = start(x0, cent)
        pushes = pushes_for(s0)
        unpushed = s.rollout_policy(s0, xs, D, 2, integrator="rk4", controller=controller, initial_step=H)
        s.set_pushes(pushes)
        r = s.rollout_policy(s0, xs, D, 2, integrator="rk4", controller=controller, initial_step=H)
        assert (r["status"] == 0).all() and (r["rejected"] == 0).all()
        pols = policies(s, out, dts, dt, grid, cent)
        flow = flow_of(model, cent, oracle, coracle)
        st = R.settings(R.RK4, R.FEEDBACK if controller == "feedback" else R.FEEDFORWARD, initial_step=H)
        for b in range(B):
            xr, ur, sr, nr, _ = P.rollout(flow, pols[b], st, s0[b], xs[b], D, 2, pushes[b], 0.0)
            assert sr == R.OK and r["steps"][b] == nr, (b, r["steps"][b], nr)
            err = np.abs(r["x"][b] - xr).max() / max(1.0, np.abs(xr).max())
            erru = np.abs(r["u"][b] - ur).max() / max(1.0, np.abs(ur).max())
            print(f"{formulation} {grid} {controller} instance {b}: steps {nr}, x error {err:.2e}, u error {erru:.2e}")
            assert err <= 1e-10, (b, err)                      # tests/test_gpu_rollout.py::test_rk4_matches_the_oracle's bounds
            assert erru <= 1e-9, (b, erru)
        assert (r["steps"][1:] > unpushed["steps"][1:]).all()      # the edges restart the step sequence
        assert np.abs(r["x"][1:] - unpushed["x"][1:]).max() > 1e-6  # and the pushes are felt
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 2. ODE45 against a tight solution
def tight_solution(pflow, pol, controller, s0, x0, duration, pushes, steps_per_second=4096):
    """RK4 with steps of at most 1 / 4096 s on the reference, piece by piece between the break points (events, push edges).  On a piece the
    controller is the interpolant of that piece up to and including its end: a stage at the end time of a piece that ends at an event is
    evaluated one ulp before it, since AT the stamp the policy already answers from the post-event node.  (The restatement of
    push_ref.rollout follows the device there, and a fixed-step RK4 then carries the jump of the input with weight h / 6 of its last step:
    4.6e-4 in x at 1 / 4096 s on the events grid, whatever the step.  ODE45's 5th-order solution has no weight on that stage.)"""
    live = P.edges(pushes, 0.0)
    x = np.zeros(NX)
    nl = CNX if pol.cent else NX
    x[:nl] = np.asarray(x0)[:nl]
    t, tb = s0, s0 + duration
    while t < tb:
        te = P.next_break(pol, live, t, tb)
        active = [p for e0, e1, p in live if e0 <= t < e1]
        left = np.nextafter(te, t)

        def f(s, xx):
            return pflow(xx, pol.control(min(s, left), xx, controller), active)
        n = max(1, int(np.ceil((te - t) * steps_per_second)))
        h = (te - t) / n
        for i in range(n):
            a = t + i * h
            k1 = f(a, x)
            k2 = f(a + 0.5 * h, x + 0.5 * h * k1)
            k3 = f(a + 0.5 * h, x + 0.5 * h * k2)
            k4 = f(a + h, x + h * k3)
            x = x + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        t = te
    return x


@pytest.mark.parametrize("formulation,grid,controller", [("wb", "uniform", "feedforward"), ("wb", "events", "feedback"), ("centroidal", "uniform", "feedback")])
def test_ode45_with_pushes_against_a_tight_solution(model, cmodel, oracle, coracle, formulation, grid, controller):
    """Shaped like tests/test_gpu_rollout.py::test_ode45_against_a_tight_solution, with its tolerances.  The tight solution: tight_solution
    above (restarted at the events and the push edges; no window holds a node stamp that is not an event)."""
    cent = formulation == "centroidal"
    s, out, dts, dt, x0 = solved(cmodel if cent else model, cent, grid)
    try:
        s0 = S0[grid]
        T = 1.0 / 60.0
        xs = start(x0, cent, 1)
        pushes = pushes_for(s0)
        pols = policies(s, out, dts, dt, grid, cent)
        flow = flow_of(model, cent, oracle, coracle)
        ctl = R.FEEDBACK if controller == "feedback" else R.FEEDFORWARD
        refs = [tight_solution(flow, pols[b], ctl, s0[b], xs[b], T, pushes[b]) for b in range(B)]
        assert all(np.isfinite(x).all() for x in refs)
        s.set_pushes(pushes)
        r = s.rollout_policy(s0, xs, T, 1, controller=controller)
        assert (r["status"] == 0).all()
        r2 = s.rollout_policy(s0, xs, T, 1, controller=controller, abs_tol=1e-10, rel_tol=1e-10)
        assert (r2["status"] == 0).all() and (r2["steps"] > r["steps"]).all()
        errs = [float(np.abs(r2["x"][b, 0] - refs[b]).max()) for b in range(B)]
        stamps = np.concatenate([[0.0], np.cumsum(dts if grid == "events" else np.full(N, dt))])
        ratios = [float((np.abs(r["x"][b, 0] - refs[b]) / (1e-5 + 1e-3 * np.abs(refs[b]))).max()) for b in range(B)]
        print(f"{formulation} {grid} {controller}: steps {r['steps']} rejected {r['rejected']} error / tolerance {np.round(ratios, 2)}; "
              f"tight steps {r2['steps']} tight errors {errs}")
        for b in range(B):
            assert errs[b] <= 1e-7, (b, errs)
            kink = ((stamps > s0[b]) & (stamps < s0[b] + T)).any()
            assert ratios[b] <= (50.0 if kink else 10.0), (b, kink, ratios)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 3. the unpushed paths, bit for bit
def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS)


@pytest.mark.parametrize("formulation", ["wb", "centroidal"])
def test_inert_tables_equal_a_run_without_the_feature(model, cmodel, formulation):
    cent = formulation == "centroidal"
    s, out, dts, dt, x0 = solved(cmodel if cent else model, cent, "events")
    try:
        s0 = S0["events"]
        xs = start(x0, cent, 2)
        outside = [P.push(TORSO, -1.0, 1.0, [0, 0, 0.1], [90.0, 0, 0]), P.push(BASE, s0.max() + D, 1.0, [0, 0, 0], [0, 90.0, 0]),
                   P.push(L_FOOT, 0.05, 0.0, [0, 0, 0], [0, 0, 90.0])]
        for controller in ("feedforward", "feedback"):
            for integrator in ("ode45", "rk4"):
                kw = dict(integrator=integrator, controller=controller, initial_step=H if integrator == "rk4" else 0.015)
                s.clear_pushes()
                want = s.rollout_policy(s0, xs, D, 2, **kw)
                s.set_pushes([[], [], []])
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "n_pushes all zero"
                s.set_pushes([outside] * B)
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "pushes wholly outside the window"
                s.set_pushes(pushes_for(s0))
                assert not same(s.rollout_policy(s0, xs, D, 2, **kw), want)
                s.clear_pushes()
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "cleared table"
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 4. the unpushed instance, batch order
def test_the_unpushed_instance_equals_its_solo_rollout_and_batch_order_does_not_matter(model):
    perm = np.array([2, 0, 1])
    s, _, _, _, x0 = solved(model, False, "events")
    sp, _, _, _, _ = solved(model, False, "events", rows=perm)
    solo, _, _, _, _ = solved(model, False, "events", rows=slice(0, 1))
    try:
        s0 = S0["events"]
        xs = start(x0, False, 4)
        pushes = pushes_for(s0)
        s.set_pushes(pushes)
        sp.set_pushes([pushes[i] for i in perm])
        for controller in ("feedforward", "feedback"):
            r = s.rollout_policy(s0, xs, D, 2, controller=controller)
            rp = sp.rollout_policy(s0[perm], xs[perm], D, 2, controller=controller)
            r1 = solo.rollout_policy(s0[:1], xs[:1], D, 2, controller=controller)
            for k in KEYS:
                assert np.array_equal(rp[k], r[k][perm]), (controller, k)
                assert np.array_equal(r1[k], r[k][:1]), (controller, k)
    finally:
        s.close()
        sp.close()
        solo.close()


# ---------------------------------------------------------------------------------------------- 5. chained calls
@pytest.mark.parametrize("formulation", ["wb", "centroidal"])
def test_chained_calls_equal_one_call_with_pushes(model, cmodel, formulation):
    cent = formulation == "centroidal"
    s, out, dts, dt, x0 = solved(cmodel if cent else model, cent, "events")
    try:
        s0 = np.array([0.0, 2.0 ** -5, 2.0 ** -4])          # the last one: [0.0625, 0.078125] over the event at 0.07
        d = 2.0 ** -8
        xs = start(x0, cent, 2)
        s.set_pushes(pushes_for(s0))
        for controller in ("feedforward", "feedback"):
            for integrator in ("ode45", "rk4"):
                kw = dict(integrator=integrator, controller=controller, initial_step=0.003 if integrator == "rk4" else 0.015)
                r = s.rollout_policy(s0, xs, 4 * d, 4, **kw)
                assert (r["status"] == 0).all()
                xc, steps = xs.copy(), np.zeros(B, np.int64)
                for j in range(4):
                    rj = s.rollout_policy(s0 + j * d, xc, d, 1, **kw)
                    assert np.array_equal(rj["x"][:, 0], r["x"][:, j]) and np.array_equal(rj["u"][:, 0], r["u"][:, j]), (controller, integrator, j)
                    xc = rj["x"][:, 0]
                    steps += rj["steps"]
                assert np.array_equal(steps, r["steps"])
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 6. the resident loop
PERIOD, CYCLES = 1.0 / 60.0, 4


def loop_pushes(t0=0.0):
    """On the loop's clock: start in cycle 1, end in cycle 2."""
    return [[],
            [P.push(TORSO, t0 + 1.4 * PERIOD, 1.2 * PERIOD, [0.0, 0.0, 0.2], [80.0, 30.0, 0.0])],
            [P.push(BASE, t0 + 1.25 * PERIOD, 1.0 * PERIOD, [0.0, 0.0, 0.0], [0.0, -70.0, 0.0]), P.push(L_ELBOW, t0 + 1.5 * PERIOD, 1.0 * PERIOD, [0.0, 0.0, -0.1], [30.0, 0.0, 0.0])]]


def loop_start(s, model, case, rows=slice(None), t0=0.0, x0=None, controller="feedforward"):
    st = s.loop_settings(N, model.sqp["dt"], period=PERIOD, filter_alpha=0.8, iterations=1, take_step=True, linesearch=True, controller=controller)
    s.loop_start(st, t0, case["x0"][rows] if x0 is None else x0, case["cmd"][rows], case["ne"][rows], case["ev"][rows], case["seq"][rows])


def by_hand(s, model, case, cycles, controller):
    """The cycles through the public calls (tests/test_gpu_loop.py::by_hand on this file's horizon)."""
    dt, sw = model.sqp["dt"], swing_config(model)
    x, cmd = case["x0"].copy(), case["cmd"].copy()
    vf, t = cmd.copy(), 0.0
    xs, us = [], []
    for c in range(cycles):
        tt, ts, vf = s.command_targets(cmd, x, t, N * dt, filter_alpha=0.8, v_filt=vf)
        s.upload_reference_warm(x, N, dt, t, case["ne"], case["ev"], case["seq"], tt, ts, sw, mode="cold" if c == 0 else "shift")
        s.iterate(1, take_step=True, linesearch=True)
        r = s.rollout_policy(np.zeros(len(x)), x, PERIOD, 1, controller=controller)
        x = r["x"][:, 0].copy()
        xs.append(x)
        us.append(r["u"][:, 0].copy())
        t += PERIOD
    return dict(x=np.array(xs), u=np.array(us))


@pytest.mark.parametrize("controller", ["feedforward", "feedback"])
def test_the_loop_applies_the_pushes_on_its_clock(model, controller):
    case = loop_case(model, batch=B)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        loop_start(s, model, case, controller=controller)
        plain = s.loop_run(CYCLES)
        s.set_pushes(loop_pushes())
        want = by_hand(s, model, case, CYCLES, controller)          # the table survives the uploads
        loop_start(s, model, case, controller=controller)            # ... and the start of a loop
        got = s.loop_run(CYCLES)
        assert s.get_pushes() == loop_pushes()
    finally:
        s.close()
    assert got["cycles_done"] == CYCLES and np.isfinite(got["x"]).all()
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])                  # the loop's contract
    assert np.array_equal(got["x"][:, 0], plain["x"][:, 0]) and np.array_equal(got["u"][:, 0], plain["u"][:, 0])   # the unpushed instance
    for b in (1, 2):
        assert np.array_equal(got["x"][0, b], plain["x"][0, b]), b       # nothing before cycle 1
        for c in range(1, CYCLES):
            assert not np.array_equal(got["x"][c, b], plain["x"][c, b]), (b, c)
        print(f"{controller} instance {b}: pushed - unpushed per cycle", [float(np.abs(got['x'][c, b] - plain['x'][c, b]).max()) for c in range(CYCLES)])


def test_a_restarted_instance_keeps_its_pushes_on_the_loops_clock(model):
    """Instance 1 starts from a NaN state under RESET: the triage restarts it at t = one period from x_reset.  From then on it equals, bit for bit,
    a fresh one-instance loop started at that time with the same pushes (which start in cycle 1 and end in cycle 2 of the loop's clock)."""
    case = loop_case(model, batch=B)
    sick = case["x0"].copy()
    sick[1, 7] = np.nan
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        s.set_pushes(loop_pushes())
        loop_start(s, model, case, x0=sick)
        s.loop_isolate(s.episode_settings("reset"), x_reset=case["x0"])
        first = s.loop_run(1)
        t1 = s.loop_state()[0]
        rest = s.loop_run(CYCLES - 1)
        ep = s.loop_episodes()
        assert t1 == PERIOD and np.isnan(first["x"][0, 1]).all() and ep["n_episodes"][1] == 2 and ep["state"][1] == _abi.EP_ALIVE
        one = slice(1, 2)
        s.set_pushes(loop_pushes()[one])
        loop_start(s, model, case, rows=one, t0=t1)
        fresh = s.loop_run(CYCLES - 1)
        s.clear_pushes()
        loop_start(s, model, case, rows=one, t0=t1)
        plain = s.loop_run(CYCLES - 1)
    finally:
        s.close()
    assert np.isfinite(fresh["x"]).all()
    assert np.array_equal(rest["x"][:, one], fresh["x"]) and np.array_equal(rest["u"][:, one], fresh["u"])
    assert not np.array_equal(fresh["x"], plain["x"])


# ---------------------------------------------------------------------------------------------- 7. the iteration is untouched
def test_the_iteration_after_a_pushed_rollout_is_the_iteration_on_that_state(model):
    x0, x, u, par, dt = problem(model, False, 5)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    twin = HipSqpSolver(model, max_nodes=N, max_batch=B)
    try:
        s0 = S0["uniform"]
        s.set_pushes(pushes_for(s0))
        for h in (s, twin):
            h.upload(x0, x, u, par, dt)
            h.iterate(1, take_step=True)
        a, b = s.download(), twin.download()
        assert all(np.array_equal(a[k], b[k]) for k in ("x", "u", "dx", "du"))
        ra, rb = s.rollout_policy(s0, x0, D, 2), twin.rollout_policy(s0, x0, D, 2)
        assert not np.array_equal(ra["x"], rb["x"]) and np.array_equal(ra["x"][0], rb["x"][0])
        for h in (s, twin):
            h.iterate(1, take_step=True)
        a, b = s.download(), twin.download()
        assert all(np.array_equal(a[k], b[k]) for k in ("x", "u", "dx", "du"))
    finally:
        s.close()
        twin.close()


# ---------------------------------------------------------------------------------------------- 8. errors, get, the device entry point
def test_errors_get_and_the_device_entry_point(model):
    x0, x, u, par, dt = problem(model, False, 5)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True)
    ip = C.POINTER(C.c_int32)
    pp = C.POINTER(_abi.Push)

    def refused(what, pushes=None, batch=None, max_pushes=None, raw=None):
        if raw is None:
            n, tab, mp = s.pack_pushes(pushes, max_pushes)
            raw = (len(pushes) if batch is None else batch, mp if max_pushes is None else max_pushes, n.ctypes.data_as(ip), C.cast(tab, pp))
        rc = s.lib.hsqp_push_set(s.h, *raw)
        msg = s.lib.hsqp_last_error(s.h).decode()
        assert rc == _abi.ERR_BAD_ARG and "hsqp_push_set" in msg and what in msg, (what, rc, msg)

    good = P.push(TORSO, 0.0, 0.1, [0, 0, 0], [10.0, 0, 0])
    try:
        with pytest.raises(HsqpError) as ei:
            s.get_pushes()
        assert ei.value.code == _abi.ERR_BAD_ARG and "no push table" in str(ei.value)
        n1, tab1, _ = s.pack_pushes([[good]])
        refused("null", raw=(1, 1, None, C.cast(tab1, pp)))
        refused("null", raw=(1, 1, n1.ctypes.data_as(ip), None))
        refused("batch outside", raw=(0, 1, n1.ctypes.data_as(ip), C.cast(tab1, pp)))
        refused("batch outside", [[good]] * (B + 1))
        refused("max_pushes outside", raw=(1, 0, n1.ctypes.data_as(ip), C.cast(tab1, pp)))
        refused("max_pushes outside", [[good]], max_pushes=_abi.PUSH_MAX + 1)
        n_bad = np.array([2], np.int32)
        refused("n_pushes outside", raw=(1, 1, n_bad.ctypes.data_as(ip), C.cast(tab1, pp)))
        n_bad[0] = -1
        refused("n_pushes outside", raw=(1, 1, n_bad.ctypes.data_as(ip), C.cast(tab1, pp)))
        refused("body outside the tree", [[dict(good, body=_abi.NB)]])
        refused("body outside the tree", [[dict(good, body=-1)]])
        refused("reserved", [[dict(good, reserved=1)]])
        refused("negative duration", [[dict(good, duration=-1e-3)]])
        for k, v in (("duration", np.inf), ("t_start", np.nan), ("point", [0.0, np.inf, 0.0]), ("force", [np.nan, 0.0, 0.0])):
            refused("non-finite", [[good], [dict(good, **{k: v})]])
        with pytest.raises(HsqpError):
            s.get_pushes()                                   # no refused call left a table behind
        # get returns what set was given
        pushes = pushes_for(S0["uniform"])
        s.set_pushes(pushes, max_pushes=3)
        assert s.get_pushes() == pushes
        # a batch mismatch: at the rollout ...
        s.upload(x0, x, u, par, dt)
        s.iterate(1, take_step=True)
        want = s.rollout_policy(S0["uniform"], x0, D, 2)
        s.set_pushes(pushes[:2])
        with pytest.raises(HsqpError) as ei:
            s.rollout_policy(S0["uniform"], x0, D, 2)
        assert ei.value.code == _abi.ERR_BAD_ARG and "push table holds 2 instances" in str(ei.value)
        # ... and at the loop
        case = loop_case(model, batch=B)
        loop_start(s, model, case)
        with pytest.raises(HsqpError) as ei:
            s.loop_run(1)
        assert ei.value.code == _abi.ERR_BAD_ARG and "hsqp_loop_run" in str(ei.value) and "push table holds 2 instances" in str(ei.value)
        assert ei.value.result["cycles_done"] == 0
        # hsqp_push_set_device equals hsqp_push_set
        s.upload(x0, x, u, par, dt)
        s.iterate(1, take_step=True)
        n, tab, mp = s.pack_pushes(pushes, 3)
        raw = bytes(tab)
        dn, dp = DeviceBuffer((2,)), DeviceBuffer((len(raw) // 8,))
        try:
            dn.upload(np.frombuffer(n.tobytes() + b"\0" * 4, dtype=np.float64))
            dp.upload(np.frombuffer(raw, dtype=np.float64))
            s.set_pushes_device(B, mp, dn.ptr.value, dp.ptr.value)
            assert s.get_pushes() == pushes
            got = s.rollout_policy(S0["uniform"], x0, D, 2)
        finally:
            dn.free()
            dp.free()
        assert all(np.array_equal(got[k], want[k]) for k in KEYS)
    finally:
        s.close()
