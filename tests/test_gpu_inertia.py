"""Per-instance inertial variations of the torque plant (include/hsqp_inertia.h) on the MI355X: plant_dynamics and RK4 rollouts against the unchanged
oracle on merged models (tests/inertia_ref.py), the neutral settings bit for bit on all four plant variants, batch independence, the resident loop,
one physical check, and the argument errors.  The small handles of tests/test_gpu_push.py: 8 nodes, 3 instances — here neutral, link scales only,
link scales + two payloads, so that one launch takes every path through inertia_apply and the table indexing."""
import ctypes as C
import signal

import numpy as np
import pytest

import actuator_ref as A
import contact_ref as CR
import inertia_ref as IR
import plant_ref as PL
import rollout_ref as R
from test_contact import RK4_STEP, grounded
from test_gpu_actuator import LIMITED
from test_gpu_contact import X_TOL as X_TOL_GROUND, grounds
from test_gpu_loop import loop_case
from test_gpu_plant import GAINS, U_TOL, plant_pushes
from test_gpu_push import B, CYCLES, D, H, KEYS, N, PERIOD, S0, by_hand, loop_start, problem, same, solved, start
from test_gpu_rollout import policies
from test_inertia import COND_MAX, DYN_FLOOR
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu
NX, NU, NV, NJ, NB = _abi.NX, _abi.NU, _abi.NV, _abi.NJ, _abi.NB
# M, nle against the merged oracles: ten times the host build's measured nominal error (1.59e-16, tests/test_inertia.py), not below 1e-12
DYN_TOL = max(10 * 1.59e-16, DYN_FLOOR)
# x against the reference: ten times the host emulation's error against the same reference (tests/test_inertia.py::test_rk4_rollout_matches_numpy prints
# 5.6e-16 and 1.4e-15), not below 1e-10 — the convention of tests/test_gpu_plant.py X_TOL
X_TOL = max(10 * 1.4e-15, 1e-10)
VARIANTS = ("plain", "ground", "actuator", "ground + actuator")     # PlantStage, PlantContactStage, PlantActStage, PlantContactActStage
HOLD = 0.003


@pytest.fixture(autouse=True)
def time_limit():
    def expired(signum, frame):
        raise TimeoutError("test_gpu_inertia: a test ran past its 120 s limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def table():
    """The three instances: [(mass_scale [24], payloads)] — neutral, scales only, scales + both payloads (the draw of tests/test_inertia.py)."""
    return IR.variations(np.random.default_rng(2026))


def set_table(s, tab):
    s.set_inertia_instances(np.array([t[0] for t in tab]), [t[1] for t in tab])


@pytest.fixture(scope="module")
def merged(model):
    return [IR.merged_oracle(model, *t) for t in table()]


def configure(s, variant, oracle, model, xs):
    """The torque plant of the variant on the handle; returns the ground table (None: no ground)."""
    s.set_plant(**GAINS)
    g = None
    if "ground" in variant:
        g = grounds(oracle, model, xs)
        s.set_contact()
        s.set_contact_instances(g)
    if "actuator" in variant:
        s.set_actuator(command_period=HOLD, **LIMITED)
    return g


# ---------------------------------------------------------------------------------------------- 1. plant_dynamics against the merged oracles
def test_plant_dynamics_match_the_merged_oracles(model, oracle, merged):
    xs = start(problem(model, False)[0], False, 6)
    xs[:, NV:] += 0.3 * np.random.default_rng(6).standard_normal((B, NV))
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)        # no problem, no solution
    try:
        M, nle, mass = s.plant_dynamics(xs)
        for b in range(B):                                   # no table: the nominal model's, whatever the instance
            Mr, nr = oracle.full_dynamics(xs[b])
            eM, en = np.abs(M[b] - Mr).max() / max(1.0, np.abs(Mr).max()), np.abs(nle[b] - nr).max() / max(1.0, np.abs(nr).max())
            print(f"no table, instance {b}: M error {eM:.2e}, nle error {en:.2e}")
            assert eM <= DYN_TOL and en <= DYN_TOL and abs(mass[b] - oracle.total_mass()) <= 1e-13 * mass[b], (b, eM, en)
        tab = table()
        set_table(s, tab)
        s.set_plant(kind="flow", **GAINS)                    # whatever the plant kind
        M, nle, mass = s.plant_dynamics(xs)
        for b in range(B):
            Mr, nr = merged[b].full_dynamics(xs[b])
            assert np.linalg.cond(Mr) <= COND_MAX
            eM, en = np.abs(M[b] - Mr).max() / max(1.0, np.abs(Mr).max()), np.abs(nle[b] - nr).max() / max(1.0, np.abs(nr).max())
            want = sum(p[0] for p in IR.merged_bodies(model.raw, *tab[b]))
            print(f"instance {b}: mass {mass[b]:.3f} kg, M error {eM:.2e}, nle error {en:.2e}")
            assert eM <= DYN_TOL and en <= DYN_TOL, (b, eM, en)
            assert np.array_equal(M[b], M[b].T) and abs(mass[b] - want) <= 1e-13 * want, (b, mass[b], want)
        assert mass[2] - mass[0] > 5.0                       # the payloads are carried
        # one instance alone, and any output may be NULL
        x1 = np.ascontiguousarray(xs[2:3])
        nle1 = np.zeros((1, NV))
        s.set_inertia_instances(tab[2][0][None], [tab[2][1]])
        s._check(s.lib.hsqp_inertia_eval(s.h, 1, x1.ctypes.data_as(C.POINTER(C.c_double)), None, nle1.ctypes.data_as(C.POINTER(C.c_double)), None))
        assert np.array_equal(nle1[0], nle[2])
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 2. RK4 against the reference
@pytest.mark.parametrize("grid,controller", [("uniform", "feedforward"), ("events", "feedback")])
def test_rk4_matches_the_reference(model, oracle, merged, grid, controller):
    s, out, dts, dt, x0 = solved(model, False, grid)
    try:
        s0 = S0[grid]
        xs = start(x0, False)
        pushes = plant_pushes(s0)
        s.set_plant(**GAINS)
        s.set_pushes(pushes)
        nominal = s.rollout_policy(s0, xs, D, 2, integrator="rk4", controller=controller, initial_step=H)
        set_table(s, table())
        r = s.rollout_policy(s0, xs, D, 2, integrator="rk4", controller=controller, initial_step=H)
        assert (r["status"] == 0).all() and (r["rejected"] == 0).all()
        pl = PL.plant(**GAINS)
        pols = policies(s, out, dts, dt, grid, False)
        ctl = R.FEEDBACK if controller == "feedback" else R.FEEDFORWARD
        st = R.settings(R.RK4, ctl, initial_step=H)
        for b in range(B):
            cl = IR.closed_loop(oracle, merged[b], model, pols[b], out["x"][b], pl, ctl)
            xr, ur, sr, nr, _ = PL.rollout(cl, pols[b], st, s0[b], xs[b], D, 2, pushes[b])
            assert sr == R.OK and r["steps"][b] == nr, (b, r["steps"][b], nr)
            err = np.abs(r["x"][b] - xr).max() / max(1.0, np.abs(xr).max())
            erru = np.abs(r["u"][b] - ur).max() / max(1.0, np.abs(ur).max())
            print(f"{grid} {controller} instance {b}: steps {nr}, x error {err:.2e}, u error {erru:.2e}")
            assert err <= X_TOL, (b, err)
            assert erru <= U_TOL, (b, erru)
        assert np.array_equal(r["x"][0], nominal["x"][0])                                       # the neutral instance
        assert not np.array_equal(r["x"][1], nominal["x"][1]) and not np.array_equal(r["x"][2], nominal["x"][2])
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 3. on the ground, under the actuator model
def test_rk4_on_the_ground_under_the_actuator_model_matches_the_reference(model, oracle, merged):
    """The instantiation with the ground, the actuator model and the table, against contact_ref + actuator_ref on the merged oracles; the bound and
    the step of tests/test_gpu_contact.py (the reference's contact force carries a central-difference Jacobian)."""
    s, out, dts, dt, x0 = solved(model, False, "events")
    try:
        s0 = S0["events"]
        xs = start(x0, False)
        pushes = plant_pushes(s0)
        g = configure(s, "ground + actuator", oracle, model, xs)
        s.set_pushes(pushes)
        set_table(s, table())
        r = s.rollout_policy(s0, xs, D, 2, integrator="rk4", controller="feedback", initial_step=RK4_STEP)
        assert (r["status"] == 0).all() and (r["rejected"] == 0).all()
        pl, ac = PL.plant(**GAINS), A.actuator(HOLD, **LIMITED)
        pols = policies(s, out, dts, dt, "events", False)
        st = R.settings(R.RK4, R.FEEDBACK, initial_step=RK4_STEP)
        for b in range(B):
            cl = IR.ActuatedClosedLoop(oracle, merged[b], model, pols[b], out["x"][b], pl, R.FEEDBACK, ac, CR.with_ground(CR.contact(model), g[b]))
            xr, ur, sr, nr, _, _ = A.rollout(cl, pols[b], st, s0[b], xs[b], D, 2, pushes[b])
            assert sr == R.OK and r["steps"][b] == nr, (b, r["steps"][b], nr)
            err = np.abs(r["x"][b] - xr).max() / max(1.0, np.abs(xr).max())
            erru = np.abs(r["u"][b] - ur).max() / max(1.0, np.abs(ur).max())
            print(f"ground + actuator instance {b}: steps {nr}, x error {err:.2e}, u error {erru:.2e}")
            assert err <= X_TOL_GROUND, (b, err)
            assert erru <= U_TOL, (b, erru)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 4. neutrality, bit for bit
@pytest.mark.parametrize("variant", VARIANTS)
def test_a_neutral_and_a_cleared_table_equal_a_fresh_handle(model, oracle, variant):
    s, _, _, _, x0 = solved(model, False, "events")
    fresh, _, _, _, _ = solved(model, False, "events")
    try:
        s0 = S0["events"]
        xs = start(x0, False, 2)
        pushes = plant_pushes(s0)
        for h in (s, fresh):
            h.set_pushes(pushes)
            configure(h, variant, oracle, model, xs)
        tab = table()
        for controller in ("feedforward", "feedback"):
            kw = dict(controller=controller)                       # ODE45: the step control sees every bit
            want = fresh.rollout_policy(s0, xs, D, 2, **kw)
            s.set_inertia_instances(np.ones(B))
            assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "neutral table"
            s.set_inertia_instances(np.ones((1, NB)))              # a table shorter than the batch: the instances past it are neutral
            assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "short neutral table"
            set_table(s, tab)
            r = s.rollout_policy(s0, xs, D, 2, **kw)
            assert not same(r, want) and np.array_equal(r["x"][0], want["x"][0])
            s.clear_inertia()
            assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "cleared table"
            set_table(s, tab)
            s.set_inertia_instances(None)
            assert same(s.rollout_policy(s0, xs, D, 2, **kw), want), "NULL table"
    finally:
        s.close()
        fresh.close()


def test_a_table_is_inert_on_the_flow_plant(model):
    s, _, _, _, x0 = solved(model, False, "events")
    try:
        s0 = S0["events"]
        xs = start(x0, False, 2)
        want = s.rollout_policy(s0, xs, D, 2)
        set_table(s, table())
        assert same(s.rollout_policy(s0, xs, D, 2), want), "no plant"
        s.set_plant(kind="flow", **GAINS)
        assert same(s.rollout_policy(s0, xs, D, 2), want), "kind flow"
        ms, pay = s.get_inertia_instances(B)                       # stored all the same
        assert np.array_equal(ms, np.array([t[0] for t in table()])) and pay == [t[1] for t in table()]
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 5. batch independence
@pytest.mark.parametrize("variant", VARIANTS)
def test_every_instance_equals_its_solo_rollout(model, oracle, variant):
    s, _, _, _, x0 = solved(model, False, "events")
    tab = table()
    try:
        s0 = S0["events"]
        xs = start(x0, False, 4)
        pushes = plant_pushes(s0)
        g = configure(s, variant, oracle, model, xs)
        s.set_pushes(pushes)
        set_table(s, tab)
        r = s.rollout_policy(s0, xs, D, 2, controller="feedback")
    finally:
        s.close()
    for b in range(B):
        solo, _, _, _, _ = solved(model, False, "events", rows=slice(b, b + 1))
        try:
            configure(solo, variant, oracle, model, xs[b:b + 1])
            if g is not None:
                solo.set_contact_instances(g[b:b + 1])
            solo.set_pushes(pushes[b:b + 1])
            set_table(solo, tab[b:b + 1])
            r1 = solo.rollout_policy(s0[b:b + 1], xs[b:b + 1], D, 2, controller="feedback")
            for k in KEYS:
                assert np.array_equal(r1[k], r[k][b:b + 1]), (variant, b, k)
        finally:
            solo.close()


def test_sixty_four_copies_equal_the_solo_result(model):
    x0, x, u, par, dt = problem(model, False)
    one = slice(2, 3)
    tab = table()[one]
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
            set_table(h, tab * n)
        r1 = solo.rollout_policy(s0, xs, D, 2, controller="feedback")
        r = big.rollout_policy(np.repeat(s0, 64), np.repeat(xs, 64, axis=0), D, 2, controller="feedback")
        assert (r1["status"] == 0).all()
        for k in KEYS:
            assert np.array_equal(r[k], np.repeat(r1[k], 64, axis=0)), k
        M, nle, mass = big.plant_dynamics(np.repeat(xs, 64, axis=0))
        M1, nle1, mass1 = solo.plant_dynamics(xs)
        assert np.array_equal(M, np.repeat(M1, 64, axis=0)) and np.array_equal(nle, np.repeat(nle1, 64, axis=0)) and np.array_equal(mass, np.repeat(mass1, 64))
    finally:
        big.close()
        solo.close()


# ---------------------------------------------------------------------------------------------- 6. the resident loop
def test_the_loop_runs_on_the_varied_plant(model):
    case = loop_case(model, batch=B)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        s.set_plant(**GAINS)
        loop_start(s, model, case)
        plain = s.loop_run(3)
        set_table(s, table())
        want = by_hand(s, model, case, 3, "feedforward")         # the table survives the uploads
        loop_start(s, model, case)                               # ... and the start of a loop
        got = s.loop_run(3)
    finally:
        s.close()
    assert got["cycles_done"] == 3 and np.isfinite(got["x"]).all()
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])
    assert np.array_equal(got["x"][:, 0], plain["x"][:, 0])                                     # the neutral instance
    assert not np.array_equal(got["x"][:, 1], plain["x"][:, 1]) and not np.array_equal(got["x"][:, 2], plain["x"][:, 2])


def test_a_restarted_instance_keeps_its_body(model):
    """Instance 1 starts from a NaN state under RESET (tests/test_gpu_push.py): the triage restarts it at t = one period.  The table is still in
    force: from then on the instance equals, bit for bit, a fresh one-instance loop started at that time with its entry, and not a neutral one."""
    case = loop_case(model, batch=B)
    sick = case["x0"].copy()
    sick[1, 7] = np.nan
    tab = table()
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        s.set_plant(**GAINS)
        set_table(s, tab)
        loop_start(s, model, case, x0=sick)
        s.loop_isolate(s.episode_settings("reset"), x_reset=case["x0"])
        first = s.loop_run(1)
        t1 = s.loop_state()[0]
        rest = s.loop_run(CYCLES - 1)
        ep = s.loop_episodes()
        assert t1 == PERIOD and np.isnan(first["x"][0, 1]).all() and ep["n_episodes"][1] == 2 and ep["state"][1] == _abi.EP_ALIVE
        one = slice(1, 2)
        set_table(s, tab[one])
        loop_start(s, model, case, rows=one, t0=t1)
        fresh = s.loop_run(CYCLES - 1)
        s.set_inertia_instances(np.ones(1))
        loop_start(s, model, case, rows=one, t0=t1)
        neutral = s.loop_run(CYCLES - 1)
    finally:
        s.close()
    assert np.isfinite(fresh["x"]).all()
    assert np.array_equal(rest["x"][:, one], fresh["x"]) and np.array_equal(rest["u"][:, one], fresh["u"])
    assert not np.array_equal(fresh["x"], neutral["x"])


def test_the_table_is_in_force_after_a_reset_request(model):
    """hsqp_loop_reset_instances on instance 1 after one cycle: the table reads back unchanged, and the restarted instance's next cycle is its varied
    body's — it differs from the same sequence with a neutral entry 1, while its neighbours, whose entries are the same in both, do not."""
    case = loop_case(model, batch=B)
    tab = table()
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")

    def sequence(t):
        set_table(s, t)
        loop_start(s, model, case)
        s.loop_isolate(s.episode_settings("reset"), x_reset=case["x0"])
        s.loop_run(1)
        s.loop_reset([1])
        ms, pay = s.get_inertia_instances(B)
        assert np.array_equal(ms, np.array([e[0] for e in t])) and pay == [e[1] for e in t]
        return s.loop_run(1)
    try:
        s.set_plant(**GAINS)
        varied = sequence(tab)
        neutral = sequence([tab[0], (np.ones(NB), []), tab[2]])
    finally:
        s.close()
    assert np.isfinite(varied["x"]).all() and np.isfinite(neutral["x"]).all()
    assert not np.array_equal(varied["x"][0, 1], neutral["x"][0, 1])
    assert np.array_equal(varied["x"][0, 0], neutral["x"][0, 0]) and np.array_equal(varied["x"][0, 2], neutral["x"][0, 2])


# ---------------------------------------------------------------------------------------------- 7. one physical check
def test_a_heavier_robot_sinks_on_the_same_ground(model, oracle):
    """Three copies of one instance at rest on one ground, 3 mm into it with the lowest sole corner: the contact forces (contact_forces) are the
    same whatever the table, the base's vertical acceleration over one RK4 step is not.  Instance 1 has EVERY link 15 % heavier: its mass matrix and
    bias are 1.15 times the nominal ones, so vd = M^-1 (tau + J^T f) / 1.15 - M^-1 nle, and at rest the base's vertical row of M^-1 nle is g: with
    A = [M^-1 (tau + J^T f)]_z the acceleration is A / s - g, lower for the heavier robot where the ground pushes up (A > 0, asserted on the
    reference).  Instance 2 carries the two payloads on top.  The acceleration is (v_z(h) - 0) / h of a one-step rollout, device and reference
    alike; its bound is the x bound of the rollouts on the ground (tests/test_gpu_contact.py X_TOL, of max(1, |x|)) over h.  No other threshold."""
    rows = np.array([1, 1, 1])
    s, out, dts, dt, x0 = solved(model, False, "uniform", rows=rows)
    try:
        h = RK4_STEP
        s0 = np.full(B, S0["uniform"][1])
        xs = np.repeat(start(x0, False, 7)[:1], B, axis=0)
        xs[:, NV:] = 0.0
        ct = CR.contact(model, ground_height=grounded(oracle, model, xs[0], 3e-3))
        tab = [(np.ones(NB), []), (np.full(NB, 1.15), []), (np.full(NB, 1.15), IR.PAYLOADS)]
        s.set_plant(**GAINS)
        s.set_contact(ground_height=ct["ground_height"])
        set_table(s, tab)
        f, d = s.contact_forces(xs)
        assert np.array_equal(f[0], f[1]) and np.array_equal(f[0], f[2]) and f[0][..., 2].sum() > 0.0
        r = s.rollout_policy(s0, xs, h, 1, integrator="rk4", controller="feedforward", initial_step=h)
        assert (r["status"] == 0).all() and (r["steps"] == 1).all()
        got = r["x"][:, 0, NV + 2] / h
        pl = PL.plant(**GAINS)
        pols = policies(s, out, dts, dt, "uniform", False)
        st = R.settings(R.RK4, R.FEEDFORWARD, initial_step=h)
        want = np.zeros(B)
        for b in range(B):
            cl = IR.closed_loop(oracle, IR.merged_oracle(model, *tab[b]), model, pols[b], out["x"][b], pl, R.FEEDFORWARD, ct)
            xr, _, sr, nr, _ = PL.rollout(cl, pols[b], st, s0[b], xs[b], h, 1)
            assert sr == R.OK and nr == 1
            want[b] = xr[0, NV + 2] / h
            tol = X_TOL_GROUND * max(1.0, np.abs(xr).max()) / h
            print(f"instance {b}: base vertical acceleration {got[b]:.6f} m/s^2, reference {want[b]:.6f}, bound {tol:.2e}")
            assert abs(got[b] - want[b]) <= tol, (b, got[b], want[b], tol)
        assert want[0] + 9.81 > 0.0 and want[1] < want[0]            # the reference: the ground pushes up, and the heavier robot sinks
        assert got[1] < got[0]                                       # ... and so does the device's
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 8. errors
def test_errors(model, cmodel):
    c = HipSqpSolver(cmodel, max_nodes=N, max_batch=B)
    try:
        for call, who in ((lambda: c.set_inertia_instances(np.ones(1)), "hsqp_inertia_set_instances"), (lambda: c.set_inertia_instances(None), "hsqp_inertia_set_instances"),
                          (c.clear_inertia, "hsqp_inertia_clear"), (lambda: c.get_inertia_instances(1), "hsqp_inertia_get_instances"),
                          (lambda: c.plant_dynamics(np.zeros((1, NX))), "hsqp_inertia_eval")):
            with pytest.raises(HsqpError) as ei:
                call()
            assert ei.value.code == _abi.ERR_BAD_ARG and who in str(ei.value) and "whole-body handles only" in str(ei.value)
    finally:
        c.close()
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)

    def refused(what, tab, batch=None, who="hsqp_inertia_set_instances"):
        rc = s.lib.hsqp_inertia_set_instances(s.h, len(tab) if batch is None else batch, tab)
        msg = s.lib.hsqp_last_error(s.h).decode()
        assert rc == _abi.ERR_BAD_ARG and who in msg and what in msg, (what, rc, msg)

    def entry(b=2, **kw):
        """The table with one field of instance b (or of its payload 1) replaced."""
        tab = HipSqpSolver.pack_inertia(np.array([t[0] for t in table()]), [t[1] if i != b else IR.PAYLOADS for i, t in enumerate(table())])
        for k, v in kw.items():
            if k == "scale":
                tab[b].mass_scale[7] = v
            elif k in ("n_payloads", "reserved"):
                setattr(tab[b], k, v)
            elif k == "payload_reserved":
                tab[b].payload[1].reserved = v
            elif k in ("body", "mass"):
                setattr(tab[b].payload[1], k, v)
            else:
                getattr(tab[b].payload[1], k)[:] = v
        return tab
    try:
        set_table(s, table())
        before = s.get_inertia_instances(B)
        x = np.zeros((B, NX))
        dp = C.POINTER(C.c_double)
        refused("batch", entry(), batch=0)
        refused("batch", entry(), batch=-1)
        refused("batch", (_abi.InertiaInstance * (B + 1))(), batch=B + 1)
        assert s.lib.hsqp_inertia_set_instances(s.h, B + 1, None) == _abi.ERR_BAD_ARG and "batch" in s.lib.hsqp_last_error(s.h).decode()
        assert s.lib.hsqp_inertia_set_instances(s.h, -1, None) == _abi.ERR_BAD_ARG and "batch" in s.lib.hsqp_last_error(s.h).decode()
        refused("instance 2: reserved", entry(reserved=1))
        for v in (0.0, -1.0, np.inf, np.nan):
            refused("instance 2: mass_scale[7]", entry(scale=v))
            refused("instance 0: mass_scale[7]", entry(b=0, scale=v))
        for v in (-1, _abi.INERTIA_PAYLOADS + 1):
            refused("instance 2: n_payloads", entry(n_payloads=v))
        refused("instance 2: payload 1: reserved", entry(payload_reserved=3))
        for v in (-1, NB):
            refused("instance 2: payload 1: body", entry(body=v))
        for v in (-0.5, np.inf, np.nan):
            refused("instance 2: payload 1: mass", entry(mass=v))
        for v in (np.inf, np.nan):
            refused("instance 2: payload 1: com", entry(com=[0.0, v, 0.0]))
            refused("instance 2: payload 1: inertia", entry(inertia=[0.01, 0.0, 0.0, v, 0.0, 0.01]))
        refused("instance 0: payload 1: inertia", entry(b=0, inertia=[-0.01, 0.0, 0.0, 0.01, 0.0, 0.01]))        # a negative diagonal entry
        refused("instance 2: payload 1: inertia", entry(inertia=[0.01, 0.02, 0.0, 0.01, 0.0, 0.01]))             # a negative 2 x 2 minor
        refused("instance 2: payload 1: inertia", entry(inertia=[1.0, 0.9, 0.9, 1.0, -0.9, 1.0]))                # a negative determinant
        # a rank-deficient inertia in general axes — a thin rod along d, whose determinant and minors are zero up to rounding — is positive semidefinite
        for d in ([0.3, -0.5, 0.8], [1.0, 1.0, 0.0], [0.0, 0.6, -0.8], [-0.7, 0.1, 0.2]):
            d = np.array(d) / np.linalg.norm(d)
            J = 0.02 * (np.eye(3) - np.outer(d, d))
            s._check(s.lib.hsqp_inertia_set_instances(s.h, B, entry(inertia=[J[0, 0], J[0, 1], J[0, 2], J[1, 1], J[1, 2], J[2, 2]])))
        # a payload past n_payloads is not looked at
        ok = entry(n_payloads=1, body=-5)
        s._check(s.lib.hsqp_inertia_set_instances(s.h, B, ok))
        set_table(s, table())
        for call, who in ((lambda: s.lib.hsqp_inertia_get_instances(s.h, 0, entry()), "hsqp_inertia_get_instances"),
                          (lambda: s.lib.hsqp_inertia_get_instances(s.h, B + 1, (_abi.InertiaInstance * (B + 1))()), "hsqp_inertia_get_instances"),
                          (lambda: s.lib.hsqp_inertia_get_instances(s.h, B, None), "hsqp_inertia_get_instances"),
                          (lambda: s.lib.hsqp_inertia_eval(s.h, 0, x.ctypes.data_as(dp), None, None, None), "hsqp_inertia_eval"),
                          (lambda: s.lib.hsqp_inertia_eval(s.h, B + 1, x.ctypes.data_as(dp), None, None, None), "hsqp_inertia_eval"),
                          (lambda: s.lib.hsqp_inertia_eval(s.h, B, None, None, None, None), "hsqp_inertia_eval"),
                          (lambda: s.lib.hsqp_inertia_eval_device(s.h, B + 1, x.ctypes.data_as(dp), None, None, None), "hsqp_inertia_eval_device")):
            assert call() == _abi.ERR_BAD_ARG and who in s.lib.hsqp_last_error(s.h).decode(), who
        after = s.get_inertia_instances(B)                        # no refused call replaced the table
        assert np.array_equal(after[0], before[0]) and after[1] == before[1]
        ms, pay = s.get_inertia_instances(B)
        s.set_inertia_instances(ms[:1], pay[:1])
        ms1, pay1 = s.get_inertia_instances(B)                    # instances past the table: neutral
        assert np.array_equal(ms1[1:], np.ones((B - 1, NB))) and pay1[1:] == [[], []] and np.array_equal(ms1[0], ms[0])
        s.clear_inertia()
        assert np.array_equal(s.get_inertia_instances(B)[0], np.ones((B, NB)))
    finally:
        s.close()
