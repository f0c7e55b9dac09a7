"""The ground contact of the torque plant (include/hsqp_contact.h) on the MI355X: the contact forces and the RK4 rollout against the numpy restatement
(tests/contact_ref.py) on the CPU oracle's unchanged body_placements / full_dynamics, ODE45 against a tight RK4 solution of that reference, the paths
without a ground bit for bit, batch independence and chaining, the friction coefficient, the resident loop, the iteration untouched, and the
argument errors.  The shapes of tests/test_gpu_plant.py: 8 nodes, 3 instances, 2^-6 s, the tests' gains and armature 0.01.  The ground of every
instance lies 1 mm above its lowest sole corner at the start state (a per-instance table)."""
import ctypes as C
import signal

import numpy as np
import pytest

import contact_ref as CR
import plant_ref as PL
import rollout_ref as R
from test_contact import EPS, RK4_STEP, grounded
from test_gpu_feedback_policy import DeviceBuffer
from test_gpu_loop import loop_case
from test_gpu_plant import GAINS, U_TOL, plant_pushes
from test_gpu_push import B, D, KEYS, N, S0, by_hand, loop_start, problem, same, solved, start
from test_gpu_rollout import policies
from test_plant import FD_TOL
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu
NX, NU, NV, NJ = _abi.NX, _abi.NU, _abi.NV, _abi.NJ
# x against the reference: the reference's generalised contact force carries a central-difference Jacobian, FD_TOL on the accelerations (tests/test_plant.py),
# over the duration, times 10 — the bound of tests/test_contact.py::test_rk4_rollout_matches_numpy, which the host build meets at <= 3e-9; the device's own
# rounding (1e-11 on the torque plant, tests/test_gpu_plant.py) is far below it
X_TOL = FD_TOL * D * 10


@pytest.fixture(autouse=True)
def time_limit():
    def expired(signum, frame):
        raise TimeoutError("test_gpu_contact: a test ran past its 120 s limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def grounds(oracle, model, xs, mus=(0.2, 0.6, 1.0)):
    """(height, mu) per instance: 1 mm above the lowest sole corner of its start state."""
    return np.array([(grounded(oracle, model, x), mus[b % len(mus)]) for b, x in enumerate(xs)])


# ---------------------------------------------------------------------------------------------- 1. contact_forces against contact_ref
def test_contact_forces_match_the_reference(model, oracle):
    """The bound of tests/test_contact.py::test_forces_and_penetrations_match_the_reference (tests/test_gpu_plant.py does not hold the device and the
    host build to bits): A = k 64 eps (|P_z| + |ground_height|) absolute and relative, the reference's velocities in closed form.  States: the start
    states of the rollout tests, and the same with the base pushed down by 2 mm and the joint velocities scaled by 3."""
    x0 = problem(model, False)[0]
    xs = start(x0, False)
    deep = xs.copy()
    deep[:, 2] -= 0.002
    deep[:, NV + 6:] *= 3.0
    s = HipSqpSolver(model, max_nodes=N, max_batch=2 * B)
    try:
        g = np.concatenate([grounds(oracle, model, xs), grounds(oracle, model, xs)])
        xa = np.concatenate([xs, deep])
        s.set_contact()
        s.set_contact_instances(g)
        f, d = s.contact_forces(xa)
        ct0 = CR.contact(model)
        active = 0
        for b in range(2 * B):
            ct = CR.with_ground(ct0, g[b])
            ref = CR.forces(oracle, model, xa[b], ct, velocity="frame")
            scale = np.abs(ref["P"][:, 2]) + abs(ct["ground_height"])
            A = ct["stiffness"] * 64 * EPS * scale[:, None]
            err_d, err_f = np.abs(d[b].ravel() - ref["d"]), np.abs(f[b].reshape(8, 3) - ref["f"])
            print(f"instance {b}: classes {''.join(ref['cls'])}, |f| {np.abs(ref['f']).max():.3e}, force error {err_f.max():.2e}, d error {err_d.max():.2e}")
            assert (err_d <= 64 * EPS * scale).all(), (b, err_d.max())
            assert (err_f <= A + A * np.linalg.norm(ref["f"], axis=1)[:, None]).all(), (b, err_f.max())
            active += ref["cls"].count("a")
        assert active >= B
        # the device entry points: the table and the states in device memory give the same bits
        dg, dx, df, dd = DeviceBuffer(g.shape), DeviceBuffer(xa.shape), DeviceBuffer(f.shape), DeviceBuffer(d.shape)
        try:
            dg.upload(g)
            dx.upload(xa)
            s.set_contact_instances(None)
            assert not np.array_equal(s.contact_forces(xa)[0], f)
            s.set_contact_instances_device(2 * B, dg.ptr.value)
            cast = lambda p: C.cast(p.ptr, C.POINTER(C.c_double))   # noqa: E731
            s._check(s.lib.hsqp_contact_eval_device(s.h, 2 * B, cast(dx), cast(df), cast(dd)))
            assert np.array_equal(df.numpy(), f) and np.array_equal(dd.numpy(), d)
        finally:
            for buf in (dg, dx, df, dd):
                buf.free()
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 2. RK4 against contact_ref
@pytest.mark.parametrize("grid,controller", [("uniform", "feedforward"), ("events", "feedback"), ("uniform", "feedback"), ("events", "feedforward")])
def test_rk4_matches_the_reference(model, oracle, grid, controller):
    s, out, dts, dt, x0 = solved(model, False, grid)
    try:
        s0 = S0[grid]
        xs = start(x0, False)
        pushes = plant_pushes(s0)                      # instance 1: the elbow; instance 2: the elbow and the pelvis
        g = grounds(oracle, model, xs)
        s.set_plant(**GAINS)
        s.set_pushes(pushes)
        free = s.rollout_policy(s0, xs, D, 2, integrator="rk4", controller=controller, initial_step=RK4_STEP)
        s.set_contact()
        s.set_contact_instances(g)
        r = s.rollout_policy(s0, xs, D, 2, integrator="rk4", controller=controller, initial_step=RK4_STEP)
        assert (r["status"] == 0).all() and (r["rejected"] == 0).all()
        assert np.abs(r["x"] - free["x"]).max() > 1e-6                   # the ground is felt
        pl, ct0 = PL.plant(**GAINS), CR.contact(model)
        pols = policies(s, out, dts, dt, grid, False)
        ctl = R.FEEDBACK if controller == "feedback" else R.FEEDFORWARD
        st = R.settings(R.RK4, ctl, initial_step=RK4_STEP)
        for b in range(B):
            cl = CR.closed_loop(oracle, model, pols[b], out["x"][b], pl, ctl, CR.with_ground(ct0, g[b]))
            xr, ur, sr, nr, _ = PL.rollout(cl, pols[b], st, s0[b], xs[b], D, 2, pushes[b])
            assert sr == R.OK and r["steps"][b] == nr, (b, r["steps"][b], nr)
            err = np.abs(r["x"][b] - xr).max() / max(1.0, np.abs(xr).max())
            erru = np.abs(r["u"][b] - ur).max() / max(1.0, np.abs(ur).max())
            print(f"{grid} {controller} instance {b}: steps {nr}, x error {err:.2e}, u error {erru:.2e}")
            assert err <= X_TOL, (b, err)
            assert erru <= U_TOL, (b, erru)
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 3. ODE45 against a tight solution
def test_ode45_against_a_tight_solution(model, oracle):
    """tests/test_gpu_plant.py::test_ode45_against_a_tight_solution on the ground, with its tolerance rule; the tight solution is RK4 at 2^-15 s on
    contact_ref, for ONE instance (instance 1).  Measured on the MI355X: instances 0 / 1 / 2 take 7 / 6 / 92 accepted + 10 / 3 / 25 rejected
    steps over 2^-6 s (the torque plant without a ground: 4 + 1), error / tolerance 0.56 for instance 1; at tolerances of 1e-10 114 / 87 / 660
    accepted + 39 / 11 / 54 rejected steps, tight error 1.2e-10."""
    s, out, dts, dt, x0 = solved(model, False, "uniform")
    try:
        s0 = S0["uniform"]
        T = 2.0 ** -6
        xs = start(x0, False, 1)
        g = grounds(oracle, model, xs)
        pl, ct0 = PL.plant(**GAINS), CR.contact(model)
        pols = policies(s, out, dts, dt, "uniform", False)
        b = 1
        cl = CR.closed_loop(oracle, model, pols[b], out["x"][b], pl, R.FEEDFORWARD, CR.with_ground(ct0, g[b]))
        ref = PL.tight_solution(cl, pols[b], s0[b], xs[b], T)
        assert np.isfinite(ref).all()
        s.set_plant(**GAINS)
        s.set_contact()
        s.set_contact_instances(g)
        r = s.rollout_policy(s0, xs, T, 1)
        assert (r["status"] == 0).all() and (r["steps"] < 10000).all()
        r2 = s.rollout_policy(s0, xs, T, 1, abs_tol=1e-10, rel_tol=1e-10)
        assert (r2["status"] == 0).all() and (r2["steps"] > r["steps"]).all() and (r2["steps"] < 10000).all()
        err = float(np.abs(r2["x"][b, 0] - ref).max())
        ratio = float((np.abs(r["x"][b, 0] - ref) / (1e-5 + 1e-3 * np.abs(ref))).max())
        print(f"T {T}: steps {r['steps']} rejected {r['rejected']} error / tolerance {ratio:.2f}; tight steps {r2['steps']} rejected {r2['rejected']} "
              f"tight error {err:.2e}")
        stamps = np.arange(N + 1) * dt
        kink = any(((stamps - la > s0[b]) & (stamps - la < s0[b] + T)).any() for la in (0.0, pl["lookahead"]))
        assert ratio <= (50.0 if kink else 10.0), (kink, ratio)
        assert err <= 1e-7, err
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 4. the paths without a ground, bit for bit
def test_clear_disabled_and_kind_flow_equal_a_fresh_handle(model, oracle):
    s, _, _, _, x0 = solved(model, False, "events")
    fresh, _, _, _, _ = solved(model, False, "events")
    try:
        s0 = S0["events"]
        xs = start(x0, False, 2)
        g = grounds(oracle, model, xs)
        for controller in ("feedforward", "feedback"):
            for integrator in ("ode45", "rk4"):
                kw = dict(integrator=integrator, controller=controller, initial_step=RK4_STEP if integrator == "rk4" else 0.015)
                fresh.clear_plant()
                flow = fresh.rollout_policy(s0, xs, D, 2, **kw)
                fresh.set_plant(**GAINS)
                torque = fresh.rollout_policy(s0, xs, D, 2, **kw)
                s.set_plant(**GAINS)
                s.set_contact()
                s.set_contact_instances(g)
                assert not same(s.rollout_policy(s0, xs, D, 2, **kw), torque), "contact set"
                s.set_contact(enabled=False)
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), torque), "enabled = 0"
                s.set_contact()
                s.clear_contact()
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), torque), "cleared"
                s.set_contact()
                s.set_contact_instances(g)
                s.set_plant(kind="flow", **GAINS)
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), flow), "kind flow, contact set"
                s.clear_plant()
                assert same(s.rollout_policy(s0, xs, D, 2, **kw), flow), "no plant, contact set"
                assert s.get_contact()["enabled"]                        # stored and inert
                s.clear_contact()
    finally:
        s.close()
        fresh.close()


def test_run_is_bit_identical_with_and_without_a_contact_setting(model):
    x0, x, u, par, dt = problem(model, False, 5)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    twin = HipSqpSolver(model, max_nodes=N, max_batch=B)
    try:
        s.set_plant(**GAINS)
        s.set_contact(ground_height=0.002)
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


# ---------------------------------------------------------------------------------------------- 5. batch behaviour
def test_every_instance_equals_its_solo_rollout(model, oracle):
    s, _, _, _, x0 = solved(model, False, "events")
    try:
        s0 = S0["events"]
        xs = start(x0, False, 4)
        pushes = plant_pushes(s0)
        g = grounds(oracle, model, xs)
        s.set_plant(**GAINS)
        s.set_pushes(pushes)
        s.set_contact()
        s.set_contact_instances(g)
        rs = {c: s.rollout_policy(s0, xs, D, 2, controller=c) for c in ("feedforward", "feedback")}
        assert not np.array_equal(rs["feedforward"]["x"][0], rs["feedforward"]["x"][1])
    finally:
        s.close()
    for b in range(B):
        solo, _, _, _, _ = solved(model, False, "events", rows=slice(b, b + 1))
        try:
            solo.set_plant(**GAINS)
            solo.set_pushes(pushes[b:b + 1])
            solo.set_contact()
            solo.set_contact_instances(g[b:b + 1])
            for c, r in rs.items():
                r1 = solo.rollout_policy(s0[b:b + 1], xs[b:b + 1], D, 2, controller=c)
                for k in KEYS:
                    assert np.array_equal(r1[k], r[k][b:b + 1]), (b, c, k)
        finally:
            solo.close()


def test_sixty_four_copies_equal_the_solo_result(model, oracle):
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
        g = grounds(oracle, model, xs)
        push = plant_pushes(S0["uniform"])[one]
        for h, n in ((big, 64), (solo, 1)):
            h.set_plant(**GAINS)
            h.set_pushes(push * n)
            h.set_contact()
            h.set_contact_instances(np.repeat(g, n, axis=0))
        r1 = solo.rollout_policy(s0, xs, D, 2, controller="feedback")
        r = big.rollout_policy(np.repeat(s0, 64), np.repeat(xs, 64, axis=0), D, 2, controller="feedback")
        assert (r1["status"] == 0).all()
        for k in KEYS:
            assert np.array_equal(r[k], np.repeat(r1[k], 64, axis=0)), k
    finally:
        big.close()
        solo.close()


def test_chained_calls_equal_one_call(model, oracle):
    s, _, _, _, x0 = solved(model, False, "events")
    try:
        s0 = np.array([0.0, 2.0 ** -5, 2.0 ** -4])
        d = 2.0 ** -7
        xs = start(x0, False, 2)
        s.set_plant(**GAINS)
        s.set_pushes(plant_pushes(s0))
        s.set_contact()
        s.set_contact_instances(grounds(oracle, model, xs))
        for controller in ("feedforward", "feedback"):
            for integrator in ("ode45", "rk4"):
                kw = dict(integrator=integrator, controller=controller, initial_step=RK4_STEP if integrator == "rk4" else 0.015)
                r = s.rollout_policy(s0, xs, 2 * d, 2, **kw)
                assert (r["status"] == 0).all()
                a = s.rollout_policy(s0, xs, d, 1, **kw)
                b = s.rollout_policy(s0 + d, a["x"][:, 0].copy(), d, 1, **kw)
                assert np.array_equal(a["x"][:, 0], r["x"][:, 0]) and np.array_equal(a["u"][:, 0], r["u"][:, 0]), (controller, integrator)
                assert np.array_equal(b["x"][:, 0], r["x"][:, 1]) and np.array_equal(b["u"][:, 0], r["u"][:, 1]), (controller, integrator)
                assert np.array_equal(a["steps"] + b["steps"], r["steps"])
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 6. the friction coefficient
def test_a_lower_mu_changes_the_slide(model, oracle):
    """Two instances in one state, the base sliding at 0.3 m/s, the ground 2 mm above the lowest corner, mu 0.2 and 1.0: the normal forces are the same
    bits, the tangential ones in the ratio of the coefficients (ft = -mu fn v_t / |.|: one product apart, a few eps), and the rollouts differ."""
    s, _, _, _, x0 = solved(model, False, "uniform")
    try:
        x = start(x0, False, 3)[0]
        x[NV] += 0.3
        xs = np.array([x, x, x])
        hgt = grounded(oracle, model, x, 2e-3)
        s.set_plant(**GAINS)
        s.set_contact()
        s.set_contact_instances([(hgt, 0.2), (hgt, 1.0), (hgt, 1.0)])
        f, d = s.contact_forces(xs[:2])
        on = f[0, :, :, 2] > 0.0
        assert on.any() and np.array_equal(f[0, :, :, 2], f[1, :, :, 2]) and np.array_equal(d[0], d[1])
        t0, t1 = f[0][on][:, :2], f[1][on][:, :2]
        assert np.abs(t0).max() > 0.1
        assert (np.abs(t1 - 5.0 * t0) <= 8 * EPS * np.abs(t1)).all(), np.abs(t1 / t0 - 5.0).max()
        assert (np.linalg.norm(t1, axis=1) < 1.0 * f[1][on][:, 2]).all()        # inside the cone: the regularisation never reaches mu fn
        # the slide itself: instance 0's rollout under either coefficient (the other rows keep theirs, and their bits)
        r = s.rollout_policy(np.zeros(3), xs, D, 1)
        s.set_contact_instances([(hgt, 1.0), (hgt, 1.0), (hgt, 1.0)])
        r2 = s.rollout_policy(np.zeros(3), xs, D, 1)
        assert (r["status"] == 0).all() and (r2["status"] == 0).all()
        assert np.array_equal(r["x"][1:], r2["x"][1:]) and np.abs(r["x"][0] - r2["x"][0]).max() > 1e-6
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- 7. the resident loop
def test_the_loop_runs_on_the_contact_plant_and_keeps_it(model, oracle):
    case = loop_case(model, batch=B)
    g = grounds(oracle, model, case["x0"], mus=(0.3, 0.6, 1.0))      # (the soles of the loop's start states stand 3 .. 7 mm above z = 0)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        s.set_plant(**GAINS)
        loop_start(s, model, case)
        plain = s.loop_run(2)
        s.set_contact(stiffness=4e4)
        s.set_contact_instances(g)
        want = by_hand(s, model, case, 2, "feedforward")         # the ground survives the uploads
        loop_start(s, model, case)                               # ... and the start of a loop
        got = s.loop_run(2)
        assert s.get_contact()["enabled"]
        s.loop_isolate(s.episode_settings("reset"), x_reset=case["x0"])
        s.loop_reset([1])
        c = s.get_contact()
        assert c["enabled"] and c["stiffness"] == 4e4 and c["damping"] == 10.0 and c["mu"] == model.desc.friction_mu and c["slip_velocity"] == 0.01
        f, _ = s.contact_forces(case["x0"])                      # the table too: every instance stands on its own ground
        assert (f[:, :, :, 2].sum(axis=(1, 2)) > 0.0).all()
        s.set_contact_instances(None)                            # ... and without it on the setting's, at z = 0 below the soles
        assert not s.contact_forces(case["x0"])[0].any()
    finally:
        s.close()
    assert got["cycles_done"] == 2 and np.isfinite(got["x"]).all()
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])
    assert not np.array_equal(got["x"], plain["x"])


# ---------------------------------------------------------------------------------------------- 8. errors
def test_errors(model, cmodel):
    c = HipSqpSolver(cmodel, max_nodes=N, max_batch=B)
    try:
        for call in (lambda: c.set_contact(mu=0.5), lambda: c.set_contact_instances([(0.0, 0.5)]), lambda: c.contact_forces(np.zeros((1, NX)))):
            with pytest.raises(HsqpError) as ei:
                call()
            assert ei.value.code == _abi.ERR_BAD_ARG and "hsqp_contact_" in str(ei.value) and "whole-body handles only" in str(ei.value)
    finally:
        c.close()
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)

    def refused(what, **kw):
        st = s.contact_settings(**kw)
        rc = s.lib.hsqp_contact_set(s.h, C.byref(st))
        msg = s.lib.hsqp_last_error(s.h).decode()
        assert rc == _abi.ERR_BAD_ARG and "hsqp_contact_set" in msg and what in msg, (what, rc, msg)

    def refused_table(what, ground, batch=None, entry="hsqp_contact_set_instances"):
        g = np.ascontiguousarray(ground, dtype=float).reshape(-1, 2)
        rc = s.lib.hsqp_contact_set_instances(s.h, len(g) if batch is None else batch, C.cast(g.ctypes.data_as(C.POINTER(C.c_double)), C.POINTER(_abi.ContactGround)))
        msg = s.lib.hsqp_last_error(s.h).decode()
        assert rc == _abi.ERR_BAD_ARG and entry in msg and what in msg, (what, rc, msg)
    try:
        d = s.get_contact()
        assert not d["enabled"] and d["mu"] == model.desc.friction_mu and d["stiffness"] == 5e4
        st = s.contact_settings()
        assert st.enabled == 1 and st.mu == model.desc.friction_mu       # the defaults take the model's friction coefficient
        err = lambda: s.lib.hsqp_last_error(s.h).decode()   # noqa: E731
        assert s.lib.hsqp_contact_set(s.h, None) == _abi.ERR_BAD_ARG and "hsqp_contact_set" in err() and "null" in err()
        assert s.lib.hsqp_contact_get(s.h, None) == _abi.ERR_BAD_ARG and "hsqp_contact_get" in err() and "null" in err()
        assert s.lib.hsqp_contact_eval(s.h, 1, None, None, None) == _abi.ERR_BAD_ARG and "hsqp_contact_eval" in err() and "null" in err()
        assert s.lib.hsqp_contact_eval_device(s.h, 1, None, None, None) == _abi.ERR_BAD_ARG and "hsqp_contact_eval_device" in err()
        refused("reserved", reserved=1)
        for name in ("stiffness", "damping", "mu", "slip_velocity", "ground_height"):
            refused("non-finite", **{name: np.nan})
            refused("non-finite", **{name: np.inf})
        refused("stiffness", stiffness=0.0)
        refused("stiffness", stiffness=-1.0)
        refused("damping", damping=-1e-3)
        refused("mu", mu=-0.1)
        refused("slip_velocity", slip_velocity=0.0)
        refused("slip_velocity", slip_velocity=-0.01)
        assert not s.get_contact()["enabled"]                    # no refused call left a setting behind
        z = np.zeros((B + 1, 2))
        refused_table("batch", z[:1], batch=0)
        refused_table("batch", z, batch=B + 1)
        refused_table("instance 1", [(0.0, 0.5), (np.nan, 0.5)])
        refused_table("instance 2", [(0.0, 0.5), (0.0, 0.5), (0.0, np.inf)])
        refused_table("instance 0", [(0.0, -0.5)])
        x = np.zeros((B + 1, NX))
        for batch in (0, B + 1):
            assert s.lib.hsqp_contact_eval(s.h, batch, x.ctypes.data_as(C.POINTER(C.c_double)), None, None) == _abi.ERR_BAD_ARG
            assert "hsqp_contact_eval" in err() and "batch" in err()
        s.set_contact(damping=0.0, mu=0.0, ground_height=-0.5)   # the edges of the allowed ranges
        g = s.get_contact()
        assert g["enabled"] and g["damping"] == 0.0 and g["mu"] == 0.0 and g["ground_height"] == -0.5
        s.clear_contact()
        assert not s.get_contact()["enabled"] and s.get_contact()["ground_height"] == 0.0
    finally:
        s.close()
