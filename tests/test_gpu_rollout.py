"""The batched policy rollout (include/hsqp_rollout.h) on the MI355X: RK4 against the numpy restatement on the CPU oracle's flow maps with the
downloaded policy, ODE45 against an independent tight solution (scipy DOP853 segmented at every node stamp and event), agreement with the
policy entry points, chaining, batch order and the device entry point bit for bit, validity and argument errors, a closed receding-horizon
loop, and the C++ adaptor's rolloutPolicy."""
import os
import subprocess

import numpy as np
import pytest
from scipy.integrate import solve_ivp

import rollout_ref as R
from test_gpu_feedback_policy import DeviceBuffer
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import make_centroidal_problem, make_problem, pack_reference, swing_config, tile_gait, velocity_command_targets
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu
NX, NU, CNX = _abi.NX, _abi.NU, _abi.CNX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "wb_humanoid_mpc_amd")
B = 4
N = 20


def event_dts(dt, n):
    dts = np.full(n, dt)
    dts[[4, 9, 10, 15]] = 0.0          # an event, and two in a row
    return dts


def solved(m, cent, grid, batch=B, seed=3, perm=None):
    """A solver holding one successful iteration of a perturbed problem: (solver, downloaded solution, dts, x0 [B][58])."""
    x0, x, u, par, dt = (make_centroidal_problem if cent else make_problem)(m, n_nodes=N, batch=batch, perturb=True, seed=seed)
    if perm is not None:
        x0, x, u, par = x0[perm], x[perm], u[perm], par[perm]
    dts = event_dts(dt, N) if grid == "events" else np.full(N, dt)
    s = HipSqpSolver(m, max_nodes=N, max_batch=batch)
    out = s.run(x0, x, u, par, dts if grid == "events" else dt)
    return s, out, dts, dt, x0


def policies(s, out, dts, dt, grid, cent):
    K, uff = s.feedback_policy()
    return [R.Policy(out["u"][b], dt, dts if grid == "events" else None, K[b], uff[b], 0, cent) for b in range(out["u"].shape[0])]


def start(x0, cent, seed=0):
    rng = np.random.default_rng(seed)
    x = x0.copy()
    nl = CNX if cent else NX
    x[:, :nl] += 0.01 * rng.standard_normal((len(x), nl))
    if cent:
        x[:, CNX:] = 0.0
    return x


S0 = np.array([0.0, 0.01, 0.023, 0.05])
S0_EVENTS = np.array([0.0, 0.135, 0.27, 0.45])  # (dt = 0.035) the last three windows of 1/60 s hold the event stamps 0.14, 0.28 (twice), 0.455
CASES = [(f, g, c) for f in ("wb", "centroidal") for g in ("uniform", "events") for c in ("feedforward", "feedback")]


@pytest.mark.parametrize("formulation,grid,controller", CASES)
def test_rk4_matches_the_oracle(model, cmodel, oracle, coracle, formulation, grid, controller):
    cent = formulation == "centroidal"
    m = cmodel if cent else model
    s, out, dts, dt, x0 = solved(m, cent, grid)
    try:
        s0 = S0 if grid == "uniform" else S0_EVENTS
        xs = start(x0, cent)
        r = s.rollout_policy(s0, xs, 1.0 / 60.0, 1, integrator="rk4", controller=controller, initial_step=0.001)
        assert (r["status"] == 0).all() and (r["rejected"] == 0).all()
        pols = policies(s, out, dts, dt, grid, cent)
        flow = R.cent_flow(coracle) if cent else R.wb_flow(oracle)
        st = R.settings(R.RK4, R.FEEDBACK if controller == "feedback" else R.FEEDFORWARD, initial_step=0.001)
        for b in range(B):
            xr, ur, sr, nr, _ = R.rollout(flow, pols[b], st, s0[b], xs[b], 1.0 / 60.0, 1)
            assert sr == R.OK and r["steps"][b] == nr
            err = np.abs(r["x"][b, 0] - xr[0]).max() / max(1.0, np.abs(xr[0]).max())
            assert err <= 1e-10, (b, err)
            assert np.abs(r["u"][b, 0] - ur[0]).max() <= 1e-9 * max(1.0, np.abs(ur[0]).max())
    finally:
        s.close()


def tight_solution(flow, pol, controller, s0, x0, duration):
    """scipy DOP853 at rtol = atol = 1e-12, restarted at every node stamp and event inside the interval (the input has kinks there)."""
    dts = pol.dts if pol.dts is not None else np.full(pol.N, pol.dt)
    stamps = np.concatenate([[0.0], np.cumsum(dts)])
    cuts = [s0] + sorted({t for t in stamps if s0 < t < s0 + duration}) + [s0 + duration]
    nl = CNX if pol.cent else NX
    x = np.asarray(x0[:nl], dtype=float)

    def rhs(t, y):
        xx = np.zeros(NX)
        xx[:nl] = y
        return flow(xx, pol.control(t, xx, controller))[:nl]
    for a, b in zip(cuts[:-1], cuts[1:]):
        # the restart at a stamp starts on the side the controller takes after it (the post-event node)
        x = solve_ivp(rhs, (a, b), x, method="DOP853", rtol=1e-12, atol=1e-12).y[:, -1]
    out = np.zeros(NX)
    out[:nl] = x
    return out


@pytest.mark.parametrize("formulation,grid,controller", [("wb", "uniform", "feedforward"), ("wb", "events", "feedback"), ("centroidal", "uniform", "feedback")])
def test_ode45_against_a_tight_solution(model, cmodel, oracle, coracle, formulation, grid, controller):
    cent = formulation == "centroidal"
    m = cmodel if cent else model
    s, out, dts, dt, x0 = solved(m, cent, grid)
    try:
        s0 = S0 if grid == "uniform" else S0_EVENTS
        xs = start(x0, cent, 1)
        pols = policies(s, out, dts, dt, grid, cent)
        flow = R.cent_flow(coracle) if cent else R.wb_flow(oracle)
        ctl = R.FEEDBACK if controller == "feedback" else R.FEEDFORWARD
        refs = [tight_solution(flow, pols[b], ctl, s0[b], xs[b], 1.0 / 60.0) for b in range(B)]
        r = s.rollout_policy(s0, xs, 1.0 / 60.0, 1, controller=controller)
        assert (r["status"] == 0).all()
        assert (r["steps"] < 10000 * 1.0).all()
        r2 = s.rollout_policy(s0, xs, 1.0 / 60.0, 1, controller=controller, abs_tol=1e-10, rel_tol=1e-10)
        assert (r2["status"] == 0).all() and (r2["steps"] > r["steps"]).all()
        for b in range(B):
            assert np.abs(r2["x"][b, 0] - refs[b]).max() <= 1e-7, (b, np.abs(r2["x"][b, 0] - refs[b]).max())
        # the step control bounds the LOCAL error of a step by the tolerance.  A window without a node stamp inside stays within 10 x the
        # tolerance; one that crosses a stamp (a kink of the interpolated controller, which ODE45 steps over as ocs2's does, or an event)
        # was measured up to 11.6 x (wb, uniform, s0 = 0.023) and 22.8 x (wb, events, feedback, s0 = 0.45): bound 50 x there
        stamps = np.concatenate([[0.0], np.cumsum(dts if grid == "events" else np.full(N, dt))])
        ratios = [float((np.abs(r["x"][b, 0] - refs[b]) / (1e-5 + 1e-3 * np.abs(refs[b]))).max()) for b in range(B)]
        for b in range(B):
            kink = ((stamps > s0[b]) & (stamps < s0[b] + 1.0 / 60.0)).any()
            assert ratios[b] <= (50.0 if kink else 10.0), (b, kink, ratios)
        print(f"{formulation} {grid} {controller}: steps {r['steps']} rejected {r['rejected']} error / tolerance {np.round(ratios, 2)}; "
              f"tight steps {r2['steps']}")
    finally:
        s.close()


@pytest.mark.parametrize("formulation,grid", [("wb", "uniform"), ("wb", "events"), ("centroidal", "events")])
def test_agreement_with_the_policy_entry_points(model, cmodel, formulation, grid):
    cent = formulation == "centroidal"
    m = cmodel if cent else model
    s, out, dts, dt, x0 = solved(m, cent, grid)
    try:
        s0 = np.array([0.0, 2.0 ** -6, 2.0 ** -4, 2.0 ** -3])
        d = 2.0 ** -6
        xs = start(x0, cent, 2)
        for controller in ("feedforward", "feedback"):
            for integrator in ("ode45", "rk4"):
                r = s.rollout_policy(s0, xs, 4 * d, 4, integrator=integrator, controller=controller, initial_step=0.004 if integrator == "rk4" else 0.015)
                assert (r["status"] == 0).all()
                for j in range(4):
                    t = s0 + (j + 1) * d
                    if controller == "feedforward":
                        _, u, _ = s.evaluate_policy(t)
                        assert np.array_equal(r["u"][:, j], u), j
                    else:
                        _, u, _ = s.evaluate_feedback_policy(t, r["x"][:, j])
                        assert np.abs(r["u"][:, j] - u).max() <= 1e-13 * max(1.0, np.abs(u).max()), j
                # four chained calls
                xc, steps = xs.copy(), np.zeros(B, np.int64)
                for j in range(4):
                    rj = s.rollout_policy(s0 + j * d, xc, d, 1, integrator=integrator, controller=controller,
                                          initial_step=0.004 if integrator == "rk4" else 0.015)
                    assert np.array_equal(rj["x"][:, 0], r["x"][:, j]) and np.array_equal(rj["u"][:, 0], r["u"][:, j]), (controller, integrator, j)
                    xc = rj["x"][:, 0]
                    steps += rj["steps"]
                assert np.array_equal(steps, r["steps"])
            # the device entry point writes the same bits
            bufs = dict(s0=DeviceBuffer((B,)), x0=DeviceBuffer((B, NX)), x=DeviceBuffer((B, 4, NX)), u=DeviceBuffer((B, 4, NU)), st=DeviceBuffer((B,)),
                        steps=DeviceBuffer((B,)), rej=DeviceBuffer((B,)))
            try:
                bufs["s0"].upload(s0)
                bufs["x0"].upload(xs)
                r = s.rollout_policy(s0, xs, 4 * d, 4, controller=controller)
                rc = s.rollout_policy_device(bufs["s0"].ptr.value, bufs["x0"].ptr.value, 4 * d, 4, bufs["x"].ptr.value, bufs["u"].ptr.value,
                                             bufs["st"].ptr.value, bufs["steps"].ptr.value, bufs["rej"].ptr.value, controller=controller)
                assert rc == 0
                assert np.array_equal(bufs["x"].numpy(), r["x"]) and np.array_equal(bufs["u"].numpy(), r["u"])
                ints = lambda buf: np.frombuffer(buf.numpy().tobytes()[:4 * B], dtype=np.int32)  # noqa: E731
                assert np.array_equal(ints(bufs["st"]), r["status"]) and np.array_equal(ints(bufs["steps"]), r["steps"])
                assert np.array_equal(ints(bufs["rej"]), r["rejected"])
            finally:
                for bb in bufs.values():
                    bb.free()
    finally:
        s.close()


def test_batch_order_does_not_matter(model):
    perm = np.array([2, 0, 3, 1])
    s, out, _, _, x0 = solved(model, False, "events")
    sp, outp, _, _, _ = solved(model, False, "events", perm=perm)
    try:
        assert np.array_equal(outp["x"], out["x"][perm]) and np.array_equal(outp["u"], out["u"][perm])
        s0 = S0_EVENTS
        xs = start(x0, False, 4)
        for controller in ("feedforward", "feedback"):
            r = s.rollout_policy(s0, xs, 1.0 / 60.0, 2, controller=controller)
            rp = sp.rollout_policy(s0[perm], xs[perm], 1.0 / 60.0, 2, controller=controller)
            for k in ("x", "u", "status", "steps", "rejected"):
                assert np.array_equal(rp[k], r[k][perm]), (controller, k)
    finally:
        s.close()
        sp.close()


def test_validity_and_bad_arguments(model):
    x0, x, u, par, dt = make_problem(model, n_nodes=N, batch=2, perturb=True, seed=5)
    s = HipSqpSolver(model, max_nodes=N, max_batch=2)
    twin = HipSqpSolver(model, max_nodes=N, max_batch=2)
    try:
        s.upload(x0, x, u, par, dt)
        twin.upload(x0, x, u, par, dt)

        def bad(**kw):
            args = dict(s0=np.zeros(2), x0=x0, duration=1.0 / 60.0, n_samples=1)
            args.update(kw)
            with pytest.raises(HsqpError) as ei:
                s.rollout_policy(**args)
            assert ei.value.code == _abi.ERR_BAD_ARG, kw
        bad()                                       # after an upload, before any iteration
        s.iterate(1, take_step=True)
        twin.iterate(1, take_step=True)
        s.rollout_policy(np.zeros(2), x0, 1.0 / 60.0)  # valid now
        for kw in (dict(duration=-1e-3), dict(duration=np.inf), dict(n_samples=0), dict(abs_tol=0.0), dict(rel_tol=-1.0), dict(initial_step=0.0),
                   dict(max_steps_per_second=0.0), dict(s0=np.array([0.0, np.nan])), dict(s0=np.array([np.inf, 0.0])), dict(integrator=7),
                   dict(controller=-1)):
            bad(**kw)
        # the failed calls left the resident solution alone: the next iteration gives the bits of the twin that never saw them
        a, b = s.download(), twin.download()
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["u"], b["u"])
        s.iterate(1, take_step=True)
        twin.iterate(1, take_step=True)
        a, b = s.download(), twin.download()
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["u"], b["u"])
        s.upload(x0, x, u, par, dt)
        bad()                                       # an upload invalidates the policy
    finally:
        s.close()
        twin.close()


def closed_loop(m, Bn, Nn, cycles, period=1.0 / 60.0):
    dt = m.sqp["dt"]
    t_final = cycles * period + Nn * dt + 1.0
    schedules = [tile_gait(m.gaits["walk"], 0.3 + 0.5 * b / Bn, t_final) for b in range(Bn)]
    targets = velocity_command_targets(m, (0.3, 0.0, 0.7925, 0.0), 0.0, m.initial_state, t_final)
    ref = pack_reference(schedules, [targets] * Bn)
    rng = np.random.default_rng(20250808)
    x_init = np.tile(m.initial_state, (Bn, 1))
    x_init[:, 6:6 + m.nj] += 0.01 * rng.standard_normal((Bn, m.nj))
    sw = swing_config(m)
    s = HipSqpSolver(m, max_nodes=Nn, max_batch=Bn, linesearch=True)
    s.set_scan_backoff_persistent(True)
    heights, xs, t = [], [], 0.0
    try:
        for c in range(cycles):
            s.upload_reference_warm(x_init, Nn, dt, t, *ref, sw, mode="cold" if c == 0 else "shift")
            s.iterate(1, take_step=True, linesearch=True)
            r = s.rollout_policy(np.zeros(Bn), x_init, period, 1)
            assert (r["status"] == 0).all(), c
            x_init = r["x"][:, 0]
            assert np.isfinite(x_init).all() and np.isfinite(r["u"]).all()
            heights.append(x_init[:, 2].copy())
            xs.append(x_init.copy())
            t += period
    finally:
        s.close()
    return np.array(heights), np.array(xs), targets


def test_closed_loop(model):
    h1, x1, targets = closed_loop(model, 8, 40, 20)
    h2, x2, _ = closed_loop(model, 8, 40, 20)
    z = 0.7925                                     # the commanded base height of the targets
    assert np.abs(h1 - z).max() <= 0.1, (h1.min(), h1.max(), z)
    assert np.array_equal(x1, x2)


def test_adaptor_rollout_policy(tmp_path, model):
    from test_adaptor import write_case
    exe = tmp_path / "adaptor_rollout_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs", "ocs2"), "-I", os.path.join(LIBDIR, "host"),
                           "-I", os.path.join(ROOT, "tests", "adaptor"), os.path.join(ROOT, "tests", "adaptor_rollout", "adaptor_rollout_driver.cpp"),
                           "-L", LIBDIR, "-lhsqp_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", str(exe)])
    schedule = tile_gait(model.gaits["walk"], 0.3, 6.0)
    targets = velocity_command_targets(model, (0.3, 0.0, 0.7925, 0.0), 0.0, model.initial_state, 3.0)
    write_case(tmp_path, model, schedule, targets, model.initial_state, 1.05, 0.02, 2, _abi.NX)
    image = os.path.join(LIBDIR, "data", "g1_wb.json")
    for fb in ("0", "1"):
        r = subprocess.run([str(exe), image, str(tmp_path / "case.txt"), str(tmp_path / "out.txt"), fb], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (fb, r.returncode, r.stdout, r.stderr)
        assert "rollout ok" in r.stdout, r.stdout
