"""The velocity-command targets and the resident closed loop (include/hsqp_loop.h) on the GPU: k_command_targets against the fixtures of the
reference-compiled generator and the numpy mirror, and hsqp_loop_run against the public calls it replaces — bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_feedback_policy import DeviceBuffer
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import pack_reference, swing_config, tile_gait, velocity_command_targets
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "ref_terms.npz"))
NX, NU, NJ = _abi.NX, _abi.NU, _abi.NJ
B, N, CYCLES, PERIOD = 8, 20, 5, 1.0 / 60.0
# parameters generated on the device: the bound tests/test_device_params.py sets (fixture states are at most 1.3 and times at most 6.6 in
# magnitude, so two ulp of a device sin / cos stay three orders below it)
ATOL_DEVICE = 1e-13


@pytest.fixture(scope="module")
def small(model):
    s = HipSqpSolver(model, max_nodes=N, max_batch=64, linesearch=True)
    yield s
    s.close()


def test_command_targets_against_the_reference_fixtures(small, model):
    for c, x0, h, t0, tt, ts in zip(G["tgt.cmd"], G["tgt.x0"], G["tgt.horizon"], G["tgt.t0"], G["tgt.times"], G["tgt.states"]):
        got_t, got_s, vf = small.command_targets(c, x0, float(t0), float(h), filter_alpha=0.0, v_filt=np.full(4, 1e300))
        print("fixture", np.abs(got_t[0] - tt).max(), np.abs(got_s[0] - ts).max())
        np.testing.assert_allclose(got_t[0], tt, rtol=0, atol=ATOL_DEVICE)
        np.testing.assert_allclose(got_s[0], ts, rtol=0, atol=ATOL_DEVICE)
        assert np.array_equal(vf[0], c)
    # the first-call transient of the reference's static filter, as tests/golden/make_ref_terms_golden.py recorded it
    _, got_s, _ = small.command_targets((5.0, 0.0, 0.7925, 0.0), model.initial_state, 0.0, 2.0, filter_alpha=0.8, v_filt=G["tgt.cmd"][-1])
    print("first call", np.abs(got_s[0] - G["tgt.first_call_states"]).max())
    np.testing.assert_allclose(got_s[0], G["tgt.first_call_states"], rtol=0, atol=ATOL_DEVICE)


def random_cases(model, n, seed):
    rng = np.random.default_rng(seed)
    x0 = np.tile(model.initial_state, (n, 1)) + 0.05 * rng.standard_normal((n, NX))
    x0[:, 3] = rng.uniform(-1.2, 1.2, n)                               # yaw
    cmd = np.column_stack([rng.uniform(-0.5, 0.8, n), rng.uniform(-0.2, 0.2, n), rng.uniform(0.7, 0.8, n), rng.uniform(-0.4, 0.4, n)])
    vf = cmd + 0.1 * rng.standard_normal((n, 4))
    return x0, cmd, vf


@pytest.mark.parametrize("alpha", [0.0, 0.8])
def test_command_targets_against_the_mirror(small, model, alpha):
    x0, cmd, vf = random_cases(model, 64, 11)
    tt, ts, vf_new = small.command_targets(cmd, x0, 1.25, 2.0, filter_alpha=alpha, v_filt=vf)
    err_t = err_s = err_f = 0.0
    for b in range(64):
        f = vf[b].copy()
        ref = velocity_command_targets(model, tuple(cmd[b]), 1.25, x0[b], 2.0, filter_alpha=alpha, v_filt=f)
        err_t = max(err_t, np.abs(tt[b] - np.asarray(ref.times)).max())
        err_s = max(err_s, np.abs(ts[b] - np.asarray(ref.states)).max())
        err_f = max(err_f, np.abs(vf_new[b] - f).max())
    print("mirror", alpha, err_t, err_s, err_f)
    assert err_t <= ATOL_DEVICE and err_s <= ATOL_DEVICE and err_f == 0.0      # (the filter has no transcendental in it)


def test_command_targets_device_twin(small, model):
    x0, cmd, vf = random_cases(model, 16, 5)
    tt, ts, vf_new = small.command_targets(cmd, x0, 0.5, 1.1, filter_alpha=0.8, v_filt=vf)
    d = [DeviceBuffer(a.shape) for a in (cmd, vf, x0, tt, ts)]
    try:
        for buf, a in zip(d[:3], (cmd, vf, x0)):
            buf.upload(a)
        small.command_targets_device(16, d[0].ptr.value, d[1].ptr.value, d[2].ptr.value, 0.5, 1.1, d[3].ptr.value, d[4].ptr.value, filter_alpha=0.8)
        assert np.array_equal(d[3].numpy(), tt) and np.array_equal(d[4].numpy(), ts) and np.array_equal(d[1].numpy(), vf_new)
    finally:
        for buf in d:
            buf.free()


# ---------------------------------------------------------------------------------------------- the loop against the calls it replaces
def loop_case(model, batch=B, seed=20260116):
    rng = np.random.default_rng(seed)
    t_final = 2 * CYCLES * PERIOD + N * model.sqp["dt"] + 1.0
    schedules = [tile_gait(model.gaits["walk"], 0.3 + 0.5 * b / batch, t_final) for b in range(batch)]
    dummy = velocity_command_targets(model, (0.0, 0.0, 0.79, 0.0), 0.0, model.initial_state, 1.0)
    ne, ev, seq = pack_reference(schedules, [dummy] * batch)[:3]
    x0 = np.tile(model.initial_state, (batch, 1))
    x0[:, 6:6 + NJ] += 0.01 * rng.standard_normal((batch, NJ))
    x0[:, 3] += 0.05 * rng.standard_normal(batch)
    cmd = np.column_stack([rng.uniform(0.0, 0.5, batch), rng.uniform(-0.1, 0.1, batch), rng.uniform(0.77, 0.8, batch), rng.uniform(-0.2, 0.2, batch)])
    return dict(ne=ne, ev=ev, seq=seq, x0=x0, cmd=cmd)


def by_hand(s, model, case, cycles, alpha=0.8, integrator="ode45", controller="feedforward", commands=None, rows=slice(None)):
    """The cycles driven from Python through the public calls: hsqp_command_targets, hsqp_upload_reference (cold, then shift),
    hsqp_iterate_device, hsqp_rollout_policy.  commands: {cycle: new commands} in effect from that cycle on."""
    dt, sw = model.sqp["dt"], swing_config(model)
    x, cmd = case["x0"][rows].copy(), case["cmd"][rows].copy()
    vf, t = cmd.copy(), 0.0
    xs, us = [], []
    for c in range(cycles):
        if commands and c in commands:
            cmd = commands[c][rows].copy()
        tt, ts, vf = s.command_targets(cmd, x, t, N * dt, filter_alpha=alpha, v_filt=vf)
        s.upload_reference_warm(x, N, dt, t, case["ne"][rows], case["ev"][rows], case["seq"][rows], tt, ts, sw, mode="cold" if c == 0 else "shift")
        s.iterate(1, take_step=True, linesearch=True)
        r = s.rollout_policy(np.zeros(len(x)), x, PERIOD, 1, integrator=integrator, controller=controller)
        x = r["x"][:, 0].copy()
        xs.append(x)
        us.append(r["u"][:, 0].copy())
        t += PERIOD
    X, U = s.device_trajectory()
    return dict(x=np.array(xs), u=np.array(us), vf=vf, t=t, X=X, U=U, stamps=s.stamps())


def start(s, model, case, alpha=0.8, integrator="ode45", controller="feedforward", rows=slice(None), x0=None):
    st = s.loop_settings(N, model.sqp["dt"], period=PERIOD, filter_alpha=alpha, iterations=1, take_step=True, linesearch=True, integrator=integrator,
                         controller=controller)
    s.loop_start(st, 0.0, case["x0"][rows] if x0 is None else x0, case["cmd"][rows], case["ne"][rows], case["ev"][rows], case["seq"][rows])


def resident(s):
    X, U = s.device_trajectory()
    return X, U, s.stamps()


@pytest.mark.parametrize("integrator,controller", [("ode45", "feedforward"), ("ode45", "feedback"), ("rk4", "feedforward"), ("rk4", "feedback")])
def test_loop_equals_the_calls_it_replaces(model, integrator, controller):
    case = loop_case(model)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True)
    try:
        want = by_hand(s, model, case, CYCLES, integrator=integrator, controller=controller)
        start(s, model, case, integrator=integrator, controller=controller)
        got = s.loop_run(CYCLES)
        t, x, vf = s.loop_state()
        X, U, stamps = resident(s)
    finally:
        s.close()
    assert got["cycles_done"] == CYCLES and np.isfinite(got["x"]).all() and np.isfinite(got["u"]).all()
    assert not np.array_equal(want["x"][0, 0], want["x"][0, 1])                    # distinct instances
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])
    assert np.array_equal(vf, want["vf"]) and np.array_equal(x, want["x"][-1]) and t == want["t"]
    assert np.array_equal(X, want["X"]) and np.array_equal(U, want["U"]) and np.array_equal(stamps, want["stamps"])


def test_new_commands_take_effect_with_the_next_cycle_and_runs_chain(model):
    case = loop_case(model)
    cmd2 = case["cmd"] + np.array([0.3, 0.05, 0.0, 0.1])
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True)
    try:
        start(s, model, case)
        one = s.loop_run(5)
        one_state, one_res = s.loop_state(), resident(s)
        start(s, model, case)
        a, b = s.loop_run(3), s.loop_run(2)
        two_state, two_res = s.loop_state(), resident(s)
        start(s, model, case)
        c = s.loop_run(3)
        s.loop_command(cmd2)
        d = s.loop_run(2)
        switched_vf = s.loop_state()[2]
        want = by_hand(s, model, case, 5, commands={3: cmd2})
        # the device twins: commands, logs and state in device memory
        bufs = [DeviceBuffer(sh) for sh in ((B, 4), (2, B, NX), (2, B, NU), (B, NX), (B, 4))]
        try:
            start(s, model, case)
            s.loop_run(3, log=False)
            bufs[0].upload(cmd2)
            s.loop_command_device(bufs[0].ptr.value)
            assert s.loop_run_device(2, bufs[1].ptr.value, bufs[2].ptr.value) == 2
            t_dev = s.loop_state_device(bufs[3].ptr.value, bufs[4].ptr.value)
            dev = [buf.numpy() for buf in bufs]
        finally:
            for buf in bufs:
                buf.free()
    finally:
        s.close()
    # 3 + 2 cycles are 5 cycles
    assert np.array_equal(np.concatenate([a["x"], b["x"]]), one["x"]) and np.array_equal(np.concatenate([a["u"], b["u"]]), one["u"])
    assert one_state[0] == two_state[0] and all(np.array_equal(p, q) for p, q in zip(one_state[1:], two_state[1:]))
    assert all(np.array_equal(p, q) for p, q in zip(one_res, two_res))
    # the new commands change cycle 3 and nothing before it
    assert np.array_equal(c["x"], one["x"][:3]) and np.array_equal(c["u"], one["u"][:3])
    assert not np.array_equal(d["x"][0], one["x"][3])
    assert np.array_equal(np.concatenate([c["x"], d["x"]]), want["x"]) and np.array_equal(np.concatenate([c["u"], d["u"]]), want["u"])
    assert np.array_equal(switched_vf, want["vf"])
    assert np.array_equal(dev[1], d["x"]) and np.array_equal(dev[2], d["u"]) and np.array_equal(dev[3], d["x"][-1]) and np.array_equal(dev[4], switched_vf)
    assert t_dev == want["t"]


def test_instances_are_independent(model):
    """Instance 3 of the batch of 8 equals the same instance run alone, on handles that always take the serial recursion (the default sweep is
    chosen by batch size, so without the flag the two runs would not take the same path)."""
    case = loop_case(model)
    rows = slice(3, 4)
    out = []
    for r in (slice(None), rows):
        s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
        try:
            start(s, model, case, rows=r)
            got = s.loop_run(CYCLES)
            out.append((got["x"], got["u"], s.loop_state()[2], *resident(s)))
        finally:
            s.close()
    for k, (whole, alone) in enumerate(zip(*out)):
        assert np.array_equal(whole[:, 3:4] if k < 2 else whole[3:4], alone), k      # (the logs are [cycle][instance], the rest [instance])


def test_a_failed_cycle_stops_the_loop(model):
    """A NaN in one instance's start state (the input tests/test_gpu_parity.py feeds the iteration: it must surface as NUMERIC, not hang): the loop
    ends in the first cycle with the code the public calls give, no cycle is counted, the state is the start state, and a new start runs."""
    case = loop_case(model)
    bad = case["x0"].copy()
    bad[2, 7] = np.nan
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True)
    try:
        with pytest.raises(HsqpError) as by_calls:
            by_hand(s, model, dict(case, x0=bad), 1)
        start(s, model, case, x0=bad)
        with pytest.raises(HsqpError) as e:
            s.loop_run(3)
        assert e.value.code == by_calls.value.code == _abi.ERR_NUMERIC, (e.value.code, by_calls.value.code, str(e.value))
        assert e.value.result["cycles_done"] == 0 and e.value.result["x"].shape[0] == 0
        t, x, vf = s.loop_state()
        assert t == 0.0 and np.array_equal(x, bad, equal_nan=True) and np.array_equal(vf, case["cmd"])
        start(s, model, case)
        got = s.loop_run(2)
        assert got["cycles_done"] == 2 and np.isfinite(got["x"]).all()
        want = by_hand(s, model, case, 2)
        assert np.array_equal(got["x"], want["x"])
    finally:
        s.close()


def test_bad_arguments(model, cmodel):
    case = loop_case(model)
    dt = model.sqp["dt"]
    c = HipSqpSolver(cmodel, max_nodes=8, max_batch=2)
    try:
        lib, p = c.lib, np.zeros(3 * NX).ctypes.data_as(C.POINTER(C.c_double))
        i = np.ones(2, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
        st = _abi.LoopSettings()
        lib.hsqp_loop_defaults(c.h, C.byref(st))
        assert st.n_nodes == 8
        done = C.c_int(0)
        for rc in (lib.hsqp_command_targets(c.h, 1, p, p, 0.0, p, 0.0, 1.0, p, p), lib.hsqp_command_targets_device(c.h, 1, p, p, 0.0, p, 0.0, 1.0, p, p),
                   lib.hsqp_loop_start(c.h, C.byref(st), 1, 0.0, p, p, 1, i, p, i)):
            assert rc == _abi.ERR_BAD_ARG and b"whole-body handles only" in lib.hsqp_last_error(c.h)
        for rc in (lib.hsqp_loop_run(c.h, 1, None, None, C.byref(done)), lib.hsqp_loop_command(c.h, p), lib.hsqp_loop_state(c.h, None, None, None)):
            assert rc == _abi.ERR_BAD_ARG and lib.hsqp_last_error(c.h)
    finally:
        c.close()
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True)
    try:
        def refused(what, **kw):
            with pytest.raises(HsqpError) as e:
                what(**kw)
            assert e.value.code == _abi.ERR_BAD_ARG and str(e.value), kw
        with pytest.raises(HsqpError) as e:      # no loop yet
            s.loop_run(1)
        assert e.value.code == _abi.ERR_BAD_ARG and "hsqp_loop_start" in str(e.value)
        refused(s.loop_command, v_cmd=case["cmd"])
        refused(s.loop_state)
        ok = dict(n_nodes=N, dt=dt, period=PERIOD, filter_alpha=0.8)
        for change in (dict(n_nodes=N + 1), dict(n_nodes=0), dict(period=0.0), dict(period=float("nan")), dict(period=float("inf")), dict(dt=-1.0),
                       dict(dt=float("nan")), dict(filter_alpha=1.0), dict(filter_alpha=-0.1), dict(filter_alpha=float("nan")), dict(iterations=0),
                       dict(integrator=7), dict(abs_tol=0.0)):
            st = s.loop_settings(**dict(ok, **change))
            refused(s.loop_start, settings=st, t0=0.0, x0=case["x0"], v_cmd=case["cmd"], n_events=case["ne"], event_times=case["ev"], mode_sequence=case["seq"])
        st = s.loop_settings(**ok)
        st.iterate_flags |= 8                     # HSQP_ITER_UNTIL_CONVERGED
        refused(s.loop_start, settings=st, t0=0.0, x0=case["x0"], v_cmd=case["cmd"], n_events=case["ne"], event_times=case["ev"], mode_sequence=case["seq"])
        st = s.loop_settings(**ok)
        good = dict(settings=st, t0=0.0, x0=case["x0"], v_cmd=case["cmd"], n_events=case["ne"], event_times=case["ev"], mode_sequence=case["seq"])
        nan_cmd = case["cmd"].copy()
        nan_cmd[1, 0] = np.nan
        refused(s.loop_start, **dict(good, v_cmd=nan_cmd))
        refused(s.loop_start, **dict(good, t0=float("nan")))
        refused(s.loop_start, **dict(good, n_events=np.zeros(B, np.int32)))
        big = np.tile(case["x0"], (2, 1))         # batch over max_batch
        refused(s.loop_start, settings=st, t0=0.0, x0=big, v_cmd=np.tile(case["cmd"], (2, 1)), n_events=np.tile(case["ne"], 2), event_times=np.tile(case["ev"], (2, 1)),
                mode_sequence=np.tile(case["seq"], (2, 1)))
        lib = s.lib
        p = case["x0"].ctypes.data_as(C.POINTER(C.c_double))
        i = case["ne"].ctypes.data_as(C.POINTER(C.c_int32))
        assert lib.hsqp_loop_start(s.h, C.byref(st), B, 0.0, None, p, 1, i, p, i) == _abi.ERR_BAD_ARG and lib.hsqp_last_error(s.h)
        assert lib.hsqp_loop_start(s.h, None, B, 0.0, p, p, 1, i, p, i) == _abi.ERR_BAD_ARG and lib.hsqp_last_error(s.h)
        refused(s.command_targets, v_cmd=nan_cmd, x0=case["x0"], t0=0.0, horizon=1.0)
        refused(s.command_targets, v_cmd=case["cmd"], x0=case["x0"], t0=0.0, horizon=0.0)
        refused(s.command_targets, v_cmd=case["cmd"], x0=case["x0"], t0=0.0, horizon=1.0, filter_alpha=1.0)
        refused(s.command_targets, v_cmd=np.tile(case["cmd"], (2, 1)), x0=big, t0=0.0, horizon=1.0)
        # a started loop: bad run / command arguments, and every upload ends it
        s.loop_start(**good)
        refused(s.loop_run, n_cycles=0)
        refused(s.loop_command, v_cmd=nan_cmd)
        assert lib.hsqp_loop_command(s.h, None) == _abi.ERR_BAD_ARG
        assert s.loop_run(1)["cycles_done"] == 1
        tt, ts, _ = s.command_targets(case["cmd"], case["x0"], 0.0, N * dt)
        s.upload_reference_warm(case["x0"], N, dt, 0.0, case["ne"], case["ev"], case["seq"], tt, ts, swing_config(model), mode="shift")
        with pytest.raises(HsqpError) as e:
            s.loop_run(1)
        assert e.value.code == _abi.ERR_BAD_ARG and "ends a loop" in str(e.value)
        s.loop_start(**good)
        assert s.loop_run(1)["cycles_done"] == 1
    finally:
        s.close()


# what `bench.py --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline --sustained 0 --dump-outputs DIR` (BASELINE config 4: 256 x 100) wrote on the commit
# before the loop existed: the first 16 hex digits of the SHA-256 of every array's bytes (profiles/device_loop_cycle.txt has the two runs side by side)
PARENT_DUMP = {"x": "00a433cfb82d5dff", "u": "2e5d2f7e247294d2", "dx": "c4cca7d4e9f324d7", "du": "55b306454426aef2",
               "perf_before": "390566942ee1ecb2", "perf_after": "c5407981d8c6fd82"}


def test_bench_outputs_are_the_parents(tmp_path):
    """Additions only: the iteration computes bit for bit what it computed before include/hsqp_loop.h existed."""
    import hashlib
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "3", "--no-cpu-baseline", "--sustained", "0",
                        "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    got = {k: hashlib.sha256(np.load(tmp_path / "dump" / (k + ".npy")).tobytes()).hexdigest()[:16] for k in PARENT_DUMP}
    print(got)
    assert got == PARENT_DUMP
