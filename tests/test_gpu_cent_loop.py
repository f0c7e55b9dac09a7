"""The centroidal velocity-command targets and the centroidal resident loop (include/hsqp_cent_loop.h) on the GPU: k_command_targets_cent against the
numpy mirror (reference.centroidal_velocity_command_targets, reference.centroidal_base_velocity — the yardstick), and the loop started by
hsqp_loop_start_centroidal against the public calls it replaces, bit for bit.

Bounds: targets and base velocity 1e-12 absolute (the bound tests/test_device_params.py sets for the centroidal node table, whose torso velocity goes
through the same solve; the knots multiply the base velocity by at most 0.35 horizon); the filter state bit-equal (no transcendental).
Shapes: B <= 8, N = 12."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_gpu_feedback_policy import DeviceBuffer
from test_cent_loop import CNX, NJ, NX, mirror, random_cases
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import centroidal_velocity_command_targets, pack_reference, pad_targets, swing_config, tile_gait
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NU = _abi.NU
B, N, CYCLES, PERIOD = 4, 12, 4, 0.01
ATOL = 1e-12
ALIVE, NUMERIC, ROLLOUT, BOUNDS = _abi.EP_ALIVE, _abi.EP_FAILED_NUMERIC, _abi.EP_FAILED_ROLLOUT, _abi.EP_FAILED_BOUNDS
_dp = C.POINTER(C.c_double)
_p = lambda a: a.ctypes.data_as(_dp)  # noqa: E731


@pytest.fixture(scope="module")
def small(cmodel):
    s = HipSqpSolver(cmodel, max_nodes=N, max_batch=8, linesearch=True)
    yield s
    s.close()


def batch_of(cases):
    return (np.stack([c[3] for c in cases]), np.stack([c[4] for c in cases]), np.stack([c[5] for c in cases]))


# ---------------------------------------------------------------------------------------------- 1. device against the mirror
@pytest.mark.parametrize("alpha", [0.0, 0.8])
@pytest.mark.parametrize("batch", [1, 3, 8])
def test_device_against_the_mirror(small, cmodel, batch, alpha):
    cmd, vf, x0 = batch_of(random_cases(cmodel, batch, 31 + batch))
    tt, ts, vf_new, bv = small.command_targets(cmd, x0, 1.25, 2.0, filter_alpha=alpha, v_filt=vf, base_velocity=True)
    err_t = err_s = err_b = 0.0
    for b in range(batch):
        wt, ws, wvf, wbv = mirror(cmodel, alpha, 1.25, 2.0, cmd[b], vf[b], x0[b])
        err_t, err_s, err_b = max(err_t, np.abs(tt[b] - wt).max()), max(err_s, np.abs(ts[b] - ws).max()), max(err_b, np.abs(bv[b] - wbv).max())
        assert np.array_equal(vf_new[b], wvf)
    print("mirror", batch, alpha, err_t, err_s, err_b)
    assert err_t <= ATOL and err_s <= ATOL and err_b <= ATOL
    assert np.all(ts[:, :, CNX:] == 0.0) and np.all(ts[:, :, 10:12] == 0.0) and np.array_equal(ts[:, 0, 8], vf_new[:, 2])
    # without the by-product: the same targets
    tt2, ts2, vf2 = small.command_targets(cmd, x0, 1.25, 2.0, filter_alpha=alpha, v_filt=vf)
    assert np.array_equal(tt2, tt) and np.array_equal(ts2, ts) and np.array_equal(vf2, vf_new)


# ---------------------------------------------------------------------------------------------- 2. host entry = device twin
def test_host_entry_equals_the_device_twin(small, cmodel):
    cmd, vf, x0 = batch_of(random_cases(cmodel, 8, 5))
    tt, ts, vf_new, bv = small.command_targets(cmd, x0, 0.5, 1.1, filter_alpha=0.8, v_filt=vf, base_velocity=True)
    d = [DeviceBuffer(a.shape) for a in (cmd, vf, x0, tt, ts, bv)]
    try:
        for buf, a in zip(d[:3], (cmd, vf, x0)):
            buf.upload(a)
        small.command_targets_device(8, d[0].ptr.value, d[1].ptr.value, d[2].ptr.value, 0.5, 1.1, d[3].ptr.value, d[4].ptr.value, filter_alpha=0.8,
                                     base_vel_ptr=d[5].ptr.value)
        assert np.array_equal(d[3].numpy(), tt) and np.array_equal(d[4].numpy(), ts) and np.array_equal(d[1].numpy(), vf_new) and np.array_equal(d[5].numpy(), bv)
        d[1].upload(vf)
        small.command_targets_device(8, d[0].ptr.value, d[1].ptr.value, d[2].ptr.value, 0.5, 1.1, d[3].ptr.value, d[4].ptr.value, filter_alpha=0.8)   # no by-product
        assert np.array_equal(d[4].numpy(), ts) and np.array_equal(d[1].numpy(), vf_new)
    finally:
        for buf in d:
            buf.free()


# ---------------------------------------------------------------------------------------------- 3. batch independence
def test_an_instance_does_not_depend_on_its_place_in_the_batch(small, cmodel):
    cmd, vf, x0 = batch_of(random_cases(cmodel, 8, 39))
    tt, ts, vf_new, bv = small.command_targets(cmd, x0, 1.25, 2.0, filter_alpha=0.8, v_filt=vf, base_velocity=True)
    for b in range(8):
        t1, s1, f1, b1 = small.command_targets(cmd[b], x0[b], 1.25, 2.0, filter_alpha=0.8, v_filt=vf[b], base_velocity=True)
        assert np.array_equal(t1[0], tt[b]) and np.array_equal(s1[0], ts[b]) and np.array_equal(f1[0], vf_new[b]) and np.array_equal(b1[0], bv[b]), b


# ---------------------------------------------------------------------------------------------- 4. the loop against the calls it replaces
def loop_case(cmodel, batch=B, seed=20261020):
    rng = np.random.default_rng(seed)
    dt = cmodel.sqp["dt"]
    t_final = 2 * 8 * PERIOD + N * dt + 1.0
    schedules = [tile_gait(cmodel.gaits["walk"], 0.3 + 0.5 * b / batch, t_final) for b in range(batch)]
    dummy = pad_targets(centroidal_velocity_command_targets(cmodel, (0.0, 0.0, 0.79, 0.0), 0.0, cmodel.initial_state, 1.0))
    ne, ev, seq = pack_reference(schedules, [dummy] * batch)[:3]
    x0 = np.zeros((batch, NX))
    x0[:, :CNX] = cmodel.initial_state
    x0[:, 12:CNX] += 0.01 * rng.standard_normal((batch, NJ))
    x0[:, 9] += 0.05 * rng.standard_normal(batch)
    cmd = np.column_stack([rng.uniform(0.0, 0.5, batch), rng.uniform(-0.1, 0.1, batch), rng.uniform(0.77, 0.8, batch), rng.uniform(-0.2, 0.2, batch)])
    return dict(ne=ne, ev=ev, seq=seq, x0=x0, cmd=cmd)


def by_hand(s, cmodel, case, cycles, alpha=0.8, integrator="ode45", controller="feedforward", commands=None):
    """The cycles driven from Python through the public calls: hsqp_centroidal_command_targets, hsqp_upload_reference (cold, then shift),
    hsqp_iterate_device, hsqp_rollout_policy.  commands: {cycle: new commands} in effect from that cycle on."""
    dt, sw = cmodel.sqp["dt"], swing_config(cmodel)
    x, cmd = case["x0"].copy(), case["cmd"].copy()
    vf, t = cmd.copy(), 0.0
    xs, us = [], []
    for c in range(cycles):
        if commands and c in commands:
            cmd = commands[c].copy()
        tt, ts, vf = s.command_targets(cmd, x, t, N * dt, filter_alpha=alpha, v_filt=vf)
        s.upload_reference_warm(x, N, dt, t, case["ne"], case["ev"], case["seq"], tt, ts, sw, mode="cold" if c == 0 else "shift")
        s.iterate(1, take_step=True, linesearch=True)
        r = s.rollout_policy(np.zeros(len(x)), x, PERIOD, 1, integrator=integrator, controller=controller)
        x = r["x"][:, 0].copy()
        xs.append(x)
        us.append(r["u"][:, 0].copy())
        t += PERIOD
    X, U = s.device_trajectory()
    return dict(x=np.array(xs), u=np.array(us), vf=vf, t=t, X=X, U=U, stamps=s.stamps())


def settings(s, cmodel, alpha=0.8, integrator="ode45", controller="feedforward"):
    return s.loop_settings(N, cmodel.sqp["dt"], period=PERIOD, filter_alpha=alpha, iterations=1, take_step=True, linesearch=True, integrator=integrator,
                           controller=controller)


def start(s, cmodel, case, rows=slice(None), x0=None, **kw):
    s.loop_start(settings(s, cmodel, **kw), 0.0, case["x0"][rows] if x0 is None else x0, case["cmd"][rows], case["ne"][rows], case["ev"][rows], case["seq"][rows])


def resident(s):
    return (*s.device_trajectory(), s.stamps())


@pytest.mark.parametrize("integrator,controller", [("ode45", "feedforward"), ("rk4", "feedback")])
def test_loop_equals_the_calls_it_replaces(cmodel, integrator, controller):
    case = loop_case(cmodel)
    s = HipSqpSolver(cmodel, max_nodes=N, max_batch=B, linesearch=True)
    try:
        want = by_hand(s, cmodel, case, CYCLES, integrator=integrator, controller=controller)
        start(s, cmodel, case, integrator=integrator, controller=controller)
        got = s.loop_run(CYCLES)
        t, x, vf = s.loop_state()
        X, U, stamps = resident(s)
    finally:
        s.close()
    assert got["cycles_done"] == CYCLES and np.isfinite(got["x"]).all() and np.isfinite(got["u"]).all()
    assert not np.array_equal(want["x"][0, 0], want["x"][0, 1])                    # distinct instances
    assert np.all(got["x"][:, :, CNX:] == 0.0)                                     # the padding of every logged state
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])
    assert np.array_equal(vf, want["vf"]) and np.array_equal(x, want["x"][-1]) and t == want["t"]
    assert np.array_equal(X, want["X"]) and np.array_equal(U, want["U"]) and np.array_equal(stamps, want["stamps"])


# ---------------------------------------------------------------------------------------------- 5. commands and chaining
def test_new_commands_take_effect_with_the_next_cycle_and_runs_chain(cmodel):
    case = loop_case(cmodel)
    cmd2 = case["cmd"] + np.array([0.3, 0.05, 0.0, 0.1])
    s = HipSqpSolver(cmodel, max_nodes=N, max_batch=B, linesearch=True)
    try:
        start(s, cmodel, case)
        one = s.loop_run(4)
        one_state, one_res = s.loop_state(), resident(s)
        start(s, cmodel, case)
        a, b = s.loop_run(2), s.loop_run(2)
        two_state, two_res = s.loop_state(), resident(s)
        start(s, cmodel, case)
        c = s.loop_run(2)
        s.loop_command(cmd2)
        d = s.loop_run(2)
        switched_vf = s.loop_state()[2]
        want = by_hand(s, cmodel, case, 4, commands={2: cmd2})
    finally:
        s.close()
    assert np.array_equal(np.concatenate([a["x"], b["x"]]), one["x"]) and np.array_equal(np.concatenate([a["u"], b["u"]]), one["u"])
    assert one_state[0] == two_state[0] and all(np.array_equal(p, q) for p, q in zip(one_state[1:], two_state[1:]))
    assert all(np.array_equal(p, q) for p, q in zip(one_res, two_res))
    assert np.array_equal(c["x"], one["x"][:2]) and np.array_equal(c["u"], one["u"][:2])
    assert not np.array_equal(d["x"][0], one["x"][2])
    assert np.array_equal(np.concatenate([c["x"], d["x"]]), want["x"]) and np.array_equal(np.concatenate([c["u"], d["u"]]), want["u"])
    assert np.array_equal(switched_vf, want["vf"])


# ---------------------------------------------------------------------------------------------- 6. isolation
SICK = 2
HEALTHY = np.array([b for b in range(B) if b != SICK])


@pytest.mark.parametrize("policy", ["park", "reset"])
def test_a_failed_instance_is_isolated_and_restarted(cmodel, policy):
    case = loop_case(cmodel)
    bad = case["x0"].copy()
    bad[SICK, 12 + 7] = np.nan                                               # a joint angle
    s = HipSqpSolver(cmodel, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        start(s, cmodel, case, rows=HEALTHY)
        s.loop_isolate(s.episode_settings(policy), x_reset=case["x0"][HEALTHY])
        want = s.loop_run(3)
        want_state = s.loop_state()
        start(s, cmodel, case, x0=bad)
        s.loop_isolate(s.episode_settings(policy), x_reset=case["x0"])
        got = s.loop_run(3)
        got_state, ep = s.loop_state(), s.loop_episodes()
        # the host restarts it
        s.loop_reset(np.array([SICK], np.int32), x0=case["x0"][SICK:SICK + 1])
        after = s.loop_run(1)
        ep_after = s.loop_episodes()
    finally:
        s.close()
    assert want["cycles_done"] == 3 and got["cycles_done"] == 3 and np.isfinite(want["x"]).all()
    assert np.array_equal(got["x"][:, HEALTHY], want["x"]) and np.array_equal(got["u"][:, HEALTHY], want["u"])
    assert got_state[0] == want_state[0] and np.array_equal(got_state[1][HEALTHY], want_state[1]) and np.array_equal(got_state[2][HEALTHY], want_state[2])
    print("episodes", ep)
    assert ep["cause"][SICK] in (NUMERIC, ROLLOUT) and ep["fail_cycle"][SICK] == 0 and ep["n_failures"][SICK] == 1
    assert np.isnan(got["x"][0, SICK]).all() and np.isfinite(got_state[1]).all()
    assert (ep["state"][HEALTHY] == ALIVE).all() and (ep["n_failures"][HEALTHY] == 0).all()
    if policy == "park":
        assert ep["state"][SICK] == ep["cause"][SICK] and ep["n_episodes"][SICK] == 1 and np.isnan(got["x"][:, SICK]).all()
        stance = np.array([0.0, 0.0, case["x0"][SICK, 8], 0.0])              # the stance command takes the height of the centroidal pose
        want_vf = stance.copy()
        for _ in range(2):
            want_vf = 0.8 * want_vf + (1.0 - 0.8) * stance
        assert np.array_equal(got_state[2][SICK], want_vf)
    else:
        assert ep["state"][SICK] == ALIVE and ep["n_episodes"][SICK] == 2 and np.isfinite(got["x"][1:, SICK]).all()
    assert ep_after["state"][SICK] == ALIVE and ep_after["n_episodes"][SICK] == ep["n_episodes"][SICK] + 1 and np.isfinite(after["x"]).all()


def test_the_height_box_is_read_at_the_centroidal_pose(cmodel):
    """Instance SICK starts 4 cm below the standing height h0, the floor lies at h0 - 2 cm: it fails the bounds in cycle 0.  Every instance's x[2] — a
    momentum entry, about zero — lies below the floor: read at the whole-body index, every instance would fail."""
    case = loop_case(cmodel)
    h0 = float(cmodel.initial_state[8])
    low = case["x0"].copy()
    low[SICK, 8] = h0 - 0.04
    floor = h0 - 0.02
    s = HipSqpSolver(cmodel, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        start(s, cmodel, case, x0=low)
        plain = s.loop_run(3)
        start(s, cmodel, case, x0=low)
        s.loop_isolate(s.episode_settings("park", min_base_height=floor, max_tilt=1.0), x_reset=case["x0"])
        got = s.loop_run(3)
        ep = s.loop_episodes()
    finally:
        s.close()
    z = plain["x"][:, :, 8]
    print("base heights without isolation", z.min(axis=0), z.max(axis=0), "x[2]", plain["x"][:, :, 2].max())
    assert (z[:, HEALTHY] > floor).all() and z[0, SICK] < floor and (plain["x"][:, :, 2] < floor).all()      # the scenario is what it is meant to be
    assert ep["cause"][SICK] == BOUNDS and ep["state"][SICK] == BOUNDS and ep["fail_cycle"][SICK] == 0
    assert (ep["state"][HEALTHY] == ALIVE).all() and (ep["n_failures"][HEALTHY] == 0).all()
    assert np.array_equal(got["x"][:, HEALTHY], plain["x"][:, HEALTHY]) and np.isnan(got["x"][:, SICK]).all()


# ---------------------------------------------------------------------------------------------- 7. refusals
def refused(fn, *text):
    with pytest.raises(HsqpError) as ei:
        fn()
    assert ei.value.code == _abi.ERR_BAD_ARG and all(t in str(ei.value) for t in text), str(ei.value)


def test_refusals(model, cmodel, small):
    case = loop_case(cmodel)
    lib = small.lib
    ip = C.POINTER(C.c_int32)
    ne, seq = np.ascontiguousarray(case["ne"], np.int32), np.ascontiguousarray(case["seq"], np.int32)
    ev, x0, cmd = np.ascontiguousarray(case["ev"]), case["x0"].copy(), np.ascontiguousarray(case["cmd"])
    E = ev.shape[1]
    tt, ts, vf = np.zeros((B, 3)), np.zeros((B, 3, NX)), cmd.copy()
    # the new entries on a whole-body handle
    wb = HipSqpSolver(model, max_nodes=N, max_batch=B)
    try:
        st = settings(wb, model)
        xw = np.tile(model.initial_state, (B, 1))
        for rc in (lib.hsqp_centroidal_command_targets(wb.h, B, _p(cmd), _p(vf), 0.0, _p(xw), 0.0, 1.0, _p(tt), _p(ts), None),
                   lib.hsqp_centroidal_command_targets_device(wb.h, B, _p(cmd), _p(vf), 0.0, _p(xw), 0.0, 1.0, _p(tt), _p(ts), None),
                   lib.hsqp_loop_start_centroidal(wb.h, C.byref(st), B, 0.0, _p(xw), _p(cmd), E, ne.ctypes.data_as(ip), _p(ev), seq.ctypes.data_as(ip))):
            assert rc == _abi.ERR_BAD_ARG and "centroidal handles only" in lib.hsqp_last_error(wb.h).decode()
    finally:
        wb.close()
    # the whole-body entries on the centroidal handle still refuse
    st = settings(small, cmodel)
    for rc in (lib.hsqp_command_targets(small.h, B, _p(cmd), _p(vf), 0.0, _p(x0), 0.0, 1.0, _p(tt), _p(ts)),
               lib.hsqp_loop_start(small.h, C.byref(st), B, 0.0, _p(x0), _p(cmd), E, ne.ctypes.data_as(ip), _p(ev), seq.ctypes.data_as(ip))):
        assert rc == _abi.ERR_BAD_ARG and "whole-body handles only" in lib.hsqp_last_error(small.h).decode()
    # padding, arguments
    pad = x0.copy()
    pad[1, 40] = 1e-300
    refused(lambda: small.command_targets(cmd, pad, 0.0, 1.0), "entries 35..57 of every state row must be zero")
    refused(lambda: small.loop_start(st, 0.0, pad, cmd, ne, ev, seq), "entries 35..57 of every state row must be zero")
    refused(lambda: small.command_targets(cmd, x0, 0.0, 1.0, filter_alpha=1.0), "filter_alpha")
    refused(lambda: small.command_targets(cmd, x0, 0.0, 0.0), "horizon")
    refused(lambda: small.command_targets(cmd, x0, np.inf, 1.0), "t0")
    nan_cmd = cmd.copy()
    nan_cmd[0, 1] = np.nan
    refused(lambda: small.command_targets(nan_cmd, x0, 0.0, 1.0), "non-finite command")
    refused(lambda: small.loop_start(st, 0.0, x0, nan_cmd, ne, ev, seq), "non-finite command")
    assert lib.hsqp_centroidal_command_targets(small.h, 0, _p(cmd), _p(vf), 0.0, _p(x0), 0.0, 1.0, _p(tt), _p(ts), None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_centroidal_command_targets(small.h, 9, _p(cmd), _p(vf), 0.0, _p(x0), 0.0, 1.0, _p(tt), _p(ts), None) == _abi.ERR_BAD_ARG
    assert "batch outside" in lib.hsqp_last_error(small.h).decode()
    assert lib.hsqp_centroidal_command_targets(small.h, B, None, _p(vf), 0.0, _p(x0), 0.0, 1.0, _p(tt), _p(ts), None) == _abi.ERR_BAD_ARG
    assert "null array" in lib.hsqp_last_error(small.h).decode()
    bad_st = settings(small, cmodel)
    bad_st.n_nodes = N + 1
    refused(lambda: small.loop_start(bad_st, 0.0, x0, cmd, ne, ev, seq), "n_nodes")
    bad_ne = ne.copy()
    bad_ne[0] = E + 1
    refused(lambda: small.loop_start(st, 0.0, x0, cmd, bad_ne, ev, seq), "n_events")
    # a gait on a centroidal solver reaches hsqp_loop_start_gait and is refused there
    from wb_humanoid_mpc_amd.reference import gait_settings
    refused(lambda: small.loop_start(st, 0.0, x0, cmd, gait=gait_settings(model)), "whole-body handles only")
    # no default joint state: a handle of its own, made without the binding's constructor
    h = C.c_void_p()
    hs = _abi.Settings(max_nodes=N, max_batch=B, device=0, flags=0)
    assert lib.hsqp_create(C.byref(cmodel.desc), C.byref(hs), C.byref(h)) == 0
    try:
        assert lib.hsqp_centroidal_command_targets(h, B, _p(cmd), _p(vf), 0.0, _p(x0), 0.0, 1.0, _p(tt), _p(ts), None) == _abi.ERR_BAD_ARG
        assert "no default joint state" in lib.hsqp_last_error(h).decode()
        assert lib.hsqp_loop_start_centroidal(h, C.byref(st), B, 0.0, _p(x0), _p(cmd), E, ne.ctypes.data_as(ip), _p(ev), seq.ctypes.data_as(ip)) == _abi.ERR_BAD_ARG
        assert "no default joint state" in lib.hsqp_last_error(h).decode()
    finally:
        lib.hsqp_destroy(h)
    # after a start: what stays whole-body only, and the padding of reset states
    small.loop_start(st, 0.0, x0, cmd, ne, ev, seq)
    for rc in (lib.hsqp_loop_event_grid(small.h, None), lib.hsqp_loop_ground(small.h, None, None), lib.hsqp_loop_perceive(small.h, None),
               lib.hsqp_loop_metrics_enable(small.h)):
        assert rc == _abi.ERR_BAD_ARG and "whole-body handles only" in lib.hsqp_last_error(small.h).decode()
    refused(lambda: small.loop_isolate(small.episode_settings("park"), x_reset=pad), "entries 35..57")
    small.loop_isolate(small.episode_settings("park"), x_reset=x0)
    refused(lambda: small.loop_reset(np.array([1], np.int32), x0=pad[1:2]), "entries 35..57")


# ---------------------------------------------------------------------------------------------- 8. the C++ wrapper
def test_cpp_wrapper_runs_the_centroidal_loop(tmp_path, cmodel):
    case = loop_case(cmodel)
    s = HipSqpSolver(cmodel, max_nodes=N, max_batch=B, linesearch=True)
    try:
        st = settings(s, cmodel)
        start(s, cmodel, case)
        want = s.loop_run(2)["x"][-1]
    finally:
        s.close()
    libdir = os.path.join(ROOT, "wb_humanoid_mpc_amd")
    exe = tmp_path / "cent_loop_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(libdir, "host"), os.path.join(ROOT, "tests", "cent_loop", "cent_loop_driver.cpp"),
                           "-L", libdir, "-lhsqp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", str(exe)])
    (tmp_path / "desc.bin").write_bytes(bytes(cmodel.desc))
    (tmp_path / "settings.bin").write_bytes(bytes(st))
    E = case["ev"].shape[1]
    doubles = np.concatenate([[float(B), float(E)], cmodel.default_joint_state, case["x0"].ravel(), case["cmd"].ravel(), np.asarray(case["ev"], dtype=float).ravel()])
    (tmp_path / "doubles.bin").write_bytes(doubles.astype(np.float64).tobytes())
    ints = np.concatenate([np.asarray(case["ne"], np.int32).ravel(), np.asarray(case["seq"], np.int32).ravel()])
    (tmp_path / "ints.bin").write_bytes(ints.astype(np.int32).tobytes())
    r = subprocess.run([str(exe)] + [str(tmp_path / n) for n in ("desc.bin", "settings.bin", "doubles.bin", "ints.bin")] + [str(N)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr)
    got = np.array([float.fromhex(v) for v in r.stdout.split()]).reshape(B, NX)
    assert np.array_equal(got, want)
