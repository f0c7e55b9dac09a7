"""Per-instance failure isolation and episode reset of the resident loop (include/hsqp_episode.h) on the GPU.  Everything is held to "bit for
bit": the instances of a batch are arithmetically independent on the serial sweep (tests/test_gpu_loop.py::test_instances_are_independent), so
no tolerance has to be chosen.  The handles take the serial recursion on request, so a batch, the batch without one instance and a one-instance
loop take the same path.  The only sick input is NaN data, the means tests/test_gpu_loop.py uses; every test runs under a time limit of its own."""
import ctypes as C
import signal

import numpy as np
import pytest

from test_gpu_loop import loop_case
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import gait_settings
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu

NX, NU = _abi.NX, _abi.NU
B, N, PERIOD, CYC, SICK = 5, 20, 1.0 / 60.0, 6, 2          # (N: the horizon tests/test_gpu_loop.py::loop_case tiles its schedules for)
ALIVE, NUMERIC, ROLLOUT, BOUNDS = _abi.EP_ALIVE, _abi.EP_FAILED_NUMERIC, _abi.EP_FAILED_ROLLOUT, _abi.EP_FAILED_BOUNDS
HEALTHY = np.array([b for b in range(B) if b != SICK])


@pytest.fixture(autouse=True)
def time_limit():
    def expired(signum, frame):
        raise TimeoutError("test_gpu_episode: a test ran past its 300 s limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(300)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture
def s(model):
    h = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    yield h
    h.close()


def start(s, model, case, gait, rows=slice(None), t0=0.0, x0=None, cmd=None):
    """A loop on the instances `rows` of the case (x0 / cmd: their states / commands instead of the case's), with the resident gait or the case's schedules"""
    st = s.loop_settings(N, model.sqp["dt"], period=PERIOD, filter_alpha=0.8, iterations=1, take_step=True, linesearch=True)
    x0 = case["x0"][rows] if x0 is None else x0
    cmd = case["cmd"][rows] if cmd is None else cmd
    if gait:
        s.loop_start(st, t0, x0, cmd, gait=gait_settings(model))
    else:
        s.loop_start(st, t0, x0, cmd, case["ne"][rows], case["ev"][rows], case["seq"][rows])


def snapshot(s, gait):
    """where the loop stands: (t, x, v_filt) and the gait state's arrays"""
    t, x, vf = s.loop_state()
    g = s.gait_state() if gait else {}
    return dict(t=t, x=x, vf=vf, **g)


def assert_rows_equal(got, want, rows_got, rows_want=slice(None)):
    """the logs are [cycle][instance], a snapshot's arrays [instance]"""
    for k in want:
        if k == "t":
            assert got[k] == want[k]
        else:
            assert np.array_equal(got[k][rows_got], want[k][rows_want]), k


def sick_start(case):
    bad = case["x0"].copy()
    bad[SICK, 7] = np.nan
    return bad


# ---------------------------------------------------------------------------------------------- 1. nobody fails
@pytest.mark.parametrize("gait", [False, True])
@pytest.mark.parametrize("policy", ["park", "reset"])
def test_isolation_changes_nothing_when_nobody_fails(s, model, gait, policy):
    case = loop_case(model, batch=B)
    start(s, model, case, gait)
    off = s.loop_run(CYC)
    off_state, off_res = snapshot(s, gait), (*s.device_trajectory(), s.stamps())
    start(s, model, case, gait)
    s.loop_isolate(s.episode_settings(policy))
    on = s.loop_run(CYC - 2)
    more = s.loop_run(2)
    on_state, on_res = snapshot(s, gait), (*s.device_trajectory(), s.stamps())
    ep = s.loop_episodes()
    assert off["cycles_done"] == CYC and on["cycles_done"] + more["cycles_done"] == CYC and np.isfinite(off["x"]).all()
    assert np.array_equal(np.concatenate([on["x"], more["x"]]), off["x"]) and np.array_equal(np.concatenate([on["u"], more["u"]]), off["u"])
    assert_rows_equal(on_state, off_state, slice(None))
    assert all(np.array_equal(a, b) for a, b in zip(on_res, off_res))
    assert (ep["state"] == ALIVE).all() and (ep["cause"] == ALIVE).all() and (ep["fail_cycle"] == -1).all() and (ep["n_failures"] == 0).all() and (ep["n_episodes"] == 1).all()


# ---------------------------------------------------------------------------------------------- 2. isolation
@pytest.mark.parametrize("gait", [False, True])
def test_a_failed_instance_is_parked_and_the_others_go_on(s, model, gait):
    """Instance SICK starts from a state with a NaN (PARK, x_reset = the case's finite start): the run completes with HSQP_OK, and the healthy
    instances equal, bit for bit, the loop run on them alone.  Without include/hsqp_episode.h the loop returns HSQP_ERR_NUMERIC with cycles_done == 0
    (tests/test_gpu_loop.py::test_a_failed_cycle_stops_the_loop)."""
    case = loop_case(model, batch=B)
    start(s, model, case, gait, rows=HEALTHY)
    want = s.loop_run(CYC)
    want_state = snapshot(s, gait)
    assert want["cycles_done"] == CYC and np.isfinite(want["x"]).all()
    start(s, model, case, gait, x0=sick_start(case))
    s.loop_isolate(s.episode_settings("park"), x_reset=case["x0"])
    got = s.loop_run(CYC)                                       # (raises unless HSQP_OK)
    got_state, ep = snapshot(s, gait), s.loop_episodes()
    assert got["cycles_done"] == CYC
    assert np.array_equal(got["x"][:, HEALTHY], want["x"]) and np.array_equal(got["u"][:, HEALTHY], want["u"])
    assert_rows_equal(got_state, want_state, HEALTHY)
    print("episodes", ep)
    assert ep["cause"][SICK] in (NUMERIC, ROLLOUT) and ep["fail_cycle"][SICK] == 0 and ep["state"][SICK] == ep["cause"][SICK]
    assert np.isnan(got["x"][:, SICK]).all() and np.isnan(got["u"][:, SICK]).all()          # parked: every row
    assert ep["n_failures"][SICK] == 1 and (ep["n_episodes"] == 1).all()                     # it ran on from x_reset without failing again
    assert (ep["state"][HEALTHY] == ALIVE).all() and (ep["n_failures"][HEALTHY] == 0).all() and (ep["fail_cycle"][HEALTHY] == -1).all()
    stance = np.array([0.0, 0.0, case["x0"][SICK, 2], 0.0])          # the filter seeded with the stance command, then advanced under it (csrc/hsqp_loop.h)
    want_vf = stance.copy()
    for _ in range(CYC - 1):
        want_vf = 0.8 * want_vf + (1.0 - 0.8) * stance
    assert np.isfinite(got_state["x"]).all() and np.array_equal(got_state["vf"][SICK], want_vf)
    # a new command does not reach the parked instance, and reaches the others
    s.loop_command(case["cmd"] + np.array([0.1, 0.0, 0.0, 0.0]))
    s.loop_run(1)
    vf = s.loop_state()[2]
    assert np.array_equal(vf[SICK], 0.8 * want_vf + (1.0 - 0.8) * stance) and not np.array_equal(vf[HEALTHY], got_state["vf"][HEALTHY])


# ---------------------------------------------------------------------------------------------- 3. RESET
@pytest.mark.parametrize("gait", [False, True])
def test_a_reset_instance_equals_a_fresh_loop_from_that_time(s, model, gait):
    case = loop_case(model, batch=B)
    start(s, model, case, gait, x0=sick_start(case))
    s.loop_isolate(s.episode_settings("reset"), x_reset=case["x0"])
    first = s.loop_run(1)
    t1 = s.loop_state()[0]
    rest = s.loop_run(CYC - 1)
    got_state, ep = snapshot(s, gait), s.loop_episodes()
    assert t1 == PERIOD and first["cycles_done"] == 1 and rest["cycles_done"] == CYC - 1
    assert np.isnan(first["x"][0, SICK]).all() and np.isnan(first["u"][0, SICK]).all() and np.isfinite(first["x"][0, HEALTHY]).all()
    assert ep["state"][SICK] == ALIVE and ep["cause"][SICK] in (NUMERIC, ROLLOUT) and ep["fail_cycle"][SICK] == 0
    assert ep["n_episodes"][SICK] == 2 and ep["n_failures"][SICK] == 1 and (ep["n_episodes"][HEALTHY] == 1).all()
    one = slice(SICK, SICK + 1)
    start(s, model, case, gait, rows=one, t0=t1)                # COLD in its first cycle, SHIFT after, the filter seeded with the command, the gait reset at t1
    fresh = s.loop_run(CYC - 1)
    fresh_state = snapshot(s, gait)
    assert np.isfinite(fresh["x"]).all()
    assert np.array_equal(rest["x"][:, one], fresh["x"]) and np.array_equal(rest["u"][:, one], fresh["u"])
    assert_rows_equal(got_state, fresh_state, one)


# ---------------------------------------------------------------------------------------------- 4. bounds
@pytest.mark.parametrize("gait", [False, True])
def test_the_callers_box(s, model, gait):
    """The chosen instance starts 4 cm below the standing height h0 and the box's floor lies at h0 - 2 cm: it leaves the box in cycle 0 (a floor just
    ABOVE h0 would be left by every instance at once, they all stand at h0).  Its start is finite, so the same batch runs without isolation too:
    the others equal that run bit for bit.  With RESET and x_reset = the low state it fails in every cycle: known counters."""
    case = loop_case(model, batch=B)
    h0 = float(model.initial_state[2])
    low = case["x0"].copy()
    low[SICK, 2] = h0 - 0.04
    floor = h0 - 0.02
    start(s, model, case, gait, x0=low)
    plain = s.loop_run(CYC)
    plain_state = snapshot(s, gait)
    z = plain["x"][:, :, 2]
    print("base heights without isolation", z.min(axis=0), z.max(axis=0))
    assert (z[:, HEALTHY] > floor).all() and z[0, SICK] < floor           # the scenario is what it is meant to be
    start(s, model, case, gait, x0=low)
    s.loop_isolate(s.episode_settings("park", min_base_height=floor), x_reset=case["x0"])
    got = s.loop_run(CYC)
    got_state, ep = snapshot(s, gait), s.loop_episodes()
    assert np.array_equal(got["x"][:, HEALTHY], plain["x"][:, HEALTHY]) and np.array_equal(got["u"][:, HEALTHY], plain["u"][:, HEALTHY])
    assert_rows_equal(got_state, plain_state, HEALTHY, HEALTHY)
    assert ep["cause"][SICK] == BOUNDS and ep["state"][SICK] == BOUNDS and ep["fail_cycle"][SICK] == 0 and ep["n_failures"][SICK] == 1
    assert (ep["state"][HEALTHY] == ALIVE).all() and np.isnan(got["x"][:, SICK]).all()
    # the ceiling and the tilt box: nobody is near them
    start(s, model, case, gait, x0=low)
    s.loop_isolate(s.episode_settings("park", max_base_height=h0 + 0.2, max_tilt=1.0), x_reset=case["x0"])
    assert np.array_equal(s.loop_run(CYC)["x"], plain["x"]) and (s.loop_episodes()["state"] == ALIVE).all()
    # RESET onto the low state: one failure per cycle
    start(s, model, case, gait, x0=low)
    s.loop_isolate(s.episode_settings("reset", min_base_height=floor), x_reset=low)
    got = s.loop_run(CYC)
    ep = s.loop_episodes()
    assert np.array_equal(got["x"][:, HEALTHY], plain["x"][:, HEALTHY]) and np.isnan(got["x"][:, SICK]).all()
    assert ep["n_failures"][SICK] == CYC and ep["n_episodes"][SICK] == CYC + 1 and ep["fail_cycle"][SICK] == CYC - 1 and ep["state"][SICK] == ALIVE and ep["cause"][SICK] == BOUNDS


# ---------------------------------------------------------------------------------------------- 5. host reset
@pytest.mark.parametrize("gait", [False, True])
def test_the_host_starts_new_episodes_on_chosen_instances(s, model, gait):
    case = loop_case(model, batch=B)
    rng = np.random.default_rng(7)
    moved, rest_ids, cut = np.array([3, 0], np.int32), np.array([1, 4]), 3
    new_x = np.tile(model.initial_state, (2, 1))
    new_x[:, 6:6 + _abi.NJ] += 0.01 * rng.standard_normal((2, _abi.NJ))
    new_cmd = np.array([[0.25, 0.05, 0.78, -0.1], [0.0, 0.0, 0.79, 0.15]])
    start(s, model, case, gait, rows=HEALTHY)
    undisturbed = s.loop_run(CYC)
    undisturbed_state = snapshot(s, gait)
    start(s, model, case, gait, x0=sick_start(case))
    s.loop_isolate(s.episode_settings("park"), x_reset=case["x0"])
    a = s.loop_run(cut)
    t_cut = s.loop_state()[0]
    assert s.loop_episodes()["state"][SICK] != ALIVE
    s.loop_reset(moved, x0=new_x, v_cmd=new_cmd)
    s.loop_reset([SICK])                                         # x_reset, the command it has
    mid = s.loop_episodes()
    assert (mid["state"] == ALIVE).all() and list(mid["n_episodes"]) == [2, 1, 2, 2, 1] and mid["fail_cycle"][SICK] == 0 and mid["n_failures"][SICK] == 1
    t_mid, x_mid, vf_mid = s.loop_state()
    assert t_mid == t_cut and np.array_equal(x_mid[moved], new_x) and np.array_equal(vf_mid[moved], new_cmd)
    assert np.array_equal(x_mid[SICK], case["x0"][SICK]) and np.array_equal(vf_mid[SICK], case["cmd"][SICK])
    b = s.loop_run(CYC - cut)
    got_state, ep = snapshot(s, gait), s.loop_episodes()
    assert (ep["state"] == ALIVE).all() and np.isfinite(b["x"]).all()
    # the rest: the undisturbed run on the healthy instances (HEALTHY is [0, 1, 3, 4]: instances 1 and 4 are its rows 1 and 3)
    whole_x, whole_u = np.concatenate([a["x"], b["x"]]), np.concatenate([a["u"], b["u"]])
    assert np.array_equal(whole_x[:, rest_ids], undisturbed["x"][:, [1, 3]]) and np.array_equal(whole_u[:, rest_ids], undisturbed["u"][:, [1, 3]])
    assert_rows_equal(got_state, undisturbed_state, rest_ids, [1, 3])
    assert np.array_equal(a["x"][:, moved], undisturbed["x"][:cut][:, [2, 0]])              # and the moved ones up to the reset
    # the moved instances and the parked one: fresh loops from t_cut
    for ids, x0, cmd in ((moved, new_x, new_cmd), (np.array([SICK]), case["x0"][[SICK]], case["cmd"][[SICK]])):
        start(s, model, case, gait, rows=ids, t0=t_cut, x0=x0, cmd=cmd)
        fresh = s.loop_run(CYC - cut)
        fresh_state = snapshot(s, gait)
        assert np.array_equal(b["x"][:, ids], fresh["x"]) and np.array_equal(b["u"][:, ids], fresh["u"]), ids
        assert_rows_equal(got_state, fresh_state, ids)


# ---------------------------------------------------------------------------------------------- 6. buffers laid out a second time
def test_a_restart_on_more_instances_equals_a_fresh_handle(s, model):
    """One handle, the resident gait: a loop on 2 instances, isolated, 2 cycles; then a loop on all B instances, isolated (the loop's, the gait's and
    the episodes' buffers are outgrown and laid out again: loop_layout, gait_layout, episode_layout of csrc/hsqp_capi.hip), 2 cycles, a host reset
    of instances [3, 0] with new states and commands, 2 more cycles.  Everything equals, bit for bit, a fresh handle taken through the B-instance
    part alone.
    Both handles lay their buffers out through the same function, so a request staging that lay on x_reset or on the command in use would be the
    same mistake on both.  Two checks therefore do not compare handles: the instances the request does not name equal a run without the request (a
    staging on the command in use leaves new_cmd[1] as instance 1's command), and at the end instance 1 restarts from its x_reset (a staging on
    x_reset leaves new_x[1] there)."""
    case = loop_case(model, batch=B)
    rng = np.random.default_rng(11)
    moved, rest = np.array([3, 0], np.int32), np.array([1, 2, 4])
    new_x = np.tile(model.initial_state, (2, 1))
    new_x[:, 6:6 + _abi.NJ] += 0.01 * rng.standard_normal((2, _abi.NJ))
    new_cmd = np.array([[0.2, -0.05, 0.78, 0.1], [0.1, 0.0, 0.79, -0.15]])

    def whole_batch_part(h):
        start(h, model, case, True)
        h.loop_isolate(h.episode_settings("park"))
        first = h.loop_run(2)
        h.loop_reset(moved, x0=new_x, v_cmd=new_cmd)
        last = h.loop_run(2)
        assert first["cycles_done"] == 2 and last["cycles_done"] == 2 and np.isfinite(last["x"]).all()
        return dict(state=snapshot(h, True), ep=h.loop_episodes(), x=last["x"], u=last["u"])

    start(s, model, case, True, rows=slice(0, 2))
    s.loop_isolate(s.episode_settings("park"))
    assert s.loop_run(2)["cycles_done"] == 2
    got = whole_batch_part(s)
    fresh = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        want = whole_batch_part(fresh)
        start(fresh, model, case, True)                          # the same four cycles without the request
        fresh.loop_isolate(fresh.episode_settings("park"))
        plain = fresh.loop_run(4)
        plain_state = snapshot(fresh, True)
    finally:
        fresh.close()
    assert_rows_equal(got["state"], want["state"], slice(None))
    assert sorted(got["ep"]) == ["cause", "fail_cycle", "n_episodes", "n_failures", "state"]
    for k in want["ep"]:
        assert np.array_equal(got["ep"][k], want["ep"][k]), k
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])
    assert (got["ep"]["state"] == ALIVE).all() and list(got["ep"]["n_episodes"]) == [2, 1, 1, 2, 1]
    # the instances the request does not name
    assert np.array_equal(got["x"][:, rest], plain["x"][2:][:, rest]) and np.array_equal(got["u"][:, rest], plain["u"][2:][:, rest])
    assert_rows_equal(got["state"], plain_state, rest, rest)
    # x_reset is still the start of the whole-batch loop
    s.loop_reset([1])
    assert np.array_equal(s.loop_state()[1][1], case["x0"][1])


# ---------------------------------------------------------------------------------------------- 7. bad arguments
def test_bad_arguments(s, model, cmodel):
    case = loop_case(model, batch=B)
    lib = s.lib
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    five = np.zeros(B, np.int32)
    i5 = five.ctypes.data_as(ip)

    def refused(what, *a, **kw):
        with pytest.raises(HsqpError) as e:
            what(*a, **kw)
        assert e.value.code == _abi.ERR_BAD_ARG and str(e.value), (a, kw)
        return str(e.value)
    # no loop started
    assert "hsqp_loop_start" in refused(s.loop_isolate)
    refused(s.loop_reset, [0])
    refused(s.loop_episodes)
    assert lib.hsqp_loop_episodes_device(s.h, i5, i5, i5, i5, i5) == _abi.ERR_BAD_ARG
    # a started loop without isolation
    start(s, model, case, False)
    assert "hsqp_loop_isolate" in refused(s.loop_reset, [0])
    refused(s.loop_episodes)
    # the settings
    assert lib.hsqp_loop_isolate(s.h, None, None) == _abi.ERR_BAD_ARG and lib.hsqp_last_error(s.h)
    bad = s.episode_settings("park")
    bad.on_failure = 2
    refused(s.loop_isolate, bad)
    for kw in (dict(min_base_height=float("nan")), dict(max_base_height=float("nan")), dict(max_tilt=float("nan")), dict(min_base_height=0.9, max_base_height=0.8),
               dict(max_tilt=-0.1)):
        refused(s.loop_isolate, s.episode_settings("reset", **kw))
    nan_x = case["x0"].copy()
    nan_x[1, 3] = np.inf
    refused(s.loop_isolate, s.episode_settings("park"), x_reset=nan_x)
    assert s.loop_run(1)["cycles_done"] == 1                     # none of the refusals ended or isolated the loop
    refused(s.loop_episodes)
    # the reset request
    s.loop_isolate(s.episode_settings("park"))
    assert (s.loop_episodes()["state"] == ALIVE).all()
    for ids in ([-1], [B], [1, 1], [0, 1, 2, 3, 4, 0]):
        refused(s.loop_reset, ids)
    one = np.zeros(1, np.int32).ctypes.data_as(ip)
    assert lib.hsqp_loop_reset_instances(s.h, 0, one, None, None) == _abi.ERR_BAD_ARG and lib.hsqp_last_error(s.h)
    assert lib.hsqp_loop_reset_instances(s.h, 1, None, None, None) == _abi.ERR_BAD_ARG and lib.hsqp_last_error(s.h)
    refused(s.loop_reset, [1], x0=nan_x[1:2])
    refused(s.loop_reset, [1], v_cmd=[0.1, np.nan, 0.78, 0.0])
    assert (s.loop_episodes()["n_episodes"] == 1).all()          # no refused request reset anything
    s.loop_reset([1])
    assert list(s.loop_episodes()["n_episodes"]) == [1, 2, 1, 1, 1]
    # every hsqp_loop_start turns isolation off; every upload ends the loop
    start(s, model, case, False)
    refused(s.loop_episodes)
    s.loop_isolate()
    s.loop_run(1)
    tt, ts, _ = s.command_targets(case["cmd"], case["x0"], 0.0, N * model.sqp["dt"])
    from wb_humanoid_mpc_amd.reference import swing_config
    s.upload_reference_warm(case["x0"], N, model.sqp["dt"], 0.0, case["ne"], case["ev"], case["seq"], tt, ts, swing_config(model), mode="cold")
    for what, a in ((s.loop_isolate, ()), (s.loop_reset, ([0],)), (s.loop_episodes, ())):
        assert "ends a loop" in refused(what, *a)
    # a handle that would take a KKT-gated sweep: one verdict per batch
    g = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="parallel")
    try:
        start(g, model, case, False)
        assert "HSQP_FLAG_SERIAL_RICCATI" in refused(g.loop_isolate)
        assert g.loop_run(1)["cycles_done"] == 1
    finally:
        g.close()
    # centroidal handles have no loop
    c = HipSqpSolver(cmodel, max_nodes=8, max_batch=2)
    try:
        st = _abi.EpisodeSettings()
        lib.hsqp_episode_defaults(C.byref(st))
        assert lib.hsqp_loop_isolate(c.h, C.byref(st), None) == _abi.ERR_BAD_ARG and lib.hsqp_last_error(c.h)
    finally:
        c.close()
