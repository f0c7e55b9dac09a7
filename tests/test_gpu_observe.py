"""The observation model of the resident loop (include/hsqp_observe.h) on the MI355X: hsqp_observe_eval against the numpy restatement
(tests/observe_ref.py), a neutral model against no model bit for bit, the loop against the public calls it replaces bit for bit, the delay read
back through hsqp_observe_last, independence of the batch and of the other instances, isolation, and the refusals.  Small handles: 8 nodes,
3 instances, the serial recursion (the instances of a batch are then arithmetically independent), 4 to 6 cycles."""
import signal

import numpy as np
import pytest

import observe_ref as O
from test_gpu_feedback_policy import DeviceBuffer
from test_gpu_loop import loop_case
from test_gpu_push import PERIOD, loop_start
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import gait_settings, swing_config
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu
NX, NU = _abi.NX, _abi.NU
B, N, CYCLES, SEED = 3, 8, 5, 2026


@pytest.fixture(autouse=True)
def time_limit():
    def expired(signum, frame):
        raise TimeoutError("test_gpu_observe: a test ran past its 120 s limit")
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


def noise_table(rows=B, seed=5):
    """A bias of centimetres / hundredths of a radian and noise of the size of the model file's gyro and accelerometer figures, on every entry"""
    rng = np.random.default_rng(seed)
    bias, sigma = 0.01 * rng.standard_normal((B, NX)), np.abs(5e-3 * rng.standard_normal((B, NX)))
    bias[:, 2] = -0.02                                                 # 2 cm of base-height bias
    return bias[:rows], sigma[:rows]


def start(s, model, case, gait=False, rows=slice(None), controller="feedforward", x0=None):
    if gait:
        st = s.loop_settings(N, model.sqp["dt"], period=PERIOD, filter_alpha=0.8, iterations=1, take_step=True, linesearch=True, controller=controller)
        s.loop_start(st, 0.0, case["x0"][rows] if x0 is None else x0, case["cmd"][rows], gait=gait_settings(model))
    else:
        loop_start(s, model, case, rows=rows, x0=x0, controller=controller)


# ---------------------------------------------------------------------------------------------- 1. observe against observe_ref
def test_observe_matches_the_restatement(s):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((B, NX))
    x[0] = 0.0                                                         # instance 0: y = z
    x[2, 5], x[2, 9] = -0.0, np.array([0x7FF8000000000123], np.uint64).view(np.float64)[0]
    bias, sigma = np.zeros((B, NX)), np.zeros((B, NX))
    sigma[0] = 1.0
    bias[1], sigma[1] = 0.1 * rng.standard_normal(NX), np.abs(0.05 * rng.standard_normal(NX))
    bias[1, ::5], sigma[1, ::3] = 0.0, 0.0
    s.set_observation(seed=SEED)
    s.set_observation_instances(bias, sigma)
    for draw in (0, 7, 2 ** 32 - 1):
        y = s.observe(x, draw)
        want = O.observe(x, bias, sigma, SEED, draw)
        bound = sigma * 1e-13 + 2.0 * np.spacing(np.abs(want))
        live = (bias != 0.0) | (sigma != 0.0)
        err = np.abs(y - want)[live]
        print(f"draw {draw}: max |dy| {err.max():.3e}, max |dy| / bound {np.max(err / bound[live]):.3f}")
        assert (err <= bound[live]).all()
        assert np.array_equal(y.view(np.uint64)[~live], x.view(np.uint64)[~live])            # copied: the neutral instance and every neutral entry
        assert np.abs(y[0] - O.normals(SEED, 0, draw)).max() <= 1e-13
    # the device entry point, in place
    d = DeviceBuffer((B, NX))
    try:
        d.upload(x)
        s.observe_device(B, 7, d.ptr.value, d.ptr.value)
        assert np.array_equal(d.numpy().view(np.uint64), s.observe(x, 7).view(np.uint64))
    finally:
        d.free()
    got = s.get_observation(B)
    assert (got["sensor_delay"], got["compute_delay"], got["seed"]) == (0, 0, SEED) and np.array_equal(got["bias"], bias) and np.array_equal(got["sigma"], sigma)
    s.set_observation_instances(bias[:2], sigma[:2])                    # instances past the table are neutral
    assert np.array_equal(s.observe(x, 7)[2].view(np.uint64), x[2].view(np.uint64)) and not s.get_observation(B)["sigma"][2].any()
    s.clear_observation()
    assert np.array_equal(s.observe(x, 7).view(np.uint64), x.view(np.uint64))


# ---------------------------------------------------------------------------------------------- 2. neutral is the parent
def run_and_snapshot(s, cycles):
    r = s.loop_run(cycles)
    t, x, vf = s.loop_state()
    return dict(x=r["x"], u=r["u"], t=np.array(t), x_end=x, vf=vf, **{"ep_" + k: v for k, v in s.loop_episodes().items()})


@pytest.mark.parametrize("plant", ["flow", "torque"])
def test_a_neutral_model_is_the_loop_without_one(s, model, plant):
    case = loop_case(model, batch=B)
    if plant == "torque":
        s.set_plant("torque")
    start(s, model, case)
    s.loop_isolate(s.episode_settings("reset"), x_reset=case["x0"])
    want = run_and_snapshot(s, CYCLES)
    assert np.isfinite(want["x"]).all()
    for table in (False, True):
        s.set_observation(0, 0, seed=SEED)
        if table:
            s.set_observation_instances(np.zeros((B, NX)), np.zeros((B, NX)))
        start(s, model, case)
        s.loop_isolate(s.episode_settings("reset"), x_reset=case["x0"])
        got = run_and_snapshot(s, CYCLES)
        for k in want:
            assert np.array_equal(got[k], want[k]), (plant, table, k)
        y, tp = s.last_observation()
        t_last = 0.0
        for _ in range(CYCLES - 1):
            t_last += PERIOD
        assert np.array_equal(y, want["x"][-2]) and tp == t_last       # the last cycle measured the state and the time it started from
    s.clear_observation()
    start(s, model, case)
    s.loop_isolate(s.episode_settings("reset"), x_reset=case["x0"])
    got = run_and_snapshot(s, CYCLES)
    assert all(np.array_equal(got[k], want[k]) for k in want)


# ---------------------------------------------------------------------------------------------- 3. the loop is the public calls
def by_hand(s, model, case, cycles, controller, gait, sensor_delay, compute_delay):
    """The cycles of include/hsqp_observe.h through the public calls; the ring is observe_ref's."""
    dt, sw = model.sqp["dt"], swing_config(model)
    x, cmd = case["x0"].copy(), case["cmd"].copy()
    vf, t, k = cmd.copy(), 0.0, compute_delay
    ring = O.Ring(len(x), sensor_delay + compute_delay)
    ne, ev, seq = case["ne"], case["ev"], case["seq"]
    if gait:
        s.gait_reset(gait_settings(model), len(x), O.problem_time(t, k, PERIOD))
    xs, us, ys = [], [], []
    for c in range(cycles):
        y = s.observe(ring.cycle(c, x, np.full(len(x), c == 0)), c)
        tp = O.problem_time(t, k, PERIOD)
        tt, ts, vf = s.command_targets(cmd, y, tp, N * dt, filter_alpha=0.8, v_filt=vf)
        if gait:
            ne, ev, seq = s.gait_update(tp, N * dt, vf, y)
        s.upload_reference_warm(y, N, dt, tp, ne, ev, seq, tt, ts, sw, mode="cold" if c == 0 else "shift")
        s.iterate(1, take_step=True, linesearch=True)
        r = s.rollout_policy(np.full(len(x), O.policy_time(k, PERIOD)), x, PERIOD, 1, controller=controller)
        x = r["x"][:, 0].copy()
        xs.append(x); us.append(r["u"][:, 0].copy()); ys.append(y)
        t += PERIOD
    return dict(x=np.array(xs), u=np.array(us), y=np.array(ys), t=t, tp=tp, vf=vf, stamps=s.stamps(), gait=s.gait_state() if gait else {})


@pytest.mark.parametrize("controller,gait", [("feedforward", False), ("feedback", False), ("feedforward", True), ("feedback", True)])
def test_the_loop_equals_the_public_calls(s, model, controller, gait):
    case = loop_case(model, batch=B)
    if gait:
        case["cmd"][:, 0] = [0.0, 0.2, 0.3]                            # the ladder's first rung is left by two instances
    s.set_observation(sensor_delay=1, compute_delay=1, seed=SEED)
    s.set_observation_instances(*noise_table())
    want = by_hand(s, model, case, CYCLES, controller, gait, 1, 1)
    start(s, model, case, gait=gait, controller=controller)
    got = s.loop_run(CYCLES)
    t, x_end, vf = s.loop_state()
    y, tp = s.last_observation()
    stamps, state = s.stamps(), (s.gait_state() if gait else {})
    assert got["cycles_done"] == CYCLES and np.isfinite(got["x"]).all()
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])
    assert t == want["t"] and np.array_equal(x_end, want["x"][-1]) and np.array_equal(vf, want["vf"])
    assert np.array_equal(y, want["y"][-1]) and tp == want["tp"] and np.array_equal(stamps, want["stamps"])
    assert stamps[0, 0] == tp                                          # the problem is posed at the observation's time
    for k in state:
        assert np.array_equal(state[k], want["gait"][k]), k
    s.clear_observation()                                              # and the model is felt
    start(s, model, case, gait=gait, controller=controller)
    plain = s.loop_run(CYCLES)
    assert np.isfinite(plain["x"]).all() and not np.array_equal(plain["x"], got["x"])


# ---------------------------------------------------------------------------------------------- 4. the delay, read back
@pytest.mark.parametrize("delays", [(2, 0), (0, 2)])
def test_the_delay_read_back(s, model, delays):
    sd, cd = delays
    a = sd + cd
    case = loop_case(model, batch=B)
    s.set_observation(sensor_delay=sd, compute_delay=cd)
    start(s, model, case)
    log = []
    for c in range(a + 3):
        t = s.loop_state()[0]
        log.append(s.loop_run(1)["x"][0])
        y, tp = s.last_observation()
        assert np.array_equal(y, case["x0"] if c <= a else log[c - 1 - a]), c
        assert tp == t - cd * PERIOD, c
    assert np.isfinite(np.array(log)).all()
    s.clear_observation()
    start(s, model, case)
    assert not np.array_equal(s.loop_run(a + 3)["x"][1:], np.array(log)[1:])   # the first cycle sees x0 either way


# ---------------------------------------------------------------------------------------------- 5. independence and reproducibility
def test_independence_and_reproducibility(s, model):
    case = loop_case(model, batch=B)
    bias, sigma = noise_table()

    def run(rows, seed):
        s.set_observation(sensor_delay=1, compute_delay=0, seed=seed)
        s.set_observation_instances(bias[:rows], sigma[:rows])
        start(s, model, case, rows=slice(0, rows))
        return s.loop_run(CYCLES)
    three, again, two, other = run(3, SEED), run(3, SEED), run(2, SEED), run(3, SEED + 1)
    assert np.isfinite(three["x"]).all()
    assert np.array_equal(three["x"], again["x"]) and np.array_equal(three["u"], again["u"])
    assert np.array_equal(three["x"][:, :2], two["x"]) and np.array_equal(three["u"][:, :2], two["u"])
    assert not np.array_equal(three["x"], other["x"])


# ---------------------------------------------------------------------------------------------- 6. isolation
def test_a_restarted_instance_reads_its_reset_state(s, model):
    """The technique of tests/test_gpu_episode.py::test_the_callers_box: instance 1 starts 4 cm low, the box's floor lies 2 cm below the standing
    height, so it leaves the box in cycle 0 and restarts from x_reset in cycle 1: the observations of cycles 1 .. 1 + a are x_reset."""
    a, sick, healthy, cycles = 2, 1, [0, 2], 6
    case = loop_case(model, batch=B)
    h0 = float(model.initial_state[2])
    low = case["x0"].copy()
    low[sick, 2] = h0 - 0.04
    s.set_observation(sensor_delay=a)
    start(s, model, case, x0=low)
    plain = s.loop_run(cycles)
    assert (plain["x"][:, healthy, 2] > h0 - 0.02).all() and plain["x"][0, sick, 2] < h0 - 0.02
    start(s, model, case, x0=low)
    s.loop_isolate(s.episode_settings("reset", min_base_height=h0 - 0.02), x_reset=case["x0"])
    log = []
    for c in range(cycles):
        log.append(s.loop_run(1)["x"][0])
        y = s.last_observation()[0]
        if c == 0:
            assert np.array_equal(y[sick], low[sick])
        elif c <= 1 + a:
            assert np.array_equal(y[sick], case["x0"][sick]), c
        else:
            assert np.array_equal(y[sick], log[c - 1 - a][sick]), c
    log = np.array(log)
    ep = s.loop_episodes()
    assert ep["n_failures"][sick] == 1 and ep["fail_cycle"][sick] == 0 and ep["cause"][sick] == _abi.EP_FAILED_BOUNDS and (ep["n_failures"][healthy] == 0).all()
    assert np.array_equal(log[:, healthy], plain["x"][:, healthy]) and np.isfinite(log[1:]).all()
    # the same through hsqp_loop_reset_instances between cycles 1 and 2
    new_x = case["x0"][[sick]].copy()
    new_x[0, 6:12] += 0.01
    start(s, model, case, x0=low)
    s.loop_isolate(s.episode_settings("park"), x_reset=case["x0"])
    log = [s.loop_run(1)["x"][0] for _ in range(2)]
    s.loop_reset([sick], x0=new_x)
    for c in range(2, cycles):
        log.append(s.loop_run(1)["x"][0])
        y = s.last_observation()[0]
        assert np.array_equal(y[sick], new_x[0] if c <= 2 + a else log[c - 1 - a][sick]), c
    log = np.array(log)
    assert np.array_equal(log[:, healthy], plain["x"][:, healthy]) and np.array_equal(log[:2, sick], plain["x"][:2, sick])
    assert np.isfinite(log).all() and s.loop_episodes()["n_episodes"][sick] == 2


# ---------------------------------------------------------------------------------------------- 7. refusals
def test_refusals(s, model, cmodel):
    case = loop_case(model, batch=B)

    def refused(what, call, *args, **kw):
        with pytest.raises(HsqpError) as ei:
            call(*args, **kw)
        assert ei.value.code == _abi.ERR_BAD_ARG and what in str(ei.value), (what, str(ei.value))
        return ei.value
    refused("hsqp_observe_set: negative delay", s.set_observation, -1, 0)
    refused("hsqp_observe_set: negative delay", s.set_observation, 0, -1)
    refused("HSQP_OBS_MAX_DELAY", s.set_observation, 5, 4)
    zero = np.zeros((B, NX))
    for bad in (np.nan, np.inf):
        t = zero.copy(); t[2, 7] = bad
        refused("hsqp_observe_set_instances: instance 2: bias[7]", s.set_observation_instances, t, zero)
        refused("hsqp_observe_set_instances: instance 2: sigma[7]", s.set_observation_instances, zero, t)
    t = zero.copy(); t[1, 57] = -1e-9
    refused("instance 1: sigma[57]", s.set_observation_instances, zero, t)
    refused("batch outside", s.set_observation_instances, np.zeros((B + 1, NX)), np.zeros((B + 1, NX)))
    refused("batch outside", s.observe, np.zeros((B + 1, NX)), 0)
    refused("batch outside", s.get_observation, B + 1)
    assert not s.get_observation(B)["sigma"].any()                      # no refused call left anything behind
    refused("hsqp_observe_last", s.last_observation)                    # no loop
    # delays under a started loop; the seed and the table may change
    s.set_observation(sensor_delay=1, compute_delay=1, seed=1)
    start(s, model, case)
    refused("hsqp_observe_last", s.last_observation)                    # no completed cycle
    refused("restart the loop", s.set_observation, 1, 0, 1)
    refused("restart the loop", s.set_observation, 2, 1, 1)
    s.set_observation(sensor_delay=1, compute_delay=1, seed=2)
    assert s.get_observation(1)["seed"] == 2 and s.get_observation(1)["sensor_delay"] == 1
    # the table's batch against the loop's
    s.set_observation_instances(zero[:2], zero[:2])
    e = refused("observation table holds 2 instances", s.loop_run, 1)
    assert "hsqp_loop_run" in str(e) and e.result["cycles_done"] == 0
    s.set_observation_instances(None, None)
    assert s.loop_run(1)["cycles_done"] == 1 and s.last_observation()[1] == -PERIOD
    # the horizon: 2 nodes of 0.035 s are 4.2 periods (a handle of its own: this one's loop holds its delays)
    h = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        h.set_observation(compute_delay=4)
        st = h.loop_settings(2, model.sqp["dt"], period=PERIOD, filter_alpha=0.8)
        h.loop_start(st, 0.0, case["x0"], case["cmd"], case["ne"], case["ev"], case["seq"])
        with pytest.raises(HsqpError) as ei:
            h.loop_run(1)
        assert ei.value.code == _abi.ERR_BAD_ARG and "hsqp_loop_run" in str(ei.value) and "past its horizon" in str(ei.value) and ei.value.result["cycles_done"] == 0
    finally:
        h.close()
    # centroidal handles
    c = HipSqpSolver(cmodel, max_nodes=N, max_batch=B)
    try:
        with pytest.raises(HsqpError) as ei:
            c.set_observation()
        assert ei.value.code == _abi.ERR_BAD_ARG and "whole-body handles only" in str(ei.value)
    finally:
        c.close()
