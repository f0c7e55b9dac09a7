"""The per-instance gait schedule and gait ladder (include/hsqp_gait.h) on the GPU: k_gait_update against the Python mirror bit for bit, and the
resident loop started through hsqp_loop_start_gait against the public calls it replaces, through a stance -> walk -> stance ladder scenario
and far past anything that was ever uploaded.

Pinned against reference-compiled code: one insert followed by one query (tests/test_gait.py, tests/golden/ref_gait.npz).  Not pinned: chains of
updates and ProceduralMpcMotionManager.cpp itself; here the device is held to the mirror, which restates them line by line."""
import numpy as np
import pytest

from test_gait import _x, events_bound, ladder_sequence, padded_row
from test_gpu_feedback_policy import DeviceBuffer
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import GAIT_OK, LF, RF, STANCE, GaitInstance, gait_cycle, gait_settings, swing_config
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu

NX, NU, NJ = _abi.NX, _abi.NU, _abi.NJ
B, N, PERIOD, ALPHA = 4, 30, 1.0 / 60.0, 0.8
HEIGHT = 0.7925


def mirror_states(settings, rows, t0=0.0):
    return [GaitInstance(settings, t0) for _ in range(rows)]


def assert_state_equals_mirror(state, mirror, E):
    for b, m in enumerate(mirror):
        e, s = padded_row(m.schedule.event_times, m.schedule.mode_sequence, E)
        assert state["n_events"][b] == len(m.schedule.event_times) and np.array_equal(state["event_times"][b], e) and np.array_equal(state["mode_sequence"][b], s), b
        assert state["rung"][b] == m.rung and state["last_change_time"][b] == m.last_change_time, b


# ---------------------------------------------------------------------------------------------- the update on its own
@pytest.mark.parametrize("pts", [0.0, 0.1])
def test_update_and_its_device_twin_equal_the_mirror(model, pts):
    """The 2000-update sequence of tests/test_gait.py (600 at 60 Hz, 1400 at 20 Hz), 8 instances: outputs and read-back state, bit for bit."""
    rows, H = 8, N * model.sqp["dt"]
    settings = gait_settings(model, phase_transition_stance_time=pts)
    E = settings.max_events
    s = HipSqpSolver(model, max_nodes=N, max_batch=rows)
    ints = lambda count: DeviceBuffer(((count + 1) // 2,))  # noqa: E731
    bufs = [DeviceBuffer((rows, 4)), DeviceBuffer((rows, NX)), ints(rows), DeviceBuffer((rows, E)), ints(rows * (E + 1)), ints(rows), DeviceBuffer((rows,))]
    try:
        for updates, period in ((600, 1.0 / 60.0), (1400, 0.05)):
            s.gait_reset(settings, rows)
            mirror = mirror_states(settings, rows)
            for k, (t, v, x) in enumerate(ladder_sequence(model, rows, updates, period, seed=20261016)):
                if k % 2 == 0:
                    ne, ev, seq = s.gait_update(t, H, v, x)
                else:
                    bufs[0].upload(v); bufs[1].upload(x)
                    s.gait_update_device(rows, t, H, *[b.ptr.value for b in bufs[:5]])
                    ne = bufs[2].numpy().view(np.int32)[:rows]
                    ev, seq = bufs[3].numpy(), bufs[4].numpy().view(np.int32)[:rows * (E + 1)].reshape(rows, E + 1)
                for b, m in enumerate(mirror):
                    st, mev, mseq = gait_cycle(m, t, H, [float(a) for a in v[b]], x[b])
                    assert st == GAIT_OK
                    e, q = padded_row(mev, mseq, E)
                    assert ne[b] == len(mev) and np.array_equal(ev[b], e) and np.array_equal(seq[b], q), (t, b)
                if k % 50 == 49 or k == updates - 1:
                    assert_state_equals_mirror(s.gait_state(), mirror, E)
            s.gait_state_device(bufs[5].ptr.value, bufs[6].ptr.value)
            assert list(bufs[5].numpy().view(np.int32)[:rows]) == [m.rung for m in mirror]
            assert list(bufs[6].numpy()) == [m.last_change_time for m in mirror]
            assert {m.rung for m in mirror} != {0}
    finally:
        for b in bufs:
            b.free()
        s.close()


# ---------------------------------------------------------------------------------------------- the loop
def scenario(model, rows=B):
    """instance 0: zero command throughout; 1: 0.2 m/s from cycle 10; 2: 0.2 m/s from cycle 10, zero again from cycle 40; 3: a yaw-rate command from cycle 10.
    Why cycle 40: slow_walk's events fall on 1.0 (first lift-off), 1.65, 1.85, 2.5 s, and the stance template goes in at the first event behind
    t + 0.7 H = t + 0.735 s.  The descent needs the filtered command below 0.05 (seven cycles after the stop) AND the base below 0.1 m/s; if
    it comes before t = 1.115 s the walk ends at 1.0 or 1.85 s, otherwise at 2.5 s, which is cycle 150 itself — the end of the run."""
    x0 = np.tile(model.initial_state, (rows, 1))
    zero = np.tile((0.0, 0.0, HEIGHT, 0.0), (rows, 1))
    go = zero.copy()
    go[1, 0] = go[2, 0] = 0.2
    go[3, 3] = 0.3
    stop = go.copy()
    stop[2, 0] = 0.0
    return dict(x0=x0, cmd=zero, commands={10: go, 40: stop})


def start_gait(s, model, settings, case, rows=slice(None), riccati_settings=None):
    st = s.loop_settings(N, model.sqp["dt"], period=PERIOD, filter_alpha=ALPHA, iterations=1, take_step=True, linesearch=True)
    s.loop_start(st, 0.0, case["x0"][rows], case["cmd"][rows], gait=settings)


def run_gait_loop(s, case, cycles, rows=slice(None), per_cycle=None):
    """loop_run in the pieces the command changes cut (or cycle by cycle with per_cycle(c) called after each): the logs of all cycles"""
    xs, us, c = [], [], 0
    cuts = sorted(k for k in case["commands"] if k < cycles) + [cycles]
    while c < cycles:
        if c in case["commands"]:
            s.loop_command(case["commands"][c][rows])
        n = 1 if per_cycle else next(k for k in cuts if k > c) - c
        r = s.loop_run(n)
        xs.append(r["x"]); us.append(r["u"])
        c += n
        if per_cycle:
            per_cycle(c - 1)
    return np.concatenate(xs), np.concatenate(us)


def gait_by_hand(s, model, settings, case, cycles):
    """The cycles through the public calls: hsqp_command_targets, hsqp_gait_update, hsqp_upload_reference with the returned schedule,
    hsqp_iterate_device, hsqp_rollout_policy."""
    dt, sw = model.sqp["dt"], swing_config(model)
    x, cmd = case["x0"].copy(), case["cmd"].copy()
    vf, t = cmd.copy(), 0.0
    xs, us = [], []
    s.gait_reset(settings, len(x), 0.0)
    for c in range(cycles):
        if c in case["commands"]:
            cmd = case["commands"][c].copy()
        tt, ts, vf = s.command_targets(cmd, x, t, N * dt, filter_alpha=ALPHA, v_filt=vf)
        ne, ev, seq = s.gait_update(t, N * dt, vf, x)
        s.upload_reference_warm(x, N, dt, t, ne, ev, seq, tt, ts, sw, mode="cold" if c == 0 else "shift")
        s.iterate(1, take_step=True, linesearch=True)
        r = s.rollout_policy(np.zeros(len(x)), x, PERIOD, 1)
        x = r["x"][:, 0].copy()
        xs.append(x); us.append(r["u"][:, 0].copy())
        t += PERIOD
    X, U = s.device_trajectory()
    return dict(x=np.array(xs), u=np.array(us), vf=vf, t=t, X=X, U=U, stamps=s.stamps(), gait=s.gait_state())


def test_loop_equals_the_calls_it_replaces(model):
    settings, case, cycles = gait_settings(model), scenario(model), 30
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True)
    try:
        want = gait_by_hand(s, model, settings, case, cycles)
        start_gait(s, model, settings, case)
        x, u = run_gait_loop(s, case, cycles)
        t, x_end, vf = s.loop_state()
        X, U = s.device_trajectory()
        stamps, gait = s.stamps(), s.gait_state()
    finally:
        s.close()
    assert x.shape[0] == cycles and np.isfinite(x).all() and np.isfinite(u).all()
    assert np.array_equal(x, want["x"]) and np.array_equal(u, want["u"])
    assert np.array_equal(vf, want["vf"]) and np.array_equal(x_end, want["x"][-1]) and t == want["t"]
    assert np.array_equal(X, want["X"]) and np.array_equal(U, want["U"]) and np.array_equal(stamps, want["stamps"])
    for k in gait:
        assert np.array_equal(gait[k], want["gait"][k]), k
    assert gait["rung"][1] == 1 and gait["rung"][0] == 0               # the ladder moved inside the thirty cycles


def mirror_rungs(model, settings, case, x_log, cycles, rows):
    """The mirror driven with the loop's own measured states and the filter recursion of csrc/hsqp_loop.h: rung [cycles][rows] after every cycle"""
    mirror = mirror_states(settings, rows)
    cmd = case["cmd"].copy()
    vf, t, H = cmd.copy(), 0.0, N * model.sqp["dt"]
    out = []
    for c in range(cycles):
        if c in case["commands"]:
            cmd = case["commands"][c].copy()
        vf = ALPHA * vf + (1.0 - ALPHA) * cmd
        x = case["x0"] if c == 0 else x_log[c - 1]
        for b, m in enumerate(mirror):
            assert gait_cycle(m, t, H, [float(a) for a in vf[b]], x[b])[0] == GAIT_OK
        out.append([m.rung for m in mirror])
        t += PERIOD
    return np.array(out), mirror


def test_ladder_scenario(model):
    """150 cycles (2.5 s), B = 4, N = 30, on handles that always take the serial recursion (the default sweep is chosen by batch size, so without the
    flag the batch and the solo runs would not take the same path)."""
    settings, case, cycles = gait_settings(model), scenario(model), 150
    E = settings.max_events
    swing = np.zeros((cycles, B, N + 1), bool)       # a node with a foot in the air
    rung = np.zeros((cycles, B), np.int32)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        start_gait(s, model, settings, case)

        def look(c):
            swing[c] = (s.device_params()[:, :, _abi.P_CONTACT:_abi.P_CONTACT + 2] < 0.5).any(axis=2)
            rung[c] = s.gait_state()["rung"]
        x, u = run_gait_loop(s, case, cycles, per_cycle=look)
        state = s.gait_state()
        solo = []
        for b in range(B):
            start_gait(s, model, settings, case, rows=slice(b, b + 1))
            solo.append(run_gait_loop(s, case, cycles, rows=slice(b, b + 1)))
    finally:
        s.close()
    z = x[:, :, 2]
    print("pelvis height per instance: min", z.min(axis=0), "max", z.max(axis=0))
    print("rungs at the end", rung[-1], "first swing node per cycle, instance 1:", [int(np.argmax(r)) if r.any() else -1 for r in swing[:, 1]])
    assert np.isfinite(x).all() and np.isfinite(u).all()
    # instance 0 never lifts a foot
    assert not swing[:, 0].any() and (rung[:, 0] == 0).all()
    # instance 1: the swing enters at the tail (not in front of earliestSwitchingTime = t + 0.7 H) and reaches node 0 later
    first = next(c for c in range(cycles) if swing[c, 1].any())
    assert first >= 10 and int(np.argmax(swing[first, 1])) >= int(0.7 * N) - 1
    at_zero = next(c for c in range(cycles) if swing[c, 1, 0])
    assert at_zero > first
    lead = [int(np.argmax(swing[c, 1])) for c in range(first, at_zero + 1)]
    assert all(b <= a for a, b in zip(lead, lead[1:]))                     # it moves towards node 0
    # instance 2 walked and returns to all-stance
    assert swing[:, 2].any() and not swing[-1, 2].any() and rung[-1, 2] == 0 and (rung[:, 2] == 1).any()
    # instance 3: the yaw-rate command alone leaves stance
    assert rung[-1, 3] >= 1
    # the rungs are the mirror's, cycle by cycle, and so is the state at the end
    want, mirror = mirror_rungs(model, settings, case, x, cycles, B)
    assert np.array_equal(rung, want)
    assert_state_equals_mirror(state, mirror, E)
    # every instance equals its solo run
    for b in range(B):
        assert np.array_equal(solo[b][0][:, 0], x[:, b]) and np.array_equal(solo[b][1][:, 0], u[:, b]), b
    # the pelvis stays up: the band of tests/test_gpu_convergence.py and tests/test_oracle_convergence.py
    assert z.min() >= 0.74 and z.max() <= 0.82, (z.min(axis=0), z.max(axis=0))


def test_fifteen_seconds_past_anything_uploaded(model):
    """900 cycles: finite, the schedule bounded, the walking instance still alternating feet in the last cycle.  No physical band: no number
    exists for a run of that length."""
    settings, cycles = gait_settings(model), 900
    case = dict(x0=np.tile(model.initial_state, (2, 1)), cmd=np.tile((0.0, 0.0, HEIGHT, 0.0), (2, 1)),
                commands={10: np.array([[0.0, 0.0, HEIGHT, 0.0], [0.2, 0.0, HEIGHT, 0.0]])})
    bound = events_bound(settings, N * model.sqp["dt"])
    s = HipSqpSolver(model, max_nodes=N, max_batch=2, linesearch=True)
    try:
        start_gait(s, model, settings, case)
        n_max = 0
        xs = []
        for c0 in range(0, cycles, 100):
            if c0 == 0:
                r = s.loop_run(10); s.loop_command(case["commands"][10]); r2 = s.loop_run(90)
                xs += [r["x"], r2["x"]]
            else:
                xs.append(s.loop_run(100)["x"])
            n_max = max(n_max, int(s.gait_state()["n_events"].max()))
        x = np.concatenate(xs)
        state = s.gait_state()
        contact = s.device_params()[:, :, _abi.P_CONTACT:_abi.P_CONTACT + 2] > 0.5
    finally:
        s.close()
    print("n_events max", n_max, "bound", bound, "pelvis height range", x[:, :, 2].min(axis=0), x[:, :, 2].max(axis=0))
    assert x.shape[0] == cycles and np.isfinite(x).all()
    assert n_max <= bound <= settings.max_events
    seq = list(state["mode_sequence"][1][:state["n_events"][1] + 1])
    swings = [m for m in seq if m in (LF, RF)]
    assert state["rung"][1] >= 1 and len(swings) >= 3 and all(a != b for a, b in zip(swings, swings[1:]))
    assert state["event_times"][1][0] > 900 * PERIOD - 2 * N * model.sqp["dt"] - 2.5          # the history is trimmed: nothing from the start is left
    left_up, right_up = ~contact[1, :, 0], ~contact[1, :, 1]
    assert left_up.any() and right_up.any() and not (left_up & right_up).any()                # both feet swing inside the last horizon, never together
    assert contact[0].all() and state["rung"][0] == 0


def test_forced_overflow_stops_the_loop_in_the_documented_state(model):
    settings = gait_settings(model, max_events=8)
    case = dict(x0=np.tile(model.initial_state, (2, 1)), cmd=np.array([[0.0, 0.0, HEIGHT, 0.0], [0.3, 0.0, HEIGHT, 0.0]]), commands={})
    mirror = mirror_states(settings, 2)
    s = HipSqpSolver(model, max_nodes=N, max_batch=2, linesearch=True)
    try:
        start_gait(s, model, settings, case)
        with pytest.raises(HsqpError) as e:
            s.loop_run(120)
        done = e.value.result["cycles_done"]
        assert e.value.code == _abi.ERR_BAD_ARG and "max_events" in str(e.value) and 0 < done < 120
        t, x, vf = s.loop_state()
        state = s.gait_state()
        # the loop stands at the last completed cycle, the gait state with it; the next run fails in the same cycle again
        xl = e.value.result["x"]
        tt, H, f = 0.0, N * model.sqp["dt"], case["cmd"].copy()
        for c in range(done):
            f = ALPHA * f + (1.0 - ALPHA) * case["cmd"]
            for b, m in enumerate(mirror):
                assert gait_cycle(m, tt, H, [float(a) for a in f[b]], (case["x0"] if c == 0 else xl[c - 1])[b])[0] == GAIT_OK
            tt += PERIOD
        assert t == tt and np.array_equal(x, xl[-1]) and np.array_equal(vf, f)
        assert_state_equals_mirror(state, mirror, settings.max_events)
        f = ALPHA * f + (1.0 - ALPHA) * case["cmd"]
        failing = [b for b, m in enumerate(mirror) if gait_cycle(m, tt, H, [float(a) for a in f[b]], x[b])[0] != GAIT_OK]
        assert failing and f"instance {failing[0]}" in str(e.value)
        with pytest.raises(HsqpError) as e2:
            s.loop_run(1)
        assert e2.value.code == _abi.ERR_BAD_ARG and e2.value.result["cycles_done"] == 0 and s.loop_state()[0] == tt
    finally:
        s.close()


def test_old_entry_after_a_gait_loop_and_the_reverse(model):
    from test_gpu_loop import CYCLES, loop_case, start
    import test_gpu_loop
    settings, gcase = gait_settings(model), scenario(model)
    gcase["cmd"] = gcase["commands"][10]
    gcase["commands"] = {}
    case = loop_case(model, batch=B)
    s = HipSqpSolver(model, max_nodes=max(N, test_gpu_loop.N), max_batch=B, linesearch=True)
    try:
        start(s, model, case)
        old_a = s.loop_run(CYCLES)
        with pytest.raises(HsqpError):                  # no gait state yet, and an old-entry loop has none
            s.gait_state()
        start_gait(s, model, settings, gcase)
        gait_a = s.loop_run(20)
        state_a = s.gait_state()
        start(s, model, case)
        old_b = s.loop_run(CYCLES)
        start_gait(s, model, settings, gcase)
        gait_b = s.loop_run(20)
        state_b = s.gait_state()
        # hsqp_gait_update on the handle hands the state back to the caller: the gait loop is over
        s.gait_update(20 * PERIOD, N * model.sqp["dt"], gcase["cmd"], gcase["x0"])
        with pytest.raises(HsqpError) as e:
            s.loop_run(1)
        assert e.value.code == _abi.ERR_BAD_ARG and "hsqp_loop_start" in str(e.value)
    finally:
        s.close()
    assert np.array_equal(old_a["x"], old_b["x"]) and np.array_equal(old_a["u"], old_b["u"])
    assert np.array_equal(gait_a["x"], gait_b["x"]) and np.array_equal(gait_a["u"], gait_b["u"])
    assert all(np.array_equal(state_a[k], state_b[k]) for k in state_a) and state_a["rung"][1] == 1


def test_bad_arguments(model, cmodel):
    import ctypes as C
    good = gait_settings(model)
    c = HipSqpSolver(cmodel, max_nodes=8, max_batch=2)
    try:
        with pytest.raises(HsqpError) as e:
            c.gait_reset(good, 1)
        assert e.value.code == _abi.ERR_BAD_ARG and "whole-body handles only" in str(e.value)
        st = _abi.LoopSettings()
        c.lib.hsqp_loop_defaults(c.h, C.byref(st))
        p = np.zeros(2 * NX).ctypes.data_as(C.POINTER(C.c_double))
        assert c.lib.hsqp_loop_start_gait(c.h, C.byref(st), C.byref(good), 1, 0.0, p, p) == _abi.ERR_BAD_ARG and b"whole-body handles only" in c.lib.hsqp_last_error(c.h)
    finally:
        c.close()
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True)
    try:
        def refused(what, *a, text="", **kw):
            with pytest.raises(HsqpError) as e:
                what(*a, **kw)
            assert e.value.code == _abi.ERR_BAD_ARG and text in str(e.value), str(e.value)
        refused(s.gait_state, text="hsqp_gait_reset")
        refused(s.gait_update, 0.0, 1.0, np.zeros((1, 4)), np.zeros((1, NX)), text="hsqp_gait_reset")
        skip = gait_settings(model, ladder=(("stance", -0.1, 0.1, -0.1, 0.1, 10.0, 10.0), ("skip", 0.05, 0.3, 0.05, 0.2, 0.05, 0.05)))
        refused(s.gait_reset, skip, 1, text="skip")
        for change in (dict(n_rungs=0), dict(n_rungs=17), dict(max_events=1), dict(max_events=257), dict(phase_transition_stance_time=float("nan")),
                       dict(phase_transition_stance_time=-0.1), dict(min_change_interval=float("inf")), dict(min_change_interval=-0.1)):
            bad = gait_settings(model)
            for k, v in change.items():
                setattr(bad, k, v)
            refused(s.gait_reset, bad, 1)
        bad = gait_settings(model); bad.rungs[2].max_lin_vel_cmd = float("nan")
        refused(s.gait_reset, bad, 1, text="walk")
        bad = gait_settings(model); bad.rungs[1].n_phases = 7
        refused(s.gait_reset, bad, 1)
        bad = gait_settings(model); bad.rungs[1].modes[0] = 4
        refused(s.gait_reset, bad, 1)
        refused(s.gait_reset, good, 0)
        refused(s.gait_reset, good, B + 1)
        refused(s.gait_reset, good, 1, float("nan"))
        assert s.lib.hsqp_gait_reset(s.h, None, 1, 0.0) == _abi.ERR_BAD_ARG
        s.gait_reset(good, 2)
        x = np.tile(_x(model), (2, 1))
        refused(s.gait_update, float("nan"), 1.0, np.zeros((2, 4)), x)
        refused(s.gait_update, 0.0, 0.0, np.zeros((2, 4)), x)
        refused(s.gait_update, 0.0, float("inf"), np.zeros((2, 4)), x)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        z, zi = np.zeros(2 * NX), np.zeros(2 * (good.max_events + 1), np.int32)
        assert s.lib.hsqp_gait_update(s.h, 1, 0.0, 1.0, z.ctypes.data_as(dp), z.ctypes.data_as(dp), zi.ctypes.data_as(ip), np.zeros(2 * good.max_events).ctypes.data_as(dp),
                                      zi.ctypes.data_as(ip)) == _abi.ERR_BAD_ARG and b"batch" in s.lib.hsqp_last_error(s.h)
        assert s.lib.hsqp_gait_update(s.h, 2, 0.0, 1.0, None, None, None, None, None) == _abi.ERR_BAD_ARG
        ne, ev, seq = s.gait_update(0.0, 1.0, np.zeros((2, 4)), x)          # and the state still works
        assert (ne >= 1).all() and (seq == STANCE).all() and (ev[:, 0] == 0.5).all()
        st = s.loop_settings(N, model.sqp["dt"], period=PERIOD)
        refused(s.loop_start, st, 0.0, x, np.zeros((2, 4)), gait=skip, text="skip")
        with pytest.raises(ValueError):
            s.loop_start(st, 0.0, x, np.zeros((2, 4)), n_events=np.ones(2, np.int32), gait=good)
    finally:
        s.close()
