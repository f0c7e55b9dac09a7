"""The per-foot swing heights read from the height map (include/hsqp_perceive.h) on the MI355X: k_foot_heights and its device twin against the numpy
restatement (tests/perceive_ref.py) — footholds within the project's device bound, heights bit-equal to hsqp_terrain_eval at the returned footholds —,
hsqp_upload_reference_heights against the mirror's node parameters, against hsqp_upload_reference_ground on constant rows bit for bit and on the ledge,
the resident loop with the setting on against the public calls it replaces bit for bit (plain, the ground estimate on, a resident gait, the observation
model with delays), against the loop without the setting on a flat ground bit for bit, one instance failing alone, and the refusals.
Shapes: B = 3, N = 8, max_events = 6, three cycles (tests/perceive_ref.py, case); the loop on the flow plant with the serial recursion."""
import ctypes as C
import signal

import numpy as np
import pytest

import ground_ref as G
import observe_ref as O
import perceive_ref as P
from test_gpu_feedback_policy import DeviceBuffer
from test_gpu_grid import int_buffer
from test_ground import ATOL_DEVICE
from test_perceive import bits, structure_holds
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd import reference as ref
from wb_humanoid_mpc_amd.reference import ModeSchedule, gait_settings, swing_config
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu

NX, NU, NJ, KNOTS = _abi.NX, _abi.NU, _abi.NJ, _abi.CMD_KNOTS
B, N, E = P.B, P.N, P.E
CYCLES, PERIOD, ALPHA = 3, 1.0 / 60.0, 0.8
TOL_PARAMS = 1e-13   # tests/test_device_params.py: the device's node parameters against the mirror's
_ip, _dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)


@pytest.fixture(autouse=True)
def time_limit():
    def expired(signum, frame):
        raise TimeoutError("test_gpu_perceive: a test ran past its 120 s limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


@pytest.fixture(scope="module")
def case(model):
    return P.case(model)


def lay_terrain(h, case, flat=False):
    """The case's maps, placements and contact ground heights resident in the handle (flat: every instance on map -1 over a ground at 0)."""
    rows = len(case["x"])
    h.set_contact(enabled=False)
    h.set_contact_instances(np.column_stack([np.zeros(rows) if flat else case["ground"], np.full(rows, 0.6)]))
    h.set_terrain_maps([(m["H"], m["cell"]) for m in case["maps"]])
    h.set_terrain_instances([dict(map=-1)] * rows if flat else case["place"])


@pytest.fixture
def s(model, case):
    h = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    lay_terrain(h, case)
    yield h
    h.close()


def settings(s, model, integrator="ode45", controller="feedforward"):
    return s.loop_settings(N, model.sqp["dt"], period=PERIOD, filter_alpha=ALPHA, iterations=1, take_step=True, linesearch=True, integrator=integrator,
                           controller=controller)


# ---------------------------------------------------------------------------------------------- 1. the kernel against the mirror
def test_foot_heights_and_the_device_twin_equal_the_mirror(s, model, case):
    CANARY = -12345.678
    began = ahead = 0
    for t in P.TIMES:
        lift, touch, fxy = s.foot_heights(case["x"], t, case["ne"], case["ev"], case["seq"], case["tt"], case["ts"], case["offset"])
        want = P.batch_sequences(model, case, t)
        dxy, dh = np.abs(fxy - want[2]).max(), max(np.abs(lift - want[0]).max(), np.abs(touch - want[1]).max())
        print(f"t = {t}: footholds max |d| {dxy:.3e} (bound {ATOL_DEVICE:.0e}), heights against the mirror {dh:.3e}")
        assert dxy <= ATOL_DEVICE
        assert dh <= 4 * ATOL_DEVICE                                       # (the ledge's slope is 3: a foothold off by d moves a height by 3 d)
        sample = s.terrain_height(fxy.reshape(B, -1, 2))[0].reshape(B, 2, E + 1)
        structure_holds(case, lift, touch, fxy, sample)                    # the heights ARE hsqp_terrain_eval at the returned footholds, bit for bit
        for b in range(B):
            p_now = int(np.searchsorted(case["ev"][b][:case["ne"][b]], t, side="left"))
            for f in range(2):
                for a, _ in P.runs([ref.mode_to_contact_flags(int(m))[f] for m in case["seq"][b][:case["ne"][b] + 1]]):
                    began, ahead = began + (a <= p_now), ahead + (a > p_now)
        # the device twin: the same bits, nothing written past the rows; once with and once without the footholds
        bufs = [DeviceBuffer((B, NX)), int_buffer(case["ne"], B), DeviceBuffer((B, E)), int_buffer(case["seq"], B), DeviceBuffer((B, KNOTS)), DeviceBuffer((B, KNOTS, NX)),
                DeviceBuffer((B + 1, 2, E + 1), fill=CANARY), DeviceBuffer((B + 1, 2, E + 1), fill=CANARY), DeviceBuffer((B + 1, 2, E + 1, 2), fill=CANARY)]
        try:
            bufs[0].upload(case["x"]); bufs[2].upload(case["ev"]); bufs[4].upload(case["tt"]); bufs[5].upload(case["ts"])
            for with_xy in (True, False):
                s.foot_heights_device(B, t, bufs[0].ptr.value, E, bufs[1].ptr.value, bufs[2].ptr.value, bufs[3].ptr.value, KNOTS, bufs[4].ptr.value, bufs[5].ptr.value,
                                      case["offset"], bufs[6].ptr.value, bufs[7].ptr.value, bufs[8].ptr.value if with_xy else 0)
                dl, dt_, dx = bufs[6].numpy(), bufs[7].numpy(), bufs[8].numpy()
                assert np.array_equal(bits(dl[:B]), bits(lift)) and np.array_equal(bits(dt_[:B]), bits(touch)) and np.array_equal(bits(dx[:B]), bits(fxy)), t
                assert (dl[B] == CANARY).all() and (dt_[B] == CANARY).all() and (dx[B] == CANARY).all()
        finally:
            for b in bufs:
                b.free()
    assert began > 20 and ahead > 20
    # a batch of one, and the ledge case of tests/test_perceive.py on the device
    one = s.foot_heights(case["x"][:1], 0.3, case["ne"][:1], case["ev"][:1], case["seq"][:1], case["tt"][:1], case["ts"][:1], case["offset"])
    lift, touch, fxy = s.foot_heights(case["x"], 0.3, case["ne"], case["ev"], case["seq"], case["tt"], case["ts"], case["offset"])
    assert all(np.array_equal(bits(a[0]), bits(b[0])) for a, b in zip(one, (lift, touch, fxy)))
    assert np.array_equal(lift[0, 0, 1:3], [0.0, 0.0]) and np.array_equal(touch[0, 0, 1:3], np.full(2, P.LEDGE_HEIGHT + case["offset"]))
    # a non-finite state: NaN rows for that instance alone
    x = case["x"].copy()
    x[1, 40] = np.inf
    sick = s.foot_heights(x, 0.3, case["ne"], case["ev"], case["seq"], case["tt"], case["ts"], case["offset"])
    for a, b in zip(sick, (lift, touch, fxy)):
        assert np.isnan(a[1, :, :5]).all() and np.array_equal(bits(a[[0, 2]]), bits(b[[0, 2]]))


# ---------------------------------------------------------------------------------------------- 2. the upload with the three-argument planner
def test_upload_reference_heights(s, model, case):
    sw = swing_config(model)
    ref_args = (case["ne"], case["ev"], case["seq"], case["tt"], case["ts"], sw)
    for t0, dt in ((0.0, 0.0625), (1.5, 0.25)):                             # nodes exactly on events of instances 0, 1 (0.125 .. 0.5) and of instance 2 (2.0, 3.0)
        lift, touch, _ = s.foot_heights(case["x"], t0, case["ne"], case["ev"], case["seq"], case["tt"], case["ts"], case["offset"])
        s.upload_reference_heights(case["x"], N, dt, t0, *ref_args, lift, touch, mode="cold")
        got = s.device_params()
        for b in range(B):
            n_ev = int(case["ne"][b])
            sched = ModeSchedule(case["ev"][b][:n_ev], case["seq"][b][:n_ev + 1])
            want = ref.build_node_params(model, sched, case["knots"][b], t0, dt, N, lift=lift[b], touch=touch[b])
            print(f"t0 = {t0}, instance {b}: node parameters against the mirror, max |d| {np.abs(got[b] - want).max():.3e} (bound {TOL_PARAMS:.0e})")
            np.testing.assert_allclose(got[b], want, rtol=0, atol=TOL_PARAMS)
        if t0 == 0.0:
            # the ledge instance: its left foot lands at 0.375 = node 6, where its z reference is the ledge's height plus the offset; a scalar terrain height
            # of 0 (where the foot stands now) would put it 3 cm inside the ledge
            z = got[0, 6, _abi.P_SWING]
            assert got[0, 6, _abi.P_CONTACT] == 0.0 and got[0, 7, _abi.P_CONTACT] == 1.0
            assert abs(z - (P.LEDGE_HEIGHT + case["offset"])) <= ATOL_DEVICE
            assert got[0, 7, _abi.P_SWING] == P.LEDGE_HEIGHT and got[0, 0, _abi.P_SWING] == 0.0   # the stance references: the run's own height
    # constant rows are the per-instance terrain height, bit for bit: the parameters and the cold start
    g = np.array([0.03, -0.0175, 0.0])
    lift = np.repeat(g[:, None, None], 2 * (E + 1), axis=2).reshape(B, 2, E + 1)
    touch = lift + case["offset"]
    lift[:, :, 5:], touch[:, :, 5:] = np.nan, np.inf                        # phases past n_events = 4 are never read, and not checked
    s.upload_reference_ground(case["x"], N, 0.0625, 0.0, *ref_args, g, mode="cold")
    want = (s.device_params(), *s.device_trajectory())
    s.upload_reference_heights(case["x"], N, 0.0625, 0.0, *ref_args, lift, touch, mode="cold")
    got = (s.device_params(), *s.device_trajectory())
    for a, b in zip(got, want):
        assert np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------- 3. the loop against the calls it replaces
def by_hand(s, model, case, cycles, gait=None, delays=None, ground=False):
    """The cycles through the public calls: (hsqp_observe_eval,) hsqp_command_targets, (hsqp_gait_update,) (hsqp_ground_estimate and the adds,)
    hsqp_foot_heights, hsqp_upload_reference_heights, hsqp_iterate_device, hsqp_rollout_policy."""
    dt, sw = model.sqp["dt"], swing_config(model)
    x, cmd = case["x"].copy(), case["cmd"].copy()
    rows = len(x)
    vf, t = cmd.copy(), 0.0
    k = delays[1] if delays else 0
    ring = O.Ring(rows, sum(delays)) if delays else None
    g = np.zeros(rows)
    ne, ev, seq = case["ne"], case["ev"], case["seq"]
    if gait is not None:
        s.gait_reset(gait, rows, O.problem_time(t, k, PERIOD) if delays else t)
    xs, us, heights = [], [], None
    for c in range(cycles):
        y = s.observe(ring.cycle(c, x, np.full(rows, c == 0)), c) if delays else x
        tp = O.problem_time(t, k, PERIOD) if delays else t
        tt, ts, vf = s.command_targets(cmd, y, tp, N * dt, filter_alpha=ALPHA, v_filt=vf)
        if gait is not None:
            ne, ev, seq = s.gait_update(tp, N * dt, vf, y)
        if ground:
            g, _ = s.ground_estimate(y, tp, ne, ev, seq, g, 0.0)
            ts = G.shift_knots(ts, g)
        heights = s.foot_heights(y, tp, ne, ev, seq, tt, ts, sw.touch_down_height_offset)
        s.upload_reference_heights(y, N, dt, tp, ne, ev, seq, tt, ts, sw, heights[0], heights[1], mode="cold" if c == 0 else "shift")
        s.iterate(1, take_step=True, linesearch=True)
        r = s.rollout_policy(np.full(rows, O.policy_time(k, PERIOD) if delays else 0.0), x, PERIOD, 1)
        x = r["x"][:, 0].copy()
        xs.append(x); us.append(r["u"][:, 0].copy())
        t += PERIOD
    X, U = s.device_trajectory()
    return dict(x=np.array(xs), u=np.array(us), vf=vf, t=t, X=X, U=U, stamps=s.stamps(), par=s.device_params(), heights=heights, g=g)


def assert_loop_equals(s, got, want):
    t, x_end, vf = s.loop_state()
    X, U = s.device_trajectory()
    assert got["cycles_done"] == len(want["x"]) and np.isfinite(got["x"]).all() and np.isfinite(got["u"]).all()
    assert np.array_equal(got["x"], want["x"]) and np.array_equal(got["u"], want["u"])
    assert np.array_equal(vf, want["vf"]) and np.array_equal(x_end, want["x"][-1]) and t == want["t"]
    assert np.array_equal(X, want["X"]) and np.array_equal(U, want["U"]) and np.array_equal(s.stamps(), want["stamps"])
    assert np.array_equal(bits(s.device_params()), bits(want["par"]))
    for a, b in zip(s.loop_foot_heights(), want["heights"]):                 # the rows of the last completed cycle
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("variant", ["plain", "ground", "gait", "observed"])
def test_loop_equals_the_calls_it_replaces(s, model, case, variant):
    gait = gait_settings(model) if variant == "gait" else None
    delays = (1, 1) if variant == "observed" else None
    if delays:
        rng = np.random.default_rng(5)
        s.set_observation(sensor_delay=1, compute_delay=1, seed=2026)
        s.set_observation_instances(0.01 * rng.standard_normal((B, NX)), np.abs(5e-3 * rng.standard_normal((B, NX))))
    want = by_hand(s, model, case, CYCLES, gait=gait, delays=delays, ground=variant == "ground")
    if gait is not None:
        s.loop_start(settings(s, model), 0.0, case["x"], case["cmd"], gait=gait)
    else:
        s.loop_start(settings(s, model), 0.0, case["x"], case["cmd"], case["ne"], case["ev"], case["seq"])
    if variant == "ground":
        s.loop_ground(s.ground_settings())
    s.loop_perceive()
    assert not any(a.any() for a in s.loop_foot_heights())                   # zeros before the first cycle
    got = s.loop_run(CYCLES)
    assert_loop_equals(s, got, want)
    if variant == "ground":
        assert np.array_equal(s.loop_ground_state()[0], want["g"])
    if variant in ("plain", "ground"):
        # the test's own preconditions: the rows differ from foot to foot and from lift-off to touch-down somewhere — no scalar terrain height says this
        lift, touch, _ = want["heights"]
        assert np.ptp(lift[0, :, :5]) > 0.02 and np.abs(lift[2, 0, :5] - lift[2, 1, :5]).max() > 1e-3
        # the device getter
        bufs = [DeviceBuffer((B, 2, E + 1)), DeviceBuffer((B, 2, E + 1)), DeviceBuffer((B, 2, E + 1, 2))]
        try:
            s.loop_foot_heights_device(bufs[0].ptr.value, bufs[1].ptr.value, bufs[2].ptr.value)
            for a, b in zip(bufs, want["heights"]):
                assert np.array_equal(bits(a.numpy()), bits(b))
        finally:
            for b in bufs:
                b.free()
        # and the setting is felt: the same loop without it is another run
        s.loop_start(settings(s, model), 0.0, case["x"], case["cmd"], case["ne"], case["ev"], case["seq"])
        if variant == "ground":
            s.loop_ground(s.ground_settings())
        plain = s.loop_run(CYCLES)
        assert np.isfinite(plain["x"]).all() and not np.array_equal(plain["x"], got["x"])


def test_on_a_flat_ground_the_setting_changes_nothing(s, model, case):
    """Every instance on map -1 over a ground at 0, terrain_height 0: the rows are (0, 0 + offset), the constants of the two-argument form."""
    lay_terrain(s, case, flat=True)
    runs = []
    for on in (False, True):
        s.loop_start(settings(s, model), 0.0, case["x"], case["cmd"], case["ne"], case["ev"], case["seq"])
        if on:
            s.loop_perceive()
        runs.append(s.loop_run(CYCLES))
        if on:
            lift, touch, _ = s.loop_foot_heights()
            assert not lift.any() and np.array_equal(touch[:, :, :5], np.full((B, 2, 5), case["offset"]))
    for k in ("x", "u"):
        assert np.isfinite(runs[0][k]).all() and np.array_equal(bits(runs[0][k]), bits(runs[1][k])), k


def test_a_nan_instance_fails_alone(s, model, case):
    runs = []
    for sick in (False, True):
        x0 = case["x"].copy()
        if sick:
            x0[1, 7] = np.nan
        s.loop_start(settings(s, model), 0.0, x0, case["cmd"], case["ne"], case["ev"], case["seq"])
        s.loop_isolate(s.episode_settings("park"), x_reset=case["x"])
        s.loop_perceive()
        first = s.loop_run(1)
        rows1 = s.loop_foot_heights()
        rest = s.loop_run(CYCLES - 1)
        runs.append(dict(x=np.concatenate([first["x"], rest["x"]]), u=np.concatenate([first["u"], rest["u"]]), rows1=rows1, rows=s.loop_foot_heights(),
                         ep=s.loop_episodes()))
    a, b = runs
    keep = [0, 2]
    assert (a["ep"]["state"] == _abi.EP_ALIVE).all() and b["ep"]["state"][1] != _abi.EP_ALIVE and (b["ep"]["state"][keep] == _abi.EP_ALIVE).all()
    assert b["ep"]["n_failures"][1] >= 1 and np.isfinite(a["x"]).all()
    for k in ("x", "u"):
        assert np.array_equal(bits(a[k][:, keep]), bits(b[k][:, keep])), k
    for ra, rb in zip(a["rows1"] + a["rows"], b["rows1"] + b["rows"]):
        assert np.array_equal(bits(ra[keep]), bits(rb[keep]))
    assert all(np.isnan(r[1, :, :5]).all() for r in b["rows1"])              # the failing cycle's rows
    assert all(np.isfinite(r[1]).all() for r in b["rows"])                   # parked at x_reset: the same rule from its own state


# ---------------------------------------------------------------------------------------------- 4. refusals and lifetime
def test_refusals_and_lifetime(s, model, cmodel, case):
    lib = s.lib
    ne, ev, seq, x, tt, ts = case["ne"], case["ev"], case["seq"], case["x"], case["tt"], case["ts"]
    lift, touch, fxy = np.zeros((B, 2, E + 1)), np.zeros((B, 2, E + 1)), np.zeros((B, 2, E + 1, 2))
    Pd, Pi = lambda a: a.ctypes.data_as(_dp), lambda a: a.ctypes.data_as(_ip)  # noqa: E731

    def refused(h, what, name, *args):
        rc = getattr(lib, name)(h.h, *args)
        msg = lib.hsqp_last_error(h.h).decode()
        assert rc == _abi.ERR_BAD_ARG and name in msg and what in msg, (name, what, rc, msg)

    def call(name="hsqp_foot_heights", batch=B, t=0.1, max_events=E, n_knots=KNOTS, offset=-0.001, arrays=None):
        a = [Pd(x), Pi(ne), Pd(ev), Pi(seq), Pd(tt), Pd(ts), Pd(lift), Pd(touch), Pd(fxy)] if arrays is None else arrays
        return (name, batch, t, a[0], max_events, a[1], a[2], a[3], n_knots, a[4], a[5], offset, a[6], a[7], a[8])

    for name in ("hsqp_foot_heights", "hsqp_foot_heights_device"):
        refused(s, "batch", *call(name, batch=0))
        refused(s, "batch", *call(name, batch=B + 1))
        refused(s, "t not finite", *call(name, t=float("nan")))
        refused(s, "touch_down_height_offset", *call(name, offset=float("inf")))
        refused(s, "max_events", *call(name, max_events=0))
        refused(s, "n_knots", *call(name, n_knots=0))
        for k in range(8):                                                   # foothold_xy may be NULL, nothing else
            arrays = [Pd(x), Pi(ne), Pd(ev), Pi(seq), Pd(tt), Pd(ts), Pd(lift), Pd(touch), Pd(fxy)]
            arrays[k] = None
            refused(s, "null array", *call(name, arrays=arrays))
    bad = ne.copy()
    for v in (E + 1, 0):
        bad[2] = v
        refused(s, "n_events", *call(arrays=[Pd(x), Pi(bad), Pd(ev), Pi(seq), Pd(tt), Pd(ts), Pd(lift), Pd(touch), Pd(fxy)]))
    assert lib.hsqp_foot_heights(s.h, *call(arrays=[Pd(x), Pi(ne), Pd(ev), Pi(seq), Pd(tt), Pd(ts), Pd(lift), Pd(touch), None])[1:]) == 0   # foothold_xy NULL
    # the upload: a non-finite entry inside the phases of an instance is refused and leaves the resident problem alone, one past them is not read
    dt, sw = model.sqp["dt"], swing_config(model)
    args = (x, N, dt, 0.0, ne, ev, seq, tt, ts, sw)
    rows = s.foot_heights(x, 0.0, ne, ev, seq, tt, ts, case["offset"])
    s.upload_reference_heights(*args, rows[0], rows[1])
    before = s.device_params()
    for which in (0, 1):
        broken = [rows[0].copy(), rows[1].copy()]
        broken[which][2, 1, 4] = np.nan
        with pytest.raises(HsqpError) as ei:
            s.upload_reference_heights(*args, *broken)
        assert ei.value.code == _abi.ERR_BAD_ARG and "hsqp_upload_reference_heights" in str(ei.value) and "instance 2" in str(ei.value)
    assert np.array_equal(bits(s.device_params()), bits(before))
    broken = [rows[0].copy(), rows[1].copy()]
    broken[0][2, 1, 5] = np.nan
    s.upload_reference_heights(*args, *broken)
    assert np.array_equal(bits(s.device_params()), bits(before))
    refused(s, "null", "hsqp_upload_reference_heights", None, None, Pd(lift), Pd(touch))
    # the loop entry points without a loop
    ok = s.perceive_settings()
    refused(s, "no loop started", "hsqp_loop_perceive", C.byref(ok))
    refused(s, "no loop started", "hsqp_loop_foot_heights", Pd(lift), Pd(touch), Pd(fxy))
    refused(s, "no loop started", "hsqp_loop_foot_heights_device", None, None, None)
    # a centroidal handle
    c = HipSqpSolver(cmodel, max_nodes=N, max_batch=B)
    try:
        refused(c, "whole-body handles only", *call("hsqp_foot_heights"))
        refused(c, "whole-body handles only", *call("hsqp_foot_heights_device"))
        refused(c, "whole-body handles only", "hsqp_upload_reference_heights", None, None, Pd(lift), Pd(touch))
        refused(c, "whole-body handles only", "hsqp_loop_perceive", C.byref(ok))
        refused(c, "whole-body handles only", "hsqp_loop_foot_heights", Pd(lift), Pd(touch), Pd(fxy))
        refused(c, "whole-body handles only", "hsqp_loop_foot_heights_device", None, None, None)
    finally:
        c.close()
    # a handle without a terrain: no maps, then maps without a placement table
    bare = HipSqpSolver(model, max_nodes=N, max_batch=B, linesearch=True, riccati="serial")
    try:
        refused(bare, "no terrain resident", *call("hsqp_foot_heights"))
        bare.set_terrain_maps([(m["H"], m["cell"]) for m in case["maps"]])
        refused(bare, "no terrain resident", *call("hsqp_foot_heights_device"))
        bare.loop_start(settings(bare, model), 0.0, case["x"], case["cmd"], ne, ev, seq)
        refused(bare, "no terrain resident", "hsqp_loop_perceive", C.byref(ok))
        plain = bare.loop_run(2)                                             # (a refused switch leaves the loop as it was)
        assert plain["cycles_done"] == 2 and np.isfinite(plain["x"]).all()
    finally:
        bare.close()
    # a started loop
    start = lambda: s.loop_start(settings(s, model), 0.0, case["x"], case["cmd"], ne, ev, seq)  # noqa: E731
    start()
    refused(s, "are off", "hsqp_loop_foot_heights", Pd(lift), Pd(touch), Pd(fxy))
    s.loop_perceive()
    assert s.loop_run(1)["cycles_done"] == 1
    kept = s.loop_foot_heights()
    refused(s, "0 or 1", "hsqp_loop_perceive", C.byref(_abi.PerceiveSettings(enabled=2)))
    refused(s, "0 or 1", "hsqp_loop_perceive", C.byref(_abi.PerceiveSettings(enabled=1, reserved=1)))
    for a, b in zip(s.loop_foot_heights(), kept):                            # a refused call leaves the setting, and the rows, in place
        assert np.array_equal(bits(a), bits(b))
    on = s.loop_run(1)
    # off again: NULL settings, enabled 0, and every start
    for off in (lambda: s.loop_perceive(on=False), lambda: s.loop_perceive(s.perceive_settings(enabled=False))):
        start()
        s.loop_perceive()
        off()
        refused(s, "are off", "hsqp_loop_foot_heights", Pd(lift), Pd(touch), Pd(fxy))
    start()
    plain = s.loop_run(2)
    start()
    s.loop_perceive()
    assert s.loop_run(1)["cycles_done"] == 1
    start()                                                                  # hsqp_loop_start switches the setting off again
    refused(s, "are off", "hsqp_loop_foot_heights", Pd(lift), Pd(touch), Pd(fxy))
    again = s.loop_run(2)
    assert np.array_equal(plain["x"], again["x"]) and np.array_equal(plain["u"], again["u"]) and np.isfinite(on["x"]).all()
    s.upload_reference_warm(x, N, dt, 0.0, ne, ev, seq, tt, ts, sw, mode="cold")                  # an upload ends the loop
    refused(s, "no loop started", "hsqp_loop_perceive", C.byref(ok))
