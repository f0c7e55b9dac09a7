"""The actuator model on the torque plant (include/hsqp_actuator.h, csrc/hsqp_actuator.h) on the CPU: the header and the exported entry points, and the
host build of the kernel source (tests/actuator/actuator_emu.cpp, -ffp-contract=off) against the numpy restatement tests/actuator_ref.py on top of
tests/plant_ref.py / tests/contact_ref.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import actuator_ref as A
import contact_ref as CR
import plant_ref as PL
import push_ref as P
import rollout_emu as E
import rollout_ref as R
from test_contact import contact_struct, grounded
from test_plant import L_ELBOW, plant_case, settings_struct
from test_rollout import rel, start_states
from wb_humanoid_mpc_amd import _abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
LIBDIR = os.path.join(ROOT, "wb_humanoid_mpc_amd")
NX, NU, NV, NJ = _abi.NX, _abi.NU, _abi.NV, _abi.NJ
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_pp = C.POINTER(_abi.Push)
_pl = C.POINTER(_abi.PlantSettings)
_as = C.POINTER(_abi.ActuatorSettings)
_cs = C.POINTER(_abi.ContactSettings)
D = 2.0 ** -6
HOLDS = {"off": 0.0, "2^-8": 2.0 ** -8, "0.003": 0.003}
LIMITED = dict(effort_limit=5.0, damping=0.05, friction=0.1)   # the setting of the rollout tests (tests/test_gpu_actuator.py uses the same)


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def actuator_struct(ac, enabled=1):
    st = _abi.ActuatorSettings()
    st.enabled, st.reserved, st.command_period, st.friction_velocity = enabled, 0, ac["command_period"], ac["friction_velocity"]
    st.effort_limit[:], st.damping[:], st.friction[:] = list(ac["effort_limit"]), list(ac["damping"]), list(ac["friction"])
    return st


# ---------------------------------------------------------------------------------------------- header, exports, defaults, argument errors
def test_header_compiles_and_the_library_exports_the_entry_points(tmp_path):
    src = tmp_path / "a.c"
    src.write_text('#include <stdio.h>\n#include "hsqp_actuator.h"\n'
                   'int main(void){ hsqp_actuator_settings s;\n'
                   ' void (*a)(hsqp_actuator_settings*) = hsqp_actuator_defaults;\n'
                   ' int (*b)(hsqp_handle*, const hsqp_actuator_settings*) = hsqp_actuator_set;\n'
                   ' int (*c)(hsqp_handle*) = hsqp_actuator_clear;\n'
                   ' int (*d)(hsqp_handle*, hsqp_actuator_settings*) = hsqp_actuator_get;\n'
                   ' int (*e)(hsqp_handle*, int, double*, double*, double*) = hsqp_actuator_last;\n'
                   ' int (*f)(hsqp_handle*, int, double*, double*, double*) = hsqp_actuator_last_device;\n'
                   ' s.enabled = 1; s.reserved = 0; s.command_period = s.effort_limit[HSQP_NJ - 1] = s.damping[0] = s.friction[0] = s.friction_velocity = 0.0;\n'
                   ' printf("%d %d %d\\n", HSQP_ABI_VERSION, a != 0 && b != 0 && c != 0 && d != 0 && e != 0 && f != 0, (int)sizeof s + s.enabled); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "a.o")])
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    assert len(_abi.ACTUATOR_ENTRY_POINTS) == 6
    for n in _abi.ACTUATOR_ENTRY_POINTS:
        assert n in names and getattr(lib, n).argtypes is not None, n
    assert C.sizeof(_abi.ActuatorSettings) == 16 + (3 * NJ + 1) * 8
    assert _abi.ABI_VERSION == 7           # additions only: no revision bump


def test_defaults_and_null_arguments():
    lib = solver.load_library()
    st = _abi.ActuatorSettings()
    st.reserved = 5
    lib.hsqp_actuator_defaults(C.byref(st))
    assert (st.enabled, st.reserved, st.command_period, st.friction_velocity) == (1, 0, 0.002, 0.01)
    assert list(st.effort_limit) == [np.inf] * NJ and list(st.damping) == [0.0] * NJ and list(st.friction) == [0.0] * NJ
    lib.hsqp_actuator_defaults(None)       # a NULL struct is ignored
    # a NULL handle is a bad argument, with or without a device
    out = np.zeros(NJ)
    assert lib.hsqp_actuator_set(None, C.byref(st)) == _abi.ERR_BAD_ARG
    assert lib.hsqp_actuator_set(None, None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_actuator_clear(None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_actuator_get(None, C.byref(st)) == _abi.ERR_BAD_ARG
    assert lib.hsqp_actuator_last(None, 1, _p(out), None, None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_actuator_last_device(None, 1, None, None, None) == _abi.ERR_BAD_ARG
    # the binding's struct builder: scalars broadcast, 23 values taken as they are

    class Stub:
        pass
    stub = Stub()
    stub.lib = lib
    s2 = solver.HipSqpSolver.actuator_settings(stub, command_period=0.0, effort_limit=np.arange(1, NJ + 1), damping=0.05, friction_velocity=0.02)
    assert list(s2.effort_limit) == list(map(float, range(1, NJ + 1))) and list(s2.damping) == [0.05] * NJ and list(s2.friction) == [0.0] * NJ
    assert (s2.enabled, s2.reserved, s2.command_period, s2.friction_velocity) == (1, 0, 0.0, 0.02)
    assert solver.HipSqpSolver.actuator_settings(stub, enabled=False).enabled == 0
    assert solver.HipSqpSolver.actuator_settings(stub).command_period == 0.002


# ---------------------------------------------------------------------------------------------- host build of the kernel source
def build_emu(path, *defines):
    lib = E.build(path, os.path.join("actuator", "actuator_emu.cpp"), "-ffp-contract=off", *defines)
    lib.ace_law.argtypes = [_as, _dp, _dp, _dp, _dp, _dp, _dp, _dp]
    lib.ace_tick.argtypes = [C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int), _dp]
    return lib


class Emu:
    def __init__(self, lib, model):
        self.lib, self.h = lib, E.create(lib, model)

    def close(self):
        self.lib.emu_destroy(self.h)

    def law(self, ac, pl, cmd, x):
        out = np.zeros((4, NJ))
        st = actuator_struct(ac)
        self.lib.ace_law(C.byref(st), _p(pl["kp"]), _p(pl["kd"]), _p(np.ascontiguousarray(cmd[0])), _p(np.ascontiguousarray(cmd[1])),
                         _p(np.ascontiguousarray(cmd[2])), _p(np.ascontiguousarray(x)), _p(out))
        return out

    def tick(self, s0, period, t):
        on, nxt = C.c_int(0), C.c_double(0.0)
        self.lib.ace_tick(s0, period, t, C.byref(on), C.byref(nxt))
        return bool(on.value), nxt.value

    def rollout(self, pl, ac, st, case, s0, x0, duration, n, pushes=None, ct=None, enabled=1):
        """(x, u, status, steps, rejected, last [B][3][23]); ac None: no actuator set; ct: a contact_ref setting (None: no ground)."""
        return E.rollout(self.lib, self.h, case, st, s0, x0, duration, n, plant=settings_struct(pl), actuator=None if ac is None else actuator_struct(ac, enabled),
                         contact=None if ct is None else contact_struct(ct), pushes=pushes)


@pytest.fixture(scope="module")
def emu(tmp_path_factory, model):
    e = Emu(build_emu(tmp_path_factory.mktemp("actuator") / "libactuator_emu.so"), model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def emu_reverse(tmp_path_factory, model):
    e = Emu(build_emu(tmp_path_factory.mktemp("actuator_rev") / "libactuator_emu_rev.so", "-DHSQP_EMU_REVERSE"), model)
    yield e
    e.close()


def same(a, b):
    return all(np.array_equal(va, vb, equal_nan=True) for va, vb in zip(a, b))


# ---------------------------------------------------------------------------------------------- the joint law, point-wise
def test_joint_law_matches_the_reference_point_wise(emu, model, rng):
    pl = PL.plant()
    lim = np.full(NJ, 5.0)
    lim[3], lim[17] = np.inf, np.inf
    ac = A.actuator(0.002, lim, 0.05 + 0.01 * np.arange(NJ), 0.1, 0.01)
    clamped = free = 0
    for i in range(8):
        x = start_states(model, False, rng, 1)[0]
        if i == 0:
            x[NV + 6:] = 0.0                                      # v = 0: no passive torque, whatever the friction
        if i == 1:
            x[NV + 6:] *= 1e-4                                    # far inside the regularisation
        cmd = (x[6:NV] + 0.02 * rng.standard_normal(NJ), x[NV + 6:] + 0.2 * rng.standard_normal(NJ), 4.0 * rng.standard_normal(NJ), np.zeros(12))
        got = emu.law(ac, pl, cmd, x)
        want = np.array(A.joint_law(ac, pl, cmd, x))
        # the same few operations in the same order, no contraction on either side: bits
        assert np.array_equal(got, want), np.abs(got - want).max()
        tau, tcmd, tact, tpas = got
        over = np.abs(tcmd) > lim
        clamped += int(over.sum())
        free += int((~over).sum())
        assert (np.abs(tact) <= lim).all() and np.array_equal(tact[~over], tcmd[~over]) and np.array_equal(np.abs(tact[over]), lim[over])
        assert not over[3] and not over[17]                       # +inf: never clamped
        if i == 0:
            assert (tpas == 0.0).all() and np.array_equal(tau, tact)
        else:
            assert (tpas * x[NV + 6:] < 0.0).all()                # the passive torques oppose the motion
            assert (np.abs(tpas) < ac["damping"] * np.abs(x[NV + 6:]) + ac["friction"]).all()
    assert clamped >= 8 and free >= 8, (clamped, free)
    # a NaN command stays NaN (the clamp is written with comparisons)
    cmd = (x[6:NV], x[NV + 6:], np.full(NJ, np.nan), np.zeros(12))
    assert np.isnan(emu.law(ac, pl, cmd, x)[:3]).all()


def test_tick_schedule(emu):
    for s0, period in ((0.0, 2.0 ** -8), (0.013, 0.003), (2.0 ** -5, 0.002), (0.003, 1e-7)):
        on, nxt = emu.tick(s0, period, s0)
        assert on and nxt == s0 + 1.0 * period
        for k in (1, 2, 7, 1000):
            t = s0 + k * period
            on, nxt = emu.tick(s0, period, t)
            assert on and nxt == s0 + (k + 1.0) * period, (s0, period, k)
            mid = s0 + (k + 0.5) * period
            assert emu.tick(s0, period, mid) == (False, nxt)
    # a period that cannot advance the time: the next tick is not after t (the rollout ends the instance)
    on, nxt = emu.tick(1.0, 1e-300, 1.0)
    assert not nxt > 1.0 or not np.isfinite(nxt)


# ---------------------------------------------------------------------------------------------- RK4 rollouts against actuator_ref
CASES = [(c, g, hold) for c in (R.FEEDFORWARD, R.FEEDBACK) for g in ("uniform", "events") for hold in HOLDS]


@pytest.mark.parametrize("controller,grid,hold", CASES)
def test_rk4_rollout_matches_numpy(emu, model, oracle, controller, grid, hold):
    """Printed: the worst relative x and u errors of the emulation against actuator_ref — the GPU tolerance of tests/test_gpu_actuator.py is ten times
    the x error (not below 1e-10).  Measured: x <= 2.91e-11, u <= 1.0e-12 over the twelve cases."""
    rng = np.random.default_rng(77 + controller)
    case = plant_case(model, grid, rng)
    pl = PL.plant()
    period = HOLDS[hold]
    ac = A.actuator(period, **LIMITED)
    # hold 2^-8: binary start, step 2^-8 — every tick is a step boundary and the first sample (s0 + 2^-7) a tick; 0.003: a sample inside a hold
    # interval, a partial last interval
    step = 2.0 ** -8 if hold == "2^-8" else 0.004
    st = R.settings(R.RK4, controller, initial_step=step)
    x0 = start_states(model, False, rng, 1)
    s0 = np.array([2.0 ** -7 if hold == "2^-8" else 0.003])
    pushes = [[P.push(L_ELBOW, s0[0] + 0.0015, 0.009, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0])]]
    x, u, status, steps, rej, last = emu.rollout(pl, ac, st, case, s0, x0, D, 2, pushes)
    pol = R.Policy(case["ut"], case["dt"], case["dts"], case["K"], case["uff"], 0, False)
    cl = A.ClosedLoop(oracle, model, pol, case["xt"], pl, controller, ac)
    segs = []
    xr, ur, sr, nr, rr, rec = A.rollout(cl, pol, st, s0[0], x0[0], D, 2, pushes[0], segments=segs)
    assert status[0] == sr == R.OK and rej[0] == rr == 0
    assert steps[0] == nr, (steps[0], nr)
    ex, eu = rel(x[0], xr), rel(u[0], ur)
    er = np.abs(last[0] - rec).max() / max(1.0, np.abs(rec).max())
    print(f"controller {controller} {grid} hold {hold}: steps {nr}, emulation against numpy: x error {ex:.2e}, u error {eu:.2e}, record error {er:.2e}")
    assert ex <= 1e-10 and eu <= 1e-9, (ex, eu)                  # the bounds of tests/test_plant.py::test_rk4_rollout_matches_numpy (unpushed), kept with the push
    # the record: tau_cmd ~ 1e2 N m from gains of 1e2 on errors of x: the x bound times kp + kd, relative
    assert er <= 1e-8, er
    assert (np.abs(last[0, 1]) <= 5.0).all() and (np.abs(last[0, 0]) > 5.0).any()      # saturated somewhere, clamped everywhere
    # the structure the case was chosen for
    n_sampled = sum(1 for s in segs if s[2])
    if hold == "off":
        assert n_sampled == 0
    else:
        assert n_sampled == len(A.ticks_upto(s0[0], period, s0[0] + D)), (n_sampled, segs)
        mid = s0[0] + D / 2
        on_tick = any(t == mid for t in A.ticks_upto(s0[0], period, s0[0] + D))
        assert on_tick == (hold == "2^-8")
        if hold == "0.003":
            assert (s0[0] + D - A.ticks_upto(s0[0], period, s0[0] + D)[-1]) < period * 0.999      # a partial last interval
    # and the model is felt: the plant without it ends elsewhere
    x1 = emu.rollout(pl, None, st, case, s0, x0, D, 2, pushes)[0]
    assert rel(x[0], x1[0]) > 1e-6


# ---------------------------------------------------------------------------------------------- inert settings, bit for bit
@pytest.mark.parametrize("ground", [False, True])
def test_a_neutral_or_disabled_setting_is_the_plant_bit_for_bit(emu, model, oracle, rng, ground):
    case = plant_case(model, "events", rng)
    pl = PL.plant()
    x0 = start_states(model, False, rng, 2)
    s0 = np.array([0.0, 0.013])
    ct = CR.contact(model, ground_height=min(grounded(oracle, model, x) for x in x0)) if ground else None
    pushes = [[P.push(L_ELBOW, 0.003, 0.0065, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0])], []]
    neutral = A.actuator(0.0)
    for integrator in (R.ODE45, R.RK4):
        for controller in (R.FEEDFORWARD, R.FEEDBACK):
            st = R.settings(integrator, controller, initial_step=0.004 if integrator == R.RK4 else 0.015)
            want = emu.rollout(pl, None, st, case, s0, x0, D, 2, pushes, ct)
            assert (want[2] == R.OK).all()
            got = emu.rollout(pl, neutral, st, case, s0, x0, D, 2, pushes, ct)
            assert same(got[:5], want[:5]), ("neutral", integrator, controller)
            assert np.isfinite(got[5]).all() and np.array_equal(got[5][:, 0], got[5][:, 1]) and (got[5][:, 2] == 0.0).all()
            off = emu.rollout(pl, A.actuator(0.002, **LIMITED), st, case, s0, x0, D, 2, pushes, ct, enabled=0)
            assert same(off[:5], want[:5]) and (off[5] == -7.0).all(), ("enabled = 0", integrator, controller)
            # each part of the model on its own is felt
            for ac in (A.actuator(0.002), A.actuator(0.0, effort_limit=5.0), A.actuator(0.0, damping=0.05), A.actuator(0.0, friction=0.1)):
                assert not same(emu.rollout(pl, ac, st, case, s0, x0, D, 2, pushes, ct)[:2], want[:2])


# ---------------------------------------------------------------------------------------------- chained calls
def test_chained_calls_equal_one_call_when_the_split_is_on_a_tick(emu, model, rng):
    case = plant_case(model, "events", rng)
    pl = PL.plant()
    ac = A.actuator(2.0 ** -9, **LIMITED)
    s0 = np.array([0.0, 2.0 ** -5, 2.0 ** -4])
    d = 2.0 ** -7
    x0 = start_states(model, False, rng, 3)
    pushes = [[], [P.push(L_ELBOW, 2.0 ** -5 + 0.003, 0.009, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0])], []]
    for integrator in (R.ODE45, R.RK4):
        for controller in (R.FEEDFORWARD, R.FEEDBACK):
            st = R.settings(integrator, controller, initial_step=0.003 if integrator == R.RK4 else 0.015)
            r = emu.rollout(pl, ac, st, case, s0, x0, 2 * d, 2, pushes)
            assert (r[2] == R.OK).all()
            a = emu.rollout(pl, ac, st, case, s0, x0, d, 1, pushes)
            b = emu.rollout(pl, ac, st, case, s0 + d, a[0][:, 0].copy(), d, 1, pushes)
            assert np.array_equal(a[0][:, 0], r[0][:, 0]) and np.array_equal(a[1][:, 0], r[1][:, 0]), (integrator, controller)
            assert np.array_equal(b[0][:, 0], r[0][:, 1]) and np.array_equal(b[1][:, 0], r[1][:, 1]), (integrator, controller)
            assert np.array_equal(a[3] + b[3], r[3]) and np.array_equal(b[5], r[5])
            # a split that is not on a tick restarts the schedule: another result
            ac3 = A.actuator(0.003, **LIMITED)
            r3 = emu.rollout(pl, ac3, st, case, s0, x0, 2 * d, 2, pushes)
            a3 = emu.rollout(pl, ac3, st, case, s0, x0, d, 1, pushes)
            b3 = emu.rollout(pl, ac3, st, case, s0 + d, a3[0][:, 0].copy(), d, 1, pushes)
            assert np.array_equal(a3[0][:, 0], r3[0][:, 0]) and not np.array_equal(b3[0][:, 0], r3[0][:, 1])


# ---------------------------------------------------------------------------------------------- the step cap bounds a tiny period
def test_a_period_far_below_the_step_ends_at_the_step_cap(emu, model, rng):
    case = plant_case(model, "uniform", rng)
    pl = PL.plant()
    x0 = start_states(model, False, rng, 1)
    for integrator in (R.ODE45, R.RK4):
        st = R.settings(integrator, R.FEEDFORWARD, initial_step=0.004, max_steps_per_second=50.0)
        x, u, status, steps, rej, last = emu.rollout(pl, A.actuator(1e-7), st, case, np.array([0.003]), x0, D, 1)
        assert status[0] == R.MAX_STEPS and steps[0] == 50, (status, steps)          # one step per interval between ticks, the cap's number of them
        assert np.isnan(x).all() and np.isnan(u).all() and np.isnan(last).all()
        # ... and one that cannot advance the time at all ends at once
        x, u, status, steps, rej, last = emu.rollout(pl, A.actuator(1e-300), st, case, np.array([1.0]), x0, D, 1)
        assert status[0] == R.MAX_STEPS and steps[0] == 0 and np.isnan(last).all()


# ---------------------------------------------------------------------------------------------- race check
def test_reverse_order_emulation_is_bit_identical(emu, emu_reverse, model, oracle, rng):
    case = plant_case(model, "events", rng)
    pl = PL.plant()
    x0 = start_states(model, False, rng, 2)
    s0 = np.array([0.0, 0.013])
    pushes = [[P.push(L_ELBOW, 0.003, 0.0065, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0])], []]
    ct = CR.contact(model, ground_height=min(grounded(oracle, model, x) for x in x0))
    for period in (0.0, 0.003):
        for integrator in (R.ODE45, R.RK4):
            for c in (None, ct):
                st = R.settings(integrator, R.FEEDBACK, initial_step=0.004 if integrator == R.RK4 else 0.015)
                a = emu.rollout(pl, A.actuator(period, **LIMITED), st, case, s0, x0, D, 2, pushes, c)
                b = emu_reverse.rollout(pl, A.actuator(period, **LIMITED), st, case, s0, x0, D, 2, pushes, c)
                assert (a[2] == R.OK).all()
                assert same(a, b), (period, integrator)


def test_the_workspaces_fit_the_lds(emu):
    plain, ground = emu.lib.emu_ws_bytes(0, 1, 0, 1, 0), emu.lib.emu_ws_bytes(0, 1, 1, 1, 0)
    print(f"rollout workspace under the actuator model: {plain} bytes, on the ground {ground} bytes")
    assert plain <= 65536 and ground <= 65536 and ground > plain


# ---------------------------------------------------------------------------------------------- sanitizers: a program of its own
def test_held_rollout_and_record_under_sanitizers(tmp_path, model):
    exe, desc = tmp_path / "actuator_sanitize", tmp_path / "desc.bin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "actuator", "actuator_emu.cpp"),
                           os.path.join(ROOT, "tests", "actuator", "actuator_sanitize.cpp"), "-o", str(exe)])
    desc.write_bytes(bytes(model.desc))
    out = subprocess.check_output([str(exe), str(desc)], text=True)
    assert out.strip() == "actuator ok"
