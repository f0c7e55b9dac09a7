"""The torque plant of the rollout (include/hsqp_plant.h, csrc/hsqp_plant.h) on the CPU: the header and the exported entry points, and the host
build of the kernel source (tests/plant/plant_emu.cpp, -ffp-contract=off) against the numpy restatement tests/plant_ref.py on the oracle's
unchanged full_dynamics / foot_kinematics / body_placements / flow_map."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plant_ref as PL
import push_ref as P
import rollout_emu as E
import rollout_ref as R
from test_rollout import make_case, rel, start_states, state_input
from wb_humanoid_mpc_amd import _abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
LIBDIR = os.path.join(ROOT, "wb_humanoid_mpc_amd")
NX, NU, NV, NJ = _abi.NX, _abi.NU, _abi.NV, _abi.NJ
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_pp = C.POINTER(_abi.Push)
_pl = C.POINTER(_abi.PlantSettings)
BASE, L_FOOT, R_FOOT, TORSO, L_ELBOW = 0, 6, 12, 15, 19   # links of the G1 tree (data/g1_wb.json)
D = 2.0 ** -6
# accelerations against np.linalg.solve: eps cond(M) ~ 2.5e-11 at the measured cond(M) = 1.1e5 (armature 0), 40 x margin
ACC_TOL = 1e-9


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def settings_struct(pl, kind=_abi.PLANT_TORQUE):
    st = _abi.PlantSettings()
    st.kind, st.reserved, st.lookahead = kind, 0, pl["lookahead"]
    st.kp[:], st.kd[:], st.armature[:] = list(pl["kp"]), list(pl["kd"]), list(pl["armature"])
    return st


# ---------------------------------------------------------------------------------------------- header, exports, defaults, argument errors
def test_header_compiles_and_the_library_exports_the_entry_points(tmp_path):
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include "hsqp_plant.h"\n'
                   'int main(void){ hsqp_plant_settings s;\n'
                   ' void (*a)(hsqp_plant_settings*) = hsqp_plant_defaults;\n'
                   ' int (*b)(hsqp_handle*, const hsqp_plant_settings*) = hsqp_plant_set;\n'
                   ' int (*c)(hsqp_handle*) = hsqp_plant_clear;\n'
                   ' int (*d)(hsqp_handle*, hsqp_plant_settings*) = hsqp_plant_get;\n'
                   ' s.kind = HSQP_PLANT_TORQUE; s.reserved = HSQP_PLANT_FLOW; s.lookahead = s.kp[HSQP_NJ - 1] = s.kd[0] = s.armature[0] = 0.0;\n'
                   ' printf("%d %d %d\\n", HSQP_ABI_VERSION, a != 0 && b != 0 && c != 0 && d != 0, (int)sizeof s + s.kind); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "p.o")])
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.PLANT_ENTRY_POINTS:
        assert n in names and getattr(lib, n).argtypes is not None, n
    assert C.sizeof(_abi.PlantSettings) == 16 + 3 * NJ * 8 and (_abi.PLANT_FLOW, _abi.PLANT_TORQUE) == (0, 1)
    assert _abi.ABI_VERSION == 7           # additions only: no revision bump


def test_defaults_and_null_arguments():
    lib = solver.load_library()
    st = _abi.PlantSettings()
    st.reserved = 5
    lib.hsqp_plant_defaults(C.byref(st))
    assert (st.kind, st.reserved, st.lookahead) == (_abi.PLANT_TORQUE, 0, 0.005)
    assert list(st.kp) == [1200.0] * NJ and list(st.kd) == [10.0] * NJ and list(st.armature) == [0.0] * NJ
    lib.hsqp_plant_defaults(None)          # a NULL struct is ignored
    # a NULL handle is a bad argument, with or without a device
    assert lib.hsqp_plant_set(None, C.byref(st)) == _abi.ERR_BAD_ARG
    assert lib.hsqp_plant_set(None, None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_plant_clear(None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_plant_get(None, C.byref(st)) == _abi.ERR_BAD_ARG
    # the binding's struct builder: scalars broadcast, 23 values taken as they are
    class Stub:
        pass
    stub = Stub()
    stub.lib = lib
    s2 = solver.HipSqpSolver.plant_settings(stub, "torque", kp=100.0, kd=np.arange(NJ), armature=0.01, lookahead=0.0)
    assert list(s2.kp) == [100.0] * NJ and list(s2.kd) == list(map(float, range(NJ))) and list(s2.armature) == [0.01] * NJ and s2.lookahead == 0.0
    assert solver.HipSqpSolver.plant_settings(stub, "flow").kind == _abi.PLANT_FLOW


# ---------------------------------------------------------------------------------------------- host build of the kernel source
def build_emu(path, *defines):
    lib = E.build(path, os.path.join("plant", "plant_emu.cpp"), "-ffp-contract=off", *defines)
    lib.ple_accel.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, C.c_int, _pp, _dp]
    lib.ple_tau.argtypes = [C.c_void_p, _dp, _dp, _dp]
    lib.ple_eval.argtypes = [C.c_void_p, _pl, C.c_int, C.c_int, _dp, C.c_double, _dp, _dp, _dp, _dp, C.c_int, C.c_int, C.c_double, _dp, C.c_int, _pp, _dp]
    return lib


class Emu:
    def __init__(self, lib, model):
        self.lib, self.h = lib, E.create(lib, model)

    def close(self):
        self.lib.emu_destroy(self.h)

    def accel(self, x, W, tau, armature, pushes=()):
        _, tab, _ = solver.HipSqpSolver.pack_pushes([list(pushes)])
        vd = np.zeros(NV)
        self.lib.ple_accel(self.h, _p(np.ascontiguousarray(x)), _p(np.ascontiguousarray(W)), _p(np.ascontiguousarray(tau)), _p(np.ascontiguousarray(armature)),
                           len(pushes), C.cast(tab, _pp), _p(vd))
        return vd

    def tau(self, x, u):
        t = np.zeros(NJ)
        self.lib.ple_tau(self.h, _p(np.ascontiguousarray(x)), _p(np.ascontiguousarray(u)), _p(t))
        return t

    def eval(self, pl, controller, case, s, x, pushes=()):
        _, tab, _ = solver.HipSqpSolver.pack_pushes([list(pushes)])
        k = np.zeros(NX)
        st = settings_struct(pl)
        self.lib.ple_eval(self.h, C.byref(st), controller, len(case["ut"]), _p(case["dts"]), case["dt"], _p(case["xt"]), _p(case["ut"]), _p(case["K"]), _p(case["uff"]),
                          0, len(case["K"]), s, _p(np.ascontiguousarray(x)), len(pushes), C.cast(tab, _pp), _p(k))
        return k

    def rollout(self, pl, st, case, s0, x0, duration, n, pushes=None):
        return E.rollout(self.lib, self.h, case, st, s0, x0, duration, n, plant=settings_struct(pl), pushes=pushes)[:5]


@pytest.fixture(scope="module")
def emu(tmp_path_factory, model):
    e = Emu(build_emu(tmp_path_factory.mktemp("plant") / "libplant_emu.so"), model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def emu_reverse(tmp_path_factory, model):
    e = Emu(build_emu(tmp_path_factory.mktemp("plant_rev") / "libplant_emu_rev.so", "-DHSQP_EMU_REVERSE"), model)
    yield e
    e.close()


def plant_case(model, grid, rng):
    """make_case of tests/test_rollout.py with a nominal state trajectory xt [N + 1][58] that drifts from node to node."""
    case = make_case(model, False, grid, rng)
    N = len(case["ut"])
    xa, xb = state_input(model, False, rng, 0.5)[0], state_input(model, False, rng, 0.5)[0]
    case["xt"] = np.ascontiguousarray([xa + 0.01 * k * (xb - xa) for k in range(N + 1)])
    case["ut"], case["K"], case["uff"] = (np.ascontiguousarray(case[k]) for k in ("ut", "K", "uff"))
    return case


def states(model, rng):
    """(label, x, W, tau) of eight perturbed states: double support, either single support (the swing foot's wrench zero), large velocities,
    and a state at rest."""
    out = []
    for i, label in enumerate(("double", "double", "left only", "right only", "left only", "right only", "fast", "rest")):
        x, u = state_input(model, False, rng, 2.0 if label == "fast" else 1.0)
        W = u[:12].copy()
        W[2] += model.total_mass * 9.81 / 2
        W[8] += model.total_mass * 9.81 / 2
        if label == "left only":
            W[6:] = 0.0
        if label == "right only":
            W[:6] = 0.0
        if label == "rest":
            x[NV:] = 0.0
        out.append((label, x, W, 20.0 * rng.standard_normal(NJ)))
    return out


# ---------------------------------------------------------------------------------------------- 1, 2: accelerations and the residual
def test_accelerations_match_a_dense_solve_on_the_oracles_mass_matrix(emu, model, oracle, rng):
    conds = []
    for i, (label, x, W, tau) in enumerate(states(model, rng)):
        arm = np.zeros(NJ) if i == 1 else np.full(NJ, 0.01)
        got = emu.accel(x, W, tau, arm)
        want, (MA, nle, jw) = PL.accel(oracle, x, tau, W, arm)
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        conds.append(np.linalg.cond(MA))
        print(f"{label}: armature {arm[0]}, cond {conds[-1]:.2e}, |vd| {np.abs(want).max():.2e}, error {err:.2e}")
        assert np.isfinite(got).all() and err <= ACC_TOL, (label, err)
        # 2. the residual of the equation of motion, against its largest term
        terms = [MA @ got, nle, jw, np.r_[np.zeros(6), tau]]
        res = terms[0] + terms[1] - terms[2] - terms[3]
        assert np.abs(res).max() <= 1e-9 * max(np.abs(t).max() for t in terms), (label, np.abs(res).max())
    assert max(conds) > 1e4      # the armature-free case is the ill-conditioned one the bound was sized for


# ---------------------------------------------------------------------------------------------- 3: internal torques
def test_internal_torques_do_not_move_the_centre_of_mass(emu, model, oracle, rng):
    for label, x, W, tau in states(model, rng)[:4]:
        arm = np.full(NJ, 0.01)
        M, _ = oracle.full_dynamics(x)
        tau2 = tau + 30.0 * rng.standard_normal(NJ)
        a1, a2 = emu.accel(x, W, tau, arm), emu.accel(x, W, tau2, arm)
        assert np.abs(a1 - a2).max() > 1.0                     # the torques are felt ...
        lin = (M @ (a1 - a2))[:3]                              # ... but not by the total linear momentum (rows 0..2 of M: m times the com's Jacobian)
        assert np.abs(lin).max() <= ACC_TOL * max(1.0, np.abs(M @ a1).max(), np.abs(M @ a2).max()), (label, lin)


def test_without_gains_the_policy_state_enters_through_the_feedforward_torque_only(emu, model, rng):
    case = plant_case(model, "uniform", rng)
    pl = PL.plant(kp=0.0, kd=0.0, armature=0.01, lookahead=0.005)
    x = start_states(model, False, rng, 1)[0]
    pol = R.Policy(case["ut"], case["dt"], case["dts"], case["K"], case["uff"], 0, False)
    for controller in (R.FEEDFORWARD, R.FEEDBACK):
        for s in (0.0, 0.0137):
            xp, up = PL.policy(pol, case["xt"], pl, controller, s, x)
            k = emu.eval(pl, controller, case, s, x)
            want = emu.accel(x, up[:12], emu.tau(xp, up), pl["armature"])
            assert np.array_equal(k[:NV], x[NV:])
            assert rel(k[NV:], want) <= 1e-10, (controller, s, rel(k[NV:], want))
            # and with gains the joint law is the only difference
            pg = PL.plant(kp=100.0, kd=2.0, armature=0.01, lookahead=0.005)
            tau = (emu.tau(xp, up) + pg["kp"] * (xp[6:NV] - x[6:NV])) + pg["kd"] * (xp[NV + 6:] - x[NV + 6:])
            kg = emu.eval(pg, controller, case, s, x)
            assert rel(kg[NV:], emu.accel(x, up[:12], tau, pg["armature"])) <= 1e-10
            assert rel(kg[NV:], k[NV:]) > 1e-3


# ---------------------------------------------------------------------------------------------- 4: pushes through the tree
# central difference with step h = 1e-6 of a world point of scale ~ 1 m: rounding eps / h ~ 2e-10 and truncation h^2 ~ 1e-12 per Jacobian entry;
# times |f| <= 100 N and (M^-1) entries up to 1 / 3.9e-4 + armature ... the armature 0.01 bounds the joint diagonal of M^-1 by 100: 2e-10 * 100 N
# * 100 = 2e-6 absolute at worst, on accelerations of 1e2 .. 1e3: bound 1e-6 of max(1, |vd|)
FD_TOL = 1e-6


def test_a_push_on_the_elbow_or_the_torso_acts_through_the_tree(emu, model, oracle, rng):
    arm = np.full(NJ, 0.01)
    for label, x, W, tau in states(model, rng)[:3]:
        base = emu.accel(x, W, tau, arm)
        for body in (L_ELBOW, TORSO, BASE):
            pushes = [P.push(body, 0.0, 1.0, 0.1 * rng.standard_normal(3), 50.0 * rng.standard_normal(3))]
            got = emu.accel(x, W, tau, arm, pushes)
            want, _ = PL.accel(oracle, x, tau, W, arm, PL.push_force(oracle, model, x, pushes))
            err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
            print(f"{label} body {body}: |vd| {np.abs(want).max():.2e}, error {err:.2e}")
            assert err <= FD_TOL, (label, body, err)
            moved = np.abs(got - base)[6:]
            if body == L_ELBOW:
                assert moved[L_ELBOW - 1] > 1.0                  # the arm gives way: the compliance the flow-map plant lacks
        # the same push on a foot: the exact wrench form, at the bound of the accelerations
        for foot, body in ((0, L_FOOT), (1, R_FOOT)):
            pushes = [P.push(body, 0.0, 1.0, 0.1 * rng.standard_normal(3), 50.0 * rng.standard_normal(3))]
            got = emu.accel(x, W, tau, arm, pushes)
            want, _ = PL.accel(oracle, x, tau, W, arm, PL.push_force(oracle, model, x, pushes))
            also = emu.accel(x, W + P.delta_u(model, x, False, pushes, foot)[:12], tau, arm)
            err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
            assert err <= ACC_TOL and rel(got, also) <= ACC_TOL, (label, body, err, rel(got, also))
            fd, _ = PL.accel(oracle, x, tau, W, arm, PL.push_force(oracle, model, x, pushes, exact_feet=False))
            assert np.abs(fd - want).max() / max(1.0, np.abs(want).max()) <= FD_TOL      # the two forms of the reference agree with each other


# ---------------------------------------------------------------------------------------------- 5: race check
def test_reverse_order_emulation_is_bit_identical(emu, emu_reverse, model, rng):
    case = plant_case(model, "events", rng)
    pl = PL.plant()
    for label, x, W, tau in states(model, rng)[:3]:
        pushes = [P.push(L_ELBOW, 0.0, 1.0, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0]), P.push(R_FOOT, 0.0, 1.0, [0.0, 0.02, 0.0], [0.0, 0.0, 45.0])]
        assert np.array_equal(emu.accel(x, W, tau, pl["armature"], pushes), emu_reverse.accel(x, W, tau, pl["armature"], pushes))
    x0 = start_states(model, False, rng, 2)
    s0 = np.array([0.0, 0.013])
    pushes = [[P.push(TORSO, 0.003, 0.0065, [0.0, 0.05, 0.2], [70.0, -20.0, 0.0])], []]
    for integrator in (R.ODE45, R.RK4):
        st = R.settings(integrator, R.FEEDBACK, initial_step=0.004 if integrator == R.RK4 else 0.015)
        a = emu.rollout(pl, st, case, s0, x0, D, 2, pushes)
        b = emu_reverse.rollout(pl, st, case, s0, x0, D, 2, pushes)
        assert (a[2] == R.OK).all()
        for va, vb in zip(a, b):
            assert np.array_equal(va, vb), integrator


# ---------------------------------------------------------------------------------------------- 6: RK4 rollout against plant_ref
@pytest.mark.parametrize("controller", [R.FEEDFORWARD, R.FEEDBACK])
def test_rk4_rollout_matches_numpy(emu, model, oracle, controller):
    rng = np.random.default_rng(31 + controller)
    case = plant_case(model, "uniform", rng)
    pl = PL.plant()
    st = R.settings(R.RK4, controller, initial_step=0.004)
    x0 = start_states(model, False, rng, 1)
    s0 = np.array([0.003])
    pushes = [[P.push(L_ELBOW, 0.0045, 0.009, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0])]]
    x, u, status, steps, rej = emu.rollout(pl, st, case, s0, x0, D, 2, pushes)
    pol = R.Policy(case["ut"], case["dt"], case["dts"], case["K"], case["uff"], 0, False)
    cl = PL.closed_loop(oracle, model, pol, case["xt"], pl, controller)
    xr, ur, sr, nr, rr = PL.rollout(cl, pol, st, s0[0], x0[0], D, 2, pushes[0])
    assert status[0] == sr == R.OK and rej[0] == rr == 0
    assert steps[0] == nr, (steps[0], nr)
    ex, eu = rel(x[0], xr), rel(u[0], ur)
    print(f"controller {controller}: steps {nr}, emulation against numpy: x error {ex:.2e}, u error {eu:.2e}")
    # finite-difference push Jacobian in the reference: FD_TOL on the accelerations, over 2^-6 s
    assert ex <= FD_TOL * D * 10 and eu <= 1e-9, (ex, eu)
    # the unpushed rollout, where the reference has no finite difference in it: the bound of the flow-map rollouts' host tests, loosened by cond(M)
    x1, u1, s1, n1, _ = emu.rollout(pl, st, case, s0, x0, D, 2)
    xr1, ur1, sr1, nr1, _ = PL.rollout(cl, pol, st, s0[0], x0[0], D, 2)
    e1 = rel(x1[0], xr1)
    print(f"controller {controller}: unpushed steps {nr1}, emulation against numpy: x error {e1:.2e}")
    assert s1[0] == sr1 == R.OK and n1[0] == nr1 and e1 <= 1e-10, e1
    assert rel(x[0], x1[0]) > 1e-7                               # the push is felt
