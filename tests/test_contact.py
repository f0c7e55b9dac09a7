"""The ground contact of the torque plant (include/hsqp_contact.h, csrc/hsqp_contact.h) on the CPU: the header and the exported entry points, and the
host build of the kernel source (tests/contact/contact_emu.cpp, -ffp-contract=off) against the numpy restatement tests/contact_ref.py on the oracle's
unchanged body_placements / full_dynamics / foot_kinematics."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import contact_ref as CR
import plant_ref as PL
import push_ref as P
import rollout_emu as E
import rollout_ref as R
from test_plant import ACC_TOL, FD_TOL, Emu as PlantEmu, build_emu as build_plant_emu, plant_case, settings_struct
from test_rollout import rel, start_states, state_input
from wb_humanoid_mpc_amd import _abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
LIBDIR = os.path.join(ROOT, "wb_humanoid_mpc_amd")
NX, NU, NV, NJ = _abi.NX, _abi.NU, _abi.NV, _abi.NJ
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_pp = C.POINTER(_abi.Push)
_pl = C.POINTER(_abi.PlantSettings)
_cs = C.POINTER(_abi.ContactSettings)
_cg = C.POINTER(_abi.ContactGround)
L_ELBOW = 19
D = 2.0 ** -6
EPS = np.finfo(float).eps
RK4_STEP = 0.001    # the caller's choice (assumption C2 of the header): the sole's contact rate sqrt(4 k / m_foot) ~ 6e2 1/s leaves 0.004 s at RK4's stability limit


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def contact_struct(ct, enabled=1):
    return _abi.ContactSettings(enabled=enabled, reserved=0, stiffness=ct["stiffness"], damping=ct["damping"], mu=ct["mu"], slip_velocity=ct["slip_velocity"],
                                ground_height=ct["ground_height"])


def ground_array(ground):
    if ground is None:
        return None
    g = (_abi.ContactGround * len(ground))()
    for e, (hgt, mu) in zip(g, ground):
        e.height, e.mu = float(hgt), float(mu)
    return g


# ---------------------------------------------------------------------------------------------- header, exports, defaults, argument errors
def test_header_compiles_and_the_library_exports_the_entry_points(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include "hsqp_contact.h"\n'
                   'int main(void){ hsqp_contact_settings s; hsqp_contact_ground g;\n'
                   ' void (*a)(const hsqp_handle*, hsqp_contact_settings*) = hsqp_contact_defaults;\n'
                   ' int (*b)(hsqp_handle*, const hsqp_contact_settings*) = hsqp_contact_set;\n'
                   ' int (*c)(hsqp_handle*, int, const hsqp_contact_ground*) = hsqp_contact_set_instances;\n'
                   ' int (*d)(hsqp_handle*, int, const hsqp_contact_ground*) = hsqp_contact_set_instances_device;\n'
                   ' int (*e)(hsqp_handle*) = hsqp_contact_clear;\n'
                   ' int (*f)(hsqp_handle*, hsqp_contact_settings*) = hsqp_contact_get;\n'
                   ' int (*i)(hsqp_handle*, int, const double*, double*, double*) = hsqp_contact_eval;\n'
                   ' int (*j)(hsqp_handle*, int, const double*, double*, double*) = hsqp_contact_eval_device;\n'
                   ' s.enabled = 1; s.reserved = 0; s.stiffness = s.damping = s.mu = s.slip_velocity = s.ground_height = 0.0; g.height = g.mu = 0.0;\n'
                   ' printf("%d %d %d\\n", HSQP_ABI_VERSION, a != 0 && b != 0 && c != 0 && d != 0 && e != 0 && f != 0 && i != 0 && j != 0,'
                   ' (int)sizeof s + (int)sizeof g + s.enabled + (int)g.mu + HSQP_CONTACT_FEET * HSQP_CONTACT_CORNERS); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "c.o")])
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.CONTACT_ENTRY_POINTS:
        assert n in names and getattr(lib, n).argtypes is not None, n
    assert C.sizeof(_abi.ContactSettings) == 8 + 5 * 8 and C.sizeof(_abi.ContactGround) == 16
    assert (_abi.CONTACT_FEET, _abi.CONTACT_CORNERS) == (2, 4)
    assert _abi.ABI_VERSION == 7           # additions only: no revision bump


def test_defaults_and_null_arguments():
    lib = solver.load_library()
    st = _abi.ContactSettings()
    st.reserved = 5
    lib.hsqp_contact_defaults(None, C.byref(st))
    assert (st.enabled, st.reserved, st.stiffness, st.damping, st.slip_velocity, st.ground_height) == (1, 0, 5e4, 10.0, 0.01, 0.0)
    assert math.isnan(st.mu)               # without a handle there is no model to take friction_mu from: the caller fills it in
    lib.hsqp_contact_defaults(None, None)  # a NULL struct is ignored
    # a NULL handle is a bad argument, with or without a device
    z, g = np.zeros(NX), ground_array([(0.0, 0.5)])
    assert lib.hsqp_contact_set(None, C.byref(st)) == _abi.ERR_BAD_ARG
    assert lib.hsqp_contact_set(None, None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_contact_set_instances(None, 1, g) == _abi.ERR_BAD_ARG
    assert lib.hsqp_contact_set_instances_device(None, 1, g) == _abi.ERR_BAD_ARG
    assert lib.hsqp_contact_clear(None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_contact_get(None, C.byref(st)) == _abi.ERR_BAD_ARG
    assert lib.hsqp_contact_eval(None, 1, _p(z), None, None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_contact_eval_device(None, 1, _p(z), None, None) == _abi.ERR_BAD_ARG

    # the binding's struct builder: the defaults with the given fields replaced
    class Stub:
        pass
    stub = Stub()
    stub.lib = lib
    s2 = solver.HipSqpSolver.contact_settings(stub, stiffness=2e4, mu=0.3, ground_height=-0.01)
    assert (s2.enabled, s2.reserved, s2.stiffness, s2.damping, s2.mu, s2.slip_velocity, s2.ground_height) == (1, 0, 2e4, 10.0, 0.3, 0.01, -0.01)
    assert solver.HipSqpSolver.contact_settings(stub, enabled=False, mu=0.5).enabled == 0


# ---------------------------------------------------------------------------------------------- host build of the kernel source
def build_emu(path, *defines):
    lib = E.build(path, os.path.join("contact", "contact_emu.cpp"), "-ffp-contract=off", *defines)
    lib.cte_eval.argtypes = [C.c_void_p, _cs, _cg, _dp, _dp, _dp]
    lib.cte_accel.argtypes = [C.c_void_p, _cs, _cg, _dp, _dp, _dp, _dp, C.c_int, _pp, _dp]
    return lib


class Emu:
    def __init__(self, lib, model):
        self.lib, self.h = lib, E.create(lib, model)

    def close(self):
        self.lib.emu_destroy(self.h)

    def eval(self, ct, x, ground=None):
        """(force [8][3], penetration [8]); ground: (height, mu) of the instance's table entry."""
        f, d = np.zeros((8, 3)), np.zeros(8)
        cs = contact_struct(ct)
        self.lib.cte_eval(self.h, C.byref(cs), ground_array(None if ground is None else [ground]), _p(np.ascontiguousarray(x)), _p(f), _p(d))
        return f, d

    def accel(self, ct, x, W, tau, armature, pushes=()):
        _, tab, _ = solver.HipSqpSolver.pack_pushes([list(pushes)])
        vd = np.zeros(NV)
        cs = None if ct is None else contact_struct(ct)
        self.lib.cte_accel(self.h, None if cs is None else C.byref(cs), None, _p(np.ascontiguousarray(x)), _p(np.ascontiguousarray(W)), _p(np.ascontiguousarray(tau)),
                           _p(np.ascontiguousarray(armature)), len(pushes), C.cast(tab, _pp), _p(vd))
        return vd

    def rollout(self, pl, ct, st, case, s0, x0, duration, n, pushes=None, ground=None):
        return E.rollout(self.lib, self.h, case, st, s0, x0, duration, n, plant=settings_struct(pl), contact=None if ct is None else contact_struct(ct),
                         ground=ground_array(ground), pushes=pushes)[:5]


@pytest.fixture(scope="module")
def emu(tmp_path_factory, model):
    e = Emu(build_emu(tmp_path_factory.mktemp("contact") / "libcontact_emu.so"), model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def emu_reverse(tmp_path_factory, model):
    e = Emu(build_emu(tmp_path_factory.mktemp("contact_rev") / "libcontact_emu_rev.so", "-DHSQP_EMU_REVERSE"), model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def plant_emu(tmp_path_factory, model):
    e = PlantEmu(build_plant_emu(tmp_path_factory.mktemp("contact_plant") / "libplant_emu.so"), model)
    yield e
    e.close()


def grounded(oracle, model, x, above=1e-3):
    """The ground height `above` the lowest sole corner of the state x."""
    return float(CR.points(oracle, model, x[:NV])[:, 2].min() + above)


def contact_cases(model, oracle):
    """(label, x, setting) of the case set: start states of tests/test_rollout.py and the model's initial posture, the base pitched and rolled by
    +-0.02 rad so that the 0.18 m x 0.06 m soles have corners on both sides of the plane, the ground 1 mm above the lowest sole corner (two more
    with the ground 4 mm above it: several corners of a sole in contact), and the joint velocities of every second case scaled by 3 so that a
    penetrating corner separates faster than 1 / c and is clamped.  Chosen here on the CPU, with the reference, so that the three classes of
    tests/contact_ref.py are all met (asserted by the force test)."""
    rng = np.random.default_rng(4242)
    out = []
    tilts = [(0.02, 0.02), (-0.02, 0.02), (0.02, -0.02), (-0.02, -0.02)]
    for i in range(10):
        if i < 4:
            x = start_states(model, False, rng, 1)[0]
        else:
            x = model.initial_state.copy()
            x[NV:] = state_input(model, False, rng, 0.5)[0][NV:]
        x[4] += tilts[i % 4][0]
        x[5] += tilts[i % 4][1]
        if i % 2:
            x[NV + 6:] *= 3.0
        above = 4e-3 if i >= 8 else 1e-3
        ct = CR.contact(model, ground_height=grounded(oracle, model, x, above))
        out.append((f"{'start' if i < 4 else 'posture'} {i}", x, ct))
    return out


@pytest.fixture(scope="module")
def cases(model, oracle):
    return contact_cases(model, oracle)


# ---------------------------------------------------------------------------------------------- forces and penetrations
def test_forces_and_penetrations_match_the_reference(emu, model, oracle, cases):
    """Tolerance: P is a sum of O(1) terms in double (a chain of up to 8 placements, each a few roundings), so two evaluations of the penetration
    d = ground_height - P_z differ by at most dd = 64 eps (|P_z| + |ground_height|) — a millimetre-scale difference has no relative accuracy of its
    own.  A force component is k d times factors of order one, so dd moves it by A = k dd: the absolute part, which covers the components near
    zero.  For a component of size |f| the same dd is the relative error dd / d = A / (k d), and k d is the force scale of a point, newtons to
    hundreds of newtons for millimetres at k = 5e4 N/m: allowing A again as the relative tolerance (A |f| with A read as a pure number, the
    convention of atol = rtol) bounds dd / d for every point that carries a newton or more and grows with |f| as the factors (1 + c ddot),
    mu v_t / |.| do.  So: |f - f_ref| <= A + A |f_ref| per component, A = k 64 eps (|P_z| + |ground_height|) of the point.
    The reference's velocities here are the closed form (frame_velocities); the finite-difference form of the same reference carries its own 2e-10
    per Jacobian entry and is held against the closed form at that size, not against the kernel at this one."""
    count = dict(a=0, b=0, c=0)
    for label, x, ct in cases:
        f, d = emu.eval(ct, x)
        ref = CR.forces(oracle, model, x, ct, velocity="frame")
        for c in ref["cls"]:
            count[c] += 1
        scale = np.abs(ref["P"][:, 2]) + abs(ct["ground_height"])
        err_d = np.abs(d - ref["d"])
        assert (err_d <= 64 * EPS * scale).all(), (label, err_d.max())
        A = ct["stiffness"] * 64 * EPS * scale[:, None]
        tol = A + A * np.linalg.norm(ref["f"], axis=1)[:, None]
        err_f = np.abs(f - ref["f"])
        print(f"{label}: classes {''.join(ref['cls'])}, |f| {np.abs(ref['f']).max():.3e}, force error {err_f.max():.2e} (bounds from {tol.min():.2e}), d error {err_d.max():.2e}")
        assert (err_f <= tol).all(), (label, err_f.max(), tol.min())
        for i, c in enumerate(ref["cls"]):
            if c != "a":
                assert not f[i].any()          # no force: exactly zero, every component
        # the finite-difference form of the reference against its closed form: |v|_1 times the rounding share of a Jacobian entry, through k d c
        fd = CR.forces(oracle, model, x, ct)
        assert np.abs(fd["Pdot"] - ref["Pdot"]).max() <= 2e-10 * np.abs(x[NV:]).sum()
    print("points per class:", count)
    assert count["a"] > 0 and count["b"] > 0 and count["c"] > 0, count


def test_the_per_instance_entry_replaces_height_and_mu(emu, model, oracle, cases):
    _, x, ct = cases[8]
    ground = (ct["ground_height"] + 0.002, 0.2)
    f, d = emu.eval(ct, x, ground)
    f2, d2 = emu.eval(CR.with_ground(ct, ground), x)
    assert np.array_equal(f, f2) and np.array_equal(d, d2)
    f0, d0 = emu.eval(ct, x)
    assert np.abs(d - d0 - 0.002).max() <= 64 * EPS and f[:, 2].sum() > f0[:, 2].sum() > 0.0


# ---------------------------------------------------------------------------------------------- accelerations
def test_accelerations_match_the_reference(emu, model, oracle, cases):
    """test_plant.py's rule (error over max(1, |vd|) within ACC_TOL), plus the central difference's own error in the reference's generalised force
    J_P^T f: the 2e-10 rounding share of a Jacobian entry (plant_ref.FD_STEP) times the force scale k d_max of the case."""
    rng = np.random.default_rng(7)
    for label, x, ct in cases:
        tau, arm = 20.0 * rng.standard_normal(NJ), np.full(NJ, 0.01)
        W = state_input(model, False, rng)[1][:12]       # (ignored on the ground: the prescribed wrenches are dropped)
        got = emu.accel(ct, x, W, tau, arm)
        ref = CR.forces(oracle, model, x, ct)
        want, _ = PL.accel(oracle, x, tau, np.zeros(12), arm, CR.generalised_force(ref))
        d_max = max(ref["d"].max(), 0.0)
        tol = ACC_TOL + ct["stiffness"] * d_max * 2e-10
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        print(f"{label}: classes {''.join(ref['cls'])}, |vd| {np.abs(want).max():.2e}, error {err:.2e} (bound {tol:.2e})")
        assert np.isfinite(got).all() and err <= tol, (label, err, tol)
        assert np.array_equal(got, emu.accel(ct, x, np.zeros(12), tau, arm))           # the policy's wrenches do not reach the plant ...
        if "a" in ref["cls"]:
            assert np.abs(got - emu.accel(None, x, np.zeros(12), tau, arm)).max() > 1e-3   # ... and the ground does


def test_pushes_and_the_ground_act_together(emu, model, oracle, cases):
    rng = np.random.default_rng(8)
    _, x, ct = cases[9]
    tau, arm = 20.0 * rng.standard_normal(NJ), np.full(NJ, 0.01)
    pushes = [P.push(L_ELBOW, 0.0, 1.0, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0]), P.push(0, 0.0, 1.0, [0.0, 0.05, 0.1], [60.0, 0.0, 0.0])]
    got = emu.accel(ct, x, np.zeros(12), tau, arm, pushes)
    want = CR.accel(oracle, model, x, tau, arm, ct, PL.push_force(oracle, model, x, pushes))
    err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
    assert err <= FD_TOL, err                  # (the pushes' finite-difference Jacobian: test_plant.py's bound)


# ---------------------------------------------------------------------------------------------- the ground far below
def zero_wrench_case(model, grid, rng):
    """plant_case with a policy whose contact wrenches are zero (feed-forward and feedback): on it the plant without a ground and the plant over
    a ground it never touches integrate the same right-hand side."""
    case = plant_case(model, grid, rng)
    case["ut"][:, :12] = 0.0
    case["K"][:, :12, :] = 0.0
    case["uff"][:, :12] = 0.0
    return case


def test_with_the_ground_far_below_nothing_changes_bit_for_bit(emu, plant_emu, model, cases):
    rng = np.random.default_rng(9)
    arm = np.full(NJ, 0.01)
    for label, x, ct in cases[:4]:
        far = dict(ct, ground_height=ct["ground_height"] - 10.0)
        tau = 20.0 * rng.standard_normal(NJ)
        pushes = [P.push(L_ELBOW, 0.0, 1.0, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0])]
        for ps in ((), pushes):
            assert np.array_equal(emu.accel(far, x, np.zeros(12), tau, arm, ps), plant_emu.accel(x, np.zeros(12), tau, arm, ps)), label
    pl = PL.plant()
    x0 = np.array([cases[0][1], cases[1][1]])
    s0 = np.array([0.0, 0.013])
    far = dict(cases[0][2], ground_height=-10.0)
    for grid in ("uniform", "events"):
        case = zero_wrench_case(model, grid, rng)
        for controller in (R.FEEDFORWARD, R.FEEDBACK):
            st = R.settings(R.RK4, controller, initial_step=0.004)
            a = emu.rollout(pl, far, st, case, s0, x0, D, 2)
            b = plant_emu.rollout(pl, st, case, s0, x0, D, 2)
            assert (a[2] == R.OK).all()
            for va, vb in zip(a, b):
                assert np.array_equal(va, vb), (grid, controller)
            # and with contact off the host build of this file is the plant's
            c = emu.rollout(pl, None, st, case, s0, x0, D, 2)
            assert all(np.array_equal(vc, vb) for vc, vb in zip(c, b))


# ---------------------------------------------------------------------------------------------- RK4 rollout against contact_ref
@pytest.mark.parametrize("grid", ["uniform", "events"])
@pytest.mark.parametrize("controller", [R.FEEDFORWARD, R.FEEDBACK])
def test_rk4_rollout_matches_numpy(emu, model, oracle, cases, controller, grid):
    """Two instances from one state with their own ground (height, mu): each matches its own reference, and they differ from each other.  The
    bound is the one of test_plant.py's pushed rollout — the reference carries a finite-difference Jacobian: FD_TOL on the accelerations over the
    duration, times 10."""
    rng = np.random.default_rng(41 + controller)
    case = plant_case(model, grid, rng)
    pl = PL.plant()
    st = R.settings(R.RK4, controller, initial_step=RK4_STEP)
    _, x, ct = cases[8]
    x0 = np.array([x, x])
    s0 = np.array([0.003, 0.003])
    ground = [(ct["ground_height"], 0.2), (ct["ground_height"] + 0.002, 1.0)]
    xs, us, status, steps, rej = emu.rollout(pl, ct, st, case, s0, x0, D, 2, ground=ground)
    pol = R.Policy(case["ut"], case["dt"], case["dts"], case["K"], case["uff"], 0, False)
    for b in range(2):
        cl = CR.closed_loop(oracle, model, pol, case["xt"], pl, controller, CR.with_ground(ct, ground[b]))
        xr, ur, sr, nr, rr = PL.rollout(cl, pol, st, s0[b], x0[b], D, 2)
        assert status[b] == sr == R.OK and rej[b] == rr == 0 and steps[b] == nr, (status[b], sr, steps[b], nr)
        ex, eu = rel(xs[b], xr), rel(us[b], ur)
        print(f"controller {controller}, {grid}, instance {b}: steps {nr}, emulation against numpy: x error {ex:.2e}, u error {eu:.2e}")
        assert ex <= FD_TOL * D * 10 and eu <= 1e-9, (ex, eu)
    assert rel(xs[0], xs[1]) > 1e-6                                  # the two grounds are felt
    # the ground is felt at all: the same rollout under the policy's prescribed wrenches
    x1 = emu.rollout(pl, None, st, case, s0, x0, D, 2)[0]
    assert rel(xs[0], x1[0]) > 1e-6


# ---------------------------------------------------------------------------------------------- race check
def test_reverse_order_emulation_is_bit_identical(emu, emu_reverse, model, cases):
    rng = np.random.default_rng(10)
    arm = np.full(NJ, 0.01)
    for label, x, ct in cases:
        for va, vb in zip(emu.eval(ct, x), emu_reverse.eval(ct, x)):
            assert np.array_equal(va, vb), label
        tau = 20.0 * rng.standard_normal(NJ)
        pushes = [P.push(L_ELBOW, 0.0, 1.0, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0])]
        assert np.array_equal(emu.accel(ct, x, np.zeros(12), tau, arm, pushes), emu_reverse.accel(ct, x, np.zeros(12), tau, arm, pushes)), label
    case = plant_case(model, "events", rng)
    pl = PL.plant()
    _, x, ct = cases[8]
    x0, s0 = np.array([x, cases[9][1]]), np.array([0.0, 0.013])
    ground = [(ct["ground_height"], 0.2), (cases[9][2]["ground_height"], 1.0)]
    pushes = [[P.push(15, 0.003, 0.0065, [0.0, 0.05, 0.2], [70.0, -20.0, 0.0])], []]
    for integrator in (R.ODE45, R.RK4):
        st = R.settings(integrator, R.FEEDBACK, initial_step=RK4_STEP if integrator == R.RK4 else 0.015)
        a = emu.rollout(pl, ct, st, case, s0, x0, D, 2, pushes, ground)
        b = emu_reverse.rollout(pl, ct, st, case, s0, x0, D, 2, pushes, ground)
        assert (a[2] == R.OK).all(), a[2]
        for va, vb in zip(a, b):
            assert np.array_equal(va, vb), integrator


def test_the_workspace_fits_the_lds(emu):
    n, n0 = emu.lib.emu_ws_bytes(0, 1, 1, 0, 0), emu.lib.emu_ws_bytes(0, 1, 0, 0, 0)
    print("sizeof(RolloutWS<PlantContactStage>) =", n, " sizeof(RolloutWS<PlantStage>) =", n0)
    assert n0 == 33200                      # the plant without a ground keeps its workspace
    assert n0 < n <= n0 + 2048              # the contact set is well under 2 KB on top of it
