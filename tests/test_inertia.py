"""Per-instance inertial variations of the torque plant (include/hsqp_inertia.h, csrc/hsqp_inertia.h) on the CPU: the header and the exported entry
points, and the host build of the kernel source (tests/inertia/inertia_emu.cpp, -ffp-contract=off) against the UNCHANGED oracle on a merged model
(tests/inertia_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import contact_ref as CR
import inertia_ref as IR
import plant_ref as PL
import push_ref as P
import rollout_emu as E
import rollout_ref as R
from test_contact import contact_struct, grounded, zero_wrench_case
from test_plant import ACC_TOL, FD_TOL, Emu as PlantEmu, build_emu as build_plant_emu, plant_case, settings_struct, states
from test_rollout import rel, start_states
from wb_humanoid_mpc_amd import _abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
LIBDIR = os.path.join(ROOT, "wb_humanoid_mpc_amd")
NX, NU, NV, NJ, NB = _abi.NX, _abi.NU, _abi.NV, _abi.NJ, _abi.NB
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_pp = C.POINTER(_abi.Push)
_pl = C.POINTER(_abi.PlantSettings)
_ii = C.POINTER(_abi.InertiaInstance)
_cs = C.POINTER(_abi.ContactSettings)
TORSO, L_ELBOW = IR.TORSO, IR.L_ELBOW
D = 2.0 ** -6
GAINS = dict(kp=100.0, kd=2.0, armature=0.01, lookahead=0.005)   # tests/test_gpu_plant.py GAINS
COND_MAX = 2.5e5                       # the reference's own conditioning is asserted first: a badly drawn case cannot hide behind the tolerance
# the nominal error of the emulation's (M, nle) against oracle.full_dynamics, relative to max(1, max|.|), printed by
# test_mass_matrix_and_bias_match_the_merged_oracle: 1.59e-16 on this source (the varied cases: up to 1.6e-16) -> ten times it is below the floor,
# so the bound of the varied cases, here and in tests/test_gpu_inertia.py, is the floor 1e-12
DYN_FLOOR = 1e-12


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def table_of(variations):
    """The ctypes table of a list of (mass_scale [24], payloads)."""
    return solver.HipSqpSolver.pack_inertia(np.array([v[0] for v in variations]), [v[1] for v in variations])


# ---------------------------------------------------------------------------------------------- 1, 2: header, exports, defaults, argument errors
def test_header_compiles_and_the_library_exports_the_entry_points(tmp_path):
    src = tmp_path / "i.c"
    src.write_text('#include <stdio.h>\n#include "hsqp_inertia.h"\n'
                   'int main(void){ hsqp_inertia_instance v; hsqp_inertia_payload p;\n'
                   ' void (*a)(hsqp_inertia_instance*) = hsqp_inertia_defaults;\n'
                   ' int (*b)(hsqp_handle*, int, const hsqp_inertia_instance*) = hsqp_inertia_set_instances;\n'
                   ' int (*c)(hsqp_handle*, int, const hsqp_inertia_instance*) = hsqp_inertia_set_instances_device;\n'
                   ' int (*d)(hsqp_handle*) = hsqp_inertia_clear;\n'
                   ' int (*e)(hsqp_handle*, int, hsqp_inertia_instance*) = hsqp_inertia_get_instances;\n'
                   ' int (*f)(hsqp_handle*, int, const double*, double*, double*, double*) = hsqp_inertia_eval;\n'
                   ' int (*g)(hsqp_handle*, int, const double*, double*, double*, double*) = hsqp_inertia_eval_device;\n'
                   ' v.mass_scale[HSQP_NB - 1] = 1.0; v.n_payloads = HSQP_INERTIA_PAYLOADS; v.reserved = 0; p.body = p.reserved = 0; p.mass = p.com[2] = p.inertia[5] = 0.0;\n'
                   ' v.payload[HSQP_INERTIA_PAYLOADS - 1] = p;\n'
                   ' printf("%d %d %d %d %d\\n", HSQP_ABI_VERSION, a && b && c && d && e && f && g, (int)sizeof v, (int)sizeof p, v.n_payloads); return 0; }\n')
    inc = os.path.join(ROOT, "include")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", inc, str(src), "-o", str(tmp_path / "i.o")])
    # the sizes the C compiler gives the public structs
    size = tmp_path / "s.c"
    size.write_text('#include <stdio.h>\n#include "hsqp_inertia.h"\nint main(void){ printf("%d %d %d\\n", (int)sizeof(hsqp_inertia_instance), (int)sizeof(hsqp_inertia_payload), '
                    'HSQP_INERTIA_PAYLOADS); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(size), "-o", str(tmp_path / "s")])
    c_inst, c_pay, c_n = map(int, subprocess.check_output([str(tmp_path / "s")], text=True).split())
    assert (C.sizeof(_abi.InertiaInstance), C.sizeof(_abi.InertiaPayload), _abi.INERTIA_PAYLOADS) == (c_inst, c_pay, c_n)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.INERTIA_ENTRY_POINTS:
        assert n in names and getattr(lib, n).argtypes is not None, n
    assert _abi.ABI_VERSION == 7           # additions only: no revision bump


def test_defaults_and_null_handles():
    lib = solver.load_library()
    v = _abi.InertiaInstance()
    C.memset(C.byref(v), 0x5A, C.sizeof(v))
    lib.hsqp_inertia_defaults(C.byref(v))
    assert list(v.mass_scale) == [1.0] * NB and (v.n_payloads, v.reserved) == (0, 0)
    assert bytes(v)[NB * 8:] == bytes(C.sizeof(v) - NB * 8)          # everything else is zero
    lib.hsqp_inertia_defaults(None)        # a NULL struct is ignored
    x, out = np.zeros(NX), np.zeros(NV * NV)
    assert lib.hsqp_inertia_set_instances(None, 1, C.byref(v)) == _abi.ERR_BAD_ARG
    assert lib.hsqp_inertia_set_instances(None, 0, None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_inertia_set_instances_device(None, 1, C.byref(v)) == _abi.ERR_BAD_ARG
    assert lib.hsqp_inertia_clear(None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_inertia_get_instances(None, 1, C.byref(v)) == _abi.ERR_BAD_ARG
    assert lib.hsqp_inertia_eval(None, 1, _p(x), _p(out), None, None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_inertia_eval_device(None, 1, _p(x), _p(out), None, None) == _abi.ERR_BAD_ARG
    # the binding's table builder: a scale per instance broadcast over the links, payload fields default to zero
    tab = solver.HipSqpSolver.pack_inertia([1.0, 1.15], [[], [dict(body=TORSO, mass=5.0)]])
    assert list(tab[1].mass_scale) == [1.15] * NB and tab[0].n_payloads == 0 and tab[1].n_payloads == 1
    assert (tab[1].payload[0].body, tab[1].payload[0].mass, list(tab[1].payload[0].com), list(tab[1].payload[0].inertia)) == (TORSO, 5.0, [0.0] * 3, [0.0] * 6)
    with pytest.raises(ValueError):
        solver.HipSqpSolver.pack_inertia([1.0], [[dict(body=0, mass=1.0)] * 3])


# ---------------------------------------------------------------------------------------------- host build of the kernel source
def build_emu(path, *defines):
    lib = E.build(path, os.path.join("inertia", "inertia_emu.cpp"), "-ffp-contract=off", *defines)
    lib.ine_eval.argtypes = [C.c_void_p, _ii, _dp, _dp, _dp, _dp]
    lib.ine_accel.argtypes = [C.c_void_p, _ii, _cs, _dp, _dp, _dp, _dp, C.c_int, _pp, _dp]
    return lib


class Emu:
    """variation: (mass_scale [24], payloads) of one instance, or None: no table."""

    def __init__(self, lib, model):
        self.lib, self.h = lib, E.create(lib, model)

    def close(self):
        self.lib.emu_destroy(self.h)

    def dynamics(self, variation, x):
        M, nle, mass = np.zeros((NV, NV)), np.zeros(NV), np.zeros(1)
        self.lib.ine_eval(self.h, None if variation is None else table_of([variation]), _p(np.ascontiguousarray(x)), _p(M), _p(nle), _p(mass))
        return M, nle, mass[0]

    def accel(self, variation, x, W, tau, armature, pushes=(), ct=None):
        _, tab, _ = solver.HipSqpSolver.pack_pushes([list(pushes)])
        vd = np.zeros(NV)
        cs = None if ct is None else C.byref(contact_struct(ct))
        self.lib.ine_accel(self.h, None if variation is None else table_of([variation]), cs, _p(np.ascontiguousarray(x)), _p(np.ascontiguousarray(W)),
                           _p(np.ascontiguousarray(tau)), _p(np.ascontiguousarray(armature)), len(pushes), C.cast(tab, _pp), _p(vd))
        return vd

    def rollout(self, pl, variations, st, case, s0, x0, duration, n, pushes=None):
        return E.rollout(self.lib, self.h, case, st, s0, x0, duration, n, plant=settings_struct(pl), inertia=None if variations is None else table_of(variations),
                         pushes=pushes)[:5]


@pytest.fixture(scope="module")
def emu(tmp_path_factory, model):
    e = Emu(build_emu(tmp_path_factory.mktemp("inertia") / "libinertia_emu.so"), model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def emu_reverse(tmp_path_factory, model):
    e = Emu(build_emu(tmp_path_factory.mktemp("inertia_rev") / "libinertia_emu_rev.so", "-DHSQP_EMU_REVERSE"), model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def plant_emu(tmp_path_factory, model):
    e = PlantEmu(build_plant_emu(tmp_path_factory.mktemp("inertia_plant") / "libplant_emu.so"), model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def varied(model):
    """[(label, (mass_scale, payloads), merged oracle)] of the three variations: neutral, scales only, scales + the two payloads."""
    rng = np.random.default_rng(2026)
    return [(label, v, IR.merged_oracle(model, *v)) for label, v in zip(("neutral", "scales", "scales + payloads"), IR.variations(rng))]


NEUTRAL = (np.ones(NB), [])


def dyn_err(got, want):
    return np.abs(got - want).max() / max(1.0, np.abs(want).max())


# ---------------------------------------------------------------------------------------------- 3: M, nle, mass
def test_mass_matrix_and_bias_match_the_merged_oracle(emu, model, oracle, varied, rng):
    xs = [x for _, x, _, _ in states(model, rng)[:2]]
    # the tolerance is measured, not chosen: the emulation's error on the NOMINAL model against oracle.full_dynamics ...
    nominal = 0.0
    for x in xs:
        M, nle, mass = emu.dynamics(None, x)
        Mr, nr = oracle.full_dynamics(x)
        nominal = max(nominal, dyn_err(M, Mr), dyn_err(nle, nr))
        assert abs(mass - oracle.total_mass()) <= 1e-13 * mass
    tol = max(10.0 * nominal, DYN_FLOOR)   # ... times ten for the extra sums of the merge, and not below 1e-12
    print(f"nominal model: error {nominal:.2e} of max(1, max|.|) -> bound for the varied cases {tol:.2e}")
    for label, v, vo in varied:
        for x in xs:
            Mr, nr = vo.full_dynamics(x)
            cond = np.linalg.cond(Mr)
            assert cond <= COND_MAX, (label, cond)
            M, nle, mass = emu.dynamics(v, x)
            eM, en = dyn_err(M, Mr), dyn_err(nle, nr)
            want_mass = sum(b[0] for b in IR.merged_bodies(model.raw, *v))
            print(f"{label}: mass {mass:.3f} kg, cond(M) {cond:.2e}, M error {eM:.2e}, nle error {en:.2e}")
            assert eM <= tol and en <= tol, (label, eM, en, tol)
            assert np.array_equal(M, M.T)                                  # both triangles from the same expression
            assert abs(mass - want_mass) <= 1e-13 * want_mass, (label, mass, want_mass)
    # the variations are felt: the scaled and the loaded plant are not the nominal one
    assert dyn_err(emu.dynamics(varied[1][1], xs[0])[0], emu.dynamics(None, xs[0])[0]) > 1e-3
    assert emu.dynamics(varied[2][1], xs[0])[2] - emu.dynamics((varied[2][1][0], []), xs[0])[2] == pytest.approx(6.0, abs=1e-12)


# ---------------------------------------------------------------------------------------------- 4: accelerations
def test_accelerations_match_a_dense_solve_on_the_merged_model(emu, model, oracle, varied, rng):
    cases = states(model, rng)
    for label, v, vo in varied[1:]:
        for i, (what, x, W, tau) in enumerate(cases[:4]):
            arm = np.zeros(NJ) if i == 1 else np.full(NJ, 0.01)
            want, (MA, _, _) = PL.accel(vo, x, tau, W, arm)
            assert np.linalg.cond(vo.full_dynamics(x)[0]) <= COND_MAX
            got = emu.accel(v, x, W, tau, arm)
            err = dyn_err(got, want)
            print(f"{label}, {what}: armature {arm[0]}, cond {np.linalg.cond(MA):.2e}, |vd| {np.abs(want).max():.2e}, error {err:.2e}")
            assert np.isfinite(got).all() and err <= ACC_TOL, (label, what, err)
            assert dyn_err(got, emu.accel(None, x, W, tau, arm)) > 1e-4        # the variation is felt
        # with pushes: one on a foot (the exact wrench form: ACC_TOL) and one through the tree (the reference's central-difference Jacobian: FD_TOL)
        _, x, W, tau = cases[4]
        arm = np.full(NJ, 0.01)
        for pushes, tol in (([P.push(6, 0.0, 1.0, [0.02, 0.0, 0.0], [10.0, -20.0, 45.0])], ACC_TOL),
                            ([P.push(L_ELBOW, 0.0, 1.0, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0]), P.push(TORSO, 0.0, 1.0, [0.0, 0.05, 0.2], [60.0, 0.0, 0.0])], FD_TOL)):
            got = emu.accel(v, x, W, tau, arm, pushes)
            want, _ = PL.accel(vo, x, tau, W, arm, PL.push_force(oracle, model, x, pushes))
            assert dyn_err(got, want) <= tol, (label, dyn_err(got, want), tol)
        # on the ground: the contact forces come through the reference's central-difference Jacobian (test_contact.py: FD_TOL); they do not depend on
        # the inertial model, so the nominal oracle forms them
        x = model.initial_state.copy()
        x[NV:] = cases[5][1][NV:]
        x[4] += 0.02
        ct = CR.contact(model, ground_height=grounded(oracle, model, x, 1e-3))
        ref = CR.forces(oracle, model, x, ct)
        assert "a" in ref["cls"]
        got = emu.accel(v, x, np.zeros(12), tau, arm, (), ct)
        want, _ = PL.accel(vo, x, tau, np.zeros(12), arm, CR.generalised_force(ref))
        err = dyn_err(got, want)
        print(f"{label}, on the ground: classes {''.join(ref['cls'])}, error {err:.2e}")
        assert err <= FD_TOL, (label, err)


# ---------------------------------------------------------------------------------------------- 5, 6: neutrality, bit for bit
def test_neutral_table_no_table_and_the_plant_emulation_are_bit_identical(emu, plant_emu, model, rng):
    pl = PL.plant(**GAINS)
    for _, x, W, tau in states(model, rng)[:3]:
        pushes = [P.push(L_ELBOW, 0.0, 1.0, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0])]
        want = plant_emu.accel(x, W, tau, pl["armature"], pushes)
        for v in (NEUTRAL, None):
            assert emu.accel(v, x, W, tau, pl["armature"], pushes).tobytes() == want.tobytes()
    case = plant_case(model, "events", rng)
    x0 = start_states(model, False, rng, 2)
    s0 = np.array([0.0, 0.013])
    pushes = [[P.push(TORSO, 0.003, 0.0065, [0.0, 0.05, 0.2], [70.0, -20.0, 0.0])], []]
    st = R.settings(R.RK4, R.FEEDBACK, initial_step=0.004)
    want = plant_emu.rollout(pl, st, case, s0, x0, D, 2, pushes)
    assert (want[2] == R.OK).all()
    for variations in ([NEUTRAL, NEUTRAL], None):      # a neutral table; no table / a cleared one: the plant's own instantiation
        got = emu.rollout(pl, variations, st, case, s0, x0, D, 2, pushes)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
    # a non-neutral table is not
    assert emu.rollout(pl, [NEUTRAL, (np.full(NB, 1.1), [])], st, case, s0, x0, D, 2, pushes)[0][1].tobytes() != want[0][1].tobytes()


def test_a_massless_payload(emu, model, rng):
    _, x, W, tau = states(model, rng)[0]
    arm = np.full(NJ, 0.01)
    M0 = emu.dynamics(NEUTRAL, x)[0]
    # mass 0 with an inertia: the rotational inertia is felt
    M1 = emu.dynamics((np.ones(NB), [IR.payload(TORSO, 0.0, (0.0, 0.0, 0.0), (0.02, 0.0, 0.0, 0.03, 0.0, 0.01))]), x)[0]
    assert np.abs(M1 - M0).max() > 1e-3 and np.array_equal(M1[:3, :3], M0[:3, :3])
    # mass 0 and no inertia: bit for bit no payload
    empty = (np.ones(NB), [IR.payload(TORSO, 0.0, (0.05, 0.0, 0.2)), IR.payload(0, 0.0)])
    assert emu.accel(empty, x, W, tau, arm).tobytes() == emu.accel(NEUTRAL, x, W, tau, arm).tobytes()
    for a, b in zip(emu.dynamics(empty, x), emu.dynamics(NEUTRAL, x)):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ---------------------------------------------------------------------------------------------- 7: RK4 rollout against the reference
# printed x errors of the emulation against the numpy reference on this source: (uniform, feedforward) 5.6e-16, (events, feedback) 1.4e-15 — below
# 1e-11, so the GPU bound derived from them (ten times, not below 1e-10: tests/test_gpu_inertia.py) is its floor
ROLLOUT_TOL = 1e-10


def rollout_case(model, grid, controller):
    """(case, pl, st, s0, x0, pushes) of the rollout tests: D = 2^-6, step 0.004, two samples."""
    rng = np.random.default_rng(57 + controller)
    case = plant_case(model, grid, rng)
    return case, PL.plant(**GAINS), R.settings(R.RK4, controller, initial_step=0.004), np.array([0.003]), start_states(model, False, rng, 1)


@pytest.mark.parametrize("grid,controller", [("uniform", R.FEEDFORWARD), ("events", R.FEEDBACK)])
def test_rk4_rollout_matches_numpy(emu, model, oracle, varied, grid, controller):
    case, pl, st, s0, x0 = rollout_case(model, grid, controller)
    pol = R.Policy(case["ut"], case["dt"], case["dts"], case["K"], case["uff"], 0, False)
    label, v, vo = varied[2]
    x, u, status, steps, rej = emu.rollout(pl, [v], st, case, s0, x0, D, 2)
    cl = IR.closed_loop(oracle, vo, model, pol, case["xt"], pl, controller)
    xr, ur, sr, nr, rr = PL.rollout(cl, pol, st, s0[0], x0[0], D, 2)
    assert status[0] == sr == R.OK and rej[0] == rr == 0 and steps[0] == nr, (status[0], steps[0], nr)
    ex, eu = rel(x[0], xr), rel(u[0], ur)
    print(f"{grid}, controller {controller}: steps {nr}, emulation against numpy: x error {ex:.2e}, u error {eu:.2e}")
    assert ex <= ROLLOUT_TOL and eu <= 1e-9, (ex, eu)
    # the mismatch is felt: the nominal plant under the same policy ends elsewhere
    assert rel(emu.rollout(pl, None, st, case, s0, x0, D, 2)[0][0], x[0]) > 1e-7


# ---------------------------------------------------------------------------------------------- 8: race check
def test_reverse_order_emulation_is_bit_identical(emu, emu_reverse, model, varied, rng):
    pl = PL.plant(**GAINS)
    v = varied[2][1]
    both = (v[0], [IR.PAYLOADS[0], IR.payload(TORSO, 1.0, (0.1, 0.0, 0.0))])      # two payloads on ONE link: their order inside the item is fixed
    for _, x, W, tau in states(model, rng)[:3]:
        pushes = [P.push(L_ELBOW, 0.0, 1.0, [0.1, 0.0, 0.0], [0.0, 40.0, 15.0])]
        for var in (v, both):
            assert np.array_equal(emu.accel(var, x, W, tau, pl["armature"], pushes), emu_reverse.accel(var, x, W, tau, pl["armature"], pushes))
            for a, b in zip(emu.dynamics(var, x), emu_reverse.dynamics(var, x)):
                assert np.array_equal(a, b)
    case = plant_case(model, "events", rng)
    x0 = start_states(model, False, rng, 2)
    s0 = np.array([0.0, 0.013])
    for integrator in (R.ODE45, R.RK4):
        st = R.settings(integrator, R.FEEDBACK, initial_step=0.004 if integrator == R.RK4 else 0.015)
        a = emu.rollout(pl, [v, varied[1][1]], st, case, s0, x0, D, 2)
        b = emu_reverse.rollout(pl, [v, varied[1][1]], st, case, s0, x0, D, 2)
        assert (a[2] == R.OK).all()
        for va, vb in zip(a, b):
            assert np.array_equal(va, vb), integrator


# ---------------------------------------------------------------------------------------------- every instantiation of the torque plant
def test_every_torque_configuration_with_inert_parts_is_the_plant_bit_for_bit(emu, model, oracle):
    """The eight configurations of the torque plant (ground x actuator x inertia table) through the one emulated entry, every part that is on inert: a
    neutral table, the ground 10 m below the feet under a policy without contact wrenches, the actuator at its defaults with a continuous command.  Each
    runs its own instantiation (the library's rule picks it) and gives the bits of the plain torque plant."""
    lib = solver.load_library()
    rng = np.random.default_rng(73)
    B, N, n = 2, 4, 2
    full = zero_wrench_case(model, "uniform", rng)
    case = dict(full, ut=full["ut"][:N], xt=full["xt"][:N + 1], K=full["K"][:N + 1], uff=full["uff"][:N + 1])
    x0, s0 = start_states(model, False, rng, B), np.array([0.0, 0.003])
    pl = settings_struct(PL.plant(**GAINS))
    far = contact_struct(CR.contact(model, ground_height=min(grounded(oracle, model, x, above=-10.0) for x in x0)))
    act = _abi.ActuatorSettings()
    lib.hsqp_actuator_defaults(C.byref(act))
    act.command_period = 0.0
    neutral = (_abi.InertiaInstance * B)()
    for e in neutral:
        lib.hsqp_inertia_defaults(C.byref(e))
    sizes = set()
    for controller in (R.FEEDFORWARD, R.FEEDBACK):
        st = R.settings(R.RK4, controller, initial_step=0.004)
        run = lambda g, a, v: E.rollout(emu.lib, emu.h, case, st, s0, x0, 1.0 / 64.0, n, plant=pl, contact=far if g else None,   # noqa: E731
                                        actuator=act if a else None, inertia=neutral if v else None)
        want = run(0, 0, 0)
        assert (want[2] == R.OK).all() and (want[3] == 4).all()
        for g, a, v in [(g, a, v) for v in (0, 1) for a in (0, 1) for g in (0, 1)][1:]:
            got = run(g, a, v)
            sizes.add(emu.lib.emu_ws_bytes(0, 1, g, a, v))
            for name, x, y in zip(("x", "u", "status", "steps"), got, want):
                assert x.tobytes() == y.tobytes(), (controller, g, a, v, name)
    assert len(sizes) == 7          # seven workspaces of their own beside the plain plant's: no two configurations ran the same instantiation


# ---------------------------------------------------------------------------------------------- 9: LDS
def test_every_workspace_fits_the_lds(emu):
    sizes = [emu.lib.emu_ws_bytes(0, 1, k & 1, k >> 1, 1) for k in range(4)] + [emu.lib.ine_eval_ws_bytes()]
    print("rollout workspaces on the varied plant (plain, ground, actuator, both) and hsqp_inertia_eval's:", sizes)
    assert all(0 < s <= 65536 for s in sizes), sizes
    assert sizes[0] < sizes[1] < sizes[3] and sizes[0] < sizes[2] < sizes[3]
