"""External pushes on the plant of the rollout (include/hsqp_push.h, csrc/hsqp_push.h, csrc/hsqp_rollout.h) on the CPU: the header and the
exported entry points, and the host build of the kernel source (tests/push/push_emu.cpp, -ffp-contract=off) against identities that need no
new oracle code —
  E1  a push on a foot equals a change of that foot's contact wrench in u;
  E2  the same world point and force on any body give the same flow;
  E3  moving the point along the force changes nothing —
and against the numpy restatement of the break points and the activity rule (tests/push_ref.py) on the oracle's unchanged flow maps."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import push_ref as P
import rollout_emu as E
import rollout_ref as R
from test_rollout import make_case, near_threshold, rel, start_states, state_input
from wb_humanoid_mpc_amd import _abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
LIBDIR = os.path.join(ROOT, "wb_humanoid_mpc_amd")
NX, NU, CNX = _abi.NX, _abi.NU, _abi.CNX
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_pp = C.POINTER(_abi.Push)
BASE, L_FOOT, R_FOOT, TORSO, L_ELBOW = 0, 6, 12, 15, 19   # links of the G1 tree (data/g1_wb.json)


def test_header_compiles_and_the_library_exports_the_entry_points(tmp_path, model):
    assert [model.raw["bodies"][i]["joint"] for i in (L_FOOT, R_FOOT, TORSO, L_ELBOW)] == \
        ["left_ankle_roll_joint", "right_ankle_roll_joint", "waist_pitch_joint", "left_elbow_joint"]
    src = tmp_path / "p.c"
    src.write_text('#include <stdio.h>\n#include "hsqp_push.h"\n'
                   'int main(void){ hsqp_push p;\n'
                   ' int (*a)(hsqp_handle*, int, int, const int32_t*, const hsqp_push*) = hsqp_push_set;\n'
                   ' int (*b)(hsqp_handle*, int, int, const int32_t*, const hsqp_push*) = hsqp_push_set_device;\n'
                   ' int (*c)(hsqp_handle*) = hsqp_push_clear;\n'
                   ' int (*d)(hsqp_handle*, int*, int*, int32_t*, hsqp_push*) = hsqp_push_get;\n'
                   ' p.body = 0; p.reserved = 0; p.t_start = p.duration = p.point[2] = p.force[2] = 0.0;\n'
                   ' printf("%d %d %d %d\\n", HSQP_ABI_VERSION, a != 0 && b != 0 && c != 0 && d != 0, HSQP_PUSH_MAX, (int)sizeof p + p.body); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "p.o")])
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.PUSH_ENTRY_POINTS:
        assert n in names and getattr(lib, n).argtypes is not None, n
    assert C.sizeof(_abi.Push) == 72 and _abi.PUSH_MAX == 8
    assert _abi.ABI_VERSION == 7           # additions only: no revision bump
    # a NULL handle is a bad argument, with or without a device
    n, tab = np.zeros(1, np.int32), (_abi.Push * 1)()
    assert lib.hsqp_push_set(None, 1, 1, n.ctypes.data_as(_ip), tab) == _abi.ERR_BAD_ARG
    assert lib.hsqp_push_set_device(None, 1, 1, n.ctypes.data_as(_ip), tab) == _abi.ERR_BAD_ARG
    assert lib.hsqp_push_clear(None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_push_get(None, None, None, None, None) == _abi.ERR_BAD_ARG


def test_pack_pushes_takes_dicts_and_tuples():
    n, tab, mp = solver.HipSqpSolver.pack_pushes([[], [P.push(3, 0.5, 0.1, (0.1, 0.2, 0.3), (1.0, 2.0, 3.0))],
                                                  [(1, 0.0, 1.0, (0, 0, 0), (0, 0, 5)), dict(body=2, t_start=1.0, duration=0.0, force=(1, 0, 0))]])
    assert list(n) == [0, 1, 2] and mp == 2
    assert (tab[1][0].body, tab[1][0].t_start, tab[1][0].duration, list(tab[1][0].point), list(tab[1][0].force)) == (3, 0.5, 0.1, [0.1, 0.2, 0.3], [1.0, 2.0, 3.0])
    assert (tab[2][0].body, list(tab[2][0].force), tab[2][1].body, list(tab[2][1].point), tab[2][1].reserved) == (1, [0.0, 0.0, 5.0], 2, [0.0, 0.0, 0.0], 0)


# ---------------------------------------------------------------------------------------------- host build of the kernel source
def build_emu(path, *defines):
    lib = E.build(path, os.path.join("push", "push_emu.cpp"), "-ffp-contract=off", *defines)
    lib.pe_flow.argtypes = [C.c_void_p, _dp, _dp, C.c_int, _pp, _dp]
    return lib


class Emu:
    def __init__(self, lib, model, cmodel):
        self.lib, self.h = lib, {"wb": E.create(lib, model), "centroidal": E.create(lib, cmodel)}

    def close(self):
        for h in self.h.values():
            self.lib.emu_destroy(h)

    def flow(self, name, x, u, pushes):
        xp = np.zeros(NX)
        xp[:len(x)] = x
        _, tab, _ = solver.HipSqpSolver.pack_pushes([pushes])
        xd = np.zeros(NX)
        self.lib.pe_flow(self.h[name], _p(xp), _p(np.ascontiguousarray(u)), len(pushes), C.cast(tab, _pp), _p(xd))
        return xd

    def rollout(self, name, st, case, s0, x0, duration, n, pushes=None, stamp0=None):
        """The host build over a batch: (x [B][n][58], u [B][n][35], status, steps, rejected).  pushes: a list per instance, or None: no table."""
        return E.rollout(self.lib, self.h[name], case, st, s0, x0, duration, n, pushes=pushes, stamp0=stamp0)[:5]


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu(tmp_path_factory, model, cmodel):
    e = Emu(build_emu(tmp_path_factory.mktemp("push") / "libpush_emu.so"), model, cmodel)
    yield e
    e.close()


@pytest.fixture(scope="module")
def emu_reverse(tmp_path_factory, model, cmodel):
    e = Emu(build_emu(tmp_path_factory.mktemp("push_rev") / "libpush_emu_rev.so", "-DHSQP_EMU_REVERSE"), model, cmodel)
    yield e
    e.close()


FLOW_TOL = 1e-12   # tests/test_rollout.py::test_flow_maps_match_the_oracle: the emulation's flow against the oracle's


def flows(model, cmodel, oracle, coracle):
    return (("wb", False, R.wb_flow(oracle)), ("centroidal", True, R.cent_flow(coracle)))


def padded(x):
    xp = np.zeros(NX)
    xp[:len(x)] = x
    return xp


def test_e1_a_push_on_a_foot_is_a_change_of_its_contact_wrench(emu, model, cmodel, oracle, coracle, rng):
    for name, cent, flow in flows(model, cmodel, oracle, coracle):
        for foot, body in ((0, L_FOOT), (1, R_FOOT)):
            for swing in (False, True):
                x, u = state_input(model, cent, rng)
                if swing:
                    u[6 * foot:6 * foot + 6] = 0.0            # a swing foot: no wrench of its own (the flow map reads the entries whatever the flag)
                xp = padded(x)
                pushes = [P.push(body, 0.0, 1.0, 0.1 * rng.standard_normal(3), 60.0 * rng.standard_normal(3))]
                got = emu.flow(name, xp, u, pushes)
                want = flow(xp, u + P.delta_u(model, xp, cent, pushes, foot))
                assert rel(got, want) <= FLOW_TOL, (name, foot, swing, rel(got, want))
                assert rel(got, flow(xp, u)) > 1e-3               # and the push is felt
                # only the base rows / the momentum rows change
                rows = slice(0, 6) if cent else slice(_abi.NV, _abi.NV + 6)
                d = got - emu.flow(name, xp, u, [])
                d[rows] = 0.0
                assert not d.any()


def test_e2_the_same_world_point_on_any_body(emu, model, cmodel, oracle, coracle, rng):
    for name, cent, flow in flows(model, cmodel, oracle, coracle):
        x, u = state_input(model, cent, rng)
        xp = padded(x)
        q = P.config(xp, cent)
        f = 80.0 * rng.standard_normal(3)
        Pw = P.world_point(model, q, L_FOOT, [0.05, -0.02, 0.03])
        ref = None
        for body in (L_FOOT, BASE, TORSO, L_ELBOW, R_FOOT):
            pushes = [P.push(body, 0.0, 1.0, P.local_point(model, q, body, Pw), f)]
            got = emu.flow(name, xp, u, pushes)
            ref = got if ref is None else ref
            assert rel(got, ref) <= FLOW_TOL, (name, body, rel(got, ref))
            for foot in (0, 1):   # with E1: the placement of every body is pinned against the independent Python placements
                want = flow(xp, u + P.delta_u(model, xp, cent, pushes, foot))
                assert rel(got, want) <= FLOW_TOL, (name, body, foot, rel(got, want))


def test_e3_the_line_of_action_and_the_sum_of_pushes(emu, model, cmodel, oracle, coracle, rng):
    for name, cent, flow in flows(model, cmodel, oracle, coracle):
        x, u = state_input(model, cent, rng)
        xp = padded(x)
        q = P.config(xp, cent)
        f = 70.0 * rng.standard_normal(3)
        Pw = P.world_point(model, q, TORSO, [0.0, 0.1, 0.2])
        a = emu.flow(name, xp, u, [P.push(TORSO, 0.0, 1.0, P.local_point(model, q, TORSO, Pw), f)])
        b = emu.flow(name, xp, u, [P.push(TORSO, 0.0, 1.0, P.local_point(model, q, TORSO, Pw + 0.004 * f), f)])
        assert rel(a, b) <= FLOW_TOL, (name, rel(a, b))
        # overlapping pushes add
        two = [P.push(TORSO, 0.0, 1.0, [0.0, 0.1, 0.2], f), P.push(L_ELBOW, 0.0, 1.0, [0.1, 0.0, 0.0], -0.5 * f), P.push(BASE, 0.0, 1.0, [0.0, 0.0, 0.0], [0.0, 30.0, 0.0])]
        got = emu.flow(name, xp, u, two)
        want = flow(xp, u + P.delta_u(model, xp, cent, two))
        assert rel(got, want) <= FLOW_TOL, (name, rel(got, want))


# ---------------------------------------------------------------------------------------------- break points and activity
STAMP0 = 0.25            # the first node's stamp: every edge below is an exact binary fraction behind it or survives the subtraction exactly
D = 2.0 ** -6            # a sample interval


def edge_pushes(t0=STAMP0):
    """Wholly inside the first interval; straddling the sample time D; two that overlap; one with duration 0; one that ends exactly at D."""
    return [P.push(TORSO, t0 + 3 * 2.0 ** -10, 6 * 2.0 ** -10, [0.0, 0.0, 0.2], [60.0, 0.0, 0.0]),            # [0.0029.., 0.0087..)
            P.push(L_ELBOW, t0 + 12 * 2.0 ** -10, 7 * 2.0 ** -10, [0.05, 0.0, 0.0], [0.0, 40.0, 10.0]),       # [0.0117.., 0.0185..) over D = 0.0156..
            P.push(BASE, t0 + 20 * 2.0 ** -10, 6 * 2.0 ** -10, [0.0, 0.0, 0.0], [-50.0, 20.0, 0.0]),          # [0.0195.., 0.0253..)
            P.push(R_FOOT, t0 + 23 * 2.0 ** -10, 6 * 2.0 ** -10, [0.0, 0.02, 0.0], [0.0, 0.0, 45.0]),         # [0.0224.., 0.0283..)
            P.push(TORSO, t0 + 28 * 2.0 ** -10, 0.0, [0.0, 0.0, 0.2], [500.0, 0.0, 0.0]),                     # duration 0: inert
            P.push(L_FOOT, t0 + 2.0 ** -7, 2.0 ** -7, [0.0, 0.0, 0.0], [10.0, -30.0, 0.0])]                   # [D / 2, D)


def test_the_reference_breaks_at_every_edge_and_holds_the_activity_per_segment(model, oracle):
    rng = np.random.default_rng(2)
    case = make_case(model, False, "uniform", rng)
    pol = R.Policy(case["ut"], case["dt"], case["dts"], case["K"], case["uff"], 0, False)
    x0 = start_states(model, False, rng, 1)[0]
    seg = []
    st = R.settings(R.RK4, R.FEEDFORWARD, initial_step=1.0)        # one step per segment
    pushes = edge_pushes()
    P.rollout(P.pushed_flow(R.wb_flow(oracle), model, False), pol, st, 0.0, x0, 2 * D, 2, pushes, STAMP0, segments=seg)
    k = 2.0 ** -10
    cuts = [0.0, 3 * k, 8 * k, 9 * k, 12 * k, 16 * k, 19 * k, 20 * k, 23 * k, 26 * k, 29 * k, 32 * k]       # (28 k: the inert push is no break point)
    assert [s[0] for s in seg] == cuts[:-1] and [s[1] for s in seg] == cuts[1:]
    assert [s[2] for s in seg] == [[], [0], [0, 5], [5], [1, 5], [1], [], [2], [2, 3], [3], []]
    assert [s[3] for s in seg] == [1] * 11


@pytest.mark.parametrize("formulation,grid,controller", [("wb", "uniform", R.FEEDFORWARD), ("wb", "events", R.FEEDBACK), ("centroidal", "events", R.FEEDFORWARD),
                                                         ("centroidal", "uniform", R.FEEDBACK)])
def test_rk4_with_pushes_matches_numpy(emu, model, cmodel, oracle, coracle, formulation, grid, controller):
    cent = formulation == "centroidal"
    rng = np.random.default_rng(hash(("push", formulation, grid, controller)) & 0xFFFF)
    case = make_case(model, cent, grid, rng)
    flow = P.pushed_flow(R.cent_flow(coracle) if cent else R.wb_flow(oracle), model, cent)
    st = R.settings(R.RK4, controller, initial_step=0.004)
    s0 = np.array([0.0, 0.0155, 0.013])                     # the last two cross the events at 0.02 and 0.03
    stamp0 = np.array([STAMP0, 0.0, -1.0])
    x0 = start_states(model, cent, rng, 3)
    pushes = [edge_pushes(STAMP0), [], [P.push(TORSO, -1.0 + 0.018, 0.004, [0.0, 0.0, 0.1], [0.0, 70.0, 0.0]), P.push(BASE, -1.0 + 0.02, 0.1, [0.1, 0.0, 0.0], [30.0, 0.0, 0.0])]]
    x, u, status, steps, rej = emu.rollout(formulation, st, case, s0, x0, 2 * D, 2, pushes, stamp0)
    pol = R.Policy(case["ut"], case["dt"], case["dts"], case["K"], case["uff"], 0, cent)
    for b in range(3):
        seg = []
        xr, ur, sr, nr, rr = P.rollout(flow, pol, st, s0[b], x0[b], 2 * D, 2, pushes[b], stamp0[b], segments=seg)
        assert status[b] == sr == R.OK and rej[b] == rr == 0
        assert steps[b] == nr, (b, steps[b], nr)                 # every edge restarts the step sequence
        assert rel(x[b], xr) <= 1e-12, (b, rel(x[b], xr))        # (tests/test_rollout.py::test_rk4_matches_numpy's bounds)
        assert rel(u[b], ur) <= 1e-11, (b, rel(u[b], ur))
        if b == 0 and grid == "uniform":
            assert nr == sum(s[3] for s in seg) and len(seg) == 11 and nr > 11
    # the unpushed instance is the unpushed rollout, bit for bit; the pushed ones are not
    x_un, u_un, _, steps_un, _ = emu.rollout(formulation, st, case, s0, x0, 2 * D, 2)
    assert np.array_equal(x[1], x_un[1]) and np.array_equal(u[1], u_un[1]) and steps[1] == steps_un[1]
    assert rel(x[0], x_un[0]) > 1e-7 and rel(x[2], x_un[2]) > 1e-7 and steps[0] > steps_un[0]


def test_ode45_with_pushes_matches_numpy(emu, model, oracle):
    rng = np.random.default_rng(77)
    case = make_case(model, False, "events", rng)
    flow = P.pushed_flow(R.wb_flow(oracle), model, False)
    pol = R.Policy(case["ut"], case["dt"], case["dts"], case["K"], case["uff"], 0, False)
    for tol in (dict(), dict(abs_tol=1e-10, rel_tol=1e-10)):
        st = R.settings(R.ODE45, R.FEEDBACK, **tol)
        s0 = np.array([0.0, 0.0155])
        x0 = start_states(model, False, rng, 2)
        pushes = [edge_pushes(0.0), [P.push(L_ELBOW, 0.02, 0.005, [0.0, 0.0, 0.0], [0.0, 0.0, -80.0])]]
        x, u, status, steps, rej = emu.rollout("wb", st, case, s0, x0, 2 * D, 2, pushes)
        for b in range(2):
            log = []
            xr, ur, sr, nr, rr = P.rollout(flow, pol, st, s0[b], x0[b], 2 * D, 2, pushes[b], 0.0, log)
            assert status[b] == sr == R.OK
            if (steps[b], rej[b]) != (nr, rr):
                assert near_threshold(log), (b, steps[b], rej[b], nr, rr)   # only a step at a threshold may go either way
                continue
            assert rel(x[b], xr) <= 1e-11, (b, rel(x[b], xr))               # (tests/test_rollout.py::test_ode45_matches_numpy's bounds)
            assert rel(u[b], ur) <= 1e-10, (b, rel(u[b], ur))


@pytest.mark.parametrize("integrator", [R.ODE45, R.RK4])
@pytest.mark.parametrize("formulation", ["wb", "centroidal"])
def test_chained_calls_equal_one_multi_sample_call_with_pushes(emu, model, integrator, formulation):
    cent = formulation == "centroidal"
    rng = np.random.default_rng(11)
    case = make_case(model, cent, "events", rng)
    st = R.settings(integrator, R.FEEDBACK, initial_step=0.004 if integrator == R.RK4 else 0.015)
    s0 = np.array([0.0, 2.0 ** -7])
    stamp0 = np.array([STAMP0, 0.0])
    x0 = start_states(model, cent, rng, 2)
    pushes = [edge_pushes(STAMP0), edge_pushes(0.0)[:4]]
    x, u, status, steps, _ = emu.rollout(formulation, st, case, s0, x0, 4 * D, 4, pushes, stamp0)
    assert (status == R.OK).all()
    xc, total = x0.copy(), np.zeros(2, np.int64)
    for j in range(4):
        xj, uj, sj, nj, _ = emu.rollout(formulation, st, case, s0 + j * D, xc, D, 1, pushes, stamp0)
        assert (sj == R.OK).all()
        assert np.array_equal(xj[:, 0], x[:, j]) and np.array_equal(uj[:, 0], u[:, j]), j
        xc = xj[:, 0]
        total += nj
    assert np.array_equal(total, steps)


def test_inert_tables_equal_no_table_bit_for_bit(emu, model):
    rng = np.random.default_rng(4)
    case = make_case(model, False, "events", rng)
    s0 = np.array([0.0, 0.0155])
    x0 = start_states(model, False, rng, 2)
    for integrator in (R.ODE45, R.RK4):
        st = R.settings(integrator, R.FEEDFORWARD, initial_step=0.004 if integrator == R.RK4 else 0.015)
        want = emu.rollout("wb", st, case, s0, x0, 2 * D, 2)
        outside = [P.push(TORSO, -1.0, 1.0, [0, 0, 0], [90.0, 0, 0]), P.push(TORSO, s0.max() + 2 * D, 1.0, [0, 0, 0], [90.0, 0, 0]),   # ends at the start: [-1, 0)
                   P.push(BASE, 0.01, 0.0, [0, 0, 0], [90.0, 0, 0])]
        for pushes in ([[], []], [outside, outside]):
            got = emu.rollout("wb", st, case, s0, x0, 2 * D, 2, pushes)
            for a, b in zip(got, want):
                assert np.array_equal(a, b)


def test_reverse_order_emulation_is_bit_identical(emu, emu_reverse, model, cmodel, rng):
    for formulation in ("wb", "centroidal"):
        cent = formulation == "centroidal"
        case = make_case(model, cent, "events", rng)
        x0 = start_states(model, cent, rng, 2)
        s0 = np.array([0.0, 0.013])
        pushes = [edge_pushes(STAMP0), edge_pushes(0.0)[1:4]]
        for integrator in (R.ODE45, R.RK4):
            st = R.settings(integrator, R.FEEDBACK, initial_step=0.004 if integrator == R.RK4 else 0.015)
            a = emu.rollout(formulation, st, case, s0, x0, 2 * D, 2, pushes, np.array([STAMP0, 0.0]))
            b = emu_reverse.rollout(formulation, st, case, s0, x0, 2 * D, 2, pushes, np.array([STAMP0, 0.0]))
            for va, vb in zip(a, b):
                assert np.array_equal(va, vb), (formulation, integrator)
        x, u = state_input(model, cent, rng)
        assert np.array_equal(emu.flow(formulation, padded(x), u, edge_pushes()[:4]), emu_reverse.flow(formulation, padded(x), u, edge_pushes()[:4]))
