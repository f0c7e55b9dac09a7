"""The per-foot swing heights read from the height map (include/hsqp_perceive.h, csrc/hsqp_perceive.h, csrc/hsqp_params.h) on the CPU: the header, the
exported entry points and the binding's struct; the planner's three-argument update — the host build of the kernel source (tests/perceive/perceive_emu.cpp)
and the mirror in reference.py against the restatement composed from the reference's own compiled SplineCpg (tests/perceive_ref.py, oracle/ref_swing.py),
constant rows against the two-argument form bit for bit; the rule that fills the rows — the host build against the numpy restatement, its heights against
its own terrain sample at its own footholds bit for bit; the sanitizer program; the binding's own checks.
Shapes: B = 3, N = 8, max_events = 6 (tests/perceive_ref.py, case)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import perceive_ref as P
from test_ground import ATOL_DEVICE
from wb_humanoid_mpc_amd import _abi, solver
from wb_humanoid_mpc_amd import reference as ref
from wb_humanoid_mpc_amd.reference import ModeSchedule, TargetTrajectories, swing_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_swing  # noqa: E402

NX, NP = _abi.NX, _abi.NODE_PARAMS
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
# tests/test_ref_swing.py holds the two-argument form to these: the mirror to the reference's compiled planner, and the host build of hsqp_params.h to it
TOL_MIRROR, TOL_HOST = 1e-12, 1e-11
B, N, E = P.B, P.N, P.E


# ---------------------------------------------------------------------------------------------- 1. header, library, binding
def _header_functions():
    src = open(os.path.join(ROOT, "include", "hsqp_perceive.h")).read()
    src = src[src.index("#ifndef HSQP_PERCEIVE_H"):]
    return sorted(set(re.findall(r"\b(hsqp_[a-z_]+)\s*\(", src)))


def test_header_library_and_binding_agree(tmp_path):
    assert _header_functions() == sorted(_abi.PERCEIVE_ENTRY_POINTS)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "wb_humanoid_mpc_amd", "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.PERCEIVE_ENTRY_POINTS:
        assert n in names, n
        assert getattr(lib, n).argtypes is not None, n
    body = ('#include <stddef.h>\n#include <stdio.h>\n#include "hsqp_perceive.h"\nint main(void){printf("%zu %zu %zu %d %d\\n", sizeof(hsqp_perceive_settings),'
            ' offsetof(hsqp_perceive_settings, enabled), offsetof(hsqp_perceive_settings, reserved), HSQP_NX, HSQP_ABI_VERSION);return 0;}\n')
    S = _abi.PerceiveSettings
    want = [C.sizeof(S), S.enabled.offset, S.reserved.offset, 58, 7]
    assert want[:3] == [8, 0, 4]
    for name, cc, std in (("sz.c", "gcc", "-std=c99"), ("sz.cpp", "g++", "-std=c++17")):      # the header as C and as C++
        (tmp_path / name).write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / name), "-o", str(tmp_path / "sz")])
        assert [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()] == want, cc
    assert _abi.ABI_VERSION == 7 and lib.hsqp_abi_version() == 7                                # additions only


def test_defaults_and_null_handle():
    lib = solver.load_library()
    st = _abi.PerceiveSettings(enabled=7, reserved=5)
    lib.hsqp_perceive_defaults(C.byref(st))
    assert (st.enabled, st.reserved) == (1, 0)
    lib.hsqp_perceive_defaults(None)
    d, i = np.zeros(4 * NX).ctypes.data_as(_dp), np.ones(8, np.int32).ctypes.data_as(_ip)
    bad = _abi.ERR_BAD_ARG
    assert lib.hsqp_upload_reference_heights(None, None, None, d, d) == bad
    assert lib.hsqp_foot_heights(None, 1, 0.0, d, 1, i, d, i, 1, d, d, 0.0, d, d, d) == bad
    assert lib.hsqp_foot_heights_device(None, 1, 0.0, d, 1, i, d, i, 1, d, d, 0.0, d, d, d) == bad
    assert lib.hsqp_loop_perceive(None, C.byref(st)) == bad
    assert lib.hsqp_loop_foot_heights(None, d, d, d) == bad
    assert lib.hsqp_loop_foot_heights_device(None, d, d, d) == bad


def test_the_other_headers_point_here():
    for name in ("hsqp_terrain.h", "hsqp_ground.h"):
        assert "include/hsqp_perceive.h" in open(os.path.join(ROOT, "include", name)).read(), name
    text = open(os.path.join(ROOT, "include", "hsqp_perceive.h")).read()
    assert "OURS" in text and "Out of scope" in text                       # the rule is declared as the project's own


# ---------------------------------------------------------------------------------------------- the host build of the kernel sources
class PcTerrain(C.Structure):   # pc_terrain (tests/perceive/perceive_emu.h)
    _fields_ = [("n_maps", C.c_int32), ("reserved", C.c_int32), ("nx", _ip), ("ny", _ip), ("cell", _dp), ("heights", _dp),
                ("place", C.POINTER(_abi.TerrainPlacement)), ("ground_height", _dp)]


def _p(a):
    if a is None:
        return None
    return a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


class Emu:
    def __init__(self, path, model):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fPIC", "-shared",
                               "-I", CSRC, os.path.join(ROOT, "tests", "perceive", "perceive_emu.cpp"), "-o", str(path)])
        lib = self.lib = C.CDLL(str(path))
        lib.pc_create.restype = C.c_void_p
        lib.pc_create.argtypes = [C.c_void_p, _dp, C.c_char_p, C.c_int]
        lib.pc_destroy.argtypes = [C.c_void_p]
        lib.pc_node_params.argtypes = [C.POINTER(_abi.SwingConfig), C.c_double, C.c_int, C.c_int, C.c_int, _dp, _ip, C.c_int, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp]
        lib.pc_foot_heights.argtypes = [C.c_void_p, C.POINTER(PcTerrain), C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _dp, _ip, _dp, _ip, _dp, _dp, _dp, _dp, _dp]
        lib.pc_terrain_eval.argtypes = [C.POINTER(PcTerrain), C.c_int, C.c_int, _dp, _dp]
        err = C.create_string_buffer(256)
        joints = np.ascontiguousarray(model.default_joint_state, dtype=float)
        h = lib.pc_create(C.byref(model.desc), _p(joints), err, 256)
        assert h, err.value
        self.h = C.c_void_p(h)
        self.model = model

    def close(self):
        self.lib.pc_destroy(self.h)

    def _terrain(self, c):
        """(pc_terrain, the arrays it points to)"""
        nx, ny, cell, heights = solver.HipSqpSolver.pack_terrain_maps([(m["H"], m["cell"]) for m in c["maps"]])
        place = solver.HipSqpSolver.pack_terrain_instances(c["place"])
        ground = np.ascontiguousarray(c["ground"], dtype=float)
        keep = (nx, ny, cell, heights, place, ground)
        return PcTerrain(len(nx), 0, _p(nx), _p(ny), _p(cell), _p(heights), place, _p(ground)), keep

    def node_params(self, cfg, n_ev, ev, seq, tt, ts, times, lift=None, touch=None, terrain=0.0):
        """(par [len(times)][NODE_PARAMS], the number of times the planner failed at) of one instance; lift, touch [2][len(seq)] or None"""
        ev, tt, ts, times = (np.ascontiguousarray(a, dtype=float) for a in (ev, tt, ts, times))
        seq = np.ascontiguousarray(seq, dtype=np.int32)
        lift = None if lift is None else np.ascontiguousarray(lift, dtype=float)
        touch = None if touch is None else np.ascontiguousarray(touch, dtype=float)
        par = np.full((len(times), NP), np.nan)
        bad = self.lib.pc_node_params(C.byref(cfg), terrain, 1, len(ev), int(n_ev), _p(ev), _p(seq), len(tt), _p(tt), _p(ts), len(times), _p(times), _p(lift), _p(touch),
                                      _p(par))
        return par, bad

    def foot_heights(self, c, t, x=None):
        x = np.ascontiguousarray(c["x"] if x is None else x)
        rows = len(x)
        ter, keep = self._terrain(c)
        lift, touch, fxy = np.full((rows, 2, E + 1), np.nan), np.full((rows, 2, E + 1), np.nan), np.full((rows, 2, E + 1, 2), np.nan)
        ne, seq = np.ascontiguousarray(c["ne"], dtype=np.int32), np.ascontiguousarray(c["seq"], dtype=np.int32)
        ev, tt, ts = (np.ascontiguousarray(c[k], dtype=float) for k in ("ev", "tt", "ts"))
        self.lib.pc_foot_heights(self.h, C.byref(ter), rows, E, tt.shape[1], t, c["offset"], _p(x), _p(ne), _p(ev), _p(seq), _p(tt), _p(ts), _p(lift), _p(touch), _p(fxy))
        del keep
        return lift, touch, fxy

    def terrain_eval(self, c, xy):
        """[B][n]: the emulator's own terrain sample (hsqp_terrain_eval's lane function) under xy [B][n][2]"""
        xy = np.ascontiguousarray(xy, dtype=float)
        ter, keep = self._terrain(c)
        out = np.full(xy.shape[:2], np.nan)
        self.lib.pc_terrain_eval(C.byref(ter), xy.shape[0], xy.shape[1], _p(xy), _p(out))
        del keep
        return out


@pytest.fixture(scope="module")
def emu(tmp_path_factory, model):
    e = Emu(tmp_path_factory.mktemp("perceive") / "libperceive_emu.so", model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def case(model):
    return P.case(model)


def bits(a):
    return np.ascontiguousarray(a, dtype=float).view(np.uint64)


# ---------------------------------------------------------------------------------------------- 2. the three-argument planner
def planner_rows(model, case):
    """Per instance the rows the planner is checked on: the rule's own at a time with runs ahead (the ledge instance's differ from foot to foot and from
    lift-off to touch-down), and random ones."""
    rng = np.random.default_rng(7)
    lift, touch, _ = P.batch_sequences(model, case, 0.0)
    out = [(lift[b], touch[b]) for b in range(B)]
    out += [(rng.uniform(-0.05, 0.1, (2, E + 1)), rng.uniform(-0.05, 0.1, (2, E + 1))) for _ in range(B)]
    return out


def planner_times(ev, n_ev):
    """a dense grid over the schedule, the events themselves, and points just off them"""
    ev = np.asarray(ev[:n_ev])
    grid = np.linspace(ev[0] - 0.1, ev[-1] + 0.1, 41)
    return np.concatenate([grid, ev, ev - 1e-9, ev + 1e-9])


@pytest.mark.skipif(not ref_swing.available(), reason="oracle/_ref/libref_swing.so (the reference's compiled SplineCpg) is absent")
def test_three_argument_planner_against_the_reference_compiled_splines(emu, model, case):
    rs = ref_swing.RefSwing()
    cfg = swing_config(model)
    rows = planner_rows(model, case)
    worst = {"mirror": 0.0, "host": 0.0}
    for k, (lift, touch) in enumerate(rows):
        b = k % B
        n_ev, ev, seq = int(case["ne"][b]), case["ev"][b], case["seq"][b]
        times = planner_times(ev, n_ev)
        want = P.planner_oracle(rs, model.swing, ev[:n_ev], seq[:n_ev + 1], lift, touch, times)
        planner = ref.SwingTrajectoryPlanner(model.swing, ModeSchedule(ev[:n_ev], seq[:n_ev + 1]), lift=lift, touch=touch)
        mirror = np.array([[planner.z_refs(leg, t) for leg in range(2)] for t in times])
        par, bad = emu.node_params(cfg, n_ev, ev, seq, case["tt"][b], case["ts"][b], times, lift, touch)
        host = par[:, _abi.P_SWING:_abi.P_SWING + 6].reshape(-1, 2, 3)
        assert bad == 0
        worst["mirror"] = max(worst["mirror"], np.abs(mirror - want).max())
        worst["host"] = max(worst["host"], np.abs(host - want).max())
        assert np.abs(want[..., 0]).max() > 0.02 and np.abs(want[..., 2]).max() > 1.0           # swings were met
    print(f"three-argument planner against the reference's compiled SplineCpg: mirror max |d| {worst['mirror']:.3e} (bound {TOL_MIRROR:.0e}), "
          f"host build {worst['host']:.3e} (bound {TOL_HOST:.0e})")
    assert worst["mirror"] <= TOL_MIRROR and worst["host"] <= TOL_HOST


def test_planner_reads_the_rows_where_the_reference_reads_its_sequences(emu, model, case):
    """Known answers, no oracle needed: a stance phase has z = lift[f][p] exactly with zero velocity and acceleration; a plain swing starts at lift[f][p]
    and ends at touch[f][p] (the planner adds no offset), read at phase p and at no other."""
    cfg = swing_config(model)
    rng = np.random.default_rng(11)
    lift, touch = rng.uniform(-0.05, 0.1, (2, E + 1)), rng.uniform(-0.05, 0.1, (2, E + 1))
    b = 1                                                                  # STANCE, RF, FLY, RF, STANCE: the right foot swings in phase 2 alone
    ev, seq = case["ev"][b], case["seq"][b]
    times = np.array([0.0, 0.125, 0.2, 0.25, 0.375, 0.45, 0.6])          # phases 0, 0, 1, 1, 2, 3, 4
    phases = [0, 0, 1, 1, 2, 3, 4]
    par, bad = emu.node_params(cfg, 4, ev, seq, case["tt"][b], case["ts"][b], times, lift, touch)
    assert bad == 0
    z = par[:, _abi.P_SWING:_abi.P_SWING + 6].reshape(-1, 2, 3)
    for k, p in enumerate(phases):
        if p != 2:
            assert z[k, 1, 0] == lift[1, p] and z[k, 1, 1] == 0.0 and z[k, 1, 2] == 0.0, (k, p)
        if p in (0, 4):
            assert z[k, 0, 0] == lift[0, p] and z[k, 0, 1] == 0.0
    assert abs(z[4, 1, 0] - touch[1, 2]) <= ATOL_DEVICE                    # t = 0.375 ends phase 2: the touch-down node of the right foot
    # the left foot is in the air over phases 1 .. 3: in phase 2 (last, current and next phase in the air) it holds touch[0][2] + swingHeight, phase 3 lands
    # on touch[0][3]
    assert abs(z[4, 0, 0] - (touch[0, 2] + model.swing["swingHeight"])) <= ATOL_DEVICE          # phase 2 holds touch[0][2] + swingHeight
    end3, _ = emu.node_params(cfg, 4, ev, seq, case["tt"][b], case["ts"][b], np.array([0.5]), lift, touch)
    assert abs(end3[0, _abi.P_SWING] - touch[0, 3]) <= ATOL_DEVICE         # t = 0.5 ends phase 3 at touch[0][3]


def test_constant_rows_are_the_two_argument_form_bit_for_bit(emu, model, case):
    cfg = swing_config(model)
    offset = model.swing["touchDownHeightOffset"]
    for b in range(B):
        n_ev, ev, seq = int(case["ne"][b]), case["ev"][b], case["seq"][b]
        times = planner_times(ev, n_ev)
        for g in (0.0, 0.03, -0.0175):
            lift, touch = np.full((2, E + 1), g), np.full((2, E + 1), g + offset)
            got, bad = emu.node_params(cfg, n_ev, ev, seq, case["tt"][b], case["ts"][b], times, lift, touch, terrain=123.0)   # (the scalar is not read)
            want, bad2 = emu.node_params(cfg, n_ev, ev, seq, case["tt"][b], case["ts"][b], times, terrain=g)
            assert bad == bad2 == 0 and np.array_equal(bits(got), bits(want)), (b, g)
            sched, targets = ModeSchedule(ev[:n_ev], seq[:n_ev + 1]), TargetTrajectories(case["tt"][b], case["ts"][b])
            a = ref.build_node_params_at(model, sched, targets, times, lift=lift, touch=touch)
            c = ref.build_node_params_at(model, sched, targets, times, terrain_height=g)
            assert np.array_equal(bits(a), bits(c)), (b, g)
            assert np.abs(got - a).max() <= TOL_HOST
    # and the mirror without rows is what it was: terrain_height 0
    assert np.array_equal(bits(ref.build_node_params_at(model, sched, targets, times)), bits(ref.build_node_params_at(model, sched, targets, times, terrain_height=0.0)))


# ---------------------------------------------------------------------------------------------- 3. the rule against the restatement
def structure_holds(case, lift, touch, fxy, sample):
    """The rows of a launch against its OWN footholds and terrain sample, bit for bit: sample [B][2][E + 1] = the terrain under fxy.  Contact phases carry
    the sample at their foothold; swing phases the neighbouring runs' values."""
    offset = case["offset"]
    for b in range(len(lift)):
        n = int(case["ne"][b]) + 1
        for f in range(2):
            c = [ref.mode_to_contact_flags(int(m))[f] for m in case["seq"][b][:n]]
            for p in range(n):
                before = [q for q in range(p) if c[q]]
                after = [q for q in range(p + 1, n) if c[q]]
                if c[p]:
                    assert lift[b, f, p] == sample[b, f, p] and touch[b, f, p] == lift[b, f, p] + offset, (b, f, p)
                    if p > 0 and c[p - 1]:
                        assert np.array_equal(fxy[b, f, p], fxy[b, f, p - 1])                    # one foothold per run
                    continue
                if before:
                    assert lift[b, f, p] == lift[b, f, before[-1]], (b, f, p)
                assert touch[b, f, p] == (lift[b, f, after[0]] if after else lift[b, f, p]) + offset, (b, f, p)
                if after:
                    assert np.array_equal(fxy[b, f, p], fxy[b, f, after[0]]), (b, f, p)
            assert not lift[b, f, n:].any() and not touch[b, f, n:].any() and not fxy[b, f, n:].any()   # phases past n_events: written 0


def test_rule_matches_the_restatement(emu, model, case):
    began, ahead = 0, 0
    worst_xy, worst_h = 0.0, 0.0
    for t in P.TIMES:
        lift, touch, fxy = emu.foot_heights(case, t)
        want = P.batch_sequences(model, case, t)
        worst_xy = max(worst_xy, np.abs(fxy - want[2]).max())
        # the heights: the ledge's one-cell slope is 0.03 / 0.01 = 3, so a foothold off by d moves a height by at most 3 d (+ the sum's own rounding)
        worst_h = max(worst_h, np.abs(lift - want[0]).max(), np.abs(touch - want[1]).max())
        structure_holds(case, lift, touch, fxy, emu.terrain_eval(case, fxy.reshape(B, -1, 2)).reshape(B, 2, E + 1))
        mirror = [ref.foot_height_sequences(model, case["x"][b], t, ModeSchedule(case["ev"][b][:4], case["seq"][b][:5]), case["knots"][b],
                                            P.ground_of(case["maps"], case["place"][b], case["ground"][b])) for b in range(B)]
        for b in range(B):                                                 # reference.py's mirror is the restatement, phase for phase
            for k in range(3):
                assert np.abs(mirror[b][k] - want[k][b][:, :5]).max() <= 1e-15, (t, b, k)
        for b in range(B):
            p_now = int(np.searchsorted(case["ev"][b][:4], t, side="left"))
            for f in range(2):
                c = [ref.mode_to_contact_flags(int(m))[f] for m in case["seq"][b][:5]]
                for a, _ in P.runs(c):
                    began, ahead = began + (a <= p_now), ahead + (a > p_now)
                    if a <= p_now:
                        assert np.abs(fxy[b, f, a] - P.contact_xy(model, case["x"][b], f)).max() <= ATOL_DEVICE
    print(f"rule, host build against numpy over {len(P.TIMES)} times: footholds max |d| {worst_xy:.3e}, heights {worst_h:.3e}; runs begun {began}, ahead {ahead}")
    assert worst_xy <= ATOL_DEVICE and worst_h <= 4 * ATOL_DEVICE
    assert began > 20 and ahead > 20


def test_the_ledge_lies_between_the_foot_and_its_foothold(emu, model, case):
    """Instance 0 at t = 0.3: its left foot is in the air (phase 2), lifted off the low side and lands on the ledge — the two heights a scalar terrain
    height cannot tell apart; its right foot, in contact, stands on the low side and will land on the ledge as well."""
    lift, touch, fxy = emu.foot_heights(case, 0.3)
    step_lo, step_hi = case["place"][0]["origin"][0] + 0.02, case["place"][0]["origin"][0] + 0.03
    P_left = P.contact_xy(model, case["x"][0], 0)
    assert P_left[0] < step_lo and fxy[0, 0, 3, 0] > step_hi
    assert lift[0, 0, 0] == 0.0 and np.array_equal(lift[0, 0, 1:3], [0.0, 0.0])                  # lift-off from the low side
    assert np.array_equal(touch[0, 0, 1:3], np.full(2, P.LEDGE_HEIGHT + case["offset"]))         # touch-down on the ledge, offset included
    assert np.array_equal(lift[0, 0, 3:5], np.full(2, P.LEDGE_HEIGHT))
    assert np.array_equal(fxy[0, 0, 1], fxy[0, 0, 3]) and np.array_equal(fxy[0, 0, 0], fxy[0, 0, 0])
    # the plane (instance 1): the contact ground height everywhere; the ramp (instance 2): its feet stand at different heights
    assert np.array_equal(lift[1, :, :5], np.full((2, 5), 0.02)) and np.array_equal(touch[1, :, :5], np.full((2, 5), 0.02 + case["offset"]))
    assert abs(lift[2, 0, 0] - lift[2, 1, 0]) > 1e-3


def test_a_non_finite_state_gives_nan_rows_and_the_others_their_bits(emu, model, case):
    x = case["x"].copy()
    x[1, 40] = np.inf                                                      # (a velocity entry: the kinematics would not have seen it)
    for t in (0.0, 0.3):
        want = emu.foot_heights(case, t)
        got = emu.foot_heights(case, t, x)
        for a, b in zip(got, want):
            assert np.isnan(a[1, :, :5]).all() and not a[1, :, 5:].any()
            assert np.array_equal(bits(a[[0, 2]]), bits(b[[0, 2]]))
        ref_rows = P.batch_sequences(model, case, t, x)
        assert np.isnan(ref_rows[0][1, :, :5]).all()


# ---------------------------------------------------------------------------------------------- 4. sanitizers: a program of its own
def test_the_rule_under_sanitizers(tmp_path, model):
    exe, desc = tmp_path / "perceive_sanitize", tmp_path / "desc.bin"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "perceive", "perceive_emu.cpp"),
                           os.path.join(ROOT, "tests", "perceive", "perceive_sanitize.cpp"), "-o", str(exe)])
    desc.write_bytes(bytes(model.desc))
    out = subprocess.check_output([str(exe), str(desc)], text=True)
    assert out.strip() == "perceive ok"


# ---------------------------------------------------------------------------------------------- 5. the binding's own checks
def test_binding_settings_and_shapes():
    lib = solver.load_library()

    class Stub(solver.HipSqpSolver):
        def __init__(self):
            self.lib = lib
    s = Stub()
    st = s.perceive_settings()
    assert (st.enabled, st.reserved) == (1, 0) and s.perceive_settings(enabled=False).enabled == 0
    with pytest.raises(ValueError):
        s.foot_heights(np.zeros((2, NX)), 0.0, np.ones(2, np.int32), np.zeros((2, 3)), np.zeros((2, 3), np.int32), np.zeros((2, 3)), np.zeros((2, 3, NX)), 0.0)
    with pytest.raises(ValueError):
        s.foot_heights(np.zeros((2, NX)), 0.0, np.ones(2, np.int32), np.zeros((2, 3)), np.zeros((2, 4), np.int32), np.zeros((2, 3)), np.zeros((2, 2, NX)), 0.0)
