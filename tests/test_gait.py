"""The per-instance gait schedule and gait ladder (include/hsqp_gait.h, csrc/hsqp_gait.h) on the CPU: the header, the exported entry points and
the binding's structs; the Python mirror (reference.GaitSchedule, gait_cycle) against tests/golden/ref_gait.npz, recorded from the reference's own
GaitSchedule.cpp compiled in place (tests/golden/make_ref_gait_golden.py); the host build of the kernel source (tests/gait/gait_emu.cpp) against
the mirror, bit for bit.

What the fixture pins: ONE insertModeSequenceTemplate followed by ONE getModeSchedule on a fresh schedule, for the fifteen well-formed templates
of gait.info.  What it does not pin: chains of updates on a trimmed schedule, GaitScheduleUpdater::updateGaitSchedule and
ProceduralMpcMotionManager.cpp themselves — none is reachable through the committed driver (oracle/ref_driver.cpp).  Those rest on the
line-by-line restatement, the predicate known answers written from the table of ProceduralMpcMotionManager.h:110-118 and the invariants below."""
import bisect
import copy
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from wb_humanoid_mpc_amd import _abi, solver
from wb_humanoid_mpc_amd.reference import (GAIT_BAD_TILING, GAIT_LADDER, GAIT_OK, GAIT_OVERFLOW, LF, MODE_BY_NAME, RF, STANCE, GaitInstance, GaitSchedule,
                                           GaitTilingError, gait_cycle, gait_settings, transition_to_faster_gait, transition_to_slower_gait)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
G = np.load(os.path.join(ROOT, "tests", "golden", "ref_gait.npz"))
NX, NJ = _abi.NX, _abi.NJ
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


# ---------------------------------------------------------------------------------------------- header, library, binding
def _header_functions():
    src = open(os.path.join(ROOT, "include", "hsqp_gait.h")).read()
    src = src[src.index("#ifndef HSQP_GAIT_H"):]
    return sorted(set(re.findall(r"\b(hsqp_[a-z_]+)\s*\(", src)))


def test_header_library_and_binding_agree(tmp_path):
    assert _header_functions() == sorted(_abi.GAIT_ENTRY_POINTS)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "wb_humanoid_mpc_amd", "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.GAIT_ENTRY_POINTS:
        assert n in names, n
        assert getattr(lib, n).argtypes is not None, n
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "hsqp_gait.h"\nint main(void){printf("%zu %zu %d %d %d %d %d\\n", sizeof(hsqp_gait_settings), sizeof(hsqp_gait_rung),'
                   ' HSQP_GAIT_MAX_RUNGS, HSQP_GAIT_MAX_PHASES, HSQP_GAIT_MAX_EVENTS, HSQP_GAIT_NAME_LEN, HSQP_ABI_VERSION);return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    out = [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert out == [C.sizeof(_abi.GaitSettings), C.sizeof(_abi.GaitRung), _abi.GAIT_MAX_RUNGS, _abi.GAIT_MAX_PHASES, _abi.GAIT_MAX_EVENTS, _abi.GAIT_NAME_LEN, 7]
    assert _abi.ABI_VERSION == 7


def test_maxima_cover_gait_info(model):
    assert len(model.gaits) <= _abi.GAIT_MAX_RUNGS
    assert max(len(g["modeSequence"]) for g in model.gaits.values()) == _abi.GAIT_MAX_PHASES      # skip


def test_ladder_defaults_are_the_table(model):
    lib = solver.load_library()
    d = _abi.GaitSettings()
    lib.hsqp_gait_ladder_defaults(C.byref(d))
    s = gait_settings(model)
    assert (d.n_rungs, d.max_events, d.min_change_interval, d.phase_transition_stance_time) == (7, 128, 0.2, 0.0)
    assert (s.n_rungs, s.max_events, s.min_change_interval, s.phase_transition_stance_time) == (7, 128, 0.2, model.raw["phase_transition_stance_time"])
    for r, row in enumerate(GAIT_LADDER):
        for c in (d.rungs[r], s.rungs[r]):
            assert c.name.decode() == row[0]
            assert (c.min_lin_vel_cmd, c.max_lin_vel_cmd, c.min_ang_vel_cmd, c.max_ang_vel_cmd, c.lin_vel_error_thresh, c.ang_vel_error_thresh) == row[1:]
        assert d.rungs[r].n_phases == 0                              # the templates are the caller's
        g = model.gaits[row[0]]
        assert list(s.rungs[r].switching_times[:s.rungs[r].n_phases + 1]) == g["switchingTimes"]
        assert list(s.rungs[r].modes[:s.rungs[r].n_phases]) == [MODE_BY_NAME[m] for m in g["modeSequence"]]
    assert [row[0] for row in GAIT_LADDER] == ["stance", "slow_walk", "walk", "slower_trot", "slow_trot", "trot", "run"]


def test_null_handle_is_a_bad_argument(model):
    lib = solver.load_library()
    z = np.zeros(3 * NX)
    p, i = z.ctypes.data_as(_dp), np.ones(4, np.int32).ctypes.data_as(_ip)
    s, ls = gait_settings(model), _abi.LoopSettings()
    assert lib.hsqp_gait_reset(None, C.byref(s), 1, 0.0) == _abi.ERR_BAD_ARG
    assert lib.hsqp_gait_update(None, 1, 0.0, 1.0, p, p, i, p, i) == _abi.ERR_BAD_ARG
    assert lib.hsqp_gait_update_device(None, 1, 0.0, 1.0, p, p, i, p, i) == _abi.ERR_BAD_ARG
    assert lib.hsqp_gait_state(None, None, None, None, None, None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_gait_state_device(None, None, None, None, None, None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_loop_start_gait(None, C.byref(ls), C.byref(s), 1, 0.0, p, p) == _abi.ERR_BAD_ARG
    lib.hsqp_gait_ladder_defaults(None)


def test_binding_raises_no_device_without_a_gpu(model):
    if solver.load_library().hsqp_device_count() > 0:
        pytest.skip("a GPU is visible: the binding is exercised by tests/test_gpu_gait.py")
    with pytest.raises(solver.HsqpError) as ei:
        solver.HipSqpSolver(model, max_nodes=8, max_batch=1).gait_reset(gait_settings(model), 1)
    assert ei.value.code == _abi.ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------- the mirror against the reference-compiled GaitSchedule
def _mirror_case(model, name, start, final, lower, upper, pts):
    tpl = model.gaits[name]
    gs = GaitSchedule([0.5], [STANCE, STANCE], ([0.0, 0.5], [STANCE]), pts)
    try:
        gs.insert_template((tpl["switchingTimes"], [MODE_BY_NAME[k] for k in tpl["modeSequence"]]), start, final)
        return gs.get_mode_schedule(lower, upper)
    except GaitTilingError:
        return None


def test_mirror_equals_the_fixture_exactly(model):
    assert len(G["gaits"]) == 15 and "skip" not in set(G["gaits"]) and set(G["gaits"]) | {"skip"} == set(model.gaits)
    grid = G["grid"]
    # the grid covers what the issue asks for
    assert (grid[:, 0] < 0.5).any() and (grid[:, 0] == 0.5).any() and (grid[:, 0] > 0.5).any() and (grid[:, 1] <= grid[:, 0]).any()
    assert (grid[:, 2] < 0.5).any() and (grid[:, 2] > 0.5).any() and set(grid[:, 4]) == {0.0, 0.1}
    for g, name in enumerate(G["gaits"]):
        for c, (s, f, lo, hi, p) in enumerate(grid):
            got, n = _mirror_case(model, str(name), s, f, lo, hi, p), int(G["n_events"][g, c])
            if n < 0:
                assert got is None, (name, c)
                continue
            assert got is not None and got[0] == list(G["event_times"][g, c, :n]) and got[1] == list(G["mode_sequence"][g, c, :n + 1]), (name, c)


def test_mirror_equals_the_reference_library_where_present(model):
    import ref_swing
    if not ref_swing.available():
        pytest.skip("oracle/_ref is not built and the reference checkout is absent")
    ref = ref_swing.RefSwing()
    rng = np.random.default_rng(7)
    for name in G["gaits"]:
        tpl = model.gaits[str(name)]
        for _ in range(20):
            s, f, lo, hi = rng.uniform(0.0, 2.0), rng.uniform(0.0, 4.0), rng.uniform(-1.0, 2.0), rng.uniform(2.0, 6.0)
            p = float(rng.choice([0.0, 0.1]))
            want = ref.gait_schedule(tpl["switchingTimes"], [MODE_BY_NAME[k] for k in tpl["modeSequence"]], p, s, f, lo, hi)
            got = _mirror_case(model, str(name), s, f, lo, hi, p)
            assert got[0] == list(want[0]) and got[1] == list(want[1]), (name, s, f, lo, hi, p)


# ---------------------------------------------------------------------------------------------- predicates: known answers written from the table
ROWS = [row[1:] for row in GAIT_LADDER]
ZERO6 = [0.0] * 6


def test_predicates_at_each_rung_boundary():
    for r, (mn_l, mx_l, mn_a, mx_a, th_l, th_a) in enumerate(ROWS):
        eps = 1e-9
        # up: the command above maxLinVelCmd AND the base within linVelErrorThresh of it
        fast = [mx_l - th_l + eps, 0.0, 0.0, 0.0, 0.0, 0.0]
        assert transition_to_faster_gait([mx_l + eps, 0.0, 0.8, 0.0], fast, ROWS[r])
        assert not transition_to_faster_gait([mx_l, 0.0, 0.8, 0.0], fast, ROWS[r])                               # strictly above
        if mx_l - th_l - eps >= 0.0:
            assert not transition_to_faster_gait([mx_l + eps, 0.0, 0.8, 0.0], [mx_l - th_l - eps, 0, 0, 0, 0, 0], ROWS[r])   # base too slow
        assert transition_to_faster_gait([0.0, -(mx_l + eps), 0.8, 0.0], [0.0, -(mx_l - th_l + eps), 0, 0, 0, 0], ROWS[r])   # |vy|
        if mx_a < 10.0:
            assert transition_to_faster_gait([0.0, 0.0, 0.8, mx_a + eps], [0, 0, 0, mx_a - th_a + eps, 0, 0], ROWS[r])        # yaw rate: baseVelocity(3)
        # down: the command below minLinVelCmd / minAngVelCmd AND the base below minLinVelCmd + linVelErrorThresh
        if mn_l > 0.0:
            slow_cmd = [mn_l - eps, 0.0, 0.8, 0.0]
            assert transition_to_slower_gait(slow_cmd, [mn_l + th_l - eps, 0, 0, 0, 0, 0], ROWS[r])
            assert not transition_to_slower_gait(slow_cmd, [mn_l + th_l + eps, 0, 0, 0, 0, 0], ROWS[r])
            assert not transition_to_slower_gait([mn_l, 0.0, 0.8, 0.0], ZERO6, ROWS[r])
            assert not transition_to_slower_gait([0.0, 0.0, 0.8, mn_a], ZERO6, ROWS[r])


def test_stance_leaves_on_the_command_alone_and_never_descends():
    assert transition_to_faster_gait([0.2, 0.0, 0.8, 0.0], ZERO6, ROWS[0])          # 0 > 0.1 - 10: the base velocity does not matter
    assert transition_to_faster_gait([0.0, 0.0, 0.8, 0.11], ZERO6, ROWS[0])
    assert not transition_to_faster_gait([0.1, 0.1, 0.8, 0.1], ZERO6, ROWS[0])
    assert not transition_to_slower_gait([0.0, 0.0, 0.8, 0.0], ZERO6, ROWS[0])      # |v| < -0.1 never holds


def test_slower_test_reads_the_commanded_yaw_rate_not_the_base():
    """ProceduralMpcMotionManager.cpp:110 tests velCommandVec(3): a base that still turns fast does not hold the gait up."""
    cmd = [0.0, 0.0, 0.8, 0.0]
    assert transition_to_slower_gait(cmd, [0.0, 0.0, 0.0, 5.0, 0.0, 0.0], ROWS[2])
    assert not transition_to_slower_gait(cmd, [0.31, 0.0, 0.0, 0.0, 0.0, 0.0], ROWS[2])


def _x(model, vx=0.0, wz=0.0):
    x = np.array(model.initial_state, dtype=float)
    x[6 + NJ], x[6 + NJ + 3] = vx, wz
    return x


def test_hold_off_is_0_2_seconds_and_the_rung_is_clamped(model):
    st = GaitInstance(gait_settings(model))
    cmd = [0.4, 0.0, 0.8, 0.0]
    assert gait_cycle(st, 0.0, 1.05, cmd, _x(model))[0] == GAIT_OK and st.rung == 0          # 0 > 0 + 0.2 is false
    assert gait_cycle(st, 0.2, 1.05, cmd, _x(model))[0] == GAIT_OK and st.rung == 0          # strictly later than 0.2
    assert gait_cycle(st, 0.21, 1.05, cmd, _x(model))[0] == GAIT_OK and st.rung == 1 and st.last_change_time == 0.21
    assert gait_cycle(st, 0.4, 1.05, cmd, _x(model, vx=0.3))[0] == GAIT_OK and st.rung == 1   # 0.4 > 0.21 + 0.2 is false
    assert gait_cycle(st, 0.42, 1.05, cmd, _x(model, vx=0.3))[0] == GAIT_OK and st.rung == 2
    # a table of two rungs whose top rung still asks for more: the reference would index past its table, here the rung stays
    two = gait_settings(model, ladder=(GAIT_LADDER[0], ("slow_walk", 0.05, 0.3, 0.05, 0.2, 10.0, 10.0)))
    st = GaitInstance(two)
    for k, t in enumerate((0.3, 0.6, 0.9)):
        assert gait_cycle(st, t, 1.05, [1.0, 0.0, 0.8, 0.0], _x(model))[0] == GAIT_OK
        assert st.rung == 1 and st.last_change_time == t


# ---------------------------------------------------------------------------------------------- the host build of the kernel source against the mirror
@pytest.fixture(scope="module")
def gemu(tmp_path_factory):
    lib_path = tmp_path_factory.mktemp("gait") / "libgait_emu.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fPIC", "-shared",
                           "-I", CSRC, os.path.join(ROOT, "tests", "gait", "gait_emu.cpp"), "-o", str(lib_path)])
    lib = C.CDLL(str(lib_path))
    lib.gt_update.argtypes = [C.POINTER(_abi.GaitSettings), C.c_int, _ip, _dp, _ip, _ip, _dp, C.c_double, C.c_double, _dp, _dp, _ip, _dp, _ip, _ip]
    return lib


class EmuBatch:
    """B instances in the device layout, advanced by the host build."""

    def __init__(self, lib, settings, B, t0=0.0):
        E = settings.max_events
        self.lib, self.settings, self.B, self.E = lib, settings, B, E
        self.n, self.ev, self.seq = np.ones(B, np.int32), np.full((B, E), t0 + 0.5), np.full((B, E + 1), STANCE, np.int32)
        self.scal, self.tc = np.zeros((B, 4), np.int32), np.full(B, float(t0))

    def update(self, t, H, v, x):
        B, E = self.B, self.E
        v, x = np.ascontiguousarray(v, dtype=float), np.ascontiguousarray(x, dtype=float)
        ne, ev, seq, status = np.zeros(B, np.int32), np.zeros((B, E)), np.zeros((B, E + 1), np.int32), np.zeros(B, np.int32)
        ok = self.lib.gt_update(C.byref(self.settings), B, self.n.ctypes.data_as(_ip), self.ev.ctypes.data_as(_dp), self.seq.ctypes.data_as(_ip),
                                self.scal.ctypes.data_as(_ip), self.tc.ctypes.data_as(_dp), t, H, v.ctypes.data_as(_dp), x.ctypes.data_as(_dp),
                                ne.ctypes.data_as(_ip), ev.ctypes.data_as(_dp), seq.ctypes.data_as(_ip), status.ctypes.data_as(_ip))
        return bool(ok), status, ne, ev, seq


def ladder_sequence(model, B, updates, period, seed):
    """Piecewise-constant random commands that sweep the whole ladder up and down, random base velocities near the command: yields (t, v [B][4], x [B][58])."""
    rng = np.random.default_rng(seed)
    x = np.tile(model.initial_state, (B, 1))
    v = np.zeros((B, 4))
    t = 0.0
    for k in range(updates):
        if k % 25 == 0:
            phase = (k // 25 + np.arange(B)) % 16                     # a triangle wave over the ladder's speeds, shifted per instance
            level = np.where(phase < 8, phase, 16 - phase) / 8.0
            v = np.column_stack([1.6 * level * rng.uniform(0.8, 1.2, B), rng.uniform(-0.05, 0.05, B), np.full(B, 0.79),
                                 np.where(rng.uniform(size=B) < 0.2, rng.uniform(-0.8, 0.8, B), 0.0)])
        x[:, 6 + NJ:12 + NJ] = 0.0
        x[:, 6 + NJ] = v[:, 0] * rng.uniform(0.6, 1.1, B)
        x[:, 6 + NJ + 1] = v[:, 1] + 0.02 * rng.standard_normal(B)
        x[:, 6 + NJ + 3] = v[:, 3] * rng.uniform(0.6, 1.1, B)
        yield t, v.copy(), x.copy()
        t += period


def padded_row(ev, seq, E):
    e, s = np.full(E, ev[-1]), np.full(E + 1, STANCE, np.int32)
    e[:len(ev)], s[:len(seq)] = ev, seq
    return e, s


def events_bound(settings, H):
    """A bound on n_events that does not grow with the cycle count: the events of an updated schedule lie between the event in front of t - H (at most
    one phase, D_max, earlier) and the end of the tiling (less than one template period, T_max, past t + 2 H); two of them are at least the shortest
    phase d_min apart, except where a template was inserted, which happens at most once per min_change_interval; plus the two ends."""
    rungs = [settings.rungs[r] for r in range(settings.n_rungs)]
    d = [c.switching_times[i + 1] - c.switching_times[i] for c in rungs for i in range(c.n_phases)]
    t_max = max(c.switching_times[c.n_phases] - c.switching_times[0] for c in rungs)
    span = 3.0 * H + max(max(d), 0.5) + t_max
    return int(math.ceil(span / min(d)) + math.ceil(span / settings.min_change_interval) + 2)


def check_invariants(ev, seq, t, H, bound):
    assert len(seq) == len(ev) + 1
    assert all(b > a for a, b in zip(ev, ev[1:]))
    assert seq[0] == STANCE and seq[-1] == STANCE
    assert ev[-1] >= (t + H) + ((t + H) - t)                  # the tiling passed t + 2 H: the schedule covers it
    assert len(ev) <= bound


def check_insert(mev, mseq, sch, t, H, template, pts):
    """'The events between t - H and the insert point are unchanged by an insert', with the insert point recomputed here from this cycle's
    schedule (mev, mseq) by the rule of GaitScheduleUpdater.cpp:51-66 rather than taken from the code under test: the first event behind
    0.7 (t + H) + 0.3 t, the event before it if the mode in front of it is LF, t + H if there is none.  The resident schedule `sch` must be this
    cycle's from the event in front of t (updateGaitSchedule's own getModeSchedule(t, ...) trims there and makes the front mode STANCE) up to
    the insert point, with its modes; the insert point must be one of its events; behind it (and the optional intermediate stance phase) come
    whole periods of the new template, none at all once the insert point is past 1.5 H (the duration-for-a-time quirk), and the final STANCE."""
    final_time = t + H
    th = final_time - t
    first = bisect.bisect_left(mev, t)
    j = max(first - 1, 0)
    tail, tail_modes = mev[j:], list(mseq[j:])
    if first > 0:
        tail_modes[0] = STANCE
    earliest = 0.7 * final_time + 0.3 * t
    behind = [i for i, e in enumerate(tail) if e > earliest]
    if not behind:
        nxt = final_time
    elif tail_modes[behind[0]] == LF:
        nxt = tail[behind[0] - 1]
    else:
        nxt = tail[behind[0]]
    kept = [e for e in tail if e < nxt]
    k = len(kept)
    assert sch.event_times[:k] == kept and sch.mode_sequence[:k + 1] == tail_modes[:k + 1]
    assert len(sch.event_times) > k and sch.event_times[k] == nxt
    k0 = k
    if pts > 0.0 and tail_modes[k] != STANCE:                                # the intermediate stance phase
        assert sch.mode_sequence[k + 1] == STANCE and sch.event_times[k + 1] == nxt + pts
        k0 = k + 1
    times, modes = template
    tiled_modes, tiled_events = sch.mode_sequence[k0 + 1:-1], sch.event_times[k0 + 1:]
    assert len(tiled_modes) == len(tiled_events) and len(tiled_modes) % len(modes) == 0
    assert tiled_modes == modes * (len(tiled_modes) // len(modes)) and sch.mode_sequence[-1] == STANCE
    assert (len(tiled_events) == 0) == (sch.event_times[k0] >= 1.5 * th)
    back = sch.event_times[k0]
    for i, e in enumerate(tiled_events):
        p = i % len(modes)
        assert e == back + (times[p + 1] - times[p])
        back = e
    if tiled_events:     # "while (eventTimes.back() < finalTime)": every period but the last started in front of 1.5 H, the last one ends behind it
        starts = [sch.event_times[k0]] + tiled_events[len(modes) - 1:-1:len(modes)]
        assert all(e < 1.5 * th for e in starts) and back >= 1.5 * th


@pytest.mark.parametrize("pts", [0.0, 0.1])
@pytest.mark.parametrize("updates,period", [(600, 1.0 / 60.0), (1400, 0.05)])
def test_host_build_equals_the_mirror_bit_for_bit(gemu, model, pts, updates, period):
    """2000 updates in all (600 cycles at 60 Hz and 1400 at 20 Hz) of 8 instances: this cycle's schedule and the resident state after every update."""
    B, H = 8, 30 * model.sqp["dt"]
    settings = gait_settings(model, phase_transition_stance_time=pts)
    E = settings.max_events
    emu = EmuBatch(gemu, settings, B)
    mirror = [GaitInstance(settings) for _ in range(B)]
    bound = events_bound(settings, H)
    assert bound <= E
    rungs_seen = set()
    for t, v, x in ladder_sequence(model, B, updates, period, seed=20261016):
        before = [copy.deepcopy(m.schedule) for m in mirror]
        ok, status, ne, ev, seq = emu.update(t, H, v, x)
        assert ok and not status.any()
        for b, m in enumerate(mirror):
            was_cmd = m.last_command
            st, mev, mseq = gait_cycle(m, t, H, [float(a) for a in v[b]], x[b])
            assert st == GAIT_OK
            e, s = padded_row(mev, mseq, E)
            assert ne[b] == len(mev) and np.array_equal(ev[b], e) and np.array_equal(seq[b], s), (t, b)
            e, s = padded_row(m.schedule.event_times, m.schedule.mode_sequence, E)
            assert emu.n[b] == len(m.schedule.event_times) and np.array_equal(emu.ev[b], e) and np.array_equal(emu.seq[b], s), (t, b)
            assert list(emu.scal[b]) == [m.rung, m.command, m.last_command, m.command] and emu.tc[b] == m.last_change_time
            check_invariants(mev, mseq, t, H, bound)
            sch = m.schedule
            assert len(sch.mode_sequence) == len(sch.event_times) + 1 and sch.mode_sequence[-1] == STANCE and len(sch.event_times) <= bound
            assert all(q > p for p, q in zip(sch.event_times, sch.event_times[1:]))
            if m.last_command != was_cmd:
                check_insert(mev, mseq, sch, t, H, m.template_of(m.command), pts)
                assert before[b].event_times != sch.event_times
            rungs_seen.add(m.rung)
    assert rungs_seen == set(range(7))                          # the whole ladder, up and down


def test_walking_alternates_feet(model):
    st = GaitInstance(gait_settings(model))
    H = 1.05
    for k in range(240):
        t = k / 60.0
        status, ev, seq = gait_cycle(st, t, H, [0.2, 0.0, 0.79, 0.0], _x(model, vx=0.15))
        assert status == GAIT_OK
    assert st.rung == 1
    swings = [m for m in seq if m in (LF, RF)]
    assert len(swings) >= 3 and all(a != b for a, b in zip(swings, swings[1:]))


def test_overflow_leaves_the_state_as_it_was(gemu, model):
    settings = gait_settings(model, max_events=8)
    H = 30 * model.sqp["dt"]
    emu, m = EmuBatch(gemu, settings, 2), [GaitInstance(settings) for _ in range(2)]
    x = np.tile(_x(model), (2, 1))
    v = np.array([[0.0, 0.0, 0.79, 0.0], [0.2, 0.0, 0.79, 0.0]])          # instance 0 stays in stance (7 events at most), instance 1 starts to walk
    failed = None
    for k in range(120):
        t = k / 60.0
        snap = [a.copy() for a in (emu.n, emu.ev, emu.seq, emu.scal, emu.tc)]
        msnap = copy.deepcopy(m)
        ok, status, ne, ev, seq = emu.update(t, H, v, x)
        got = [gait_cycle(m[b], t, H, [float(a) for a in v[b]], x[b])[0] for b in range(2)]
        assert list(status) == got
        if not ok:
            failed = k
            assert status[0] == GAIT_OK and status[1] == GAIT_OVERFLOW
            for a, b in zip(snap, (emu.n, emu.ev, emu.seq, emu.scal, emu.tc)):
                assert np.array_equal(a, b)                                  # BOTH instances: the call is all or nothing
            assert m[1].schedule.event_times == msnap[1].schedule.event_times and m[1].rung == msnap[1].rung
            break
    assert failed is not None


def test_bad_state_is_reported_not_followed(gemu, model):
    settings = gait_settings(model)
    emu = EmuBatch(gemu, settings, 1)
    emu.n[0] = 0
    ok, status, *_ = emu.update(0.0, 1.05, np.zeros((1, 4)), np.tile(_x(model), (1, 1)))
    assert not ok and status[0] == GAIT_BAD_TILING
