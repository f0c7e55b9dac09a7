"""The per-instance ground-height estimate from the stance feet (include/hsqp_ground.h, csrc/hsqp_ground.h) on the CPU: the header, the exported
entry points and the binding's struct; the host build of the kernel's sources (tests/ground/ground_emu.cpp) against the numpy restatement
(tests/ground_ref.py) — the contact-frame heights within the accuracy of a chain of seven rotations, the rule, the latch and the shift of the knots
exactly — the known answer of the zero configuration, the order independence of the launch, the loop's phase of the launch (g_init on a new episode,
a parked instance's knots left alone), the base-height box above the ground, and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ground_ref as G
from wb_humanoid_mpc_amd import _abi, solver
from wb_humanoid_mpc_amd.reference import FLY, LF, RF, STANCE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
NX, NJ, KNOTS = _abi.NX, _abi.NJ, _abi.CMD_KNOTS
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
_gs, _es = C.POINTER(_abi.GroundSettings), C.POINTER(_abi.EpisodeSettings)
ATOL_DEVICE = 1e-13   # the project's bound for device-generated parameters; the magnitudes here are below 1.5 and the chain has seven rotations

# one schedule that holds every mode: STANCE until 1, LF until 2, RF until 3, FLY until 4, STANCE after; padded as pack_reference pads
EVENTS = np.array([1.0, 2.0, 3.0, 4.0, 4.0, 4.0])
SEQ = np.array([STANCE, LF, RF, FLY, STANCE, STANCE, STANCE], np.int32)
N_EVENTS = 4
TIMES = {"stance": 0.5, "left": 1.5, "right": 2.5, "flight": 3.5, "on_event": 2.0, "after": 9.0}
MODE_AT = {"stance": STANCE, "left": LF, "right": RF, "flight": FLY, "on_event": LF, "after": STANCE}   # lower_bound: an event time belongs to the phase it ends


# ---------------------------------------------------------------------------------------------- 1. header, library, binding
def _header_functions():
    src = open(os.path.join(ROOT, "include", "hsqp_ground.h")).read()
    src = src[src.index("#ifndef HSQP_GROUND_H"):]
    return sorted(set(re.findall(r"\b(hsqp_[a-z_]+)\s*\(", src)))


def test_header_library_and_binding_agree(tmp_path):
    assert _header_functions() == sorted(_abi.GROUND_ENTRY_POINTS)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "wb_humanoid_mpc_amd", "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.GROUND_ENTRY_POINTS:
        assert n in names, n
        assert getattr(lib, n).argtypes is not None, n
    body = ('#include <stddef.h>\n#include <stdio.h>\n#include "hsqp_ground.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(hsqp_ground_settings),'
            ' offsetof(hsqp_ground_settings, enabled), offsetof(hsqp_ground_settings, box_above_ground), offsetof(hsqp_ground_settings, filter_alpha),'
            ' offsetof(hsqp_ground_settings, initial_height), HSQP_NX, HSQP_ABI_VERSION);return 0;}\n')
    S = _abi.GroundSettings
    want = [C.sizeof(S), S.enabled.offset, S.box_above_ground.offset, S.filter_alpha.offset, S.initial_height.offset, 58, 7]
    assert want[:5] == [24, 0, 4, 8, 16]
    for name, cc, std in (("sz.c", "gcc", "-std=c99"), ("sz.cpp", "g++", "-std=c++17")):      # the header as C and as C++
        (tmp_path / name).write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / name), "-o", str(tmp_path / "sz")])
        assert [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()] == want, cc
    assert _abi.ABI_VERSION == 7 and lib.hsqp_abi_version() == 7


def test_defaults_and_null_handle():
    lib = solver.load_library()
    st = _abi.GroundSettings(enabled=7, box_above_ground=5, filter_alpha=0.3, initial_height=2.0)
    lib.hsqp_ground_defaults(C.byref(st))
    assert (st.enabled, st.box_above_ground, st.filter_alpha, st.initial_height) == (1, 0, 0.0, 0.0)
    lib.hsqp_ground_defaults(None)
    d, i = np.zeros(2 * NX).ctypes.data_as(_dp), np.ones(8, np.int32).ctypes.data_as(_ip)
    bad = _abi.ERR_BAD_ARG
    assert lib.hsqp_ground_estimate(None, 1, 0.0, d, 1, i, d, i, 0.0, d, d) == bad
    assert lib.hsqp_ground_estimate_device(None, 1, 0.0, d, 1, i, d, i, 0.0, d, d) == bad
    assert lib.hsqp_upload_reference_ground(None, None, None, d) == bad
    assert lib.hsqp_loop_ground(None, C.byref(st), d) == bad
    assert lib.hsqp_loop_ground_state(None, d, d) == bad
    assert lib.hsqp_loop_ground_state_device(None, d, d) == bad


def test_the_other_headers_point_here():
    for name in ("hsqp_terrain.h", "hsqp_episode.h", "hsqp_loop.h"):
        assert "include/hsqp_ground.h" in open(os.path.join(ROOT, "include", name)).read(), name


# ---------------------------------------------------------------------------------------------- the host build of the kernel sources
def _build(path, *defines):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-march=x86-64-v3", "-ffp-contract=off", *defines, "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fPIC", "-shared",
                           "-I", CSRC, os.path.join(ROOT, "tests", "ground", "ground_emu.cpp"), "-o", str(path)])
    lib = C.CDLL(str(path))
    lib.gr_create.restype = C.c_void_p
    lib.gr_create.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.gr_destroy.argtypes = [C.c_void_p]
    lib.gr_foot_heights.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    lib.gr_estimate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, _dp, _ip, _dp, _ip, _dp, _dp, _dp, _dp, _ip, _ip, _dp, _dp]
    lib.gr_rule.argtypes = [_dp, C.c_int, _dp, _ip, C.c_double, C.c_double, C.c_double]
    lib.gr_rule.restype = C.c_double
    lib.gr_verdict.argtypes = [_es, _dp, _dp]
    return lib


def _p(a):
    if a is None:
        return None
    return a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


class Emu:
    def __init__(self, lib, model):
        self.lib = lib
        err = C.create_string_buffer(256)
        h = lib.gr_create(C.byref(model.desc), err, 256)
        assert h, err.value
        self.h = C.c_void_p(h)

    def close(self):
        self.lib.gr_destroy(self.h)

    def foot_heights(self, x):
        x = np.ascontiguousarray(np.atleast_2d(x))
        out = np.zeros((len(x), 2))
        self.lib.gr_foot_heights(self.h, len(x), _p(x), _p(out))
        return out

    def estimate(self, x, t, g, alpha=0.0, g_init=None, mode_b=None, parked=None, ts=None, want_terrain=False, schedule=None):
        """One launch over the batch x [B][58] on the module's schedule (or schedule = (n_events, event_times, mode_sequence)): (g_out, foot_z, terrain_b);
        ts is shifted in place."""
        x = np.ascontiguousarray(np.atleast_2d(x))
        B = len(x)
        if schedule is None:
            schedule = (np.full(B, N_EVENTS, np.int32), np.tile(EVENTS, (B, 1)), np.tile(SEQ, (B, 1)))
        ne, ev, seq = (np.ascontiguousarray(a) for a in schedule)
        g_in, g_out, fz = np.ascontiguousarray(g, dtype=float), np.full(B, np.nan), np.full((B, 2), np.nan)
        terrain = np.full(B, np.nan) if want_terrain else None
        self.lib.gr_estimate(self.h, B, ev.shape[1], t, alpha, _p(x), _p(ne), _p(ev), _p(seq), _p(g_in), _p(g_out), _p(fz), _p(g_init), _p(mode_b), _p(parked), _p(ts),
                             _p(terrain))
        return g_out, fz, terrain


@pytest.fixture(scope="module")
def emu(tmp_path_factory, model):
    e = Emu(_build(tmp_path_factory.mktemp("ground") / "libground_emu.so"), model)
    yield e
    e.close()


@pytest.fixture(scope="module")
def emu_reverse(tmp_path_factory, model):
    e = Emu(_build(tmp_path_factory.mktemp("ground_rev") / "libground_emu_rev.so", "-DHSQP_EMU_REVERSE"), model)
    yield e
    e.close()


def random_states(model, n=64, seed=20251019):
    """initial_state + 0.05 sigma, yaw in +-1.2, base z in [0.6, 1.0]"""
    rng = np.random.default_rng(seed)
    x = model.initial_state[None] + 0.05 * rng.standard_normal((n, NX))
    x[:, 3] = rng.uniform(-1.2, 1.2, n)
    x[:, 2] = rng.uniform(0.6, 1.0, n)
    return x


# ---------------------------------------------------------------------------------------------- 2. heights and estimate against the mirror
def test_heights_and_estimate_match_the_mirror(emu, model):
    x = random_states(model)
    want_fz = np.array([G.foot_heights(model, xb) for xb in x])
    assert np.abs(want_fz).max() < 1.5 and np.ptp(want_fz) > 0.3
    got_fz = emu.foot_heights(x)
    print(f"contact-frame heights, host build against numpy over 64 states: max |dz| {np.abs(got_fz - want_fz).max():.3e}")
    assert np.abs(got_fz - want_fz).max() <= ATOL_DEVICE
    g0 = np.linspace(-0.2, 0.3, len(x))
    for name, t in TIMES.items():
        for alpha in (0.0, 0.8):
            g, fz, _ = emu.estimate(x, t, g0, alpha)
            want, _ = G.estimate(model, x, t, np.full(len(x), N_EVENTS), np.tile(EVENTS, (len(x), 1)), np.tile(SEQ, (len(x), 1)), g0, alpha)
            assert G.mode_at(N_EVENTS, EVENTS, SEQ, t) == MODE_AT[name], name
            assert np.array_equal(fz, got_fz), name                      # the read-back is the walk's own result
            assert np.abs(g - want).max() <= ATOL_DEVICE, (name, alpha)
    # the yaw and the planar position do not enter a height; the base height enters as itself
    moved = x.copy()
    moved[:, 0] += 3.0; moved[:, 1] -= 2.0; moved[:, 3] += 0.7
    assert np.array_equal(emu.foot_heights(moved), got_fz)
    lifted = x.copy()
    lifted[:, 2] += 0.125
    assert np.abs(emu.foot_heights(lifted) - got_fz - 0.125).max() <= 4 * np.finfo(float).eps


def test_rule_latch_and_flight_are_exact(emu, model):
    """Given the heights, the rule has no transcendental in it: the host build equals the numpy restatement bit for bit, over a latch carried through
    six cycles (stance, left, right, flight, flight, stance) with filter_alpha 0 and 0.8."""
    x = random_states(model, 16, seed=7)
    fz = emu.foot_heights(x)
    B = len(x)
    sched = (np.full(B, N_EVENTS), np.tile(EVENTS, (B, 1)), np.tile(SEQ, (B, 1)))
    for alpha in (0.0, 0.8):
        g = np.linspace(-0.1, 0.4, B)
        g_ref = g.copy()
        for t in (0.5, 1.5, 2.5, 3.5, 3.9, 9.0):
            before = g.copy()
            g, _, _ = emu.estimate(x, t, g, alpha)
            g_ref, _ = G.estimate(model, x, t, *sched, g_ref, alpha, foot_z=fz)
            assert np.array_equal(g, g_ref), (alpha, t)
            if G.mode_at(N_EVENTS, EVENTS, SEQ, t) == FLY:
                assert np.array_equal(g, before)                         # flight: the latch, unchanged
            elif alpha == 0.0:
                assert not np.array_equal(g, before)
        for b in range(B):                                               # the rule alone, one call per instance
            got = emu.lib.gr_rule(_p(fz[b].copy()), N_EVENTS, _p(EVENTS), _p(SEQ), 0.5, alpha, 0.25)
            assert got == G.rule(fz[b], STANCE, 0.25, alpha)
    assert G.rule([0.25, 0.75], STANCE, 9.0) == 0.5 and G.rule([0.25, 0.75], LF, 9.0) == 0.25 and G.rule([0.25, 0.75], RF, 9.0) == 0.75
    assert G.rule([0.25, 0.75], FLY, 9.0) == 9.0 and G.rule([0.25, 0.75], STANCE, 1.0, 0.5) == 0.75


def test_zero_configuration_known_answer(emu, model):
    """The contact-frame height tests/test_model.py pins: 0.0496 m under a pelvis at 0.8415 m with every joint at zero."""
    x = np.zeros(NX)
    x[2] = 0.8415
    fz = emu.foot_heights(x)[0]
    assert fz[0] == fz[1] and abs(fz[0] - 0.0496) < 1e-4
    assert abs((0.8415 - fz[0]) - 0.7919) < 1e-3
    assert np.abs(fz - G.foot_heights(model, x)).max() <= ATOL_DEVICE


def test_instances_in_reverse_order_give_the_same_bits(emu, emu_reverse, model):
    x = random_states(model, 33, seed=11)
    B = len(x)
    g0, g_init = np.linspace(-0.2, 0.3, B), np.linspace(1.0, 2.0, B)
    mode_b = np.where(np.arange(B) % 5 == 0, _abi.WARM_COLD, _abi.WARM_SHIFT).astype(np.int32)
    parked = (np.arange(B) % 7 == 3).astype(np.int32)
    for t in TIMES.values():
        outs = []
        for e in (emu, emu_reverse):
            ts = np.arange(B * KNOTS * NX, dtype=float).reshape(B, KNOTS, NX) / 1000.0
            g, fz, terrain = e.estimate(x, t, g0, 0.8, g_init=g_init, mode_b=mode_b, parked=parked, ts=ts, want_terrain=True)
            outs.append((g, fz, terrain, ts))
        for a, b in zip(*outs):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------------------------------------- 3. the loop's phase of the launch
def test_loop_phase_shifts_the_knots_and_restarts_new_episodes(emu, model, rng):
    x = random_states(model, 9, seed=3)
    B = len(x)
    fz = emu.foot_heights(x)
    g0, g_init = rng.uniform(-0.2, 0.2, B), rng.uniform(0.4, 0.6, B)
    mode_b = np.full(B, _abi.WARM_SHIFT, np.int32)
    mode_b[[2, 5]] = _abi.WARM_COLD
    parked = np.zeros(B, np.int32)
    parked[[5, 7]] = 3                                                   # any state but ALIVE
    ts0 = rng.standard_normal((B, KNOTS, NX))
    sched = (np.full(B, N_EVENTS), np.tile(EVENTS, (B, 1)), np.tile(SEQ, (B, 1)))
    for t, alpha in ((0.5, 0.8), (1.5, 0.0), (3.5, 0.0)):
        ts = ts0.copy()
        g, _, terrain = emu.estimate(x, t, g0, alpha, g_init=g_init, mode_b=mode_b, parked=parked, ts=ts, want_terrain=True)
        start = np.where(mode_b == _abi.WARM_COLD, g_init, g0)           # a new episode starts from its g_init, not from its latch
        want, _ = G.estimate(model, x, t, *sched, start, alpha, foot_z=fz)
        assert np.array_equal(g, want) and np.array_equal(terrain, g)
        assert np.array_equal(ts, G.shift_knots(ts0, g, parked))         # one add per knot, entry 2 alone, a parked instance's knots untouched
        assert np.array_equal(ts[[5, 7]], ts0[[5, 7]]) and not np.array_equal(ts[0, :, 2], ts0[0, :, 2])
        if t == 3.5:                                                     # flight: the start value comes back
            assert np.array_equal(g, start)
    # without the loop's arrays the launch is the stand-alone estimate: the latch always, nothing shifted
    g, _, terrain = emu.estimate(x, 0.5, g0, 0.8)
    want, _ = G.estimate(model, x, 0.5, *sched, g0, 0.8, foot_z=fz)
    assert np.array_equal(g, want) and terrain is None


def test_an_instance_reads_its_own_schedule(emu, model):
    """Four instances in one state, each with a schedule that puts t = 1.0 in another mode; n_events bounds the look-up."""
    x = np.tile(random_states(model, 1, seed=5), (4, 1))
    ev = np.array([[2.0, 3.0, 3.0], [0.5, 3.0, 3.0], [0.2, 0.6, 3.0], [0.2, 0.6, 0.9]])
    seq = np.array([[STANCE, LF, STANCE, STANCE], [STANCE, LF, STANCE, STANCE], [STANCE, LF, RF, STANCE], [STANCE, LF, RF, FLY]], np.int32)
    ne = np.array([2, 2, 3, 3], np.int32)
    g, fz, _ = emu.estimate(x, 1.0, np.full(4, 7.0), schedule=(ne, ev, seq))
    z = fz[0]
    assert np.array_equal(g, [0.5 * (z[0] + z[1]), z[0], z[1], 7.0])
    ne[3] = 2                                                            # the same rows with two events: t is behind the last one, mode_sequence[2]
    g, _, _ = emu.estimate(x, 1.0, np.full(4, 7.0), schedule=(ne, ev, seq))
    assert g[3] == z[1]


# ---------------------------------------------------------------------------------------------- 4. the box above the ground
def test_the_height_box_above_the_ground(emu, model):
    st = _abi.EpisodeSettings()
    solver.load_library().hsqp_episode_defaults(C.byref(st))
    st.min_base_height, st.max_base_height = 0.6, 1.0
    x = model.initial_state.copy()
    x[2] += 0.5
    ground = np.array([0.5])
    assert emu.lib.gr_verdict(C.byref(st), _p(x), None) == _abi.EP_FAILED_BOUNDS
    assert emu.lib.gr_verdict(C.byref(st), _p(x), _p(ground)) == _abi.EP_ALIVE
    x[2] = model.initial_state[2]
    assert emu.lib.gr_verdict(C.byref(st), _p(x), None) == _abi.EP_ALIVE
    assert emu.lib.gr_verdict(C.byref(st), _p(x), _p(ground)) == _abi.EP_FAILED_BOUNDS       # 0.29 m above a ground at 0.5: below the box
    x[4] = 2.0
    st.max_tilt = 1.0
    assert emu.lib.gr_verdict(C.byref(st), _p(x), _p(np.array([0.0]))) == _abi.EP_FAILED_BOUNDS   # the tilt test is what it was


# ---------------------------------------------------------------------------------------------- 5. the binding's own checks
def test_binding_settings_and_shapes():
    lib = solver.load_library()

    class Stub(solver.HipSqpSolver):
        def __init__(self):
            self.lib = lib
    s = Stub()
    st = s.ground_settings()
    assert (st.enabled, st.box_above_ground, st.filter_alpha, st.initial_height) == (1, 0, 0.0, 0.0)
    st = s.ground_settings(box_above_ground=True, filter_alpha=0.8, initial_height=0.5)
    assert (st.enabled, st.box_above_ground, st.filter_alpha, st.initial_height) == (1, 1, 0.8, 0.5)
    assert s.ground_settings(enabled=False).enabled == 0
    with pytest.raises(ValueError):
        s.ground_estimate(np.zeros((2, NX)), 0.0, np.ones(2, np.int32), np.zeros((2, 3)), np.zeros((2, 3), np.int32))
