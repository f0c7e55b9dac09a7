"""Per-instance failure isolation and episode reset of the resident loop (include/hsqp_episode.h, csrc/hsqp_episode.h) on the CPU: the header, the
exported entry points and the binding's struct; the host build of the triage / reset sources (tests/episode/episode_emu.cpp) against a numpy
restatement, exactly (the logic is comparisons and copies); the warm start with a per-instance mode (csrc/hsqp_warm.h, WarmArgs::mode_b) against
the existing host build of the batch-wide mode (tests/warm/warm_emu.cpp), bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_warm_start import MASS, build_emu, previous_solution, run_emu, uniform_grid
from wb_humanoid_mpc_amd import _abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
NX, NU, CMD_N = _abi.NX, _abi.NU, _abi.CMD_N
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
ALIVE, NUMERIC, ROLLOUT, BOUNDS = _abi.EP_ALIVE, _abi.EP_FAILED_NUMERIC, _abi.EP_FAILED_ROLLOUT, _abi.EP_FAILED_BOUNDS
STANCE = 3


# ---------------------------------------------------------------------------------------------- header, library, binding
def _header_functions():
    src = open(os.path.join(ROOT, "include", "hsqp_episode.h")).read()
    src = src[src.index("#ifndef HSQP_EPISODE_H"):]
    return sorted(set(re.findall(r"\b(hsqp_[a-z_]+)\s*\(", src)))


def test_header_library_and_binding_agree(tmp_path):
    assert _header_functions() == sorted(_abi.EPISODE_ENTRY_POINTS)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "wb_humanoid_mpc_amd", "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.EPISODE_ENTRY_POINTS:
        assert n in names, n
        assert getattr(lib, n).argtypes is not None, n
    body = ('#include <stddef.h>\n#include <stdio.h>\n#include "hsqp_episode.h"\nint main(void){printf("%zu %zu %zu %zu %zu %d %d %d %d %d %d %d\\n", sizeof(hsqp_episode_settings),'
            ' offsetof(hsqp_episode_settings, on_failure), offsetof(hsqp_episode_settings, min_base_height), offsetof(hsqp_episode_settings, max_base_height),'
            ' offsetof(hsqp_episode_settings, max_tilt), HSQP_EPISODE_PARK, HSQP_EPISODE_RESET, HSQP_EP_ALIVE, HSQP_EP_FAILED_NUMERIC, HSQP_EP_FAILED_ROLLOUT,'
            ' HSQP_EP_FAILED_BOUNDS, HSQP_ABI_VERSION);return 0;}\n')
    E = _abi.EpisodeSettings
    want = [C.sizeof(E), E.on_failure.offset, E.min_base_height.offset, E.max_base_height.offset, E.max_tilt.offset, _abi.EPISODE_PARK, _abi.EPISODE_RESET,
            ALIVE, NUMERIC, ROLLOUT, BOUNDS, 7]
    for name, cc, std in (("sz.c", "gcc", "-std=c99"), ("sz.cpp", "g++", "-std=c++17")):      # the header as C and as C++
        (tmp_path / name).write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / name), "-o", str(tmp_path / "sz")])
        assert [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()] == want, cc
    assert _abi.ABI_VERSION == 7


def test_defaults_and_null_handle():
    lib = solver.load_library()
    st = _abi.EpisodeSettings()
    st.on_failure = 5
    lib.hsqp_episode_defaults(C.byref(st))
    assert (st.on_failure, st.min_base_height, st.max_base_height, st.max_tilt) == (_abi.EPISODE_PARK, -np.inf, np.inf, np.inf)
    lib.hsqp_episode_defaults(None)
    i = np.zeros(2, np.int32).ctypes.data_as(_ip)
    assert lib.hsqp_loop_isolate(None, C.byref(st), None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_loop_reset_instances(None, 1, i, None, None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_loop_episodes(None, i, i, i, i, i) == _abi.ERR_BAD_ARG
    assert lib.hsqp_loop_episodes_device(None, i, i, i, i, i) == _abi.ERR_BAD_ARG


# ---------------------------------------------------------------------------------------------- the host build of the kernel sources
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    lib_path = tmp_path_factory.mktemp("episode") / "libepisode_emu.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fPIC", "-shared",
                           "-I", CSRC, os.path.join(ROOT, "tests", "episode", "episode_emu.cpp"), "-o", str(lib_path)])
    lib = C.CDLL(str(lib_path))
    lib.ep_triage.argtypes = [C.POINTER(_abi.EpisodeSettings), C.c_int, C.c_int, _ip, _dp, _ip, _dp, _dp, _dp] + [_ip] * 7 + [_dp] * 5 + [_ip]
    lib.ep_host_reset.argtypes = [C.c_int, _ip, _dp, _dp, _dp] + [_ip] * 7 + [_dp] * 4
    lib.ep_commands.argtypes = [C.c_int, _ip, _dp, _dp, _dp]
    lib.ep_gait_reset.argtypes = [C.c_int, C.c_int, _ip, _ip, C.c_double, _ip, _dp, _ip, _ip, _dp]
    lib.ep_warm.argtypes = [C.c_int, _ip, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double] + [_dp] * 10
    return lib


def _p(a):
    if a is None:
        return None
    return a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


INT_KEYS = ("state", "cause", "fail_cycle", "n_failures", "n_episodes", "mode", "reset")


class Batch:
    """The resident arrays of B instances in the device layout."""

    def __init__(self, rng, B):
        self.B = B
        self.state, self.cause, self.n_failures = (np.zeros(B, np.int32) for _ in range(3))
        self.fail_cycle, self.n_episodes = np.full(B, -1, np.int32), np.ones(B, np.int32)
        self.mode, self.reset = np.full(B, _abi.WARM_SHIFT, np.int32), np.zeros(B, np.int32)
        self.x_reset, self.v_cmd = rng.standard_normal((B, NX)), rng.standard_normal((B, CMD_N))
        self.x, self.v_filt, self.v_use = rng.standard_normal((B, NX)), rng.standard_normal((B, CMD_N)), self.v_cmd.copy()

    def copy(self):
        c = object.__new__(Batch)
        c.__dict__ = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()}
        return c

    def assert_equal(self, other, where):
        for k, v in self.__dict__.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(v, other.__dict__[k], equal_nan=True), (where, k)


def settings(on_failure, lo=-np.inf, hi=np.inf, tilt=np.inf):
    st = _abi.EpisodeSettings()
    st.on_failure, st.min_base_height, st.max_base_height, st.max_tilt = on_failure, lo, hi, tilt
    return st


def np_verdict(st, it_status, perf, ro_status, xs):
    """include/hsqp_episode.h, step 6, restated"""
    if it_status != 0 or not np.isfinite(perf).all():
        return NUMERIC
    if ro_status != _abi.ROLLOUT_OK or not np.isfinite(xs).all():
        return ROLLOUT
    if xs[2] < st.min_base_height or xs[2] > st.max_base_height or abs(xs[4]) > st.max_tilt or abs(xs[5]) > st.max_tilt:
        return BOUNDS
    return ALIVE


def np_command(state, v_cmd, x_reset):
    return v_cmd.copy() if state == ALIVE else np.array([0.0, 0.0, x_reset[2], 0.0])


def np_triage(st, cycle, bt, it_status, perf, ro_status, xs, x_log, u_log):
    causes = []
    for b in range(bt.B):
        before = bt.state[b]
        cause = np_verdict(st, it_status[b], perf[b], ro_status[b], xs[b])
        failed = cause != ALIVE
        after = (ALIVE if st.on_failure == _abi.EPISODE_RESET else cause) if failed else before
        if failed:
            bt.x[b] = bt.x_reset[b]
            bt.v_filt[b] = np_command(after, bt.v_cmd[b], bt.x_reset[b])
            bt.state[b], bt.cause[b], bt.fail_cycle[b] = after, cause, cycle
            bt.n_failures[b] += 1
            if st.on_failure == _abi.EPISODE_RESET:
                bt.n_episodes[b] += 1
        bt.v_use[b] = np_command(after, bt.v_cmd[b], bt.x_reset[b])
        if failed or before != ALIVE:
            if x_log is not None:
                x_log[b] = np.nan
            if u_log is not None:
                u_log[b] = np.nan
        bt.mode[b] = _abi.WARM_COLD if failed else _abi.WARM_SHIFT
        bt.reset[b] = 1 if failed else 0
        causes.append(cause)
    return np.array(causes, np.int32)


def emu_triage(lib, st, cycle, bt, it_status, perf, ro_status, xs, x_log, u_log):
    out = np.zeros(bt.B, np.int32)
    lib.ep_triage(C.byref(st), cycle, bt.B, _p(it_status), _p(perf), _p(ro_status), _p(xs), _p(bt.x_reset), _p(bt.v_cmd), *[_p(getattr(bt, k)) for k in INT_KEYS],
                  _p(bt.x), _p(bt.v_filt), _p(bt.v_use), _p(x_log), _p(u_log), _p(out))
    return out


def random_cycle(rng, B, lo, hi, tilt):
    """What a cycle leaves on the device for B instances: every cause, and every way into it, at random"""
    it_status = np.where(rng.random(B) < 0.12, rng.integers(1, 4, B), 0).astype(np.int32)
    perf = rng.standard_normal((B, 4))
    for b in np.flatnonzero(rng.random(B) < 0.12):
        perf[b, rng.integers(0, 4)] = rng.choice([np.nan, np.inf, -np.inf])
    ro_status = np.where(rng.random(B) < 0.15, rng.integers(1, 3, B), 0).astype(np.int32)
    xs = 0.1 * rng.standard_normal((B, NX))
    xs[:, 2] = 0.5 * (lo + hi) + 0.7 * (hi - lo) * (rng.random(B) - 0.5) if np.isfinite(lo + hi) else rng.standard_normal(B)
    if np.isfinite(tilt):
        xs[:, 4:6] = 1.4 * tilt * (rng.random((B, 2)) - 0.5) * 2.0
    for b in np.flatnonzero(rng.random(B) < 0.12):
        xs[b, rng.integers(0, NX)] = rng.choice([np.nan, np.inf, -np.inf])
    return it_status, perf, ro_status, xs


@pytest.mark.parametrize("policy", [_abi.EPISODE_PARK, _abi.EPISODE_RESET])
@pytest.mark.parametrize("box", [(-np.inf, np.inf, np.inf), (0.7, 0.9, 0.3), (0.75, np.inf, np.inf)])
def test_triage_equals_the_restatement(emu, rng, policy, box):
    B, cycles = 96, 40
    st = settings(policy, *box)
    got, want = Batch(rng, B), None
    want = got.copy()
    seen, refail, host_resets = set(), 0, 0
    for c in range(cycles):
        cyc = random_cycle(rng, B, *box)
        got.x[:] = cyc[3]; want.x[:] = cyc[3]                          # step 5 has copied the rolled-out state
        logs = [rng.standard_normal((B, NX)), rng.standard_normal((B, NU))] if c % 3 else [None, None]
        logs_w = [None if a is None else a.copy() for a in logs]
        parked_before = want.state != ALIVE
        cg = emu_triage(emu, st, c, got, *cyc, *logs)
        cw = np_triage(st, c, want, *cyc, *logs_w)
        assert np.array_equal(cg, cw), c
        got.assert_equal(want, c)
        for a, b in zip(logs, logs_w):
            assert a is None or np.array_equal(a, b, equal_nan=True)
        seen |= set(cw.tolist())
        refail += int((parked_before & (cw != ALIVE)).sum())
        # invariants of include/hsqp_episode.h
        failed = cw != ALIVE
        assert np.array_equal(got.x[failed], got.x_reset[failed]) and np.array_equal(got.x[~failed], cyc[3][~failed], equal_nan=True)
        assert (got.fail_cycle[failed] == c).all() and (got.mode == np.where(failed, _abi.WARM_COLD, _abi.WARM_SHIFT)).all() and (got.reset == failed).all()
        if policy == _abi.EPISODE_RESET:
            assert (got.state == ALIVE).all() and np.array_equal(got.n_episodes, 1 + got.n_failures + host_resets * np.isin(np.arange(B), [1, 5, 9])) and np.array_equal(got.v_use, got.v_cmd)
            assert np.array_equal(got.v_filt[failed], got.v_cmd[failed])
        else:
            parked = got.state != ALIVE
            assert np.array_equal(got.state[parked], got.cause[parked]) and (got.n_episodes == 1 + host_resets * np.isin(np.arange(B), [1, 5, 9])).all()
            stance = np.zeros((B, CMD_N)); stance[:, 2] = got.x_reset[:, 2]
            assert np.array_equal(got.v_use, np.where(parked[:, None], stance, got.v_cmd)) and np.array_equal(got.v_filt[failed], stance[failed])
            if logs[0] is not None:
                assert np.isnan(logs[0][parked]).all() and np.isnan(logs[1][parked]).all() and np.isfinite(logs[0][~parked]).all()
        if c % 10 == 9:                                                # the host puts three instances back on their feet, one with a new state and command
            ids = np.array([5, 1, 9], np.int32)
            x0, vn = (rng.standard_normal((3, NX)), rng.standard_normal((3, CMD_N))) if c % 20 == 9 else (None, None)
            emu.ep_host_reset(3, _p(ids), _p(x0), _p(vn), _p(got.x_reset), *[_p(getattr(got, k)) for k in INT_KEYS], _p(got.x), _p(got.v_cmd), _p(got.v_filt), _p(got.v_use))
            for i, b in enumerate(ids):
                want.x[b] = want.x_reset[b] if x0 is None else x0[i]
                if vn is not None:
                    want.v_cmd[b] = vn[i]
                want.v_filt[b] = want.v_use[b] = want.v_cmd[b]
                want.state[b], want.mode[b], want.reset[b] = ALIVE, _abi.WARM_COLD, 1
                want.n_episodes[b] += 1
            host_resets += 1
            got.assert_equal(want, ("host reset", c))
            assert (got.state[ids] == ALIVE).all()
    finite_box = np.isfinite(box[0]) or np.isfinite(box[2])
    assert seen == ({ALIVE, NUMERIC, ROLLOUT, BOUNDS} if finite_box else {ALIVE, NUMERIC, ROLLOUT})
    assert got.n_failures.max() >= 2
    if policy == _abi.EPISODE_PARK:
        assert refail > 0                                              # a parked instance failed again and was reset the same way


def test_verdict_order_and_known_answers(emu, rng):
    """One instance per row of the table: the first cause that applies wins; bounds are strict comparisons; -inf / +inf switch a bound off."""
    st = settings(_abi.EPISODE_PARK, 0.7, 0.9, 0.3)
    ok_x = np.zeros(NX); ok_x[2] = 0.8
    rows = [(0, [1, 1, 0, 0], 0, {}, ALIVE), (2, [1, 1, 0, 0], 2, {2: np.nan}, NUMERIC), (0, [np.inf, 1, 0, 0], 0, {}, NUMERIC), (0, [1, 1, np.nan, 0], 1, {2: 5.0}, NUMERIC),
            (0, [1, 1, 0, 0], 1, {2: 5.0}, ROLLOUT), (0, [1, 1, 0, 0], 2, {}, ROLLOUT), (0, [1, 1, 0, 0], 0, {57: np.nan, 2: 5.0}, ROLLOUT), (0, [1, 1, 0, 0], 0, {2: -np.inf}, ROLLOUT),
            (0, [1, 1, 0, 0], 0, {2: 0.7}, ALIVE), (0, [1, 1, 0, 0], 0, {2: 0.9}, ALIVE), (0, [1, 1, 0, 0], 0, {2: 0.6999}, BOUNDS), (0, [1, 1, 0, 0], 0, {2: 0.9001}, BOUNDS),
            (0, [1, 1, 0, 0], 0, {4: 0.3}, ALIVE), (0, [1, 1, 0, 0], 0, {4: -0.31}, BOUNDS), (0, [1, 1, 0, 0], 0, {5: 0.31}, BOUNDS), (0, [1, 1, 0, 0], 0, {3: 3.0}, ALIVE)]
    B = len(rows)
    xs = np.tile(ok_x, (B, 1))
    for b, r in enumerate(rows):
        for k, v in r[3].items():
            xs[b, k] = v
    it, perf, ro = np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], float), np.array([r[2] for r in rows], np.int32)
    bt = Batch(rng, B)
    assert list(emu_triage(emu, st, 0, bt, it, perf, ro, xs, None, None)) == [r[4] for r in rows]
    off = Batch(rng, B)
    got = emu_triage(emu, settings(_abi.EPISODE_PARK), 0, off, it, perf, ro, xs, None, None)
    assert list(got) == [ALIVE if r[4] == BOUNDS else r[4] for r in rows]


def test_command_in_use(emu, rng):
    B = 9
    state = rng.integers(0, 4, B).astype(np.int32)
    v_cmd, x_reset, out = rng.standard_normal((B, CMD_N)), rng.standard_normal((B, NX)), np.zeros((B, CMD_N))
    emu.ep_commands(B, _p(state), _p(v_cmd), _p(x_reset), _p(out))
    assert np.array_equal(out, np.array([np_command(s, v, x) for s, v, x in zip(state, v_cmd, x_reset)]))


@pytest.mark.parametrize("by_ids", [False, True])
def test_gait_reset_of_chosen_instances(emu, rng, by_ids):
    """The chosen instances get the state hsqp_gait_reset gives every instance at t; the others keep theirs to the bit."""
    B, E, t = 7, 12, 0.1 + 1.0 / 3.0
    n = rng.integers(1, E, B).astype(np.int32)
    ev, seq = rng.standard_normal((B, E)), rng.integers(0, 4, (B, E + 1)).astype(np.int32)
    scal, tc = rng.integers(0, 5, (B, 4)).astype(np.int32), rng.standard_normal(B)
    before = [a.copy() for a in (n, ev, seq, scal, tc)]
    chosen = np.array([4, 0, 6], np.int32)
    flags = np.isin(np.arange(B), chosen).astype(np.int32)
    if by_ids:
        emu.ep_gait_reset(E, len(chosen), _p(chosen), None, t, _p(n), _p(ev), _p(seq), _p(scal), _p(tc))
    else:
        emu.ep_gait_reset(E, B, None, _p(flags), t, _p(n), _p(ev), _p(seq), _p(scal), _p(tc))
    for b in range(B):
        if flags[b]:
            assert n[b] == 1 and (ev[b] == t + 0.5).all() and (seq[b] == STANCE).all() and (scal[b] == 0).all() and tc[b] == t
        else:
            assert all(np.array_equal(a[b], o[b]) for a, o in zip((n, ev, seq, scal, tc), before))


# ---------------------------------------------------------------------------------------------- k_warm_start's node logic with a mode per instance
def emu_warm(lib, mode, mode_b, grid, x_init, prev):
    B, N, Np = grid.B, grid.N, prev["u"].shape[1]
    x, u, st = np.full((B, N + 1, NX), -1.0), np.full((B, N, NU), -1.0), np.full((B, N + 1), -1.0)
    par, dts = np.zeros((B, N + 1, lib.ep_node_params())), np.zeros((B, N))
    arrays = [np.ascontiguousarray(a, dtype=float) for a in (grid.flags, x_init, prev["x"], prev["u"], prev["stamps"])]
    lib.ep_warm(mode, _p(mode_b), B, N, Np, 0, grid.t0, grid.dt, MASS, *[_p(a) for a in arrays], _p(par), _p(dts), _p(x), _p(u), _p(st))
    return x, u, st


def test_warm_start_with_a_mode_per_instance(emu, tmp_path, rng):
    exe = build_emu(tmp_path)                                          # the existing host build: the batch-wide mode (WarmArgs::mode_b == null)
    B = 6
    old, new = uniform_grid(B, 20, 0.0, rng), uniform_grid(B, 18, 0.0437, rng)
    prev = previous_solution(rng, old)
    x_init = rng.standard_normal((B, NX))
    whole = {m: run_emu(exe, tmp_path, m, new, x_init, prev) for m in (_abi.WARM_SHIFT, _abi.WARM_COLD)}
    assert not np.array_equal(whole[_abi.WARM_SHIFT][0], whole[_abi.WARM_COLD][0])
    for m in (_abi.WARM_SHIFT, _abi.WARM_COLD):                        # the new source, no array / a uniform array: the batch-wide mode bit for bit
        for mode_b in (None, np.full(B, m, np.int32)):
            got = emu_warm(emu, _abi.WARM_SHIFT if mode_b is not None else m, mode_b, new, x_init, prev)
            assert all(np.array_equal(g, w) for g, w in zip(got, whole[m])), (m, mode_b is None)
    mixed = np.array([_abi.WARM_SHIFT, _abi.WARM_COLD, _abi.WARM_COLD, _abi.WARM_SHIFT, _abi.WARM_COLD, _abi.WARM_SHIFT], np.int32)
    got = emu_warm(emu, _abi.WARM_SHIFT, mixed, new, x_init, prev)
    for b in range(B):                                                 # every instance equals the batch-wide run of its own mode
        assert all(np.array_equal(g[b], w[b]) for g, w in zip(got, whole[int(mixed[b])])), b
    # a COLD instance does not read its previous solution: all NaN there, finite out, and the same bits
    sick = dict(x=prev["x"].copy(), u=prev["u"].copy(), stamps=prev["stamps"].copy())
    for b in np.flatnonzero(mixed == _abi.WARM_COLD):
        sick["x"][b] = np.nan; sick["u"][b] = np.nan; sick["stamps"][b] = np.nan
    again = emu_warm(emu, _abi.WARM_SHIFT, mixed, new, x_init, sick)
    assert all(np.isfinite(a).all() for a in again) and all(np.array_equal(a, g) for a, g in zip(again, got))
