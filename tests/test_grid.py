"""The ocs2 event-node time grid built per instance with a node count common to the batch (include/hsqp_grid.h, csrc/hsqp_grid.h) on the CPU: the
header, the exported entry points and the binding's struct; the properties of the Python mirror (reference.padded_event_grid) against
reference.event_grid; the host build of the kernel source (tests/grid/grid_emu.cpp) against the mirror, bit for bit; adversarial event arrays with
canaries round every output; a sanitizer program of its own (tests/grid/grid_sanitize.cpp); the padding rule on the CPU oracle (inert) and in the
host warm start (its one, stated consequence)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from wb_humanoid_mpc_amd import _abi, solver
from wb_humanoid_mpc_amd.reference import (EVENT_EPS, GridOverflow, build_node_params_at, cold_start, event_grid, host_warm_start, mode_to_contact_flags,
                                           padded_event_grid, raw_stamps, tile_gait, velocity_command_targets)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
N_NODES, DT, EVENT_NODES, DT_MIN = 12, 0.035, 6, 1e-4
N = N_NODES + EVENT_NODES


def schedules(model, t_final=14.0):
    """walk, run, trot and stance schedules at several phases: (name, event_times)"""
    return [("%s@%g" % (g, s), tile_gait(model.gaits[g], s, t_final).event_times) for g in ("walk", "run", "trot", "stance") for s in (-0.45, -0.2, 0.013)]


# ---------------------------------------------------------------------------------------------- 1. header, library, binding
def _header_functions():
    src = open(os.path.join(ROOT, "include", "hsqp_grid.h")).read()
    src = src[src.index("#ifndef HSQP_GRID_H"):]
    return sorted(set(re.findall(r"\b(hsqp_[a-z_]+)\s*\(", src)))


def test_header_library_and_binding_agree(tmp_path):
    assert _header_functions() == sorted(_abi.GRID_ENTRY_POINTS)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "wb_humanoid_mpc_amd", "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.GRID_ENTRY_POINTS:
        assert n in names, n
        assert getattr(lib, n).argtypes is not None, n
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "hsqp_grid.h"\nint main(void){printf("%zu %d %d %d\\n", sizeof(hsqp_grid_settings), HSQP_GRID_OK, HSQP_GRID_OVERFLOW,'
                   ' HSQP_ABI_VERSION);return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    out = [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert out == [C.sizeof(_abi.GridSettings), _abi.GRID_OK, _abi.GRID_OVERFLOW, 7]
    assert _abi.ABI_VERSION == 7


def test_defaults_and_null_handle():
    lib = solver.load_library()
    d = _abi.GridSettings(event_nodes=-1, reserved=5, dt_min=7.0)
    lib.hsqp_grid_defaults(C.byref(d))
    assert (d.event_nodes, d.reserved, d.dt_min) == (32, 0, 1e-4)
    lib.hsqp_grid_defaults(None)
    z, i = np.zeros(64), np.zeros(8, np.int32)
    p, q = z.ctypes.data_as(_dp), i.ctypes.data_as(_ip)
    assert lib.hsqp_event_grid(None, C.byref(d), 1, 0.0, 4, 0.035, 4, q, p, q, p, p, q) == _abi.ERR_BAD_ARG
    assert lib.hsqp_event_grid_device(None, C.byref(d), 1, 0.0, 4, 0.035, 4, q, p, q, p, p, q) == _abi.ERR_BAD_ARG
    assert lib.hsqp_loop_event_grid(None, C.byref(d)) == _abi.ERR_BAD_ARG
    assert lib.hsqp_loop_grid(None, q, p, p) == _abi.ERR_BAD_ARG and lib.hsqp_loop_grid_device(None, q, p, p) == _abi.ERR_BAD_ARG


def test_the_headers_no_longer_leave_event_grids_out():
    for name in ("hsqp_loop.h", "hsqp_gait.h", "hsqp_episode.h", "hsqp_observe.h", "hsqp_metrics.h"):
        src = open(os.path.join(ROOT, "include", name)).read()
        scope = src[src.index("Out of scope"):] if "Out of scope" in src else ""
        assert "event grids" not in scope.split("*/")[0], name


# ---------------------------------------------------------------------------------------------- 2. properties of the mirror
def test_mirror_pads_the_ocs2_grid_to_a_common_count(model):
    counts = {}
    for name, ev in schedules(model):
        seen = set()
        for c in range(600):   # t0 in steps of 1 / 60 s over 10 s
            t0 = c / 60.0
            dts, nts, nb = padded_event_grid(t0, N_NODES, DT, ev, EVENT_NODES, DT_MIN)
            want_d, want_t = event_grid(t0, t0 + N_NODES * DT, DT, ev)
            assert len(dts) == N and len(nts) == N + 1 and nb + (N - nb) == 18 and nb == len(want_d), (name, c)
            # the real part: nodes 0 .. nb - 1 and the last node, intervals 0 .. nb - 2 and the last interval
            assert np.array_equal(nts[:nb], want_t[:nb]) and nts[N] == want_t[nb], (name, c)
            assert np.array_equal(dts[:nb - 1], want_d[:nb - 1]) and dts[N - 1] == want_d[nb - 1], (name, c)
            # the padding: zero-length intervals whose nodes duplicate node nb - 1, sampling time and all
            assert not dts[nb - 1:N - 1].any() and np.all(nts[nb - 1:N] == nts[nb - 1]), (name, c)
            assert np.all(np.diff(nts) >= 0.0) and dts[N - 1] > 0.0 and np.all(dts >= 0.0), (name, c)
            seen.add(nb)
        counts[name.split("@")[0]] = counts.get(name.split("@")[0], set()) | seen
    for g in ("walk", "run", "trot"):
        assert max(counts[g]) > N_NODES + 1 and max(counts[g]) <= N, (g, counts[g])   # event_nodes = 6 is enough, 1 is not
    with pytest.raises(GridOverflow):
        worst = next(ev for name, ev in schedules(model) if name.startswith("run"))
        for c in range(600):
            padded_event_grid(c / 60.0, N_NODES, DT, worst, 1, DT_MIN)


@pytest.mark.parametrize("n", [1, 2, 8, 12, 100])
def test_mirror_without_an_event_has_n_nodes_intervals(n):
    rng = np.random.default_rng(n)
    for t0 in np.concatenate([np.arange(200) / 60.0, rng.uniform(0.0, 50.0, 300)]):
        for ev in ([], [t0 - 0.3, t0 + n * DT + 0.01]):
            dts, nts, nb = padded_event_grid(t0, n, DT, ev, 3, DT_MIN)
            assert nb == n and not dts[n - 1:n + 2].any() and dts[n + 2] > 0.0 and nts[n + 3] == t0 + n * DT, (n, t0)


def test_mirror_crafted_cases():
    # an event 5e-5 s after t0: the first interval is the event, node 0 sits on the event
    dts, nts, nb = padded_event_grid(0.2, N_NODES, DT, [0.2 + 5e-5], EVENT_NODES)
    assert dts[0] == 0.0 and nts[0] == 0.2 + 5e-5 and nts[1] == 0.2 + 5e-5 + EVENT_EPS and nb == 13
    # an event 5e-5 s after a regular node replaces that node
    t = 0.2
    for _ in range(3):
        t = t + DT
    dts, nts, nb = padded_event_grid(0.2, N_NODES, DT, [t + 5e-5], EVENT_NODES)
    assert t not in nts and nts[3] == t + 5e-5 and dts[3] == 0.0 and nb == 13
    # event_nodes = 0: the uniform count or nothing
    dts, nts, nb = padded_event_grid(0.2, N_NODES, DT, [], 0)
    assert nb == N_NODES and len(dts) == N_NODES
    with pytest.raises(GridOverflow):
        padded_event_grid(0.2, N_NODES, DT, [0.3], 0)
    # an event one rounding error in front of tf (t0 + n_nodes * dt rounds): ocs2 keeps it, with a last interval of 1e-15 s; the raw stamps do not decrease
    t0, e = 0.19999999999999998, 3.6999999999999997
    assert e < t0 + 100 * DT
    dts, nts, nb = padded_event_grid(t0, 100, DT, [e], 4)
    want_d, want_t = event_grid(t0, t0 + 100 * DT, DT, [e])
    assert nb == len(want_d) == 102 and dts[103] == want_d[-1] and 0.0 < dts[103] < 1e-14 and np.array_equal(nts[:nb], want_t[:nb]) and nts[104] == want_t[-1]
    assert np.all(np.diff(raw_stamps(dts, nts)) >= 0.0) and np.diff(nts).min() > -1.0001 * EVENT_EPS
    for bad in ([0.5, 0.3], [float("nan"), 0.3, 0.25]):
        with pytest.raises(GridOverflow):
            padded_event_grid(0.2, N_NODES, DT, bad, EVENT_NODES)
    with pytest.raises(GridOverflow):
        padded_event_grid(1e20, N_NODES, DT, [], EVENT_NODES)   # t + dt == t: the loop gives up


# ---------------------------------------------------------------------------------------------- 3. the host build of the kernel source against the mirror
@pytest.fixture(scope="module")
def gemu(tmp_path_factory):
    lib_path = tmp_path_factory.mktemp("grid") / "libgrid_emu.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fPIC", "-shared",
                           "-I", CSRC, os.path.join(ROOT, "tests", "grid", "grid_emu.cpp"), "-o", str(lib_path)])
    lib = C.CDLL(str(lib_path))
    lib.gr_build.argtypes = [C.c_int, C.c_double, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, _ip, _dp, _ip, _dp, _dp, _ip]
    return lib


CANARY = -12345.678


def emu_build(lib, t0, n_nodes, dt, dt_min, event_nodes, n_events, events):
    """The host build over B instances, with a canary row in front of and behind every output: (n_intervals, dts, nts, status)."""
    n_events, events = np.ascontiguousarray(n_events, dtype=np.int32), np.ascontiguousarray(events, dtype=np.float64)
    B, E, n = events.shape[0], events.shape[1], n_nodes + event_nodes
    ni, st = np.full(B + 2, -7, np.int32), np.full(B + 2, -7, np.int32)
    dts, nts = np.full((B + 2, n), CANARY), np.full((B + 2, n + 1), CANARY)
    keep = events.copy()
    lib.gr_build(B, t0, n_nodes, dt, dt_min, event_nodes, E, n_events.ctypes.data_as(_ip), events.ctypes.data_as(_dp), ni[1:].ctypes.data_as(_ip), dts[1:].ctypes.data_as(_dp),
                 nts[1:].ctypes.data_as(_dp), st[1:].ctypes.data_as(_ip))
    assert ni[0] == ni[-1] == st[0] == st[-1] == -7 and np.all(dts[[0, -1]] == CANARY) and np.all(nts[[0, -1]] == CANARY)
    assert np.array_equal(keep, events, equal_nan=True)
    return ni[1:-1], dts[1:-1], nts[1:-1], st[1:-1]


def assert_equals_mirror(got, b, t0, n_nodes, dt, dt_min, event_nodes, events):
    ni, dts, nts, st = got
    try:
        want = padded_event_grid(t0, n_nodes, dt, events, event_nodes, dt_min)
    except GridOverflow:
        assert st[b] == _abi.GRID_OVERFLOW and ni[b] == 0, (t0, events)
        t = np.concatenate([[t0], t0 + np.zeros(n_nodes + event_nodes)])
        for k in range(n_nodes + event_nodes):
            t[k + 1] = t[k] + dt
        assert np.array_equal(nts[b], t) and np.array_equal(dts[b], np.diff(t)), (t0, events)   # the filler: the uniform grid
        return False
    assert st[b] == _abi.GRID_OK and ni[b] == want[2], (t0, events)
    assert np.array_equal(dts[b], want[0]) and np.array_equal(nts[b], want[1]), (t0, events)
    return True


def test_host_build_equals_the_mirror_bit_for_bit(model, gemu):
    rng = np.random.default_rng(20261019)
    scheds = [np.array(ev) for _, ev in schedules(model)]
    ok = bad = 0
    for case in range(3000):
        n_nodes, event_nodes = int(rng.integers(1, 20)), int(rng.integers(0, 9))
        dt = DT if case % 3 else float(rng.uniform(0.01, 0.06))
        t0 = float(rng.uniform(0.0, 10.0)) if case % 2 else int(rng.integers(0, 600)) / 60.0
        ev = scheds[case % len(scheds)]
        ev = ev[(ev > t0 - 0.5) & (ev < t0 + n_nodes * dt + 0.5)][:16]
        row = np.concatenate([ev, np.full(16 - len(ev), ev[-1] if len(ev) else 0.0)])
        got = emu_build(gemu, t0, n_nodes, dt, DT_MIN, event_nodes, [len(ev)], row[None])
        if assert_equals_mirror(got, 0, t0, n_nodes, dt, DT_MIN, event_nodes, list(ev)):
            ok += 1
        else:
            bad += 1
    assert ok > 1000 and bad > 100, (ok, bad)   # the sweep has both grids and overflows
    # the crafted cases, one batch: first-interval event, a node replaced, event_nodes = 0 (own call), overflow by one interval
    t3 = 0.2
    for _ in range(3):
        t3 = t3 + DT
    rows = [[0.2 + 5e-5], [t3 + 5e-5], [0.3], [0.25, 0.3]]
    ev = np.array([r + [r[-1]] * (4 - len(r)) for r in rows])
    got = emu_build(gemu, 0.2, N_NODES, DT, DT_MIN, EVENT_NODES, [len(r) for r in rows], ev)
    for b, r in enumerate(rows):
        assert assert_equals_mirror(got, b, 0.2, N_NODES, DT, DT_MIN, EVENT_NODES, r)
    assert got[1][0, 0] == 0.0 and got[0].tolist() == [13, 13, 14, 16]
    got = emu_build(gemu, 0.2, N_NODES, DT, DT_MIN, 0, [0, 1], np.array([[0.3], [0.3]]))
    assert assert_equals_mirror(got, 0, 0.2, N_NODES, DT, DT_MIN, 0, []) and not assert_equals_mirror(got, 1, 0.2, N_NODES, DT, DT_MIN, 0, [0.3])
    got = emu_build(gemu, 0.2, N_NODES, DT, DT_MIN, 3, [2, 2], np.array([[0.25, 0.3], [0.25, 0.9]]))
    assert got[3].tolist() == [_abi.GRID_OVERFLOW, _abi.GRID_OK]           # 16 intervals do not fit 15; the neighbour is untouched by it
    assert assert_equals_mirror(got, 1, 0.2, N_NODES, DT, DT_MIN, 3, [0.25, 0.9])


# ---------------------------------------------------------------------------------------------- 4. unsorted and non-finite event arrays
def test_adversarial_events_end_with_a_status_inside_their_rows(gemu):
    nan, inf = float("nan"), float("inf")
    rows = [[0.5, 0.3, 0.4, 0.25], [nan, 0.3, inf, -inf], [nan] * 4, [0.3, 0.3, 0.3, 0.3], [0.6, 0.5, 0.4, 0.3], [0.3, nan, 0.25, 0.31], [0.25, 0.3, 0.45, 0.9]]
    ev = np.array(rows)
    for n_events in ([4] * len(rows), [1000000] * len(rows), [-3] * len(rows), [2] * len(rows)):
        ni, dts, nts, st = got = emu_build(gemu, 0.2, N_NODES, DT, DT_MIN, EVENT_NODES, n_events, ev)   # (the canaries are checked inside)
        assert set(st.tolist()) <= {_abi.GRID_OK, _abi.GRID_OVERFLOW}
        assert np.isfinite(dts).all() and np.isfinite(nts).all() and np.all(dts >= 0.0) and np.all(np.diff(nts, axis=1) >= -1.0001 * EVENT_EPS)
        for b, r in enumerate(rows):
            assert_equals_mirror(got, b, 0.2, N_NODES, DT, DT_MIN, EVENT_NODES, r[:min(max(n_events[b], 0), 4)])
        if n_events[0] in (4, 1000000):   # (n_events is clamped to max_events) unsorted rows have no grid, NaN entries are filtered out, the sorted row has one
            assert st.tolist() == [_abi.GRID_OVERFLOW, _abi.GRID_OK, _abi.GRID_OK, _abi.GRID_OVERFLOW, _abi.GRID_OVERFLOW, _abi.GRID_OVERFLOW, _abi.GRID_OK]
            assert ni.tolist()[:6] == [0, 14, 12, 0, 0, 0] and ni[6] > 14
        if n_events[0] == -3:
            assert st.tolist() == [_abi.GRID_OK] * len(rows) and ni.tolist() == [12] * len(rows)


# ---------------------------------------------------------------------------------------------- 5. sanitizers: a program of its own
def test_adversarial_inputs_under_sanitizers(tmp_path):
    exe = tmp_path / "grid_sanitize"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tests", "grid", "grid_emu.cpp"),
                           os.path.join(ROOT, "tests", "grid", "grid_sanitize.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    assert out.strip() == "grid ok"


# ---------------------------------------------------------------------------------------------- 6. padding is inert on the oracle
def pad_map(nb, n):
    """index of the unpadded node behind every node of the padded grid [n + 1], and of the unpadded interval behind every padded interval [n]
    (-1: a padding interval)"""
    nodes = list(range(nb)) + [nb - 1] * (n - nb) + [nb]
    intervals = list(range(nb - 1)) + [-1] * (n - nb) + [nb - 1]
    return np.array(nodes), np.array(intervals)


def walk_case(model, want_nb=15, want_events=2):
    """a start time at which the walk's ocs2 grid over 12 x 0.035 s has `want_nb` intervals with `want_events` events"""
    ev = tile_gait(model.gaits["walk"], -0.45, 6.0)
    for c in range(600):
        t0 = 0.2 + c / 60.0
        dts, nts, nb = padded_event_grid(t0, N_NODES, DT, ev.event_times, EVENT_NODES, DT_MIN)
        if nb == want_nb and int((dts[:nb - 1] == 0.0).sum()) == want_events:   # (from interval nb - 1 on: the padding, then the last real interval)
            return t0, ev, dts, nts, nb
    raise AssertionError("no such start time")


def test_padding_is_inert_on_the_oracle(model, oracle):
    t0, schedule, dts, nts, nb = walk_case(model)
    assert nb == 15 and N - nb == 3
    nodes, intervals = pad_map(nb, N)
    real_nodes = np.concatenate([np.arange(nb), [N]])
    ud, ut = np.concatenate([dts[:nb - 1], dts[N - 1:]]), nts[real_nodes]
    assert np.array_equal(ud, event_grid(t0, t0 + N_NODES * DT, DT, schedule.event_times)[0])
    rng = np.random.default_rng(5)
    x0 = model.initial_state.copy()
    x0[6:6 + model.nj] += 0.03 * rng.standard_normal(model.nj)
    x0[6 + model.nj:] += 0.05 * rng.standard_normal(6 + model.nj)
    targets = velocity_command_targets(model, (0.3, 0.0, 0.7925, 0.0), t0, x0, N_NODES * DT)
    par = build_node_params_at(model, schedule, targets, ut)
    x, u = cold_start(model, x0, par)
    x, u = x + 0.01 * rng.standard_normal(x.shape), u + 0.5 * rng.standard_normal(u.shape)
    # the padded problem: parameters from its own node times, the trajectory of the node each padded node duplicates
    par_p = build_node_params_at(model, schedule, targets, nts)
    assert np.array_equal(par_p, par[nodes])
    x_p, u_p = x[nodes], u[np.where(intervals < 0, nb - 1, intervals)]
    out = []
    for grid, args in ((ud, (x0, x, u, par)), (dts, (x0, x_p, u_p, par_p))):
        oracle.set_grid(grid)
        try:
            out.append(oracle.sqp_iteration(0.0, *args, threads=1))
        finally:
            oracle.set_grid(None)
    a, b = out
    real_iv = np.flatnonzero(intervals >= 0)
    assert np.array_equal(b["dx"][real_nodes], a["dx"]) and np.array_equal(b["du"][real_iv], a["du"])
    assert np.array_equal(b["dx"][nb - 1:N], np.repeat(a["dx"][nb - 1:nb], N - nb + 1, axis=0)) and not b["du"][intervals < 0].any()
    for k in ("perf_before", "perf_after"):
        assert a[k] == b[k], k
    assert np.array_equal(a["kkt"], b["kkt"])


# ---------------------------------------------------------------------------------------------- 7. the warm-start consequence
def test_padding_changes_the_shifted_inputs_only_inside_the_last_but_one_interval(model):
    schedule = tile_gait(model.gaits["walk"], -0.45, 6.0)
    contact = lambda nts: np.array([[mode_to_contact_flags(schedule.mode_at(t)) for t in nts]], dtype=float)  # noqa: E731
    F = lambda s: np.stack([np.sin(0.7 * j + 3.0 * s) for j in range(_abi.NX)], axis=-1)[None]  # noqa: E731  (a state is a function of the stamp: continuous over an event)
    rng = np.random.default_rng(11)
    x_init = F(np.array([0.0]))[:, 0]
    prev_u = prev_p = None
    differing = padded_cycles = 0
    for c in range(41):
        t0 = 0.2 + c / 60.0
        dts, nts, nb = padded_event_grid(t0, N_NODES, DT, schedule.event_times, EVENT_NODES, DT_MIN)
        nodes, intervals = pad_map(nb, N)
        real_nodes, real_iv = np.concatenate([np.arange(nb), [N]]), np.flatnonzero(intervals >= 0)
        ud, ut = dts[real_iv], nts[real_nodes]
        st_u, st_p = raw_stamps(ud, ut), raw_stamps(dts, nts)
        assert np.array_equal(st_p[real_nodes], st_u) and np.array_equal(st_p, st_u[nodes])
        if prev_u is not None:
            xu, uu = host_warm_start(model.total_mass, x_init, st_u, contact(ut), prev_u)
            xp, up = host_warm_start(model.total_mass, x_init, st_p, contact(nts), prev_p)
            assert np.array_equal(xp[:, real_nodes], xu), c                                  # states: bit-identical
            assert np.array_equal(xp, xu[:, nodes]), c
            lo, hi = prev_u["times"][-3], prev_u["times"][-2]                                # the old grid's last-but-one real interval
            inside = (st_u[:nb] > lo) & (st_u[:nb] < hi)                                     # (the input of interval k lives on node k)
            same = np.all(up[0, real_iv] == uu[0], axis=1)
            assert np.all(same | inside), (c, np.flatnonzero(~same), inside)
            assert inside.sum() <= 1 or prev_pad == 0, c
            differing += int((~same).sum())
            padded_cycles += int(prev_pad > 0)
        # this cycle's "solution": states a function of the stamp, inputs independent per real interval; padding intervals hold garbage
        x_u, u_u = F(st_u), rng.standard_normal((1, nb, _abi.NU))
        u_p = np.where((intervals >= 0)[None, :, None], u_u[:, np.maximum(intervals, 0)], 1e3)
        prev_u, prev_p, prev_pad = dict(times=st_u, x=x_u, u=u_u), dict(times=st_p, x=x_u[:, nodes], u=u_p), N - nb
    assert padded_cycles == 40 and differing >= 1   # every cycle is padded, and the consequence does occur
