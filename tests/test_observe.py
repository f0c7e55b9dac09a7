"""The observation model of the resident loop (include/hsqp_observe.h, csrc/hsqp_observe.h) on the CPU: the header, the exported entry points and the
binding's structs; the host build of the kernel's sources (tests/observe/observe_emu.cpp) against the numpy restatement (tests/observe_ref.py) — the
generator's integers exactly, the normals within the accuracy of the library functions, the statistics of the stream, the arithmetic of y, the ring
and a cycle's bookkeeping exactly — and the argument checks that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import observe_ref as O
from wb_humanoid_mpc_amd import _abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
NX = _abi.NX
_dp, _ip, _up = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
_oi, _os = C.POINTER(_abi.ObserveInstance), C.POINTER(_abi.ObserveSettings)
SEED = 2026


# ---------------------------------------------------------------------------------------------- 1. header, library, binding
def _header_functions():
    src = open(os.path.join(ROOT, "include", "hsqp_observe.h")).read()
    src = src[src.index("#ifndef HSQP_OBSERVE_H"):]
    return sorted(set(re.findall(r"\b(hsqp_[a-z_]+)\s*\(", src)))


def test_header_library_and_binding_agree(tmp_path):
    assert _header_functions() == sorted(_abi.OBSERVE_ENTRY_POINTS)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "wb_humanoid_mpc_amd", "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.OBSERVE_ENTRY_POINTS:
        assert n in names, n
        assert getattr(lib, n).argtypes is not None, n
    body = ('#include <stddef.h>\n#include <stdio.h>\n#include "hsqp_observe.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(hsqp_observe_settings),'
            ' offsetof(hsqp_observe_settings, sensor_delay), offsetof(hsqp_observe_settings, compute_delay), offsetof(hsqp_observe_settings, seed),'
            ' sizeof(hsqp_observe_instance), offsetof(hsqp_observe_instance, bias), offsetof(hsqp_observe_instance, sigma), HSQP_OBS_MAX_DELAY, HSQP_NX,'
            ' HSQP_ABI_VERSION);return 0;}\n')
    S, I = _abi.ObserveSettings, _abi.ObserveInstance
    want = [C.sizeof(S), S.sensor_delay.offset, S.compute_delay.offset, S.seed.offset, C.sizeof(I), I.bias.offset, I.sigma.offset, _abi.OBS_MAX_DELAY, 58, 7]
    assert want[:7] == [16, 0, 4, 8, 2 * 58 * 8, 0, 58 * 8]
    for name, cc, std in (("sz.c", "gcc", "-std=c99"), ("sz.cpp", "g++", "-std=c++17")):      # the header as C and as C++
        (tmp_path / name).write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / name), "-o", str(tmp_path / "sz")])
        assert [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()] == want, cc
    assert _abi.ABI_VERSION == 7 and lib.hsqp_abi_version() == 7


def test_defaults_and_null_handle():
    lib = solver.load_library()
    st = _abi.ObserveSettings()
    st.sensor_delay, st.compute_delay, st.seed = 3, 4, 5
    lib.hsqp_observe_defaults(C.byref(st))
    assert (st.sensor_delay, st.compute_delay, st.seed) == (0, 0, 0)
    e = _abi.ObserveInstance()
    e.bias[7], e.sigma[57] = 1.0, 2.0
    lib.hsqp_observe_instance_defaults(C.byref(e))
    assert not any(e.bias) and not any(e.sigma)
    lib.hsqp_observe_defaults(None)
    lib.hsqp_observe_instance_defaults(None)
    d = np.zeros(NX).ctypes.data_as(_dp)
    bad = _abi.ERR_BAD_ARG
    assert lib.hsqp_observe_set(None, C.byref(st)) == bad
    assert lib.hsqp_observe_set_instances(None, 1, C.byref(e)) == bad
    assert lib.hsqp_observe_set_instances_device(None, 1, C.byref(e)) == bad
    assert lib.hsqp_observe_clear(None) == bad
    assert lib.hsqp_observe_get(None, C.byref(st), 1, C.byref(e)) == bad
    assert lib.hsqp_observe_eval(None, 1, 0, d, d) == bad
    assert lib.hsqp_observe_eval_device(None, 1, 0, d, d) == bad
    assert lib.hsqp_observe_last(None, d, d) == bad
    assert lib.hsqp_observe_last_device(None, d, d) == bad


# ---------------------------------------------------------------------------------------------- the host build of the kernel sources
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    lib_path = tmp_path_factory.mktemp("observe") / "libobserve_emu.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fPIC", "-shared",
                           "-I", CSRC, os.path.join(ROOT, "tests", "observe", "observe_emu.cpp"), "-o", str(lib_path)])
    lib = C.CDLL(str(lib_path))
    lib.obs_philox.argtypes = [_up, _up, _up]
    lib.obs_normals.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, _dp]
    lib.obs_cycle.argtypes = [_oi, C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, C.c_double]
    lib.obs_policy_time.argtypes = [C.c_int, C.c_double]
    lib.obs_policy_time.restype = C.c_double
    lib.obs_problem_time.argtypes = [C.c_double, C.c_double]
    lib.obs_problem_time.restype = C.c_double
    lib.obs_settings_refused.argtypes = [_os]
    lib.obs_entry_error.argtypes = [_oi]
    lib.obs_horizon_ok.argtypes = [C.c_int, C.c_double, C.c_int, C.c_double]
    return lib


def _p(a):
    if a is None:
        return None
    return a.ctypes.data_as({np.dtype(np.int32): _ip, np.dtype(np.uint32): _up}.get(a.dtype, _dp))


def emu_philox(lib, counter, key):
    c, k, out = np.array(counter, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
    lib.obs_philox(_p(c), _p(k), _p(out))
    return out


def emu_normals(lib, seed, b, n):
    z = np.zeros(NX)
    lib.obs_normals(seed, int(b), int(n), _p(z))
    return z


def emu_cycle(lib, table, seed, cycle, delay, x, ring=None, fresh_all=0, mode_b=None, s0=None, s0_value=0.0):
    y = np.full_like(x, np.nan)
    lib.obs_cycle(table, seed, int(cycle), delay, len(x), fresh_all, _p(mode_b), _p(x), _p(ring), _p(y), _p(s0), s0_value)
    return y


# ---------------------------------------------------------------------------------------------- 2. the generator
KNOWN = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
         ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]


def test_philox_known_answers_and_the_restatement(emu, rng):
    for counter, key, want in KNOWN:                                   # the Random123 known-answer vectors
        assert list(emu_philox(emu, counter, key)) == want
        assert list(O.philox4x32_10(np.array(counter), np.array(key))) == want
    counters, keys = rng.integers(0, 2 ** 32, (500, 4), dtype=np.uint64), rng.integers(0, 2 ** 32, (500, 2), dtype=np.uint64)
    counters[:8] = [[0xFFFFFFFF] * 4, [0, 0xFFFFFFFF, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [14, 255, 0xFFFFFFFF, 0], [0x80000000] * 4]
    want = O.philox4x32_10(counters, keys)
    for c, k, w in zip(counters, keys, want):
        assert np.array_equal(emu_philox(emu, c, k), w), (c, k)


# ---------------------------------------------------------------------------------------------- 3. the normals
def test_normals_match_the_restatement(emu, rng):
    """|dz| <= 1e-13: |z| < 6.8 (u >= 2^-33), the library functions are good to a few ulp, and the rounding of 2 pi u moves the angle by at most 9e-16."""
    worst = 0.0
    for seed in (SEED, 0xFEDCBA9876543210):
        bs = np.concatenate([[0, 1, 2, 255, 2 ** 32 - 1], rng.integers(0, 2 ** 20, 15)])
        ns = np.concatenate([[0, 1, 7, 2 ** 32 - 1], rng.integers(0, 2 ** 32, 11)])
        want = O.normals(seed, bs[:, None], ns[None, :])
        assert want.shape == (20, 15, NX) and np.isfinite(want).all() and np.abs(want).max() < 6.8
        for i, b in enumerate(bs):
            for j, n in enumerate(ns):
                worst = max(worst, float(np.abs(emu_normals(emu, seed, b, n) - want[i, j]).max()))
    print(f"normals, host build against numpy over 600 (b, n): max |dz| {worst:.3e}")
    assert worst <= 1e-13
    z = O.normals(SEED, 0, 0)
    assert np.allclose(z[:4], [-1.2845247705728435, -0.18145609956950937, -0.24229194189080355, 0.8049075145184901], rtol=0, atol=1e-13)
    assert abs(O.normals(SEED, 2, 7)[57] - -0.5722673792247618) <= 1e-13
    assert np.abs(emu_normals(emu, SEED, 0, 0)[:4] - [-1.2845247705728435, -0.18145609956950937, -0.24229194189080355, 0.8049075145184901]).max() <= 1e-13
    assert abs(emu_normals(emu, SEED, 2, 7)[57] - -0.5722673792247618) <= 1e-13


# ---------------------------------------------------------------------------------------------- 4. the statistics of the shipped stream
def test_statistics_of_the_stream(emu):
    """Five standard errors each, on the stream the host build of the kernel source gives: seed 2026, b = 0 .. 2, n = 0 .. 4095, all 58 entries."""
    N = 4096
    z = np.zeros((3, N, NX))
    for b in range(3):
        for n in range(N):
            emu.obs_normals(SEED, b, n, z[b, n].ctypes.data_as(_dp))
    assert np.abs(z - O.normals(SEED, np.arange(3)[:, None], np.arange(N)[None, :])).max() <= 1e-13
    mean, var = np.abs(z.mean(axis=1)).max(), np.abs(z.var(axis=1) - 1.0).max()
    corr = np.corrcoef(z.reshape(3 * N, NX), rowvar=False)
    off = np.abs(corr - np.diag(np.diag(corr))).max()
    zc = z - z.mean(axis=1, keepdims=True)
    lag1 = np.abs((zc[:, 1:] * zc[:, :-1]).sum(axis=1) / (zc * zc).sum(axis=1)).max()
    print(f"stream statistics: |mean| {mean:.4f}, |var - 1| {var:.4f}, off-diagonal correlation {off:.4f}, lag-1 autocorrelation {lag1:.4f}")
    assert mean <= 5.0 / np.sqrt(N)
    assert var <= 5.0 * np.sqrt(2.0 / N)
    assert off <= 5.0 / np.sqrt(3 * N)
    assert lag1 <= 5.0 / np.sqrt(N)


# ---------------------------------------------------------------------------------------------- 5. the arithmetic of y
def table_of(bias, sigma):
    return solver.HipSqpSolver.pack_observation(bias, sigma)


def test_y_arithmetic_and_copied_entries(emu, rng):
    B = 5
    x = rng.standard_normal((B, NX)) * 3.0
    bias, sigma = 0.1 * rng.standard_normal((B, NX)), np.abs(0.05 * rng.standard_normal((B, NX)))
    bias[rng.random((B, NX)) < 0.4] = 0.0
    sigma[rng.random((B, NX)) < 0.4] = 0.0
    sigma[1, 8:12] = 0.0                                               # a block that draws nothing, with a bias
    bias[4], sigma[4] = 0.0, 0.0                                       # a neutral instance
    untouched = (bias == 0.0) & (sigma == 0.0)
    assert untouched.sum() > 60 and (~untouched).sum() > 100
    x[untouched & (rng.random((B, NX)) < 0.3)] = -0.0
    nan_bits = np.array([0x7FF8000000000123, 0xFFF800000000BEEF], np.uint64).view(np.float64)   # quiet NaNs with payloads, either sign
    x[4, 3], x[4, 57] = nan_bits
    x[0, np.flatnonzero(untouched[0])[:2]] = nan_bits
    for draw in (0, 7, 2 ** 32 - 1):
        y = emu_cycle(emu, table_of(bias, sigma), SEED, draw, -1, x)
        assert np.array_equal(y.view(np.uint64)[untouched], x.view(np.uint64)[untouched])           # copied: NaN payloads and the sign of zero kept
        z = O.normals(SEED, np.arange(B), draw)
        want = x + (bias + sigma * z)
        bound = 2.0 * np.spacing(np.abs(want)) + sigma * 1e-13
        err = np.abs(y - want)[~untouched]
        print(f"draw {draw}: max |y - numpy| / bound {np.max(err / bound[~untouched]):.3f}")
        assert (err <= bound[~untouched]).all()
        assert np.array_equal(y[1, 8:12], x[1, 8:12] + bias[1, 8:12])                              # no draw: the bias alone
    # no table: every instance is copied
    assert np.array_equal(emu_cycle(emu, None, SEED, 3, -1, x).view(np.uint64), x.view(np.uint64))
    # the stream does not depend on the batch or on the other instances
    y3 = emu_cycle(emu, table_of(bias, sigma), SEED, 7, -1, x)
    y2 = emu_cycle(emu, table_of(bias[:2], sigma[:2]), SEED, 7, -1, x[:2].copy())
    assert np.array_equal(y2.view(np.uint64), y3[:2].view(np.uint64))
    assert not np.array_equal(emu_cycle(emu, table_of(bias, sigma), SEED + 1, 7, -1, x)[~untouched], y3[~untouched])


# ---------------------------------------------------------------------------------------------- 6. the ring and a cycle's bookkeeping
@pytest.mark.parametrize("delays", [(0, 0), (1, 0), (0, 2), (3, 2), (5, 3)])
def test_ring_and_cycle_bookkeeping(emu, rng, delays):
    """No table: copies and indices, so the host build equals the restatement exactly.  Instance 1 starts an episode in cycle 3."""
    sd, cd = delays
    a, B, cycles, P, t0 = sd + cd, 3, max(8, sd + cd + 6), 1.0 / 60.0, 0.25
    ring = np.full((a + 1, B, NX), np.nan) if a else None              # NaN: a read of a slot never written would show
    ref = O.Ring(B, a)
    xs = rng.standard_normal((cycles, B, NX))                          # the plant's state at the start of every cycle
    starts = {b: 0 for b in range(B)}
    s0 = np.full(B, np.nan)
    t = t0
    for c in range(cycles):
        fresh = np.zeros(B, bool)
        if c == 0:
            fresh[:] = True
        if c == 3:
            fresh[1] = True
            starts[1] = 3
        mode = np.where(fresh, _abi.WARM_COLD, _abi.WARM_SHIFT).astype(np.int32)
        args = dict(ring=ring, fresh_all=int(c == 0), mode_b=None if c == 0 else mode, s0=s0, s0_value=emu.obs_policy_time(cd, P))
        y = emu_cycle(emu, None, SEED, c, a, xs[c], **args)
        want = ref.cycle(c, xs[c], fresh)
        assert np.array_equal(y, want), c
        if a:
            assert np.array_equal(ring, ref.slots, equal_nan=True), c
        for b in range(B):                                             # the state at the start of cycle c - a, or the episode's start state
            assert np.array_equal(y[b], xs[max(c - a, starts[b])][b]), (c, b)
        before = None if ring is None else ring.copy()
        again = emu_cycle(emu, None, SEED, c, a, xs[c], **args)         # a repeated cycle writes the same bytes
        assert np.array_equal(again, y) and (ring is None or np.array_equal(ring, before, equal_nan=True))
        assert np.array_equal(s0, np.full(B, O.policy_time(cd, P)))
        assert emu.obs_problem_time(t, emu.obs_policy_time(cd, P)) == O.problem_time(t, cd, P)
        t += P
    assert O.problem_time(t0, 0, P) == t0 and O.policy_time(0, P) == 0.0


def test_noise_rides_on_the_delayed_state(emu, rng):
    """With a table the observation of cycle c is observe(state of cycle c - a, draw = c): the draw index is the cycle in which it is USED."""
    a, B = 2, 3
    bias, sigma = 0.01 * rng.standard_normal((B, NX)), np.full((B, NX), 0.05)
    ring, ref = np.zeros((a + 1, B, NX)), O.Ring(B, a)
    xs = rng.standard_normal((6, B, NX))
    for c in range(6):
        y = emu_cycle(emu, table_of(bias, sigma), SEED, c, a, xs[c], ring=ring, fresh_all=int(c == 0))
        delayed = ref.cycle(c, xs[c], np.full(B, c == 0))
        assert np.array_equal(delayed, xs[max(c - a, 0)])
        assert np.array_equal(y, emu_cycle(emu, table_of(bias, sigma), SEED, c, -1, delayed))
        assert np.abs(y - O.observe(delayed, bias, sigma, SEED, c)).max() <= 1e-14


# ---------------------------------------------------------------------------------------------- 7. the argument checks that need no device
def test_argument_checks(emu):
    def refused(sd, cd):
        st = _abi.ObserveSettings()
        st.sensor_delay, st.compute_delay = sd, cd
        return emu.obs_settings_refused(C.byref(st))
    assert not refused(0, 0) and not refused(8, 0) and not refused(0, 8) and not refused(3, 5)
    assert refused(-1, 0) and refused(0, -1) and refused(9, 0) and refused(4, 5) and refused(2 ** 31 - 1, 2 ** 31 - 1)
    e = _abi.ObserveInstance()
    assert emu.obs_entry_error(C.byref(e)) == 0
    e.bias[5], e.sigma[57] = -3.0, 1e300
    assert emu.obs_entry_error(C.byref(e)) == 0
    for value in (np.nan, np.inf, -np.inf):
        e.bias[9] = value
        assert emu.obs_entry_error(C.byref(e)) == 1 + 9
    e.bias[9] = 0.0
    for value in (np.nan, np.inf, -1e-300, -np.inf):
        e.sigma[31] = value
        assert emu.obs_entry_error(C.byref(e)) == -(1 + 31)
    e.sigma[31] = 0.0
    assert emu.obs_entry_error(C.byref(e)) == 0
    P = 1.0 / 60.0
    assert emu.obs_horizon_ok(0, P, 8, 0.035) and emu.obs_horizon_ok(15, P, 8, 0.035) and not emu.obs_horizon_ok(16, P, 8, 0.035)   # 8 x 0.035 = 0.28 = 16.8 periods
    assert emu.obs_horizon_ok(0, 0.035, 1, 0.035) and not emu.obs_horizon_ok(1, 0.035, 1, 0.035)
    with pytest.raises(ValueError):
        solver.HipSqpSolver.pack_observation(np.zeros((2, NX)), np.zeros((3, NX)))
