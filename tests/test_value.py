"""The Riccati value function (include/hsqp_value.h, csrc/hsqp_value.h) on the CPU: the header, the exported entry points and the binding; the two
float64 references of tests/value_ref.py against each other on the golden fixtures (the yardstick of tests/value_tolerances.py) and against central
differences of the dense KKT optimum; the host build of the kernel source (tests/value/value_emu.cpp) against the numpy mirror, bit for bit, with
canaries round every output; a sanitizer program of its own (tests/value/value_sanitize.cpp)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import value_ref as V
from event_grid_cases import CASES, event_intervals
from value_tolerances import FD_STEP, FD_VALUE_REL, REF_DISCREPANCY_S, REF_DISCREPANCY_s
from wb_humanoid_mpc_amd import _abi, solver
from wb_humanoid_mpc_amd.reference import padded_event_grid, tile_gait

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURES = ("wb_stance_n4", "wb_walk_n8", "cent_walk_n8")
NX, CNX, VF = _abi.NX, _abi.CNX, _abi.VF_SIZE
_dp = C.POINTER(C.c_double)
CANARY = -12345.678


# ---------------------------------------------------------------------------------------------- 1. header, library, binding
def test_header_library_and_binding_agree(tmp_path):
    src = open(os.path.join(ROOT, "include", "hsqp_value.h")).read()
    body = src[src.index("#ifndef HSQP_VALUE_H"):]
    assert sorted(set(re.findall(r"\b(hsqp_[a-z_]+)\s*\(", body))) == sorted(_abi.VALUE_ENTRY_POINTS)
    assert "1/2 (S + S^T)" in src                                   # the header says what it returns
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "wb_humanoid_mpc_amd", "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.VALUE_ENTRY_POINTS:
        assert n in names, n
        assert getattr(lib, n).argtypes is not None, n
    c = tmp_path / "flag.c"
    c.write_text('#include <stdio.h>\n#include "hsqp_value.h"\nint main(void){printf("%d %d %d\\n", HSQP_ITER_VALUE_FUNCTION, HSQP_ABI_VERSION,'
                 ' HSQP_ITER_TAKE_STEP | HSQP_ITER_KKT | HSQP_ITER_LINESEARCH | HSQP_ITER_UNTIL_CONVERGED);return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(tmp_path / "flag")])
    out = [int(v) for v in subprocess.check_output([str(tmp_path / "flag")]).split()]
    assert out == [_abi.ITER_VALUE_FUNCTION, _abi.ABI_VERSION, 15] and _abi.ITER_VALUE_FUNCTION == 16 and _abi.ABI_VERSION == 7   # a bit of its own; the ABI stays


def test_null_handle():
    lib = solver.load_library()
    z = np.zeros(NX * NX)
    p = z.ctypes.data_as(_dp)
    assert lib.hsqp_value_function(None, 0, 0, p, p, p) == _abi.ERR_BAD_ARG
    assert lib.hsqp_value_function_device(None, 0, 0, p, p, p) == _abi.ERR_BAD_ARG
    assert lib.hsqp_evaluate_value_function(None, 1, p, p, p, p, p) == _abi.ERR_BAD_ARG
    assert lib.hsqp_evaluate_value_function_device(None, 1, p, p, p, p, p) == _abi.ERR_BAD_ARG


# ---------------------------------------------------------------------------------------------- 2. the two references
_refs = {}


def references(name, model, cmodel, oracle, coracle):
    """(lq, Hf, gf, nx, (S, s) dense, (S, s) riccati) of a golden fixture: computed once per process, handed out read-only"""
    if name not in _refs:
        cent = name.startswith("cent")
        d = np.load(os.path.join(GOLDEN, name + ".npz"))
        lq, Hf, gf, nx = V.qp_blocks(cmodel if cent else model, coracle if cent else oracle, d["x"], d["u"], d["par"], d["dt"], cent)
        out = (lq, Hf, gf, nx, V.dense_tail_value(lq, Hf, gf, nx), V.riccati_value(lq, Hf, gf, nx))
        for a in out[4] + out[5]:
            a.setflags(write=False)
        _refs[name] = out
    return _refs[name]


@pytest.mark.parametrize("name", FIXTURES)
def test_the_two_references_agree(model, cmodel, oracle, coracle, name):
    lq, Hf, gf, nx, (S1, s1), (S2, s2) = references(name, model, cmodel, oracle, coracle)
    eS, es = V.node_error(S2, s2, S1, s1)
    print(f"{name}: reference discrepancy eS {eS:.3g} es {es:.3g} (constants {REF_DISCREPANCY_S:g} / {REF_DISCREPANCY_s:g})")
    assert eS <= REF_DISCREPANCY_S and es <= REF_DISCREPANCY_s           # the yardstick of value_tolerances.py is not stale
    N = lq["AB"].shape[0]
    assert S1.shape == (N + 1, NX, NX) and np.array_equal(S1[N, :nx, :nx], np.diag(Hf)) and np.array_equal(s1[N, :nx], gf)
    assert not S1[:, nx:].any() and not S1[:, :, nx:].any() and not s1[:, nx:].any()
    for k in range(N + 1):   # a cost-to-go: symmetric, positive semidefinite on the live states
        assert np.abs(S1[k] - S1[k].T).max() <= 10 * REF_DISCREPANCY_S * np.abs(S1[k]).max()
        assert np.linalg.eigvalsh(0.5 * (S1[k] + S1[k].T)[:nx, :nx]).min() >= -10 * REF_DISCREPANCY_S * np.abs(S1[k]).max()


@pytest.mark.parametrize("name", FIXTURES)
def test_central_differences_of_the_dense_optimum(model, cmodel, oracle, coracle, name):
    lq, Hf, gf, nx, (S1, s1), _ = references(name, model, cmodel, oracle, coracle)
    N = lq["AB"].shape[0]
    rng = np.random.default_rng(20261020)
    h = FD_STEP
    for k in sorted({0, N // 2, N - 1}):
        for _ in range(5):
            xi = rng.standard_normal(nx)
            xi /= np.linalg.norm(xi)
            vp, vm, v0 = (V.tail_optimum(lq, Hf, gf, nx, k, a * xi) for a in (h, -h, 0.0))
            quad, lin = (vp + vm - 2.0 * v0) / h ** 2, (vp - vm) / (2.0 * h)
            want_q, want_l = xi @ S1[k, :nx, :nx] @ xi, s1[k, :nx] @ xi
            lim_q = FD_VALUE_REL * (abs(vp) + abs(vm) + 2.0 * abs(v0)) / h ** 2 + REF_DISCREPANCY_S * np.abs(S1[k]).max()
            lim_l = FD_VALUE_REL * (abs(vp) + abs(vm)) / (2.0 * h) + REF_DISCREPANCY_s * np.abs(s1[k]).max()
            assert abs(quad - want_q) <= lim_q, (name, k, quad, want_q, lim_q)
            assert abs(lin - want_l) <= lim_l, (name, k, lin, want_l, lim_l)


# ---------------------------------------------------------------------------------------------- 3. the host build of the kernel source against the mirror
EMU_FLAGS = ["-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I", CSRC]


@pytest.fixture(scope="module")
def vemu(tmp_path_factory):
    lib_path = tmp_path_factory.mktemp("value") / "libvalue_emu.so"
    subprocess.check_call(["g++", "-O2", "-march=x86-64-v3", *EMU_FLAGS, "-fPIC", "-shared", os.path.join(ROOT, "tests", "value", "value_emu.cpp"), "-o", str(lib_path)])
    return load_emu(str(lib_path))


def load_emu(path):
    lib = C.CDLL(path)
    lib.val_record.argtypes = [C.c_int] * 5 + [_dp] * 5
    lib.val_record.restype = None
    lib.val_eval.argtypes = [C.c_int, C.c_int, C.c_double, _dp, C.c_int, C.c_int] + [_dp] * 7
    lib.val_eval.restype = None
    assert lib.val_vf_size() == VF
    return lib


def emu_eval(lib, vf, xbar, dt, dts, cent, sq, xq):
    """The host build over B instances and n queries each, with a canary query in front of and behind the outputs: (dV [B][n], dfdx, dfdxx)."""
    vf, xbar, sq, xq = (np.ascontiguousarray(a, dtype=np.float64) for a in (vf, xbar, sq, xq))
    B, N, n = vf.shape[0], vf.shape[1] - 1, sq.shape[1]
    dts = None if dts is None else np.ascontiguousarray(dts, dtype=np.float64)
    flat = [np.full(B * n + 2, CANARY), np.full((B * n + 2, NX), CANARY), np.full((B * n + 2, NX, NX), CANARY)]
    keep = [a.copy() for a in (vf, xbar, sq, xq)]
    lib.val_eval(B, N, float(dt), None if dts is None else dts.ctypes.data_as(_dp), int(cent), n, vf.ctypes.data_as(_dp), xbar.ctypes.data_as(_dp),
                 sq.ctypes.data_as(_dp), xq.ctypes.data_as(_dp), *[a[1:].ctypes.data_as(_dp) for a in flat])
    for a in flat:
        assert np.all(a[0] == CANARY) and np.all(a[-1] == CANARY)
    for a, b in zip(keep, (vf, xbar, sq, xq)):
        assert np.array_equal(a, b, equal_nan=True)
    return flat[0][1:-1].reshape(B, n), flat[1][1:-1].reshape(B, n, NX), flat[2][1:-1].reshape(B, n, NX, NX)


def random_record(rng, B, N, cent):
    """a record with the magnitudes of a real one (S entries over six orders of magnitude, not symmetric to the last bit); centroidal: NaN in the padding"""
    nc = CNX if cent else NX
    vf = np.zeros((B, N + 1, VF))
    for b in range(B):
        for k in range(N + 1):
            A = rng.standard_normal((NX, NX)) * 10.0 ** rng.uniform(-3, 3, (NX, 1))
            S = A @ A.T
            S += 1e-13 * np.abs(S) * rng.standard_normal((NX, NX))
            vf[b, k, :NX * NX], vf[b, k, NX * NX:] = S.ravel(), 30.0 * rng.standard_normal(NX)
    xbar = rng.standard_normal((B, N + 1, NX))
    if cent:
        Sv = vf[..., :NX * NX].reshape(B, N + 1, NX, NX)
        Sv[:, :, nc:, :], Sv[:, :, :, nc:] = np.nan, np.nan
        vf[..., NX * NX + nc:], xbar[..., nc:] = np.nan, np.nan
    return vf, xbar


def padded_grid(model):
    """an instance's padded event grid with an event inside and a run of zero-length padding intervals in front of the last interval"""
    _, n_nodes, event_nodes, gait, _ = CASES["A_walk"]
    ev = tile_gait(model.gaits[gait], -0.45, 6.0).event_times
    for c in range(600):
        dts, nts, nb = padded_event_grid(0.2 + c / 60.0, n_nodes, 0.035, ev, event_nodes, 1e-4)
        N = len(dts)
        if N - nb >= 2 and len(event_intervals(dts[:nb - 1])) >= 1:
            return np.asarray(dts), nb
    raise AssertionError("no such grid")


@pytest.mark.parametrize("cent", [False, True], ids=["wb", "centroidal"])
def test_host_build_equals_the_mirror_bit_for_bit(model, vemu, cent):
    rng = np.random.default_rng(7 + cent)
    dts, nb = padded_grid(model)
    N, B, dt = len(dts), 2, 0.035
    vf, xbar = random_record(rng, B, N, cent)
    stamps = np.concatenate([[0.0], np.cumsum(dts)])
    zero = event_intervals(dts)
    pad0 = int(zero[zero >= nb - 1][0])                    # the first padding interval
    horizon = stamps[-1]
    for grid in (None, dts):
        t = stamps if grid is not None else dt * np.arange(N + 1)
        sq = np.array([t[3],                               # on a node
                       0.5 * (t[5] + t[6]) if t[6] > t[5] else t[5] + 0.4 * dt,   # mid-interval
                       0.0, t[-1],                         # both ends
                       t[-1] + 0.37, -0.2, 1e300,          # clamped
                       stamps[pad0], stamps[int(zero[0])], # on a zero-length interval of the padded grid: the padding run, the event
                       t[2] + 0.25 * dt, t[7]])
        n = len(sq)
        sqs = np.tile(sq, (B, 1))
        xq = xbar[:, rng.integers(0, N + 1, n)] + 0.05 * rng.standard_normal((B, n, NX))
        if cent:
            xq[..., CNX:] = rng.standard_normal((B, n, NX - CNX))      # the padding of a query state does not count
        xq[1, 4, 7] = np.nan                                            # a NaN query: its outputs alone are not finite
        dV, g, H = emu_eval(vemu, vf, xbar, dt, None if grid is None else np.tile(grid, (B, 1)), cent, sqs, xq)
        for b in range(B):
            mdV, mg, mH = V.evaluate_mirror(vf[b], xbar[b], N, dt, grid, cent, sqs[b], xq[b])
            assert np.array_equal(dV[b], mdV, equal_nan=True) and np.array_equal(g[b], mg, equal_nan=True) and np.array_equal(H[b], mH)
        assert np.isnan(dV[1, 4]) and np.isnan(g[1, 4]).any() and np.isfinite(H).all()
        ok = np.ones((B, n), bool)
        ok[1, 4] = False
        assert np.isfinite(dV[ok]).all() and np.isfinite(g[ok]).all()
        assert np.array_equal(H, H.transpose(0, 1, 3, 2))
        if cent:
            assert not H[..., CNX:, :].any() and not H[..., :, CNX:].any() and not g[ok][:, CNX:].any()
        # on a node: the node's own record, blended with weight 0; at the end: node N; clamped queries: the ends
        S, s, xb = V.record_mirror(vf, xbar, cent)
        exact = 0
        for i in range(n):
            k, a = V.state_segment(N, dt, min(sq[i], 2.0 * N * dt) if grid is None else sq[i], grid)
            if a in (0.0, 1.0):
                assert np.array_equal(H[:, i], S[:, k + int(a)]), i
                exact += 1
        assert exact >= 4 and np.array_equal(H[:, 4], S[:, N]) and np.array_equal(H[:, 6], S[:, N]) and np.array_equal(H[:, 5], H[:, 2])
        if grid is not None:   # on the zero-length intervals the post-event node is taken, never a blend across the jump
            k_pad, k_ev = V.state_segment(N, dt, stamps[pad0], dts), V.state_segment(N, dt, stamps[int(zero[0])], dts)
            assert dts[k_pad[0]] > 0.0 and k_pad == (N - 1, 0.0) and dts[k_ev[0]] > 0.0 and k_ev == (int(zero[0]) + 1, 0.0)
            assert np.array_equal(H[:, 7], S[:, N - 1]) and np.array_equal(H[:, 8], S[:, int(zero[0]) + 1])
    # the record entry point through the same source
    Sg, sg, xg = (np.full((B + 2, 3, NX, NX), CANARY), np.full((B + 2, 3, NX), CANARY), np.full((B + 2, 3, NX), CANARY))
    vemu.val_record(B, N, 2, 4, int(cent), vf.ctypes.data_as(_dp), xbar.ctypes.data_as(_dp), Sg[1:].ctypes.data_as(_dp), sg[1:].ctypes.data_as(_dp), xg[1:].ctypes.data_as(_dp))
    for a in (Sg, sg, xg):
        assert np.all(a[[0, -1]] == CANARY)
    assert np.array_equal(Sg[1:-1], S[:, 2:5]) and np.array_equal(sg[1:-1], s[:, 2:5]) and np.array_equal(xg[1:-1], xbar[:, 2:5], equal_nan=True)


def test_the_quadratic_model_is_what_the_outputs_say(vemu):
    """dfdx and dV against plain numpy on a mid-interval query (not bit for bit: the order of the sums differs), and dV as the integral of dfdx"""
    rng = np.random.default_rng(3)
    N, dt = 6, 0.02
    vf, xbar = random_record(rng, 1, N, False)
    sq = np.array([[0.047]])
    xq = xbar[:, 2:3] + 0.1 * rng.standard_normal((1, 1, NX))
    dV, g, H = emu_eval(vemu, vf, xbar, dt, None, False, sq, xq)
    k, a = V.state_segment(N, dt, 0.047)
    assert k == 2 and 0.3 < a < 0.4
    S, s, _ = V.record_mirror(vf, xbar, False)
    Sb, sb, xb = (1 - a) * S[0, k] + a * S[0, k + 1], (1 - a) * s[0, k] + a * s[0, k + 1], (1 - a) * xbar[0, k] + a * xbar[0, k + 1]
    dx = xq[0, 0] - xb
    terms = np.abs(Sb) @ np.abs(dx) + np.abs(sb)
    assert np.all(np.abs(g[0, 0] - (sb + Sb @ dx)) <= 1e-14 * terms) and np.abs(H[0, 0] - Sb).max() <= 1e-15 * np.abs(Sb).max()
    assert abs(dV[0, 0] - (sb @ dx + 0.5 * dx @ Sb @ dx)) <= 1e-14 * (np.abs(dx) @ terms)
    g0 = emu_eval(vemu, vf, xbar, dt, None, False, sq, xb[None, None])[1][0, 0]
    assert abs(dV[0, 0] - 0.5 * (g0 + g[0, 0]) @ dx) <= 1e-13 * (np.abs(dx) @ terms)    # a quadratic: the trapezoid rule is exact


# ---------------------------------------------------------------------------------------------- 4. sanitizers: a program of its own
def test_adversarial_queries_under_sanitizers(tmp_path):
    exe = tmp_path / "value_sanitize"
    subprocess.check_call(["g++", "-O1", "-g", *EMU_FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "value", "value_emu.cpp"),
                           os.path.join(ROOT, "tests", "value", "value_sanitize.cpp"), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True)
    assert out.strip() == "value ok"
