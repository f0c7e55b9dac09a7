"""The velocity-command targets and the resident closed loop (include/hsqp_loop.h, csrc/hsqp_loop.h) on the CPU: the header, the exported entry
points and the binding's struct, the host build of the generator's source (tests/loop/loop_emu.cpp) against the fixtures recorded from the
reference-compiled generator (tests/golden/ref_terms.npz, keys tgt.*) and against the numpy mirror (reference.velocity_command_targets)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from wb_humanoid_mpc_amd import _abi, solver
from wb_humanoid_mpc_amd.reference import velocity_command_targets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
G = np.load(os.path.join(ROOT, "tests", "golden", "ref_terms.npz"))
NX, NJ = _abi.NX, _abi.NJ
_dp = C.POINTER(C.c_double)


def _header_functions():
    src = open(os.path.join(ROOT, "include", "hsqp_loop.h")).read()
    src = src[src.index("#ifndef HSQP_LOOP_H"):]   # (the leading comment names entry points of other headers)
    return sorted(set(re.findall(r"\b(hsqp_[a-z_]+)\s*\(", src)))


def test_header_library_and_binding_agree(tmp_path):
    """test_abi.py's method for the new header: every declared entry point is exported by the library and declared by the binding, the struct
    has the size the C compiler gives it, and the older headers' revision is untouched (additions only)."""
    assert _header_functions() == sorted(_abi.LOOP_ENTRY_POINTS)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "wb_humanoid_mpc_amd", "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.LOOP_ENTRY_POINTS:
        assert n in names, n
        assert getattr(lib, n).argtypes is not None, n     # the binding declares the argument types of each
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "hsqp_loop.h"\nint main(void){printf("%zu %zu %d %d %d\\n", sizeof(hsqp_loop_settings), sizeof(hsqp_rollout_settings),'
                   ' HSQP_CMD_N, HSQP_CMD_KNOTS, HSQP_ABI_VERSION);return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    out = [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()]
    assert out == [C.sizeof(_abi.LoopSettings), C.sizeof(_abi.RolloutSettings), _abi.CMD_N, _abi.CMD_KNOTS, 7]
    assert _abi.ABI_VERSION == 7


def test_loop_defaults_follow_task_info(model):
    lib = solver.load_library()
    st = _abi.LoopSettings()
    lib.hsqp_loop_defaults(None, C.byref(st))
    assert st.period == 1.0 / 60.0 and st.filter_alpha == 0.8          # mpcDesiredFrequency 60; the generator's filter constant
    assert st.dt == model.sqp["dt"] and st.n_nodes == 100               # the exported model's sqp dt
    assert (st.iterations, st.iterate_flags, st.arm_swing, st.terrain_height) == (1, 1 | 4, 1, 0.0)
    ro = _abi.RolloutSettings()
    lib.hsqp_rollout_defaults(C.byref(ro))
    assert bytes(st.rollout) == bytes(ro)
    from wb_humanoid_mpc_amd.reference import swing_config
    assert bytes(st.swing) == bytes(swing_config(model))              # the exported model's swing_trajectory_config


def test_null_handle_is_a_bad_argument():
    lib = solver.load_library()
    z = np.zeros(3 * NX)
    p = z.ctypes.data_as(_dp)
    st = _abi.LoopSettings()
    i = np.ones(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.hsqp_set_default_joint_state(None, p) == _abi.ERR_BAD_ARG
    assert lib.hsqp_command_targets(None, 1, p, p, 0.0, p, 0.0, 1.0, p, p) == _abi.ERR_BAD_ARG
    assert lib.hsqp_command_targets_device(None, 1, p, p, 0.0, p, 0.0, 1.0, p, p) == _abi.ERR_BAD_ARG
    assert lib.hsqp_loop_start(None, C.byref(st), 1, 0.0, p, p, 1, i, p, i) == _abi.ERR_BAD_ARG
    done = C.c_int(7)
    assert lib.hsqp_loop_run(None, 1, None, None, C.byref(done)) == _abi.ERR_BAD_ARG and done.value == 0
    for f in (lib.hsqp_loop_command, lib.hsqp_loop_command_device):
        assert f(None, p) == _abi.ERR_BAD_ARG
    for f in (lib.hsqp_loop_state, lib.hsqp_loop_state_device):
        assert f(None, None, None, None) == _abi.ERR_BAD_ARG


def test_binding_raises_no_device_without_a_gpu(model):
    if solver.load_library().hsqp_device_count() > 0:
        pytest.skip("a GPU is visible: the binding is exercised by tests/test_gpu_loop.py")
    with pytest.raises(solver.HsqpError) as ei:
        solver.HipSqpSolver(model, max_nodes=8, max_batch=1).command_targets((0.3, 0.0, 0.79, 0.0), model.initial_state, 0.0, 1.0)
    assert ei.value.code == _abi.ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------- host build of the generator's source
@pytest.fixture(scope="module")
def lemu(tmp_path_factory):
    lib_path = tmp_path_factory.mktemp("loop") / "libloop_emu.so"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-march=x86-64-v3", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-fPIC", "-shared",
                           "-I", CSRC, os.path.join(ROOT, "tests", "loop", "loop_emu.cpp"), "-o", str(lib_path)])
    lib = C.CDLL(str(lib_path))
    lib.lp_command_targets.argtypes = [_dp, C.c_double, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, _dp, _dp]
    lib.lp_command_targets.restype = None
    return lib


def emu_targets(lemu, model, v_cmd, v_filt, alpha, x0, t0, horizon):
    """(times [B][3], states [B][3][58], v_filt after [B][4]) from the host build"""
    x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=float)
    B = x0.shape[0]
    v_cmd = np.ascontiguousarray(np.broadcast_to(v_cmd, (B, 4)), dtype=float)
    vf = np.array(np.broadcast_to(v_filt, (B, 4)), dtype=float)
    jt = np.ascontiguousarray(model.default_joint_state, dtype=float)
    tt, ts = np.full((B, 3), np.nan), np.full((B, 3, NX), np.nan)
    lemu.lp_command_targets(jt.ctypes.data_as(_dp), alpha, B, v_cmd.ctypes.data_as(_dp), vf.ctypes.data_as(_dp), x0.ctypes.data_as(_dp), t0, horizon,
                            tt.ctypes.data_as(_dp), ts.ctypes.data_as(_dp))
    return tt, ts, vf


def test_host_build_equals_the_reference_compiled_generator(lemu, model):
    """alpha = 0 on the six recorded cases, within the bound tests/test_ref_terms.py sets for the host mirror (rtol 1e-15 on times, atol 1e-14 on
    states); the filter state a garbage value, which alpha = 0 must ignore."""
    for c, x0, h, t0, tt, ts in zip(G["tgt.cmd"], G["tgt.x0"], G["tgt.horizon"], G["tgt.t0"], G["tgt.times"], G["tgt.states"]):
        got_t, got_s, vf = emu_targets(lemu, model, c, np.full(4, np.nan), 0.0, x0, float(t0), float(h))
        np.testing.assert_allclose(got_t[0], tt, rtol=1e-15, atol=0)
        np.testing.assert_allclose(got_s[0], ts, rtol=0, atol=1e-14)
        assert np.array_equal(vf[0], c)


def test_host_build_reproduces_the_first_call_transient(lemu, model):
    """alpha = 0.8, one call from where the 200 calls of the last recorded case left the reference's (static) filter, the new command
    (5, 0, 0.7925, 0): tgt.first_call_states, the way tests/golden/make_ref_terms_golden.py recorded it."""
    _, got_s, vf = emu_targets(lemu, model, (5.0, 0.0, 0.7925, 0.0), G["tgt.cmd"][-1], 0.8, model.initial_state, 0.0, 2.0)
    np.testing.assert_allclose(got_s[0], G["tgt.first_call_states"], rtol=0, atol=1e-14)
    np.testing.assert_allclose(vf[0], 0.8 * G["tgt.cmd"][-1] + 0.2 * np.array([5.0, 0.0, 0.7925, 0.0]), rtol=0, atol=1e-15)


def test_mirror_default_is_unchanged_and_filters_on_request(model):
    c, x0 = (0.4, -0.1, 0.78, 0.2), model.initial_state
    a = velocity_command_targets(model, c, 0.5, x0, 1.5)
    b = velocity_command_targets(model, c, 0.5, x0, 1.5, filter_alpha=0.0, v_filt=None)
    assert np.array_equal(np.asarray(a.states), np.asarray(b.states)) and np.array_equal(np.asarray(a.times), np.asarray(b.times))
    vf = np.array([0.1, 0.0, 0.8, 0.0])
    f = velocity_command_targets(model, c, 0.5, x0, 1.5, filter_alpha=0.8, v_filt=vf)
    want = 0.8 * np.array([0.1, 0.0, 0.8, 0.0]) + (1.0 - 0.8) * np.array(c)
    assert np.array_equal(vf, want)
    g = velocity_command_targets(model, tuple(want), 0.5, x0, 1.5)
    assert np.array_equal(np.asarray(f.states), np.asarray(g.states))


def test_filter_recursion_over_20_calls_equals_the_mirror(lemu, model):
    """Twenty calls with a command that changes every five, a state that moves, alpha = 0.8, four instances with their own filter states: the
    host build and the numpy mirror agree on the filter states bit for bit (the same IEEE operations) and on the knots to the fixtures' bound."""
    rng = np.random.default_rng(20260116)
    B = 4
    x0 = np.tile(model.initial_state, (B, 1))
    vf_emu = rng.uniform(-0.3, 0.3, (B, 4))
    vf_emu[:, 2] = 0.79
    vf_np = vf_emu.copy()
    cmd = None
    for call in range(20):
        if call % 5 == 0:
            cmd = np.column_stack([rng.uniform(-0.5, 0.8, B), rng.uniform(-0.2, 0.2, B), rng.uniform(0.7, 0.8, B), rng.uniform(-0.4, 0.4, B)])
        x0[:, :6] += 0.01 * rng.standard_normal((B, 6))
        x0[:, 6 + NJ:12 + NJ] = 0.1 * rng.standard_normal((B, 6))
        t0 = call / 60.0
        tt, ts, vf_emu = emu_targets(lemu, model, cmd, vf_emu, 0.8, x0, t0, 1.1)
        for b in range(B):
            ref = velocity_command_targets(model, tuple(cmd[b]), t0, x0[b], 1.1, filter_alpha=0.8, v_filt=vf_np[b])
            np.testing.assert_allclose(tt[b], np.asarray(ref.times), rtol=1e-15, atol=0)
            np.testing.assert_allclose(ts[b], np.asarray(ref.states), rtol=0, atol=1e-14)
        assert np.array_equal(vf_emu, vf_np), call
