"""The centroidal velocity-command targets and the centroidal resident loop (include/hsqp_cent_loop.h, csrc/hsqp_cent_loop.h) on the CPU: the header,
the exported entry points and the binding; the host build of the generator's source (tests/cent_loop/cent_loop_emu.cpp) against the numpy mirror
(reference.centroidal_velocity_command_targets, reference.centroidal_base_velocity); the mirror's default; the sanitizer program.

Bounds: times rtol 1e-15; states and base velocity 1e-12 absolute — the bound tests/test_device_params.py sets for the centroidal node table, whose torso
velocity goes through the same solve; the knots multiply the base velocity by at most 0.35 horizon = 0.7.  The filter state has no transcendental: bit-equal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from wb_humanoid_mpc_amd import _abi, solver
from wb_humanoid_mpc_amd.reference import centroidal_base_velocity, centroidal_velocity_command_targets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
HERE = os.path.join(ROOT, "tests", "cent_loop")
NX, NJ, CNX = _abi.NX, _abi.NJ, _abi.CNX
SEED = 20261020
_dp = C.POINTER(C.c_double)
_p = lambda a: a.ctypes.data_as(_dp)  # noqa: E731
GXX = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I", CSRC]


def _header_functions():
    src = open(os.path.join(ROOT, "include", "hsqp_cent_loop.h")).read()
    src = src[src.index("#ifndef HSQP_CENT_LOOP_H"):]
    return sorted(set(re.findall(r"\b(hsqp_[a-z_]+)\s*\(", src)))


# ---------------------------------------------------------------------------------------------- 1. ABI
def test_header_library_and_binding_agree(tmp_path):
    assert _header_functions() == sorted(_abi.CENT_LOOP_ENTRY_POINTS)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "wb_humanoid_mpc_amd", "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    lib = solver.load_library()
    for n in _abi.CENT_LOOP_ENTRY_POINTS:
        assert n in names, n
        assert getattr(lib, n).argtypes is not None, n
    body = '#include <stdio.h>\n#include "hsqp_cent_loop.h"\nint main(void){printf("%zu %d\\n", sizeof(hsqp_loop_settings), HSQP_ABI_VERSION);return 0;}\n'
    for name, cc, std in (("sz.c", "gcc", "-std=c99"), ("sz.cpp", "g++", "-std=c++17")):      # the header as C and as C++
        (tmp_path / name).write_text(body)
        subprocess.check_call([cc, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / name), "-o", str(tmp_path / "sz")])
        out = [int(v) for v in subprocess.check_output([str(tmp_path / "sz")]).split()]
        assert out == [C.sizeof(_abi.LoopSettings), _abi.ABI_VERSION]
    assert _abi.ABI_VERSION == 7                                                             # additions only


def test_null_handle_is_a_bad_argument():
    lib = solver.load_library()
    z = np.zeros(3 * NX)
    p = _p(z)
    st = _abi.LoopSettings()
    i = np.ones(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.hsqp_centroidal_command_targets(None, 1, p, p, 0.0, p, 0.0, 1.0, p, p, None) == _abi.ERR_BAD_ARG
    assert lib.hsqp_centroidal_command_targets_device(None, 1, p, p, 0.0, p, 0.0, 1.0, p, p, p) == _abi.ERR_BAD_ARG
    assert lib.hsqp_loop_start_centroidal(None, C.byref(st), 1, 0.0, p, p, 1, i, p, i) == _abi.ERR_BAD_ARG


def test_binding_raises_no_device_without_a_gpu(cmodel):
    if solver.load_library().hsqp_device_count() > 0:
        pytest.skip("a GPU is visible: the binding is exercised by tests/test_gpu_cent_loop.py")
    with pytest.raises(solver.HsqpError) as ei:
        x0 = np.zeros(NX)
        x0[:CNX] = cmodel.initial_state
        solver.HipSqpSolver(cmodel, max_nodes=8, max_batch=1).command_targets((0.3, 0.0, 0.79, 0.0), x0, 0.0, 1.0)
    assert ei.value.code == _abi.ERR_NO_DEVICE


def test_the_other_headers_point_here():
    for name in ("hsqp_loop.h", "hsqp_episode.h"):
        assert "include/hsqp_cent_loop.h" in open(os.path.join(ROOT, "include", name)).read(), name


# ---------------------------------------------------------------------------------------------- 2. host build of the generator's source
class Emu:
    def __init__(self, path, cmodel):
        subprocess.check_call(GXX + ["-O2", "-march=x86-64-v3", "-fPIC", "-shared", os.path.join(HERE, "cent_loop_emu.cpp"), "-o", str(path)])
        lib = self.lib = C.CDLL(str(path))
        lib.cl_create.restype = C.c_void_p
        lib.cl_create.argtypes = [C.c_void_p, _dp, C.c_char_p, C.c_int]
        lib.cl_destroy.argtypes = [C.c_void_p]
        lib.cl_total_mass.restype = C.c_double
        lib.cl_total_mass.argtypes = [C.c_void_p]
        lib.cl_command_targets.restype = None
        lib.cl_command_targets.argtypes = [C.c_void_p, C.c_double, C.c_int, _dp, _dp, _dp, C.c_double, C.c_double, _dp, _dp, _dp]
        err = C.create_string_buffer(256)
        h = lib.cl_create(C.byref(cmodel.desc), _p(np.ascontiguousarray(cmodel.default_joint_state, dtype=float)), err, 256)
        assert h, err.value
        self.h = C.c_void_p(h)

    def targets(self, v_cmd, v_filt, alpha, x0, t0, horizon):
        """(times [B][3], states [B][3][58], v_filt after [B][4], base_vel [B][6])"""
        x0 = np.ascontiguousarray(np.atleast_2d(x0), dtype=float)
        B = x0.shape[0]
        v_cmd = np.ascontiguousarray(np.broadcast_to(v_cmd, (B, 4)), dtype=float)
        vf = np.array(np.broadcast_to(v_filt, (B, 4)), dtype=float)
        tt, ts, bv = np.full((B, 3), np.nan), np.full((B, 3, NX), np.nan), np.full((B, 6), np.nan)
        self.lib.cl_command_targets(self.h, alpha, B, _p(v_cmd), _p(vf), _p(x0), t0, horizon, _p(tt), _p(ts), _p(bv))
        return tt, ts, vf, bv


@pytest.fixture(scope="module")
def emu(tmp_path_factory, cmodel):
    return Emu(tmp_path_factory.mktemp("cent_loop") / "libcent_loop_emu.so", cmodel)


def random_cases(cmodel, n=32, seed=SEED):
    """[(alpha, t0, horizon, v_cmd [4], v_filt [4], x0 [58])]: joints at the default +- 0.05, yaw +-1.2, roll and pitch +-0.1, momentum +-0.3, horizon 2.0,
    alpha in {0, 0.8}"""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(n):
        x0 = np.zeros(NX)
        x0[:6] = rng.uniform(-0.3, 0.3, 6)
        x0[6:9] = (rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), rng.uniform(0.7, 0.85))
        x0[9] = rng.uniform(-1.2, 1.2)
        x0[10:12] = rng.uniform(-0.1, 0.1, 2)
        x0[12:CNX] = cmodel.default_joint_state + rng.uniform(-0.05, 0.05, NJ)
        v_cmd = np.array([rng.uniform(-0.5, 0.8), rng.uniform(-0.2, 0.2), rng.uniform(0.7, 0.8), rng.uniform(-0.4, 0.4)])
        v_filt = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.1, 0.1), 0.79, rng.uniform(-0.2, 0.2)])
        out.append((0.8 if c % 2 else 0.0, float(rng.uniform(0.0, 3.0)), 2.0, v_cmd, v_filt, x0))
    return out


def mirror(cmodel, alpha, t0, horizon, v_cmd, v_filt, x0):
    """(times [3], states [3][58], v_filt after [4], base_vel [6]) from the numpy mirror"""
    vf = v_filt.copy()
    tg = centroidal_velocity_command_targets(cmodel, tuple(v_cmd), t0, x0[:CNX], horizon, filter_alpha=alpha, v_filt=vf)
    st = np.zeros((3, NX))
    st[:, :CNX] = np.asarray(tg.states)
    return np.asarray(tg.times), st, vf, centroidal_base_velocity(cmodel, x0[6:CNX], x0[:6])


def test_host_build_against_the_mirror(emu, cmodel):
    assert emu.lib.cl_total_mass(emu.h) == cmodel.total_mass
    worst = 0.0
    for alpha, t0, horizon, v_cmd, v_filt, x0 in random_cases(cmodel):
        tt, ts, vf, bv = emu.targets(v_cmd, v_filt, alpha, x0, t0, horizon)
        wt, ws, wvf, wbv = mirror(cmodel, alpha, t0, horizon, v_cmd, v_filt, x0)
        worst = max(worst, np.abs(ts[0] - ws).max(), np.abs(bv[0] - wbv).max())
        np.testing.assert_allclose(tt[0], wt, rtol=1e-15, atol=0)
        np.testing.assert_allclose(ts[0], ws, rtol=0, atol=1e-12)
        np.testing.assert_allclose(bv[0], wbv, rtol=0, atol=1e-12)
        assert np.array_equal(vf[0], wvf)
    print(f"host build against the mirror: worst absolute difference {worst:.3e}")


def test_filter_recursion_over_20_calls_equals_the_mirror(emu, cmodel):
    rng = np.random.default_rng(SEED + 1)
    B = 4
    x0 = np.stack([c[5] for c in random_cases(cmodel, B, SEED + 2)])
    vf_emu = rng.uniform(-0.3, 0.3, (B, 4))
    vf_emu[:, 2] = 0.79
    vf_np = vf_emu.copy()
    cmd = None
    for call in range(20):
        if call % 5 == 0:
            cmd = np.column_stack([rng.uniform(-0.5, 0.8, B), rng.uniform(-0.2, 0.2, B), rng.uniform(0.7, 0.8, B), rng.uniform(-0.4, 0.4, B)])
        x0[:, 6:8] += 0.01 * rng.standard_normal((B, 2))
        x0[:, :6] = 0.1 * rng.standard_normal((B, 6))
        t0 = call / 60.0
        tt, ts, vf_emu, _ = emu.targets(cmd, vf_emu, 0.8, x0, t0, 1.1)
        for b in range(B):
            wt, ws, _, _ = mirror(cmodel, 0.8, t0, 1.1, cmd[b], vf_np[b], x0[b])
            vf_np[b] = 0.8 * vf_np[b] + (1.0 - 0.8) * cmd[b]
            np.testing.assert_allclose(tt[b], wt, rtol=1e-15, atol=0)
            np.testing.assert_allclose(ts[b], ws, rtol=0, atol=1e-12)
        assert np.array_equal(vf_emu, vf_np), call


def test_mirror_default_is_unchanged_and_filters_on_request(cmodel):
    c, x0 = (0.4, -0.1, 0.78, 0.2), random_cases(cmodel, 1)[0][5][:CNX]
    a = centroidal_velocity_command_targets(cmodel, c, 0.5, x0, 1.5)
    b = centroidal_velocity_command_targets(cmodel, c, 0.5, x0, 1.5, filter_alpha=0.0, v_filt=None)
    assert np.array_equal(np.asarray(a.states), np.asarray(b.states)) and np.array_equal(np.asarray(a.times), np.asarray(b.times))
    # the default call restated from the mirror's parts: what it computed before the keyword arguments
    vb = centroidal_base_velocity(cmodel, x0[6:CNX], x0[:6])
    yaw = x0[9]
    gvx, gvy = np.cos(yaw) * c[0] - np.sin(yaw) * c[1], np.sin(yaw) * c[0] + np.cos(yaw) * c[1]
    mid = np.array([x0[6] + (vb[0] + gvx) / 2 * (0.7 * 1.5), x0[7] + (vb[1] + gvy) / 2 * (0.7 * 1.5), c[2], yaw + (vb[5] + c[3]) / 2 * (0.7 * 1.5), 0.0, 0.0])
    np.testing.assert_allclose(np.asarray(a.states)[1][6:12], mid, rtol=0, atol=1e-15)
    assert np.asarray(a.states)[1][5] == c[3] / cmodel.total_mass
    vf = np.array([0.1, 0.0, 0.8, 0.0])
    f = centroidal_velocity_command_targets(cmodel, c, 0.5, x0, 1.5, filter_alpha=0.8, v_filt=vf)
    want = 0.8 * np.array([0.1, 0.0, 0.8, 0.0]) + (1.0 - 0.8) * np.array(c)
    assert np.array_equal(vf, want)
    g = centroidal_velocity_command_targets(cmodel, tuple(want), 0.5, x0, 1.5)
    assert np.array_equal(np.asarray(f.states), np.asarray(g.states))


def test_padding_and_the_first_knot(emu, cmodel):
    cases = random_cases(cmodel, 8, SEED + 3)
    x0 = np.stack([c[5] for c in cases])
    v_cmd = np.stack([c[3] for c in cases])
    tt, ts, vf, bv = emu.targets(v_cmd, v_cmd, 0.0, x0, 0.5, 2.0)
    assert np.all(ts[:, :, CNX:] == 0.0)                                  # the padding of every knot
    assert np.all(ts[:, :, 10:12] == 0.0)                                 # roll and pitch of every knot
    assert np.array_equal(ts[:, 0, 8], v_cmd[:, 2]) and np.array_equal(ts[:, 0, 6:8], x0[:, 6:8]) and np.array_equal(ts[:, 0, 9], x0[:, 9])
    assert np.array_equal(ts[:, :, 12:CNX], np.broadcast_to(cmodel.default_joint_state, (8, 3, NJ)))
    assert np.array_equal(tt, np.broadcast_to([0.5, 0.5 + 0.7 * 2.0, 2.5], (8, 3)))
    # an instance's result does not depend on its place in the batch
    for b in range(8):
        t1, s1, _, b1 = emu.targets(v_cmd[b], v_cmd[b], 0.0, x0[b], 0.5, 2.0)
        assert np.array_equal(s1[0], ts[b]) and np.array_equal(b1[0], bv[b])


# ---------------------------------------------------------------------------------------------- 3. sanitizers: a program of its own
def test_the_generator_under_sanitizers(tmp_path, cmodel):
    exe, desc, cases = tmp_path / "cent_loop_sanitize", tmp_path / "desc.bin", tmp_path / "cases.bin"
    subprocess.check_call(GXX + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "cent_loop_emu.cpp"),
                                 os.path.join(HERE, "cent_loop_sanitize.cpp"), "-o", str(exe)])
    desc.write_bytes(bytes(cmodel.desc))
    rows = [np.asarray(cmodel.default_joint_state, dtype=float), np.array([32.0])]
    for alpha, t0, horizon, v_cmd, v_filt, x0 in random_cases(cmodel):
        wt, ws, wvf, wbv = mirror(cmodel, alpha, t0, horizon, v_cmd, v_filt, x0)
        rows += [np.array([alpha, t0, horizon]), v_cmd, v_filt, x0, wt, ws.ravel(), wbv, wvf]
    cases.write_bytes(np.concatenate(rows).astype(np.float64).tobytes())
    out = subprocess.check_output([str(exe), str(desc), str(cases)], text=True)
    assert out.startswith("cent loop ok"), out
