"""The Riccati feedback policy (include/hsqp_feedback.h, csrc/hsqp_feedback.h) on the CPU: the header and the exported entry points, the host
build of the kernel's node logic (tests/feedback/feedback_emu.cpp) against numpy on random records with event intervals and both
formulations' padding, the numpy restatements the GPU tests rely on, and the adaptor built with useFeedbackPolicy = true."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from wb_humanoid_mpc_amd import _abi, solver
from wb_humanoid_mpc_amd.reference import feedback_gains, feedback_source_nodes, linear_controller_input, policy_input_segment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "wb_humanoid_mpc_amd", "csrc")
LIBDIR = os.path.join(ROOT, "wb_humanoid_mpc_amd")
NX, NU, NUT, CNX = _abi.NX, _abi.NU, 23, _abi.CNX
# the QP / Riccati record layout (csrc/hsqp_project.h, csrc/hsqp_riccati.h) the tests read raw debug blocks 101 / 102 with
LAYOUT = dict(QP_SIZE=12936, QP_PX=10064, QP_PU=12094, QP_NUT=12934, RIC_SIZE=1360, RIC_K=0)
ENTRY_POINTS = ("hsqp_feedback_policy", "hsqp_feedback_policy_device", "hsqp_evaluate_feedback_policy")


def test_header_compiles_and_the_library_exports_the_entry_points(tmp_path):
    src = tmp_path / "f.c"
    src.write_text('#include <stdio.h>\n#include "hsqp_feedback.h"\n'
                   'int main(void){ int (*a)(hsqp_handle*, int, int, double*, double*) = hsqp_feedback_policy;\n'
                   ' int (*b)(hsqp_handle*, int, int, double*, double*) = hsqp_feedback_policy_device;\n'
                   ' int (*c)(hsqp_handle*, const double*, const double*, double*, double*, double*) = hsqp_evaluate_feedback_policy;\n'
                   ' printf("%d %d\\n", HSQP_ABI_VERSION, a != 0 && b != 0 && c != 0); return 0; }\n')
    obj = tmp_path / "f.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(obj)])
    syms = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(LIBDIR, "libhsqp_hip.so")], text=True)
    names = {line.split()[-1] for line in syms.splitlines() if line.strip()}
    assert all(n in names for n in ENTRY_POINTS)
    lib = solver.load_library()
    # a NULL handle is a bad argument, with or without a device
    z = np.zeros(4 * NU * NX)
    dp = z.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.hsqp_feedback_policy(None, 0, 1, dp, dp) == _abi.ERR_BAD_ARG
    assert lib.hsqp_feedback_policy_device(None, 0, 1, dp, dp) == _abi.ERR_BAD_ARG
    assert lib.hsqp_evaluate_feedback_policy(None, dp, dp, dp, dp, dp) == _abi.ERR_BAD_ARG
    assert _abi.ABI_VERSION == 7           # additions only: no revision bump


def test_binding_raises_no_device_without_a_gpu(model):
    if solver.load_library().hsqp_device_count() > 0:
        pytest.skip("a GPU is visible: the binding is exercised by tests/test_gpu_feedback_policy.py")
    with pytest.raises(solver.HsqpError) as ei:
        solver.HipSqpSolver(model, max_nodes=8, max_batch=1).feedback_policy()
    assert ei.value.code == _abi.ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------- host build of the node logic
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fb") / "feedback_emu"
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-march=x86-64-v3", "-Wall", "-Wno-unknown-pragmas", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "feedback", "feedback_emu.cpp"), "-o", str(exe)])
    layout = [int(v) for v in subprocess.check_output([str(exe), "--layout"]).split()]
    layout = dict(zip(("QP_SIZE", "QP_PX", "QP_PU", "QP_NUT", "RIC_SIZE", "RIC_K"), layout))
    assert layout == LAYOUT
    return exe, layout


def random_records(rng, L, N, cent, nuts):
    """Random QP / Riccati records with NaN wherever the policy must not read: the padded projected inputs, the centroidal padding states,
    and every other region of the records."""
    qp = np.full((N, L["QP_SIZE"]), np.nan)
    ric = np.full((N, L["RIC_SIZE"]), np.nan)
    nc = CNX if cent else NX
    Px, Pu, Kt = np.full((N, NU, NX), np.nan), np.full((N, NU, NUT), np.nan), np.full((N, NUT, NX), np.nan)
    for k in range(N):
        nut = nuts[k]
        Px[k][:, :nc] = rng.standard_normal((NU, nc))
        Pu[k][:, :nut] = rng.standard_normal((NU, nut))
        Kt[k][:nut, :nc] = rng.standard_normal((nut, nc))
        qp[k, L["QP_PX"]:L["QP_PX"] + NU * NX] = Px[k].ravel()
        qp[k, L["QP_PU"]:L["QP_PU"] + NU * NUT] = Pu[k].ravel()
        qp[k, L["QP_NUT"]] = nut
        ric[k, L["RIC_K"]:L["RIC_K"] + NUT * NX] = Kt[k].ravel()
    x = np.full((N + 1, NX), np.nan)
    x[:, :nc] = rng.standard_normal((N + 1, nc))
    u = rng.standard_normal((N, NU))
    return qp, ric, x, u, Px, Pu, Kt


def run_emu(emu, tmp_path, dts, qp, ric, x, u, cent):
    exe, _ = emu
    N = len(dts)
    parts = [np.array([N, int(cent)], dtype=np.int32).tobytes()] + [np.ascontiguousarray(a, dtype=float).tobytes() for a in (dts, qp, ric, x, u)]
    (tmp_path / "in.bin").write_bytes(b"".join(parts))
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(tmp_path / "out.bin")
    K = out[:(N + 1) * NU * NX].reshape(N + 1, NU, NX)
    return K, out[(N + 1) * NU * NX:].reshape(N + 1, NU)


GRIDS = {
    "uniform": [0.02] * 9,
    "first_event": [0.0, 0.02, 0.02, 0.0, 0.02, 0.02],
    "consecutive_events": [0.02, 0.0, 0.0, 0.0, 0.02, 0.01, 0.0, 0.02],
    "last_event": [0.02, 0.02, 0.0, 0.02, 0.0],
    "single": [0.02],
}


@pytest.mark.parametrize("grid", sorted(GRIDS))
@pytest.mark.parametrize("formulation", ["wb", "centroidal"])
def test_node_logic_matches_numpy(emu, tmp_path, grid, formulation):
    rng = np.random.default_rng(hash((grid, formulation)) & 0xFFFF)
    cent = formulation == "centroidal"
    dts = np.array(GRIDS[grid])
    N = len(dts)
    nuts = rng.choice([21, 22, 23], N)
    nuts[0] = 21                                              # a padded record at node 0 ...
    nuts[-1] = 23
    qp, ric, x, u, Px, Pu, Kt = random_records(rng, emu[1], N, cent, nuts)
    K, uff = run_emu(emu, tmp_path, dts, qp, ric, x, u, cent)
    src = feedback_source_nodes(dts)
    assert src[N] == src[N - 1]
    assert np.isfinite(K).all() and np.isfinite(uff).all()   # nothing of the NaN padding leaks in
    nc = CNX if cent else NX
    for i in range(N + 1):
        k = src[i]
        Kr = feedback_gains(Px[k], Pu[k], Kt[k], nuts[k], cent)
        ur = u[k] - Kr[:, :nc] @ x[k, :nc]
        assert np.abs(K[i] - Kr).max() <= 1e-14 * max(1.0, np.abs(Kr).max()), (i, np.abs(K[i] - Kr).max())
        assert np.abs(uff[i] - ur).max() <= 1e-14 * max(1.0, np.abs(ur).max(), np.abs(Kr).max() * np.abs(x[k, :nc]).max())
        assert np.array_equal(K[i], K[k]) and np.array_equal(uff[i], uff[k])   # copied entries are bit copies
        if cent:
            assert (K[i][:, CNX:] == 0.0).all()
    if grid not in ("uniform", "single"):
        assert (src != np.minimum(np.arange(N + 1), N - 1)).any()   # the grid has pre-event entries


def test_source_node_rule():
    assert list(feedback_source_nodes([0.02] * 3)) == [0, 1, 2, 2]
    assert list(feedback_source_nodes([0.0, 0.02, 0.0, 0.0, 0.02])) == [0, 1, 1, 1, 4, 4]
    assert list(feedback_source_nodes([0.02, 0.02, 0.0])) == [0, 1, 1, 1]


def test_linear_controller_restatement():
    """reference.linear_controller_input is ocs2's LinearController on LinearInterpolation::timeSegment."""
    rng = np.random.default_rng(7)
    times = np.array([0.0, 0.1, 0.2, 0.2, 0.3])
    uff, K, x = rng.standard_normal((5, 3)), rng.standard_normal((5, 3, 4)), rng.standard_normal(4)
    at = lambda i: uff[i] + K[i] @ x  # noqa: E731
    for i in (0, 1, 2, 4):
        assert np.allclose(linear_controller_input(times, uff, K, times[i], x), at(i), rtol=1e-14, atol=1e-14)
    assert np.allclose(linear_controller_input(times, uff, K, -1.0, x), at(0))
    assert np.allclose(linear_controller_input(times, uff, K, 9.0, x), at(4))
    mid = linear_controller_input(times, uff, K, 0.125, x)
    assert np.allclose(mid, 0.75 * uff[1] + 0.25 * uff[2] + (0.75 * K[1] + 0.25 * K[2]) @ x)
    # the segment rule of the evaluation: uniform grids and event grids
    assert policy_input_segment(10, 0.02, 0.05) == (2, pytest.approx(0.5))
    assert policy_input_segment(10, 0.02, 1.0) == (8, 1.0)
    assert policy_input_segment(4, None, 0.03, dts=np.array([0.02, 0.02, 0.0, 0.02])) == (1, 0.0)


def test_adaptor_compiles_with_the_feedback_policy(tmp_path, model):
    """The adaptor builds against the stand-in ocs2 headers with useFeedbackPolicy = true (its LinearController branch); without a device it
    fails loudly like the feed-forward driver."""
    from test_adaptor import write_case
    from wb_humanoid_mpc_amd.reference import tile_gait, velocity_command_targets
    exe = tmp_path / "adaptor_feedback_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs", "ocs2"), "-I", os.path.join(LIBDIR, "host"),
                           "-I", os.path.join(ROOT, "tests", "adaptor"), os.path.join(ROOT, "tests", "adaptor_feedback", "adaptor_feedback_driver.cpp"),
                           "-L", LIBDIR, "-lhsqp_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", str(exe)])
    if solver.load_library().hsqp_device_count() > 0:
        pytest.skip("a GPU is visible: the run itself is covered by the gpu test")
    schedule = tile_gait(model.gaits["walk"], 0.3, 6.0)
    targets = velocity_command_targets(model, (0.3, 0.0, 0.7925, 0.0), 0.0, model.initial_state, 3.0)
    write_case(tmp_path, model, schedule, targets, model.initial_state, 1.05, 0.02, 2, _abi.NX)
    image = os.path.join(LIBDIR, "data", "g1_wb.json")
    r = subprocess.run([str(exe), image, str(tmp_path / "case.txt"), str(tmp_path / "out.txt"), "1"], capture_output=True, text=True)
    assert r.returncode == 3 and "runtime_error" in r.stdout and "(-2)" in r.stdout, (r.returncode, r.stdout, r.stderr)
