"""The Riccati feedback policy (include/hsqp_feedback.h) on the MI355X: the gains explain the QP's response to the initial state (the step is
affine in x_init) for every backward sweep, agree with the CPU oracle's response, have the structure of ocs2's LinearController (copies,
padding, windows, device destinations, Px + Pu K~ of the raw records), evaluate like LinearController::computeInput, are valid exactly
between a successful iteration and the next upload, and reach the C++ adaptor's PrimalSolution as a LinearController."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_feedback_policy import LAYOUT
from tolerances import TRAJ_ABS
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import (feedback_gains, feedback_source_nodes, linear_controller_input, make_centroidal_problem, make_problem,
                                           policy_input_segment)
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu
NX, NU, CNX = _abi.NX, _abi.NU, _abi.CNX
EPS = 1e-3


def problem(m, cent, N, B=1, seed=3):
    return (make_centroidal_problem if cent else make_problem)(m, n_nodes=N, batch=B, perturb=True, seed=seed)


def event_dts(dt, N):
    dts = np.full(N, dt)
    dts[[4, 9, 10, 15]] = 0.0          # an event, and two in a row
    return dts


def replicate(prob, x_inits):
    x0, x, u, par, dt = prob
    B = len(x_inits)
    rep = lambda a: np.repeat(a[:1], B, axis=0)  # noqa: E731
    return np.asarray(x_inits), rep(x), rep(u), rep(par), dt


def check_affine_response(K, out, dts, bound=1e-9):
    """instance 0 is the base, the others moved x_init: du_k - K_k dx_k vanishes at every non-event node k < N (K: instance 0's)."""
    x, u = out["x"], out["u"]
    N = u.shape[1]
    worst = 0.0
    for j in range(1, x.shape[0]):
        for k in range(N):
            if dts[k] == 0.0:
                continue
            dx, du = x[j, k] - x[0, k], u[j, k] - u[0, k]
            r = np.abs(du - K[0, k] @ dx).max()
            lim = bound * max(1.0, np.abs(K[0, k]).sum(axis=1).max() * np.abs(dx).max())
            assert r <= lim, (j, k, r, lim)
            worst = max(worst, r / lim)
    return worst


@pytest.mark.parametrize("case", ["wb", "centroidal", "wb_events"])
def test_gains_explain_the_response_to_the_initial_state(model, cmodel, case):
    cent = case == "centroidal"
    m = cmodel if cent else model
    N = 20
    base = problem(m, cent, N)
    nx = CNX if cent else NX
    x_inits = [base[0][0]] + [base[0][0] + EPS * np.eye(NX)[i] for i in range(nx)]
    x0, x, u, par, dt = replicate(base, x_inits)
    dts = event_dts(dt, N) if case == "wb_events" else np.full(N, dt)
    B = len(x_inits)
    s = HipSqpSolver(m, max_nodes=N, max_batch=B)
    try:
        out = s.run(x0, x, u, par, dts if case == "wb_events" else dt)
        assert (out["step_type"] == _abi.STEP_FULL).all()
        K, uff = s.feedback_policy()
        assert K.shape == (B, N + 1, NU, NX)
        check_affine_response(K, out, dts)
        # column j of K_0 is the response of u_0 to x_init's entry j
        col = (out["u"][1:, 0] - out["u"][0, 0]).T / EPS
        assert np.abs(col - K[0, 0][:, :nx]).max() <= 1e-9 * max(1.0, np.abs(K[0, 0]).max()) / EPS
        if cent:
            assert (K[:, :, :, CNX:] == 0.0).all()
    finally:
        s.close()


@pytest.mark.parametrize("riccati", ["parallel_auto", "segmented"])
def test_gains_of_the_scan_and_the_segmented_sweep(model, riccati):
    N = 48 if riccati == "parallel_auto" else 40
    B = 2 if riccati == "parallel_auto" else 6
    base = problem(model, False, N)
    rng = np.random.default_rng(11)
    x_inits = [base[0][0]] + [base[0][0] + 1e-3 * rng.standard_normal(NX) for _ in range(B - 1)]
    x0, x, u, par, dt = replicate(base, x_inits)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, riccati="auto" if riccati == "parallel_auto" else "segmented")
    try:
        before = s.scan_fallbacks()
        out = s.run(x0, x, u, par, dt)
        K, _ = s.feedback_policy()
        assert s.scan_fallbacks() == before            # the gains are the gated sweep's own
        check_affine_response(K, out, np.full(N, dt))
    finally:
        s.close()


@pytest.mark.parametrize("formulation", ["wb", "centroidal"])
def test_gains_against_the_cpu_oracle(model, cmodel, oracle, coracle, formulation):
    cent = formulation == "centroidal"
    m, orc = (cmodel, coracle) if cent else (model, oracle)
    N = 10
    base = problem(m, cent, N)
    rng = np.random.default_rng(5)
    nx = CNX if cent else NX
    d = np.zeros(NX)
    d[:nx] = 1e-3 * rng.standard_normal(nx)
    x0, x, u, par, dt = replicate(base, [base[0][0], base[0][0] + d])
    s = HipSqpSolver(m, max_nodes=N, max_batch=2)
    try:
        s.run(x0, x, u, par, dt)
        K, _ = s.feedback_policy()
    finally:
        s.close()
    it = orc.cent_sqp_iteration if cent else orc.sqp_iteration
    r0, r1 = (it(dt, x0[b], x[0], u[0], par[0], threads=4) for b in (0, 1))
    worst = 0.0
    for k in range(N):
        dxo, duo = r1["x"][k] - r0["x"][k], r1["u"][k] - r0["u"][k]
        err = np.abs(duo - K[0, k] @ dxo).max()
        lim = 2 * TRAJ_ABS * (1.0 + np.abs(K[0, k]).sum(axis=1).max())
        assert err <= lim, (k, err, lim)
        worst = max(worst, err / lim)
    print(f"oracle {formulation}: worst |du_oracle - K_gpu dx_oracle| / bound = {worst:.3g}")


class DeviceBuffer:
    """hipMalloc'd doubles through the HIP runtime the library is linked against (device destinations of hsqp_feedback_policy_device)."""
    _hip = None

    def __init__(self, shape, fill=np.nan):
        if DeviceBuffer._hip is None:
            for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
                try:
                    DeviceBuffer._hip = C.CDLL(name)
                    break
                except OSError:
                    pass
        self.shape, self.nbytes = shape, int(np.prod(shape)) * 8
        self.ptr = C.c_void_p()
        assert self._hip.hipMalloc(C.byref(self.ptr), C.c_size_t(self.nbytes)) == 0
        self.upload(np.full(shape, fill))

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert self._hip.hipMemcpy(self.ptr, a.ctypes.data_as(C.c_void_p), C.c_size_t(self.nbytes), 1) == 0   # hipMemcpyHostToDevice

    def numpy(self):
        a = np.empty(self.shape)
        assert self._hip.hipMemcpy(a.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(self.nbytes), 2) == 0   # hipMemcpyDeviceToHost
        return a

    def free(self):
        self._hip.hipFree(self.ptr)


def raw_records(s, B, N):
    L = LAYOUT
    ric = np.zeros((B, N, L["RIC_SIZE"]))
    qp = np.zeros((B, N, L["QP_SIZE"]))
    assert s.lib.hsqp_debug_read(s.h, 101, ric.ctypes.data_as(C.c_void_p), ric.nbytes) == ric.nbytes
    assert s.lib.hsqp_debug_read(s.h, 102, qp.ctypes.data_as(C.c_void_p), qp.nbytes) == qp.nbytes
    Px = qp[..., L["QP_PX"]:L["QP_PX"] + NU * NX].reshape(B, N, NU, NX)
    Pu = qp[..., L["QP_PU"]:L["QP_PU"] + NU * 23].reshape(B, N, NU, 23)
    nut = qp[..., L["QP_NUT"]].astype(int)
    Kt = ric[..., L["RIC_K"]:L["RIC_K"] + 23 * NX].reshape(B, N, 23, NX)
    return Px, Pu, Kt, nut


@pytest.mark.parametrize("formulation", ["wb", "centroidal"])
def test_policy_structure(model, cmodel, formulation):
    cent = formulation == "centroidal"
    m = cmodel if cent else model
    N, B = 20, 3
    x0, x, u, par, dt = problem(m, cent, N, B)
    dts = np.tile(event_dts(dt, N), (B, 1))
    s = HipSqpSolver(m, max_nodes=N, max_batch=B)
    try:
        s.upload(x0, x, u, par, dts)
        s.iterate(1, take_step=True, kkt=True)        # (the KKT report makes k_project write the whole record: block 102)
        out = s.download()
        K, uff = s.feedback_policy()
        src = feedback_source_nodes(dts[0])
        for i in range(N + 1):
            if src[i] != i:                            # pre-event and terminal entries: bit copies
                assert np.array_equal(K[:, i], K[:, src[i]]) and np.array_equal(uff[:, i], uff[:, src[i]])
        assert src[N] == N - 1 and (src[:N] != np.arange(N)).sum() == 4
        if cent:
            assert (K[..., CNX:] == 0.0).all()
        xs, us = out["x"], out["u"]
        for b in range(B):
            for i in range(N):
                if src[i] == i:
                    r = K[b, i] @ xs[b, i] + uff[b, i] - us[b, i]
                    assert np.abs(r).max() <= 1e-13 * max(1.0, np.abs(us[b, i]).max(), np.abs(K[b, i]).max() * np.abs(xs[b, i]).max())
        for first, count in ((0, 1), (3, 5), (N, 1), (N - 4, 5), (9, 3)):
            Kw, uw = s.feedback_policy(first, count)
            assert np.array_equal(Kw, K[:, first:first + count]) and np.array_equal(uw, uff[:, first:first + count])
        dK, du, du2 = DeviceBuffer((B, N + 1, NU, NX)), DeviceBuffer((B, N + 1, NU)), DeviceBuffer((B, 4, NU))
        try:
            s.feedback_policy_device(0, N + 1, dK.ptr.value, du.ptr.value)
            assert np.array_equal(dK.numpy(), K) and np.array_equal(du.numpy(), uff)
            s.feedback_policy_device(2, 4, 0, du2.ptr.value)   # uff only
            assert np.array_equal(du2.numpy(), uff[:, 2:6])
        finally:
            for d in (dK, du, du2):
                d.free()
        Px, Pu, Kt, nut = raw_records(s, B, N)
        for b in range(B):
            for i in range(N + 1):
                k = src[i]
                Kr = feedback_gains(Px[b, k], Pu[b, k], Kt[b, k], nut[b, k], cent)
                assert np.abs(K[b, i] - Kr).max() <= 1e-13 * max(1.0, np.abs(Kr).max()), (b, i)
    finally:
        s.close()


@pytest.mark.parametrize("case", ["wb", "centroidal", "wb_events"])
def test_evaluate_feedback_policy(model, cmodel, case):
    cent = case == "centroidal"
    m = cmodel if cent else model
    N, B = 20, 8
    x0, x, u, par, dt = problem(m, cent, N, B)
    grid = case == "wb_events"
    dts = np.tile(event_dts(dt, N), (B, 1)) if grid else np.full((B, N), dt)
    nx = CNX if cent else NX
    rng = np.random.default_rng(17)
    s = HipSqpSolver(m, max_nodes=N, max_batch=B)
    try:
        out = s.run(x0, x, u, par, dts if grid else dt)
        K, uff = s.feedback_policy()
        stamps = np.concatenate([np.zeros((B, 1)), np.cumsum(dts, axis=1)], axis=1)
        cases = [rng.uniform(0, N * dt, B), stamps[np.arange(B), rng.integers(0, N, B)], np.full(B, N * dt + 0.1),
                 stamps[:, 4], stamps[:, 10] + 0.3 * dt, np.zeros(B)]
        for sv in cases:
            xm = np.zeros((B, NX))
            xm[:, :nx] = out["x"][:, 3, :nx] + 0.01 * rng.standard_normal((B, nx))
            xf, uf, tf = s.evaluate_feedback_policy(sv, xm)
            xp, up, tp = s.evaluate_policy(sv)
            assert np.array_equal(xf, xp)
            assert np.array_equal(tf, s.joint_torques(xf, uf))
            for b in range(B):
                ku, au = policy_input_segment(N, dt, sv[b], dts=dts[b] if grid else None)
                ref = linear_controller_input([0.0, 1.0], uff[b, [ku, ku + 1]], K[b, [ku, ku + 1]], au, xm[b])
                scale = max(1.0, np.abs(ref).max(), np.abs(K[b, ku]).max() * np.abs(xm[b]).max())
                assert np.abs(uf[b] - ref).max() <= 1e-12 * scale, (b, sv[b])
        # at the stamp of a node that carries its own entry, at the optimal state there, the feedback input is the optimal input
        src = feedback_source_nodes(dts[0])
        for k in (0, 2, 7, 13):
            if src[k] != k or (k + 1 <= N - 1 and dts[0, k + 1] == 0.0) or (k > 0 and dts[0, k - 1] == 0.0):
                continue
            sv = stamps[:, k]
            xf, uf, _ = s.evaluate_feedback_policy(sv, out["x"][:, k])
            _, up, _ = s.evaluate_policy(sv)
            for b in range(B):
                assert np.abs(uf[b] - up[b]).max() <= 1e-11 * max(1.0, np.abs(up[b]).max(), np.abs(K[b, k]).max() * np.abs(out["x"][b, k]).max()), (k, b)
    finally:
        s.close()


def test_validity(model):
    from test_gpu_warm_start import Loop
    N, B = 12, 2
    x0, x, u, par, dt = problem(model, False, N, B)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    bad = lambda: pytest.raises(HsqpError, match="hsqp error -1")  # noqa: E731
    z = np.zeros(B * (N + 1) * NU * NX)
    dp = z.ctypes.data_as(C.POINTER(C.c_double))
    try:
        assert s.lib.hsqp_feedback_policy(s.h, 0, 1, dp, dp) == _abi.ERR_BAD_ARG      # fresh handle
        s.upload(x0, x, u, par, dt)
        with bad():
            s.feedback_policy()
        with bad():
            s.evaluate_feedback_policy(np.zeros(B), x0)
        s.iterate(1, take_step=True)
        K, _ = s.feedback_policy()
        for first, count in ((-1, 2), (0, 0), (0, N + 2), (N, 2), (N + 1, 1)):
            with bad():
                s.feedback_policy(first, count)
        s.upload(x0, x, u, par, dt)                   # every upload invalidates it
        with bad():
            s.feedback_policy()
        s.iterate(1, take_step=True)
        assert np.array_equal(s.feedback_policy()[0], K)
    finally:
        s.close()
    loop = Loop(model, 2, horizon=0.7, event_nodes=False)
    s = HipSqpSolver(model, max_nodes=40, max_batch=2, linesearch=True)
    try:
        loop.upload_warm(s, 0.0, loop.x_init, "cold")
        s.iterate(1, take_step=True, linesearch=True)
        s.feedback_policy()
        loop.upload_warm(s, 0.02, loop.x_init, "shift")
        with bad():
            s.feedback_policy()
        s.iterate(1, take_step=True, linesearch=True)
        K, uff = s.feedback_policy()
        out = s.download()
        assert np.abs(np.einsum("bkij,bkj->bki", K[:, :-1], out["x"][:, :-1]) + uff[:, :-1] - out["u"]).max() < 1e-9
    finally:
        s.close()


@pytest.mark.parametrize("formulation", ["wb", "centroidal"])
def test_adaptor_builds_a_linear_controller(tmp_path, model, cmodel, formulation):
    from test_adaptor import LIBDIR, ROOT, write_case
    from wb_humanoid_mpc_amd.reference import centroidal_velocity_command_targets, tile_gait, velocity_command_targets
    cent = formulation == "centroidal"
    m = cmodel if cent else model
    nx = CNX if cent else NX
    schedule = tile_gait(m.gaits["walk"], 0.3, 6.0)
    x0 = m.initial_state.copy()
    targets = (centroidal_velocity_command_targets if cent else velocity_command_targets)(m, (0.3, 0.0, 0.7925, 0.0), 0.0, x0, 3.0)
    write_case(tmp_path, m, schedule, targets, x0, 0.6 if cent else 1.05, 0.02, 3, nx)
    exe = tmp_path / "adaptor_feedback_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs", "ocs2"), "-I", os.path.join(LIBDIR, "host"),
                           "-I", os.path.join(ROOT, "tests", "adaptor"), os.path.join(ROOT, "tests", "adaptor_feedback", "adaptor_feedback_driver.cpp"),
                           "-L", LIBDIR, "-lhsqp_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", str(exe)])
    image = os.path.join(LIBDIR, "data", "g1_centroidal.json" if cent else "g1_wb.json")
    outs = []
    for flag in (0, 1):
        out = tmp_path / f"out{flag}.txt"
        r = subprocess.run([str(exe), image, str(tmp_path / "case.txt"), str(out), str(flag)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f"useFeedbackPolicy={flag}" in r.stdout, (r.stdout, r.stderr)
        outs.append(out.read_text().splitlines())
    plain, fb, extra = outs[0], [], []
    lines = outs[1]
    i = 0
    while i < len(lines):
        n = int(lines[i].split()[0])
        fb += lines[i:i + n + 2]
        extra.append(lines[i + n + 2].split())
        i += n + 3
    assert len(plain) > 3 * 10 and fb == plain                 # trajectories and performance indices: bit-identical
    for is_linear, arr_diff, in_diff, entries in extra:
        assert is_linear == "1" and float(arr_diff) == 0.0 and float(in_diff) <= 1e-12 and int(entries) > 10
