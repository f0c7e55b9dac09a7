"""The Riccati value function (include/hsqp_value.h) on the MI355X: the record every backward sweep leaves against the float64 references of
tests/value_ref.py (bounds and their derivation: tests/value_tolerances.py), the snapshot of the linearisation trajectory, the evaluation kernel
against the host build of its own source bit for bit, the costate the KKT report reads, the validity rules, batch against solo, the flag's
iteration against the plain one, and the C++ adaptor's getValueFunction."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import event_grid_cases as EG
import value_ref as V
from test_value import emu_eval, vemu  # noqa: F401  (vemu: the module-scoped fixture that builds tests/value/value_emu.cpp)
from tolerances import assert_kkt
from value_tolerances import device_bound
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import make_problem
from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NX, NU, CNX, VF = _abi.NX, _abi.NU, _abi.CNX, _abi.VF_SIZE
B = 3
_dp = C.POINTER(C.c_double)
_cache = {}


SEG_NAME = "wb_walk_n12"   # the smallest horizon the two-level sweep applies to (segment_count: N / 4 >= 3 gives P = 3 at B = 3)


def instances(name, model=None):
    """(x0 [3][58], x, u, par, dt): instance 0 is the golden fixture, 1 and 2 the same problem linearised at perturbed trajectories; read-only.
    SEG_NAME: three perturbed instances of make_problem's walk on 12 nodes, linearised off the cold start."""
    if ("prob", name) not in _cache and name == SEG_NAME:
        x0, x, u, par, dt = make_problem(model, n_nodes=12, batch=B, gait="walk", perturb=True, seed=12)
        rng = np.random.default_rng(12)
        out = (x0, x + 0.005 * rng.standard_normal(x.shape), u + 0.2 * rng.standard_normal(u.shape), par, float(dt))
        for a in out[:4]:
            a.setflags(write=False)
        _cache["prob", name] = out
    if ("prob", name) not in _cache:
        d = np.load(os.path.join(GOLDEN, name + ".npz"))
        nx = CNX if name.startswith("cent") else NX
        rng = np.random.default_rng(len(name))
        x, u = np.repeat(d["x"][None], B, axis=0), np.repeat(d["u"][None], B, axis=0)
        x[1:, :, :nx] += 0.005 * rng.standard_normal((B - 1,) + x.shape[1:2] + (nx,))
        u[1:] += 0.2 * rng.standard_normal(u[1:].shape)
        out = (np.repeat(d["x_init"][None], B, axis=0), x, u, np.repeat(d["par"][None], B, axis=0), float(d["dt"]))
        for a in out[:4]:
            a.setflags(write=False)
        _cache["prob", name] = out
    return _cache["prob", name]


def reference(name, models, oracles):
    """(S [3][N + 1][58][58], s [3][N + 1][58]) of value_ref.dense_tail_value: once per process, read-only"""
    if ("ref", name) not in _cache:
        cent = name.startswith("cent")
        x0, x, u, par, dt = instances(name, models[0])
        rows = [V.dense_tail_value(*V.qp_blocks(models[cent], oracles[cent], x[b], u[b], par[b], dt, cent)) for b in range(B)]
        S, s = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
        S.setflags(write=False)
        s.setflags(write=False)
        _cache["ref", name] = (S, s)
    return _cache["ref", name]


def make_solver(m, N, sweep, batch=B):
    if sweep == "dense":
        os.environ["HSQP_RICCATI_DENSE"] = "1"
    try:
        s = HipSqpSolver(m, max_nodes=N, max_batch=batch, riccati={"parallel": "parallel", "segmented": "segmented"}.get(sweep, "auto"))
    finally:
        os.environ.pop("HSQP_RICCATI_DENSE", None)
    if sweep == "dense":
        assert not s.kernel_forms()["ric_fact"]
    return s


# ---------------------------------------------------------------------------------------------- the record against the references
@pytest.mark.parametrize("name,sweep", [("wb_stance_n4", "serial"), ("wb_walk_n8", "serial"), ("wb_stance_n4", "dense"), ("wb_walk_n8", "dense"),
                                        ("wb_stance_n4", "parallel"), ("wb_walk_n8", "parallel"), ("wb_stance_n4", "segmented"), ("wb_walk_n8", "segmented"),
                                        ("cent_walk_n8", "centroidal")])
def test_record_against_the_reference(model, cmodel, oracle, coracle, name, sweep):
    """The bounds are 10 x the discrepancy of the two CPU references (x 10 more for the two-level sweep), not tuned to the device.  Measured on
    MI355X (profiles/value_parity.txt): whole-body eS 5.0e-13 .. 1.0e-12, es 3.0e-13 .. 6.1e-13 against 1e-11 / 5e-11; centroidal 1.8e-12 / 4.7e-12.
    N = 4 and 8 are below the two-level sweep's range (segment_count: N / 4 >= 3), so its cases here run the serial recursion behind the flag;
    test_two_level_sweep_record_against_the_reference is the one on a horizon it applies to."""
    cent = sweep == "centroidal"
    x0, x, u, par, dt = instances(name)
    S_ref, s_ref = reference(name, (model, cmodel), (oracle, coracle))
    N = u.shape[1]
    s = make_solver(cmodel if cent else model, N, sweep)
    try:
        s.upload(x0, x, u, par, dt)
        s.iterate(1, take_step=True, value_function=True)
        S, sv, xbar = s.value_function()
        out = s.download()
    finally:
        s.close()
    eS, es = V.node_error(S, sv, S_ref, s_ref)
    bS, bs = device_bound(sweep)
    print(f"value parity {name} {sweep}: eS {eS:.3g} (bound {bS:g}) es {es:.3g} (bound {bs:g})")
    assert S.shape == (B, N + 1, NX, NX) and np.array_equal(S, S.transpose(0, 1, 3, 2))
    assert np.array_equal(xbar, x) and not np.array_equal(out["x"], x)             # the step moved x, the record's centre is the uploaded trajectory
    if cent:
        assert not S[:, :, CNX:].any() and not S[:, :, :, CNX:].any() and not sv[:, :, CNX:].any()
    assert eS <= bS and es <= bs, (eS, bS, es, bs)


def test_two_level_sweep_record_against_the_reference(model, cmodel, oracle, coracle):
    """N = 12, B = 3: P = 3 segments.  The record is the two-level sweep's own when the gate accepts it (then it is NOT the serial recursion's bits) and
    the serial fallback's, bit for bit, when the gate rejects it; either way it is held to value_ref.dense_tail_value, with the two-level sweep's
    bound only where that sweep produced it.  With and without the flag the iteration gives the same bits, KKT report included."""
    x0, x, u, par, dt = instances(SEG_NAME, model)
    S_ref, s_ref = reference(SEG_NAME, (model, cmodel), (oracle, coracle))
    N = u.shape[1]
    rec, outs = {}, {}
    for sweep in ("serial", "segmented"):
        s = make_solver(model, N, sweep)
        try:
            for flag, kkt in ((False, False), (True, False), (True, True)):
                before = s.scan_fallbacks()
                s.upload(x0, x, u, par, dt)
                s.iterate(1, take_step=True, kkt=kkt, value_function=flag)
                outs[sweep, flag, kkt] = s.download()
                if flag:
                    rec[sweep, kkt] = s.value_function() + (s.scan_fallbacks() - before,)
        finally:
            s.close()
    for sweep in ("serial", "segmented"):
        for key in ("x", "u", "dx", "du"):
            assert np.array_equal(outs[sweep, False, False][key], outs[sweep, True, False][key]) and np.array_equal(outs[sweep, True, False][key], outs[sweep, True, True][key])
        assert outs[sweep, False, False]["perf_after"] == outs[sweep, True, False]["perf_after"]
        for a, b in zip(rec[sweep, False][:3], rec[sweep, True][:3]):        # the record does not depend on whether the KKT report ran beside it
            assert np.array_equal(a, b)
    assert rec["serial", False][3] == 0
    S, sv, xbar, fallbacks = rec["segmented", False]
    accepted = fallbacks == 0
    if accepted:
        assert not np.array_equal(S, rec["serial", False][0])              # the two-level sweep's own value functions, not the serial recursion's
    else:
        assert np.array_equal(S, rec["serial", False][0]) and np.array_equal(sv, rec["serial", False][1])
    eS, es = V.node_error(S, sv, S_ref, s_ref)
    bS, bs = device_bound("segmented" if accepted else "serial")
    e1 = V.node_error(rec["serial", False][0], rec["serial", False][1], S_ref, s_ref)
    print(f"value parity {SEG_NAME} two-level sweep ({'accepted' if accepted else 'fell back'}): eS {eS:.3g} (bound {bS:g}) es {es:.3g} (bound {bs:g}); serial {e1[0]:.3g} {e1[1]:.3g}")
    assert np.array_equal(xbar, x) and np.array_equal(S, S.transpose(0, 1, 3, 2))
    assert e1[0] <= device_bound("serial")[0] and e1[1] <= device_bound("serial")[1], e1
    assert eS <= bS and es <= bs, (eS, bS, es, bs)
    assert accepted       # on this problem the gate accepts the two-level sweep: the case above IS that sweep's record (a rejection would leave it untested)


# ---------------------------------------------------------------------------------------------- evaluation, costates, windows
@pytest.mark.parametrize("name", ["wb_walk_n8", "cent_walk_n8"])
def test_evaluate_equals_the_host_build_and_the_kkt_costate(model, cmodel, vemu, name):
    cent = name.startswith("cent")
    nx = CNX if cent else NX
    x0, x, u, par, dt = instances(name)
    N = u.shape[1]
    rng = np.random.default_rng(4)
    s = make_solver(cmodel if cent else model, N, "serial")
    try:
        s.upload(x0, x, u, par, dt)
        s.iterate(1, take_step=True, kkt=True, value_function=True)
        out = s.download()
        for b in range(B):   # the KKT report reads lam_k = S_k dx_k + s_k from the same buffer the record is: it still passes
            assert_kkt(out["kkt"][b], out["grad_inf"][b], f"{name} instance {b}")
        S, sv, xbar = s.value_function()
        raw = np.zeros((B, N + 1, VF))    # the record as the sweep stored it (debug-free: symmetric up to rounding, so rebuilt from S for the host build)
        raw[..., :NX * NX], raw[..., NX * NX:] = S.reshape(B, N + 1, -1), sv
        sq = np.tile(np.array([0.0, dt, 2.5 * dt, N * dt, N * dt + 1.0, -0.3, 0.37 * dt, (N - 1) * dt + 1e-9]), (B, 1))
        n = sq.shape[1]
        xq = np.zeros((B, n, NX))
        xq[..., :nx] = x[:, rng.integers(0, N + 1, n), :nx] + 0.02 * rng.standard_normal((B, n, nx))
        dV, g, H = s.evaluate_value_function(sq, xq)
        eV, eg, eH = emu_eval(vemu, raw, xbar, dt, None, cent, sq, xq)
        assert np.array_equal(dV, eV) and np.array_equal(g, eg) and np.array_equal(H, eH)
        dV2, g2, none = s.evaluate_value_function(sq, xq, hessian=False)
        assert none is None and np.array_equal(dV2, dV) and np.array_equal(g2, g)
        # at the QP's own solution xbar_k + dx_k the gradient is the costate of node k
        for k in (0, 3, N):
            gk = s.evaluate_value_function(np.full(B, k * dt), xbar[:, k] + out["dx"][:, k])[1][:, 0]
            lam = np.einsum("bij,bj->bi", S[:, k], out["dx"][:, k]) + sv[:, k]
            assert np.abs(gk - lam).max() <= 1e-13 * (np.abs(S[:, k]).max() * np.abs(out["dx"][:, k]).max() * NX + np.abs(sv[:, k]).max())
        # a NaN state: that query alone
        xq[1, 2, 5] = np.nan
        dVn, gn, Hn = s.evaluate_value_function(sq, xq)
        ok = np.ones((B, n), bool)
        ok[1, 2] = False
        assert np.isnan(dVn[1, 2]) and np.array_equal(dVn[ok], dV[ok]) and np.array_equal(gn[ok], g[ok]) and np.array_equal(Hn, H)
        # windows and NULL outputs
        for k0, k1 in ((0, 0), (2, 5), (N, N), (N - 1, N)):
            Sw, sw, xw = s.value_function(k0, k1)
            assert np.array_equal(Sw, S[:, k0:k1 + 1]) and np.array_equal(sw, sv[:, k0:k1 + 1]) and np.array_equal(xw, xbar[:, k0:k1 + 1])
        only_s = np.full((B, 2, NX), -7.0)
        assert s.lib.hsqp_value_function(s.h, 1, 2, None, only_s.ctypes.data_as(_dp), None) == 0 and np.array_equal(only_s, sv[:, 1:3])
    finally:
        s.close()


def test_evaluate_on_per_instance_event_grids(model, vemu):
    """The non-uniform branch of k_value_eval: every instance on its own padded event grid (tests/event_grid_cases.py, case A_walk: B = 5, N = 18),
    queries on nodes, on the zero-length intervals of an event and of the padding run, mid-interval, at and beyond both ends — bit for bit the host
    build with the same dt_nodes."""
    prob = EG.case(model, "A_walk")
    Bp, N = prob.dts.shape
    stamps = np.concatenate([np.zeros((Bp, 1)), np.cumsum(prob.dts, axis=1)], axis=1)
    rng = np.random.default_rng(9)
    rows = []
    for b in range(Bp):
        zero = EG.event_intervals(prob.dts[b])
        pad0 = int(zero[zero >= prob.n_intervals[b] - 1][0])
        rows.append([stamps[b, 3], stamps[b, int(zero[0])], stamps[b, pad0], 0.5 * (stamps[b, 1] + stamps[b, 2]), 0.0, stamps[b, -1], stamps[b, -1] + 0.5, -0.1,
                     rng.uniform(0.0, stamps[b, -1]), stamps[b, N - 1] + 1e-9])
    sq = np.array(rows)
    n = sq.shape[1]
    s = HipSqpSolver(model, max_nodes=N, max_batch=Bp)
    try:
        s.upload(prob.x0, prob.x, prob.u, prob.par, prob.dts)
        s.iterate(1, take_step=True, value_function=True)
        S, sv, xbar = s.value_function()
        assert np.array_equal(xbar, prob.x)
        xq = prob.x[:, rng.integers(0, N + 1, n)] + 0.02 * rng.standard_normal((Bp, n, NX))
        dV, g, H = s.evaluate_value_function(sq, xq)
    finally:
        s.close()
    raw = np.zeros((Bp, N + 1, VF))
    raw[..., :NX * NX], raw[..., NX * NX:] = S.reshape(Bp, N + 1, -1), sv
    eV, eg, eH = emu_eval(vemu, raw, xbar, 0.0, prob.dts, False, sq, xq)
    assert np.array_equal(dV, eV) and np.array_equal(g, eg) and np.array_equal(H, eH)
    assert np.isfinite(dV).all() and np.isfinite(g).all()
    differ = 0
    for b in range(Bp):   # each instance took ITS grid: on a zero-length interval the post-event node, never a blend across the jump
        for q in (1, 2):
            k, a = V.state_segment(N, 0.0, sq[b, q], prob.dts[b])
            assert a == 0.0 and prob.dts[b, k] > 0.0 and prob.dts[b, k - 1] == 0.0 and np.array_equal(H[b, q], S[b, k]), (b, q)
        differ += V.state_segment(N, 0.0, sq[b, 1], prob.dts[b])[0] != V.state_segment(N, 0.0, sq[b, 1], prob.dts[(b + 1) % Bp])[0]
    assert differ >= 1   # a kernel that read a neighbour's row would land on another node


# ---------------------------------------------------------------------------------------------- validity
def test_validity_rules(model):
    x0, x, u, par, dt = instances("wb_stance_n4")
    N = u.shape[1]
    s = make_solver(model, N, "serial")
    bad = lambda: pytest.raises(HsqpError, match="hsqp error -1")  # noqa: E731
    z = np.zeros(B * NX * NX)
    p = z.ctypes.data_as(_dp)
    try:
        assert s.lib.hsqp_value_function(s.h, 0, 0, p, p, p) == _abi.ERR_BAD_ARG           # fresh handle
        s.upload(x0, x, u, par, dt)
        with bad():
            s.value_function()
        s.iterate(1, take_step=True, kkt=True)                                             # HSQP_ITER_KKT alone fills the buffer, not the record
        with bad():
            s.value_function()
        with bad():
            s.evaluate_value_function(np.zeros(B), x0)
        s.upload(x0, x, u, par, dt)
        s.iterate(1, take_step=True, value_function=True)
        S, sv, xbar = s.value_function()
        # arguments
        for k0, k1 in ((-1, 0), (2, 1), (0, N + 1), (N + 1, N + 1)):
            with bad():
                s.value_function(k0, k1)
        assert s.lib.hsqp_evaluate_value_function(s.h, 0, p, p, p, p, p) == _abi.ERR_BAD_ARG
        assert s.lib.hsqp_evaluate_value_function(s.h, 1, None, p, p, p, p) == _abi.ERR_BAD_ARG
        assert s.lib.hsqp_evaluate_value_function(s.h, 1, p, None, p, p, p) == _abi.ERR_BAD_ARG
        for v in (np.nan, np.inf):
            with bad():
                s.evaluate_value_function(np.array([0.0, v, 0.0]), x0)
        assert np.array_equal(s.value_function()[0], S)                                    # refused calls leave the record alone
        # every clearing event, each followed by a fresh record
        w = s.term_weights()
        clear = {"upload": lambda: s.upload(x0, x, u, par, dt), "solve": lambda: s.run(x0, x, u, par, dt),
                 "update_weights": lambda: s.update_weights(Q=np.array(model.desc.Q[:])),
                 "update_term_weights": lambda: s.update_term_weights(w),
                 "iteration without the flag": lambda: s.iterate(1, take_step=False)}
        for what, call in clear.items():
            call()
            with bad():
                s.value_function()
            s.upload(x0, x, u, par, dt)
            s.iterate(1, take_step=True, value_function=True)
            assert np.array_equal(s.value_function()[0], S), what
        # a failed iteration: n_iterations < 1 is refused, and the record is gone.  (This is an argument refusal, the only failure that can be had on
        # purpose without feeding the sweep a broken problem; it never reaches the sweep.  An iteration that fails later — a HIP error, an allocation —
        # returns through the same path: hsqp_iterate_device clears the mark on entry and sets it only in front of its `return HSQP_OK`.)
        assert s.lib.hsqp_iterate_device(s.h, 0, _abi.ITER_VALUE_FUNCTION) == _abi.ERR_BAD_ARG
        with bad():
            s.value_function()
        # two iterations in one call: the record is the second one's — centred on the first one's result
        s.upload(x0, x, u, par, dt)
        s.iterate(1, take_step=True, value_function=True)
        x1 = s.download()["x"]
        s.upload(x0, x, u, par, dt)
        s.iterate(2, take_step=True, value_function=True)
        S2, _, xbar2 = s.value_function()
        assert np.array_equal(xbar2, x1) and not np.array_equal(S2, S)
        u1 = s.download()["u"]
        assert u1.shape == u.shape
    finally:
        s.close()


# ---------------------------------------------------------------------------------------------- batch against solo, flag against no flag
@pytest.mark.parametrize("name,sweep", [("wb_walk_n8", "serial"), ("wb_walk_n8", "parallel"), ("cent_walk_n8", "centroidal")])
def test_batch_equals_solo_and_the_flag_changes_nothing(model, cmodel, name, sweep):
    cent = sweep == "centroidal"
    m = cmodel if cent else model
    x0, x, u, par, dt = instances(name)
    N = u.shape[1]
    keys = ("x", "u", "dx", "du", "alpha", "step_type")
    s = make_solver(m, N, sweep)
    try:
        runs = {}
        for flag in (False, True):
            s.upload(x0, x, u, par, dt)
            assert s.iterate(1, take_step=True, linesearch=True, until_converged=True, value_function=flag) == 1
            runs[flag] = (s.download(), s.iteration_log(0))
        for k in keys:
            assert np.array_equal(runs[False][0][k], runs[True][0][k]), k
        assert runs[False][0]["perf_after"] == runs[True][0]["perf_after"] and runs[False][0]["perf_before"] == runs[True][0]["perf_before"]
        (pa, aa, ta), (pb, ab, tb) = runs[False][1], runs[True][1]
        assert pa == pb and np.array_equal(aa, ab) and np.array_equal(ta, tb)
        S, sv, xbar = s.value_function()
        sq = np.array([[0.3 * dt, 4.0 * dt]] * B)
        ev = s.evaluate_value_function(sq, x[:, 2])
    finally:
        s.close()
    if sweep == "parallel":   # (the gate accepts or rejects the scan for the batch as a whole: a solo solve may take the other sweep)
        return
    solo = make_solver(m, N, sweep, batch=1)
    try:
        b = 1
        solo.upload(x0[b:b + 1], x[b:b + 1], u[b:b + 1], par[b:b + 1], dt)
        solo.iterate(1, take_step=True, linesearch=True, until_converged=True, value_function=True)
        S1, s1, xb1 = solo.value_function()
        assert np.array_equal(S1[0], S[b]) and np.array_equal(s1[0], sv[b]) and np.array_equal(xb1[0], xbar[b])
        e1 = solo.evaluate_value_function(sq[b:b + 1], x[b:b + 1, 2])
        for got, want in zip(e1, ev):
            assert np.array_equal(got[0], want[b])
    finally:
        solo.close()


# ---------------------------------------------------------------------------------------------- the adaptor
def test_adaptor_get_value_function(tmp_path, model):
    from test_adaptor import LIBDIR, write_case
    from wb_humanoid_mpc_amd.reference import tile_gait, velocity_command_targets
    schedule = tile_gait(model.gaits["walk"], 0.3, 6.0)
    x0 = model.initial_state.copy()
    targets = velocity_command_targets(model, (0.3, 0.0, 0.7925, 0.0), 0.0, x0, 3.0)
    write_case(tmp_path, model, schedule, targets, x0, 0.5, 0.02, 2, NX)
    exe = tmp_path / "adaptor_value_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs", "ocs2"), "-I", os.path.join(LIBDIR, "host"),
                           "-I", os.path.join(ROOT, "tests", "adaptor"), os.path.join(ROOT, "tests", "adaptor_value", "adaptor_value_driver.cpp"),
                           "-L", LIBDIR, "-lhsqp_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", str(exe)])
    image = os.path.join(LIBDIR, "data", "g1_wb.json")
    outs = []
    for flag in (0, 1):
        out = tmp_path / f"out{flag}.txt"
        r = subprocess.run([str(exe), image, str(tmp_path / "case.txt"), str(out), str(flag)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and f"createValueFunction={flag}" in r.stdout, (r.stdout, r.stderr)
        outs.append(out.read_text().splitlines())
    base, extra = [[], []], [[], []]
    for f in (0, 1):
        i, lines = 0, outs[f]
        while i < len(lines):
            n = int(lines[i].split()[0])
            base[f] += lines[i:i + n + 2]
            extra[f].append(lines[i + n + 2])
            i += n + 3
    assert len(base[0]) > 2 * 10 and base[0] == base[1]                      # trajectories and performance indices: bit-identical with and without the record
    for line in extra[0]:
        assert line.startswith("threw: ") and "createValueFunction" in line and "not implemented" not in line
    for line in extra[1]:
        f, dq, da, dV, gmax, asym, ham, lag = line.split()
        assert float(f) == 0.0 and float(dq) == 0.0 and float(da) == 0.0 and float(asym) == 0.0 and float(gmax) > 0.0 and np.isfinite(float(dV))
        assert (ham, lag) == ("1", "1")                                      # the other two queries keep throwing
