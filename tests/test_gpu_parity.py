"""GPU parity tests: the HIP path, called through the C ABI, against the CPU oracle and the committed
golden fixtures.  Tolerances = BASELINE.md §6 without relaxation (tests/tolerances.py): trajectories / steps max-abs <= 1e-8
absolute, QP KKT residuals <= 1e-9 * max(1, |g|_inf), performance-index terms rel <= 1e-10."""
import os

import numpy as np
import pytest

from test_oracle_lq import perturbed_problem
from tolerances import KKT_REL, TRAJ_ABS, assert_kkt, assert_perf, assert_perf_arrays, assert_step, assert_linear_residual
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.reference import make_problem

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NX, NU, NZ = _abi.NX, _abi.NU, _abi.NZ


@pytest.fixture(scope="module")
def gpu_solver(model):
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    s = HipSqpSolver(model, max_nodes=100, max_batch=8)
    yield s
    s.close()


def rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


@pytest.mark.parametrize("name", ["wb_stance_n4", "wb_walk_n8", "wb_run_n14"])
def test_against_golden_fixtures(gpu_solver, name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    out = gpu_solver.run(g["x_init"], g["x"], g["u"], g["par"], float(g["dt"]))
    assert_step(out, dict(dx=g["dx"], du=g["du"], x=g["x"] + g["dx"], u=g["u"] + g["du"]), 0, name)
    pb, pa = out["perf_before"][0], out["perf_after"][0]
    for got, want in ((pb, g["perf_before"]), (pa, g["perf_after"])):
        assert_perf_arrays([got["cost"], got["dynamics_sse"], got["equality_sse"]], want, name)
    assert_kkt(out["kkt"][0], np.abs(g["g"]).max(), name)
    # intermediate blocks
    assert rel(gpu_solver.debug_read(_abi.BLK_BVEC)[0], g["b"]) <= 1e-12
    assert rel(gpu_solver.debug_read(_abi.BLK_G)[0], g["g"]) <= 1e-11
    assert rel(gpu_solver.debug_read(_abi.BLK_COST)[0], g["cost"]) <= 1e-11
    assert rel(gpu_solver.debug_read(_abi.BLK_FLOW)[0], g["flow"]) <= 1e-12
    assert np.array_equal(gpu_solver.debug_read(_abi.BLK_NE)[0], g["ne"])
    assert rel(gpu_solver.debug_read(_abi.BLK_CDE)[0][:, :, -1], g["e"]) <= 1e-11
    assert rel(gpu_solver.debug_read(_abi.BLK_AB)[0][:, 29, :], g["AB_row29"]) <= 1e-11
    assert rel(np.einsum("kii->ki", gpu_solver.debug_read(_abi.BLK_H)[0]), g["H_diag"]) <= 1e-11


@pytest.mark.parametrize("gait,n", [("stance", 5), ("walk", 10), ("run", 14)])
def test_lq_blocks_against_oracle(gpu_solver, model, oracle, gait, n):
    x0, x, u, par, dt = perturbed_problem(model, n, gait, seed=31)
    gpu_solver.run(x0, x, u, par, dt)
    lq = oracle.lq(dt, x, u, par, threads=4)
    for blk, key in ((_abi.BLK_AB, "AB"), (_abi.BLK_BVEC, "b"), (_abi.BLK_H, "H"), (_abi.BLK_G, "g"), (_abi.BLK_CDE, "CDe"),
                     (_abi.BLK_COST, "cost"), (_abi.BLK_FLOW, "flow")):
        assert rel(gpu_solver.debug_read(blk)[0], lq[key]) <= 1e-11, key
    assert np.array_equal(gpu_solver.debug_read(_abi.BLK_NE)[0], lq["ne"])


@pytest.fixture(scope="module")
def limb_solver(model):
    """A handle on the limb-lane form of the whole-body LQ approximation (hsqp_lql.h: k_lq_limb + k_lq_rows + k_lq_chain) — what handles sized to
    fill the GPU run; a handle this small would take the phase form (k_lq<true>) by itself, HSQP_LQ_LIMB_FORM at hsqp_create forces it."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    os.environ["HSQP_LQ_LIMB_FORM"] = "1"
    try:
        s = HipSqpSolver(model, max_nodes=37, max_batch=5)
    finally:
        os.environ.pop("HSQP_LQ_LIMB_FORM", None)
    yield s
    s.close()


@pytest.mark.parametrize("gait,n", [("stance", 5), ("walk", 10), ("run", 14)])
def test_lq_blocks_of_the_limb_lane_form_against_oracle(limb_solver, model, oracle, gait, n):
    """The LQ blocks of the limb-lane kernels (a lane per limb, 16 nodes per wave; residual / equality rows stored transposed) against the oracle:
    the same bound as the phase form's.  n = 5, 10, 14 nodes: every wave carries padding quads; `run` has active collision rows."""
    x0, x, u, par, dt = perturbed_problem(model, n, gait, seed=31)
    limb_solver.run(x0, x, u, par, dt)
    lq = oracle.lq(dt, x, u, par, threads=4)
    for blk, key in ((_abi.BLK_AB, "AB"), (_abi.BLK_BVEC, "b"), (_abi.BLK_H, "H"), (_abi.BLK_G, "g"), (_abi.BLK_CDE, "CDe"),
                     (_abi.BLK_COST, "cost"), (_abi.BLK_FLOW, "flow")):
        assert rel(limb_solver.debug_read(blk)[0], lq[key]) <= 1e-11, key
    assert np.array_equal(limb_solver.debug_read(_abi.BLK_NE)[0], lq["ne"])


def test_limb_lane_form_equals_the_phase_form(limb_solver, gpu_solver, model, oracle):
    """One SQP iteration (line search included) through either form of the LQ kernel: the same step to rounding (1e-10 of its scale), both
    within the oracle's bound; a batch of 5 x 37 nodes = 185 nodes (11.6 waves of 16: the last wave of the batch is part padding), and
    the contact modes change along the horizon — rows that were written for a foot in contact must read zero once it swings
    (second solve on the same handle with the gait phase shifted)."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    for seed, gait in ((21, "walk"), (22, "run"), (23, "walk")):
        x0, x, u, par, dt = make_problem(model, n_nodes=37, batch=5, perturb=True, seed=seed, gait=gait)
        a = limb_solver.run(x0, x, u, par, dt)
        b = gpu_solver.run(x0, x, u, par, dt)
        sc = max(1.0, np.abs(b["dx"]).max(), np.abs(b["du"]).max())
        assert np.abs(a["dx"] - b["dx"]).max() <= 1e-10 * sc and np.abs(a["du"] - b["du"]).max() <= 1e-10 * sc
        for pa, pb in zip(a["perf_before"], b["perf_before"]):
            for key in ("cost", "dynamics_sse", "equality_sse"):
                assert abs(pa[key] - pb[key]) <= 1e-12 * max(1.0, abs(pb[key])), (key, pa, pb)
        r = oracle.sqp_iteration(dt, x0[2], x[2], u[2], par[2], threads=4)
        assert_step(a, r, 2)
        assert_kkt(a["kkt"][2], a["grad_inf"][2], "limb form")


def test_batch_of_perturbed_instances_against_oracle(gpu_solver, model, oracle):
    """BASELINE config 4 inputs at a size the oracle finishes in seconds: B = 6 perturbed instances, N = 16."""
    x0, x, u, par, dt = make_problem(model, n_nodes=16, batch=6, perturb=True)
    out = gpu_solver.run(x0, x, u, par, dt)
    for b in range(6):
        r = oracle.sqp_iteration(dt, x0[b], x[b], u[b], par[b], threads=4)
        assert_step(out, r, b)
        assert_perf(out["perf_before"][b], r["perf_before"], f"instance {b} before")
        assert_perf(out["perf_after"][b], r["perf_after"], f"instance {b} after")
    # instances are independent: solving one alone gives the same bits as inside the batch
    solo = gpu_solver.run(x0[3], x[3], u[3], par[3], dt)
    assert np.array_equal(solo["dx"][0], out["dx"][3]) and np.array_equal(solo["du"][0], out["du"][3])


def test_full_size_properties(gpu_solver, model):
    """BASELINE config 3/4 size (N = 100): size-independent properties of the QP step, no oracle needed."""
    x0, x, u, par, dt = make_problem(model, n_nodes=100, batch=4, perturb=True)
    x0 = x0 + 1e-3  # non-zero dx_0
    out = gpu_solver.run(x0, x, u, par, dt)
    dx, du = out["dx"], out["du"]
    AB = gpu_solver.debug_read(_abi.BLK_AB)
    b = gpu_solver.debug_read(_abi.BLK_BVEC)
    CDe = gpu_solver.debug_read(_abi.BLK_CDE)
    ne = gpu_solver.debug_read(_abi.BLK_NE)
    assert np.abs(dx[:, 0] - (x0 - x[:, 0])).max() <= 1e-12
    z = np.concatenate([dx[:, :-1], du], axis=2)
    defect = dx[:, 1:] - np.einsum("bkij,bkj->bki", AB, z) - b
    assert_linear_residual(AB, z, np.abs(b) + np.abs(dx[:, 1:]), defect, 1e-10, "linearised dynamics")
    eq = np.einsum("bkrj,bkj->bkr", CDe[..., :NZ], z) + CDe[..., NZ]
    assert_linear_residual(CDe[..., :NZ], z, CDe[..., NZ], eq, 1e-10, "linearised equality constraints")
    assert set(np.unique(ne)) <= {12, 13, 14} and 13 in ne
    g = gpu_solver.debug_read(_abi.BLK_G)
    for bb in range(4):
        assert_kkt(out["kkt"][bb], np.abs(g[bb]).max(), f"instance {bb}")
    assert np.all(np.isfinite(out["x"])) and np.all(np.isfinite(out["u"]))
    # the full step is x + dx
    assert np.abs(out["x"] - (x + dx)).max() <= 1e-12 and np.abs(out["u"] - (u + du)).max() <= 1e-11


def test_device_resident_iterations_equal_repeated_solves(gpu_solver, model):
    x0, x, u, par, dt = make_problem(model, n_nodes=12, batch=2, gait="stance", v_cmd=(0, 0, 0.7925, 0))
    a = gpu_solver.run(x0, x, u, par, dt)
    b = gpu_solver.run(x0, a["x"], a["u"], par, dt)
    gpu_solver.upload(x0, x, u, par, dt)
    gpu_solver.iterate(2, take_step=True, kkt=True)
    c = gpu_solver.download()
    assert np.array_equal(b["x"], c["x"]) and np.array_equal(b["u"], c["u"])
    ms = gpu_solver.kernel_ms()
    assert ms["total"] > 0.0 and abs(ms["total"] - (ms["lq"] + ms["project"] + ms["riccati"] + ms["step_perf"])) < 1e-4
    # stance from rest converges (same behaviour as the oracle, tests/test_oracle_lq.py::test_sqp_converges_on_stance)
    assert np.abs(c["dx"]).max() < np.abs(a["dx"]).max()


def test_error_behaviour(gpu_solver, model):
    from wb_humanoid_mpc_amd.solver import HsqpError
    x0, x, u, par, dt = make_problem(model, n_nodes=4, batch=1)
    with pytest.raises(HsqpError) as e:
        gpu_solver.run(x0, x, u, par, -1.0)
    assert e.value.code == _abi.ERR_BAD_ARG
    big = make_problem(model, n_nodes=101, batch=1)
    with pytest.raises(HsqpError) as e:
        gpu_solver.run(*big)
    assert e.value.code == _abi.ERR_BAD_ARG
    # rank-deficient equality Jacobian is impossible to construct through valid inputs; a NaN state must surface as NUMERIC, not hang
    xb = x.copy()
    xb[0, 2, 7] = np.nan
    with pytest.raises(HsqpError) as e:
        gpu_solver.run(x0, xb, u, par, dt)
    assert e.value.code == _abi.ERR_NUMERIC


@pytest.mark.parametrize("override", [{}, {"gamma_c": 0.6}, {"gamma_c": 0.9, "g_max": 1e-9, "g_min": 1e-12}])
def test_filter_linesearch_against_oracle(gpu_solver, model, oracle, override):
    """step length, step type, accepted trajectory and its performance index of the device line search
    equal the oracle's restatement of ocs2::FilterLinesearch / SqpSolver::takeStep, per instance, including the
    back-tracking ({gamma_c: 0.6}) and the zero-step ({gamma_c: 0.9, g_max: 1e-9, g_min: 1e-12}) branches."""
    B, N = 4, 8
    x0, x, u, par, dt = make_problem(model, n_nodes=N, batch=B, perturb=True, seed=5)
    rng = np.random.default_rng(3)
    x = x + 0.01 * rng.standard_normal(x.shape)          # leave the cold start so that every term is active
    u = u + 0.3 * rng.standard_normal(u.shape)
    gpu_solver.set_linesearch(**override)
    try:
        gpu_solver.upload(x0, x, u, par, dt)
        gpu_solver.iterate(1, linesearch=True)
        out = gpu_solver.download()
    finally:
        gpu_solver.set_linesearch()
    alphas = []
    for b in range(B):
        r = oracle.sqp_iteration(dt, x0[b], x[b], u[b], par[b], threads=4)
        ls = oracle.linesearch(dt, x[b], u[b], r["dx"], r["du"], par[b], r["armijo"], threads=4, **override)
        assert out["armijo"][b] == pytest.approx(r["armijo"], rel=1e-9, abs=1e-9)
        assert out["alpha"][b] == ls["alpha"] and out["step_type"][b] == ls["step_type"], (b, out["alpha"][b], ls)
        assert np.abs(out["x"][b] - ls["x"]).max() <= TRAJ_ABS and np.abs(out["u"][b] - ls["u"]).max() <= TRAJ_ABS
        assert_perf(out["perf_after"][b], ls["perf"], f"instance {b} accepted trial")
        alphas.append(ls["alpha"])
    if override.get("g_max") == 1e-9:
        assert all(a == 0.0 for a in alphas)            # nothing can be accepted: zero step, trajectory kept
        assert np.array_equal(out["x"], x) and np.array_equal(out["u"], u)
    if override == {"gamma_c": 0.6}:
        assert any(0.0 < a < 1.0 for a in alphas) or all(a in (0.0, 1.0) for a in alphas)


def test_full_step_reports_alpha_one(gpu_solver, model):
    x0, x, u, par, dt = make_problem(model, n_nodes=6, batch=2, perturb=True)
    out = gpu_solver.run(x0, x, u, par, dt)
    assert np.array_equal(out["alpha"], np.ones(2)) and np.array_equal(out["step_type"], np.full(2, _abi.STEP_FULL))


def test_multi_iteration_sqp_with_linesearch(model):
    """sqpIteration > 1 with the filter line search, device resident: equal to repeated hsqp_solve calls
    of a line-search solver, and the constraint violation of a perturbed walk problem decreases monotonically."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    x0, x, u, par, dt = make_problem(model, n_nodes=10, batch=3, perturb=True, seed=9)
    s = HipSqpSolver(model, max_nodes=10, max_batch=3, linesearch=True)
    try:
        xs, us, viol = x, u, []
        for _ in range(3):
            out = s.run(x0, xs, us, par, dt)
            assert np.all(out["step_type"] != _abi.STEP_FULL)
            viol.append([np.sqrt(p["dynamics_sse"] + p["equality_sse"]) for p in out["perf_after"]])
            xs, us = out["x"], out["u"]
        s.upload(x0, x, u, par, dt)
        s.iterate(3, take_step=True, linesearch=True)
        res = s.download()
        assert np.array_equal(res["x"], xs) and np.array_equal(res["u"], us)
        viol = np.array(viol)
        assert np.all(viol[1:] <= viol[:-1] * (1 + 1e-12))
    finally:
        s.close()


def test_instances_of_a_large_batch_equal_their_solo_solves(model):
    """Independence of the batch axis under full occupancy: with several workgroups resident per CU every instance must get
    bit-identical results to the same instance solved alone, and the batch must be repeatable (catches intra-workgroup races
    that lock-step execution of a lone workgroup hides)."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    B, N = 96, 60
    x0, x, u, par, dt = make_problem(model, n_nodes=N, batch=B, perturb=True, seed=77)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B, riccati="serial")   # a lone instance on 60 nodes would otherwise take the parallel-in-time sweep
    try:
        a = s.run(x0, x, u, par, dt)
        b = s.run(x0, x, u, par, dt)
        assert np.array_equal(a["dx"], b["dx"]) and np.array_equal(a["du"], b["du"])
        for i in range(0, B, 7):
            solo = s.run(x0[i], x[i], u[i], par[i], dt)
            assert np.array_equal(solo["dx"][0], a["dx"][i]) and np.array_equal(solo["du"][0], a["du"][i]), i
            assert solo["perf_after"][0] == a["perf_after"][i]
    finally:
        s.close()


def test_config4_instances_against_oracle_at_full_size(model, oracle):
    """BASELINE config 4 at full size (N = 100, 256 perturbed instances, every CU busy): seventeen instances of the batch against the CPU oracle
    (step max-abs <= 1e-8; performance index before / after the step — at this size the value pass runs on quads of lanes, 16 nodes per wave), and
    EVERY instance through the size-independent property the device reports itself: the KKT residual of its QP within 1e-9 max(1, |g|_inf)."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    B, N = 256, 100
    x0, x, u, par, dt = make_problem(model, n_nodes=N, batch=B, perturb=True)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    try:
        assert s.kernel_forms() == {"lq_limb": True, "value_quad": True, "lq_ranges": 2, "ric_fact": True, "chain_fused": True}
        out = s.run(x0, x, u, par, dt)
    finally:
        s.close()
    # the limb-lane LQ kernels ran in two node ranges on two streams (a launch of 25 600 nodes is more than one round of the chip): the
    # same numbers, bit for bit, as one launch per kernel
    os.environ["HSQP_LQ_SPLIT"] = "1"
    try:
        s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    finally:
        os.environ.pop("HSQP_LQ_SPLIT", None)
    try:
        assert s.kernel_forms()["lq_ranges"] == 1
        one = s.run(x0, x, u, par, dt)
    finally:
        s.close()
    assert np.array_equal(one["dx"], out["dx"]) and np.array_equal(one["du"], out["du"])
    for b in list(range(0, B, 17)) + [255]:          # 17 instances spread over the batch (both node ranges of the LQ kernels, every XCD)
        r = oracle.sqp_iteration(dt, x0[b], x[b], u[b], par[b], threads=os.cpu_count() or 4)
        assert_step(out, r, b, "config 4")
        assert_perf(out["perf_before"][b], r["perf_before"], f"config 4 instance {b} before")
        assert_perf(out["perf_after"][b], r["perf_after"], f"config 4 instance {b} after")
    for b in range(B):
        assert_kkt(out["kkt"][b], out["grad_inf"][b], f"config 4 instance {b}")


def test_node_ranges_of_the_limb_lane_kernels_on_an_odd_shape(model):
    """173 instances x 97 nodes = 16 781 nodes = 525 workgroups of the limb-lane LQ kernels (more than one round of 512): the two node ranges on two streams
    (range boundary at node 8384, inside an instance; the last workgroup part padding) give bit for bit what one launch per kernel gives."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    B, N = 173, 97
    x0, x, u, par, dt = make_problem(model, n_nodes=N, batch=B, perturb=True, seed=3)
    outs = []
    for split in ("2", "1"):
        os.environ["HSQP_LQ_SPLIT"] = split
        try:
            s = HipSqpSolver(model, max_nodes=N, max_batch=B)
        finally:
            os.environ.pop("HSQP_LQ_SPLIT", None)
        try:
            assert s.kernel_forms()["lq_ranges"] == int(split)
            outs.append(s.run(x0, x, u, par, dt))
        finally:
            s.close()
    assert np.array_equal(outs[0]["dx"], outs[1]["dx"]) and np.array_equal(outs[0]["du"], outs[1]["du"])
    for b in range(B):
        assert_kkt(outs[0]["kkt"][b], outs[0]["grad_inf"][b], f"instance {b}")


@pytest.mark.parametrize("riccati", ["serial", "auto"])
def test_config3_exactly_against_the_oracle(model, oracle, riccati):
    """BASELINE config 3 as specified: whole-body, N = 100, ONE unperturbed instance, walk, cold start — against the CPU oracle at
    the BASELINE.md §6 tolerances, with the QP's KKT residuals judged against the STAGE gradients (|g|_inf = 0.7, so the bound is 1e-9
    absolute) like every other test.  riccati = "auto" is the default path: one instance on 100 nodes takes the parallel-in-time sweep
    (accepted by its KKT gate on this QP); its stationarity is 9.2e-10 — 0.92 of the bound (round 2: 1.07, and the test then judged it
    against the gradient of the projected QP, 38) —, the serial recursion's 3e-12."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    x0, x, u, par, dt = make_problem(model, n_nodes=100, batch=1, gait="walk")
    s = HipSqpSolver(model, max_nodes=100, max_batch=1, riccati=riccati)
    try:
        out = s.run(x0, x, u, par, dt)
        g = s.debug_read(_abi.BLK_G)
        fallbacks = s.scan_fallbacks()
    finally:
        s.close()
    r = oracle.sqp_iteration(dt, x0[0], x[0], u[0], par[0], threads=os.cpu_count() or 4)
    assert_step(out, r, 0, "config 3")
    assert_perf(out["perf_before"][0], r["perf_before"], "config 3 before")
    assert_perf(out["perf_after"][0], r["perf_after"], "config 3 after")
    assert_kkt(out["kkt"][0], np.abs(g[0]).max(), "config 3")
    assert out["alpha"][0] == 1.0 and out["step_type"][0] == _abi.STEP_FULL
    # The scan's stationarity on this QP sits at 0.8 of the gate's bound (tests/tolerances.py): a change of rounding upstream of the sweep may send the
    # iteration to the serial recursion.  What is asserted above is the GATED result — inside BASELINE.md §6 either way; the sweep that produced it
    # is reported, not required (round 5 review, item 8).  The serial handle never scans.
    assert fallbacks in ((0,) if riccati == "serial" else (0, 1)), fallbacks


@pytest.mark.parametrize("B,N,gait", [(3, 40, "walk"), (33, 100, "run"), (2, 1, "walk"), (2, 2, "walk"), (2, 3, "run"), (2, 5, "walk"), (2, 6, "run"), (2, 7, "walk")])
def test_factored_serial_sweep_equals_the_dense_stage_on_the_device(model, B, N, gait):
    """k_riccati_fact (csrc/hsqp_riccati_fact.h: the whole-body serial sweep on the factors of [A~ | B~], what every whole-body handle runs) against
    the dense stage k_riccati<58> (HSQP_RICCATI_DENSE in the environment at hsqp_create) on the same device, same inputs: the same minimiser to
    1e-9 of the step's scale (the yardstick of the randomly perturbed population, tests/tolerances.py: two correct f64 sweeps of the ill-conditioned
    run-gait QPs — |step| 1e3 — differ by 1.5e-10 of scale; on the walk problems by 1e-11), and bit-identical whether or not the joint rows of A~ / B~ are written (with the KKT report k_project writes them,
    without it does not: the factored sweep may not read them).  The short horizons cover the roll-out's groups of three stages (N % 3 = 0, 1, 2; fewer stages than
    register sets) and the backward sweep without a successor stage."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    x0, x, u, par, dt = make_problem(model, n_nodes=N, batch=B, gait=gait, perturb=True, seed=77)
    outs = {}
    for name in ("dense", "fact"):
        if name == "dense":
            os.environ["HSQP_RICCATI_DENSE"] = "1"
        try:
            s = HipSqpSolver(model, max_nodes=N, max_batch=B, riccati="serial")
        finally:
            os.environ.pop("HSQP_RICCATI_DENSE", None)
        try:
            assert s.kernel_forms()["ric_fact"] == (name == "fact")
            s.upload(x0, x, u, par, dt)
            s.iterate(1, take_step=False, kkt=False)
            a = s.download()
            s.iterate(1, take_step=False, kkt=True)
            b = s.download()
            assert np.array_equal(a["dx"], b["dx"]) and np.array_equal(a["du"], b["du"]), name
            outs[name] = b
        finally:
            s.close()
    d, f = outs["dense"], outs["fact"]
    for i in range(B):
        sc = max(1.0, np.abs(d["dx"][i]).max(), np.abs(d["du"][i]).max())
        err = max(np.abs(d["dx"][i] - f["dx"][i]).max(), np.abs(d["du"][i] - f["du"][i]).max())
        assert err <= 1e-9 * sc, (i, err, sc)
        assert_kkt(f["kkt"][i], f["grad_inf"][i], f"factored sweep, instance {i}")


@pytest.mark.parametrize("B,N,gait", [(5, 37, "walk"), (3, 20, "run")])
def test_chain_fused_into_the_projection_equals_the_chain_kernel(model, B, N, gait):
    """Limb-lane handles: the RK4 chain of the columns of [A|B] inside k_project (project_node, chain: from the stage Jacobians REC_GS, on the waves that
    wait for the factorisation) against the chain in k_lq_chain with P6 / V6 through the LQ record (HSQP_LQ_CHAIN_SEPARATE at hsqp_create): the same
    function of the same numbers (lq_chain_column_pv, hsqp_lq.h), so the step is identical bit for bit."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    x0, x, u, par, dt = make_problem(model, n_nodes=N, batch=B, gait=gait, perturb=True, seed=91)
    outs = {}
    for name in ("separate", "fused"):
        os.environ["HSQP_LQ_LIMB_FORM"] = "1"
        if name == "separate":
            os.environ["HSQP_LQ_CHAIN_SEPARATE"] = "1"
        try:
            s = HipSqpSolver(model, max_nodes=N, max_batch=B, riccati="serial")
        finally:
            os.environ.pop("HSQP_LQ_LIMB_FORM", None)
            os.environ.pop("HSQP_LQ_CHAIN_SEPARATE", None)
        try:
            forms = s.kernel_forms()
            assert forms["lq_limb"] and forms["chain_fused"] == (name == "fused")
            s.upload(x0, x, u, par, dt)
            s.iterate(1, take_step=False, kkt=True)
            outs[name] = (s.download(), s.debug_read(_abi.BLK_AB)[0], s.debug_read(_abi.BLK_BVEC)[0])
        finally:
            s.close()
    (a, ab_a, b_a), (f, ab_f, b_f) = outs["separate"], outs["fused"]
    # (on a fused handle the debug read chains the columns on the HOST from the device's stage Jacobians — REC_PV does not exist there —, so the [A|B] blocks agree to
    #  rounding; the device-side results below are compared bit for bit)
    assert np.abs(ab_a - ab_f).max() <= 1e-13 * max(1.0, np.abs(ab_a).max()) and np.array_equal(b_a, b_f)
    assert np.array_equal(a["dx"], f["dx"]) and np.array_equal(a["du"], f["du"])
    for i in range(B):
        assert_kkt(f["kkt"][i], f["grad_inf"][i], f"fused chain, instance {i}")


def test_parallel_in_time_sweep_is_repeatable(model):
    """The scan's elimination is a pipeline over the waves of a workgroup (one wave eliminates M and posts the multipliers, seven apply
    them a chunk behind): a missing barrier or a mailbox race would show as run-to-run differences — twenty repeated solves of two
    instances (202 workgroups per level) must agree bit for bit."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    x0, x, u, par, dt = make_problem(model, n_nodes=100, batch=2, gait="walk", perturb=True)
    s = HipSqpSolver(model, max_nodes=100, max_batch=2)
    try:
        ref = s.run(x0, x, u, par, dt)
        for _ in range(20):
            out = s.run(x0, x, u, par, dt)
            assert np.array_equal(out["dx"], ref["dx"]) and np.array_equal(out["du"], ref["du"])
        assert s.scan_fallbacks() == 0
    finally:
        s.close()


def test_kkt_gate_sends_an_ill_conditioned_qp_back_to_the_serial_recursion(model):
    """A randomly perturbed run-gait QP (|du| ~ 1e3; tests/test_hostemu.py shows the scan 3e-8 of the step's scale off on its like) in
    the automatic range of the parallel-in-time sweep: the KKT gate rejects the scan's result and the iteration is redone with the
    serial recursion — the output equals the serial-only solver's bit for bit."""
    from test_oracle_lq import perturbed_problem
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    n = 60
    x0, x, u, par, dt = perturbed_problem(model, n, "run", seed=5)
    outs = {}
    for mode in ("auto", "serial"):
        s = HipSqpSolver(model, max_nodes=n, max_batch=1, riccati=mode)
        try:
            outs[mode] = s.run(x0, x, u, par, dt)
            outs[mode]["fallbacks"] = s.scan_fallbacks()
        finally:
            s.close()
    assert outs["auto"]["fallbacks"] == 1 and outs["serial"]["fallbacks"] == 0
    for key in ("dx", "du", "x", "u"):
        assert np.array_equal(outs["auto"][key], outs["serial"][key]), key
    assert outs["auto"]["perf_after"][0] == outs["serial"]["perf_after"][0]


@pytest.mark.parametrize("n,batch", [(100, 1), (100, 2), (37, 3)])
def test_whole_body_parallel_in_time_sweep_against_the_serial_recursion(model, n, batch):
    """The whole-body backward sweep as an associative scan over the stages (hsqp_scan.h at n = 58: k_scan_init / k_scan_combine /
    k_scan_gains / k_scan_forward) against k_riccati<58> on the same QPs, BASELINE config 3 among them (where it is chosen
    automatically; batch 3 forces it beyond its automatic range).  DECLARED TOLERANCE: the scan inverts I + C1 J2 of two partial
    horizons, whose condition number reaches 1e9 on this problem; on these cold-start QPs its step agrees with the serial recursion's
    to 1.5e-11 .. 7e-11 of the step's scale (measured; 4.5e-9 absolute on config 3, 1.4e-8 on a perturbed instance with |du| = 200).
    Asserted: 2e-10 of the step's scale, the KKT residual of the QP at BASELINE.md §6, the performance index of the stepped
    trajectory to 1e-9 relative, and that the KKT gate accepted the scan (no fallback to the serial recursion)."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    x0, x, u, par, dt = make_problem(model, n_nodes=n, batch=batch, gait="walk", perturb=batch > 1)
    outs, fallbacks = {}, {}
    for mode in ("serial", "parallel"):
        s = HipSqpSolver(model, max_nodes=n, max_batch=batch, riccati=mode)
        try:
            outs[mode] = s.run(x0, x, u, par, dt)
            fallbacks[mode] = s.scan_fallbacks()
            ms = s.kernel_ms()
            print(f"N={n} B={batch} {mode}: sweep {ms['riccati']:.3f} ms of {ms['total']:.3f}")
        finally:
            s.close()
    a, b = outs["serial"], outs["parallel"]
    assert fallbacks["parallel"] == 0 and fallbacks["serial"] == 0      # the cold-start QPs pass the KKT gate
    for i in range(batch):
        sc = max(1.0, np.abs(a["dx"][i]).max(), np.abs(a["du"][i]).max())
        err = max(np.abs(a["dx"][i] - b["dx"][i]).max(), np.abs(a["du"][i] - b["du"][i]).max())
        print(f"N={n} B={batch} instance {i}: scan vs serial {err:.3e} = {err / sc:.2e} of the step's scale {sc:.3g}, kkt {b['kkt'][i]}")
        assert err <= 2e-10 * sc, f"instance {i}: scan vs serial {err:.3e} = {err / sc:.2e} of the step's scale {sc:.3g}"
        assert_kkt(b["kkt"][i], b["grad_inf"][i], f"scan, instance {i}")     # what the gate checks (gradient of the projected QP)
        assert_perf(b["perf_after"][i], a["perf_after"][i], f"scan vs serial, instance {i}", rel=1e-9)
    assert np.all(b["alpha"] == 1.0)


def test_config5_slice_against_the_oracle(model, oracle):
    """BASELINE config 5 (N = 200 long horizon, slow_walk, 6-DoF contact constraints as scheduled, perturbed instances): the first
    8 of its 1024 instances against the CPU oracle at full horizon length."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    B, N = 8, 200
    x0, x, u, par, dt = make_problem(model, n_nodes=N, batch=B, gait="slow_walk", perturb=True)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    try:
        out = s.run(x0, x, u, par, dt)
        g = s.debug_read(_abi.BLK_G)
        ne = s.debug_read(_abi.BLK_NE)
    finally:
        s.close()
    assert set(np.unique(ne)) <= {12, 13} and 12 in ne and 13 in ne      # double and single support both occur
    for b in range(B):
        r = oracle.sqp_iteration(dt, x0[b], x[b], u[b], par[b], threads=os.cpu_count() or 4)
        assert_step(out, r, b, "config 5")
        assert_perf(out["perf_before"][b], r["perf_before"], f"config 5 instance {b} before")
        assert_perf(out["perf_after"][b], r["perf_after"], f"config 5 instance {b} after")
        assert_kkt(out["kkt"][b], np.abs(g[b]).max(), f"config 5 instance {b}")


def test_edge_sizes_and_settings_errors(model, oracle):
    """Smallest problem (one interval, one instance), handle capacity limits, invalid line-search settings, a reference whose
    schedule ends in the air (the reference's swing planner throws there)."""
    from wb_humanoid_mpc_amd.reference import pack_reference, swing_config, ModeSchedule, TargetTrajectories
    from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError
    s = HipSqpSolver(model, max_nodes=3, max_batch=2)
    try:
        x0, x, u, par, dt = make_problem(model, n_nodes=1, batch=1, perturb=True, seed=4)
        out = s.run(x0, x, u, par, dt)
        r = oracle.sqp_iteration(dt, x0[0], x[0], u[0], par[0])
        assert_step(out, r, 0, "N = 1")
        with pytest.raises(HsqpError) as e:                                # batch larger than the handle
            s.run(*make_problem(model, n_nodes=2, batch=3))
        assert e.value.code == _abi.ERR_BAD_ARG
        for bad in ({"alpha_decay": 1.5}, {"alpha_min": 0.0}, {"g_max": 1e-9, "g_min": 1e-3}):
            with pytest.raises(HsqpError) as e:
                s.set_linesearch(**bad)
            assert e.value.code == _abi.ERR_BAD_ARG
        with pytest.raises(ValueError):
            s.set_linesearch(no_such_setting=1.0)
        # a schedule that ends in flight has no touch-down for the last swing phase
        x0, x, u, par, dt = make_problem(model, n_nodes=3, batch=1)
        sched = ModeSchedule([0.0, 0.05], [3, 2, 0])                      # STANCE, LF, FLY
        tgt = TargetTrajectories([0.0], [par[0, 0, :_abi.NX]])
        with pytest.raises(HsqpError) as e:
            s.upload_reference(x0, x, u, dt, 0.0, *pack_reference([sched], [tgt]), swing_config(model))
        assert e.value.code == _abi.ERR_BAD_ARG
    finally:
        s.close()


def test_receding_horizon_loop_with_device_parameters(model):
    """A short closed MPC loop the way the reference runs it (advanceMpc every control tick): device-generated parameters
    for the shifted grid, warm start from the previous solution (shifted by one node, tail repeated), one SQP iteration with
    line search, policy evaluation.  The constraint violation at the start of every cycle keeps falling (one real-time
    iteration per cycle), and everything stays finite."""
    from wb_humanoid_mpc_amd.reference import pack_reference, swing_config
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    B, N = 2, 20
    x0, x, u, par, dt, (schedules, targets, t0) = make_problem(model, n_nodes=N, batch=B, perturb=True, seed=12, with_reference=True)
    ref = pack_reference(schedules, targets)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    try:
        viol = []
        for cycle in range(4):
            s.upload_reference(x0, x, u, dt, t0 + cycle * dt, *ref, swing_config(model))
            s.iterate(1, take_step=True, linesearch=True)
            out = s.download()
            assert np.all(np.isfinite(out["x"])) and np.all(np.isfinite(out["u"])) and np.all(out["alpha"] > 0.0)
            viol.append([np.sqrt(p["dynamics_sse"] + p["equality_sse"]) for p in out["perf_before"]])
            xp, up, tau = s.evaluate_policy(np.full(B, 0.005))
            assert np.all(np.isfinite(tau)) and np.abs(tau).max() < 500.0
            # next cycle: the plant follows the plan for one node; warm start = shifted solution
            x0 = out["x"][:, 1].copy()
            x = np.concatenate([out["x"][:, 1:], out["x"][:, -1:]], axis=1)
            u = np.concatenate([out["u"][:, 1:], out["u"][:, -1:]], axis=1)
        viol = np.array(viol)
        assert np.all(viol[1:] < viol[:-1]) and np.all(viol[-1] < 0.6 * viol[0])
    finally:
        s.close()


def test_until_converged_runs_the_iterations_of_repeated_single_calls(model):
    """HSQP_ITER_UNTIL_CONVERGED (sqpIteration > 1 in ONE device call): the same trajectory, iteration log and count as
    driving single iterations from the host and applying ocs2's step-size test there; a generous deltaTol ends the loop early."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    x0, x, u, par, dt = make_problem(model, n_nodes=12, batch=3, gait="stance", perturb=True, seed=5)
    s = HipSqpSolver(model, max_nodes=12, max_batch=3)
    try:
        s.upload(x0, x, u, par, dt)
        n = s.iterate(4, take_step=True, kkt=True, linesearch=True, until_converged=True)
        assert n == 4                                  # far from converged at deltaTol = 1e-4
        out = s.download()
        logs = [s.iteration_log(i) for i in range(n)]
        # the same through single-iteration calls with a host round trip in between
        xs, us = x.copy(), u.copy()
        for i in range(n):
            s.upload(x0, xs, us, par, dt)
            s.iterate(1, take_step=True, kkt=True, linesearch=True)
            o = s.download()
            xs, us = o["x"], o["u"]
            assert np.array_equal(logs[i][1], o["alpha"]) and np.array_equal(logs[i][2], o["step_type"])
            assert all(abs(logs[i][0][b]["cost"] - o["perf_after"][b]["cost"]) <= 1e-9 * max(1.0, abs(o["perf_after"][b]["cost"])) for b in range(3))
        assert np.array_equal(out["x"], xs) and np.array_equal(out["u"], us)
        # early exit: with a huge deltaTol every instance is "converged" after the first iteration
        s.set_linesearch(delta_tol=1e6)
        s.upload(x0, x, u, par, dt)
        assert s.iterate(5, take_step=True, linesearch=True, until_converged=True) == 1
        with pytest.raises(Exception):
            s.iteration_log(1)
    finally:
        s.close()


def test_update_weights_equals_a_handle_created_with_them(model):
    """hsqp_update_weights (the gains receiver's hook): a live handle whose Q / R / Qf were replaced solves like a
    handle created with those weights."""
    import copy
    from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError
    x0, x, u, par, dt = make_problem(model, n_nodes=10, batch=2, perturb=True, seed=9)
    Q = np.array(model.desc.Q) * np.linspace(0.5, 2.0, _abi.NX)
    R = np.array(model.desc.R) * 3.0
    Qf = np.array(model.desc.Qf) * 0.25
    s = HipSqpSolver(model, max_nodes=10, max_batch=2)
    try:
        base = s.run(x0, x, u, par, dt)
        s.update_weights(Q, R, Qf)
        got = s.run(x0, x, u, par, dt)
        with pytest.raises(HsqpError):
            s.update_weights(Q=-Q)
    finally:
        s.close()
    m2 = copy.copy(model)
    m2.desc = type(model.desc).from_buffer_copy(model.desc)
    m2.desc.Q[:], m2.desc.R[:], m2.desc.Qf[:] = Q.tolist(), R.tolist(), Qf.tolist()
    s2 = HipSqpSolver(m2, max_nodes=10, max_batch=2)
    try:
        want = s2.run(x0, x, u, par, dt)
    finally:
        s2.close()
    assert np.array_equal(got["dx"], want["dx"]) and np.array_equal(got["du"], want["du"])
    assert not np.array_equal(got["dx"], base["dx"])


SEG_REL = 1e-9   # declared relaxation of the OPT-IN two-level sweep: measured 4e-11 .. 4e-10 of the step's scale from the serial recursion (include/hsqp.h)


@pytest.mark.parametrize("B,N,seed", [(3, 28, 77), (32, 100, 3), (32, 100, 1), (16, 60, 77), (8, 100, 77)])
def test_two_level_sweep_against_the_serial_recursion(model, oracle, B, N, seed):
    """The opt-in segmented (two-level) sweep of hsqp_segment.h (HSQP_FLAG_SEGMENTED_RICCATI; BASELINE config 4 as written puts 32 instances on
    each of 8 GPUs): the step within SEG_REL of its scale of the serial recursion's (seed 1 is the worst batch of tools/gpu_seg_fuzz.py:
    3.6e-10 when it passes the gate, which it does or does not by a hair), the same performance index, the KKT residual of the QP at the gate's
    bound, no fallback on the other walk-gait batches, bit-repeatable;
    one instance of the small case also against the oracle."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    x0, x, u, par, dt = make_problem(model, n_nodes=N, batch=B, perturb=True, seed=seed)
    outs = {}
    for md in ("serial", "segmented", "again"):
        s = HipSqpSolver(model, max_nodes=N, max_batch=B, riccati="serial" if md == "serial" else "segmented")
        try:
            s.upload(x0, x, u, par, dt)
            s.iterate(1, take_step=True, kkt=True)
            outs[md] = s.download()
            outs[md]["fallbacks"] = s.scan_fallbacks()
            outs[md]["backoffs"] = s.scan_backoffs()
        finally:
            s.close()
    a, b = outs["serial"], outs["segmented"]
    assert np.array_equal(b["dx"], outs["again"]["dx"]) and np.array_equal(b["du"], outs["again"]["du"])     # no atomics, fixed combine order
    assert b["backoffs"] == 0          # a FORCED sweep is attempted every iteration
    # What holds whatever the gate decided: the step within SEG_REL of its scale of the serial recursion's.  (The gate sits where the populations
    # separate — DESIGN.md §6: about one perturbed 32-instance batch in five has an instance whose boundary-stage KKT residual crosses it; a rejected
    # sweep is redone with the serial recursion and is then its result bit for bit, so the bound below covers both outcomes with ONE assertion.)
    sc = max(1.0, np.abs(a["dx"]).max(), np.abs(a["du"]).max())
    err = max(np.abs(a["dx"] - b["dx"]).max(), np.abs(a["du"] - b["du"]).max())
    print(f"two-level sweep B={B} N={N} seed {seed}: |step - serial| = {err:.2e} ({err / sc:.1e} of the scale), KKT {b['kkt'].max():.1e} (serial {a['kkt'].max():.1e}), fallbacks {b['fallbacks']}")
    assert err <= SEG_REL * sc
    assert b["fallbacks"] <= (1 if (B, seed) == (32, 1) else 0)       # no fallback on the other batches
    assert np.array_equal(a["dx"], b["dx"]) == (b["fallbacks"] == 1)  # the other algorithm unless the gate sent the iteration back
    for i in range(B):
        assert b["kkt"][i].max() <= 1e-7, f"instance {i}: KKT residual {b['kkt'][i].max():.2e} passed the gate"
        assert_perf(b["perf_after"][i], a["perf_after"][i], f"instance {i}", rel=1e-9)
    if B <= 4:
        r = oracle.sqp_iteration(dt, x0[1], x[1], u[1], par[1], threads=os.cpu_count() or 4)
        assert_step(b, r, 1, "two-level sweep vs oracle", rel=SEG_REL)    # the declared relaxation of the opt-in sweep


def test_two_level_sweep_gate_rejects_a_badly_scaled_batch(cmodel):
    """A perturbed centroidal batch (|S| ~ 4e6: the combination of its segment elements loses digits) fails the gate — the KKT residual of the
    segments' last stages —, and every iteration is redone with the serial recursion (bit for bit the serial handle's result)."""
    from wb_humanoid_mpc_amd.reference import make_centroidal_problem
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    B, N = 8, 100
    x0, x, u, par, dt = make_centroidal_problem(cmodel, n_nodes=N, batch=B, perturb=True)
    res = {}
    for md in ("serial", "segmented"):
        s = HipSqpSolver(cmodel, max_nodes=N, max_batch=B, riccati=md)
        try:
            s.upload(x0, x, u, par, dt)
            for _ in range(6):
                s.iterate(1)
            s.iterate(1, kkt=True)
            res[md] = (s.download(), s.scan_fallbacks())
        finally:
            s.close()
    # riccati="segmented" FORCES the sweep: it is attempted (and rejected) in every one of the seven iterations — the back-off belongs to the
    # automatic sweep choice only, see test_scan_back_off_is_per_problem_and_only_for_the_automatic_choice
    assert res["serial"][1] == 0 and res["segmented"][1] == 7
    assert np.array_equal(res["segmented"][0]["dx"], res["serial"][0]["dx"]) and np.array_equal(res["segmented"][0]["du"], res["serial"][0]["du"])


def test_page_locked_caller_buffers_give_the_same_solution(model):
    """hsqp_host_register / hsqp_host_unregister (include/hsqp.h): hsqp_solve on page-locked caller buffers returns bit for bit what it returns
    on pageable ones; an empty buffer is an error code, not a crash."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError
    x0, x, u, par, dt = make_problem(model, n_nodes=12, batch=3, perturb=True)
    s = HipSqpSolver(model, max_nodes=12, max_batch=3)
    try:
        want = s.run(x0, x, u, par, dt)
        want = {k: np.array(want[k]) for k in ("x", "u", "dx", "du")}
        arrs = [np.ascontiguousarray(a) for a in (x0, x, u, par)]
        into = s.alloc_solution(3, 12)
        bufs = arrs + [into[1][k] for k in ("x", "u", "dx", "du")]
        s.pin(*bufs)
        got = s.run(*arrs, dt, into=into)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        s.unpin(*bufs)
        with pytest.raises(HsqpError):
            s.pin(np.zeros(0))          # nothing to lock: BAD_ARG, not a crash
    finally:
        s.close()


def test_update_term_weights_equals_a_handle_created_with_them(model):
    """hsqp_update_term_weights (what the reference's other gains updaters retune — foot-cost weights, foot-constraint
    gains, barrier parameters): a live handle whose term weights were replaced solves like a handle created with them; an invalid set is
    rejected by the model validation of hsqp_create and leaves the handle unchanged."""
    import copy
    from wb_humanoid_mpc_amd.solver import HipSqpSolver, HsqpError
    x0, x, u, par, dt = make_problem(model, n_nodes=10, batch=2, perturb=True, seed=9)
    s = HipSqpSolver(model, max_nodes=10, max_batch=2)
    try:
        base = s.run(x0, x, u, par, dt)
        w = s.term_weights()
        assert list(w.foot_sqrt_w) == list(model.desc.foot_sqrt_w) and w.gain_linvel_z == model.desc.gain_linvel_z
        for i in range(18):
            w.foot_sqrt_w[i] *= 1.5
        w.gain_pos_z, w.gain_linvel_xy, w.gain_angacc = 2.0 * w.gain_pos_z, 0.5 * w.gain_linvel_xy, 1.25 * w.gain_angacc
        w.friction_barrier.mu *= 0.5
        w.moment_barrier.delta *= 2.0
        w.joint_limit_barrier.mu *= 3.0
        s.update_term_weights(w)
        got = s.run(x0, x, u, par, dt)
        bad = s.term_weights()
        bad.friction_barrier.mu = 0.0
        with pytest.raises(HsqpError):
            s.update_term_weights(bad)
        again = s.run(x0, x, u, par, dt)
    finally:
        s.close()
    # ... and hsqp_create applies the SAME validation (it used to accept what the updaters reject): a relaxed barrier with mu = 0, a
    # non-positive input weight and a NaN gain are refused; a piecewise-polynomial penalty switched off with mu = 0 is a valid model
    for field, value in (("friction_barrier.mu", 0.0), ("moment_barrier.delta", -1.0), ("gain_ori", float("nan"))):
        mb = copy.copy(model)
        mb.desc = type(model.desc).from_buffer_copy(model.desc)
        obj, name = mb.desc, field
        while "." in name:
            head, name = name.split(".", 1)
            obj = getattr(obj, head)
        setattr(obj, name, value)
        with pytest.raises(HsqpError):
            HipSqpSolver(mb, max_nodes=4, max_batch=1)
    mb = copy.copy(model)
    mb.desc = type(model.desc).from_buffer_copy(model.desc)
    mb.desc.R[3] = 0.0
    with pytest.raises(HsqpError):
        HipSqpSolver(mb, max_nodes=4, max_batch=1)
    mb.desc.R[3] = model.desc.R[3]
    mb.desc.collision_barrier.mu = 0.0
    HipSqpSolver(mb, max_nodes=4, max_batch=1).close()
    m2 = copy.copy(model)
    m2.desc = type(model.desc).from_buffer_copy(model.desc)
    for i in range(18):
        m2.desc.foot_sqrt_w[i] *= 1.5
    m2.desc.gain_pos_z, m2.desc.gain_linvel_xy, m2.desc.gain_angacc = 2.0 * model.desc.gain_pos_z, 0.5 * model.desc.gain_linvel_xy, 1.25 * model.desc.gain_angacc
    m2.desc.friction_barrier.mu *= 0.5
    m2.desc.moment_barrier.delta *= 2.0
    m2.desc.joint_limit_barrier.mu *= 3.0
    s2 = HipSqpSolver(m2, max_nodes=10, max_batch=2)
    try:
        want = s2.run(x0, x, u, par, dt)
    finally:
        s2.close()
    assert np.array_equal(got["dx"], want["dx"]) and np.array_equal(got["du"], want["du"])
    assert np.array_equal(again["dx"], got["dx"])
    assert not np.array_equal(got["dx"], base["dx"])


def test_scan_back_off_is_per_problem_and_only_for_the_automatic_choice(model, oracle):
    """the gate's back-off (after a rejected parallel-in-time sweep the next 1, 3, 7, .. iterations go straight to the
    serial recursion) is state of the AUTOMATIC sweep choice: it works inside one multi-iteration call, is reset by every upload, is
    counted (hsqp_scan_backoffs) and never applies to a sweep forced by a flag."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    N = 100
    x0, x, u, par, dt = make_problem(model, n_nodes=N, batch=1, gait="walk")
    counts = {}
    for md in ("auto", "parallel"):
        s = HipSqpSolver(model, max_nodes=N, max_batch=1, linesearch=True, riccati=md)
        try:
            s.upload(x0, x, u, par, dt)
            s.iterate(4, take_step=True, linesearch=True)     # iterate 1 passes the gate, the far-from-feasible iterates after it do not
            first = (s.scan_fallbacks(), s.scan_backoffs())
            s.upload(x0, x, u, par, dt)                        # the same problem again: same decisions, whatever the handle did before
            s.iterate(4, take_step=True, linesearch=True)
            counts[md] = (first, (s.scan_fallbacks() - first[0], s.scan_backoffs() - first[1]))
        finally:
            s.close()
    (a1, a2), (p1, p2) = counts["auto"], counts["parallel"]
    assert a1 == a2 and p1 == p2, counts                       # per problem, not per handle history
    assert a1[0] >= 1 and a1[1] >= 1 and a1[0] + a1[1] <= 3, counts   # rejected, then backed off
    assert p1[1] == 0 and p1[0] >= a1[0], counts               # forced: attempted every time


def test_scan_back_off_can_persist_over_the_cycles_of_a_receding_horizon(model):
    """ocs2's MPC_BASE::run uploads the shifted problem every cycle and runs ONE iteration; with the back-off reset by every
    upload a regime whose iterates fail the KKT gate paid the rejected parallel-in-time sweep in every cycle.  hsqp_set_scan_backoff_persistent
    (host/HipSqpSolver.h switches it on) keeps the back-off over uploads of the same shape: the same four 'cycles' (upload + iterations from a
    far-from-feasible iterate) attempt the scan less often and back off instead; the solutions are those of the serial recursion either way."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    N = 100
    x0, x, u, par, dt = make_problem(model, n_nodes=N, batch=1, gait="walk")
    counts, sols = {}, {}
    for persistent in (False, True):
        s = HipSqpSolver(model, max_nodes=N, max_batch=1, linesearch=True, riccati="auto")
        try:
            if persistent:
                s.set_scan_backoff_persistent(True)
            s.upload(x0, x, u, par, dt)
            s.iterate(2, take_step=True, linesearch=True)      # leaves a far-from-feasible iterate: the next sweeps fail the gate
            xs, us = s.download()["x"], s.download()["u"]
            f0, b0 = s.scan_fallbacks(), s.scan_backoffs()
            for _ in range(4):                                  # four cycles from that iterate: upload, one iteration
                s.upload(x0, xs, us, par, dt)
                s.iterate(1, take_step=False, linesearch=True)
            counts[persistent] = (s.scan_fallbacks() - f0, s.scan_backoffs() - b0)
            sols[persistent] = s.download()["dx"].copy()
        finally:
            s.close()
    assert counts[False][1] == 0 and counts[False][0] >= 3, counts          # per problem: every cycle pays scan + fallback
    assert counts[True][1] >= 2 and counts[True][0] < counts[False][0], counts   # persistent: backs off over the cycles
    assert np.array_equal(sols[False], sols[True])                             # the serial recursion's step in both runs


def test_value_pass_on_quads_of_lanes_equals_the_phase_form(model):
    """The whole-body value pass (performance index of the stepped trajectory, line-search trials) runs on quads of lanes — a lane per limb,
    16 nodes per wave (hsqp_lqv.h) — for handles sized to fill the GPU; HSQP_VALUE_PHASE_FORM / HSQP_VALUE_QUAD_FORM at hsqp_create force its phase form (one wave per
    node, fused with the step) / the quad form.  Same
    numbers up to the order of the sums over bodies and cost terms; the step itself is bit-identical.  A batch whose node count is not a multiple
    of 16 (padding quads) and a line-search run (masked instances) are part of the case."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    res = {"quad": [], "phase": []}
    x0, x, u, par, dt = make_problem(model, n_nodes=37, batch=5, perturb=True, seed=21)
    for form in ("quad", "phase"):
        for linesearch in (False, True):
            key = "HSQP_VALUE_PHASE_FORM" if form == "phase" else "HSQP_VALUE_QUAD_FORM"   # (a handle this small would take the phase form by itself)
            os.environ[key] = "1"
            try:
                s = HipSqpSolver(model, max_nodes=37, max_batch=5, linesearch=linesearch)
            finally:
                os.environ.pop(key, None)
            try:
                res[form].append(s.run(x0, x, u, par, dt))
            finally:
                s.close()
    for a, b in zip(res["quad"], res["phase"]):
        assert np.array_equal(a["dx"], b["dx"]) and np.array_equal(a["du"], b["du"])
        assert np.array_equal(a["alpha"], b["alpha"]) and np.array_equal(a["step_type"], b["step_type"])
        assert np.array_equal(a["x"], b["x"]) and np.array_equal(a["u"], b["u"])
        for pa, pb in zip(a["perf_after"], b["perf_after"]):
            for key in ("cost", "dynamics_sse", "equality_sse"):
                assert abs(pa[key] - pb[key]) <= 1e-12 * max(1.0, abs(pb[key])), (key, pa, pb)


def _poisoned_and_clean(model, make, **solver_kw):
    """Two solves of the same problem: on a handle created with HSQP_POISON_LDS (every kernel launch preceded by one that fills the LDS of every
    CU with NaN bit patterns: csrc/hsqp_capi.hip, k_poison_lds) and on a clean one (the flags are read at hsqp_create and belong to the handle)."""
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    outs = []
    for poison in (True, False):
        if poison:
            os.environ["HSQP_POISON_LDS"] = "1"
            os.environ["HSQP_POISON_HBM"] = "1"   # ... and every device buffer the library allocates starts as NaN patterns instead of the allocator's zeros
        try:
            s = HipSqpSolver(model, **solver_kw)
        finally:
            os.environ.pop("HSQP_POISON_LDS", None)
            os.environ.pop("HSQP_POISON_HBM", None)
        try:
            outs.append([s.run(*p) for p in make()])
        finally:
            s.close()
    return outs


@pytest.mark.parametrize("form", ["serial", "dense_stage", "limb_lanes", "linesearch", "parallel", "segmented"])
def test_no_kernel_reads_lds_it_did_not_write(model, form):
    """LDS keeps what the previous kernel left in it.  A kernel that reads a word it never wrote — the padding row of an operand that is `multiplied
    by zero`, the tail of a union — works until the leftover is a NaN: the serial sweep's Ph4 did exactly that (row NUT of Zs beyond SB's storage)
    and failed about one run in ten with `reduced Hessian not positive definite`.  With NaN patterns in every LDS word in front of every launch the
    iteration has to give the same bits as without."""
    kw = dict(max_nodes=100, max_batch=4)
    env = None
    if form == "limb_lanes":
        env = "HSQP_LQ_LIMB_FORM"
    elif form == "dense_stage":
        env = "HSQP_RICCATI_DENSE"
        kw["riccati"] = "serial"
    elif form == "linesearch":
        kw["linesearch"] = True
    elif form in ("parallel", "segmented"):
        kw["riccati"] = form
    else:
        kw["riccati"] = "serial"

    def make():
        return [make_problem(model, n_nodes=n, batch=b, gait=g, perturb=True, seed=5 + n) for n, b, g in ((100, 2, "walk"), (37, 4, "run"), (8, 1, "stance"))]
    if env:
        os.environ[env] = "1"
    try:
        poisoned, clean = _poisoned_and_clean(model, make, **kw)
    finally:
        if env:
            os.environ.pop(env, None)
    for a, b in zip(poisoned, clean):
        for key in ("dx", "du", "x", "u", "kkt"):
            assert np.isfinite(a[key]).all(), (form, key)
            assert np.array_equal(a[key], b[key]), (form, key)


def test_raw_qp_block_is_refused_when_k_project_skipped_the_joint_rows(model):
    """Debug block 102 hands out the raw QP record of the last iteration.  Without a KKT report the whole-body serial sweep on the factors has
    k_project skip the joint rows of A~ / B~ and the lower triangle of Q~ (csrc/hsqp_project.h, QP_A): they keep what was there before, so the
    block is refused.  After an iteration that wrote them it is returned, and its A~ is the one of the dense stage's handle (which always
    writes them)."""
    import ctypes as C
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    B, N = 2, 20
    problem = make_problem(model, n_nodes=N, batch=B, gait="walk", perturb=True, seed=3)

    def raw_qp(s):
        size = s.lib.hsqp_debug_read(s.h, 102, None, 0)
        assert size > 0 and size % (B * N * 8) == 0, size
        qp = np.full(size // 8, np.nan)
        assert s.lib.hsqp_debug_read(s.h, 102, qp.ctypes.data_as(C.c_void_p), qp.nbytes) == size
        return qp.reshape(B * N, -1)

    s = HipSqpSolver(model, max_nodes=N, max_batch=B, riccati="serial")
    try:
        assert s.kernel_forms()["ric_fact"]
        s.upload(*problem)
        s.iterate(kkt=False)
        assert s.lib.hsqp_debug_read(s.h, 102, None, 0) == _abi.ERR_BAD_ARG
        assert "joint rows" in s.lib.hsqp_last_error(s.h).decode()
        s.iterate(kkt=True)
        fact = raw_qp(s)
    finally:
        s.close()
    os.environ["HSQP_RICCATI_DENSE"] = "1"
    try:
        s = HipSqpSolver(model, max_nodes=N, max_batch=B, riccati="serial")
    finally:
        os.environ.pop("HSQP_RICCATI_DENSE", None)
    try:
        assert not s.kernel_forms()["ric_fact"]
        s.upload(*problem)
        s.iterate(kkt=False)
        dense = raw_qp(s)
    finally:
        s.close()
    A = slice(0, _abi.NX * _abi.NX)
    assert np.isfinite(fact[:, A]).all()
    assert np.array_equal(fact[:, A], dense[:, A])
