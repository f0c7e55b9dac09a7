"""The kernel forms bench.py times, on PER-INSTANCE event grids (tests/event_grid_cases.py), against the CPU oracle and against each other on the device.

hsqp_problem::dt_nodes is [B][N]; twelve kernels index it themselves.  Every other oracle comparison on an event grid shares ONE grid over the batch and
runs on handles of a few dozen nodes, which take the phase forms: here the limb-lane LQ kernels (16 nodes of different instances per wave), the RK4
chain fused into k_project, k_value_quad with its line-search mask, k_riccati_fact, the two node ranges with k_jump on an aux stream, the two-level
sweep and the scans meet grids that differ from instance to instance, dt = 0 runs of different lengths included.  The forms are forced with the
create-time switches the product already has; kernel_forms() is asserted on every handle.

Bounds (tests/tolerances.py; nothing is taken from the code under test).  Against the oracle: assert_step(rel=1e-10) = TRAJ_ABS + 1e-10 x the step's
scale, the form tests/test_event_nodes.py holds event grids to — the unrelaxed 1e-8 absolute has NO margin on this population (|step| up to 2e3: on the
MI355X the serial sweeps' worst absolute error is 4.0e-9, the accepted scan's 3.1e-8 = 4.6e-11 of the scale; on the host 6.3e-9) —, assert_perf at
PERF_REL, assert_kkt at KKT_REL.  No device result needed more than rel = 1e-10 (worst 4.6e-11 of the scale, the scan; serial sweeps 1.2e-11).  Form against form: the bounds of the tests in
tests/test_gpu_parity.py named in each docstring.  Worst measured values, host and device: profiles/event_forms_parity.txt.

Shapes: case A 5 x 18 nodes (walk and run), S 6 x 40, P 3 x 64, the centroidal twin 3 x 18, the node ranges 173 x 97."""
import os
import signal

import numpy as np
import pytest

import event_grid_cases as EG
from tolerances import PERF_REL, assert_kkt, assert_perf, assert_step
from wb_humanoid_mpc_amd import _abi
from wb_humanoid_mpc_amd.solver import HipSqpSolver

pytestmark = pytest.mark.gpu

NX = _abi.NX
ORACLE_REL = 1e-10      # of the step's scale on top of TRAJ_ABS (tests/test_event_nodes.py)
SEG_REL = 1e-9          # the declared relaxation of the opt-in two-level sweep (tests/test_gpu_parity.py)
TIMED = {"HSQP_LQ_LIMB_FORM": "1", "HSQP_VALUE_QUAD_FORM": "1", "HSQP_LQ_SPLIT": "1"}
TIMED_FORMS = {"lq_limb": True, "value_quad": True, "ric_fact": True, "chain_fused": True, "lq_ranges": 1}
PHASE = {"HSQP_LQ_PHASE_FORM": "1", "HSQP_VALUE_PHASE_FORM": "1"}
PHASE_FORMS = {"lq_limb": False, "value_quad": False, "ric_fact": True, "chain_fused": False, "lq_ranges": 0}
LQ_BLOCKS = ((_abi.BLK_AB, "AB"), (_abi.BLK_BVEC, "b"), (_abi.BLK_H, "H"), (_abi.BLK_G, "g"), (_abi.BLK_CDE, "CDe"), (_abi.BLK_COST, "cost"), (_abi.BLK_FLOW, "flow"))
STEP_KEYS = ("dx", "du", "x", "u")


@pytest.fixture(autouse=True)
def time_limit():
    def expired(signum, frame):
        raise TimeoutError("test_gpu_event_forms: a test ran past its 120 s limit")
    old = signal.signal(signal.SIGALRM, expired)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def create(model, switches, forms, **kw):
    """A handle with create-time switches in the environment around hsqp_create only; its kernel forms are asserted (a dict, or the keys given)."""
    for k, v in switches.items():
        os.environ[k] = v
    try:
        s = HipSqpSolver(model, **kw)
    finally:
        for k in switches:
            os.environ.pop(k, None)
    try:
        got = s.kernel_forms()
        assert {k: got[k] for k in forms} == forms, (switches, got)
    except BaseException:
        s.close()
        raise
    return s


def solve(s, prob):
    return s.run(prob.x0, prob.x, prob.u, prob.par, prob.dts)


def rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def scale_of(out):
    return max(1.0, np.abs(out["dx"]).max(), np.abs(out["du"]).max())


def step_diff(a, b):
    return max(np.abs(a["dx"] - b["dx"]).max(), np.abs(a["du"] - b["du"]).max())


def assert_events_keep_their_inputs(out, prob):
    for b in range(len(prob.dts)):
        assert not out["du"][b, EG.event_intervals(prob.dts[b])].any(), b


def assert_bits(a, b, keys=STEP_KEYS, what=""):
    for key in keys:
        assert np.array_equal(a[key], b[key]), (what, key)


def assert_against_oracle(out, oracle, prob, what, rel_step=ORACLE_REL, instances=None):
    """step, performance index before and after, KKT residual of the given instances (default: all) against the oracle on each instance's own grid;
    returns (worst step error / scale, worst absolute step error, worst relative performance-index error)"""
    worst = [0.0, 0.0, 0.0]
    for b in range(len(prob.dts)) if instances is None else instances:
        r = EG.oracle_iteration(oracle, prob, b)
        err, sc = EG.step_error(out, r, b), EG.step_scale(r)
        perf = max(abs(out[w][b][k] - r[w][k]) / abs(r[w][k]) for w in ("perf_before", "perf_after") for k in ("cost", "dynamics_sse", "equality_sse") if abs(r[w][k]) > 1e-3)
        print(f"  {what} instance {b}: step error {err:.2e} = {err / sc:.2e} of the scale {sc:.3g}, performance index {perf:.2e}, kkt {out['kkt'][b]}")
        worst = [max(worst[0], err / sc), max(worst[1], err), max(worst[2], perf)]
        assert_step(out, r, b, what, rel=rel_step)
        assert_perf(out["perf_before"][b], r["perf_before"], f"{what} instance {b} before")
        assert_perf(out["perf_after"][b], r["perf_after"], f"{what} instance {b} after", rel=PERF_REL if rel_step <= ORACLE_REL else 1e-9)
        assert_kkt(out["kkt"][b], out["grad_inf"][b], f"{what} instance {b}")
    return worst


@pytest.fixture(scope="module")
def timed(model):
    """The forms a handle sized to fill the GPU runs — limb-lane LQ kernels with the chain fused into k_project, value pass on quads of lanes, factored
    serial sweep — forced on a 5 x 18 handle, one node range."""
    s = create(model, TIMED, TIMED_FORMS, max_nodes=18, max_batch=5, riccati="serial")
    yield s
    s.close()


# ---------------------------------------------------------------------------------------------- 1. the timed forms against the oracle
@pytest.mark.parametrize("name", ["A_walk", "A_run"])
def test_timed_forms_on_per_instance_grids_against_the_oracle(timed, model, oracle, name):
    """Case A through the forced limb-lane / quad / factored handle: every instance's step, performance index (before, after) and KKT residual against
    the oracle on the instance's own grid; every LQ block at the 1e-11 of test_lq_blocks_of_the_limb_lane_form_against_oracle; on zero-length intervals
    [A|B] = [I|0], no cost, no equality rows, the defect x_k - x_k+1, du = 0 exactly.
    Measured on MI355X: step 4.9e-12 of the scale (2.8e-9 absolute), performance index 1.6e-11, LQ blocks 4.4e-15 (profiles/event_forms_parity.txt)."""
    prob = EG.case(model, name)
    out = solve(timed, prob)
    assert timed.kernel_forms() == TIMED_FORMS
    blocks = {key: timed.debug_read(blk) for blk, key in LQ_BLOCKS}
    ne = timed.debug_read(_abi.BLK_NE)
    worst = assert_against_oracle(out, oracle, prob, name)
    worst_blk = 0.0
    for b in range(len(prob.dts)):
        lq = EG.oracle_iteration(oracle, prob, b)["lq"]
        ev = EG.event_intervals(prob.dts[b])
        real = np.setdiff1d(np.arange(prob.dts.shape[1]), ev)
        for _, key in LQ_BLOCKS:
            # [A|B], the defect, the cost gradient, the equality rows and the cost on EVERY interval.  H and the flow on the intervals of non-zero length:
            # on a zero-length interval the oracle's block carries the jump stage's unit input weight (jump_node_lq: H_uu = I) and no flow, while the
            # device keeps that stage in its QP record (jump_node_qp) — its dt * Hessian there is 0 (asserted below), its flow nobody reads
            rows = real if key in ("H", "flow") else np.arange(lq[key].shape[0])
            e = rel(blocks[key][b][rows], lq[key][rows])
            worst_blk = max(worst_blk, e)
            assert e <= 1e-11, (name, b, key, e)
        assert np.array_equal(ne[b], lq["ne"]), (name, b)
        for k in ev:
            AB = blocks["AB"][b, k]
            assert np.array_equal(AB[:, :NX], np.eye(NX)) and not AB[:, NX:].any(), (name, b, k)
            assert blocks["cost"][b, k] == 0.0 and ne[b, k] == 0 and not blocks["H"][b, k].any() and not blocks["g"][b, k].any(), (name, b, k)
            assert np.array_equal(blocks["b"][b, k], prob.x[b, k] - prob.x[b, k + 1]), (name, b, k)
    assert_events_keep_their_inputs(out, prob)
    print(f"event forms {name} timed forms vs oracle: step {worst[0]:.2e} of the scale ({worst[1]:.2e} absolute), performance index {worst[2]:.2e}, LQ blocks {worst_blk:.2e}")


# ---------------------------------------------------------------------------------------------- 2. the batch axis
def test_batch_axis_of_the_timed_forms(timed, model):
    """Case A (walk) on the same handle: a permutation of the batch rows, dt_nodes included, returns the permuted result bit for bit; instance 3 alone
    equals its row bit for bit; and — the control — with every grid replaced by instance 0's the other instances' dx change: the test would see a kernel
    that reads another instance's row of dt_nodes.
    Measured on MI355X: instance 0's grid moves the other instances' dx by 1.3e-3 .. 8.4e-3 of the step's scale (the oracle's bound: 1e-10)."""
    prob = EG.case(model, "A_walk")
    out = solve(timed, prob)
    perm = np.array([3, 0, 4, 1, 2])
    got = solve(timed, EG.permuted(prob, perm))
    for key in STEP_KEYS:
        assert np.array_equal(got[key], out[key][perm]), key
    assert got["perf_after"] == [out["perf_after"][i] for i in perm]
    solo = timed.run(prob.x0[3], prob.x[3], prob.u[3], prob.par[3], prob.dts[3])
    for key in STEP_KEYS:
        assert np.array_equal(solo[key][0], out[key][3]), key
    assert solo["perf_after"][0] == out["perf_after"][3]
    shared = timed.run(prob.x0, prob.x, prob.u, prob.par, np.tile(prob.dts[0], (len(prob.dts), 1)))
    assert np.array_equal(shared["dx"][0], out["dx"][0])
    moved = [np.abs(shared["dx"][b] - out["dx"][b]).max() / scale_of(out) for b in range(1, len(prob.dts))]
    assert all(m > 1e3 * ORACLE_REL for m in moved), moved
    print(f"event forms batch axis: permutation and solo solve bit for bit; instance 0's grid moves the other instances' dx by {min(moved):.1e} .. {max(moved):.1e} of the scale")


# ---------------------------------------------------------------------------------------------- 3. limb / quad forms against the phase forms
@pytest.mark.parametrize("ls", [None, {}, {"gamma_c": 0.6}], ids=["full_step", "linesearch", "linesearch_gamma_c_0.6"])
def test_timed_forms_equal_the_phase_forms_on_per_instance_grids(model, oracle, ls):
    """Case A, walk and run, one iteration (full step; the filter line search at its default settings and at gamma_c = 0.6: back-tracking, masked
    instances in k_value_quad):
      * limb + quad handle against phase + phase handle: the step within 1e-10 of its scale and the performance index before the step within 1e-12
        (test_limb_lane_form_equals_the_phase_form), alpha and step type equal;
      * quad against phase value pass on the same limb-lane LQ kernels: step, alpha, step type and trajectory bit for bit, the performance index after
        the step within 1e-12 (test_value_pass_on_quads_of_lanes_equals_the_phase_form);
      * chain fused into k_project against k_lq_chain: bit for bit (test_chain_fused_into_the_projection_equals_the_chain_kernel);
      * with the line search, step length and step type against the oracle's line search and the accepted trajectory's performance index against
        oracle.performance, both on each instance's own grid (exactly, as test_filter_linesearch_against_oracle; PERF_REL).
    Measured on MI355X: limb against phase LQ kernels 5.6e-13 of the step's scale, performance index before the step 3.8e-16; quad against phase
    value pass 6.5e-16; accepted trial against the oracle 1.3e-15; default settings accept alpha = 1, 0.5 and 0.25 within one batch (instances leave
    the trial loop at different trials), gamma_c = 0.6 accepts no trial (alpha = 0) — as the oracle's line search does."""
    linesearch = ls is not None
    kw = dict(max_nodes=18, max_batch=5, riccati="serial", linesearch=linesearch)
    handles = {"timed": (TIMED, TIMED_FORMS), "phase": (PHASE, PHASE_FORMS),
               "value_phase": ({"HSQP_LQ_LIMB_FORM": "1", "HSQP_VALUE_PHASE_FORM": "1", "HSQP_LQ_SPLIT": "1"}, dict(TIMED_FORMS, value_quad=False)),
               "separate": (dict(TIMED, HSQP_LQ_CHAIN_SEPARATE="1"), dict(TIMED_FORMS, chain_fused=False))}
    outs = {}
    for hname, (switches, forms) in handles.items():
        s = create(model, switches, forms, **kw)
        try:
            if linesearch:
                s.set_linesearch(**ls)
            outs[hname] = {name: solve(s, EG.case(model, name)) for name in ("A_walk", "A_run")}
        finally:
            s.close()
    worst_step = worst_before = worst_after = worst_ls = 0.0
    for name in ("A_walk", "A_run"):
        prob = EG.case(model, name)
        t, p, v, c = (outs[h][name] for h in ("timed", "phase", "value_phase", "separate"))
        sc = scale_of(p)
        worst_step = max(worst_step, step_diff(t, p) / sc)
        assert np.abs(t["dx"] - p["dx"]).max() <= 1e-10 * sc and np.abs(t["du"] - p["du"]).max() <= 1e-10 * sc, (name, step_diff(t, p), sc)
        assert np.array_equal(t["alpha"], p["alpha"]) and np.array_equal(t["step_type"], p["step_type"]), (name, t["alpha"], p["alpha"])
        for a, b in zip(t["perf_before"], p["perf_before"]):
            for key in ("cost", "dynamics_sse", "equality_sse"):
                worst_before = max(worst_before, abs(a[key] - b[key]) / max(1.0, abs(b[key])))
                assert abs(a[key] - b[key]) <= 1e-12 * max(1.0, abs(b[key])), (name, key, a, b)
        assert_bits(t, v, STEP_KEYS + ("alpha", "step_type"), f"{name} quad vs phase value pass")
        for a, b in zip(t["perf_after"], v["perf_after"]):
            for key in ("cost", "dynamics_sse", "equality_sse"):
                worst_after = max(worst_after, abs(a[key] - b[key]) / max(1.0, abs(b[key])))
                assert abs(a[key] - b[key]) <= 1e-12 * max(1.0, abs(b[key])), (name, key, a, b)
        assert_bits(t, c, STEP_KEYS + ("alpha", "step_type"), f"{name} fused vs separate chain")
        assert_events_keep_their_inputs(t, prob)
        if linesearch:
            assert np.all(t["step_type"] != _abi.STEP_FULL)
            for b in range(len(prob.dts)):
                r = EG.oracle_iteration(oracle, prob, b)
                oracle.set_grid(prob.dts[b])
                try:
                    want = oracle.performance(0.0, t["x"][b], t["u"][b], prob.par[b], threads=4)
                    ref = oracle.linesearch(0.0, prob.x[b], prob.u[b], r["dx"], r["du"], prob.par[b], r["armijo"], threads=4, **ls)
                finally:
                    oracle.set_grid(None)
                assert t["alpha"][b] == ref["alpha"] and t["step_type"][b] == ref["step_type"], (name, b, t["alpha"][b], t["step_type"][b], ref["alpha"], ref["step_type"])
                worst_ls = max(worst_ls, max(abs(t["perf_after"][b][k] - want[k]) / abs(want[k]) for k in ("cost", "dynamics_sse", "equality_sse") if abs(want[k]) > 1e-3))
                assert_perf(t["perf_after"][b], want, f"{name} instance {b} accepted trial (alpha {t['alpha'][b]})")
            print(f"  {name}: alpha {t['alpha']}")
    print(f"event forms limb/quad vs phase ({'full step' if ls is None else 'line search ' + str(ls)}): step {worst_step:.2e} of the scale, performance index before {worst_before:.2e}, "
          f"after (value pass forms) {worst_after:.2e}, accepted trial vs oracle {worst_ls:.2e}; fused vs separate chain bit for bit")


# ---------------------------------------------------------------------------------------------- 4. factored sweep against the dense stage
@pytest.mark.parametrize("name", ["A_walk", "A_run", "S"])
def test_factored_sweep_equals_the_dense_stage_on_per_instance_grids(model, name):
    """k_riccati_fact against k_riccati<58> (HSQP_RICCATI_DENSE) behind the same limb-lane kernels, as
    test_factored_serial_sweep_equals_the_dense_stage_on_the_device: within 1e-9 of the step's scale, bit-identical with and without the KKT report.
    The per-instance grids put zero-length intervals on all three positions of the roll-out's groups of three stages and a run of padding in front
    of the last stage.
    Measured on MI355X: 2.9e-12 (A walk), 6.2e-12 (A run), 9.0e-12 (S) of the step's scale."""
    prob = EG.case(model, name)
    B, N = prob.dts.shape
    positions = {int(k) % 3 for b in range(B) for k in EG.event_intervals(prob.dts[b])}
    assert positions == {0, 1, 2}
    outs = {}
    for form in ("dense", "fact"):
        switches = dict(TIMED, HSQP_RICCATI_DENSE="1") if form == "dense" else TIMED
        s = create(model, switches, dict(TIMED_FORMS, ric_fact=form == "fact"), max_nodes=N, max_batch=B, riccati="serial")
        try:
            s.upload(prob.x0, prob.x, prob.u, prob.par, prob.dts)
            s.iterate(1, take_step=False, kkt=False)
            a = s.download()
            s.iterate(1, take_step=False, kkt=True)
            b = s.download()
            assert_bits(a, b, ("dx", "du"), f"{name} {form} with / without the KKT report")
            outs[form] = b
        finally:
            s.close()
    d, f = outs["dense"], outs["fact"]
    worst = 0.0
    for i in range(B):
        sc = max(1.0, np.abs(d["dx"][i]).max(), np.abs(d["du"][i]).max())
        err = max(np.abs(d["dx"][i] - f["dx"][i]).max(), np.abs(d["du"][i] - f["du"][i]).max())
        worst = max(worst, err / sc)
        assert err <= 1e-9 * sc, (name, i, err, sc)
        assert_kkt(f["kkt"][i], f["grad_inf"][i], f"{name} factored sweep, instance {i}")
    assert_events_keep_their_inputs(f, prob)
    print(f"event forms {name} factored vs dense stage: {worst:.2e} of the scale")


# ---------------------------------------------------------------------------------------------- 5. two node ranges
def test_node_ranges_on_per_instance_grids(model, oracle):
    """173 x 97 nodes on per-instance grids (no instance overflows, some pad >= 2: tests/test_event_forms.py): the limb-lane kernels and k_jump in two
    node ranges on two streams against one range, bit for bit (test_node_ranges_of_the_limb_lane_kernels_on_an_odd_shape); every instance's KKT
    residual; the instance that holds the range boundary node (events on both sides of it) and the last instance against the oracle.
    Measured on MI355X: instances 86 / 172 against the oracle 8.7e-12 / 1.1e-11 of the step's scale (1.7e-9 / 3.5e-9 absolute), performance index
    1.7e-11."""
    prob = EG.range_case(model)
    B, N = prob.dts.shape
    boundary = (B * N // 2) // 32 * 32
    bb, kb = divmod(boundary, N)
    ev = EG.event_intervals(prob.dts[bb])
    real = ev[ev < prob.n_intervals[bb] - 1]
    assert (real < kb).any() and (real > kb).any()
    outs = []
    for split in ("2", "1"):
        s = create(model, {"HSQP_LQ_SPLIT": split}, {"lq_limb": True, "value_quad": True, "ric_fact": True, "chain_fused": True, "lq_ranges": int(split)},
                   max_nodes=N, max_batch=B)
        try:
            outs.append(solve(s, prob))
        finally:
            s.close()
    assert_bits(outs[0], outs[1], STEP_KEYS, "two node ranges vs one")
    assert outs[0]["perf_after"] == outs[1]["perf_after"]
    for b in range(B):
        assert_kkt(outs[0]["kkt"][b], outs[0]["grad_inf"][b], f"instance {b}")
    assert_events_keep_their_inputs(outs[0], prob)
    worst = assert_against_oracle(outs[0], oracle, prob, "node ranges", instances=(bb, B - 1))
    print(f"event forms node ranges (boundary node {boundary} = instance {bb} node {kb}): bit for bit; vs oracle step {worst[0]:.2e} of the scale "
          f"({worst[1]:.2e} absolute), performance index {worst[2]:.2e}; worst KKT {outs[0]['kkt'].max():.2e}")


# ---------------------------------------------------------------------------------------------- 6. the two-level sweep
def test_two_level_sweep_on_per_instance_grids(model, oracle):
    """Case S (events on a segment's last and on a segment's first stage) through the opt-in two-level sweep against the serial recursion, in the shape of
    test_two_level_sweep_against_the_serial_recursion: within SEG_REL of the step's scale whatever the gate decided, repeatable bit for bit, no
    back-off; every instance — those with an event on a segment's last stage among them — against the oracle with the sweep's declared rel = SEG_REL.
    Measured on MI355X: 6.0e-12 of the step's scale from the serial recursion (8.7e-9 absolute), KKT 3.2e-10, no fallback; the serial handle against
    the oracle 6.7e-12 of the scale (3.3e-9 absolute), performance index 3.6e-11."""
    prob = EG.case(model, "S")
    B, N = prob.dts.shape
    outs = {}
    for md in ("serial", "segmented", "again"):
        s = HipSqpSolver(model, max_nodes=N, max_batch=B, riccati="serial" if md == "serial" else "segmented")
        try:
            assert s.kernel_forms()["ric_fact"]
            s.upload(prob.x0, prob.x, prob.u, prob.par, prob.dts)
            s.iterate(1, take_step=True, kkt=True)
            outs[md] = s.download()
            outs[md]["fallbacks"], outs[md]["backoffs"] = s.scan_fallbacks(), s.scan_backoffs()
        finally:
            s.close()
    a, b = outs["serial"], outs["segmented"]
    assert_bits(b, outs["again"], ("dx", "du"), "two-level sweep repeated")
    assert b["backoffs"] == 0 and a["fallbacks"] == 0
    sc, err = scale_of(a), step_diff(a, b)
    print(f"event forms two-level sweep S: |step - serial| = {err:.2e} ({err / sc:.1e} of the scale), KKT {b['kkt'].max():.1e} (serial {a['kkt'].max():.1e}), fallbacks {b['fallbacks']}")
    assert err <= SEG_REL * sc
    assert np.array_equal(a["dx"], b["dx"]) == (b["fallbacks"] == 1)
    for i in range(B):
        assert b["kkt"][i].max() <= 1e-7, f"instance {i}: KKT residual {b['kkt'][i].max():.2e} passed the gate"
        assert_perf(b["perf_after"][i], a["perf_after"][i], f"instance {i}", rel=1e-9)
    assert_events_keep_their_inputs(b, prob)
    for i in range(B):
        assert_step(b, EG.oracle_iteration(oracle, prob, i), i, "two-level sweep vs oracle", rel=SEG_REL)
    worst = assert_against_oracle(a, oracle, prob, "S serial")
    print(f"event forms S serial vs oracle: step {worst[0]:.2e} of the scale ({worst[1]:.2e} absolute), performance index {worst[2]:.2e}")


# ---------------------------------------------------------------------------------------------- 7. the parallel-in-time sweep
def test_scan_on_per_instance_grids(model, oracle):
    """The first two instances of case P (N = 64, two different grids): the default path takes the parallel-in-time sweep, as
    test_parallel_in_time_sweep_on_a_long_event_grid: the scan's result if its KKT gate accepted it (<= 2e-10 of the step's scale from the serial
    recursion), else the serial recursion's bit for bit; the gated result against the oracle.
    Measured on MI355X: the gate accepts the scan, 4.6e-11 of the step's scale from the serial recursion and from the oracle (3.1e-8 absolute at
    |step| = 680: above the unrelaxed 1e-8, inside TRAJ_ABS + 1e-10 x scale = 7.8e-8)."""
    full = EG.case(model, "P")
    prob = EG.EventProblem(*(a[:2] for a in full))
    N = prob.dts.shape[1]
    outs = {}
    for mode in ("auto", "serial"):
        s = HipSqpSolver(model, max_nodes=N, max_batch=2, riccati=mode)
        try:
            outs[mode] = solve(s, prob)
            outs[mode]["fallbacks"] = s.scan_fallbacks()
        finally:
            s.close()
    a, b = outs["serial"], outs["auto"]
    assert_events_keep_their_inputs(b, prob)
    sc, err = scale_of(a), step_diff(a, b)
    if b["fallbacks"]:
        assert_bits(a, b, ("dx", "du"), "rejected scan")
    else:
        assert err <= 2e-10 * sc, (err, sc)
        for i in range(2):
            assert_perf(b["perf_after"][i], a["perf_after"][i], "scan vs serial on per-instance grids", rel=1e-9)
    print(f"event forms scan P: fallbacks {b['fallbacks']}, |step - serial| = {err:.2e} ({err / sc:.1e} of the scale)")
    worst = [0.0, 0.0]
    for i in range(2):
        r = EG.oracle_iteration(oracle, full, i)
        e = EG.step_error(b, r, i)
        worst = [max(worst[0], e / EG.step_scale(r)), max(worst[1], e)]
        print(f"  gated result instance {i}: step error {e:.2e} = {e / EG.step_scale(r):.2e} of the scale")
        assert_step(b, r, i, "gated scan vs oracle", rel=ORACLE_REL)
        assert_kkt(b["kkt"][i], b["grad_inf"][i], f"gated scan, instance {i}")
    print(f"event forms scan P gated result vs oracle: step {worst[0]:.2e} of the scale ({worst[1]:.2e} absolute)")


# ---------------------------------------------------------------------------------------------- 8. the centroidal formulation
@pytest.mark.parametrize("riccati", ["serial", "parallel"])
def test_centroidal_kernels_on_per_instance_grids(cmodel, coracle, riccati):
    """The centroidal twin (3 x 18 nodes: k_lq_cent2, k_lq_cent2_value, the serial sweep / the scan kernels) against its oracle per instance, and the
    permutation of the batch rows bit for bit.
    Measured on MI355X: serial 1.2e-11 of the step's scale (4.0e-9 absolute), scan 1.1e-11 (3.7e-9), performance index 5.0e-13."""
    prob = EG.centroidal_case(cmodel)
    B, N = prob.dts.shape
    s = HipSqpSolver(cmodel, max_nodes=N, max_batch=B, riccati=riccati)
    try:
        out = solve(s, prob)
        perm = np.array([2, 0, 1])
        got = solve(s, EG.permuted(prob, perm))
    finally:
        s.close()
    worst = [0.0, 0.0, 0.0]
    for b in range(B):
        r = EG.oracle_iteration(coracle, prob, b)
        e, sc = EG.step_error(out, r, b), EG.step_scale(r)
        perf = max(abs(out["perf_after"][b][k] - r["perf_after"][k]) / abs(r["perf_after"][k]) for k in ("cost", "dynamics_sse", "equality_sse") if abs(r["perf_after"][k]) > 1e-3)
        worst = [max(worst[0], e / sc), max(worst[1], e), max(worst[2], perf)]
        print(f"  centroidal {riccati} instance {b}: step error {e:.2e} = {e / sc:.2e} of the scale {sc:.3g}, performance index {perf:.2e}")
        assert_step(out, r, b, f"centroidal {riccati}", rel=ORACLE_REL)
        assert_perf(out["perf_before"][b], r["perf_before"], f"centroidal instance {b} before")
        assert_perf(out["perf_after"][b], r["perf_after"], f"centroidal instance {b} after")
    assert_events_keep_their_inputs(out, prob)
    for key in STEP_KEYS:
        assert np.array_equal(got[key], out[key][perm]), key
    assert got["perf_after"] == [out["perf_after"][i] for i in perm]
    print(f"event forms centroidal {riccati} vs oracle: step {worst[0]:.2e} of the scale ({worst[1]:.2e} absolute), performance index {worst[2]:.2e}; permutation bit for bit")


# ---------------------------------------------------------------------------------------------- 9. poison
def test_poisoned_lds_and_hbm_on_per_instance_grids(model):
    """Case A on the forced limb / quad handle with NaN patterns in every LDS word in front of every launch and in every device buffer at creation
    (HSQP_POISON_LDS, HSQP_POISON_HBM: the handles of tests/test_gpu_parity.py::_poisoned_and_clean, with the forms asserted) against a clean handle:
    finite and bit-equal.  The run case, then the walk case on the SAME handle: a record entry that only an event node leaves unwritten meets a
    non-zero leftover of the solve before it, not the allocator's zeros."""
    probs = [EG.case(model, "A_run"), EG.case(model, "A_walk")]
    outs = []
    for poison in (True, False):
        switches = dict(TIMED, HSQP_POISON_LDS="1", HSQP_POISON_HBM="1") if poison else TIMED
        s = create(model, switches, TIMED_FORMS, max_nodes=18, max_batch=5, riccati="serial")
        try:
            outs.append([solve(s, p) for p in probs])
        finally:
            s.close()
    for a, b, p in zip(outs[0], outs[1], probs):
        for key in STEP_KEYS + ("kkt",):
            assert np.isfinite(a[key]).all(), key
            assert np.array_equal(a[key], b[key]), key
        assert a["perf_after"] == b["perf_after"] and a["perf_before"] == b["perf_before"]
        assert_events_keep_their_inputs(a, p)
    print("event forms poison: LDS and HBM poisoned handle equals the clean one bit for bit on the run case and on the walk case after it")
