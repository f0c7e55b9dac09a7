"""k_project's Gram accumulation keeps every sum of the QP record in the order of the kernel it replaced: the record (A~, B~, b~, Q~, P~, R~, q~, r~, Px, Pu, Pe,
nut of every node) and the step (dx, du, perf_after) of the bench problem (256 x 100, limb-lane LQ kernels, RK4 chain inside k_project), of a centroidal handle and
of a small whole-body handle (phase-form LQ kernel, row-major residual rows) are BIT FOR BIT those recorded from the parent of the pair-of-rows border sums
(tests/golden/gram_tail_parent.json: the first 16 hex digits of the SHA-256 of each array's bytes).  array_equal, not a tolerance: the change re-groups LDS reads
and threads, never the order of a sum.

    python tests/test_gpu_gram_tail.py --record      (on a GPU, with the library whose results are to be recorded) rewrites the golden file."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
GOLDEN = os.path.join(ROOT, "tests", "golden", "gram_tail_parent.json")
CASES = ("bench", "centroidal", "phase_form")


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()[:16]


def _case(name):
    from qp_layout import QP
    from wb_humanoid_mpc_amd import load_model
    from wb_humanoid_mpc_amd.reference import BENCH_SEED, make_centroidal_problem, make_problem
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    if name == "bench":
        model = load_model()
        B, N = 256, 100
        problem = make_problem(model, n_nodes=N, batch=B, gait="walk", perturb=True, seed=BENCH_SEED)
    elif name == "centroidal":
        model = load_model(formulation="centroidal")
        B, N = 4, 24
        problem = make_centroidal_problem(model, n_nodes=N, batch=B, gait="walk", perturb=True, seed=3)
    else:
        model = load_model()
        B, N = 3, 20
        problem = make_problem(model, n_nodes=N, batch=B, gait="run", perturb=True, seed=3)
    s = HipSqpSolver(model, max_nodes=N, max_batch=B)
    try:
        forms = s.kernel_forms()
        assert forms["lq_limb"] == (name == "bench"), forms
        s.upload(*problem)
        s.iterate(1, kkt=True)   # with the KKT report k_project writes the whole record (joint rows of A~ / B~, lower triangle of Q~)
        size = s.lib.hsqp_debug_read(s.h, 102, None, 0)
        assert size == B * N * QP["QP_SIZE"] * 8, (size, s.lib.hsqp_last_error(s.h))
        qp = np.full(size // 8, np.nan)
        assert s.lib.hsqp_debug_read(s.h, 102, qp.ctypes.data_as(C.c_void_p), qp.nbytes) == size
        out = s.download()
    finally:
        s.close()
    qp = qp.reshape(B * N, QP["QP_SIZE"])[:, :QP["QP_NUT"] + 1]   # (behind nut: padding nobody writes)
    assert np.isfinite(qp).all() and np.isfinite(out["dx"]).all() and np.isfinite(out["du"]).all()
    got = {"qp": _digest(qp), "dx": _digest(out["dx"]), "du": _digest(out["du"]),
           "perf_after": _digest(np.array([[p["merit"], p["cost"], p["dynamics_sse"], p["equality_sse"]] for p in out["perf_after"]]))}
    for key in ("QP_Q", "QP_P", "QP_R", "QP_QV", "QP_RV"):   # the blocks gram_store writes, one by one: a mismatch says which
        nxt = min(v for k, v in QP.items() if k.startswith("QP_") and k != "QP_SIZE" and v > QP[key])
        got[key] = _digest(qp[:, QP[key]:nxt])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_qp_record_and_step_are_bit_for_bit_the_recorded_parents(name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = _case(name)
    print(got)
    assert got == want


if __name__ == "__main__":
    assert "--record" in sys.argv
    rec = {name: _case(name) for name in CASES}
    with open(sys.argv[sys.argv.index("--record") + 1] if len(sys.argv) > 2 else GOLDEN, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, indent=1, sort_keys=True))
