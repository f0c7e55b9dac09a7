"""The projected cost blocks of project_node (host build of csrc/hsqp_project.h) against the oracle's LQ blocks, whole-body and centroidal: Q~, P~, R~, q~, r~
of the QP record must be T^T H T and T^T (g + H t) with T = [I 0; Px Pu], t = [0; Pe] — H, g and the equality rows from the oracle, the projection from the record
(checked against the oracle's equality rows: C + D Px = 0, D Pu = 0, D Pe + e = 0).  Guards the arithmetic of the Gram accumulation (residual rows in three passes,
then the input-weight rows with d_u and g_u) where no GPU is present; the device's own accumulation is pinned by tests/test_gpu_gram_tail.py."""
import ctypes as C

import numpy as np
import pytest

from qp_layout import NUT, QP
from test_hostemu import P, emu  # noqa: F401  (fixture)
from test_hostemu_centroidal import cemu  # noqa: F401  (fixture)
from test_oracle_centroidal_ocp import perturbed_centroidal_problem
from test_oracle_lq import perturbed_problem
from wb_humanoid_mpc_amd import _abi

NX, NU = _abi.NX, _abi.NU


def _check(lib, h, lq, problem, n):
    x0, x, u, par, dt = problem
    xn, un, dx, du = np.zeros_like(x), np.zeros_like(u), np.zeros_like(x), np.zeros_like(u)
    kkt, pb, pa = np.zeros(2), np.zeros(3), np.zeros(3)
    assert lib.emu_qp_size() == QP["QP_SIZE"]
    qp = np.zeros((n, QP["QP_SIZE"]))
    assert lib.emu_sqp_iteration(h, n, C.c_double(dt), P(x0), P(x), P(u), P(par), P(xn), P(un), P(dx), P(du), P(kkt), P(pb), P(pa), P(qp), None) == 0
    for k in range(n):
        q = qp[k]
        nut, ne = int(q[QP["QP_NUT"]]), int(lq["ne"][k])
        assert nut == NU - ne and 0 < nut <= NUT
        Px, Pu, Pe = q[QP["QP_PX"]:QP["QP_PU"]].reshape(NU, NX), q[QP["QP_PU"]:QP["QP_PE"]].reshape(NU, NUT)[:, :nut], q[QP["QP_PE"]:QP["QP_PE"] + NU]
        CDe = lq["CDe"][k][:ne]
        Cm, D, e = CDe[:, :NX], CDe[:, NX:NX + NU], CDe[:, NX + NU]
        cs = max(1.0, np.abs(CDe).max())
        assert np.abs(Cm + D @ Px).max() <= 1e-10 * cs and np.abs(D @ Pu).max() <= 1e-10 * cs and np.abs(D @ Pe + e).max() <= 1e-10 * cs
        assert np.abs(Pu.T @ Pu - np.eye(nut)).max() <= 1e-12
        H, g = lq["H"][k], lq["g"][k]
        T = np.zeros((NX + NU, NX + nut))
        T[:NX, :NX] = np.eye(NX)
        T[NX:, :NX], T[NX:, NX:] = Px, Pu
        t = np.concatenate([np.zeros(NX), Pe])
        Ht, gt = T.T @ H @ T, T.T @ (g + H @ t)
        Q, Pm, R = (q[QP["QP_Q"]:QP["QP_P"]].reshape(NX, NX), q[QP["QP_P"]:QP["QP_R"]].reshape(NUT, NX), q[QP["QP_R"]:QP["QP_QV"]].reshape(NUT, NUT))
        # 1e-11 of the block's scale: the bound the LQ record is held to against the oracle (test_lq_record_expands_to_the_oracle_blocks)
        hs, gs = max(1.0, np.abs(Ht).max()), max(1.0, np.abs(gt).max())
        errs = (np.abs(np.triu(Q) - np.triu(Ht[:NX, :NX])).max() / hs, np.abs(Pm[:nut] - Ht[NX:, :NX]).max() / hs, np.abs(R[:nut, :nut] - Ht[NX:, NX:]).max() / hs,
                np.abs(q[QP["QP_QV"]:QP["QP_QV"] + NX] - gt[:NX]).max() / gs, np.abs(q[QP["QP_RV"]:QP["QP_RV"] + nut] - gt[NX:]).max() / gs)
        print(f"node {k}: nut {nut}  Q~ {errs[0]:.2e} P~ {errs[1]:.2e} R~ {errs[2]:.2e} q~ {errs[3]:.2e} r~ {errs[4]:.2e} of the scale")
        assert max(errs) <= 1e-11
        assert np.array_equal(R[nut:, nut:], np.eye(NUT - nut)) and not R[:nut, nut:].any() and not Pm[nut:].any()


@pytest.mark.parametrize("gait,n", [("stance", 4), ("walk", 8), ("run", 14)])
def test_projected_cost_blocks_match_the_oracle(model, oracle, emu, gait, n):  # noqa: F811
    lib, h = emu
    problem = perturbed_problem(model, n, gait, seed=5)
    x0, x, u, par, dt = problem
    _check(lib, h, oracle.lq(dt, x, u, par), problem, n)


@pytest.mark.parametrize("gait,n", [("stance", 4), ("walk", 8), ("run", 14)])
def test_projected_cost_blocks_match_the_oracle_centroidal(cmodel, coracle, cemu, gait, n):  # noqa: F811
    lib, h = cemu
    problem = perturbed_centroidal_problem(cmodel, n, gait, seed=5)
    x0, x, u, par, dt = problem
    _check(lib, h, coracle.cent_lq(dt, x, u, par), problem, n)
