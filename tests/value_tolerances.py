"""Tolerances of the value-function tests (tests/test_value.py, tests/test_gpu_value.py), with their derivation.

What is compared.  The record (S_k, s_k) of include/hsqp_value.h against tests/value_ref.py, per node and RELATIVE to the node's own magnitude,
    eS_k = max|S_k - S_k^ref| / max|S_k^ref|,      es_k = max|s_k - s_k^ref| / max|s_k^ref|        (value_ref.node_error: the worst node),
because the entries of S span many orders of magnitude (joint-velocity rows ~1e-2, base-position rows ~1e5) and the reduced Hessian the sweeps
factor reaches cond ~ 1e7: an absolute bound would be either vacuous for the small nodes or unattainable for the large ones.

The yardstick.  No bound on eS, es can be derived from the number format alone: it is (condition of the recursion) x eps, and the condition is a
property of the fixture.  What CAN be measured without the code under test is how far two correct float64 computations of the same quantity land
from each other: value_ref.dense_tail_value (one dense KKT solve per node) and value_ref.riccati_value (a numpy Riccati recursion on QR-projected
stages) share no intermediate result.  REF_DISCREPANCY is the worst eS / es between the two over the fixtures tests/golden/wb_stance_n4.npz,
wb_walk_n8.npz and cent_walk_n8.npz, measured by tests/test_value.py::test_the_two_references_agree, which asserts that the measurement does not
exceed the constant (so the constant cannot silently go stale) and prints it.

The device bound.  The device evaluates the same recursion in another order again (factored stage, matrix-core tiles, for the gated sweeps an
associative scan), so it is a third sample of the same population: DEVICE_FACTOR = 10 samples' spread is allowed.  The parallel-in-time scan and the
two-level sweep carry the extra factor their declared STEP tolerances carry over the serial sweep in tests/tolerances.py: the scan is held to the
serial sweep's bound there (TRAJ_ABS, 1e-10 of the step's scale on event grids: factor 1), the two-level sweep to its declared 1e-9 of the step's scale
against 1e-10 (factor 10).  The bounds are NOT tuned to the device's result: profiles/value_parity.txt records the device's worst error beside them.

Bit-for-bit checks (host build of the kernel source against the numpy mirror, device against the host build, batch against solo, flag against no
flag) have no tolerance.

Central differences (tests/test_value.py).  The tail problem is exactly quadratic, so with V(+h xi), V(-h xi), V(0) from three dense KKT solves
    (V(+h) - V(-h)) / 2h = s' xi,      (V(+h) + V(-h) - 2 V(0)) / h^2 = xi' S xi
hold up to the rounding of the three values.  A computed optimum carries a relative error of about FD_VALUE_REL = 1e-11 (residual of a backward-stable
dense solve times the multipliers: cond ~ 1e5 headroom over eps); the differences divide it by 2h and h^2, so the bounds are
FD_VALUE_REL (|V(+h)| + |V(-h)| + 2 |V(0)|) / h^2  and  FD_VALUE_REL (|V(+h)| + |V(-h)|) / 2h, plus REF_DISCREPANCY of the compared quantity itself."""

# worst relative node error between the two CPU references over the three fixtures, rounded UP to one digit (measured: eS 2.4e-13 / 6.2e-13 / 9.4e-13,
# es 3.3e-13 / 4.2e-13 / 4.2e-12 on wb_stance_n4 / wb_walk_n8 / cent_walk_n8; profiles/value_parity.txt)
REF_DISCREPANCY_S = 1e-12
REF_DISCREPANCY_s = 5e-12
DEVICE_FACTOR = 10.0
SWEEP_FACTOR = {"serial": 1.0, "dense": 1.0, "centroidal": 1.0, "parallel": 1.0, "segmented": 10.0}

FD_VALUE_REL = 1e-11
FD_STEP = 0.1


def device_bound(sweep):
    """(bound on eS, bound on es) of the record against value_ref.dense_tail_value"""
    f = DEVICE_FACTOR * SWEEP_FACTOR[sweep]
    return f * REF_DISCREPANCY_S, f * REF_DISCREPANCY_s
