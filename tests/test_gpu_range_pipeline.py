"""The node-range pipeline of hsqp_iterate_device (csrc/hsqp_capi.hip): with HSQP_LQ_SPLIT = S > 1 and a launch of more than one round of
the chip, every range runs k_lq_limb -> k_lq_rows -> k_project (-> k_jump) on a stream of its own, and the ranges join in front of the backward
sweep.  Only launch geometry and stream order change, so every number the handle returns must equal, bit for bit, what HSQP_LQ_SPLIT=1 (one
launch per kernel, one stream) returns.

At (173, 97) the range boundaries lie inside an instance.  perf_after is the figure that would catch a value pass that ran ahead of its
neighbour's step (the dynamics defect of node k reads x_new of node k + 1): k_step / k_value_quad were taken through the same ranges, measured
slower and left on one stream — the cases stay, so that whoever tries again has the check."""
import os

import numpy as np
import pytest

from wb_humanoid_mpc_amd.reference import make_problem

pytestmark = pytest.mark.gpu

ARRAYS = ("x", "u", "dx", "du", "kkt")
SHAPES = [(256, 100), (173, 97)]


def _handle(model, B, N, split, poison=False, **kw):
    from wb_humanoid_mpc_amd.solver import HipSqpSolver
    os.environ["HSQP_LQ_SPLIT"] = str(split)
    if poison:
        os.environ["HSQP_POISON_LDS"] = "1"
    try:
        return HipSqpSolver(model, max_nodes=N, max_batch=B, **kw)
    finally:
        os.environ.pop("HSQP_LQ_SPLIT", None)
        os.environ.pop("HSQP_POISON_LDS", None)


def _both(model, B, N, split, poison=False):
    """(run() with the KKT report, iterate(1, take_step=False) + download()) of one handle."""
    prob = make_problem(model, n_nodes=N, batch=B, perturb=True, seed=3)
    s = _handle(model, B, N, split, poison)
    try:
        forms = s.kernel_forms()
        assert forms["lq_limb"] and forms["value_quad"] and forms["lq_ranges"] == split, forms
        solved = s.run(*prob)          # KKT report: joint_rows on, k_kkt behind the step
        s.upload(*prob)
        s.iterate(1, take_step=False)  # the bench's call: no joint rows
        plain = s.download()
    finally:
        s.close()
    return solved, plain


def _assert_same(got, want, what, arrays=ARRAYS):
    for key in arrays:
        assert np.isfinite(got[key]).all(), (what, key)
        assert np.array_equal(got[key], want[key]), (what, key)
    for key in ("perf_before", "perf_after"):
        assert got[key] == want[key], (what, key)


_single = {}


def _single_stream(model, B, N):
    if (B, N) not in _single:
        _single[(B, N)] = _both(model, B, N, 1)
    return _single[(B, N)]


@pytest.mark.parametrize("split", [1, 2, 3])
@pytest.mark.parametrize("B,N", SHAPES)
def test_ranges_give_the_bits_of_one_launch_per_kernel(model, B, N, split):
    """(256, 100): 800 workgroups of 32 nodes, boundaries at whole workgroups; (173, 97): 525 workgroups, every boundary inside an instance and
    the last workgroup part padding.  x, u, dx, du, kkt and both performance indices, with and without the KKT report."""
    want_solved, want_plain = _single_stream(model, B, N)
    solved, plain = _both(model, B, N, split)
    _assert_same(solved, want_solved, f"run, {B} x {N}, {split} ranges")
    _assert_same(plain, want_plain, f"iterate, {B} x {N}, {split} ranges", arrays=("x", "u", "dx", "du"))


def _iterated(model, B, N, split, poison=False, **iterate_kw):
    prob = make_problem(model, n_nodes=N, batch=B, perturb=True, seed=5)
    s = _handle(model, B, N, split, poison)
    try:
        s.upload(*prob)
        s.iterate(**iterate_kw)
        return s.download()
    finally:
        s.close()


@pytest.mark.parametrize("iterate_kw", [dict(n_iterations=2, take_step=True), dict(n_iterations=3, take_step=True, linesearch=True)],
                         ids=["take_step", "linesearch"])
def test_iterations_that_take_the_step_keep_the_order_across_streams(model, iterate_kw):
    """Several iterations in one call: the next iteration's LQ ranges on the aux streams must come behind x <- x_new (and the line search's
    trials) on h->stream, and the backward sweep behind every range's k_project.  (Full steps: two iterations, one such copy between them — a third full step
    from these perturbed starts leaves the region where the reduced Hessian is positive definite, on one stream as on several.)"""
    B, N = 173, 97
    want = _iterated(model, B, N, 1, **iterate_kw)
    for split in (2, 3):
        _assert_same(_iterated(model, B, N, split, **iterate_kw), want, f"{iterate_kw}, {split} ranges", arrays=("x", "u", "dx", "du"))


def test_ranges_with_poisoned_lds(model):
    """HSQP_POISON_LDS puts a kernel that fills every CU's LDS with NaN patterns in front of every launch, on that launch's stream: the ranges
    on two streams give the bits of the clean single-stream handle."""
    B, N = 173, 97
    want_solved, want_plain = _single_stream(model, B, N)
    solved, plain = _both(model, B, N, 2, poison=True)
    _assert_same(solved, want_solved, "poisoned run")
    _assert_same(plain, want_plain, "poisoned iterate", arrays=("x", "u", "dx", "du"))


def test_a_launch_of_less_than_one_round_stays_on_one_stream(model):
    """32 x 100 nodes are 100 workgroups of the limb-lane kernels, under one round of the chip: the handle reports the ranges it was created with,
    launches every kernel once on its own stream, and returns the bits of HSQP_LQ_SPLIT=1."""
    B, N = 32, 100
    solved, plain = _both(model, B, N, 2)
    want_solved, want_plain = _both(model, B, N, 1)
    _assert_same(solved, want_solved, "small run")
    _assert_same(plain, want_plain, "small iterate", arrays=("x", "u", "dx", "du"))
