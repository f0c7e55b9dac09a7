/*
 * hsqp_value.h — the Riccati value function of the MI355X SQP library (upstream ocs2_sqp SqpSolver::getValueFunction with
 * sqp::Settings::createValueFunction = true): the quadratic cost-to-go of the LAST QP solved.  For node k of instance b the backward sweep
 * leaves S_k (58 x 58) and s_k (58), and the cost-to-go of the QP's tail problem from node k is, up to a constant that is not computed,
 *   V_k(dx) = s_k^T dx + 1/2 dx^T S_k dx,   dx = x - xbar_k,
 * where xbar is the trajectory the QP was LINEARISED at (hsqp_problem::x_traj of the last iteration; after HSQP_ITER_TAKE_STEP the resident
 * solution hsqp_download returns is xbar + alpha dx and is NOT the centre of the model).  Declared difference from upstream as recalled:
 * ocs2 re-centres its value function on the post-step nominal trajectory; this library keeps the centre xbar, where the quadratic lives.
 *
 * Keeping the record: an iteration keeps S_k, s_k of all nodes and a bit copy of xbar only when hsqp_iterate_device runs with
 * HSQP_ITER_VALUE_FUNCTION (below); the record is that of the sweep whose step the iteration accepted (a rejected parallel-in-time or
 * two-level sweep leaves the serial recursion's), of the LAST iteration of the call.  Without the flag an iteration launches the same kernels
 * with the same arguments as before.  Memory: the flag allocates [max_batch][max_nodes + 1][58 * 58 + 58] doubles on first use (0.7 GB at
 * 256 x 100; HSQP_ERR_OOM names the size) plus the copy of xbar.
 *
 * Validity: the record is valid after an hsqp_iterate_device call that ran with the flag and returned HSQP_OK.  Every hsqp_upload*,
 * hsqp_solve, hsqp_update_weights, hsqp_update_term_weights, every failed iteration and every iteration WITHOUT the flag clears it; the calls
 * below then return HSQP_ERR_BAD_ARG (message in hsqp_last_error), as they do for a NULL handle or input, nodes outside [0, N], k0 > k1,
 * n_queries < 1 or (host form) a non-finite s_query.
 *
 * S is returned SYMMETRIC: 1/2 (S + S^T) of what the sweep stored (the sweeps keep S symmetric up to rounding).  Centroidal handles: the
 * leading 35 x 35 / 35 entries are the value function, the padding rows and columns are exact zeros, and the first 35 entries of a query
 * state count.
 *
 * ABI: these entry points are additions only — no public struct and no entry point of hsqp.h changes, so HSQP_ABI_VERSION (hsqp.h) needs
 * no revision bump.
 */
#ifndef HSQP_VALUE_H
#define HSQP_VALUE_H

#include "hsqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* hsqp_iterate_device flag (beside HSQP_ITER_TAKE_STEP ... HSQP_ITER_UNTIL_CONVERGED of hsqp.h): keep the value-function record */
#define HSQP_ITER_VALUE_FUNCTION 16

/* The record of nodes k0 .. k1 (0 <= k0 <= k1 <= N) of every instance, n = k1 - k0 + 1: S [B][n][58][58], s [B][n][58], xbar [B][n][58],
 * row-major; any of the three may be NULL. */
int hsqp_value_function(hsqp_handle* h, int k0, int k1, double* S, double* s, double* xbar);
/* the same into DEVICE memory of the handle's GPU (like hsqp_download_device) */
int hsqp_value_function_device(hsqp_handle* h, int k0, int k1, double* d_S, double* d_s, double* d_xbar);

/* SolverBase::getValueFunction(t, x), n_queries per instance: query q of instance b asks at s_query[b][q] seconds after the first node (as
 * hsqp_evaluate_policy; outside [0, horizon] it clamps as the policy does) and at the state x_query[b][q].  The segment and the weight are
 * the ones hsqp_evaluate_policy takes for the STATE (event nodes, zero-length intervals, per-instance grids included); S, s and xbar are
 * blended linearly between the segment's two nodes, dx = x_query - xbar(s), and
 *   dfdx  = s + S dx                    [B][n_queries][58]
 *   dfdxx = S (symmetric)               [B][n_queries][58][58]
 *   dV    = s^T dx + 1/2 dx^T S dx      [B][n_queries]      the value relative to the nominal (this library's addition; the constant of the
 *                                                           cost-to-go is not computed, an ocs2 caller reports f = 0)
 * Any output may be NULL.  A non-finite x_query gives non-finite outputs for that query alone.  Every sum is taken in an order fixed by the
 * index, so results are reproducible run to run. */
int hsqp_evaluate_value_function(hsqp_handle* h, int n_queries, const double* s_query, const double* x_query, double* dV, double* dfdx, double* dfdxx);
/* the same with every array in DEVICE memory of the handle's GPU (s_query is not checked for finiteness) */
int hsqp_evaluate_value_function_device(hsqp_handle* h, int n_queries, const double* d_s_query, const double* d_x_query, double* d_dV, double* d_dfdx,
                                        double* d_dfdxx);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_VALUE_H */
