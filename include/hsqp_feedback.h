/*
 * hsqp_feedback.h — the Riccati feedback policy of the MI355X SQP library (upstream ocs2_sqp SqpSolver::setPrimalSolution with
 * sqp::Settings::useFeedbackPolicy = true, its default): the linear controller u = uff + K x of ocs2's LinearController, whose gains come
 * from the LAST QP solved and whose biases from the final trajectory.  For node i of instance b of the resident solution (hsqp_download's
 * x, u: after the step of the last iteration, whatever its length, HSQP_STEP_ZERO included):
 *   K_i = Px_i + Pu_i K~_i   (35 x 58: the equality projection du = Px dx + Pu ut + Pe and the Riccati gain ut = K~ dx + k~ of the node)
 *   uff_i = u_i - K_i x_i
 * A pre-event node (0 < i < N, dt_nodes[b][i] == 0) takes the entries of node i - 1, chained over consecutive events; node N those of node
 * N - 1.  So the policy has N + 1 entries per instance, and the copies are bit copies.  Centroidal handles: columns 35..57 of K are zero.
 *
 * Validity: the policy is available after a successful hsqp_solve or hsqp_iterate_device (any sweep, any flags).  Every hsqp_upload*
 * call and every hsqp_iterate_device call that fails invalidates it; the calls below then return HSQP_ERR_BAD_ARG (message in
 * hsqp_last_error), as they do for a window outside [0, N] or a NULL handle.  HSQP_ERR_NUMERIC as hsqp_download if an instance of the
 * solution failed.  The gains are formed on the device when asked for: an iteration does no extra work.
 *
 * ABI: these entry points are additions only — no public struct and no entry point of hsqp.h changes, so by the rule above
 * HSQP_ABI_VERSION (hsqp.h) needs no revision bump.
 */
#ifndef HSQP_FEEDBACK_H
#define HSQP_FEEDBACK_H

#include "hsqp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* gains / biases of nodes [first, first + count) of every instance, count <= N + 1 - first; K [B][count][35][58], uff [B][count][35],
 * row-major; either may be NULL */
int hsqp_feedback_policy(hsqp_handle* h, int first, int count, double* K, double* uff);
/* the same into DEVICE memory of the handle's GPU (like hsqp_download_device) */
int hsqp_feedback_policy_device(hsqp_handle* h, int first, int count, double* d_K, double* d_uff);
/* MPC_MRT_Interface::evaluatePolicy with a LinearController (humanoid_wb_mpc/src/mrt/WBMpcMrtJointController.cpp:136-147: "Evaluate
 * policy with feedback if activated in config"), s[b] seconds after the first node:
 *   x = the optimal state there (bit-identical to hsqp_evaluate_policy's x),
 *   u = uff(s) + K(s) x_meas[b], K and uff interpolated on the segment and with the weight hsqp_evaluate_policy uses for the input,
 *   tau = the joint torques at (x, u) through the path of hsqp_evaluate_policy.
 * s [B], x_meas [B][58] (centroidal: the first 35 entries of a row count); x [B][58], u [B][35], tau [B][23]: any output may be NULL.
 * Only the entries of the two nodes around s[b] are formed. */
int hsqp_evaluate_feedback_policy(hsqp_handle* h, const double* s, const double* x_meas, double* x, double* u, double* tau);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_FEEDBACK_H */
