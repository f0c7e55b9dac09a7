/*
 * hsqp_rollout.h — batched policy rollout of the MI355X SQP library: the plant moved forward under the resident policy, on the device
 * (upstream ocs2 MRT_BASE::rolloutPolicy with a TimeTriggeredRollout of the system flow map, as the reference's dummy-simulation nodes
 * set it up with mrt.initRollout(&interface.getRollout())).  The plant is the MPC's own flow map: the whole-body
 * xdot = [v, a_b(x, u), qdd_j] or the centroidal flow map, with the input of the controller at (t, x).
 *
 * Times: s seconds after the first node of the resident solution, the frame of hsqp_evaluate_policy.  Instance b starts at x0[b] at s0[b]
 * and reports the state and input at the n_samples times s0[b] + duration * (j + 1) / n_samples (the last one: s0[b] + duration).
 *
 * One sample interval is one MRT_BASE::rolloutPolicy call: the integration restarts at the start of every interval with the step
 * min(initial_step, remaining) and a fresh flow evaluation, so a call with n_samples = n equals n chained calls of duration / n bit for bit
 * when the times are exact binary fractions.  x[b][j] is the last state of the interval (stateTrajectory.back()), u[b][j] the controller's
 * input at the sample time and that state: for HSQP_ROLLOUT_FEEDFORWARD the arithmetic of hsqp_evaluate_policy's u, for
 * HSQP_ROLLOUT_FEEDBACK that of hsqp_evaluate_feedback_policy's u.
 *
 * Events: inside an interval the integration also restarts (step min(initial_step, remaining), fresh flow evaluation) at every event of
 * the resident grid, the shared stamp of a pre- and a post-event node (dt_nodes == 0); the jump map is the identity, as in
 * TimeTriggeredRollout's split at the switching times.  A uniform grid has no event nodes.  ocs2 also restarts at mode-schedule events that
 * fall between nodes; this rollout does not see those (the mode schedule is not resident): that changes the step sequence only, not the
 * solution beyond the integration tolerance.
 *
 * HSQP_ROLLOUT_ODE45: Dormand–Prince 5(4) with FSAL, the 5th-order solution propagated, steps clipped to land on sample and event times.
 * Step control (boost odeint's default_error_checker / default_step_adjuster as ocs2's ODE45 uses them through runge_kutta_dopri5 —
 * restated from memory, neither library is a dependency): with x, xdot at the start of a step of length h and the embedded error e,
 *   err = max_i |e_i| / (abs_tol + rel_tol (|x_i| + h |xdot_i|));
 *   err > 1: rejected, h *= max(0.9 err^(-1/3), 0.2);   accepted and err < 0.5: h *= 0.9 max(err, 5^-5)^(-1/5).
 * More than 500 rejections in a row end the instance like the step cap (odeint's failed-step checker).
 * HSQP_ROLLOUT_RK4: classical RK4 with the fixed step initial_step; the last step before a sample or event time is shortened.
 * Step cap (ocs2's maxNumStepsPerSecond, also from memory): at most max_steps_per_second * max(1 s, interval length) accepted steps per sample
 * interval; an instance that needs more gets status HSQP_ROLLOUT_MAX_STEPS and NaN outputs from that sample on.  A non-finite flow or
 * input value gives HSQP_ROLLOUT_NONFINITE, the same way.
 *
 * Centroidal handles: the first 35 entries of a state row are live (x0's others are ignored, x's are written as zero); u is the centroidal
 * input.
 *
 * Validity: as the feedback policy (hsqp_feedback.h) — after a successful hsqp_solve or hsqp_iterate_device, not after any hsqp_upload*
 * call or a failed iteration.  Otherwise HSQP_ERR_BAD_ARG (message in hsqp_last_error), as for duration < 0 or not finite, n_samples < 1,
 * a non-positive (or non-finite) tolerance, initial_step or max_steps_per_second, a non-finite s0, an unknown integrator or controller, or a
 * NULL s0 / x0 / status.  A call never changes the resident solution.  Return value: HSQP_OK; HSQP_ERR_NOT_CONVERGED if an instance hit the
 * step cap, HSQP_ERR_NUMERIC if one was non-finite (this one wins over the cap); every other instance's outputs are complete and correct in
 * both cases and status[b] names the failed ones.  Outputs x, u, steps (accepted steps over the call), rejected may be NULL.
 *
 * Cost: one launch for the whole integration (one workgroup per instance: the adaptive loop, the samples and the events run inside it);
 * the feedback controller first forms the gain entries of the window the call spans ([min s0, max s0 + duration]) with the kernel of
 * hsqp_feedback_policy.  The iteration is not changed by any of it.
 *
 * ABI: additions only — no public struct and no entry point of hsqp.h changes, so HSQP_ABI_VERSION (hsqp.h) needs no revision bump.
 */
#ifndef HSQP_ROLLOUT_H
#define HSQP_ROLLOUT_H

#include "hsqp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSQP_ROLLOUT_ODE45 0        /* adaptive Dormand–Prince 5(4): ocs2 IntegratorType::ODE45                                   */
#define HSQP_ROLLOUT_RK4 1          /* classical RK4, fixed step = initial_step, last step of a segment shortened                  */
#define HSQP_ROLLOUT_FEEDFORWARD 0  /* ocs2 FeedforwardController: u(t) interpolated as hsqp_evaluate_policy does                 */
#define HSQP_ROLLOUT_FEEDBACK 1     /* ocs2 LinearController: u(t, x) = uff(t) + K(t) x, as hsqp_evaluate_feedback_policy          */
#define HSQP_ROLLOUT_OK 0
#define HSQP_ROLLOUT_MAX_STEPS 1    /* step cap hit: this instance's outputs from that sample on are NaN                           */
#define HSQP_ROLLOUT_NONFINITE 2    /* a stage evaluation produced a non-finite value                                              */

typedef struct hsqp_rollout_settings {
  int32_t integrator, controller;   /* HSQP_ROLLOUT_ODE45 / _RK4, HSQP_ROLLOUT_FEEDFORWARD / _FEEDBACK */
  double abs_tol, rel_tol;          /* AbsTolODE, RelTolODE (ODE45 only)                                */
  double initial_step;              /* timeStep [s]                                                     */
  double max_steps_per_second;      /* maxNumStepsPerSecond                                             */
} hsqp_rollout_settings;

/* the rollout block of the reference's task.info (ODE45, AbsTolODE 1e-5, RelTolODE 1e-3, timeStep 0.015, maxNumStepsPerSecond 10000) with
 * the feed-forward controller (useFeedbackPolicy false) */
void hsqp_rollout_defaults(hsqp_rollout_settings* s);

/* s0 [B], x0 [B][58]; x [B][n_samples][58], u [B][n_samples][35], status / steps / rejected [B] (host memory) */
int hsqp_rollout_policy(hsqp_handle* h, const hsqp_rollout_settings* st, const double* s0, const double* x0, double duration, int n_samples,
                        double* x, double* u, int32_t* status, int32_t* steps, int32_t* rejected);
/* the same, every array argument in DEVICE memory of the handle's GPU (st: host memory) */
int hsqp_rollout_policy_device(hsqp_handle* h, const hsqp_rollout_settings* st, const double* d_s0, const double* d_x0, double duration, int n_samples,
                               double* d_x, double* d_u, int32_t* d_status, int32_t* d_steps, int32_t* d_rejected);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_ROLLOUT_H */
