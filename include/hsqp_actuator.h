/*
 * hsqp_actuator.h — an actuator model on the torque plant (hsqp_plant.h): a joint command that is sampled at a control rate and held, effort
 * limits, and passive joint torques (viscous damping and dry friction), evaluated inside every flow evaluation of hsqp_rollout_policy* and so of
 * every cycle of hsqp_loop_run*.  A resident setting of the handle.  The MPC never sees it: the iteration kernels, the node parameters and the
 * warm start are untouched.  With no actuator set, after hsqp_actuator_clear, with enabled = 0 or with the plant kind HSQP_PLANT_FLOW every
 * rollout is bit for bit what it was without this header; so is one under an enabled NEUTRAL setting (command_period 0, every limit +inf,
 * damping 0, friction 0).
 *
 * What it restates: the reference computes a joint command (q_des, qd_des, kp, kd, tau_ff) at mrtDesiredFrequency (500 Hz) and hands it to the
 * simulator, which at every simulator step forms the actuator effort from the HELD command and the CURRENT joint state
 * (MujocoSimInterface::simulationStep, getTotalFeedbackTorque) and clamps it to the actuator's force range.
 *
 * The model replaces step 3 of hsqp_plant.h for one flow evaluation at rollout time s and plant state x = [q; v]:
 *   command   (q_p, v_p, tau_ff, W_p):  command_period == 0: steps 1-2 of hsqp_plant.h at this evaluation (the continuous controller);
 *             command_period > 0: the values sampled at the last tick T_k <= s (below), held
 *   tau_cmd_j = tau_ff_j + kp_j (q_p_j - q_j) + kd_j (v_p_j - v_j)            (q, v ALWAYS the plant's current state)
 *   tau_act_j = min(max(tau_cmd_j, -effort_limit_j), +effort_limit_j)
 *   tau_pas_j = -damping_j v_j - friction_j v_j / sqrt(v_j^2 + v_s^2)         (v_s = friction_velocity)
 *   tau_j     = tau_act_j + tau_pas_j                                         (the passive torques are not clamped)
 * tau_j enters step 4 of hsqp_plant.h unchanged.  All of it is plain double arithmetic.
 *
 * Ticks (command_period > 0).  A rollout call samples at its own start: T_k = s0 + k * command_period, k = 0, 1, ..., each formed by that one
 * product and sum, never by accumulation.  A tick strictly inside a sample interval is a break point of the integration, beside the grid's
 * events and the push edges: the integrator restarts there.  A tick that coincides with an event, a push edge or a sample time samples once.
 * A sample time is not a tick: the held command runs on across the samples of one call.  At tick T_k, from the plant state x(T_k):
 *   the policy is evaluated at T_k + lookahead (clamped as the evaluators clamp); feedback controller: u_p = uff + K x(T_k), x_p the interpolated
 *   nominal state; tau_ff = the joint torques of hsqp_evaluate_policy at (x_p, u_p); q_p, v_p (the joint rows of x_p) and tau_ff are held until the
 *   next tick.  On the plant without a ground W_p = u_p[0..11] is held too; on the ground of hsqp_contact.h those wrenches are dropped as before.
 * The output u of a sample keeps its meaning: the controller's input at the sample time and state, without lookahead, evaluated continuously.
 * The step cap of the rollout (max_steps_per_second) bounds the work whatever the period: every interval between ticks costs at least one step,
 * so a period far below the step size ends the instance with HSQP_ROLLOUT_MAX_STEPS (so does a period too small to advance the time at all).
 *
 * hsqp_actuator_last: one record per instance of the most recent rollout (of the last completed cycle of the resident loop), written only while
 * the model is active: tau_cmd, tau_act and tau_pas at the instance's FINAL state of the last sample, under the command in force there — with a
 * held command the one sampled at the last tick before the end of the call, else the continuous one at the end time.  One more evaluation of the
 * joint law, no dynamics.  The rows of an instance that did not end with HSQP_ROLLOUT_OK are NaN.  |tau_cmd_j| > effort_limit_j is how a
 * caller sees saturation.
 *
 * ASSUMPTIONS:
 *   A1. Friction loss is a constraint in MuJoCo.  Here it is the regularised form the contact model uses for Coulomb friction: stick is
 *       approximate, a joint held by friction creeps back with a rate of about friction / (v_s (I + armature)).
 *   A2. Ticks restart with every call; in the resident loop that is once per MPC period, when the new policy arrives.  The reference's MRT thread
 *       runs on the wall clock, independent of policy arrival.
 *   A3. The clamp puts kinks in the flow, and a tick a jump; the ticks are break points, the kinks are not: there is no event detection
 *       (as C2 of hsqp_contact.h: ODE45 rejects and shortens steps, RK4 is first-order accurate across a kink).
 *   A4. The defaults for damping and friction are 0 (the reference's model file has neither), the default limits +inf (hsqp_model_desc carries
 *       none; the reference's actuatorfrcrange values are +-88 / +-139 / +-50 N m on the legs and +-25 N m on the arms).
 *
 * Lifetime: the setting belongs to the handle and survives what the contact setting survives (hsqp_upload*, hsqp_solve, hsqp_loop_start*,
 * hsqp_loop_reset_instances, the weight updates, hsqp_plant_set / _clear, hsqp_contact_*).  It acts only while the plant kind is
 * HSQP_PLANT_TORQUE; with HSQP_PLANT_FLOW it is stored and inert.  Whole-body handles only.
 *
 * Errors: HSQP_ERR_BAD_ARG, message in hsqp_last_error naming the entry point and the field, for a NULL argument, a centroidal handle,
 * reserved != 0, a negative or non-finite command_period, an effort_limit <= 0 or NaN ("joint J"), a negative or non-finite damping or
 * friction ("joint J"), a friction_velocity <= 0 or non-finite; hsqp_actuator_last*: a batch other than that of the rollout the record is of, or
 * no rollout on the actuator model since it was set.  A refused call leaves the previous setting in place.
 *
 * ABI: additions only — no public struct and no entry point of the other headers changes, so HSQP_ABI_VERSION (hsqp.h) needs no bump.
 */
#ifndef HSQP_ACTUATOR_H
#define HSQP_ACTUATOR_H

#include "hsqp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsqp_actuator_settings {
  int32_t enabled, reserved;        /* reserved == 0 */
  double command_period;            /* [s] >= 0, finite.  0: continuous controller; > 0: the joint command is sampled and held */
  double effort_limit[HSQP_NJ];     /* [N m] > 0, +inf allowed (no limit): clamp of the actuator torque */
  double damping[HSQP_NJ];          /* [N m s/rad] >= 0, finite */
  double friction[HSQP_NJ];         /* [N m] >= 0, finite: dry friction, regularised */
  double friction_velocity;         /* [rad/s] > 0, finite: v_s of the regularisation */
} hsqp_actuator_settings;

/* enabled 1, period 0.002 (mrtDesiredFrequency 500), limits +inf, damping 0, friction 0, v_s 0.01 */
void hsqp_actuator_defaults(hsqp_actuator_settings* s);
int hsqp_actuator_set(hsqp_handle* h, const hsqp_actuator_settings* s);
int hsqp_actuator_clear(hsqp_handle* h);
int hsqp_actuator_get(hsqp_handle* h, hsqp_actuator_settings* s);
/* tau_cmd, tau_act, tau_passive [batch][HSQP_NJ] each, any may be NULL */
int hsqp_actuator_last(hsqp_handle* h, int batch, double* tau_cmd, double* tau_act, double* tau_passive);
int hsqp_actuator_last_device(hsqp_handle* h, int batch, double* d_tau_cmd, double* d_tau_act, double* d_tau_passive);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_ACTUATOR_H */
