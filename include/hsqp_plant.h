/*
 * hsqp_plant.h — the plant of the batched policy rollout (hsqp_rollout.h) and, through it, of the resident closed loop (hsqp_loop.h): a
 * resident setting that chooses between the MPC's own flow map (what every rollout integrates by default) and a torque-level plant, full
 * forward dynamics of the whole-body tree under the joint PD law of the reference's WBMpcMrtJointController::computeJointControlAction
 * (humanoid_wb_mpc/src/mrt/WBMpcMrtJointController.cpp:125-194), which sends q_des, qd_des, a feed-forward effort and kp / kd to a
 * rigid-body simulator.  The MPC never sees the setting: the iteration kernels, the node parameters and the warm start are untouched.
 * With no plant set, after hsqp_plant_clear, or with kind = HSQP_PLANT_FLOW every rollout is bit for bit what it was without this header.
 *
 * Lifetime: the setting belongs to the handle.  It survives hsqp_upload*, hsqp_solve, hsqp_loop_start*, hsqp_loop_reset_instances and the
 * weight updates; hsqp_plant_clear or a new hsqp_plant_set replaces it.  Whole-body handles only.
 *
 * HSQP_PLANT_TORQUE: one flow evaluation of hsqp_rollout_policy* (and so of every cycle of hsqp_loop_run*) at rollout time s and plant state
 * x = [q; v]:
 *   1. policy     (x_p, u_p) at s + lookahead, clamped as the evaluators clamp.  Feed-forward controller: the interpolated state and input of
 *                 hsqp_evaluate_policy.  Feedback controller: u_p = uff + K x with the measured plant state x and x_p the interpolated nominal
 *                 state — the arithmetic of hsqp_evaluate_feedback_policy; the gain window of the call covers + lookahead.
 *   2. effort     tau_ff = the joint torques of hsqp_evaluate_policy at (x_p, u_p).
 *   3. joint law  tau_j = tau_ff,j + kp_j (q_p,j - q_j) + kd_j (v_p,j - v_j).
 *   4. dynamics   vd = (M(q) + diag(0_6, armature))^-1 ([0; tau] + sum_feet J^T W - nle(q, v) + sum_pushes J_P^T f),   xdot = [v; vd],
 *                 with the contact wrenches W = u_p[0..11] applied at the plant's own contact frames (no contact model: the wrenches stay
 *                 prescribed) and the complete 29 x 29 mass matrix in the coordinates of the state (world linear velocity, euler rates,
 *                 joint rates), the linear / angular coupling of the base included.
 *   5. pushes     a push of hsqp_push.h acts through the whole tree: its wrench about the base origin enters the base rows, and the row
 *                 of every joint between the base and the pushed body.  Edges, activity per segment and break points are unchanged.
 * A pivot of the factorisation that is not positive gives a non-finite xdot and ends the instance with HSQP_ROLLOUT_NONFINITE.  The outputs x,
 * u, status, steps and rejected keep their meaning; u is the controller's input at the sample time, without lookahead.
 *
 * Stiffness: with the reference's gains the joint law has rates up to (M^-1)_jj kd ~ 3e4 1/s on the lightest joints (smallest joint
 * inertia 3.9e-4 kg m^2), so an explicit integrator needs steps of ~0.1 ms; simulators add rotor armature to the joint diagonal of M, which is
 * what `armature` is.  The controller is continuous (evaluated at every stage) unless hsqp_actuator.h says otherwise: a sampled
 * and held joint command, effort limits, joint friction and damping are that header's (its joint law replaces step 3).  Not modelled: the
 * centroidal formulation.  The plant's inertial parameters are the model's unless hsqp_inertia.h gives an instance its own (link mass scales,
 * payloads).  Contact and friction on the plant: hsqp_contact.h (a ground under the feet; with it set, the prescribed wrenches of
 * step 4 give way to the contact model's forces).
 *
 * Errors: HSQP_ERR_BAD_ARG, message in hsqp_last_error, for a NULL argument, a centroidal handle, an unknown kind, reserved != 0, and a
 * negative or non-finite lookahead, kp, kd or armature entry.
 *
 * ABI: additions only — no public struct and no entry point of the other headers changes, so HSQP_ABI_VERSION (hsqp.h) needs no bump.
 */
#ifndef HSQP_PLANT_H
#define HSQP_PLANT_H

#include "hsqp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSQP_PLANT_FLOW   0   /* the MPC's own flow map: what every rollout is without a setting */
#define HSQP_PLANT_TORQUE 1   /* forward dynamics under the joint PD law above */

typedef struct hsqp_plant_settings {
  int32_t kind, reserved;          /* reserved == 0 */
  double lookahead;                /* [s] >= 0: the policy is evaluated at s + lookahead (reference: 0.005) */
  double kp[HSQP_NJ], kd[HSQP_NJ]; /* >= 0, finite (reference: 1200, 10 on every MPC joint) */
  double armature[HSQP_NJ];        /* >= 0, finite [kg m^2]: added to the joint diagonal of M (default 0) */
} hsqp_plant_settings;

void hsqp_plant_defaults(hsqp_plant_settings* s);   /* TORQUE, 0.005, 1200, 10, 0 */
int hsqp_plant_set(hsqp_handle* h, const hsqp_plant_settings* s);
int hsqp_plant_clear(hsqp_handle* h);               /* back to HSQP_PLANT_FLOW */
int hsqp_plant_get(hsqp_handle* h, hsqp_plant_settings* s);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_PLANT_H */
