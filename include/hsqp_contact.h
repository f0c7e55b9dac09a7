/*
 * hsqp_contact.h — a ground under the torque plant (hsqp_plant.h): compliant contact with Coulomb friction at the four corners of both soles,
 * evaluated inside every flow evaluation of hsqp_rollout_policy* and so of every cycle of hsqp_loop_run*.  A resident setting of the handle, with
 * a per-instance table of ground height and friction coefficient.  The MPC never sees it: the iteration kernels, the node parameters, the warm
 * start and the cone of the MPC (hsqp_model_desc::friction_mu) are untouched.  With no contact set, after hsqp_contact_clear, with enabled = 0
 * or with the plant kind HSQP_PLANT_FLOW every rollout is bit for bit what it was without this header.
 *
 * The model, for one flow evaluation of HSQP_PLANT_TORQUE at the plant's own state (q, v) (step 4 of hsqp_plant.h):
 *   points    foot f in {0, 1}, corner c in {0 .. 3}: p_fc = contact_p[f] + (x, y, 0) in the axes of contact_body[f], (x, y) the corners of the
 *             model's contact rectangle in the order (x_min, y_min), (x_max, y_min), (x_max, y_max), (x_min, y_max).  P: the world position of
 *             the point, Pdot: its world velocity.  Point index = 4 f + c.
 *   normal    d = ground_height - P_z (penetration), ddot = -Pdot_z;  fn = max(0, k d (1 + c ddot)) for d > 0, else 0  (Hunt-Crossley, exponent 1)
 *   friction  ft = -mu fn v_t / sqrt(|v_t|^2 + v_s^2),  v_t = (Pdot_x, Pdot_y)  (regularised Coulomb: |ft| < mu fn, ~ mu fn once |v_t| >> v_s)
 *   wrench    the force (ft_x, ft_y, fn) acts at P: like a push of hsqp_push.h it enters the base rows and the row of every joint between the
 *             base and the foot.
 *   policy    with contact on, the prescribed term sum_feet J^T W of step 4 is DROPPED on the plant: the ground reaction is the model's, not
 *             the MPC's plan.  The feed-forward effort tau_ff of step 2 is still formed from (x_p, u_p) with the policy's wrenches, unchanged.
 * The ground is a horizontal plane (hsqp_terrain.h puts a per-instance height map under it: the height and the normal then come from the map under
 * each point, everything else of this header holds).  All of it is plain double arithmetic.
 *
 * ASSUMPTIONS (stated here the way hsqp_rollout.h states those of its integrators):
 *   C1. This is a penalty model, NOT the soft-constraint contact solver of the MuJoCo front end of the reference, which cannot be restated
 *       here: forces, penetrations and stick / slip transitions differ from that simulator's.  No self-collision, no geometry other than the
 *       eight sole corners, no torsional or rolling friction.
 *   C2. The force is continuous at touchdown (fn = 0 at d = 0) but has a kink there, and another where a separating point's force is clamped
 *       at zero (ddot < -1 / c).  There is no event detection: HSQP_ROLLOUT_ODE45's step control handles the kinks by rejecting and shortening
 *       steps; with HSQP_ROLLOUT_RK4 the step is the caller's choice and a step across a kink is first-order accurate.
 *   C3. The defaults are design choices, not measurements: stiffness 5e4 N/m per point (static penetration m g / (8 k) ~ 0.9 mm for the
 *       35.1 kg G1), damping 10 s/m, slip velocity 0.01 m/s, ground height 0, mu = the model's friction_mu — the ground the MPC assumes.
 *       (The MuJoCo model file of the reference uses a friction coefficient of 3.0.)
 *
 * Lifetime: the setting and the table belong to the handle and survive what the plant setting survives (hsqp_upload*, hsqp_solve,
 * hsqp_loop_start*, hsqp_loop_reset_instances, the weight updates, hsqp_plant_set / _clear).  The setting acts only while the plant kind is
 * HSQP_PLANT_TORQUE; with HSQP_PLANT_FLOW it is stored and inert.  Whole-body handles only.
 *
 * The per-instance table gives instance b its own ground_height and mu (terrain-height and friction randomisation across a batch);
 * instances past the table's batch, and every instance without a table, take the setting's values.  A new hsqp_contact_set keeps the table.
 *
 * hsqp_contact_eval evaluates the model at given states with the handle's setting and table — whatever `enabled` and the plant kind are, and
 * with no resident solution: force[b][f][c] = (ft_x, ft_y, fn) in world axes, penetration[b][f][c] = d (negative above the ground).  It is
 * how a caller logs ground reaction forces.
 *
 * Errors: HSQP_ERR_BAD_ARG, message in hsqp_last_error naming the entry point, for a NULL argument, a centroidal handle, reserved != 0, a
 * non-finite field, stiffness <= 0, damping < 0, mu < 0, slip_velocity <= 0, batch outside [1, max_batch], and a non-finite or negative-mu
 * table entry (host arrays only: device arrays are not read back).
 *
 * ABI: additions only — no public struct and no entry point of the other headers changes, so HSQP_ABI_VERSION (hsqp.h) needs no bump.
 */
#ifndef HSQP_CONTACT_H
#define HSQP_CONTACT_H

#include "hsqp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSQP_CONTACT_FEET    2
#define HSQP_CONTACT_CORNERS 4

typedef struct hsqp_contact_settings {
  int32_t enabled, reserved;       /* reserved == 0 */
  double stiffness;                /* k  [N/m] per point, > 0 */
  double damping;                  /* c  [s/m], >= 0 */
  double mu;                       /* >= 0 */
  double slip_velocity;            /* v_s [m/s], > 0 */
  double ground_height;            /* [m] */
} hsqp_contact_settings;

typedef struct hsqp_contact_ground { double height, mu; } hsqp_contact_ground;   /* per instance */

/* enabled 1, 5e4, 10, the model's friction_mu, 0.01, 0.  A NULL handle leaves mu NaN (hsqp_contact_set refuses it): fill it in. */
void hsqp_contact_defaults(const hsqp_handle* h, hsqp_contact_settings* s);
int hsqp_contact_set(hsqp_handle* h, const hsqp_contact_settings* s);
/* ground [batch]; NULL: no table — every instance back to the setting's values */
int hsqp_contact_set_instances(hsqp_handle* h, int batch, const hsqp_contact_ground* ground);
int hsqp_contact_set_instances_device(hsqp_handle* h, int batch, const hsqp_contact_ground* d_ground);
int hsqp_contact_clear(hsqp_handle* h);             /* contact off, no table */
int hsqp_contact_get(hsqp_handle* h, hsqp_contact_settings* s);
/* x [batch][58]; force [batch][2][4][3], penetration [batch][2][4]: either may be NULL */
int hsqp_contact_eval(hsqp_handle* h, int batch, const double* x, double* force, double* penetration);
int hsqp_contact_eval_device(hsqp_handle* h, int batch, const double* d_x, double* d_force, double* d_penetration);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_CONTACT_H */
