/*
 * hsqp_inertia.h — per-instance inertial variations of the torque plant (hsqp_plant.h): a scale on the mass and rotational inertia of every link
 * and up to HSQP_INERTIA_PAYLOADS rigid payloads, applied inside every flow evaluation of hsqp_rollout_policy* and so of every cycle of
 * hsqp_loop_run*.  A resident per-instance table of the handle, of the PLANT ONLY.  The MPC never sees it: the iteration kernels, the node
 * parameters, the warm start, hsqp_joint_torques, hsqp_evaluate_policy and the feed-forward effort tau_ff of step 2 of hsqp_plant.h (formed at
 * (x_p, u_p) on the handle's nominal model) are untouched — that is the model mismatch being modelled: a robot 15 % heavier than the controller
 * believes, or one that carries 5 kg on the torso.  With no table, after hsqp_inertia_clear, with the plant kind HSQP_PLANT_FLOW, or under a table
 * whose entries are all neutral (every scale 1, no payload) every rollout is bit for bit what it was without this header.
 *
 * The model, for one flow evaluation of HSQP_PLANT_TORQUE at the plant's own state (q, v) (step 4 of hsqp_plant.h).  The plant's mass matrix and
 * bias forces are formed from the spatial inertia In_i of every link about the base origin and the net force f_i = In_i a_i + v_i x* In_i v_i on
 * it (gravity in a_i); both are LINEAR in the link's inertial parameters (m, m c, I), because the Newton-Euler equations are.  So, before anything
 * is summed over the tree:
 *   scales    In_i <- s_i In_i,  f_i <- s_i f_i,  s_i = mass_scale[i]: mass AND rotational inertia of link i times s_i, its centre of mass kept
 *   payloads  payload p on link b adds the spatial inertia about the base origin and the net force of a rigid body (m_p, R_b com_p + r_b,
 *             R_b I_p R_b^T), formed the way a link's are; it is rigidly attached, so it shares the link's velocity and acceleration.
 *             Mass scales do not apply to payloads.
 * Everything downstream does not depend on the inertial model and is untouched: contact forces (hsqp_contact.h), pushes (hsqp_push.h), the
 * actuator law (hsqp_actuator.h) and the armature.  All of it is plain double arithmetic.
 *
 * ASSUMPTIONS:
 *   I1. A scale keeps the link's centre of mass and the shape of its inertia tensor: the link's density is scaled.  Anything else about a link
 *       is a payload.
 *   I2. A payload is rigid and fixed in its link's frame; it has no geometry: it does not collide, and on a foot link it does not move the
 *       contact points.
 *   I3. Kinematics are the nominal model's.  Out of scope: per-instance joint placements, link lengths or anything else that changes
 *       kinematics; variation of the MPC's own model; the centroidal formulation; several GPUs.
 *
 * Lifetime: the table belongs to the handle and survives hsqp_upload*, hsqp_solve, hsqp_loop_start*, hsqp_loop_reset_instances (a restarted
 * instance keeps its body), the weight updates, hsqp_plant_set / _clear, hsqp_contact_* and hsqp_actuator_*.  It acts only while the plant kind
 * is HSQP_PLANT_TORQUE; with HSQP_PLANT_FLOW it is stored and inert.  Instances past the table's batch are neutral.  Whole-body handles only.
 *
 * hsqp_inertia_eval evaluates the plant's inertial model at given states with instance b's entry — whatever the plant kind, and with no resident
 * solution: M[b] the 29 x 29 mass matrix in the coordinates of the state, WITHOUT armature, both triangles filled; nle[b] the bias forces (the
 * right-hand side of step 4 negated, with tau = 0, no wrenches and no pushes); mass[b] the total mass.  With no table it gives the nominal model's.
 *
 * Errors: HSQP_ERR_BAD_ARG, message in hsqp_last_error naming the entry point, the instance and the field ("instance 2: mass_scale[7]",
 * "instance 0: payload 1: inertia"), for a NULL handle, a centroidal handle, batch outside [1, max_batch] (hsqp_inertia_set_instances with NULL
 * also takes 0), reserved != 0, a scale <= 0 or non-finite, n_payloads outside [0, HSQP_INERTIA_PAYLOADS], a payload body outside [0, HSQP_NB),
 * a negative or non-finite payload mass, a non-finite com, and a payload inertia that is non-finite or not positive semidefinite (a negative
 * principal minor; a minor may be negative by rounding, 16 eps of trace^2 / trace^3, so that a rod or a plate rotated into the link's axes passes).
 * Only the first n_payloads payloads are looked at.  Host arrays only are checked: device arrays are not read back, and the kernels clamp a
 * device table's n_payloads into the range and ignore a body outside it.  A refused call leaves the previous table in place; a HIP error while
 * the table is copied (HSQP_ERR_HIP, HSQP_ERR_OOM), unlike a refusal, leaves NO table.
 *
 * ABI: additions only — no public struct and no entry point of the other headers changes, so HSQP_ABI_VERSION (hsqp.h) needs no bump.
 */
#ifndef HSQP_INERTIA_H
#define HSQP_INERTIA_H

#include "hsqp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSQP_INERTIA_PAYLOADS 2

typedef struct hsqp_inertia_payload {
  int32_t body, reserved;   /* link index 0 .. HSQP_NB-1 (0: the base), reserved == 0 */
  double mass;              /* [kg] >= 0, finite */
  double com[3];            /* [m] its centre of mass in the axes and from the origin of the link's body frame, finite */
  double inertia[6];        /* [kg m^2] xx, xy, xz, yy, yz, zz about ITS com, link axes; positive semidefinite (all zero: a point mass) */
} hsqp_inertia_payload;

typedef struct hsqp_inertia_instance {
  double mass_scale[HSQP_NB];      /* > 0, finite: mass AND rotational inertia of link i times s_i, its com kept */
  int32_t n_payloads, reserved;    /* 0 .. HSQP_INERTIA_PAYLOADS */
  hsqp_inertia_payload payload[HSQP_INERTIA_PAYLOADS];
} hsqp_inertia_instance;

/* neutral: every scale 1, no payload, everything else 0 */
void hsqp_inertia_defaults(hsqp_inertia_instance* v);
/* table [batch]; NULL (batch 0 .. max_batch): no table */
int hsqp_inertia_set_instances(hsqp_handle* h, int batch, const hsqp_inertia_instance* table);
int hsqp_inertia_set_instances_device(hsqp_handle* h, int batch, const hsqp_inertia_instance* d_table);   /* not checked */
int hsqp_inertia_clear(hsqp_handle* h);
/* table [batch]: the entries in force; instances past the table: neutral */
int hsqp_inertia_get_instances(hsqp_handle* h, int batch, hsqp_inertia_instance* table);
/* x [batch][58]; M [batch][29][29] (no armature), nle [batch][29], mass [batch]: any may be NULL */
int hsqp_inertia_eval(hsqp_handle* h, int batch, const double* x, double* M, double* nle, double* mass);
int hsqp_inertia_eval_device(hsqp_handle* h, int batch, const double* d_x, double* d_M, double* d_nle, double* d_mass);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_INERTIA_H */
