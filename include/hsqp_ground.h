/*
 * hsqp_ground.h — per-instance ground-height estimate from the stance feet of the MI355X SQP library, and the resident loop that follows it.
 *
 * Without this header the MPC of the resident loop (include/hsqp_loop.h) lives on one absolute ground: the height entry of the velocity command is a
 * world height, and hsqp_loop_settings::terrain_height — one constant for the batch and the run — is the stance-foot z reference, the lift-off and
 * the touch-down height of every swing.  On the terrain of include/hsqp_terrain.h (assumption T5 there) a robot two metres up a 5 degree ramp stands
 * 17 cm above that ground, is asked for a pelvis 17 cm too low and for feet landing under the surface, and the absolute box of
 * include/hsqp_episode.h reports a fall for a robot that is climbing.
 *
 * The reference has the mechanism for this: SwitchedModelReferenceManager::modifyReferences -> adaptToCurrentGroundHeight
 * (humanoid_common_mpc/src/reference_manager/SwitchedModelReferenceManager.cpp:83-104,140-154) estimates the ground from the contact-frame heights of
 * the feet the measured mode says are in contact (getGroundHeightEstimate, humanoid_common_mpc/src/pinocchio_model/DynamicsHelperFunctions.cpp:168-190),
 * shifts the base height of every target knot and hands the height to SwingTrajectoryPlanner::update(modeSchedule, terrainHeight).  This header
 * restates it on the device, per instance, with three DECLARED deviations from the reference's snapshot:
 *   (1) it is switched on: the snapshot overwrites the estimate (`terrainHeight = 0.0;`, line 89);
 *   (2) the knots are shifted by the estimate itself, not by its increment since the last call: the snapshot's increment is written for targets that
 *       persist across cycles; ours (and the reference's ProceduralMpcMotionManager's) are regenerated in every cycle from the absolute command;
 *   (3) the "last value" of the flight case is a latch per instance, not one function-local static shared by everybody (the treatment the command
 *       filter's static got in include/hsqp_loop.h).
 *
 * ---- the estimate of one instance
 * z_f: the world height of contact frame f (hsqp_model_desc::contact[f]) at the configuration part of the state row — forward kinematics down that leg.
 * mode = mode_sequence[lower_bound(event_times, t)]: the rule of the node parameters for a node at t, so the feet it selects are the ones the contact
 * flags of node 0 of a problem posed at t select.
 *   both feet in contact   raw = 0.5 (z_0 + z_1)
 *   one foot in contact    raw = its z
 *   flight                 the latch g is returned unchanged
 *   otherwise              g_new = filter_alpha == 0 ? raw : filter_alpha * g + (1 - filter_alpha) * raw       (0: the reference's raw estimate)
 * Every product-sum is evaluated unfused; given z_0 and z_1 the rule has no transcendental in it.
 *
 * ---- in the resident loop
 * hsqp_loop_ground switches the started loop, effective with the next cycle.  With it on, a cycle runs one more small kernel between step 1 (the
 * targets; the gait update where a gait is resident) and step 2: from the state the MPC reads (the observation of include/hsqp_observe.h when that
 * model is in force) at the cycle's problem time and the cycle's schedule it advances every instance's latch into a shadow, adds the new value to entry
 * 2 of the instance's three target knots (one IEEE add each: the command's height entry now means HEIGHT ABOVE THE ESTIMATED GROUND), and hands the
 * value to step 2 as that instance's terrain height in place of hsqp_loop_settings::terrain_height (stance-foot z, lift-off, touch-down).  The shadow
 * becomes the latch at step 5, like the filter state: a cycle that stops early leaves it where it was.  Under include/hsqp_episode.h an instance that
 * takes HSQP_WARM_COLD in a cycle (a new episode) starts from its g_init instead of its latch, and the knots of a parked instance are not shifted (its
 * stance command is absolute).  With box_above_ground the height test of the triage is on x[2] - g, g the latch the cycle has just committed.
 * So a cycle equals the caller making hsqp_command_targets, (hsqp_gait_update,) hsqp_ground_estimate, the three adds on the host,
 * hsqp_upload_reference_ground, hsqp_iterate_device and hsqp_rollout_policy, bit for bit.  Nothing new crosses to the host inside hsqp_loop_run.
 * OFF after every hsqp_loop_start / hsqp_loop_start_gait: a loop that never switches it on launches the kernels it always launched, and assumption
 * T5 of include/hsqp_terrain.h holds exactly while it is off.
 *
 * HSQP_ERR_BAD_ARG (message in hsqp_last_error, naming the entry point) for: a NULL handle / array / problem / reference, a centroidal handle
 * ("whole-body handles only"), a batch outside [1, max_batch], filter_alpha outside [0, 1), a non-finite initial_height, t, g, g_init or
 * terrain_heights (host arrays), max_events < 1, n_events outside [1, max_events] (host arrays), enabled / box_above_ground other than 0 / 1, the loop
 * entry points without a started loop, hsqp_loop_ground_state while the setting is off.  A refused call leaves the previous setting in place.
 *
 * Out of scope: the MPC reading the map's slope, contact detection from forces, metrics relative to the ground, centroidal handles, several GPUs.
 * (Per-foot lift-off / touch-down height sequences — the planner's three-argument update — read from the height map are include/hsqp_perceive.h; with
 * both settings on this one keeps its shift of the knots and its box, and step 2 takes that header's rows for the stance z, lift-off and touch-down.)
 *
 * ABI: additions only — no public struct and no entry point of the other headers changes, HSQP_ABI_VERSION stays.
 */
#ifndef HSQP_GROUND_H
#define HSQP_GROUND_H

#include "hsqp.h"
#include "hsqp_loop.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsqp_ground_settings {
  int32_t enabled, box_above_ground;   /* 0 / 1 each; box_above_ground: the base-height box of include/hsqp_episode.h is on x[2] - g */
  double filter_alpha;                 /* [0, 1); 0 = the raw estimate, as the reference */
  double initial_height;               /* the latch before the first contact, and after an episode reset (where g_init is not given) */
} hsqp_ground_settings;

/* enabled 1, box_above_ground 0, filter_alpha 0.0, initial_height 0.0 */
void hsqp_ground_defaults(hsqp_ground_settings* s);

/* Stand-alone.  x [B][58]; n_events [B], event_times [B][max_events], mode_sequence [B][max_events + 1] as hsqp_reference's; g [B] in / out: the
 * latch; foot_z [B][2] out, may be NULL: the heights of both contact frames.  Host arrays. */
int hsqp_ground_estimate(hsqp_handle* h, int batch, double t, const double* x, int max_events, const int32_t* n_events, const double* event_times,
                         const int32_t* mode_sequence, double filter_alpha, double* g, double* foot_z);
/* every array in DEVICE memory of the handle's GPU; the schedule and g are not checked */
int hsqp_ground_estimate_device(hsqp_handle* h, int batch, double t, const double* d_x, int max_events, const int32_t* d_n_events, const double* d_event_times,
                                const int32_t* d_mode_sequence, double filter_alpha, double* d_g, double* d_foot_z);

/* hsqp_upload_reference with one terrain height per instance, terrain_heights [B] (host), in place of ref->terrain_height (which is not read) */
int hsqp_upload_reference_ground(hsqp_handle* h, const hsqp_problem* problem, const hsqp_reference* ref, const double* terrain_heights);

/* the resident loop: after hsqp_loop_start / hsqp_loop_start_gait; NULL settings or enabled 0 switches it off; g_init [B] (host) or NULL: every instance's
 * initial_height.  Every call with the setting on puts every latch to its g_init; effective with the next cycle */
int hsqp_loop_ground(hsqp_handle* h, const hsqp_ground_settings* settings, const double* g_init);
/* the latches g [B] and the contact-frame heights foot_z [B][2] of the last completed cycle (the g_init and zeros before the first); either may be NULL */
int hsqp_loop_ground_state(hsqp_handle* h, double* g, double* foot_z);
int hsqp_loop_ground_state_device(hsqp_handle* h, double* d_g, double* d_foot_z);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_GROUND_H */
