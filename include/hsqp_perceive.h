/*
 * hsqp_perceive.h — per-foot swing heights read from the height map: the MPC of the MI355X SQP library sees the terrain of include/hsqp_terrain.h.
 *
 * Without this header the swing planner of the node parameters gets ONE height per instance (hsqp_reference::terrain_height, or the estimate of
 * include/hsqp_ground.h) and uses it three ways: as the stance reference of both feet, as the lift-off height and as the touch-down height of every
 * swing.  A foot about to land on a 3 cm ledge is planned to land 3 cm inside it; on a ramp both feet are planned onto one level (assumption T5 of
 * include/hsqp_terrain.h).
 *
 * The reference has the mechanism: SwingTrajectoryPlanner::update(modeSchedule, liftOffHeightSequence, touchDownHeightSequence)
 * (humanoid_common_mpc/src/swing_foot_planner/SwingTrajectoryPlanner.cpp:101-191) takes one height per foot and phase; its two-argument form, the one
 * hsqp_upload_reference restates, fills those sequences with a constant.  What the reference lacks is a source for the heights.  THE RULE BELOW THAT
 * FILLS THEM FROM THE RESIDENT HEIGHT MAPS IS OURS, not the reference's: it has no perception.
 *
 * ---- 1. the three-argument planner
 * hsqp_upload_reference_heights is hsqp_upload_reference with two rows per instance, lift_off [B][2][max_events + 1] and touch_down
 * [B][2][max_events + 1] (foot the outer index — 0 left, 1 right, as the contact flags — phase the inner), in place of ref->terrain_height, which is
 * not read.  Phase p of foot f reads lift_off[f][p] and touch_down[f][p] exactly where the reference reads liftOffHeightSequence[j][p] and
 * touchDownHeightSequence[j][p]: a stance phase has z = lift_off[f][p] with zero velocity and acceleration, the four swing cases are those of lines
 * 130-175.  touch_down already contains touchDownHeightOffset: the planner adds nothing to it.  Constant rows (g, g + offset) are the two-argument
 * form at terrain height g, bit for bit.  Entries of phases past n_events[b] are never read.
 *
 * ---- 2. the height sequences of one instance from the map
 * For foot f, state x, time t, schedule (n_events, event_times ev, mode_sequence seq) and target knots (target_times, target_states):
 *   c[p]   = foot f is in contact in mode seq[p];  p_now = lower_bound(ev, t), the phase of a node at t
 *   P      = the world xy of contact frame f at x (forward kinematics down that leg)
 *   o      = the xy of contact frame f with the base at the origin, zero Euler angles and the joints at the default joint state
 *            (hsqp_set_default_joint_state; without it the calls are refused)
 *   A contact run is a maximal range of consecutive phases with c true; a its first phase.  Its foothold F:
 *     a <= p_now   F = P: the foot stands there
 *     otherwise    t_c = ev[a - 1]; (X, Y, psi) = entries 0, 1, 3 of the clamped piece-wise linear interpolation of the knots at t_c (the desired-state
 *                  rule of the node parameters);  F = (X + cos psi o_x - sin psi o_y,  Y + sin psi o_x + cos psi o_y)
 *   Its height h = what hsqp_terrain_eval answers for the instance at F (steps 1-8 of include/hsqp_terrain.h: map -1 is the plane, a non-finite
 *   coordinate never becomes an index, clamps happen in double before any conversion to an integer).
 *   contact phase p of the run   lift_off[f][p] = h,  touch_down[f][p] = h + touch_down_height_offset,  foothold_xy[f][p] = F
 *   swing phase p                lift_off[f][p]   = h of the nearest run before it; none: the ground at P
 *                                touch_down[f][p] = h of the nearest run after it + offset; none: lift_off[f][p] + offset
 *                                foothold_xy[f][p] = F of the nearest run after it; none: P
 *   (in the no-run cases the planner reports its usual failure anyway: the values only have to be finite and defined)
 * Every product-sum is evaluated unfused.  An instance whose state row is not finite gets NaN rows and no map is read for it; entries of phases past
 * n_events are written 0.
 * hsqp_foot_heights needs maps and a placement table resident (hsqp_terrain_set_maps, hsqp_terrain_set_instances) and reads hsqp_contact.h's
 * per-instance ground height under the map, like hsqp_terrain_eval; whatever the plant kind, with no resident solution.
 *
 * ---- 3. in the resident loop
 * hsqp_loop_perceive switches the started loop, effective with the next cycle.  With it on, a cycle runs one more small kernel (k_foot_heights, one
 * lane per instance and foot) behind the targets of step 1, behind the gait update where a gait is resident and behind the ground estimate of
 * include/hsqp_ground.h where that is on: from the state the MPC reads (the observation of include/hsqp_observe.h when that model is in force) at the
 * cycle's problem time, the cycle's schedule and the cycle's targets (after the ground shift, if any) it writes every instance's rows, and step 2
 * takes the rows in place of the scalar or per-instance terrain height — for the stance z, the lift-off and the touch-down only: the ground setting
 * keeps its shift of the knots and its box.  So a cycle equals the caller making hsqp_command_targets, (hsqp_gait_update,) (hsqp_ground_estimate and
 * the adds,) hsqp_foot_heights, hsqp_upload_reference_heights, hsqp_iterate_device and hsqp_rollout_policy, bit for bit.  Nothing new crosses to the
 * host inside hsqp_loop_run.  Parked and restarted instances (include/hsqp_episode.h) take the same rule from their own state; an instance with a
 * non-finite state gets NaN rows and fails alone through the existing status path, the others go on bit for bit.
 * OFF after every hsqp_loop_start / hsqp_loop_start_gait: a loop that never switches it on launches the kernels it always launched.
 *
 * HSQP_ERR_BAD_ARG (message in hsqp_last_error, naming the entry point) for: a NULL handle / array / problem / reference, a centroidal handle
 * ("whole-body handles only"), a batch outside [1, max_batch], max_events < 1, n_knots < 1, a non-finite t, n_events outside [1, max_events] (host
 * arrays), a non-finite lift_off / touch_down entry in phases 0 .. n_events[b], no default joint state, no maps or no placement table resident
 * (hsqp_foot_heights*, hsqp_loop_perceive), enabled other than 0 / 1, reserved != 0, the loop entry points without a started loop,
 * hsqp_loop_foot_heights while the setting is off.  A refused call leaves the previous setting in place.
 *
 * Out of scope: the slope or a foot orientation in the MPC, base-height knots that follow the map ahead, foothold optimisation or avoidance of edges,
 * centroidal handles, several GPUs.
 *
 * ABI: additions only — no public struct and no entry point of the other headers changes, HSQP_ABI_VERSION stays.
 */
#ifndef HSQP_PERCEIVE_H
#define HSQP_PERCEIVE_H

#include "hsqp.h"
#include "hsqp_loop.h"
#include "hsqp_terrain.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hsqp_perceive_settings {
  int32_t enabled, reserved;   /* enabled 0 / 1; reserved == 0 */
} hsqp_perceive_settings;

/* enabled 1, reserved 0 */
void hsqp_perceive_defaults(hsqp_perceive_settings* s);

/* hsqp_upload_reference with the planner's three-argument update: lift_off, touch_down [B][2][max_events + 1] (host), B = problem->batch and
 * max_events = ref->max_events; ref->terrain_height is not read */
int hsqp_upload_reference_heights(hsqp_handle* h, const hsqp_problem* problem, const hsqp_reference* ref, const double* lift_off, const double* touch_down);

/* Stand-alone.  x [B][58]; n_events [B], event_times [B][max_events], mode_sequence [B][max_events + 1], target_times [B][n_knots], target_states
 * [B][n_knots][58] as hsqp_reference's; touch_down_height_offset: hsqp_swing_config's; lift_off, touch_down [B][2][max_events + 1] out; foothold_xy
 * [B][2][max_events + 1][2] out, may be NULL.  Host arrays. */
int hsqp_foot_heights(hsqp_handle* h, int batch, double t, const double* x, int max_events, const int32_t* n_events, const double* event_times,
                      const int32_t* mode_sequence, int n_knots, const double* target_times, const double* target_states, double touch_down_height_offset,
                      double* lift_off, double* touch_down, double* foothold_xy);
/* every array in DEVICE memory of the handle's GPU; the schedule and the targets are not checked */
int hsqp_foot_heights_device(hsqp_handle* h, int batch, double t, const double* d_x, int max_events, const int32_t* d_n_events, const double* d_event_times,
                             const int32_t* d_mode_sequence, int n_knots, const double* d_target_times, const double* d_target_states,
                             double touch_down_height_offset, double* d_lift_off, double* d_touch_down, double* d_foothold_xy);

/* the resident loop: after hsqp_loop_start / hsqp_loop_start_gait; NULL settings or enabled 0 switches it off; effective with the next cycle */
int hsqp_loop_perceive(hsqp_handle* h, const hsqp_perceive_settings* settings);
/* the rows of the last completed cycle (zeros before the first; a cycle that stops behind the kernel has written its own): lift_off, touch_down
 * [B][2][max_events + 1], foothold_xy [B][2][max_events + 1][2], max_events that of the loop's schedule (a resident gait: its settings'); any may be NULL */
int hsqp_loop_foot_heights(hsqp_handle* h, double* lift_off, double* touch_down, double* foothold_xy);
int hsqp_loop_foot_heights_device(hsqp_handle* h, double* d_lift_off, double* d_touch_down, double* d_foothold_xy);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_PERCEIVE_H */
