/*
 * hsqp_cent_loop.h — the resident closed MPC loop (hsqp_loop.h) for the CENTROIDAL formulation.
 *
 * What a batch user of the centroidal MPC otherwise does on the host in every cycle, the way the reference's CentroidalMpcSqpNode does it:
 * the TargetTrajectories from the measured state and the filtered velocity command
 *   (humanoid_centroidal_mpc CentroidalMpcTargetTrajectoriesCalculator::commandedVelocityToTargetTrajectories),
 * then hsqp_upload_reference, hsqp_iterate_device, hsqp_rollout_policy.  The entry points of hsqp_loop.h refuse a centroidal handle (their
 * generator reads the base velocity from the whole-body state row); the three below are their centroidal forms, and they refuse a whole-body
 * handle with "centroidal handles only".
 *
 * ---- velocity-command targets
 * The arrays of hsqp_command_targets: v_cmd [B][4] = {vx, vy, height, yaw rate}, v_filt [B][4] (in / out), x0 [B][58] — a centroidal state
 * row [h/m (6) | base pose (6) | joints (23) | 23 zeros] — target_times [B][3], target_states [B][3][58] (entries 35..57 of every knot zero).
 *   v_filt <- filter_alpha v_filt + (1 - filter_alpha) v_cmd, filter_alpha == 0 takes the command itself;
 *   vb = [pdot; euler rates] of the base at x0 from the centroidal momentum, vb = A_b(q)^-1 (m h) with q = x0[6..34], the joint rates and
 *   the wrenches zero (the reference: "assumes no joint velocities") — a walk over the kinematic tree and a 3 x 3 solve per instance, on the
 *   device;
 *   the filtered command rotated by the yaw x0[9]; pose = {x0[6], x0[7], height, x0[9], 0, 0}; knots at t0, t0 + 0.7 horizon, t0 + horizon;
 *   the mid knot integrated with ((vb[0] + gvx) / 2, (vb[1] + gvy) / 2, (vb[5] + wz) / 2) — vb[5], the euler X rate, is read where a yaw rate
 *   is meant: the reference reads that entry and this library reproduces it — the last knot with the command;
 *   a knot's state row is [gvx, gvy, 0, 0, 0, wz / m | pose | default joint state | 23 zeros].
 * base_vel [B][6] (may be NULL): the by-product vb of every instance.
 * The solve uses the momentum m h (reference.centroidal_base_velocity); DESIGN.md records why and where the other reading would go.
 * A default joint state must be set (hsqp_set_default_joint_state).
 *
 * ---- the resident loop
 * hsqp_loop_start_centroidal is hsqp_loop_start on a centroidal handle.  After it hsqp_loop_run*, hsqp_loop_command* and hsqp_loop_state* work
 * unchanged: step 1 of a cycle runs the generator above, steps 2 to 5 the code of the public calls, so a loop equals the calls
 * hsqp_centroidal_command_targets, hsqp_upload_reference (COLD, then SHIFT), hsqp_iterate_device, hsqp_rollout_policy made by the caller, bit
 * for bit.  Resident pushes (hsqp_push.h) act in step 4 as they do in hsqp_rollout_policy on a centroidal handle.
 * hsqp_loop_defaults keeps its values on a centroidal handle: they are the WHOLE-BODY task file's (dt 0.035, 60 Hz).  The centroidal task's
 * sqp dt and MPC frequency are the caller's to set from the exported model's sqp block.
 * Failure isolation (hsqp_episode.h: hsqp_loop_isolate, hsqp_loop_reset_instances, hsqp_loop_episodes*) works on this loop; the height and
 * tilt box is read at the centroidal pose (x[8], x[10], x[11]) and the stance command of a parked instance takes x_reset[8].  x_reset and
 * reset states must have zero padding.
 *
 * HSQP_ERR_BAD_ARG (message in hsqp_last_error): what the whole-body entries refuse, and: a whole-body handle ("centroidal handles only"), no
 * default joint state, host arrays with a non-zero entry 35..57 in an x0 row (the message of hsqp_upload).  The device twin checks neither
 * v_cmd nor the padding.
 *
 * Out of scope (each still answers "whole-body handles only"): the resident gait ladder (hsqp_gait.h; it would read base_vel in place of the
 * whole-body velocity block), the event grid, the ground estimate, perception, the observation model and the metrics on centroidal handles;
 * the torque plant; commandedPositionToTargetTrajectories; several GPUs.
 *
 * ABI: additions only, HSQP_ABI_VERSION stays.
 */
#ifndef HSQP_CENT_LOOP_H
#define HSQP_CENT_LOOP_H

#include "hsqp_loop.h"

#ifdef __cplusplus
extern "C" {
#endif

/* host arrays; base_vel [B][6] may be NULL */
int hsqp_centroidal_command_targets(hsqp_handle* h, int batch, const double* v_cmd, double* v_filt, double filter_alpha, const double* x0, double t0,
                                    double horizon, double* target_times, double* target_states, double* base_vel);
/* every array in DEVICE memory of the handle's GPU; neither v_cmd nor the padding of x0 is checked */
int hsqp_centroidal_command_targets_device(hsqp_handle* h, int batch, const double* d_v_cmd, double* d_v_filt, double filter_alpha, const double* d_x0,
                                           double t0, double horizon, double* d_target_times, double* d_target_states, double* d_base_vel);
/* the arguments of hsqp_loop_start; x0 [B][58] centroidal state rows with zero padding */
int hsqp_loop_start_centroidal(hsqp_handle* h, const hsqp_loop_settings* settings, int batch, double t0, const double* x0, const double* v_cmd,
                               int max_events, const int32_t* n_events, const double* event_times, const int32_t* mode_sequence);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_CENT_LOOP_H */
