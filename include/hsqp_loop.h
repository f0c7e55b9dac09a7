/*
 * hsqp_loop.h — the closed MPC loop of the MI355X SQP library, resident on the device, with per-instance velocity commands.
 *
 * Two things a batch caller otherwise does on the host between MPC cycles:
 *  (1) the TargetTrajectories of every cycle, rebuilt from the MEASURED state and the filtered velocity command
 *      (humanoid_common_mpc ProceduralMpcMotionManager::preSolverRun -> WBMpcTargetTrajectoriesCalculator::
 *      commandedVelocityToTargetTrajectories(filteredCmd, initTime, finalTime, initState)): hsqp_command_targets;
 *  (2) the cycle itself — targets, hsqp_upload_reference with the device-built warm start, hsqp_iterate_device,
 *      hsqp_rollout_policy_device over one MPC period, the rolled-out state as the next measured state: hsqp_loop_*.
 * Whole-body handles only: on a centroidal handle every entry point below returns HSQP_ERR_BAD_ARG with a message saying so (its generator
 * needs the base velocity from the centroidal momentum); the centroidal forms are in include/hsqp_cent_loop.h.
 *
 * ---- velocity-command targets
 * v_cmd [B][4] = {vx, vy, height, yaw rate} (WalkingVelocityCommand::toVector), v_filt [B][4] the filter state (in / out), x0 [B][58]:
 *   v_filt <- filter_alpha v_filt + (1 - filter_alpha) v_cmd   (TargetTrajectoriesCalculatorBase::filterAndTransformVelCommandToLocal; the
 *                                                               reference calls it with 0.8)
 *   the filtered command rotated by x0's yaw; roll and pitch zeroed; knots at t0, t0 + 0.7 horizon, t0 + horizon; the mid knot integrated
 *   with the mean of the measured and the commanded base velocity, the last one with the commanded velocity; joints at the model's default
 *   joint state; the target velocity in the velocity block.
 * filter_alpha == 0 takes the command itself, whatever v_filt held (the filter at steady state).  The reference's filter state is ONE
 * function-local static shared by every caller; here each instance owns its own, which is what a batch needs.
 * Out: target_times [B][3], target_states [B][3][58], the layout hsqp_reference takes (n_knots = 3).
 * The default joint state (reference.info defaultJointState) is not part of hsqp_model_desc: hand it over once with
 * hsqp_set_default_joint_state; until then the generator and the loop return HSQP_ERR_BAD_ARG.
 *
 * ---- the resident loop
 * hsqp_loop_start uploads the state, the commands and the mode schedules ONCE.  hsqp_loop_run(n_cycles) then runs, for every cycle at time t
 * with measured state x, entirely from resident buffers:
 *   1. the targets from (v_cmd, v_filt, x, t, horizon = n_nodes * dt);
 *   2. the work of hsqp_upload_reference with x_init = x, the resident mode schedule, those targets, the uniform grid at t0 = t, and
 *      warm_start = HSQP_WARM_COLD in the first cycle after hsqp_loop_start, HSQP_WARM_SHIFT afterwards;
 *   3. the work of hsqp_iterate_device(h, iterations, iterate_flags);
 *   4. the work of hsqp_rollout_policy_device with s0 = 0, x0 = x, duration = period, n_samples = 1;
 *   5. x <- the rolled-out state, t <- t + period (accumulated in this order, so n cycles give the t of n additions); the sample's x, u go
 *      to row c of the logs.
 * Steps 2 to 4 run the code of the public calls, so a loop equals the same calls made by the caller bit for bit.  Inside hsqp_loop_run no
 * array whose size grows with B crosses between host and device except the per-instance int32 status words the public calls read themselves
 * (DESIGN.md lists them); host logs are copied once, after the last cycle.
 *
 * Stopping: if step 2, 3 or 4 returns anything but HSQP_OK the loop ends after that step and returns that code; *cycles_done counts the
 * cycles that completed all five steps, hsqp_loop_state answers with the last completed cycle's state (t, x, v_filt), and the log rows of the
 * completed cycles are delivered.  The loop stays started: a later hsqp_loop_run goes on from that state, with the warm start of the
 * situation (COLD if no cycle has completed).  The policy, feedback and rollout entry points stay valid on the resident solution of the last
 * completed iteration, by their own rules.  Any hsqp_upload* or hsqp_solve call ends the loop: hsqp_loop_run / _command / _state then
 * return HSQP_ERR_BAD_ARG until hsqp_loop_start is called again.
 *
 * HSQP_ERR_BAD_ARG (message in hsqp_last_error) also for: a NULL handle / settings / array, batch outside [1, max_batch], n_nodes outside
 * [1, max_nodes], a non-finite or non-positive period or dt, filter_alpha outside [0, 1), iterations < 1, iterate_flags with
 * HSQP_ITER_UNTIL_CONVERGED (its per-iteration read-back grows with B; the reference runs sqpIteration = 1 per cycle), rollout settings
 * hsqp_rollout_policy refuses, n_events outside [1, max_events], n_cycles < 1, a non-finite command (host arrays) or t0.  Start states are
 * not checked: a non-finite one surfaces the way it does in the underlying calls (HSQP_ERR_NUMERIC from the solution's status).
 *
 * The gait auto-transition of preSolverRun (transitionToFasterGait / ...Slower...) and the re-tiling of the schedule in every cycle are in
 * include/hsqp_gait.h: hsqp_loop_start_gait starts this loop with a per-instance gait schedule and ladder resident on the device.
 * The measured state x of steps 1 and 2 IS the plant's state unless include/hsqp_observe.h says otherwise: a resident observation model (bias,
 * noise, sensor and compute delay) between the plant's state and everything the MPC reads; with none set the cycle is exactly the one above.
 * The uniform grid of step 2 is the default: include/hsqp_grid.h switches the started loop to ocs2's event-node grid (hsqp_reference::node_times),
 * built per instance on the device in every cycle.
 * The command's height entry is a world height and terrain_height one constant unless include/hsqp_ground.h switches the started loop to the
 * per-instance ground-height estimate from the stance feet.
 * The swing references take that one height for both feet, lift-off and touch-down alike, unless include/hsqp_perceive.h switches the started loop to
 * per-foot lift-off and touch-down heights read from the resident height maps.
 * Out of scope: the motion manager's own BreakFrequencyAlphaFilter in front of the generator, several GPUs.  The centroidal formulation:
 * hsqp_centroidal_command_targets and hsqp_loop_start_centroidal of include/hsqp_cent_loop.h, after which the run / command / state calls below work.
 *
 * ABI: additions only — no public struct and no entry point of hsqp.h, hsqp_feedback.h or hsqp_rollout.h changes, HSQP_ABI_VERSION stays.
 */
#ifndef HSQP_LOOP_H
#define HSQP_LOOP_H

#include "hsqp.h"
#include "hsqp_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSQP_CMD_N 4            /* vx, vy, height, yaw rate */
#define HSQP_CMD_KNOTS 3

/* reference.info defaultJointState [HSQP_NJ] (finite); kept across hsqp_update_weights / hsqp_update_term_weights */
int hsqp_set_default_joint_state(hsqp_handle* h, const double* q);

/* host arrays */
int hsqp_command_targets(hsqp_handle* h, int batch, const double* v_cmd, double* v_filt, double filter_alpha, const double* x0, double t0, double horizon,
                         double* target_times, double* target_states);
/* every array in DEVICE memory of the handle's GPU; v_cmd is not checked for non-finite values */
int hsqp_command_targets_device(hsqp_handle* h, int batch, const double* d_v_cmd, double* d_v_filt, double filter_alpha, const double* d_x0, double t0,
                                double horizon, double* d_target_times, double* d_target_states);

typedef struct hsqp_loop_settings {
  double period;                    /* MPC period [s]: 1 / mpcDesiredFrequency                                    */
  double filter_alpha;              /* command filter, [0, 1)                                                     */
  int32_t n_nodes;                  /* N of every cycle's problem (uniform grid)                                  */
  int32_t iterations;               /* sqpIteration                                                               */
  double dt;                        /* node spacing                                                               */
  int32_t iterate_flags;            /* HSQP_ITER_* as hsqp_iterate_device takes them (not HSQP_ITER_UNTIL_CONVERGED) */
  int32_t arm_swing;                /* hsqp_reference::arm_swing                                                  */
  hsqp_rollout_settings rollout;
  hsqp_swing_config swing;
  double terrain_height;
} hsqp_loop_settings;

/* task.info: period 1 / 60 s (mpcDesiredFrequency 60), filter_alpha 0.8 (the generator's constant), dt 0.035 (sqp dt), one iteration
 * (sqpIteration 1) with HSQP_ITER_TAKE_STEP | HSQP_ITER_LINESEARCH, hsqp_rollout_defaults, swing_trajectory_config, terrain 0, arm swing on.
 * n_nodes: the handle's max_nodes, at most 100 (h may be NULL: 100); the task's horizon is the caller's choice of n_nodes * dt. */
void hsqp_loop_defaults(const hsqp_handle* h, hsqp_loop_settings* s);

/* x0 [B][58], v_cmd [B][4], n_events [B], event_times [B][max_events], mode_sequence [B][max_events + 1]: host arrays, uploaded once.
 * The filter state starts at v_cmd (a converged filter). */
int hsqp_loop_start(hsqp_handle* h, const hsqp_loop_settings* settings, int batch, double t0, const double* x0, const double* v_cmd, int max_events,
                    const int32_t* n_events, const double* event_times, const int32_t* mode_sequence);
/* new commands [B][4]; they take effect with the next cycle */
int hsqp_loop_command(hsqp_handle* h, const double* v_cmd);
int hsqp_loop_command_device(hsqp_handle* h, const double* d_v_cmd);
/* x_log [n_cycles][B][58], u_log [n_cycles][B][35]: optional; cycles_done: optional */
int hsqp_loop_run(hsqp_handle* h, int n_cycles, double* x_log, double* u_log, int* cycles_done);
int hsqp_loop_run_device(hsqp_handle* h, int n_cycles, double* d_x_log, double* d_u_log, int* cycles_done);
/* where the loop stands: t (host), x [B][58], v_filt [B][4]; any may be NULL */
int hsqp_loop_state(hsqp_handle* h, double* t, double* x, double* v_filt);
int hsqp_loop_state_device(hsqp_handle* h, double* t, double* d_x, double* d_v_filt);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_LOOP_H */
