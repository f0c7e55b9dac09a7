/*
 * hsqp_gait.h — per-instance gait schedule and gait ladder of the MI355X SQP library, resident on the device.
 *
 * What the reference does on the host in front of every MPC cycle and include/hsqp_loop.h left to the caller:
 *  (1) SwitchedModelReferenceManager::modifyReferences -> GaitSchedule::getModeSchedule(initTime - H, finalTime + H): the resident schedule
 *      trimmed, re-tiled with the current template and handed to the cycle's problem (GaitSchedule.cpp:85-110);
 *  (2) ProceduralMpcMotionManager::preSolverRun (ProceduralMpcMotionManager.cpp:130-159): the ladder of gaits climbed or descended from the
 *      filtered velocity command and the measured base velocity, and, when the gait command changed,
 *      GaitScheduleUpdater::updateGaitSchedule (GaitScheduleUpdater.cpp:45-69) inserting the new template.
 * Whole-body handles only.  DESIGN.md ("Per-instance gait schedule and ladder") has the restatement line by line and the quirks that are kept.
 *
 * ---- state, per instance
 * the mode schedule (event_times [n], mode_sequence [n + 1], n <= max_events), the current template (held as the rung it came from), the rung
 * currentGaitMode_, currentGaitCommand_ and lastGaitCommand_ (held as rung indices) and lastGaitChangeTime_.
 * hsqp_gait_reset: schedule {[t0 + 0.5], [STANCE, STANCE]} (reference.info initialModeSchedule, offset by t0), template = rung 0's, rung 0,
 * both commands rung 0, lastGaitChangeTime = t0.  At t0 = 0 this is the reference's state.
 *
 * ---- one update at time t with horizon H, the filtered command v [4] = {vx, vy, height, yaw rate} and the measured state x [58]
 * With finalTime = t + H and th = finalTime - t (the reference's timeHorizon, computed this way), in the order of upstream ocs2
 * SolverBase::preRun (reference manager first, then the synchronized modules):
 *   1. getModeSchedule(t - th, finalTime + th); the result goes to the caller's (n_events, event_times, mode_sequence) in the layout
 *      hsqp_reference takes (entries behind n_events: the last event time / STANCE) — this cycle's schedule;
 *   2. if t > lastGaitChangeTime + min_change_interval: transitionToFasterGait -> rung + 1, else transitionToSlowerGait -> rung - 1, both with
 *      the CURRENT rung's thresholds and baseVelocity = x[6 + 23 .. 6 + 23 + 6) (WBAccelMpcRobotModel.h:131-134); the new rung is clamped to
 *      [0, n_rungs - 1] (the reference indexes its table unclamped; with its own table it cannot leave it), the gait command becomes the new
 *      rung's and lastGaitChangeTime = t, also where the clamp kept the rung;
 *   3. if the gait command differs from the last one: getModeSchedule(t, finalTime + th) once more, earliestSwitchingTime =
 *      0.7 finalTime + 0.3 t, nextEventTime = the first event after it (the event before that one if the mode in front of it is LF;
 *      finalTime if there is none), insertModeSequenceTemplate(the rung's template, nextEventTime, 1.5 th).
 * The update is all-or-nothing per call: the kernel reads the live copy of the state and writes a shadow copy and one int32 status per
 * instance; the host reads the status words and swaps the copies only if every instance answered HSQP_GAIT_OK.  A failed call leaves the
 * state as it was (the caller's output arrays are still written).
 *
 * ---- in the resident loop
 * hsqp_loop_start_gait starts a loop (include/hsqp_loop.h) whose mode schedule is this state instead of an uploaded one: hsqp_loop_run then runs
 * the update between its steps 1 and 2, with v = the cycle's filtered command and x = the measured state, and hands the schedule of step 1
 * above to its step 2.  A failed update stops the cycle the way a failed step does (HSQP_ERR_BAD_ARG; the loop's state, the gait state
 * included, is that of the last completed cycle).  hsqp_gait_state reads the loop's gait state; hsqp_gait_reset or hsqp_gait_update on the
 * handle while such a loop is started ends the loop.  A loop started through hsqp_loop_start is untouched by any of this.
 *
 * HSQP_ERR_BAD_ARG (message in hsqp_last_error) for: a NULL handle / settings / array, a centroidal handle, batch outside [1, max_batch],
 * n_rungs outside [1, HSQP_GAIT_MAX_RUNGS], n_phases outside [1, HSQP_GAIT_MAX_PHASES], max_events outside [2, HSQP_GAIT_MAX_EVENTS], a mode
 * outside 0 .. 3, non-finite thresholds, times, t0, t or H, H <= 0, a negative phase_transition_stance_time or min_change_interval, a
 * template whose switching times are not strictly increasing (gait.info's `skip` is one: 0.75 is followed by 0.08), an update without a
 * reset or with another batch, and a schedule that would exceed max_events or whose tiling would not start behind its last event (found on
 * the device, reported through the status words).
 *
 * Out of scope: the motion manager's BreakFrequencyAlphaFilter and command scaling, gait commands from a topic
 * (GaitScheduleUpdater::updateModeSequence), centroidal handles, several GPUs, reading gait.info in C++.  (Event grids: include/hsqp_grid.h
 * builds the cycle's grid from this schedule on the device.)
 *
 * ABI: additions only — no public struct and no entry point of the other headers changes, HSQP_ABI_VERSION stays.
 */
#ifndef HSQP_GAIT_H
#define HSQP_GAIT_H

#include "hsqp.h"
#include "hsqp_loop.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSQP_GAIT_MAX_RUNGS 16      /* gait.info defines sixteen gaits                                    */
#define HSQP_GAIT_MAX_PHASES 6      /* its longest template (skip) has six phases                         */
#define HSQP_GAIT_MAX_EVENTS 256
#define HSQP_GAIT_NAME_LEN 16

/* status words of an update */
#define HSQP_GAIT_OK 0
#define HSQP_GAIT_OVERFLOW 1        /* the schedule would exceed max_events                                */
#define HSQP_GAIT_BAD_TILING 2      /* "The initial time for template-tiling is not greater than the last event time", or an empty schedule */

/* ModeNumber (MotionPhaseDefinition.h) */
#define HSQP_MODE_FLY 0
#define HSQP_MODE_RF 1
#define HSQP_MODE_LF 2
#define HSQP_MODE_STANCE 3

typedef struct hsqp_gait_rung {   /* GaitModeStateConfig + the ModeSequenceTemplate of its gait command */
  double min_lin_vel_cmd, max_lin_vel_cmd, min_ang_vel_cmd, max_ang_vel_cmd, lin_vel_error_thresh, ang_vel_error_thresh;
  int32_t n_phases;
  int32_t reserved;
  double switching_times[HSQP_GAIT_MAX_PHASES + 1];   /* [n_phases + 1], strictly increasing */
  int32_t modes[HSQP_GAIT_MAX_PHASES];                /* [n_phases]                          */
  char name[HSQP_GAIT_NAME_LEN];
} hsqp_gait_rung;

typedef struct hsqp_gait_settings {
  int32_t n_rungs;
  int32_t max_events;                     /* capacity of a schedule; the E of every (event_times [B][E], mode_sequence [B][E + 1]) below */
  double phase_transition_stance_time;    /* task.info phaseTransitionStanceTime (0.0)                                                  */
  double min_change_interval;             /* 0.2 (ProceduralMpcMotionManager.cpp:134; its comment says 0.5)                             */
  hsqp_gait_rung rungs[HSQP_GAIT_MAX_RUNGS];
} hsqp_gait_settings;

/* the seven rungs of ProceduralMpcMotionManager.h:110-118 (thresholds and names), min_change_interval 0.2, phase_transition_stance_time 0,
 * max_events 128.  The templates are the caller's (hsqp_model_desc holds no gaits): n_phases is left 0. */
void hsqp_gait_ladder_defaults(hsqp_gait_settings* s);

int hsqp_gait_reset(hsqp_handle* h, const hsqp_gait_settings* settings, int batch, double t0);

/* v_filt [B][4], x [B][58] in; n_events [B], event_times [B][max_events], mode_sequence [B][max_events + 1] out: host arrays */
int hsqp_gait_update(hsqp_handle* h, int batch, double t, double horizon, const double* v_filt, const double* x, int32_t* n_events,
                     double* event_times, int32_t* mode_sequence);
/* every array in DEVICE memory of the handle's GPU */
int hsqp_gait_update_device(hsqp_handle* h, int batch, double t, double horizon, const double* d_v_filt, const double* d_x, int32_t* d_n_events,
                            double* d_event_times, int32_t* d_mode_sequence);

/* rung [B], last_change_time [B] and the resident schedule; any may be NULL */
int hsqp_gait_state(hsqp_handle* h, int32_t* rung, double* last_change_time, int32_t* n_events, double* event_times, int32_t* mode_sequence);
int hsqp_gait_state_device(hsqp_handle* h, int32_t* d_rung, double* d_last_change_time, int32_t* d_n_events, double* d_event_times,
                           int32_t* d_mode_sequence);

/* hsqp_loop_start with the resident gait state (hsqp_gait_reset(h, gait, batch, t0)) in place of uploaded schedules */
int hsqp_loop_start_gait(hsqp_handle* h, const hsqp_loop_settings* settings, const hsqp_gait_settings* gait, int batch, double t0, const double* x0,
                         const double* v_cmd);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_GAIT_H */
