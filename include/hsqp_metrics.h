/*
 * hsqp_metrics.h — per-instance episode metrics of the resident closed loop (include/hsqp_loop.h, include/hsqp_episode.h), accumulated on the device.
 *
 * The loop tells the host where every instance IS (hsqp_loop_state), one log row per cycle and instance if asked, and under isolation the episode
 * words.  How an instance FARED — how well it tracked its command, how far it walked, what its joints and its feet did, how the solver stood — is
 * a fixed-size record per instance that lives on the device beside the episode arrays.  One kernel (k_loop_metrics, one workgroup per instance)
 * adds the sample of a cycle behind the cycle's rollout; the record is cut at episode boundaries and read back once, after the run.  Opt-in:
 * metrics are OFF after every hsqp_loop_start / hsqp_loop_start_gait.  With metrics off no kernel is launched and no buffer is allocated; with
 * metrics on nothing the loop computes changes by a bit, nothing is read back per cycle, and nothing is added to what crosses between host and
 * device in a cycle (the kernel's launch apart).
 *
 * ---- the two records of an instance
 * HSQP_METRICS_CURRENT is the open record of the instance's running episode, HSQP_METRICS_PREVIOUS the record of the last episode that was closed
 * (an empty record: none yet).  An EMPTY record: every count 0, first_cycle -1, end_cause HSQP_METRICS_END_OPEN, every double 0 except
 * height_min = +inf and height_max = -inf.
 *
 * ---- the sample of one cycle (instance b, cycle c counted from hsqp_loop_start)
 * x_before: the plant state the cycle's rollout started from; x: the rolled-out row; cmd: the command step 1 of that cycle read (v_cmd, under
 * isolation the command in use); T: the loop's period.
 *   motion   psi = x[3]; want = (cos psi cmd[0] - sin psi cmd[1], sin psi cmd[0] + cos psi cmd[1]); e2 = (x[29] - want[0])^2 + (x[30] - want[1])^2:
 *            vel_err_sq += e2, vel_err_max = max(., sqrt(e2)); yaw_rate_err_sq += (x[32] - cmd[3])^2; height_err_sq += (x[2] - cmd[2])^2;
 *            height_min / height_max follow x[2], tilt_max follows max(|x[4]|, |x[5]|); path_length += |x.xy - x_before.xy|; end_xy = x.xy;
 *            start_xy = x_before.xy on the record's first sample, whose cycle index is first_cycle.
 *   torque   only while the actuator model of hsqp_actuator.h is active on the torque plant.  Reads the record of hsqp_actuator_last that the
 *            cycle's rollout has just written (tau_cmd, tau_act) and the resident effort limits; v_j = x[35 + j].  torque_samples + 1;
 *            saturated_joint_samples + the number of joints with |tau_cmd_j| > effort_limit_j, saturated_samples + 1 if there is one;
 *            tau_sq += sum_j tau_act_j^2; tau_ratio_max = max(., max_j |tau_cmd_j| / effort_limit_j) (0 for a limit of +inf);
 *            work_pos += T sum_j max(0, tau_act_j v_j); work_abs += T sum_j |tau_act_j v_j|.
 *            An enabled NEUTRAL actuator setting (command_period 0, every limit +inf, damping 0, friction 0) leaves every bit of the rollout as
 *            it was (hsqp_actuator.h), so a caller who wants these fields without an actuator model sets that one.
 *   ground   only while the ground of hsqp_contact.h is in force on the torque plant.  The contact model is formed at x by the source of
 *            hsqp_contact_eval (on the height map of hsqp_terrain.h while a terrain is resident) with the handle's setting and tables for
 *            instance b.  A corner is loaded when its force vector is not all zero, a foot when one of its four corners is.  ground_samples + 1;
 *            flight_samples + 1 if no corner is loaded; touchdowns[f] + 1 if foot f is loaded and was not in the record's previous ground sample
 *            (a record's first ground sample counts none); load = the sum over the eight corners of the world-z force: load_sum += load,
 *            load_max = max(., load); penetration_max = max(., d_i) over the corners.
 *   solver   cost_sum += perf.cost; dynamics_sse_max / equality_sse_max take the maxima of the iteration's hsqp_perf after the step;
 *            rollout_steps / rollout_rejected add the accepted / rejected integrator steps of the cycle's rollout.
 *   cycles + 1, duration = cycles * T (formed by that product).
 * Arithmetic is plain double, never contracted; every per-joint and per-corner sum is taken in index order.
 *
 * ASSUMPTION M1: every quantity is sampled ONCE per MPC period, at the period's end.  work_pos / work_abs are a rectangle rule at that rate, not an
 * integral over the actuator's ticks; maxima are maxima over the samples, not over the trajectory between them.  The integration itself is untouched.
 *
 * ---- episode boundaries
 * Without isolation every instance accumulates every completed cycle.  Under isolation the verdict is the triage's own (the same function on the
 * same words, hsqp_episode.h step 6):
 *   an instance that is HSQP_EP_ALIVE before the cycle and passes the verdict accumulates the sample;
 *   an instance that fails in cycle c does not accumulate it: its CURRENT record is closed with end_cause = the verdict and becomes PREVIOUS,
 *     CURRENT becomes empty.  Under HSQP_EPISODE_RESET its next sample opens at first_cycle = c + 1 with start_xy from x_reset;
 *   a parked instance accumulates nothing;
 *   hsqp_loop_reset_instances and hsqp_loop_metrics_restart close with HSQP_METRICS_END_HOST;
 *   closing an empty record does nothing, so a parked instance's PREVIOUS survives the host's reset.
 * cycles + first_cycle of a record closed by a failure equals the instance's fail_cycle.
 *
 * HSQP_ERR_BAD_ARG (message in hsqp_last_error, naming the entry point) for: a NULL handle or out, no loop started, a centroidal handle, an
 * unknown `which`, n < 1, ids outside [0, B) or repeated, hsqp_loop_metrics_restart / the getters before hsqp_loop_metrics_enable.
 *
 * Out of scope: quantities integrated inside the rollout, a batch reduction on the device, centroidal handles, several GPUs, slip distance.
 *
 * ABI: additions only — no public struct and no entry point of the other headers changes, HSQP_ABI_VERSION stays.
 */
#ifndef HSQP_METRICS_H
#define HSQP_METRICS_H

#include "hsqp.h"
#include "hsqp_episode.h"
#include "hsqp_loop.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSQP_METRICS_CURRENT 0    /* the open record of the instance's running episode              */
#define HSQP_METRICS_PREVIOUS 1   /* the record of the last episode that was closed (empty: none)   */
#define HSQP_METRICS_END_OPEN -1  /* end_cause of a record that is still open / of an empty record  */
#define HSQP_METRICS_END_HOST 0   /* closed by hsqp_loop_reset_instances / hsqp_loop_metrics_restart */
                                  /* else the HSQP_EP_FAILED_* verdict that closed it               */

typedef struct hsqp_metrics {     /* 8-byte fields only */
  int64_t cycles;                 /* samples in the record                                            */
  int64_t first_cycle;            /* loop cycle index (from hsqp_loop_start) of its first sample, -1  */
  int64_t end_cause;
  int64_t torque_samples;         /* samples taken while the actuator model was in force              */
  int64_t ground_samples;         /* samples taken while the ground of hsqp_contact.h was in force    */
  int64_t flight_samples;         /* ground samples with no loaded sole corner                        */
  int64_t touchdowns[2];          /* per foot: ground samples in which it is loaded and was not in the record's previous ground sample */
  int64_t saturated_samples;      /* torque samples with |tau_cmd_j| > effort_limit_j at some joint   */
  int64_t saturated_joint_samples;/* (sample, joint) pairs of the same                                */
  int64_t rollout_steps, rollout_rejected;   /* accepted / rejected integrator steps, summed          */
  double duration;                /* cycles * period, formed by that product                          */
  double start_xy[2], end_xy[2];  /* base x, y of the state the first sample was rolled out FROM / of the last sample */
  double path_length;             /* sum of |xy(after) - xy(before)| over the samples                 */
  double vel_err_sq, vel_err_max; /* planar base velocity against the rotated command (above)         */
  double yaw_rate_err_sq, height_err_sq;
  double height_min, height_max, tilt_max;   /* x[2]; max(|x[4]|, |x[5]|)                             */
  double tau_sq, tau_ratio_max;   /* sum_j tau_act_j^2 summed; max_j |tau_cmd_j| / effort_limit_j (0 for +inf) */
  double work_pos, work_abs;      /* period * sum_j max(0, tau_act_j v_j); period * sum_j |tau_act_j v_j|     */
  double load_sum, load_max;      /* sum over the eight corners of the world-z force: summed over samples; largest sample */
  double penetration_max;         /* largest corner penetration d                                     */
  double cost_sum, dynamics_sse_max, equality_sse_max;   /* the iteration's hsqp_perf after the step   */
} hsqp_metrics;

/* after hsqp_loop_start*: metrics on, every record empty */
int hsqp_loop_metrics_enable(hsqp_handle* h);
/* accumulation stops; the records stay readable until the next start */
int hsqp_loop_metrics_disable(hsqp_handle* h);
/* close (HSQP_METRICS_END_HOST) and reopen the records of n chosen instances without touching their episodes; ids NULL: all (n is not read) */
int hsqp_loop_metrics_restart(hsqp_handle* h, int n, const int32_t* ids);
/* which: HSQP_METRICS_CURRENT / _PREVIOUS; out [B] host */
int hsqp_loop_metrics(hsqp_handle* h, int which, hsqp_metrics* out);
int hsqp_loop_metrics_device(hsqp_handle* h, int which, hsqp_metrics* d_out);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_METRICS_H */
