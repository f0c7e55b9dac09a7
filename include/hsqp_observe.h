/*
 * hsqp_observe.h — the observation model of the resident loop (hsqp_loop.h): what the MPC measures of the plant.  A per-instance constant bias,
 * per-instance white Gaussian noise from a counter-based generator on the device, a sensor delay the controller does not know about and a
 * compute delay it does know about.  Resident settings of the handle, of the MEASUREMENT ONLY: the plant, the rollout kernels and the
 * iteration kernels are untouched.  Without it the loop uses one array for the plant's true state and for the state the MPC measures (the x0
 * of the velocity-command targets, the x of the gait update, x_init of hsqp_upload_reference), and the policy is in force the instant the
 * measurement is taken.  With no settings and no table (never set, or after hsqp_observe_clear) hsqp_loop_run* takes exactly that path: no
 * extra launch, no extra buffer.  With settings in force but neutral (both delays 0, no table or an all-zero table) every output of the loop
 * is bit for bit what it was without this header.
 *
 * The model.  NOISE AND BIAS: for instance b, draw index n and state entry i (the layout of x, 58 entries), block k = i / 4 and lane i % 4:
 *   (r0, r1, r2, r3) = Philox4x32-10(counter = {k, b, n, 0}, key = {seed & 0xffffffff, seed >> 32})
 *   u_j = (r_j + 0.5) 2^-32;  lanes 0, 1: z = sqrt(-2 ln u_0) {cos, sin}(2 pi u_1);  lanes 2, 3 the same from (u_2, u_3); block 14: lanes 0, 1 only
 *   y_i = x_i + (bias_i + sigma_i z_i), evaluated unfused in double precision.
 * An entry with bias_i == 0 and sigma_i == 0 is COPIED with no arithmetic (a NaN keeps its payload, a zero its sign); a block whose sigmas
 * are all 0 draws nothing.  The stream depends on (seed, b, n, i) and on nothing else: not on the batch size, the launch shape or the other
 * instances.  In the loop n is the index of the cycle in which the observation is USED, counted from hsqp_loop_start* (the noise is white, so
 * drawing at use time equals drawing at sampling time).
 *
 * DELAY: a = sensor_delay + compute_delay, k = compute_delay, P the loop's period, t the loop's (the plant's) time.  A ring of a + 1 slots
 * [B][58] holds the plant's true states at the starts of the last cycles.  A cycle with the model in force (steps of hsqp_loop.h):
 *   0. (new, one launch) the plant's state goes into slot cycle mod (a + 1); y is formed from slot (cycle - a) mod (a + 1) — with a == 0 from
 *      the plant's state itself.  An instance that starts an episode in this cycle first has EVERY slot set to its state: every instance in
 *      the first cycle after hsqp_loop_start*, and under isolation (hsqp_episode.h) an instance whose warm start of this cycle is
 *      HSQP_WARM_COLD.  The step is idempotent: a cycle that fails later and is run again writes the same bytes.
 *   1 - 3. the targets, the gait update if resident, x_init with the warm start and the iteration take y where they took the plant's state,
 *      and the PROBLEM TIME t_p = t - k P where they took t.  The gait's clock is t_p everywhere, the per-instance gait reset behind the triage
 *      and behind hsqp_loop_reset_instances included (t_p of the next cycle), and hsqp_loop_start_gait resets the gait state at t0 - k P.
 *   4. the rollout starts from the plant's TRUE state at s0 = k P in the policy's own frame, for every instance, over one period: the plant
 *      moves over [t, t + P] under the policy solved from the observation of t - a P.
 *   5, 6. unchanged: logs, hsqp_loop_state and the triage's bounds see the TRUE rolled-out state and the time t.  A fall is a fall of the plant.
 * Successive problems are still one period apart, so HSQP_WARM_SHIFT is unchanged.
 *
 * ASSUMPTIONS:
 *   O1. The plant rested at its start state for the a periods before an episode: the ring of an instance that starts one is filled with it.
 *   O2. Both delays are whole MPC periods and the same for every instance.
 *   O3. Pushes, actuator and contact run on the clock of the node stamps; absolute time is unchanged there because t_p + s0 = t.  The actuator's
 *       tick grid (hsqp_actuator.h) lives on the s clock: with k > 0 its phase against absolute time shifts by k P mod command_period.
 *   O4. With compute_delay > 0 the policy is solved from an older state and plans its own inputs over the k periods the plant actually spent under
 *       the previous policies (no input commitment, as in ocs2's MRT).  The feed-forward controller of hsqp_rollout.h then applies inputs planned
 *       for a state the plant is not in; the feedback controller corrects for the difference (DESIGN.md records what either does to a walk).
 *   Out of scope: coloured noise or random-walk drift; quantisation; an estimator low-pass; delays that are not whole periods; per-instance
 *   delays; noise on the rollout's own feedback term inside a period (the rollout's feedback controller reads the true state); centroidal
 *   handles; several GPUs.
 *
 * Lifetime: settings and table belong to the handle and survive hsqp_upload*, hsqp_solve, hsqp_loop_start*, hsqp_loop_reset_instances and the
 * plant settings (hsqp_plant_*, hsqp_contact_*, hsqp_actuator_*, hsqp_inertia_*, hsqp_push_*).  The ring belongs to the loop and is seeded at
 * every start.  The table and the seed may change while a loop is started: the change takes effect with the next cycle.  hsqp_observe_set with
 * delays that differ from those in force while a loop is started is refused (restart the loop: the ring and the problem clock would lose their
 * meaning; set the delays before hsqp_loop_start*, and any hsqp_upload* or hsqp_solve call ends a started loop); hsqp_observe_clear is always taken, and the next cycle is posed at the plant's time from the plant's state.  Instances past the
 * table's batch are neutral.  Whole-body handles only.
 *
 * hsqp_observe_eval applies bias and noise of instance b's entry to x[b] at a given draw index — no delay, no loop and no resident solution
 * needed; x and y may be the same array.  hsqp_observe_last gives the observation the last completed cycle used, and its problem time.
 *
 * Errors: HSQP_ERR_BAD_ARG, message in hsqp_last_error naming the entry point, the instance and the field ("instance 2: sigma[7]"), for a NULL
 * handle, a centroidal handle, a negative delay, sensor_delay + compute_delay > HSQP_OBS_MAX_DELAY, batch outside [1, max_batch]
 * (hsqp_observe_set_instances with NULL also takes 0), a non-finite bias, a negative or non-finite sigma (host tables only: device tables are
 * not read back), NULL x / y, hsqp_observe_last without a completed cycle of a loop that has the model in force; at hsqp_loop_run*:
 * (compute_delay + 1) period > n_nodes dt (the policy would be evaluated past its horizon) and a table whose batch differs from the loop's.
 * A refused call leaves what was in force; a HIP error while a table is copied (HSQP_ERR_HIP, HSQP_ERR_OOM) leaves NO table.
 *
 * ABI: additions only — no public struct and no entry point of the other headers changes, so HSQP_ABI_VERSION (hsqp.h) needs no bump.
 */
#ifndef HSQP_OBSERVE_H
#define HSQP_OBSERVE_H

#include "hsqp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSQP_OBS_MAX_DELAY 8            /* sensor_delay + compute_delay, in MPC periods */

typedef struct hsqp_observe_settings {
  int32_t  sensor_delay;    /* >= 0, whole MPC periods: age of the measurement the controller does NOT know about        */
  int32_t  compute_delay;   /* >= 0, whole MPC periods between an observation and the moment its policy takes over (known) */
  uint64_t seed;            /* key of the noise stream                                                                   */
} hsqp_observe_settings;

typedef struct hsqp_observe_instance {
  double bias[58];          /* finite; added to the state row, same layout as x                */
  double sigma[58];         /* finite, >= 0; standard deviation of the white noise per entry   */
} hsqp_observe_instance;

void hsqp_observe_defaults(hsqp_observe_settings* s);            /* 0, 0, 0 */
void hsqp_observe_instance_defaults(hsqp_observe_instance* v);   /* all zero: neutral */
int  hsqp_observe_set(hsqp_handle* h, const hsqp_observe_settings* s);
/* table [batch]; NULL (batch 0 .. max_batch): no table */
int  hsqp_observe_set_instances(hsqp_handle* h, int batch, const hsqp_observe_instance* table);
int  hsqp_observe_set_instances_device(hsqp_handle* h, int batch, const hsqp_observe_instance* d_table);   /* not checked */
int  hsqp_observe_clear(hsqp_handle* h);                          /* settings and table gone */
/* the settings and the entries in force; either may be NULL; instances past the table: neutral */
int  hsqp_observe_get(hsqp_handle* h, hsqp_observe_settings* s, int batch, hsqp_observe_instance* table);
/* y[b] = what instance b's entry makes of x[b] at draw index `draw`: bias and noise only, no delay; x, y [batch][58] */
int  hsqp_observe_eval(hsqp_handle* h, int batch, uint32_t draw, const double* x, double* y);
int  hsqp_observe_eval_device(hsqp_handle* h, int batch, uint32_t draw, const double* d_x, double* d_y);
/* the observation the last completed cycle of the loop used: y [B][58], its problem time t_p; either may be NULL */
int  hsqp_observe_last(hsqp_handle* h, double* y, double* t_p);
int  hsqp_observe_last_device(hsqp_handle* h, double* d_y, double* t_p);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_OBSERVE_H */
