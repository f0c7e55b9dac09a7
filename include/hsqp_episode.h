/*
 * hsqp_episode.h — per-instance failure isolation and episode reset of the resident closed loop (include/hsqp_loop.h, include/hsqp_gait.h).
 *
 * The loop of hsqp_loop.h is fail-stop for the whole batch: one instance with a non-finite state, one that hits the rollout's step cap, ends
 * hsqp_loop_run for every instance.  With isolation on, a failed instance is recorded and parked or restarted on the device, the others go on
 * bit for bit as if it were not there, and the host may start a new episode on chosen instances without touching the rest.  Opt-in: isolation
 * is OFF after every hsqp_loop_start / hsqp_loop_start_gait, and a loop that never calls hsqp_loop_isolate behaves exactly as hsqp_loop.h says.
 *
 * ---- a cycle under isolation
 * The five steps of hsqp_loop.h, with three differences, and one more step behind the rollout:
 *   1. the targets are built from the command in USE: the instance's command, or for a parked instance the stance command
 *      {0, 0, x_reset[2], 0};
 *   2. the warm start is chosen per instance: HSQP_WARM_COLD for an instance that starts an episode in this cycle, HSQP_WARM_SHIFT for the
 *      others (COLD for all in the first cycle after hsqp_loop_start).  A COLD instance reads nothing of its previous solution;
 *   3., 4. the iteration and the rollout report per instance: an instance's status word is not turned into the batch's return code, and the
 *      policy, feedback and rollout records of the other instances are valid after an iteration in which one failed;
 *   6. the triage (k_loop_triage, one wave per instance) reads what lies on the device — the iteration's status word and performance index,
 *      the rollout's status word, the rolled-out state row — and decides, in this order:
 *        HSQP_EP_FAILED_NUMERIC  the status word of the iteration is not 0, or its performance index (merit, cost, dynamics_sse,
 *                                equality_sse after the step) is not finite;
 *        HSQP_EP_FAILED_ROLLOUT  the rollout answered HSQP_ROLLOUT_NONFINITE or HSQP_ROLLOUT_MAX_STEPS, or an entry of the rolled-out state
 *                                is not finite;
 *        HSQP_EP_FAILED_BOUNDS   state entry 2 (base height) outside [min_base_height, max_base_height], or |entry 4| or |entry 5|
 *                                (pitch, roll) above max_tilt.
 * For an instance that failed in cycle c (counted from hsqp_loop_start): cause = the verdict, fail_cycle = c, n_failures + 1; row c of x_log
 * and u_log is NaN; its measured state becomes x_reset[b]; its command filter is re-seeded with the command it will use; with a resident gait
 * its gait state becomes what hsqp_loop_start_gait would give that one instance at the loop time of the next cycle ({[t + 0.5], [STANCE,
 * STANCE]}, rung 0, lastGaitChangeTime = t: k_gait_reset_instances); it takes HSQP_WARM_COLD in the next cycle.
 *   HSQP_EPISODE_RESET: the instance is HSQP_EP_ALIVE again from the next cycle, keeps its command, n_episodes + 1.
 *   HSQP_EPISODE_PARK:  the instance stays failed (state = its cause).  It runs on from x_reset under the stance command, so every kernel keeps
 *                       seeing a well-posed problem; its log rows stay NaN; if it fails again it is reset the same way (cause, fail_cycle and
 *                       n_failures follow the last failure).  It comes back only through hsqp_loop_reset_instances.
 * cause and fail_cycle are a record of the LAST failure: they stay when the instance is alive again.  Loop time t is global: it is not reset.
 * A failed instance's gait update of the failing cycle is overwritten by the reset; a gait update that fails (HSQP_GAIT_OVERFLOW /
 * _BAD_TILING) and a swing phase without lift-off are faults of the schedule, not of an episode: they stop the loop as before.
 *
 * hsqp_loop_run / hsqp_loop_run_device under isolation return HSQP_OK whatever single instances did; only what is not per instance still
 * stops them (HIP errors, bad arguments, a failed allocation, the two schedule faults above).  Inside hsqp_loop_run nothing whose size grows
 * with B crosses to the host beyond the int32 status words the underlying calls read already; the triage reads nothing back.
 *
 * ---- which handles
 * Isolation needs that one instance's NaN cannot change another instance's bits.  The serial backward sweep (the default from three
 * whole-body instances on, or HSQP_FLAG_SERIAL_RICCATI) is free of such coupling ("Per-instance failure isolation", lists every
 * batch-wide decision of an iteration).  The KKT-GATED sweeps are coupled: the gate of the parallel-in-time and of the two-level sweep is ONE
 * verdict per batch, so one instance's NaN sends every instance through the serial recursion instead.  hsqp_loop_isolate therefore returns
 * HSQP_ERR_BAD_ARG on a loop whose handle would take a gated sweep: HSQP_FLAG_PARALLEL_RICCATI, HSQP_FLAG_SEGMENTED_RICCATI, or the automatic
 * choice with batch <= HSQP_SCAN_AUTO_BATCH and n_nodes >= HSQP_SCAN_AUTO_MIN_NODES.  Create such a handle with HSQP_FLAG_SERIAL_RICCATI.
 *
 * HSQP_ERR_BAD_ARG (message in hsqp_last_error) also for: a NULL handle, no loop started (every hsqp_upload* / hsqp_solve ends a loop), a NULL
 * settings pointer, an unknown on_failure, NaN bounds, min_base_height > max_base_height, max_tilt < 0, a non-finite x_reset / x0 / v_cmd
 * (host arrays), n < 1, NULL ids, ids outside [0, B) or repeated, hsqp_loop_reset_instances / hsqp_loop_episodes without hsqp_loop_isolate.
 *
 * On a loop started by hsqp_loop_start_centroidal (include/hsqp_cent_loop.h) the box is read at the centroidal pose (x[8], x[10], x[11]), a parked
 * instance's stance command takes x_reset[8], and x_reset / x0 rows must have zero padding.
 * Out of scope: fall detection beyond the caller's box, per-instance loop time, several GPUs.  (On the event-node
 * grid of include/hsqp_grid.h an instance whose schedule overflows the grid stops the cycle for all: it is a fault of the schedule, not of an episode.)
 * The base-height box is absolute unless include/hsqp_ground.h (box_above_ground) puts it on the height above the estimated ground.
 *
 * ABI: additions only — no public struct and no entry point of the other headers changes, HSQP_ABI_VERSION stays.
 */
#ifndef HSQP_EPISODE_H
#define HSQP_EPISODE_H

#include "hsqp.h"
#include "hsqp_gait.h"
#include "hsqp_loop.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSQP_EPISODE_PARK 0    /* a failed instance is parked until the host resets it */
#define HSQP_EPISODE_RESET 1   /* a failed instance starts a new episode by itself     */

#define HSQP_EP_ALIVE 0
#define HSQP_EP_FAILED_NUMERIC 1   /* the iteration left a status word / a non-finite performance index for this instance    */
#define HSQP_EP_FAILED_ROLLOUT 2   /* HSQP_ROLLOUT_NONFINITE or HSQP_ROLLOUT_MAX_STEPS, or a non-finite rolled-out state          */
#define HSQP_EP_FAILED_BOUNDS 3    /* rolled-out base height / tilt outside the caller's box                                      */

typedef struct hsqp_episode_settings {
  int32_t on_failure;                       /* HSQP_EPISODE_PARK / _RESET                              */
  int32_t reserved;
  double min_base_height, max_base_height;  /* on state entry 2; defaults -inf / +inf (off)            */
  double max_tilt;                          /* on |pitch|, |roll| (state entries 4, 5); default +inf   */
} hsqp_episode_settings;

/* HSQP_EPISODE_PARK, bounds off */
void hsqp_episode_defaults(hsqp_episode_settings* s);

/* after hsqp_loop_start / hsqp_loop_start_gait: isolation on, every instance HSQP_EP_ALIVE in its first episode, the counters zeroed.
 * x_reset [B][58] host, NULL = the measured state the loop holds now (the x0 it was started with, if no cycle has run). */
int hsqp_loop_isolate(hsqp_handle* h, const hsqp_episode_settings* settings, const double* x_reset);
/* a new episode for n chosen instances, failed or not, effective with the next cycle: ids [n]; x0 [n][58] or NULL (= x_reset of the instance);
 * v_cmd [n][4] or NULL (= keep).  The instance is HSQP_EP_ALIVE, n_episodes + 1.  Host arrays. */
int hsqp_loop_reset_instances(hsqp_handle* h, int n, const int32_t* ids, const double* x0, const double* v_cmd);
/* state [B] (HSQP_EP_*), cause [B] (HSQP_EP_* of the last failure), fail_cycle [B] (cycle index since hsqp_loop_start, -1: none),
 * n_failures [B], n_episodes [B] (1 in the first episode); any may be NULL */
int hsqp_loop_episodes(hsqp_handle* h, int32_t* state, int32_t* cause, int32_t* fail_cycle, int32_t* n_failures, int32_t* n_episodes);
int hsqp_loop_episodes_device(hsqp_handle* h, int32_t* d_state, int32_t* d_cause, int32_t* d_fail_cycle, int32_t* d_n_failures, int32_t* d_n_episodes);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_EPISODE_H */
