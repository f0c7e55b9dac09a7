/*
 * hsqp_grid.h — the ocs2 event-node time grid of the MI355X SQP library, built per instance on the device, and the resident loop on it.
 *
 * Every receding-horizon path of the library solves on ocs2's multiple-shooting grid, timeDiscretizationWithEvents: nodes every dt from the initial
 * time, split at the mode-switch times, each event a pre-event node and a post-event node joined by an identity jump (a zero-length interval), the
 * last interval shortened to the final time.  hsqp_problem::dt_nodes and hsqp_reference::node_times take such a grid; the ocs2 adaptor builds it on
 * the host in every run().  This header builds it on the device, for a batch, and lets the resident loop (include/hsqp_loop.h) pose every cycle's
 * problem on it: the loop's schedule of a cycle may exist only on the device (include/hsqp_gait.h), so the host cannot.
 *
 * ---- the grid of one instance
 * Inputs t0, n_nodes, dt, dt_min and the instance's (n_events, event_times[]).  tf = t0 + n_nodes * dt, computed once.  The node times are
 * reference.time_discretization_with_events(t0, tf, dt, events, dt_min), operation by operation: they accumulate as times[-1] + dt (no product is
 * formed); an event e with t0 < e < tf reached by the next step becomes a pre-event node and a post-event node with the same time; a node closer
 * than dt_min to the one before it replaces it (not a post-event node: that one always stays); the last step ends at tf.
 *   dt_nodes[k]   = times[k + 1] - times[k]                      (0 on a pre -> post event interval)
 *   node_times[k] = times[k] + 1e-9 on a post-event node         (the adaptor's kEventEps: look-ups by lower_bound see the new mode), times[k] elsewhere
 *
 * ---- one node count for a batch
 * A batch needs ONE number of intervals, the ocs2 grid of every instance has its own, N_b.  The output always has N = n_nodes + event_nodes
 * intervals: an instance with N_b < N is padded with N - N_b zero-length intervals DIRECTLY IN FRONT OF ITS LAST INTERVAL.  The padding nodes
 * duplicate node N_b - 1 and carry its node_time (the epsilon included if it has one), so the padding never makes node_times step back and the
 * last interval stays the real, positive one.  (The ocs2 grid itself can step back by the epsilon where an event lies within 1e-9 s in front of the
 * next node — an event one rounding error before tf; the raw stamps, which carry no epsilon and which HSQP_WARM_SHIFT interpolates on, never
 * decrease, and the loop goes on where a caller's hsqp_upload_reference, which judges by node_times, would refuse the next SHIFT.)
 * n_intervals[b] = N_b tells where the padding sits: intervals [N_b - 1, N - 1) are padding, interval N - 1 is the instance's last real one.
 * A zero-length interval is the identity jump the kernels already have (A = I, B = 0, no cost, no constraints, du = 0), and the padded problem has
 * the solution of the unpadded one on the real nodes ("Event-node grid of the resident loop", has the measurements).  The one downstream
 * effect is in the next HSQP_WARM_SHIFT: a padding node is a pre-event node, so its stamped input is the one of the node before it (upstream
 * toPrimalSolution).  Warm-start states are bit-identical to those of the unpadded grid; warm-start inputs differ only at new nodes whose stamp
 * lies strictly inside the old grid's last-but-one real interval — at most one node, at the far end of the horizon.  That is the price of a common
 * N with the warm start left as it is.
 *
 * ---- status, per instance
 * HSQP_GRID_OK, or HSQP_GRID_OVERFLOW: the ocs2 grid needs more than N intervals.  The builder never writes outside the instance's rows and its
 * loop is bounded whatever the data: device event arrays are not checked by the host, and unsorted or non-finite entries, or a time so large that
 * t + dt == t, end with HSQP_GRID_OVERFLOW after at most N + n_events + 2 steps — as does a grid that would have a negative or non-finite
 * interval or no positive last interval.  On HSQP_GRID_OVERFLOW the instance's rows hold the uniform grid of N intervals of dt and n_intervals
 * is 0.
 *
 * ---- in the resident loop
 * hsqp_loop_event_grid switches the grid of the started loop, effective with the next cycle.  With it on, a cycle builds its grid on the device
 * between the gait update (where a gait is resident) and step 2, from the cycle's resident schedule and the cycle's problem time (the observation
 * model's, include/hsqp_observe.h, when that is in force), and step 2 runs on N = n_nodes + event_nodes intervals with that grid.  Steps 3 and 4
 * are the code of the public calls on an event grid, so the loop equals the caller making hsqp_command_targets, hsqp_gait_update where a gait is
 * resident, hsqp_event_grid, hsqp_upload_reference (with dt_nodes, node_times and the same warm-start mode), hsqp_iterate_device and
 * hsqp_rollout_policy, bit for bit.  The horizon n_nodes * dt, the targets, the gait update, the triage, the metrics and the observation ring are
 * what they are on the uniform grid.  Per cycle the host reads one more 4-byte word, inside a synchronisation the cycle already has; the
 * per-instance status words are read only after a failure; the grid itself is fetched once, at the end of hsqp_loop_run.
 * An overflow is a fault of the schedule, like HSQP_GAIT_OVERFLOW: it stops the cycle (HSQP_ERR_BAD_ARG), also under isolation, and the loop's
 * state is that of the last completed cycle.  hsqp_loop_start and hsqp_loop_start_gait switch the event grid off again.  A loop that never
 * switches it on launches the kernels it always launched.
 *
 * HSQP_ERR_BAD_ARG (message in hsqp_last_error, naming the entry point and the field) for: a NULL handle / settings / array, reserved != 0,
 * event_nodes < 0, dt_min not finite or < 0, dt <= dt_min, n_nodes < 1, n_nodes + event_nodes > max_nodes (the message names both numbers),
 * batch outside [1, max_batch], max_events < 1, a non-finite t0 or dt, host event times that are non-finite or decrease within n_events, host
 * n_events outside [0, max_events], no loop started, a centroidal handle (the loop entry points: the loop is whole-body; hsqp_event_grid works
 * on any handle), an overflow (the message names the first instance; the outputs are still written).
 *
 * Out of scope: the centroidal loop, per-instance n_nodes or horizons, a change of the warm start's stamped-input rule, several GPUs.
 *
 * ABI: additions only — no public struct and no entry point of the other headers changes, HSQP_ABI_VERSION stays.
 */
#ifndef HSQP_GRID_H
#define HSQP_GRID_H

#include "hsqp.h"
#include "hsqp_loop.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status words of a grid */
#define HSQP_GRID_OK 0
#define HSQP_GRID_OVERFLOW 1        /* the ocs2 grid needs more than n_nodes + event_nodes intervals (or the event data admit no grid) */

typedef struct hsqp_grid_settings {
  int32_t event_nodes;              /* intervals on top of n_nodes: two per event inside the horizon, less what dt_min merges */
  int32_t reserved;                 /* 0 */
  double dt_min;                    /* a node closer than this to the one before it replaces it */
} hsqp_grid_settings;

/* event_nodes 32, dt_min 1e-4 (the ocs2 adaptor's) */
void hsqp_grid_defaults(hsqp_grid_settings* s);

/* Stand-alone, any formulation.  n_events [B], event_times [B][max_events] in; n_intervals [B], dt_nodes [B][N], node_times [B][N + 1],
 * status [B] (may be NULL) out, N = n_nodes + event_nodes: host arrays. */
int hsqp_event_grid(hsqp_handle* h, const hsqp_grid_settings* settings, int batch, double t0, int n_nodes, double dt, int max_events, const int32_t* n_events,
                    const double* event_times, int32_t* n_intervals, double* dt_nodes, double* node_times, int32_t* status);
/* every array in DEVICE memory of the handle's GPU; the events are not checked */
int hsqp_event_grid_device(hsqp_handle* h, const hsqp_grid_settings* settings, int batch, double t0, int n_nodes, double dt, int max_events,
                           const int32_t* d_n_events, const double* d_event_times, int32_t* d_n_intervals, double* d_dt_nodes, double* d_node_times,
                           int32_t* d_status);

/* the resident loop: after hsqp_loop_start / hsqp_loop_start_gait; NULL settings = back to the uniform grid; effective with the next cycle */
int hsqp_loop_event_grid(hsqp_handle* h, const hsqp_grid_settings* settings);
/* the grid of the last completed cycle, which must have run on the event grid (HSQP_ERR_BAD_ARG otherwise): n_intervals [B], dt_nodes [B][N],
 * node_times [B][N + 1]; any may be NULL.  A failed cycle does not touch it; hsqp_loop_event_grid with another event_nodes discards it */
int hsqp_loop_grid(hsqp_handle* h, int32_t* n_intervals, double* dt_nodes, double* node_times);
int hsqp_loop_grid_device(hsqp_handle* h, int32_t* d_n_intervals, double* d_dt_nodes, double* d_node_times);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_GRID_H */
