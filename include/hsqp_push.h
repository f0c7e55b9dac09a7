/*
 * hsqp_push.h — per-instance external pushes on the plant of the batched policy rollout (hsqp_rollout.h) and, through it, of the resident
 * closed loop (hsqp_loop.h): a resident table of up to HSQP_PUSH_MAX pushes per instance, each a constant world-frame force at a point of a
 * link during a time window.  The equivalent of the perturbation forces a user applies to a body in the reference's MuJoCo front end.
 * The MPC never sees a push: the iteration kernels, the node parameters and the warm start are untouched — an unmodelled disturbance on
 * purpose.  With no table set every rollout is bit for bit what it was without this header.
 *
 * Lifetime: the table belongs to the handle, is uploaded once and stays resident.  It survives hsqp_upload*, hsqp_solve, hsqp_loop_start*,
 * hsqp_loop_reset_instances and the weight updates; hsqp_push_clear or a new hsqp_push_set replaces it.  A rollout (hsqp_rollout_policy*) or a
 * loop cycle (hsqp_loop_run*) whose batch differs from the table's returns HSQP_ERR_BAD_ARG with a message: instances are never matched
 * silently.
 *
 * Clock: a push lives on the clock of the node stamps of the resident problem.  For instance b, rollout time s (seconds after the first
 * node, the frame of hsqp_rollout_policy) is clock time stamps[b][0] + s, with stamps[b][0] read on the device from the raw stamps the
 * warm start keeps (hsqp_upload_reference).  A resident problem without stamps (hsqp_upload, hsqp_solve) has its first node at 0.  In the
 * resident loop this clock is the loop's t: a push at t_start = 0.5 hits in the cycle that contains 0.5 s, with no per-cycle bookkeeping,
 * and an instance the triage restarts (hsqp_episode.h) keeps its pushes on that clock.
 *
 * Physics: while a push is active, the force f acts at the world position P of `point` on `body`.
 *   whole-body flow map:  the wrench (f, (P - r_base) x f) is added to the external wrench of the Newton-Euler balance that gives the
 *     base acceleration, where the feet's contact wrenches enter: before the two 3 x 3 base solves, with the same neglect of the
 *     linear / angular coupling.  The joint rows are unchanged: joint accelerations are INPUTS of this formulation, so the joints follow
 *     their commanded accelerations (ideal acceleration sources) and the base takes the push.
 *   centroidal flow map:  f / m goes into the linear and (P - com) x f / m into the angular rows of the normalised momentum rate; the joint
 *     rows (commanded joint velocities) are unchanged.
 * Overlapping pushes of one instance add (in the order of the table).  What this model of a push leaves out: joint compliance (see above),
 * and contact slip — a stance foot stays where the policy's wrenches hold it, no friction limit is enforced on the plant.
 * The compliant plant is hsqp_plant.h: with HSQP_PLANT_TORQUE set a push acts through the whole tree (the base rows and every joint between the
 * base and the pushed body) under the joint PD law; edges, activity and break points are the ones above.
 *
 * Piecewise-constant forcing, exact restarts: the edges of every push of an instance are break points of the integration, like the event
 * stamps of the grid.  Edge arithmetic: in rollout time an edge is
 *     edge_start = t_start - stamps[b][0],      edge_end = (t_start + duration) - stamps[b][0],
 * each formed once per call.  A push with edge_end <= edge_start (duration 0, or one lost to rounding) is inert: never active, no break
 * point.  At an edge strictly inside a sample interval the integrator restarts with the step min(initial_step, remaining) and a fresh flow
 * evaluation, as at an event.  Whether a push is active is decided once per segment (the stretch between two consecutive break points or
 * sample times), from the segment's start time ts,
 *     active  iff  edge_start <= ts < edge_end,
 * and held for every stage evaluation of the segment: a stage evaluated at the segment's end time does not see the next regime.  So the
 * chained-call property of hsqp_rollout.h keeps holding with pushes set: n_samples = n equals n chained calls of duration / n bit for bit
 * when the times are exact binary fractions.
 *
 * Errors: HSQP_ERR_BAD_ARG, message in hsqp_last_error, for a NULL handle or array, batch outside [1, max_batch], max_pushes outside
 * [1, HSQP_PUSH_MAX], an n_pushes[b] outside [0, max_pushes], a body outside the tree [0, HSQP_NB), reserved != 0, a negative duration, a
 * non-finite duration, t_start, point or force (the host entry point checks every used entry; hsqp_push_set_device checks the scalars only:
 * on the device an entry with a body outside the tree is inert and n_pushes[b] is clamped to [0, max_pushes]), and hsqp_push_get with no
 * table set.
 *
 * ABI: additions only — no public struct and no entry point of the other headers changes, so HSQP_ABI_VERSION (hsqp.h) needs no bump.
 */
#ifndef HSQP_PUSH_H
#define HSQP_PUSH_H

#include "hsqp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSQP_PUSH_MAX 8                 /* pushes per instance */

typedef struct hsqp_push {
  int32_t body;                         /* link index of the model's kinematic tree (0 = base link) */
  int32_t reserved;                     /* 0 */
  double t_start, duration;             /* [s], on the clock above; duration >= 0, 0 = never active */
  double point[3];                      /* point of application, in the body's frame */
  double force[3];                      /* [N], world frame, constant while the push is active */
} hsqp_push;

/* n_pushes [batch], pushes [batch][max_pushes] (host memory; entries from n_pushes[b] on are ignored) */
int hsqp_push_set(hsqp_handle* h, int batch, int max_pushes, const int32_t* n_pushes, const hsqp_push* pushes);
/* the same, both arrays in DEVICE memory of the handle's GPU; their values are not checked */
int hsqp_push_set_device(hsqp_handle* h, int batch, int max_pushes, const int32_t* d_n_pushes, const hsqp_push* d_pushes);
/* no table: every rollout is the unpushed one */
int hsqp_push_clear(hsqp_handle* h);
/* the resident table: batch, max_pushes, n_pushes [batch], pushes [batch][max_pushes] (host memory); any output may be NULL */
int hsqp_push_get(hsqp_handle* h, int* batch, int* max_pushes, int32_t* n_pushes, hsqp_push* pushes);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_PUSH_H */
