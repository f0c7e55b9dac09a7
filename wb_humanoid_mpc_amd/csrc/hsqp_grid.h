// The ocs2 multiple-shooting time grid of ONE instance with a node count common to the batch (include/hsqp_grid.h): upstream ocs2_oc
// timeDiscretizationWithEvents as reference.time_discretization_with_events restates it, operation by operation, then padded to N intervals.
//
// Shape: the recurrence is serial (times[-1] + dt, one comparison with the next event, one with the final time) and a few flops per node, so ONE
// lane builds the grid of one instance straight into the instance's rows of the outputs: dt_nodes [N], node_times [N + 1].  Of the grid under
// construction only three scalars live in registers — the last node's time, the time of the node before it, whether the last node is a post-event
// node — because the reference touches nothing else: it appends a node or it replaces the last one.  An instance reads its own events and writes its
// own rows; nothing is shared, so one instance's data cannot change another's bits.
//
// Bounds: a node is stored only under `n <= N`, an interval only under `n - 1 < N`; an append past that is HSQP_GRID_OVERFLOW.  Every pass of the
// loop appends a node, or replaces the last node by the final time and ends, or (a time so large that t + dt == t, a non-finite event that slipped
// through a comparison) does neither: the passes are counted and the loop gives up with HSQP_GRID_OVERFLOW after N + n_events + 2 of them, whatever
// the data.  The events are the caller's device array: unsorted and non-finite entries are filtered the way the reference filters them
// (t0 < e < tf, in array order); a grid whose intervals then come out negative or not finite, or that has no positive last interval, is answered
// with HSQP_GRID_OVERFLOW as well.  On HSQP_GRID_OVERFLOW the rows hold the uniform grid of N intervals of dt from t0 — finite numbers a later kernel
// can read — and n_intervals is 0.
//
// Padding ("Event-node grid of the resident loop"): an instance whose grid has N_b < N intervals gets N - N_b zero-length intervals
// directly in front of its last interval.  The padding nodes duplicate node N_b - 1, its sampling time included (the epsilon of a post-event node
// too), so the padding adds no step back to node_times and the last interval stays the real, positive one.  (The ocs2 grid itself can step back
// by the epsilon: an event one rounding error in front of the final time — tf = t0 + n_nodes dt rounds — leaves a last interval of 1e-15 s whose
// end node is sampled at tf, below the post-event node's t_event + 1e-9.  The raw stamps, which carry no epsilon, never decrease.)
// A zero-length interval is the identity jump the kernels already have (A = I, B = 0, no cost, no constraints, du = 0).  Its one downstream
// effect: in the next cycle's HSQP_WARM_SHIFT a padding node is a pre-event node, whose stamped input is the one of the node before it
// (reference.stamped_inputs); warm-start states are bit-identical to the unpadded grid's, inputs differ only at new nodes whose stamp lies
// strictly inside the old grid's last-but-one real interval.
//
// Arithmetic: additions, subtractions, one product (the horizon n_nodes * dt), comparisons — unfused (`#pragma clang fp contract(off)`), so the
// device, the host build of this source (tests/grid/grid_emu.cpp, -ffp-contract=off) and the Python mirror (reference.padded_event_grid) agree bit
// for bit.
#pragma once
#include "hsqp_common.h"
#include "../../include/hsqp_grid.h"

namespace hsqp {

constexpr double GRID_EVENT_EPS = 1e-9;   // reference.EVENT_EPS / the adaptor's kEventEps: a post-event node is sampled at t_event + 1e-9

// One instance.  ev [n_events] (n_events is clamped to [0, max_events]); dts [N], nts [N + 1]: the instance's rows; N = n_nodes + event_nodes.
// Returns the status word; *n_intervals = N_b (0 on HSQP_GRID_OVERFLOW).
HSQP_HD int grid_build_instance(double t0, int n_nodes, double dt, double dt_min, int event_nodes, int max_events, int n_events, const double* ev, int* n_intervals,
                                double* dts, double* nts) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int N = n_nodes + event_nodes;
  const int ne = n_events < 0 ? 0 : n_events > max_events ? max_events : n_events;
  const double horizon = n_nodes * dt;
  const double tf = t0 + horizon;
  int status = HSQP_GRID_OK;
  int n = 1, ie = 0;                       // nodes stored so far, the next entry of ev
  double last = t0, prev = t0;             // times[-1], times[-2]
  bool last_post = false;                  // post[-1]
  nts[0] = t0;
  const int cap = N + ne + 2;
  int pass = 0;
  while (last < tf) {
    if (++pass > cap) { status = HSQP_GRID_OVERFLOW; break; }
    while (ie < ne && !(t0 < ev[ie] && ev[ie] < tf)) ++ie;   // the reference's filter [e for e in events if t0 < e < tf]
    double t_next = last + dt;
    bool is_event = false;
    if (ie < ne && t_next >= ev[ie]) { t_next = ev[ie]; is_event = true; ++ie; }
    if (t_next >= tf) { t_next = tf; is_event = false; }
    if (t_next > last + dt_min || last_post) {               // times.append(t_next)
      if (n > N) { status = HSQP_GRID_OVERFLOW; break; }
      nts[n] = t_next; dts[n - 1] = t_next - last;
      ++n; prev = last; last = t_next; last_post = false;
    } else {                                                 // times[-1] = t_next (never a post-event node, never node 0's row alone)
      nts[n - 1] = t_next;
      if (n > 1) dts[n - 2] = t_next - prev;
      last = t_next;
    }
    if (is_event) {                                          // the post-event node: same time stamp, sampled an epsilon later
      if (n > N) { status = HSQP_GRID_OVERFLOW; break; }
      nts[n] = t_next + GRID_EVENT_EPS; dts[n - 1] = t_next - last;
      ++n; prev = last; last = t_next; last_post = true;
    }
  }
  const int Nb = n - 1;
  if (status == HSQP_GRID_OK) {
    // what set_grid asks of host arrays: every interval finite and >= 0 (so the raw stamps do not decrease, which the next HSQP_WARM_SHIFT needs), the
    // last one no event
    if (Nb < 1 || !(dts[Nb - 1] > 0.0)) status = HSQP_GRID_OVERFLOW;
    for (int k = 0; k < Nb && status == HSQP_GRID_OK; ++k)
      if (!(dts[k] >= 0.0) || !(dts[k] <= 1e6)) status = HSQP_GRID_OVERFLOW;
  }
  if (status != HSQP_GRID_OK) {
    double t = t0;
    nts[0] = t0;
    for (int k = 0; k < N; ++k) { const double tn = t + dt; dts[k] = tn - t; nts[k + 1] = tn; t = tn; }
    *n_intervals = 0;
    return status;
  }
  // padding: N - Nb zero-length intervals in front of the last interval, their nodes duplicates of node Nb - 1
  if (Nb < N) {
    const double d_last = dts[Nb - 1], t_end = nts[Nb], t_dup = nts[Nb - 1];
    for (int k = Nb - 1; k < N - 1; ++k) { dts[k] = 0.0; nts[k + 1] = t_dup; }
    dts[N - 1] = d_last; nts[N] = t_end;
  }
  *n_intervals = Nb;
  return status;
}

}  // namespace hsqp
