// Batched policy rollout (include/hsqp_rollout.h; upstream ocs2 MRT_BASE::rolloutPolicy: a TimeTriggeredRollout of the flow map under the
// current controller).  One workgroup integrates one instance over all its sample intervals: the adaptive loop, the restarts at samples and
// events and the step control run inside, every decision uniform across the workgroup (each thread runs the same scalar control on values
// read from LDS after a barrier; the error norm is a workgroup reduction).
//   flow maps:   whole-body  xdot = [x[29..57], a_b, u[12..34]]  (stage_topology + stage_eval<false>, hsqp_model.h, as policy_node fills it);
//                centroidal  xdot = [12 dense rows of cent_lane_flow<double> (CK_NONE), u[12..34]]  (hsqp_cent_lq.h)
//   controllers: feed-forward  u(s) = the input hsqp_evaluate_policy interpolates (policy_segment_*, hsqp_feedback.h);
//                feedback      u(s, x) = uff(s) + K(s) x blended on the same segment in the order of k_feedback_eval (hsqp_capi.hip), from a
//                              window of policy entries [first, first + count) formed beforehand by k_feedback_gains
//   integrators: Dormand–Prince 5(4) with FSAL and odeint's step control (ODE45), classical RK4 with a fixed step; the step-control
//                rules and the step cap are restated from memory of boost odeint / ocs2 (include/hsqp_rollout.h: the assumptions).
//   pushes:      the external pushes of the instance (include/hsqp_push.h, hsqp_push.h) act on the plant only: rollout_push adds the active
//                ones behind the flow evaluation of the rollout (no other user of stage_eval<false> / cent_lane_flow sees them), their edges
//                are break points beside the grid's events, and a segment's activity is fixed at its start.  An instance without pushes
//                never enters that code.
//   plant:       with the torque plant set (include/hsqp_plant.h, hsqp_plant.h) the compliant plant replaces the flow evaluation: full forward dynamics
//                under the joint PD law, the pushes acting through the whole tree.  Its options — the ground of include/hsqp_contact.h (penalty forces
//                at the eight sole corners in place of the policy's contact wrenches), the actuator model of include/hsqp_actuator.h (the joint command
//                sampled at ticks and held, effort limits, passive joint torques: rollout_instance drives the ticks and writes the record of the
//                last torques) and the per-instance link scales and payloads of include/hsqp_inertia.h (inertia_apply behind the stage_eval<false>
//                at the plant's own state; the policy and tau_ff stay on the nominal model) and the height-map terrain of include/hsqp_terrain.h under
//                that ground (each sole corner on the map's height and normal under it) — are parameters of the instantiation, not run-time
//                branches: an option that is off is not in the code that runs.
// ONE entry and ONE rule hold the instantiations together:
//   rollout_entry     what one workgroup does for one instance of a call: the entry of the host emulation (tests/rollout/rollout_emu.h, one-lane
//                     context).  k_rollout / k_rollout_plant (hsqp_capi.hip) spell the same statements out: called through it they measured slower
//   rollout_dispatch  (host) the stage workspace a configuration gets: the one list of the fourteen types
#pragma once
#include "hsqp_policy.h"
#include "hsqp_cent_lq.h"
#include "hsqp_feedback.h"
#include "hsqp_push.h"
#include "hsqp_plant.h"
#include "../../include/hsqp_rollout.h"

namespace hsqp {

constexpr int RO_THREADS = 128;                  // threads of the rollout workgroup (the stage evaluations' width: k_policy_torques)
constexpr int RO_MAX_REJECTS = 500;              // consecutive rejected ODE45 steps that end an instance (odeint's failed-step checker)

// The resident policy of ONE instance
struct RolloutPolicy {
  const double* ut;       // [N][NU] optimal inputs (feed-forward controller)
  const double* dts;      // [N] interval lengths (0: event) of a non-uniform grid, or null: uniform grid of spacing dt (no events)
  int N;
  double dt;
  const double* K;        // [count][NU][NX] gain entries first .. first + count - 1 (feedback controller)
  const double* uff;      // [count][NU]
  int first, count;
  int cent;               // centroidal handle: 35 live states
};

template <class SW>
struct RolloutWS {
  SW sw;                  // stage workspace of the flow evaluation (StageWST<false> / CentWST<false>)
  double k[7][NX];        // stage derivatives (k[0]: at the start of the step)
  double x[NX];           // state at the start of the step
  double xs[NX];          // stage state
  double xn[NX];          // state at the end of the step
  double u[NU];           // controller input of the evaluation
  double red[RO_THREADS]; // per-thread partials of the workgroup reductions (error norm, finiteness)
  PushSet push;           // the instance's pushes (read once at the start of rollout_instance)
};

HSQP_HD bool ro_finite(double v) { return v - v == 0.0; }

// ---- flow maps: xdot [NX] of (x, u) through the workspace.  Entries of the centroidal padding are zero.
HSQP_HD void rollout_topology(const Ctx& ctx, const DevModel& dm, StageWST<false>& ws) { stage_topology(ctx, dm, ws); }
HSQP_HD void rollout_topology(const Ctx& ctx, const DevModel& dm, CentWST<false>& ws) { cent_ws_topology(ctx, dm, ws); }
HSQP_HD void rollout_topology(const Ctx& ctx, const DevModel& dm, PlantStage& ws) { stage_topology(ctx, dm, ws.st); }
HSQP_HD void rollout_topology(const Ctx& ctx, const DevModel& dm, PlantContactStage& ws) { stage_topology(ctx, dm, ws.st); }
HSQP_HD void rollout_topology(const Ctx& ctx, const DevModel& dm, PlantActStage& ws) { stage_topology(ctx, dm, ws.st); }
HSQP_HD void rollout_topology(const Ctx& ctx, const DevModel& dm, PlantContactActStage& ws) { stage_topology(ctx, dm, ws.st); }
HSQP_HD void rollout_topology(const Ctx& ctx, const DevModel& dm, PlantTerrainStage& ws) { stage_topology(ctx, dm, ws.st); }
HSQP_HD void rollout_topology(const Ctx& ctx, const DevModel& dm, PlantTerrainActStage& ws) { stage_topology(ctx, dm, ws.st); }

// whether the stage workspace carries the actuator model (ws.act)
template <class SW> struct RolloutActuated { static constexpr bool value = false; };
template <> struct RolloutActuated<PlantActStage> { static constexpr bool value = true; };
template <> struct RolloutActuated<PlantContactActStage> { static constexpr bool value = true; };
template <> struct RolloutActuated<PlantTerrainActStage> { static constexpr bool value = true; };
template <class Base> struct RolloutActuated<PlantVaried<Base>> : RolloutActuated<Base> {};

HSQP_HD void rollout_flow(const Ctx& ctx, const DevModel& dm, StageWST<false>& ws, const double* x, const double* u, double* xdot) {
  WG_FOR(ctx, i, NV + NV + NJ + 12) {
    if (i < NV) ws.q[i] = x[i];
    else if (i < 2 * NV) ws.v[i - NV] = x[i];
    else if (i < 2 * NV + NJ) ws.qddj[i - 2 * NV] = u[12 + i - 2 * NV];
    else ws.W[i - 2 * NV - NJ] = u[i - 2 * NV - NJ];
  }
  WG_SYNC(ctx);
  stage_eval<false>(ctx, dm, ws);
  WG_FOR(ctx, i, NX) {
    xdot[i] = i < NV ? x[NV + i] : (i < NV + 6 ? ws.ab[i - NV] : u[12 + (i - NV - 6)]);
  }
  WG_SYNC(ctx);
}

HSQP_HD void rollout_flow(const Ctx& ctx, const DevModel& dm, CentWST<false>& ws, const double* x, const double* u, double* xdot) {
  WG_FOR(ctx, i, CNX + NU) { if (i < CNX) ws.x[i] = x[i]; else ws.u[i - CNX] = u[i - CNX]; }
  WG_SYNC(ctx);
  cent_stage_values(ctx, dm, ws, 0, 0.0);
  WG_FOR(ctx, it, 1) {
    CentBase<double> base;
    double xd[12];
    cent_lane_flow<double>(dm, ws, CentCol{CK_NONE, 0}, xd, base);
    for (int r = 0; r < 12; ++r) xdot[r] = xd[r];
  }
  WG_FOR(ctx, i, NX - 12) xdot[12 + i] = i < CNX - 12 ? u[12 + i] : 0.0;
  WG_SYNC(ctx);
}

// ---- external pushes (include/hsqp_push.h): the pushes `mask` names, applied to the xdot rollout_flow has just formed from the same workspace.
// The placements R / r of every body (relative to the base origin O) are those of the evaluation.
// Whole-body: the wrench {P x f, f} about O joins F_ext - F in Ftil, where the contact wrenches entered, and the two base solves of
// stage_eval's totals are redone on it (Iinv, Einv and the total mass are still in the workspace).
HSQP_HD void rollout_push(const Ctx& ctx, const DevModel&, StageWST<false>& ws, PushSet& ps, unsigned mask, double* xdot) {
  WG_FOR(ctx, i, ps.n) {
    if (!((mask >> i) & 1u)) continue;
    const int b = ps.body[i];
    double P[3], mom[3];
    m3_mulv(ws.R[b], ps.point[i], P);
    for (int k = 0; k < 3; ++k) P[k] += ws.r[b][k];
    v3_cross(P, ps.force[i], mom);
    for (int k = 0; k < 3; ++k) { ps.wr[i][k] = mom[k]; ps.wr[i][3 + k] = ps.force[i][k]; }
  }
  WG_SYNC(ctx);
  WG_FOR(ctx, it, 1) {
    for (int i = 0; i < ps.n; ++i)
      if ((mask >> i) & 1u) for (int k = 0; k < 6; ++k) ws.Ftil[k] += ps.wr[i][k];
    m3_mulv(ws.Iinv, ws.Ftil, ws.y);
    const double minv = 1.0 / ws.Ic[0][0];
    for (int k = 0; k < 3; ++k) ws.ab[k] = ws.Ftil[3 + k] * minv;
    m3_mulv(ws.Einv, ws.y, ws.ab + 3);
    for (int k = 0; k < 6; ++k) xdot[NV + k] = ws.ab[k];
  }
  WG_SYNC(ctx);
}
// Centroidal: f / m into the linear, (P - com) x f / m into the angular rows of the normalised momentum rate (com as cent_finish forms it)
HSQP_HD void rollout_push(const Ctx& ctx, const DevModel& dm, CentWST<false>& ws, PushSet& ps, unsigned mask, double* xdot) {
  WG_FOR(ctx, i, ps.n) {
    if (!((mask >> i) & 1u)) continue;
    const int b = ps.body[i];
    const double iM = 1.0 / dm.total_mass;
    double P[3], arm[3], mom[3];
    m3_mulv(ws.R[b], ps.point[i], P);
    for (int k = 0; k < 3; ++k) arm[k] = (P[k] + ws.r[b][k]) - ws.sums[k] * iM;
    v3_cross(arm, ps.force[i], mom);
    for (int k = 0; k < 3; ++k) { ps.wr[i][k] = ps.force[i][k] * iM; ps.wr[i][3 + k] = mom[k] * iM; }
  }
  WG_SYNC(ctx);
  WG_FOR(ctx, r, 6) {
    double acc = xdot[r];
    for (int i = 0; i < ps.n; ++i)
      if ((mask >> i) & 1u) acc += ps.wr[i][r];
    xdot[r] = acc;
  }
  WG_SYNC(ctx);
}

// ---- controller input u [NU] at s seconds after the first node and the state x
HSQP_HD void rollout_control(const Ctx& ctx, const RolloutPolicy& p, int controller, double s, const double* x, double* u) {
  const PolicySegment g = p.dts ? policy_segment_grid(p.N, p.dts, s) : policy_segment_uniform(p.N, p.dt, s);
  if (controller == HSQP_ROLLOUT_FEEDFORWARD) {
    const int ku = g.ku;
    const double au = g.au;
    WG_FOR(ctx, c, NU) u[c] = p.N >= 2 ? (1.0 - au) * p.ut[(size_t)ku * NU + c] + au * p.ut[(size_t)(ku + 1) * NU + c] : p.ut[c];
  } else {
    // entries ku, ku + 1 of the policy inside the window (the window covers every time of the call; the clamp only keeps reads in bounds)
    int e = g.ku - p.first;
    e = e < 0 ? 0 : (e > p.count - 2 ? p.count - 2 : e);
    const double* K0 = p.K + (size_t)e * NU * NX;
    const double* K1 = K0 + NU * NX;
    const double* u0 = p.uff + (size_t)e * NU;
    const double* u1 = u0 + NU;
    const double a = g.au;
    const int nc = p.cent ? CNX : NX;
    WG_FOR(ctx, r, NU) {
      double kx = 0.0;
      for (int c = 0; c < nc; ++c) kx += ((1.0 - a) * K0[(size_t)r * NX + c] + a * K1[(size_t)r * NX + c]) * x[c];
      u[r] = ((1.0 - a) * u0[r] + a * u1[r]) + kx;
    }
  }
  WG_SYNC(ctx);
}

// one evaluation of the closed loop: k = f(x, u(s, x)) (a non-finite input reaches k: its joint part is copied, the wrenches enter a_b),
// with the pushes `mask` of the segment (0: none)
template <class SW>
HSQP_HD void rollout_eval(const Ctx& ctx, const DevModel& dm, RolloutWS<SW>& w, const RolloutPolicy& p, int controller, double s, const double* x,
                          double* k, unsigned mask) {
  rollout_control(ctx, p, controller, s, x, w.u);
  rollout_flow(ctx, dm, w.sw, x, w.u, k);
  if (mask) rollout_push(ctx, dm, w.sw, w.push, mask, k);
}

// The same with the torque plant (include/hsqp_plant.h; the workspace's plant setting was loaded by plant_load): the policy (x_p, u_p) at
// s + lookahead — feedback: u_p = uff + K x at the measured plant state, x_p the interpolated nominal state —, tau_ff = joint_torques at
// (x_p, u_p), the joint law, then forward dynamics at the plant's own state under the policy's contact wrenches and the pushes `mask`.  With the
// ground of include/hsqp_contact.h (workspace RolloutWS<PlantContactStage>, an instantiation of its own) the contact model's forces at
// the plant's own (q, v) replace the policy's wrenches in the dynamics; tau_ff keeps them.
// rollout_plant_command: steps 1-2 of include/hsqp_plant.h at time s and the measured state x — (x_p, u_p) into pl.xp / w.u, tau_ff into pl.tau (no
// barrier behind it); the plant's own joint law and the actuator model's command (below) both start from it.
template <class SW>
HSQP_HD void rollout_plant_command(const Ctx& ctx, const DevModel& dm, RolloutWS<SW>& w, const RolloutPolicy& p, int controller, double s, const double* x) {
  PlantWS& pl = w.sw.pl;
  const double sl = s + pl.lookahead;
  rollout_control(ctx, p, controller, sl, x, w.u);
  const PolicySegment g = p.dts ? policy_segment_grid(p.N, p.dts, sl) : policy_segment_uniform(p.N, p.dt, sl);
  WG_FOR(ctx, i, NX) pl.xp[i] = (1.0 - g.ax) * pl.xt[(size_t)g.kx * NX + i] + g.ax * pl.xt[(size_t)(g.kx + 1) * NX + i];
  WG_SYNC(ctx);
  plant_inputs(ctx, w.sw.st, pl.xp, w.u, false);
  stage_eval<false>(ctx, dm, w.sw.st);
  joint_torques(ctx, dm, w.sw.st, pl.tau);
}
template <class SW, class CT>
HSQP_HD void rollout_eval_plant(const Ctx& ctx, const DevModel& dm, RolloutWS<SW>& w, CT* ct, const RolloutPolicy& p, int controller, double s,
                                const double* x, double* k, unsigned mask) {
  PlantWS& pl = w.sw.pl;
  rollout_plant_command(ctx, dm, w, p, controller, s, x);
  WG_FOR(ctx, j, NJ) pl.tau[j] = (pl.tau[j] + pl.kp[j] * (pl.xp[6 + j] - x[6 + j])) + pl.kd[j] * (pl.xp[NV + 6 + j] - x[NV + 6 + j]);
  plant_inputs(ctx, w.sw.st, x, w.u, true);   // (its barrier also closes the joint law)
  stage_eval<false>(ctx, dm, w.sw.st);
  if constexpr (PlantIsVaried<SW>::value) inertia_apply(ctx, w.sw.st, w.sw.iw);   // (the plant's own body: include/hsqp_inertia.h)
  plant_forward_dynamics(ctx, dm, w.sw.st, pl, w.push, mask, ct);
  WG_FOR(ctx, i, NX) k[i] = i < NV ? x[NV + i] : pl.vd[i - NV];
  WG_SYNC(ctx);
}
HSQP_HD void rollout_eval(const Ctx& ctx, const DevModel& dm, RolloutWS<PlantStage>& w, const RolloutPolicy& p, int controller, double s, const double* x,
                          double* k, unsigned mask) {
  rollout_eval_plant(ctx, dm, w, (ContactSet*)nullptr, p, controller, s, x, k, mask);
}
HSQP_HD void rollout_eval(const Ctx& ctx, const DevModel& dm, RolloutWS<PlantContactStage>& w, const RolloutPolicy& p, int controller, double s,
                          const double* x, double* k, unsigned mask) {
  rollout_eval_plant(ctx, dm, w, &w.sw.ct, p, controller, s, x, k, mask);
}

// The same under the actuator model (include/hsqp_actuator.h; the workspace's setting was loaded by actuator_load).
// rollout_actuator_sample: the joint command of time s and the measured state x — steps 1-2 above — into the workspace, where it is held: at a
// tick of a sampled command (rollout_instance), or at every evaluation of a continuous one.  Ends with a barrier.
template <class SW>
HSQP_HD void rollout_actuator_sample(const Ctx& ctx, const DevModel& dm, RolloutWS<SW>& w, const RolloutPolicy& p, int controller, double s, const double* x) {
  PlantWS& pl = w.sw.pl;
  ActuatorWS& ac = w.sw.act;
  rollout_plant_command(ctx, dm, w, p, controller, s, x);
  WG_FOR(ctx, j, NJ) { ac.tff[j] = pl.tau[j]; ac.qp[j] = pl.xp[6 + j]; ac.vp[j] = pl.xp[NV + 6 + j]; }
  WG_FOR(ctx, i, 12) ac.Wp[i] = w.u[i];   // (w.u itself is the sample outputs' too: rollout_instance overwrites it)
  WG_SYNC(ctx);
}
// one evaluation: the command in force (a continuous one is formed here), the joint law at the plant's own state, forward dynamics
template <class SW, class CT>
HSQP_HD void rollout_eval_actuated(const Ctx& ctx, const DevModel& dm, RolloutWS<SW>& w, CT* ct, const RolloutPolicy& p, int controller, double s,
                                   const double* x, double* k, unsigned mask) {
  PlantWS& pl = w.sw.pl;
  ActuatorWS& ac = w.sw.act;
  if (!(ac.period > 0.0)) rollout_actuator_sample(ctx, dm, w, p, controller, s, x);
  actuator_law(ctx, ac, pl.kp, pl.kd, x, pl.tau, nullptr);
  plant_inputs(ctx, w.sw.st, x, ac.Wp, true);   // (reads the twelve wrenches only; its barrier also closes the joint law)
  stage_eval<false>(ctx, dm, w.sw.st);
  if constexpr (PlantIsVaried<SW>::value) inertia_apply(ctx, w.sw.st, w.sw.iw);   // (the plant's own body: include/hsqp_inertia.h)
  plant_forward_dynamics(ctx, dm, w.sw.st, pl, w.push, mask, ct);
  WG_FOR(ctx, i, NX) k[i] = i < NV ? x[NV + i] : pl.vd[i - NV];
  WG_SYNC(ctx);
}
HSQP_HD void rollout_eval(const Ctx& ctx, const DevModel& dm, RolloutWS<PlantActStage>& w, const RolloutPolicy& p, int controller, double s, const double* x,
                          double* k, unsigned mask) {
  rollout_eval_actuated(ctx, dm, w, (ContactSet*)nullptr, p, controller, s, x, k, mask);
}
HSQP_HD void rollout_eval(const Ctx& ctx, const DevModel& dm, RolloutWS<PlantContactActStage>& w, const RolloutPolicy& p, int controller, double s,
                          const double* x, double* k, unsigned mask) {
  rollout_eval_actuated(ctx, dm, w, &w.sw.ct, p, controller, s, x, k, mask);
}
// ... and either grounded one on the height-map terrain (include/hsqp_terrain.h; the workspace's map was loaded by terrain_load)
HSQP_HD void rollout_eval(const Ctx& ctx, const DevModel& dm, RolloutWS<PlantTerrainStage>& w, const RolloutPolicy& p, int controller, double s,
                          const double* x, double* k, unsigned mask) {
  rollout_eval_plant(ctx, dm, w, &w.sw.ct, p, controller, s, x, k, mask);
}
HSQP_HD void rollout_eval(const Ctx& ctx, const DevModel& dm, RolloutWS<PlantTerrainActStage>& w, const RolloutPolicy& p, int controller, double s,
                          const double* x, double* k, unsigned mask) {
  rollout_eval_actuated(ctx, dm, w, &w.sw.ct, p, controller, s, x, k, mask);
}
// ... and any of the six on a varied plant (include/hsqp_inertia.h; the workspace's entry was loaded by inertia_load)
template <class Base>
HSQP_HD void rollout_eval(const Ctx& ctx, const DevModel& dm, RolloutWS<PlantVaried<Base>>& w, const RolloutPolicy& p, int controller, double s, const double* x,
                          double* k, unsigned mask) {
  typename PlantGroundSet<Base>::type* ct = nullptr;
  if constexpr (PlantGrounded<Base>::value) ct = &w.sw.ct;
  if constexpr (RolloutActuated<Base>::value) rollout_eval_actuated(ctx, dm, w, ct, p, controller, s, x, k, mask);
  else rollout_eval_plant(ctx, dm, w, ct, p, controller, s, x, k, mask);
}
// the record of include/hsqp_actuator.h at the instance's final state w.x (time s): the joint law once more under the command in force, or NaN rows
template <class SW>
HSQP_HD void rollout_actuator_record(const Ctx& ctx, const DevModel& dm, RolloutWS<SW>& w, const RolloutPolicy& p, int controller, double s, bool ok) {
  PlantWS& pl = w.sw.pl;
  ActuatorWS& ac = w.sw.act;
  WG_SYNC(ctx);   // (the sample outputs have been read from w.u)
  if (!ok) {
    WG_FOR(ctx, i, 3 * NJ) ac.rec[i] = __builtin_nan("");
    return;
  }
  if (!(ac.period > 0.0)) rollout_actuator_sample(ctx, dm, w, p, controller, s, w.x);
  actuator_law(ctx, ac, pl.kp, pl.kd, w.x, pl.tau, ac.rec);
}

// whether any of the first n entries of rows r0 .. r1 - 1 of v (row stride NX) is not finite: a workgroup reduction, uniform
template <class SW>
HSQP_HD bool rollout_nonfinite(const Ctx& ctx, RolloutWS<SW>& w, const double* v, int r0, int r1, int n) {
  double f = 0.0;
  WG_FOR(ctx, i, n) for (int r = r0; r < r1; ++r) if (!ro_finite(v[(size_t)r * NX + i])) f = 1.0;
  w.red[ctx.tid] = f;
  WG_SYNC(ctx);
  bool any = false;
  for (int t = 0; t < ctx.nthreads; ++t) any = any || w.red[t] != 0.0;
  WG_SYNC(ctx);
  return any;
}

// Dormand–Prince 5(4) tableau: c, a (row s: the ns = s coefficients of stage s), the 5th-order weights b (= row 6 of a), b - b* (error)
struct Dopri {
  static constexpr double c2 = 1.0 / 5.0, c3 = 3.0 / 10.0, c4 = 4.0 / 5.0, c5 = 8.0 / 9.0;
  static constexpr double a21 = 1.0 / 5.0;
  static constexpr double a31 = 3.0 / 40.0, a32 = 9.0 / 40.0;
  static constexpr double a41 = 44.0 / 45.0, a42 = -56.0 / 15.0, a43 = 32.0 / 9.0;
  static constexpr double a51 = 19372.0 / 6561.0, a52 = -25360.0 / 2187.0, a53 = 64448.0 / 6561.0, a54 = -212.0 / 729.0;
  static constexpr double a61 = 9017.0 / 3168.0, a62 = -355.0 / 33.0, a63 = 46732.0 / 5247.0, a64 = 49.0 / 176.0, a65 = -5103.0 / 18656.0;
  static constexpr double b1 = 35.0 / 384.0, b3 = 500.0 / 1113.0, b4 = 125.0 / 192.0, b5 = -2187.0 / 6784.0, b6 = 11.0 / 84.0;
  static constexpr double e1 = 35.0 / 384.0 - 5179.0 / 57600.0, e3 = 500.0 / 1113.0 - 7571.0 / 16695.0, e4 = 125.0 / 192.0 - 393.0 / 640.0,
                          e5 = -2187.0 / 6784.0 + 92097.0 / 339200.0, e6 = 11.0 / 84.0 - 187.0 / 2100.0, e7 = -1.0 / 40.0;
};

// Row s of the tableau of either integrator: the coefficient of k[j] in the state of stage s (ODE45: s = 1 .. 6, row 6 = the 5th-order
// weights; RK4: s = 1 .. 3), and the stage's time as a fraction of the step (c)
HSQP_HD double rollout_a(bool ode45, int s, int j) {
  if (!ode45) return j == s - 1 ? (s == 3 ? 1.0 : 0.5) : 0.0;
  switch (s) {
    case 1: return Dopri::a21;
    case 2: return j == 0 ? Dopri::a31 : Dopri::a32;
    case 3: return j == 0 ? Dopri::a41 : (j == 1 ? Dopri::a42 : Dopri::a43);
    case 4: return j == 0 ? Dopri::a51 : (j == 1 ? Dopri::a52 : (j == 2 ? Dopri::a53 : Dopri::a54));
    case 5: return j == 0 ? Dopri::a61 : (j == 1 ? Dopri::a62 : (j == 2 ? Dopri::a63 : (j == 3 ? Dopri::a64 : Dopri::a65)));
    default: return j == 0 ? Dopri::b1 : (j == 1 ? 0.0 : (j == 2 ? Dopri::b3 : (j == 3 ? Dopri::b4 : (j == 4 ? Dopri::b5 : Dopri::b6))));
  }
}
HSQP_HD double rollout_c(bool ode45, int s) {
  if (!ode45) return s == 0 ? 0.0 : (s == 3 ? 1.0 : 0.5);
  return s == 0 ? 0.0 : (s == 1 ? Dopri::c2 : (s == 2 ? Dopri::c3 : (s == 3 ? Dopri::c4 : (s == 4 ? Dopri::c5 : 1.0))));
}

// out = x + h sum_{j < s} a_sj k[j] over the nl live entries (the accumulation runs in j order)
template <class SW>
HSQP_HD void rollout_combine(const Ctx& ctx, RolloutWS<SW>& w, int nl, bool ode45, int s, double h, double* out) {
  WG_FOR(ctx, i, nl) {
    double acc = 0.0;
    for (int j = 0; j < s; ++j) acc += rollout_a(ode45, s, j) * w.k[j][i];
    out[i] = w.x[i] + h * acc;
  }
  WG_SYNC(ctx);
}

// The stage evaluations of one step of length h from (t, w.x) ending at tn: k[first_stage .. last_stage] (ODE45: 1 .. 6, k[0] is the FSAL
// derivative, the stage-6 state — the 5th-order solution — goes to w.xn; RK4: 0 .. 3).  One call site of the flow evaluation per step.
template <class SW>
HSQP_HD void rollout_stages(const Ctx& ctx, const DevModel& dm, RolloutWS<SW>& w, const RolloutPolicy& p, int controller, bool ode45, int nl, double t,
                            double h, double tn, unsigned mask) {
  for (int s = ode45 ? 1 : 0; s < (ode45 ? 7 : 4); ++s) {
    const double c = rollout_c(ode45, s);
    double* xe = s == 6 ? w.xn : w.xs;
    if (s > 0) rollout_combine(ctx, w, nl, ode45, s, h, xe);
    rollout_eval(ctx, dm, w, p, controller, c == 1.0 ? tn : t + c * h, s > 0 ? xe : w.x, w.k[s], mask);
  }
}

// err = max_i |h sum e_j k_j| / (abs_tol + rel_tol (|x_i| + h |k1_i|)) over the live entries (NaN propagates); uniform across the workgroup
template <class SW>
HSQP_HD double rollout_error(const Ctx& ctx, RolloutWS<SW>& w, int nl, double h, double abs_tol, double rel_tol) {
  double m = 0.0;
  WG_FOR(ctx, i, nl) {
    const double e = h * (Dopri::e1 * w.k[0][i] + Dopri::e3 * w.k[2][i] + Dopri::e4 * w.k[3][i] + Dopri::e5 * w.k[4][i] + Dopri::e6 * w.k[5][i] +
                          Dopri::e7 * w.k[6][i]);
    const double r = fabs(e) / (abs_tol + rel_tol * (fabs(w.x[i]) + h * fabs(w.k[0][i])));
    if (!(r <= m)) m = r;
  }
  w.red[ctx.tid] = m;
  WG_SYNC(ctx);
  double err = 0.0;
  for (int t = 0; t < ctx.nthreads; ++t) { const double v = w.red[t]; if (!(v <= err)) err = v; }
  WG_SYNC(ctx);
  return err;
}

// Integrates w.x from ta to tb (no event and no push edge inside) and returns HSQP_ROLLOUT_*.  acc: accepted steps of the sample interval so
// far (cap: its limit), nacc / nrej: the instance's accepted / rejected steps.  The pushes that act are those active at ta, for every stage
// evaluation of the segment (the one at tb included).
template <class SW>
HSQP_HD int rollout_segment(const Ctx& ctx, const DevModel& dm, RolloutWS<SW>& w, const RolloutPolicy& p, const hsqp_rollout_settings& st, double ta,
                            double tb, double cap, int& acc, int& nacc, int& nrej) {
  const int nl = p.cent ? CNX : NX;
  const bool ode45 = st.integrator == HSQP_ROLLOUT_ODE45;
  double h = st.initial_step < tb - ta ? st.initial_step : tb - ta;
  double t = ta;
  int fails = 0;
  const unsigned mask = w.push.n ? push_active(w.push, ta) : 0u;
  if (ode45) {   // FSAL: the derivative at the start of the segment, then the last stage of every accepted step
    rollout_eval(ctx, dm, w, p, st.controller, t, w.x, w.k[0], mask);
    if (rollout_nonfinite(ctx, w, &w.k[0][0], 0, 1, nl)) return HSQP_ROLLOUT_NONFINITE;
  }
  while (t < tb) {
    if ((double)acc >= cap) return HSQP_ROLLOUT_MAX_STEPS;
    if (ode45) {
      const bool last = tb - t <= h;
      if (last) h = tb - t;
      const double tn = last ? tb : t + h;
      rollout_stages(ctx, dm, w, p, st.controller, true, nl, t, h, tn, mask);
      if (rollout_nonfinite(ctx, w, &w.k[0][0], 1, 7, nl)) return HSQP_ROLLOUT_NONFINITE;
      const double err = rollout_error(ctx, w, nl, h, st.abs_tol, st.rel_tol);
      if (!(err <= 1.0)) {
        if (err != err) return HSQP_ROLLOUT_NONFINITE;
        const double f = 0.9 * pow(err, -1.0 / 3.0);
        h *= f > 0.2 ? f : 0.2;
        ++nrej;
        if (++fails > RO_MAX_REJECTS) return HSQP_ROLLOUT_MAX_STEPS;
        continue;
      }
      fails = 0;
      WG_FOR(ctx, i, nl) { w.x[i] = w.xn[i]; w.k[0][i] = w.k[6][i]; }
      WG_SYNC(ctx);
      t = tn;
      ++acc; ++nacc;
      if (err < 0.5) {
        const double e = err > 1.0 / 3125.0 ? err : 1.0 / 3125.0;   // max(err, 5^-5)
        h *= 0.9 * pow(e, -1.0 / 5.0);
      }
    } else {
      const bool last = tb - t <= h;
      const double hs = last ? tb - t : h, tn = last ? tb : t + hs;
      rollout_stages(ctx, dm, w, p, st.controller, false, nl, t, hs, tn, mask);
      if (rollout_nonfinite(ctx, w, &w.k[0][0], 0, 4, nl)) return HSQP_ROLLOUT_NONFINITE;
      WG_FOR(ctx, i, nl) w.x[i] = w.x[i] + hs / 6.0 * (w.k[0][i] + 2.0 * w.k[1][i] + 2.0 * w.k[2][i] + w.k[3][i]);
      WG_SYNC(ctx);
      t = tn;
      ++acc; ++nacc;
    }
  }
  return HSQP_ROLLOUT_OK;
}

// the first break point strictly inside (t, tb), else tb: an event stamp of the grid (stamps summed in the order of policy_segment_grid) or an
// edge of one of the instance's pushes
HSQP_HD double rollout_next_event(const RolloutPolicy& p, const PushSet& ps, double t, double tb) {
  double te = tb;
  if (p.dts) {
    double tk = 0.0;
    for (int k = 0; k < p.N; ++k) {
      if (p.dts[k] == 0.0 && tk > t && tk < tb) { te = tk; break; }
      tk += p.dts[k];
    }
  }
  return ps.n ? push_next_edge(ps, t, te) : te;
}
// ... or the next tick of a sampled joint command (include/hsqp_actuator.h; tick > t), whichever comes first
HSQP_HD double rollout_next_event(const RolloutPolicy& p, const PushSet& ps, double t, double tb, double tick) {
  return rollout_next_event(p, ps, t, tick < tb ? tick : tb);
}

// sample j of n: s0 + duration (j + 1) / n, the last one s0 + duration exactly
HSQP_HD double rollout_sample_time(double s0, double duration, int j, int n) { return j + 1 == n ? s0 + duration : s0 + duration * (double)(j + 1) / (double)n; }

// One instance: x0 at s0, n samples over duration.  xo [n][NX], uo [n][NU] (may be null); the counters are written by item 0.
// tbl, b: the resident push table and the instance's row in it (the default: no table).
template <class SW>
HSQP_HD void rollout_instance(const Ctx& ctx, const DevModel& dm, RolloutWS<SW>& w, const RolloutPolicy& p, const hsqp_rollout_settings& st, double s0,
                              const double* x0, double duration, int n, double* xo, double* uo, int32_t* status, int32_t* steps, int32_t* rejected,
                              const PushTable& tbl = PushTable{nullptr, nullptr, 0, nullptr, 0}, int b = 0) {
  const int nl = p.cent ? CNX : NX;
  push_load(ctx, tbl, b, w.push);
  rollout_topology(ctx, dm, w.sw);
  WG_FOR(ctx, i, NX) w.x[i] = i < nl ? x0[i] : 0.0;
  WG_SYNC(ctx);
  int stat = HSQP_ROLLOUT_OK, nacc = 0, nrej = 0;
  double ta = s0;
  for (int j = 0; j < n; ++j) {
    const double tb = rollout_sample_time(s0, duration, j, n);
    if (stat == HSQP_ROLLOUT_OK) {
      const double len = tb - ta;
      const double cap = st.max_steps_per_second * (len > 1.0 ? len : 1.0);
      int acc = 0;
      double t = ta;
      while (stat == HSQP_ROLLOUT_OK && t < tb) {
        double te;
        if constexpr (RolloutActuated<SW>::value) {
          // a sampled command: the command is taken where the segment starts on a tick (the call's start is tick 0), the next tick ends the segment
          double tick = tb;
          if (w.sw.act.period > 0.0) {
            const ActuatorTick tk = actuator_tick(s0, w.sw.act.period, t);
            if (!(tk.next > t) || !ro_finite(tk.next)) { stat = HSQP_ROLLOUT_MAX_STEPS; break; }
            if (tk.on) rollout_actuator_sample(ctx, dm, w, p, st.controller, t, w.x);
            tick = tk.next;
          }
          te = rollout_next_event(p, w.push, t, tb, tick);
        } else {
          te = rollout_next_event(p, w.push, t, tb);
        }
        stat = rollout_segment(ctx, dm, w, p, st, t, te, cap, acc, nacc, nrej);
        t = te;
      }
      if (stat == HSQP_ROLLOUT_OK) {
        rollout_control(ctx, p, st.controller, tb, w.x, w.u);
        if (rollout_nonfinite(ctx, w, w.u, 0, 1, NU)) stat = HSQP_ROLLOUT_NONFINITE;
      }
    }
    const bool ok = stat == HSQP_ROLLOUT_OK;
    const double nan = __builtin_nan("");
    if (xo) WG_FOR(ctx, i, NX) xo[(size_t)j * NX + i] = ok ? (i < nl ? w.x[i] : 0.0) : nan;
    if (uo) WG_FOR(ctx, r, NU) uo[(size_t)j * NU + r] = ok ? w.u[r] : nan;
    ta = tb;
  }
  if constexpr (RolloutActuated<SW>::value) rollout_actuator_record(ctx, dm, w, p, st.controller, s0 + duration, stat == HSQP_ROLLOUT_OK);
  WG_FOR(ctx, i, 1) {
    *status = stat;
    if (steps) *steps = nacc;
    if (rejected) *rejected = nrej;
  }
}

// The arguments of one rollout call over the batch, as the kernels take them
struct RolloutArgs {
  const double* ut; const double* dts; int N; double dt;   // resident inputs and grid (dts null: uniform)
  const double* K; const double* uff; int first, count;     // gain window [B][count] (feedback controller)
  hsqp_rollout_settings st;
  const double* s0; const double* x0; double duration; int n;
  double* x; double* u; int32_t* status; int32_t* steps; int32_t* rejected;
  PushTable push;                                           // the resident push table (include/hsqp_push.h; n null: none)
};

// whether the stage workspace is one of the torque plant's (ws.pl) and not a flow map's
template <class SW> struct RolloutOnPlant { static constexpr bool value = true; };
template <> struct RolloutOnPlant<StageWST<false>> { static constexpr bool value = false; };
template <> struct RolloutOnPlant<CentWST<false>> { static constexpr bool value = false; };

// Instance b of the call: its policy, the parts of the plant's setting that SW carries (a flow workspace: none, pp .. ip are not read), the integration
template <class SW>
HSQP_HD void rollout_entry(const Ctx& ctx, const DevModel& dm, RolloutWS<SW>& w, const RolloutArgs& a, const PlantParams& pp, const ContactParams& cp,
                           const ActuatorParams& ap, const InertiaParams& ip, const TerrainParams& tp, int b) {
  const RolloutPolicy p{a.ut + (size_t)b * a.N * NU, a.dts ? a.dts + (size_t)b * a.N : nullptr, a.N, a.dt, a.K ? a.K + (size_t)b * a.count * NU * NX : nullptr,
                        a.uff ? a.uff + (size_t)b * a.count * NU : nullptr, a.first, a.count,
                        !RolloutOnPlant<SW>::value && dm.formulation == HSQP_FORM_CENTROIDAL ? 1 : 0};
  if constexpr (RolloutOnPlant<SW>::value) plant_load(ctx, pp, b, a.N, w.sw.pl);
  if constexpr (PlantGrounded<SW>::value) contact_load(ctx, cp, b, w.sw.ct);
  if constexpr (PlantOnTerrain<SW>::value) terrain_load(ctx, tp, b, w.sw.ct.ter);
  if constexpr (RolloutActuated<SW>::value) actuator_load(ctx, ap, b, w.sw.act);
  if constexpr (PlantIsVaried<SW>::value) inertia_load(ctx, ip, b, w.sw.iw);
  rollout_instance(ctx, dm, w, p, a.st, a.s0[b], a.x0 + (size_t)b * NX, a.duration, a.n, a.x ? a.x + (size_t)b * a.n * NX : nullptr,
                   a.u ? a.u + (size_t)b * a.n * NU : nullptr, a.status + b, a.steps ? a.steps + b : nullptr, a.rejected ? a.rejected + b : nullptr, a.push, b);
}

// ... of a configuration without a terrain (SW carries none: tp is not read).  A caller that goes through rollout_dispatch instantiates this for the
// terrain's workspaces too; the rule gives those only to a variant with maps and a table, which this caller's variant never has: not reached, nothing to do
template <class SW>
HSQP_HD void rollout_entry(const Ctx& ctx, const DevModel& dm, RolloutWS<SW>& w, const RolloutArgs& a, const PlantParams& pp, const ContactParams& cp,
                           const ActuatorParams& ap, const InertiaParams& ip, int b) {
  if constexpr (!PlantOnTerrain<SW>::value) rollout_entry(ctx, dm, w, a, pp, cp, ap, ip, TerrainParams{nullptr, nullptr, nullptr, 0}, b);
}

// ---- host side: which instantiation a configuration gets.  The options count on the torque plant only: the ground and the actuator model while
// their setting is enabled, the variation while a table is resident, the terrain (include/hsqp_terrain.h) on the ground while both a map and a placement
// table are resident.
struct RolloutVariant {
  bool cent, torque, ground, actuated, varied, terrain;
  RolloutVariant(bool centroidal, bool torque_plant, bool contact_enabled, bool actuator_enabled, bool inertia_table, bool terrain_maps = false,
                 bool terrain_table = false)
      : cent(centroidal), torque(torque_plant), ground(torque_plant && contact_enabled), actuated(torque_plant && actuator_enabled),
        varied(torque_plant && inertia_table), terrain(torque_plant && contact_enabled && terrain_maps && terrain_table) {}
};
template <class SW> struct RolloutStageType { using type = SW; };
// f(RolloutStageType<SW>{}) for the stage workspace SW of the configuration.  The fourteen instantiations are listed here and nowhere else.
template <class F>
auto rollout_dispatch(const RolloutVariant& v, F&& f) {
  if (!v.torque) return v.cent ? f(RolloutStageType<CentWST<false>>{}) : f(RolloutStageType<StageWST<false>>{});
  if (v.terrain) switch ((v.varied ? 2 : 0) | (v.actuated ? 1 : 0)) {
    case 0: return f(RolloutStageType<PlantTerrainStage>{});
    case 1: return f(RolloutStageType<PlantTerrainActStage>{});
    case 2: return f(RolloutStageType<PlantVaried<PlantTerrainStage>>{});
    default: return f(RolloutStageType<PlantVaried<PlantTerrainActStage>>{});
  }
  switch ((v.varied ? 4 : 0) | (v.actuated ? 2 : 0) | (v.ground ? 1 : 0)) {
    case 0: return f(RolloutStageType<PlantStage>{});
    case 1: return f(RolloutStageType<PlantContactStage>{});
    case 2: return f(RolloutStageType<PlantActStage>{});
    case 3: return f(RolloutStageType<PlantContactActStage>{});
    case 4: return f(RolloutStageType<PlantVaried<PlantStage>>{});
    case 5: return f(RolloutStageType<PlantVaried<PlantContactStage>>{});
    case 6: return f(RolloutStageType<PlantVaried<PlantActStage>>{});
    default: return f(RolloutStageType<PlantVaried<PlantContactActStage>>{});
  }
}

}  // namespace hsqp
