// Per-foot swing heights read from the height map (include/hsqp_perceive.h): for every instance and foot the lift-off and touch-down height of every
// phase of the mode schedule, the sequences the reference's three-argument SwingTrajectoryPlanner::update takes
//   humanoid_common_mpc/src/swing_foot_planner/SwingTrajectoryPlanner.cpp:101-191   (restated in csrc/hsqp_params.h, node_params_eval)
// The RULE that fills them is OURS — the reference has no perception, its two-argument update fills the sequences with one constant: a contact run
// that has begun stands where the foot is, a run ahead lands where the target trajectory carries the nominal foothold at its touch-down time, and the
// run's height is the resident height map (include/hsqp_terrain.h, steps 1-8) under that point.
//
// Shape: one lane per (instance, foot).  A lane walks the forward kinematics of ITS leg (rows 0 and 1 of every rotation on the path: the world xy of the
// contact frame), then the phases of its schedule serially, at most max_events + 1 of them, forwards and backwards, with one map sample per contact run
// (and one under the foot itself where the schedule begins in the air).  A lane owns its rows: no exchange, no atomics, no barrier.
// Bounds: n_events is clamped into [0, max_events] and n_knots' look-up into the knots before either bounds a loop or forms an index (the arrays of the
// _device entry are not read back); the leg walk is bounded by NANC; every map index comes from terrain_height, which clamps in double first.
//
// Arithmetic: every product-sum is evaluated unfused (`#pragma clang fp contract(off)`; hipcc contracts device code by default), so the device differs
// from the host build of this source (tests/perceive/perceive_emu.cpp, -ffp-contract=off) only by its sin / cos.  The map sample is terrain_height
// itself, the function hsqp_terrain_eval runs: a height is that entry point's answer at the returned foothold.
#pragma once
#include "hsqp_common.h"
#include "hsqp_contact.h"
#include "hsqp_model.h"
#include "hsqp_params.h"
#include "hsqp_terrain.h"
#include "../../include/hsqp_perceive.h"

namespace hsqp {

// World xy of contact frame f: the walk base -> ancestors of contact_body[f] -> the frame, rows 0 and 1 only.  pose = {X, Y, Z, yaw, pitch, roll}
// (Z is not read), qj [NJ] the joint angles (body i turns by qj[i - 1]).
HSQP_HD void perceive_foot_xy(const DevModel& dm, const double* pose, const double* qj, int f, double* xy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int body = dm.contact_body[f];
  const double cz = cos(pose[3]), sz = sin(pose[3]), cy = cos(pose[4]), sy = sin(pose[4]), cx = cos(pose[5]), sx = sin(pose[5]);
  double r0[3] = {cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx};   // rows 0 and 1 of Rz Ry Rx
  double r1[3] = {sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx};
  double X = pose[0], Y = pose[1];
  const int na = dm.n_anc[body];
  for (int n = 0; n < NANC && n < na; ++n) {
    const int i = dm.anc[body][n];
    double Rq[9], M[9];
    rot_axis_cs(dm.axis[i], cos(qj[i - 1]), sin(qj[i - 1]), Rq);
    m3_mul(dm.Rfix[i], Rq, M);
    X = X + (r0[0] * dm.pfix[i][0] + r0[1] * dm.pfix[i][1] + r0[2] * dm.pfix[i][2]);
    Y = Y + (r1[0] * dm.pfix[i][0] + r1[1] * dm.pfix[i][1] + r1[2] * dm.pfix[i][2]);
    const double a0 = r0[0] * M[0] + r0[1] * M[3] + r0[2] * M[6], a1 = r0[0] * M[1] + r0[1] * M[4] + r0[2] * M[7], a2 = r0[0] * M[2] + r0[1] * M[5] + r0[2] * M[8];
    const double b0 = r1[0] * M[0] + r1[1] * M[3] + r1[2] * M[6], b1 = r1[0] * M[1] + r1[1] * M[4] + r1[2] * M[7], b2 = r1[0] * M[2] + r1[1] * M[5] + r1[2] * M[8];
    r0[0] = a0; r0[1] = a1; r0[2] = a2;
    r1[0] = b0; r1[1] = b1; r1[2] = b2;
  }
  xy[0] = X + (r0[0] * dm.contact_p[f][0] + r0[1] * dm.contact_p[f][1] + r0[2] * dm.contact_p[f][2]);
  xy[1] = Y + (r1[0] * dm.contact_p[f][0] + r1[1] * dm.contact_p[f][1] + r1[2] * dm.contact_p[f][2]);
}

// Entries 0, 1 and 3 (X, Y, yaw) of the clamped piece-wise linear interpolation of the target knots at t: the desired-state rule of node_params_eval,
// the same expression order.
HSQP_HD void perceive_target_pose(int n_knots, const double* tt, const double* ts /*[n_knots][NX]*/, double t, double* Xd, double* Yd, double* psi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (t <= tt[0] || n_knots < 2) { *Xd = ts[0]; *Yd = ts[1]; *psi = ts[3]; return; }
  const double* last = ts + (size_t)(n_knots - 1) * NX;
  if (t >= tt[n_knots - 1]) { *Xd = last[0]; *Yd = last[1]; *psi = last[3]; return; }
  int i0 = 0;
  while (i0 + 2 < n_knots && tt[i0 + 1] <= t) ++i0;   // (i0 + 1 stays a knot whatever the times hold: a NaN among them ends in the clamp above or here)
  const double a = (tt[i0 + 1] - t) / (tt[i0 + 1] - tt[i0]);
  const double* s0 = ts + (size_t)i0 * NX;
  const double* s1 = s0 + NX;
  *Xd = a * s0[0] + (1.0 - a) * s1[0];
  *Yd = a * s0[1] + (1.0 - a) * s1[1];
  *psi = a * s0[3] + (1.0 - a) * s1[3];
}

// the ground of one instance under (X, Y): steps 1-8 of include/hsqp_terrain.h, what hsqp_terrain_eval answers
HSQP_HD double perceive_ground(const TerrainSet& ter, double ground_height, double X, double Y) {
  double hm, n[3];
  terrain_height(ter, X, Y, &hm, n);
  return ground_height + hm;
}

// The rows of one (instance, foot): lift [E + 1], touch [E + 1], fxy [E + 1][2] (all three given).  x [NX] the state the MPC reads, t the problem time,
// (n_ev, ev [E], seq [E + 1]) the schedule, (n_knots, tt, ts) the targets, offset = touch_down_height_offset.  Entries of phases past n_ev are written 0.
HSQP_HD void perceive_foot_rows(const DevModel& dm, const TerrainSet& ter, double ground_height, const double* x, double t, int E, int n_ev, const double* ev,
                                const int* seq, int n_knots, const double* tt, const double* ts, double offset, int f, double* lift, double* touch, double* fxy) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  n_ev = n_ev < 0 ? 0 : (n_ev > E ? E : n_ev);
  const int n = n_ev + 1;   // phases
  for (int p = n; p <= E; ++p) { lift[p] = 0.0; touch[p] = 0.0; fxy[2 * p] = 0.0; fxy[2 * p + 1] = 0.0; }
  bool finite = true;
  for (int i = 0; i < NX; ++i) finite = finite && (x[i] - x[i] == 0.0);
  if (!finite) {   // the instance fails alone through the status path of the iteration: its rows are NaN, no map is read
    const double nan = __builtin_nan("");
    for (int p = 0; p < n; ++p) { lift[p] = nan; touch[p] = nan; fxy[2 * p] = nan; fxy[2 * p + 1] = nan; }
    return;
  }
  double P[2], o[2];
  perceive_foot_xy(dm, x, x + 6, f, P);
  const double zero[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  perceive_foot_xy(dm, zero, dm.default_joint_state, f, o);
  const int p_now = ev_lower(ev, n_ev, t);
  // forwards: the contact runs (foothold, height) and every swing phase's lift-off from the run before it
  double h_prev = 0.0, F[2] = {P[0], P[1]};
  if (!mode_contact(seq[0], f)) h_prev = perceive_ground(ter, ground_height, P[0], P[1]);   // no run before the leading swing phases: the ground under the foot
  for (int p = 0; p < n; ++p) {
    if (mode_contact(seq[p], f)) {
      if (p == 0 || !mode_contact(seq[p - 1], f)) {   // phase a = p begins a run
        if (p <= p_now) { F[0] = P[0]; F[1] = P[1]; }
        else {
          double Xd, Yd, psi;
          perceive_target_pose(n_knots, tt, ts, ev[p - 1], &Xd, &Yd, &psi);
          const double c = cos(psi), s = sin(psi);
          F[0] = Xd + c * o[0] - s * o[1];
          F[1] = Yd + s * o[0] + c * o[1];
        }
        h_prev = perceive_ground(ter, ground_height, F[0], F[1]);
      }
      lift[p] = h_prev; touch[p] = h_prev + offset;
      fxy[2 * p] = F[0]; fxy[2 * p + 1] = F[1];
    } else {
      lift[p] = h_prev;   // (the run before it, or the ground under the foot)
    }
  }
  // backwards: every swing phase's touch-down and foothold from the run behind it
  bool have_next = false;
  double h_next = 0.0, Fn[2] = {P[0], P[1]};
  for (int p = n - 1; p >= 0; --p) {
    if (mode_contact(seq[p], f)) { have_next = true; h_next = lift[p]; Fn[0] = fxy[2 * p]; Fn[1] = fxy[2 * p + 1]; }
    else {
      touch[p] = have_next ? h_next + offset : lift[p] + offset;
      fxy[2 * p] = Fn[0]; fxy[2 * p + 1] = Fn[1];
    }
  }
}

// what k_foot_heights hands over besides the model, the contact ground and the terrain; every array is the batch's
struct PerceiveArgs {
  int B, E, K;                   // instances, max_events, n_knots
  double t, offset;              // the problem time; hsqp_swing_config::touch_down_height_offset
  const double* x;               // [B][NX]
  const int* ne; const double* ev; const int* seq;   // [B], [B][E], [B][E + 1]
  const double* tt; const double* ts;                // [B][K], [B][K][NX]
  double* lift; double* touch;   // [B][2][E + 1]
  double* fxy;                   // [B][2][E + 1][2]
};

// lane (instance b, foot f), b < a.B
HSQP_HD void perceive_lane(const DevModel& dm, const ContactParams& cp, const TerrainParams& tp, const PerceiveArgs& a, int b, int f) {
  TerrainSet ter;
  terrain_load_lane(tp, b, ter);
  const size_t row = ((size_t)b * 2 + f) * (size_t)(a.E + 1);
  perceive_foot_rows(dm, ter, cp.ground[b].height, a.x + (size_t)b * NX, a.t, a.E, a.ne[b], a.ev + (size_t)b * a.E, a.seq + (size_t)b * (a.E + 1), a.K,
                     a.tt + (size_t)b * a.K, a.ts + (size_t)b * a.K * NX, a.offset, f, a.lift + row, a.touch + row, a.fxy + 2 * row);
}

}  // namespace hsqp
