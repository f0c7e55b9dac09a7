// Velocity-command targets of the CENTROIDAL formulation on the device (include/hsqp_cent_loop.h): the TargetTrajectories the reference's
// CentroidalMpcSqpNode rebuilds in every MPC cycle,
//   CentroidalMpcTargetTrajectoriesCalculator::commandedVelocityToTargetTrajectories
//   (humanoid_centroidal_mpc/src/command/CentroidalMpcTargetTrajectoriesCalculator.cpp:88-158)
// restated as reference.centroidal_velocity_command_targets restates it on the host.  The whole-body generator (hsqp_loop.h) reads the base
// velocity from the state row; a centroidal state row carries the normalised momentum instead, so the generator first needs
//   vb = A_b(q)^-1 (momentum)      at the measured state, joint rates zero ("assumes no joint velocities"), wrenches zero:
// the model pass of the centroidal LQ kernel (cent_ws_topology, cent_stage_values: the tree walk across the lanes) and its closing 3 x 3
// solve (cent_lane_flow -> cent_finish) on one lane — what cent_params_torso and cent_base_velocity run — and then the knots, three lanes.
//
// The command filter and the pose integration ARE hsqp_loop.h's (command_filter, command_integrate_pose).
//
// Arithmetic: every product-sum of this file is evaluated unfused (`#pragma clang fp contract(off)`), the model pass as the LQ kernel
// evaluates it.  The same source compiles for the host with a one-lane Ctx (tests/cent_loop/cent_loop_emu.cpp).
#pragma once
#include "hsqp_cent_lq.h"
#include "hsqp_loop.h"

namespace hsqp {

// [pdot; euler rates] of the base at the measured centroidal state row x0 (q = x0[6 .. 34], joint rates and wrenches zero) into ws.kv[0][0 .. 5].
//
// THE MASS FACTOR.  x0[0 .. 5] is the NORMALISED momentum h; the solve runs on the momentum m h: cent_finish forms `h[3 + r] * M - angJ[r]`
// and `h[r] - lin / M` (csrc/hsqp_cent.h), the only place of this generator where the total mass meets h — as reference.centroidal_base_velocity
// evaluates A_b^-1 (m h).  The reference's source multiplies A_b^-1 by initState.head(6) without a mass factor; whether its A is the normalised
// matrix cannot be settled from the sources at hand (DESIGN.md, next to assumptions A7 / A9).  To take that other reading, scale ws.x[0 .. 5]
// by 1 / dm.total_mass HERE, in front of cent_stage_values, and nowhere else.
template <class W>
HSQP_HD void cent_command_base_velocity(const Ctx& ctx, const DevModel& dm, W& ws, const double* x0) {
  cent_ws_topology(ctx, dm, ws);
  WG_FOR(ctx, i, CNX + NU) { if (i < CNX) ws.x[i] = x0[i]; else ws.u[i - CNX] = 0.0; }
  WG_SYNC(ctx);
  cent_stage_values(ctx, dm, ws, 0, 0.0);
  WG_FOR(ctx, it, 1) {
    CentBase<double> base;
    double xdot[12];
    cent_lane_flow<double>(dm, ws, CentCol{CK_NONE, 0}, xdot, base);
    for (int k = 0; k < 6; ++k) ws.kv[0][k] = base.vb[k];   // (stage 0 reads no kv row: the row is free)
  }
  WG_SYNC(ctx);
}

// Knot `knot` (0, 1, 2) of one instance from the FILTERED command v = {vx, vy, height, yaw rate} and the base velocity vb [6]: its time and its
// state row [NX] = [gvx, gvy, 0, 0, 0, wz / m | pose | default joint state | zeros].  vb[5] — the euler X rate — is read as the yaw rate, as
// the reference reads it.
HSQP_HD void cent_command_target_knot(const double* v, const double* x0, const double* vb, const double* jt, double mass, double t0, double horizon, int knot,
                                      double* time, double* state) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double vx = v[0], vy = v[1], height = v[2], wz = v[3];
  const double yaw = x0[9];
  const double c = cos(yaw), s = sin(yaw);
  const double gvx = c * vx - s * vy, gvy = s * vx + c * vy;
  const double t_mid = 0.7 * horizon;
  double pose[6] = {x0[6], x0[7], height, x0[9], 0.0, 0.0}, mid[6], fin[6];
  const double* p = pose;
  *time = t0;
  if (knot >= 1) {
    command_integrate_pose(pose, (vb[0] + gvx) / 2, (vb[1] + gvy) / 2, (vb[5] + wz) / 2, height, t_mid, mid);
    p = mid;
    *time = t0 + t_mid;
  }
  if (knot >= 2) {
    command_integrate_pose(mid, gvx, gvy, wz, height, horizon - t_mid, fin);
    p = fin;
    *time = t0 + horizon;
  }
  state[0] = gvx; state[1] = gvy; state[2] = 0.0; state[3] = 0.0; state[4] = 0.0; state[5] = wz / mass;
  for (int i = 0; i < 6; ++i) state[6 + i] = p[i];
  for (int i = 0; i < NJ; ++i) state[12 + i] = jt[i];
  for (int i = CNX; i < NX; ++i) state[i] = 0.0;
}

// One instance (one wave on the device): v_cmd [4], v_filt [4] in / out (in place), x0 [NX], tt [3], ts [3][NX], base_vel [6] or null.
// Every lane filters the command into registers before anything is written; the lane of knot 0 stores the new filter state (and base_vel).
template <class W>
HSQP_HD void cent_command_targets_instance(const Ctx& ctx, const DevModel& dm, W& ws, double alpha, const double* v_cmd, double* v_filt, const double* x0, double t0,
                                           double horizon, double* tt, double* ts, double* base_vel) {
  double v[CMD_N];
  for (int i = 0; i < CMD_N; ++i) v[i] = v_filt[i];
  command_filter(alpha, v_cmd, v);
  cent_command_base_velocity(ctx, dm, ws, x0);   // (its barriers stand between the read above and the store below)
  WG_FOR(ctx, knot, CMD_KNOTS) {
    cent_command_target_knot(v, x0, ws.kv[0], dm.default_joint_state, dm.total_mass, t0, horizon, knot, tt + knot, ts + (size_t)knot * NX);
    if (knot == 0) {
      for (int i = 0; i < CMD_N; ++i) v_filt[i] = v[i];
      if (base_vel) for (int i = 0; i < 6; ++i) base_vel[i] = ws.kv[0][i];
    }
  }
}

}  // namespace hsqp
