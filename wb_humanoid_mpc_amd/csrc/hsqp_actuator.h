// Actuator model on the torque plant of the rollout (include/hsqp_actuator.h): the resident setting as the kernel sees it, one instance's
// parameters and held joint command in the rollout workspace, the joint law with effort limits and passive torques, and the tick schedule.
//   actuator_load    instance b of the setting into the workspace (the actuator instantiations of the rollout kernel only: the handle launches
//                    them while the model is active, so the plant's own instantiations carry none of this)
//   actuator_law     tau_cmd = tau_ff + kp (q_p - q) + kd (v_p - v) from the command in the workspace and the plant's CURRENT (q, v), the clamp,
//                    the passive torques; tau = tau_act + tau_pas.  The expression of tau_cmd is the one of the plant's joint law, and the clamp is
//                    written with comparisons, so a NaN command stays NaN and a neutral setting leaves every bit of tau as it was.
//   actuator_tick    where a time t stands in the schedule T_k = s0 + k period: whether it is a tick, and the first tick after it
// The sampling of a command and the evaluation that uses it are in hsqp_rollout.h (they need the controller and the plant).
// Everything is uniform across the workgroup; the same source builds for the host with a one-lane context (tests/actuator/actuator_emu.cpp).
#pragma once
#include "hsqp_common.h"
#include "../../include/hsqp_actuator.h"

namespace hsqp {

// The resident setting, as the kernels that have an actuator model see it
struct ActuatorParams {
  const double* table;    // effort_limit | damping | friction, [NJ] each
  double period, vs;      // command_period, friction_velocity
  double* last;           // [B][3][NJ] the record of hsqp_actuator_last: tau_cmd | tau_act | tau_pas of every instance
};
// (host) the public setting as ActuatorParams::table reads it: t [3 NJ]
inline void actuator_pack_table(const hsqp_actuator_settings& s, double* t) {
  for (int j = 0; j < NJ; ++j) { t[j] = s.effort_limit[j]; t[NJ + j] = s.damping[j]; t[2 * NJ + j] = s.friction[j]; }
}

// ONE instance's setting and the joint command in force
struct ActuatorWS {
  double period, vs;
  double* rec;                          // the instance's record [3][NJ]
  double limit[NJ], damp[NJ], fric[NJ];
  double qp[NJ], vp[NJ], tff[NJ];       // the command: joint set-points and feed-forward effort
  double Wp[12];                        // the policy's contact wrenches that go with it (the plant without a ground applies them)
};

// instance b of the setting into the workspace.  Ends with a barrier.
HSQP_HD void actuator_load(const Ctx& ctx, const ActuatorParams& ap, int b, ActuatorWS& ac) {
  WG_FOR(ctx, i, 3 * NJ + 1) {
    if (i == 3 * NJ) { ac.period = ap.period; ac.vs = ap.vs; ac.rec = ap.last + (size_t)b * 3 * NJ; continue; }
    (i < NJ ? ac.limit[i] : (i < 2 * NJ ? ac.damp[i - NJ] : ac.fric[i - 2 * NJ])) = ap.table[i];
  }
  WG_SYNC(ctx);
}

// tau [NJ] of the command in force at the plant state x; rec (null: none): tau_cmd | tau_act | tau_pas [NJ] each.  One item per joint; no barrier.
HSQP_HD void actuator_law(const Ctx& ctx, const ActuatorWS& ac, const double* kp, const double* kd, const double* x, double* tau, double* rec) {
  WG_FOR(ctx, j, NJ) {
    const double v = x[NV + 6 + j], lim = ac.limit[j];
    const double cmd = (ac.tff[j] + kp[j] * (ac.qp[j] - x[6 + j])) + kd[j] * (ac.vp[j] - v);
    const double act = cmd > lim ? lim : (cmd < -lim ? -lim : cmd);
    const double pas = -ac.damp[j] * v - ac.fric[j] * v / sqrt(v * v + ac.vs * ac.vs);
    tau[j] = act + pas;
    if (rec) { rec[j] = cmd; rec[NJ + j] = act; rec[2 * NJ + j] = pas; }
  }
}

// t >= s0 in the schedule T_k = s0 + k period (period > 0): on — t is a tick; next — the first tick after t.  Every tick is formed by the one
// product and sum (never contracted, never accumulated), so a time that was taken from `next` is found `on`.  A period too small to advance the
// time gives a `next` that is not after t, or not finite: the caller ends the instance.
struct ActuatorTick { bool on; double next; };
HSQP_HD ActuatorTick actuator_tick(double s0, double period, double t) {
#pragma clang fp contract(off)
  double k = floor((t - s0) / period);
  if (s0 + k * period > t) k -= 1.0;                       // (the quotient's rounding puts k at most one off)
  else if (s0 + (k + 1.0) * period <= t) k += 1.0;
  return ActuatorTick{s0 + k * period == t, s0 + (k + 1.0) * period};
}

}  // namespace hsqp
