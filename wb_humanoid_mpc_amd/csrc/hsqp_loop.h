// Velocity-command targets on the device (include/hsqp_loop.h): the TargetTrajectories the reference rebuilds in every MPC cycle from the
// measured state and the filtered velocity command,
//   ProceduralMpcMotionManager::preSolverRun -> WBMpcTargetTrajectoriesCalculator::commandedVelocityToTargetTrajectories
//   TargetTrajectoriesCalculatorBase::filterAndTransformVelCommandToLocal (the first-order command filter, alpha = 0.8 in the reference)
// restated as reference.velocity_command_targets restates it on the host: the filtered command rotated by the measured yaw, roll and pitch
// zeroed, three knots at t0, t0 + 0.7 horizon, t0 + horizon, the mid knot integrated with the mean of the measured and the commanded base
// velocity, the joints at the model's default joint state, the target velocity in the velocity block.
//
// The reference keeps ONE filter state (a function-local static); here every instance owns its own (v_filt [B][4], in / out).
// filter_alpha == 0 takes the command itself, whatever v_filt held ("filter at steady state", the host mirror's default).
//
// Arithmetic: every product-sum is evaluated unfused (`#pragma clang fp contract(off)`; hipcc contracts device code by default), so the
// device differs from the host mirror only by its sin / cos.  The same source compiles for the host with a one-lane loop
// (tests/loop/loop_emu.cpp, -ffp-contract=off).
#pragma once
#include "hsqp_common.h"

namespace hsqp {

constexpr int CMD_N = 4;        // WalkingVelocityCommand::toVector: vx, vy, height, yaw rate
constexpr int CMD_KNOTS = 3;

// v_filt <- alpha v_filt + (1 - alpha) v_cmd
HSQP_HD void command_filter(double alpha, const double* v_cmd, double* v_filt) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  for (int i = 0; i < CMD_N; ++i) v_filt[i] = alpha == 0.0 ? v_cmd[i] : alpha * v_filt[i] + (1.0 - alpha) * v_cmd[i];
}

// integrateTargetBasePose: planar position and yaw advanced by v3 = {vx, vy, yaw rate} over dt, the height set, roll and pitch zero
HSQP_HD void command_integrate_pose(const double* p, double v0, double v1, double v2, double height, double dt, double* q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  q[0] = p[0] + v0 * dt;
  q[1] = p[1] + v1 * dt;
  q[2] = height;
  q[3] = p[3] + v2 * dt;
  q[4] = q[5] = 0.0;
}

// Knot `knot` (0, 1, 2) of one instance from the FILTERED command v = {vx, vy, height, yaw rate}: its time and its state row [NX].
// jt: the model's default joint state [NJ].
HSQP_HD void command_target_knot(const double* v, const double* x0, const double* jt, double t0, double horizon, int knot, double* time, double* state) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double vx = v[0], vy = v[1], height = v[2], wz = v[3];
  const double yaw = x0[3];
  const double c = cos(yaw), s = sin(yaw);
  const double gvx = c * vx - s * vy, gvy = s * vx + c * vy;
  const double* base_vel = x0 + 6 + NJ;
  const double t_mid = 0.7 * horizon;
  double pose[6] = {x0[0], x0[1], height, x0[3], 0.0, 0.0}, mid[6], fin[6];
  const double* p = pose;
  *time = t0;
  if (knot >= 1) {
    command_integrate_pose(pose, (base_vel[0] + gvx) / 2, (base_vel[1] + gvy) / 2, (base_vel[5] + wz) / 2, height, t_mid, mid);
    p = mid;
    *time = t0 + t_mid;
  }
  if (knot >= 2) {
    command_integrate_pose(mid, gvx, gvy, wz, height, horizon - t_mid, fin);
    p = fin;
    *time = t0 + horizon;
  }
  for (int i = 0; i < 6; ++i) state[i] = p[i];
  for (int i = 0; i < NJ; ++i) state[6 + i] = jt[i];
  state[6 + NJ + 0] = gvx; state[6 + NJ + 1] = gvy; state[6 + NJ + 2] = 0.0;
  state[6 + NJ + 3] = wz;  state[6 + NJ + 4] = 0.0; state[6 + NJ + 5] = 0.0;
  for (int i = 0; i < NJ; ++i) state[12 + NJ + i] = 0.0;
}

// Item id = instance * 3 + knot of a batch, in place on v_filt: every item filters its instance's command into registers; between `load` and
// `store` the caller puts a barrier that covers the three items of an instance (the kernel: workgroups of a multiple of three items; the host:
// the three items of an instance in one call each, load before store), and the item of knot 0 stores the new filter state.
struct CommandItem { double v[CMD_N]; };
HSQP_HD CommandItem command_item_load(double alpha, const double* v_cmd, const double* v_filt, int id) {
  const int b = id / CMD_KNOTS;
  CommandItem it;
  for (int i = 0; i < CMD_N; ++i) it.v[i] = v_filt[(size_t)b * CMD_N + i];
  command_filter(alpha, v_cmd + (size_t)b * CMD_N, it.v);
  return it;
}
HSQP_HD void command_item_store(const CommandItem& it, const double* jt, const double* x0, double t0, double horizon, int id, double* v_filt,
                                double* target_times, double* target_states) {
  const int b = id / CMD_KNOTS, knot = id % CMD_KNOTS;
  command_target_knot(it.v, x0 + (size_t)b * NX, jt, t0, horizon, knot, target_times + id, target_states + (size_t)id * NX);
  if (knot == 0)
    for (int i = 0; i < CMD_N; ++i) v_filt[(size_t)b * CMD_N + i] = it.v[i];
}

}  // namespace hsqp
