// TEST INFRASTRUCTURE: the host build of the actuator model on the torque plant of the rollout (wb_humanoid_mpc_amd/csrc/hsqp_actuator.h, hsqp_rollout.h,
// k_rollout_plant) with a one-lane context, for tests/test_actuator.py (compiled by the test with -ffp-contract=off, also
// with -DHSQP_EMU_REVERSE) and tests/actuator/actuator_sanitize.cpp.  A shared library loaded through ctypes: the shared entries of
// tests/rollout/rollout_emu.h (the rollout itself), and
//   ace_law(as, kp [23], kd [23], qp [23], vp [23], tff [23], x [58], out [4][23]): the joint law at the plant state x under the given command:
//           tau | tau_cmd | tau_act | tau_pas
//   ace_tick(s0, period, t, on, next): where t stands in the tick schedule
#include "../rollout/rollout_emu.h"

extern "C" {

void ace_law(const hsqp_actuator_settings* as, const double* kp, const double* kd, const double* qp, const double* vp, const double* tff, const double* x,
             double* out) {
  auto ac = fresh<ActuatorWS>();
  const Ctx ctx{0, 1, nullptr};
  double t[3 * NJ], rec[3 * NJ];
  actuator_pack_table(*as, t);
  actuator_load(ctx, ActuatorParams{t, as->command_period, as->friction_velocity, rec}, 0, *ac);
  for (int j = 0; j < NJ; ++j) { ac->qp[j] = qp[j]; ac->vp[j] = vp[j]; ac->tff[j] = tff[j]; }
  actuator_law(ctx, *ac, kp, kd, x, out, ac->rec);
  for (int i = 0; i < 3 * NJ; ++i) out[NJ + i] = rec[i];
}

void ace_tick(double s0, double period, double t, int* on, double* next) {
  const ActuatorTick tk = actuator_tick(s0, period, t);
  *on = tk.on ? 1 : 0;
  *next = tk.next;
}

}  // extern "C"
