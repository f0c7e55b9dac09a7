// TEST INFRASTRUCTURE: the host build of the per-instance inertial variations of the torque plant (wb_humanoid_mpc_amd/csrc/hsqp_inertia.h, hsqp_plant.h,
// hsqp_rollout.h, k_rollout_plant, k_inertia_eval) with a one-lane context, for tests/test_inertia.py (compiled by the test with -ffp-contract=off, also
// with -DHSQP_EMU_REVERSE).  A shared library loaded through ctypes: the shared entries of tests/rollout/rollout_emu.h (the rollout itself), and the
// point-wise ones below.  table: the instance's entry (null: no table).
//   ine_eval(h, table [1] or null, x [58], M [29][29], nle [29], mass [1]): hsqp_inertia_eval for one instance
//   ine_accel(h, table [1] or null, cs, x [58], W [12], tau [23], armature [23], n_push, pushes, vd [29]): forward dynamics at the state x under the joint
//              torques tau, every given push and — cs non-null and enabled: on the ground — the contact forces, else the contact wrenches W
//   ine_eval_ws_bytes(): sizeof of hsqp_inertia_eval's workspace
#include "../rollout/rollout_emu.h"

using WSC = RolloutWS<PlantVaried<PlantContactStage>>;  // the varied plant on the ground

extern "C" {

void ine_eval(void* h, const hsqp_inertia_instance* table, const double* x, double* M, double* nle, double* mass) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  auto w = fresh<InertiaEvalWS>();
  inertia_eval_instance(Ctx{0, 1, nullptr}, dm, *w, InertiaParams{table}, 0, x, M, nle, mass);
}

void ine_accel(void* h, const hsqp_inertia_instance* table, const hsqp_contact_settings* cs, const double* x, const double* W, const double* tau,
               const double* armature, int n_push, const hsqp_push* pushes, double* vd) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  auto w = fresh<WSC>();
  const Ctx ctx{0, 1, nullptr};
  const bool ground = cs && cs->enabled;
  const hsqp_contact_ground g{ground ? cs->ground_height : 0.0, ground ? cs->mu : 0.0};
  const unsigned mask = load_pushes(ctx, n_push, pushes, w->push);
  rollout_topology(ctx, dm, w->sw);
  double u[NU] = {0.0};
  for (int i = 0; i < 12; ++i) u[i] = W[i];
  for (int j = 0; j < NJ; ++j) { w->sw.pl.tau[j] = tau[j]; w->sw.pl.arm[j] = armature[j]; }
  if (ground) contact_load(ctx, ContactParams{&g, cs->stiffness, cs->damping, cs->slip_velocity}, 0, w->sw.ct);
  if (table) inertia_load(ctx, InertiaParams{table}, 0, w->sw.iw);
  plant_inputs(ctx, w->sw.st, x, u, true);
  stage_eval<false>(ctx, dm, w->sw.st);
  if (table) inertia_apply(ctx, w->sw.st, w->sw.iw);
  plant_forward_dynamics(ctx, dm, w->sw.st, w->sw.pl, w->push, mask, ground ? &w->sw.ct : nullptr);
  for (int i = 0; i < NV; ++i) vd[i] = w->sw.pl.vd[i];
}

int ine_eval_ws_bytes() { return (int)sizeof(InertiaEvalWS); }

}  // extern "C"
