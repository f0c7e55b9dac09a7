// TEST INFRASTRUCTURE: the host build of the ground contact of the torque plant (wb_humanoid_mpc_amd/csrc/hsqp_contact.h, hsqp_plant.h, hsqp_rollout.h,
// k_rollout_plant, k_contact_eval) with a one-lane context, for tests/test_contact.py (compiled by the test with -ffp-contract=off, also with
// -DHSQP_EMU_REVERSE).  A shared library loaded through ctypes: the shared entries of tests/rollout/rollout_emu.h (the rollout itself), and the point-wise
// ones below.  cs: the contact setting (null or enabled = 0: no contact), ground: the per-instance table [1] (null: the setting's values).
//   cte_eval(h, cs, ground [1] or null, x [58], force [8][3], pen [8]): hsqp_contact_eval for one instance
//   cte_accel(h, cs, ground [1] or null, x [58], W [12], tau [23], armature [23], n_push, pushes, vd [29]): forward dynamics at the state x under the
//              joint torques tau, every given push and — contact on — the contact forces, else the contact wrenches W
#include "../rollout/rollout_emu.h"

using WS = RolloutWS<PlantContactStage>;   // the instantiation on the ground

// the kernels' view of the setting: the ground of B instances in `store`
static ContactParams params_of(const hsqp_contact_settings* cs, const hsqp_contact_ground* ground, int B, std::vector<hsqp_contact_ground>& store) {
  if (!cs || !cs->enabled) return ContactParams{nullptr, 0.0, 0.0, 0.0};
  store.resize(B);
  contact_fill_ground(*cs, ground, B, B, store.data());
  return ContactParams{store.data(), cs->stiffness, cs->damping, cs->slip_velocity};
}

extern "C" {

void cte_eval(void* h, const hsqp_contact_settings* cs, const hsqp_contact_ground* ground, const double* x, double* force, double* pen) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  auto w = fresh<ContactEvalWS>();
  std::vector<hsqp_contact_ground> store;
  hsqp_contact_settings on = *cs;
  on.enabled = 1;   // (hsqp_contact_eval evaluates the model whatever `enabled` is)
  contact_eval_instance(Ctx{0, 1, nullptr}, dm, *w, params_of(&on, ground, 1, store), 0, x, force, pen);
}

void cte_accel(void* h, const hsqp_contact_settings* cs, const hsqp_contact_ground* ground, const double* x, const double* W, const double* tau,
               const double* armature, int n_push, const hsqp_push* pushes, double* vd) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  auto w = fresh<WS>();
  const Ctx ctx{0, 1, nullptr};
  std::vector<hsqp_contact_ground> store;
  const ContactParams cp = params_of(cs, ground, 1, store);   // (contact off: the same workspace, the set unused — plant_forward_dynamics with no ground)
  const unsigned mask = load_pushes(ctx, n_push, pushes, w->push);
  rollout_topology(ctx, dm, w->sw);
  double u[NU] = {0.0};
  for (int i = 0; i < 12; ++i) u[i] = W[i];
  for (int j = 0; j < NJ; ++j) { w->sw.pl.tau[j] = tau[j]; w->sw.pl.arm[j] = armature[j]; }
  if (cp.ground) contact_load(ctx, cp, 0, w->sw.ct);
  plant_inputs(ctx, w->sw.st, x, u, true);
  stage_eval<false>(ctx, dm, w->sw.st);
  plant_forward_dynamics(ctx, dm, w->sw.st, w->sw.pl, w->push, mask, cp.ground ? &w->sw.ct : nullptr);
  for (int i = 0; i < NV; ++i) vd[i] = w->sw.pl.vd[i];
}

}  // extern "C"
