// TEST INFRASTRUCTURE: the host build of the torque plant of the rollout (wb_humanoid_mpc_amd/csrc/hsqp_plant.h, hsqp_rollout.h, k_rollout_plant)
// with a one-lane context, for tests/test_plant.py (compiled by the test with -ffp-contract=off, also with -DHSQP_EMU_REVERSE).  A shared library
// loaded through ctypes: the shared entries of tests/rollout/rollout_emu.h (the rollout itself), and
//   ple_accel(h, x [58], W [12], tau [23], armature [23], n_push, pushes [n_push], vd [29]): forward dynamics at the state x under the joint torques
//              tau, the contact wrenches W and every given push
//   ple_tau(h, x [58], u [35], tau [23]): the feed-forward torques (policy_node)
//   ple_eval(h, plant, controller, N, dts [N] or null, dt, xt [N + 1][58], ut [N][35], K [count][35][58], uff [count][35], first, count, s, x [58],
//            n_push, pushes, k [58]): one evaluation of the closed loop on the torque plant
#include "../rollout/rollout_emu.h"

using WS = RolloutWS<PlantStage>;

extern "C" {

void ple_accel(void* h, const double* x, const double* W, const double* tau, const double* armature, int n_push, const hsqp_push* pushes, double* vd) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  auto w = fresh<WS>();
  const Ctx ctx{0, 1, nullptr};
  const unsigned mask = load_pushes(ctx, n_push, pushes, w->push);
  rollout_topology(ctx, dm, w->sw);
  double u[NU] = {0.0};
  for (int i = 0; i < 12; ++i) u[i] = W[i];
  for (int j = 0; j < NJ; ++j) { w->sw.pl.tau[j] = tau[j]; w->sw.pl.arm[j] = armature[j]; }
  plant_inputs(ctx, w->sw.st, x, u, true);
  stage_eval<false>(ctx, dm, w->sw.st);
  plant_forward_dynamics(ctx, dm, w->sw.st, w->sw.pl, w->push, mask);
  for (int i = 0; i < NV; ++i) vd[i] = w->sw.pl.vd[i];
}

void ple_tau(void* h, const double* x, const double* u, double* tau) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  auto w = fresh<WS>();
  policy_node(Ctx{0, 1, nullptr}, dm, w->sw.st, x, u, tau);
}

void ple_eval(void* h, const hsqp_plant_settings* ps, int controller, int N, const double* dts, double dt, const double* xt, const double* ut, const double* K,
              const double* uff, int first, int count, double s, const double* x, int n_push, const hsqp_push* pushes, double* k) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  auto w = fresh<WS>();
  const Ctx ctx{0, 1, nullptr};
  double g[3 * NJ];
  plant_pack_gains(*ps, g);
  plant_load(ctx, PlantParams{g, ps->lookahead, xt}, 0, N, w->sw.pl);
  const unsigned mask = load_pushes(ctx, n_push, pushes, w->push);
  rollout_topology(ctx, dm, w->sw);
  const RolloutPolicy p{ut, dts, N, dt, K, uff, first, count, 0};
  rollout_eval(ctx, dm, *w, p, controller, s, x, k, mask);
}

}  // extern "C"
