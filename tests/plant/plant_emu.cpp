// TEST INFRASTRUCTURE: the host build of the torque plant of the rollout (wb_humanoid_mpc_amd/csrc/hsqp_plant.h, hsqp_rollout.h, k_rollout_plant)
// with a one-lane context, for tests/test_plant.py (compiled by the test with -ffp-contract=off, also with -DHSQP_EMU_REVERSE).  A shared library
// loaded through ctypes (the model image comes from the binding's hsqp_model_desc):
//   ple_create(desc, err, len) / ple_destroy(h)
//   ple_accel(h, x [58], W [12], tau [23], armature [23], n_push, pushes [n_push], vd [29]): forward dynamics at the state x under the joint torques
//              tau, the contact wrenches W and every given push
//   ple_tau(h, x [58], u [35], tau [23]): the feed-forward torques (policy_node)
//   ple_eval(h, plant, controller, N, dts [N] or null, dt, xt [N + 1][58], ut [N][35], K [count][35][58], uff [count][35], first, count, s, x [58],
//            n_push, pushes, k [58]): one evaluation of the closed loop on the torque plant
//   ple_rollout(h, plant, settings, N, dts [B][N] or null, dt, xt [B][N + 1][58], ut [B][N][35], K, uff, first, count, B, s0 [B], x0 [B][58], duration, n,
//               n_pushes [B] or null, pushes [B][max_pushes], max_pushes, stamp0 [B] or null, x [B][n][58], u [B][n][35], status / steps / rejected [B])
//   ple_ws_bytes(): sizeof of the rollout workspace (the kernel's LDS)
#include <cstring>
#include <memory>
#include <string>

#include "hsqp_host.h"
#include "hsqp_rollout.h"

using namespace hsqp;

using WS = RolloutWS<PlantStage>;

static std::unique_ptr<WS> fresh() {
  // the workspace starts as NaN bit patterns, like the device's uninitialised LDS: a read of something never written shows
  std::unique_ptr<WS> w(new WS);
  std::memset(static_cast<void*>(w.get()), 0xFF, sizeof(WS));
  return w;
}

static void gains_of(const hsqp_plant_settings& ps, double* g) {
  for (int j = 0; j < NJ; ++j) { g[j] = ps.kp[j]; g[NJ + j] = ps.kd[j]; g[2 * NJ + j] = ps.armature[j]; }
}

// every push active from 0 for one second; the segment starts at 0
static unsigned load_pushes(const Ctx& ctx, int n_push, const hsqp_push* pushes, PushSet& set) {
  std::unique_ptr<hsqp_push[]> tab(new hsqp_push[n_push > 0 ? n_push : 1]);
  for (int i = 0; i < n_push; ++i) { tab[i] = pushes[i]; tab[i].t_start = 0.0; tab[i].duration = 1.0; }
  const int32_t np = n_push;
  push_load(ctx, PushTable{&np, tab.get(), n_push > 0 ? n_push : 1, nullptr, 0}, 0, set);
  return push_active(set, 0.0);
}

extern "C" {

void* ple_create(const hsqp_model_desc* md, char* err, int errlen) {
  auto* dm = new DevModel;
  const std::string e = build_dev_model(*md, *dm);
  if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); delete dm; return nullptr; }
  return dm;
}
void ple_destroy(void* h) { delete static_cast<DevModel*>(h); }

void ple_accel(void* h, const double* x, const double* W, const double* tau, const double* armature, int n_push, const hsqp_push* pushes, double* vd) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  auto w = fresh();
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
  auto w = fresh();
  policy_node(Ctx{0, 1, nullptr}, dm, w->sw.st, x, u, tau);
}

void ple_eval(void* h, const hsqp_plant_settings* ps, int controller, int N, const double* dts, double dt, const double* xt, const double* ut, const double* K,
              const double* uff, int first, int count, double s, const double* x, int n_push, const hsqp_push* pushes, double* k) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  auto w = fresh();
  const Ctx ctx{0, 1, nullptr};
  double g[3 * NJ];
  gains_of(*ps, g);
  plant_load(ctx, PlantParams{g, ps->lookahead, xt}, 0, N, w->sw.pl);
  const unsigned mask = load_pushes(ctx, n_push, pushes, w->push);
  rollout_topology(ctx, dm, w->sw);
  const RolloutPolicy p{ut, dts, N, dt, K, uff, first, count, 0};
  rollout_eval(ctx, dm, *w, p, controller, s, x, k, mask);
}

void ple_rollout(void* h, const hsqp_plant_settings* ps, const hsqp_rollout_settings* st, int N, const double* dts, double dt, const double* xt, const double* ut,
                 const double* K, const double* uff, int first, int count, int B, const double* s0, const double* x0, double duration, int n,
                 const int32_t* n_pushes, const hsqp_push* pushes, int max_pushes, const double* stamp0, double* x, double* u, int32_t* status, int32_t* steps,
                 int32_t* rejected) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  const PushTable tbl{n_pushes, pushes, max_pushes, stamp0, 1};
  auto w = fresh();
  const Ctx ctx{0, 1, nullptr};
  double g[3 * NJ];
  gains_of(*ps, g);
  const PlantParams pp{g, ps->lookahead, xt};
  for (int b = 0; b < B; ++b) {
    const RolloutPolicy p{ut + (size_t)b * N * NU, dts ? dts + (size_t)b * N : nullptr, N, dt, K ? K + (size_t)b * count * NU * NX : nullptr,
                          uff ? uff + (size_t)b * count * NU : nullptr, first, count, 0};
    plant_load(ctx, pp, b, N, w->sw.pl);
    rollout_instance(ctx, dm, *w, p, *st, s0[b], x0 + (size_t)b * NX, duration, n, x ? x + (size_t)b * n * NX : nullptr, u ? u + (size_t)b * n * NU : nullptr,
                     status + b, steps ? steps + b : nullptr, rejected ? rejected + b : nullptr, tbl, b);
  }
}

int ple_ws_bytes() { return (int)sizeof(WS); }

}  // extern "C"
