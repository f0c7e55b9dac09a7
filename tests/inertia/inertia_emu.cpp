// TEST INFRASTRUCTURE: the host build of the per-instance inertial variations of the torque plant (wb_humanoid_mpc_amd/csrc/hsqp_inertia.h, hsqp_plant.h,
// hsqp_rollout.h, k_rollout_plant, k_inertia_eval) with a one-lane context, for tests/test_inertia.py (compiled by the test with -ffp-contract=off, also
// with -DHSQP_EMU_REVERSE).  A shared library loaded through ctypes (the model image comes from the binding's hsqp_model_desc).  table: the
// per-instance entries (null: no table — the instantiation the handle launches then is the plant's own, which has no variation in it).
//   ine_create(desc, err, len) / ine_destroy(h)
//   ine_eval(h, table [1] or null, x [58], M [29][29], nle [29], mass [1]): hsqp_inertia_eval for one instance
//   ine_accel(h, table [1] or null, cs, x [58], W [12], tau [23], armature [23], n_push, pushes, vd [29]): forward dynamics at the state x under the joint
//              torques tau, every given push and — cs non-null and enabled: on the ground — the contact forces, else the contact wrenches W
//   ine_rollout(h, plant, table [B] or null, settings, N, dts, dt, xt, ut, K, uff, first, count, B, s0, x0, duration, n, n_pushes, pushes, max_pushes, stamp0,
//               x, u, status, steps, rejected): ple_rollout of tests/plant/plant_emu.cpp on the varied plant
//   ine_ws_bytes(which): sizeof of the rollout workspace on the varied plant — 0: plain, 1: on the ground, 2: actuator, 3: both — and 4: of hsqp_inertia_eval's
#include <cstring>
#include <memory>
#include <string>

#include "hsqp_host.h"
#include "hsqp_rollout.h"

using namespace hsqp;

using WS = RolloutWS<PlantVaried<PlantStage>>;          // the varied plant
using WSC = RolloutWS<PlantVaried<PlantContactStage>>;  // ... on the ground
using WS0 = RolloutWS<PlantStage>;                      // the plant's own (no table)

template <class T>
static std::unique_ptr<T> fresh() {
  // the workspace starts as NaN bit patterns, like the device's uninitialised LDS: a read of something never written shows
  std::unique_ptr<T> w(new T);
  std::memset(static_cast<void*>(w.get()), 0xFF, sizeof(T));
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

void* ine_create(const hsqp_model_desc* md, char* err, int errlen) {
  auto* dm = new DevModel;
  const std::string e = build_dev_model(*md, *dm);
  if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); delete dm; return nullptr; }
  return dm;
}
void ine_destroy(void* h) { delete static_cast<DevModel*>(h); }

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

void ine_rollout(void* h, const hsqp_plant_settings* ps, const hsqp_inertia_instance* table, const hsqp_rollout_settings* st, int N, const double* dts, double dt,
                 const double* xt, const double* ut, const double* K, const double* uff, int first, int count, int B, const double* s0, const double* x0, double duration,
                 int n, const int32_t* n_pushes, const hsqp_push* pushes, int max_pushes, const double* stamp0, double* x, double* u, int32_t* status, int32_t* steps,
                 int32_t* rejected) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  const PushTable tbl{n_pushes, pushes, max_pushes, stamp0, 1};
  auto w = fresh<WS>();
  auto w0 = fresh<WS0>();
  const Ctx ctx{0, 1, nullptr};
  double g[3 * NJ];
  gains_of(*ps, g);
  const PlantParams pp{g, ps->lookahead, xt};
  for (int b = 0; b < B; ++b) {
    const RolloutPolicy p{ut + (size_t)b * N * NU, dts ? dts + (size_t)b * N : nullptr, N, dt, K ? K + (size_t)b * count * NU * NX : nullptr,
                          uff ? uff + (size_t)b * count * NU : nullptr, first, count, 0};
    // the instantiation the handle launches: the varied plant, or the plant's own
    if (table) {
      plant_load(ctx, pp, b, N, w->sw.pl);
      inertia_load(ctx, InertiaParams{table}, b, w->sw.iw);
      rollout_instance(ctx, dm, *w, p, *st, s0[b], x0 + (size_t)b * NX, duration, n, x ? x + (size_t)b * n * NX : nullptr, u ? u + (size_t)b * n * NU : nullptr,
                       status + b, steps ? steps + b : nullptr, rejected ? rejected + b : nullptr, tbl, b);
    } else {
      plant_load(ctx, pp, b, N, w0->sw.pl);
      rollout_instance(ctx, dm, *w0, p, *st, s0[b], x0 + (size_t)b * NX, duration, n, x ? x + (size_t)b * n * NX : nullptr, u ? u + (size_t)b * n * NU : nullptr,
                       status + b, steps ? steps + b : nullptr, rejected ? rejected + b : nullptr, tbl, b);
    }
  }
}

int ine_ws_bytes(int which) {
  switch (which) {
    case 0: return (int)sizeof(RolloutWS<PlantVaried<PlantStage>>);
    case 1: return (int)sizeof(RolloutWS<PlantVaried<PlantContactStage>>);
    case 2: return (int)sizeof(RolloutWS<PlantVaried<PlantActStage>>);
    case 3: return (int)sizeof(RolloutWS<PlantVaried<PlantContactActStage>>);
    default: return (int)sizeof(InertiaEvalWS);
  }
}

}  // extern "C"
