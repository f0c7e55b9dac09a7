// TEST INFRASTRUCTURE: the host build of the actuator model on the torque plant of the rollout (wb_humanoid_mpc_amd/csrc/hsqp_actuator.h, hsqp_rollout.h,
// k_rollout_plant's four instantiations) with a one-lane context, for tests/test_actuator.py (compiled by the test with -ffp-contract=off, also
// with -DHSQP_EMU_REVERSE) and tests/actuator/actuator_sanitize.cpp.  A shared library loaded through ctypes (the model image comes from the
// binding's hsqp_model_desc):
//   ace_create(desc, err, len) / ace_destroy(h)
//   ace_law(as, kp [23], kd [23], qp [23], vp [23], tff [23], x [58], out [4][23]): the joint law at the plant state x under the given command:
//           tau | tau_cmd | tau_act | tau_pas
//   ace_tick(s0, period, t, on, next): where t stands in the tick schedule
//   ace_rollout(h, plant, as or null, cs or null, settings, N, dts [B][N] or null, dt, xt, ut, K, uff, first, count, B, s0 [B], x0 [B][58], duration, n,
//               n_pushes [B] or null, pushes [B][max_pushes], max_pushes, stamp0 [B] or null, x [B][n][58], u [B][n][35], status / steps / rejected [B],
//               last [B][3][23] or null): ple_rollout of tests/plant/plant_emu.cpp through the instantiation the handle launches — as null or
//               enabled = 0: the plant's own (last is left alone), cs null or enabled = 0: without a ground
//   ace_ws_bytes(contact): sizeof of the rollout workspace of an actuator instantiation (the kernel's LDS)
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "hsqp_host.h"
#include "hsqp_rollout.h"

using namespace hsqp;

template <class T>
static std::unique_ptr<T> fresh() {
  // the workspace starts as NaN bit patterns, like the device's uninitialised LDS: a read of something never written shows
  std::unique_ptr<T> w(new T);
  std::memset(static_cast<void*>(w.get()), 0xFF, sizeof(T));
  return w;
}

struct Call {
  const DevModel* dm;
  PlantParams pp;
  ContactParams cp;
  ActuatorParams ap;
  const hsqp_rollout_settings* st;
  int N; const double* dts; double dt; const double* ut; const double* K; const double* uff; int first, count, B;
  const double* s0; const double* x0; double duration; int n;
  PushTable tbl;
  double* x; double* u; int32_t* status; int32_t* steps; int32_t* rejected;
};

// what k_rollout_plant<SW> does for every instance
template <class SW>
static void run(const Call& c) {
  auto w = fresh<RolloutWS<SW>>();
  const Ctx ctx{0, 1, nullptr};
  for (int b = 0; b < c.B; ++b) {
    const RolloutPolicy p{c.ut + (size_t)b * c.N * NU, c.dts ? c.dts + (size_t)b * c.N : nullptr, c.N, c.dt, c.K ? c.K + (size_t)b * c.count * NU * NX : nullptr,
                          c.uff ? c.uff + (size_t)b * c.count * NU : nullptr, c.first, c.count, 0};
    plant_load(ctx, c.pp, b, c.N, w->sw.pl);
    if constexpr (std::is_same<SW, PlantContactStage>::value || std::is_same<SW, PlantContactActStage>::value) contact_load(ctx, c.cp, b, w->sw.ct);
    if constexpr (RolloutActuated<SW>::value) actuator_load(ctx, c.ap, b, w->sw.act);
    rollout_instance(ctx, *c.dm, *w, p, *c.st, c.s0[b], c.x0 + (size_t)b * NX, c.duration, c.n, c.x ? c.x + (size_t)b * c.n * NX : nullptr,
                     c.u ? c.u + (size_t)b * c.n * NU : nullptr, c.status + b, c.steps ? c.steps + b : nullptr, c.rejected ? c.rejected + b : nullptr, c.tbl, b);
  }
}

static void table_of(const hsqp_actuator_settings& as, double* t) {
  for (int j = 0; j < NJ; ++j) { t[j] = as.effort_limit[j]; t[NJ + j] = as.damping[j]; t[2 * NJ + j] = as.friction[j]; }
}

extern "C" {

void* ace_create(const hsqp_model_desc* md, char* err, int errlen) {
  auto* dm = new DevModel;
  const std::string e = build_dev_model(*md, *dm);
  if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); delete dm; return nullptr; }
  return dm;
}
void ace_destroy(void* h) { delete static_cast<DevModel*>(h); }

void ace_law(const hsqp_actuator_settings* as, const double* kp, const double* kd, const double* qp, const double* vp, const double* tff, const double* x,
             double* out) {
  auto ac = fresh<ActuatorWS>();
  const Ctx ctx{0, 1, nullptr};
  double t[3 * NJ], rec[3 * NJ];
  table_of(*as, t);
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

void ace_rollout(void* h, const hsqp_plant_settings* ps, const hsqp_actuator_settings* as, const hsqp_contact_settings* cs, const hsqp_rollout_settings* st, int N,
                 const double* dts, double dt, const double* xt, const double* ut, const double* K, const double* uff, int first, int count, int B, const double* s0,
                 const double* x0, double duration, int n, const int32_t* n_pushes, const hsqp_push* pushes, int max_pushes, const double* stamp0, double* x, double* u,
                 int32_t* status, int32_t* steps, int32_t* rejected, double* last) {
  double g[3 * NJ], t[3 * NJ];
  for (int j = 0; j < NJ; ++j) { g[j] = ps->kp[j]; g[NJ + j] = ps->kd[j]; g[2 * NJ + j] = ps->armature[j]; }
  std::vector<hsqp_contact_ground> ground;
  ContactParams cp{nullptr, 0.0, 0.0, 0.0};
  if (cs && cs->enabled) {
    ground.assign(B, hsqp_contact_ground{cs->ground_height, cs->mu});
    cp = ContactParams{ground.data(), cs->stiffness, cs->damping, cs->slip_velocity};
  }
  std::vector<double> own_last((size_t)B * 3 * NJ);
  ActuatorParams ap{nullptr, 0.0, 0.0, nullptr};
  if (as && as->enabled) {
    table_of(*as, t);
    ap = ActuatorParams{t, as->command_period, as->friction_velocity, last ? last : own_last.data()};
  }
  const Call c{static_cast<DevModel*>(h), PlantParams{g, ps->lookahead, xt}, cp, ap, st, N, dts, dt, ut, K, uff, first, count, B, s0, x0, duration, n,
               PushTable{n_pushes, pushes, max_pushes, stamp0, 1}, x, u, status, steps, rejected};
  if (ap.table && cp.ground) run<PlantContactActStage>(c);
  else if (ap.table) run<PlantActStage>(c);
  else if (cp.ground) run<PlantContactStage>(c);
  else run<PlantStage>(c);
}

int ace_ws_bytes(int contact) { return contact ? (int)sizeof(RolloutWS<PlantContactActStage>) : (int)sizeof(RolloutWS<PlantActStage>); }

}  // extern "C"
