// TEST INFRASTRUCTURE: what every host emulator of the rollout shares (tests/*/*_emu.cpp include it; tests/rollout_emu.py is its Python side).  The host
// build of the rollout's per-instance entry (wb_humanoid_mpc_amd/csrc/hsqp_rollout.h: rollout_entry, what k_rollout / k_rollout_plant do) with a
// one-lane context, the instantiation chosen by the library's own rule (rollout_dispatch) from parameter blocks packed by the library's own functions:
//   emu_create(desc, err, len) / emu_destroy(h)     the model image comes from the binding's hsqp_model_desc
//   emu_rollout(h, call)                            one rollout over a batch, whatever the configuration
//   emu_ws_bytes(cent, torque, ground, actuated, varied)   sizeof of the rollout workspace (the kernel's LDS) of a configuration
// and for the point-wise entries of the emulators: fresh<T>() (a NaN-filled workspace), load_pushes.
// A program that only calls the entries defines ROLLOUT_EMU_DECLARATIONS_ONLY in front (tests/actuator/actuator_sanitize.cpp).
#pragma once
#include <cstdint>

#include "../../include/hsqp_actuator.h"
#include "../../include/hsqp_contact.h"
#include "../../include/hsqp_inertia.h"
#include "../../include/hsqp_plant.h"
#include "../../include/hsqp_push.h"
#include "../../include/hsqp_rollout.h"

// One rollout call.  Optional pointers: null means off / not wanted.
struct emu_rollout_call {
  // the policy: inputs ut [B][N][35] on the grid dts [B][N] (null: uniform dt), gain window K [B][count][35][58], uff [B][count][35] from entry `first`
  // (feedback controller), nominal states xt [B][N + 1][58] (torque plant)
  const double* ut; const double* dts; const double* xt; const double* K; const double* uff;
  double dt;
  int32_t N, first, count, B;
  const hsqp_rollout_settings* st;
  const double* s0;                  // [B]
  const double* x0;                  // [B][58]
  double duration;
  int32_t n, max_pushes;
  const int32_t* n_pushes;           // [B] (null: no push table)
  const hsqp_push* pushes;           // [B][max_pushes]
  const double* stamp0;              // [B] (null: first node at 0)
  double* x; double* u;              // [B][n][58], [B][n][35]
  int32_t* status; int32_t* steps; int32_t* rejected;   // [B]
  double* last;                      // [B][3][23] the actuator record (written on the actuator model only)
  const hsqp_plant_settings* plant;          // null or kind FLOW: the flow map of the handle's formulation
  const hsqp_contact_settings* contact;      // null or enabled = 0: no ground
  const hsqp_contact_ground* ground;         // [B] (null: the setting's values)
  const hsqp_actuator_settings* actuator;    // null or enabled = 0: no actuator model
  const hsqp_inertia_instance* inertia;      // [B] (null: no table)
};

extern "C" {
void* emu_create(const hsqp_model_desc* md, char* err, int errlen);
void emu_destroy(void* h);
void emu_rollout(void* h, const emu_rollout_call* c);
int emu_ws_bytes(int cent, int torque, int ground, int actuated, int varied);
}

#ifndef ROLLOUT_EMU_DECLARATIONS_ONLY
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "hsqp_host.h"
#include "hsqp_rollout.h"

using namespace hsqp;

// the workspace starts as NaN bit patterns, like the device's uninitialised LDS: a read of something never written shows
template <class T>
std::unique_ptr<T> fresh() {
  std::unique_ptr<T> w(new T);
  std::memset(static_cast<void*>(w.get()), 0xFF, sizeof(T));
  return w;
}

// every push active from 0 for one second; the segment starts at 0
inline unsigned load_pushes(const Ctx& ctx, int n_push, const hsqp_push* pushes, PushSet& set) {
  std::unique_ptr<hsqp_push[]> tab(new hsqp_push[n_push > 0 ? n_push : 1]);
  for (int i = 0; i < n_push; ++i) { tab[i] = pushes[i]; tab[i].t_start = 0.0; tab[i].duration = 1.0; }
  const int32_t np = n_push;
  push_load(ctx, PushTable{&np, tab.get(), n_push > 0 ? n_push : 1, nullptr, 0}, 0, set);
  return push_active(set, 0.0);
}

extern "C" {

void* emu_create(const hsqp_model_desc* md, char* err, int errlen) {
  auto* dm = new DevModel;
  const std::string e = build_dev_model(*md, *dm);
  if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); delete dm; return nullptr; }
  return dm;
}
void emu_destroy(void* h) { delete static_cast<DevModel*>(h); }

void emu_rollout(void* h, const emu_rollout_call* c) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  const size_t B = (size_t)c->B;
  const bool torque = c->plant && c->plant->kind == HSQP_PLANT_TORQUE;
  const RolloutVariant v(dm.formulation == HSQP_FORM_CENTROIDAL, torque, c->contact && c->contact->enabled, c->actuator && c->actuator->enabled, c->inertia);
  double gains[3 * NJ], table[3 * NJ];
  std::vector<hsqp_contact_ground> ground(B);
  std::vector<double> own_last(B * 3 * NJ);
  PlantParams pp{};
  ContactParams cp{};
  ActuatorParams ap{};
  if (torque) { plant_pack_gains(*c->plant, gains); pp = PlantParams{gains, c->plant->lookahead, c->xt}; }
  if (v.ground) {
    contact_fill_ground(*c->contact, c->ground, B, B, ground.data());
    cp = ContactParams{ground.data(), c->contact->stiffness, c->contact->damping, c->contact->slip_velocity};
  }
  if (v.actuated) {
    actuator_pack_table(*c->actuator, table);
    ap = ActuatorParams{table, c->actuator->command_period, c->actuator->friction_velocity, c->last ? c->last : own_last.data()};
  }
  const InertiaParams ip{v.varied ? c->inertia : nullptr};
  const RolloutArgs a{c->ut, c->dts, c->N, c->dt, c->K, c->uff, c->first, c->count, *c->st, c->s0, c->x0, c->duration, c->n, c->x, c->u, c->status, c->steps,
                      c->rejected, PushTable{c->n_pushes, c->pushes, c->max_pushes, c->stamp0, 1}};
  rollout_dispatch(v, [&](auto stage) {
    auto w = fresh<RolloutWS<typename decltype(stage)::type>>();
    const Ctx ctx{0, 1, nullptr};
    for (int b = 0; b < c->B; ++b) rollout_entry(ctx, dm, *w, a, pp, cp, ap, ip, b);
  });
}

int emu_ws_bytes(int cent, int torque, int ground, int actuated, int varied) {
  return rollout_dispatch(RolloutVariant(cent, torque, ground, actuated, varied), [](auto stage) { return (int)sizeof(RolloutWS<typename decltype(stage)::type>); });
}

}  // extern "C"
#endif
