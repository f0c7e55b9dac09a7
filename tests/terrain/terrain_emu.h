// TEST INFRASTRUCTURE: what the host emulator of the terrain adds to the shared entries of tests/rollout/rollout_emu.h (which it includes, unchanged):
//   emu_rollout_terrain(h, call, terrain)     emu_rollout with a height-map terrain resident (include/hsqp_terrain.h).  A configuration the library's rule
//                                             gives no terrain instantiation — terrain null, no maps, no placement table, no ground — IS emu_rollout;
//                                             the others run rollout_entry on the terrain's stage workspace, packed by the library's own functions
//   emu_ws_bytes_terrain(actuated, varied)    sizeof of the rollout workspace of a configuration on the terrain
//   emu_terrain_eval / emu_contact_eval       the point-wise entries (tests/terrain/terrain_emu.cpp)
// A program that only calls the entries defines ROLLOUT_EMU_DECLARATIONS_ONLY in front (tests/terrain/terrain_sanitize.cpp).
#pragma once
#include "../rollout/rollout_emu.h"
#include "../../include/hsqp_terrain.h"

// The resident terrain of a call: what hsqp_terrain_set_maps and hsqp_terrain_set_instances take
struct emu_terrain {
  int32_t n_maps, reserved;
  const int32_t* nx; const int32_t* ny; const double* cell;   // [n_maps]
  const double* heights;                     // the maps concatenated
  const hsqp_terrain_placement* place;       // [B] (null: no table — the terrain is inert)
};

extern "C" {
void emu_rollout_terrain(void* h, const emu_rollout_call* c, const emu_terrain* t);
int emu_ws_bytes_terrain(int actuated, int varied);
void emu_terrain_eval(const hsqp_contact_settings* cs, const hsqp_contact_ground* ground, const emu_terrain* t, int n_pts, const double* xy, double* height,
                      double* normal);
void emu_contact_eval(void* h, const hsqp_contact_settings* cs, const hsqp_contact_ground* ground, const emu_terrain* t, const double* x, double* force,
                      double* pen);
}

#ifndef ROLLOUT_EMU_DECLARATIONS_ONLY
// the kernels' view of a terrain over B instances (t null: none); the descriptors and the placements live in the object
struct EmuTerrain {
  std::vector<TerrainMap> maps;
  std::vector<hsqp_terrain_placement> place;
  TerrainParams tp{};
  EmuTerrain(const emu_terrain* t, size_t B) {
    if (!t) return;
    size_t first = 0;
    for (int m = 0; m < t->n_maps; ++m) { maps.push_back(TerrainMap{t->nx[m], t->ny[m], t->cell[m], first}); first += (size_t)t->nx[m] * t->ny[m]; }
    place.resize(B);
    terrain_fill_place(t->place, B, B, place.data());
    tp = TerrainParams{maps.data(), t->heights, place.data(), t->n_maps};
  }
};

extern "C" {

void emu_rollout_terrain(void* h, const emu_rollout_call* c, const emu_terrain* t) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  const size_t B = (size_t)c->B;
  const bool torque = c->plant && c->plant->kind == HSQP_PLANT_TORQUE;
  const RolloutVariant v(dm.formulation == HSQP_FORM_CENTROIDAL, torque, c->contact && c->contact->enabled, c->actuator && c->actuator->enabled, c->inertia,
                         t && t->n_maps > 0, t && t->place);
  if (!v.terrain) return emu_rollout(h, c);
  // (the packing of emu_rollout for a torque plant on the ground, and the terrain's)
  double gains[3 * NJ], table[3 * NJ];
  std::vector<hsqp_contact_ground> ground(B);
  std::vector<double> own_last(B * 3 * NJ);
  plant_pack_gains(*c->plant, gains);
  const PlantParams pp{gains, c->plant->lookahead, c->xt};
  contact_fill_ground(*c->contact, c->ground, B, B, ground.data());
  const ContactParams cp{ground.data(), c->contact->stiffness, c->contact->damping, c->contact->slip_velocity};
  ActuatorParams ap{};
  if (v.actuated) {
    actuator_pack_table(*c->actuator, table);
    ap = ActuatorParams{table, c->actuator->command_period, c->actuator->friction_velocity, c->last ? c->last : own_last.data()};
  }
  const InertiaParams ip{v.varied ? c->inertia : nullptr};
  const EmuTerrain ter(t, B);
  const RolloutArgs a{c->ut, c->dts, c->N, c->dt, c->K, c->uff, c->first, c->count, *c->st, c->s0, c->x0, c->duration, c->n, c->x, c->u, c->status, c->steps,
                      c->rejected, PushTable{c->n_pushes, c->pushes, c->max_pushes, c->stamp0, 1}};
  rollout_dispatch(v, [&](auto stage) {
    using SW = typename decltype(stage)::type;
    if constexpr (PlantOnTerrain<SW>::value) {
      auto w = fresh<RolloutWS<SW>>();
      const Ctx ctx{0, 1, nullptr};
      for (int b = 0; b < c->B; ++b) rollout_entry(ctx, dm, *w, a, pp, cp, ap, ip, ter.tp, b);
    }
  });
}

int emu_ws_bytes_terrain(int actuated, int varied) {
  return rollout_dispatch(RolloutVariant(false, true, true, actuated, varied, true, true), [](auto stage) { return (int)sizeof(RolloutWS<typename decltype(stage)::type>); });
}

}  // extern "C"
#endif
