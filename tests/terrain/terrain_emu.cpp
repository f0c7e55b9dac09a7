// TEST INFRASTRUCTURE: the host build of the height-map terrain under the torque plant (wb_humanoid_mpc_amd/csrc/hsqp_terrain.h, hsqp_contact.h, hsqp_plant.h,
// hsqp_rollout.h, k_rollout_plant, k_contact_eval, k_terrain_eval) with a one-lane context, for tests/test_terrain.py (compiled by the test with
// -ffp-contract=off) and tests/terrain/terrain_sanitize.cpp.  The shared entries of tests/rollout/rollout_emu.h, the rollout on the terrain (tests/terrain/terrain_emu.h:
// emu_rollout_terrain), and the point-wise ones below.  cs: the contact setting, ground: the per-instance table [1] (null: the setting's values), t: the terrain with the placement
// [1] of the instance (null, no maps or no placement: none).
//   emu_terrain_eval(cs, ground, t, n_pts, xy [n][2], height [n], normal [n][3]): hsqp_terrain_eval for one instance
//   emu_contact_eval(h, cs, ground, t, x [58], force [8][3], pen [8]): hsqp_contact_eval for one instance — on the terrain model while t has maps and a placement
#include "terrain_emu.h"

static ContactParams params_of(const hsqp_contact_settings* cs, const hsqp_contact_ground* ground, std::vector<hsqp_contact_ground>& store) {
  store.resize(1);
  contact_fill_ground(*cs, ground, 1, 1, store.data());
  return ContactParams{store.data(), cs->stiffness, cs->damping, cs->slip_velocity};
}

extern "C" {

void emu_terrain_eval(const hsqp_contact_settings* cs, const hsqp_contact_ground* ground, const emu_terrain* t, int n_pts, const double* xy, double* height,
                      double* normal) {
  std::vector<hsqp_contact_ground> store;
  const ContactParams cp = params_of(cs, ground, store);
  EmuTerrain ter(t, 1);
  if (!t) { ter.place.resize(1); terrain_fill_place(nullptr, 0, 1, ter.place.data()); ter.tp = TerrainParams{nullptr, nullptr, ter.place.data(), 0}; }
  auto ts = fresh<TerrainSet>();
  terrain_eval_instance(Ctx{0, 1, nullptr}, cp, ter.tp, *ts, 0, n_pts, xy, height, normal);
}

void emu_contact_eval(void* h, const hsqp_contact_settings* cs, const hsqp_contact_ground* ground, const emu_terrain* t, const double* x, double* force,
                      double* pen) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  std::vector<hsqp_contact_ground> store;
  const ContactParams cp = params_of(cs, ground, store);
  if (t && t->n_maps > 0 && t->place) {
    const EmuTerrain ter(t, 1);
    auto w = fresh<ContactEvalWST<ContactTerrainSet>>();
    contact_eval_instance(Ctx{0, 1, nullptr}, dm, *w, cp, &ter.tp, 0, x, force, pen);
  } else {
    auto w = fresh<ContactEvalWS>();
    contact_eval_instance(Ctx{0, 1, nullptr}, dm, *w, cp, 0, x, force, pen);
  }
}

}  // extern "C"
