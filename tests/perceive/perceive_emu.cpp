// TEST INFRASTRUCTURE: the host build of the per-foot swing heights' sources (wb_humanoid_mpc_amd/csrc/hsqp_perceive.h: k_foot_heights' lane function;
// csrc/hsqp_params.h: the node parameters with the planner's three-argument update) with a one-lane loop, for tests/test_perceive.py and
// tests/perceive/perceive_sanitize.cpp.  Every array is the caller's, in the device layout.  Built with -ffp-contract=off: the arithmetic the device
// evaluates unfused.  The entries are declared in tests/perceive/perceive_emu.h.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "hsqp_host.h"
#include "hsqp_perceive.h"

#include "perceive_emu.h"

using namespace hsqp;

namespace {
// the kernels' view of a terrain and of the contact ground over B instances
struct EmuGround {
  std::vector<TerrainMap> maps;
  std::vector<hsqp_contact_ground> ground;
  TerrainParams tp{};
  ContactParams cp{};
  EmuGround(const pc_terrain* t, size_t B) {
    size_t first = 0;
    for (int m = 0; m < t->n_maps; ++m) { maps.push_back(TerrainMap{t->nx[m], t->ny[m], t->cell[m], first}); first += (size_t)t->nx[m] * t->ny[m]; }
    for (size_t b = 0; b < B; ++b) ground.push_back(hsqp_contact_ground{t->ground_height[b], 0.6});
    tp = TerrainParams{maps.data(), t->heights, t->place, t->n_maps};
    cp = ContactParams{ground.data(), 0.0, 0.0, 0.0};
  }
};
}  // namespace

extern "C" {

// the model image from the binding's hsqp_model_desc, with the default joint state hsqp_set_default_joint_state would give it
void* pc_create(const hsqp_model_desc* md, const double* default_joint_state, char* err, int errlen) {
  auto* dm = new DevModel;
  const std::string e = build_dev_model(*md, *dm);
  if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); delete dm; return nullptr; }
  dm->has_default_joint_state = 1;
  memcpy(dm->default_joint_state, default_joint_state, sizeof(dm->default_joint_state));
  return dm;
}
void pc_destroy(void* h) { delete static_cast<DevModel*>(h); }

// par [n_t][HSQP_NODE_PARAMS]: node_params_eval of one instance at every time; lift, touch [2][E + 1] or both null (the two-argument form at `terrain`).
// Returns the number of times the planner reported its failure at.
int pc_node_params(const hsqp_swing_config* cfg, double terrain, int arm_swing, int E, int n_ev, const double* ev, const int* seq, int n_knots, const double* tt,
                   const double* ts, int n_t, const double* times, const double* lift, const double* touch, double* par) {
  int bad = 0;
  for (int k = 0; k < n_t; ++k)
    if (!node_params_eval(*cfg, terrain, arm_swing, n_ev, ev, seq, n_knots, tt, ts, times[k], par + (size_t)k * HSQP_NODE_PARAMS, lift, touch, E + 1)) ++bad;
  return bad;
}

// one launch of k_foot_heights over B instances: lift, touch [B][2][E + 1], fxy [B][2][E + 1][2]
void pc_foot_heights(void* h, const pc_terrain* t, int B, int E, int K, double time, double offset, const double* x, const int* ne, const double* ev, const int* seq,
                     const double* tt, const double* ts, double* lift, double* touch, double* fxy) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  const EmuGround g(t, (size_t)B);
  PerceiveArgs a{};
  a.B = B; a.E = E; a.K = K; a.t = time; a.offset = offset;
  a.x = x; a.ne = ne; a.ev = ev; a.seq = seq; a.tt = tt; a.ts = ts; a.lift = lift; a.touch = touch; a.fxy = fxy;
  for (int b = 0; b < B; ++b)
    for (int f = 0; f < 2; ++f) perceive_lane(dm, g.cp, g.tp, a, b, f);
}

// height [B][n_pts]: hsqp_terrain_eval's answer (terrain_eval_instance) under the points xy [B][n_pts][2]
void pc_terrain_eval(const pc_terrain* t, int B, int n_pts, const double* xy, double* height) {
  const EmuGround g(t, (size_t)B);
  for (int b = 0; b < B; ++b) {
    TerrainSet ts;
    terrain_eval_instance(Ctx{0, 1, nullptr}, g.cp, g.tp, ts, b, n_pts, xy + (size_t)b * n_pts * 2, height + (size_t)b * n_pts, nullptr);
  }
}

}  // extern "C"
