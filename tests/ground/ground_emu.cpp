// TEST INFRASTRUCTURE: the host build of the ground-height estimate's sources (wb_humanoid_mpc_amd/csrc/hsqp_ground.h: k_ground_estimate's lane
// function, the rule, the shift of the knots) with a one-lane loop, for tests/test_ground.py.  A shared library loaded through ctypes; every array
// is the caller's, in the device layout.  Built with -ffp-contract=off: the arithmetic the device evaluates unfused.  -DHSQP_EMU_REVERSE: the
// instances (and the two feet of an instance) are visited in reverse order — every instance owns its entries, so the bits must not change.
#include <cstdio>
#include <string>

#include "hsqp_episode.h"
#include "hsqp_ground.h"
#include "hsqp_host.h"

using namespace hsqp;

extern "C" {

// the model image from the binding's hsqp_model_desc
void* gr_create(const hsqp_model_desc* md, char* err, int errlen) {
  auto* dm = new DevModel;
  const std::string e = build_dev_model(*md, *dm);
  if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); delete dm; return nullptr; }
  return dm;
}
void gr_destroy(void* h) { delete static_cast<DevModel*>(h); }

// foot_z [B][2]: the heights of both contact frames at every state row x [B][58]
void gr_foot_heights(void* h, int B, const double* x, double* foot_z) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  for (int b = 0; b < B; ++b)
    for (int f = 0; f < 2; ++f) foot_z[2 * b + f] = ground_foot_height(dm, x + (size_t)b * NX, f);
}

// one launch of k_ground_estimate over B instances; the optional arrays (foot_z, g_init, mode_b, parked, ts, terrain_b) may be null
void gr_estimate(void* h, int B, int E, double t, double filter_alpha, const double* x, const int* ne, const double* ev, const int* seq, const double* g_in,
                 double* g_out, double* foot_z, const double* g_init, const int* mode_b, const int* parked, double* ts, double* terrain_b) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  GroundArgs a{};
  a.B = B; a.E = E; a.t = t; a.filter_alpha = filter_alpha;
  a.x = x; a.ne = ne; a.ev = ev; a.seq = seq; a.g_in = g_in; a.g_out = g_out; a.foot_z = foot_z;
  a.g_init = g_init; a.mode_b = mode_b; a.parked = parked; a.ts = ts; a.terrain_b = terrain_b;
#if defined(HSQP_EMU_REVERSE)
  for (int b = B - 1; b >= 0; --b) {
    double z[2];
    for (int f = 1; f >= 0; --f) z[f] = ground_foot_height(dm, x + (size_t)b * NX, f);
#else
  for (int b = 0; b < B; ++b) {
    double z[2];
    for (int f = 0; f < 2; ++f) z[f] = ground_foot_height(dm, x + (size_t)b * NX, f);
#endif
    ground_instance_finish(a, b, z);
  }
}

// the rule alone, from given heights z [2]
double gr_rule(const double* z, int n_ev, const double* ev, const int* seq, double t, double filter_alpha, double g_old) {
  return ground_estimate_instance(z, n_ev, ev, seq, t, filter_alpha, g_old, nullptr);
}

// the triage's verdict on one rolled-out state xs [58] with a clean iteration and rollout; ground null: the absolute box
int gr_verdict(const hsqp_episode_settings* st, const double* xs, const double* ground) {
  hsqp_perf perf{};
  return episode_verdict(Ctx{0, 1, nullptr}, *st, 0, perf, HSQP_ROLLOUT_OK, xs, ground);
}

}  // extern "C"
