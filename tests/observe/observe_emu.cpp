// TEST INFRASTRUCTURE: the host build of the observation model's sources (wb_humanoid_mpc_amd/csrc/hsqp_observe.h: k_observe's item function, the
// generator, a cycle's bookkeeping and the argument checks) with a one-lane loop, for tests/test_observe.py.  A shared library loaded through ctypes;
// every array is the caller's, in the device layout.  Built with -ffp-contract=off: the arithmetic the device evaluates unfused.
#include "hsqp_observe.h"

using namespace hsqp;

static const Ctx kLane{0, 1, nullptr};

extern "C" {

void obs_philox(const uint32_t* counter, const uint32_t* key, uint32_t* out) {
  const Philox4 p = philox4x32_10(counter[0], counter[1], counter[2], counter[3], key[0], key[1]);
  for (int i = 0; i < 4; ++i) out[i] = p.r[i];
}

// z [58]: the normals of every entry of instance b at draw n
void obs_normals(uint64_t seed, uint32_t b, uint32_t n, double* z) {
  for (int k = 0; k < OBS_BLOCKS; ++k) {
    double four[OBS_BLOCK];
    observe_normals((uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), (uint32_t)k, b, n, four);
    for (int j = 0; j < OBS_BLOCK && k * OBS_BLOCK + j < NX; ++j) z[k * OBS_BLOCK + j] = four[j];
  }
}

// step 0 of cycle `cycle` (the draw index) of B instances with `delay` = sensor_delay + compute_delay; delay < 0: hsqp_observe_eval (no ring, ring may be
// null).  table, mode_b, s0 may be null.  Every workgroup of the launch, one lane each.
void obs_cycle(const hsqp_observe_instance* table, uint64_t seed, uint32_t cycle, int delay, int B, int fresh_all, const int* mode_b, const double* x, double* ring,
               double* y, double* s0, double s0_value) {
  ObserveArgs a{};
  a.table = table;
  a.key0 = (uint32_t)(seed & 0xffffffffu); a.key1 = (uint32_t)(seed >> 32);
  a.draw = cycle; a.B = B; a.slots = 1;
  if (delay >= 0) observe_cycle_slots((int)cycle, delay, a);
  a.fresh_all = fresh_all; a.mode_b = mode_b;
  a.x = x; a.ring = ring; a.y = y; a.s0 = s0; a.s0_value = s0_value;
  for (int g = 0; g < (B * OBS_BLOCKS + OBS_THREADS - 1) / OBS_THREADS; ++g) observe_group(kLane, a, g);
}

double obs_policy_time(int compute_delay, double period) { return observe_policy_time(compute_delay, period); }
double obs_problem_time(double t, double s0) { return observe_problem_time(t, s0); }

// the argument checks: 0 accepted, 1 refused (settings); 0 / 1 + i / -(1 + i) (entry, observe_entry_error); 1 inside the horizon
int obs_settings_refused(const hsqp_observe_settings* s) { return observe_settings_error(*s) ? 1 : 0; }
int obs_entry_error(const hsqp_observe_instance* e) { return observe_entry_error(*e); }
int obs_horizon_ok(int compute_delay, double period, int n_nodes, double dt) { return observe_horizon_ok(compute_delay, period, n_nodes, dt) ? 1 : 0; }

}  // extern "C"
