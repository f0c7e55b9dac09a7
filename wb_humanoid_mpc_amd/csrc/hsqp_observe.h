// The observation model of the resident loop (include/hsqp_observe.h): what the MPC measures of the plant's state — a per-instance bias, white
// Gaussian noise from a counter-based generator, and a delay of whole MPC periods through a ring of the plant's states at the cycle starts.
//
// Shape: one item per (instance, block of four state entries), 15 items per instance (the last block holds two entries); an item loads its
// entries of the plant's state, stores them into the ring (every slot when the instance starts an episode), loads the delayed entries, draws
// the block's four normals if any of its sigmas is nonzero, and stores its entries of y.  Items share nothing: no LDS, no barrier, no atomics,
// ordinary vector loads and stores.  The item of block 0 also stores the instance's policy time s0 (ObserveArgs::s0).
//
// The generator is Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) restated here so that the
// stream can be restated anywhere: counter {block, instance, draw, 0}, key {seed low, seed high}.  The four words become four uniforms
// u = (r + 0.5) 2^-32 in (0, 1) and two Box-Muller pairs.  The stream depends on (seed, instance, draw, entry) and on nothing else.
//
// Arithmetic: y_i = x_i + (bias_i + sigma_i z_i), unfused (`#pragma clang fp contract(off)`), so the device differs from the host build of this
// source (tests/observe/observe_emu.cpp) and from the numpy restatement (tests/observe_ref.py) only by its log / sqrt / sin / cos.  An entry
// with bias_i == 0 and sigma_i == 0 is COPIED: no arithmetic touches it, so a NaN keeps its payload and a zero its sign.
#pragma once
#include "hsqp_common.h"
#include "../../include/hsqp_observe.h"

namespace hsqp {

constexpr int OBS_BLOCK = 4;                                   // entries per item: the words of one Philox call
constexpr int OBS_BLOCKS = (NX + OBS_BLOCK - 1) / OBS_BLOCK;   // 15 items per instance
constexpr int OBS_THREADS = 64;                                // items per workgroup of k_observe

struct Philox4 { uint32_t r[4]; };

HSQP_HD void philox_mulhilo(uint32_t a, uint32_t b, uint32_t* hi, uint32_t* lo) {
#if defined(__HIP_DEVICE_COMPILE__)
  *hi = __umulhi(a, b);
  *lo = a * b;
#else
  const uint64_t p = (uint64_t)a * (uint64_t)b;
  *hi = (uint32_t)(p >> 32);
  *lo = (uint32_t)p;
#endif
}

// Philox4x32 with ten rounds: counter c[4], key k[2]
HSQP_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    uint32_t hi0, lo0, hi1, lo1;
    philox_mulhilo(0xD2511F53u, c0, &hi0, &lo0);
    philox_mulhilo(0xCD9E8D57u, c2, &hi1, &lo1);
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the four standard normals of block `block` of instance b at draw `draw`: lanes 0, 1 from (u_0, u_1), lanes 2, 3 from (u_2, u_3)
HSQP_HD void observe_normals(uint32_t key0, uint32_t key1, uint32_t block, uint32_t b, uint32_t draw, double* z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const Philox4 p = philox4x32_10(block, b, draw, 0u, key0, key1);
  const double scale = 1.0 / 4294967296.0, two_pi = 6.283185307179586;
  // (one argument reduction per pair on the device, sincos: four inlined reductions, sin and cos of both pairs, are far more registers than a copy
  // of 58 doubles deserves)
  for (int pair = 0; pair < 2; ++pair) {
    const double u0 = ((double)p.r[2 * pair] + 0.5) * scale, u1 = ((double)p.r[2 * pair + 1] + 0.5) * scale;
    const double radius = sqrt(-2.0 * log(u0)), angle = two_pi * u1;
    double sn, cs;
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(angle, &sn, &cs);
#else
    sn = sin(angle); cs = cos(angle);
#endif
    z[2 * pair] = radius * cs;
    z[2 * pair + 1] = radius * sn;
  }
}

struct ObserveArgs {
  const hsqp_observe_instance* table;   // [B] the entries in force, or null: every instance neutral
  uint32_t key0, key1;                  // the seed's low and high word
  uint32_t draw;                        // the draw index: in the loop the index of the cycle that uses the observation
  int B;
  int slots;                            // sensor_delay + compute_delay + 1 slots of the ring; 1: no ring, y is formed from x
  int write_slot, read_slot;            // cycle mod slots, (cycle - delay) mod slots
  int fresh_all;                        // every instance starts an episode in this cycle
  const int* mode_b;                    // [B] the per-instance warm-start mode of this cycle (HSQP_WARM_COLD: the instance starts an episode), or null
  const double* x;                      // [B][NX] the plant's state
  double* ring;                         // [slots][B][NX], or null with slots == 1
  double* y;                            // [B][NX] the observation
  double* s0;                           // [B] the time in the policy's frame at which the plant takes it over, or null
  double s0_value;
};

// item (b, block)
HSQP_HD void observe_item(const ObserveArgs& a, int b, int block) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int i0 = block * OBS_BLOCK, n = NX - i0 < OBS_BLOCK ? NX - i0 : OBS_BLOCK;
  const size_t row = (size_t)b * NX + i0, slot = (size_t)a.B * NX;
  double v[OBS_BLOCK];
  for (int j = 0; j < n; ++j) v[j] = a.x[row + j];
  if (a.ring && a.slots > 1) {
    const bool fresh = a.fresh_all || (a.mode_b && a.mode_b[b] == HSQP_WARM_COLD);
    if (fresh) {   // the plant rested at its start state for the periods before the episode
      for (int s = 0; s < a.slots; ++s)
        for (int j = 0; j < n; ++j) a.ring[s * slot + row + j] = v[j];
    } else {
      for (int j = 0; j < n; ++j) a.ring[a.write_slot * slot + row + j] = v[j];
      for (int j = 0; j < n; ++j) v[j] = a.ring[a.read_slot * slot + row + j];
    }
  }
  if (a.table) {
    const hsqp_observe_instance& e = a.table[b];
    double bias[OBS_BLOCK], sigma[OBS_BLOCK], z[OBS_BLOCK] = {0.0, 0.0, 0.0, 0.0};
    bool any = false;
    for (int j = 0; j < n; ++j) { bias[j] = e.bias[i0 + j]; sigma[j] = e.sigma[i0 + j]; any = any || sigma[j] != 0.0; }
    if (any) observe_normals(a.key0, a.key1, (uint32_t)block, (uint32_t)b, a.draw, z);
    for (int j = 0; j < n; ++j) {
      if (bias[j] == 0.0 && sigma[j] == 0.0) continue;   // copied
      const double noise = sigma[j] * z[j];
      const double offset = bias[j] + noise;
      v[j] = v[j] + offset;
    }
  }
  for (int j = 0; j < n; ++j) a.y[row + j] = v[j];
  if (block == 0 && a.s0) a.s0[b] = a.s0_value;
}

// ---- a cycle's bookkeeping (the library's loop_cycle and the host build share it)
// the ring of cycle `cycle` with `delay` = sensor_delay + compute_delay periods: delay + 1 slots, written at cycle mod slots, read at (cycle - delay) mod slots
HSQP_HD void observe_cycle_slots(int cycle, int delay, ObserveArgs& a) {
  a.slots = delay + 1;
  a.write_slot = cycle % a.slots;
  a.read_slot = (cycle + 1) % a.slots;   // cycle - delay = cycle + 1 - slots
}
// the time in the policy's frame at which the plant takes it over, s0 = compute_delay period
HSQP_HD double observe_policy_time(int compute_delay, double period) { return compute_delay * period; }
// the problem time t_p = t - s0
HSQP_HD double observe_problem_time(double t, double s0) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return t - s0;
}

// ---- the argument checks of include/hsqp_observe.h that need no device (the library and the host build share them)
HSQP_HD bool observe_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and +-inf
// what is wrong with the settings (null: nothing)
HSQP_HD const char* observe_settings_error(const hsqp_observe_settings& s) {
  if (s.sensor_delay < 0 || s.compute_delay < 0) return "negative delay";
  if (s.sensor_delay > HSQP_OBS_MAX_DELAY || s.compute_delay > HSQP_OBS_MAX_DELAY || s.sensor_delay + s.compute_delay > HSQP_OBS_MAX_DELAY)
    return "sensor_delay + compute_delay > HSQP_OBS_MAX_DELAY";
  return nullptr;
}
// the first field of an entry that is refused: 0 none, 1 + i: bias[i] non-finite, -(1 + i): sigma[i] negative or non-finite
HSQP_HD int observe_entry_error(const hsqp_observe_instance& e) {
  for (int i = 0; i < NX; ++i) {
    if (!observe_finite(e.bias[i])) return 1 + i;
    if (!(e.sigma[i] >= 0.0) || !observe_finite(e.sigma[i])) return -(1 + i);
  }
  return 0;
}
// the policy of a problem of n_nodes intervals of dt is evaluated over [k P, (k + 1) P]: inside its horizon
HSQP_HD bool observe_horizon_ok(int compute_delay, double period, int n_nodes, double dt) { return !((compute_delay + 1) * period > n_nodes * dt); }

// the items of workgroup `group`
HSQP_HD void observe_group(const Ctx& ctx, const ObserveArgs& a, int group) {
  WG_FOR(ctx, j, OBS_THREADS) {
    const int id = group * OBS_THREADS + j;
    if (id < a.B * OBS_BLOCKS) observe_item(a, id / OBS_BLOCKS, id % OBS_BLOCKS);
  }
}

}  // namespace hsqp
