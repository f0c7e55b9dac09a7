// TEST INFRASTRUCTURE: the entries of tests/metrics/metrics_emu.cpp, for tests/test_metrics.py (its ctypes mirror is MetCall) and for
// tests/metrics/metrics_sanitize.cpp, which links that source.
#pragma once
#include <cstdint>

#include "../../include/hsqp_contact.h"
#include "../../include/hsqp_metrics.h"

// One launch of k_loop_metrics.  Optional pointers: null means off.
struct met_call {
  int32_t B, isolate, cycle, form;          // form: 0 no ground, 1 ContactSet, 2 ContactTerrainSet with every instance on the plane
  double period;
  const hsqp_episode_settings* st;          // isolate only
  const int32_t* it_status;                 // [B]
  const hsqp_perf* perf;                    // [B]
  const int32_t* ro_status;                 // [B]
  const double* xs;                         // [B][58]
  const double* x_before;                   // [B][58]
  const double* cmd;                        // [B][4]
  const int32_t* ep_state;                  // [B], isolate only
  const int32_t* steps; const int32_t* rejected;   // [B]
  const double* act_last;                   // [B][3][23] or null: no torque group
  const double* act_limit;                  // [23]
  hsqp_metrics* rec;                        // [B][2]
  int32_t* feet;                            // [B][2]
  const hsqp_contact_settings* contact;     // form != 0
  const hsqp_contact_ground* ground;        // [B] or null: the setting's values
};

extern "C" {
void met_open(int B, hsqp_metrics* rec, int32_t* feet);
void met_cycle(void* h, const met_call* c);
void met_host_close(int n, const int32_t* ids, hsqp_metrics* rec, int32_t* feet);
int met_ws_bytes(int form);
}
