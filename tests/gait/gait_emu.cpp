// TEST INFRASTRUCTURE: the host build of the gait schedule and ladder update (wb_humanoid_mpc_amd/csrc/hsqp_gait.h, k_gait_update) with a one-lane
// loop, for tests/test_gait.py.  A shared library loaded through ctypes; the state of B instances is the caller's arrays in the device layout:
//   gt_update(settings, B, n [B], ev [B][E], seq [B][E + 1], scal [B][4], t_change [B]   in / out,
//             t, horizon, v_filt [B][4], x [B][58], n_out [B], ev_out [B][E], seq_out [B][E + 1], status [B])
// All or nothing like the entry point: the shadow copy replaces the caller's state only if every instance answered HSQP_GAIT_OK (returns 1).
// Built with -ffp-contract=off: the arithmetic the device evaluates unfused.
#include <cstring>
#include <vector>

#include "hsqp_gait.h"

using namespace hsqp;

extern "C" int gt_update(const hsqp_gait_settings* gs, int B, int* n, double* ev, int* seq, int* scal, double* t_change, double t, double horizon,
                         const double* v_filt, const double* x, int* n_out, double* ev_out, int* seq_out, int* status) {
  const size_t E = gs->max_events;
  std::vector<int> n2(B), seq2(B * (E + 1)), scal2(B * GAIT_SCAL);
  std::vector<double> ev2(B * E), tc2(B);
  const GaitState in{n, ev, seq, scal, t_change}, out{n2.data(), ev2.data(), seq2.data(), scal2.data(), tc2.data()};
  static GaitWork w;
  bool ok = true;
  for (int b = 0; b < B; ++b) {
    status[b] = gait_update_instance(Ctx{0, 1, nullptr}, *gs, w, in, out, b, t, horizon, v_filt + (size_t)b * 4, x + (size_t)b * NX, n_out + b, ev_out + b * E,
                                     seq_out + b * (E + 1));
    ok = ok && status[b] == HSQP_GAIT_OK;
  }
  if (!ok) return 0;
  memcpy(n, n2.data(), B * sizeof(int)); memcpy(seq, seq2.data(), seq2.size() * sizeof(int)); memcpy(scal, scal2.data(), scal2.size() * sizeof(int));
  memcpy(ev, ev2.data(), ev2.size() * 8); memcpy(t_change, tc2.data(), B * 8);
  return 1;
}
