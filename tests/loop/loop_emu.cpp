// TEST INFRASTRUCTURE: the host build of the velocity-command target generator (wb_humanoid_mpc_amd/csrc/hsqp_loop.h, k_command_targets) with a
// one-lane loop, for tests/test_loop.py.  A shared library loaded through ctypes:
//   lp_command_targets(jt [23], alpha, B, v_cmd [B][4], v_filt [B][4] in / out, x0 [B][58], t0, horizon, target_times [B][3], target_states [B][3][58])
// Built with -ffp-contract=off: the arithmetic the device evaluates unfused.
#include "hsqp_loop.h"

using namespace hsqp;

extern "C" void lp_command_targets(const double* jt, double alpha, int B, const double* v_cmd, double* v_filt, const double* x0, double t0, double horizon,
                                   double* target_times, double* target_states) {
  for (int b = 0; b < B; ++b) {
    CommandItem it[CMD_KNOTS];   // the kernel's barrier: every item of the instance loads before any stores
    for (int k = 0; k < CMD_KNOTS; ++k) it[k] = command_item_load(alpha, v_cmd, v_filt, b * CMD_KNOTS + k);
    for (int k = 0; k < CMD_KNOTS; ++k) command_item_store(it[k], jt, x0, t0, horizon, b * CMD_KNOTS + k, v_filt, target_times, target_states);
  }
}
