// TEST INFRASTRUCTURE: the host build of the centroidal velocity-command target generator (wb_humanoid_mpc_amd/csrc/hsqp_cent_loop.h,
// k_command_targets_cent) with a one-lane Ctx, for tests/test_cent_loop.py and tests/cent_loop/cent_loop_sanitize.cpp.  Every array is the caller's,
// in the device layout.  Built with -ffp-contract=off: the arithmetic the device evaluates unfused.  The entries are declared in cent_loop_emu.h.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>

#include "hsqp_host.h"
#include "hsqp_cent_loop.h"

#include "cent_loop_emu.h"

using namespace hsqp;

extern "C" {

void* cl_create(const hsqp_model_desc* md, const double* default_joint_state, char* err, int errlen) {
  auto* dm = new DevModel;
  const std::string e = build_dev_model(*md, *dm);
  if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); delete dm; return nullptr; }
  dm->has_default_joint_state = 1;
  memcpy(dm->default_joint_state, default_joint_state, sizeof(dm->default_joint_state));
  return dm;
}
void cl_destroy(void* h) { delete static_cast<DevModel*>(h); }
double cl_total_mass(void* h) { return static_cast<DevModel*>(h)->total_mass; }

void cl_command_targets(void* h, double alpha, int B, const double* v_cmd, double* v_filt, const double* x0, double t0, double horizon, double* target_times,
                        double* target_states, double* base_vel) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  const Ctx ctx{0, 1, nullptr};
  auto ws = std::make_unique<CentWST<false>>();   // one workgroup's LDS
  for (size_t b = 0; b < (size_t)B; ++b)
    cent_command_targets_instance(ctx, dm, *ws, alpha, v_cmd + b * CMD_N, v_filt + b * CMD_N, x0 + b * NX, t0, horizon, target_times + b * CMD_KNOTS,
                                  target_states + b * CMD_KNOTS * NX, base_vel ? base_vel + b * 6 : nullptr);
}

}
