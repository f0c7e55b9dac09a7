// TEST INFRASTRUCTURE: the host build of the policy rollout (wb_humanoid_mpc_amd/csrc/hsqp_rollout.h) with a one-lane context, for
// tests/test_rollout.py.  A shared library loaded through ctypes: the shared entries of tests/rollout/rollout_emu.h, and
//   ro_flow(h, x, u, xdot): the flow map of the handle's formulation, xdot [58]
#include "rollout_emu.h"

extern "C" {

void ro_flow(void* h, const double* x, const double* u, double* xdot) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  const Ctx ctx{0, 1, nullptr};
  if (dm.formulation == HSQP_FORM_CENTROIDAL) {
    auto w = std::make_unique<CentWST<false>>();
    rollout_topology(ctx, dm, *w);
    rollout_flow(ctx, dm, *w, x, u, xdot);
  } else {
    auto w = std::make_unique<StageWST<false>>();
    rollout_topology(ctx, dm, *w);
    rollout_flow(ctx, dm, *w, x, u, xdot);
  }
}

}  // extern "C"
