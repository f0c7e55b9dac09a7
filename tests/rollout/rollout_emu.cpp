// TEST INFRASTRUCTURE: the host build of the policy rollout (wb_humanoid_mpc_amd/csrc/hsqp_rollout.h, k_rollout) with a one-lane context, for
// tests/test_rollout.py.  A shared library loaded through ctypes (the model image comes from the binding's hsqp_model_desc):
//   ro_create(desc, err, len) / ro_destroy(h)
//   ro_rollout(h, settings, N, dts [B][N] or null (uniform dt), dt, ut [B][N][35], K [B][count][35][58], uff [B][count][35], first, count, cent,
//              B, s0 [B], x0 [B][58], duration, n, x [B][n][58], u [B][n][35], status / steps / rejected [B])
//   ro_flow(h, x, u, xdot): the flow map of the handle's formulation, xdot [58]
#include <cstring>
#include <memory>
#include <string>

#include "hsqp_host.h"
#include "hsqp_rollout.h"

using namespace hsqp;

template <class SW>
static void run(const DevModel& dm, const hsqp_rollout_settings* st, int N, const double* dts, double dt, const double* ut, const double* K,
                const double* uff, int first, int count, int cent, int B, const double* s0, const double* x0, double duration, int n, double* x, double* u,
                int32_t* status, int32_t* steps, int32_t* rejected) {
  // the workspace starts as NaN bit patterns, like the device's uninitialised LDS: a read of something never written shows
  std::unique_ptr<RolloutWS<SW>> w(new RolloutWS<SW>);
  std::memset(static_cast<void*>(w.get()), 0xFF, sizeof(RolloutWS<SW>));
  const Ctx ctx{0, 1, nullptr};
  for (int b = 0; b < B; ++b) {
    const RolloutPolicy p{ut + (size_t)b * N * NU, dts ? dts + (size_t)b * N : nullptr, N, dt, K ? K + (size_t)b * count * NU * NX : nullptr,
                          uff ? uff + (size_t)b * count * NU : nullptr, first, count, cent};
    rollout_instance(ctx, dm, *w, p, *st, s0[b], x0 + (size_t)b * NX, duration, n, x ? x + (size_t)b * n * NX : nullptr, u ? u + (size_t)b * n * NU : nullptr,
                     status + b, steps ? steps + b : nullptr, rejected ? rejected + b : nullptr);
  }
}

extern "C" {

void* ro_create(const hsqp_model_desc* md, char* err, int errlen) {
  auto* dm = new DevModel;
  const std::string e = build_dev_model(*md, *dm);
  if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); delete dm; return nullptr; }
  return dm;
}
void ro_destroy(void* h) { delete static_cast<DevModel*>(h); }

void ro_rollout(void* h, const hsqp_rollout_settings* st, int N, const double* dts, double dt, const double* ut, const double* K, const double* uff, int first,
                int count, int cent, int B, const double* s0, const double* x0, double duration, int n, double* x, double* u, int32_t* status, int32_t* steps,
                int32_t* rejected) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  if (cent) run<CentWST<false>>(dm, st, N, dts, dt, ut, K, uff, first, count, cent, B, s0, x0, duration, n, x, u, status, steps, rejected);
  else run<StageWST<false>>(dm, st, N, dts, dt, ut, K, uff, first, count, cent, B, s0, x0, duration, n, x, u, status, steps, rejected);
}

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
