// TEST INFRASTRUCTURE: the host build of the policy rollout with external pushes (wb_humanoid_mpc_amd/csrc/hsqp_rollout.h, hsqp_push.h, k_rollout)
// with a one-lane context, for tests/test_push.py (compiled by the test with -ffp-contract=off, also with -DHSQP_EMU_REVERSE).  A shared library
// loaded through ctypes (the model image comes from the binding's hsqp_model_desc):
//   pe_create(desc, err, len) / pe_destroy(h)
//   pe_rollout(h, settings, N, dts [B][N] or null (uniform dt), dt, ut [B][N][35], K [B][count][35][58], uff [B][count][35], first, count, cent,
//              B, s0 [B], x0 [B][58], duration, n, n_pushes [B] or null (no table), pushes [B][max_pushes], max_pushes, stamp0 [B] or null
//              (first node at 0), x [B][n][58], u [B][n][35], status / steps / rejected [B])
//   pe_flow(h, x, u, n_push, pushes [n_push], xdot): the flow map of the handle's formulation with every given push active, xdot [58]
//   pe_ws_bytes(cent): sizeof of the rollout workspace (the kernel's LDS)
#include <cstring>
#include <memory>
#include <string>

#include "hsqp_host.h"
#include "hsqp_rollout.h"

using namespace hsqp;

template <class SW>
static void run(const DevModel& dm, const hsqp_rollout_settings* st, int N, const double* dts, double dt, const double* ut, const double* K,
                const double* uff, int first, int count, int cent, int B, const double* s0, const double* x0, double duration, int n,
                const PushTable& tbl, double* x, double* u, int32_t* status, int32_t* steps, int32_t* rejected) {
  // the workspace starts as NaN bit patterns, like the device's uninitialised LDS: a read of something never written shows
  std::unique_ptr<RolloutWS<SW>> w(new RolloutWS<SW>);
  std::memset(static_cast<void*>(w.get()), 0xFF, sizeof(RolloutWS<SW>));
  const Ctx ctx{0, 1, nullptr};
  for (int b = 0; b < B; ++b) {
    const RolloutPolicy p{ut + (size_t)b * N * NU, dts ? dts + (size_t)b * N : nullptr, N, dt, K ? K + (size_t)b * count * NU * NX : nullptr,
                          uff ? uff + (size_t)b * count * NU : nullptr, first, count, cent};
    rollout_instance(ctx, dm, *w, p, *st, s0[b], x0 + (size_t)b * NX, duration, n, x ? x + (size_t)b * n * NX : nullptr, u ? u + (size_t)b * n * NU : nullptr,
                     status + b, steps ? steps + b : nullptr, rejected ? rejected + b : nullptr, tbl, b);
  }
}

template <class SW>
static void flow(const DevModel& dm, const double* x, const double* u, int n_push, const hsqp_push* pushes, double* xdot) {
  std::unique_ptr<RolloutWS<SW>> w(new RolloutWS<SW>);
  std::memset(static_cast<void*>(w.get()), 0xFF, sizeof(RolloutWS<SW>));
  const Ctx ctx{0, 1, nullptr};
  // every push active from 0 for one second; the segment starts at 0
  std::unique_ptr<hsqp_push[]> tab(new hsqp_push[n_push > 0 ? n_push : 1]);
  for (int i = 0; i < n_push; ++i) { tab[i] = pushes[i]; tab[i].t_start = 0.0; tab[i].duration = 1.0; }
  const int32_t np = n_push;
  push_load(ctx, PushTable{&np, tab.get(), n_push > 0 ? n_push : 1, nullptr, 0}, 0, w->push);
  rollout_topology(ctx, dm, w->sw);
  rollout_flow(ctx, dm, w->sw, x, u, xdot);
  const unsigned mask = push_active(w->push, 0.0);
  if (mask) rollout_push(ctx, dm, w->sw, w->push, mask, xdot);
}

extern "C" {

void* pe_create(const hsqp_model_desc* md, char* err, int errlen) {
  auto* dm = new DevModel;
  const std::string e = build_dev_model(*md, *dm);
  if (!e.empty()) { snprintf(err, errlen, "%s", e.c_str()); delete dm; return nullptr; }
  return dm;
}
void pe_destroy(void* h) { delete static_cast<DevModel*>(h); }

void pe_rollout(void* h, const hsqp_rollout_settings* st, int N, const double* dts, double dt, const double* ut, const double* K, const double* uff, int first,
                int count, int cent, int B, const double* s0, const double* x0, double duration, int n, const int32_t* n_pushes, const hsqp_push* pushes,
                int max_pushes, const double* stamp0, double* x, double* u, int32_t* status, int32_t* steps, int32_t* rejected) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  const PushTable tbl{n_pushes, pushes, max_pushes, stamp0, 1};
  if (cent) run<CentWST<false>>(dm, st, N, dts, dt, ut, K, uff, first, count, cent, B, s0, x0, duration, n, tbl, x, u, status, steps, rejected);
  else run<StageWST<false>>(dm, st, N, dts, dt, ut, K, uff, first, count, cent, B, s0, x0, duration, n, tbl, x, u, status, steps, rejected);
}

void pe_flow(void* h, const double* x, const double* u, int n_push, const hsqp_push* pushes, double* xdot) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  if (dm.formulation == HSQP_FORM_CENTROIDAL) flow<CentWST<false>>(dm, x, u, n_push, pushes, xdot);
  else flow<StageWST<false>>(dm, x, u, n_push, pushes, xdot);
}

int pe_ws_bytes(int cent) { return cent ? (int)sizeof(RolloutWS<CentWST<false>>) : (int)sizeof(RolloutWS<StageWST<false>>); }

}  // extern "C"
