// TEST INFRASTRUCTURE: the host build of the episode metrics of the resident loop (wb_humanoid_mpc_amd/csrc/hsqp_metrics.h: k_loop_metrics,
// k_metrics_host_close) with a one-lane context, for tests/test_metrics.py and tests/metrics/metrics_sanitize.cpp (compiled with -ffp-contract=off,
// also with -DHSQP_EMU_REVERSE).  A shared library loaded through ctypes, or linked into a program; every array is the caller's, in the device
// layout.  The model image comes through the shared entries of tests/rollout/rollout_emu.h (emu_create / emu_destroy).
//   met_open(B, rec, feet)                      2 B empty records, the feet's flags zeroed (what hsqp_loop_metrics_enable uploads)
//   met_cycle(h, call)                          one launch of k_loop_metrics over B instances: form 0 no ground, 1 the plane (ContactSet), 2 a terrain
//                                               set with every instance on the plane (map = -1: ContactTerrainSet)
//   met_host_close(n, ids or null, rec, feet)   one launch of k_metrics_host_close
//   met_ws_bytes(form)                          sizeof of the kernel's workspace (its LDS)
#include "metrics_emu.h"

#include "../rollout/rollout_emu.h"
#include "hsqp_metrics.h"

static const Ctx kMetLane{0, 1, nullptr};

static MetricsArgs args_of(const met_call* c) {
  MetricsArgs a{};
  a.isolate = c->isolate; a.cycle = c->cycle; a.period = c->period;
  if (c->st) a.st = *c->st;
  a.it_status = c->it_status; a.perf = c->perf; a.ro_status = c->ro_status;
  a.xs = c->xs; a.x_before = c->x_before; a.cmd = c->cmd; a.ep_state = c->ep_state;
  a.steps = c->steps; a.rejected = c->rejected;
  a.act_last = c->act_last; a.act_limit = c->act_limit;
  a.rec = c->rec; a.feet = c->feet;
  return a;
}

template <class CT>
static void run_form(const DevModel& dm, const met_call* c, const ContactParams& cp, const TerrainParams* tp) {
  auto w = fresh<MetricsWST<CT>>();
  const MetricsArgs a = args_of(c);
  for (int b = 0; b < c->B; ++b) metrics_instance<CT>(kMetLane, dm, *w, a, cp, tp, b);
}

extern "C" {

void met_open(int B, hsqp_metrics* rec, int32_t* feet) {
  for (int b = 0; b < B; ++b)
    for (int r = 0; r < 2; ++r) metrics_open(kMetLane, rec + 2 * b + r, feet + 2 * b);
}

void met_cycle(void* h, const met_call* c) {
  const DevModel& dm = *static_cast<DevModel*>(h);
  std::vector<hsqp_contact_ground> ground((size_t)c->B);
  ContactParams cp{nullptr, 0.0, 0.0, 0.0};
  if (c->form) {
    contact_fill_ground(*c->contact, c->ground, (size_t)c->B, (size_t)c->B, ground.data());
    cp = ContactParams{ground.data(), c->contact->stiffness, c->contact->damping, c->contact->slip_velocity};
  }
  if (c->form == 0) run_form<MetricsNoGround>(dm, c, cp, nullptr);
  else if (c->form == 1) run_form<ContactSet>(dm, c, cp, nullptr);
  else {
    std::vector<hsqp_terrain_placement> place((size_t)c->B);
    terrain_fill_place(nullptr, 0, place.size(), place.data());
    const TerrainParams tp{nullptr, nullptr, place.data(), 0};
    run_form<ContactTerrainSet>(dm, c, cp, &tp);
  }
}

void met_host_close(int n, const int32_t* ids, hsqp_metrics* rec, int32_t* feet) {
  for (int i = 0; i < n; ++i) metrics_host_close(kMetLane, ids, rec, feet, i);
}

int met_ws_bytes(int form) {
  return form == 0 ? (int)sizeof(MetricsWST<MetricsNoGround>) : (form == 1 ? (int)sizeof(MetricsWST<ContactSet>) : (int)sizeof(MetricsWST<ContactTerrainSet>));
}

}  // extern "C"
