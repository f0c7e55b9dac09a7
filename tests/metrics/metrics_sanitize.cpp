// TEST INFRASTRUCTURE: a program of its own that takes the host build of the episode metrics (tests/metrics/metrics_emu.cpp, compiled beside this file)
// through every path, for a run under the address and undefined-behaviour sanitizers (tests/test_metrics.py).
//   metrics_sanitize DESC_FILE     DESC_FILE: the bytes of the binding's hsqp_model_desc
// B = 1 and B = 5; the three kernel forms; the torque group with finite and infinite limits; NaN and infinite states, performance indices and
// records of the actuator; under isolation a failure of every cause, a parked instance, the host's closing of chosen and of all records, and the
// closing of an empty record.  Every array is exactly as long as the kernel may read or write, so an access past an end is seen.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#define ROLLOUT_EMU_DECLARATIONS_ONLY
#include "../rollout/rollout_emu.h"
#include "metrics_emu.h"

namespace {

const int NX = HSQP_NX, NJ = HSQP_NJ;
const double kNaN = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

struct Batch {
  int B;
  std::vector<hsqp_metrics> rec;
  std::vector<int32_t> feet, it_status, ro_status, ep_state, steps, rejected;
  std::vector<hsqp_perf> perf;
  std::vector<double> xs, x_before, cmd, act, limit;
  explicit Batch(int B_)
      : B(B_), rec(2 * B_), feet(2 * B_, 9), it_status(B_, 0), ro_status(B_, 0), ep_state(B_, 0), steps(B_, 7), rejected(B_, 1), perf(B_), xs((size_t)B_ * NX),
        x_before((size_t)B_ * NX), cmd((size_t)B_ * 4), act((size_t)B_ * 3 * NJ), limit(NJ) {
    met_open(B, rec.data(), feet.data());
  }
  // a standing state per instance, cycle c: the base a little lower every cycle, so that the soles meet the ground at z = 0 on the way
  void fill(int c) {
    for (int b = 0; b < B; ++b) {
      for (int i = 0; i < NX; ++i) { x_before[(size_t)b * NX + i] = xs[(size_t)b * NX + i]; xs[(size_t)b * NX + i] = 0.01 * ((i * 7 + b * 3 + c) % 11 - 5); }
      xs[(size_t)b * NX + 2] = 0.80 - 0.01 * c;
      for (int i = 0; i < 4; ++i) cmd[(size_t)b * 4 + i] = i == 2 ? 0.78 : 0.1 * (i + b);
      for (int i = 0; i < 3 * NJ; ++i) act[(size_t)b * 3 * NJ + i] = 0.3 * ((i + b + c) % 9 - 4);
      perf[b] = hsqp_perf{1.0 + c, 2.0 + b, 1e-3, 1e-4};
      it_status[b] = 0; ro_status[b] = HSQP_ROLLOUT_OK;
    }
  }
  met_call call(int c, int form, bool isolate, bool torque, const hsqp_episode_settings* st, const hsqp_contact_settings* cs, const hsqp_contact_ground* g) {
    met_call k = {};
    k.B = B; k.isolate = isolate ? 1 : 0; k.cycle = c; k.form = form; k.period = 1.0 / 60.0;
    k.st = isolate ? st : nullptr; k.ep_state = isolate ? ep_state.data() : nullptr;
    k.it_status = it_status.data(); k.perf = perf.data(); k.ro_status = ro_status.data();
    k.xs = xs.data(); k.x_before = x_before.data(); k.cmd = cmd.data(); k.steps = steps.data(); k.rejected = rejected.data();
    k.act_last = torque ? act.data() : nullptr; k.act_limit = torque ? limit.data() : nullptr;
    k.rec = rec.data(); k.feet = feet.data(); k.contact = form ? cs : nullptr; k.ground = form ? g : nullptr;
    return k;
  }
};

bool run(void* h, int B) {
  bool ok = true;
  hsqp_contact_settings cs = {};
  cs.enabled = 1; cs.stiffness = 5e4; cs.damping = 10.0; cs.mu = 0.6; cs.slip_velocity = 0.01; cs.ground_height = 0.0;
  std::vector<hsqp_contact_ground> ground(B);
  for (int b = 0; b < B; ++b) ground[b] = hsqp_contact_ground{0.001 * b, 0.5};
  hsqp_episode_settings st = {};
  st.on_failure = HSQP_EPISODE_RESET; st.min_base_height = 0.5; st.max_base_height = 1.0; st.max_tilt = 0.5;
  for (int form = 0; form < 3; ++form) {
    Batch bt(B);
    // without isolation: every instance accumulates; finite, then infinite limits
    for (int c = 0; c < 12; ++c) {
      bt.fill(c);
      for (int j = 0; j < NJ; ++j) bt.limit[j] = c < 6 ? 0.5 : (j % 2 ? kInf : 0.0);
      const met_call k = bt.call(c, form, false, c % 4 != 3, nullptr, &cs, c % 2 ? ground.data() : nullptr);
      met_cycle(h, &k);
    }
    for (int b = 0; b < B; ++b) {
      const hsqp_metrics& r = bt.rec[2 * b];
      ok = ok && r.cycles == 12 && r.first_cycle == 0 && r.end_cause == HSQP_METRICS_END_OPEN && r.torque_samples == 9 && r.ground_samples == (form ? 12 : 0);
      ok = ok && std::isfinite(r.vel_err_sq) && std::isfinite(r.load_sum) && r.rollout_steps == 12 * 7 && bt.rec[2 * b + 1].cycles == 0;
    }
    // under isolation: sick data of every kind in the last instance, one cause per cycle; PARK in the second half
    for (int c = 12; c < 24; ++c) {
      bt.fill(c - 12);
      if (c == 18) { st.on_failure = HSQP_EPISODE_PARK; }
      const int sick = B - 1, kind = c % 6;
      double* xs = bt.xs.data() + (size_t)sick * NX;
      if (kind == 0) bt.it_status[sick] = 3;
      if (kind == 1) bt.perf[sick].cost = kNaN;
      if (kind == 2) bt.ro_status[sick] = HSQP_ROLLOUT_MAX_STEPS;
      if (kind == 3) xs[NX - 1] = kInf;
      if (kind == 4) xs[2] = 1.2;
      if (kind == 5) { bt.act[(size_t)sick * 3 * NJ] = kNaN; bt.act[(size_t)sick * 3 * NJ + NJ + 1] = -kInf; }   // (no failure: NaN goes into the sums)
      const met_call k = bt.call(c, form, true, true, &st, &cs, ground.data());
      met_cycle(h, &k);
      const bool failed = kind < 5;
      if (failed && st.on_failure == HSQP_EPISODE_PARK) bt.ep_state[sick] = HSQP_EP_FAILED_BOUNDS;      // what the triage would leave
      ok = ok && (!failed || bt.rec[2 * sick].cycles == 0);
    }
    st.on_failure = HSQP_EPISODE_RESET;
    ok = ok && bt.rec[2 * (B - 1)].cycles == 0 && bt.rec[2 * (B - 1) + 1].end_cause > 0;     // parked: nothing accumulated; the last closed record: a failure's
    // the host: chosen instances (twice: the second closes empty records), then all
    const int32_t ids[2] = {0, B - 1};
    for (int twice = 0; twice < 2; ++twice) met_host_close(B > 1 ? 2 : 1, ids, bt.rec.data(), bt.feet.data());
    if (B > 1) ok = ok && bt.rec[0].cycles == 0 && bt.rec[1].end_cause == HSQP_METRICS_END_HOST && bt.rec[1].cycles == 24;
    else ok = ok && bt.rec[0].cycles == 0 && bt.rec[1].end_cause == HSQP_EP_FAILED_NUMERIC && bt.rec[1].cycles == 1;   // (its record was empty: the failure's stays)
    met_host_close(B, nullptr, bt.rec.data(), bt.feet.data());
    for (int b = 0; b < B; ++b) ok = ok && bt.rec[2 * b].cycles == 0 && bt.rec[2 * b].first_cycle == -1 && bt.rec[2 * b].height_min == kInf && bt.feet[2 * b] == 0;
    if (!ok) { fprintf(stderr, "B = %d, form %d\n", B, form); return false; }
  }
  return ok && met_ws_bytes(2) <= 65536;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: metrics_sanitize DESC_FILE\n"); return 2; }
  std::vector<char> image(sizeof(hsqp_model_desc));
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(image.data(), 1, image.size(), f) != image.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  fclose(f);
  char err[256] = "";
  void* h = emu_create(reinterpret_cast<const hsqp_model_desc*>(image.data()), err, sizeof err);
  if (!h) { fprintf(stderr, "%s\n", err); return 1; }
  const bool ok = run(h, 1) && run(h, 5);
  emu_destroy(h);
  printf(ok ? "metrics ok\n" : "metrics FAILED\n");
  return ok ? 0 : 1;
}
