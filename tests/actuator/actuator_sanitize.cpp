// TEST INFRASTRUCTURE: a program of its own that takes the host build of the actuator model (tests/actuator/actuator_emu.cpp, compiled beside this file)
// through one held RK4 rollout and the record write, for a run under the address and undefined-behaviour sanitizers (tests/test_actuator.py).
//   actuator_sanitize DESC_FILE     DESC_FILE: the bytes of the binding's hsqp_model_desc
// The policy is weight compensation at a standing state, two instances, a command period that puts a sample inside a hold interval.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#define ROLLOUT_EMU_DECLARATIONS_ONLY
#include "../rollout/rollout_emu.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: actuator_sanitize DESC_FILE\n"); return 2; }
  std::vector<char> image(sizeof(hsqp_model_desc));
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(image.data(), 1, image.size(), f) != image.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  fclose(f);
  char err[256] = "";
  void* h = emu_create(reinterpret_cast<const hsqp_model_desc*>(image.data()), err, sizeof err);
  if (!h) { fprintf(stderr, "%s\n", err); return 1; }
  const int N = 4, B = 2, n = 2, NX = HSQP_NX, NU = HSQP_NU, NJ = HSQP_NJ;
  std::vector<double> xt((size_t)B * (N + 1) * NX, 0.0), ut((size_t)B * N * NU, 0.0), x0((size_t)B * NX, 0.0);
  for (int b = 0; b < B; ++b) {
    for (int k = 0; k <= N; ++k) xt[((size_t)b * (N + 1) + k) * NX + 2] = 0.75;
    for (int k = 0; k < N; ++k) ut[((size_t)b * N + k) * NU + 2] = ut[((size_t)b * N + k) * NU + 8] = 170.0;
    x0[(size_t)b * NX + 2] = 0.75;
    x0[(size_t)b * NX + 6 + 3] = 0.2 * (b + 1);       // a bent knee: the joint law has something to pull on
  }
  hsqp_plant_settings ps = {};
  ps.kind = HSQP_PLANT_TORQUE; ps.lookahead = 0.005;
  hsqp_actuator_settings as = {};
  as.enabled = 1; as.command_period = 0.003; as.friction_velocity = 0.01;
  for (int j = 0; j < NJ; ++j) { ps.kp[j] = 100.0; ps.kd[j] = 2.0; ps.armature[j] = 0.01; as.effort_limit[j] = 5.0; as.damping[j] = 0.05; as.friction[j] = 0.1; }
  const hsqp_rollout_settings st = {HSQP_ROLLOUT_RK4, HSQP_ROLLOUT_FEEDFORWARD, 1e-5, 1e-3, 0.004, 10000.0};
  const double s0[2] = {0.0, 0.003};
  std::vector<double> x((size_t)B * n * NX), u((size_t)B * n * NU), last((size_t)B * 3 * NJ);
  int32_t status[2], steps[2], rejected[2];
  emu_rollout_call c = {};
  c.ut = ut.data(); c.xt = xt.data(); c.dt = 0.01; c.N = N; c.B = B; c.st = &st; c.s0 = s0; c.x0 = x0.data(); c.duration = 1.0 / 64.0; c.n = n;
  c.x = x.data(); c.u = u.data(); c.status = status; c.steps = steps; c.rejected = rejected; c.last = last.data(); c.plant = &ps; c.actuator = &as;
  emu_rollout(h, &c);
  emu_destroy(h);
  bool ok = true;
  for (int b = 0; b < B; ++b) ok = ok && status[b] == HSQP_ROLLOUT_OK && steps[b] >= 6;
  for (double v : x) ok = ok && std::isfinite(v);
  for (double v : last) ok = ok && std::isfinite(v);
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < NJ; ++j) ok = ok && std::fabs(last[((size_t)b * 3 + 1) * NJ + j]) <= 5.0;
  printf(ok ? "actuator ok\n" : "actuator FAILED\n");
  return ok ? 0 : 1;
}
