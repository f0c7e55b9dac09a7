// TEST INFRASTRUCTURE: a program of its own that takes the host build of the event-node grid builder (tests/grid/grid_emu.cpp, compiled beside this file)
// through adversarial inputs under -fsanitize=address,undefined (tests/test_grid.py runs it as a child process; nothing is preloaded).
//   grid_sanitize            prints "grid ok" and returns 0
// Every output array is a heap block of exactly its size, so a store outside an instance's rows is the sanitizer's finding; the rows of the
// neighbouring instances hold canaries that must survive.  Inputs: sorted schedules, unsorted and non-finite event arrays, events within dt_min of
// t0 and of a regular node, n_events outside [0, max_events], event_nodes = 0, times so large that t + dt == t, overflow by one interval.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/hsqp_grid.h"

extern "C" int gr_build(int B, double t0, int n_nodes, double dt, double dt_min, int event_nodes, int max_events, const int* n_events, const double* event_times,
                        int* n_intervals, double* dt_nodes, double* node_times, int* status);

static const double CANARY = -12345.678;
static int failures = 0;
#define EXPECT(cond)                                                           \
  do {                                                                         \
    if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

// instance 1 of three is the one built: instances 0 and 2 keep their canaries
static int one(double t0, int n_nodes, double dt, double dt_min, int event_nodes, int max_events, int n_events, const std::vector<double>& events, int* nb_out = nullptr) {
  const size_t N = (size_t)n_nodes + event_nodes, E = max_events;
  int* ne = new int[1]{n_events};
  double* ev = new double[E];
  for (size_t i = 0; i < E; ++i) ev[i] = i < events.size() ? events[i] : 0.0;
  int* ni = new int[3]{-7, -7, -7};
  int* st = new int[3]{-7, -7, -7};
  double* dts = new double[3 * N];
  double* nts = new double[3 * (N + 1)];
  for (size_t i = 0; i < 3 * N; ++i) dts[i] = CANARY;
  for (size_t i = 0; i < 3 * (N + 1); ++i) nts[i] = CANARY;
  gr_build(1, t0, n_nodes, dt, dt_min, event_nodes, max_events, ne, ev, ni + 1, dts + N, nts + (N + 1), st + 1);
  for (size_t i = 0; i < N; ++i) EXPECT(dts[i] == CANARY && dts[2 * N + i] == CANARY);
  for (size_t i = 0; i <= N; ++i) EXPECT(nts[i] == CANARY && nts[2 * (N + 1) + i] == CANARY);
  EXPECT(ni[0] == -7 && ni[2] == -7 && st[0] == -7 && st[2] == -7);
  const int status = st[1], nb = ni[1];
  EXPECT(status == HSQP_GRID_OK || status == HSQP_GRID_OVERFLOW);
  // whatever the status, the rows are fully written; with finite t0 and dt they are finite and non-negative
  if (std::isfinite(t0) && std::fabs(t0) < 1e12 && dt_min >= 0.0 && dt > dt_min) {   // (what the host checks before it launches the builder)
    for (size_t i = 0; i < N; ++i) EXPECT(std::isfinite(dts[N + i]) && dts[N + i] >= 0.0);
    for (size_t i = 0; i < N; ++i) EXPECT(nts[(N + 1) + i + 1] >= nts[(N + 1) + i] - 1.0001e-9);   // (a post-event node's epsilon: the only step back)
  }
  if (status == HSQP_GRID_OK) {
    EXPECT(nb >= 1 && nb <= (int)N && dts[N + N - 1] > 0.0);
    for (int k = nb - 1; k < (int)N - 1; ++k) EXPECT(dts[N + k] == 0.0);
  } else {
    EXPECT(nb == 0);
  }
  if (nb_out) *nb_out = nb;
  delete[] ne; delete[] ev; delete[] ni; delete[] st; delete[] dts; delete[] nts;
  return status;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double dt = 0.035, dm = 1e-4;
  int nb = 0;
  // sorted schedules
  EXPECT(one(0.0, 12, dt, dm, 6, 8, 0, {}, &nb) == HSQP_GRID_OK && nb == 12);
  EXPECT(one(0.2, 12, dt, dm, 6, 8, 3, {0.25, 0.3, 0.5}, &nb) == HSQP_GRID_OK && nb >= 14);
  EXPECT(one(0.2, 12, dt, dm, 6, 8, 1, {0.2 + 5e-5}, &nb) == HSQP_GRID_OK && nb == 13);              // the first interval is the event
  EXPECT(one(0.2, 12, dt, dm, 6, 8, 1, {0.2 + 3 * dt + 5e-5}, &nb) == HSQP_GRID_OK);                  // an event replaces a regular node
  EXPECT(one(0.2, 12, dt, dm, 0, 8, 0, {}, &nb) == HSQP_GRID_OK && nb == 12);                         // event_nodes = 0
  EXPECT(one(0.2, 12, dt, dm, 0, 8, 1, {0.3}) == HSQP_GRID_OVERFLOW);
  EXPECT(one(0.2, 12, dt, dm, 1, 8, 2, {0.3, 0.4}) == HSQP_GRID_OVERFLOW);                            // overflow by intervals
  EXPECT(one(0.2, 1, dt, dm, 0, 1, 0, {}, &nb) == HSQP_GRID_OK && nb == 1);
  // unsorted, non-finite, duplicated
  one(0.2, 12, dt, dm, 6, 8, 4, {0.5, 0.3, 0.4, 0.25});
  one(0.2, 12, dt, dm, 6, 8, 4, {nan, 0.3, inf, -inf});
  one(0.2, 12, dt, dm, 6, 8, 8, {nan, nan, nan, nan, nan, nan, nan, nan});
  one(0.2, 12, dt, dm, 6, 8, 3, {0.3, 0.3, 0.3});
  one(0.2, 12, dt, dm, 40, 64, 64, std::vector<double>(64, 0.3));
  one(0.2, 12, dt, dm, 6, 8, 8, {0.6, 0.55, 0.5, 0.45, 0.4, 0.35, 0.3, 0.25});
  // n_events outside [0, max_events]: clamped
  one(0.2, 12, dt, dm, 6, 4, 1000000, {0.25, 0.3, 0.35, 0.4});
  one(0.2, 12, dt, dm, 6, 4, -5, {0.25, 0.3, 0.35, 0.4});
  // times the step cannot move, non-finite times
  EXPECT(one(1e20, 12, dt, dm, 6, 8, 0, {}) == HSQP_GRID_OVERFLOW);
  one(1e15, 12, dt, dm, 6, 8, 1, {1e15 + 0.125});
  one(nan, 12, dt, dm, 6, 8, 1, {0.3});
  one(inf, 12, dt, dm, 6, 8, 1, {0.3});
  one(0.2, 12, nan, dm, 6, 8, 1, {0.3});
  one(0.2, 12, dt, nan, 6, 8, 1, {0.3});
  one(0.2, 12, dt, 1.0, 6, 8, 1, {0.3});                                                               // dt < dt_min (the host refuses it)
  one(0.2, 12, 0.0, 0.0, 6, 8, 1, {0.3});
  one(0.2, 12, -dt, dm, 6, 8, 1, {0.3});
  // a long random sweep
  unsigned long long s = 88172645463325252ull;
  auto rnd = [&s]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0; };
  for (int c = 0; c < 4000; ++c) {
    const int n_nodes = 1 + (int)(rnd() * 20), event_nodes = (int)(rnd() * 8), E = 1 + (int)(rnd() * 10);
    std::vector<double> ev(E);
    const double t0 = rnd() * 10.0;
    for (double& e : ev) e = rnd() < 0.05 ? nan : t0 - 0.2 + rnd() * (n_nodes * dt + 0.4);
    one(t0, n_nodes, dt, dm, event_nodes, E, (int)(rnd() * (E + 2)) - 1, ev);
  }
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("grid ok\n");
  return 0;
}
