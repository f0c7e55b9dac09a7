// TEST INFRASTRUCTURE: a program of its own that takes the host build of the value-function kernels' source (tests/value/value_emu.cpp, compiled beside
// this file) through adversarial queries under -fsanitize=address,undefined (tests/test_value.py runs it as a child process; nothing is preloaded).
//   value_sanitize            prints "value ok" and returns 0
// Every array is a heap block of exactly its size, so a load or store outside the record or outside a query's outputs is the sanitizer's finding; the
// outputs of the neighbouring queries hold canaries that must survive.  Queries: on nodes, mid-interval, at both ends, far outside the horizon (1e300),
// on zero-length intervals of a padded event grid, N = 1, non-finite states, centroidal padding filled with NaN, each with every subset of the outputs.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

extern "C" int val_vf_size();
extern "C" void val_record(int B, int N, int k0, int k1, int cent, const double* vf, const double* xbar, double* S, double* s, double* xb);
extern "C" void val_eval(int B, int N, double dt, const double* dts, int cent, int n, const double* vf, const double* xbar, const double* s_query,
                         const double* x_query, double* dV, double* dfdx, double* dfdxx);

static const int NX = 58, CNX = 35;
static const double CANARY = -12345.678;
static int failures = 0;
#define EXPECT(cond)                                                           \
  do {                                                                         \
    if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static unsigned long long rng_state = 88172645463325252ull;
static double rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (double)(rng_state >> 11) / 9007199254740992.0; }

// one instance of N intervals; query 1 of three is the one evaluated (queries 0 and 2 keep their canaries); outputs chosen by the bits of `which`
static void one(int N, const double* dts_in, int cent, double sq, const std::vector<double>& xq_in, int which, bool expect_finite) {
  const size_t VF = (size_t)val_vf_size();
  double* vf = new double[(size_t)(N + 1) * VF];
  double* xbar = new double[(size_t)(N + 1) * NX];
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t i = 0; i < (size_t)(N + 1) * VF; ++i) vf[i] = rnd() - 0.5;
  for (size_t i = 0; i < (size_t)(N + 1) * NX; ++i) xbar[i] = rnd() - 0.5;
  if (cent)   // the padding of a centroidal record is never read into a result
    for (int k = 0; k <= N; ++k) {
      for (int r = 0; r < NX; ++r)
        for (int c = 0; c < NX; ++c)
          if (r >= CNX || c >= CNX) vf[k * VF + r * NX + c] = nan;
      for (int r = CNX; r < NX; ++r) { vf[k * VF + NX * NX + r] = nan; xbar[k * NX + r] = nan; }
    }
  double* dts = dts_in ? new double[N] : nullptr;
  for (int i = 0; dts && i < N; ++i) dts[i] = dts_in[i];
  double* s = new double[1]{sq};
  double* xq = new double[NX];
  for (int i = 0; i < NX; ++i) xq[i] = xq_in[i];
  double* dV = new double[3]{CANARY, CANARY, CANARY};
  double* g = new double[3 * NX];
  double* H = new double[3 * NX * NX];
  for (int i = 0; i < 3 * NX; ++i) g[i] = CANARY;
  for (int i = 0; i < 3 * NX * NX; ++i) H[i] = CANARY;
  val_eval(1, N, 0.02, dts, cent, 1, vf, xbar, s, xq, (which & 1) ? dV + 1 : nullptr, (which & 2) ? g + NX : nullptr, (which & 4) ? H + NX * NX : nullptr);
  EXPECT(dV[0] == CANARY && dV[2] == CANARY);
  for (int i = 0; i < NX; ++i) EXPECT(g[i] == CANARY && g[2 * NX + i] == CANARY);
  for (int i = 0; i < NX * NX; ++i) EXPECT(H[i] == CANARY && H[2 * NX * NX + i] == CANARY);
  EXPECT((which & 1) ? dV[1] != CANARY : dV[1] == CANARY);
  for (int i = 0; i < NX; ++i) EXPECT((which & 2) ? g[NX + i] != CANARY : g[NX + i] == CANARY);
  if (which & 4)
    for (int r = 0; r < NX; ++r)
      for (int c = 0; c < NX; ++c) {
        const double v = H[NX * NX + r * NX + c];
        EXPECT(std::isfinite(v) && v == H[NX * NX + c * NX + r]);                 // S never depends on the query state; symmetric
        if (cent && (r >= CNX || c >= CNX)) EXPECT(v == 0.0);
      }
  if (expect_finite) {
    if (which & 1) EXPECT(std::isfinite(dV[1]));
    for (int i = 0; (which & 2) && i < NX; ++i) EXPECT(std::isfinite(g[NX + i]));
    for (int i = CNX; cent && (which & 2) && i < NX; ++i) EXPECT(g[NX + i] == 0.0);
  } else {
    if (which & 1) EXPECT(!std::isfinite(dV[1]));
  }
  // the record of every node through the same source
  double* S = new double[(size_t)(N + 1) * NX * NX];
  double* sv = new double[(size_t)(N + 1) * NX];
  double* xb = new double[(size_t)(N + 1) * NX];
  val_record(1, N, 0, N, cent, vf, xbar, S, sv, xb);
  for (int k = 0; k <= N; ++k)
    for (int r = 0; r < NX; ++r) {
      const bool pad = cent && r >= CNX;
      EXPECT(pad ? sv[k * NX + r] == 0.0 : sv[k * NX + r] == vf[k * VF + NX * NX + r]);
      for (int c = 0; c < NX; ++c) EXPECT(S[(k * NX + r) * NX + c] == S[(k * NX + c) * NX + r] && std::isfinite(S[(k * NX + r) * NX + c]));
    }
  val_record(1, N, N, N, cent, vf, xbar, nullptr, sv, nullptr);
  delete[] vf; delete[] xbar; delete[] dts; delete[] s; delete[] xq; delete[] dV; delete[] g; delete[] H; delete[] S; delete[] sv; delete[] xb;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> x(NX);
  for (double& v : x) v = rnd() - 0.5;
  const double grid[8] = {0.02, 0.0, 0.02, 0.013, 0.0, 0.0, 0.0, 0.007};   // an event, and a run of three zero-length intervals in front of the last one
  const double offsets[] = {0.0, 0.02, 0.03, 0.04, 0.053, 0.0531, 0.06, 0.16, 1.0, -1.0, 1e300, -1e300, 5e-324};
  for (int cent = 0; cent < 2; ++cent)
    for (int which = 0; which < 8; ++which)
      for (double sq : offsets) {
        one(8, nullptr, cent, sq, x, which, true);
        one(8, grid, cent, sq, x, which, true);
        one(1, nullptr, cent, sq, x, which, true);
        one(1, grid + 7, cent, sq, x, which, true);
        one(2, grid, cent, sq, x, which, true);
      }
  // non-finite query states: non-finite outputs for that query, nothing outside it
  for (int cent = 0; cent < 2; ++cent)
    for (double bad : {nan, inf, -inf}) {
      std::vector<double> xb = x;
      xb[3] = bad;
      one(8, grid, cent, 0.03, xb, 7, false);
      xb = x;
      xb[NX - 1] = bad;                      // whole-body: a live state; centroidal: padding, which does not count
      one(8, nullptr, cent, 0.03, xb, 7, cent != 0);
    }
  // a random sweep
  for (int c = 0; c < 300; ++c) {
    const int N = 1 + (int)(rnd() * 12);
    std::vector<double> dts(N);
    for (double& d : dts) d = rnd() < 0.3 ? 0.0 : 0.005 + 0.03 * rnd();
    dts[N - 1] = 0.01;
    one(N, rnd() < 0.5 ? dts.data() : nullptr, c & 1, -0.1 + rnd() * (0.03 * N + 0.2), x, 1 + (int)(rnd() * 7), true);
  }
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("value ok\n");
  return 0;
}
