// TEST INFRASTRUCTURE: a program of its own that takes the host build of the per-foot swing heights (tests/perceive/perceive_emu.cpp, compiled beside this
// file) to the edges of its index arithmetic, for a run under the address and undefined-behaviour sanitizers (tests/test_perceive.py): states at NaN and
// +-1e300, an all-swing schedule, n_events equal to max_events, n_events outside its range (as an array that came through the _device entry could hold),
// maps of the minimum size (2 x 2) and of the maximum size (HSQP_TERRAIN_MAX_DIM), a placement whose map index is out of range.  Every array is on the
// heap and exactly as long as the layout says: a read or write past it is the sanitizer's to see.  A finite state gives finite rows; a non-finite one NaN.
//   perceive_sanitize DESC_FILE     DESC_FILE: the bytes of the binding's hsqp_model_desc
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "perceive_emu.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: perceive_sanitize DESC_FILE\n"); return 2; }
  std::vector<char> image(sizeof(hsqp_model_desc));
  FILE* fp = fopen(argv[1], "rb");
  if (!fp || fread(image.data(), 1, image.size(), fp) != image.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  fclose(fp);
  char err[256] = "";
  const std::vector<double> joints(HSQP_NX, 0.1);   // (more than the joints there are: pc_create copies the model's count)
  void* h = pc_create(reinterpret_cast<const hsqp_model_desc*>(image.data()), joints.data(), err, sizeof err);
  if (!h) { fprintf(stderr, "%s\n", err); return 1; }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  constexpr int E = 4, K = 3, NXS = HSQP_NX, B = 6;
  // the maps: 2 x 2 and HSQP_TERRAIN_MAX_DIM squared
  const int D = HSQP_TERRAIN_MAX_DIM;
  const std::vector<int32_t> nx = {2, D}, ny = {2, D};
  const std::vector<double> cell = {0.5, 0.01};
  std::vector<double> heights = {0.0, 0.1, 0.2, 0.4};
  for (int i = 0; i < D * D; ++i) heights.push_back(0.001 * (i % 97));
  // states: the zero configuration, +-1e300 in the planar position, 1e300 in a joint and in the yaw, NaN
  std::vector<double> x((size_t)B * NXS, 0.0);
  for (int b = 0; b < B; ++b) x[(size_t)b * NXS + 2] = 0.8;
  x[1 * NXS + 0] = 1e300; x[1 * NXS + 1] = -1e300;
  x[2 * NXS + 0] = -1e300; x[2 * NXS + 3] = 1e300;
  x[3 * NXS + 9] = 1e300;
  x[4 * NXS + 7] = nan;
  const std::vector<double> ground(B, 0.25);
  const int FLY = 0, RF = 1, LF = 2, STANCE = 3;
  struct Sched { const char* name; std::vector<int> ne; std::vector<int> seq; };
  const std::vector<Sched> scheds = {
      {"walk", std::vector<int>(B, 3), {STANCE, LF, RF, STANCE, STANCE}},
      {"all swing", std::vector<int>(B, E), {FLY, FLY, FLY, FLY, FLY}},
      {"n_events == max_events", std::vector<int>(B, E), {STANCE, RF, FLY, LF, STANCE}},
      {"n_events out of range", {-3, 0, E + 1, 1000000, INT32_MAX, INT32_MIN}, {LF, FLY, RF, FLY, STANCE}},
  };
  bool ok = true;
  for (const Sched& sc : scheds)
    for (const int map : {0, 1, -1, 7, INT32_MAX, INT32_MIN})
      for (const double t : {-1.0, 0.2, 0.3, 5.0, 1e300, -1e300}) {
        std::vector<hsqp_terrain_placement> place(B, hsqp_terrain_placement{map, 0, 0.1, -0.2, 0.7});
        const pc_terrain ter = {2, 0, nx.data(), ny.data(), cell.data(), heights.data(), place.data(), ground.data()};
        std::vector<double> ev((size_t)B * E), tt((size_t)B * K), ts((size_t)B * K * NXS, 0.0);
        std::vector<int> seq((size_t)B * (E + 1));
        for (int b = 0; b < B; ++b) {
          for (int i = 0; i < E; ++i) ev[(size_t)b * E + i] = 0.1 * (i + 1);
          for (int i = 0; i <= E; ++i) seq[(size_t)b * (E + 1) + i] = sc.seq[i];
          for (int k = 0; k < K; ++k) { tt[(size_t)b * K + k] = 0.25 * k; ts[((size_t)b * K + k) * NXS] = b == 5 ? 1e300 * k : 0.3 * k; ts[((size_t)b * K + k) * NXS + 3] = 0.2 * k; }
        }
        const size_t rows = (size_t)B * 2 * (E + 1);
        std::vector<double> lift(rows, -7.0), touch(rows, -7.0), fxy(rows * 2, -7.0);
        pc_foot_heights(h, &ter, B, E, K, t, -0.001, x.data(), sc.ne.data(), ev.data(), seq.data(), tt.data(), ts.data(), lift.data(), touch.data(), fxy.data());
        for (int b = 0; b < B && ok; ++b) {
          const int ne = sc.ne[b] < 0 ? 0 : (sc.ne[b] > E ? E : sc.ne[b]);
          for (int f = 0; f < 2; ++f)
            for (int p = 0; p <= E; ++p) {
              const size_t i = ((size_t)b * 2 + f) * (E + 1) + p;
              if (p > ne) ok = ok && lift[i] == 0.0 && touch[i] == 0.0 && fxy[2 * i] == 0.0 && fxy[2 * i + 1] == 0.0;
              else if (b == 4) ok = ok && std::isnan(lift[i]) && std::isnan(touch[i]) && std::isnan(fxy[2 * i]);
              else ok = ok && std::isfinite(lift[i]) && std::isfinite(touch[i]) && lift[i] >= 0.25 && lift[i] <= 0.65 && std::isfinite(fxy[2 * i]) && std::isfinite(fxy[2 * i + 1]);
              if (!ok) { fprintf(stderr, "%s, map %d, t %g: instance %d foot %d phase %d: lift %g touch %g foothold (%g, %g)\n", sc.name, map, t, b, f, p, lift[i], touch[i], fxy[2 * i], fxy[2 * i + 1]); break; }
            }
        }
        if (!ok) return 1;
        // the three-argument planner over the same rows, at times around and far beyond the events (instance 0's rows)
        const hsqp_swing_config cfg = {0.05, -0.0, 0.08, -0.001, 0.4, 0.005, -0.15, 0.3};
        const std::vector<double> times = {-1e300, 0.0, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4, 1e300};
        std::vector<double> par(times.size() * HSQP_NODE_PARAMS);
        const int ne0 = sc.ne[0] < 1 ? 1 : (sc.ne[0] > E ? E : sc.ne[0]);   // (the upload refuses n_events outside [1, max_events])
        pc_node_params(&cfg, 0.0, 1, E, ne0, ev.data(), seq.data(), K, tt.data(), ts.data(), (int)times.size(), times.data(), lift.data(), touch.data(), par.data());
      }
  pc_destroy(h);
  printf(ok ? "perceive ok\n" : "perceive FAILED\n");
  return ok ? 0 : 1;
}
