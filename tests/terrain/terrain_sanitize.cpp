// TEST INFRASTRUCTURE: a program of its own that takes the host build of the terrain (tests/terrain/terrain_emu.cpp, compiled beside this file) to the edges
// of its index arithmetic, for a run under the address and undefined-behaviour sanitizers (tests/test_terrain.py): terrain_height and the terrain's
// contact_point with coordinates at +-1e300, +-inf and NaN on a 2 x 2 map, and a placement whose map index is out of range, as a table that came through the
// _device entry could be.  A finite coordinate gives a clamped, finite height; a non-finite one gives NaN without the map being read.
//   terrain_sanitize DESC_FILE     DESC_FILE: the bytes of the binding's hsqp_model_desc
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#define ROLLOUT_EMU_DECLARATIONS_ONLY
#include "terrain_emu.h"

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: terrain_sanitize DESC_FILE\n"); return 2; }
  std::vector<char> image(sizeof(hsqp_model_desc));
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(image.data(), 1, image.size(), f) != image.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  fclose(f);
  char err[256] = "";
  void* h = emu_create(reinterpret_cast<const hsqp_model_desc*>(image.data()), err, sizeof err);
  if (!h) { fprintf(stderr, "%s\n", err); return 1; }
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // the 2 x 2 map on the heap, exactly its four heights long: a read past it is the sanitizer's to see
  std::vector<double> H = {0.0, 0.1, 0.2, 0.4};
  const int32_t nx = 2, ny = 2;
  const double cell = 0.5;
  hsqp_contact_settings cs = {};
  cs.enabled = 1; cs.stiffness = 5e4; cs.damping = 10.0; cs.mu = 0.6; cs.slip_velocity = 0.01; cs.ground_height = 0.25;
  const double far[] = {1e300, -1e300, inf, -inf, nan, 0.3, -0.2, 0.5, 0.0};
  const int nf = (int)(sizeof far / sizeof far[0]);
  bool ok = true;
  for (const int map : {0, -1, 1, 7, INT32_MAX, INT32_MIN}) {          // (0: the map; -1: the plane; the others are clamped to one of the two)
    for (const double yaw : {0.0, 0.7}) {
      hsqp_terrain_placement pl = {map, 0, 0.1, -0.2, yaw};
      const emu_terrain t = {1, 0, &nx, &ny, &cell, H.data(), &pl};
      std::vector<double> xy, hgt((size_t)nf * nf), nrm((size_t)nf * nf * 3);
      for (int i = 0; i < nf; ++i) for (int j = 0; j < nf; ++j) { xy.push_back(far[i]); xy.push_back(far[j]); }
      emu_terrain_eval(&cs, nullptr, &t, nf * nf, xy.data(), hgt.data(), nrm.data());
      const bool plane = map < 0;
      for (int i = 0; i < nf; ++i) for (int j = 0; j < nf; ++j) {
        const double g = hgt[(size_t)i * nf + j];
        const double* n = &nrm[((size_t)i * nf + j) * 3];
        const bool fin = std::isfinite(far[i]) && std::isfinite(far[j]);
        if (plane) { ok = ok && g == 0.25 && n[2] == 1.0; continue; }
        if (fin) ok = ok && g >= 0.25 && g <= 0.65 && std::isfinite(n[0]) && std::isfinite(n[1]) && n[2] > 0.0 && n[2] <= 1.0;
        else ok = ok && std::isnan(g) && n[2] == 1.0;
        if (!ok) { fprintf(stderr, "terrain_height: map %d yaw %g point (%g, %g): g %g n (%g, %g, %g)\n", map, yaw, far[i], far[j], g, n[0], n[1], n[2]); return 1; }
      }
      // the terrain's contact_point: the base at the far coordinate, the soles through the ground
      for (int i = 0; i < nf; ++i) {
        std::vector<double> x(HSQP_NX, 0.0), force(8 * 3), pen(8);
        x[0] = far[i]; x[1] = far[(i + 3) % nf]; x[2] = 0.2;
        emu_contact_eval(h, &cs, nullptr, &t, x.data(), force.data(), pen.data());
        const bool fin = std::isfinite(x[0]) && std::isfinite(x[1]);
        for (int p = 0; p < 8; ++p) {
          if (fin || plane) ok = ok && std::isfinite(pen[p]) && std::isfinite(force[3 * p]) && std::isfinite(force[3 * p + 2]);
          else ok = ok && std::isnan(pen[p]) && std::isnan(force[3 * p + 2]);
        }
        if (!ok) { fprintf(stderr, "contact_point: map %d yaw %g base (%g, %g)\n", map, yaw, x[0], x[1]); return 1; }
      }
    }
  }
  emu_destroy(h);
  printf(ok ? "terrain ok\n" : "terrain FAILED\n");
  return ok ? 0 : 1;
}
