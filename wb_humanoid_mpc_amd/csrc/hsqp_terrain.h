// Height-map terrain under the torque plant (include/hsqp_terrain.h): the resident maps and placements as the kernels see them, one instance's map and
// the bilinear height and normal under a world point.
//   terrain_load     instance b's placement into the workspace: the map's pointer, dimensions and cell size, the origin, cos / sin of yaw — once per
//                    call (the terrain instantiations of the rollout kernel and the two evaluation kernels only).  A map index outside [-1, n_maps)
//                    — a table set through the _device entry is not read back — is clamped into it here, so no index of the pool comes from the table
//   terrain_height   steps 1-7 of the public header at (X, Y): the map's height hm and the unit normal n.  The coordinates are clamped in double before
//                    they become integers, and a non-finite one never becomes an index: hm is NaN and the map is not read
// The quotients by the cell size are divisions, as the public header states them (a point on a cell line stays on it), not products with 1 / cell.
// Everything is uniform across the workgroup; the same source builds for the host with a one-lane context (tests/terrain/terrain_emu.cpp).
#pragma once
#include "hsqp_common.h"
#include "../../include/hsqp_terrain.h"

namespace hsqp {

// one resident map: its heights are pool[first .. first + nx ny)
struct TerrainMap {
  int32_t nx, ny;
  double cell;
  size_t first;
};
// The resident terrain, as the kernels that have one see it
struct TerrainParams {
  const TerrainMap* maps;                    // [n_maps]
  const double* pool;                        // the maps' heights, concatenated
  const hsqp_terrain_placement* place;       // [max_batch] the placement of every instance: the table's entry, or map = -1
  int n_maps;
};
// (host) n entries as TerrainParams::place reads them: the table's first (n_table of them; table null: none), behind them the plane
inline void terrain_fill_place(const hsqp_terrain_placement* table, size_t n_table, size_t n, hsqp_terrain_placement* out) {
  for (size_t i = 0; i < n; ++i) out[i] = table && i < n_table ? table[i] : hsqp_terrain_placement{-1, 0, 0.0, 0.0, 0.0};
}

// ONE instance's map (H null: the horizontal plane)
struct TerrainSet {
  const double* H;
  int nx, ny;
  double cell, ox, oy, cy, sy;
};

// instance b of the terrain, by the calling lane alone (no barrier): terrain_load's work, and a lane-per-instance kernel's whole load (csrc/hsqp_perceive.h)
HSQP_HD void terrain_load_lane(const TerrainParams& tp, int b, TerrainSet& ts) {
  const hsqp_terrain_placement pl = tp.place[b];
  int m = pl.map;
  m = m < -1 ? -1 : (m > tp.n_maps - 1 ? tp.n_maps - 1 : m);
  if (m < 0) {
    ts.H = nullptr; ts.nx = ts.ny = 2; ts.cell = 1.0; ts.ox = ts.oy = 0.0; ts.cy = 1.0; ts.sy = 0.0;
  } else {
    const TerrainMap mp = tp.maps[m];
    ts.H = tp.pool + mp.first; ts.nx = mp.nx; ts.ny = mp.ny; ts.cell = mp.cell;
    ts.ox = pl.origin_x; ts.oy = pl.origin_y; ts.cy = cos(pl.yaw); ts.sy = sin(pl.yaw);
  }
}

// instance b of the terrain into the workspace.  Ends with a barrier.
HSQP_HD void terrain_load(const Ctx& ctx, const TerrainParams& tp, int b, TerrainSet& ts) {
  WG_FOR(ctx, i, 1) terrain_load_lane(tp, b, ts);
  WG_SYNC(ctx);
}

// one grid coordinate: clamped into [0, n - 1] in double, then the cell index i <= n - 2 and the fraction s; returns whether it was clamped
HSQP_HD bool terrain_cell(double a, int n, int& i, double& s) {
  bool clamped = false;
  const double top = (double)(n - 1);
  if (a < 0.0) { a = 0.0; clamped = true; }
  else if (a > top) { a = top; clamped = true; }
  i = (int)a;
  if (i > n - 2) i = n - 2;
  s = a - (double)i;
  return clamped;
}

// the map's height hm (*g) and the unit normal n [3] of the ground under the world point (X, Y); the plane: 0 and (-0, -0, 1)
HSQP_HD void terrain_height(const TerrainSet& ts, double X, double Y, double* g, double* n) {
  double hm = 0.0, hx = 0.0, hy = 0.0;
  if (ts.H) {
    const double dx = X - ts.ox, dy = Y - ts.oy;
    const double a = (ts.cy * dx + ts.sy * dy) / ts.cell, b = (ts.cy * dy - ts.sy * dx) / ts.cell;
    if (!(a - a == 0.0) || !(b - b == 0.0)) {
      hm = __builtin_nan("");   // (no index is formed: the instance ends non-finite)
    } else {
      int i, j;
      double s, t;
      const bool ca = terrain_cell(a, ts.nx, i, s), cb = terrain_cell(b, ts.ny, j, t);
      const double* r0 = ts.H + (size_t)j * ts.nx + i;
      const double* r1 = r0 + ts.nx;
      const double h00 = r0[0], h10 = r0[1], h01 = r1[0], h11 = r1[1];
      const double e0 = h10 - h00, e1 = h11 - h01;
      const double h0 = h00 + s * e0, h1 = h01 + s * e1;
      hm = h0 + t * (h1 - h0);
      const double gx = ca ? 0.0 : (e0 + t * (e1 - e0)) / ts.cell, gy = cb ? 0.0 : (h1 - h0) / ts.cell;
      hx = ts.cy * gx - ts.sy * gy;
      hy = ts.sy * gx + ts.cy * gy;
    }
  }
  const double r = sqrt((1.0 + hx * hx) + hy * hy);
  *g = hm;
  n[0] = -hx / r; n[1] = -hy / r; n[2] = 1.0 / r;
}

}  // namespace hsqp
