/*
 * hsqp_terrain.h — uneven ground under the torque plant (hsqp_plant.h, hsqp_contact.h): per-instance height-map terrain.  The contact model of
 * hsqp_contact.h reads one height per instance and assumes the normal (0, 0, 1); with a terrain resident each sole corner reads the height and the
 * gradient of a height map under its own (X, Y) and the force acts along the local normal.  The MPC never sees it: the iteration kernels, the node
 * parameters, the warm start, the triage box of hsqp_episode.h (absolute base height) and hsqp_loop_settings::terrain_height are untouched.  With no
 * terrain set, after hsqp_terrain_clear, with contact off or with the plant kind HSQP_PLANT_FLOW every rollout is bit for bit what it was without
 * this header: the terrain is a parameter of the rollout's instantiation, not a run-time branch.
 *
 * Maps.  A handle holds up to HSQP_TERRAIN_MAX_MAPS height maps, shared by all instances, in device memory, read-only to the kernels.  Map m is a
 * regular grid of nx x ny heights H[iy][ix] (row-major, double), 2 <= nx, ny <= HSQP_TERRAIN_MAX_DIM, with one cell size `cell` > 0 for both axes.
 *
 * Placement.  Instance b has {map, reserved, origin_x, origin_y, yaw}: map = -1 is the horizontal plane of hsqp_contact.h; origin is the world
 * position of grid node (0, 0); yaw rotates the map about the vertical through the origin.  Instances past the table, and every instance without
 * a table, have map = -1.
 *
 * Height at a world point (X, Y):
 *   1. map-local coordinates (xl, yl) = Rz(-yaw) (X - origin_x, Y - origin_y),  a = xl / cell,  b = yl / cell
 *   2. a is clamped to [0, nx - 1] and b to [0, ny - 1] in double, before any conversion to an integer
 *   3. i = min((int) a, nx - 2), s = a - i;  j = min((int) b, ny - 2), t = b - j
 *   4. h00 = H[j][i], h10 = H[j][i + 1], h01 = H[j + 1][i], h11 = H[j + 1][i + 1]
 *   5. h0 = h00 + s (h10 - h00),  h1 = h01 + s (h11 - h01),  hm = h0 + t (h1 - h0)
 *   6. gx = ((h10 - h00) + t ((h11 - h01) - (h10 - h00))) / cell,  gy = (h1 - h0) / cell;  a component is 0 where its coordinate was clamped: the
 *      map continues flat past its edge
 *   7. world gradient (hx, hy) = Rz(yaw) (gx, gy)
 *   8. ground g = ground_height_b + hm: ground_height_b and mu_b stay those of hsqp_contact.h, the per-instance height is an offset under the map
 * A non-finite X or Y never becomes an index: the point's hm is NaN without the map being read, and the instance ends HSQP_ROLLOUT_NONFINITE.
 *
 * Force at a point with world position P and velocity Pdot (k, c, v_s, mu of hsqp_contact.h):
 *   n  = (-hx, -hy, 1) / sqrt(1 + hx^2 + hy^2)
 *   d  = (g - P_z) n_z                      (the distance to the local tangent plane)
 *   vn = Pdot . n,  ddot = -vn;   fn = max(0, k d (1 + c ddot)) for d > 0, else 0
 *   v_t = Pdot - vn n;   ft = -mu fn v_t / sqrt(|v_t|^2 + v_s^2);   F = fn n + ft,  wrench about the base origin {P x F, F}
 * Everything else is what hsqp_contact.h describes: the prescribed wrenches are dropped on the plant, tau_ff keeps them, a point without force
 * stores +0, a NaN stays.
 *
 * ASSUMPTIONS:
 *   T1. Bilinear patches are C0 with kinks at the cell lines — assumption C2 of hsqp_contact.h once more: HSQP_ROLLOUT_ODE45 shortens its steps,
 *       HSQP_ROLLOUT_RK4 is first-order across a kink.
 *   T2. A true vertical step is represented as a one-cell ramp.
 *   T3. For a plane map d and ddot are exact; on curved patches they are first order in the curvature.
 *   T4. There is no edge or corner contact of the sole other than its eight points.
 *   T5. The MPC, the triage box of hsqp_episode.h (absolute base height) and hsqp_loop_settings::terrain_height do not see the map.
 *       (It holds while the ground-height estimate of include/hsqp_ground.h is off: with it on the loop follows the ground under the stance feet.)
 *       With the per-foot swing heights of include/hsqp_perceive.h on, the swing references of the MPC read the map: lift-off and touch-down height per foot.
 *
 * Lifetime: that of the contact table (hsqp_upload*, hsqp_solve, hsqp_loop_start*, the weight updates, hsqp_plant_set / _clear, hsqp_contact_set
 * keep it).  The terrain acts only while the plant kind is HSQP_PLANT_TORQUE, contact is enabled, and both maps and a placement table are
 * resident; otherwise it is stored and inert.  Whole-body handles only.
 *
 * hsqp_terrain_eval samples the ground of each instance at given world points — whatever the plant kind, with no resident solution:
 * height[b][p] = g, normal[b][p] = n.  hsqp_contact_eval* answers with the model above while a terrain is resident (maps and a table).
 *
 * Errors: HSQP_ERR_BAD_ARG, message in hsqp_last_error naming the entry point, for a NULL argument, a centroidal handle, reserved != 0, n_maps,
 * nx, ny, batch or n_pts out of range, cell not finite or <= 0, a non-finite height, origin or yaw (host arrays), map outside [-1, n_maps) (host arrays),
 * and hsqp_terrain_set_maps with fewer maps than a resident placement table refers to.  A placement set through the _device entry is not read
 * back: the kernel clamps map into [-1, n_maps) itself when it loads the instance, and hsqp_terrain_set_maps cannot check it.
 *
 * ABI: additions only — HSQP_ABI_VERSION (hsqp.h) needs no bump.
 */
#ifndef HSQP_TERRAIN_H
#define HSQP_TERRAIN_H

#include "hsqp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define HSQP_TERRAIN_MAX_MAPS 16
#define HSQP_TERRAIN_MAX_DIM  256
#define HSQP_TERRAIN_MAX_POINTS (1 << 24)   /* points per instance of one hsqp_terrain_eval call */

typedef struct hsqp_terrain_placement {
  int32_t map, reserved;           /* map in [-1, n_maps), -1: the horizontal plane; reserved == 0 */
  double origin_x, origin_y;       /* world position of grid node (0, 0) [m] */
  double yaw;                      /* [rad] */
} hsqp_terrain_placement;

/* nx, ny, cell [n_maps]; heights: the maps concatenated, map m nx[m] * ny[m] doubles.  n_maps = 0 frees them (the arrays may be NULL) */
int hsqp_terrain_set_maps(hsqp_handle* h, int n_maps, const int32_t* nx, const int32_t* ny, const double* cell, const double* heights);
/* place [batch]; NULL: no table — every instance back to map = -1 */
int hsqp_terrain_set_instances(hsqp_handle* h, int batch, const hsqp_terrain_placement* place);
int hsqp_terrain_set_instances_device(hsqp_handle* h, int batch, const hsqp_terrain_placement* d_place);
int hsqp_terrain_clear(hsqp_handle* h);             /* no maps, no table */
/* n_maps [1]; nx, ny, cell [HSQP_TERRAIN_MAX_MAPS] (the first n_maps are written); heights: the maps concatenated, at most max_heights doubles
 * (NULL: not wanted; fewer than the maps hold: HSQP_ERR_BAD_ARG).  Any array may be NULL */
int hsqp_terrain_get_maps(hsqp_handle* h, int32_t* n_maps, int32_t* nx, int32_t* ny, double* cell, double* heights, size_t max_heights);
int hsqp_terrain_get_instances(hsqp_handle* h, int batch, hsqp_terrain_placement* place);
/* xy [batch][n_pts][2], 1 <= n_pts <= HSQP_TERRAIN_MAX_POINTS; height [batch][n_pts], normal [batch][n_pts][3]: either may be NULL */
int hsqp_terrain_eval(hsqp_handle* h, int batch, int n_pts, const double* xy, double* height, double* normal);
int hsqp_terrain_eval_device(hsqp_handle* h, int batch, int n_pts, const double* d_xy, double* d_height, double* d_normal);

#ifdef __cplusplus
}
#endif
#endif /* HSQP_TERRAIN_H */
