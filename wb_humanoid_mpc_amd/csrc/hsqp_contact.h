// Ground contact on the torque plant of the rollout (include/hsqp_contact.h): the resident setting as the kernel sees it, one instance's
// parameters and the eight sole corners of one flow evaluation in the rollout workspace.  Penalty model: Hunt-Crossley normal force with exponent
// 1, regularised Coulomb friction, a horizontal plane (assumption C1 of the public header: not the reference's MuJoCo solver).
//   contact_load     instance b of the setting into the workspace (the contact instantiation of the rollout kernel only: the handle launches it
//                    when contact is on, so the set carries no switch and the plant's own instantiation carries no set)
//   contact_forces   from what stage_eval<false> leaves at the plant's own (q, v): the placements R / r relative to the base origin O and the
//                    spatial velocity vl = {omega, v_O} of the foot link about O.  P = r_b + R_b p_fc, Pdot = v_O + omega x P; the height of the
//                    point adds the base position q[2].  The eight points are eight work items; each leaves P, d, the force and its wrench
//                    {P x f, f} about O, which plant_forward_dynamics picks up per coordinate by the subtree test of the pushes.
// A point without normal force stores +0 in every entry of force and wrench: subtracting it changes no bit of the right-hand side.
// On a height map (include/hsqp_terrain.h) the set carries the instance's map too and a second contact_point reads height and normal under each point.
// Everything is uniform across the workgroup; the same source builds for the host with a one-lane context (tests/contact/contact_emu.cpp).
#pragma once
#include <type_traits>

#include "hsqp_model.h"
#include "hsqp_terrain.h"
#include "../../include/hsqp_contact.h"

namespace hsqp {

constexpr int CT_PTS = HSQP_CONTACT_FEET * HSQP_CONTACT_CORNERS;

// The resident setting, as the kernels that have a ground see it
struct ContactParams {
  const hsqp_contact_ground* ground;   // [max_batch] the ground of every instance: the table's entry, or the setting's values
  double k, c, vs;                     // stiffness, damping, slip velocity
};
// (host) n entries as ContactParams::ground reads them: the per-instance table's first (n_table of them; table null: none), behind them the setting's values
inline void contact_fill_ground(const hsqp_contact_settings& s, const hsqp_contact_ground* table, size_t n_table, size_t n, hsqp_contact_ground* out) {
  for (size_t i = 0; i < n; ++i) out[i] = table && i < n_table ? table[i] : hsqp_contact_ground{s.ground_height, s.mu};
}

// ONE instance's ground and the points of one flow evaluation
struct ContactSet {
  double k, c, vs, height, mu;
  double P[CT_PTS][3];          // the points relative to the base origin O, world axes
  double d[CT_PTS];             // penetration (negative: above the ground)
  double f[CT_PTS][3];          // force on the foot, world axes (ft_x, ft_y, fn)
  double wr[CT_PTS][6];         // its wrench about O {moment, force}
};

// instance b of the setting into the workspace.  Ends with a barrier.
HSQP_HD void contact_load(const Ctx& ctx, const ContactParams& cp, int b, ContactSet& ct) {
  WG_FOR(ctx, i, 1) {
    ct.k = cp.k; ct.c = cp.c; ct.vs = cp.vs;
    ct.height = cp.ground[b].height; ct.mu = cp.ground[b].mu;
  }
  WG_SYNC(ctx);
}

// corner c of the contact rectangle of foot f, in the axes of the foot's body
HSQP_HD void contact_corner(const DevModel& dm, int f, int c, double* p) {
  p[0] = dm.contact_p[f][0] + ((c == 1 || c == 2) ? dm.rect_x_max : dm.rect_x_min);
  p[1] = dm.contact_p[f][1] + (c >= 2 ? dm.rect_y_max : dm.rect_y_min);
  p[2] = dm.contact_p[f][2];
}

// point i of the set at the evaluation stage_eval<false> has just run on ws (its q, v).  One work item; no barrier.
HSQP_HD void contact_point(const DevModel& dm, const StageWST<false>& ws, ContactSet& ct, int i) {
  const int f = i / HSQP_CONTACT_CORNERS, b = dm.contact_body[f];
  double p[3], P[3], wxP[3];
  contact_corner(dm, f, i % HSQP_CONTACT_CORNERS, p);
  m3_mulv(ws.R[b], p, P);
  for (int k = 0; k < 3; ++k) P[k] += ws.r[b][k];
  const double* vl = ws.vl[b + 2];
  v3_cross(vl, P, wxP);
  const double vx = vl[3] + wxP[0], vy = vl[4] + wxP[1], vz = vl[5] + wxP[2];
  const double d = ct.height - (ws.q[2] + P[2]), ddot = -vz;
  double fn = d > 0.0 ? ct.k * d * (1.0 + ct.c * ddot) : 0.0;
  if (!(fn > 0.0) && fn == fn) fn = 0.0;   // (a NaN stays: the instance ends non-finite)
  double F[3] = {0.0, 0.0, 0.0}, mom[3] = {0.0, 0.0, 0.0};
  if (fn != 0.0) {
    const double s = -ct.mu * fn / sqrt((vx * vx + vy * vy) + ct.vs * ct.vs);
    F[0] = s * vx; F[1] = s * vy; F[2] = fn;
    v3_cross(P, F, mom);
  }
  ct.d[i] = d;
  for (int k = 0; k < 3; ++k) { ct.P[i][k] = P[k]; ct.f[i][k] = F[k]; ct.wr[i][k] = mom[k]; ct.wr[i][3 + k] = F[k]; }
}

// ... and ONE instance's ground on a height map (include/hsqp_terrain.h): the set above — its height is the offset under the map — and the instance's map.
// A type of its own: the plane's set, its contact_point and every instantiation built on them stay what they were.
struct ContactTerrainSet : ContactSet {
  TerrainSet ter;
};
// point i on the terrain: the height and the normal n of the map under the point's own (X, Y); d is the distance to the local tangent plane, the normal
// force acts along n, friction against the tangential velocity.  A NaN height (a non-finite X or Y) stays in fn: the instance ends non-finite.
HSQP_HD void contact_point(const DevModel& dm, const StageWST<false>& ws, ContactTerrainSet& ct, int i) {
  const int f = i / HSQP_CONTACT_CORNERS, b = dm.contact_body[f];
  double p[3], P[3], wxP[3], n[3], hm;
  contact_corner(dm, f, i % HSQP_CONTACT_CORNERS, p);
  m3_mulv(ws.R[b], p, P);
  for (int k = 0; k < 3; ++k) P[k] += ws.r[b][k];
  const double* vl = ws.vl[b + 2];
  v3_cross(vl, P, wxP);
  const double V[3] = {vl[3] + wxP[0], vl[4] + wxP[1], vl[5] + wxP[2]};
  terrain_height(ct.ter, ws.q[0] + P[0], ws.q[1] + P[1], &hm, n);
  const double d = ((ct.height + hm) - (ws.q[2] + P[2])) * n[2];
  const double vn = (V[0] * n[0] + V[1] * n[1]) + V[2] * n[2], ddot = -vn;
  double fn = d > 0.0 ? ct.k * d * (1.0 + ct.c * ddot) : (d == d ? 0.0 : d);
  if (!(fn > 0.0) && fn == fn) fn = 0.0;   // (a NaN stays: the instance ends non-finite)
  double F[3] = {0.0, 0.0, 0.0}, mom[3] = {0.0, 0.0, 0.0};
  if (fn != 0.0) {
    const double vt[3] = {V[0] - vn * n[0], V[1] - vn * n[1], V[2] - vn * n[2]};
    const double s = -ct.mu * fn / sqrt(((vt[0] * vt[0] + vt[1] * vt[1]) + vt[2] * vt[2]) + ct.vs * ct.vs);
    for (int k = 0; k < 3; ++k) F[k] = fn * n[k] + s * vt[k];
    v3_cross(P, F, mom);
  }
  ct.d[i] = d;
  for (int k = 0; k < 3; ++k) { ct.P[i][k] = P[k]; ct.f[i][k] = F[k]; ct.wr[i][k] = mom[k]; ct.wr[i][3 + k] = F[k]; }
}

template <class CT>
HSQP_HD void contact_forces(const Ctx& ctx, const DevModel& dm, const StageWST<false>& ws, CT& ct) {
  WG_FOR(ctx, i, CT_PTS) contact_point(dm, ws, ct, i);
  WG_SYNC(ctx);
}

// The workspace of hsqp_contact_eval: the stage's, and the set (CT: ContactSet, or ContactTerrainSet while a terrain is resident)
template <class CT>
struct ContactEvalWST {
  StageWST<false> st;
  CT ct;
};
using ContactEvalWS = ContactEvalWST<ContactSet>;

// hsqp_contact_eval for one instance: the model at state x [58] with instance b of the setting (tp: the resident terrain, read on a ContactTerrainSet
// only); force [8][3], pen [8] (either may be null)
template <class CT>
HSQP_HD void contact_eval_instance(const Ctx& ctx, const DevModel& dm, ContactEvalWST<CT>& w, const ContactParams& cp, const TerrainParams* tp, int b, const double* x,
                                   double* force, double* pen) {
  stage_topology(ctx, dm, w.st, false);
  WG_FOR(ctx, i, NV + NV + NJ + 12) {
    if (i < NV) w.st.q[i] = x[i];
    else if (i < 2 * NV) w.st.v[i - NV] = x[i];
    else if (i < 2 * NV + NJ) w.st.qddj[i - 2 * NV] = 0.0;
    else w.st.W[i - 2 * NV - NJ] = 0.0;
  }
  if constexpr (!std::is_same<CT, ContactSet>::value) terrain_load(ctx, *tp, b, w.ct.ter);
  contact_load(ctx, cp, b, w.ct);   // (its barrier closes the topology and the inputs)
  stage_eval<false>(ctx, dm, w.st);
  contact_forces(ctx, dm, w.st, w.ct);
  WG_FOR(ctx, i, CT_PTS * 4) {
    const int pt = i / 4, k = i % 4;
    if (k < 3) { if (force) force[pt * 3 + k] = w.ct.f[pt][k]; }
    else if (pen) pen[pt] = w.ct.d[pt];
  }
}
HSQP_HD void contact_eval_instance(const Ctx& ctx, const DevModel& dm, ContactEvalWS& w, const ContactParams& cp, int b, const double* x, double* force,
                                   double* pen) {
  contact_eval_instance(ctx, dm, w, cp, nullptr, b, x, force, pen);
}

// hsqp_terrain_eval for one instance: the ground g [n_pts] = the instance's height + the map's, and the normal [n_pts][3], at the points xy [n_pts][2]
// (either output may be null).  ts: the instance's map in the workgroup's memory.
HSQP_HD void terrain_eval_instance(const Ctx& ctx, const ContactParams& cp, const TerrainParams& tp, TerrainSet& ts, int b, int n_pts, const double* xy,
                                   double* height, double* normal) {
  terrain_load(ctx, tp, b, ts);
  WG_FOR(ctx, i, n_pts) {
    double hm, n[3];
    terrain_height(ts, xy[2 * i], xy[2 * i + 1], &hm, n);
    if (height) height[i] = cp.ground[b].height + hm;
    if (normal) for (int k = 0; k < 3; ++k) normal[3 * i + k] = n[k];
  }
}

}  // namespace hsqp
