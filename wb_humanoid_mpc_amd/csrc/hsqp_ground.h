// Per-instance ground-height estimate from the stance feet (include/hsqp_ground.h): what the reference's
//   SwitchedModelReferenceManager::modifyReferences -> adaptToCurrentGroundHeight      humanoid_common_mpc/src/reference_manager/SwitchedModelReferenceManager.cpp:83-104,140-154
//   getGroundHeightEstimate                                                           humanoid_common_mpc/src/pinocchio_model/DynamicsHelperFunctions.cpp:168-190
// evidently mean: the ground under an instance is the mean height of the contact frames of the feet its mode says are in contact, one foot's height
// in single support, the last value in flight; the base height of every target knot is shifted by it and the swing planner takes it as its terrain
// height.  The reference keeps ONE last value (a function-local static); here every instance owns its latch (g [B], in / out).
//
// Shape: one lane per (instance, foot).  A lane walks the forward kinematics from the base down ITS leg only — the z row of every rotation on the path
// and the z component of every offset, nothing else of the tree; the two lanes of an instance exchange their height, the lane of foot 0 applies the rule.
//
// Arithmetic: every product-sum is evaluated unfused (`#pragma clang fp contract(off)`; hipcc contracts device code by default), so the device differs
// from the host build of this source (tests/ground/ground_emu.cpp, -ffp-contract=off) only by its sin / cos.  The rule itself (mean, latch, filter, the
// shift of the knots) has no transcendental in it: given the two heights it is the same bits everywhere.
#pragma once
#include "hsqp_common.h"
#include "hsqp_loop.h"
#include "hsqp_model.h"
#include "hsqp_params.h"
#include "../../include/hsqp_ground.h"

namespace hsqp {

// World z of contact frame f at the configuration part of the state row x [NX]: the walk base -> ancestors of contact_body[f] -> the frame, row 2 only.
// Row 2 of R_i = (row 2 of R_parent) Rfix_i Rot(axis_i, q_i); z of r_i = z of r_parent + (row 2 of R_parent) . pfix_i.
HSQP_HD double ground_foot_height(const DevModel& dm, const double* x, int f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int body = dm.contact_body[f];
  const double cy = cos(x[4]), sy = sin(x[4]), cx = cos(x[5]), sx = sin(x[5]);
  double row[3] = {-sy, cy * sx, cy * cx};   // row 2 of Rz Ry Rx: the yaw does not enter a height
  double z = x[2];
  for (int n = 0; n < dm.n_anc[body]; ++n) {
    const int i = dm.anc[body][n];
    double Rq[9], M[9];
    rot_axis_cs(dm.axis[i], cos(x[5 + i]), sin(x[5 + i]), Rq);
    m3_mul(dm.Rfix[i], Rq, M);
    z = z + (row[0] * dm.pfix[i][0] + row[1] * dm.pfix[i][1] + row[2] * dm.pfix[i][2]);
    const double r0 = row[0] * M[0] + row[1] * M[3] + row[2] * M[6];
    const double r1 = row[0] * M[1] + row[1] * M[4] + row[2] * M[7];
    const double r2 = row[0] * M[2] + row[1] * M[5] + row[2] * M[8];
    row[0] = r0; row[1] = r1; row[2] = r2;
  }
  return z + (row[0] * dm.contact_p[f][0] + row[1] * dm.contact_p[f][1] + row[2] * dm.contact_p[f][2]);
}

// The rule for one instance from the heights z = {foot 0, foot 1} of its contact frames.  The mode is seq[ev_lower(ev, n_ev, t)], what node_params_eval
// takes for a node at t, so the feet it selects are the ones P_CONTACT of node 0 flags.  Returns the new latch: g_old in flight, else the raw estimate
// (filter_alpha == 0) or alpha g_old + (1 - alpha) raw.  foot_z (may be null): both heights, for read-back.
HSQP_HD double ground_estimate_instance(const double* z, int n_ev, const double* ev, const int* seq, double t, double filter_alpha, double g_old, double* foot_z) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (foot_z) { foot_z[0] = z[0]; foot_z[1] = z[1]; }
  const int mode = seq[ev_lower(ev, n_ev, t)];
  const bool c0 = mode_contact(mode, 0), c1 = mode_contact(mode, 1);
  if (!c0 && !c1) return g_old;
  const double raw = c0 && c1 ? 0.5 * (z[0] + z[1]) : (c0 ? z[0] : z[1]);
  return filter_alpha == 0.0 ? raw : filter_alpha * g_old + (1.0 - filter_alpha) * raw;
}

// The shift of one instance's target knots [CMD_KNOTS][NX]: the command's height entry means height above the estimated ground.  One IEEE add per knot.
HSQP_HD void ground_apply_instance(double g, double* ts) {
  for (int k = 0; k < CMD_KNOTS; ++k) ts[(size_t)k * NX + 2] = ts[(size_t)k * NX + 2] + g;
}

// what the kernel hands over besides the model; every array is the batch's
struct GroundArgs {
  int B, E;                      // instances, max_events
  double t, filter_alpha;
  const double* x;               // [B][NX]
  const int* ne; const double* ev; const int* seq;   // [B], [B][E], [B][E + 1]
  const double* g_in; double* g_out;                 // [B] the latch, [B] its new value (may be the same array: an instance reads and writes its own entry)
  double* foot_z;                // [B][2] or null
  // the loop's cycle (all null / 0 in the stand-alone call)
  const double* g_init;          // [B]: with mode_b, an instance that starts an episode in this cycle (HSQP_WARM_COLD) starts from it instead of its latch
  const int* mode_b;             // [B] HSQP_WARM_SHIFT / _COLD or null
  const int* parked;             // [B] episode state (non-zero: parked, its stance command is absolute: no shift) or null
  double* ts;                    // [B][CMD_KNOTS][NX] target knots to shift, or null
  double* terrain_b;             // [B] the terrain height of step 2, or null
};

// lane (instance b, foot 0) behind the exchange: z = both heights of instance b
HSQP_HD void ground_instance_finish(const GroundArgs& a, int b, const double* z) {
  const double g_old = a.mode_b && a.mode_b[b] == HSQP_WARM_COLD ? a.g_init[b] : a.g_in[b];
  const double g = ground_estimate_instance(z, a.ne[b], a.ev + (size_t)b * a.E, a.seq + (size_t)b * (a.E + 1), a.t, a.filter_alpha, g_old,
                                            a.foot_z ? a.foot_z + (size_t)b * 2 : nullptr);
  a.g_out[b] = g;
  if (a.ts && !(a.parked && a.parked[b] != 0)) ground_apply_instance(g, a.ts + (size_t)b * CMD_KNOTS * NX);
  if (a.terrain_b) a.terrain_b[b] = g;
}

}  // namespace hsqp
