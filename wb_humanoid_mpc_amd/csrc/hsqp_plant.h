// Torque-level plant of the rollout (include/hsqp_plant.h): full forward dynamics of the whole-body tree under the joint PD law of the
// reference's WBMpcMrtJointController::computeJointControlAction (humanoid_wb_mpc/src/mrt/WBMpcMrtJointController.cpp:125-194),
//     (M(q) + diag(0_6, armature)) vd = [0; tau] + sum_feet J^T W - nle(q, v) + sum_pushes J_P^T f.
// Everything is formed from what stage_eval<false> leaves in the stage workspace at (q, v, qdd_j = 0, W): the spatial inertias In[i] and the
// bias forces f[i] of every body about the base origin O (gravity trick, zero base acceleration), the motion axes S, the contact wrenches Fx.
//   composites:  I^c_b, f^c_b = sums over the depth-first range [b, b + sub_b) of the subtree of b
//   mass matrix: M_rc = S_r . (I^c_c S_c) for r an ancestor-or-self of c (coordinates 0..2: unit translations, 3..5: the euler axes — the
//                floating base is the chain x, y, z, rz, ry', rx'', so every base coordinate carries the total inertia), mirrored, else 0
//   bias:        nle_c = S_c . f^c_c;  the generalised force of a wrench {moment, force} about O on a body below c is S_c . wrench
//   solve:       Cholesky of the system bordered by the right-hand side as row 29 (the forward substitution rides on the trailing updates),
//                then one back substitution.  A pivot that is not positive makes the solution non-finite (HSQP_ROLLOUT_NONFINITE).
// Ground contact (include/hsqp_contact.h, hsqp_contact.h): with the instance's ContactSet on, the prescribed contact wrenches Fx are dropped and the
// wrenches of the eight sole corners, formed beside the push wrenches at the plant's own (q, v), take their place in the right-hand side.
// Actuator model (include/hsqp_actuator.h, hsqp_actuator.h): two more stage workspaces carry the instance's ActuatorWS — the held command, the limits and
// the passive torques — beside the plant's; the forward dynamics below are the same under either joint law.
// Inertial variations (include/hsqp_inertia.h, hsqp_inertia.h): four more stage workspaces, PlantVaried<...> of the four above, carry the instance's
// InertiaWS; in them inertia_apply runs between stage_eval<false> and the composites.  plant_forward_dynamics<false> stops behind the assembly (the
// filled bordered system), which is what hsqp_inertia_eval reads; it is ONE function body with a compile-time flag, not two functions: split in two,
// the four rollout kernels that existed before compiled to another schedule of the right-hand-side phase and measured 3.8 % slower.
// Phase style of hsqp_common.h: the same source builds for the host with a one-lane context (tests/plant/plant_emu.cpp).
#pragma once
#include "hsqp_policy.h"
#include "hsqp_push.h"
#include "hsqp_contact.h"
#include "hsqp_actuator.h"
#include "hsqp_inertia.h"
#include "../../include/hsqp_plant.h"

namespace hsqp {

constexpr int PL_N = NV + 1;      // the bordered system: row NV is the right-hand side
constexpr int PL_LD = PL_N + 1;   // odd leading dimension

// The resident plant setting as the kernel sees it (gains null: HSQP_PLANT_FLOW, nothing else is read)
struct PlantParams {
  const double* gains;    // kp [NJ], kd [NJ], armature [NJ]
  double lookahead;
  const double* xt;       // [B][N + 1][NX] nominal states of the resident policy (the state hsqp_evaluate_policy interpolates)
};
// (host) the public setting as PlantParams::gains reads it: g [3 NJ]
inline void plant_pack_gains(const hsqp_plant_settings& s, double* g) {
  for (int j = 0; j < NJ; ++j) { g[j] = s.kp[j]; g[NJ + j] = s.kd[j]; g[2 * NJ + j] = s.armature[j]; }
}

struct PlantWS {
  const double* xt;                 // nominal states of THIS instance
  double lookahead;
  double kp[NJ], kd[NJ], arm[NJ];
  double xp[NX];                    // policy state at s + lookahead
  double tau[NJ];                   // feed-forward torques, then the joint law's torques
  double Ic[NB][10], fc[NB][6];     // composites of In / f over the subtrees
  double Fc[NV][6];                 // I^c_c S_c per coordinate
  double A[PL_N][PL_LD];            // the bordered system, then its Cholesky factor (lower)
  double l[PL_N];                   // the scaled pivot column of one elimination step
  double dinv[NV];                  // reciprocals of the factor's diagonal
  double vd[NV];                    // the accelerations
};

// The stage workspace of the torque plant: the flow map's, and the plant's own
struct PlantStage {
  StageWST<false> st;
  PlantWS pl;
};
// ... and of the torque plant on the ground of include/hsqp_contact.h: contact is a parameter of the instantiation, not a run-time branch — the plant
// without a ground is the code and the workspace it was before there was one
struct PlantContactStage {
  StageWST<false> st;
  PlantWS pl;
  ContactSet ct;                    // the instance's ground and the contact points of one evaluation
};

// ... and either of them under the actuator model of include/hsqp_actuator.h: again a parameter of the instantiation — the two above are the code and
// the workspace they were before there was one
struct PlantActStage {
  StageWST<false> st;
  PlantWS pl;
  ActuatorWS act;                   // the instance's actuator setting and the joint command in force
};
struct PlantContactActStage {
  StageWST<false> st;
  PlantWS pl;
  ContactSet ct;
  ActuatorWS act;
};

// ... and either grounded one on the height-map terrain of include/hsqp_terrain.h: the set carries the instance's map, the second contact_point of
// hsqp_contact.h reads it — again a parameter of the instantiation: the four above are the code and the workspace they were before there was a terrain
struct PlantTerrainStage {
  StageWST<false> st;
  PlantWS pl;
  ContactTerrainSet ct;
};
struct PlantTerrainActStage {
  StageWST<false> st;
  PlantWS pl;
  ContactTerrainSet ct;
  ActuatorWS act;
};

// ... and any of the six under the per-instance inertial variations of include/hsqp_inertia.h: once more a parameter of the instantiation — the four
// above are the code and the workspace they were before there was a table
template <class Base>
struct PlantVaried : Base {
  InertiaWS iw;                     // the instance's link scales and payloads
};
// whether the stage workspace carries the ground (ws.ct), the terrain (ws.ct.ter), the inertial variation (ws.iw)
template <class SW> struct PlantGrounded { static constexpr bool value = false; };
template <> struct PlantGrounded<PlantContactStage> { static constexpr bool value = true; };
template <> struct PlantGrounded<PlantContactActStage> { static constexpr bool value = true; };
template <> struct PlantGrounded<PlantTerrainStage> { static constexpr bool value = true; };
template <> struct PlantGrounded<PlantTerrainActStage> { static constexpr bool value = true; };
template <class Base> struct PlantGrounded<PlantVaried<Base>> : PlantGrounded<Base> {};
template <class SW> struct PlantOnTerrain { static constexpr bool value = false; };
template <> struct PlantOnTerrain<PlantTerrainStage> { static constexpr bool value = true; };
template <> struct PlantOnTerrain<PlantTerrainActStage> { static constexpr bool value = true; };
template <class Base> struct PlantOnTerrain<PlantVaried<Base>> : PlantOnTerrain<Base> {};
// the type of the ground's set in the stage workspace (of a workspace without a ground: the null pointer's)
template <class SW> struct PlantGroundSet { using type = typename std::conditional<PlantOnTerrain<SW>::value, ContactTerrainSet, ContactSet>::type; };
template <class SW> struct PlantIsVaried { static constexpr bool value = false; };
template <class Base> struct PlantIsVaried<PlantVaried<Base>> { static constexpr bool value = true; };

// instance b of the setting into the workspace
HSQP_HD void plant_load(const Ctx& ctx, const PlantParams& pp, int b, int N, PlantWS& pl) {
  WG_FOR(ctx, i, 3 * NJ + 1) {
    if (i == 3 * NJ) { pl.xt = pp.xt + (size_t)b * (N + 1) * NX; pl.lookahead = pp.lookahead; continue; }
    (i < NJ ? pl.kp[i] : (i < 2 * NJ ? pl.kd[i - NJ] : pl.arm[i - 2 * NJ])) = pp.gains[i];
  }
  WG_SYNC(ctx);
}

// (q, v, qdd_j, W) of one evaluation into the stage workspace
HSQP_HD void plant_inputs(const Ctx& ctx, StageWST<false>& ws, const double* x, const double* u, bool zero_qdd) {
  WG_FOR(ctx, i, NV + NV + NJ + 12) {
    if (i < NV) ws.q[i] = x[i];
    else if (i < 2 * NV) ws.v[i - NV] = x[i];
    else if (i < 2 * NV + NJ) ws.qddj[i - 2 * NV] = zero_qdd ? 0.0 : u[12 + i - 2 * NV];
    else ws.W[i - 2 * NV - NJ] = u[i - 2 * NV - NJ];
  }
  WG_SYNC(ctx);
}

// motion axis of generalised coordinate c
HSQP_HD void plant_axis(const StageWST<false>& ws, int c, double* s) {
  if (c < 3) { for (int k = 0; k < 6; ++k) s[k] = k == 3 + c ? 1.0 : 0.0; }
  else { for (int k = 0; k < 6; ++k) s[k] = ws.S[c - 3][k]; }
}
// the body whose subtree coordinate c moves, and one past the last body of that subtree
HSQP_HD int plant_body(int c) { return c < 6 ? 0 : c - 5; }
HSQP_HD int plant_end(const StageWST<false>& ws, int c) { return c < 6 ? NB : (c - 5) + (int)ws.sub[c - 5]; }

// vd [NV] (into pl.vd) of the plant at the state and the contact wrenches stage_eval<false> has just been run on (qdd_j = 0), under the joint
// torques pl.tau and the pushes `mask` of ps (0: none).  ct (null: none; a constant of the caller's instantiation, folded when this is inlined) —
// the ground of the instance (CT: ContactSet, or ContactTerrainSet on a height map): its contact forces replace the contact wrenches.  Ends with a barrier.
// SOLVE = false: the assembly only — the bordered system pl.A is left as it is filled: rows 0 .. NV - 1 the mass matrix with the armature pl.arm, both
// triangles; row NV the right-hand side; pl.Ic[0][0] the total mass.
template <bool SOLVE = true, class CT = ContactSet>
HSQP_HD void plant_forward_dynamics(const Ctx& ctx, const DevModel& dm, StageWST<false>& ws, PlantWS& pl, PushSet& ps, unsigned mask, CT* ct = nullptr) {
  // ---- composites over the subtrees; the wrench {P x f, f} about O of every active push and of every contact point
  WG_FOR(ctx, it, NB * 16 + HSQP_PUSH_MAX + (ct ? CT_PTS : 0)) {
    if (it >= NB * 16 + HSQP_PUSH_MAX) { contact_point(dm, ws, *ct, it - NB * 16 - HSQP_PUSH_MAX); continue; }
    if (it >= NB * 16) {
      const int i = it - NB * 16;
      if (!((mask >> i) & 1u)) continue;
      const int b = ps.body[i];
      double P[3], mom[3];
      m3_mulv(ws.R[b], ps.point[i], P);
      for (int k = 0; k < 3; ++k) P[k] += ws.r[b][k];
      v3_cross(P, ps.force[i], mom);
      for (int k = 0; k < 3; ++k) { ps.wr[i][k] = mom[k]; ps.wr[i][3 + k] = ps.force[i][k]; }
      continue;
    }
    const int b = it / 16, e = it % 16, end = b + (int)ws.sub[b];
    double s = 0.0;
    if (e < 10) { for (int i = b; i < end; ++i) s += ws.In[i][e]; pl.Ic[b][e] = s; }
    else { for (int i = b; i < end; ++i) s += ws.f[i][e - 10]; pl.fc[b][e - 10] = s; }
  }
  WG_SYNC(ctx);
  // ---- per coordinate: I^c S, and the right-hand side  tau - S . (f^c - contact wrenches (or contact forces) below - push wrenches below)  into the border row
  WG_FOR(ctx, c, NV + 1) {
    if (c == NV) { pl.A[NV][NV] = 0.0; continue; }   // (the border's corner: carried through the updates, never used)
    const int b = plant_body(c), end = plant_end(ws, c);
    double Sx[6], F[6];
    plant_axis(ws, c, Sx);
    inertia_apply(pl.Ic[b], Sx, pl.Fc[c]);
    for (int k = 0; k < 6; ++k) F[k] = pl.fc[b][k];
    for (int f = 0; f < 2; ++f) {
      const int cb = dm.contact_body[f];
      if (!(cb >= b && cb < end)) continue;
      if (!ct) { for (int k = 0; k < 6; ++k) F[k] -= ws.Fx[f][k]; continue; }
      for (int i = HSQP_CONTACT_CORNERS * f; i < HSQP_CONTACT_CORNERS * (f + 1); ++i)
        for (int k = 0; k < 6; ++k) F[k] -= ct->wr[i][k];
    }
    for (int i = 0; i < HSQP_PUSH_MAX; ++i) {
      if (!((mask >> i) & 1u)) continue;
      const int pb = ps.body[i];
      if (pb >= b && pb < end) for (int k = 0; k < 6; ++k) F[k] -= ps.wr[i][k];
    }
    double s = 0.0;
    for (int k = 0; k < 6; ++k) s += Sx[k] * F[k];
    pl.A[NV][c] = (c < 6 ? 0.0 : pl.tau[c - 6]) - s;
  }
  WG_SYNC(ctx);
  // ---- mass matrix: both triangles from the same expression (exactly symmetric), the armature on the joint diagonal
  WG_FOR(ctx, it, NV * NV) {
    const int i = it / NV, j = it % NV, r = i < j ? i : j, c = i < j ? j : i;
    const int bc = plant_body(c);
    double m = 0.0;
    if (r < 6 || (bc >= plant_body(r) && bc < plant_end(ws, r))) {
      double Sx[6];
      plant_axis(ws, r, Sx);
      for (int k = 0; k < 6; ++k) m += Sx[k] * pl.Fc[c][k];
    }
    if (i == j && i >= 6) m += pl.arm[i - 6];
    pl.A[i][j] = m;
  }
  WG_SYNC(ctx);
  if (!SOLVE) return;
  // ---- Cholesky of the leading NV x NV block, the border row eliminated along: after step k the border holds y_k = (L^-1 rhs)_k
  for (int k = 0; k < NV; ++k) {
    WG_FOR(ctx, i, PL_N - k) {
      const double piv = pl.A[k][k];
      const double inv = piv > 0.0 ? inv_sqrt(piv) : __builtin_nan("");
      pl.l[k + i] = pl.A[k + i][k] * inv;
      if (i == 0) pl.dinv[k] = inv;
    }
    WG_SYNC(ctx);
    const int n = PL_N - k;   // rows k .. NV: item (i, 0) stores the column, items (i, j), 1 <= j <= i, update the trailing block
    WG_FOR(ctx, it, n * n) {
      const int i = it / n, j = it % n;
      if (j > i) continue;
      if (j == 0) pl.A[k + i][k] = pl.l[k + i];
      else pl.A[k + i][k + j] -= pl.l[k + i] * pl.l[k + j];
    }
    WG_SYNC(ctx);
  }
  // ---- back substitution L^T vd = y
  WG_FOR(ctx, it, 1) {
    for (int k = NV - 1; k >= 0; --k) {
      double s = pl.A[NV][k];
      for (int i = k + 1; i < NV; ++i) s -= pl.A[i][k] * pl.vd[i];
      pl.vd[k] = s * pl.dinv[k];
    }
  }
  WG_SYNC(ctx);
}

// The workspace of hsqp_inertia_eval: the stage's, the plant's and the instance's variation (push: never read, the assembly runs with no push active)
struct InertiaEvalWS {
  StageWST<false> st;
  PlantWS pl;
  InertiaWS iw;
  PushSet push;
};

// hsqp_inertia_eval for one instance: the plant's inertial model at state x [58] with instance b of the table (null: the nominal model) — M [29][29]
// without armature, nle [29] (the right-hand side under tau = 0, no wrenches, no pushes, negated), mass [1]; any may be null
HSQP_HD void inertia_eval_instance(const Ctx& ctx, const DevModel& dm, InertiaEvalWS& w, const InertiaParams& ip, int b, const double* x, double* M, double* nle,
                                   double* mass) {
  stage_topology(ctx, dm, w.st, false);
  WG_FOR(ctx, i, NV + NV + NJ + 12 + 2 * NJ) {
    if (i < NV) w.st.q[i] = x[i];
    else if (i < 2 * NV) w.st.v[i - NV] = x[i];
    else if (i < 2 * NV + NJ) w.st.qddj[i - 2 * NV] = 0.0;
    else if (i < 2 * NV + NJ + 12) w.st.W[i - 2 * NV - NJ] = 0.0;
    else if (i < 2 * NV + 2 * NJ + 12) w.pl.tau[i - 2 * NV - NJ - 12] = 0.0;
    else w.pl.arm[i - 2 * NV - 2 * NJ - 12] = 0.0;
  }
  inertia_load(ctx, ip, b, w.iw);   // (its barrier closes the topology and the inputs)
  stage_eval<false>(ctx, dm, w.st);
  inertia_apply(ctx, w.st, w.iw);
  plant_forward_dynamics<false>(ctx, dm, w.st, w.pl, w.push, 0u);
  WG_FOR(ctx, it, NV * NV + NV + 1) {
    if (it < NV * NV) { if (M) M[it] = w.pl.A[it / NV][it % NV]; }
    else if (it < NV * NV + NV) { if (nle) nle[it - NV * NV] = -w.pl.A[NV][it - NV * NV]; }
    else if (mass) *mass = w.pl.Ic[0][0];
  }
}

}  // namespace hsqp
