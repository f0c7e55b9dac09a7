// Per-instance inertial variations of the torque plant of the rollout (include/hsqp_inertia.h): the resident table as the kernel sees it, one
// instance's link scales and payloads in the rollout workspace, and the one phase that applies them.
//   inertia_load     instance b of the table into the workspace (the varied instantiations of the rollout kernel only: the handle launches them
//                    while a table is set, so the plant's other instantiations carry none of this)
//   inertia_apply    between stage_eval<false> at the plant's own state and the composites of plant_forward_dynamics (hsqp_plant.h): what stage_eval leaves —
//                    the spatial inertia In[i] about the base origin O and the net force f[i] of every body — is linear in the body's inertial
//                    parameters, so link i times s_i is In[i] *= s_i, f[i] *= s_i, and a payload on link i adds its own In and f, formed as
//                    stage_eval forms a body's from (m, R_i com + r_i, R_i I R_i^T) and the link's vl / al.  One item per link: item i writes rows i
//                    only, so there are no atomics and no second phase.  A scale of 1.0 changes no bit, a payload past n is not looked at.
// stage_eval and the iteration kernels are untouched: nothing here is seen by any user of stage_eval other than the plant.
// Everything is uniform across the workgroup; the same source builds for the host with a one-lane context (tests/inertia/inertia_emu.cpp).
#pragma once
#include "hsqp_model.h"
#include "../../include/hsqp_inertia.h"

namespace hsqp {

constexpr int IN_PAY = HSQP_INERTIA_PAYLOADS;

// The resident table, as the kernels that have one see it
struct InertiaParams {
  const hsqp_inertia_instance* table;   // [max_batch] the entry of every instance (past the table's batch: neutral), or null: none
};

// ONE instance's scales and payloads
struct InertiaWS {
  double scale[NB];
  int n, body[IN_PAY];
  double mass[IN_PAY], com[IN_PAY][3], I[IN_PAY][9];   // I: the full symmetric matrix about the payload's com, link axes
};

// instance b of the table into the workspace (no table: the neutral entry).  Ends with a barrier.
HSQP_HD void inertia_load(const Ctx& ctx, const InertiaParams& ip, int b, InertiaWS& iw) {
  const hsqp_inertia_instance* e = ip.table ? ip.table + b : nullptr;
  WG_FOR(ctx, i, NB + IN_PAY + 1) {
    if (i < NB) { iw.scale[i] = e ? e->mass_scale[i] : 1.0; continue; }
    if (i == NB + IN_PAY) {   // (a table from the device is not checked: the count is kept inside the arrays)
      const int n = e ? (int)e->n_payloads : 0;
      iw.n = n < 0 ? 0 : (n > IN_PAY ? IN_PAY : n);
      continue;
    }
    const int p = i - NB;
    if (!e) { iw.body[p] = -1; continue; }
    const hsqp_inertia_payload& pl = e->payload[p];
    iw.body[p] = (int)pl.body;
    iw.mass[p] = pl.mass;
    for (int k = 0; k < 3; ++k) iw.com[p][k] = pl.com[k];
    const double* J = pl.inertia;   // xx, xy, xz, yy, yz, zz
    double* I = iw.I[p];
    I[0] = J[0]; I[1] = J[1]; I[2] = J[2]; I[3] = J[1]; I[4] = J[3]; I[5] = J[4]; I[6] = J[2]; I[7] = J[4]; I[8] = J[5];
  }
  WG_SYNC(ctx);
}

// payload p, rigidly attached to link i: its spatial inertia about O and its net force join the link's (the inertia items of stage_eval, restated)
HSQP_HD void inertia_payload(StageWST<false>& ws, const InertiaWS& iw, int p, int i) {
  const double* Rb = ws.R[i];
  double c[3], t[9], Iw[9];
  m3_mulv(Rb, iw.com[p], c);
  for (int k = 0; k < 3; ++k) c[k] += ws.r[i][k];
  m3_mul(Rb, iw.I[p], t);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) Iw[3 * a + b] = t[3 * a] * Rb[3 * b] + t[3 * a + 1] * Rb[3 * b + 1] + t[3 * a + 2] * Rb[3 * b + 2];
  const double m = iw.mass[p], cc = v3_dot(c, c);
  double In[10];
  In[0] = m; In[1] = m * c[0]; In[2] = m * c[1]; In[3] = m * c[2];
  In[4] = Iw[0] + m * (cc - c[0] * c[0]); In[5] = Iw[1] - m * c[0] * c[1]; In[6] = Iw[2] - m * c[0] * c[2];
  In[7] = Iw[4] + m * (cc - c[1] * c[1]); In[8] = Iw[5] - m * c[1] * c[2]; In[9] = Iw[8] + m * (cc - c[2] * c[2]);
  const int jc = i + 2;
  double h[6], fa[6], fv[6];
  inertia_apply(In, ws.vl[jc], h);
  inertia_apply(In, ws.al[jc], fa);
  mxf(ws.vl[jc], h, fv);
  for (int e = 0; e < 10; ++e) ws.In[i][e] += In[e];
  for (int k = 0; k < 6; ++k) ws.f[i][k] += fa[k] + fv[k];
}

// the instance's variation on what stage_eval<false> has just left in ws.  Ends with a barrier.
HSQP_HD void inertia_apply(const Ctx& ctx, StageWST<false>& ws, const InertiaWS& iw) {
  WG_FOR(ctx, i, NB) {
    const double s = iw.scale[i];
    for (int e = 0; e < 10; ++e) ws.In[i][e] *= s;
    for (int k = 0; k < 6; ++k) ws.f[i][k] *= s;
    for (int p = 0; p < iw.n; ++p)
      if (iw.body[p] == i) inertia_payload(ws, iw, p, i);
  }
  WG_SYNC(ctx);
}

}  // namespace hsqp
