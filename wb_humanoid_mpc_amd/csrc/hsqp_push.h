// External pushes on the plant of the rollout (include/hsqp_push.h): the resident table as the kernel sees it, one instance's pushes in the
// rollout workspace, the break-point search and the activity of a segment.  Everything here is uniform across the workgroup: the set is
// read from LDS after a barrier and every thread runs the same scalar code on it.
#pragma once
#include "hsqp_common.h"
#include "../../include/hsqp_push.h"

namespace hsqp {

// The resident table (n null: no table — nothing else is read)
struct PushTable {
  const int32_t* n;        // [B]
  const hsqp_push* p;      // [B][max_pushes]
  int max_pushes;
  const double* stamps;    // raw stamps of the resident grid, row stride `stride` (null: the first node is at 0)
  int stride;
};

// The pushes of ONE instance in rollout time (seconds after the first node), read once at the start of rollout_instance
struct PushSet {
  int n;                               // 0: no push — the rollout takes the unpushed path
  int body[HSQP_PUSH_MAX];
  double e0[HSQP_PUSH_MAX], e1[HSQP_PUSH_MAX];   // edges; a push with e1 <= e0 (or a body outside the tree) is inert: stored as e0 = e1 = 0
  double point[HSQP_PUSH_MAX][3], force[HSQP_PUSH_MAX][3];
  double wr[HSQP_PUSH_MAX][6];         // per push of one flow evaluation: its wrench about the base origin {moment, force} / its share of the momentum rate
};

// instance b of the table into the workspace (tbl.n null: the empty set).  The edges are formed once, here.
HSQP_HD void push_load(const Ctx& ctx, const PushTable& tbl, int b, PushSet& s) {
  WG_FOR(ctx, i, HSQP_PUSH_MAX + 1) {
    int n = 0;
    if (tbl.n) { n = tbl.n[b]; n = n < 0 ? 0 : (n > tbl.max_pushes ? tbl.max_pushes : n); }
    if (i == HSQP_PUSH_MAX) { s.n = n; continue; }
    if (i >= n) continue;
    const hsqp_push& p = tbl.p[(size_t)b * tbl.max_pushes + i];
    const double t0 = tbl.stamps ? tbl.stamps[(size_t)b * tbl.stride] : 0.0;
    const double e0 = p.t_start - t0, e1 = (p.t_start + p.duration) - t0;
    const bool live = e0 < e1 && p.body >= 0 && p.body < NB;
    s.body[i] = live ? p.body : 0;
    s.e0[i] = live ? e0 : 0.0;
    s.e1[i] = live ? e1 : 0.0;
    for (int k = 0; k < 3; ++k) { s.point[i][k] = p.point[k]; s.force[i][k] = p.force[k]; }
  }
  WG_SYNC(ctx);
}

// the first edge of a push strictly inside (t, tb), else tb
HSQP_HD double push_next_edge(const PushSet& s, double t, double tb) {
  double te = tb;
  for (int i = 0; i < s.n; ++i) {
    if (!(s.e0[i] < s.e1[i])) continue;
    if (s.e0[i] > t && s.e0[i] < te) te = s.e0[i];
    if (s.e1[i] > t && s.e1[i] < te) te = s.e1[i];
  }
  return te;
}

// bit i: push i is active on the segment that starts at ts (edge_start <= ts < edge_end)
HSQP_HD unsigned push_active(const PushSet& s, double ts) {
  unsigned m = 0;
  for (int i = 0; i < s.n; ++i)
    if (s.e0[i] <= ts && ts < s.e1[i]) m |= 1u << i;
  return m;
}

}  // namespace hsqp
