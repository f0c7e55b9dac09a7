// Riccati value function (include/hsqp_value.h; upstream ocs2_sqp SqpSolver::getValueFunction with createValueFunction): the quadratic
// cost-to-go  V_k(dx) = s_k^T dx + 1/2 dx^T S_k dx,  dx = x - xbar_k,  of the last QP solved, read from the record the backward sweeps leave
// (vf [N + 1][VF_SIZE]: S_k row-major with leading dimension NX, then s_k; hsqp_riccati.h) and the snapshot xbar [N + 1][NX] of the trajectory
// the QP was linearised at.
//   value_record_node: one node of the record as the public interface hands it out — S symmetrised, 1/2 (S + S^T), centroidal padding zeroed.
//   value_eval:        one query (s, x) — the state segment and weight of the policy evaluation (policy_segment_*, hsqp_feedback.h), S, s and
//                      xbar blended linearly between the segment's two nodes, then dfdx = s + S dx, dfdxx = S, dV = s^T dx + 1/2 dx^T S dx.
//                      Each node's S is symmetrised FIRST and the two symmetric blocks are blended, so a query evaluated from the record
//                      value_record_node hands out gives the same bits as one evaluated from the sweep's own.
// Memory: a query streams the two nodes' S blocks once (2 x 26.9 KB, 16 bytes per lane and load on the device) into LDS and symmetrises and
// blends from there; the kernel is bound by that traffic, the products are plain vector arithmetic.
// Arithmetic: every product-sum is evaluated unfused (`#pragma clang fp contract(off)`; hipcc contracts device code by default) and every sum
// runs in an order fixed by the item index — a row's product over four interleaved column classes p = c mod 4, combined (p0 + p1) + (p2 + p3);
// dV the same over the rows — so the device, the host build of this source (tests/value/value_emu.cpp, -ffp-contract=off) and the numpy mirror
// (tests/value_ref.py: evaluate_mirror) agree bit for bit.
#pragma once
#include "hsqp_feedback.h"   // PolicySegment, policy_segment_*
#include "../../include/hsqp_value.h"

namespace hsqp {

constexpr int VAL_THREADS = 256;
constexpr int VAL_LD = NX + 1;   // odd leading dimension: the transposed read S[c][r] of the symmetrisation walks the LDS banks
struct ValueWS {
  double S[2][NX][VAL_LD];       // S of the segment's two nodes as stored by the sweep, padding zeroed
  double sb[NX], dx[NX], q[NX];  // blended s, x - xbar, the rows' terms of dV
  double part[NX][4];            // a row's partial products over the column classes c mod 4
};
static_assert(sizeof(ValueWS) <= 65536, "the value-function kernels run without a dynamic-LDS attribute");

// two consecutive doubles of a record (p is 16-byte aligned on the device: VF_SIZE * 8 and the pair offsets are multiples of 16)
HSQP_HD void value_load2(const double* p, double& a, double& b) {
#if defined(__HIP_DEVICE_COMPILE__)
  const double2 v = *reinterpret_cast<const double2*>(p);
  a = v.x; b = v.y;
#else
  a = p[0]; b = p[1];
#endif
}

// w.S[e] = the S of node record v with the padding zeroed.  No barrier.
HSQP_HD void value_load_S(const Ctx& ctx, const double* v, int nc, int e, ValueWS& w) {
  static_assert((NX * NX) % 2 == 0 && NX % 2 == 0 && VF_SIZE % 2 == 0, "pairs of a record never straddle a row of S or two nodes");
  WG_FOR(ctx, i, NX * NX / 2) {
    double p0, p1;
    value_load2(v + 2 * i, p0, p1);
    const int r = (2 * i) / NX, c = (2 * i) % NX;
    w.S[e][r][c] = (r < nc && c < nc) ? p0 : 0.0;
    w.S[e][r][c + 1] = (r < nc && c + 1 < nc) ? p1 : 0.0;
  }
}
// entry (r, c) of 1/2 (S + S^T) of node e of the segment
HSQP_HD double value_sym(const ValueWS& w, int e, int r, int c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return 0.5 * (w.S[e][r][c] + w.S[e][c][r]);
}

// One node of the record: S_out [NX][NX] = 1/2 (S + S^T), s_out [NX], xbar_out [NX] (any may be null).  v: the node's VF_SIZE doubles,
// xb: its row of the snapshot.
HSQP_HD void value_record_node(const Ctx& ctx, const double* v, const double* xb, int cent, double* S_out, double* s_out, double* xbar_out, ValueWS& w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int nc = cent ? HSQP_CNX : NX;
  if (S_out) value_load_S(ctx, v, nc, 0, w);
  WG_SYNC(ctx);
  if (S_out) WG_FOR(ctx, i, NX * NX) S_out[i] = value_sym(w, 0, i / NX, i % NX);
  if (s_out) WG_FOR(ctx, i, NX) s_out[i] = i < nc ? v[NX * NX + i] : 0.0;
  if (xbar_out) WG_FOR(ctx, i, NX) xbar_out[i] = xb[i];
}

// One query.  vf [N + 1][VF_SIZE], xbar [N + 1][NX], dts [N] (null: the uniform grid of spacing dt): the instance's rows; xq [NX];
// dV [1], dfdx [NX], dfdxx [NX][NX]: the query's outputs, any may be null.
HSQP_HD void value_eval(const Ctx& ctx, const double* vf, const double* xbar, const double* dts, int N, double dt, int cent, double sq, const double* xq,
                        double* dV, double* dfdx, double* dfdxx, ValueWS& w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  // (uniform grid: every s >= N dt takes the last segment with weight 1; 2 N dt stands for all of them, so that s / dt always fits the rule's int)
  if (!dts && sq > 2.0 * N * dt) sq = 2.0 * N * dt;
  const PolicySegment g = dts ? policy_segment_grid(N, dts, sq) : policy_segment_uniform(N, dt, sq);
  const int k = g.kx < 0 ? 0 : (g.kx > N - 1 ? N - 1 : g.kx);   // (the segment rule keeps kx in [0, N - 1] for every finite s; no s reads outside the record)
  const double a1 = g.ax, a0 = 1.0 - g.ax;
  const int nc = cent ? HSQP_CNX : NX;
  const double* v0 = vf + (size_t)k * VF_SIZE;
  const double* x0 = xbar + (size_t)k * NX;
  value_load_S(ctx, v0, nc, 0, w);
  value_load_S(ctx, v0 + VF_SIZE, nc, 1, w);
  WG_FOR(ctx, i, NX) {
    w.sb[i] = i < nc ? a0 * v0[NX * NX + i] + a1 * v0[VF_SIZE + NX * NX + i] : 0.0;
    w.dx[i] = i < nc ? xq[i] - (a0 * x0[i] + a1 * x0[NX + i]) : 0.0;
  }
  WG_SYNC(ctx);
  WG_FOR(ctx, i, NX * 4) {
    const int r = i >> 2, p = i & 3;
    double acc = 0.0;
    for (int c = p; c < NX; c += 4) acc += (a0 * value_sym(w, 0, r, c) + a1 * value_sym(w, 1, r, c)) * w.dx[c];
    w.part[r][p] = acc;
  }
  if (dfdxx) WG_FOR(ctx, i, NX * NX) dfdxx[i] = a0 * value_sym(w, 0, i / NX, i % NX) + a1 * value_sym(w, 1, i / NX, i % NX);
  WG_SYNC(ctx);
  WG_FOR(ctx, r, NX) {
    const double Sdx = (w.part[r][0] + w.part[r][1]) + (w.part[r][2] + w.part[r][3]);
    if (dfdx) dfdx[r] = w.sb[r] + Sdx;
    w.q[r] = w.dx[r] * (w.sb[r] + 0.5 * Sdx);
  }
  WG_SYNC(ctx);
  if (dV) WG_FOR(ctx, i, 1) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int r = 0; r < NX; r += 4) {
      s0 += w.q[r];
      if (r + 1 < NX) s1 += w.q[r + 1];
      if (r + 2 < NX) s2 += w.q[r + 2];
      if (r + 3 < NX) s3 += w.q[r + 3];
    }
    dV[0] = (s0 + s1) + (s2 + s3);
  }
}

}  // namespace hsqp
