// Riccati feedback policy (include/hsqp_feedback.h; upstream ocs2_sqp SqpSolver::setPrimalSolution with useFeedbackPolicy): the linear
// controller u = uff + K x of the last QP solved, in ocs2's LinearController convention.
//   The projected input step of node k is  du = Px dx + Pu ut + Pe  (QP record, hsqp_project.h) with  ut = K~ dx + k~  (Riccati record,
//   hsqp_riccati.h), so the gain of the full input is  K = Px + Pu K~  (35 x 58) and the bias is taken at the final trajectory:
//   uff = u - K x  (x, u: the resident solution d_xnew / d_unew after the step of the last iteration, whatever its length).
//   Only the first QP_NUT columns of Pu / rows of K~ enter the product: padded projected inputs contribute exactly nothing.  A centroidal
//   record has 35 live states: columns 35..57 of K are exactly zero.
//   Policy entries: nodes 0 .. N.  A PRE-event node i (0 < i, interval i an event, dts[i] == 0) carries no optimised input of its own and takes
//   the entry of node i - 1 (chained over consecutive events), node N the entry of node N - 1: the copies are bit copies.
// The same source builds for the host with a one-lane context (tests/feedback/feedback_emu.cpp).
#pragma once
#include "hsqp_linalg.h"
#include "hsqp_project.h"
#include "hsqp_riccati.h"

namespace hsqp {

// the node whose gains entry `i` (0 .. N) of the policy carries; dts: the instance's N interval lengths
HSQP_HD int feedback_source_node(const double* dts, int N, int i) {
  int k = i < N ? i : N - 1;
  while (k > 0 && dts[k] == 0.0) --k;
  return k;
}

// Where the policy is evaluated at s seconds after the first node (MPC_MRT_Interface::evaluatePolicy on the PrimalSolution stamps):
// the state blends nodes kx, kx + 1 with weight ax, the input (and the feedback entries) nodes ku, ku + 1 with weight au.
// Shared with the feed-forward evaluation (hsqp_policy.h), so that both take the same segment.
struct PolicySegment { int kx; double ax; int ku; double au; };

// uniform grid of spacing dt
HSQP_HD PolicySegment policy_segment_uniform(int N, double dt, double s) {
  double a = s / dt;
  if (a < 0.0) a = 0.0;
  int kx = (int)a;
  if (kx > N - 1) kx = N - 1;
  double ax = a - kx;
  if (ax > 1.0) ax = 1.0;
  int ku = (int)a;
  double au = a - ku;
  if (ku > N - 2) { ku = N - 2 > 0 ? N - 2 : 0; au = N >= 2 ? (a - ku > 1.0 ? 1.0 : a - ku) : 0.0; }
  return PolicySegment{kx, ax, ku, au};
}

// non-uniform grid (hsqp_problem::dt_nodes; zero-length event intervals): node k of the state trajectory sits at t_k = sum_{i<k} dts[i], the
// inputs at t_0 .. t_{N-1}.  At an event time the post-event node is taken (the last node with t_k <= s).
HSQP_HD PolicySegment policy_segment_grid(int N, const double* dts, double s) {
  if (s < 0.0) s = 0.0;
  double tk = 0.0;       // start of interval kx
  int kx = 0;
  while (kx < N - 1 && tk + dts[kx] <= s) { tk += dts[kx]; ++kx; }
  while (kx < N - 1 && dts[kx] == 0.0) ++kx;              // never interpolate across a jump
  const double h = dts[kx];
  double ax = h > 0.0 ? (s - tk) / h : 1.0;
  if (ax > 1.0) ax = 1.0;
  // inputs: stamps t_0 .. t_{N-1}; beyond the last stamp the last input is held
  int ku = kx;
  double au = ax;
  if (ku > N - 2) { ku = N - 2 > 0 ? N - 2 : 0; au = N >= 2 ? 1.0 : 0.0; }
  if (N >= 2 && dts[ku] == 0.0) au = 1.0;
  // node ku + 1 is a PRE-event node when interval ku + 1 is an event: it carries no optimised input of its own (du = 0 there;
  // upstream multiple_shooting::toPrimalSolution gives it the input of the node before), so the input is held up to the switch
  else if (N >= 2 && ku + 1 <= N - 1 && dts[ku + 1] == 0.0) au = 0.0;
  return PolicySegment{kx, ax, ku, au};
}

constexpr int LDPU = NU + 1;   // leading dimension of Pu^T in LDS
struct FeedbackWS {
  double K[NU][NX];            // gain of the entry
  double PuT[NUT][LDPU];       // Pu of the node, transposed: the matrix-core products are X^T Y
  double uff[NU];
};

// Gain K (into w.K) and bias uff (into w.uff) of one node from its QP record qp, Riccati record ric, state x and input u.
// cent: centroidal record (35 live states).  Ends with a barrier.
HSQP_HD void feedback_node(const Ctx& ctx, const double* qp, const double* ric, const double* x, const double* u, int cent, FeedbackWS& w) {
  const int nc = cent ? HSQP_CNX : NX;
  int nut = (int)qp[QP_NUT];                 // (-1: rank-deficient D, reported through the numeric status)
  nut = nut < 0 ? 0 : (nut > NUT ? NUT : nut);
  WG_FOR(ctx, i, NU * NUT) w.PuT[i % NUT][i / NUT] = qp[QP_PU + i];
  WG_FOR(ctx, i, NU * (NX - nc)) w.K[i / (NX - nc)][nc + i % (NX - nc)] = 0.0;
  WG_SYNC(ctx);
  // K = Px + Pu K~ over the live projected inputs: 3 x 4 tiles of 16 x 16, ceil(nut / 4) steps of 4
  const XtyJob job = xty_job(NU, nc, nut, &w.PuT[0][0], LDPU, ric + RIC_K, NX, &w.K[0][0], NX, qp + QP_PX, NX);
  wg_xty_jobs(ctx, &job, 1);
  WG_SYNC(ctx);
  WG_FOR(ctx, r, NU) {
    double kx = 0.0;
    for (int c = 0; c < nc; ++c) kx += w.K[r][c] * x[c];
    w.uff[r] = u[r] - kx;
  }
  WG_SYNC(ctx);
}

}  // namespace hsqp
