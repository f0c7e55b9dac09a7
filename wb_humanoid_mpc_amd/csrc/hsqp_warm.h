// Receding-horizon warm start on the device (hsqp_reference::warm_start, include/hsqp.h): the linearisation trajectory of the
// next MPC cycle built from the solution resident in the handle, as HipSqpSolverAdaptor::runImpl builds it on the host
// (steps 2 and 5, upstream ocs2 SqpSolver::runImpl):
//   - the previous primal solution, linearly interpolated (clamped, std::upper_bound on its raw time stamps) onto the new grid;
//     its inputs are the STAMPED ones of PrimalSolution: input j = u[min(j, N - 1)], and a pre-event node (zero-length interval j,
//     0 < j < N) carries the input of the node before it (upstream multiple_shooting::toPrimalSolution);
//   - the nodes past the last stamp T of the previous solution from the reference's WeightCompInitializer
//     (humanoid_common_mpc/src/initialization/WeightCompInitializer.cpp:66-70): the state of the node before (x_init for node 0),
//     the weight-compensating input of the node's contact flags (row k of the node-parameter table, written by k_params).
// COLD is the same with no previous solution.  Raw stamps: at an event the pre- and the post-event node share one stamp; the
// post-event node's sampling time (t_event + kEventEps) is replaced by the stamp of the node before it, never by a subtraction.
//
// Bit-exactness with the host: every blend (1 - a) v0 + a v1 and the uniform stamp t0 + k dt are evaluated unfused
// (`#pragma clang fp contract(off)` in each function that does arithmetic; hipcc contracts device code by default), the
// interpolation weight by an IEEE division, the weight compensation as total_mass * 9.81 / n_stance like hsqp_node.h.
// The same source compiles for the host with a one-lane context (tests/warm/warm_emu.cpp, -ffp-contract=off).
#pragma once
#include "hsqp_common.h"

namespace hsqp {

struct WarmArgs {
  int mode;                  // HSQP_WARM_CALLER (stamps only), HSQP_WARM_SHIFT, HSQP_WARM_COLD
  const int* mode_b;         // [B] HSQP_WARM_SHIFT / _COLD per instance (the isolated loop, include/hsqp_episode.h), or null: `mode` for all
  int B, N, N_prev;          // batch, intervals of the new grid, intervals of the previous solution
  int cent;                  // centroidal handle: entries HSQP_CNX.. of a state row are zero
  double t0, dt;             // uniform grid (node_times == null)
  double total_mass;         // DevModel::total_mass
  const double* node_times;  // [B][N+1] sampling times of the new grid, or null
  const double* dts;         // [B][N]   interval lengths of the new grid (0: event)
  const double* par;         // [B][N+1][NP] node parameters of the new grid (contact flags)
  const double* x_init;      // [B][NX]
  const double* x_prev;      // [B][N_prev+1][NX] previous solution
  const double* u_prev;      // [B][N_prev][NU]
  const double* stamps_prev; // [B][N_prev+1] raw stamps of the previous solution (the kernel stages an instance's row in LDS)
  double* x;                 // [B][N+1][NX] out: linearisation trajectory
  double* u;                 // [B][N][NU]
  double* stamps;            // [B][N+1] out: raw stamps of the new grid
};

// the mode of instance b.  A COLD instance reads nothing of the previous solution (x_prev, u_prev, stamps_prev): it may be NaN.
HSQP_HD int warm_mode(const WarmArgs& w, int b) { return w.mode_b ? w.mode_b[b] : w.mode; }

// raw stamp of node k of instance b of the new grid
HSQP_HD double warm_stamp(const WarmArgs& w, int b, int k) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (!w.node_times) return w.t0 + (double)k * w.dt;
  const double* d = w.dts + (size_t)b * w.N;
  while (k > 0 && d[k - 1] == 0.0) --k;   // a post-event node takes the stamp of the node before it
  return w.node_times[(size_t)b * (w.N + 1) + k];
}

// std::upper_bound over t[0..n): the first index whose stamp is greater than tau
HSQP_HD int warm_upper_bound(const double* t, int n, double tau) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (t[mid] > tau) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// stamped input j of the previous solution -> row of u_prev (tp: its N_prev + 1 raw stamps)
HSQP_HD int warm_input_row(const double* tp, int N_prev, int j) {
  int r = j < N_prev - 1 ? j : N_prev - 1;
  while (r > 0 && tp[r + 1] == tp[r]) --r;   // pre-event node: the input of the node before it
  return r;
}

// Where a row of the previous solution is sampled at tau: front / back row (copied) or the blend of rows i-1, i with weight a.
struct WarmSample { int lo, hi; double a; };
HSQP_HD WarmSample warm_locate(const double* tp, int N_prev, double tau) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (tau <= tp[0]) return WarmSample{0, 0, 0.0};
  if (tau >= tp[N_prev]) return WarmSample{N_prev, N_prev, 0.0};
  const int i = warm_upper_bound(tp, N_prev + 1, tau);   // tp[i-1] <= tau < tp[i]
  const double h = tp[i] - tp[i - 1];
  return WarmSample{i - 1, i, h > 0.0 ? (tau - tp[i - 1]) / h : 1.0};
}
HSQP_HD double warm_blend(const WarmSample& s, double v0, double v1) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return s.lo == s.hi ? v0 : (1.0 - s.a) * v0 + s.a * v1;
}

// Node k of instance b: the raw stamp, and (SHIFT / COLD) the state row and, for k < N, the input row.  ctx: the lanes of one
// wave (one lane on the host).  tp: the previous solution's N_prev + 1 stamps of instance b (LDS on the device); unused for COLD.
HSQP_HD void warm_node(const Ctx& ctx, const WarmArgs& w, const double* tp, int b, int k) {
  const int N = w.N, Np = w.N_prev;
  const double tau = warm_stamp(w, b, k);
  if (ctx.tid == 0) w.stamps[(size_t)b * (N + 1) + k] = tau;
  const int mode = warm_mode(w, b);
  if (mode == HSQP_WARM_CALLER) return;
  const bool shift = mode == HSQP_WARM_SHIFT;
  const double T = shift ? tp[Np] : 0.0;
  const bool covered = shift && tau <= T;
  // the state: interpolated at node src's stamp; a node past T keeps the state of the last covered node before it (src), x_init
  // if there is none (the serial chain x_k = x_{k-1} of the initializer, resolved without a chain: the stamps do not decrease)
  int src = k;
  if (!covered) {
    int lo = 0, hi = shift ? k : 0;   // covered nodes form a prefix [0, lo)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (warm_stamp(w, b, mid) <= T) lo = mid + 1;
      else hi = mid;
    }
    src = lo - 1;
  }
  double* xo = w.x + ((size_t)b * (N + 1) + k) * NX;
  const int nx = w.cent ? HSQP_CNX : NX;
  if (src < 0) {
    const double* x0 = w.x_init + (size_t)b * NX;
    WG_FOR(ctx, i, NX) xo[i] = i < nx ? x0[i] : 0.0;
  } else {
    const WarmSample s = warm_locate(tp, Np, src == k ? tau : warm_stamp(w, b, src));
    const double* x0 = w.x_prev + ((size_t)b * (Np + 1) + s.lo) * NX;
    const double* x1 = w.x_prev + ((size_t)b * (Np + 1) + s.hi) * NX;
    WG_FOR(ctx, i, NX) xo[i] = i < nx ? warm_blend(s, x0[i], x1[i]) : 0.0;
  }
  if (k == N) return;
  double* uo = w.u + ((size_t)b * N + k) * NU;
  if (covered) {
    const WarmSample s = warm_locate(tp, Np, tau);
    const double* u0 = w.u_prev + ((size_t)b * Np + warm_input_row(tp, Np, s.lo)) * NU;
    const double* u1 = w.u_prev + ((size_t)b * Np + warm_input_row(tp, Np, s.hi)) * NU;
    WG_FOR(ctx, i, NU) uo[i] = warm_blend(s, u0[i], u1[i]);
  } else {
    // weightCompensatingInput (DynamicsHelperFunctions.h:178-193) of the node's contact flags, the expression of hsqp_node.h
    const double* pr = w.par + ((size_t)b * (N + 1) + k) * NP;
    const int c0 = pr[HSQP_P_CONTACT] > 0.5, c1 = pr[HSQP_P_CONTACT + 1] > 0.5;
    WG_FOR(ctx, i, NU) uo[i] = ((i == 2 && c0) || (i == 8 && c1)) ? w.total_mass * 9.81 / (c0 + c1) : 0.0;
  }
}

}  // namespace hsqp
