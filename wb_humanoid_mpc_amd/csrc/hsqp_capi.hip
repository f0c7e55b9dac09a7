// C ABI (include/hsqp.h) of the MI355X SQP library: HIP kernels + host orchestration.
// Product path: there is NO CPU fallback — without a usable HIP device every entry point fails with
// HSQP_ERR_NO_DEVICE / HSQP_ERR_HIP.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <type_traits>
#include <string>
#include <vector>

#include "hsqp_host.h"
#include "hsqp_riccati.h"
#include "hsqp_riccati_fact.h"
#include "hsqp_params.h"
#include "hsqp_policy.h"
#include "hsqp_feedback.h"
#include "../../include/hsqp_feedback.h"
#include "hsqp_value.h"
#include "hsqp_rollout.h"
#include "hsqp_loop.h"
#include "../../include/hsqp_loop.h"
#include "hsqp_cent_loop.h"
#include "../../include/hsqp_cent_loop.h"
#include "hsqp_gait.h"
#include "hsqp_grid.h"
#include "hsqp_ground.h"
#include "hsqp_perceive.h"
#include "hsqp_episode.h"
#include "hsqp_metrics.h"
#include "hsqp_observe.h"
#include "hsqp_warm.h"
#include "hsqp_cent.h"
#include "hsqp_cent_lq.h"
#include "hsqp_scan.h"
#include "hsqp_segment.h"
#include "hsqp_lqv.h"
#include "hsqp_lql.h"
#include "hsqp_carve.h"

using namespace hsqp;

namespace {

// launch shapes of the LQ kernels
constexpr int LQ_THREADS = 128, LQ_WPE = 2;    // 40 KB workspace: 4 workgroups of 2 waves per CU, no register spills
constexpr int LQV_THREADS = 64, LQV_WPE = 2;   // value-only pass (19.2 KB workspace: 8 one-wave workgroups per CU): its phases rarely have more than one wave
                                               // of work; one wave needs no barrier hardware (A/B: 0.95 vs 0.99 ms)

constexpr size_t VALUE_QUAD_MIN_NODES = 2048;   // handles sized below this keep the phase form of the whole-body value pass (hsqp_create)
constexpr size_t LQ_LIMB_MIN_NODES = 2048;      // handles sized below this keep the phase form of the whole-body LQ kernel (hsqp_create)
constexpr int PROJ_THREADS = 256, PROJ_WPE = 3;   // 49.5 KB workspace: three workgroups of four waves per CU
static_assert(PROJ_THREADS == 256 && PROJ_THREADS - hsqp::GRAM_BP >= 192, "gram_rows (hsqp_project.h): four waves carry the fifteen tiles, the border pairs sit on the last lanes of wave 3");
static_assert(PROJ_THREADS >= 256 && PROJ_THREADS % 64 == 0, "project_node hoists its staging loads assuming >= 256 threads; the Gram tiles are dealt to waves 0..3");
// Every kernel hands its workgroup size to the device functions as the CONSTANT it is launched with (Ctx::nthreads), not as blockDim.x: the item loops
// (WG_FOR) then have constant strides and trip counts, and the paths written for other workgroup shapes (the host build's) are not compiled into the
// kernels — k_riccati alone shrank from 16.7 k to 9 k instructions and from 1.518 to 1.463 ms (256 instances; 1.378 -> 1.317 at 32).
constexpr int RIC_THREADS = 512;
static_assert(sizeof(LqWST<false>) <= 163840 / 8, "value-only workspace: eight workgroups per CU");

extern __shared__ __attribute__((aligned(16))) unsigned char hsqp_smem[];

// ---- test aid (HSQP_POISON_LDS in the environment at hsqp_create: hsqp_handle::poison_lds): every kernel launch of the handle is preceded by one that fills the LDS of every CU
// with NaN bit patterns.  LDS keeps what the previous kernel left there, so a kernel that reads a word it never wrote (say a padding row that is
// "multiplied by zero") works until the leftover happens to be a NaN — tests/test_gpu_parity.py runs the iteration with and without the poison
// and asks for the same bits.
constexpr int POISON_LDS_BYTES = 163400;   // what hipFuncSetAttribute(MaxDynamicSharedMemorySize) accepts on gfx950: one such workgroup per CU at a time
__global__ __launch_bounds__(256) void k_poison_lds() {
  volatile unsigned long long* p = reinterpret_cast<volatile unsigned long long*>(hsqp_smem);
  for (int i = threadIdx.x; i < POISON_LDS_BYTES / 8; i += 256) p[i] = 0x7ff8dead7ff8deadull;   // a NaN as a double and as two floats
}
// every kernel launch of the library: `h` is the handle in scope
#define HSQP_LAUNCH(kernel, grid, block, lds, st, ...)                                                                  \
  do {                                                                                                                 \
    if (h->poison_lds) hipLaunchKernelGGL(k_poison_lds, dim3(h->poison_blocks), dim3(256), POISON_LDS_BYTES, (st));    \
    hipLaunchKernelGGL(kernel, (grid), (block), (lds), (st), __VA_ARGS__);                                             \
  } while (0)

// ---- LQ approximation: one workgroup per (instance, node)
template <bool DERIV>
__global__ __launch_bounds__(DERIV ? LQ_THREADS : LQV_THREADS, DERIV ? LQ_WPE : LQV_WPE) void k_lq(const DevModel* __restrict__ dm, const double* __restrict__ x,
                                                   const double* __restrict__ u, const double* __restrict__ par, const double* __restrict__ dts, int N,
                                                   double* __restrict__ rec, double* __restrict__ misc, long long* prof,
                                                   const LsState* __restrict__ ls) {
  const int node = blockIdx.x, b = node / N, k = node % N;
  if (ls && !ls[b].active) return;   // line search: only the instances whose trial is pending are re-evaluated
  LqWST<DERIV>& w = *reinterpret_cast<LqWST<DERIV>*>(hsqp_smem);
  const Ctx ctx{(int)threadIdx.x, (int)blockDim.x, blockIdx.x == 0 ? prof : nullptr};   // (the constant crashes this compiler's register allocator on k_lq<false>)
  PH_TICK(ctx, 126);  // re-arm the phase clock (bucket 126 is a sink)
  const double* xk = x + ((size_t)b * (N + 1) + k) * NX;
  lq_node<DERIV>(ctx, *dm, w, xk, u + ((size_t)b * N + k) * NU, xk + NX, par + ((size_t)b * (N + 1) + k) * NP, dts[node],
                 DERIV ? rec + (size_t)node * REC_SIZE : nullptr,
                 DERIV ? rec + (size_t)node * REC_SIZE + REC_MISC : misc + (size_t)node * 8);
}

// ---- centroidal LQ approximation, second form (hsqp_cent_lq.h): one 128-thread workgroup per (instance, node), values once per node in an LDS
//      workspace, tangent lanes on closed-form seeds; four workgroups per CU
static_assert(sizeof(CentWST<true>) <= 163840 / 4, "centroidal LQ workspace: four workgroups per CU");
__global__ __launch_bounds__(CLQ_THREADS, 2) void k_lq_cent2(const DevModel* __restrict__ dm, const double* __restrict__ x, const double* __restrict__ u,
                                                             const double* __restrict__ par, const double* __restrict__ dts, int N, double* __restrict__ rec) {
  const int node = blockIdx.x, b = node / N, k = node % N;
  CentWST<true>& w = *reinterpret_cast<CentWST<true>*>(hsqp_smem);
  const Ctx ctx{(int)threadIdx.x, (int)blockDim.x, nullptr};   // (this kernel is faster with the run-time value: 0.121 against 0.165 ms at N = 100 — the constant changes its unrolling and with it the spills)
  const double* xk = x + ((size_t)b * (N + 1) + k) * NX;
  double* r = rec + (size_t)node * REC_SIZE;
  cent_lq_node2<true>(ctx, *dm, w, xk, u + ((size_t)b * N + k) * NU, xk + NX, par + ((size_t)b * (N + 1) + k) * NP, dts[node], r, r + REC_MISC);
}
// ---- centroidal value-only pass (performance index, line-search trials): the same node function without derivative storage, one wave per
//      (instance, node), 13 KB of LDS
static_assert(sizeof(CentWST<false>) <= 163840 / 8, "centroidal value-only workspace: eight workgroups per CU");
__global__ __launch_bounds__(64) void k_lq_cent2_value(const DevModel* __restrict__ dm, const double* __restrict__ x, const double* __restrict__ u,
                                                       const double* __restrict__ par, const double* __restrict__ dts, int N, double* __restrict__ misc,
                                                       const LsState* __restrict__ ls) {
  const int node = blockIdx.x, b = node / N, k = node % N;
  if (ls && !ls[b].active) return;
  CentWST<false>& w = *reinterpret_cast<CentWST<false>*>(hsqp_smem);
  const Ctx ctx{(int)threadIdx.x, 64, nullptr};
  const double* xk = x + ((size_t)b * (N + 1) + k) * NX;
  cent_lq_node2<false>(ctx, *dm, w, xk, u + ((size_t)b * N + k) * NU, xk + NX, par + ((size_t)b * (N + 1) + k) * NP, dts[node], nullptr, misc + (size_t)node * 8);
}
// ---- torso task-space reference of the node parameters of a centroidal handle (behind k_params): one wave per (instance, node)
__global__ __launch_bounds__(64) void k_params_cent_torso(const DevModel* __restrict__ dm, double* __restrict__ par) {
  CentWST<false>& w = *reinterpret_cast<CentWST<false>*>(hsqp_smem);
  const Ctx ctx{(int)threadIdx.x, 64, nullptr};
  cent_params_torso(ctx, *dm, w, par + (size_t)blockIdx.x * NP);
}

// ---- projection: one workgroup per (instance, node); n0: the first node of the launch's node range (hsqp_iterate_device)
__global__ __launch_bounds__(PROJ_THREADS, PROJ_WPE) void k_project(const double* __restrict__ rec, const double* __restrict__ dts, double* __restrict__ qp, long long* prof, int cent, int joint_rows, int chain, int n0) {
  ProjWS& w = *reinterpret_cast<ProjWS*>(hsqp_smem);
  const int node = n0 + blockIdx.x;
  const Ctx ctx{(int)threadIdx.x, PROJ_THREADS, node == 0 ? prof : nullptr};
  PH_TICK(ctx, 126);  // re-arm the phase clock (bucket 126 is a sink)
  project_node(ctx, w, rec + (size_t)node * REC_SIZE, dts[node], qp + (size_t)node * QP_SIZE, cent != 0, joint_rows != 0, chain != 0);
}

// ---- event intervals (jump_node_qp, hsqp_project.h): one workgroup per node; only launched when the grid has such intervals
__global__ __launch_bounds__(256) void k_jump(const double* __restrict__ dts, const double* __restrict__ rec, double* __restrict__ qp, int n0) {
  const int node = n0 + blockIdx.x;
  if (dts[node] != 0.0) return;
  const Ctx ctx{(int)threadIdx.x, 256, nullptr};
  jump_node_qp(ctx, rec + (size_t)node * REC_SIZE, qp + (size_t)node * QP_SIZE);
}

// ---- Riccati backward sweep + closed-loop forward sweep (dx): one workgroup per instance
template <int NXE>
__global__ __launch_bounds__(RIC_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_riccati(const DevModel* __restrict__ dm, const double* __restrict__ x_init,
                                                         const double* __restrict__ x, const double* __restrict__ par,
                                                         const double* __restrict__ qp, double* __restrict__ ric, int N,
                                                         double* __restrict__ dx, int* __restrict__ status, long long* prof,
                                                         double* __restrict__ vf, double* __restrict__ ut) {
  const int b = blockIdx.x;
  RicWS& w = *reinterpret_cast<RicWS*>(hsqp_smem);
  const Ctx ctx{(int)threadIdx.x, RIC_THREADS, blockIdx.x == 0 ? prof : nullptr};
  PH_TICK(ctx, 126);  // re-arm the phase clock (bucket 126 is a sink)
  const double* xb = x + (size_t)b * (N + 1) * NX;
  const double* parN = par + ((size_t)b * (N + 1) + N) * NP;
  const double* qpb = qp + (size_t)b * N * QP_SIZE;
  double* ricb = ric + (size_t)b * N * RIC_SIZE;
  int mybad = 0;  // projection failures of this instance (rank-deficient D)
  for (int k = threadIdx.x; k < N; k += blockDim.x)
    if (qpb[(size_t)k * QP_SIZE + QP_NUT] < 0.0) mybad = 1;
  const int bad = __syncthreads_or(mybad);
  riccati_backward<NXE>(ctx, w, dm->Qf, xb + (size_t)N * NX, parN, qpb, ricb, N, vf ? vf + (size_t)b * (N + 1) * VF_SIZE : nullptr);
  PH_TICK(ctx, 0);
  riccati_forward<NXE>(ctx, w, x_init + (size_t)b * NX, xb, qpb, ricb, N, dx + (size_t)b * (N + 1) * NX, ut + (size_t)b * N * NUT);
  PH_TICK(ctx, 10);
  // OR-accumulated over the iterations of one hsqp_iterate_device call (the host clears it once per call): a numeric failure
  // in an early iteration must not be masked by a later clean one
  if (threadIdx.x == 0) { const int st = (bad ? 1 : 0) | (w.ok ? 0 : 2); if (st) atomicOr(&status[b], st); }
}

// ---- the whole-body serial sweep on the FACTORS of [A~ | B~] (hsqp_riccati_fact.h): what every whole-body handle's serial recursion runs
__global__ __launch_bounds__(RIC_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_riccati_fact(const DevModel* __restrict__ dm, const double* __restrict__ x_init,
                                                         const double* __restrict__ x, const double* __restrict__ par,
                                                         const double* __restrict__ qp, const double* __restrict__ dts, double* __restrict__ ric, int N,
                                                         double* __restrict__ dx, int* __restrict__ status, long long* prof,
                                                         double* __restrict__ vf, double* __restrict__ ut, double* __restrict__ fj) {
  const int b = blockIdx.x;
  RicFWS& w = *reinterpret_cast<RicFWS*>(hsqp_smem);
  const Ctx ctx{(int)threadIdx.x, RIC_THREADS, blockIdx.x == 0 ? prof : nullptr};
  PH_TICK(ctx, 126);  // re-arm the phase clock (bucket 126 is a sink)
  const double* xb = x + (size_t)b * (N + 1) * NX;
  const double* parN = par + ((size_t)b * (N + 1) + N) * NP;
  const double* qpb = qp + (size_t)b * N * QP_SIZE;
  const double* dtb = dts + (size_t)b * N;
  double* ricb = ric + (size_t)b * N * RIC_SIZE;
  int mybad = 0;  // projection failures of this instance (rank-deficient D)
  for (int k = threadIdx.x; k < N; k += RIC_THREADS)
    if (qpb[(size_t)k * QP_SIZE + QP_NUT] < 0.0) mybad = 1;
  const int bad = __syncthreads_or(mybad);
  riccati_backward_fact(ctx, w, dm->Qf, xb + (size_t)N * NX, parN, qpb, dtb, ricb, N, vf ? vf + (size_t)b * (N + 1) * VF_SIZE : nullptr);
  PH_TICK(ctx, 0);
  riccati_forward_fact(ctx, w, x_init + (size_t)b * NX, xb, qpb, dtb, ricb, N, dx + (size_t)b * (N + 1) * NX, ut + (size_t)b * N * NUT, fj + (size_t)b * N * NJ);
  PH_TICK(ctx, 10);
  if (threadIdx.x == 0) { const int st = (bad ? 1 : 0) | (w.ok ? 0 : 2); if (st) atomicOr(&status[b], st); }
}

// ---- parallel-in-time backward sweep (hsqp_scan.h).  Elements: [B][N + 1][ScanEl<n>::SIZE], two buffers (ping-pong per level).
constexpr int SCAN_INIT_THREADS = 256, SCAN_COMB_THREADS = 512, SCAN_FWD_THREADS = 256;
static_assert(4 * NX <= SCAN_FWD_THREADS, "closed_loop_forward: one item per thread");
template <int n>
__global__ __launch_bounds__(SCAN_INIT_THREADS) void k_scan_init(const DevModel* __restrict__ dm, const double* __restrict__ x, const double* __restrict__ par,
                                                                 const double* __restrict__ qp, int N, double* __restrict__ el, int* __restrict__ status) {
  ScanInitWS<n>& w = *reinterpret_cast<ScanInitWS<n>*>(hsqp_smem);
  const int id = blockIdx.x, b = id / (N + 1), k = id % (N + 1);
  const Ctx ctx{(int)threadIdx.x, SCAN_INIT_THREADS, nullptr};
  __shared__ int ok;
  if (threadIdx.x == 0) ok = 1;
  __syncthreads();
  scan_init_node<n>(ctx, w, qp + ((size_t)b * N + (k < N ? k : 0)) * QP_SIZE, el + (size_t)id * ScanEl<n>::SIZE, k == N, dm->Qf,
                    x + ((size_t)b * (N + 1) + N) * NX, par + ((size_t)b * (N + 1) + N) * NP, &ok);
  __syncthreads();
  if (threadIdx.x == 0 && !ok) atomicOr(&status[b], 2);   // R~ of a stage not positive definite (the gate sees the flag)
}
template <int n>
__global__ __launch_bounds__(SCAN_COMB_THREADS) void k_scan_combine(const double* __restrict__ ein, double* __restrict__ eout, int N, int d, int* __restrict__ status,
                                                                    long long* prof) {
  ScanCombWS<n>& w = *reinterpret_cast<ScanCombWS<n>*>(hsqp_smem);
  const int id = blockIdx.x, b = id / (N + 1), k = id % (N + 1);
  const Ctx ctx{(int)threadIdx.x, SCAN_COMB_THREADS, blockIdx.x == 0 ? prof : nullptr};
  constexpr int SZ = ScanEl<n>::SIZE;
  if (k + d <= N) {
    __shared__ int ok;
    if (threadIdx.x == 0) ok = 1;
    __syncthreads();
    scan_combine<n>(ctx, w, ein + (size_t)id * SZ, ein + (size_t)(id + d) * SZ, eout + (size_t)id * SZ, &ok);
    __syncthreads();
    if (threadIdx.x == 0 && !ok) atomicOr(&status[b], 2);
  } else {
    for (int i = threadIdx.x; i < SZ; i += blockDim.x) eout[(size_t)id * SZ + i] = ein[(size_t)id * SZ + i];
  }
}
// one stage of the Riccati code per node, started from the value function of node k + 1: the scanned one (element el; vf_in = null)
// or, in the refinement pass, the one the first pass computed (vf_in: [N + 1][VF_SIZE] per instance).  Applying the exact Riccati map
// once more contracts the scan's rounding error (oracle-level experiment: 5e-8 -> 5e-9 on the worst whole-body case).
template <int n>
__global__ __launch_bounds__(RIC_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_scan_gains(const DevModel* __restrict__ dm, const double* __restrict__ x, const double* __restrict__ par,
                                                            const double* __restrict__ qp, const double* __restrict__ el, const double* __restrict__ vf_in,
                                                            double* __restrict__ ric, int N, int* __restrict__ status, double* __restrict__ vf, double* __restrict__ acl) {
  RicWS& w = *reinterpret_cast<RicWS*>(hsqp_smem);
  const int node = blockIdx.x, b = node / N, k = node % N;
  const Ctx ctx{(int)threadIdx.x, RIC_THREADS, nullptr};
  const double* en = el + ((size_t)b * (N + 1) + k + 1) * ScanEl<n>::SIZE;
  const double* vn = vf_in ? vf_in + ((size_t)b * (N + 1) + k + 1) * VF_SIZE : nullptr;
  const double* q = qp + (size_t)node * QP_SIZE;
  riccati_backward<n>(ctx, w, dm->Qf, x + ((size_t)b * (N + 1) + N) * NX, par + ((size_t)b * (N + 1) + N) * NP, q, ric + (size_t)node * RIC_SIZE, 1,
                      vf ? vf + ((size_t)b * (N + 1) + k) * VF_SIZE : nullptr, vn ? vn : en + ScanEl<n>::J, vn ? vn + NX * NX : en + ScanEl<n>::ETA, k == N - 1,
                      vn ? 1.0 : -1.0, vn ? NX : n);
  if (threadIdx.x == 0) {
    const int st = (q[QP_NUT] < 0.0 ? 1 : 0) | (w.ok ? 0 : 2);
    if (st) atomicOr(&status[b], st);
  }
  if (acl) closed_loop_record<n>(ctx, w, acl + (size_t)node * ACL_SIZE<n>);   // the last pass: closed loop of this stage for the roll-out
}
template <int n>
__global__ __launch_bounds__(SCAN_FWD_THREADS) void k_scan_forward(const double* __restrict__ x_init, const double* __restrict__ x, const double* __restrict__ acl,
                                                              int N, double* __restrict__ dx) {
  RicWS& w = *reinterpret_cast<RicWS*>(hsqp_smem);
  const int b = blockIdx.x;
  const Ctx ctx{(int)threadIdx.x, SCAN_FWD_THREADS, nullptr};
  closed_loop_forward<n>(ctx, w, x_init + (size_t)b * NX, x + (size_t)b * (N + 1) * NX, acl + (size_t)b * N * ACL_SIZE<n>, N, dx + (size_t)b * (N + 1) * NX);
}

// ---- two-level (segmented) backward sweep (hsqp_segment.h): B P workgroups, segment p of instance b covers the stages [p N / P, (p + 1) N / P)
constexpr int SEG_ACC_THREADS = 512;
// 1a: Riccati recursion over the segment from J = 0, eta = 0 (zero: n x n + n zeros): gains and (L^-1)^T of every stage, (J, s) at its first node
template <int n>
__global__ __launch_bounds__(RIC_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_seg_elem_ric(const DevModel* __restrict__ dm, const double* __restrict__ x, const double* __restrict__ par,
                                                              const double* __restrict__ qp, const double* __restrict__ zero, double* __restrict__ ric_tmp,
                                                              double* __restrict__ linv, double* __restrict__ vf0, int N, int P, int* __restrict__ status) {
  RicWS& w = *reinterpret_cast<RicWS*>(hsqp_smem);
  const int seg = blockIdx.x, b = seg / P, p = seg % P, k0 = seg_bound(p, N, P), L = seg_bound(p + 1, N, P) - k0;
  const Ctx ctx{(int)threadIdx.x, RIC_THREADS, nullptr};
  const size_t s0 = (size_t)b * N + k0;
  riccati_backward<n>(ctx, w, dm->Qf, x + ((size_t)b * (N + 1) + N) * NX, par + ((size_t)b * (N + 1) + N) * NP, qp + s0 * QP_SIZE, ric_tmp + s0 * RIC_SIZE, L,
                      vf0 + (size_t)seg * VF_SIZE, zero, zero + n * n, false, 1.0, n, linv + s0 * LDB * LDB, 1);
  if (threadIdx.x == 0 && !w.ok) atomicOr(&status[b], 2);
}
// 1b: the (A, b, C) part of the segment's element by prepending its stages; el: [B][P + 1][ScanEl<n>::SIZE]
template <int n>
__global__ __launch_bounds__(SEG_ACC_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_seg_accumulate(const double* __restrict__ qp, const double* __restrict__ ric_tmp, const double* __restrict__ linv,
                                                                   const double* __restrict__ vf0, int N, int P, double* __restrict__ el) {
  SegAccWS& w = *reinterpret_cast<SegAccWS*>(hsqp_smem);
  const int seg = blockIdx.x, b = seg / P, p = seg % P, k0 = seg_bound(p, N, P), L = seg_bound(p + 1, N, P) - k0;
  const Ctx ctx{(int)threadIdx.x, SEG_ACC_THREADS, nullptr};
  const size_t s0 = (size_t)b * N + k0;
  seg_accumulate<n>(ctx, w, qp + s0 * QP_SIZE, ric_tmp + s0 * RIC_SIZE, linv + s0 * LDB * LDB, L, vf0 + (size_t)seg * VF_SIZE,
                    el + ((size_t)b * (P + 1) + p) * ScanEl<n>::SIZE);
}
// the terminal cost as element P of every instance
template <int n>
__global__ __launch_bounds__(256) void k_seg_terminal(const DevModel* __restrict__ dm, const double* __restrict__ x, const double* __restrict__ par, int N, int P,
                                                      double* __restrict__ el) {
  const int b = blockIdx.x;
  const Ctx ctx{(int)threadIdx.x, 256, nullptr};
  scan_terminal_element<n>(ctx, el + ((size_t)b * (P + 1) + P) * ScanEl<n>::SIZE, dm->Qf, x + ((size_t)b * (N + 1) + N) * NX, par + ((size_t)b * (N + 1) + N) * NP);
}
// 3: the gains of the segment's stages from the value function at its end (suffix element p + 1 of the scanned array)
template <int n>
__global__ __launch_bounds__(RIC_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_seg_riccati(const DevModel* __restrict__ dm, const double* __restrict__ x, const double* __restrict__ par,
                                                             const double* __restrict__ qp, const double* __restrict__ el, double* __restrict__ ric, int N, int P,
                                                             int* __restrict__ status, double* __restrict__ vf, int vf_mode) {
  RicWS& w = *reinterpret_cast<RicWS*>(hsqp_smem);
  const int seg = blockIdx.x, b = seg / P, p = seg % P, k0 = seg_bound(p, N, P), L = seg_bound(p + 1, N, P) - k0;
  const Ctx ctx{(int)threadIdx.x, RIC_THREADS, nullptr};
  const size_t s0 = (size_t)b * N + k0;
  const double* en = el + ((size_t)b * (P + 1) + p + 1) * ScanEl<n>::SIZE;
  int mybad = 0;
  for (int k = threadIdx.x; k < L; k += blockDim.x)
    if (qp[(s0 + k) * QP_SIZE + QP_NUT] < 0.0) mybad = 1;
  const int bad = __syncthreads_or(mybad);
  // vf: this segment writes the value functions of its nodes k0 .. k0 + L - 1 (vf_mode 0: all — the KKT report; 2: its first node and its last
  // stage's node — what the gate's boundary stages need); the last segment also the terminal node
  riccati_backward<n>(ctx, w, dm->Qf, x + ((size_t)b * (N + 1) + N) * NX, par + ((size_t)b * (N + 1) + N) * NP, qp + s0 * QP_SIZE, ric + s0 * RIC_SIZE, L,
                      vf ? vf + ((size_t)b * (N + 1) + k0) * VF_SIZE : nullptr, en + ScanEl<n>::J, en + ScanEl<n>::ETA, p == P - 1, -1.0, n, nullptr, vf_mode);
  if (threadIdx.x == 0) { const int st = (bad ? 1 : 0) | (w.ok ? 0 : 2); if (st) atomicOr(&status[b], st); }
}
// 4: the roll-out alone (k_riccati runs it behind its backward sweep)
template <int NXE>
__global__ __launch_bounds__(RIC_THREADS) void k_ric_forward(const double* __restrict__ x_init, const double* __restrict__ x, const double* __restrict__ qp,
                                                             const double* __restrict__ ric, int N, double* __restrict__ dx, double* __restrict__ ut) {
  RicWS& w = *reinterpret_cast<RicWS*>(hsqp_smem);
  const int b = blockIdx.x;
  const Ctx ctx{(int)threadIdx.x, RIC_THREADS, nullptr};
  riccati_forward<NXE>(ctx, w, x_init + (size_t)b * NX, x + (size_t)b * (N + 1) * NX, qp + (size_t)b * N * QP_SIZE, ric + (size_t)b * N * RIC_SIZE, N,
                       dx + (size_t)b * (N + 1) * NX, ut + (size_t)b * N * NUT);
}

// ---- input recovery + step: one 64-thread workgroup per (instance, node); the last node of an instance also steps x_N.
//      ut_given: ut holds ut = k + K dx of every node already (the serial roll-out writes it as it goes) and the gains are not read
__global__ __launch_bounds__(64) void k_step(const double* __restrict__ qp, const double* __restrict__ ric, const double* __restrict__ dx,
                                             const double* __restrict__ x, const double* __restrict__ u, int N, double alpha,
                                             double* ut, double* __restrict__ du, double* __restrict__ x_new,
                                             double* __restrict__ u_new, double* __restrict__ info, int ut_given, const double* __restrict__ fj) {
  __shared__ StepWS w;
  const int node = blockIdx.x, b = node / N, k = node % N;
  const Ctx ctx{(int)threadIdx.x, 64, nullptr};
  const size_t xo = ((size_t)b * (N + 1) + k) * NX, uo = (size_t)node * NU;
  step_node(ctx, w, qp + (size_t)node * QP_SIZE, ric + (size_t)node * RIC_SIZE, dx + xo, x + xo, u + uo, alpha, ut + (size_t)node * NUT,
            du + uo, x_new + xo, u_new + uo, info + (size_t)node * 4, ut_given ? ut + (size_t)node * NUT : nullptr, fj ? fj + (size_t)node * NJ : nullptr);
  if (k == N - 1)
    for (int i = threadIdx.x; i < NX; i += blockDim.x) x_new[xo + NX + i] = x[xo + NX + i] + alpha * dx[xo + NX + i];
}

// ---- input recovery + full-step trial + its value pass in ONE kernel (the first evaluation of every iteration): k_step alone is
//      HBM-bound (35 KB of gains / projection per node, 3.8 TB/s) while the value pass is issue-bound, so the reads of the one hide
//      under the arithmetic of the other.  One wave per node; the step's scratch aliases the stage workspace (dead until the value
//      pass starts), the stepped (x, u, x_next) go straight into the value pass's input slots — results are bit-identical to
//      k_step followed by k_lq<false>.
__global__ __launch_bounds__(LQV_THREADS, LQV_WPE) void k_step_value(const DevModel* __restrict__ dm, const double* __restrict__ qp, const double* __restrict__ ric,
                                                                          const double* __restrict__ dx, const double* __restrict__ x, const double* __restrict__ u,
                                                                          const double* __restrict__ par, const double* __restrict__ dts, int N, double alpha,
                                                                          double* ut, double* __restrict__ du, double* __restrict__ x_new,
                                                                          double* __restrict__ u_new, double* __restrict__ info, double* __restrict__ misc, long long* prof,
                                                                          int ut_given, const double* __restrict__ fj) {
  const int node = blockIdx.x, b = node / N, k = node % N;
  LqWST<false>& w = *reinterpret_cast<LqWST<false>*>(hsqp_smem);
  static_assert(sizeof(StepWS) <= sizeof(w.st), "the step scratch aliases the stage workspace");
  StepWS& sw = *reinterpret_cast<StepWS*>(&w.st);
  const Ctx ctx{(int)threadIdx.x, LQV_THREADS, blockIdx.x == 0 ? prof : nullptr};   // phase profile (profile builds): slot 3, labelled k_lq<false>
  PH_TICK(ctx, 126);
  const size_t xo = ((size_t)b * (N + 1) + k) * NX, uo = (size_t)node * NU;
  step_node(ctx, sw, qp + (size_t)node * QP_SIZE, ric + (size_t)node * RIC_SIZE, dx + xo, x + xo, u + uo, alpha, ut + (size_t)node * NUT,
            du + uo, x_new + xo, u_new + uo, info + (size_t)node * 4, ut_given ? ut + (size_t)node * NUT : nullptr, fj ? fj + (size_t)node * NJ : nullptr);
  WG_SYNC(ctx);
  WG_FOR(ctx, i, NX + NU + NX) {
    if (i < NX) w.nw.x[i] = x[xo + i] + alpha * sw.dx[i];
    else if (i < NX + NU) w.nw.u[i - NX] = u[uo + i - NX] + alpha * sw.du[i - NX];
    else {
      const int j = i - NX - NU;
      const double v = x[xo + NX + j] + alpha * dx[xo + NX + j];
      w.xnext[j] = v;
      if (k == N - 1) x_new[xo + NX + j] = v;   // the last node of an instance also steps x_N
    }
  }
  WG_SYNC(ctx);
  lq_node<false, true>(ctx, *dm, w, nullptr, nullptr, nullptr, par + ((size_t)b * (N + 1) + k) * NP, dts[node], nullptr, misc + (size_t)node * 8);
}

// (x, u) of the 16 nodes of a wave -> LDS: lane i < 64 takes entries i and i + 64 of every node's [x; u] row, 32 loads per lane issued back to back;
// the node arithmetic is the wave's (scalar: node0 through readfirstlane, no division per element).  The first form — one entry per lane and
// iteration with its indices by division — kept one load in flight per iteration and spent ~150 instructions per element on the indices.
__device__ __forceinline__ void quad_load_xu(double (*xs)[NX], double (*us)[NU], const double* __restrict__ x, const double* __restrict__ u, int node0_, int nodes,
                                             int N, int lane) {
  static_assert(QV_NODES == 16 && NZ <= 128 && NX <= 64, "two entries per lane and node");
  const int node0 = __builtin_amdgcn_readfirstlane(node0_);
  int b = node0 / N, k = node0 - b * N;
  double t0[QV_NODES], t1[QV_NODES];
#pragma unroll
  for (int n2 = 0; n2 < QV_NODES; ++n2) {
    const bool pad = node0 + n2 >= nodes;                          // a padding quad repeats the last node
    const int nd = pad ? nodes - 1 : node0 + n2;
    const size_t xrow = pad ? (size_t)(nodes - 1) + (nodes - 1) / N : (size_t)b * (N + 1) + k;
    t0[n2] = lane < NX ? x[xrow * NX + lane] : u[(size_t)nd * NU + (lane - NX)];
    t1[n2] = u[(size_t)nd * NU + (lane + 64 - NX < NU ? lane + 64 - NX : NU - 1)];
    if (++k == N) { k = 0; ++b; }
  }
#pragma unroll
  for (int n2 = 0; n2 < QV_NODES; ++n2) {
    if (lane < NX) xs[n2][lane] = t0[n2]; else us[n2][lane - NX] = t0[n2];
    if (lane + 64 < NZ) us[n2][lane + 64 - NX] = t1[n2];
  }
}

// ---- whole-body value pass on quads of lanes (hsqp_lqv.h): a wave evaluates QV_NODES nodes, one lane per limb; misc as k_lq<false> writes it.
//      Nodes of instances whose line search is over (ls) are evaluated with the rest of their wave but not written.
__global__ __launch_bounds__(QV_THREADS * QV_WAVES) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_value_quad(const DevModel* __restrict__ dm, const double* __restrict__ x,
                                                          const double* __restrict__ u, const double* __restrict__ par, const double* __restrict__ dts, int N, int nodes,
                                                          double* __restrict__ misc, const LsState* __restrict__ ls) {
  __shared__ QvWS ws;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nn = lane >> 2, L = lane & 3;
  auto& w = ws.wv[wave];
  const int node0 = (blockIdx.x * QV_WAVES + wave) * QV_NODES, node = node0 + nn < nodes ? node0 + nn : nodes - 1;   // (a padding quad repeats the last node)
  const int b = node / N, k = node % N;
  const bool live = node0 + nn < nodes && (!ls || ls[b].active);
  if (__syncthreads_or(live) == 0) return;
  const Ctx ctx{(int)threadIdx.x, QV_THREADS * QV_WAVES, nullptr};
  qv_load_const(ctx, *dm, ws.k, [] {});
  quad_load_xu(w.x, w.u, x, u, node0, nodes, N, lane);
  __syncthreads();
  const double* xs = w.x[nn];
  const double* us = w.u[nn];
  const double* pn = par + ((size_t)b * (N + 1) + k) * NP;
  const double dt = dts[node];
#if defined(__HIP_DEVICE_COMPILE__)
  auto quad_sum = [](double v) { v += quad_perm_f64<0xB1>(v); v += quad_perm_f64<0x4E>(v); return v; };   // the sum over the node's four lanes, in all of them
#else
  auto quad_sum = [](double v) { return v; };
#endif
  QvCarry c;
  qv_carry_init(c);
  double cost = 0.0, eq = 0.0;
  auto stage = [&](int s) {
    double part[16];
    qv_limb_stage(*dm, ws.k, xs, us, L, s, dt, c, part, w.cp[nn]);
#pragma unroll
    for (int e = 0; e < 16; ++e) part[e] = quad_sum(part[e]);
    qv_base_solve(part, xs, s, dt, c);
  };
  // the first stage apart from the loop: what it captures for the node terms (the foot frame, 33 doubles per lane) is dead before the second
  stage(0);
  __syncthreads();   // orders the collision points of a node's four lanes before their readers
  qv_node_terms(*dm, xs, us, pn, L, c, w.cp[nn], cost, eq);
#pragma unroll 1
  for (int s = 1; s < 4; ++s) stage(s);
  double dyn = qv_defect(xs, us, x + ((size_t)b * (N + 1) + k + 1) * NX, L, dt, c);
  cost = quad_sum(cost); eq = quad_sum(eq); dyn = quad_sum(dyn);
  if (live && L == 0) qv_write_misc(pn, dt, cost, eq, dyn, misc + (size_t)node * 8);
}

// ---- whole-body LQ approximation on limb lanes (hsqp_lql.h), kernel 1 of 3: the rigid-body model and its Jacobian at the four RK4 stages.  A wave
//      evaluates QL_NODES nodes, one lane per limb; writes REC_GS (transposed) and REC_AS of the node's record.
constexpr int LQ_SPLIT_DEFAULT = 2;   // node ranges of the limb-lane LQ kernels and of k_project behind them, on streams of their own (hsqp_iterate_device)
constexpr int QL_WAVES = 2;           // waves per workgroup: they share the body constants
constexpr int QL_WPE = 1, QR_WPE = 1;   // waves per SIMD the register budget of k_lq_limb / k_lq_rows is cut for (1: 512 registers per lane)
struct QlWS {
  QvConst k;
  struct {
    double x[QL_NODES][NX], u[QL_NODES][NU];
    double csn[QL_MAXLEN][QL_THREADS][2];   // cos / sin of the joints a lane passed on its way to the leaf, for the way back
  } wv[QL_WAVES];
};
#if defined(__HIP_DEVICE_COMPILE__)
#define QL_QUAD_OPS                                                                                                                                    \
  auto quad_sum = [](double v) { v += quad_perm_f64<0xB1>(v); v += quad_perm_f64<0x4E>(v); return v; }; /* the sum over the node's four lanes, in all of them */ \
  auto quad_x1 = [](double v) { return quad_perm_f64<0xB1>(v); }; /* the value of lane L ^ 1 / L ^ 2 / L ^ 3 of the quad */                       \
  auto quad_x2 = [](double v) { return quad_perm_f64<0x4E>(v); };                                                                                 \
  auto quad_x3 = [](double v) { return quad_perm_f64<0x1B>(v); };                                                                                 \
  (void)quad_x1; (void)quad_x2; (void)quad_x3
#else
#define QL_QUAD_OPS                             \
  auto quad_sum = [](double v) { return v; };  \
  auto quad_x1 = quad_sum, quad_x2 = quad_sum, quad_x3 = quad_sum; (void)quad_x1; (void)quad_x2; (void)quad_x3
#endif
__global__ __launch_bounds__(QL_THREADS * QL_WAVES) __attribute__((amdgpu_waves_per_eu(QL_WPE, QL_WPE))) void k_lq_limb(
    const DevModel* __restrict__ dm, const double* __restrict__ x, const double* __restrict__ u, const double* __restrict__ dts, int N, int nodes,
    double* __restrict__ rec, long long* prof, int node_base) {   // the launch covers the nodes [node_base, nodes)
  __shared__ QlWS ws;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nn = lane >> 2, L = lane & 3;
  auto& w = ws.wv[wave];
  const int node0 = node_base + (blockIdx.x * QL_WAVES + wave) * QL_NODES, node = node0 + nn < nodes ? node0 + nn : nodes - 1;   // (a padding quad repeats the last node)
  const bool live = node0 + nn < nodes;
  const Ctx ctx{(int)threadIdx.x, QL_THREADS * QL_WAVES, blockIdx.x == 0 ? prof : nullptr};
  PH_TICK(ctx, 126);
  qv_load_const(ctx, *dm, ws.k, [] {});
  quad_load_xu(w.x, w.u, x, u, node0, nodes, N, lane);
  __syncthreads();
  const double* xs = w.x[nn];
  const double* us = w.u[nn];
  const double dt = dts[node];
  double* grec = rec + (size_t)node * REC_SIZE;
  double* csn = &w.csn[0][lane][0];
  constexpr int CSN_LD = QL_THREADS * 2;
  QL_QUAD_OPS;
  const QlLimb lb = ql_limb(*dm, L);
  const int max_len = lb.max_len;
  const bool own_root = (dm->limb_own[L] & 1u) != 0;
  QlCarry c;
  for (int i = 0; i < 6; ++i) { c.vb[i] = 0.0; c.ap[i] = 0.0; }
#pragma unroll 1
  for (int s = 0; s < 4; ++s) {
    QlBaseKin bk;
    QlState st;
    QlShared sh;
    double rP[3], Ff[3];
    PH_TICK(ctx, 0);
    ql_base_kin(*dm, xs, s, dt, c, bk);
    {
      double part[16];
      ql_forward(*dm, ws.k, lb, xs, us, L, s, dt, bk, st, part, csn, CSN_LD, rP, Ff);
#pragma unroll
      for (int e = 0; e < 16; ++e) part[e] = quad_sum(part[e]);
      ql_base_solve(part, bk, sh);
    }
    PH_TICK(ctx, 1);
    if (live && L == 0)
      for (int i = 0; i < 6; ++i) grec[REC_AS + 6 * s + i] = sh.ab[i];
    double* gs = grec + REC_GS + (size_t)s * LDJ * GT_LD;
    auto putg = [&](int col, const double* g) {
      if (!live) return;
      ql_st2(gs + col * GT_LD, g[0], g[1]); ql_st2(gs + col * GT_LD + 2, g[2], g[3]); ql_st2(gs + col * GT_LD + 4, g[4], g[5]);
    };
    double cmp[NCMP];
#pragma unroll
    for (int e = 0; e < NCMP; ++e) cmp[e] = 0.0;
#pragma unroll 1
    for (int t = max_len - 1; t >= 0; --t) {
      // limbs that join below this step hand over their composites (the G1 tree: the two arm lanes, once, at the torso)
      const unsigned mg = dm->limb_merge[t][L];
      const unsigned anym = (unsigned)dm->limb_merge[t][0] | dm->limb_merge[t][1] | dm->limb_merge[t][2] | dm->limb_merge[t][3];
      if (anym & 2u) {
        const double m = (mg & 2u) ? 1.0 : 0.0;
#pragma unroll
        for (int e = 0; e < NCMP; ++e) cmp[e] += m * quad_x1(cmp[e]);
      }
      if (anym & 4u) {
        const double m = (mg & 4u) ? 1.0 : 0.0;
#pragma unroll
        for (int e = 0; e < NCMP; ++e) cmp[e] += m * quad_x2(cmp[e]);
      }
      if (anym & 8u) {
        const double m = (mg & 8u) ? 1.0 : 0.0;
#pragma unroll
        for (int e = 0; e < NCMP; ++e) cmp[e] += m * quad_x3(cmp[e]);
      }
      ql_back_step(*dm, ws.k, lb, xs, us, L, s, dt, t, st, cmp, sh, csn, CSN_LD, rP, Ff, putg);
    }
    PH_TICK(ctx, 3);
    // ---- the base: composite of the whole robot = the limbs that own their root-side body + the base body; its columns
    {
      const double r0[3] = {0.0, 0.0, 0.0};
      double In[10], own[NCMP];
      ql_inertia(ws.k, 0, bk.R, r0, In);
      ql_body_comp(In, bk.vl[2], bk.al[2], own);
      const double mk = own_root ? 1.0 : 0.0;
#pragma unroll
      for (int e = 0; e < NCMP; ++e) cmp[e] = quad_sum(mk * cmp[e]) + own[e];
    }
    double dext_e[9];
#pragma unroll
    for (int jc = 0; jc < 3; ++jc) {
      double dr[3], tt[3];
      v3_cross(bk.w[jc], rP, dr);
      v3_cross(dr, Ff, tt);   // (a lane without a foot carries rP = Ff = 0)
      for (int i = 0; i < 3; ++i) dext_e[3 * jc + i] = quad_sum(tt[i]);
    }
    ql_base_columns(*dm, L, bk, cmp, sh, dext_e, rP, putg);
    ql_carry_advance(xs, s, dt, sh, c);
    PH_TICK(ctx, 4);
  }
}

// ---- ... kernel 2 of 3: the node terms of RK4 stage 1 — values, penalties, and the residual / equality rows of every column, formed by the lane
//      that owns the column from the stage-1 Jacobian columns kernel 1 left in the record (a kinematics-only walk of the limb).  Writes REC_J,
//      REC_CDE (transposed), REC_RHO, REC_D, REC_GD, REC_FLOW, REC_MISC.
struct QrWS {
  QvConst k;
  struct {
    double x[QL_NODES][NX], u[QL_NODES][NU];
    double csn[QL_MAXLEN][QL_THREADS][2];
    QlNodeLds nl[QL_NODES];                 // what the four lanes of a node share (foot frames, collision points, row scalings)
  } wv[QL_WAVES];
};
static_assert(sizeof(QrWS) * (4 / QL_WAVES) <= 163840, "four waves per CU");
__global__ __launch_bounds__(QL_THREADS * QL_WAVES) __attribute__((amdgpu_waves_per_eu(QR_WPE, QR_WPE))) void k_lq_rows(
    const DevModel* __restrict__ dm, const double* __restrict__ x, const double* __restrict__ u, const double* __restrict__ par, const double* __restrict__ dts,
    int N, int nodes, double* __restrict__ rec, long long* prof, int node_base, int defect) {
  __shared__ QrWS ws;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nn = lane >> 2, L = lane & 3;
  auto& w = ws.wv[wave];
  const int node0 = node_base + (blockIdx.x * QL_WAVES + wave) * QL_NODES, node = node0 + nn < nodes ? node0 + nn : nodes - 1;
  const int b = node / N, k = node % N;
  const bool live = node0 + nn < nodes;
  const Ctx ctx{(int)threadIdx.x, QL_THREADS * QL_WAVES, blockIdx.x == 0 ? prof : nullptr};   // phase profile (profile builds): slot 3, ids 10..15
  PH_TICK(ctx, 126);
  qv_load_const(ctx, *dm, ws.k, [] {});
  quad_load_xu(w.x, w.u, x, u, node0, nodes, N, lane);
  __syncthreads();
  PH_TICK(ctx, 10);
  const double* xs = w.x[nn];
  const double* us = w.u[nn];
  const double* pn = par + ((size_t)b * (N + 1) + k) * NP;
  QlNodeLds& nl = w.nl[nn];
  const double dt = dts[node];
  double* grec = rec + (size_t)node * REC_SIZE;
  double* csn = &w.csn[0][lane][0];
  constexpr int CSN_LD = QL_THREADS * 2;
  QL_QUAD_OPS;
  const QlLimb lb = ql_limb(*dm, L);
  const int max_len = lb.max_len;
  QlCarry c;
  for (int i = 0; i < 6; ++i) { c.vb[i] = 0.0; c.ap[i] = 0.0; }
  QlBaseKin bk;
  QlState st;
  QlShared sh;
  QlRows rw;
  ql_base_kin(*dm, xs, 0, dt, c, bk);
  ql_kin_to_leaf(*dm, ws.k, lb, xs, us, L, bk, csn, CSN_LD, st, nl);
  ql_shared_from_record(bk, grec, sh);
  double dsq = 0.0;   // defect = 1 (the chain is fused into k_project, k_lq_chain is not launched): the node's defect and its squared norm on the four lanes, in front of every store of the kernel
  if (defect) dsq = ql_defect_lane(xs, us, x + ((size_t)b * (N + 1) + k + 1) * NX, grec + REC_AS, dt, L, grec, live);
  PH_TICK(ctx, 11);
  {
    // the lane's foot and its share of the cost (pass A), then what needs every lane's pass A (pass B).  The four lanes of a node sit in one
    // wave: a wave-level fence orders their LDS traffic
    double cost, eq, cost2;
    int any;
    WV_SYNC();
    ql_terms_a(*dm, xs, us, pn, L, dt, sh, nl, grec, live, cost, eq);
    WV_SYNC();
    ql_terms_b(*dm, xs, us, pn, L, dt, sh, nl, grec, live, cost2, any);
    WV_SYNC();
    cost = quad_sum(cost + cost2); eq = quad_sum(eq);
    const int coll = quad_sum((double)any) > 0.0 ? 1 : 0;
    ql_rows_setup(*dm, pn, L, dt, coll, rw);
    if (live && L == 0) ql_write_misc(pn, dt, cost, eq, coll, grec + REC_MISC);
    if (defect) { dsq = quad_sum(dsq); if (live && L == 0) grec[REC_MISC + 3] = (dt > 0.0 ? dt : 1.0) * dsq; }
  }
  PH_TICK(ctx, 12);
  const double* gs = grec + REC_GS;
  double gcur[3][6];   // the three stage-Jacobian columns of the step about to run (ql_rows_back_step keeps them one step ahead)
#pragma unroll
  for (int q = 0; q < 3; ++q) ql_rows_fetch(gs, ql_rows_column(lb, max_len - 1, q), gcur[q]);
#pragma unroll 1
  for (int t = max_len - 1; t >= 0; --t) ql_rows_back_step(*dm, ws.k, lb, rw, nl, xs, us, t, st, csn, CSN_LD, bk.w, gs, gcur, grec, live);
  PH_TICK(ctx, 13);
  ql_rows_base(*dm, rw, nl, us, L, bk, sh, gs, grec, live);
  PH_TICK(ctx, 14);
}

// ---- ... kernel 3 of 3: the RK4 chain and the defect: one workgroup per (instance, node), a lane per column of [A|B] (lq_chain_node, hsqp_lql.h)
constexpr int LQC_THREADS = 128, LQC_WPE = 3;   // (the 64 defect items must be one wave: lq_chain_node sums their squares with a butterfly)
__global__ __launch_bounds__(LQC_THREADS, LQC_WPE) void k_lq_chain(const double* __restrict__ x, const double* __restrict__ u, const double* __restrict__ dts, int N,
                                                         double* __restrict__ rec, int node_base, int columns) {
  __shared__ LqChainWS w;
  const int node = node_base + blockIdx.x, b = node / N, k = node % N;
  const Ctx ctx{(int)threadIdx.x, LQC_THREADS, nullptr};
  const double* xk = x + ((size_t)b * (N + 1) + k) * NX;
  lq_chain_node(ctx, w, xk, u + (size_t)node * NU, xk + NX, dts[node], rec + (size_t)node * REC_SIZE, columns != 0);
}

// ---- line search: per-instance reduction of the step info (+ terminal node), state initialisation
__device__ inline void ls_init_instance(int b, const DevModel* __restrict__ dm, const double* __restrict__ info, const double* __restrict__ x,
                                        const double* __restrict__ dx, const double* __restrict__ par, int N, LsState* __restrict__ ls) {
  __shared__ double red[3][64];
  double a = 0.0, nx2 = 0.0, nu2 = 0.0;
  for (int k = threadIdx.x; k < N; k += blockDim.x) {
    const double* m = info + ((size_t)b * N + k) * 4;
    a += m[0]; nx2 += m[1]; nu2 += m[2];
  }
  if (threadIdx.x < NX) {   // terminal node: gradient of the terminal cost times dx_N
    const size_t o = ((size_t)b * (N + 1) + N) * NX + threadIdx.x;
    const double d = dx[o];
    a += dm->Qf[threadIdx.x] * (x[o] - par[((size_t)b * (N + 1) + N) * NP + HSQP_P_XDES + threadIdx.x]) * d;
    nx2 += d * d;
  }
  red[0][threadIdx.x] = a; red[1][threadIdx.x] = nx2; red[2][threadIdx.x] = nu2;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < 64; ++i) { s0 += red[0][i]; s1 += red[1][i]; s2 += red[2][i]; }
    LsState st;
    st.alpha = 1.0; st.armijo = s0; st.dxnorm = sqrt(s1); st.dunorm = sqrt(s2);
    st.active = 1; st.dirty = 0; st.step_type = HSQP_STEP_FULL; st.trials = 0;
    ls[b] = st;
  }
}
__global__ __launch_bounds__(64) void k_ls_init(const DevModel* __restrict__ dm, const double* __restrict__ info, const double* __restrict__ x,
                                                const double* __restrict__ dx, const double* __restrict__ par, int N, LsState* __restrict__ ls) {
  ls_init_instance(blockIdx.x, dm, info, x, dx, par, N, ls);
}

// ---- line search: decide the pending trials; counts[0] = instances that need a new trajectory, counts[1] = still active
__global__ void k_ls_decide(LsSettings st, const hsqp_perf* __restrict__ base, hsqp_perf* __restrict__ trial, int B, LsState* __restrict__ ls,
                            int* __restrict__ counts) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  LsState s = ls[b];
  if (!s.active) { if (s.dirty) { s.dirty = 0; ls[b] = s; } return; }
  ls_decide(st, base[b], trial[b], s);
  if (s.step_type == HSQP_STEP_ZERO && !s.active) trial[b] = base[b];   // no step: the performance index is the baseline's
  if (s.dirty) { s.active = s.step_type == HSQP_STEP_ZERO ? 0 : 1; atomicAdd(&counts[0], 1); }
  if (s.active) atomicAdd(&counts[1], 1);
  ls[b] = s;
}

// ---- line search: recompute x_new, u_new of the instances whose step length changed
__global__ __launch_bounds__(64) void k_ls_retake(const double* __restrict__ x, const double* __restrict__ u, const double* __restrict__ dx,
                                                  const double* __restrict__ du, int N, const LsState* __restrict__ ls,
                                                  double* __restrict__ x_new, double* __restrict__ u_new) {
  const int node = blockIdx.x, b = node / N, k = node % N;
  if (!ls[b].dirty) return;
  const double alpha = ls[b].alpha;
  const size_t xo = ((size_t)b * (N + 1) + k) * NX, uo = (size_t)node * NU;
  for (int i = threadIdx.x; i < NX; i += blockDim.x) x_new[xo + i] = x[xo + i] + alpha * dx[xo + i];
  for (int i = threadIdx.x; i < NU; i += blockDim.x) u_new[uo + i] = u[uo + i] + alpha * du[uo + i];
  if (k == N - 1)
    for (int i = threadIdx.x; i < NX; i += blockDim.x) x_new[xo + NX + i] = x[xo + NX + i] + alpha * dx[xo + NX + i];
}

// ---- KKT residual of the projected QP (reporting only, not part of an SQP step): one workgroup per (instance, node), the
//      per-instance maxima by atomic max on the bit patterns of the (non-negative) residuals
__global__ __launch_bounds__(256, 4) void k_kkt(const double* __restrict__ x_init, const double* __restrict__ x, const double* __restrict__ qp,
                                             const double* __restrict__ vf, const double* __restrict__ dx, const double* __restrict__ ut, int N,
                                             double* __restrict__ kkt, double* __restrict__ ginf) {
  __shared__ KktWS w;
  __shared__ double dx0[NX], r2[2], gred[128];
  const int node = blockIdx.x, b = node / N, k = node % N;
  const Ctx ctx{(int)threadIdx.x, 256, nullptr};
  if (k == 0) {
    for (int i = threadIdx.x; i < NX; i += blockDim.x) dx0[i] = x_init[(size_t)b * NX + i] - x[(size_t)b * (N + 1) * NX + i];
    __syncthreads();
  }
  const double* vfb = vf + (size_t)b * (N + 1) * VF_SIZE;
  const double* dxb = dx + (size_t)b * (N + 1) * NX;
  kkt_node(ctx, w, qp + (size_t)node * QP_SIZE, vfb + (size_t)k * VF_SIZE, vfb + (size_t)(k + 1) * VF_SIZE, dxb + (size_t)k * NX,
           dxb + (size_t)(k + 1) * NX, ut + (size_t)node * NUT, k == 0 ? dx0 : nullptr, r2);
  if (threadIdx.x < 2) atomicMax(reinterpret_cast<unsigned long long*>(kkt + 2 * b + threadIdx.x), (unsigned long long)__double_as_longlong(r2[threadIdx.x]));
  // |g|_inf of the projected QP: q~ (58) and r~ (23) of this node
  {
    const double* q = qp + (size_t)node * QP_SIZE;
    const int i = threadIdx.x;
    if (i < 128) gred[i] = i < NX ? fabs(q[QP_QV + i]) : (i < NX + NUT ? fabs(q[QP_RV + i - NX]) : 0.0);
    __syncthreads();
    if (i == 0) {
      double m = 0.0;
      for (int l = 0; l < 128; ++l) m = (gred[l] != gred[l]) ? HUGE_VAL : fmax(m, gred[l]);
      atomicMax(reinterpret_cast<unsigned long long*>(ginf + b), (unsigned long long)__double_as_longlong(m));
    }
  }
}

// ---- gate of the two-level sweep: the KKT residual of the LAST stage of every segment but the last one.  Inside a segment the gains come
//      from an exact recursion started at the segment's end, so its stages are stationary up to rounding; what the scanned boundary value
//      functions got wrong shows at stage k_p - 1, whose gains were derived from the scanned suffix p while its successor costate is the
//      value function segment p's own recursion arrives at (vf: written by k_seg_riccati for exactly these nodes).  B (P - 1) workgroups
//      instead of the B N of k_kkt (135 us at 32 x 100 nodes).
__global__ __launch_bounds__(256, 4) void k_kkt_boundaries(const double* __restrict__ x_init, const double* __restrict__ x, const double* __restrict__ qp,
                                                        const double* __restrict__ vf, const double* __restrict__ dx, const double* __restrict__ ut, int N, int P,
                                                        double* __restrict__ kkt, double* __restrict__ ginf) {
  __shared__ KktWS w;
  __shared__ double r2[2], gred[128];
  const int b = blockIdx.x / (P - 1), p = 1 + blockIdx.x % (P - 1), k = seg_bound(p, N, P) - 1;
  const Ctx ctx{(int)threadIdx.x, 256, nullptr};
  const double* vfb = vf + (size_t)b * (N + 1) * VF_SIZE;
  const double* dxb = dx + (size_t)b * (N + 1) * NX;
  const size_t node = (size_t)b * N + k;
  (void)x_init; (void)x;   // (k >= 1 here: the initial-condition residual belongs to stage 0, which is no boundary stage)
  kkt_node(ctx, w, qp + node * QP_SIZE, vfb + (size_t)k * VF_SIZE, vfb + (size_t)(k + 1) * VF_SIZE, dxb + (size_t)k * NX, dxb + (size_t)(k + 1) * NX, ut + node * NUT, nullptr, r2);
  if (threadIdx.x < 2) atomicMax(reinterpret_cast<unsigned long long*>(kkt + 2 * b + threadIdx.x), (unsigned long long)__double_as_longlong(r2[threadIdx.x]));
  {
    const double* q = qp + node * QP_SIZE;
    const int i = threadIdx.x;
    if (i < 128) gred[i] = i < NX ? fabs(q[QP_QV + i]) : (i < NX + NUT ? fabs(q[QP_RV + i - NX]) : 0.0);
    __syncthreads();
    if (i == 0) {
      double m = 0.0;
      for (int l = 0; l < 128; ++l) m = (gred[l] != gred[l]) ? HUGE_VAL : fmax(m, gred[l]);
      atomicMax(reinterpret_cast<unsigned long long*>(ginf + b), (unsigned long long)__double_as_longlong(m));
    }
  }
}

// ---- per-node parameter table from the compact per-instance reference: one thread per (instance, node)
__global__ __launch_bounds__(64) void k_params(const DevModel* __restrict__ dm, hsqp_swing_config cfg, double terrain, int arm_swing, int max_events,
                                               const int* __restrict__ n_events, const double* __restrict__ ev, const int* __restrict__ seq, int n_knots,
                                               const double* __restrict__ tt, const double* __restrict__ ts, double t0, double dt, const double* __restrict__ times,
                                               int N, int B, double* __restrict__ par, int* __restrict__ bad, const double* __restrict__ terrain_b,
                                               const double* __restrict__ lift_rows, const double* __restrict__ touch_rows) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= B * (N + 1)) return;
  const int b = id / (N + 1), k = id % (N + 1);
  // terrain_b (may be null): one terrain height per instance in place of `terrain` (include/hsqp_ground.h)
  // lift_rows, touch_rows (both null or both given): [B][2][max_events + 1], the planner's three-argument update (include/hsqp_perceive.h)
  const size_t rows = (size_t)b * 2 * (max_events + 1);
  const bool ok = node_params_eval(cfg, terrain_b ? terrain_b[b] : terrain, arm_swing, n_events[b], ev + (size_t)b * max_events, seq + (size_t)b * (max_events + 1), n_knots,
                                   tt + (size_t)b * n_knots, ts + (size_t)b * n_knots * NX, times ? times[id] : t0 + k * dt, par + (size_t)id * NP,
                                   lift_rows ? lift_rows + rows : nullptr, lift_rows ? touch_rows + rows : nullptr, max_events + 1);
  if (!ok) atomicExch(bad, 1);
}

// ---- velocity-command targets (hsqp_loop.h): one thread per instance-knot; a workgroup holds whole instances (CMDT_THREADS is a multiple of three), so
// the barrier between the read of the filter state and its update in place covers the three items that read it
constexpr int CMDT_THREADS = 192;
static_assert(CMDT_THREADS % CMD_KNOTS == 0 && CMDT_THREADS % 64 == 0, "whole instances and whole waves per workgroup");
__global__ __launch_bounds__(CMDT_THREADS) void k_command_targets(const DevModel* __restrict__ dm, double alpha, const double* __restrict__ v_cmd, double* v_filt,
                                                                  const double* __restrict__ x0, double t0, double horizon, int B, double* __restrict__ tt,
                                                                  double* __restrict__ ts) {
  const int id = blockIdx.x * CMDT_THREADS + threadIdx.x;
  const bool live = id < B * CMD_KNOTS;
  CommandItem it{};
  if (live) it = command_item_load(alpha, v_cmd, v_filt, id);
  __syncthreads();
  if (live) command_item_store(it, dm->default_joint_state, x0, t0, horizon, id, v_filt, tt, ts);
}

// ---- velocity-command targets of the centroidal formulation (hsqp_cent_loop.h): one wave per instance on a CentWST<false> workspace in LDS (the launch shape of
// k_params_cent_torso and k_cent_policy_map: eight such workgroups per CU).  The tree walk of the base-velocity solve runs across the lanes, one lane closes the
// solve, three lanes write the knots; the lane of knot 0 writes the new filter state and base_vel [B][6] (may be null).  No atomics, nothing but the grid depends on B
__global__ __launch_bounds__(64) void k_command_targets_cent(const DevModel* __restrict__ dm, double alpha, const double* __restrict__ v_cmd, double* v_filt,
                                                             const double* __restrict__ x0, double t0, double horizon, double* __restrict__ tt, double* __restrict__ ts,
                                                             double* __restrict__ base_vel) {
  CentWST<false>& w = *reinterpret_cast<CentWST<false>*>(hsqp_smem);
  const Ctx ctx{(int)threadIdx.x, 64, nullptr};
  const size_t b = blockIdx.x;
  cent_command_targets_instance(ctx, *dm, w, alpha, v_cmd + b * CMD_N, v_filt + b * CMD_N, x0 + b * NX, t0, horizon, tt + b * CMD_KNOTS, ts + b * CMD_KNOTS * NX,
                                base_vel ? base_vel + b * 6 : nullptr);
}

// ---- ground-height estimate from the stance feet (hsqp_ground.h): one lane per (instance, foot), 32 instances per 64-lane workgroup.  A lane walks the
// kinematics of its leg; the two lanes of an instance are neighbours in one wave and exchange their height with a lane shuffle, OUTSIDE the live guard
// (a dead lane's partner is dead too: B instances are 2 B lanes); the lane of foot 0 applies the rule, writes g_out (the loop: the latch's shadow) and
// both heights, and — the loop's second phase, k_ground_apply's work in the same launch — shifts the instance's three target knots and writes its
// terrain height for k_params.  No atomics, no barrier
constexpr int GROUND_THREADS = 64;
__global__ __launch_bounds__(GROUND_THREADS) void k_ground_estimate(const DevModel* __restrict__ dm, GroundArgs a) {
  const int id = blockIdx.x * GROUND_THREADS + threadIdx.x, b = id / 2, f = id % 2;
  const bool live = b < a.B;
  double z = 0.0;
  if (live) z = ground_foot_height(*dm, a.x + (size_t)b * NX, f);
  const double other = __shfl_xor(z, 1);
  if (live && f == 0) {
    const double both[2] = {z, other};
    ground_instance_finish(a, b, both);
  }
}

// ---- per-foot swing heights from the height map (hsqp_perceive.h): one lane per (instance, foot), 32 instances per 64-lane workgroup.  A lane walks the
// kinematics of its leg and the phases of its schedule and writes its own rows; lanes exchange nothing.  A dead lane (b >= B) reads and writes nothing.
// No atomics, no barrier, no cross-lane operation
constexpr int PERCEIVE_THREADS = 64;
__global__ __launch_bounds__(PERCEIVE_THREADS) void k_foot_heights(const DevModel* __restrict__ dm, ContactParams cp, TerrainParams tp, PerceiveArgs a) {
  const int id = blockIdx.x * PERCEIVE_THREADS + threadIdx.x, b = id / 2, f = id % 2;
  if (b >= a.B) return;
  perceive_lane(*dm, cp, tp, a, b, f);
}

// ---- gait schedule and ladder (hsqp_gait.h): one wave per instance, the work row of its schedule in LDS; reads the live state `in`, writes the shadow
// state `out` and one status word per instance (the host swaps the two after it has read the words)
__global__ __launch_bounds__(64) void k_gait_update(const hsqp_gait_settings* __restrict__ gs, GaitState in, GaitState out, double t, double horizon,
                                                    const double* __restrict__ v_filt, const double* __restrict__ x, int* __restrict__ n_out,
                                                    double* __restrict__ ev_out, int* __restrict__ seq_out, int* __restrict__ status) {
  __shared__ GaitWork w;
  const int b = blockIdx.x, E = gs->max_events;
  const int st = gait_update_instance(Ctx{(int)threadIdx.x, 64, nullptr}, *gs, w, in, out, b, t, horizon, v_filt + (size_t)b * CMD_N, x + (size_t)b * NX, n_out + b,
                                      ev_out + (size_t)b * E, seq_out + (size_t)b * (E + 1));
  if (threadIdx.x == 0) status[b] = st;
}

// ---- the event-node time grid (hsqp_grid.h): the recurrence is serial and a few flops per node, so one LANE per instance, 64 instances per workgroup.
// An instance reads its own events and writes its own rows (dt_nodes, node_times, n_intervals, status); `any_bad` (may be null) is set, never cleared,
// by an instance that fails; dts_keep (may be null): a second copy of the instance's interval lengths (the loop's record of the cycle)
__global__ __launch_bounds__(64) void k_event_grid(double t0, int n_nodes, double dt, double dt_min, int event_nodes, int B, int max_events,
                                                   const int* __restrict__ n_events, const double* __restrict__ event_times, int* __restrict__ n_intervals,
                                                   double* __restrict__ dts, double* __restrict__ nts, int* __restrict__ status, int* any_bad,
                                                   double* __restrict__ dts_keep) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const size_t N = (size_t)n_nodes + event_nodes;
  int nb = 0;
  const int st = grid_build_instance(t0, n_nodes, dt, dt_min, event_nodes, max_events, n_events[b], event_times + (size_t)b * max_events, &nb, dts + (size_t)b * N,
                                     nts + (size_t)b * (N + 1));
  n_intervals[b] = nb;
  if (status) status[b] = st;
  if (st != HSQP_GRID_OK && any_bad) *any_bad = 1;
  if (dts_keep) for (size_t k = 0; k < N; ++k) dts_keep[(size_t)b * N + k] = dts[(size_t)b * N + k];
}

// ---- failure isolation and episode reset of the resident loop (hsqp_episode.h): one wave per instance
__global__ __launch_bounds__(64) void k_loop_triage(TriageArgs a) { triage_instance(Ctx{(int)threadIdx.x, 64, nullptr}, a, blockIdx.x); }
// step 0 of a cycle with the observation model in force, and hsqp_observe_eval (include/hsqp_observe.h, csrc/hsqp_observe.h): OBS_THREADS items
// (instance, block of four entries) per workgroup
__global__ __launch_bounds__(OBS_THREADS) void k_observe(ObserveArgs a) {
  const Ctx ctx{(int)threadIdx.x, OBS_THREADS, nullptr};
  observe_group(ctx, a, blockIdx.x);
}
// entry blockIdx.x of a hsqp_loop_reset_instances request
__global__ __launch_bounds__(64) void k_episode_host_reset(HostResetArgs a) { host_reset_instance(Ctx{(int)threadIdx.x, 64, nullptr}, a, blockIdx.x); }
// the command in use of every instance from its state (behind hsqp_loop_isolate and hsqp_loop_command): one thread per entry
__global__ __launch_bounds__(64) void k_episode_commands(const int* __restrict__ state, const double* __restrict__ v_cmd, const double* __restrict__ x_reset, int B,
                                                         double* __restrict__ v_use, int pose) {
  const int id = blockIdx.x * 64 + threadIdx.x, b = id / CMD_N, i = id % CMD_N;
  if (b < B) v_use[id] = episode_command_entry(state[b], v_cmd + (size_t)b * CMD_N, x_reset + (size_t)b * NX, i, pose);
}
// the per-instance gait reset at time t.  ids == null: workgroup b serves instance b if flags[b] is set (behind the triage); otherwise workgroup i
// serves instance ids[i] (hsqp_loop_reset_instances)
__global__ __launch_bounds__(64) void k_gait_reset_instances(GaitState s, int E, const int* __restrict__ ids, const int* __restrict__ flags, double t) {
  const int b = ids ? ids[blockIdx.x] : (int)blockIdx.x;
  if (!ids && !flags[b]) return;
  gait_reset_instance(Ctx{(int)threadIdx.x, 64, nullptr}, s, E, b, t);
}

// ---- receding-horizon warm start (hsqp_warm.h) behind k_params: one wave per node of the new grid, WARM_WAVES nodes per workgroup
// (blockIdx.x), one instance per blockIdx.y; the instance's previous stamps are staged in LDS once per workgroup (SHIFT)
constexpr int WARM_WAVES = 4;
__global__ __launch_bounds__(64 * WARM_WAVES) void k_warm_start(WarmArgs w) {
  double* tp = reinterpret_cast<double*>(hsqp_smem);
  const int b = blockIdx.y, k = blockIdx.x * WARM_WAVES + wave_index(threadIdx.x);
  if (warm_mode(w, b) == HSQP_WARM_SHIFT) {   // (uniform: a workgroup serves one instance)
    const double* src = w.stamps_prev + (size_t)b * (w.N_prev + 1);
    for (int i = threadIdx.x; i <= w.N_prev; i += blockDim.x) tp[i] = src[i];
    __syncthreads();
  }
  if (k > w.N) return;
  warm_node(Ctx{(int)(threadIdx.x & 63), 64, nullptr}, w, tp, b, k);
}

// ---- policy evaluation / joint torques in three small kernels.
//  k_policy_inputs: one workgroup per pair — xt != null: interpolate the trajectories of instance blockIdx.x at s[blockIdx.x]
//                   (uniform grid, or dts != null: the instance's interval lengths); otherwise take the pair from xin / uin.
//  k_cent_policy_map (centroidal handles): one wave per pair — the whole-body (x, u) computeJointTorques needs
//                   (CentroidalMpcMrtJointController::computeJointControlAction, humanoid_centroidal_mpc/src/mrt/
//                   CentroidalMpcMrtJointController.cpp:155-175): q = getGeneralizedCoordinates(x), qd = getGeneralizedVelocities(x, u)
//                   with the base velocity from the centroidal momentum, v_b = A_b^-1 (m h - A_j qd_j) = rows 6..11 of the flow map,
//                   the contact wrenches, and the desired joint accelerations carried in entries 35..57 of the INPUT state row.
//  k_policy_torques: one workgroup per pair — model evaluation + torques (hsqp_policy.h).
__global__ __launch_bounds__(64) void k_policy_inputs(const double* __restrict__ xt, const double* __restrict__ ut, int N, double dt, const double* __restrict__ dts,
                                                      const double* __restrict__ s, const double* __restrict__ xin, const double* __restrict__ uin,
                                                      double* __restrict__ xout, double* __restrict__ uout) {
  const int b = blockIdx.x;
  const Ctx ctx{(int)threadIdx.x, 64, nullptr};
  if (xt) {
    if (dts) policy_interpolate_grid(ctx, xt + (size_t)b * (N + 1) * NX, ut + (size_t)b * N * NU, N, dts + (size_t)b * N, s[b], xout + (size_t)b * NX, uout + (size_t)b * NU);
    else policy_interpolate(ctx, xt + (size_t)b * (N + 1) * NX, ut + (size_t)b * N * NU, N, dt, s[b], xout + (size_t)b * NX, uout + (size_t)b * NU);
  } else {
    for (int i = threadIdx.x; i < NX + NU; i += blockDim.x) { if (i < NX) xout[(size_t)b * NX + i] = xin[(size_t)b * NX + i]; else uout[(size_t)b * NU + i - NX] = uin[(size_t)b * NU + i - NX]; }
  }
}
__global__ __launch_bounds__(64) void k_cent_policy_map(const DevModel* __restrict__ dm, int n, const double* __restrict__ xc, const double* __restrict__ uc,
                                                        double* __restrict__ xwb, double* __restrict__ uwb) {
  const int b = blockIdx.x;
  CentWST<false>& w = *reinterpret_cast<CentWST<false>*>(hsqp_smem);
  const Ctx ctx{(int)threadIdx.x, 64, nullptr};
  const double* x = xc + (size_t)b * NX;
  const double* u = uc + (size_t)b * NU;
  double* xo = xwb + (size_t)b * NX;
  double* uo = uwb + (size_t)b * NU;
  cent_base_velocity(ctx, *dm, w, x, u, xo + NV);     // [pdot; euler rates] -> the base velocities of the whole-body state
  for (int i = threadIdx.x; i < NX + NU; i += blockDim.x) {
    if (i < NV) xo[i] = x[6 + i];
    else if (i >= NV + 6 && i < NX) { const int j = i - NV - 6; xo[i] = u[12 + j]; }
    else if (i >= NX && i < NX + 12) uo[i - NX] = u[i - NX];
    else if (i >= NX + 12) { const int j = i - NX - 12; uo[12 + j] = x[HSQP_CNX + j]; }
  }
}
struct PolicyWS { StageWST<false> st; double x[NX], u[NU]; };
__global__ __launch_bounds__(128) void k_policy_torques(const DevModel* __restrict__ dm, const double* __restrict__ xwb, const double* __restrict__ uwb,
                                                        double* __restrict__ tau) {
  PolicyWS& w = *reinterpret_cast<PolicyWS*>(hsqp_smem);
  const int b = blockIdx.x;
  const Ctx ctx{(int)threadIdx.x, 128, nullptr};
  for (int i = threadIdx.x; i < NX + NU; i += blockDim.x) { if (i < NX) w.x[i] = xwb[(size_t)b * NX + i]; else w.u[i - NX] = uwb[(size_t)b * NU + i - NX]; }
  __syncthreads();
  policy_node(ctx, *dm, w.st, w.x, w.u, tau + (size_t)b * NJ);
}

// ---- Riccati feedback policy (hsqp_feedback.h), formed lazily by the feedback entry points: nothing of it runs inside an iteration.
//  k_feedback_gains: one workgroup per (entry first + blockIdx.x, instance blockIdx.y) — (K, uff) of the entry's source node into
//                    K [B][count][35][58] / uff [B][count][35] (either may be null).
//  k_feedback_eval:  one workgroup per instance — the entries of the input segment at s[b] (policy_segment_*: the one the feed-forward
//                    evaluation takes), blended with its weight, applied to the measured state: u[b] = uff(s) + K(s) x_meas[b].
constexpr int FB_THREADS = 256;
__global__ __launch_bounds__(FB_THREADS) void k_feedback_gains(const double* __restrict__ qp, const double* __restrict__ ric, const double* __restrict__ x,
                                                               const double* __restrict__ u, const double* __restrict__ dts, int N, int first, int count, int cent,
                                                               double* __restrict__ K, double* __restrict__ uff) {
  FeedbackWS& w = *reinterpret_cast<FeedbackWS*>(hsqp_smem);
  const int j = blockIdx.x, b = blockIdx.y;
  const int k = feedback_source_node(dts + (size_t)b * N, N, first + j);
  const size_t node = (size_t)b * N + k;
  feedback_node(Ctx{(int)threadIdx.x, FB_THREADS, nullptr}, qp + node * QP_SIZE, ric + node * RIC_SIZE, x + ((size_t)b * (N + 1) + k) * NX, u + node * NU, cent, w);
  const size_t e = (size_t)b * count + j;
  if (K) for (int i = threadIdx.x; i < NU * NX; i += FB_THREADS) K[e * NU * NX + i] = (&w.K[0][0])[i];
  if (uff) for (int i = threadIdx.x; i < NU; i += FB_THREADS) uff[e * NU + i] = w.uff[i];
}
struct FeedbackEvalWS { FeedbackWS fb; double K0[NU][NX]; double uff0[NU]; double xm[NX]; };
static_assert(sizeof(FeedbackEvalWS) <= 65536, "the feedback kernels run without a dynamic-LDS attribute");
__global__ __launch_bounds__(FB_THREADS) void k_feedback_eval(const double* __restrict__ qp, const double* __restrict__ ric, const double* __restrict__ x,
                                                              const double* __restrict__ u, const double* __restrict__ dts, int N, double dt, int uniform, int cent,
                                                              const double* __restrict__ s, const double* __restrict__ x_meas, double* __restrict__ u_out) {
  FeedbackEvalWS& w = *reinterpret_cast<FeedbackEvalWS*>(hsqp_smem);
  const int b = blockIdx.x;
  const Ctx ctx{(int)threadIdx.x, FB_THREADS, nullptr};
  const double* db = dts + (size_t)b * N;
  const PolicySegment g = uniform ? policy_segment_uniform(N, dt, s[b]) : policy_segment_grid(N, db, s[b]);
  const double a = g.au;
  for (int i = threadIdx.x; i < NX; i += FB_THREADS) w.xm[i] = x_meas[(size_t)b * NX + i];
  for (int e = 0; e < 2; ++e) {
    const int k = feedback_source_node(db, N, g.ku + e);
    const size_t node = (size_t)b * N + k;
    feedback_node(ctx, qp + node * QP_SIZE, ric + node * RIC_SIZE, x + ((size_t)b * (N + 1) + k) * NX, u + node * NU, cent, w.fb);
    if (e == 0) {
      for (int i = threadIdx.x; i < NU * NX + NU; i += FB_THREADS) {
        if (i < NU * NX) (&w.K0[0][0])[i] = (&w.fb.K[0][0])[i];
        else w.uff0[i - NU * NX] = w.fb.uff[i - NU * NX];
      }
      __syncthreads();
    }
  }
  // (entry ku + 1 is in w.fb) interpolated gain and bias, then the linear controller at the measured state
  const int nc = cent ? HSQP_CNX : NX;
  for (int r = threadIdx.x; r < NU; r += FB_THREADS) {
    double kx = 0.0;
    for (int c = 0; c < nc; ++c) kx += ((1.0 - a) * w.K0[r][c] + a * w.fb.K[r][c]) * w.xm[c];
    u_out[(size_t)b * NU + r] = ((1.0 - a) * w.uff0[r] + a * w.fb.uff[r]) + kx;
  }
}

// ---- Riccati value function (include/hsqp_value.h, csrc/hsqp_value.h), launched by its entry points only: nothing of it runs inside an iteration.
//  k_value_record: one workgroup per (node k0 + blockIdx.x, instance blockIdx.y) — the node's S (symmetrised), s and xbar into S [B][count][58][58] /
//                  s [B][count][58] / xbar [B][count][58] (any may be null).
//  k_value_eval:   one workgroup per (query blockIdx.x, instance blockIdx.y) — value_eval at (s_query, x_query) into dV [B][n] / dfdx [B][n][58] /
//                  dfdxx [B][n][58][58] (any may be null).
__global__ __launch_bounds__(VAL_THREADS) void k_value_record(const double* __restrict__ vf, const double* __restrict__ xbar, int N, int k0, int count, int cent,
                                                              double* __restrict__ S, double* __restrict__ s, double* __restrict__ xb) {
  ValueWS& w = *reinterpret_cast<ValueWS*>(hsqp_smem);
  const int j = blockIdx.x, b = blockIdx.y;
  const size_t node = (size_t)b * (N + 1) + k0 + j, e = (size_t)b * count + j;
  value_record_node(Ctx{(int)threadIdx.x, VAL_THREADS, nullptr}, vf + node * VF_SIZE, xbar + node * NX, cent, S ? S + e * NX * NX : nullptr, s ? s + e * NX : nullptr,
                    xb ? xb + e * NX : nullptr, w);
}
__global__ __launch_bounds__(VAL_THREADS) void k_value_eval(const double* __restrict__ vf, const double* __restrict__ xbar, const double* __restrict__ dts, int N, double dt,
                                                            int uniform, int cent, int n, const double* __restrict__ s_query, const double* __restrict__ x_query,
                                                            double* __restrict__ dV, double* __restrict__ dfdx, double* __restrict__ dfdxx) {
  ValueWS& w = *reinterpret_cast<ValueWS*>(hsqp_smem);
  const int q = blockIdx.x, b = blockIdx.y;
  const size_t e = (size_t)b * n + q;
  value_eval(Ctx{(int)threadIdx.x, VAL_THREADS, nullptr}, vf + (size_t)b * (N + 1) * VF_SIZE, xbar + (size_t)b * (N + 1) * NX, uniform ? nullptr : dts + (size_t)b * N, N, dt,
             cent, s_query[e], x_query + e * NX, dV ? dV + e : nullptr, dfdx ? dfdx + e * NX : nullptr, dfdxx ? dfdxx + e * NX * NX : nullptr, w);
}

// ---- batched policy rollout (include/hsqp_rollout.h, csrc/hsqp_rollout.h), launched by the rollout entry points only.
//  k_rollout_window: one workgroup — over the instances, the policy entries the call's times [s0, s0 + duration] reach (the feedback
//                    controller's gain window [out[0], out[1]]) and whether an s0 is not finite (out[2]).
//  k_rollout:        one workgroup per instance — the whole integration of the instance (all samples, events, step control).
constexpr int RO_WIN_THREADS = 256;
__global__ __launch_bounds__(RO_WIN_THREADS) void k_rollout_window(const double* __restrict__ s0, int B, double duration, const double* __restrict__ dts, int N,
                                                                   double dt, int uniform, int* __restrict__ out) {
  __shared__ int lo[RO_WIN_THREADS], hi[RO_WIN_THREADS], bad[RO_WIN_THREADS];
  const int t = threadIdx.x;
  int l = N, u = 0, f = 0;
  for (int b = t; b < B; b += RO_WIN_THREADS) {
    const double s = s0[b];
    if (!ro_finite(s)) { f = 1; continue; }
    const double* db = dts + (size_t)b * N;
    const PolicySegment g0 = uniform ? policy_segment_uniform(N, dt, s) : policy_segment_grid(N, db, s);
    const PolicySegment g1 = uniform ? policy_segment_uniform(N, dt, s + duration) : policy_segment_grid(N, db, s + duration);
    l = g0.ku < l ? g0.ku : l;
    u = g1.ku + 1 > u ? g1.ku + 1 : u;
  }
  lo[t] = l; hi[t] = u; bad[t] = f;
  __syncthreads();
  if (t == 0) {
    for (int i = 1; i < RO_WIN_THREADS; ++i) { l = lo[i] < l ? lo[i] : l; u = hi[i] > u ? hi[i] : u; f |= bad[i]; }
    out[0] = l; out[1] = u; out[2] = f;
  }
}

// What either kernel does for its instance is rollout_entry (hsqp_rollout.h), which the host emulation runs.  The kernels spell the same statements out instead of
// calling it: through one more inlined call the compiler schedules the plant kernels differently (same registers, LDS and scratch, other SGPR spills) and the
// loop on the torque plant with every option measured 2.7 .. 3.1 % slower than with these bodies (profiles/rollout_entry_ab.txt).  Keep the two in step.
// k_rollout: the flow maps.  k_rollout_plant: the torque plant (include/hsqp_plant.h), one instantiation per set of its options — the ground (cp), the actuator
// model (ap), the inertial variation (ip), the height-map terrain under the ground (tp): a block is read only by the instantiations whose SW carries its part.  An option is a parameter of the instantiation
// because as a run-time branch the contact alone costs the rollout without a ground 3.6 % (measured); whether the command is held (ap.period > 0)
// is a run-time, workgroup-uniform branch.  rollout_impl picks SW through rollout_dispatch.
template <class SW>
__global__ __launch_bounds__(RO_THREADS) void k_rollout(const DevModel* __restrict__ dm, RolloutArgs a) {
  RolloutWS<SW>& w = *reinterpret_cast<RolloutWS<SW>*>(hsqp_smem);
  const int b = blockIdx.x;
  const RolloutPolicy p{a.ut + (size_t)b * a.N * NU, a.dts ? a.dts + (size_t)b * a.N : nullptr, a.N, a.dt, a.K ? a.K + (size_t)b * a.count * NU * NX : nullptr,
                        a.uff ? a.uff + (size_t)b * a.count * NU : nullptr, a.first, a.count, dm->formulation == HSQP_FORM_CENTROIDAL ? 1 : 0};
  rollout_instance(Ctx{(int)threadIdx.x, RO_THREADS, nullptr}, *dm, w, p, a.st, a.s0[b], a.x0 + (size_t)b * NX, a.duration, a.n,
                   a.x ? a.x + (size_t)b * a.n * NX : nullptr, a.u ? a.u + (size_t)b * a.n * NU : nullptr, a.status + b, a.steps ? a.steps + b : nullptr,
                   a.rejected ? a.rejected + b : nullptr, a.push, b);
}
template <class SW>
__global__ __launch_bounds__(RO_THREADS) void k_rollout_plant(const DevModel* __restrict__ dm, RolloutArgs a, PlantParams pp, ContactParams cp, ActuatorParams ap,
                                                              InertiaParams ip, TerrainParams tp) {
  RolloutWS<SW>& w = *reinterpret_cast<RolloutWS<SW>*>(hsqp_smem);
  const int b = blockIdx.x;
  const Ctx ctx{(int)threadIdx.x, RO_THREADS, nullptr};
  const RolloutPolicy p{a.ut + (size_t)b * a.N * NU, a.dts ? a.dts + (size_t)b * a.N : nullptr, a.N, a.dt, a.K ? a.K + (size_t)b * a.count * NU * NX : nullptr,
                        a.uff ? a.uff + (size_t)b * a.count * NU : nullptr, a.first, a.count, 0};
  plant_load(ctx, pp, b, a.N, w.sw.pl);
  if constexpr (PlantGrounded<SW>::value) contact_load(ctx, cp, b, w.sw.ct);
  if constexpr (PlantOnTerrain<SW>::value) terrain_load(ctx, tp, b, w.sw.ct.ter);
  if constexpr (RolloutActuated<SW>::value) actuator_load(ctx, ap, b, w.sw.act);
  if constexpr (PlantIsVaried<SW>::value) inertia_load(ctx, ip, b, w.sw.iw);
  rollout_instance(ctx, *dm, w, p, a.st, a.s0[b], a.x0 + (size_t)b * NX, a.duration, a.n, a.x ? a.x + (size_t)b * a.n * NX : nullptr,
                   a.u ? a.u + (size_t)b * a.n * NU : nullptr, a.status + b, a.steps ? a.steps + b : nullptr, a.rejected ? a.rejected + b : nullptr, a.push, b);
}
// hsqp_inertia_eval (include/hsqp_inertia.h): one workgroup per instance — the plant's mass matrix, bias forces and total mass at a given state: stage
// topology, one stage_eval<false>, the instance's variation, the assembly of the plant's bordered system
__global__ __launch_bounds__(RO_THREADS) void k_inertia_eval(const DevModel* __restrict__ dm, InertiaParams ip, const double* __restrict__ x, double* __restrict__ M,
                                                             double* __restrict__ nle, double* __restrict__ mass) {
  InertiaEvalWS& w = *reinterpret_cast<InertiaEvalWS*>(hsqp_smem);
  const int b = blockIdx.x;
  const Ctx ctx{(int)threadIdx.x, RO_THREADS, nullptr};
  inertia_eval_instance(ctx, *dm, w, ip, b, x + (size_t)b * NX, M ? M + (size_t)b * NV * NV : nullptr, nle ? nle + (size_t)b * NV : nullptr, mass ? mass + b : nullptr);
}
static_assert(sizeof(InertiaEvalWS) <= 65536, "hsqp_inertia_eval runs without a dynamic-LDS attribute");
// hsqp_contact_eval (include/hsqp_contact.h): one workgroup per instance — the contact model at a given state: stage topology, one stage_eval<false>
// for the placements and the link velocities, the eight points.  CT: ContactSet, or ContactTerrainSet while a terrain is resident (tp is read by that one only)
template <class CT>
__global__ __launch_bounds__(RO_THREADS) void k_contact_eval(const DevModel* __restrict__ dm, ContactParams cp, TerrainParams tp, const double* __restrict__ x,
                                                             double* __restrict__ force, double* __restrict__ pen) {
  ContactEvalWST<CT>& w = *reinterpret_cast<ContactEvalWST<CT>*>(hsqp_smem);
  const int b = blockIdx.x;
  contact_eval_instance(Ctx{(int)threadIdx.x, RO_THREADS, nullptr}, *dm, w, cp, &tp, b, x + (size_t)b * NX, force ? force + (size_t)b * CT_PTS * 3 : nullptr,
                        pen ? pen + (size_t)b * CT_PTS : nullptr);
}
static_assert(sizeof(ContactEvalWST<ContactTerrainSet>) <= 65536, "hsqp_contact_eval runs without a dynamic-LDS attribute");
// the episode metrics of the resident loop (include/hsqp_metrics.h, csrc/hsqp_metrics.h): one workgroup per instance behind the rollout of a cycle.
// CT: MetricsNoGround (the light path: no stage evaluation), ContactSet, or ContactTerrainSet while a terrain is resident (tp is read by that one only)
template <class CT>
__global__ __launch_bounds__(RO_THREADS) void k_loop_metrics(const DevModel* __restrict__ dm, MetricsArgs a, ContactParams cp, TerrainParams tp) {
  MetricsWST<CT>& w = *reinterpret_cast<MetricsWST<CT>*>(hsqp_smem);
  metrics_instance<CT>(Ctx{(int)threadIdx.x, RO_THREADS, nullptr}, *dm, w, a, cp, &tp, blockIdx.x);
}
static_assert(sizeof(MetricsWST<ContactTerrainSet>) <= 65536, "k_loop_metrics runs without a dynamic-LDS attribute");
// ... and the host's closing of n records (hsqp_loop_reset_instances, hsqp_loop_metrics_restart): one wave per request entry
__global__ __launch_bounds__(64) void k_metrics_host_close(const int* __restrict__ ids, hsqp_metrics* rec, int* feet) {
  metrics_host_close(Ctx{(int)threadIdx.x, 64, nullptr}, ids, rec, feet, blockIdx.x);
}
// hsqp_terrain_eval (include/hsqp_terrain.h): one workgroup per instance — the ground's height and normal under n_pts world points
__global__ __launch_bounds__(RO_THREADS) void k_terrain_eval(ContactParams cp, TerrainParams tp, int n_pts, const double* __restrict__ xy, double* __restrict__ height,
                                                             double* __restrict__ normal) {
  __shared__ TerrainSet ts;
  const size_t b = blockIdx.x, n = (size_t)n_pts;
  terrain_eval_instance(Ctx{(int)threadIdx.x, RO_THREADS, nullptr}, cp, tp, ts, (int)b, n_pts, xy + b * n * 2, height ? height + b * n : nullptr,
                        normal ? normal + b * n * 3 : nullptr);
}

// ---- per-instance performance index from per-node {ne, dt*cost, dt*eq^2, dt*dyn^2} + terminal cost
__device__ inline void perf_reduce_instance(int b, const DevModel* __restrict__ dm, const double* __restrict__ misc, int misc_stride, const double* __restrict__ x,
                                            const double* __restrict__ par, int N, hsqp_perf* __restrict__ out, const LsState* __restrict__ ls) {
  if (ls && !ls[b].active) return;
  __shared__ double red[3][64];
  double c = 0.0, e = 0.0, d = 0.0;
  for (int k = threadIdx.x; k < N; k += blockDim.x) {
    const double* m = misc + ((size_t)b * N + k) * misc_stride;
    c += m[1]; e += m[2]; d += m[3];
  }
  if (threadIdx.x < NX) {  // terminal QuadraticStateCost(Q_final * scaling): HumanoidCostConstraintFactory.cpp:218-228
    const double dd = x[((size_t)b * (N + 1) + N) * NX + threadIdx.x] - par[((size_t)b * (N + 1) + N) * NP + HSQP_P_XDES + threadIdx.x];
    c += 0.5 * dm->Qf[threadIdx.x] * dd * dd;
  }
  red[0][threadIdx.x] = c; red[1][threadIdx.x] = e; red[2][threadIdx.x] = d;
  __syncthreads();
  if (threadIdx.x == 0) {
    double cs = 0.0, es = 0.0, ds = 0.0;
    for (int i = 0; i < 64; ++i) { cs += red[0][i]; es += red[1][i]; ds += red[2][i]; }
    out[b].cost = cs; out[b].merit = cs; out[b].equality_sse = es; out[b].dynamics_sse = ds;
  }
}
__global__ void k_perf_reduce(const DevModel* __restrict__ dm, const double* __restrict__ misc, int misc_stride, const double* __restrict__ x,
                              const double* __restrict__ par, int N, hsqp_perf* __restrict__ out, const LsState* __restrict__ ls) {
  perf_reduce_instance(blockIdx.x, dm, misc, misc_stride, x, par, N, out, ls);
}
// the three per-instance reductions that follow the full-step trial in ONE launch (blockIdx.y: performance index of the iterate, of the trial, the
// line-search state): three back-to-back launches of 5 us kernels cost their launch gaps
__global__ __launch_bounds__(64) void k_perf_trio(const DevModel* __restrict__ dm, const double* __restrict__ misc0, int stride0, const double* __restrict__ x,
                                                  const double* __restrict__ misc1, int stride1, const double* __restrict__ x_new, const double* __restrict__ par, int N,
                                                  hsqp_perf* __restrict__ before, hsqp_perf* __restrict__ after, const double* __restrict__ info,
                                                  const double* __restrict__ dx, LsState* __restrict__ ls) {
  if (blockIdx.y == 0) perf_reduce_instance(blockIdx.x, dm, misc0, stride0, x, par, N, before, nullptr);
  else if (blockIdx.y == 1) perf_reduce_instance(blockIdx.x, dm, misc1, stride1, x_new, par, N, after, nullptr);
  else ls_init_instance(blockIdx.x, dm, info, x, dx, par, N, ls);
}

}  // namespace

// =================================================================================================
// a device buffer of the handle: dev_ensure allocates it (grow-only), its destructor frees it.  Reads as the T* it holds.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  operator T*() const { return p; }
};

// the gate block of a handle for max_batch instances (d_kkt, h_gate): kkt [2 per instance] | |g|_inf | flags of the scan kernels (bad pivot, rank-deficient D,
// failed Lam) of the current attempt: one memset, one read-back for the scan's gate.  A null block: the sizing pass.
// (the block's own packing, which the kernels index, not Carve::take: nothing inside it is 256-byte aligned)
struct GateView { double* kkt; double* ginf; int* flags; size_t bytes; };
static GateView gate_view(double* block, size_t max_batch) {
  double* end = block ? block + 3 * max_batch : nullptr;
  return {block, block ? block + 2 * max_batch : nullptr, reinterpret_cast<int*>(end), max_batch * 3 * 8 + ((max_batch * sizeof(int) + 7) / 8) * 8};
}

struct hsqp_handle {
  hsqp_model_desc md;
  hsqp_settings st;
  DevModel hdm;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[6] = {};
  static constexpr int LQ_SPLIT_MAX = 8;
  int lq_round_blocks = 512;                   // workgroups of k_lq_limb / k_lq_rows the chip holds at once (4 waves per CU, QL_WAVES per workgroup)
  int lq_split = 1;                            // node ranges of the limb-lane LQ kernels and of k_project behind them, each on its own stream (HSQP_LQ_SPLIT in the environment at hsqp_create)
  hipStream_t aux[LQ_SPLIT_MAX - 1] = {};
  hipEvent_t ev_fork = nullptr, ev_join[LQ_SPLIT_MAX - 1] = {};
  DevBuf<DevModel> d_dm;
  DevBuf<double> d_xinit, d_x, d_u, d_par;
  DevBuf<double> d_rec, d_qp, d_ric;
  DevBuf<double> d_dx, d_du, d_ut, d_xnew, d_unew;
  DevBuf<double> d_fj;            // [B][N][NJ] rows 12 .. 34 of Px dx + Pu ut as the factored roll-out forms them (k_step then reads the wrench rows of Px / Pu only)
  DevBuf<double> d_misc, d_kkt;
  GateView gate = {};             // d_kkt's parts (gate_view)
  DevBuf<double> d_dt;            // [B][N] length of every interval (uniform grids: filled with dt)
  std::vector<double> h_dt;       // host copy (debug reads), empty for device-resident uploads
  bool uniform_grid = true, has_events = false;
  bool grid_resident = false;     // d_dt / h_dt hold the uniform grid (h_dt.size() / grid_N instances, grid_N intervals of grid_dt): set_grid
  int grid_N = 0;
  double grid_dt = 0.0;
  DevBuf<double> d_vf;            // [B][N+1][VF_SIZE] value function of the last Riccati sweep (allocated when a KKT check is first asked for)
  DevBuf<double> d_vf2;           // scan path: value functions of the refinement pass (the KKT check then reads these)
  double* h_gate = nullptr;       // pinned host copy of the gate block
  long long scan_fallbacks = 0;   // iterations whose scan result failed the KKT gate and were redone with the serial recursion
  DevBuf<double> d_acl;           // scan path: closed loop [B][N][ACL_SIZE] of every stage for the roll-out (allocated when the scan is first used)
  // segmented sweep (allocated when first used): gains of the J = 0 recursions, (L^-1)^T of every stage, (J, s) at the segment starts, zeros
  DevBuf<double> d_ric2, d_linv, d_vf0, d_zero;
  bool qp_joint_rows = false;                 // the last k_project wrote the joint rows of A~ / B~ and all of Q~ (joint_rows, hsqp_iterate_device): debug block 102
  int seg_backoff = 0, seg_backoff_len = 0;   // after a rejected gated sweep the next seg_backoff iterations go straight to the serial recursion (doubling, <= 64);
                                              // state of the AUTOMATIC sweep choice only (choose_sweep), reset by every upload
  bool backoff_persistent = false;            // hsqp_set_scan_backoff_persistent: uploads of the same (B, N) keep the back-off
  long long backoff_iterations = 0;           // iterations that ran the serial recursion because of the back-off (hsqp_scan_backoffs)
  bool seg_debug = false;                     // HSQP_SEG_DEBUG in the environment at hsqp_create
  // test aids, from the environment at hsqp_create: HSQP_POISON_LDS (k_poison_lds in front of every launch, HSQP_LAUNCH) and HSQP_POISON_HBM (every device
  // buffer the handle allocates starts as NaN bit patterns, 0xFF bytes, instead of whatever the allocator returns — usually zeros, which hide a read of
  // something never written.  Not the LQ record: the limb-lane kernels rely on its zero fill, hsqp_lql.h)
  bool poison_lds = false, poison_hbm = false;
  int poison_blocks = 512;                    // workgroups of k_poison_lds: two per CU (set from the device's CU count at hsqp_create)
  bool chain_fused = false;                   // limb-lane form: the RK4 chain of the columns of [A|B] runs inside k_project (project_node, chain), the defect on the lanes of k_lq_rows (ql_defect_lane), k_lq_chain is not launched; HSQP_LQ_CHAIN_SEPARATE in the environment at hsqp_create keeps the chain in k_lq_chain (A/B runs)
  bool lq_limb = false;                       // whole-body LQ approximation on limb lanes (hsqp_lql.h: k_lq_limb + k_lq_rows + k_lq_chain) instead of the phase form k_lq<true> (HSQP_LQ_PHASE_FORM / HSQP_LQ_LIMB_FORM in the environment at hsqp_create force either)
  bool ric_fact = false;                      // whole-body serial sweep on the factors of [A~ | B~] (hsqp_riccati_fact.h: k_riccati_fact; HSQP_RICCATI_DENSE in the environment at hsqp_create: the dense stage k_riccati<58>, for A/B runs)
  bool value_quad = false;                    // whole-body value pass on quads of lanes (hsqp_lqv.h): the tree has at most four limbs (HSQP_VALUE_PHASE_FORM in the environment at hsqp_create: the phase form, for A/B runs)
  DevBuf<hsqp_perf> d_perf_before, d_perf_after;
  DevBuf<int> d_status;
  DevBuf<double> d_stepinfo;      // [B][N][4] per-node {armijo, |dx|^2, |du|^2}
  DevBuf<LsState> d_ls;
  DevBuf<int> d_counts;
  hsqp_linesearch_settings ls_settings;
  std::vector<LsState> h_ls;                  // host copies for HSQP_ITER_UNTIL_CONVERGED (reused across iterations and calls)
  std::vector<hsqp_perf> h_perf_before;
  DevBuf<double> d_el[2];         // scan elements (allocated when the parallel-in-time sweep is first used)
  DevBuf<char> d_stage;           // staging area for the small per-call inputs (reference, policy queries: ref_stage_layout, policy_stage_layout)
  bool ls_ran = false;
  DevBuf<long long> d_prof;       // [4][128] phase-profile ticks (k_lq<true>, k_project, k_riccati, k_lq<false>)
  int B = 0, N = 0;
  double dt = 0.0;
  bool have_problem = false, have_solution = false;
  bool have_policy = false;       // the QP / Riccati records and the solution are those of the last successful iteration (feedback entry points)
  DevBuf<double> d_fb;            // staging of hsqp_feedback_policy (host destinations)
  // the value-function record (include/hsqp_value.h): kept by an iteration that ran with HSQP_ITER_VALUE_FUNCTION
  bool have_value = false;        // vf_record / d_xbar are those of the last iteration, which ran with the flag and succeeded
  const double* vf_record = nullptr;   // d_vf or d_vf2: the value functions of the sweep whose step that iteration accepted
  DevBuf<double> d_xbar;          // [B][N+1][58] the trajectory that iteration's QP was linearised at (a bit copy of d_x taken before any step)
  DevBuf<double> d_val;           // staging of the value-function entry points (host arrays)
  DevBuf<double> d_ro_gain;       // gain window of the rollout's feedback controller: K [B][count][35][58], then uff [B][count][35] (allocated when first used, sized by the window)
  DevBuf<char> d_ro;              // staging of the rollout (s0, x0, outputs of the host entry point, window, statuses)
  // the resident push table (include/hsqp_push.h): n_pushes [push_B] (int32, padded to 256 bytes), then pushes [push_B][push_max]; push_B == 0: no table
  DevBuf<char> d_push;
  int push_B = 0, push_max = 0;
  // the resident plant setting (include/hsqp_plant.h): kind FLOW = none; d_plant: kp, kd, armature [23] each
  hsqp_plant_settings plant = [] { hsqp_plant_settings p; hsqp_plant_defaults(&p); p.kind = HSQP_PLANT_FLOW; return p; }();
  DevBuf<double> d_plant;
  // the resident ground of the torque plant (include/hsqp_contact.h): enabled = 0 until hsqp_contact_set.  d_contact (contact_layout): the ground of every
  // instance [max_batch] — the first contact_B entries the per-instance table's, the rest the setting's values; contact_current: it holds that
  hsqp_contact_settings contact = {};
  DevBuf<char> d_contact, d_contact_stage;   // d_contact_stage: staging of hsqp_contact_eval's host arrays (contact_stage_layout)
  int contact_B = 0;
  bool contact_current = false;
  // the resident actuator model of the torque plant (include/hsqp_actuator.h): enabled = 0 until hsqp_actuator_set.  d_actuator (actuator_layout): the
  // setting's table, and the record of the last torques; actuator_last_B: the batch of the rollout the record is of (0: none since the setting was made)
  hsqp_actuator_settings actuator = [] { hsqp_actuator_settings a; hsqp_actuator_defaults(&a); a.enabled = 0; return a; }();
  DevBuf<char> d_actuator;
  int actuator_last_B = 0;
  // the resident inertial variations of the torque plant (include/hsqp_inertia.h).  d_inertia (inertia_layout): the entry of every instance [max_batch] — the
  // first inertia_B the table's, the rest neutral; inertia_B = 0: no table.  d_inertia_stage: staging of hsqp_inertia_eval's host arrays (inertia_stage_layout)
  DevBuf<char> d_inertia, d_inertia_stage;
  int inertia_B = 0;
  // the resident terrain under that ground (include/hsqp_terrain.h).  terrain_maps: the descriptors of the resident maps (empty: none), which d_terrain_maps
  // (terrain_maps_layout) holds with the heights.  d_terrain_place (terrain_place_layout): the placement of every instance [max_batch] — the first terrain_B the
  // table's, the rest map = -1; terrain_B = 0: no table; terrain_place_current: it holds that; terrain_top: the largest map index of a table that came as a host
  // array (-1: none, or a device array).  d_terrain_stage: staging of hsqp_terrain_eval's host arrays (terrain_stage_layout)
  std::vector<TerrainMap> terrain_maps;
  DevBuf<char> d_terrain_maps, d_terrain_place, d_terrain_stage;
  int terrain_B = 0, terrain_top = -1;
  bool terrain_place_current = false;
  // the resident observation model of the loop (include/hsqp_observe.h).  observe_set: hsqp_observe_set made settings; d_observe_table (observe_table_layout):
  // the entry of every instance [max_batch] — the first observe_B the table's, the rest neutral; observe_B = 0: no table.  d_observe (observe_layout): the
  // loop's ring and its two observation rows; d_observe_stage: staging of hsqp_observe_eval's host arrays (observe_stage_layout)
  hsqp_observe_settings observe = {};
  bool observe_set = false;
  int observe_B = 0;
  DevBuf<char> d_observe_table, d_observe, d_observe_stage;
  bool stamps_resident = false;   // d_stamps[stamps_cur] holds the raw stamps of the resident problem (it came through hsqp_upload_reference or the loop): the pushes' clock
  // raw time stamps of the resident grid (hsqp_reference::warm_start): two [max_batch][max_nodes + 1] buffers, d_stamps[stamps_cur] belongs to the
  // resident problem; a SHIFT upload reads it while it writes the other one.  have_stamps: the resident problem came through hsqp_upload_reference
  // with non-decreasing stamps
  DevBuf<double> d_stamps[2];
  int stamps_cur = 0;
  bool have_stamps = false;
  // the resident closed loop (include/hsqp_loop.h): settings, where it stands, and its arrays in d_loop (loop_layout)
  struct Loop {
    bool started = false, have_cycle = false;   // have_cycle: a cycle has completed since hsqp_loop_start (the next one shifts)
    hsqp_loop_settings st;
    int B = 0, E = 0;
    double t = 0.0;
    int* ne = nullptr; int* seq = nullptr; int* bad = nullptr; int32_t* ro_status = nullptr;
    double* ev = nullptr; double* tt = nullptr; double* ts = nullptr; double* s0 = nullptr;
    double* v_cmd = nullptr; double* v_filt = nullptr; double* x = nullptr; double* xs = nullptr; double* us = nullptr;
    bool gait = false;                          // started through hsqp_loop_start_gait: ne / seq / ev are written by k_gait_update in every cycle
    int cycle = 0;                              // cycles completed since hsqp_loop_start
    // failure isolation (include/hsqp_episode.h): off after every start; the episode arrays, x_reset [B][58], the command in use [B][4] and a reset request's staging in d_episode (episode_layout)
    bool isolate = false;
    hsqp_episode_settings ep_st;
    EpisodeState ep = {};
    double* x_reset = nullptr; double* v_use = nullptr;
    int* req_ids = nullptr; double* req_x0 = nullptr; double* req_v = nullptr;
    // episode metrics (include/hsqp_metrics.h): off after every start.  metrics: the kernel runs behind every rollout; metrics_made: the records exist since
    // the start (readable after a disable).  In d_metrics (metrics_layout): the records [B][2], the rollout's step counts, the feet's flags, a request's ids
    bool metrics = false, metrics_made = false;
    hsqp_metrics* met_rec = nullptr;
    int32_t* met_steps = nullptr; int32_t* met_rejected = nullptr;
    int* met_feet = nullptr; int* met_ids = nullptr;
    // the observation model (include/hsqp_observe.h): the ring [delay + 1][B][58] (null without a delay) and the observations of the even and the odd
    // cycles [B][58] in d_observe (observe_layout); obs_last: a cycle with the model in force has completed since the start, obs_tp its problem time
    double* obs_ring = nullptr; double* obs_y[2] = {nullptr, nullptr};
    bool obs_last = false;
    double obs_tp = 0.0;
    // the event-node grid (include/hsqp_grid.h): off after every start.  In d_grid (grid_layout): two records of (n_intervals [B], dt_nodes [B][N],
    // node_times [B][N + 1]) — a cycle builds into grid_rec[grid_cur ^ 1], which becomes grid_rec[grid_cur] when the cycle completes — the status words and
    // the one word the cycle reads back.  grid_have: grid_rec[grid_cur] is the grid of the last completed cycle
    bool grid = false, grid_have = false;
    hsqp_grid_settings grid_st = {};
    int grid_cur = 0;
    struct GridRec { int* ni; double* dts; double* nts; } grid_rec[2] = {};
    int* grid_status = nullptr; int* grid_bad = nullptr;
    // the ground-height estimate (include/hsqp_ground.h): off after every start.  In d_ground (ground_layout): the latch and its shadow, gnd_g[ground_cur] the
    // live one (a cycle writes the other, which becomes the live one at step 5), the contact-frame heights [B][2] likewise, g_init [B] and the terrain
    // height of step 2 [B]
    bool ground = false;
    hsqp_ground_settings ground_st = {};
    int ground_cur = 0;
    double* gnd_g[2] = {nullptr, nullptr}; double* gnd_fz[2] = {nullptr, nullptr};
    double* gnd_init = nullptr; double* gnd_terrain = nullptr;
    // the per-foot swing heights from the height map (include/hsqp_perceive.h): off after every start.  In d_perceive (perceive_layout): the rows a cycle
    // writes and step 2 reads — lift, touch [B][2][E + 1], footholds [B][2][E + 1][2]
    bool perceive = false;
    double* pcv_lift = nullptr; double* pcv_touch = nullptr; double* pcv_fxy = nullptr;
  } loop;
  // the resident gait state (include/hsqp_gait.h): two copies in d_gait (gait_layout), s[cur] the live one; ne / ev / seq: the cycle's schedule of the host entry point
  struct Gait {
    bool ready = false;
    hsqp_gait_settings st;
    int B = 0, cur = 0;
    hsqp_gait_settings* d_st = nullptr;
    GaitState s[2] = {};
    int* status = nullptr; int* ne = nullptr; int* seq = nullptr;
    double* ev = nullptr; double* v = nullptr; double* x = nullptr;
  } gait;
  DevBuf<char> d_gait, d_episode, d_metrics, d_grid, d_ground, d_perceive;
  DevBuf<char> d_perceive_stage;  // staging of hsqp_foot_heights' host arrays and of hsqp_upload_reference_heights' rows (perceive_stage_layout)
  DevBuf<char> d_ground_stage;    // staging of hsqp_ground_estimate's host arrays and of hsqp_upload_reference_ground's heights (ground_stage_layout)
  DevBuf<char> d_grid_stage;      // staging of hsqp_event_grid's host arrays (grid_stage_layout)
  DevBuf<char> d_loop, d_loop_log;   // the loop's resident arrays; staging of hsqp_loop_run's host logs and of hsqp_command_targets' host arrays
  double kernel_ms[5] = {0, 0, 0, 0, 0};
  int last_iterations = 0;
  struct IterLog { std::vector<hsqp_perf> perf; std::vector<double> alpha; std::vector<int> type; };
  std::vector<IterLog> iter_log;   // HSQP_ITER_UNTIL_CONVERGED: what every iteration of the last call ended with
  std::string err;
};

static std::string g_create_error;

// makes sure `buf` holds at least `bytes` (grow-only: a larger request replaces the buffer, the contents are not kept).  A new buffer starts as
// 0xFF bytes under HSQP_POISON_HBM.  On failure the buffer is empty and h->err names it.
template <class T>
static int dev_ensure(hsqp_handle* h, DevBuf<T>& buf, size_t bytes, const char* what) {
  if (buf.p && bytes <= buf.bytes) return HSQP_OK;
  if (buf.p) (void)hipFree(buf.p);
  buf.p = nullptr; buf.bytes = 0;
  if (hipMalloc(&buf.p, bytes) != hipSuccess) { buf.p = nullptr; h->err = std::string("hipMalloc failed (") + what + ", " + std::to_string(bytes) + " bytes)"; return HSQP_ERR_OOM; }
  if (h->poison_hbm) (void)hipMemset(buf.p, 0xFF, bytes);
  buf.bytes = bytes;
  return HSQP_OK;
}
#define DEV_ENSURE(buf, bytes, what) do { const int rc_ = dev_ensure(h, (buf), (bytes), (what)); if (rc_ != HSQP_OK) return rc_; } while (0)

// [max_batch][max_nodes + 1][VF_SIZE]: d_vf, d_vf2
static size_t vf_bytes(const hsqp_handle* h) { return (size_t)h->st.max_batch * (h->st.max_nodes + 1) * VF_SIZE * 8; }

#define HCHECK(call)                                                                                   \
  do {                                                                                                 \
    hipError_t e_ = (call);                                                                            \
    if (e_ != hipSuccess) {                                                                            \
      h->err = std::string(#call) + ": " + hipGetErrorString(e_);                                      \
      return HSQP_ERR_HIP;                                                                             \
    }                                                                                                  \
  } while (0)

// ---- the layouts of the handle's carved buffers (hsqp_carve.h).  Each states its buffer's regions once, in order, and tells the bytes they take; a
// caller runs it on a sizing cursor (Carve{}: null pointers, the bytes go to DEV_ENSURE) and again on the buffer.
// d_stage, hsqp_upload_reference: the compact reference (a few KB per instance)
struct RefStage { int* ne; int* seq; int* bad; double* ev; double* tt; double* ts; double* nt; size_t bytes; };
static RefStage ref_stage_layout(Carve c, size_t B, size_t N, size_t E, size_t K, bool node_times) {
  return {c.take<int>(B), c.take<int>(B * (E + 1)), c.take<int>(1), c.take<double>(B * E), c.take<double>(B * K), c.take<double>(B * K * NX),
          c.take<double>(B * (N + 1), node_times), c.bytes()};
}
// d_stage, run_policy: nin input doubles, then x, u, tau of n queries and the whole-body (x, u) of a centroidal handle's
struct PolicyStage { double* in; double* x; double* u; double* tau; double* xw; double* uw; size_t bytes; };
static PolicyStage policy_stage_layout(Carve c, size_t n, size_t nin) {
  return {c.take<double>(nin), c.take<double>(n * NX), c.take<double>(n * NU), c.take<double>(n * NJ), c.take<double>(n * NX), c.take<double>(n * NU), c.bytes()};
}
// d_ro, rollout_impl: window [3] | status, steps, rejected [B] each, one region | (host entry point) s0 [B], x0 [B][58], x [B][n][58], u [B][n][35]
struct RolloutStage { int* win; int32_t* status; int32_t* steps; int32_t* rejected; double* s0; double* x0; double* x; double* u; size_t bytes; };
static RolloutStage rollout_stage_layout(Carve c, size_t B, size_t n, bool host, bool want_x, bool want_u) {
  int* win = c.take<int>(3);
  int32_t* cnt = c.take<int32_t>(3 * B);
  return {win, cnt, cnt ? cnt + B : nullptr, cnt ? cnt + 2 * B : nullptr, c.take<double>(B, host), c.take<double>(B * NX, host),
          c.take<double>(B * n * NX, host && want_x), c.take<double>(B * n * NU, host && want_u), c.bytes()};
}
// d_loop_log, hsqp_command_targets (host arrays)
struct CommandStage { double* v_cmd; double* v_filt; double* x0; double* tt; double* ts; double* base_vel; size_t bytes; };
static CommandStage command_stage_layout(Carve c, size_t B, bool base_vel = false) {   // base_vel [B][6]: the centroidal generator's by-product (hsqp_cent_loop.h)
  CommandStage sg{c.take<double>(B * CMD_N), c.take<double>(B * CMD_N), c.take<double>(B * NX), c.take<double>(B * CMD_KNOTS), c.take<double>(B * CMD_KNOTS * NX), nullptr, 0};
  if (base_vel) sg.base_vel = c.take<double>(B * 6);
  sg.bytes = c.bytes();
  return sg;
}
// d_loop: the loop's resident arrays
static size_t loop_layout(Carve c, hsqp_handle::Loop& L, size_t B, size_t E) {
  L.ne = c.take<int>(B); L.seq = c.take<int>(B * (E + 1)); L.bad = c.take<int>(1); L.ro_status = c.take<int32_t>(B); L.ev = c.take<double>(B * E);
  L.tt = c.take<double>(B * CMD_KNOTS); L.ts = c.take<double>(B * CMD_KNOTS * NX); L.s0 = c.take<double>(B); L.v_cmd = c.take<double>(B * CMD_N);
  L.v_filt = c.take<double>(2 * B * CMD_N); L.x = c.take<double>(B * NX); L.xs = c.take<double>(B * NX); L.us = c.take<double>(B * NU);
  return c.bytes();
}
// d_gait: the settings, the status words, the host entry point's schedule and inputs, the two copies of the state
static size_t gait_layout(Carve c, hsqp_handle::Gait& G, size_t B, size_t E) {
  G.d_st = c.take<hsqp_gait_settings>(1); G.status = c.take<int>(B); G.ne = c.take<int>(B); G.seq = c.take<int>(B * (E + 1)); G.ev = c.take<double>(B * E);
  G.v = c.take<double>(B * CMD_N); G.x = c.take<double>(B * NX);
  for (GaitState& s : G.s) s = GaitState{c.take<int>(B), c.take<double>(B * E), c.take<int>(B * (E + 1)), c.take<int>(B * GAIT_SCAL), c.take<double>(B)};
  return c.bytes();
}
// d_episode: the episode arrays, x_reset, the command in use, the staging of a hsqp_loop_reset_instances request
static size_t episode_layout(Carve c, hsqp_handle::Loop& L, size_t B) {
  L.ep = EpisodeState{c.take<int>(B), c.take<int>(B), c.take<int>(B), c.take<int>(B), c.take<int>(B), c.take<int>(B), c.take<int>(B)};
  L.x_reset = c.take<double>(B * NX); L.v_use = c.take<double>(B * CMD_N);
  L.req_ids = c.take<int>(B); L.req_x0 = c.take<double>(B * NX); L.req_v = c.take<double>(B * CMD_N);
  return c.bytes();
}
// d_metrics: the records [B][2] (CURRENT, PREVIOUS), the step counts of the cycle's rollout, the feet's flags [B][2], the ids of a restart request
static size_t metrics_layout(Carve c, hsqp_handle::Loop& L, size_t B) {
  L.met_rec = c.take<hsqp_metrics>(2 * B); L.met_steps = c.take<int32_t>(B); L.met_rejected = c.take<int32_t>(B);
  L.met_feet = c.take<int>(2 * B); L.met_ids = c.take<int>(B);
  return c.bytes();
}
// d_grid: the loop's two grid records, the status words of a cycle's build, the word the cycle reads back
static size_t grid_layout(Carve c, hsqp_handle::Loop& L, size_t B, size_t N) {
  for (auto& r : L.grid_rec) r = {c.take<int>(B), c.take<double>(B * N), c.take<double>(B * (N + 1))};
  L.grid_status = c.take<int>(B); L.grid_bad = c.take<int>(1);
  return c.bytes();
}
// d_grid_stage, hsqp_event_grid (host arrays): n_events [B], event_times [B][E] | n_intervals [B], status [B], dt_nodes [B][N], node_times [B][N + 1]
struct GridStage { int* ne; int* ni; int* status; double* ev; double* dts; double* nts; size_t bytes; };
static GridStage grid_stage_layout(Carve c, size_t B, size_t N, size_t E, bool host) {
  return {c.take<int>(B, host), c.take<int>(B, host), c.take<int>(B), c.take<double>(B * E, host), c.take<double>(B * N, host), c.take<double>(B * (N + 1), host), c.bytes()};
}
// d_ground: the loop's latch and its shadow, the contact-frame heights of the two, g_init, the terrain height of step 2
static size_t ground_layout(Carve c, hsqp_handle::Loop& L, size_t B) {
  for (int i = 0; i < 2; ++i) { L.gnd_g[i] = c.take<double>(B); L.gnd_fz[i] = c.take<double>(2 * B); }
  L.gnd_init = c.take<double>(B); L.gnd_terrain = c.take<double>(B);
  return c.bytes();
}
// d_ground_stage.  hsqp_ground_estimate (host arrays): n_events [B], mode_sequence [B][E + 1], x [B][58], event_times [B][E], g [B], foot_z [B][2];
// hsqp_upload_reference_ground: terrain_heights [B] alone
struct GroundStage { int* ne; int* seq; double* x; double* ev; double* g; double* fz; double* terrain; size_t bytes; };
static GroundStage ground_stage_layout(Carve c, size_t B, size_t E, bool estimate) {
  return {c.take<int>(B, estimate), c.take<int>(B * (E + 1), estimate), c.take<double>(B * NX, estimate), c.take<double>(B * E, estimate), c.take<double>(B, estimate),
          c.take<double>(2 * B, estimate), c.take<double>(B, !estimate), c.bytes()};
}
// d_perceive: the loop's rows of the per-foot swing heights
static size_t perceive_layout(Carve c, hsqp_handle::Loop& L, size_t B, size_t E) {
  L.pcv_lift = c.take<double>(B * 2 * (E + 1)); L.pcv_touch = c.take<double>(B * 2 * (E + 1)); L.pcv_fxy = c.take<double>(B * 4 * (E + 1));
  return c.bytes();
}
// d_perceive_stage.  The rows lift, touch [B][2][E + 1] and footholds [B][2][E + 1][2] (hsqp_upload_reference_heights: the two rows alone; the _device
// entry of hsqp_foot_heights without foothold_xy: the footholds alone); hsqp_foot_heights (host arrays) behind them: n_events [B], mode_sequence
// [B][E + 1], x [B][58], event_times [B][E], target_times [B][K], target_states [B][K][58]
struct PerceiveStage { double* lift; double* touch; double* fxy; int* ne; int* seq; double* x; double* ev; double* tt; double* ts; size_t bytes; };
static PerceiveStage perceive_stage_layout(Carve c, size_t B, size_t E, size_t K, bool inputs) {
  return {c.take<double>(B * 2 * (E + 1)), c.take<double>(B * 2 * (E + 1)), c.take<double>(B * 4 * (E + 1)), c.take<int>(B, inputs), c.take<int>(B * (E + 1), inputs),
          c.take<double>(B * NX, inputs), c.take<double>(B * E, inputs), c.take<double>(B * K, inputs), c.take<double>(B * K * NX, inputs), c.bytes()};
}
// d_observe: the loop's ring of plant states (absent without a delay) and the observations of the even and the odd cycles
static size_t observe_layout(Carve c, hsqp_handle::Loop& L, size_t B, size_t slots) {
  L.obs_ring = c.take<double>(slots * B * NX, slots > 1); L.obs_y[0] = c.take<double>(B * NX); L.obs_y[1] = c.take<double>(B * NX);
  return c.bytes();
}
// d_observe_table: the observation entry of every instance [max_batch]
struct ObserveBuf { hsqp_observe_instance* table; size_t bytes; };
static ObserveBuf observe_table_layout(Carve c, size_t max_batch) { return {c.take<hsqp_observe_instance>(max_batch), c.bytes()}; }
// d_observe_stage, hsqp_observe_eval (host arrays): x [B][58] | y [B][58]
struct ObserveStage { double* x; double* y; size_t bytes; };
static ObserveStage observe_stage_layout(Carve c, size_t B) { return {c.take<double>(B * NX), c.take<double>(B * NX), c.bytes()}; }
// d_push: n_pushes [B], then pushes [B][max_pushes]
struct PushBuf { int32_t* n; hsqp_push* p; size_t bytes; };
static PushBuf push_layout(Carve c, size_t B, size_t max_pushes) { return {c.take<int32_t>(B), c.take<hsqp_push>(B * max_pushes), c.bytes()}; }
// d_contact: the ground of every instance [max_batch]
struct ContactBuf { hsqp_contact_ground* ground; size_t bytes; };
static ContactBuf contact_layout(Carve c, size_t max_batch) { return {c.take<hsqp_contact_ground>(max_batch), c.bytes()}; }
// d_actuator: effort_limit | damping | friction [NJ] each (one array: ActuatorParams::table), then the record tau_cmd | tau_act | tau_pas [NJ] each of every instance
struct ActuatorBuf { double* table; double* last; size_t bytes; };
static ActuatorBuf actuator_layout(Carve c, size_t max_batch) { return {c.take<double>(3 * NJ), c.take<double>(max_batch * 3 * NJ), c.bytes()}; }
// d_inertia: the inertial variation of every instance [max_batch]
struct InertiaBuf { hsqp_inertia_instance* table; size_t bytes; };
static InertiaBuf inertia_layout(Carve c, size_t max_batch) { return {c.take<hsqp_inertia_instance>(max_batch), c.bytes()}; }
// d_terrain_maps: the descriptors [HSQP_TERRAIN_MAX_MAPS] | the heights of all maps, concatenated
struct TerrainMapsBuf { TerrainMap* maps; double* pool; size_t bytes; };
static TerrainMapsBuf terrain_maps_layout(Carve c, size_t heights) { return {c.take<TerrainMap>(HSQP_TERRAIN_MAX_MAPS), c.take<double>(heights), c.bytes()}; }
// d_terrain_place: the placement of every instance [max_batch]
struct TerrainPlaceBuf { hsqp_terrain_placement* place; size_t bytes; };
static TerrainPlaceBuf terrain_place_layout(Carve c, size_t max_batch) { return {c.take<hsqp_terrain_placement>(max_batch), c.bytes()}; }
// d_terrain_stage, hsqp_terrain_eval (host arrays): xy [B][n][2] | height [B][n] | normal [B][n][3]
struct TerrainStage { double* xy; double* height; double* normal; size_t bytes; };
static TerrainStage terrain_stage_layout(Carve c, size_t pts, bool want_height, bool want_normal) {
  return {c.take<double>(pts * 2), c.take<double>(pts, want_height), c.take<double>(pts * 3, want_normal), c.bytes()};
}
// d_inertia_stage, hsqp_inertia_eval (host arrays): x [B][58] | M [B][29][29] | nle [B][29] | mass [B]
struct InertiaStage { double* x; double* M; double* nle; double* mass; size_t bytes; };
static InertiaStage inertia_stage_layout(Carve c, size_t B, bool want_M, bool want_nle, bool want_mass) {
  return {c.take<double>(B * NX), c.take<double>(B * NV * NV, want_M), c.take<double>(B * NV, want_nle), c.take<double>(B, want_mass), c.bytes()};
}
// d_contact_stage, hsqp_contact_eval (host arrays): x [B][58] | force [B][8][3] | penetration [B][8]
struct ContactStage { double* x; double* force; double* pen; size_t bytes; };
static ContactStage contact_stage_layout(Carve c, size_t B, bool want_force, bool want_pen) {
  return {c.take<double>(B * NX), c.take<double>(B * CT_PTS * 3, want_force), c.take<double>(B * CT_PTS, want_pen), c.bytes()};
}
// d_plant: kp | kd | armature, [NJ] each, which PlantParams::gains reads as one array (own packing, not Carve::take: plant_pack_gains, hsqp_plant.h)
// d_loop_log, hsqp_loop_run's host logs: x_log [n][B][58] | u_log [n][B][35], the cycles' rows as one array each (own packing, not Carve::take); a null block: the sizing pass
struct LoopLog { double* x; double* u; size_t bytes; };
static LoopLog loop_log_layout(double* block, size_t n, size_t B, bool want_x, bool want_u) {
  const size_t nx = want_x ? n * B * NX : 0, nu = want_u ? n * B * NU : 0;
  return {block && want_x ? block : nullptr, block && want_u ? block + nx : nullptr, (nx + nu) * 8};
}

// (the KKT gate of the parallel-in-time sweep: scan_gate_accepts, hsqp_scan.h)
// Refinement passes of the gains (one more stage of the exact Riccati map from the value functions of the previous pass).  Centroidal: one
// pass gains a digit (1e-11 -> 1e-12 of the step's scale).  Whole-body: none — the closed loop of that problem has slow modes (positions
// integrate velocities over dt = 0.02), so the map barely contracts an error in S: 0, 1, 2 or 3 passes all leave 1.4e-11 .. 8e-11
// (tests/hostemu probe, N = 16 .. 100), and each costs 24 us.
constexpr int HSQP_SCAN_WB_REFINEMENTS = 0;
// parallel-in-time backward sweep (hsqp_scan.h): elements of all stages, ceil(log2(N+1)) scan levels, single-stage gains (from the
// scanned value functions, then `refinements` times from the value functions of the previous gains pass), closed-loop roll-out
template <int n>
static int launch_scan(hsqp_handle* h, int B, int N, bool want_kkt, int refinements) {
  constexpr int SZ = ScanEl<n>::SIZE;
  const int nodes = B * N;
  for (auto& el : h->d_el) DEV_ENSURE(el, (size_t)B * (N + 1) * SZ * 8, "scan elements");
  HSQP_LAUNCH(k_scan_init<n>, dim3(B * (N + 1)), dim3(SCAN_INIT_THREADS), sizeof(ScanInitWS<n>), h->stream, h->d_dm, h->d_x, h->d_par, h->d_qp, N, h->d_el[0], h->gate.flags);
  int cur = 0;
  for (int d = 1; d < N + 1; d *= 2) {
    HSQP_LAUNCH(k_scan_combine<n>, dim3(B * (N + 1)), dim3(SCAN_COMB_THREADS), sizeof(ScanCombWS<n>), h->stream, h->d_el[cur], h->d_el[1 - cur], N, d, h->gate.flags, h->d_prof + 256);
    cur = 1 - cur;
  }
  DEV_ENSURE(h->d_vf, vf_bytes(h), "value functions");
  DEV_ENSURE(h->d_vf2, vf_bytes(h), "value functions of the gated sweep");
  DEV_ENSURE(h->d_acl, (size_t)h->st.max_batch * h->st.max_nodes * ACL_SIZE<n> * 8, "closed loop of the scan path");
  // the gains passes ping-pong between the two value-function buffers; the LAST pass writes d_vf2 (what the KKT check reads) and the closed loop
  double* vbuf[2] = {(refinements & 1) ? h->d_vf : h->d_vf2, (refinements & 1) ? h->d_vf2 : h->d_vf};
  for (int pass = 0; pass <= refinements; ++pass) {
    const bool lastp = pass == refinements;
    HSQP_LAUNCH(k_scan_gains<n>, dim3(nodes), dim3(RIC_THREADS), sizeof(RicWS), h->stream, h->d_dm, h->d_x, h->d_par, h->d_qp, h->d_el[cur],
                       pass == 0 ? (const double*)nullptr : (const double*)vbuf[(pass - 1) & 1], h->d_ric, N, h->gate.flags,
                       (lastp && !want_kkt) ? (double*)nullptr : vbuf[pass & 1], lastp ? h->d_acl : (double*)nullptr);
  }
  HSQP_LAUNCH(k_scan_forward<n>, dim3(B), dim3(SCAN_FWD_THREADS), sizeof(RicWS), h->stream, h->d_xinit, h->d_x, h->d_acl, N, h->d_dx);   // 4 n <= 256 items per stage: four waves
  return HSQP_OK;
}

// segment count of the two-level sweep for B instances on N intervals (0: not applicable).  OPT-IN (HSQP_FLAG_SEGMENTED_RICCATI): measured on
// perturbed config-4 batches of 32 (tools/gpu_seg_fuzz.py) its step is 4e-11 .. 4e-10 of the step's scale (up to 7e-8 absolute) from the serial
// recursion's — the combination of two long-segment elements solves with cond(I + C1 J2) ~ 1e9 — which is outside BASELINE.md §6's 1e-8 on
// trajectories, so the default path never takes it; a caller that accepts the declared error asks for it.  P + 1 elements per instance go
// through the suffix scan: P + 1 a power of two wastes no level, B (P + 1) <= 256 workgroups run a level in one round, and every level costs
// accuracy, hence P <= 7 (B = 32: P = 7, three levels of 256 workgroups).
static int segment_count(const hsqp_handle* h, int B, int N) {
  if (!(h->st.flags & HSQP_FLAG_SEGMENTED_RICCATI)) return 0;
  const int cap = std::min(std::min(256 / std::max(B, 1) - 1, N / 4), 7);
  if (cap < 1) return 0;
  int e = 2;
  while (2 * e <= cap + 1) e *= 2;
  return e - 1 >= 3 ? e - 1 : 0;   // 3 or 7 segments; fewer do not pay
}

// two-level sweep (hsqp_segment.h): segment elements, suffix scan over them, gains per segment, roll-out
template <int n>
static int launch_segmented(hsqp_handle* h, int B, int N, int P, bool want_vf) {
  constexpr int SZ = ScanEl<n>::SIZE;
  for (auto& el : h->d_el) DEV_ENSURE(el, (size_t)B * (P + 1) * SZ * 8, "segment elements");
  const size_t BN = (size_t)h->st.max_batch * h->st.max_nodes;
  DEV_ENSURE(h->d_ric2, BN * RIC_SIZE * 8, "segmented sweep: gains");
  DEV_ENSURE(h->d_linv, BN * LDB * LDB * 8, "segmented sweep: factors");
  if (!h->d_zero) {
    DEV_ENSURE(h->d_zero, (NX * NX + NX) * 8, "segmented sweep: zeros");
    if (hipMemsetAsync(h->d_zero, 0, (NX * NX + NX) * 8, h->stream) != hipSuccess) { h->err = "memset failed"; return HSQP_ERR_HIP; }
  }
  DEV_ENSURE(h->d_vf0, (size_t)B * P * VF_SIZE * 8, "segmented sweep: boundary value functions");
  // (the gate needs the value functions of the boundary stages' nodes; want_vf: of every node, for the KKT report)
  DEV_ENSURE(h->d_vf2, vf_bytes(h), "value functions of the gated sweep");
  const int segs = B * P;
  HSQP_LAUNCH(k_seg_elem_ric<n>, dim3(segs), dim3(RIC_THREADS), sizeof(RicWS), h->stream, h->d_dm, h->d_x, h->d_par, h->d_qp, (const double*)h->d_zero, h->d_ric2,
                     h->d_linv, h->d_vf0, N, P, h->gate.flags);
  HSQP_LAUNCH(k_seg_accumulate<n>, dim3(segs), dim3(SEG_ACC_THREADS), sizeof(SegAccWS), h->stream, (const double*)h->d_qp, (const double*)h->d_ric2,
                     (const double*)h->d_linv, (const double*)h->d_vf0, N, P, h->d_el[0]);
  HSQP_LAUNCH(k_seg_terminal<n>, dim3(B), dim3(256), 0, h->stream, h->d_dm, h->d_x, h->d_par, N, P, h->d_el[0]);
  int cur = 0;
  for (int d = 1; d < P + 1; d *= 2) {
    HSQP_LAUNCH(k_scan_combine<n>, dim3(B * (P + 1)), dim3(SCAN_COMB_THREADS), sizeof(ScanCombWS<n>), h->stream, h->d_el[cur], h->d_el[1 - cur], P, d, h->gate.flags,
                       (long long*)nullptr);
    cur = 1 - cur;
  }
  HSQP_LAUNCH(k_seg_riccati<n>, dim3(segs), dim3(RIC_THREADS), sizeof(RicWS), h->stream, h->d_dm, h->d_x, h->d_par, h->d_qp, (const double*)h->d_el[cur], h->d_ric, N, P,
                     h->gate.flags, h->d_vf2, want_vf ? 0 : 2);
  HSQP_LAUNCH(k_ric_forward<n>, dim3(B), dim3(RIC_THREADS), sizeof(RicWS), h->stream, h->d_xinit, h->d_x, h->d_qp, (const double*)h->d_ric, N, h->d_dx, h->d_ut);
  return HSQP_OK;
}

extern "C" {

const char* hsqp_version(void) { return "hsqp-hip 0.3 (gfx950, f64, abi 7)"; }
int hsqp_abi_version(void) { return HSQP_ABI_VERSION; }
int hsqp_set_scan_backoff_persistent(hsqp_handle* h, int on) {
  if (!h) return HSQP_ERR_BAD_ARG;
  h->backoff_persistent = on != 0;
  return HSQP_OK;
}

int hsqp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

long long hsqp_scan_fallbacks(const hsqp_handle* h) { return h ? h->scan_fallbacks : -1; }
long long hsqp_scan_backoffs(const hsqp_handle* h) { return h ? h->backoff_iterations : -1; }

const char* hsqp_last_error(const hsqp_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

void hsqp_destroy(hsqp_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->h_gate) (void)hipHostFree(h->h_gate);
  for (auto& e : h->ev)
    if (e) (void)hipEventDestroy(e);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  for (auto& e : h->ev_join)
    if (e) (void)hipEventDestroy(e);
  for (auto& st : h->aux)
    if (st) (void)hipStreamDestroy(st);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;   // (the device buffers free themselves: DevBuf)
}

void hsqp_linesearch_defaults(hsqp_linesearch_settings* s) {
  if (!s) return;
  s->g_max = 1e-2; s->g_min = 1e-6;      // g1_wb_mpc/config/mpc/task.info:83-84
  s->gamma_c = 1e-6; s->armijo_factor = 1e-4; s->alpha_decay = 0.5; s->alpha_min = 1e-4;   // upstream ocs2 sqp::Settings defaults
  s->delta_tol = 1e-4;                   // task.info deltaTol
  s->cost_tol = 1e-4;                    // upstream ocs2 sqp::Settings::costTol default (the task file does not set it)
}

// trials after which every instance has either accepted a step or fallen below alpha_min (zero step)
static int ls_max_trials(const hsqp_linesearch_settings& s) { return (int)ceil(log(s.alpha_min) / log(s.alpha_decay)) + 2; }
#define HSQP_LS_MAX_TRIALS 4096

int hsqp_set_linesearch(hsqp_handle* h, const hsqp_linesearch_settings* s) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (!s || !(s->alpha_decay > 0.0 && s->alpha_decay < 1.0) || !(s->alpha_min > 0.0) || !(s->g_max >= s->g_min) || !(s->cost_tol >= 0.0)) {
    h->err = "line-search settings: need 0 < alpha_decay < 1, alpha_min > 0, g_max >= g_min, cost_tol >= 0";
    return HSQP_ERR_BAD_ARG;
  }
  if (s->alpha_min < 1.0 && ls_max_trials(*s) > HSQP_LS_MAX_TRIALS) {
    h->err = "line-search settings: more than 4096 back-tracking trials (alpha_decay too close to 1 for this alpha_min)";
    return HSQP_ERR_BAD_ARG;
  }
  h->ls_settings = *s;
  return HSQP_OK;
}

int hsqp_create(const hsqp_model_desc* model, const hsqp_settings* settings, hsqp_handle** out) {
  if (!model || !settings || !out) { g_create_error = "null argument"; return HSQP_ERR_BAD_ARG; }
  *out = nullptr;
  if (settings->max_nodes < 1 || settings->max_batch < 1) { g_create_error = "max_nodes and max_batch must be >= 1"; return HSQP_ERR_BAD_ARG; }
  if ((settings->flags & HSQP_FLAG_PARALLEL_RICCATI) && (settings->flags & HSQP_FLAG_SERIAL_RICCATI)) {
    g_create_error = "HSQP_FLAG_PARALLEL_RICCATI excludes HSQP_FLAG_SERIAL_RICCATI";
    return HSQP_ERR_BAD_ARG;
  }
  if ((settings->flags & HSQP_FLAG_SEGMENTED_RICCATI) && (settings->flags & (HSQP_FLAG_PARALLEL_RICCATI | HSQP_FLAG_SERIAL_RICCATI))) {
    g_create_error = "HSQP_FLAG_SEGMENTED_RICCATI excludes HSQP_FLAG_PARALLEL_RICCATI and HSQP_FLAG_SERIAL_RICCATI";
    return HSQP_ERR_BAD_ARG;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_error = "no HIP device visible (this library has no CPU path)"; return HSQP_ERR_NO_DEVICE; }
  if (settings->device < 0 || settings->device >= ndev) { g_create_error = "device ordinal out of range"; return HSQP_ERR_BAD_ARG; }
  hsqp_handle* h = new hsqp_handle;
  h->seg_debug = getenv("HSQP_SEG_DEBUG") != nullptr;
  h->poison_lds = getenv("HSQP_POISON_LDS") != nullptr;
  h->poison_hbm = getenv("HSQP_POISON_HBM") != nullptr;
  h->ric_fact = model->formulation == HSQP_FORM_WB && getenv("HSQP_RICCATI_DENSE") == nullptr;
  h->md = *model;
  h->st = *settings;
  h->device = settings->device;
  hsqp_linesearch_defaults(&h->ls_settings);
  const std::string e = build_dev_model(*model, h->hdm);
  if (!e.empty()) { g_create_error = e; delete h; return HSQP_ERR_BAD_ARG; }
  hsqp_contact_defaults(h, &h->contact);   // (the model's friction_mu)
  h->contact.enabled = 0;
  // the value pass on quads of lanes (hsqp_lqv.h) is a throughput form: a wave evaluates 16 nodes in ~100 us whatever their number, the phase form one node
  // in ~40 us — so a handle sized for fewer nodes than fill the GPU once (config 3: one instance, 100 nodes) keeps the phase form.  Decided per HANDLE, not
  // per call: every solve of a handle runs the same arithmetic (an instance of a batch equals its solo solve bit for bit)
  h->value_quad = h->hdm.formulation == HSQP_FORM_WB && h->hdm.n_limbs > 0 && getenv("HSQP_VALUE_PHASE_FORM") == nullptr &&
                  (getenv("HSQP_VALUE_QUAD_FORM") != nullptr || (size_t)settings->max_batch * settings->max_nodes >= VALUE_QUAD_MIN_NODES);
  // the LQ approximation on limb lanes (hsqp_lql.h) is a throughput form like the quad value pass; same rule, same per-handle decision
  h->lq_limb = h->hdm.formulation == HSQP_FORM_WB && h->hdm.ql_ok && getenv("HSQP_LQ_PHASE_FORM") == nullptr &&
               (getenv("HSQP_LQ_LIMB_FORM") != nullptr || (size_t)settings->max_batch * settings->max_nodes >= LQ_LIMB_MIN_NODES);
  h->chain_fused = h->lq_limb && getenv("HSQP_LQ_CHAIN_SEPARATE") == nullptr;
  auto fail = [&](int code, const std::string& msg) { g_create_error = msg; hsqp_destroy(h); return code; };
  if (hipSetDevice(h->device) != hipSuccess) return fail(HSQP_ERR_HIP, "hipSetDevice failed");
  if (hipStreamCreate(&h->stream) != hipSuccess) return fail(HSQP_ERR_HIP, "hipStreamCreate failed");
  for (auto& ev : h->ev)
    if (hipEventCreate(&ev) != hipSuccess) return fail(HSQP_ERR_HIP, "hipEventCreate failed");
  if (h->lq_limb) {
    const char* sp = getenv("HSQP_LQ_SPLIT");
    h->lq_split = LQ_SPLIT_DEFAULT;
    if (sp) {
      char* end = nullptr;
      const long v = strtol(sp, &end, 10);
      if (end == sp || *end != '\0' || v < 1 || v > hsqp_handle::LQ_SPLIT_MAX)
        return fail(HSQP_ERR_BAD_ARG, std::string("HSQP_LQ_SPLIT=\"") + sp + "\": expected an integer in [1, " + std::to_string(hsqp_handle::LQ_SPLIT_MAX) + "]");
      h->lq_split = (int)v;
    }
    // one round of the chip = the workgroups of the two one-wave-per-SIMD kernels it holds at once: asked of the runtime for the kernels as built
    // (QL_WPE / QR_WPE), not assumed from the CU count
    int cus = 0, per_cu_limb = 0, per_cu_rows = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device) == hipSuccess && cus > 0 &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_limb, (const void*)k_lq_limb, QL_THREADS * QL_WAVES, 0) == hipSuccess &&
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu_rows, (const void*)k_lq_rows, QL_THREADS * QL_WAVES, 0) == hipSuccess &&
        per_cu_limb > 0 && per_cu_rows > 0)
      h->lq_round_blocks = cus * std::min(per_cu_limb, per_cu_rows);
    else if (cus > 0) h->lq_round_blocks = cus * 4 / QL_WAVES;
    if (h->lq_split > hsqp_handle::LQ_SPLIT_MAX) h->lq_split = hsqp_handle::LQ_SPLIT_MAX;
    if (h->lq_split > 1 && hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess) return fail(HSQP_ERR_HIP, "hipEventCreate failed");
    for (int s = 0; s + 1 < h->lq_split; ++s)
      if (hipStreamCreateWithFlags(&h->aux[s], hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&h->ev_join[s], hipEventDisableTiming) != hipSuccess)
        return fail(HSQP_ERR_HIP, "hipStreamCreate failed");
  }
  const size_t B = settings->max_batch, N = settings->max_nodes;
  int rc = HSQP_OK;
  auto alloc = [&](auto& buf, size_t bytes, const char* what) { if (rc == HSQP_OK) rc = dev_ensure(h, buf, bytes, what); };
  alloc(h->d_dm, sizeof(DevModel), "model"); alloc(h->d_xinit, B * NX * 8, "x_init"); alloc(h->d_x, B * (N + 1) * NX * 8, "x"); alloc(h->d_u, B * N * NU * 8, "u");
  alloc(h->d_par, B * (N + 1) * NP * 8, "node parameters"); alloc(h->d_rec, B * N * (size_t)REC_SIZE * 8, "LQ record");
  alloc(h->d_qp, B * N * (size_t)QP_SIZE * 8, "QP record"); alloc(h->d_ric, B * N * (size_t)RIC_SIZE * 8, "gains"); alloc(h->d_dx, B * (N + 1) * NX * 8, "dx");
  alloc(h->d_du, B * N * NU * 8, "du"); alloc(h->d_ut, B * N * NUT * 8, "ut"); alloc(h->d_fj, B * N * NJ * 8, "joint rows of the roll-out");
  alloc(h->d_xnew, B * (N + 1) * NX * 8, "x_new"); alloc(h->d_unew, B * N * NU * 8, "u_new"); alloc(h->d_misc, B * N * 8 * 8, "value-pass terms");
  alloc(h->d_kkt, gate_view(nullptr, B).bytes, "gate block"); alloc(h->d_dt, B * N * 8, "interval lengths"); alloc(h->d_perf_before, B * sizeof(hsqp_perf), "perf_before");
  alloc(h->d_perf_after, B * sizeof(hsqp_perf), "perf_after"); alloc(h->d_status, B * sizeof(int), "status"); alloc(h->d_prof, 4 * 128 * sizeof(long long), "phase profile");
  alloc(h->d_stepinfo, B * N * 4 * 8, "step terms"); alloc(h->d_ls, B * sizeof(LsState), "line-search state"); alloc(h->d_counts, 2 * sizeof(int), "line-search counters");
  alloc(h->d_stamps[0], B * (N + 1) * 8, "time stamps"); alloc(h->d_stamps[1], B * (N + 1) * 8, "time stamps");
  if (rc != HSQP_OK) return fail(rc, h->err);
  if (hipHostMalloc((void**)&h->h_gate, gate_view(nullptr, B).bytes) != hipSuccess) { h->h_gate = nullptr; return fail(HSQP_ERR_OOM, "hipHostMalloc failed (gate block)"); }
  h->gate = gate_view(h->d_kkt, B);
  if (hipMemcpy(h->d_dm, &h->hdm, sizeof(DevModel), hipMemcpyHostToDevice) != hipSuccess) return fail(HSQP_ERR_HIP, "model upload failed");
  if (hipMemset(h->d_prof, 0, 4 * 128 * sizeof(long long)) != hipSuccess) return fail(HSQP_ERR_HIP, "memset failed");
  // the limb-lane LQ kernel never writes record entries that are zero for every state (hsqp_lql.h)
  if (hipMemset(h->d_rec, 0, B * N * (size_t)REC_SIZE * 8) != hipSuccess) return fail(HSQP_ERR_HIP, "memset failed");
  if (h->poison_lds) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) h->poison_blocks = 2 * prop.multiProcessorCount;
  }
  // the kernels use up to ~158 KB of dynamic LDS (gfx950: 160 KB per workgroup)
  const struct { const void* f; int bytes; } lds_limits[] = {
      {(const void*)k_lq<true>, (int)sizeof(LqWS)},
      {h->poison_lds ? (const void*)k_poison_lds : nullptr, POISON_LDS_BYTES},
      {(const void*)k_lq<false>, (int)sizeof(LqWST<false>)}, {(const void*)k_step_value, (int)sizeof(LqWST<false>)},
      {(const void*)k_lq_cent2, (int)sizeof(CentWST<true>)}, {(const void*)k_command_targets_cent, (int)sizeof(CentWST<false>)},
      {(const void*)k_project, (int)sizeof(ProjWS)},
      {(const void*)k_riccati<NX>, (int)sizeof(RicWS)}, {(const void*)k_riccati_fact, (int)sizeof(RicFWS)}, {(const void*)k_riccati<CNX>, (int)sizeof(RicWS)},
      {(const void*)k_scan_init<CNX>, (int)sizeof(ScanInitWS<CNX>)}, {(const void*)k_scan_combine<CNX>, (int)sizeof(ScanCombWS<CNX>)},
      {(const void*)k_scan_gains<CNX>, (int)sizeof(RicWS)}, {(const void*)k_scan_forward<CNX>, (int)sizeof(RicWS)},
      {(const void*)k_scan_init<NX>, (int)sizeof(ScanInitWS<NX>)}, {(const void*)k_scan_combine<NX>, (int)sizeof(ScanCombWS<NX>)},
      {(const void*)k_scan_gains<NX>, (int)sizeof(RicWS)}, {(const void*)k_scan_forward<NX>, (int)sizeof(RicWS)},
      {(const void*)k_seg_elem_ric<NX>, (int)sizeof(RicWS)}, {(const void*)k_seg_elem_ric<CNX>, (int)sizeof(RicWS)},
      {(const void*)k_seg_riccati<NX>, (int)sizeof(RicWS)}, {(const void*)k_seg_riccati<CNX>, (int)sizeof(RicWS)},
      {(const void*)k_ric_forward<NX>, (int)sizeof(RicWS)}, {(const void*)k_ric_forward<CNX>, (int)sizeof(RicWS)},
      {(const void*)k_seg_accumulate<NX>, (int)sizeof(SegAccWS)}, {(const void*)k_seg_accumulate<CNX>, (int)sizeof(SegAccWS)}};
  for (const auto& k : lds_limits)
    if (k.f && hipFuncSetAttribute(k.f, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes) != hipSuccess)
      return fail(HSQP_ERR_HIP, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
  *out = h;
  g_create_error.clear();
  return HSQP_OK;
}

// centroidal formulation: the padding states of every state row must be zero (include/hsqp.h)
static bool padding_is_zero(hsqp_handle* h, const hsqp_problem* p) {
  if (h->hdm.formulation != HSQP_FORM_CENTROIDAL) return true;
  const size_t rows = (size_t)p->batch * (p->x_traj ? p->n_nodes + 2 : 1);   // (no x_traj: the warm start is built on the device)
  for (size_t r = 0; r < rows; ++r) {
    const double* row = r < (size_t)p->batch ? p->x_init + r * NX : p->x_traj + (r - p->batch) * NX;
    for (int i = HSQP_CNX; i < NX; ++i)
      if (row[i] != 0.0) { h->err = "centroidal formulation: entries 35..57 of every state row must be zero"; return false; }
  }
  return true;
}

// interval lengths of the problem: hsqp_problem::dt_nodes, or the uniform dt.  Host arrays are validated (finite, >= 0, no event
// as the last interval); device-resident ones are the caller's responsibility and are scanned for events on the device side later.
static int set_grid(hsqp_handle* h, const hsqp_problem* p, bool device_src) {
  const size_t B = p->batch, N = p->n_nodes;
  h->has_events = false;
  if (!p->dt_nodes) {
    // (a receding-horizon caller uploads the same uniform grid every cycle: the resident copy is kept)
    const bool resident = h->grid_resident && h->uniform_grid && h->h_dt.size() == B * N && h->grid_N == p->n_nodes && h->grid_dt == p->dt;
    h->uniform_grid = true;
    if (resident) return HSQP_OK;
    h->grid_resident = false;
    h->h_dt.assign(B * N, p->dt);
    HCHECK(hipMemcpyAsync(h->d_dt, h->h_dt.data(), B * N * 8, hipMemcpyHostToDevice, h->stream));
    h->grid_resident = true; h->grid_N = p->n_nodes; h->grid_dt = p->dt;
    return HSQP_OK;
  }
  h->uniform_grid = false; h->grid_resident = false;
  if (device_src) {
    h->h_dt.resize(B * N);
    HCHECK(hipMemcpyAsync(h->d_dt, p->dt_nodes, B * N * 8, hipMemcpyDeviceToDevice, h->stream));
    HCHECK(hipMemcpyAsync(h->h_dt.data(), h->d_dt, B * N * 8, hipMemcpyDeviceToHost, h->stream));
    HCHECK(hipStreamSynchronize(h->stream));
  } else {
    h->h_dt.assign(p->dt_nodes, p->dt_nodes + B * N);
  }
  for (size_t b = 0; b < B; ++b)
    for (size_t k = 0; k < N; ++k) {
      const double d = h->h_dt[b * N + k];
      if (!(d >= 0.0) || d > 1e6) { h->err = "dt_nodes: interval lengths must be finite and >= 0"; return HSQP_ERR_BAD_ARG; }
      if (d == 0.0) {
        // the FIRST interval may be an event: a mode switch within dt_min after the initial time replaces the initial node
        // (timeDiscretizationWithEvents), and the identity-jump stage works at node 0 like anywhere else
        if (k == N - 1) { h->err = "dt_nodes: the last interval cannot be an event (dt = 0)"; return HSQP_ERR_BAD_ARG; }
        h->has_events = true;
      }
    }
  if (!device_src) HCHECK(hipMemcpyAsync(h->d_dt, h->h_dt.data(), B * N * 8, hipMemcpyHostToDevice, h->stream));
  return HSQP_OK;
}

// the first failing call of a sequence goes to h->err and rc; the later calls are still made, their results ignored
struct StickyError {
  hsqp_handle* h; int rc = HSQP_OK;
  void operator()(hipError_t e, const char* what) { if (rc == HSQP_OK && e != hipSuccess) { h->err = std::string(what) + ": " + hipGetErrorString(e); rc = HSQP_ERR_HIP; } }
};

// the problem fits the handle (hsqp_settings::max_batch, max_nodes) and has a grid
static bool fits_handle(hsqp_handle* h, const hsqp_problem* p) {
  const bool ok = p->batch >= 1 && p->batch <= h->st.max_batch && p->n_nodes >= 1 && p->n_nodes <= h->st.max_nodes && (p->dt_nodes || p->dt > 0.0);
  if (!ok) h->err = "batch / n_nodes outside the handle's capacity, or dt <= 0";
  return ok;
}

// the uploaded problem is now the resident one (no solution yet).  The gate's history belongs to the problem that produced it: the back-off
// restarts unless the caller asked to keep it across uploads of the same shape (receding-horizon callers)
static void commit_problem(hsqp_handle* h, const hsqp_problem* p, bool have_stamps) {
  const bool same_shape = h->B == p->batch && h->N == p->n_nodes;
  h->B = p->batch; h->N = p->n_nodes; h->dt = p->dt;
  h->have_problem = true; h->have_solution = false; h->have_stamps = have_stamps;
  if (!(h->backoff_persistent && same_shape)) { h->seg_backoff = 0; h->seg_backoff_len = 0; }
}

static int upload_impl(hsqp_handle* h, const hsqp_problem* p, bool device_src) {
  if (!h) return HSQP_ERR_BAD_ARG;
  h->have_policy = false;
  h->have_value = false;
  h->loop.started = false;
  if (!p || !p->x_init || !p->x_traj || !p->u_traj || !p->node_params) { h->err = "null problem pointer"; return HSQP_ERR_BAD_ARG; }
  if (!fits_handle(h, p)) return HSQP_ERR_BAD_ARG;
  if (!device_src && !padding_is_zero(h, p)) return HSQP_ERR_BAD_ARG;   // device-resident inputs: the caller guarantees the zero padding
  HCHECK(hipSetDevice(h->device));
  const size_t B = p->batch, N = p->n_nodes;
  const hipMemcpyKind kind = device_src ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  // the grid is validated BEFORE any trajectory copy is queued; a rejected problem leaves no half-uploaded state behind
  h->have_problem = false; h->have_solution = false; h->have_stamps = false;
  { const int rc = set_grid(h, p, device_src); if (rc != HSQP_OK) return rc; }
  HCHECK(hipMemcpyAsync(h->d_xinit, p->x_init, B * NX * 8, kind, h->stream));
  HCHECK(hipMemcpyAsync(h->d_x, p->x_traj, B * (N + 1) * NX * 8, kind, h->stream));
  HCHECK(hipMemcpyAsync(h->d_u, p->u_traj, B * N * NU * 8, kind, h->stream));
  HCHECK(hipMemcpyAsync(h->d_par, p->node_params, B * (N + 1) * NP * 8, kind, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  commit_problem(h, p, false);
  h->stamps_resident = false;
  return HSQP_OK;
}

int hsqp_upload(hsqp_handle* h, const hsqp_problem* p) { return upload_impl(h, p, false); }
int hsqp_upload_device(hsqp_handle* h, const hsqp_problem* p) { return upload_impl(h, p, true); }

// the numeric status of the resident solution (d_status, read back by the caller): HSQP_ERR_NUMERIC and its message if an instance failed
static int check_status(hsqp_handle* h, const std::vector<int>& status) {
  for (size_t b = 0; b < status.size(); ++b)
    if (status[b]) {
      h->err = "instance " + std::to_string(b) + ": " + ((status[b] & 1) ? "rank-deficient equality Jacobian D " : "") +
               ((status[b] & 2) ? "reduced Hessian not positive definite" : "");
      return HSQP_ERR_NUMERIC;
    }
  return HSQP_OK;
}

// HSQP_WARM_SHIFT's preconditions, checked before anything is copied: a rejected call leaves the resident solution as it was.
// per_instance (the isolated loop): the refusal after a numeric failure is the instance's — the triage has marked it HSQP_WARM_COLD on the device
// (RefDev::warm_b), so the status words are not read here
static int warm_shift_ready(hsqp_handle* h, int batch, bool sorted, bool per_instance = false) {
  if (!h->have_solution || !h->have_stamps) {
    h->err = "warm_start SHIFT: no resident solution of a problem uploaded through hsqp_upload_reference";
    return HSQP_ERR_BAD_ARG;
  }
  if (h->B != batch) { h->err = "warm_start SHIFT: the batch differs from the resident solution's"; return HSQP_ERR_BAD_ARG; }
  if (!sorted) { h->err = "warm_start SHIFT: node_times must not decrease"; return HSQP_ERR_BAD_ARG; }
  if (per_instance) return HSQP_OK;
  std::vector<int> status(h->B);
  HCHECK(hipMemcpy(status.data(), h->d_status, status.size() * sizeof(int), hipMemcpyDeviceToHost));
  return check_status(h, status);
}

// the compact reference of a problem, every array resident on the device (hsqp_upload_reference: its staging area; the loop: its own buffers)
struct RefDev {
  int E, K;                        // max_events, n_knots
  const int* ne; const int* seq;   // [B], [B][E + 1]
  const double* ev;                // [B][E]
  const double* tt; const double* ts; const double* nt;   // [B][K], [B][K][58], [B][N + 1] or null
  int* bad;                        // one int, zeroed on the stream before the call
  double t0, dt;
  hsqp_swing_config swing; double terrain_height; int arm_swing, warm, N_prev;
  bool sorted;
  const int* warm_b = nullptr;     // [B] HSQP_WARM_SHIFT / _COLD per instance (the isolated loop; `warm` is then SHIFT), or null: `warm` for all
  const int* grid_bad = nullptr;   // one int the builder of a device-built grid has set if an instance has none (the loop on the event grid), or null
  const double* terrain_b = nullptr;   // [B] one terrain height per instance in place of terrain_height (include/hsqp_ground.h), or null
  const double* lift_rows = nullptr;   // [B][2][E + 1] the planner's lift-off and touch-down height per foot and phase (include/hsqp_perceive.h), or both null
  const double* touch_rows = nullptr;
};

// The device side of hsqp_upload_reference, behind the copies `step` has queued on the stream (x_init in d_xinit, the grid in d_dt, the CALLER warm start
// in d_x / d_u): the node-parameter table, the grid's raw stamps, the device-built warm start; then the problem is the resident one.
static int reference_build(hsqp_handle* h, const hsqp_problem* p, const RefDev& r, StickyError& step) {
  const size_t B = p->batch, N = p->n_nodes;
  if (step.rc == HSQP_OK) {
    const int total = (int)(B * (N + 1));
    HSQP_LAUNCH(k_params, dim3((total + 63) / 64), dim3(64), 0, h->stream, h->d_dm, r.swing, r.terrain_height, r.arm_swing, r.E, r.ne, r.ev, r.seq,
                       r.K, r.tt, r.ts, r.t0, r.dt, r.nt, (int)N, (int)B, h->d_par, r.bad, r.terrain_b, r.lift_rows, r.touch_rows);
    if (h->hdm.formulation == HSQP_FORM_CENTROIDAL)   // torso task-space reference of every row
      HSQP_LAUNCH(k_params_cent_torso, dim3(total), dim3(64), sizeof(CentWST<false>), h->stream, h->d_dm, h->d_par);
    step(hipGetLastError(), "k_params");
  }
  if (step.rc == HSQP_OK) {   // the grid's raw stamps (every mode) and the device-built warm start (SHIFT / COLD), after k_params wrote the contact flags
    WarmArgs w{};
    w.mode = r.warm; w.mode_b = r.warm_b; w.B = (int)B; w.N = (int)N; w.N_prev = r.warm == HSQP_WARM_SHIFT ? r.N_prev : 0; w.cent = h->hdm.formulation == HSQP_FORM_CENTROIDAL;
    w.t0 = r.t0; w.dt = r.dt; w.total_mass = h->hdm.total_mass;
    w.node_times = r.nt; w.dts = h->d_dt; w.par = h->d_par; w.x_init = h->d_xinit;
    w.x_prev = h->d_xnew; w.u_prev = h->d_unew; w.stamps_prev = h->d_stamps[h->stamps_cur];
    w.x = h->d_x; w.u = h->d_u; w.stamps = h->d_stamps[1 - h->stamps_cur];
    const size_t lds = r.warm == HSQP_WARM_SHIFT ? (size_t)(r.N_prev + 1) * 8 : 0;
    HSQP_LAUNCH(k_warm_start, dim3((unsigned)((N + 1 + WARM_WAVES - 1) / WARM_WAVES), (unsigned)B), dim3(64 * WARM_WAVES), lds, h->stream, w);
    step(hipGetLastError(), "k_warm_start");
  }
  int bad = 0, grid_bad = 0;
  step(hipMemcpyAsync(&bad, r.bad, 4, hipMemcpyDeviceToHost, h->stream), "download status");
  if (r.grid_bad) step(hipMemcpyAsync(&grid_bad, r.grid_bad, 4, hipMemcpyDeviceToHost, h->stream), "download grid status");
  step(hipStreamSynchronize(h->stream), "sync");
  if (step.rc != HSQP_OK) return step.rc;
  if (grid_bad) return HSQP_ERR_BAD_ARG;   // (the caller reads the instances' status words and writes the message)
  if (bad) { h->err = "a swing phase has no lift-off / touch-down inside the mode schedule"; return HSQP_ERR_BAD_ARG; }
  h->stamps_cur = 1 - h->stamps_cur;
  commit_problem(h, p, r.sorted);
  h->stamps_resident = true;
  return HSQP_OK;
}

static int loop_bad(hsqp_handle* h, const char* who, const char* what);   // (below, with the entry points of include/hsqp_loop.h)
static bool all_finite(const double* v, size_t n);

// hsqp_upload_reference, hsqp_upload_reference_ground (terrain_heights != null: [B] host, checked by the caller, staged here) and
// hsqp_upload_reference_heights (lift_off, touch_down != null: [B][2][E + 1] host, staged here; who: that entry point, which checks the rows here, where
// the schedule has been checked)
static int upload_reference_impl(hsqp_handle* h, const hsqp_problem* p, const hsqp_reference* r, const double* terrain_heights, const double* lift_off = nullptr,
                                 const double* touch_down = nullptr, const char* who = nullptr) {
  if (!h) return HSQP_ERR_BAD_ARG;
  h->have_policy = false;
  h->have_value = false;
  h->loop.started = false;
  if (!p || !r || !p->x_init || !r->n_events || !r->event_times || !r->mode_sequence || !r->target_times || !r->target_states) {
    h->err = "null problem / reference pointer";
    return HSQP_ERR_BAD_ARG;
  }
  const int warm = r->warm_start;
  if (warm != HSQP_WARM_CALLER && warm != HSQP_WARM_SHIFT && warm != HSQP_WARM_COLD) {
    h->err = "hsqp_reference::warm_start must be HSQP_WARM_CALLER, HSQP_WARM_SHIFT or HSQP_WARM_COLD";
    return HSQP_ERR_BAD_ARG;
  }
  if ((warm == HSQP_WARM_CALLER) != (p->x_traj && p->u_traj) || (warm != HSQP_WARM_CALLER && (p->x_traj || p->u_traj))) {
    h->err = warm == HSQP_WARM_CALLER ? "null problem / reference pointer" : "warm_start SHIFT / COLD: hsqp_problem::x_traj and u_traj must be NULL";
    return HSQP_ERR_BAD_ARG;
  }
  if (!fits_handle(h, p)) return HSQP_ERR_BAD_ARG;
  if (r->batch != p->batch || r->n_nodes != p->n_nodes || (!r->node_times && r->dt != p->dt) || r->max_events < 1 || r->n_knots < 1) {
    h->err = "reference does not match the problem (batch, n_nodes, dt) or is empty";
    return HSQP_ERR_BAD_ARG;
  }
  if ((p->dt_nodes != nullptr) != (r->node_times != nullptr)) {
    h->err = "a non-uniform grid needs both hsqp_problem::dt_nodes and hsqp_reference::node_times";
    return HSQP_ERR_BAD_ARG;
  }
  for (int b = 0; b < r->batch; ++b)
    if (r->n_events[b] < 1 || r->n_events[b] > r->max_events) { h->err = "n_events outside [1, max_events]"; return HSQP_ERR_BAD_ARG; }
  if (lift_off)   // (a refused call leaves the resident problem as it was)
    for (size_t b = 0; b < (size_t)r->batch; ++b)
      for (size_t f = 0; f < 2; ++f) {
        const size_t row = (b * 2 + f) * ((size_t)r->max_events + 1);
        if (!all_finite(lift_off + row, (size_t)r->n_events[b] + 1) || !all_finite(touch_down + row, (size_t)r->n_events[b] + 1))
          return loop_bad(h, who, ("non-finite lift_off / touch_down entry of instance " + std::to_string(b) + " in its phases 0 .. n_events").c_str());
      }
  if (!padding_is_zero(h, p)) return HSQP_ERR_BAD_ARG;
  bool sorted = true;   // raw stamps of the new grid non-decreasing (always on a uniform grid): what the interpolation of a later SHIFT needs
  for (size_t i = 1; r->node_times && sorted && i < (size_t)p->batch * (p->n_nodes + 1); ++i)
    sorted = i % (p->n_nodes + 1) == 0 || r->node_times[i] >= r->node_times[i - 1];
  HCHECK(hipSetDevice(h->device));
  const int N_prev = h->N;
  if (warm == HSQP_WARM_SHIFT) { const int rc = warm_shift_ready(h, p->batch, sorted); if (rc != HSQP_OK) return rc; }
  const size_t B = p->batch, N = p->n_nodes, E = r->max_events, K = r->n_knots;
  DEV_ENSURE(h->d_stage, ref_stage_layout(Carve{}, B, N, E, K, r->node_times).bytes, "reference staging");
  const auto [d_ne, d_seq, d_bad, d_ev, d_tt, d_ts, d_nt, staged] = ref_stage_layout(Carve{h->d_stage.p}, B, N, E, K, r->node_times);
  h->have_problem = false; h->have_solution = false; h->have_stamps = false;   // a failure below leaves no half-uploaded problem behind
  { const int rc = set_grid(h, p, false); if (rc != HSQP_OK) return rc; }
  StickyError step{h};
  if (d_nt) step(hipMemcpyAsync(d_nt, r->node_times, B * (N + 1) * 8, hipMemcpyHostToDevice, h->stream), "upload node_times");
  step(hipMemcpyAsync(d_ne, r->n_events, B * 4, hipMemcpyHostToDevice, h->stream), "upload n_events");
  step(hipMemcpyAsync(d_seq, r->mode_sequence, B * (E + 1) * 4, hipMemcpyHostToDevice, h->stream), "upload mode_sequence");
  step(hipMemcpyAsync(d_ev, r->event_times, B * E * 8, hipMemcpyHostToDevice, h->stream), "upload event_times");
  step(hipMemcpyAsync(d_tt, r->target_times, B * K * 8, hipMemcpyHostToDevice, h->stream), "upload target_times");
  step(hipMemcpyAsync(d_ts, r->target_states, B * K * NX * 8, hipMemcpyHostToDevice, h->stream), "upload target_states");
  step(hipMemsetAsync(d_bad, 0, 4, h->stream), "memset");
  step(hipMemcpyAsync(h->d_xinit, p->x_init, B * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x_init");
  if (warm == HSQP_WARM_CALLER) {
    step(hipMemcpyAsync(h->d_x, p->x_traj, B * (N + 1) * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x");
    step(hipMemcpyAsync(h->d_u, p->u_traj, B * N * NU * 8, hipMemcpyHostToDevice, h->stream), "upload u");
  }
  RefDev rd{(int)E, (int)K, d_ne, d_seq, d_ev, d_tt, d_ts, d_nt, d_bad, r->t0, r->dt, r->swing, r->terrain_height, r->arm_swing, warm, N_prev, sorted};
  if (terrain_heights) {
    DEV_ENSURE(h->d_ground_stage, ground_stage_layout(Carve{}, B, E, false).bytes, "terrain-height staging");
    double* d_terrain = ground_stage_layout(Carve{h->d_ground_stage.p}, B, E, false).terrain;
    step(hipMemcpyAsync(d_terrain, terrain_heights, B * 8, hipMemcpyHostToDevice, h->stream), "upload terrain_heights");
    rd.terrain_b = d_terrain;
  }
  if (lift_off) {
    DEV_ENSURE(h->d_perceive_stage, perceive_stage_layout(Carve{}, B, E, K, false).bytes, "height-row staging");
    const PerceiveStage sg = perceive_stage_layout(Carve{h->d_perceive_stage.p}, B, E, K, false);
    step(hipMemcpyAsync(sg.lift, lift_off, B * 2 * (E + 1) * 8, hipMemcpyHostToDevice, h->stream), "upload lift_off");
    step(hipMemcpyAsync(sg.touch, touch_down, B * 2 * (E + 1) * 8, hipMemcpyHostToDevice, h->stream), "upload touch_down");
    rd.lift_rows = sg.lift; rd.touch_rows = sg.touch;
  }
  return reference_build(h, p, rd, step);
}
int hsqp_upload_reference(hsqp_handle* h, const hsqp_problem* p, const hsqp_reference* r) { return upload_reference_impl(h, p, r, nullptr); }

// The backward sweep of an iteration: serial recursion, or — one or two instances on a long horizon, or on request — the associative scan over the
// stages (hsqp_scan.h), or on request the two-level sweep with P segments per instance (hsqp_segment.h).  The scan inverts I + C1 J2 of partial
// horizons (condition number up to 1e5 centroidal, 1e9 whole-body): on the QPs of a cold start or of a tracking MPC it reproduces the serial
// recursion to 1e-11 of the step's scale, on a far-from-feasible line-search iterate it can lose five digits.  Both are therefore GATED: the KKT
// residual of the QP is evaluated (k_kkt, one small kernel + one 3 B-double read-back) and, if a residual exceeds the gate (scan_gate_accepts,
// hsqp_scan.h), the iteration is redone with the serial recursion (hsqp_scan_fallbacks counts these).
// A problem class whose sweeps keep failing the gate (badly scaled QPs: |S| ~ 1e6 on perturbed centroidal batches) would pay sweep + fallback every
// iteration — a rejected scan costs scan + serial sweep (0.55 + 1.45 ms at one whole-body instance), and the iterates that fail the gate, far-from-
// feasible line-search iterates, come in runs: after a rejection the handle backs off to the serial recursion for 1, 3, 7, .. 63 iterations before
// it tries again.  The back-off is part of the automatic choice only: a sweep the caller FORCED by a flag (the two-level sweep always is) is
// attempted every iteration, so forced timings and the parity tests of the forced sweeps never silently measure the serial recursion.
struct Sweep { enum Kind { SERIAL, SCAN, SEGMENTED } kind; int P; };   // P: segments per instance (SEGMENTED)
static Sweep choose_sweep(hsqp_handle* h, int B, int N) {
  const int flags = h->st.flags;
  if (flags & HSQP_FLAG_SEGMENTED_RICCATI) {
    const int P = segment_count(h, B, N);
    return P > 0 ? Sweep{Sweep::SEGMENTED, P} : Sweep{Sweep::SERIAL, 0};
  }
  if (flags & HSQP_FLAG_PARALLEL_RICCATI) return {Sweep::SCAN, 0};
  if ((flags & HSQP_FLAG_SERIAL_RICCATI) || !(B <= HSQP_SCAN_AUTO_BATCH && N >= HSQP_SCAN_AUTO_MIN_NODES)) return {Sweep::SERIAL, 0};
  if (h->seg_backoff > 0) { --h->seg_backoff; ++h->backoff_iterations; return {Sweep::SERIAL, 0}; }
  return {Sweep::SCAN, 0};
}

// the value pass of the trial (d_xnew, d_unew): per-node {ne, dt*cost, dt*eq^2, dt*dyn^2} in d_misc.  mask: the line search's state (only the
// instances whose trial is pending), or null.  (Whole-body without the quad form: the step path fuses it into k_step_value)
static void launch_value_pass(hsqp_handle* h, const LsState* mask) {
  const int N = h->N, nodes = h->B * h->N;
  if (h->hdm.formulation == HSQP_FORM_CENTROIDAL)
    HSQP_LAUNCH(k_lq_cent2_value, dim3(nodes), dim3(64), sizeof(CentWST<false>), h->stream, h->d_dm, h->d_xnew, h->d_unew, h->d_par, h->d_dt, N, h->d_misc, mask);
  else if (h->value_quad)   // quads of lanes (hsqp_lqv.h)
    HSQP_LAUNCH(k_value_quad, dim3((nodes + QV_NODES * QV_WAVES - 1) / (QV_NODES * QV_WAVES)), dim3(QV_THREADS * QV_WAVES), 0, h->stream, h->d_dm, h->d_xnew, h->d_unew, h->d_par, h->d_dt,
                N, nodes, h->d_misc, mask);
  else
    HSQP_LAUNCH(k_lq<false>, dim3(nodes), dim3(LQV_THREADS), sizeof(LqWST<false>), h->stream, h->d_dm, h->d_xnew, h->d_unew, h->d_par, h->d_dt,
                N, (double*)nullptr, h->d_misc, (long long*)nullptr, mask);
}

int hsqp_iterate_device(hsqp_handle* h, int n_iterations, int flags) {
  const int take_step = flags & HSQP_ITER_TAKE_STEP, want_kkt = (flags & HSQP_ITER_KKT) ? 1 : 0, linesearch = (flags & HSQP_ITER_LINESEARCH) ? 1 : 0;
  if (!h) return HSQP_ERR_BAD_ARG;
  // HSQP_ITER_VALUE_FUNCTION (include/hsqp_value.h): the sweep whose step is accepted also leaves S_k, s_k of every node (as for the KKT report, but no
  // k_kkt launch, no joint rows, no read-back) and the iteration starts with a copy of the trajectory it linearises at
  const int want_value = (flags & HSQP_ITER_VALUE_FUNCTION) ? 1 : 0;
  h->have_policy = false;   // (a failed iteration leaves the records half written)
  h->have_value = false;    // (... and an iteration without the flag overwrites the sweep's part of the record's buffers or leaves them stale)
  if (!h->have_problem || n_iterations < 1) { h->err = "no problem uploaded or n_iterations < 1"; return HSQP_ERR_BAD_ARG; }
  HCHECK(hipSetDevice(h->device));
  const int B = h->B, N = h->N;
  const int nodes = B * N;
  const bool cent = h->hdm.formulation == HSQP_FORM_CENTROIDAL;
  HCHECK(hipMemsetAsync(h->d_status, 0, (size_t)B * sizeof(int), h->stream));   // once per call: the kernels OR into it
  const bool until_converged = (flags & HSQP_ITER_UNTIL_CONVERGED) != 0;
  h->iter_log.clear();
  h->last_iterations = 0;
  double ms_sum[4] = {0.0, 0.0, 0.0, 0.0};
  bool converged = false;
  for (int it = 0; it < n_iterations && !converged; ++it) {
    // (until_converged: any iteration may turn out to be the last one, so each is bracketed by the timing events and its times are summed)
    const bool last = it == n_iterations - 1 || until_converged;
    if (last) HCHECK(hipEventRecord(h->ev[0], h->stream));
    const Sweep sweep = choose_sweep(h, B, N);
    const int segP = sweep.kind == Sweep::SEGMENTED ? sweep.P : 0;
    const bool scan = sweep.kind != Sweep::SERIAL;   // a KKT-gated sweep with the serial recursion as fallback
    // The joint rows of A~ / B~ (46 of 58: scaled copies of rows of [Px | Pu]) are written only for those who read A~ / B~ as dense blocks: the
    // parallel-in-time and two-level sweeps, the KKT report, the centroidal stage.  The whole-body serial sweep works on the factors.
    const bool joint_rows = cent || !h->ric_fact || scan || want_kkt;
    const int proj_chain = (!cent && h->lq_limb && h->chain_fused) ? 1 : 0;
    // node ranges of the pipelined stages (S > 1: limb-lane form, a launch of more than one round of the chip): range s is the nodes
    // range_begin(s) .. range_begin(s + 1) - 1, cut at the 32-node workgroups of the limb-lane LQ kernels
    constexpr int QG = QL_NODES * QL_WAVES;
    const int S = !cent && h->lq_limb && h->lq_split > 1 && (nodes + QG - 1) / QG > h->lq_round_blocks ? h->lq_split : 1;
    auto range_begin = [&](int s) { return s >= S ? nodes : (int)(((long long)nodes * s / S) / QG * QG); };
    auto range_stream = [&](int s) { return s == 0 ? h->stream : h->aux[s - 1]; };
    if (cent) {
      HSQP_LAUNCH(k_lq_cent2, dim3(nodes), dim3(CLQ_THREADS), sizeof(CentWST<true>), h->stream, h->d_dm, h->d_x, h->d_u, h->d_par, h->d_dt, N, h->d_rec);
    }
    else if (h->lq_limb) {   // limb lanes for the model and the node terms (16 nodes per wave), then the RK4 chain, a lane per column (hsqp_lql.h)
      // Two of the three kernels run one wave per SIMD (limb, rows), so a launch of config 4 is 1.56 rounds of the chip's 1024 SIMDs and the
      // last round of each leaves 44 % of them idle.  With lq_split = 2 the nodes are cut into two ranges, each going through its LQ
      // kernels AND its k_project (and k_jump) on a stream of its own: a range's next kernel fills the SIMDs the other range's previous
      // kernel leaves, and the projection of the range that is through first starts on the CUs the other range's last k_lq_rows round
      // leaves free (a k_project workgroup is 49.5 KB of LDS and four waves of 120 VGPR: it fits wherever no LQ workgroup sits).
      // project_node and jump_node_qp see their own node's record and QP block only, so a range boundary may lie inside an instance.
      // The ranges join behind k_project: the backward sweep waits for all of the QP record.  (Measured, 256 x 100, the LQ kernels
      // alone: 1.07 -> 0.97 ms at two ranges; three and more lose again: 1.02 / 1.10 / 1.38 ms at 3 / 4 / 8.  DESIGN.md section 4 has
      // the drawing.)  Only when a launch is more than one round; S == 1 is one launch per kernel on h->stream.
      // kernel_ms: ev[1] is recorded behind range 0's k_lq_rows and ev[2] behind the join, so with S > 1 what the other ranges' LQ
      // kernels run past ev[1] lands in the project bucket; the buckets stay contiguous and sum to the total.
      const dim3 qblock(QL_THREADS * QL_WAVES);
      if (S > 1) {
        HCHECK(hipEventRecord(h->ev_fork, h->stream));
        for (int s = 1; s < S; ++s) HCHECK(hipStreamWaitEvent(h->aux[s - 1], h->ev_fork, 0));
      }
      for (int s = 0; s < S; ++s) {
        const int n0 = range_begin(s), n1 = range_begin(s + 1);
        hipStream_t st = range_stream(s);
        const dim3 qgrid((n1 - n0 + QG - 1) / QG);
        HSQP_LAUNCH(k_lq_limb, qgrid, qblock, 0, st, h->d_dm, h->d_x, h->d_u, h->d_dt, N, n1, h->d_rec, h->d_prof + 384, n0);
        HSQP_LAUNCH(k_lq_rows, qgrid, qblock, 0, st, h->d_dm, h->d_x, h->d_u, h->d_par, h->d_dt, N, n1, h->d_rec, h->d_prof + 384, n0, h->chain_fused ? 1 : 0);
        if (!h->chain_fused) HSQP_LAUNCH(k_lq_chain, dim3(n1 - n0), dim3(LQC_THREADS), 0, st, h->d_x, h->d_u, h->d_dt, N, h->d_rec, n0, 1);   // (fused: the columns' chain runs in k_project, the defect on the lanes of k_lq_rows)
        if (s == 0 && last) HCHECK(hipEventRecord(h->ev[1], h->stream));
        HSQP_LAUNCH(k_project, dim3(n1 - n0), dim3(PROJ_THREADS), sizeof(ProjWS), st, h->d_rec, h->d_dt, h->d_qp, h->d_prof + 128, 0, joint_rows ? 1 : 0, proj_chain, n0);
        if (h->has_events) HSQP_LAUNCH(k_jump, dim3(n1 - n0), dim3(256), 0, st, h->d_dt, h->d_rec, h->d_qp, n0);
        if (s > 0) HCHECK(hipEventRecord(h->ev_join[s - 1], st));
      }
      for (int s = 1; s < S; ++s) HCHECK(hipStreamWaitEvent(h->stream, h->ev_join[s - 1], 0));
    } else
      HSQP_LAUNCH(k_lq<true>, dim3(nodes), dim3(LQ_THREADS), sizeof(LqWS), h->stream, h->d_dm, h->d_x, h->d_u, h->d_par, h->d_dt, N,
                         h->d_rec, (double*)nullptr, h->d_prof, (const LsState*)nullptr);
    if (cent || !h->lq_limb) {
      if (last) HCHECK(hipEventRecord(h->ev[1], h->stream));
      HSQP_LAUNCH(k_project, dim3(nodes), dim3(PROJ_THREADS), sizeof(ProjWS), h->stream, h->d_rec, h->d_dt, h->d_qp, h->d_prof + 128, cent ? 1 : 0, joint_rows ? 1 : 0, proj_chain, 0);
      if (h->has_events) HSQP_LAUNCH(k_jump, dim3(nodes), dim3(256), 0, h->stream, h->d_dt, h->d_rec, h->d_qp, 0);
    }
    h->qp_joint_rows = joint_rows;
    if (last) HCHECK(hipEventRecord(h->ev[2], h->stream));
    if (want_kkt || want_value) DEV_ENSURE(h->d_vf, vf_bytes(h), "value functions");
    if (want_value) {   // xbar: d_x is only replaced between iterations, so the last iteration's copy is the record's
      DEV_ENSURE(h->d_xbar, (size_t)h->st.max_batch * (h->st.max_nodes + 1) * NX * 8, "value function: linearisation trajectory");
      HCHECK(hipMemcpyAsync(h->d_xbar, h->d_x, (size_t)B * (N + 1) * NX * 8, hipMemcpyDeviceToDevice, h->stream));
    }
    const bool keep_vf = want_kkt || want_value;
    const double* vf_kept = h->d_vf;   // where the sweep whose step is accepted leaves its value functions
    const int Bm = h->st.max_batch;
    const size_t gate_bytes = h->gate.bytes;
    int ut_given = 0;   // the last sweep's roll-out left ut = k + K dx of every node in d_ut (the serial roll-out does, the scan's closed-loop roll-out does not)
    int fj_given = 0;   // ... and rows 12 .. 34 of Px dx + Pu ut in d_fj (the factored roll-out does)
    auto launch_sweep = [&](bool use_scan, bool need_vf) -> int {
      ut_given = (use_scan && segP == 0) ? 0 : 1;
      fj_given = 0;
      if (use_scan && segP > 0) return cent ? launch_segmented<CNX>(h, B, N, segP, keep_vf) : launch_segmented<NX>(h, B, N, segP, keep_vf);
      if (use_scan) return cent ? launch_scan<CNX>(h, B, N, need_vf, 1) : launch_scan<NX>(h, B, N, need_vf, HSQP_SCAN_WB_REFINEMENTS);
      if (cent)   // the serial recursion on the 35 centroidal states only (the padding states are decoupled)
        HSQP_LAUNCH(k_riccati<CNX>, dim3(B), dim3(RIC_THREADS), sizeof(RicWS), h->stream, h->d_dm, h->d_xinit, h->d_x, h->d_par, h->d_qp,
                           h->d_ric, N, h->d_dx, h->d_status, h->d_prof + 256, need_vf ? h->d_vf : (double*)nullptr, h->d_ut);
      else if (h->ric_fact)
        { HSQP_LAUNCH(k_riccati_fact, dim3(B), dim3(RIC_THREADS), sizeof(RicFWS), h->stream, h->d_dm, h->d_xinit, h->d_x, h->d_par, h->d_qp, h->d_dt,
                           h->d_ric, N, h->d_dx, h->d_status, h->d_prof + 256, need_vf ? h->d_vf : (double*)nullptr, h->d_ut, h->d_fj); fj_given = 1; }
      else
        HSQP_LAUNCH(k_riccati<NX>, dim3(B), dim3(RIC_THREADS), sizeof(RicWS), h->stream, h->d_dm, h->d_xinit, h->d_x, h->d_par, h->d_qp,
                           h->d_ric, N, h->d_dx, h->d_status, h->d_prof + 256, need_vf ? h->d_vf : (double*)nullptr, h->d_ut);
      return HSQP_OK;
    };
    auto launch_step = [&]() {
      if (!cent && !h->value_quad)   // a tree with more than four limbs: the phase form of the value pass, fused with the step (k_step_value)
        HSQP_LAUNCH(k_step_value, dim3(nodes), dim3(LQV_THREADS), sizeof(LqWST<false>), h->stream, h->d_dm, h->d_qp, h->d_ric, h->d_dx, h->d_x, h->d_u,
                           h->d_par, h->d_dt, N, 1.0, h->d_ut, h->d_du, h->d_xnew, h->d_unew, h->d_stepinfo, h->d_misc, h->d_prof + 384, ut_given,
                           fj_given ? (const double*)h->d_fj : (const double*)nullptr);
      else {   // the step (HBM-bound); whole-body: then the value pass on quads of lanes (centroidal: launch_perf)
        // (k_step and k_value_quad are NOT taken through the node ranges: measured at 256 x 100 with two ranges, the value pass of the
        // high range on an aux stream beside the step of the low range, the bucket went from 0.193 to 0.228 ms — two 45 us halves of
        // k_step and two cross-stream waits cost more than the overlap returns.  DESIGN.md section 8)
        HSQP_LAUNCH(k_step, dim3(nodes), dim3(64), 0, h->stream, h->d_qp, h->d_ric, h->d_dx, h->d_x, h->d_u, N, 1.0, h->d_ut, h->d_du,
                           h->d_xnew, h->d_unew, h->d_stepinfo, ut_given, fj_given ? (const double*)h->d_fj : (const double*)nullptr);
        if (!cent) launch_value_pass(h, nullptr);
      }
    };
    // vf: the value functions of the sweep whose step is checked.  zeroed: the scan path has zeroed the block before its kernels
    auto launch_kkt = [&](const double* vf, bool zeroed) {
      const hipError_t e = zeroed ? hipSuccess : hipMemsetAsync(h->d_kkt, 0, gate_bytes, h->stream);   // kkt, |g|_inf (and the scan flags) are one block
      if (e == hipSuccess) HSQP_LAUNCH(k_kkt, dim3(nodes), dim3(256), 0, h->stream, h->d_xinit, h->d_x, h->d_qp, vf, h->d_dx, h->d_ut, N, h->d_kkt, h->gate.ginf);
      return e;
    };
    if (scan) HCHECK(hipMemsetAsync(h->d_kkt, 0, gate_bytes, h->stream));   // also the flags the scan kernels OR into
    { const int rc = launch_sweep(scan, keep_vf || scan); if (rc != HSQP_OK) return rc; }
    if (last) HCHECK(hipEventRecord(h->ev[3], h->stream));   // kernel_ms buckets: {lq, project, riccati (backward + forward sweep), step + value pass + reductions}
    launch_step();
    if (scan) {   // the gate's inputs: KKT residuals, |g|_inf and the scan kernels' flags travel to pinned host memory while the kernels below run
      // (two-level sweep: the gate block holds its boundary-consistency numbers instead — no KKT kernel; the KKT report, if asked for, follows the verdict)
      if (segP == 0) HCHECK(launch_kkt(h->d_vf2, true));
      else HSQP_LAUNCH(k_kkt_boundaries, dim3(B * (segP - 1)), dim3(256), 0, h->stream, h->d_xinit, h->d_x, h->d_qp, (const double*)h->d_vf2, h->d_dx, h->d_ut, N, segP,
                              h->d_kkt, h->gate.ginf);
      HCHECK(hipMemcpyAsync(h->h_gate, h->d_kkt, gate_bytes, hipMemcpyDeviceToHost, h->stream));
    } else if (want_kkt) {
      HCHECK(launch_kkt(h->d_vf, false));
    }
    auto launch_perf = [&]() {   // value pass of the centroidal trial, performance indices before / after, line-search state of the full-step trial
      if (cent) launch_value_pass(h, nullptr);
      HSQP_LAUNCH(k_perf_trio, dim3(B, 3), dim3(64), 0, h->stream, h->d_dm, h->d_rec + REC_MISC, REC_SIZE, h->d_x, h->d_misc, 8, h->d_xnew, h->d_par, N,
                         h->d_perf_before, h->d_perf_after, h->d_stepinfo, h->d_dx, h->d_ls);
    };
    launch_perf();   // speculatively on the scan's step: the gate is read only now, so the host round trip hides behind these kernels
    const bool ev4_early = last && !linesearch;
    if (ev4_early) HCHECK(hipEventRecord(h->ev[4], h->stream));
    if (scan) {
      HCHECK(hipStreamSynchronize(h->stream));
      const GateView hg = gate_view(h->h_gate, Bm);
      bool accept = true;
      for (int b = 0; b < B; ++b) {
        // (a flag = a bad pivot / failed factorisation inside the scan: the serial recursion decides what is reported in d_status)
        if (!scan_gate_accepts(hg.kkt[2 * b], hg.kkt[2 * b + 1], hg.ginf[b], hg.flags[b])) accept = false;
      }
      if (h->seg_debug && segP > 0) {
        double m0 = 0, m1 = 0, m2 = 0; int fl = 0;
        for (int b = 0; b < B; ++b) { m0 = fmax(m0, hg.kkt[2 * b]); m1 = fmax(m1, hg.kkt[2 * b + 1]); m2 = fmax(m2, hg.ginf[b]); fl |= hg.flags[b]; }
        fprintf(stderr, "[hsqp seg gate] P=%d boundary-stage KKT stat %.3e prim %.3e |g| %.3e flags %d accept %d\n", segP, m0, m1, m2, fl, (int)accept);
      }
      if (accept && segP > 0 && want_kkt) HCHECK(launch_kkt(h->d_vf2, false));   // the KKT report of an accepted two-level sweep (the gate block is reused)
      if (accept) { h->seg_backoff_len = 0; vf_kept = h->d_vf2; }   // (the back-off: choose_sweep)
      else {
        h->seg_backoff_len = std::min(2 * h->seg_backoff_len + 1, 63); h->seg_backoff = h->seg_backoff_len;
        ++h->scan_fallbacks;
        { const int rc = launch_sweep(false, keep_vf); if (rc != HSQP_OK) return rc; }
        if (last) HCHECK(hipEventRecord(h->ev[3], h->stream));
        launch_step();
        if (want_kkt) HCHECK(launch_kkt(h->d_vf, false));
        launch_perf();
        if (ev4_early) HCHECK(hipEventRecord(h->ev[4], h->stream));
      }
    }
    if (linesearch) {
      // back-tracking: decide the pending trials on the device, shorten the rejected steps, re-evaluate only those instances
      LsSettings lst{h->ls_settings.g_max, h->ls_settings.g_min, h->ls_settings.gamma_c, h->ls_settings.armijo_factor, h->ls_settings.alpha_decay,
                     h->ls_settings.alpha_min, h->ls_settings.delta_tol};
      // alpha_decay^n < alpha_min ends every instance's back-tracking with a zero step (ls_decide), so this bound is never the
      // reason the loop ends; hsqp_set_linesearch keeps it <= HSQP_LS_MAX_TRIALS
      const int max_trials = ls_max_trials(h->ls_settings);
      int still_active = 0;
      // Two trials per host round trip: the follow-up of a rejected trial (shortened trajectory, its value pass, its performance index) is
      // launched WITHOUT waiting for the verdict — every one of these kernels leaves the instances alone whose search is over (LsState::
      // active / dirty), so after an accepted trial they are no-ops of a few microseconds, and the host reads the counters of the second
      // decision only.  (One synchronisation per trial cost 40 us each at one instance — review item of round 1.)
      constexpr int LS_SPECULATIVE = 2;
      for (int trial = 0; trial < max_trials;) {
        int counts[2] = {0, 0};
        for (int r = 0; r < LS_SPECULATIVE && trial < max_trials; ++r, ++trial) {
          HCHECK(hipMemsetAsync(h->d_counts, 0, 2 * sizeof(int), h->stream));
          HSQP_LAUNCH(k_ls_decide, dim3((B + 63) / 64), dim3(64), 0, h->stream, lst, h->d_perf_before, h->d_perf_after, B, h->d_ls, h->d_counts);
          HSQP_LAUNCH(k_ls_retake, dim3(nodes), dim3(64), 0, h->stream, h->d_x, h->d_u, h->d_dx, h->d_du, N, h->d_ls, h->d_xnew, h->d_unew);
          launch_value_pass(h, h->d_ls);
          HSQP_LAUNCH(k_perf_reduce, dim3(B), dim3(64), 0, h->stream, h->d_dm, h->d_misc, 8, h->d_xnew, h->d_par, N, h->d_perf_after,
                             (const LsState*)h->d_ls);
        }
        HCHECK(hipMemcpyAsync(counts, h->d_counts, sizeof(counts), hipMemcpyDeviceToHost, h->stream));
        HCHECK(hipStreamSynchronize(h->stream));
        still_active = counts[1];
        if (counts[1] == 0) break;
      }
      if (still_active) { h->err = "line search: trials exhausted with instances still undecided (internal error)"; return HSQP_ERR_NUMERIC; }
    }
    h->ls_ran = linesearch != 0;
    h->vf_record = vf_kept;
    if (last && !ev4_early) HCHECK(hipEventRecord(h->ev[4], h->stream));
    h->last_iterations = it + 1;
    if (until_converged) {
      // SqpSolver::checkConvergence (upstream ocs2_sqp, restated from the published source; the fork's copy is absent): after ITERATIONS
      // (the loop bound) STEPSIZE (no step length accepted), then METRICS (|merit after - merit before| < costTol and the constraint
      // violation after the step below g_min), then PRIMAL (alpha |dx| and alpha |du| below deltaTol); the loop ends when EVERY instance
      // meets one of them.  The record of the iteration goes to the log.  The read-back lands in the handle's host buffers (no
      // allocation per iteration); with n_iterations == 1 the loop ends regardless of the verdict, but the log is still filled (the
      // adaptor reads step length and type from it).
      hsqp_handle::IterLog rec;
      rec.perf.resize(B); rec.alpha.resize(B); rec.type.resize(B);
      h->h_ls.resize(B); h->h_perf_before.resize(B);
      HCHECK(hipMemcpyAsync(h->h_ls.data(), h->d_ls, (size_t)B * sizeof(LsState), hipMemcpyDeviceToHost, h->stream));
      HCHECK(hipMemcpyAsync(rec.perf.data(), h->d_perf_after, (size_t)B * sizeof(hsqp_perf), hipMemcpyDeviceToHost, h->stream));
      HCHECK(hipMemcpyAsync(h->h_perf_before.data(), h->d_perf_before, (size_t)B * sizeof(hsqp_perf), hipMemcpyDeviceToHost, h->stream));
      HCHECK(hipStreamSynchronize(h->stream));
      const std::vector<LsState>& ls = h->h_ls;
      converged = true;
      for (int b = 0; b < B; ++b) {
        rec.alpha[b] = linesearch ? ls[b].alpha : 1.0;
        rec.type[b] = linesearch ? ls[b].step_type : HSQP_STEP_FULL;
        const bool zero_step = linesearch && ls[b].step_type == HSQP_STEP_ZERO;
        const bool metrics = fabs(rec.perf[b].merit - h->h_perf_before[b].merit) < h->ls_settings.cost_tol && ls_violation(rec.perf[b]) < h->ls_settings.g_min;
        const bool primal = rec.alpha[b] * ls[b].dxnorm < h->ls_settings.delta_tol && rec.alpha[b] * ls[b].dunorm < h->ls_settings.delta_tol;
        if (!zero_step && !metrics && !primal) converged = false;
      }
      h->iter_log.push_back(std::move(rec));
      float msi[4];
      for (int i = 0; i < 4; ++i) { HCHECK(hipEventElapsedTime(&msi[i], h->ev[i], h->ev[i + 1])); ms_sum[i] += msi[i]; }
    }
    const bool more = it + 1 < n_iterations && !converged;
    if (take_step && more) {
      HCHECK(hipMemcpyAsync(h->d_x, h->d_xnew, (size_t)B * (N + 1) * NX * 8, hipMemcpyDeviceToDevice, h->stream));
      HCHECK(hipMemcpyAsync(h->d_u, h->d_unew, (size_t)B * N * NU * 8, hipMemcpyDeviceToDevice, h->stream));
    }
  }
  HCHECK(hipGetLastError());
  HCHECK(hipStreamSynchronize(h->stream));
  if (until_converged) {
    for (int i = 0; i < 4; ++i) h->kernel_ms[i] = ms_sum[i];
  } else {
    float ms[4];
    for (int i = 0; i < 4; ++i) HCHECK(hipEventElapsedTime(&ms[i], h->ev[i], h->ev[i + 1]));
    for (int i = 0; i < 4; ++i) h->kernel_ms[i] = ms[i];
  }
  h->kernel_ms[4] = h->kernel_ms[0] + h->kernel_ms[1] + h->kernel_ms[2] + h->kernel_ms[3];
  h->have_solution = true;
  h->have_policy = true;
  h->have_value = want_value != 0;
  return HSQP_OK;
}

int hsqp_last_iterations(const hsqp_handle* h) { return h ? h->last_iterations : -1; }

int hsqp_iteration_log(const hsqp_handle* h, int iteration, hsqp_perf* perf, double* alpha, int32_t* step_type) {
  if (!h || iteration < 0 || iteration >= (int)h->iter_log.size()) return HSQP_ERR_BAD_ARG;
  const hsqp_handle::IterLog& r = h->iter_log[iteration];
  for (size_t b = 0; b < r.perf.size(); ++b) {
    if (perf) perf[b] = r.perf[b];
    if (alpha) alpha[b] = r.alpha[b];
    if (step_type) step_type[b] = r.type[b];
  }
  return HSQP_OK;
}

int hsqp_update_weights(hsqp_handle* h, const double* Q, const double* R, const double* Qf) {
  if (!h) return HSQP_ERR_BAD_ARG;
  h->have_value = false;   // (the record is the cost-to-go under the weights it was swept with)
  // explicit lengths (Q: 58, R: 35, Qf: 58; the same buffer may be passed twice) and the conditions build_dev_model (hsqp_create, hsqp_update_term_weights)
  // applies to them: state weights finite and >= 0, input weights finite and > 0 (the reduced Hessian
  // Lam = R~ + B~^T S B~ of every stage has to stay positive definite)
  const struct { const double* w; int n; bool positive; const char* name; } sets[3] = {{Q, NX, false, "Q"}, {R, NU, true, "R"}, {Qf, NX, false, "Qf"}};
  for (const auto& st : sets) {
    if (!st.w) continue;
    for (int i = 0; i < st.n; ++i) {
      const bool must_be_positive = st.positive;   // (both formulations use all 35 inputs)
      if (!std::isfinite(st.w[i]) || st.w[i] < 0.0 || (must_be_positive && !(st.w[i] > 0.0))) {
        h->err = std::string("hsqp_update_weights: ") + st.name + " must be finite and " + (st.positive ? "> 0" : ">= 0");
        return HSQP_ERR_BAD_ARG;
      }
    }
  }
  if (h->hdm.formulation == HSQP_FORM_CENTROIDAL)
    for (const double* w : {Q, Qf})
      for (int i = HSQP_CNX; w && i < NX; ++i)
        if (w[i] != 0.0) { h->err = "hsqp_update_weights: centroidal Q / Qf beyond the 35 centroidal states must be zero"; return HSQP_ERR_BAD_ARG; }
  HCHECK(hipSetDevice(h->device));
  if (Q) { memcpy(h->hdm.Q, Q, NX * 8); memcpy(h->md.Q, Q, NX * 8); }
  if (R) { memcpy(h->hdm.R, R, NU * 8); memcpy(h->md.R, R, NU * 8); }
  if (Qf) { memcpy(h->hdm.Qf, Qf, NX * 8); memcpy(h->md.Qf, Qf, NX * 8); }
  HCHECK(hipStreamSynchronize(h->stream));   // no kernel of an earlier call may still be reading the image
  HCHECK(hipMemcpy(h->d_dm, &h->hdm, sizeof(DevModel), hipMemcpyHostToDevice));
  return HSQP_OK;
}

int hsqp_get_term_weights(const hsqp_handle* h, hsqp_term_weights* out) {
  if (!h || !out) return HSQP_ERR_BAD_ARG;
  const hsqp_model_desc& m = h->md;
  memcpy(out->foot_sqrt_w, m.foot_sqrt_w, sizeof(out->foot_sqrt_w));
  out->gain_pos_z = m.gain_pos_z; out->gain_ori = m.gain_ori; out->gain_linvel_z = m.gain_linvel_z; out->gain_linvel_xy = m.gain_linvel_xy;
  out->gain_angvel = m.gain_angvel; out->gain_linacc_z = m.gain_linacc_z; out->gain_linacc_xy = m.gain_linacc_xy; out->gain_angacc = m.gain_angacc;
  out->friction_barrier = m.friction_barrier; out->moment_barrier = m.moment_barrier; out->joint_limit_barrier = m.joint_limit_barrier;
  out->collision_barrier = m.collision_barrier;
  memcpy(out->torso_sqrt_w, m.torso_sqrt_w, sizeof(out->torso_sqrt_w));
  memcpy(out->cent_foot_sqrt_w, m.cent_foot_sqrt_w, sizeof(out->cent_foot_sqrt_w));
  memcpy(out->ext_torque_sqrt_w, m.ext_torque_sqrt_w, sizeof(out->ext_torque_sqrt_w));
  return HSQP_OK;
}

int hsqp_update_term_weights(hsqp_handle* h, const hsqp_term_weights* w) {
  if (!h) return HSQP_ERR_BAD_ARG;
  h->have_value = false;
  if (!w) { h->err = "hsqp_update_term_weights: null argument"; return HSQP_ERR_BAD_ARG; }
  const double* all = reinterpret_cast<const double*>(w);
  for (size_t i = 0; i < sizeof(hsqp_term_weights) / sizeof(double); ++i)
    if (!std::isfinite(all[i])) { h->err = "hsqp_update_term_weights: every entry must be finite"; return HSQP_ERR_BAD_ARG; }
  // (the barrier parameters, weights and gains are validated by build_dev_model below: the same checks as hsqp_create)
  hsqp_model_desc m = h->md;
  memcpy(m.foot_sqrt_w, w->foot_sqrt_w, sizeof(m.foot_sqrt_w));
  m.gain_pos_z = w->gain_pos_z; m.gain_ori = w->gain_ori; m.gain_linvel_z = w->gain_linvel_z; m.gain_linvel_xy = w->gain_linvel_xy;
  m.gain_angvel = w->gain_angvel; m.gain_linacc_z = w->gain_linacc_z; m.gain_linacc_xy = w->gain_linacc_xy; m.gain_angacc = w->gain_angacc;
  m.friction_barrier = w->friction_barrier; m.moment_barrier = w->moment_barrier; m.joint_limit_barrier = w->joint_limit_barrier;
  m.collision_barrier = w->collision_barrier;
  memcpy(m.torso_sqrt_w, w->torso_sqrt_w, sizeof(m.torso_sqrt_w));
  memcpy(m.cent_foot_sqrt_w, w->cent_foot_sqrt_w, sizeof(m.cent_foot_sqrt_w));
  memcpy(m.ext_torque_sqrt_w, w->ext_torque_sqrt_w, sizeof(m.ext_torque_sqrt_w));
  DevModel dm;
  const std::string e = build_dev_model(m, dm);       // the validation of hsqp_create on the updated description
  if (!e.empty()) { h->err = "hsqp_update_term_weights: " + e; return HSQP_ERR_BAD_ARG; }
  HCHECK(hipSetDevice(h->device));
  HCHECK(hipStreamSynchronize(h->stream));   // no kernel of an earlier call may still be reading the image
  dm.has_default_joint_state = h->hdm.has_default_joint_state;   // (not part of hsqp_model_desc: hsqp_set_default_joint_state)
  memcpy(dm.default_joint_state, h->hdm.default_joint_state, sizeof(dm.default_joint_state));
  h->md = m; h->hdm = dm;
  HCHECK(hipMemcpy(h->d_dm, &h->hdm, sizeof(DevModel), hipMemcpyHostToDevice));
  return HSQP_OK;
}

static int download_impl(hsqp_handle* h, hsqp_solution* s, bool device_dst) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (!s || !h->have_solution) { h->err = "no solution on the device"; return HSQP_ERR_BAD_ARG; }
  if (device_dst && (s->alpha || s->step_type || s->armijo)) { h->err = "hsqp_download_device: alpha / step_type / armijo must be NULL (host-side fields)"; return HSQP_ERR_BAD_ARG; }
  HCHECK(hipSetDevice(h->device));
  const size_t B = h->B, N = h->N;
  const hipMemcpyKind kind = device_dst ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (s->x) HCHECK(hipMemcpy(s->x, h->d_xnew, B * (N + 1) * NX * 8, kind));
  if (s->u) HCHECK(hipMemcpy(s->u, h->d_unew, B * N * NU * 8, kind));
  if (s->dx) HCHECK(hipMemcpy(s->dx, h->d_dx, B * (N + 1) * NX * 8, kind));
  if (s->du) HCHECK(hipMemcpy(s->du, h->d_du, B * N * NU * 8, kind));
  if (s->perf_before) HCHECK(hipMemcpy(s->perf_before, h->d_perf_before, B * sizeof(hsqp_perf), kind));
  if (s->perf_after) HCHECK(hipMemcpy(s->perf_after, h->d_perf_after, B * sizeof(hsqp_perf), kind));
  if (s->kkt) HCHECK(hipMemcpy(s->kkt, h->d_kkt, B * 2 * 8, kind));
  if (s->grad_inf) HCHECK(hipMemcpy(s->grad_inf, h->gate.ginf, B * 8, kind));
  if (s->alpha || s->step_type || s->armijo) {
    std::vector<LsState> ls(B);
    HCHECK(hipMemcpy(ls.data(), h->d_ls, B * sizeof(LsState), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b) {
      if (s->alpha) s->alpha[b] = h->ls_ran ? ls[b].alpha : 1.0;
      if (s->step_type) s->step_type[b] = h->ls_ran ? ls[b].step_type : HSQP_STEP_FULL;
      if (s->armijo) s->armijo[b] = ls[b].armijo;
    }
  }
  std::vector<int> status(B);
  HCHECK(hipMemcpy(status.data(), h->d_status, B * sizeof(int), hipMemcpyDeviceToHost));
  s->timings.lq_approximation = 1e-3 * (h->kernel_ms[0] + h->kernel_ms[1]);
  s->timings.solve_qp = 1e-3 * h->kernel_ms[2];
  s->timings.linesearch = 1e-3 * h->kernel_ms[3];
  s->timings.compute_controller = 0.0;
  s->timings.total = 1e-3 * h->kernel_ms[4];
  return check_status(h, status);
}

int hsqp_download(hsqp_handle* h, hsqp_solution* s) { return download_impl(h, s, false); }
int hsqp_download_device(hsqp_handle* h, hsqp_solution* s) { return download_impl(h, s, true); }

int hsqp_host_register(void* buffer, size_t bytes) {
  if (!buffer || bytes == 0) return HSQP_ERR_BAD_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return HSQP_ERR_NO_DEVICE;
  return hipHostRegister(buffer, bytes, hipHostRegisterDefault) == hipSuccess ? HSQP_OK : ((void)hipGetLastError(), HSQP_ERR_HIP);
}
int hsqp_host_unregister(void* buffer) {
  if (!buffer) return HSQP_ERR_BAD_ARG;
  return hipHostUnregister(buffer) == hipSuccess ? HSQP_OK : ((void)hipGetLastError(), HSQP_ERR_HIP);
}

int hsqp_solve(hsqp_handle* h, const hsqp_problem* problem, hsqp_solution* solution) {
  int rc = hsqp_upload(h, problem);
  if (rc != HSQP_OK) return rc;
  // the KKT residual is a report, not part of the step: it is only computed when the caller asks for it (solution->kkt / grad_inf)
  const int want_kkt = (solution && (solution->kkt || solution->grad_inf)) ? HSQP_ITER_KKT : 0;
  rc = hsqp_iterate_device(h, 1, HSQP_ITER_TAKE_STEP | want_kkt | ((h->st.flags & HSQP_FLAG_LINESEARCH) ? HSQP_ITER_LINESEARCH : 0));
  if (rc != HSQP_OK) return rc;
  return hsqp_download(h, solution);
}

// x_meas (from_solution only; null: the feed-forward policy): the measured states of the feedback policy, whose input replaces the interpolated one
static int run_policy(hsqp_handle* h, int n, bool from_solution, const double* s_or_x, const double* u_in, const double* x_meas, double* x_out, double* u_out,
                      double* tau) {
  HCHECK(hipSetDevice(h->device));
  const bool cent = h->hdm.formulation == HSQP_FORM_CENTROIDAL;
  const size_t nin = from_solution ? (size_t)n * (x_meas ? 1 + NX : 1) : (size_t)n * (NX + NU);
  DEV_ENSURE(h->d_stage, policy_stage_layout(Carve{}, n, nin).bytes, "policy evaluation staging");
  const auto [d_in, d_x, d_u, d_tau, d_xw, d_uw, staged] = policy_stage_layout(Carve{h->d_stage.p}, n, nin);
  StickyError step{h};
  if (from_solution) {
    step(hipMemcpyAsync(d_in, s_or_x, (size_t)n * 8, hipMemcpyHostToDevice, h->stream), "upload s");
    if (x_meas) step(hipMemcpyAsync(d_in + n, x_meas, (size_t)n * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x_meas");
  } else {
    step(hipMemcpyAsync(d_in, s_or_x, (size_t)n * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x");
    step(hipMemcpyAsync(d_in + (size_t)n * NX, u_in, (size_t)n * NU * 8, hipMemcpyHostToDevice, h->stream), "upload u");
  }
  if (step.rc == HSQP_OK) {
    step(hipFuncSetAttribute((const void*)k_policy_torques, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(PolicyWS)), "hipFuncSetAttribute");
    if (from_solution)
      HSQP_LAUNCH(k_policy_inputs, dim3(n), dim3(64), 0, h->stream, (const double*)h->d_xnew, (const double*)h->d_unew, h->N, h->dt,
                         h->uniform_grid ? (const double*)nullptr : (const double*)h->d_dt, (const double*)d_in, (const double*)nullptr, (const double*)nullptr, d_x, d_u);
    else
      HSQP_LAUNCH(k_policy_inputs, dim3(n), dim3(64), 0, h->stream, (const double*)nullptr, (const double*)nullptr, 0, 0.0, (const double*)nullptr,
                         (const double*)nullptr, (const double*)d_in, (const double*)(d_in + (size_t)n * NX), d_x, d_u);
    if (from_solution && x_meas)
      HSQP_LAUNCH(k_feedback_eval, dim3(n), dim3(FB_THREADS), sizeof(FeedbackEvalWS), h->stream, (const double*)h->d_qp, (const double*)h->d_ric,
                         (const double*)h->d_xnew, (const double*)h->d_unew, (const double*)h->d_dt, h->N, h->dt, h->uniform_grid ? 1 : 0, cent ? 1 : 0,
                         (const double*)d_in, (const double*)(d_in + n), d_u);
    if (cent) {
      HSQP_LAUNCH(k_cent_policy_map, dim3(n), dim3(64), sizeof(CentWST<false>), h->stream, h->d_dm, n, (const double*)d_x, (const double*)d_u, d_xw, d_uw);
      HSQP_LAUNCH(k_policy_torques, dim3(n), dim3(128), sizeof(PolicyWS), h->stream, h->d_dm, (const double*)d_xw, (const double*)d_uw, d_tau);
    } else {
      HSQP_LAUNCH(k_policy_torques, dim3(n), dim3(128), sizeof(PolicyWS), h->stream, h->d_dm, (const double*)d_x, (const double*)d_u, d_tau);
    }
    step(hipGetLastError(), "k_policy");
  }
  if (x_out) step(hipMemcpyAsync(x_out, d_x, (size_t)n * NX * 8, hipMemcpyDeviceToHost, h->stream), "download x");
  if (u_out) step(hipMemcpyAsync(u_out, d_u, (size_t)n * NU * 8, hipMemcpyDeviceToHost, h->stream), "download u");
  if (tau) step(hipMemcpyAsync(tau, d_tau, (size_t)n * NJ * 8, hipMemcpyDeviceToHost, h->stream), "download tau");
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}

int hsqp_joint_torques(hsqp_handle* h, int n, const double* x, const double* u, double* tau) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (n < 1 || !x || !u || !tau) { h->err = "hsqp_joint_torques: n < 1 or null pointer"; return HSQP_ERR_BAD_ARG; }
  return run_policy(h, n, false, x, u, nullptr, nullptr, nullptr, tau);
}

int hsqp_evaluate_policy(hsqp_handle* h, const double* s, double* x, double* u, double* tau) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (!h->have_solution) { h->err = "no solution on the device"; return HSQP_ERR_BAD_ARG; }
  if (!s) { h->err = "hsqp_evaluate_policy: null time offsets"; return HSQP_ERR_BAD_ARG; }
  return run_policy(h, h->B, true, s, nullptr, nullptr, x, u, tau);
}

// ---- Riccati feedback policy (include/hsqp_feedback.h, csrc/hsqp_feedback.h)
// the policy of the resident solution can be formed: the last call that touched the records was a successful iteration, and no instance failed
static int feedback_ready(hsqp_handle* h, const char* who) {
  if (!h->have_policy) { h->err = std::string(who) + ": no feedback policy (no successful iteration since the last upload)"; return HSQP_ERR_BAD_ARG; }
  HCHECK(hipSetDevice(h->device));
  std::vector<int> status(h->B);
  HCHECK(hipMemcpy(status.data(), h->d_status, (size_t)h->B * sizeof(int), hipMemcpyDeviceToHost));
  return check_status(h, status);
}

static int feedback_policy_impl(hsqp_handle* h, int first, int count, double* K, double* uff, bool device_dst) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = device_dst ? "hsqp_feedback_policy_device" : "hsqp_feedback_policy";
  { const int rc = feedback_ready(h, who); if (rc != HSQP_OK) return rc; }
  if (first < 0 || count < 1 || count > h->N + 1 - first) {
    h->err = std::string(who) + ": window [first, first + count) outside the policy's entries [0, N]";
    return HSQP_ERR_BAD_ARG;
  }
  if (!K && !uff) return HSQP_OK;
  const size_t B = h->B, nK = B * count * NU * NX, nu = B * count * NU;
  double* dK = K;
  double* du = uff;
  if (!device_dst) {
    DEV_ENSURE(h->d_fb, ((K ? nK : 0) + (uff ? nu : 0)) * 8, "feedback policy staging");
    dK = K ? h->d_fb.p : nullptr;
    du = uff ? h->d_fb.p + (K ? nK : 0) : nullptr;
  }
  StickyError step{h};
  HSQP_LAUNCH(k_feedback_gains, dim3(count, B), dim3(FB_THREADS), sizeof(FeedbackWS), h->stream, (const double*)h->d_qp, (const double*)h->d_ric,
              (const double*)h->d_xnew, (const double*)h->d_unew, (const double*)h->d_dt, h->N, first, count,
              h->hdm.formulation == HSQP_FORM_CENTROIDAL ? 1 : 0, dK, du);
  step(hipGetLastError(), "k_feedback_gains");
  if (!device_dst) {
    if (K) step(hipMemcpyAsync(K, dK, nK * 8, hipMemcpyDeviceToHost, h->stream), "download K");
    if (uff) step(hipMemcpyAsync(uff, du, nu * 8, hipMemcpyDeviceToHost, h->stream), "download uff");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}

int hsqp_feedback_policy(hsqp_handle* h, int first, int count, double* K, double* uff) { return feedback_policy_impl(h, first, count, K, uff, false); }
int hsqp_feedback_policy_device(hsqp_handle* h, int first, int count, double* d_K, double* d_uff) { return feedback_policy_impl(h, first, count, d_K, d_uff, true); }

int hsqp_evaluate_feedback_policy(hsqp_handle* h, const double* s, const double* x_meas, double* x, double* u, double* tau) {
  if (!h) return HSQP_ERR_BAD_ARG;
  { const int rc = feedback_ready(h, "hsqp_evaluate_feedback_policy"); if (rc != HSQP_OK) return rc; }
  if (!s || !x_meas) { h->err = "hsqp_evaluate_feedback_policy: null time offsets or measured states"; return HSQP_ERR_BAD_ARG; }
  return run_policy(h, h->B, true, s, nullptr, x_meas, x, u, tau);
}

// ---- Riccati value function (include/hsqp_value.h, csrc/hsqp_value.h)
static int value_ready(hsqp_handle* h, const char* who) {
  if (!h->have_value || !h->vf_record) {
    h->err = std::string(who) + ": no value-function record (the last call that touched it was not a successful iteration with HSQP_ITER_VALUE_FUNCTION)";
    return HSQP_ERR_BAD_ARG;
  }
  return HSQP_OK;
}

static int value_function_impl(hsqp_handle* h, int k0, int k1, double* S, double* s, double* xbar, bool device_dst) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = device_dst ? "hsqp_value_function_device" : "hsqp_value_function";
  { const int rc = value_ready(h, who); if (rc != HSQP_OK) return rc; }
  if (k0 < 0 || k0 > k1 || k1 > h->N) { h->err = std::string(who) + ": nodes k0 .. k1 outside [0, N], or k0 > k1"; return HSQP_ERR_BAD_ARG; }
  if (!S && !s && !xbar) return HSQP_OK;
  HCHECK(hipSetDevice(h->device));
  const size_t B = h->B, count = (size_t)(k1 - k0 + 1), nS = B * count * NX * NX, nv = B * count * NX;
  double* dS = S; double* ds = s; double* dxb = xbar;
  if (!device_dst) {
    DEV_ENSURE(h->d_val, ((S ? nS : 0) + (s ? nv : 0) + (xbar ? nv : 0)) * 8, "value function staging");
    double* p = h->d_val.p;
    dS = S ? p : nullptr; p += S ? nS : 0;
    ds = s ? p : nullptr; p += s ? nv : 0;
    dxb = xbar ? p : nullptr;
  }
  StickyError step{h};
  HSQP_LAUNCH(k_value_record, dim3((unsigned)count, (unsigned)B), dim3(VAL_THREADS), sizeof(ValueWS), h->stream, h->vf_record, (const double*)h->d_xbar, h->N, k0, (int)count,
              h->hdm.formulation == HSQP_FORM_CENTROIDAL ? 1 : 0, dS, ds, dxb);
  step(hipGetLastError(), "k_value_record");
  if (!device_dst) {
    if (S) step(hipMemcpyAsync(S, dS, nS * 8, hipMemcpyDeviceToHost, h->stream), "download S");
    if (s) step(hipMemcpyAsync(s, ds, nv * 8, hipMemcpyDeviceToHost, h->stream), "download s");
    if (xbar) step(hipMemcpyAsync(xbar, dxb, nv * 8, hipMemcpyDeviceToHost, h->stream), "download xbar");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}

int hsqp_value_function(hsqp_handle* h, int k0, int k1, double* S, double* s, double* xbar) { return value_function_impl(h, k0, k1, S, s, xbar, false); }
int hsqp_value_function_device(hsqp_handle* h, int k0, int k1, double* d_S, double* d_s, double* d_xbar) { return value_function_impl(h, k0, k1, d_S, d_s, d_xbar, true); }

static int evaluate_value_impl(hsqp_handle* h, int n, const double* sq, const double* xq, double* dV, double* dfdx, double* dfdxx, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_evaluate_value_function_device" : "hsqp_evaluate_value_function";
  { const int rc = value_ready(h, who); if (rc != HSQP_OK) return rc; }
  if (n < 1) { h->err = std::string(who) + ": n_queries < 1"; return HSQP_ERR_BAD_ARG; }
  if (!sq || !xq) { h->err = std::string(who) + ": null s_query or x_query"; return HSQP_ERR_BAD_ARG; }
  const size_t B = h->B, nq = B * (size_t)n;
  if (!dev)
    for (size_t i = 0; i < nq; ++i)
      if (!std::isfinite(sq[i])) { h->err = std::string(who) + ": s_query must be finite"; return HSQP_ERR_BAD_ARG; }
  if (!dV && !dfdx && !dfdxx) return HSQP_OK;
  HCHECK(hipSetDevice(h->device));
  const double* d_sq = sq; const double* d_xq = xq;
  double* d_dV = dV; double* d_g = dfdx; double* d_H = dfdxx;
  StickyError step{h};
  if (!dev) {
    DEV_ENSURE(h->d_val, (nq + nq * NX + (dV ? nq : 0) + (dfdx ? nq * NX : 0) + (dfdxx ? nq * NX * NX : 0)) * 8, "value function staging");
    double* p = h->d_val.p;
    double* in_s = p; p += nq;
    double* in_x = p; p += nq * NX;
    d_dV = dV ? p : nullptr; p += dV ? nq : 0;
    d_g = dfdx ? p : nullptr; p += dfdx ? nq * NX : 0;
    d_H = dfdxx ? p : nullptr;
    step(hipMemcpyAsync(in_s, sq, nq * 8, hipMemcpyHostToDevice, h->stream), "upload s_query");
    step(hipMemcpyAsync(in_x, xq, nq * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x_query");
    d_sq = in_s; d_xq = in_x;
  }
  if (step.rc == HSQP_OK) {
    HSQP_LAUNCH(k_value_eval, dim3((unsigned)n, (unsigned)B), dim3(VAL_THREADS), sizeof(ValueWS), h->stream, h->vf_record, (const double*)h->d_xbar, (const double*)h->d_dt, h->N,
                h->dt, h->uniform_grid ? 1 : 0, h->hdm.formulation == HSQP_FORM_CENTROIDAL ? 1 : 0, n, d_sq, d_xq, d_dV, d_g, d_H);
    step(hipGetLastError(), "k_value_eval");
  }
  if (!dev) {
    if (dV) step(hipMemcpyAsync(dV, d_dV, nq * 8, hipMemcpyDeviceToHost, h->stream), "download dV");
    if (dfdx) step(hipMemcpyAsync(dfdx, d_g, nq * NX * 8, hipMemcpyDeviceToHost, h->stream), "download dfdx");
    if (dfdxx) step(hipMemcpyAsync(dfdxx, d_H, nq * NX * NX * 8, hipMemcpyDeviceToHost, h->stream), "download dfdxx");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}

int hsqp_evaluate_value_function(hsqp_handle* h, int n_queries, const double* s_query, const double* x_query, double* dV, double* dfdx, double* dfdxx) {
  return evaluate_value_impl(h, n_queries, s_query, x_query, dV, dfdx, dfdxx, false);
}
int hsqp_evaluate_value_function_device(hsqp_handle* h, int n_queries, const double* d_s_query, const double* d_x_query, double* d_dV, double* d_dfdx,
                                        double* d_dfdxx) {
  return evaluate_value_impl(h, n_queries, d_s_query, d_x_query, d_dV, d_dfdx, d_dfdxx, true);
}

// ---- batched policy rollout (include/hsqp_rollout.h, csrc/hsqp_rollout.h)
void hsqp_rollout_defaults(hsqp_rollout_settings* s) {
  if (!s) return;
  s->integrator = HSQP_ROLLOUT_ODE45;
  s->controller = HSQP_ROLLOUT_FEEDFORWARD;
  s->abs_tol = 1e-5;
  s->rel_tol = 1e-3;
  s->initial_step = 0.015;
  s->max_steps_per_second = 10000.0;
}

// what hsqp_rollout_policy refuses in its settings (null: nothing)
static const char* rollout_settings_error(const hsqp_rollout_settings& st) {
  const auto positive = [](double v) { return v > 0.0 && std::isfinite(v); };
  if (st.integrator != HSQP_ROLLOUT_ODE45 && st.integrator != HSQP_ROLLOUT_RK4) return "unknown integrator";
  if (st.controller != HSQP_ROLLOUT_FEEDFORWARD && st.controller != HSQP_ROLLOUT_FEEDBACK) return "unknown controller";
  if (!positive(st.abs_tol) || !positive(st.rel_tol) || !positive(st.initial_step) || !positive(st.max_steps_per_second))
    return "tolerances, initial_step and max_steps_per_second must be finite and > 0";
  return nullptr;
}

static int contact_params(hsqp_handle* h, ContactParams& cp);   // (below, with the entry points of include/hsqp_contact.h)
static int terrain_params(hsqp_handle* h, TerrainParams& tp);   // (below, with the entry points of include/hsqp_terrain.h)

// dev: every array argument is device memory of the handle's GPU
// per_instance (the isolated loop, include/hsqp_episode.h): an instance's status word — of the iteration, of the integration — is the instance's
// alone: it is written to `status`, not turned into the call's return code
static int rollout_impl(hsqp_handle* h, const hsqp_rollout_settings* st, const double* s0, const double* x0, double duration, int n, double* x, double* u,
                        int32_t* status, int32_t* steps, int32_t* rejected, bool dev, bool per_instance = false) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_rollout_policy_device" : "hsqp_rollout_policy";
  const auto bad = [&](const char* what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (!st || !s0 || !x0 || !status) return bad("null settings, s0, x0 or status");
  if (const char* what = rollout_settings_error(*st)) return bad(what);
  if (!(duration >= 0.0) || !std::isfinite(duration)) return bad("duration < 0 or not finite");
  if (n < 1) return bad("n_samples < 1");
  if (per_instance) { if (!h->have_policy) return bad("no feedback policy (no successful iteration since the last upload)"); }
  else { const int rc = feedback_ready(h, who); if (rc != HSQP_OK) return rc; }
  if (h->push_B && h->push_B != h->B)
    return bad(("the push table holds " + std::to_string(h->push_B) + " instances, the resident problem " + std::to_string(h->B) + " (hsqp_push_set / hsqp_push_clear)").c_str());
  const size_t B = h->B, nn = (size_t)n;
  const int N = h->N;
  const bool cent = h->hdm.formulation == HSQP_FORM_CENTROIDAL, feedback = st->controller == HSQP_ROLLOUT_FEEDBACK;
  DEV_ENSURE(h->d_ro, rollout_stage_layout(Carve{}, B, nn, !dev, x, u).bytes, "rollout staging");
  const RolloutStage sg = rollout_stage_layout(Carve{h->d_ro.p}, B, nn, !dev, x, u);
  int32_t* d_steps = dev ? steps : (steps ? sg.steps : nullptr);
  int32_t* d_rej = dev ? rejected : (rejected ? sg.rejected : nullptr);
  const double* d_s0 = dev ? s0 : sg.s0;
  const double* d_x0 = dev ? x0 : sg.x0;
  double* d_x = dev ? x : sg.x;
  double* d_u = dev ? u : sg.u;
  StickyError step{h};
  if (!dev) {
    step(hipMemcpyAsync(sg.s0, s0, B * 8, hipMemcpyHostToDevice, h->stream), "upload s0");
    step(hipMemcpyAsync(sg.x0, x0, B * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x0");
  }
  const double* dts = h->uniform_grid ? nullptr : (const double*)h->d_dt;
  // (the torque plant evaluates the policy up to `lookahead` past the call's last time: the gain window covers it)
  const bool torque = h->plant.kind == HSQP_PLANT_TORQUE;
  HSQP_LAUNCH(k_rollout_window, dim3(1), dim3(RO_WIN_THREADS), 0, h->stream, d_s0, (int)B, torque ? duration + h->plant.lookahead : duration, (const double*)h->d_dt, N, h->dt, h->uniform_grid ? 1 : 0, sg.win);
  step(hipGetLastError(), "k_rollout_window");
  int win[3] = {0, 0, 0};
  step(hipMemcpyAsync(win, sg.win, sizeof(win), hipMemcpyDeviceToHost, h->stream), "download window");
  step(hipStreamSynchronize(h->stream), "sync");
  if (step.rc != HSQP_OK) return step.rc;
  if (win[2]) return bad("non-finite s0");
  const int first = win[0], count = win[1] - win[0] + 1;
  if (first < 0 || count < 2 || first + count > N + 1) { h->err = std::string(who) + ": policy window out of range"; return HSQP_ERR_HIP; }
  double* dK = nullptr;
  double* duff = nullptr;
  if (feedback) {
    const size_t nK = B * count * NU * NX;
    DEV_ENSURE(h->d_ro_gain, (nK + B * count * NU) * 8, "rollout gain window");
    dK = h->d_ro_gain.p;
    duff = dK + nK;
    HSQP_LAUNCH(k_feedback_gains, dim3(count, B), dim3(FB_THREADS), sizeof(FeedbackWS), h->stream, (const double*)h->d_qp, (const double*)h->d_ric,
                (const double*)h->d_xnew, (const double*)h->d_unew, (const double*)h->d_dt, N, first, count, cent ? 1 : 0, dK, duff);
    step(hipGetLastError(), "k_feedback_gains");
  }
  PushTable pt{nullptr, nullptr, 0, nullptr, 0};
  if (h->push_B) {
    const PushBuf pb = push_layout(Carve{h->d_push.p}, h->push_B, h->push_max);
    pt = PushTable{pb.n, pb.p, h->push_max, h->stamps_resident ? (const double*)h->d_stamps[h->stamps_cur] : nullptr, N + 1};
  }
  const RolloutArgs a{h->d_unew, dts, N, h->dt, dK, duff, first, count, *st, d_s0, d_x0, duration, n, d_x, d_u, sg.status, d_steps, d_rej, pt};
  const RolloutVariant v(cent, torque, h->contact.enabled, h->actuator.enabled, h->inertia_B, !h->terrain_maps.empty(), h->terrain_B);
  ContactParams cp{nullptr, 0.0, 0.0, 0.0};
  if (v.ground) {
    const int rc = contact_params(h, cp);
    if (rc != HSQP_OK) return rc;
  }
  TerrainParams tp{nullptr, nullptr, nullptr, 0};
  if (v.terrain) {
    const int rc = terrain_params(h, tp);
    if (rc != HSQP_OK) return rc;
  }
  const PlantParams pp{torque ? (const double*)h->d_plant.p : nullptr, h->plant.lookahead, (const double*)h->d_xnew};
  ActuatorParams ap{nullptr, 0.0, 0.0, nullptr};
  if (v.actuated) {   // (hsqp_actuator_set made d_actuator)
    const ActuatorBuf ab = actuator_layout(Carve{h->d_actuator.p}, (size_t)h->st.max_batch);
    ap = ActuatorParams{ab.table, h->actuator.command_period, h->actuator.friction_velocity, ab.last};
    h->actuator_last_B = 0;              // (a failure below leaves no record)
  }
  // (hsqp_inertia_set_instances* made d_inertia)
  const InertiaParams ip{v.varied ? inertia_layout(Carve{h->d_inertia.p}, (size_t)h->st.max_batch).table : nullptr};
  rollout_dispatch(v, [&](auto stage) {
    using SW = typename decltype(stage)::type;
    static_assert(sizeof(RolloutWS<SW>) <= 65536, "the rollout runs without a dynamic-LDS attribute");
    if constexpr (RolloutOnPlant<SW>::value) HSQP_LAUNCH(k_rollout_plant<SW>, dim3(B), dim3(RO_THREADS), sizeof(RolloutWS<SW>), h->stream, h->d_dm, a, pp, cp, ap, ip, tp);
    else HSQP_LAUNCH(k_rollout<SW>, dim3(B), dim3(RO_THREADS), sizeof(RolloutWS<SW>), h->stream, h->d_dm, a);
  });
  step(hipGetLastError(), "k_rollout");
  std::vector<int32_t> hs(B);
  step(hipMemcpyAsync(hs.data(), sg.status, B * 4, hipMemcpyDeviceToHost, h->stream), "download status");
  if (dev) step(hipMemcpyAsync(status, sg.status, B * 4, hipMemcpyDeviceToDevice, h->stream), "copy status");
  else {
    if (x) step(hipMemcpyAsync(x, d_x, B * nn * NX * 8, hipMemcpyDeviceToHost, h->stream), "download x");
    if (u) step(hipMemcpyAsync(u, d_u, B * nn * NU * 8, hipMemcpyDeviceToHost, h->stream), "download u");
    if (steps) step(hipMemcpyAsync(steps, d_steps, B * 4, hipMemcpyDeviceToHost, h->stream), "download steps");
    if (rejected) step(hipMemcpyAsync(rejected, d_rej, B * 4, hipMemcpyDeviceToHost, h->stream), "download rejected");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  if (step.rc != HSQP_OK) return step.rc;
  if (ap.table) h->actuator_last_B = (int)B;
  if (!dev) memcpy(status, hs.data(), B * 4);
  if (per_instance) return HSQP_OK;
  int nonfinite = -1, capped = -1;
  for (size_t b = 0; b < B; ++b) {
    if (hs[b] == HSQP_ROLLOUT_NONFINITE && nonfinite < 0) nonfinite = (int)b;
    if (hs[b] == HSQP_ROLLOUT_MAX_STEPS && capped < 0) capped = (int)b;
  }
  if (nonfinite >= 0) { h->err = std::string(who) + ": instance " + std::to_string(nonfinite) + " produced a non-finite value"; return HSQP_ERR_NUMERIC; }
  if (capped >= 0) { h->err = std::string(who) + ": instance " + std::to_string(capped) + " hit the step cap"; return HSQP_ERR_NOT_CONVERGED; }
  return HSQP_OK;
}

int hsqp_rollout_policy(hsqp_handle* h, const hsqp_rollout_settings* st, const double* s0, const double* x0, double duration, int n_samples, double* x,
                        double* u, int32_t* status, int32_t* steps, int32_t* rejected) {
  return rollout_impl(h, st, s0, x0, duration, n_samples, x, u, status, steps, rejected, false);
}
int hsqp_rollout_policy_device(hsqp_handle* h, const hsqp_rollout_settings* st, const double* d_s0, const double* d_x0, double duration, int n_samples,
                               double* d_x, double* d_u, int32_t* d_status, int32_t* d_steps, int32_t* d_rejected) {
  return rollout_impl(h, st, d_s0, d_x0, duration, n_samples, d_x, d_u, d_status, d_steps, d_rejected, true);
}

// ---- external pushes on the plant (include/hsqp_push.h, csrc/hsqp_push.h): the resident table
static int push_set_impl(hsqp_handle* h, int batch, int max_pushes, const int32_t* n_pushes, const hsqp_push* pushes, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_push_set_device" : "hsqp_push_set";
  const auto bad = [&](const std::string& what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (!n_pushes || !pushes) return bad("null n_pushes or pushes");
  if (batch < 1 || batch > h->st.max_batch) return bad("batch outside [1, max_batch]");
  if (max_pushes < 1 || max_pushes > HSQP_PUSH_MAX) return bad("max_pushes outside [1, HSQP_PUSH_MAX]");
  if (!dev) {
    for (int b = 0; b < batch; ++b) {
      const std::string at = "instance " + std::to_string(b);
      if (n_pushes[b] < 0 || n_pushes[b] > max_pushes) return bad(at + ": n_pushes outside [0, max_pushes]");
      for (int i = 0; i < n_pushes[b]; ++i) {
        const hsqp_push& p = pushes[(size_t)b * max_pushes + i];
        const std::string pi = at + ", push " + std::to_string(i);
        if (p.body < 0 || p.body >= NB) return bad(pi + ": body outside the tree");
        if (p.reserved != 0) return bad(pi + ": reserved must be 0");
        bool finite = std::isfinite(p.t_start) && std::isfinite(p.duration);
        for (int k = 0; k < 3; ++k) finite = finite && std::isfinite(p.point[k]) && std::isfinite(p.force[k]);
        if (!finite)
          return bad(pi + ": non-finite t_start, duration, point or force");
        if (p.duration < 0.0) return bad(pi + ": negative duration");
      }
    }
  }
  HCHECK(hipSetDevice(h->device));
  h->push_B = 0;   // (a failure below leaves no table)
  DEV_ENSURE(h->d_push, push_layout(Carve{}, batch, max_pushes).bytes, "push table");
  const PushBuf pb = push_layout(Carve{h->d_push.p}, batch, max_pushes);
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  HCHECK(hipMemcpyAsync(pb.n, n_pushes, (size_t)batch * 4, kind, h->stream));
  HCHECK(hipMemcpyAsync(pb.p, pushes, (size_t)batch * max_pushes * sizeof(hsqp_push), kind, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  h->push_B = batch; h->push_max = max_pushes;
  return HSQP_OK;
}
int hsqp_push_set(hsqp_handle* h, int batch, int max_pushes, const int32_t* n_pushes, const hsqp_push* pushes) {
  return push_set_impl(h, batch, max_pushes, n_pushes, pushes, false);
}
int hsqp_push_set_device(hsqp_handle* h, int batch, int max_pushes, const int32_t* d_n_pushes, const hsqp_push* d_pushes) {
  return push_set_impl(h, batch, max_pushes, d_n_pushes, d_pushes, true);
}
int hsqp_push_clear(hsqp_handle* h) {
  if (!h) return HSQP_ERR_BAD_ARG;
  h->push_B = 0; h->push_max = 0;
  return HSQP_OK;
}
int hsqp_push_get(hsqp_handle* h, int* batch, int* max_pushes, int32_t* n_pushes, hsqp_push* pushes) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (!h->push_B) { h->err = "hsqp_push_get: no push table set"; return HSQP_ERR_BAD_ARG; }
  if (batch) *batch = h->push_B;
  if (max_pushes) *max_pushes = h->push_max;
  HCHECK(hipSetDevice(h->device));
  const PushBuf pb = push_layout(Carve{h->d_push.p}, h->push_B, h->push_max);
  if (n_pushes) HCHECK(hipMemcpyAsync(n_pushes, pb.n, (size_t)h->push_B * 4, hipMemcpyDeviceToHost, h->stream));
  if (pushes) HCHECK(hipMemcpyAsync(pushes, pb.p, (size_t)h->push_B * h->push_max * sizeof(hsqp_push), hipMemcpyDeviceToHost, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  return HSQP_OK;
}

// ---- the plant of the rollout (include/hsqp_plant.h, csrc/hsqp_plant.h): the resident setting
void hsqp_plant_defaults(hsqp_plant_settings* s) {
  if (!s) return;
  s->kind = HSQP_PLANT_TORQUE; s->reserved = 0;
  s->lookahead = 0.005;
  for (int j = 0; j < NJ; ++j) { s->kp[j] = 1200.0; s->kd[j] = 10.0; s->armature[j] = 0.0; }
}
int hsqp_plant_set(hsqp_handle* h, const hsqp_plant_settings* s) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const auto bad = [&](const char* what) { h->err = std::string("hsqp_plant_set: ") + what; return HSQP_ERR_BAD_ARG; };
  if (!s) return bad("null settings");
  if (h->hdm.formulation != HSQP_FORM_WB) return bad("whole-body handles only (the torque plant is the whole-body tree's forward dynamics)");
  if (s->kind != HSQP_PLANT_FLOW && s->kind != HSQP_PLANT_TORQUE) return bad("unknown kind");
  if (s->reserved != 0) return bad("reserved must be 0");
  const auto ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
  if (!ok(s->lookahead)) return bad("negative or non-finite lookahead");
  for (int j = 0; j < NJ; ++j)
    if (!ok(s->kp[j]) || !ok(s->kd[j]) || !ok(s->armature[j])) return bad(("joint " + std::to_string(j) + ": negative or non-finite kp, kd or armature").c_str());
  HCHECK(hipSetDevice(h->device));
  double g[3 * NJ];
  plant_pack_gains(*s, g);
  DEV_ENSURE(h->d_plant, sizeof(g), "plant gains");
  HCHECK(hipStreamSynchronize(h->stream));   // (no rollout in flight reads the gains that are replaced)
  HCHECK(hipMemcpy(h->d_plant.p, g, sizeof(g), hipMemcpyHostToDevice));
  h->plant = *s;
  return HSQP_OK;
}
int hsqp_plant_clear(hsqp_handle* h) {
  if (!h) return HSQP_ERR_BAD_ARG;
  hsqp_plant_defaults(&h->plant);
  h->plant.kind = HSQP_PLANT_FLOW;
  return HSQP_OK;
}
int hsqp_plant_get(hsqp_handle* h, hsqp_plant_settings* s) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (!s) { h->err = "hsqp_plant_get: null settings"; return HSQP_ERR_BAD_ARG; }
  *s = h->plant;
  return HSQP_OK;
}

// ---- the actuator model of the torque plant (include/hsqp_actuator.h, csrc/hsqp_actuator.h): the resident setting and the record of the last torques
void hsqp_actuator_defaults(hsqp_actuator_settings* s) {
  if (!s) return;
  s->enabled = 1; s->reserved = 0;
  s->command_period = 0.002;
  for (int j = 0; j < NJ; ++j) { s->effort_limit[j] = std::numeric_limits<double>::infinity(); s->damping[j] = 0.0; s->friction[j] = 0.0; }
  s->friction_velocity = 0.01;
}
int hsqp_actuator_set(hsqp_handle* h, const hsqp_actuator_settings* s) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const auto bad = [&](const std::string& what) { h->err = "hsqp_actuator_set: " + what; return HSQP_ERR_BAD_ARG; };
  if (!s) return bad("null settings");
  if (h->hdm.formulation != HSQP_FORM_WB) return bad("whole-body handles only (the actuator model acts on the torque plant of the whole-body tree)");
  if (s->reserved != 0) return bad("reserved must be 0");
  const auto ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
  if (!ok(s->command_period)) return bad("negative or non-finite command_period");
  for (int j = 0; j < NJ; ++j) {
    if (!(s->effort_limit[j] > 0.0)) return bad("joint " + std::to_string(j) + ": effort_limit <= 0 or NaN");
    if (!ok(s->damping[j])) return bad("joint " + std::to_string(j) + ": negative or non-finite damping");
    if (!ok(s->friction[j])) return bad("joint " + std::to_string(j) + ": negative or non-finite friction");
  }
  if (!(s->friction_velocity > 0.0) || !std::isfinite(s->friction_velocity)) return bad("friction_velocity <= 0 or non-finite");
  HCHECK(hipSetDevice(h->device));
  const size_t mb = (size_t)h->st.max_batch;
  double t[3 * NJ];
  actuator_pack_table(*s, t);
  DEV_ENSURE(h->d_actuator, actuator_layout(Carve{}, mb).bytes, "actuator table and record");
  HCHECK(hipStreamSynchronize(h->stream));   // (no rollout in flight reads the table that is replaced)
  HCHECK(hipMemcpy(actuator_layout(Carve{h->d_actuator.p}, mb).table, t, sizeof(t), hipMemcpyHostToDevice));
  h->actuator = *s;
  h->actuator_last_B = 0;
  return HSQP_OK;
}
int hsqp_actuator_clear(hsqp_handle* h) {
  if (!h) return HSQP_ERR_BAD_ARG;
  hsqp_actuator_defaults(&h->actuator);
  h->actuator.enabled = 0;
  h->actuator_last_B = 0;
  return HSQP_OK;
}
int hsqp_actuator_get(hsqp_handle* h, hsqp_actuator_settings* s) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (!s) { h->err = "hsqp_actuator_get: null settings"; return HSQP_ERR_BAD_ARG; }
  *s = h->actuator;
  return HSQP_OK;
}
static int actuator_last_impl(hsqp_handle* h, int batch, double* cmd, double* act, double* pas, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_actuator_last_device" : "hsqp_actuator_last";
  const auto bad = [&](const std::string& what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (!h->actuator_last_B) return bad("no rollout has run on the actuator model since it was set");
  if (batch != h->actuator_last_B) return bad("batch " + std::to_string(batch) + ", the last rollout on the actuator model had " + std::to_string(h->actuator_last_B));
  HCHECK(hipSetDevice(h->device));
  const double* last = actuator_layout(Carve{h->d_actuator.p}, (size_t)h->st.max_batch).last;
  double* const out[3] = {cmd, act, pas};
  for (int r = 0; r < 3; ++r)   // row r of every instance's record [3][NJ] into its own array [batch][NJ]
    if (out[r]) HCHECK(hipMemcpy2DAsync(out[r], NJ * 8, last + r * NJ, 3 * NJ * 8, NJ * 8, (size_t)batch, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  return HSQP_OK;
}
int hsqp_actuator_last(hsqp_handle* h, int batch, double* tau_cmd, double* tau_act, double* tau_passive) { return actuator_last_impl(h, batch, tau_cmd, tau_act, tau_passive, false); }
int hsqp_actuator_last_device(hsqp_handle* h, int batch, double* d_tau_cmd, double* d_tau_act, double* d_tau_passive) {
  return actuator_last_impl(h, batch, d_tau_cmd, d_tau_act, d_tau_passive, true);
}

// ---- the ground of the torque plant (include/hsqp_contact.h, csrc/hsqp_contact.h): the resident setting and the per-instance table
void hsqp_contact_defaults(const hsqp_handle* h, hsqp_contact_settings* s) {
  if (!s) return;
  s->enabled = 1; s->reserved = 0;
  s->stiffness = 5e4; s->damping = 10.0;
  s->mu = h ? h->hdm.friction_mu : std::numeric_limits<double>::quiet_NaN();
  s->slip_velocity = 0.01; s->ground_height = 0.0;
}
// makes d_contact hold the ground of every instance (entries from contact_B on: the setting's values) and gives the kernels' view of the setting
static int contact_params(hsqp_handle* h, ContactParams& cp) {
  const size_t mb = (size_t)h->st.max_batch;
  if (!h->contact_current) {
    HCHECK(hipSetDevice(h->device));
    DEV_ENSURE(h->d_contact, contact_layout(Carve{}, mb).bytes, "contact ground");
    std::vector<hsqp_contact_ground> fill(mb - (size_t)h->contact_B);   // (the table's own entries are resident already)
    contact_fill_ground(h->contact, nullptr, 0, fill.size(), fill.data());
    HCHECK(hipStreamSynchronize(h->stream));   // (no rollout in flight reads the entries that are replaced)
    if (!fill.empty())
      HCHECK(hipMemcpy(contact_layout(Carve{h->d_contact.p}, mb).ground + h->contact_B, fill.data(), fill.size() * sizeof(hsqp_contact_ground), hipMemcpyHostToDevice));
    h->contact_current = true;
  }
  cp = ContactParams{contact_layout(Carve{h->d_contact.p}, mb).ground, h->contact.stiffness, h->contact.damping, h->contact.slip_velocity};
  return HSQP_OK;
}
static int contact_handle_ok(hsqp_handle* h, const char* who) {
  if (h->hdm.formulation != HSQP_FORM_WB) { h->err = std::string(who) + ": whole-body handles only (the contact model acts on the torque plant of the whole-body tree)"; return HSQP_ERR_BAD_ARG; }
  return HSQP_OK;
}
int hsqp_contact_set(hsqp_handle* h, const hsqp_contact_settings* s) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const auto bad = [&](const char* what) { h->err = std::string("hsqp_contact_set: ") + what; return HSQP_ERR_BAD_ARG; };
  if (!s) return bad("null settings");
  if (const int rc = contact_handle_ok(h, "hsqp_contact_set")) return rc;
  if (s->reserved != 0) return bad("reserved must be 0");
  if (!std::isfinite(s->stiffness) || !std::isfinite(s->damping) || !std::isfinite(s->mu) || !std::isfinite(s->slip_velocity) || !std::isfinite(s->ground_height))
    return bad("non-finite stiffness, damping, mu, slip_velocity or ground_height");
  if (!(s->stiffness > 0.0)) return bad("stiffness must be > 0");
  if (s->damping < 0.0) return bad("damping must be >= 0");
  if (s->mu < 0.0) return bad("mu must be >= 0");
  if (!(s->slip_velocity > 0.0)) return bad("slip_velocity must be > 0");
  h->contact = *s;
  h->contact_current = false;
  ContactParams cp;
  return contact_params(h, cp);
}
static int contact_set_instances_impl(hsqp_handle* h, int batch, const hsqp_contact_ground* g, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_contact_set_instances_device" : "hsqp_contact_set_instances";
  const auto bad = [&](const std::string& what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (const int rc = contact_handle_ok(h, who)) return rc;
  if (g) {
    if (batch < 1 || batch > h->st.max_batch) return bad("batch outside [1, max_batch]");
    if (!dev)
      for (int b = 0; b < batch; ++b) {
        if (!std::isfinite(g[b].height) || !std::isfinite(g[b].mu)) return bad("instance " + std::to_string(b) + ": non-finite height or mu");
        if (g[b].mu < 0.0) return bad("instance " + std::to_string(b) + ": mu must be >= 0");
      }
  }
  HCHECK(hipSetDevice(h->device));
  h->contact_B = 0;   // (a failure below leaves no table)
  h->contact_current = false;
  if (g) {
    const size_t mb = (size_t)h->st.max_batch;
    DEV_ENSURE(h->d_contact, contact_layout(Carve{}, mb).bytes, "contact ground");
    HCHECK(hipStreamSynchronize(h->stream));
    HCHECK(hipMemcpy(contact_layout(Carve{h->d_contact.p}, mb).ground, g, (size_t)batch * sizeof(hsqp_contact_ground), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    h->contact_B = batch;
  }
  ContactParams cp;
  return contact_params(h, cp);
}
int hsqp_contact_set_instances(hsqp_handle* h, int batch, const hsqp_contact_ground* ground) { return contact_set_instances_impl(h, batch, ground, false); }
int hsqp_contact_set_instances_device(hsqp_handle* h, int batch, const hsqp_contact_ground* d_ground) { return contact_set_instances_impl(h, batch, d_ground, true); }
int hsqp_contact_clear(hsqp_handle* h) {
  if (!h) return HSQP_ERR_BAD_ARG;
  hsqp_contact_defaults(h, &h->contact);
  h->contact.enabled = 0;
  h->contact_B = 0;
  h->contact_current = false;
  return HSQP_OK;
}
int hsqp_contact_get(hsqp_handle* h, hsqp_contact_settings* s) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (!s) { h->err = "hsqp_contact_get: null settings"; return HSQP_ERR_BAD_ARG; }
  *s = h->contact;
  return HSQP_OK;
}
static int contact_eval_impl(hsqp_handle* h, int batch, const double* x, double* force, double* pen, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_contact_eval_device" : "hsqp_contact_eval";
  const auto bad = [&](const char* what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (!x) return bad("null states");
  if (const int rc = contact_handle_ok(h, who)) return rc;
  if (batch < 1 || batch > h->st.max_batch) return bad("batch outside [1, max_batch]");
  ContactParams cp;
  if (const int rc = contact_params(h, cp)) return rc;
  HCHECK(hipSetDevice(h->device));
  const size_t B = (size_t)batch;
  const double* d_x = x;
  double* d_f = force;
  double* d_p = pen;
  StickyError step{h};
  if (!dev) {
    DEV_ENSURE(h->d_contact_stage, contact_stage_layout(Carve{}, B, force, pen).bytes, "contact staging");
    const ContactStage sg = contact_stage_layout(Carve{h->d_contact_stage.p}, B, force, pen);
    d_x = sg.x; d_f = sg.force; d_p = sg.pen;
    step(hipMemcpyAsync(sg.x, x, B * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x");
  }
  TerrainParams tp{nullptr, nullptr, nullptr, 0};
  if (!h->terrain_maps.empty() && h->terrain_B) {   // (a terrain is resident: the model of include/hsqp_terrain.h)
    if (const int rc = terrain_params(h, tp)) return rc;
    HSQP_LAUNCH(k_contact_eval<ContactTerrainSet>, dim3(batch), dim3(RO_THREADS), sizeof(ContactEvalWST<ContactTerrainSet>), h->stream, h->d_dm, cp, tp, d_x, d_f, d_p);
  } else {
    HSQP_LAUNCH(k_contact_eval<ContactSet>, dim3(batch), dim3(RO_THREADS), sizeof(ContactEvalWS), h->stream, h->d_dm, cp, tp, d_x, d_f, d_p);
  }
  step(hipGetLastError(), "k_contact_eval");
  if (!dev) {
    if (force) step(hipMemcpyAsync(force, d_f, B * CT_PTS * 3 * 8, hipMemcpyDeviceToHost, h->stream), "download force");
    if (pen) step(hipMemcpyAsync(pen, d_p, B * CT_PTS * 8, hipMemcpyDeviceToHost, h->stream), "download penetration");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}
int hsqp_contact_eval(hsqp_handle* h, int batch, const double* x, double* force, double* penetration) { return contact_eval_impl(h, batch, x, force, penetration, false); }
int hsqp_contact_eval_device(hsqp_handle* h, int batch, const double* d_x, double* d_force, double* d_penetration) {
  return contact_eval_impl(h, batch, d_x, d_force, d_penetration, true);
}

// ---- height-map terrain under the ground of the torque plant (include/hsqp_terrain.h, csrc/hsqp_terrain.h): the resident maps, the placements, the evaluation
static int terrain_handle_ok(hsqp_handle* h, const char* who) {
  if (h->hdm.formulation != HSQP_FORM_WB) { h->err = std::string(who) + ": whole-body handles only (the terrain lies under the torque plant of the whole-body tree)"; return HSQP_ERR_BAD_ARG; }
  return HSQP_OK;
}
// makes d_terrain_place hold the placement of every instance (entries from terrain_B on: map = -1) and gives the kernels' view of the terrain (no maps:
// n_maps = 0, every instance on the plane)
static int terrain_params(hsqp_handle* h, TerrainParams& tp) {
  const size_t mb = (size_t)h->st.max_batch;
  if (!h->terrain_place_current || !h->d_terrain_place.p) {
    HCHECK(hipSetDevice(h->device));
    DEV_ENSURE(h->d_terrain_place, terrain_place_layout(Carve{}, mb).bytes, "terrain placements");
    std::vector<hsqp_terrain_placement> fill(mb - (size_t)h->terrain_B);   // (the table's own entries are resident already)
    terrain_fill_place(nullptr, 0, fill.size(), fill.data());
    HCHECK(hipStreamSynchronize(h->stream));   // (no rollout in flight reads the entries that are replaced)
    if (!fill.empty())
      HCHECK(hipMemcpy(terrain_place_layout(Carve{h->d_terrain_place.p}, mb).place + h->terrain_B, fill.data(), fill.size() * sizeof(hsqp_terrain_placement), hipMemcpyHostToDevice));
    h->terrain_place_current = true;
  }
  size_t heights = 0;
  for (const TerrainMap& m : h->terrain_maps) heights += (size_t)m.nx * m.ny;
  const TerrainMapsBuf mbuf = terrain_maps_layout(Carve{h->d_terrain_maps.p}, heights);
  const bool have = !h->terrain_maps.empty();
  tp = TerrainParams{have ? mbuf.maps : nullptr, have ? mbuf.pool : nullptr, terrain_place_layout(Carve{h->d_terrain_place.p}, mb).place, (int)h->terrain_maps.size()};
  return HSQP_OK;
}
int hsqp_terrain_set_maps(hsqp_handle* h, int n_maps, const int32_t* nx, const int32_t* ny, const double* cell, const double* heights) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_terrain_set_maps";
  const auto bad = [&](const std::string& what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (const int rc = terrain_handle_ok(h, who)) return rc;
  if (n_maps < 0 || n_maps > HSQP_TERRAIN_MAX_MAPS) return bad("n_maps outside [0, " + std::to_string(HSQP_TERRAIN_MAX_MAPS) + "]");
  if (n_maps && (!nx || !ny || !cell || !heights)) return bad("null nx, ny, cell or heights");
  if (h->terrain_B && n_maps <= h->terrain_top)
    return bad("the resident placement table refers to map " + std::to_string(h->terrain_top) + ", " + std::to_string(n_maps) + " maps given (hsqp_terrain_set_instances / hsqp_terrain_clear)");
  std::vector<TerrainMap> maps;
  size_t total = 0;
  for (int m = 0; m < n_maps; ++m) {
    const std::string at = "map " + std::to_string(m) + ": ";
    if (nx[m] < 2 || nx[m] > HSQP_TERRAIN_MAX_DIM || ny[m] < 2 || ny[m] > HSQP_TERRAIN_MAX_DIM) return bad(at + "nx or ny outside [2, " + std::to_string(HSQP_TERRAIN_MAX_DIM) + "]");
    if (!std::isfinite(cell[m]) || !(cell[m] > 0.0)) return bad(at + "cell not finite or <= 0");
    maps.push_back(TerrainMap{nx[m], ny[m], cell[m], total});
    const size_t cnt = (size_t)nx[m] * ny[m];
    for (size_t i = 0; i < cnt; ++i)
      if (!std::isfinite(heights[total + i])) return bad(at + "non-finite height");
    total += cnt;
  }
  HCHECK(hipSetDevice(h->device));
  HCHECK(hipStreamSynchronize(h->stream));   // (no rollout in flight reads the maps that are replaced)
  h->terrain_maps.clear();                   // (a failure below leaves no maps)
  if (!n_maps) {
    if (h->d_terrain_maps.p) { (void)hipFree(h->d_terrain_maps.p); h->d_terrain_maps.p = nullptr; h->d_terrain_maps.bytes = 0; }
    return HSQP_OK;
  }
  DEV_ENSURE(h->d_terrain_maps, terrain_maps_layout(Carve{}, total).bytes, "terrain maps");
  const TerrainMapsBuf mbuf = terrain_maps_layout(Carve{h->d_terrain_maps.p}, total);
  HCHECK(hipMemcpy(mbuf.maps, maps.data(), maps.size() * sizeof(TerrainMap), hipMemcpyHostToDevice));
  HCHECK(hipMemcpy(mbuf.pool, heights, total * sizeof(double), hipMemcpyHostToDevice));
  h->terrain_maps = std::move(maps);
  return HSQP_OK;
}
static int terrain_set_instances_impl(hsqp_handle* h, int batch, const hsqp_terrain_placement* pl, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_terrain_set_instances_device" : "hsqp_terrain_set_instances";
  const auto bad = [&](const std::string& what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (const int rc = terrain_handle_ok(h, who)) return rc;
  int top = -1;
  if (pl) {
    if (batch < 1 || batch > h->st.max_batch) return bad("batch outside [1, max_batch]");
    if (!dev)
      for (int b = 0; b < batch; ++b) {
        const std::string at = "instance " + std::to_string(b) + ": ";
        if (pl[b].reserved != 0) return bad(at + "reserved must be 0");
        if (pl[b].map < -1 || pl[b].map >= (int)h->terrain_maps.size()) return bad(at + "map outside [-1, n_maps) (" + std::to_string(h->terrain_maps.size()) + " maps resident)");
        if (!std::isfinite(pl[b].origin_x) || !std::isfinite(pl[b].origin_y) || !std::isfinite(pl[b].yaw)) return bad(at + "non-finite origin or yaw");
        top = pl[b].map > top ? pl[b].map : top;
      }
  } else if (batch < 0 || batch > h->st.max_batch) {
    return bad("batch outside [0, max_batch]");
  }
  HCHECK(hipSetDevice(h->device));
  if (pl) {
    const size_t mb = (size_t)h->st.max_batch;
    DEV_ENSURE(h->d_terrain_place, terrain_place_layout(Carve{}, mb).bytes, "terrain placements");
    HCHECK(hipStreamSynchronize(h->stream));
  }
  h->terrain_B = 0;   // (a failure below leaves no table)
  h->terrain_top = -1;
  h->terrain_place_current = false;
  if (pl) {
    HCHECK(hipMemcpy(terrain_place_layout(Carve{h->d_terrain_place.p}, (size_t)h->st.max_batch).place, pl, (size_t)batch * sizeof(hsqp_terrain_placement),
                     dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    h->terrain_B = batch;
    h->terrain_top = top;
  }
  TerrainParams tp;
  return terrain_params(h, tp);
}
int hsqp_terrain_set_instances(hsqp_handle* h, int batch, const hsqp_terrain_placement* place) { return terrain_set_instances_impl(h, batch, place, false); }
int hsqp_terrain_set_instances_device(hsqp_handle* h, int batch, const hsqp_terrain_placement* d_place) { return terrain_set_instances_impl(h, batch, d_place, true); }
int hsqp_terrain_clear(hsqp_handle* h) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (const int rc = terrain_handle_ok(h, "hsqp_terrain_clear")) return rc;
  h->terrain_B = 0;
  h->terrain_top = -1;
  h->terrain_place_current = false;
  return hsqp_terrain_set_maps(h, 0, nullptr, nullptr, nullptr, nullptr);
}
int hsqp_terrain_get_maps(hsqp_handle* h, int32_t* n_maps, int32_t* nx, int32_t* ny, double* cell, double* heights, size_t max_heights) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_terrain_get_maps";
  const auto bad = [&](const char* what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (const int rc = terrain_handle_ok(h, who)) return rc;
  if (!n_maps) return bad("null n_maps");
  size_t total = 0;
  for (const TerrainMap& m : h->terrain_maps) total += (size_t)m.nx * m.ny;
  if (heights && max_heights < total) return bad("max_heights is less than the resident maps hold");
  *n_maps = (int32_t)h->terrain_maps.size();
  for (size_t m = 0; m < h->terrain_maps.size(); ++m) {
    if (nx) nx[m] = h->terrain_maps[m].nx;
    if (ny) ny[m] = h->terrain_maps[m].ny;
    if (cell) cell[m] = h->terrain_maps[m].cell;
  }
  if (heights && total) {
    HCHECK(hipSetDevice(h->device));
    HCHECK(hipStreamSynchronize(h->stream));
    HCHECK(hipMemcpy(heights, terrain_maps_layout(Carve{h->d_terrain_maps.p}, total).pool, total * sizeof(double), hipMemcpyDeviceToHost));
  }
  return HSQP_OK;
}
int hsqp_terrain_get_instances(hsqp_handle* h, int batch, hsqp_terrain_placement* place) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_terrain_get_instances";
  const auto bad = [&](const char* what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (const int rc = terrain_handle_ok(h, who)) return rc;
  if (!place) return bad("null table");
  if (batch < 1 || batch > h->st.max_batch) return bad("batch outside [1, max_batch]");
  const int have = batch < h->terrain_B ? batch : h->terrain_B;
  if (have) {
    HCHECK(hipSetDevice(h->device));
    HCHECK(hipStreamSynchronize(h->stream));
    HCHECK(hipMemcpy(place, terrain_place_layout(Carve{h->d_terrain_place.p}, (size_t)h->st.max_batch).place, (size_t)have * sizeof(hsqp_terrain_placement), hipMemcpyDeviceToHost));
  }
  terrain_fill_place(nullptr, 0, (size_t)(batch - have), place + have);
  return HSQP_OK;
}
static int terrain_eval_impl(hsqp_handle* h, int batch, int n_pts, const double* xy, double* height, double* normal, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_terrain_eval_device" : "hsqp_terrain_eval";
  const auto bad = [&](const char* what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (const int rc = terrain_handle_ok(h, who)) return rc;
  if (!xy) return bad("null points");
  if (batch < 1 || batch > h->st.max_batch) return bad("batch outside [1, max_batch]");
  if (n_pts < 1 || n_pts > HSQP_TERRAIN_MAX_POINTS) return bad("n_pts outside [1, HSQP_TERRAIN_MAX_POINTS]");
  ContactParams cp;
  if (const int rc = contact_params(h, cp)) return rc;
  TerrainParams tp;
  if (const int rc = terrain_params(h, tp)) return rc;
  HCHECK(hipSetDevice(h->device));
  const size_t pts = (size_t)batch * (size_t)n_pts;
  const double* d_xy = xy;
  double* d_h = height;
  double* d_n = normal;
  StickyError step{h};
  if (!dev) {
    DEV_ENSURE(h->d_terrain_stage, terrain_stage_layout(Carve{}, pts, height, normal).bytes, "terrain staging");
    const TerrainStage sg = terrain_stage_layout(Carve{h->d_terrain_stage.p}, pts, height, normal);
    d_xy = sg.xy; d_h = sg.height; d_n = sg.normal;
    step(hipMemcpyAsync(sg.xy, xy, pts * 2 * 8, hipMemcpyHostToDevice, h->stream), "upload points");
  }
  HSQP_LAUNCH(k_terrain_eval, dim3(batch), dim3(RO_THREADS), 0, h->stream, cp, tp, n_pts, d_xy, d_h, d_n);
  step(hipGetLastError(), "k_terrain_eval");
  if (!dev) {
    if (height) step(hipMemcpyAsync(height, d_h, pts * 8, hipMemcpyDeviceToHost, h->stream), "download height");
    if (normal) step(hipMemcpyAsync(normal, d_n, pts * 3 * 8, hipMemcpyDeviceToHost, h->stream), "download normal");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}
int hsqp_terrain_eval(hsqp_handle* h, int batch, int n_pts, const double* xy, double* height, double* normal) { return terrain_eval_impl(h, batch, n_pts, xy, height, normal, false); }
int hsqp_terrain_eval_device(hsqp_handle* h, int batch, int n_pts, const double* d_xy, double* d_height, double* d_normal) {
  return terrain_eval_impl(h, batch, n_pts, d_xy, d_height, d_normal, true);
}

// ---- per-instance inertial variations of the torque plant (include/hsqp_inertia.h, csrc/hsqp_inertia.h): the resident table and the evaluation
void hsqp_inertia_defaults(hsqp_inertia_instance* v) {
  if (!v) return;
  memset(v, 0, sizeof(*v));
  for (int i = 0; i < NB; ++i) v->mass_scale[i] = 1.0;
}
static int inertia_handle_ok(hsqp_handle* h, const char* who) {
  if (h->hdm.formulation != HSQP_FORM_WB) { h->err = std::string(who) + ": whole-body handles only (the variations act on the torque plant of the whole-body tree)"; return HSQP_ERR_BAD_ARG; }
  return HSQP_OK;
}
// what is wrong with one entry ("" : nothing)
static std::string inertia_entry_error(const hsqp_inertia_instance& e) {
  for (int i = 0; i < NB; ++i)
    if (!(e.mass_scale[i] > 0.0) || !std::isfinite(e.mass_scale[i])) return "mass_scale[" + std::to_string(i) + "] <= 0 or non-finite";
  if (e.reserved != 0) return "reserved must be 0";
  if (e.n_payloads < 0 || e.n_payloads > HSQP_INERTIA_PAYLOADS) return "n_payloads outside [0, " + std::to_string(HSQP_INERTIA_PAYLOADS) + "]";
  for (int p = 0; p < e.n_payloads; ++p) {
    const hsqp_inertia_payload& pl = e.payload[p];
    const std::string at = "payload " + std::to_string(p) + ": ";
    if (pl.reserved != 0) return at + "reserved must be 0";
    if (pl.body < 0 || pl.body >= NB) return at + "body outside [0, " + std::to_string(NB) + ")";
    if (!(pl.mass >= 0.0) || !std::isfinite(pl.mass)) return at + "mass negative or non-finite";
    for (int k = 0; k < 3; ++k) if (!std::isfinite(pl.com[k])) return at + "com non-finite";
    for (int k = 0; k < 6; ++k) if (!std::isfinite(pl.inertia[k])) return at + "inertia non-finite";
    // positive semidefinite: every principal minor of [xx xy xz; xy yy yz; xz yz zz] is >= 0, up to the rounding of a rank-deficient tensor (a rod, a
    // plate) that was rotated into the link's axes: 16 eps of the scale tr^2 of a 2 x 2 minor, tr^3 of the determinant
    const double xx = pl.inertia[0], xy = pl.inertia[1], xz = pl.inertia[2], yy = pl.inertia[3], yz = pl.inertia[4], zz = pl.inertia[5];
    const double det = xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz) + xz * (xy * yz - yy * xz);
    const double tr = xx + yy + zz, slack = 16.0 * std::numeric_limits<double>::epsilon();
    const double m2 = -slack * tr * tr, m3 = -slack * tr * tr * tr;
    if (xx < 0.0 || yy < 0.0 || zz < 0.0 || xx * yy - xy * xy < m2 || xx * zz - xz * xz < m2 || yy * zz - yz * yz < m2 || det < m3)
      return at + "inertia not positive semidefinite";
  }
  return "";
}
static int inertia_set_instances_impl(hsqp_handle* h, int batch, const hsqp_inertia_instance* t, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_inertia_set_instances_device" : "hsqp_inertia_set_instances";
  const auto bad = [&](const std::string& what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (const int rc = inertia_handle_ok(h, who)) return rc;
  if (!t) {
    if (batch < 0 || batch > h->st.max_batch) return bad("batch outside [0, max_batch]");
    h->inertia_B = 0;
    return HSQP_OK;
  }
  if (batch < 1 || batch > h->st.max_batch) return bad("batch outside [1, max_batch]");
  if (!dev)
    for (int b = 0; b < batch; ++b) {
      const std::string what = inertia_entry_error(t[b]);
      if (!what.empty()) return bad("instance " + std::to_string(b) + ": " + what);
    }
  HCHECK(hipSetDevice(h->device));
  const size_t mb = (size_t)h->st.max_batch;
  DEV_ENSURE(h->d_inertia, inertia_layout(Carve{}, mb).bytes, "inertia table");
  hsqp_inertia_instance* d = inertia_layout(Carve{h->d_inertia.p}, mb).table;
  hsqp_inertia_instance neutral;
  hsqp_inertia_defaults(&neutral);
  const std::vector<hsqp_inertia_instance> fill(mb - (size_t)batch, neutral);
  HCHECK(hipStreamSynchronize(h->stream));   // (no rollout in flight reads the entries that are replaced)
  h->inertia_B = 0;                          // (a failure below leaves no table)
  HCHECK(hipMemcpy(d, t, (size_t)batch * sizeof(hsqp_inertia_instance), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  if (!fill.empty()) HCHECK(hipMemcpy(d + batch, fill.data(), fill.size() * sizeof(hsqp_inertia_instance), hipMemcpyHostToDevice));
  h->inertia_B = batch;
  return HSQP_OK;
}
int hsqp_inertia_set_instances(hsqp_handle* h, int batch, const hsqp_inertia_instance* table) { return inertia_set_instances_impl(h, batch, table, false); }
int hsqp_inertia_set_instances_device(hsqp_handle* h, int batch, const hsqp_inertia_instance* d_table) { return inertia_set_instances_impl(h, batch, d_table, true); }
int hsqp_inertia_clear(hsqp_handle* h) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (const int rc = inertia_handle_ok(h, "hsqp_inertia_clear")) return rc;
  h->inertia_B = 0;
  return HSQP_OK;
}
int hsqp_inertia_get_instances(hsqp_handle* h, int batch, hsqp_inertia_instance* table) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_inertia_get_instances";
  const auto bad = [&](const char* what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (const int rc = inertia_handle_ok(h, who)) return rc;
  if (!table) return bad("null table");
  if (batch < 1 || batch > h->st.max_batch) return bad("batch outside [1, max_batch]");
  const int have = batch < h->inertia_B ? batch : h->inertia_B;
  if (have) {
    HCHECK(hipSetDevice(h->device));
    HCHECK(hipStreamSynchronize(h->stream));
    HCHECK(hipMemcpy(table, inertia_layout(Carve{h->d_inertia.p}, (size_t)h->st.max_batch).table, (size_t)have * sizeof(hsqp_inertia_instance), hipMemcpyDeviceToHost));
  }
  for (int b = have; b < batch; ++b) hsqp_inertia_defaults(table + b);
  return HSQP_OK;
}
static int inertia_eval_impl(hsqp_handle* h, int batch, const double* x, double* M, double* nle, double* mass, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_inertia_eval_device" : "hsqp_inertia_eval";
  const auto bad = [&](const char* what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; };
  if (const int rc = inertia_handle_ok(h, who)) return rc;
  if (!x) return bad("null states");
  if (batch < 1 || batch > h->st.max_batch) return bad("batch outside [1, max_batch]");
  HCHECK(hipSetDevice(h->device));
  const InertiaParams ip{h->inertia_B ? inertia_layout(Carve{h->d_inertia.p}, (size_t)h->st.max_batch).table : nullptr};
  const size_t B = (size_t)batch;
  const double* d_x = x;
  double* d_M = M;
  double* d_n = nle;
  double* d_m = mass;
  StickyError step{h};
  if (!dev) {
    DEV_ENSURE(h->d_inertia_stage, inertia_stage_layout(Carve{}, B, M, nle, mass).bytes, "inertia staging");
    const InertiaStage sg = inertia_stage_layout(Carve{h->d_inertia_stage.p}, B, M, nle, mass);
    d_x = sg.x; d_M = sg.M; d_n = sg.nle; d_m = sg.mass;
    step(hipMemcpyAsync(sg.x, x, B * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x");
  }
  HSQP_LAUNCH(k_inertia_eval, dim3(batch), dim3(RO_THREADS), sizeof(InertiaEvalWS), h->stream, h->d_dm, ip, d_x, d_M, d_n, d_m);
  step(hipGetLastError(), "k_inertia_eval");
  if (!dev) {
    if (M) step(hipMemcpyAsync(M, d_M, B * NV * NV * 8, hipMemcpyDeviceToHost, h->stream), "download M");
    if (nle) step(hipMemcpyAsync(nle, d_n, B * NV * 8, hipMemcpyDeviceToHost, h->stream), "download nle");
    if (mass) step(hipMemcpyAsync(mass, d_m, B * 8, hipMemcpyDeviceToHost, h->stream), "download mass");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}
int hsqp_inertia_eval(hsqp_handle* h, int batch, const double* x, double* M, double* nle, double* mass) { return inertia_eval_impl(h, batch, x, M, nle, mass, false); }
int hsqp_inertia_eval_device(hsqp_handle* h, int batch, const double* d_x, double* d_M, double* d_nle, double* d_mass) {
  return inertia_eval_impl(h, batch, d_x, d_M, d_nle, d_mass, true);
}

static int loop_bad(hsqp_handle* h, const char* who, const char* what) { h->err = std::string(who) + ": " + what; return HSQP_ERR_BAD_ARG; }
// where the base pose starts in a state row of the handle's formulation (csrc/hsqp_episode.h: the triage's box, the stance command)
static int episode_pose_offset(const hsqp_handle* h) { return h->hdm.formulation == HSQP_FORM_CENTROIDAL ? EPISODE_POSE_CENT : EPISODE_POSE_WB; }
// whole-body handle with a default joint state
static int loop_handle_ok(hsqp_handle* h, const char* who) {
  if (h->hdm.formulation != HSQP_FORM_WB)
    return loop_bad(h, who, "whole-body handles only (the centroidal generator needs the base velocity from the centroidal momentum): hsqp_centroidal_command_targets, "
                            "hsqp_loop_start_centroidal (include/hsqp_cent_loop.h)");
  if (!h->hdm.has_default_joint_state) return loop_bad(h, who, "no default joint state: call hsqp_set_default_joint_state first");
  return HSQP_OK;
}
// centroidal handle with a default joint state (include/hsqp_cent_loop.h)
static int cent_loop_handle_ok(hsqp_handle* h, const char* who) {
  if (h->hdm.formulation != HSQP_FORM_CENTROIDAL) return loop_bad(h, who, "centroidal handles only (whole-body handles: the entry points of include/hsqp_loop.h)");
  if (!h->hdm.has_default_joint_state) return loop_bad(h, who, "no default joint state: call hsqp_set_default_joint_state first");
  return HSQP_OK;
}
// host state rows of a centroidal handle: the padding must be zero (the message of hsqp_upload)
static int cent_rows_padding_ok(hsqp_handle* h, const double* x, size_t rows) {
  for (size_t r = 0; r < rows; ++r)
    for (int i = HSQP_CNX; i < NX; ++i)
      if (x[r * NX + i] != 0.0) { h->err = "centroidal formulation: entries 35..57 of every state row must be zero"; return HSQP_ERR_BAD_ARG; }
  return HSQP_OK;
}
static bool all_finite(const double* v, size_t n) { for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false; return true; }

int hsqp_set_default_joint_state(hsqp_handle* h, const double* q) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (!q || !all_finite(q, NJ)) return loop_bad(h, "hsqp_set_default_joint_state", "null or non-finite joint state");
  HCHECK(hipSetDevice(h->device));
  memcpy(h->hdm.default_joint_state, q, NJ * 8);
  h->hdm.has_default_joint_state = 1;
  HCHECK(hipMemcpy(h->d_dm, &h->hdm, sizeof(DevModel), hipMemcpyHostToDevice));
  return HSQP_OK;
}

// queues k_command_targets on the handle's stream (device arrays)
static void launch_command_targets(hsqp_handle* h, int B, const double* d_v_cmd, double* d_v_filt, double alpha, const double* d_x0, double t0, double horizon,
                                   double* d_tt, double* d_ts) {
  HSQP_LAUNCH(k_command_targets, dim3((B * CMD_KNOTS + CMDT_THREADS - 1) / CMDT_THREADS), dim3(CMDT_THREADS), 0, h->stream, h->d_dm, alpha, d_v_cmd, d_v_filt, d_x0,
              t0, horizon, B, d_tt, d_ts);
}

// queues k_command_targets_cent on the handle's stream (device arrays; d_base_vel may be null)
static void launch_command_targets_cent(hsqp_handle* h, int B, const double* d_v_cmd, double* d_v_filt, double alpha, const double* d_x0, double t0, double horizon,
                                        double* d_tt, double* d_ts, double* d_base_vel) {
  HSQP_LAUNCH(k_command_targets_cent, dim3(B), dim3(64), sizeof(CentWST<false>), h->stream, h->d_dm, alpha, d_v_cmd, d_v_filt, d_x0, t0, horizon, d_tt, d_ts, d_base_vel);
}

// queues k_ground_estimate on the handle's stream (device arrays)
static void launch_ground_estimate(hsqp_handle* h, const GroundArgs& a) {
  HSQP_LAUNCH(k_ground_estimate, dim3((unsigned)((2 * (size_t)a.B + GROUND_THREADS - 1) / GROUND_THREADS)), dim3(GROUND_THREADS), 0, h->stream, h->d_dm, a);
}

// the resident terrain as k_foot_heights needs it: maps and a placement table (include/hsqp_perceive.h)
static int perceive_terrain_ok(hsqp_handle* h, const char* who) {
  if (h->terrain_maps.empty() || !h->terrain_B)
    return loop_bad(h, who, "no terrain resident: height maps and a placement table are needed (hsqp_terrain_set_maps, hsqp_terrain_set_instances)");
  return HSQP_OK;
}
// queues k_foot_heights on the handle's stream (device arrays), on the resident terrain and contact ground
static int launch_foot_heights(hsqp_handle* h, const char* who, const PerceiveArgs& a) {
  { const int rc = perceive_terrain_ok(h, who); if (rc != HSQP_OK) return rc; }
  ContactParams cp;
  if (const int rc = contact_params(h, cp)) return rc;
  TerrainParams tp;
  if (const int rc = terrain_params(h, tp)) return rc;
  HSQP_LAUNCH(k_foot_heights, dim3((unsigned)((2 * (size_t)a.B + PERCEIVE_THREADS - 1) / PERCEIVE_THREADS)), dim3(PERCEIVE_THREADS), 0, h->stream, h->d_dm, cp, tp, a);
  return HSQP_OK;
}

// cent: the centroidal entry points (include/hsqp_cent_loop.h); base_vel [B][6] is theirs and may be null
static int command_targets_impl(hsqp_handle* h, int batch, const double* v_cmd, double* v_filt, double alpha, const double* x0, double t0, double horizon,
                                double* tt, double* ts, bool dev, bool cent = false, double* base_vel = nullptr) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = cent ? (dev ? "hsqp_centroidal_command_targets_device" : "hsqp_centroidal_command_targets") : (dev ? "hsqp_command_targets_device" : "hsqp_command_targets");
  const char* kernel = cent ? "k_command_targets_cent" : "k_command_targets";
  { const int rc = cent ? cent_loop_handle_ok(h, who) : loop_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  if (!v_cmd || !v_filt || !x0 || !tt || !ts) return loop_bad(h, who, "null array");
  if (batch < 1 || batch > h->st.max_batch) return loop_bad(h, who, "batch outside [1, max_batch]");
  if (!(alpha >= 0.0 && alpha < 1.0)) return loop_bad(h, who, "filter_alpha outside [0, 1)");
  if (!std::isfinite(t0) || !std::isfinite(horizon) || !(horizon > 0.0)) return loop_bad(h, who, "t0 not finite, or horizon not finite and > 0");
  const size_t B = batch;
  if (!dev && !all_finite(v_cmd, B * CMD_N)) return loop_bad(h, who, "non-finite command");
  if (!dev && cent) { const int rc = cent_rows_padding_ok(h, x0, B); if (rc != HSQP_OK) return rc; }
  HCHECK(hipSetDevice(h->device));
  StickyError step{h};
  if (dev) {
    if (cent) launch_command_targets_cent(h, batch, v_cmd, v_filt, alpha, x0, t0, horizon, tt, ts, base_vel);
    else launch_command_targets(h, batch, v_cmd, v_filt, alpha, x0, t0, horizon, tt, ts);
    step(hipGetLastError(), kernel);
  } else {
    DEV_ENSURE(h->d_loop_log, command_stage_layout(Carve{}, B, base_vel != nullptr).bytes, "command-target staging");
    const CommandStage sg = command_stage_layout(Carve{h->d_loop_log.p}, B, base_vel != nullptr);
    step(hipMemcpyAsync(sg.v_cmd, v_cmd, B * CMD_N * 8, hipMemcpyHostToDevice, h->stream), "upload v_cmd");
    step(hipMemcpyAsync(sg.v_filt, v_filt, B * CMD_N * 8, hipMemcpyHostToDevice, h->stream), "upload v_filt");
    step(hipMemcpyAsync(sg.x0, x0, B * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x0");
    if (step.rc == HSQP_OK) {
      if (cent) launch_command_targets_cent(h, batch, sg.v_cmd, sg.v_filt, alpha, sg.x0, t0, horizon, sg.tt, sg.ts, sg.base_vel);
      else launch_command_targets(h, batch, sg.v_cmd, sg.v_filt, alpha, sg.x0, t0, horizon, sg.tt, sg.ts);
      step(hipGetLastError(), kernel);
    }
    if (base_vel) step(hipMemcpyAsync(base_vel, sg.base_vel, B * 6 * 8, hipMemcpyDeviceToHost, h->stream), "download base_vel");
    step(hipMemcpyAsync(v_filt, sg.v_filt, B * CMD_N * 8, hipMemcpyDeviceToHost, h->stream), "download v_filt");
    step(hipMemcpyAsync(tt, sg.tt, B * CMD_KNOTS * 8, hipMemcpyDeviceToHost, h->stream), "download target_times");
    step(hipMemcpyAsync(ts, sg.ts, B * CMD_KNOTS * NX * 8, hipMemcpyDeviceToHost, h->stream), "download target_states");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}

int hsqp_command_targets(hsqp_handle* h, int batch, const double* v_cmd, double* v_filt, double filter_alpha, const double* x0, double t0, double horizon,
                         double* target_times, double* target_states) {
  return command_targets_impl(h, batch, v_cmd, v_filt, filter_alpha, x0, t0, horizon, target_times, target_states, false);
}
int hsqp_command_targets_device(hsqp_handle* h, int batch, const double* d_v_cmd, double* d_v_filt, double filter_alpha, const double* d_x0, double t0,
                                double horizon, double* d_target_times, double* d_target_states) {
  return command_targets_impl(h, batch, d_v_cmd, d_v_filt, filter_alpha, d_x0, t0, horizon, d_target_times, d_target_states, true);
}

int hsqp_centroidal_command_targets(hsqp_handle* h, int batch, const double* v_cmd, double* v_filt, double filter_alpha, const double* x0, double t0,
                                    double horizon, double* target_times, double* target_states, double* base_vel) {
  return command_targets_impl(h, batch, v_cmd, v_filt, filter_alpha, x0, t0, horizon, target_times, target_states, false, true, base_vel);
}
int hsqp_centroidal_command_targets_device(hsqp_handle* h, int batch, const double* d_v_cmd, double* d_v_filt, double filter_alpha, const double* d_x0,
                                           double t0, double horizon, double* d_target_times, double* d_target_states, double* d_base_vel) {
  return command_targets_impl(h, batch, d_v_cmd, d_v_filt, filter_alpha, d_x0, t0, horizon, d_target_times, d_target_states, true, true, d_base_vel);
}

// (on a centroidal handle too: the values are the whole-body task file's, include/hsqp_cent_loop.h)
void hsqp_loop_defaults(const hsqp_handle* h, hsqp_loop_settings* s) {
  if (!s) return;
  memset(s, 0, sizeof(*s));
  s->period = 1.0 / 60.0;     // task.info mpcDesiredFrequency 60
  s->filter_alpha = 0.8;      // WBMpcTargetTrajectoriesCalculator.cpp:88
  s->n_nodes = h ? std::min(100, h->st.max_nodes) : 100;
  s->dt = 0.035;              // task.info sqp dt
  s->iterations = 1;          // task.info sqpIteration 1
  s->iterate_flags = HSQP_ITER_TAKE_STEP | HSQP_ITER_LINESEARCH;
  s->arm_swing = 1;
  hsqp_rollout_defaults(&s->rollout);
  s->swing = hsqp_swing_config{0.05, -0.0, 0.08, -0.001, 0.4, 0.005, -0.15, 0.3};   // task.info swing_trajectory_config
  s->terrain_height = 0.0;
}

static int gait_reset_impl(hsqp_handle* h, const char* who, const hsqp_gait_settings* gs, int batch, double t0);
static bool observe_in_force(const hsqp_handle* h);

// hsqp_loop_start (schedules uploaded once) and hsqp_loop_start_gait (gait != null: the resident gait state owns the schedule, max_events is its capacity)
// cent: hsqp_loop_start_centroidal (include/hsqp_cent_loop.h), never with a gait
static int loop_start_impl(hsqp_handle* h, const char* who, const hsqp_loop_settings* st, const hsqp_gait_settings* gait, int batch, double t0, const double* x0,
                           const double* v_cmd, int max_events, const int32_t* n_events, const double* event_times, const int32_t* mode_sequence, bool cent = false) {
  if (!h) return HSQP_ERR_BAD_ARG;
  h->loop.started = false;
  { const int rc = cent ? cent_loop_handle_ok(h, who) : loop_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  if (!st || !x0 || !v_cmd || (!gait && (!n_events || !event_times || !mode_sequence))) return loop_bad(h, who, "null settings or array");
  if (batch < 1 || batch > h->st.max_batch) return loop_bad(h, who, "batch outside [1, max_batch]");
  if (st->n_nodes < 1 || st->n_nodes > h->st.max_nodes) return loop_bad(h, who, "n_nodes outside [1, max_nodes]");
  const auto positive = [](double v) { return v > 0.0 && std::isfinite(v); };
  if (!positive(st->period) || !positive(st->dt)) return loop_bad(h, who, "period and dt must be finite and > 0");
  if (!(st->filter_alpha >= 0.0 && st->filter_alpha < 1.0)) return loop_bad(h, who, "filter_alpha outside [0, 1)");
  if (st->iterations < 1) return loop_bad(h, who, "iterations < 1");
  if (st->iterate_flags & ~(HSQP_ITER_TAKE_STEP | HSQP_ITER_KKT | HSQP_ITER_LINESEARCH))
    return loop_bad(h, who, "iterate_flags: HSQP_ITER_TAKE_STEP, HSQP_ITER_KKT, HSQP_ITER_LINESEARCH only (HSQP_ITER_UNTIL_CONVERGED reads B-sized records back per iteration)");
  if (const char* what = rollout_settings_error(st->rollout)) return loop_bad(h, who, what);
  if (!std::isfinite(t0)) return loop_bad(h, who, "t0 not finite");
  if (max_events < 1) return loop_bad(h, who, "max_events < 1");
  const size_t B = batch, E = max_events;
  if (!gait)
    for (size_t b = 0; b < B; ++b)
      if (n_events[b] < 1 || n_events[b] > max_events) return loop_bad(h, who, "n_events outside [1, max_events]");
  if (!all_finite(v_cmd, B * CMD_N)) return loop_bad(h, who, "non-finite command");
  if (cent) { const int rc = cent_rows_padding_ok(h, x0, B); if (rc != HSQP_OK) return rc; }
  HCHECK(hipSetDevice(h->device));
  // the gait's clock is the problem time (include/hsqp_observe.h): compute_delay periods behind the loop's time
  const double t_gait = observe_in_force(h) ? observe_problem_time(t0, observe_policy_time(h->observe.compute_delay, st->period)) : t0;
  if (gait) { const int rc = gait_reset_impl(h, who, gait, batch, t_gait); if (rc != HSQP_OK) return rc; }
  hsqp_handle::Loop& L = h->loop;
  DEV_ENSURE(h->d_loop, loop_layout(Carve{}, L, B, E), "loop buffers");
  loop_layout(Carve{h->d_loop.p}, L, B, E);
  StickyError step{h};
  if (!gait) {
    step(hipMemcpyAsync(L.ne, n_events, B * 4, hipMemcpyHostToDevice, h->stream), "upload n_events");
    step(hipMemcpyAsync(L.seq, mode_sequence, B * (E + 1) * 4, hipMemcpyHostToDevice, h->stream), "upload mode_sequence");
    step(hipMemcpyAsync(L.ev, event_times, B * E * 8, hipMemcpyHostToDevice, h->stream), "upload event_times");
  }
  step(hipMemcpyAsync(L.v_cmd, v_cmd, B * CMD_N * 8, hipMemcpyHostToDevice, h->stream), "upload v_cmd");
  step(hipMemcpyAsync(L.v_filt, v_cmd, B * CMD_N * 8, hipMemcpyHostToDevice, h->stream), "upload v_filt");
  step(hipMemcpyAsync(L.x, x0, B * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x0");
  step(hipMemsetAsync(L.s0, 0, B * 8, h->stream), "memset s0");
  step(hipStreamSynchronize(h->stream), "sync");
  if (step.rc != HSQP_OK) return step.rc;
  L.st = *st; L.B = batch; L.E = max_events; L.t = t0;
  L.have_cycle = false;
  L.cycle = 0;
  L.obs_last = false;
  L.isolate = false;
  L.metrics = false; L.metrics_made = false;
  L.grid = false; L.grid_have = false;
  L.ground = false;
  L.perceive = false;
  L.gait = gait != nullptr;
  L.started = true;
  return HSQP_OK;
}

int hsqp_loop_start(hsqp_handle* h, const hsqp_loop_settings* st, int batch, double t0, const double* x0, const double* v_cmd, int max_events,
                    const int32_t* n_events, const double* event_times, const int32_t* mode_sequence) {
  return loop_start_impl(h, "hsqp_loop_start", st, nullptr, batch, t0, x0, v_cmd, max_events, n_events, event_times, mode_sequence);
}

int hsqp_loop_start_centroidal(hsqp_handle* h, const hsqp_loop_settings* st, int batch, double t0, const double* x0, const double* v_cmd, int max_events,
                               const int32_t* n_events, const double* event_times, const int32_t* mode_sequence) {
  return loop_start_impl(h, "hsqp_loop_start_centroidal", st, nullptr, batch, t0, x0, v_cmd, max_events, n_events, event_times, mode_sequence, true);
}

static int loop_started(hsqp_handle* h, const char* who) {
  if (!h->loop.started) return loop_bad(h, who, "no loop started (hsqp_loop_start; every hsqp_upload* / hsqp_solve call ends a loop)");
  return HSQP_OK;
}

static int loop_command_impl(hsqp_handle* h, const double* v_cmd, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_loop_command_device" : "hsqp_loop_command";
  { const int rc = loop_started(h, who); if (rc != HSQP_OK) return rc; }
  if (!v_cmd) return loop_bad(h, who, "null commands");
  const size_t n = (size_t)h->loop.B * CMD_N;
  if (!dev && !all_finite(v_cmd, n)) return loop_bad(h, who, "non-finite command");
  HCHECK(hipSetDevice(h->device));
  HCHECK(hipMemcpyAsync(h->loop.v_cmd, v_cmd, n * 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
  if (h->loop.isolate) {   // the command in use: a parked instance keeps the stance command
    HSQP_LAUNCH(k_episode_commands, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, h->stream, h->loop.ep.state, h->loop.v_cmd, h->loop.x_reset, h->loop.B, h->loop.v_use,
                episode_pose_offset(h));
    HCHECK(hipGetLastError());
  }
  HCHECK(hipStreamSynchronize(h->stream));
  return HSQP_OK;
}
int hsqp_loop_command(hsqp_handle* h, const double* v_cmd) { return loop_command_impl(h, v_cmd, false); }
int hsqp_loop_command_device(hsqp_handle* h, const double* d_v_cmd) { return loop_command_impl(h, d_v_cmd, true); }

// ---- per-instance gait schedule and ladder (include/hsqp_gait.h, csrc/hsqp_gait.h)
static const char* gait_settings_error(const hsqp_gait_settings& g, std::string& text) {
  if (g.n_rungs < 1 || g.n_rungs > HSQP_GAIT_MAX_RUNGS) return "n_rungs outside [1, HSQP_GAIT_MAX_RUNGS]";
  if (g.max_events < 2 || g.max_events > HSQP_GAIT_MAX_EVENTS) return "max_events outside [2, HSQP_GAIT_MAX_EVENTS]";
  if (!std::isfinite(g.phase_transition_stance_time) || g.phase_transition_stance_time < 0.0) return "phase_transition_stance_time not finite and >= 0";
  if (!std::isfinite(g.min_change_interval) || g.min_change_interval < 0.0) return "min_change_interval not finite and >= 0";
  for (int r = 0; r < g.n_rungs; ++r) {
    const hsqp_gait_rung& c = g.rungs[r];
    const std::string name(c.name, strnlen(c.name, HSQP_GAIT_NAME_LEN));
    const std::string where = "rung " + std::to_string(r) + " (" + name + "): ";
    const double th[6] = {c.min_lin_vel_cmd, c.max_lin_vel_cmd, c.min_ang_vel_cmd, c.max_ang_vel_cmd, c.lin_vel_error_thresh, c.ang_vel_error_thresh};
    for (double v : th) if (!std::isfinite(v)) { text = where + "non-finite threshold"; return text.c_str(); }
    if (c.n_phases < 1 || c.n_phases > HSQP_GAIT_MAX_PHASES) { text = where + "n_phases outside [1, HSQP_GAIT_MAX_PHASES]"; return text.c_str(); }
    for (int i = 0; i < c.n_phases; ++i)
      if (c.modes[i] < HSQP_MODE_FLY || c.modes[i] > HSQP_MODE_STANCE) { text = where + "mode outside 0 .. 3"; return text.c_str(); }
    for (int i = 0; i <= c.n_phases; ++i) if (!std::isfinite(c.switching_times[i])) { text = where + "non-finite switching time"; return text.c_str(); }
    for (int i = 0; i < c.n_phases; ++i)
      if (!(c.switching_times[i + 1] > c.switching_times[i])) {
        text = where + "switching times not strictly increasing (" + std::to_string(c.switching_times[i]) + " is followed by " + std::to_string(c.switching_times[i + 1]) +
               "; gait.info's skip is such a template)";
        return text.c_str();
      }
  }
  return nullptr;
}

void hsqp_gait_ladder_defaults(hsqp_gait_settings* s) {
  if (!s) return;
  memset(s, 0, sizeof(*s));
  // ProceduralMpcMotionManager.h:110-118
  static const struct { const char* name; double v[6]; } rows[7] = {
      {"stance", {-0.1, 0.1, -0.1, 0.1, 10.0, 10.0}},   {"slow_walk", {0.05, 0.3, 0.05, 0.2, 0.05, 0.05}}, {"walk", {0.25, 0.5, 0.15, 0.35, 0.05, 0.05}},
      {"slower_trot", {0.45, 0.7, 0.3, 0.55, 0.1, 0.1}}, {"slow_trot", {0.65, 0.9, 0.5, 0.7, 0.2, 0.2}},   {"trot", {0.8, 1.3, 0.65, 10.0, 0.2, 0.2}},
      {"run", {1.2, 10.0, 0.65, 10.0, 0.2, 0.2}}};
  s->n_rungs = 7;
  s->max_events = 128;
  s->phase_transition_stance_time = 0.0;   // task.info phaseTransitionStanceTime
  s->min_change_interval = 0.2;            // ProceduralMpcMotionManager.cpp:134
  for (int r = 0; r < 7; ++r) {
    hsqp_gait_rung& c = s->rungs[r];
    c.min_lin_vel_cmd = rows[r].v[0]; c.max_lin_vel_cmd = rows[r].v[1]; c.min_ang_vel_cmd = rows[r].v[2]; c.max_ang_vel_cmd = rows[r].v[3];
    c.lin_vel_error_thresh = rows[r].v[4]; c.ang_vel_error_thresh = rows[r].v[5];
    strncpy(c.name, rows[r].name, HSQP_GAIT_NAME_LEN - 1);
  }
}

static int gait_handle_ok(hsqp_handle* h, const char* who) {
  if (h->hdm.formulation != HSQP_FORM_WB) return loop_bad(h, who, "whole-body handles only (the ladder reads the base velocity from the whole-body state)");
  return HSQP_OK;
}

// the initial state of `batch` instances at t0, in both copies' place (the live one is copy 0)
static int gait_reset_impl(hsqp_handle* h, const char* who, const hsqp_gait_settings* gs, int batch, double t0) {
  h->gait.ready = false;
  { const int rc = gait_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  if (!gs) return loop_bad(h, who, "null gait settings");
  if (batch < 1 || batch > h->st.max_batch) return loop_bad(h, who, "batch outside [1, max_batch]");
  if (!std::isfinite(t0)) return loop_bad(h, who, "t0 not finite");
  { std::string text; if (const char* what = gait_settings_error(*gs, text)) return loop_bad(h, who, what); }
  HCHECK(hipSetDevice(h->device));
  const size_t B = batch, E = gs->max_events;
  hsqp_handle::Gait& G = h->gait;
  DEV_ENSURE(h->d_gait, gait_layout(Carve{}, G, B, E), "gait state");
  gait_layout(Carve{h->d_gait.p}, G, B, E);
  // reference.info initialModeSchedule {[0.5], [STANCE, STANCE]} offset by t0; rung 0, its template, both gait commands rung 0
  std::vector<int> n(B, 1), seq(B * (E + 1), HSQP_MODE_STANCE), scal(B * GAIT_SCAL, 0);
  std::vector<double> ev(B * E, t0 + 0.5), tc(B, t0);
  StickyError step{h};
  step(hipMemcpyAsync(G.d_st, gs, sizeof(*gs), hipMemcpyHostToDevice, h->stream), "upload gait settings");
  step(hipMemcpyAsync(G.s[0].n, n.data(), B * 4, hipMemcpyHostToDevice, h->stream), "upload gait n_events");
  step(hipMemcpyAsync(G.s[0].ev, ev.data(), B * E * 8, hipMemcpyHostToDevice, h->stream), "upload gait event_times");
  step(hipMemcpyAsync(G.s[0].seq, seq.data(), B * (E + 1) * 4, hipMemcpyHostToDevice, h->stream), "upload gait mode_sequence");
  step(hipMemcpyAsync(G.s[0].scal, scal.data(), B * GAIT_SCAL * 4, hipMemcpyHostToDevice, h->stream), "upload gait rungs");
  step(hipMemcpyAsync(G.s[0].t_change, tc.data(), B * 8, hipMemcpyHostToDevice, h->stream), "upload gait change times");
  step(hipStreamSynchronize(h->stream), "sync");
  if (step.rc != HSQP_OK) return step.rc;
  G.st = *gs; G.B = batch; G.cur = 0;
  G.ready = true;
  return HSQP_OK;
}

int hsqp_gait_reset(hsqp_handle* h, const hsqp_gait_settings* settings, int batch, double t0) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (h->loop.started && h->loop.gait) h->loop.started = false;
  return gait_reset_impl(h, "hsqp_gait_reset", settings, batch, t0);
}

// queues k_gait_update on the handle's stream (device arrays), reads the B status words; the copies are NOT swapped here
static int gait_launch_and_check(hsqp_handle* h, const char* who, int batch, double t, double horizon, const double* d_v, const double* d_x, int* d_ne, double* d_ev,
                                 int* d_seq) {
  hsqp_handle::Gait& G = h->gait;
  StickyError step{h};
  HSQP_LAUNCH(k_gait_update, dim3(batch), dim3(64), 0, h->stream, G.d_st, G.s[G.cur], G.s[G.cur ^ 1], t, horizon, d_v, d_x, d_ne, d_ev, d_seq, G.status);
  step(hipGetLastError(), "k_gait_update");
  std::vector<int> status(batch);
  step(hipMemcpyAsync(status.data(), G.status, (size_t)batch * 4, hipMemcpyDeviceToHost, h->stream), "download gait status");
  step(hipStreamSynchronize(h->stream), "sync");
  if (step.rc != HSQP_OK) return step.rc;
  for (int b = 0; b < batch; ++b)
    if (status[b] != HSQP_GAIT_OK) {
      h->err = std::string(who) + ": gait update of instance " + std::to_string(b) +
               (status[b] == HSQP_GAIT_OVERFLOW ? ": the schedule would exceed max_events" : ": the template tiling would not start behind the last event of the schedule") +
               " (the gait state is unchanged)";
      return HSQP_ERR_BAD_ARG;
    }
  return HSQP_OK;
}

static int gait_update_impl(hsqp_handle* h, int batch, double t, double horizon, const double* v, const double* x, int32_t* ne, double* ev, int32_t* seq, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_gait_update_device" : "hsqp_gait_update";
  { const int rc = gait_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  hsqp_handle::Gait& G = h->gait;
  if (!G.ready) return loop_bad(h, who, "no gait state (hsqp_gait_reset)");
  if (h->loop.started && h->loop.gait) h->loop.started = false;   // the state is the caller's again
  if (batch != G.B) return loop_bad(h, who, "the batch differs from the one of hsqp_gait_reset");
  if (!v || !x || !ne || !ev || !seq) return loop_bad(h, who, "null array");
  if (!std::isfinite(t) || !std::isfinite(horizon) || !(horizon > 0.0)) return loop_bad(h, who, "t not finite, or horizon not finite and > 0");
  const size_t B = batch, E = G.st.max_events;
  HCHECK(hipSetDevice(h->device));
  int rc;
  if (dev) {
    rc = gait_launch_and_check(h, who, batch, t, horizon, v, x, ne, ev, seq);
  } else {
    StickyError step{h};
    step(hipMemcpyAsync(G.v, v, B * CMD_N * 8, hipMemcpyHostToDevice, h->stream), "upload v_filt");
    step(hipMemcpyAsync(G.x, x, B * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x");
    if (step.rc != HSQP_OK) return step.rc;
    rc = gait_launch_and_check(h, who, batch, t, horizon, G.v, G.x, G.ne, G.ev, G.seq);
    const std::string err = h->err;
    step(hipMemcpyAsync(ne, G.ne, B * 4, hipMemcpyDeviceToHost, h->stream), "download n_events");
    step(hipMemcpyAsync(ev, G.ev, B * E * 8, hipMemcpyDeviceToHost, h->stream), "download event_times");
    step(hipMemcpyAsync(seq, G.seq, B * (E + 1) * 4, hipMemcpyDeviceToHost, h->stream), "download mode_sequence");
    step(hipStreamSynchronize(h->stream), "sync");
    if (rc != HSQP_OK) h->err = err; else rc = step.rc;
  }
  if (rc == HSQP_OK) G.cur ^= 1;
  return rc;
}

int hsqp_gait_update(hsqp_handle* h, int batch, double t, double horizon, const double* v_filt, const double* x, int32_t* n_events, double* event_times,
                     int32_t* mode_sequence) {
  return gait_update_impl(h, batch, t, horizon, v_filt, x, n_events, event_times, mode_sequence, false);
}
int hsqp_gait_update_device(hsqp_handle* h, int batch, double t, double horizon, const double* d_v_filt, const double* d_x, int32_t* d_n_events,
                            double* d_event_times, int32_t* d_mode_sequence) {
  return gait_update_impl(h, batch, t, horizon, d_v_filt, d_x, d_n_events, d_event_times, d_mode_sequence, true);
}

static int gait_state_impl(hsqp_handle* h, int32_t* rung, double* t_change, int32_t* ne, double* ev, int32_t* seq, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_gait_state_device" : "hsqp_gait_state";
  { const int rc = gait_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  hsqp_handle::Gait& G = h->gait;
  if (!G.ready) return loop_bad(h, who, "no gait state (hsqp_gait_reset)");
  HCHECK(hipSetDevice(h->device));
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t B = G.B, E = G.st.max_events;
  const GaitState& s = G.s[G.cur];
  if (rung) HCHECK(hipMemcpy2DAsync(rung, 4, s.scal, GAIT_SCAL * 4, 4, B, kind, h->stream));   // column 0 of the [B][GAIT_SCAL] scalars
  if (t_change) HCHECK(hipMemcpyAsync(t_change, s.t_change, B * 8, kind, h->stream));
  if (ne) HCHECK(hipMemcpyAsync(ne, s.n, B * 4, kind, h->stream));
  if (ev) HCHECK(hipMemcpyAsync(ev, s.ev, B * E * 8, kind, h->stream));
  if (seq) HCHECK(hipMemcpyAsync(seq, s.seq, B * (E + 1) * 4, kind, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  return HSQP_OK;
}
int hsqp_gait_state(hsqp_handle* h, int32_t* rung, double* last_change_time, int32_t* n_events, double* event_times, int32_t* mode_sequence) {
  return gait_state_impl(h, rung, last_change_time, n_events, event_times, mode_sequence, false);
}
int hsqp_gait_state_device(hsqp_handle* h, int32_t* d_rung, double* d_last_change_time, int32_t* d_n_events, double* d_event_times, int32_t* d_mode_sequence) {
  return gait_state_impl(h, d_rung, d_last_change_time, d_n_events, d_event_times, d_mode_sequence, true);
}

int hsqp_loop_start_gait(hsqp_handle* h, const hsqp_loop_settings* settings, const hsqp_gait_settings* gait, int batch, double t0, const double* x0,
                         const double* v_cmd) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (!gait) { h->loop.started = false; return loop_bad(h, "hsqp_loop_start_gait", "null gait settings"); }
  return loop_start_impl(h, "hsqp_loop_start_gait", settings, gait, batch, t0, x0, v_cmd, gait->max_events, nullptr, nullptr, nullptr);
}

// One cycle from the resident buffers (include/hsqp_loop.h, steps 1 to 5).  d_xlog / d_ulog: this cycle's log rows (device) or null.  On a failure the
// loop's own state (t, x, v_filt) is that of the last completed cycle: the filter state is advanced on a copy and committed with the state.
// Under isolation (include/hsqp_episode.h): the command in use, the warm start per instance, the status words left to the triage behind step 5.
static bool observe_in_force(const hsqp_handle* h) { return h->observe_set || h->observe_B > 0; }
static void launch_observe(hsqp_handle* h, const ObserveArgs& a) {
  HSQP_LAUNCH(k_observe, dim3((a.B * OBS_BLOCKS + OBS_THREADS - 1) / OBS_THREADS), dim3(OBS_THREADS), 0, h->stream, a);
}

// the metrics kernel of the cycle that has just been rolled out: the form follows the rollout's own variant rule (ground, terrain, actuator model)
static int loop_metrics_cycle(hsqp_handle* h) {
  hsqp_handle::Loop& L = h->loop;
  const RolloutVariant v(false, h->plant.kind == HSQP_PLANT_TORQUE, h->contact.enabled, h->actuator.enabled, h->inertia_B, !h->terrain_maps.empty(), h->terrain_B);
  MetricsArgs a{};
  a.isolate = L.isolate ? 1 : 0; a.cycle = L.cycle; a.period = L.st.period;
  if (L.isolate) { a.st = L.ep_st; a.ep_state = L.ep.state; }
  if (L.isolate && L.ground && L.ground_st.box_above_ground) a.ground = L.gnd_g[L.ground_cur ^ 1];   // (before step 5: the cycle's value is still the shadow)
  a.it_status = h->d_status; a.perf = h->d_perf_after; a.ro_status = L.ro_status;
  a.xs = L.xs; a.x_before = L.x; a.cmd = L.isolate ? L.v_use : L.v_cmd;
  a.steps = L.met_steps; a.rejected = L.met_rejected;
  if (v.actuated) {   // (the rollout has just written the record)
    const ActuatorBuf ab = actuator_layout(Carve{h->d_actuator.p}, (size_t)h->st.max_batch);
    a.act_last = ab.last; a.act_limit = ab.table;
  }
  a.rec = L.met_rec; a.feet = L.met_feet;
  ContactParams cp{nullptr, 0.0, 0.0, 0.0};
  TerrainParams tp{nullptr, nullptr, nullptr, 0};
  if (v.ground) { const int rc = contact_params(h, cp); if (rc != HSQP_OK) return rc; }
  if (v.terrain) { const int rc = terrain_params(h, tp); if (rc != HSQP_OK) return rc; }
  if (v.terrain) HSQP_LAUNCH(k_loop_metrics<ContactTerrainSet>, dim3(L.B), dim3(RO_THREADS), sizeof(MetricsWST<ContactTerrainSet>), h->stream, h->d_dm, a, cp, tp);
  else if (v.ground) HSQP_LAUNCH(k_loop_metrics<ContactSet>, dim3(L.B), dim3(RO_THREADS), sizeof(MetricsWST<ContactSet>), h->stream, h->d_dm, a, cp, tp);
  else HSQP_LAUNCH(k_loop_metrics<MetricsNoGround>, dim3(L.B), dim3(RO_THREADS), sizeof(MetricsWST<MetricsNoGround>), h->stream, h->d_dm, a, cp, tp);
  HCHECK(hipGetLastError());
  return HSQP_OK;
}

// the first instance of `batch` status words (device) that has no grid, into h->err; HSQP_OK if every instance has one
static int grid_status_check(hsqp_handle* h, const char* who, const int* d_status, int batch, int n_nodes, int event_nodes) {
  std::vector<int> status(batch);
  HCHECK(hipMemcpy(status.data(), d_status, (size_t)batch * 4, hipMemcpyDeviceToHost));
  for (int b = 0; b < batch; ++b)
    if (status[b] != HSQP_GRID_OK)
      return loop_bad(h, who, ("event grid of instance " + std::to_string(b) + ": it needs more than n_nodes + event_nodes = " + std::to_string(n_nodes) + " + " +
                               std::to_string(event_nodes) + " intervals (or its event times admit no grid)").c_str());
  return HSQP_OK;
}
// step 2 of a cycle on the event grid has failed with rc: if the builder refused an instance that is the failure (the status words are read only here)
static int loop_grid_failure(hsqp_handle* h, const char* who, int rc) {
  const hsqp_handle::Loop& L = h->loop;
  const std::string err = h->err;
  const int g = grid_status_check(h, who, L.grid_status, L.B, L.st.n_nodes, L.grid_st.event_nodes);
  if (g == HSQP_ERR_BAD_ARG) return g;
  h->err = err;
  return rc;
}

static int loop_cycle(hsqp_handle* h, double* d_xlog, double* d_ulog) {
  hsqp_handle::Loop& L = h->loop;
  const hsqp_loop_settings& st = L.st;
  const size_t B = L.B;
  const bool iso = L.isolate;
  const int warm = L.have_cycle ? HSQP_WARM_SHIFT : HSQP_WARM_COLD;
  // the observation model (include/hsqp_observe.h): with it in force the MPC reads y at the problem time tp; without it the plant's state at the loop's time
  const bool obs = observe_in_force(h);
  const double lag = obs ? observe_policy_time(h->observe.compute_delay, st.period) : 0.0;
  const double tp = obs ? observe_problem_time(L.t, lag) : L.t;
  const double* xm = obs ? L.obs_y[L.cycle & 1] : L.x;
  // the event-node grid (include/hsqp_grid.h): N = n_nodes + event_nodes intervals, built into the shadow record behind the gait update
  const bool grid = L.grid;
  const hsqp_handle::Loop::GridRec* gr = grid ? &L.grid_rec[L.grid_cur ^ 1] : nullptr;
  hsqp_problem p{};
  p.batch = L.B; p.n_nodes = grid ? st.n_nodes + L.grid_st.event_nodes : st.n_nodes; p.dt = st.dt; p.x_init = xm;
  // step 2's checks come first, as in hsqp_upload_reference: a rejected cycle leaves the resident solution as it was
  h->have_policy = false;
  h->have_value = false;
  const int N_prev = h->N;
  if (warm == HSQP_WARM_SHIFT) { const int rc = warm_shift_ready(h, L.B, true, iso); if (rc != HSQP_OK) return rc; }
  StickyError step{h};
  // 0. the observation: the plant's state into the ring, y from the delayed slot, the policy time of step 4 into s0
  if (obs) {
    ObserveArgs a{};
    a.table = h->observe_B ? observe_table_layout(Carve{h->d_observe_table.p}, (size_t)h->st.max_batch).table : nullptr;
    a.key0 = (uint32_t)(h->observe.seed & 0xffffffffu); a.key1 = (uint32_t)(h->observe.seed >> 32);
    a.draw = (uint32_t)L.cycle; a.B = L.B;
    observe_cycle_slots(L.cycle, h->observe.sensor_delay + h->observe.compute_delay, a);
    a.fresh_all = L.have_cycle ? 0 : 1;
    a.mode_b = iso && L.have_cycle ? L.ep.mode : nullptr;
    a.x = L.x; a.ring = L.obs_ring; a.y = L.obs_y[L.cycle & 1]; a.s0 = L.s0; a.s0_value = lag;
    launch_observe(h, a);
    step(hipGetLastError(), "k_observe");
  }
  // 1. the targets; the filter state advances in the second half of its buffer
  double* vf_next = L.v_filt + B * CMD_N;
  step(hipMemcpyAsync(vf_next, L.v_filt, B * CMD_N * 8, hipMemcpyDeviceToDevice, h->stream), "copy v_filt");
  const bool cent = h->hdm.formulation == HSQP_FORM_CENTROIDAL;   // (a loop started by hsqp_loop_start_centroidal, include/hsqp_cent_loop.h)
  if (cent) launch_command_targets_cent(h, L.B, iso ? L.v_use : L.v_cmd, vf_next, st.filter_alpha, xm, tp, st.n_nodes * st.dt, L.tt, L.ts, nullptr);
  else launch_command_targets(h, L.B, iso ? L.v_use : L.v_cmd, vf_next, st.filter_alpha, xm, tp, st.n_nodes * st.dt, L.tt, L.ts);
  step(hipGetLastError(), cent ? "k_command_targets_cent" : "k_command_targets");
  // the gait update between steps 1 and 2 (include/hsqp_gait.h): this cycle's schedule into ne / ev / seq; the shadow state becomes the live one with step 5
  if (L.gait) {
    if (step.rc != HSQP_OK) return step.rc;
    const int rc = gait_launch_and_check(h, "hsqp_loop_run", L.B, tp, st.n_nodes * st.dt, vf_next, xm, L.ne, L.ev, L.seq);
    if (rc != HSQP_OK) return rc;
  }
  // the ground-height estimate between the targets (and the gait update) and step 2 (include/hsqp_ground.h): from the state the MPC reads and this cycle's
  // schedule the latch advances into its shadow, the knots of step 1 are shifted by it and step 2 takes it as the instance's terrain height
  const bool gnd = L.ground;
  if (gnd) {
    GroundArgs ga{};
    ga.B = L.B; ga.E = L.E; ga.t = tp; ga.filter_alpha = L.ground_st.filter_alpha;
    ga.x = xm; ga.ne = L.ne; ga.ev = L.ev; ga.seq = L.seq;
    ga.g_in = L.gnd_g[L.ground_cur]; ga.g_out = L.gnd_g[L.ground_cur ^ 1]; ga.foot_z = L.gnd_fz[L.ground_cur ^ 1];
    ga.g_init = L.gnd_init; ga.mode_b = iso ? L.ep.mode : nullptr; ga.parked = iso ? L.ep.state : nullptr;
    ga.ts = L.ts; ga.terrain_b = L.gnd_terrain;
    if (step.rc == HSQP_OK) launch_ground_estimate(h, ga);
    step(hipGetLastError(), "k_ground_estimate");
  }
  // the per-foot swing heights behind the targets, the gait update and the ground estimate (include/hsqp_perceive.h): from the state the MPC reads, this
  // cycle's schedule and this cycle's (shifted) knots every instance's rows, which step 2 takes in place of the terrain height
  const bool pcv = L.perceive;
  if (pcv) {
    PerceiveArgs pa{};
    pa.B = L.B; pa.E = L.E; pa.K = CMD_KNOTS; pa.t = tp; pa.offset = st.swing.touch_down_height_offset;
    pa.x = xm; pa.ne = L.ne; pa.ev = L.ev; pa.seq = L.seq; pa.tt = L.tt; pa.ts = L.ts;
    pa.lift = L.pcv_lift; pa.touch = L.pcv_touch; pa.fxy = L.pcv_fxy;
    if (step.rc == HSQP_OK) { const int rc = launch_foot_heights(h, "hsqp_loop_run", pa); if (rc != HSQP_OK) return rc; }
    step(hipGetLastError(), "k_foot_heights");
  }
  // 2. hsqp_upload_reference's work on the resident arrays
  h->have_problem = false; h->have_solution = false; h->have_stamps = false;
  if (grid) {   // the grid of every instance from this cycle's schedule, into d_dt and the shadow record; set_grid's part is the builder's
    h->uniform_grid = false; h->grid_resident = false; h->has_events = true;
    step(hipMemsetAsync(L.grid_bad, 0, 4, h->stream), "memset");
    HSQP_LAUNCH(k_event_grid, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, tp, st.n_nodes, st.dt, L.grid_st.dt_min, L.grid_st.event_nodes, L.B, L.E, (const int*)L.ne,
                (const double*)L.ev, gr->ni, (double*)h->d_dt, gr->nts, L.grid_status, L.grid_bad, gr->dts);
    step(hipGetLastError(), "k_event_grid");
  } else {
    const int rc = set_grid(h, &p, false); if (rc != HSQP_OK) return rc;
  }
  step(hipMemsetAsync(L.bad, 0, 4, h->stream), "memset");
  step(hipMemcpyAsync(h->d_xinit, xm, B * NX * 8, hipMemcpyDeviceToDevice, h->stream), "copy x_init");
  RefDev rd{L.E, CMD_KNOTS, L.ne, L.seq, L.ev, L.tt, L.ts, grid ? gr->nts : nullptr, L.bad, tp, st.dt, st.swing, st.terrain_height, st.arm_swing, warm, N_prev, true};
  if (iso && warm == HSQP_WARM_SHIFT) rd.warm_b = L.ep.mode;
  if (grid) rd.grid_bad = L.grid_bad;
  if (gnd) rd.terrain_b = L.gnd_terrain;
  if (pcv) { rd.lift_rows = L.pcv_lift; rd.touch_rows = L.pcv_touch; }
  { const int rc = reference_build(h, &p, rd, step);
    if (rc != HSQP_OK) return grid ? loop_grid_failure(h, "hsqp_loop_run", rc) : rc; }
  // 3. the iteration
  { const int rc = hsqp_iterate_device(h, st.iterations, st.iterate_flags); if (rc != HSQP_OK) return rc; }
  // 4. the plant under the policy over one period, from its true state (with the model in force at s0 = compute_delay periods in the policy's frame)
  { const int rc = rollout_impl(h, &st.rollout, L.s0, L.x, st.period, 1, L.xs, L.us, L.ro_status, L.metrics ? L.met_steps : nullptr, L.metrics ? L.met_rejected : nullptr, true, iso);
    if (rc != HSQP_OK) return rc; }
  // the episode metrics (include/hsqp_metrics.h): the cycle's sample, while L.x is still the state the rollout started from and the command the one step 1 read
  if (L.metrics) { const int rc = loop_metrics_cycle(h); if (rc != HSQP_OK) return rc; }
  // 5. the rolled-out state is the next measured state
  HCHECK(hipMemcpyAsync(L.x, L.xs, B * NX * 8, hipMemcpyDeviceToDevice, h->stream));
  HCHECK(hipMemcpyAsync(L.v_filt, vf_next, B * CMD_N * 8, hipMemcpyDeviceToDevice, h->stream));
  if (d_xlog) HCHECK(hipMemcpyAsync(d_xlog, L.xs, B * NX * 8, hipMemcpyDeviceToDevice, h->stream));
  if (d_ulog) HCHECK(hipMemcpyAsync(d_ulog, L.us, B * NU * 8, hipMemcpyDeviceToDevice, h->stream));
  if (L.gait) h->gait.cur ^= 1;
  if (gnd) L.ground_cur ^= 1;   // the shadow is the latch
  L.t += st.period;
  if (iso) {   // 6. the triage of every instance, and with a resident gait the reset of those that start a new episode at the new loop time
    const TriageArgs a{L.ep_st, L.cycle, h->d_status, h->d_perf_after, L.ro_status, L.xs, L.x_reset, L.v_cmd, L.ep, L.x, L.v_filt, L.v_use, d_xlog, d_ulog,
                       gnd && L.ground_st.box_above_ground ? L.gnd_g[L.ground_cur] : nullptr, episode_pose_offset(h)};
    HSQP_LAUNCH(k_loop_triage, dim3(L.B), dim3(64), 0, h->stream, a);
    if (L.gait)
      HSQP_LAUNCH(k_gait_reset_instances, dim3(L.B), dim3(64), 0, h->stream, h->gait.s[h->gait.cur], h->gait.st.max_events, (const int*)nullptr, (const int*)L.ep.reset,
                  obs ? observe_problem_time(L.t, lag) : L.t);   // the gait's clock is the problem time of the next cycle
    HCHECK(hipGetLastError());
  }
  if (obs) { L.obs_last = true; L.obs_tp = tp; }
  if (grid) L.grid_cur ^= 1;   // the shadow record is the completed cycle's
  L.grid_have = grid;
  ++L.cycle;
  L.have_cycle = true;
  return HSQP_OK;
}

static int loop_run_impl(hsqp_handle* h, int n_cycles, double* x_log, double* u_log, int* cycles_done, bool dev) {
  if (cycles_done) *cycles_done = 0;
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_loop_run_device" : "hsqp_loop_run";
  { const int rc = loop_started(h, who); if (rc != HSQP_OK) return rc; }
  if (n_cycles < 1) return loop_bad(h, who, "n_cycles < 1");
  if (h->push_B && h->push_B != h->loop.B)
    return loop_bad(h, who, ("the push table holds " + std::to_string(h->push_B) + " instances, the loop " + std::to_string(h->loop.B) + " (hsqp_push_set / hsqp_push_clear)").c_str());
  if (observe_in_force(h)) {
    hsqp_handle::Loop& L = h->loop;
    if (h->observe_B && h->observe_B != L.B)
      return loop_bad(h, who, ("the observation table holds " + std::to_string(h->observe_B) + " instances, the loop " + std::to_string(L.B) +
                               " (hsqp_observe_set_instances / hsqp_observe_clear)").c_str());
    if (!observe_horizon_ok(h->observe.compute_delay, L.st.period, L.st.n_nodes, L.st.dt))
      return loop_bad(h, who, ("(compute_delay + 1) period = " + std::to_string((h->observe.compute_delay + 1) * L.st.period) + " s exceeds the horizon n_nodes dt = " +
                               std::to_string(L.st.n_nodes * L.st.dt) + " s: the policy would be evaluated past its horizon (hsqp_observe_set)").c_str());
    HCHECK(hipSetDevice(h->device));
    const size_t slots = (size_t)(h->observe.sensor_delay + h->observe.compute_delay + 1);
    DEV_ENSURE(h->d_observe, observe_layout(Carve{}, L, (size_t)L.B, slots), "observation ring");
    observe_layout(Carve{h->d_observe.p}, L, (size_t)L.B, slots);
  }
  HCHECK(hipSetDevice(h->device));
  const size_t B = h->loop.B, nx = B * NX, nu = B * NU, n = n_cycles;
  double* d_xl = x_log;
  double* d_ul = u_log;
  if (!dev && (x_log || u_log)) {
    DEV_ENSURE(h->d_loop_log, loop_log_layout(nullptr, n, B, x_log, u_log).bytes, "loop log staging");
    const LoopLog lg = loop_log_layout(reinterpret_cast<double*>(h->d_loop_log.p), n, B, x_log, u_log);
    d_xl = lg.x; d_ul = lg.u;
  }
  int rc = HSQP_OK, done = 0;
  for (; done < n_cycles && rc == HSQP_OK; done += rc == HSQP_OK)
    rc = loop_cycle(h, d_xl ? d_xl + done * nx : nullptr, d_ul ? d_ul + done * nu : nullptr);
  if (cycles_done) *cycles_done = done;
  // the rows of the completed cycles, once (a failed cycle's error text stays in h->err)
  const std::string err = h->err;
  StickyError step{h};
  if (!dev && done > 0) {
    if (x_log) step(hipMemcpyAsync(x_log, d_xl, done * nx * 8, hipMemcpyDeviceToHost, h->stream), "download x_log");
    if (u_log) step(hipMemcpyAsync(u_log, d_ul, done * nu * 8, hipMemcpyDeviceToHost, h->stream), "download u_log");
  }
  if (h->loop.grid && !h->uniform_grid) {   // the host copy of the resident problem's device-built grid (debug reads), once per run
    h->h_dt.resize(B * (size_t)(h->loop.st.n_nodes + h->loop.grid_st.event_nodes));
    step(hipMemcpyAsync(h->h_dt.data(), h->d_dt, h->h_dt.size() * 8, hipMemcpyDeviceToHost, h->stream), "download dt_nodes");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  if (rc != HSQP_OK) { h->err = err; return rc; }
  return step.rc;
}
int hsqp_loop_run(hsqp_handle* h, int n_cycles, double* x_log, double* u_log, int* cycles_done) { return loop_run_impl(h, n_cycles, x_log, u_log, cycles_done, false); }
int hsqp_loop_run_device(hsqp_handle* h, int n_cycles, double* d_x_log, double* d_u_log, int* cycles_done) {
  return loop_run_impl(h, n_cycles, d_x_log, d_u_log, cycles_done, true);
}

static int loop_state_impl(hsqp_handle* h, double* t, double* x, double* v_filt, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  { const int rc = loop_started(h, dev ? "hsqp_loop_state_device" : "hsqp_loop_state"); if (rc != HSQP_OK) return rc; }
  HCHECK(hipSetDevice(h->device));
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t B = h->loop.B;
  if (t) *t = h->loop.t;
  if (x) HCHECK(hipMemcpyAsync(x, h->loop.x, B * NX * 8, kind, h->stream));
  if (v_filt) HCHECK(hipMemcpyAsync(v_filt, h->loop.v_filt, B * CMD_N * 8, kind, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  return HSQP_OK;
}
int hsqp_loop_state(hsqp_handle* h, double* t, double* x, double* v_filt) { return loop_state_impl(h, t, x, v_filt, false); }
int hsqp_loop_state_device(hsqp_handle* h, double* t, double* d_x, double* d_v_filt) { return loop_state_impl(h, t, d_x, d_v_filt, true); }

// ---- the event-node time grid (include/hsqp_grid.h, csrc/hsqp_grid.h): the stand-alone builder, the loop's switch, the loop's last grid
void hsqp_grid_defaults(hsqp_grid_settings* s) {
  if (!s) return;
  memset(s, 0, sizeof(*s));
  s->event_nodes = 32;
  s->dt_min = 1e-4;   // HipSqpSolverAdaptor's dtMin
}

// what every grid entry point asks of (settings, n_nodes, dt) on handle h
static int grid_settings_ok(hsqp_handle* h, const char* who, const hsqp_grid_settings* gs, int n_nodes, double dt) {
  if (!gs) return loop_bad(h, who, "null settings");
  if (gs->reserved != 0) return loop_bad(h, who, "hsqp_grid_settings::reserved must be 0");
  if (gs->event_nodes < 0) return loop_bad(h, who, "hsqp_grid_settings::event_nodes < 0");
  if (!std::isfinite(gs->dt_min) || gs->dt_min < 0.0) return loop_bad(h, who, "hsqp_grid_settings::dt_min not finite and >= 0");
  if (!std::isfinite(dt) || !(dt > gs->dt_min)) return loop_bad(h, who, ("dt = " + std::to_string(dt) + " must be finite and > hsqp_grid_settings::dt_min = " + std::to_string(gs->dt_min)).c_str());
  if (n_nodes < 1) return loop_bad(h, who, "n_nodes < 1");
  if ((long long)n_nodes + gs->event_nodes > h->st.max_nodes)
    return loop_bad(h, who, ("n_nodes + hsqp_grid_settings::event_nodes = " + std::to_string(n_nodes) + " + " + std::to_string(gs->event_nodes) + " exceeds max_nodes = " +
                             std::to_string(h->st.max_nodes)).c_str());
  return HSQP_OK;
}

static int event_grid_impl(hsqp_handle* h, const hsqp_grid_settings* gs, int batch, double t0, int n_nodes, double dt, int max_events, const int32_t* ne, const double* ev,
                           int32_t* ni, double* dts, double* nts, int32_t* status, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_event_grid_device" : "hsqp_event_grid";
  { const int rc = grid_settings_ok(h, who, gs, n_nodes, dt); if (rc != HSQP_OK) return rc; }
  if (!ne || !ev || !ni || !dts || !nts) return loop_bad(h, who, "null array");
  if (batch < 1 || batch > h->st.max_batch) return loop_bad(h, who, "batch outside [1, max_batch]");
  if (max_events < 1) return loop_bad(h, who, "max_events < 1");
  if (!std::isfinite(t0)) return loop_bad(h, who, "t0 not finite");
  const size_t B = batch, E = max_events, N = (size_t)n_nodes + gs->event_nodes;
  if (!dev)
    for (size_t b = 0; b < B; ++b) {
      if (ne[b] < 0 || ne[b] > max_events) return loop_bad(h, who, ("n_events of instance " + std::to_string(b) + " outside [0, max_events]").c_str());
      for (int i = 0; i < ne[b]; ++i)
        if (!std::isfinite(ev[b * E + i]) || (i > 0 && ev[b * E + i] < ev[b * E + i - 1]))
          return loop_bad(h, who, ("event_times of instance " + std::to_string(b) + ": entry " + std::to_string(i) + " is not finite or lies before the entry in front of it").c_str());
    }
  HCHECK(hipSetDevice(h->device));
  DEV_ENSURE(h->d_grid_stage, grid_stage_layout(Carve{}, B, N, E, !dev).bytes, "event grid staging");
  const GridStage sg = grid_stage_layout(Carve{h->d_grid_stage.p}, B, N, E, !dev);
  StickyError step{h};
  if (!dev) {
    step(hipMemcpyAsync(sg.ne, ne, B * 4, hipMemcpyHostToDevice, h->stream), "upload n_events");
    step(hipMemcpyAsync(sg.ev, ev, B * E * 8, hipMemcpyHostToDevice, h->stream), "upload event_times");
  }
  if (step.rc == HSQP_OK) {
    HSQP_LAUNCH(k_event_grid, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, h->stream, t0, n_nodes, dt, gs->dt_min, gs->event_nodes, batch, max_events,
                dev ? (const int*)ne : (const int*)sg.ne, dev ? ev : (const double*)sg.ev, dev ? (int*)ni : sg.ni, dev ? dts : sg.dts, dev ? nts : sg.nts, sg.status, (int*)nullptr,
                (double*)nullptr);
    step(hipGetLastError(), "k_event_grid");
  }
  if (!dev) {
    step(hipMemcpyAsync(ni, sg.ni, B * 4, hipMemcpyDeviceToHost, h->stream), "download n_intervals");
    step(hipMemcpyAsync(dts, sg.dts, B * N * 8, hipMemcpyDeviceToHost, h->stream), "download dt_nodes");
    step(hipMemcpyAsync(nts, sg.nts, B * (N + 1) * 8, hipMemcpyDeviceToHost, h->stream), "download node_times");
  }
  if (status) step(hipMemcpyAsync(status, sg.status, B * 4, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream), "download status");
  step(hipStreamSynchronize(h->stream), "sync");
  if (step.rc != HSQP_OK) return step.rc;
  return grid_status_check(h, who, sg.status, batch, n_nodes, gs->event_nodes);
}
int hsqp_event_grid(hsqp_handle* h, const hsqp_grid_settings* settings, int batch, double t0, int n_nodes, double dt, int max_events, const int32_t* n_events,
                    const double* event_times, int32_t* n_intervals, double* dt_nodes, double* node_times, int32_t* status) {
  return event_grid_impl(h, settings, batch, t0, n_nodes, dt, max_events, n_events, event_times, n_intervals, dt_nodes, node_times, status, false);
}
int hsqp_event_grid_device(hsqp_handle* h, const hsqp_grid_settings* settings, int batch, double t0, int n_nodes, double dt, int max_events,
                           const int32_t* d_n_events, const double* d_event_times, int32_t* d_n_intervals, double* d_dt_nodes, double* d_node_times,
                           int32_t* d_status) {
  return event_grid_impl(h, settings, batch, t0, n_nodes, dt, max_events, d_n_events, d_event_times, d_n_intervals, d_dt_nodes, d_node_times, d_status, true);
}

int hsqp_loop_event_grid(hsqp_handle* h, const hsqp_grid_settings* gs) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_loop_event_grid";
  { const int rc = loop_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  { const int rc = loop_started(h, who); if (rc != HSQP_OK) return rc; }
  hsqp_handle::Loop& L = h->loop;
  if (!gs) { L.grid = false; return HSQP_OK; }   // (the record of the last completed cycle stays readable until a cycle on the uniform grid completes)
  { const int rc = grid_settings_ok(h, who, gs, L.st.n_nodes, L.st.dt); if (rc != HSQP_OK) return rc; }
  HCHECK(hipSetDevice(h->device));
  const size_t B = L.B, N = (size_t)L.st.n_nodes + gs->event_nodes;
  const bool same = L.grid_have && L.grid_st.event_nodes == gs->event_nodes;   // the records keep their place: the completed cycle's grid stays
  DEV_ENSURE(h->d_grid, grid_layout(Carve{}, L, B, N), "loop grid records");
  grid_layout(Carve{h->d_grid.p}, L, B, N);
  if (!same) { L.grid_have = false; L.grid_cur = 0; }
  L.grid_st = *gs;
  L.grid = true;
  return HSQP_OK;
}

static int loop_grid_impl(hsqp_handle* h, int32_t* ni, double* dts, double* nts, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_loop_grid_device" : "hsqp_loop_grid";
  { const int rc = loop_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  { const int rc = loop_started(h, who); if (rc != HSQP_OK) return rc; }
  const hsqp_handle::Loop& L = h->loop;
  if (!L.grid_have) return loop_bad(h, who, "the last completed cycle did not run on the event grid (hsqp_loop_event_grid, then hsqp_loop_run)");
  HCHECK(hipSetDevice(h->device));
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t B = L.B, N = (size_t)L.st.n_nodes + L.grid_st.event_nodes;
  const hsqp_handle::Loop::GridRec& r = L.grid_rec[L.grid_cur];
  if (ni) HCHECK(hipMemcpyAsync(ni, r.ni, B * 4, kind, h->stream));
  if (dts) HCHECK(hipMemcpyAsync(dts, r.dts, B * N * 8, kind, h->stream));
  if (nts) HCHECK(hipMemcpyAsync(nts, r.nts, B * (N + 1) * 8, kind, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  return HSQP_OK;
}
int hsqp_loop_grid(hsqp_handle* h, int32_t* n_intervals, double* dt_nodes, double* node_times) { return loop_grid_impl(h, n_intervals, dt_nodes, node_times, false); }
int hsqp_loop_grid_device(hsqp_handle* h, int32_t* d_n_intervals, double* d_dt_nodes, double* d_node_times) {
  return loop_grid_impl(h, d_n_intervals, d_dt_nodes, d_node_times, true);
}

// ---- the ground-height estimate (include/hsqp_ground.h, csrc/hsqp_ground.h): the stand-alone estimate, the upload with per-instance terrain heights, the
// loop's switch and its latches
void hsqp_ground_defaults(hsqp_ground_settings* s) {
  if (!s) return;
  memset(s, 0, sizeof(*s));
  s->enabled = 1;
}

static int ground_handle_ok(hsqp_handle* h, const char* who) {
  if (h->hdm.formulation != HSQP_FORM_WB) return loop_bad(h, who, "whole-body handles only (the contact frames' heights come from the whole-body configuration)");
  return HSQP_OK;
}

static int ground_estimate_impl(hsqp_handle* h, int batch, double t, const double* x, int max_events, const int32_t* ne, const double* ev, const int32_t* seq,
                                double alpha, double* g, double* foot_z, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_ground_estimate_device" : "hsqp_ground_estimate";
  { const int rc = ground_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  if (!x || !ne || !ev || !seq || !g) return loop_bad(h, who, "null array");
  if (batch < 1 || batch > h->st.max_batch) return loop_bad(h, who, "batch outside [1, max_batch]");
  if (!(alpha >= 0.0 && alpha < 1.0)) return loop_bad(h, who, "filter_alpha outside [0, 1)");
  if (!std::isfinite(t)) return loop_bad(h, who, "t not finite");
  if (max_events < 1) return loop_bad(h, who, "max_events < 1");
  const size_t B = batch, E = max_events;
  if (!dev) {
    for (size_t b = 0; b < B; ++b)
      if (ne[b] < 1 || ne[b] > max_events) return loop_bad(h, who, "n_events outside [1, max_events]");
    if (!all_finite(g, B)) return loop_bad(h, who, "non-finite g");
  }
  HCHECK(hipSetDevice(h->device));
  GroundArgs a{};
  a.B = batch; a.E = max_events; a.t = t; a.filter_alpha = alpha;
  StickyError step{h};
  if (dev) {
    a.x = x; a.ne = ne; a.ev = ev; a.seq = seq; a.g_in = g; a.g_out = g; a.foot_z = foot_z;
    launch_ground_estimate(h, a);
    step(hipGetLastError(), "k_ground_estimate");
  } else {
    DEV_ENSURE(h->d_ground_stage, ground_stage_layout(Carve{}, B, E, true).bytes, "ground-estimate staging");
    const GroundStage sg = ground_stage_layout(Carve{h->d_ground_stage.p}, B, E, true);
    step(hipMemcpyAsync(sg.ne, ne, B * 4, hipMemcpyHostToDevice, h->stream), "upload n_events");
    step(hipMemcpyAsync(sg.seq, seq, B * (E + 1) * 4, hipMemcpyHostToDevice, h->stream), "upload mode_sequence");
    step(hipMemcpyAsync(sg.x, x, B * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x");
    step(hipMemcpyAsync(sg.ev, ev, B * E * 8, hipMemcpyHostToDevice, h->stream), "upload event_times");
    step(hipMemcpyAsync(sg.g, g, B * 8, hipMemcpyHostToDevice, h->stream), "upload g");
    a.x = sg.x; a.ne = sg.ne; a.ev = sg.ev; a.seq = sg.seq; a.g_in = sg.g; a.g_out = sg.g; a.foot_z = sg.fz;
    if (step.rc == HSQP_OK) {
      launch_ground_estimate(h, a);
      step(hipGetLastError(), "k_ground_estimate");
    }
    step(hipMemcpyAsync(g, sg.g, B * 8, hipMemcpyDeviceToHost, h->stream), "download g");
    if (foot_z) step(hipMemcpyAsync(foot_z, sg.fz, 2 * B * 8, hipMemcpyDeviceToHost, h->stream), "download foot_z");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}
int hsqp_ground_estimate(hsqp_handle* h, int batch, double t, const double* x, int max_events, const int32_t* n_events, const double* event_times,
                         const int32_t* mode_sequence, double filter_alpha, double* g, double* foot_z) {
  return ground_estimate_impl(h, batch, t, x, max_events, n_events, event_times, mode_sequence, filter_alpha, g, foot_z, false);
}
int hsqp_ground_estimate_device(hsqp_handle* h, int batch, double t, const double* d_x, int max_events, const int32_t* d_n_events, const double* d_event_times,
                                const int32_t* d_mode_sequence, double filter_alpha, double* d_g, double* d_foot_z) {
  return ground_estimate_impl(h, batch, t, d_x, max_events, d_n_events, d_event_times, d_mode_sequence, filter_alpha, d_g, d_foot_z, true);
}

int hsqp_upload_reference_ground(hsqp_handle* h, const hsqp_problem* p, const hsqp_reference* r, const double* terrain_heights) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_upload_reference_ground";
  { const int rc = ground_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  if (!p || !r || !terrain_heights) return loop_bad(h, who, "null problem / reference / terrain_heights");
  if (p->batch < 1 || p->batch > h->st.max_batch) return loop_bad(h, who, "batch outside [1, max_batch]");
  if (!all_finite(terrain_heights, (size_t)p->batch)) return loop_bad(h, who, "non-finite terrain_heights");
  return upload_reference_impl(h, p, r, terrain_heights);
}

int hsqp_loop_ground(hsqp_handle* h, const hsqp_ground_settings* gs, const double* g_init) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_loop_ground";
  { const int rc = ground_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  { const int rc = loop_started(h, who); if (rc != HSQP_OK) return rc; }
  hsqp_handle::Loop& L = h->loop;
  if (gs && ((gs->enabled != 0 && gs->enabled != 1) || (gs->box_above_ground != 0 && gs->box_above_ground != 1)))
    return loop_bad(h, who, "hsqp_ground_settings::enabled and box_above_ground must be 0 or 1");
  if (!gs || !gs->enabled) { L.ground = false; return HSQP_OK; }
  if (!(gs->filter_alpha >= 0.0 && gs->filter_alpha < 1.0)) return loop_bad(h, who, "hsqp_ground_settings::filter_alpha outside [0, 1)");
  if (!std::isfinite(gs->initial_height)) return loop_bad(h, who, "hsqp_ground_settings::initial_height not finite");
  const size_t B = L.B;
  if (g_init && !all_finite(g_init, B)) return loop_bad(h, who, "non-finite g_init");
  HCHECK(hipSetDevice(h->device));
  L.ground = false;   // (a failure below leaves no half-made state switched on)
  DEV_ENSURE(h->d_ground, ground_layout(Carve{}, L, B), "loop ground latches");
  ground_layout(Carve{h->d_ground.p}, L, B);
  const std::vector<double> init(B, gs->initial_height);
  StickyError step{h};
  step(hipMemcpyAsync(L.gnd_init, g_init ? g_init : init.data(), B * 8, hipMemcpyHostToDevice, h->stream), "upload g_init");
  step(hipMemcpyAsync(L.gnd_g[0], g_init ? g_init : init.data(), B * 8, hipMemcpyHostToDevice, h->stream), "upload g");
  step(hipMemsetAsync(L.gnd_fz[0], 0, 2 * B * 8, h->stream), "memset foot_z");
  step(hipStreamSynchronize(h->stream), "sync");
  if (step.rc != HSQP_OK) return step.rc;
  L.ground_cur = 0;
  L.ground_st = *gs;
  L.ground = true;
  return HSQP_OK;
}

static int loop_ground_state_impl(hsqp_handle* h, double* g, double* foot_z, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_loop_ground_state_device" : "hsqp_loop_ground_state";
  { const int rc = ground_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  { const int rc = loop_started(h, who); if (rc != HSQP_OK) return rc; }
  const hsqp_handle::Loop& L = h->loop;
  if (!L.ground) return loop_bad(h, who, "the ground-height estimate is off (hsqp_loop_ground; every hsqp_loop_start turns it off)");
  HCHECK(hipSetDevice(h->device));
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t B = L.B;
  if (g) HCHECK(hipMemcpyAsync(g, L.gnd_g[L.ground_cur], B * 8, kind, h->stream));
  if (foot_z) HCHECK(hipMemcpyAsync(foot_z, L.gnd_fz[L.ground_cur], 2 * B * 8, kind, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  return HSQP_OK;
}
int hsqp_loop_ground_state(hsqp_handle* h, double* g, double* foot_z) { return loop_ground_state_impl(h, g, foot_z, false); }
int hsqp_loop_ground_state_device(hsqp_handle* h, double* d_g, double* d_foot_z) { return loop_ground_state_impl(h, d_g, d_foot_z, true); }

// ---- the per-foot swing heights from the height map (include/hsqp_perceive.h, csrc/hsqp_perceive.h): the upload with the planner's three-argument
// update, the stand-alone rows, the loop's switch and its rows
void hsqp_perceive_defaults(hsqp_perceive_settings* s) {
  if (!s) return;
  memset(s, 0, sizeof(*s));
  s->enabled = 1;
}

static int perceive_handle_ok(hsqp_handle* h, const char* who) {
  if (h->hdm.formulation != HSQP_FORM_WB) return loop_bad(h, who, "whole-body handles only (the footholds come from the whole-body configuration)");
  return HSQP_OK;
}

int hsqp_upload_reference_heights(hsqp_handle* h, const hsqp_problem* p, const hsqp_reference* r, const double* lift_off, const double* touch_down) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_upload_reference_heights";
  { const int rc = perceive_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  if (!p || !r || !lift_off || !touch_down) return loop_bad(h, who, "null problem / reference / lift_off / touch_down");
  return upload_reference_impl(h, p, r, nullptr, lift_off, touch_down, who);
}

static int foot_heights_impl(hsqp_handle* h, int batch, double t, const double* x, int max_events, const int32_t* ne, const double* ev, const int32_t* seq, int n_knots,
                             const double* tt, const double* ts, double offset, double* lift, double* touch, double* fxy, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_foot_heights_device" : "hsqp_foot_heights";
  { const int rc = perceive_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  if (!x || !ne || !ev || !seq || !tt || !ts || !lift || !touch) return loop_bad(h, who, "null array");
  if (batch < 1 || batch > h->st.max_batch) return loop_bad(h, who, "batch outside [1, max_batch]");
  if (!std::isfinite(t)) return loop_bad(h, who, "t not finite");
  if (!std::isfinite(offset)) return loop_bad(h, who, "touch_down_height_offset not finite");
  if (max_events < 1) return loop_bad(h, who, "max_events < 1");
  if (n_knots < 1) return loop_bad(h, who, "n_knots < 1");
  if (!h->hdm.has_default_joint_state) return loop_bad(h, who, "no default joint state: call hsqp_set_default_joint_state first");
  { const int rc = perceive_terrain_ok(h, who); if (rc != HSQP_OK) return rc; }
  const size_t B = batch, E = max_events, K = n_knots;
  if (!dev)
    for (size_t b = 0; b < B; ++b)
      if (ne[b] < 1 || ne[b] > max_events) return loop_bad(h, who, "n_events outside [1, max_events]");
  HCHECK(hipSetDevice(h->device));
  PerceiveArgs a{};
  a.B = batch; a.E = max_events; a.K = n_knots; a.t = t; a.offset = offset;
  StickyError step{h};
  DEV_ENSURE(h->d_perceive_stage, perceive_stage_layout(Carve{}, B, E, K, !dev).bytes, "foot-height staging");
  const PerceiveStage sg = perceive_stage_layout(Carve{h->d_perceive_stage.p}, B, E, K, !dev);
  if (dev) {
    a.x = x; a.ne = ne; a.ev = ev; a.seq = seq; a.tt = tt; a.ts = ts; a.lift = lift; a.touch = touch; a.fxy = fxy ? fxy : sg.fxy;
  } else {
    step(hipMemcpyAsync(sg.ne, ne, B * 4, hipMemcpyHostToDevice, h->stream), "upload n_events");
    step(hipMemcpyAsync(sg.seq, seq, B * (E + 1) * 4, hipMemcpyHostToDevice, h->stream), "upload mode_sequence");
    step(hipMemcpyAsync(sg.x, x, B * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x");
    step(hipMemcpyAsync(sg.ev, ev, B * E * 8, hipMemcpyHostToDevice, h->stream), "upload event_times");
    step(hipMemcpyAsync(sg.tt, tt, B * K * 8, hipMemcpyHostToDevice, h->stream), "upload target_times");
    step(hipMemcpyAsync(sg.ts, ts, B * K * NX * 8, hipMemcpyHostToDevice, h->stream), "upload target_states");
    a.x = sg.x; a.ne = sg.ne; a.ev = sg.ev; a.seq = sg.seq; a.tt = sg.tt; a.ts = sg.ts; a.lift = sg.lift; a.touch = sg.touch; a.fxy = sg.fxy;
  }
  if (step.rc == HSQP_OK) {
    const int rc = launch_foot_heights(h, who, a);
    if (rc != HSQP_OK) return rc;
    step(hipGetLastError(), "k_foot_heights");
  }
  if (!dev) {
    step(hipMemcpyAsync(lift, sg.lift, B * 2 * (E + 1) * 8, hipMemcpyDeviceToHost, h->stream), "download lift_off");
    step(hipMemcpyAsync(touch, sg.touch, B * 2 * (E + 1) * 8, hipMemcpyDeviceToHost, h->stream), "download touch_down");
    if (fxy) step(hipMemcpyAsync(fxy, sg.fxy, B * 4 * (E + 1) * 8, hipMemcpyDeviceToHost, h->stream), "download foothold_xy");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}
int hsqp_foot_heights(hsqp_handle* h, int batch, double t, const double* x, int max_events, const int32_t* n_events, const double* event_times,
                      const int32_t* mode_sequence, int n_knots, const double* target_times, const double* target_states, double touch_down_height_offset,
                      double* lift_off, double* touch_down, double* foothold_xy) {
  return foot_heights_impl(h, batch, t, x, max_events, n_events, event_times, mode_sequence, n_knots, target_times, target_states, touch_down_height_offset, lift_off,
                           touch_down, foothold_xy, false);
}
int hsqp_foot_heights_device(hsqp_handle* h, int batch, double t, const double* d_x, int max_events, const int32_t* d_n_events, const double* d_event_times,
                             const int32_t* d_mode_sequence, int n_knots, const double* d_target_times, const double* d_target_states,
                             double touch_down_height_offset, double* d_lift_off, double* d_touch_down, double* d_foothold_xy) {
  return foot_heights_impl(h, batch, t, d_x, max_events, d_n_events, d_event_times, d_mode_sequence, n_knots, d_target_times, d_target_states, touch_down_height_offset,
                           d_lift_off, d_touch_down, d_foothold_xy, true);
}

int hsqp_loop_perceive(hsqp_handle* h, const hsqp_perceive_settings* ps) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_loop_perceive";
  { const int rc = perceive_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  { const int rc = loop_started(h, who); if (rc != HSQP_OK) return rc; }
  hsqp_handle::Loop& L = h->loop;
  if (ps && ((ps->enabled != 0 && ps->enabled != 1) || ps->reserved != 0)) return loop_bad(h, who, "hsqp_perceive_settings::enabled must be 0 or 1 and reserved 0");
  if (!ps || !ps->enabled) { L.perceive = false; return HSQP_OK; }
  { const int rc = perceive_terrain_ok(h, who); if (rc != HSQP_OK) return rc; }
  if (L.perceive) return HSQP_OK;   // (on already: the rows of the last cycle stay)
  HCHECK(hipSetDevice(h->device));
  const size_t B = L.B, E = L.E;
  DEV_ENSURE(h->d_perceive, perceive_layout(Carve{}, L, B, E), "loop foot-height rows");
  const size_t bytes = perceive_layout(Carve{h->d_perceive.p}, L, B, E);
  StickyError step{h};
  step(hipMemsetAsync(h->d_perceive.p, 0, bytes, h->stream), "memset rows");
  step(hipStreamSynchronize(h->stream), "sync");
  if (step.rc != HSQP_OK) return step.rc;
  L.perceive = true;
  return HSQP_OK;
}

static int loop_foot_heights_impl(hsqp_handle* h, double* lift, double* touch, double* fxy, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_loop_foot_heights_device" : "hsqp_loop_foot_heights";
  { const int rc = perceive_handle_ok(h, who); if (rc != HSQP_OK) return rc; }
  { const int rc = loop_started(h, who); if (rc != HSQP_OK) return rc; }
  const hsqp_handle::Loop& L = h->loop;
  if (!L.perceive) return loop_bad(h, who, "the per-foot swing heights are off (hsqp_loop_perceive; every hsqp_loop_start turns them off)");
  HCHECK(hipSetDevice(h->device));
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t rows = (size_t)L.B * 2 * (size_t)(L.E + 1);
  if (lift) HCHECK(hipMemcpyAsync(lift, L.pcv_lift, rows * 8, kind, h->stream));
  if (touch) HCHECK(hipMemcpyAsync(touch, L.pcv_touch, rows * 8, kind, h->stream));
  if (fxy) HCHECK(hipMemcpyAsync(fxy, L.pcv_fxy, rows * 2 * 8, kind, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  return HSQP_OK;
}
int hsqp_loop_foot_heights(hsqp_handle* h, double* lift_off, double* touch_down, double* foothold_xy) { return loop_foot_heights_impl(h, lift_off, touch_down, foothold_xy, false); }
int hsqp_loop_foot_heights_device(hsqp_handle* h, double* d_lift_off, double* d_touch_down, double* d_foothold_xy) {
  return loop_foot_heights_impl(h, d_lift_off, d_touch_down, d_foothold_xy, true);
}

// ---- the observation model of the loop (include/hsqp_observe.h, csrc/hsqp_observe.h): the resident settings and table, the evaluation, the last observation
void hsqp_observe_defaults(hsqp_observe_settings* s) { if (s) memset(s, 0, sizeof(*s)); }
void hsqp_observe_instance_defaults(hsqp_observe_instance* v) { if (v) memset(v, 0, sizeof(*v)); }
static int observe_handle_ok(hsqp_handle* h, const char* who) {
  if (h->hdm.formulation != HSQP_FORM_WB) return loop_bad(h, who, "whole-body handles only (the model acts on the whole-body state row of the resident loop)");
  return HSQP_OK;
}
int hsqp_observe_set(hsqp_handle* h, const hsqp_observe_settings* s) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_observe_set";
  if (const int rc = observe_handle_ok(h, who)) return rc;
  if (!s) return loop_bad(h, who, "null settings");
  if (const char* what = observe_settings_error(*s)) return loop_bad(h, who, what);
  if (h->loop.started && (s->sensor_delay != h->observe.sensor_delay || s->compute_delay != h->observe.compute_delay))
    return loop_bad(h, who, "the delays differ from those in force while a loop is started (the ring and the problem clock would lose their meaning): restart the loop");
  h->observe = *s;
  h->observe_set = true;
  return HSQP_OK;
}
static int observe_set_instances_impl(hsqp_handle* h, int batch, const hsqp_observe_instance* t, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_observe_set_instances_device" : "hsqp_observe_set_instances";
  if (const int rc = observe_handle_ok(h, who)) return rc;
  if (!t) {
    if (batch < 0 || batch > h->st.max_batch) return loop_bad(h, who, "batch outside [0, max_batch]");
    h->observe_B = 0;
    return HSQP_OK;
  }
  if (batch < 1 || batch > h->st.max_batch) return loop_bad(h, who, "batch outside [1, max_batch]");
  if (!dev)
    for (int b = 0; b < batch; ++b)
      if (const int f = observe_entry_error(t[b]))
        return loop_bad(h, who, ("instance " + std::to_string(b) + (f > 0 ? ": bias[" + std::to_string(f - 1) + "] non-finite" : ": sigma[" + std::to_string(-f - 1) + "] negative or non-finite")).c_str());
  HCHECK(hipSetDevice(h->device));
  const size_t mb = (size_t)h->st.max_batch;
  DEV_ENSURE(h->d_observe_table, observe_table_layout(Carve{}, mb).bytes, "observation table");
  hsqp_observe_instance* d = observe_table_layout(Carve{h->d_observe_table.p}, mb).table;
  HCHECK(hipStreamSynchronize(h->stream));   // (no cycle in flight reads the entries that are replaced)
  h->observe_B = 0;                          // (a failure below leaves no table)
  HCHECK(hipMemcpy(d, t, (size_t)batch * sizeof(hsqp_observe_instance), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
  if (mb > (size_t)batch) HCHECK(hipMemset(d + batch, 0, (mb - (size_t)batch) * sizeof(hsqp_observe_instance)));   // neutral: all bits zero
  h->observe_B = batch;
  return HSQP_OK;
}
int hsqp_observe_set_instances(hsqp_handle* h, int batch, const hsqp_observe_instance* table) { return observe_set_instances_impl(h, batch, table, false); }
int hsqp_observe_set_instances_device(hsqp_handle* h, int batch, const hsqp_observe_instance* d_table) { return observe_set_instances_impl(h, batch, d_table, true); }
int hsqp_observe_clear(hsqp_handle* h) {
  if (!h) return HSQP_ERR_BAD_ARG;
  if (const int rc = observe_handle_ok(h, "hsqp_observe_clear")) return rc;
  const bool was = observe_in_force(h);
  h->observe_set = false;
  h->observe_B = 0;
  hsqp_observe_defaults(&h->observe);
  h->loop.obs_last = false;
  if (was && h->loop.started) {   // the policy time of step 4 is zero again
    HCHECK(hipSetDevice(h->device));
    HCHECK(hipMemsetAsync(h->loop.s0, 0, (size_t)h->loop.B * 8, h->stream));
    HCHECK(hipStreamSynchronize(h->stream));
  }
  return HSQP_OK;
}
int hsqp_observe_get(hsqp_handle* h, hsqp_observe_settings* s, int batch, hsqp_observe_instance* table) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_observe_get";
  if (const int rc = observe_handle_ok(h, who)) return rc;
  if (table && (batch < 1 || batch > h->st.max_batch)) return loop_bad(h, who, "batch outside [1, max_batch]");
  if (s) *s = h->observe;
  if (!table) return HSQP_OK;
  const int have = batch < h->observe_B ? batch : h->observe_B;
  if (have) {
    HCHECK(hipSetDevice(h->device));
    HCHECK(hipStreamSynchronize(h->stream));
    HCHECK(hipMemcpy(table, observe_table_layout(Carve{h->d_observe_table.p}, (size_t)h->st.max_batch).table, (size_t)have * sizeof(hsqp_observe_instance), hipMemcpyDeviceToHost));
  }
  for (int b = have; b < batch; ++b) hsqp_observe_instance_defaults(table + b);
  return HSQP_OK;
}
static int observe_eval_impl(hsqp_handle* h, int batch, uint32_t draw, const double* x, double* y, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_observe_eval_device" : "hsqp_observe_eval";
  if (const int rc = observe_handle_ok(h, who)) return rc;
  if (!x || !y) return loop_bad(h, who, "null x or y");
  if (batch < 1 || batch > h->st.max_batch) return loop_bad(h, who, "batch outside [1, max_batch]");
  HCHECK(hipSetDevice(h->device));
  const size_t B = (size_t)batch;
  ObserveArgs a{};
  a.table = h->observe_B ? observe_table_layout(Carve{h->d_observe_table.p}, (size_t)h->st.max_batch).table : nullptr;
  a.key0 = (uint32_t)(h->observe.seed & 0xffffffffu); a.key1 = (uint32_t)(h->observe.seed >> 32);
  a.draw = draw; a.B = batch; a.slots = 1;
  a.x = x; a.y = y;
  StickyError step{h};
  if (!dev) {
    DEV_ENSURE(h->d_observe_stage, observe_stage_layout(Carve{}, B).bytes, "observation staging");
    const ObserveStage sg = observe_stage_layout(Carve{h->d_observe_stage.p}, B);
    a.x = sg.x; a.y = sg.y;
    step(hipMemcpyAsync(sg.x, x, B * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x");
  }
  if (step.rc == HSQP_OK) {
    launch_observe(h, a);
    step(hipGetLastError(), "k_observe");
  }
  if (!dev) step(hipMemcpyAsync(y, a.y, B * NX * 8, hipMemcpyDeviceToHost, h->stream), "download y");
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}
int hsqp_observe_eval(hsqp_handle* h, int batch, uint32_t draw, const double* x, double* y) { return observe_eval_impl(h, batch, draw, x, y, false); }
int hsqp_observe_eval_device(hsqp_handle* h, int batch, uint32_t draw, const double* d_x, double* d_y) { return observe_eval_impl(h, batch, draw, d_x, d_y, true); }
static int observe_last_impl(hsqp_handle* h, double* y, double* t_p, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_observe_last_device" : "hsqp_observe_last";
  if (const int rc = observe_handle_ok(h, who)) return rc;
  const hsqp_handle::Loop& L = h->loop;
  if (!L.started || !L.obs_last) return loop_bad(h, who, "no completed cycle of a started loop with the observation model in force (hsqp_observe_set, hsqp_loop_run)");
  if (t_p) *t_p = L.obs_tp;
  if (y) {
    HCHECK(hipSetDevice(h->device));
    HCHECK(hipMemcpyAsync(y, L.obs_y[(L.cycle - 1) & 1], (size_t)L.B * NX * 8, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    HCHECK(hipStreamSynchronize(h->stream));
  }
  return HSQP_OK;
}
int hsqp_observe_last(hsqp_handle* h, double* y, double* t_p) { return observe_last_impl(h, y, t_p, false); }
int hsqp_observe_last_device(hsqp_handle* h, double* d_y, double* t_p) { return observe_last_impl(h, d_y, t_p, true); }

// ---- per-instance failure isolation and episode reset (include/hsqp_episode.h, csrc/hsqp_episode.h)
void hsqp_episode_defaults(hsqp_episode_settings* s) {
  if (!s) return;
  memset(s, 0, sizeof(*s));
  s->on_failure = HSQP_EPISODE_PARK;
  s->min_base_height = -HUGE_VAL; s->max_base_height = HUGE_VAL; s->max_tilt = HUGE_VAL;
}

int hsqp_loop_isolate(hsqp_handle* h, const hsqp_episode_settings* es, const double* x_reset) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_loop_isolate";
  { const int rc = loop_started(h, who); if (rc != HSQP_OK) return rc; }
  hsqp_handle::Loop& L = h->loop;
  if (!es) return loop_bad(h, who, "null settings");
  if (es->on_failure != HSQP_EPISODE_PARK && es->on_failure != HSQP_EPISODE_RESET) return loop_bad(h, who, "on_failure must be HSQP_EPISODE_PARK or HSQP_EPISODE_RESET");
  if (es->min_base_height != es->min_base_height || es->max_base_height != es->max_base_height || es->max_tilt != es->max_tilt) return loop_bad(h, who, "NaN bound");
  if (es->min_base_height > es->max_base_height) return loop_bad(h, who, "min_base_height > max_base_height");
  if (es->max_tilt < 0.0) return loop_bad(h, who, "max_tilt < 0");
  const size_t B = L.B;
  if (x_reset && !all_finite(x_reset, B * NX)) return loop_bad(h, who, "non-finite x_reset");
  if (x_reset && h->hdm.formulation == HSQP_FORM_CENTROIDAL) { const int rc = cent_rows_padding_ok(h, x_reset, B); if (rc != HSQP_OK) return rc; }
  // the gated sweeps take ONE verdict per batch (choose_sweep, the gate in hsqp_iterate_device): one instance's NaN would change the others' bits
  const int flags = h->st.flags;
  if ((flags & (HSQP_FLAG_SEGMENTED_RICCATI | HSQP_FLAG_PARALLEL_RICCATI)) ||
      (!(flags & HSQP_FLAG_SERIAL_RICCATI) && L.B <= HSQP_SCAN_AUTO_BATCH && L.st.n_nodes >= HSQP_SCAN_AUTO_MIN_NODES))
    return loop_bad(h, who, "this loop takes a KKT-gated backward sweep (parallel-in-time or two-level), whose gate is one verdict for the whole batch: "
                            "create the handle with HSQP_FLAG_SERIAL_RICCATI");
  HCHECK(hipSetDevice(h->device));
  L.isolate = false;
  DEV_ENSURE(h->d_episode, episode_layout(Carve{}, L, B), "episode arrays");
  episode_layout(Carve{h->d_episode.p}, L, B);
  const std::vector<int> zero(B, 0), none(B, -1), one(B, 1), shift(B, HSQP_WARM_SHIFT);
  StickyError step{h};
  step(hipMemcpyAsync(L.ep.state, zero.data(), B * 4, hipMemcpyHostToDevice, h->stream), "upload episode state");
  step(hipMemcpyAsync(L.ep.cause, zero.data(), B * 4, hipMemcpyHostToDevice, h->stream), "upload episode cause");
  step(hipMemcpyAsync(L.ep.fail_cycle, none.data(), B * 4, hipMemcpyHostToDevice, h->stream), "upload episode fail_cycle");
  step(hipMemcpyAsync(L.ep.n_failures, zero.data(), B * 4, hipMemcpyHostToDevice, h->stream), "upload episode n_failures");
  step(hipMemcpyAsync(L.ep.n_episodes, one.data(), B * 4, hipMemcpyHostToDevice, h->stream), "upload episode n_episodes");
  step(hipMemcpyAsync(L.ep.mode, shift.data(), B * 4, hipMemcpyHostToDevice, h->stream), "upload episode mode");
  step(hipMemcpyAsync(L.ep.reset, zero.data(), B * 4, hipMemcpyHostToDevice, h->stream), "upload episode flags");
  step(hipMemcpyAsync(L.x_reset, x_reset ? x_reset : L.x, B * NX * 8, x_reset ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, h->stream), "upload x_reset");
  step(hipMemcpyAsync(L.v_use, L.v_cmd, B * CMD_N * 8, hipMemcpyDeviceToDevice, h->stream), "copy v_cmd");
  step(hipStreamSynchronize(h->stream), "sync");
  if (step.rc != HSQP_OK) return step.rc;
  L.ep_st = *es;
  L.isolate = true;
  return HSQP_OK;
}

static int loop_isolated(hsqp_handle* h, const char* who) {
  { const int rc = loop_started(h, who); if (rc != HSQP_OK) return rc; }
  if (!h->loop.isolate) return loop_bad(h, who, "isolation is off (hsqp_loop_isolate; every hsqp_loop_start turns it off)");
  return HSQP_OK;
}

// the ids of a request on the started loop (hsqp_loop_reset_instances, hsqp_loop_metrics_restart): n >= 1 of them, each inside [0, B), none repeated
static int loop_ids_ok(hsqp_handle* h, const char* who, int n, const int32_t* ids) {
  const int B = h->loop.B;
  if (n < 1) return loop_bad(h, who, "n < 1");
  if (!ids) return loop_bad(h, who, "null ids");
  if (n > B) return loop_bad(h, who, "more ids than instances (an id is repeated)");
  std::vector<char> seen(B, 0);
  for (int i = 0; i < n; ++i) {
    if (ids[i] < 0 || ids[i] >= B) return loop_bad(h, who, "id outside [0, B)");
    if (seen[ids[i]]) return loop_bad(h, who, "repeated id");
    seen[ids[i]] = 1;
  }
  return HSQP_OK;
}

int hsqp_loop_reset_instances(hsqp_handle* h, int n, const int32_t* ids, const double* x0, const double* v_cmd) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_loop_reset_instances";
  { const int rc = loop_isolated(h, who); if (rc != HSQP_OK) return rc; }
  hsqp_handle::Loop& L = h->loop;
  { const int rc = loop_ids_ok(h, who, n, ids); if (rc != HSQP_OK) return rc; }
  if (x0 && !all_finite(x0, (size_t)n * NX)) return loop_bad(h, who, "non-finite x0");
  if (x0 && h->hdm.formulation == HSQP_FORM_CENTROIDAL) { const int rc = cent_rows_padding_ok(h, x0, (size_t)n); if (rc != HSQP_OK) return rc; }
  if (v_cmd && !all_finite(v_cmd, (size_t)n * CMD_N)) return loop_bad(h, who, "non-finite command");
  HCHECK(hipSetDevice(h->device));
  StickyError step{h};
  step(hipMemcpyAsync(L.req_ids, ids, (size_t)n * 4, hipMemcpyHostToDevice, h->stream), "upload ids");
  if (x0) step(hipMemcpyAsync(L.req_x0, x0, (size_t)n * NX * 8, hipMemcpyHostToDevice, h->stream), "upload x0");
  if (v_cmd) step(hipMemcpyAsync(L.req_v, v_cmd, (size_t)n * CMD_N * 8, hipMemcpyHostToDevice, h->stream), "upload v_cmd");
  if (step.rc == HSQP_OK) {
    const HostResetArgs a{L.req_ids, x0 ? L.req_x0 : nullptr, v_cmd ? L.req_v : nullptr, L.x_reset, L.ep, L.x, L.v_cmd, L.v_filt, L.v_use};
    HSQP_LAUNCH(k_episode_host_reset, dim3(n), dim3(64), 0, h->stream, a);
    if (L.metrics) HSQP_LAUNCH(k_metrics_host_close, dim3(n), dim3(64), 0, h->stream, (const int*)L.req_ids, L.met_rec, L.met_feet);   // the records close with END_HOST
    const bool obs = observe_in_force(h);
    const double lag = obs ? observe_policy_time(h->observe.compute_delay, L.st.period) : 0.0;
    if (L.gait)   // the gait's clock: the problem time of the next cycle (include/hsqp_observe.h)
      HSQP_LAUNCH(k_gait_reset_instances, dim3(n), dim3(64), 0, h->stream, h->gait.s[h->gait.cur], h->gait.st.max_events, (const int*)L.req_ids, (const int*)nullptr,
                  obs ? observe_problem_time(L.t, lag) : L.t);
    step(hipGetLastError(), "k_episode_host_reset");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}

static int loop_episodes_impl(hsqp_handle* h, int32_t* state, int32_t* cause, int32_t* fail_cycle, int32_t* n_failures, int32_t* n_episodes, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  { const int rc = loop_isolated(h, dev ? "hsqp_loop_episodes_device" : "hsqp_loop_episodes"); if (rc != HSQP_OK) return rc; }
  HCHECK(hipSetDevice(h->device));
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const EpisodeState& e = h->loop.ep;
  const size_t bytes = (size_t)h->loop.B * 4;
  if (state) HCHECK(hipMemcpyAsync(state, e.state, bytes, kind, h->stream));
  if (cause) HCHECK(hipMemcpyAsync(cause, e.cause, bytes, kind, h->stream));
  if (fail_cycle) HCHECK(hipMemcpyAsync(fail_cycle, e.fail_cycle, bytes, kind, h->stream));
  if (n_failures) HCHECK(hipMemcpyAsync(n_failures, e.n_failures, bytes, kind, h->stream));
  if (n_episodes) HCHECK(hipMemcpyAsync(n_episodes, e.n_episodes, bytes, kind, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  return HSQP_OK;
}
int hsqp_loop_episodes(hsqp_handle* h, int32_t* state, int32_t* cause, int32_t* fail_cycle, int32_t* n_failures, int32_t* n_episodes) {
  return loop_episodes_impl(h, state, cause, fail_cycle, n_failures, n_episodes, false);
}
int hsqp_loop_episodes_device(hsqp_handle* h, int32_t* d_state, int32_t* d_cause, int32_t* d_fail_cycle, int32_t* d_n_failures, int32_t* d_n_episodes) {
  return loop_episodes_impl(h, d_state, d_cause, d_fail_cycle, d_n_failures, d_n_episodes, true);
}

// ---- per-instance episode metrics (include/hsqp_metrics.h, csrc/hsqp_metrics.h)
static int metrics_loop_ok(hsqp_handle* h, const char* who, bool made) {
  if (h->hdm.formulation != HSQP_FORM_WB) return loop_bad(h, who, "whole-body handles only (the record reads the whole-body state row of the resident loop)");
  { const int rc = loop_started(h, who); if (rc != HSQP_OK) return rc; }
  if (made && !h->loop.metrics_made) return loop_bad(h, who, "no metrics since the loop was started (hsqp_loop_metrics_enable; every hsqp_loop_start turns them off)");
  return HSQP_OK;
}
int hsqp_loop_metrics_enable(hsqp_handle* h) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_loop_metrics_enable";
  { const int rc = metrics_loop_ok(h, who, false); if (rc != HSQP_OK) return rc; }
  hsqp_handle::Loop& L = h->loop;
  const size_t B = L.B;
  HCHECK(hipSetDevice(h->device));
  L.metrics = false; L.metrics_made = false;
  DEV_ENSURE(h->d_metrics, metrics_layout(Carve{}, L, B), "episode metrics");
  metrics_layout(Carve{h->d_metrics.p}, L, B);
  std::vector<hsqp_metrics> empty(2 * B);
  for (hsqp_metrics& r : empty)
    for (int i = 0; i < MET_WORDS; ++i) metrics_put_empty(&r, i);
  StickyError step{h};
  step(hipMemcpyAsync(L.met_rec, empty.data(), 2 * B * sizeof(hsqp_metrics), hipMemcpyHostToDevice, h->stream), "upload empty records");
  step(hipMemsetAsync(L.met_feet, 0, 2 * B * sizeof(int), h->stream), "memset feet");
  step(hipStreamSynchronize(h->stream), "sync");
  if (step.rc != HSQP_OK) return step.rc;
  L.metrics = true; L.metrics_made = true;
  return HSQP_OK;
}
int hsqp_loop_metrics_disable(hsqp_handle* h) {
  if (!h) return HSQP_ERR_BAD_ARG;
  { const int rc = metrics_loop_ok(h, "hsqp_loop_metrics_disable", false); if (rc != HSQP_OK) return rc; }
  h->loop.metrics = false;
  return HSQP_OK;
}
int hsqp_loop_metrics_restart(hsqp_handle* h, int n, const int32_t* ids) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = "hsqp_loop_metrics_restart";
  { const int rc = metrics_loop_ok(h, who, true); if (rc != HSQP_OK) return rc; }
  hsqp_handle::Loop& L = h->loop;
  if (ids) { const int rc = loop_ids_ok(h, who, n, ids); if (rc != HSQP_OK) return rc; }
  else n = L.B;
  HCHECK(hipSetDevice(h->device));
  StickyError step{h};
  if (ids) step(hipMemcpyAsync(L.met_ids, ids, (size_t)n * 4, hipMemcpyHostToDevice, h->stream), "upload ids");
  if (step.rc == HSQP_OK) {
    HSQP_LAUNCH(k_metrics_host_close, dim3(n), dim3(64), 0, h->stream, ids ? (const int*)L.met_ids : (const int*)nullptr, L.met_rec, L.met_feet);
    step(hipGetLastError(), "k_metrics_host_close");
  }
  step(hipStreamSynchronize(h->stream), "sync");
  return step.rc;
}
static int loop_metrics_impl(hsqp_handle* h, int which, hsqp_metrics* out, bool dev) {
  if (!h) return HSQP_ERR_BAD_ARG;
  const char* who = dev ? "hsqp_loop_metrics_device" : "hsqp_loop_metrics";
  { const int rc = metrics_loop_ok(h, who, true); if (rc != HSQP_OK) return rc; }
  if (which != HSQP_METRICS_CURRENT && which != HSQP_METRICS_PREVIOUS) return loop_bad(h, who, "which must be HSQP_METRICS_CURRENT or HSQP_METRICS_PREVIOUS");
  if (!out) return loop_bad(h, who, "null out");
  HCHECK(hipSetDevice(h->device));
  // record `which` of every instance's pair into its own array [B]
  HCHECK(hipMemcpy2DAsync(out, sizeof(hsqp_metrics), h->loop.met_rec + which, 2 * sizeof(hsqp_metrics), sizeof(hsqp_metrics), (size_t)h->loop.B,
                          dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
  HCHECK(hipStreamSynchronize(h->stream));
  return HSQP_OK;
}
int hsqp_loop_metrics(hsqp_handle* h, int which, hsqp_metrics* out) { return loop_metrics_impl(h, which, out, false); }
int hsqp_loop_metrics_device(hsqp_handle* h, int which, hsqp_metrics* d_out) { return loop_metrics_impl(h, which, d_out, true); }

int hsqp_last_kernel_ms(hsqp_handle* h, double out_ms[5]) {
  if (!h || !out_ms) return HSQP_ERR_BAD_ARG;
  for (int i = 0; i < 5; ++i) out_ms[i] = h->kernel_ms[i];
  return HSQP_OK;
}

long long hsqp_debug_read(hsqp_handle* h, int what, void* dst, long long bytes) {
  if (!h) return HSQP_ERR_BAD_ARG;
  // a block that is a plain device array of `size` bytes: its first min(bytes, size) bytes to dst
  auto copy_block = [&](const void* src, long long size) -> long long {
    if (dst && bytes > 0 && hipMemcpy(dst, src, (size_t)std::min(bytes, size), hipMemcpyDeviceToHost) != hipSuccess) return HSQP_ERR_HIP;
    return size;
  };
  if (what == HSQP_BLK_FORMS) {
    const int forms[5] = {h->lq_limb ? 1 : 0, h->value_quad ? 1 : 0, h->lq_limb ? h->lq_split : 0, h->ric_fact ? 1 : 0, h->chain_fused ? 1 : 0};
    if (dst && bytes > 0) memcpy(dst, forms, (size_t)(bytes < 20 ? bytes : 20));
    return 20;
  }
  if (what == HSQP_BLK_PARAMS) {   // available as soon as a problem is resident
    if (!h->have_problem) { h->err = "no problem uploaded"; return HSQP_ERR_BAD_ARG; }
    if (hipSetDevice(h->device) != hipSuccess) return HSQP_ERR_HIP;
    return copy_block(h->d_par, (long long)h->B * (h->N + 1) * NP * 8);
  }
  if (what == HSQP_BLK_X || what == HSQP_BLK_U || what == HSQP_BLK_STAMPS) {   // the resident linearisation trajectory and grid stamps
    if (!h->have_problem || (what == HSQP_BLK_STAMPS && !h->have_stamps)) {
      h->err = what == HSQP_BLK_STAMPS ? "no stamps: the resident problem was not uploaded through hsqp_upload_reference" : "no problem uploaded";
      return HSQP_ERR_BAD_ARG;
    }
    if (hipSetDevice(h->device) != hipSuccess) return HSQP_ERR_HIP;
    const double* src = what == HSQP_BLK_X ? h->d_x : what == HSQP_BLK_U ? h->d_u : h->d_stamps[h->stamps_cur];
    return copy_block(src, (long long)h->B * (what == HSQP_BLK_X ? (h->N + 1) * NX : what == HSQP_BLK_U ? h->N * NU : h->N + 1) * 8);
  }
  if (!h->have_solution) { h->err = "no iteration has run"; return HSQP_ERR_BAD_ARG; }
  if (hipSetDevice(h->device) != hipSuccess) return HSQP_ERR_HIP;
  const size_t B = h->B, N = h->N, nodes = B * N;
  std::vector<double> out;
  std::vector<int> iout;
  auto fetch_rec = [&](std::vector<double>& rec) {
    rec.resize(nodes * (size_t)REC_SIZE);
    return hipMemcpy(rec.data(), h->d_rec, rec.size() * 8, hipMemcpyDeviceToHost) == hipSuccess;
  };
  std::vector<double> rec;
  // a zero-length interval is solved as the identity jump (k_jump overwrites its QP record): the stage has no equality rows, whatever the LQ kernels
  // left in the node's record at dt = 0
  auto event_node = [&](size_t n) { return h->h_dt.size() == nodes && h->h_dt[n] == 0.0; };
  switch (what) {
    case HSQP_BLK_AB: {
      if (!fetch_rec(rec)) return HSQP_ERR_HIP;
      out.resize(nodes * NX * NZ);
      for (size_t n = 0; n < nodes; ++n) {
        if (h->hdm.formulation == HSQP_FORM_CENTROIDAL) cent_expand_AB(&rec[n * REC_SIZE], h->h_dt[n], &out[n * NX * NZ]);
        else {
          if (h->lq_limb && h->chain_fused) {   // REC_PV is not written on this handle (k_project chains the columns itself): the same chain here, from the stage Jacobians
            double* r = &rec[n * REC_SIZE];
            double blk[3][2][6][6];
            for (int i = 0; i < 3 * 72; ++i) blk[i / 72][(i / 36) % 2][(i / 6) % 6][i % 6] = r[REC_GS + lq_chain_blk_offset(i / 72, (i / 36) % 2, (i / 6) % 6, i % 6)];
            for (int col = 0; col < LDJ; ++col) lq_chain_column<true>(blk, r + REC_GS, col, h->h_dt[n], r);
          }
          expand_AB(&rec[n * REC_SIZE], h->h_dt[n], &out[n * NX * NZ]);
        }
      }
      break;
    }
    case HSQP_BLK_BVEC: case HSQP_BLK_FLOW: {
      if (!fetch_rec(rec)) return HSQP_ERR_HIP;
      out.resize(nodes * NX);
      const int off = what == HSQP_BLK_BVEC ? REC_B : REC_FLOW;
      for (size_t n = 0; n < nodes; ++n) memcpy(&out[n * NX], &rec[n * REC_SIZE + off], NX * 8);
      break;
    }
    case HSQP_BLK_H: case HSQP_BLK_G: {
      if (!fetch_rec(rec)) return HSQP_ERR_HIP;
      const bool isH = what == HSQP_BLK_H;
      out.assign(nodes * (isH ? NZ * NZ : NZ), 0.0);
      for (size_t n = 0; n < nodes; ++n) {
        const double* r = &rec[n * REC_SIZE];
        const int nrows = (int)r[REC_NROWS];
        for (int a = 0; a < NZ; ++a) {
          if (isH) {
            for (int b = 0; b < NZ; ++b) {
              double s = a == b ? r[REC_D + a] : 0.0;
              for (int k = 0; k < nrows; ++k) s += rec_J_at(r, k, a) * rec_J_at(r, k, b);
              out[n * NZ * NZ + a * NZ + b] = s;
            }
          } else {
            double s = r[REC_GD + a];
            for (int k = 0; k < nrows; ++k) s += rec_J_at(r, k, a) * r[REC_RHO + k];
            out[n * NZ + a] = s;
          }
        }
      }
      break;
    }
    case HSQP_BLK_CDE: {
      if (!fetch_rec(rec)) return HSQP_ERR_HIP;
      out.resize(nodes * NE_MAX * (NZ + 1));
      for (size_t n = 0; n < nodes; ++n)
        for (int r = 0; r < NE_MAX; ++r) for (int c = 0; c <= NZ; ++c) out[(n * NE_MAX + r) * (NZ + 1) + c] = event_node(n) ? 0.0 : rec_CDe_at(&rec[n * REC_SIZE], r, c);
      break;
    }
    case HSQP_BLK_NE: {
      if (!fetch_rec(rec)) return HSQP_ERR_HIP;
      iout.resize(nodes);
      for (size_t n = 0; n < nodes; ++n) iout[n] = event_node(n) ? 0 : (int)rec[n * REC_SIZE + REC_MISC];
      break;
    }
    case HSQP_BLK_COST: {
      if (!fetch_rec(rec)) return HSQP_ERR_HIP;
      std::vector<double> x(B * (N + 1) * NX), par(B * (N + 1) * NP);
      if (hipMemcpy(x.data(), h->d_x, x.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return HSQP_ERR_HIP;
      if (hipMemcpy(par.data(), h->d_par, par.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return HSQP_ERR_HIP;
      out.resize(B * (N + 1));
      for (size_t b = 0; b < B; ++b) {
        for (size_t k = 0; k < N; ++k) out[b * (N + 1) + k] = rec[(b * N + k) * REC_SIZE + REC_MISC + 1];
        double c = 0.0;
        for (int i = 0; i < NX; ++i) { const double d = x[(b * (N + 1) + N) * NX + i] - par[(b * (N + 1) + N) * NP + HSQP_P_XDES + i]; c += 0.5 * h->hdm.Qf[i] * d * d; }
        out[b * (N + 1) + N] = c;
      }
      break;
    }
    case HSQP_BLK_DX: return copy_block(h->d_dx, (long long)(B * (N + 1) * NX * 8));
    case HSQP_BLK_DU: return copy_block(h->d_du, (long long)(B * N * NU * 8));
    case 100: return copy_block(h->d_prof, 4 * 128 * 8);   // phase-profile ticks (only meaningful in -DHSQP_PHASE_PROFILE builds)
    case 101: return copy_block(h->d_ric, (long long)(nodes * RIC_SIZE * 8));   // raw gains record (debug tools)
    case 102:   // raw QP record (debug tools)
      if (!h->qp_joint_rows) {
        h->err = "block 102: the last k_project did not write the joint rows of A~ / B~ or the lower triangle of Q~ (whole-body serial sweep without a KKT report)";
        return HSQP_ERR_BAD_ARG;
      }
      return copy_block(h->d_qp, (long long)(nodes * QP_SIZE * 8));
    default: h->err = "unknown block id"; return HSQP_ERR_BAD_ARG;
  }
  const long long size = iout.empty() ? (long long)out.size() * 8 : (long long)iout.size() * 4;
  const void* src = iout.empty() ? (const void*)out.data() : (const void*)iout.data();
  if (dst && bytes > 0) memcpy(dst, src, (size_t)(bytes < size ? bytes : size));
  return size;
}

}  // extern "C"
