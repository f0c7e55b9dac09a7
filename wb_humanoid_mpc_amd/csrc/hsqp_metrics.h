// Per-instance episode metrics of the resident loop (include/hsqp_metrics.h): the sample ONE instance adds to its open record behind the rollout of a
// cycle, and the closing / reopening of a record at an episode boundary.
//
// Shape: one workgroup of RO_THREADS per instance (Ctx::nthreads == 1 on the host).  Under isolation the verdict is the triage's own
// (episode_verdict, csrc/hsqp_episode.h) on the same words; its row test is a ONE-wave ballot, so wave 0 computes it and passes it through the
// workspace.  Every branch is uniform across the workgroup.  With a ground the contact model at the rolled-out state is formed by
// contact_eval_instance (csrc/hsqp_contact.h) as it is, outputs in the workspace; without one (MetricsNoGround) the workspace is one word and no
// stage is evaluated.  The sample itself is scalar work: lane 0 reads and rewrites the record, every per-joint and per-corner sum in index order.
// A record moves as MET_WORDS 8-byte words, written by the lanes side by side; everything is an ordinary vector store.
//
// Arithmetic: plain double, never contracted, so the host build of this source (tests/metrics/metrics_emu.cpp, -ffp-contract=off) agrees with the
// device apart from sin / cos and from what stage_eval contributes to the ground group.
#pragma once
#include <cstddef>

#include "hsqp_contact.h"
#include "hsqp_episode.h"
#include "../../include/hsqp_metrics.h"

namespace hsqp {

constexpr int MET_WORDS = (int)(sizeof(hsqp_metrics) / 8);
constexpr int MET_INTS = (int)(offsetof(hsqp_metrics, duration) / 8);   // the leading words are the int64 counts
static_assert(sizeof(hsqp_metrics) == 35 * 8 && MET_INTS == 12, "hsqp_metrics is 12 counts and 23 doubles, 8 bytes each");

struct MetricsArgs {
  int isolate;                   // the loop runs under isolation: the verdict decides, ep_state is read
  int cycle;                     // index of the cycle that has just been rolled out, counted from hsqp_loop_start
  hsqp_episode_settings st;
  double period;
  const int* it_status;          // [B] status words of the iteration
  const hsqp_perf* perf;         // [B] performance index after the step
  const int32_t* ro_status;      // [B] HSQP_ROLLOUT_*
  const double* xs;              // [B][NX] the rolled-out state
  const double* x_before;        // [B][NX] the plant state the rollout started from
  const double* cmd;             // [B][CMD_N] the command step 1 of the cycle read
  const int* ep_state;           // [B] HSQP_EP_* before the cycle's triage (isolate only)
  const int32_t* steps;          // [B] accepted / rejected integrator steps of the cycle's rollout
  const int32_t* rejected;
  const double* act_last;        // [B][3][NJ] the record of hsqp_actuator_last, or null: the actuator model is not in force
  const double* act_limit;       // [NJ] the resident effort limits
  hsqp_metrics* rec;             // [B][2] CURRENT, PREVIOUS
  int* feet;                     // [B][2] per foot: loaded in the open record's last ground sample
  const double* ground;          // [B] the estimated ground the triage's height box stands on (include/hsqp_ground.h, box_above_ground), or null
};

struct MetricsNoGround {};
template <class CT>
struct MetricsWST {
  ContactEvalWST<CT> ce;
  double force[CT_PTS * 3], pen[CT_PTS];
  int verdict;
};
template <>
struct MetricsWST<MetricsNoGround> {
  int verdict;
};

// word i of an empty record into r
HSQP_HD void metrics_put_empty(hsqp_metrics* r, int i) {
  char* p = reinterpret_cast<char*>(r) + 8 * i;
  if (i < MET_INTS) {
    const int64_t v = (i == (int)(offsetof(hsqp_metrics, first_cycle) / 8) || i == (int)(offsetof(hsqp_metrics, end_cause) / 8)) ? -1 : 0;
    __builtin_memcpy(p, &v, 8);
  } else {
    const double v = i == (int)(offsetof(hsqp_metrics, height_min) / 8) ? __builtin_inf() : (i == (int)(offsetof(hsqp_metrics, height_max) / 8) ? -__builtin_inf() : 0.0);
    __builtin_memcpy(p, &v, 8);
  }
}
HSQP_HD void metrics_open(const Ctx& ctx, hsqp_metrics* r, int* feet) {
  WG_FOR(ctx, i, MET_WORDS) metrics_put_empty(r, i);
  WG_FOR(ctx, i, 2) feet[i] = 0;
}

// rec[0] (CURRENT) is closed with `cause` and becomes rec[1] (PREVIOUS), rec[0] becomes empty; an empty CURRENT: nothing happens
HSQP_HD void metrics_close(const Ctx& ctx, hsqp_metrics* rec, int cause, int* feet) {
  const bool empty = rec[0].cycles == 0;
  WG_SYNC(ctx);   // every lane has read the count the lanes rewrite below
  if (empty) return;
  const int end = (int)(offsetof(hsqp_metrics, end_cause) / 8);
  WG_FOR(ctx, i, MET_WORDS) {
    int64_t v;
    __builtin_memcpy(&v, reinterpret_cast<const char*>(rec) + 8 * i, 8);
    if (i == end) v = cause;
    __builtin_memcpy(reinterpret_cast<char*>(rec + 1) + 8 * i, &v, 8);
  }
  metrics_open(ctx, rec, feet);   // (word i of CURRENT is read and rewritten by the same lane)
}

HSQP_HD double metrics_max(double m, double v) { return v > m ? v : m; }

// the sample of one cycle into the open record r (include/hsqp_metrics.h).  ONE lane.  force [8][3], pen [8]: the contact model at the rolled-out
// state, or null: no ground in force
HSQP_HD void metrics_sample(const MetricsArgs& a, int b, const double* force, const double* pen, hsqp_metrics& r, int* feet) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double* x = a.xs + (size_t)b * NX;
  const double* x0 = a.x_before + (size_t)b * NX;
  const double* cmd = a.cmd + (size_t)b * CMD_N;
  const double T = a.period;
  if (r.cycles == 0) { r.first_cycle = a.cycle; r.start_xy[0] = x0[0]; r.start_xy[1] = x0[1]; }
  r.cycles += 1;
  r.duration = (double)r.cycles * T;
  // motion
  const double c = cos(x[3]), s = sin(x[3]);
  const double wx = c * cmd[0] - s * cmd[1], wy = s * cmd[0] + c * cmd[1];
  const double ex = x[NV] - wx, ey = x[NV + 1] - wy;
  const double e2 = ex * ex + ey * ey;
  r.vel_err_sq += e2;
  r.vel_err_max = metrics_max(r.vel_err_max, sqrt(e2));
  const double ew = x[NV + 3] - cmd[3], eh = x[2] - cmd[2];
  r.yaw_rate_err_sq += ew * ew;
  r.height_err_sq += eh * eh;
  if (x[2] < r.height_min) r.height_min = x[2];
  if (x[2] > r.height_max) r.height_max = x[2];
  r.tilt_max = metrics_max(r.tilt_max, metrics_max(fabs(x[4]), fabs(x[5])));
  const double dx = x[0] - x0[0], dy = x[1] - x0[1];
  r.path_length += sqrt(dx * dx + dy * dy);
  r.end_xy[0] = x[0]; r.end_xy[1] = x[1];
  // torque
  if (a.act_last) {
    const double* tc = a.act_last + (size_t)b * 3 * NJ;
    const double* ta = tc + NJ;
    const double inf = __builtin_inf();
    int sat = 0;
    double sq = 0.0, ratio = 0.0, wp = 0.0, wa = 0.0;
    for (int j = 0; j < NJ; ++j) {
      const double lim = a.act_limit[j], ac = fabs(tc[j]);
      if (ac > lim) ++sat;
      ratio = metrics_max(ratio, lim == inf ? 0.0 : ac / lim);
      sq += ta[j] * ta[j];
      const double p = ta[j] * x[NV + 6 + j];
      wp += p > 0.0 ? p : 0.0;
      wa += fabs(p);
    }
    r.torque_samples += 1;
    r.saturated_joint_samples += sat;
    if (sat) r.saturated_samples += 1;
    r.tau_sq += sq;
    r.tau_ratio_max = metrics_max(r.tau_ratio_max, ratio);
    r.work_pos += T * wp;
    r.work_abs += T * wa;
  }
  // ground
  if (force) {
    int loaded[HSQP_CONTACT_FEET] = {0, 0};
    double load = 0.0, dmax = r.penetration_max;
    for (int i = 0; i < CT_PTS; ++i) {
      const double* f = force + 3 * i;
      if (f[0] != 0.0 || f[1] != 0.0 || f[2] != 0.0) loaded[i / HSQP_CONTACT_CORNERS] = 1;
      load += f[2];
      dmax = metrics_max(dmax, pen[i]);
    }
    if (!loaded[0] && !loaded[1]) r.flight_samples += 1;
    for (int f = 0; f < HSQP_CONTACT_FEET; ++f) {
      if (r.ground_samples > 0 && loaded[f] && !feet[f]) r.touchdowns[f] += 1;
      feet[f] = loaded[f];
    }
    r.ground_samples += 1;
    r.load_sum += load;
    r.load_max = metrics_max(r.load_max, load);
    r.penetration_max = dmax;
  }
  // solver
  const hsqp_perf& pf = a.perf[b];
  r.cost_sum += pf.cost;
  r.dynamics_sse_max = metrics_max(r.dynamics_sse_max, pf.dynamics_sse);
  r.equality_sse_max = metrics_max(r.equality_sse_max, pf.equality_sse);
  r.rollout_steps += a.steps[b];
  r.rollout_rejected += a.rejected[b];
}

// Instance b behind the rollout of cycle a.cycle, BEFORE step 5 and the triage overwrite the state the rollout started from and the command.
// CT: MetricsNoGround, ContactSet, or ContactTerrainSet while a terrain is resident (tp is read by that one only).
template <class CT>
HSQP_HD void metrics_instance(const Ctx& ctx, const DevModel& dm, MetricsWST<CT>& w, const MetricsArgs& a, const ContactParams& cp, const TerrainParams* tp, int b) {
  hsqp_metrics* rec = a.rec + (size_t)b * 2;
  int* feet = a.feet + (size_t)b * 2;
  const double* xs = a.xs + (size_t)b * NX;
  int before = HSQP_EP_ALIVE, cause = HSQP_EP_ALIVE;
  if (a.isolate) {
    before = a.ep_state[b];
    if (ctx.tid < 64) {   // (one wave: episode_row_finite is a one-wave ballot)
      const int v = episode_verdict(ctx, a.st, a.it_status[b], a.perf[b], a.ro_status[b], xs, a.ground ? a.ground + b : nullptr);
      if (ctx.tid == 0) w.verdict = v;
    }
    WG_SYNC(ctx);
    cause = w.verdict;
  }
  if (cause != HSQP_EP_ALIVE) { metrics_close(ctx, rec, cause, feet); return; }   // the failing cycle is not accumulated
  if (before != HSQP_EP_ALIVE) return;                                              // parked
  const double* force = nullptr;
  const double* pen = nullptr;
  if constexpr (!std::is_same<CT, MetricsNoGround>::value) {
    contact_eval_instance(ctx, dm, w.ce, cp, tp, b, xs, w.force, w.pen);
    WG_SYNC(ctx);
    force = w.force; pen = w.pen;
  } else {
    (void)dm; (void)cp; (void)tp;
  }
  if (ctx.tid == 0) metrics_sample(a, b, force, pen, rec[0], feet);
}

// hsqp_loop_reset_instances / hsqp_loop_metrics_restart, entry i of the request: the record of instance ids[i] (ids null: instance i) is closed by the host
HSQP_HD void metrics_host_close(const Ctx& ctx, const int* ids, hsqp_metrics* rec, int* feet, int i) {
  const int b = ids ? ids[i] : i;
  metrics_close(ctx, rec + (size_t)b * 2, HSQP_METRICS_END_HOST, feet + (size_t)b * 2);
}

}  // namespace hsqp
