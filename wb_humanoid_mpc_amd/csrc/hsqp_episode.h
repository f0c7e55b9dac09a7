// Per-instance failure isolation and episode reset of the resident loop (include/hsqp_episode.h): the triage of ONE instance behind the
// rollout of a cycle, the host-requested reset of one instance, the command in use, and the per-instance form of the gait reset.
//
// Shape: one wave per instance (Ctx::nthreads == 64 on the device, 1 on the host).  The verdict is computed from four words and one state
// row, identically by every lane (the row's finiteness is one ballot), so every branch below is uniform; the rows an instance owns (measured
// state, filter state, command in use, log rows, gait rows) are written by the lanes side by side, the scalars by lane 0, all with ordinary
// vector stores.  Nothing is read back by the host: the verdict stays in the resident episode arrays.
//
// No arithmetic but t + 0.5 (the initial schedule's event, as the host computes it in gait_reset_impl): comparisons and copies, so the device,
// the host build of this source (tests/episode/episode_emu.cpp) and the numpy restatement (tests/test_episode.py) agree exactly.
#pragma once
#include "hsqp_common.h"
#include "hsqp_gait.h"
#include "hsqp_loop.h"
#include "../../include/hsqp_episode.h"
#include "../../include/hsqp_rollout.h"

namespace hsqp {

// the resident episode arrays of a batch, [B] each: state / cause (HSQP_EP_*), fail_cycle, n_failures, n_episodes, the warm-start mode of the
// next cycle (HSQP_WARM_SHIFT / _COLD) and the flag "start a new episode" the per-instance gait reset reads
struct EpisodeState { int* state; int* cause; int* fail_cycle; int* n_failures; int* n_episodes; int* mode; int* reset; };

struct TriageArgs {
  hsqp_episode_settings st;
  int cycle;                     // index of the cycle that has just run, counted from hsqp_loop_start
  const int* it_status;          // [B] status words of the iteration
  const hsqp_perf* perf;         // [B] performance index after the step
  const int32_t* ro_status;      // [B] HSQP_ROLLOUT_*
  const double* xs;              // [B][NX] the rolled-out state
  const double* x_reset;         // [B][NX]
  const double* v_cmd;           // [B][CMD_N]
  EpisodeState ep;
  double* x;                     // [B][NX] the measured state of the next cycle (already the rolled-out one)
  double* v_filt;                // [B][CMD_N] the filter state of the next cycle (already advanced)
  double* v_use;                 // [B][CMD_N] the command in use from the next cycle on
  double* x_log; double* u_log;  // row `cycle` of the logs, [B][NX] / [B][NU], or null
  const double* ground;          // [B] the estimated ground (include/hsqp_ground.h, box_above_ground): the height test is on xs[2] - ground[b]; or null
  int pose = 0;                  // where the base pose [x, y, z, yaw, pitch, roll] starts in a state row: EPISODE_POSE_WB or EPISODE_POSE_CENT
};
constexpr int EPISODE_POSE_WB = 0, EPISODE_POSE_CENT = 6;   // whole-body rows begin with the pose; centroidal rows carry the normalised momentum in front of it

HSQP_HD bool episode_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and +-inf

// every entry of row[0 .. n) is finite (n <= 64 on the device: one ballot)
HSQP_HD bool episode_row_finite(const Ctx& ctx, const double* row, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
  const bool bad = ctx.tid < n && !episode_finite(row[ctx.tid]);
  return __ballot(bad) == 0ull;
#else
  (void)ctx;
  for (int i = 0; i < n; ++i) if (!episode_finite(row[i])) return false;
  return true;
#endif
}

// the verdict on one instance (include/hsqp_episode.h, step 6): HSQP_EP_ALIVE or the first cause that applies
// ground (may be null): the estimated ground under the instance, the base-height box is then above it; pose: the row's pose offset
HSQP_HD int episode_verdict(const Ctx& ctx, const hsqp_episode_settings& st, int it_status, const hsqp_perf& perf, int ro_status, const double* xs,
                            const double* ground = nullptr, int pose = 0) {
  if (it_status != 0 || !episode_finite(perf.merit) || !episode_finite(perf.cost) || !episode_finite(perf.dynamics_sse) || !episode_finite(perf.equality_sse))
    return HSQP_EP_FAILED_NUMERIC;
  if (ro_status != HSQP_ROLLOUT_OK || !episode_row_finite(ctx, xs, NX)) return HSQP_EP_FAILED_ROLLOUT;
  const double* p = xs + pose;
  const double height = ground ? p[2] - *ground : p[2];
  if (height < st.min_base_height || height > st.max_base_height || fabs(p[4]) > st.max_tilt || fabs(p[5]) > st.max_tilt) return HSQP_EP_FAILED_BOUNDS;
  return HSQP_EP_ALIVE;
}

// the command an instance in `state` uses: its own, or parked the stance command {0, 0, x_reset[pose + 2], 0}
HSQP_HD double episode_command_entry(int state, const double* v_cmd, const double* x_reset, int i, int pose = 0) {
  if (state == HSQP_EP_ALIVE) return v_cmd[i];
  return i == 2 ? x_reset[pose + 2] : 0.0;
}
HSQP_HD void episode_command_in_use(const Ctx& ctx, int state, const double* v_cmd, const double* x_reset, double* v_use, int pose = 0) {
  WG_FOR(ctx, i, CMD_N) v_use[i] = episode_command_entry(state, v_cmd, x_reset, i, pose);
}

// Instance b behind the rollout of cycle a.cycle.  Returns the verdict.
HSQP_HD int triage_instance(const Ctx& ctx, const TriageArgs& a, int b) {
  const EpisodeState& ep = a.ep;
  const double* xs = a.xs + (size_t)b * NX;
  const double* xr = a.x_reset + (size_t)b * NX;
  const double* vc = a.v_cmd + (size_t)b * CMD_N;
  const int before = ep.state[b];
  const int cause = episode_verdict(ctx, a.st, a.it_status[b], a.perf[b], a.ro_status[b], xs, a.ground ? a.ground + b : nullptr, a.pose);
  const bool failed = cause != HSQP_EP_ALIVE;
  const int after = failed ? (a.st.on_failure == HSQP_EPISODE_RESET ? HSQP_EP_ALIVE : cause) : before;
  WG_SYNC(ctx);   // every lane has read the words lane 0 rewrites below
  if (failed) {
    WG_FOR(ctx, i, NX) a.x[(size_t)b * NX + i] = xr[i];
    WG_FOR(ctx, i, CMD_N) a.v_filt[(size_t)b * CMD_N + i] = episode_command_entry(after, vc, xr, i, a.pose);
  }
  episode_command_in_use(ctx, after, vc, xr, a.v_use + (size_t)b * CMD_N, a.pose);
  if (failed || before != HSQP_EP_ALIVE) {   // the row of a failed cycle, and every row of a parked instance
    const double nan = __builtin_nan("");
    if (a.x_log) WG_FOR(ctx, i, NX) a.x_log[(size_t)b * NX + i] = nan;
    if (a.u_log) WG_FOR(ctx, i, NU) a.u_log[(size_t)b * NU + i] = nan;
  }
  if (ctx.tid == 0) {
    if (failed) {
      ep.state[b] = after; ep.cause[b] = cause; ep.fail_cycle[b] = a.cycle; ep.n_failures[b] += 1;
      if (a.st.on_failure == HSQP_EPISODE_RESET) ep.n_episodes[b] += 1;
    }
    ep.mode[b] = failed ? HSQP_WARM_COLD : HSQP_WARM_SHIFT;
    ep.reset[b] = failed ? 1 : 0;
  }
  return cause;
}

// hsqp_loop_reset_instances, entry i of the request: instance ids[i] starts a new episode from x0 row i (null: its x_reset) with the command
// v_new row i (null: the one it has)
struct HostResetArgs {
  const int* ids; const double* x0; const double* v_new;
  const double* x_reset;
  EpisodeState ep;
  double* x; double* v_cmd; double* v_filt; double* v_use;
};
HSQP_HD void host_reset_instance(const Ctx& ctx, const HostResetArgs& a, int i) {
  const int b = a.ids[i];
  const double* xsrc = a.x0 ? a.x0 + (size_t)i * NX : a.x_reset + (size_t)b * NX;
  WG_FOR(ctx, k, NX) a.x[(size_t)b * NX + k] = xsrc[k];
  WG_FOR(ctx, k, CMD_N) {
    const double v = a.v_new ? a.v_new[(size_t)i * CMD_N + k] : a.v_cmd[(size_t)b * CMD_N + k];
    a.v_cmd[(size_t)b * CMD_N + k] = v; a.v_filt[(size_t)b * CMD_N + k] = v; a.v_use[(size_t)b * CMD_N + k] = v;
  }
  if (ctx.tid == 0) {
    a.ep.state[b] = HSQP_EP_ALIVE; a.ep.n_episodes[b] += 1;
    a.ep.mode[b] = HSQP_WARM_COLD; a.ep.reset[b] = 1;
  }
}

// hsqp_gait_reset for ONE instance at time t: schedule {[t + 0.5], [STANCE, STANCE]} (every entry of the rows, as the batch reset fills them),
// rung 0, its template, both gait commands rung 0, lastGaitChangeTime = t
HSQP_HD void gait_reset_instance(const Ctx& ctx, const GaitState& s, int E, int b, double t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double first = t + 0.5;
  WG_FOR(ctx, i, E) s.ev[(size_t)b * E + i] = first;
  WG_FOR(ctx, i, E + 1) s.seq[(size_t)b * (E + 1) + i] = HSQP_MODE_STANCE;
  WG_FOR(ctx, i, GAIT_SCAL) s.scal[b * GAIT_SCAL + i] = 0;
  if (ctx.tid == 0) { s.n[b] = 1; s.t_change[b] = t; }
}

}  // namespace hsqp
