// Per-instance gait schedule and gait ladder (include/hsqp_gait.h): the update of ONE instance, restated from
//   GaitSchedule::insertModeSequenceTemplate / getModeSchedule / tileModeSequenceTemplate   (humanoid_common_mpc/src/gait/GaitSchedule.cpp:53-145)
//   GaitScheduleUpdater::updateGaitSchedule                                                 (…/src/gait/GaitScheduleUpdater.cpp:45-69)
//   ProceduralMpcMotionManager::transitionToFasterGait / …SlowerGait / preSolverRun         (…/src/reference_manager/ProceduralMpcMotionManager.cpp:86-159)
// as reference.gait_cycle restates it on the host.
//
// Shape: one wave per instance (Ctx::nthreads == 64 on the device, 1 on the host).  The live row of the schedule is read from global memory
// and copied, trimmed, into a work row (LDS on the device); from then on the schedule is a VIEW [off, off + n) of that row: an erase at the
// front moves `off`, an erase at the back lowers `n`, nothing is shifted in place.  lower_bound / upper_bound on the sorted row are a ballot
// and a population count per 64 events.  The tiling's running sum is a serial chain, eventTimes.back() + (T[i + 1] - T[i]) one event after
// the other exactly as the reference accumulates it (a prefix scan would round differently): every lane carries the chain in its registers,
// so the view's size and status stay uniform, and lane 0 stores the events into the row, from where all lanes copy them out coalesced.
// The update reads the live state and writes the shadow state (gait_update_instance's `in` / `out`): the caller swaps them.
//
// Arithmetic: additions, subtractions, one two-term product sum, comparisons — unfused (`#pragma clang fp contract(off)`), so the device, the
// host build of this source (tests/gait/gait_emu.cpp, -ffp-contract=off) and the Python mirror agree bit for bit.
#pragma once
#include "hsqp_common.h"
#include "../../include/hsqp_gait.h"

namespace hsqp {

constexpr int GAIT_SCAL = 4;   // int32 scalars of an instance: rung (currentGaitMode_), currentGaitCommand_, lastGaitCommand_, the template's rung
constexpr int GAIT_WORK_EVENTS = 2 * HSQP_GAIT_MAX_EVENTS;   // a view starts at most max_events into its row and holds at most max_events

// the state of a batch: n [B], ev [B][E], seq [B][E + 1], scal [B][GAIT_SCAL], t_change [B]
struct GaitState { int* n; double* ev; int* seq; int* scal; double* t_change; };
// the work row of one instance: ev [GAIT_WORK_EVENTS], seq [GAIT_WORK_EVENTS + 1]
struct GaitWork { double ev[GAIT_WORK_EVENTS]; int seq[GAIT_WORK_EVENTS + 1]; };

struct GaitView {
  double* ev; int* seq;   // the work row
  int off, n, m;          // events [off, off + n), modes [off, off + m)
  int max_events, status;
  double back;            // ev[off + n - 1] (valid while n > 0)
};

// number of ev[0 .. n) below x (upper: not above x): std::lower_bound / std::upper_bound on the sorted row
HSQP_HD int gait_bound(const Ctx& ctx, const double* ev, int n, double x, bool upper) {
  int c = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  for (int base = 0; base < n; base += 64) {   // n is uniform: every lane takes part in every ballot
    const int i = base + ctx.tid;
    const bool p = i < n && (upper ? ev[i] <= x : ev[i] < x);
    c += __popcll(__ballot(p));
  }
#else
  for (int i = 0; i < n; ++i) c += (upper ? ev[i] <= x : ev[i] < x) ? 1 : 0;
#endif
  return c;
}

HSQP_HD void gait_push_event(const Ctx& ctx, GaitView& v, double t) {
  if (v.status != HSQP_GAIT_OK) return;
  if (v.n >= v.max_events) { v.status = HSQP_GAIT_OVERFLOW; return; }
  if (ctx.tid == 0) v.ev[v.off + v.n] = t;
  ++v.n;
  v.back = t;
}
HSQP_HD void gait_push_mode(const Ctx& ctx, GaitView& v, int mode) {
  if (v.status != HSQP_GAIT_OK) return;
  if (v.m > v.max_events) { v.status = HSQP_GAIT_OVERFLOW; return; }
  if (ctx.tid == 0) v.seq[v.off + v.m] = mode;
  ++v.m;
}
// after an erase at the back: what lane 0 stored becomes visible, the last event comes back into the registers
HSQP_HD void gait_reload_back(const Ctx& ctx, GaitView& v) {
  WG_SYNC(ctx);
  if (v.n > 0) v.back = v.ev[v.off + v.n - 1];
}

// GaitSchedule::tileModeSequenceTemplate (GaitSchedule.cpp:115-145); v.back is current
HSQP_HD void gait_tile(const Ctx& ctx, GaitView& v, const hsqp_gait_rung& tpl, double start, double final_time) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (v.status != HSQP_GAIT_OK) return;
  if (v.n > 0 && start <= v.back) { v.status = HSQP_GAIT_BAD_TILING; return; }   // "The initial time for template-tiling is not greater than the last event time."
  gait_push_event(ctx, v, start);                                                  // "add a initial time"
  while (v.back < final_time && v.status == HSQP_GAIT_OK)
    for (int i = 0; i < tpl.n_phases; ++i) {
      gait_push_mode(ctx, v, tpl.modes[i]);
      const double delta = tpl.switching_times[i + 1] - tpl.switching_times[i];
      gait_push_event(ctx, v, v.back + delta);
    }
  gait_push_mode(ctx, v, HSQP_MODE_STANCE);                                        // "default final phase"
}

// GaitSchedule::getModeSchedule (GaitSchedule.cpp:85-110) behind its front erase: the last default stance phase dropped, the template tiled from the last event
HSQP_HD void gait_retile(const Ctx& ctx, GaitView& v, const hsqp_gait_rung& tpl, double upper) {
  if (v.status != HSQP_GAIT_OK) return;
  if (v.n < 1) { v.status = HSQP_GAIT_BAD_TILING; return; }   // (the reference erases end() - 1 of an empty vector here)
  gait_reload_back(ctx, v);
  const double tiling_start = v.back;
  --v.n; --v.m;
  gait_reload_back(ctx, v);
  gait_tile(ctx, v, tpl, tiling_start, upper);
}

// the front erase of getModeSchedule on the view: "keep the one before the last to make it stance"
HSQP_HD void gait_trim_front(const Ctx& ctx, GaitView& v, double lower) {
  WG_SYNC(ctx);
  const int index = gait_bound(ctx, v.ev + v.off, v.n, lower, false);
  if (index > 0) {
    v.off += index - 1; v.n -= index - 1; v.m -= index - 1;
    if (ctx.tid == 0) v.seq[v.off] = HSQP_MODE_STANCE;
  }
}

// GaitSchedule::insertModeSequenceTemplate (GaitSchedule.cpp:53-80)
HSQP_HD void gait_insert(const Ctx& ctx, GaitView& v, const hsqp_gait_rung& tpl, double pts_setting, double start, double final_time) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (v.status != HSQP_GAIT_OK) return;
  WG_SYNC(ctx);
  const int index = gait_bound(ctx, v.ev + v.off, v.n, start, false);
  if (index < v.n) { v.n = index; v.m = index + 1; }
  gait_reload_back(ctx, v);
  double pts = pts_setting;
  if (v.m > 0 && v.seq[v.off + v.m - 1] == HSQP_MODE_STANCE) pts = 0.0;
  if (pts > 0.0) {
    gait_push_event(ctx, v, start);
    gait_push_mode(ctx, v, HSQP_MODE_STANCE);
  }
  gait_tile(ctx, v, tpl, start + pts, final_time);
}

// ProceduralMpcMotionManager::transitionToFasterGait / transitionToSlowerGait (ProceduralMpcMotionManager.cpp:86-113); cmd [4], base_vel [6]
HSQP_HD bool gait_faster(const double* cmd, const double* base_vel, const hsqp_gait_rung& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool requested = fabs(cmd[0]) > c.max_lin_vel_cmd || fabs(cmd[1]) > c.max_lin_vel_cmd || fabs(cmd[3]) > c.max_ang_vel_cmd;
  const bool within = fabs(base_vel[0]) > c.max_lin_vel_cmd - c.lin_vel_error_thresh || fabs(base_vel[1]) > c.max_lin_vel_cmd - c.lin_vel_error_thresh ||
                      fabs(base_vel[3]) > c.max_ang_vel_cmd - c.ang_vel_error_thresh;
  return requested && within;
}
HSQP_HD bool gait_slower(const double* cmd, const double* base_vel, const hsqp_gait_rung& c) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const bool requested = fabs(cmd[0]) < c.min_lin_vel_cmd && fabs(cmd[1]) < c.min_lin_vel_cmd && fabs(cmd[3]) < c.min_ang_vel_cmd;
  // the third clause tests the COMMAND's yaw rate, not the base's (ProceduralMpcMotionManager.cpp:110): kept
  const bool slow_enough = fabs(base_vel[0]) < c.min_lin_vel_cmd + c.lin_vel_error_thresh && fabs(base_vel[1]) < c.min_lin_vel_cmd + c.lin_vel_error_thresh &&
                           fabs(cmd[3]) < c.min_ang_vel_cmd + c.ang_vel_error_thresh;
  return requested && slow_enough;
}

// the view [off, off + n) to a row of E events / E + 1 modes in the hsqp_reference layout (behind n: the last event time, STANCE)
HSQP_HD void gait_store_row(const Ctx& ctx, const GaitView& v, int E, int* n_out, double* ev_out, int* seq_out) {
  WG_SYNC(ctx);
  const double last = v.n > 0 ? v.ev[v.off + v.n - 1] : 0.0;
  for (int i = ctx.tid; i < E; i += ctx.nthreads) ev_out[i] = i < v.n ? v.ev[v.off + i] : last;
  for (int i = ctx.tid; i <= E; i += ctx.nthreads) seq_out[i] = i < v.m ? v.seq[v.off + i] : HSQP_MODE_STANCE;
  if (ctx.tid == 0) *n_out = v.n;
  WG_SYNC(ctx);
}

// One update of instance b (include/hsqp_gait.h, steps 1 to 3).  in: the live state, out: the shadow state (written whatever the status);
// cmd: the filtered command [4] of the instance, x: its measured state [NX]; n_out / ev_out / seq_out: this cycle's schedule (the instance's rows).
// Returns the status word.
HSQP_HD int gait_update_instance(const Ctx& ctx, const hsqp_gait_settings& gs, GaitWork& w, const GaitState& in, const GaitState& out, int b, double t,
                                 double horizon, const double* cmd, const double* x, int* n_out, double* ev_out, int* seq_out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int E = gs.max_events;
  const double* ev_in = in.ev + (size_t)b * E;
  const int* seq_in = in.seq + (size_t)b * (E + 1);
  const int n0 = in.n[b];
  int rung = in.scal[b * GAIT_SCAL + 0], command = in.scal[b * GAIT_SCAL + 1], last_command = in.scal[b * GAIT_SCAL + 2], tpl = in.scal[b * GAIT_SCAL + 3];
  double t_change = in.t_change[b];
  if (n0 < 1 || n0 > E || rung < 0 || rung >= gs.n_rungs || command < 0 || command >= gs.n_rungs || tpl < 0 || tpl >= gs.n_rungs) return HSQP_GAIT_BAD_TILING;
  const double final_time = t + horizon;
  const double th = final_time - t;   // timeHorizon as the reference computes it (SwitchedModelReferenceManager.cpp:146, GaitScheduleUpdater.cpp:50)

  // 1. getModeSchedule(t - th, finalTime + th): the front erase happens on the way into the work row
  GaitView v{w.ev, w.seq, 0, 0, 0, E, HSQP_GAIT_OK, 0.0};
  {
    const int index = gait_bound(ctx, ev_in, n0, t - th, false);
    const int skip = index > 0 ? index - 1 : 0;
    v.n = n0 - skip; v.m = v.n + 1;
    for (int i = ctx.tid; i < v.n; i += ctx.nthreads) w.ev[i] = ev_in[skip + i];
    for (int i = ctx.tid; i < v.m; i += ctx.nthreads) w.seq[i] = i == 0 && index > 0 ? HSQP_MODE_STANCE : seq_in[skip + i];
  }
  gait_retile(ctx, v, gs.rungs[tpl], final_time + th);
  gait_store_row(ctx, v, E, n_out, ev_out, seq_out);

  // 2. the ladder (ProceduralMpcMotionManager.cpp:130-152); the function-local static currentCfg is the rung's row
  const double* base_vel = x + 6 + NJ;   // WBAccelMpcRobotModel::getBaseComVelocity
  if (t > t_change + gs.min_change_interval) {
    const hsqp_gait_rung& cfg = gs.rungs[rung];
    int step = 0;
    if (gait_faster(cmd, base_vel, cfg)) step = 1;
    else if (gait_slower(cmd, base_vel, cfg)) step = -1;
    if (step != 0) {
      rung += step;
      rung = rung < 0 ? 0 : rung > gs.n_rungs - 1 ? gs.n_rungs - 1 : rung;   // (not in the reference: its table cannot be left)
      command = rung;
      t_change = t;
    }
  }

  // 3. GaitScheduleUpdater::updateGaitSchedule(template of the command, t, finalTime)
  if (command != last_command) {
    const double earliest = 0.7 * final_time + 0.3 * t;
    gait_trim_front(ctx, v, t);
    gait_retile(ctx, v, gs.rungs[tpl], final_time + th);
    WG_SYNC(ctx);
    if (v.status == HSQP_GAIT_OK) {
      const int it = gait_bound(ctx, v.ev + v.off, v.n, earliest, true);
      double next = final_time;
      if (it < v.n) {
        const double e = v.ev[v.off + it];
        const int mode = v.seq[v.off + gait_bound(ctx, v.ev + v.off, v.n, e, false)];   // modeAtTime(*it)
        if (mode == HSQP_MODE_LF) {
          if (it == 0) v.status = HSQP_GAIT_BAD_TILING;   // (*(it - 1) of begin(): not reachable, the front mode of a trimmed schedule is STANCE)
          else next = v.ev[v.off + it - 1];
        } else next = e;
      }
      tpl = command;
      gait_insert(ctx, v, gs.rungs[tpl], gs.phase_transition_stance_time, next, 1.5 * th);   // (a duration where a time is expected: kept)
    }
    last_command = command;
  }

  gait_store_row(ctx, v, E, out.n + b, out.ev + (size_t)b * E, out.seq + (size_t)b * (E + 1));
  if (ctx.tid == 0) {
    out.scal[b * GAIT_SCAL + 0] = rung; out.scal[b * GAIT_SCAL + 1] = command; out.scal[b * GAIT_SCAL + 2] = last_command; out.scal[b * GAIT_SCAL + 3] = tpl;
    out.t_change[b] = t_change;
  }
  return v.status;
}

}  // namespace hsqp
