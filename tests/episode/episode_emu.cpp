// TEST INFRASTRUCTURE: the host build of the failure isolation and episode reset sources (wb_humanoid_mpc_amd/csrc/hsqp_episode.h: k_loop_triage,
// k_episode_host_reset, k_episode_commands, k_gait_reset_instances) and of the warm start with a per-instance mode (csrc/hsqp_warm.h,
// WarmArgs::mode_b) with a one-lane loop, for tests/test_episode.py.  A shared library loaded through ctypes; every array is the caller's, in the
// device layout.  Built with -ffp-contract=off: the arithmetic the device evaluates unfused.
#include "hsqp_episode.h"
#include "hsqp_warm.h"

using namespace hsqp;

static const Ctx kLane{0, 1, nullptr};

extern "C" {

// one triage of B instances behind cycle `cycle`; cause_out [B]: the verdicts.  x_log / u_log may be null.
void ep_triage(const hsqp_episode_settings* st, int cycle, int B, const int* it_status, const hsqp_perf* perf, const int32_t* ro_status, const double* xs,
               const double* x_reset, const double* v_cmd, int* state, int* cause, int* fail_cycle, int* n_failures, int* n_episodes, int* mode, int* reset,
               double* x, double* v_filt, double* v_use, double* x_log, double* u_log, int* cause_out) {
  const TriageArgs a{*st, cycle, it_status, perf, ro_status, xs, x_reset, v_cmd, EpisodeState{state, cause, fail_cycle, n_failures, n_episodes, mode, reset},
                     x, v_filt, v_use, x_log, u_log};
  for (int b = 0; b < B; ++b) cause_out[b] = triage_instance(kLane, a, b);
}

void ep_host_reset(int n, const int* ids, const double* x0, const double* v_new, const double* x_reset, int* state, int* cause, int* fail_cycle, int* n_failures,
                   int* n_episodes, int* mode, int* reset, double* x, double* v_cmd, double* v_filt, double* v_use) {
  const HostResetArgs a{ids, x0, v_new, x_reset, EpisodeState{state, cause, fail_cycle, n_failures, n_episodes, mode, reset}, x, v_cmd, v_filt, v_use};
  for (int i = 0; i < n; ++i) host_reset_instance(kLane, a, i);
}

void ep_commands(int B, const int* state, const double* v_cmd, const double* x_reset, double* v_use) {
  for (int b = 0; b < B; ++b) episode_command_in_use(kLane, state[b], v_cmd + (size_t)b * CMD_N, x_reset + (size_t)b * NX, v_use + (size_t)b * CMD_N);
}

// ids == null: every instance whose flag is set (count = B); otherwise the instances ids[0 .. count)
void ep_gait_reset(int E, int count, const int* ids, const int* flags, double t, int* n, double* ev, int* seq, int* scal, double* t_change) {
  const GaitState s{n, ev, seq, scal, t_change};
  for (int i = 0; i < count; ++i) {
    const int b = ids ? ids[i] : i;
    if (!ids && !flags[b]) continue;
    gait_reset_instance(kLane, s, E, b, t);
  }
}

// the warm start of a uniform grid with the batch-wide mode `mode` or, mode_b != null, a mode per instance; flags [B][N + 1][2]: the contact flags
void ep_warm(int mode, const int* mode_b, int B, int N, int N_prev, int cent, double t0, double dt, double total_mass, const double* flags, const double* x_init,
             const double* x_prev, const double* u_prev, const double* stamps_prev, double* par_scratch, double* dts_scratch, double* x, double* u, double* stamps) {
  for (size_t r = 0; r < (size_t)B * (N + 1); ++r) {
    for (int i = 0; i < NP; ++i) par_scratch[r * NP + i] = 0.0;
    par_scratch[r * NP + HSQP_P_CONTACT] = flags[2 * r]; par_scratch[r * NP + HSQP_P_CONTACT + 1] = flags[2 * r + 1];
  }
  for (size_t i = 0; i < (size_t)B * N; ++i) dts_scratch[i] = dt;
  WarmArgs w{};
  w.mode = mode; w.mode_b = mode_b; w.B = B; w.N = N; w.N_prev = N_prev; w.cent = cent;
  w.t0 = t0; w.dt = dt; w.total_mass = total_mass;
  w.node_times = nullptr; w.dts = dts_scratch; w.par = par_scratch; w.x_init = x_init;
  w.x_prev = x_prev; w.u_prev = u_prev; w.stamps_prev = stamps_prev;
  w.x = x; w.u = u; w.stamps = stamps;
  for (int b = 0; b < B; ++b)
    for (int k = 0; k <= N; ++k) warm_node(kLane, w, stamps_prev + (size_t)b * (N_prev + 1), b, k);
}

int ep_node_params(void) { return NP; }

}  // extern "C"
