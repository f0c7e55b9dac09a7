// C++ host side of the drop-in boundary: a thin RAII class over the C ABI (include/hsqp.h) with the method names
// and meanings of the surface the reference consumes from its solver —
//   ocs2::SolverBase::reset / run / getPrimalSolution / getPerformanceIndeces   (lib/ocs2_ros2, missing submodule;
//     used through humanoid_nmpc/humanoid_wb_mpc_ros2/src/WBMpcSqpNode.cpp:64-89 and
//     humanoid_nmpc/humanoid_wb_mpc/src/mrt/WBMpcMrtJointController.cpp:200-213)
//   SqpSolver::getBenchmarks() {linearQuadraticApproximationTime, solveQpTime, linesearchTime, computeControllerTime}
//     (humanoid_nmpc/humanoid_common_mpc_ros2/src/benchmarks/SqpBenchmarksPublisher.cpp:44-57)
// for a batch of independent MPC instances.  It has no dependency on ocs2; the ocs2 adaptor that derives from
// ocs2::SolverBase and owns one of these is shown in INTEGRATION.md.  Failures map to std::runtime_error, which is
// what the reference's MPC thread expects from its solver (WBMpcMrtJointController.cpp:210-213).
#pragma once
#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/hsqp.h"
#include "../../include/hsqp_feedback.h"
#include "../../include/hsqp_value.h"
#include "../../include/hsqp_rollout.h"
#include "../../include/hsqp_loop.h"
#include "../../include/hsqp_cent_loop.h"
#include "../../include/hsqp_gait.h"
#include "../../include/hsqp_episode.h"
#include "../../include/hsqp_metrics.h"
#include "../../include/hsqp_grid.h"
#include "../../include/hsqp_ground.h"
#include "../../include/hsqp_perceive.h"
#include "../../include/hsqp_push.h"
#include "../../include/hsqp_plant.h"
#include "../../include/hsqp_contact.h"
#include "../../include/hsqp_actuator.h"
#include "../../include/hsqp_inertia.h"
#include "../../include/hsqp_terrain.h"
#include "../../include/hsqp_observe.h"

namespace hsqp_host {

struct Benchmarks {
  double linearQuadraticApproximationTime = 0.0, solveQpTime = 0.0, linesearchTime = 0.0, computeControllerTime = 0.0;
};

struct PrimalSolution {
  int batch = 0, nodes = 0;
  std::vector<double> stateTrajectory;   // [batch][nodes + 1][HSQP_NX]
  std::vector<double> inputTrajectory;   // [batch][nodes][HSQP_NU]
};

class HipSqpSolver {
 public:
  /** useLinesearch: run() applies the filter line search (ocs2 SqpSolver::takeStep) instead of the full step.
   *  recedingHorizon: the handle solves the SHIFTED problem of one MPC loop every cycle (MPC_BASE::run, sqpIteration = 1), so the KKT gate's back-off
   *  carries over the uploads (hsqp_set_scan_backoff_persistent).  Off by default: a batch / offline user uploads unrelated problems, and for those
   *  include/hsqp.h documents per-problem determinism (the same problem takes the same sweep whatever the handle solved before). */
  HipSqpSolver(const hsqp_model_desc& model, int maxNodes, int maxBatch = 1, int device = 0, bool useLinesearch = false, bool recedingHorizon = false) {
    hsqp_settings st{maxNodes, maxBatch, device, useLinesearch ? HSQP_FLAG_LINESEARCH : 0};
    int rc = hsqp_create(&model, &st, &h_);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_create failed (" + std::to_string(rc) + "): " + hsqp_last_error(nullptr));
    if (recedingHorizon && (rc = hsqp_set_scan_backoff_persistent(h_, 1)) != HSQP_OK) {
      const std::string msg = hsqp_last_error(h_);
      hsqp_destroy(h_);
      throw std::runtime_error("[HipSqpSolver] hsqp_set_scan_backoff_persistent failed (" + std::to_string(rc) + "): " + msg);
    }
  }
  ~HipSqpSolver() { hsqp_destroy(h_); }
  HipSqpSolver(const HipSqpSolver&) = delete;
  HipSqpSolver& operator=(const HipSqpSolver&) = delete;

  /** SolverBase::reset: forget the previous solution (the next run is a cold start supplied by the caller; runRecedingHorizon: built on the device). */
  void reset() { solution_ = PrimalSolution(); perf_.clear(); shiftable_ = false; }

  /**
   * SolverBase::run for `batch` instances on a uniform grid of `nodes` intervals: one SQP iteration
   * (task.info: sqpIteration 1) from the linearisation trajectory (xTraj, uTraj); xInit is the measured state.
   */
  void run(int batch, int nodes, double dt, const double* xInit, const double* xTraj, const double* uTraj, const double* nodeParams) {
    hsqp_problem p{batch, nodes, dt, xInit, xTraj, uTraj, nodeParams};
    solution_.batch = batch; solution_.nodes = nodes;
    solution_.stateTrajectory.assign((size_t)batch * (nodes + 1) * HSQP_NX, 0.0);
    solution_.inputTrajectory.assign((size_t)batch * nodes * HSQP_NU, 0.0);
    perf_.assign(batch, hsqp_perf{});
    perfBefore_.assign(batch, hsqp_perf{});
    kkt_.assign((size_t)batch * 2, 0.0);
    stepSize_.assign(batch, 0.0);
    stepType_.assign(batch, HSQP_STEP_FULL);
    hsqp_solution s{};
    s.alpha = stepSize_.data(); s.step_type = stepType_.data();
    s.x = solution_.stateTrajectory.data(); s.u = solution_.inputTrajectory.data();
    s.perf_before = perfBefore_.data(); s.perf_after = perf_.data(); s.kkt = reportKkt_ ? kkt_.data() : nullptr;
    shiftable_ = false;   // (hsqp_solve forgets the grid's stamps)
    const int rc = hsqp_solve(h_, &p, &s);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_solve failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    bench_.linearQuadraticApproximationTime = s.timings.lq_approximation;
    bench_.solveQpTime = s.timings.solve_qp;
    bench_.linesearchTime = s.timings.linesearch;
    bench_.computeControllerTime = s.timings.compute_controller;
  }

  /**
   * Same as run(), but the per-node parameter table is generated on the device from the compact reference — the adaptor hands
   * over the ocs2::ModeSchedule (event times, mode sequence) and the TargetTrajectories knots instead of sampling the reference
   * manager and the swing planner for every node (hsqp_upload_reference).
   */
  void runWithReference(int nodes, double dt, const double* xInit, const double* xTraj, const double* uTraj, const hsqp_reference& ref,
                        bool takeStepWithLinesearch = false, const double* dtNodes = nullptr /* non-uniform grid with event nodes: [batch][nodes] interval
                        lengths (0 = event), together with ref.node_times */,
                        int maxIterations = 1 /* sqp::Settings::sqpIteration: all of them in ONE device call, ended early by ocs2's step-size test */) {
    hsqp_reference r = ref;
    r.warm_start = HSQP_WARM_CALLER;
    uploadAndIterate(nodes, dt, xInit, xTraj, uTraj, r, takeStepWithLinesearch, dtNodes, maxIterations);
    download();
  }

  /**
   * One cycle of a receding-horizon loop (MPC_BASE::run) with the warm start built on the device (hsqp_reference::warm_start): the solution
   * of the previous cycle, resident in the handle, interpolated onto the new grid, the uncovered tail from the WeightCompInitializer — the
   * host warm start of HipSqpSolverAdaptor::runImpl without the trajectories crossing PCIe.  A cold start (x_k = xInit, weight-compensating
   * inputs) on the first call and after reset() or run(); `ref.warm_start` is ignored.  withDownload = false leaves the solution on the
   * device: getPrimalSolution() then holds no trajectories, evaluatePolicy() still works.
   */
  void runRecedingHorizon(int nodes, double dt, const double* xInit, const hsqp_reference& ref, bool takeStepWithLinesearch = false,
                          const double* dtNodes = nullptr, int maxIterations = 1, bool withDownload = true) {
    hsqp_reference r = ref;
    r.warm_start = shiftable_ ? HSQP_WARM_SHIFT : HSQP_WARM_COLD;
    uploadAndIterate(nodes, dt, xInit, nullptr, nullptr, r, takeStepWithLinesearch, dtNodes, maxIterations);
    if (withDownload) { download(); return; }
    solution_.stateTrajectory.clear(); solution_.inputTrajectory.clear();
    double ms[5];   // the benchmark buckets as hsqp_download reports them
    if (hsqp_last_kernel_ms(h_, ms) == HSQP_OK) bench_ = Benchmarks{1e-3 * (ms[0] + ms[1]), 1e-3 * ms[2], 1e-3 * ms[3], 0.0};
  }

  /** MPC_MRT_Interface::evaluatePolicy + computeJointTorques for the solution of the last run: per instance, at `secondsAfterStart`. */
  void evaluatePolicy(const std::vector<double>& secondsAfterStart, std::vector<double>& state, std::vector<double>& input, std::vector<double>& jointTorques) {
    const size_t B = (size_t)solution_.batch;
    if (secondsAfterStart.size() != B) throw std::runtime_error("[HipSqpSolver] evaluatePolicy: one time per instance expected");
    state.assign(B * HSQP_NX, 0.0); input.assign(B * HSQP_NU, 0.0); jointTorques.assign(B * HSQP_NJ, 0.0);
    const int rc = hsqp_evaluate_policy(h_, secondsAfterStart.data(), state.data(), input.data(), jointTorques.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_evaluate_policy failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }

  /** Riccati feedback policy of the last run (ocs2 LinearController, u = uff + K x; include/hsqp_feedback.h): entries [first, first + count)
   *  of every instance, K [batch][count][HSQP_NU][HSQP_NX] and uff [batch][count][HSQP_NU], row-major; count < 0: up to node N. */
  void feedbackPolicy(int first, int count, std::vector<double>& K, std::vector<double>& uff) {
    const size_t B = (size_t)solution_.batch;
    if (count < 0) count = solution_.nodes + 1 - first;
    K.assign(B * (count > 0 ? count : 0) * HSQP_NU * HSQP_NX, 0.0); uff.assign(B * (count > 0 ? count : 0) * HSQP_NU, 0.0);
    const int rc = hsqp_feedback_policy(h_, first, count, K.data(), uff.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_feedback_policy failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** MPC_MRT_Interface::evaluatePolicy with the feedback policy: the input at the measured states (one HSQP_NX row per instance). */
  void evaluatePolicy(const std::vector<double>& secondsAfterStart, const std::vector<double>& measuredState, std::vector<double>& state,
                      std::vector<double>& input, std::vector<double>& jointTorques) {
    const size_t B = (size_t)solution_.batch;
    if (secondsAfterStart.size() != B || measuredState.size() != B * HSQP_NX)
      throw std::runtime_error("[HipSqpSolver] evaluatePolicy: one time and one measured state per instance expected");
    state.assign(B * HSQP_NX, 0.0); input.assign(B * HSQP_NU, 0.0); jointTorques.assign(B * HSQP_NJ, 0.0);
    const int rc = hsqp_evaluate_feedback_policy(h_, secondsAfterStart.data(), measuredState.data(), state.data(), input.data(), jointTorques.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_evaluate_feedback_policy failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }

  /** sqp::Settings::createValueFunction: the runWithReference / runRecedingHorizon calls that follow keep the Riccati value function of their last
   *  iteration (HSQP_ITER_VALUE_FUNCTION, include/hsqp_value.h) for valueFunction / evaluateValueFunction; off by default — the record costs device
   *  memory, not time.  run() goes through hsqp_solve, which knows no such flag: it ignores this setting and clears a record kept earlier. */
  void setKeepValueFunction(bool on) { keepValue_ = on; }
  /** The record of nodes k0 .. k1 (k1 < 0: node N) of every instance: S [batch][n][HSQP_NX][HSQP_NX] (symmetric), s and xbar [batch][n][HSQP_NX], row-major;
   *  the cost-to-go is s' dx + 1/2 dx' S dx in dx = x - xbar, xbar the trajectory the last QP was linearised at. */
  void valueFunction(int k0, int k1, std::vector<double>& S, std::vector<double>& s, std::vector<double>& xbar) {
    const size_t B = (size_t)solution_.batch;
    if (k1 < 0) k1 = solution_.nodes;
    const size_t n = k1 >= k0 ? (size_t)(k1 - k0 + 1) : 0;
    S.assign(B * n * HSQP_NX * HSQP_NX, 0.0); s.assign(B * n * HSQP_NX, 0.0); xbar.assign(B * n * HSQP_NX, 0.0);
    const int rc = hsqp_value_function(h_, k0, k1, S.data(), s.data(), xbar.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_value_function failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** SolverBase::getValueFunction for nQueries (time, state) pairs per instance: secondsAfterStart [batch][nQueries], state [batch][nQueries][HSQP_NX];
   *  dV [batch][nQueries], dfdx [batch][nQueries][HSQP_NX], dfdxx [batch][nQueries][HSQP_NX][HSQP_NX] (withHessian = false leaves it empty). */
  void evaluateValueFunction(int nQueries, const std::vector<double>& secondsAfterStart, const std::vector<double>& state, std::vector<double>& dV,
                             std::vector<double>& dfdx, std::vector<double>& dfdxx, bool withHessian = true) {
    const size_t B = (size_t)solution_.batch, n = nQueries > 0 ? (size_t)nQueries : 0;
    if (nQueries < 1 || secondsAfterStart.size() != B * n || state.size() != B * n * HSQP_NX)
      throw std::runtime_error("[HipSqpSolver] evaluateValueFunction: nQueries >= 1 and one time and one state per instance and query expected");
    dV.assign(B * n, 0.0); dfdx.assign(B * n * HSQP_NX, 0.0); dfdxx.assign(withHessian ? B * n * HSQP_NX * HSQP_NX : 0, 0.0);
    const int rc = hsqp_evaluate_value_function(h_, nQueries, secondsAfterStart.data(), state.data(), dV.data(), dfdx.data(), withHessian ? dfdxx.data() : nullptr);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_evaluate_value_function failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }

  /** MRT_BASE::rolloutPolicy for every instance of the last run (include/hsqp_rollout.h): instance b from x0[b] (one HSQP_NX row per
   *  instance) at secondsAfterStart[b], under the resident policy with the integrator / controller of `st`; x [batch][nSamples][HSQP_NX],
   *  u [batch][nSamples][HSQP_NU] at the nSamples times secondsAfterStart[b] + duration (j + 1) / nSamples, status [batch].  A failed
   *  instance (step cap, non-finite value) throws like every other failure; the outputs are complete for the others. */
  void rolloutPolicy(const hsqp_rollout_settings& st, const std::vector<double>& secondsAfterStart, const std::vector<double>& x0, double duration, int nSamples,
                     std::vector<double>& x, std::vector<double>& u, std::vector<int32_t>& status) {
    const size_t B = (size_t)solution_.batch;
    if (secondsAfterStart.size() != B || x0.size() != B * HSQP_NX || nSamples < 1)
      throw std::runtime_error("[HipSqpSolver] rolloutPolicy: one time and one start state per instance, and nSamples >= 1 expected");
    x.assign(B * nSamples * HSQP_NX, 0.0); u.assign(B * nSamples * HSQP_NU, 0.0); status.assign(B, 0);
    const int rc = hsqp_rollout_policy(h_, &st, secondsAfterStart.data(), x0.data(), duration, nSamples, x.data(), u.data(), status.data(), nullptr, nullptr);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_rollout_policy failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }

  /** ---- external pushes on the plant (include/hsqp_push.h): pushes[b] are the pushes of instance b (at most HSQP_PUSH_MAX each).  The table stays
   *  resident until clearPushes() or the next setPushes(); every rolloutPolicy and every loop cycle of a batch of pushes.size() instances applies
   *  it (another batch throws).  The MPC never sees a push. */
  void setPushes(const std::vector<std::vector<hsqp_push>>& pushes) {
    size_t mp = 1;
    for (const auto& p : pushes) mp = p.size() > mp ? p.size() : mp;
    std::vector<int32_t> n(pushes.size());
    std::vector<hsqp_push> table(pushes.size() * mp, hsqp_push{});
    for (size_t b = 0; b < pushes.size(); ++b) {
      n[b] = (int32_t)pushes[b].size();
      for (size_t i = 0; i < pushes[b].size(); ++i) table[b * mp + i] = pushes[b][i];
    }
    const int rc = hsqp_push_set(h_, (int)pushes.size(), (int)mp, n.data(), table.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_push_set failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  void clearPushes() {
    const int rc = hsqp_push_clear(h_);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_push_clear failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** The resident table, as setPushes takes it (throws if none is set). */
  std::vector<std::vector<hsqp_push>> pushes() {
    int B = 0, mp = 0;
    int rc = hsqp_push_get(h_, &B, &mp, nullptr, nullptr);
    std::vector<int32_t> n((size_t)(rc == HSQP_OK ? B : 0));
    std::vector<hsqp_push> table(n.size() * (size_t)mp);
    if (rc == HSQP_OK) rc = hsqp_push_get(h_, nullptr, nullptr, n.data(), table.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_push_get failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    std::vector<std::vector<hsqp_push>> out(n.size());
    for (size_t b = 0; b < n.size(); ++b) out[b].assign(table.begin() + b * mp, table.begin() + b * mp + n[b]);
    return out;
  }

  /** ---- the plant of the rollout and the resident loop (include/hsqp_plant.h).  setPlant with kind HSQP_PLANT_TORQUE (hsqp_plant_defaults: the
   *  reference's lookahead and gains, no armature) makes every rolloutPolicy and every loop cycle integrate full forward dynamics under the
   *  joint PD law; clearPlant goes back to the MPC's own flow map.  The setting stays resident; the MPC never sees it. */
  void setPlant(const hsqp_plant_settings& settings) {
    const int rc = hsqp_plant_set(h_, &settings);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_plant_set failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  void clearPlant() {
    const int rc = hsqp_plant_clear(h_);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_plant_clear failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  hsqp_plant_settings plant() {
    hsqp_plant_settings s;
    const int rc = hsqp_plant_get(h_, &s);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_plant_get failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return s;
  }

  /** ---- the ground under the torque plant (include/hsqp_contact.h): compliant contact with Coulomb friction at the eight sole corners, inside every
   *  flow evaluation of rolloutPolicy and of the loop's cycles while the plant kind is HSQP_PLANT_TORQUE (stored and inert otherwise).
   *  contactDefaults: hsqp_contact_defaults (mu: the model's friction_mu).  setContactInstances: (height, mu) per instance, an empty vector: back to
   *  the setting's values.  contactForces: the model at the given states [B][58] — force [B][2][4][3] in world axes, penetration [B][2][4].  The MPC
   *  never sees any of it. */
  hsqp_contact_settings contactDefaults() const {
    hsqp_contact_settings s;
    hsqp_contact_defaults(h_, &s);
    return s;
  }
  void setContact(const hsqp_contact_settings& settings) {
    const int rc = hsqp_contact_set(h_, &settings);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_contact_set failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  void setContactInstances(const std::vector<hsqp_contact_ground>& ground) {
    const int rc = hsqp_contact_set_instances(h_, (int)ground.size(), ground.empty() ? nullptr : ground.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_contact_set_instances failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  void clearContact() {
    const int rc = hsqp_contact_clear(h_);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_contact_clear failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  hsqp_contact_settings contact() {
    hsqp_contact_settings s;
    const int rc = hsqp_contact_get(h_, &s);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_contact_get failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return s;
  }
  void contactForces(const std::vector<double>& x, std::vector<double>& force, std::vector<double>& penetration) {
    if (x.empty() || x.size() % HSQP_NX != 0) throw std::runtime_error("[HipSqpSolver] contactForces: states of HSQP_NX values each expected");
    const size_t B = x.size() / HSQP_NX, pts = HSQP_CONTACT_FEET * HSQP_CONTACT_CORNERS;
    force.assign(B * pts * 3, 0.0); penetration.assign(B * pts, 0.0);
    const int rc = hsqp_contact_eval(h_, (int)B, x.data(), force.data(), penetration.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_contact_eval failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }

  /** ---- height-map terrain under that ground (include/hsqp_terrain.h): up to HSQP_TERRAIN_MAX_MAPS maps shared by all instances, and a placement (map,
   *  origin, yaw; map = -1: the plane) per instance.  It acts on the torque plant with contact on while maps and a placement table are resident; the
   *  instance's contact ground height is an offset under its map.  setTerrainMaps: map m is heights[m] = nx[m] * ny[m] doubles, row-major H[iy][ix]; no
   *  maps: frees them.  setTerrainInstances: an empty vector: no table.  terrainHeight: the ground of each instance at world points xy [B][n][2] —
   *  height [B][n], normal [B][n][3].  The MPC never sees it. */
  void setTerrainMaps(const std::vector<int32_t>& nx, const std::vector<int32_t>& ny, const std::vector<double>& cell, const std::vector<std::vector<double>>& heights) {
    if (ny.size() != nx.size() || cell.size() != nx.size() || heights.size() != nx.size()) throw std::runtime_error("[HipSqpSolver] setTerrainMaps: one nx, ny, cell and height array per map expected");
    std::vector<double> pool;
    for (size_t m = 0; m < nx.size(); ++m) {
      if (nx[m] < 0 || ny[m] < 0 || heights[m].size() != (size_t)nx[m] * (size_t)ny[m]) throw std::runtime_error("[HipSqpSolver] setTerrainMaps: map " + std::to_string(m) + " needs nx * ny heights");
      pool.insert(pool.end(), heights[m].begin(), heights[m].end());
    }
    const int rc = hsqp_terrain_set_maps(h_, (int)nx.size(), nx.data(), ny.data(), cell.data(), pool.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_terrain_set_maps failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  void setTerrainInstances(const std::vector<hsqp_terrain_placement>& place) {
    const int rc = hsqp_terrain_set_instances(h_, (int)place.size(), place.empty() ? nullptr : place.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_terrain_set_instances failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  void clearTerrain() {
    const int rc = hsqp_terrain_clear(h_);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_terrain_clear failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  std::vector<hsqp_terrain_placement> terrainInstances(int batch) {
    if (batch < 1) throw std::runtime_error("[HipSqpSolver] terrainInstances: batch < 1");
    std::vector<hsqp_terrain_placement> place((size_t)batch);
    const int rc = hsqp_terrain_get_instances(h_, batch, place.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_terrain_get_instances failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return place;
  }
  void terrainHeight(int batch, const std::vector<double>& xy, std::vector<double>& height, std::vector<double>& normal) {
    if (batch < 1 || xy.empty() || xy.size() % (2 * (size_t)batch) != 0) throw std::runtime_error("[HipSqpSolver] terrainHeight: the same number of (x, y) points per instance expected");
    const size_t pts = xy.size() / 2;
    height.assign(pts, 0.0); normal.assign(pts * 3, 0.0);
    const int rc = hsqp_terrain_eval(h_, batch, (int)(pts / (size_t)batch), xy.data(), height.data(), normal.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_terrain_eval failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }

  /** ---- the actuator model on the torque plant (include/hsqp_actuator.h): the joint command sampled at a control rate and held, effort limits,
   *  joint damping and dry friction, inside every flow evaluation of rolloutPolicy and of the loop's cycles while the plant is HSQP_PLANT_TORQUE.
   *  actuatorDefaults: hsqp_actuator_defaults.  actuatorTorques: tau_cmd, tau_act, tau_passive [batch][23] each at the final state of the most
   *  recent rollout (or loop cycle) on the model; NaN rows for an instance that did not end OK.  The MPC never sees any of it. */
  static hsqp_actuator_settings actuatorDefaults() {
    hsqp_actuator_settings s;
    hsqp_actuator_defaults(&s);
    return s;
  }
  void setActuator(const hsqp_actuator_settings& settings) {
    const int rc = hsqp_actuator_set(h_, &settings);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_actuator_set failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  void clearActuator() {
    const int rc = hsqp_actuator_clear(h_);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_actuator_clear failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  hsqp_actuator_settings actuator() {
    hsqp_actuator_settings s;
    const int rc = hsqp_actuator_get(h_, &s);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_actuator_get failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return s;
  }
  void actuatorTorques(int batch, std::vector<double>& tauCmd, std::vector<double>& tauAct, std::vector<double>& tauPassive) {
    if (batch < 1) throw std::runtime_error("[HipSqpSolver] actuatorTorques: batch < 1");
    tauCmd.resize((size_t)batch * HSQP_NJ);
    tauAct.resize((size_t)batch * HSQP_NJ);
    tauPassive.resize((size_t)batch * HSQP_NJ);
    const int rc = hsqp_actuator_last(h_, batch, tauCmd.data(), tauAct.data(), tauPassive.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_actuator_last failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }

  /** ---- per-instance inertial variations of the torque PLANT (include/hsqp_inertia.h): link mass scales and up to HSQP_INERTIA_PAYLOADS rigid payloads per
   *  instance, inside every flow evaluation of rolloutPolicy and of the loop's cycles while the plant is HSQP_PLANT_TORQUE (stored and inert otherwise).
   *  inertiaDefaults: the neutral entry.  setInertiaInstances: one entry per instance, an empty vector: no table.  inertiaInstances: the entries in
   *  force (past the table: neutral).  plantDynamics: at the states [B][58] with instance b's entry — M [B][29][29] without armature, nle [B][29],
   *  mass [B].  The MPC, jointTorques and tau_ff keep the nominal model: that is the mismatch being modelled. */
  static hsqp_inertia_instance inertiaDefaults() {
    hsqp_inertia_instance v;
    hsqp_inertia_defaults(&v);
    return v;
  }
  void setInertiaInstances(const std::vector<hsqp_inertia_instance>& table) {
    const int rc = hsqp_inertia_set_instances(h_, (int)table.size(), table.empty() ? nullptr : table.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_inertia_set_instances failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  void clearInertia() {
    const int rc = hsqp_inertia_clear(h_);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_inertia_clear failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  std::vector<hsqp_inertia_instance> inertiaInstances(int batch) {
    if (batch < 1) throw std::runtime_error("[HipSqpSolver] inertiaInstances: batch < 1");
    std::vector<hsqp_inertia_instance> table((size_t)batch);
    const int rc = hsqp_inertia_get_instances(h_, batch, table.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_inertia_get_instances failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return table;
  }
  void plantDynamics(const std::vector<double>& x, std::vector<double>& M, std::vector<double>& nle, std::vector<double>& mass) {
    if (x.empty() || x.size() % HSQP_NX != 0) throw std::runtime_error("[HipSqpSolver] plantDynamics: states of HSQP_NX values each expected");
    const size_t B = x.size() / HSQP_NX;
    M.assign(B * HSQP_NV * HSQP_NV, 0.0); nle.assign(B * HSQP_NV, 0.0); mass.assign(B, 0.0);
    const int rc = hsqp_inertia_eval(h_, (int)B, x.data(), M.data(), nle.data(), mass.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_inertia_eval failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }

  /** ---- the observation model of the resident loop (include/hsqp_observe.h): what the MPC measures of the plant — a per-instance bias and white noise
   *  on the state row, a sensor delay the controller does not know about and a compute delay it does (the problem is posed compute_delay periods back
   *  and the plant enters the policy at that offset).  setObservation: the delays (whole MPC periods) and the seed.  setObservationInstances: one entry
   *  per instance, an empty vector: no table.  observation: the settings and the entries in force (past the table: neutral).  observe: bias and noise of
   *  instance b's entry on x [B][58] at a draw index, no delay.  lastObservation: what the last completed cycle of the loop used, [B][58], and its
   *  problem time.  The plant, the rollout and the iteration are untouched. */
  void setObservation(int sensor_delay = 0, int compute_delay = 0, uint64_t seed = 0) {
    hsqp_observe_settings st;
    hsqp_observe_defaults(&st);
    st.sensor_delay = sensor_delay; st.compute_delay = compute_delay; st.seed = seed;
    const int rc = hsqp_observe_set(h_, &st);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_observe_set failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  void setObservationInstances(const std::vector<hsqp_observe_instance>& table) {
    const int rc = hsqp_observe_set_instances(h_, (int)table.size(), table.empty() ? nullptr : table.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_observe_set_instances failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  void clearObservation() {
    const int rc = hsqp_observe_clear(h_);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_observe_clear failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  hsqp_observe_settings observation(int batch, std::vector<hsqp_observe_instance>& table) {
    if (batch < 1) throw std::runtime_error("[HipSqpSolver] observation: batch < 1");
    hsqp_observe_settings st;
    table.resize((size_t)batch);
    const int rc = hsqp_observe_get(h_, &st, batch, table.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_observe_get failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return st;
  }
  std::vector<double> observe(const std::vector<double>& x, uint32_t draw) {
    const size_t B = x.size() / HSQP_NX;
    if (B < 1 || x.size() != B * HSQP_NX) throw std::runtime_error("[HipSqpSolver] observe: x must hold [B][58] states");
    std::vector<double> y(x.size());
    const int rc = hsqp_observe_eval(h_, (int)B, draw, x.data(), y.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_observe_eval failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return y;
  }
  /** y: [batch][58], batch the loop's; returns the problem time */
  double lastObservation(int batch, std::vector<double>& y) {
    if (batch < 1) throw std::runtime_error("[HipSqpSolver] lastObservation: batch < 1");
    y.assign((size_t)batch * HSQP_NX, 0.0);
    double tp = 0.0;
    const int rc = hsqp_observe_last(h_, y.data(), &tp);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_observe_last failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return tp;
  }

  /** ---- the closed loop resident on the device (include/hsqp_loop.h): what ProceduralMpcMotionManager::preSolverRun's target generation, MPC_BASE::run
   *  and the dummy simulation's rolloutPolicy do per cycle, for `batch` instances with their own velocity commands.
   *  setDefaultJointState: reference.info defaultJointState (HSQP_NJ values), once, before the first startLoop. */
  void setDefaultJointState(const std::vector<double>& q) {
    if (q.size() != HSQP_NJ) throw std::runtime_error("[HipSqpSolver] setDefaultJointState: HSQP_NJ values expected");
    const int rc = hsqp_set_default_joint_state(h_, q.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_set_default_joint_state failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** hsqp_loop_defaults for this handle. */
  hsqp_loop_settings loopDefaults() const { hsqp_loop_settings st; hsqp_loop_defaults(h_, &st); return st; }
  /** x0 [batch][HSQP_NX], velocityCommands [batch][4] (vx, vy, height, yaw rate), the instances' mode schedules as hsqp_reference takes them
   *  (nEvents [batch], eventTimes [batch][maxEvents], modeSequence [batch][maxEvents + 1]); uploaded once. */
  void startLoop(const hsqp_loop_settings& st, double t0, const std::vector<double>& x0, const std::vector<double>& velocityCommands, int maxEvents,
                 const std::vector<int32_t>& nEvents, const std::vector<double>& eventTimes, const std::vector<int32_t>& modeSequence) {
    const size_t B = nEvents.size();
    loopBatch_ = 0;
    if (B == 0 || maxEvents < 1 || x0.size() != B * HSQP_NX || velocityCommands.size() != B * HSQP_CMD_N || eventTimes.size() != B * (size_t)maxEvents ||
        modeSequence.size() != B * (size_t)(maxEvents + 1))
      throw std::runtime_error("[HipSqpSolver] startLoop: inconsistent array sizes");
    const int rc = hsqp_loop_start(h_, &st, (int)B, t0, x0.data(), velocityCommands.data(), maxEvents, nEvents.data(), eventTimes.data(), modeSequence.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_start failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    loopBatch_ = B;
    loopNodes_ = (size_t)st.n_nodes; gridNodes_ = 0;
    shiftable_ = false;   // (the loop owns the resident problem until the next run* call ends it)
  }
  /** startLoop with the per-instance gait schedule and ladder resident on the device (include/hsqp_gait.h) in place of uploaded schedules: every
   *  instance starts in stance at rung 0 and climbs / descends the ladder of `gait` from its filtered command and measured base velocity.  The
   *  caller fills `gait` (hsqp_gait_ladder_defaults for thresholds and names, the templates of gait.info under the rungs). */
  void startLoopGait(const hsqp_loop_settings& st, const hsqp_gait_settings& gait, double t0, const std::vector<double>& x0, const std::vector<double>& velocityCommands) {
    const size_t B = velocityCommands.size() / HSQP_CMD_N;
    loopBatch_ = 0;
    if (B == 0 || x0.size() != B * HSQP_NX || velocityCommands.size() != B * HSQP_CMD_N) throw std::runtime_error("[HipSqpSolver] startLoopGait: inconsistent array sizes");
    const int rc = hsqp_loop_start_gait(h_, &st, &gait, (int)B, t0, x0.data(), velocityCommands.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_start_gait failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    loopBatch_ = B;
    loopNodes_ = (size_t)st.n_nodes; gridNodes_ = 0;
    shiftable_ = false;
  }
  /** ---- the centroidal forms (include/hsqp_cent_loop.h): what CentroidalMpcSqpNode does per cycle through
   *  CentroidalMpcTargetTrajectoriesCalculator::commandedVelocityToTargetTrajectories.  x0 [batch][HSQP_NX]: centroidal rows, entries 35..57 zero.
   *  centroidalCommandTargets: filteredCommands [batch][4] in / out, targetTimes [batch][3], targetStates [batch][3][HSQP_NX]; baseVelocity (optional)
   *  [batch][6], the base velocity from the centroidal momentum. */
  void centroidalCommandTargets(const std::vector<double>& velocityCommands, std::vector<double>& filteredCommands, double filterAlpha, const std::vector<double>& x0,
                                double t0, double horizon, std::vector<double>& targetTimes, std::vector<double>& targetStates, std::vector<double>* baseVelocity = nullptr) {
    const size_t B = velocityCommands.size() / HSQP_CMD_N;
    if (B == 0 || velocityCommands.size() != B * HSQP_CMD_N || filteredCommands.size() != B * HSQP_CMD_N || x0.size() != B * HSQP_NX)
      throw std::runtime_error("[HipSqpSolver] centroidalCommandTargets: inconsistent array sizes");
    targetTimes.assign(B * HSQP_CMD_KNOTS, 0.0); targetStates.assign(B * HSQP_CMD_KNOTS * HSQP_NX, 0.0);
    if (baseVelocity) baseVelocity->assign(B * 6, 0.0);
    const int rc = hsqp_centroidal_command_targets(h_, (int)B, velocityCommands.data(), filteredCommands.data(), filterAlpha, x0.data(), t0, horizon, targetTimes.data(),
                                                   targetStates.data(), baseVelocity ? baseVelocity->data() : nullptr);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_centroidal_command_targets failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** startLoop on a centroidal handle; runLoop, setLoopCommand, loopState, isolateLoop, resetLoopInstances and loopEpisodes work after either start.
   *  loopDefaults() gives the whole-body task file's dt and period: set them from the centroidal task. */
  void startLoopCentroidal(const hsqp_loop_settings& st, double t0, const std::vector<double>& x0, const std::vector<double>& velocityCommands, int maxEvents,
                           const std::vector<int32_t>& nEvents, const std::vector<double>& eventTimes, const std::vector<int32_t>& modeSequence) {
    const size_t B = nEvents.size();
    loopBatch_ = 0;
    if (B == 0 || maxEvents < 1 || x0.size() != B * HSQP_NX || velocityCommands.size() != B * HSQP_CMD_N || eventTimes.size() != B * (size_t)maxEvents ||
        modeSequence.size() != B * (size_t)(maxEvents + 1))
      throw std::runtime_error("[HipSqpSolver] startLoopCentroidal: inconsistent array sizes");
    const int rc = hsqp_loop_start_centroidal(h_, &st, (int)B, t0, x0.data(), velocityCommands.data(), maxEvents, nEvents.data(), eventTimes.data(), modeSequence.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_start_centroidal failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    loopBatch_ = B;
    loopNodes_ = (size_t)st.n_nodes; gridNodes_ = 0;
    shiftable_ = false;
  }
  /** New commands [batch][4]; in effect from the next cycle. */
  void setLoopCommand(const std::vector<double>& velocityCommands) {
    if (velocityCommands.size() != loopBatch_ * HSQP_CMD_N) throw std::runtime_error("[HipSqpSolver] setLoopCommand: four values per instance of the started loop expected");
    const int rc = hsqp_loop_command(h_, velocityCommands.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_command failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** nCycles cycles; xLog [done][batch][HSQP_NX], uLog [done][batch][HSQP_NU]: state and input at the end of every completed cycle.  A cycle that
   *  fails throws after the logs of the completed ones are in place; returns the cycles done. */
  int runLoop(int nCycles, std::vector<double>& xLog, std::vector<double>& uLog) {
    const size_t n = nCycles > 0 ? (size_t)nCycles : 0;
    xLog.assign(n * loopBatch_ * HSQP_NX, 0.0); uLog.assign(n * loopBatch_ * HSQP_NU, 0.0);
    int done = 0;
    const int rc = hsqp_loop_run(h_, nCycles, xLog.data(), uLog.data(), &done);
    xLog.resize((size_t)done * loopBatch_ * HSQP_NX); uLog.resize((size_t)done * loopBatch_ * HSQP_NU);
    if (rc != HSQP_OK)
      throw std::runtime_error("[HipSqpSolver] hsqp_loop_run failed after " + std::to_string(done) + " cycles (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return done;
  }
  /** Where the loop stands: its time, the measured states [batch][HSQP_NX] and the command filters' states [batch][4]. */
  void loopState(double& t, std::vector<double>& x, std::vector<double>& filteredCommands) {
    x.assign(loopBatch_ * HSQP_NX, 0.0); filteredCommands.assign(loopBatch_ * HSQP_CMD_N, 0.0);
    const int rc = hsqp_loop_state(h_, &t, x.data(), filteredCommands.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_state failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** ---- per-instance failure isolation and episode reset of the started loop (include/hsqp_episode.h): a failed instance is parked or reset on
   *  the device, the others go on; runLoop then throws only for what is not per instance.  xReset [batch][HSQP_NX], or empty: the measured
   *  states the loop holds now. */
  void isolateLoop(const hsqp_episode_settings& st, const std::vector<double>& xReset = {}) {
    if (!xReset.empty() && xReset.size() != loopBatch_ * HSQP_NX) throw std::runtime_error("[HipSqpSolver] isolateLoop: one state per instance of the started loop expected");
    const int rc = hsqp_loop_isolate(h_, &st, xReset.empty() ? nullptr : xReset.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_isolate failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** A new episode for the instances `ids` from the next cycle on: x0 [ids.size()][HSQP_NX] or empty (their xReset), velocityCommands
   *  [ids.size()][4] or empty (keep). */
  void resetLoopInstances(const std::vector<int32_t>& ids, const std::vector<double>& x0 = {}, const std::vector<double>& velocityCommands = {}) {
    if ((!x0.empty() && x0.size() != ids.size() * HSQP_NX) || (!velocityCommands.empty() && velocityCommands.size() != ids.size() * HSQP_CMD_N))
      throw std::runtime_error("[HipSqpSolver] resetLoopInstances: inconsistent array sizes");
    const int rc = hsqp_loop_reset_instances(h_, (int)ids.size(), ids.data(), x0.empty() ? nullptr : x0.data(), velocityCommands.empty() ? nullptr : velocityCommands.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_reset_instances failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** The episode record of every instance: HSQP_EP_* state and cause of the last failure, its cycle (-1: none), failures and episodes so far. */
  struct LoopEpisodes { std::vector<int32_t> state, cause, failCycle, nFailures, nEpisodes; };
  LoopEpisodes loopEpisodes() {
    LoopEpisodes e;
    for (std::vector<int32_t>* v : {&e.state, &e.cause, &e.failCycle, &e.nFailures, &e.nEpisodes}) v->assign(loopBatch_, 0);
    const int rc = hsqp_loop_episodes(h_, e.state.data(), e.cause.data(), e.failCycle.data(), e.nFailures.data(), e.nEpisodes.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_episodes failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return e;
  }

  /** Episode metrics of the started loop (include/hsqp_metrics.h): one record per instance accumulated on the device behind every cycle's rollout,
   *  cut at episode boundaries.  Off after every start of a loop. */
  void enableLoopMetrics() {
    const int rc = hsqp_loop_metrics_enable(h_);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_metrics_enable failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** Accumulation stops; the records stay readable until the next start. */
  void disableLoopMetrics() {
    const int rc = hsqp_loop_metrics_disable(h_);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_metrics_disable failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** The records of the instances `ids` (empty: all) are closed with HSQP_METRICS_END_HOST and reopened; their episodes are untouched. */
  void restartLoopMetrics(const std::vector<int32_t>& ids = {}) {
    const int rc = hsqp_loop_metrics_restart(h_, (int)ids.size(), ids.empty() ? nullptr : ids.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_metrics_restart failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** The record of every instance: HSQP_METRICS_CURRENT (the open one) or HSQP_METRICS_PREVIOUS (the last closed one; empty: none). */
  std::vector<hsqp_metrics> loopMetrics(int which = HSQP_METRICS_CURRENT) {
    std::vector<hsqp_metrics> out(loopBatch_);
    const int rc = hsqp_loop_metrics(h_, which, out.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_metrics failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return out;
  }

  /** The padded ocs2 event-node grid of a batch (include/hsqp_grid.h), built on the device: interval lengths [batch][N], sampling times [batch][N + 1]
   *  (what hsqp_problem::dt_nodes and hsqp_reference::node_times take) and the intervals of every instance's own grid, N = nNodes + settings.event_nodes. */
  struct EventGrid { std::vector<int32_t> nIntervals; std::vector<double> dtNodes, nodeTimes; };
  hsqp_grid_settings gridDefaults() const { hsqp_grid_settings st; hsqp_grid_defaults(&st); return st; }
  EventGrid eventGrid(const hsqp_grid_settings& settings, double t0, int nNodes, double dt, int maxEvents, const std::vector<int32_t>& nEvents,
                      const std::vector<double>& eventTimes) {
    const size_t B = nEvents.size(), N = (size_t)std::max(nNodes + settings.event_nodes, 0);
    if (B == 0 || maxEvents < 1 || eventTimes.size() != B * (size_t)maxEvents) throw std::runtime_error("[HipSqpSolver] eventGrid: inconsistent array sizes");
    EventGrid g;
    g.nIntervals.assign(B, 0); g.dtNodes.assign(B * N, 0.0); g.nodeTimes.assign(B * (N + 1), 0.0);
    const int rc = hsqp_event_grid(h_, &settings, (int)B, t0, nNodes, dt, maxEvents, nEvents.data(), eventTimes.data(), g.nIntervals.data(), g.dtNodes.data(),
                                   g.nodeTimes.data(), nullptr);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_event_grid failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return g;
  }
  /** The started loop on the event-node grid from its next cycle on (settings == nullptr: back to the uniform grid).  Off after every start. */
  void setLoopEventGrid(const hsqp_grid_settings* settings) {
    const int rc = hsqp_loop_event_grid(h_, settings);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_event_grid failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    if (settings) gridNodes_ = loopNodes_ + (size_t)settings->event_nodes;
  }
  /** The grid of the loop's last completed cycle, which ran on the event grid. */
  EventGrid loopGrid() {
    const size_t B = loopBatch_, N = gridNodes_;
    if (B == 0 || N == 0) throw std::runtime_error("[HipSqpSolver] loopGrid: no loop on the event grid (startLoop, setLoopEventGrid)");
    EventGrid g;
    g.nIntervals.assign(B, 0); g.dtNodes.assign(B * N, 0.0); g.nodeTimes.assign(B * (N + 1), 0.0);
    const int rc = hsqp_loop_grid(h_, g.nIntervals.data(), g.dtNodes.data(), g.nodeTimes.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_grid failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return g;
  }

  /** The ground height under every instance estimated from its stance feet (include/hsqp_ground.h): the new latches [batch] from the measured states
   *  [batch][58], the mode schedules at time t and the latches g; footHeights (optional): the heights of both contact frames [batch][2]. */
  hsqp_ground_settings groundDefaults() const { hsqp_ground_settings st; hsqp_ground_defaults(&st); return st; }
  std::vector<double> groundEstimate(double t, const std::vector<double>& x, int maxEvents, const std::vector<int32_t>& nEvents, const std::vector<double>& eventTimes,
                                     const std::vector<int32_t>& modeSequence, std::vector<double> g, double filterAlpha = 0.0, std::vector<double>* footHeights = nullptr) {
    const size_t B = nEvents.size();
    if (B == 0 || maxEvents < 1 || x.size() != B * HSQP_NX || eventTimes.size() != B * (size_t)maxEvents || modeSequence.size() != B * (size_t)(maxEvents + 1) || g.size() != B)
      throw std::runtime_error("[HipSqpSolver] groundEstimate: inconsistent array sizes");
    if (footHeights) footHeights->assign(2 * B, 0.0);
    const int rc = hsqp_ground_estimate(h_, (int)B, t, x.data(), maxEvents, nEvents.data(), eventTimes.data(), modeSequence.data(), filterAlpha, g.data(),
                                        footHeights ? footHeights->data() : nullptr);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_ground_estimate failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return g;
  }
  /** hsqp_upload_reference with one terrain height per instance (terrainHeights [batch]) in place of reference.terrain_height. */
  void uploadReferenceGround(const hsqp_problem& problem, const hsqp_reference& reference, const std::vector<double>& terrainHeights) {
    if (problem.batch < 1 || terrainHeights.size() != (size_t)problem.batch) throw std::runtime_error("[HipSqpSolver] uploadReferenceGround: inconsistent array sizes");
    const int rc = hsqp_upload_reference_ground(h_, &problem, &reference, terrainHeights.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_upload_reference_ground failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    loopBatch_ = 0;   // (every upload ends a loop)
    shiftable_ = false;
  }
  /** The started loop follows the ground under its stance feet from its next cycle on: the command's height entry means height above the estimated
   *  ground, step 2 takes the estimate as the instance's terrain height (settings == nullptr or enabled 0: off).  gInit [batch] or empty
   *  (settings->initial_height): the latches' start values.  Off after every start. */
  void setLoopGround(const hsqp_ground_settings* settings, const std::vector<double>& gInit = {}) {
    if (!gInit.empty() && gInit.size() != loopBatch_) throw std::runtime_error("[HipSqpSolver] setLoopGround: gInit must hold one value per instance of the loop");
    const int rc = hsqp_loop_ground(h_, settings, gInit.empty() ? nullptr : gInit.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_ground failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** The latches [batch] and the contact-frame heights [batch][2] of the loop's last completed cycle. */
  struct LoopGround { std::vector<double> g, footHeights; };
  LoopGround loopGround() {
    if (loopBatch_ == 0) throw std::runtime_error("[HipSqpSolver] loopGround: no loop started (startLoop, setLoopGround)");
    LoopGround out;
    out.g.assign(loopBatch_, 0.0); out.footHeights.assign(2 * loopBatch_, 0.0);
    const int rc = hsqp_loop_ground_state(h_, out.g.data(), out.footHeights.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_ground_state failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return out;
  }

  /** Per-foot swing heights read from the resident height map (include/hsqp_perceive.h): for every instance and foot the lift-off and touch-down height
   *  of every phase of its schedule, [batch][2][maxEvents + 1] each, and the footholds they were read at, [batch][2][maxEvents + 1][2], from the states
   *  [batch][58] at time t, the mode schedules and the target knots ([batch][nKnots], [batch][nKnots][58]).  Needs maps and a placement table. */
  struct FootHeights { std::vector<double> liftOff, touchDown, footholdXY; };
  FootHeights footHeights(double t, const std::vector<double>& x, int maxEvents, const std::vector<int32_t>& nEvents, const std::vector<double>& eventTimes,
                          const std::vector<int32_t>& modeSequence, int nKnots, const std::vector<double>& targetTimes, const std::vector<double>& targetStates,
                          double touchDownHeightOffset) {
    const size_t B = nEvents.size();
    if (B == 0 || maxEvents < 1 || nKnots < 1 || x.size() != B * HSQP_NX || eventTimes.size() != B * (size_t)maxEvents || modeSequence.size() != B * (size_t)(maxEvents + 1) ||
        targetTimes.size() != B * (size_t)nKnots || targetStates.size() != B * (size_t)nKnots * HSQP_NX)
      throw std::runtime_error("[HipSqpSolver] footHeights: inconsistent array sizes");
    FootHeights out;
    const size_t rows = B * 2 * (size_t)(maxEvents + 1);
    out.liftOff.assign(rows, 0.0); out.touchDown.assign(rows, 0.0); out.footholdXY.assign(2 * rows, 0.0);
    const int rc = hsqp_foot_heights(h_, (int)B, t, x.data(), maxEvents, nEvents.data(), eventTimes.data(), modeSequence.data(), nKnots, targetTimes.data(),
                                     targetStates.data(), touchDownHeightOffset, out.liftOff.data(), out.touchDown.data(), out.footholdXY.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_foot_heights failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return out;
  }
  /** hsqp_upload_reference with the swing planner's three-argument update: liftOff, touchDown [batch][2][max_events + 1] in place of
   *  reference.terrain_height (touchDown holds the touch-down height offset). */
  void uploadReferenceHeights(const hsqp_problem& problem, const hsqp_reference& reference, const std::vector<double>& liftOff, const std::vector<double>& touchDown) {
    const size_t rows = problem.batch < 1 || reference.max_events < 1 ? 0 : (size_t)problem.batch * 2 * (size_t)(reference.max_events + 1);
    if (rows == 0 || liftOff.size() != rows || touchDown.size() != rows) throw std::runtime_error("[HipSqpSolver] uploadReferenceHeights: inconsistent array sizes");
    const int rc = hsqp_upload_reference_heights(h_, &problem, &reference, liftOff.data(), touchDown.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_upload_reference_heights failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    loopBatch_ = 0;   // (every upload ends a loop)
    shiftable_ = false;
  }
  /** The started loop reads every instance's per-foot lift-off and touch-down heights from the height map from its next cycle on (settings == nullptr or
   *  enabled 0: off).  Off after every start. */
  void setLoopPerception(const hsqp_perceive_settings* settings) {
    const int rc = hsqp_loop_perceive(h_, settings);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_perceive failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
  }
  /** The rows of the loop's last completed cycle; maxEvents: that of the loop's schedule. */
  FootHeights loopFootHeights(int maxEvents) {
    if (loopBatch_ == 0) throw std::runtime_error("[HipSqpSolver] loopFootHeights: no loop started (startLoop, setLoopPerception)");
    if (maxEvents < 1) throw std::runtime_error("[HipSqpSolver] loopFootHeights: maxEvents < 1");
    FootHeights out;
    const size_t rows = loopBatch_ * 2 * (size_t)(maxEvents + 1);
    out.liftOff.assign(rows, 0.0); out.touchDown.assign(rows, 0.0); out.footholdXY.assign(2 * rows, 0.0);
    const int rc = hsqp_loop_foot_heights(h_, out.liftOff.data(), out.touchDown.data(), out.footholdXY.data());
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_loop_foot_heights failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    return out;
  }

  const PrimalSolution& getPrimalSolution() const { return solution_; }
  const std::vector<hsqp_perf>& getPerformanceIndeces() const { return perf_; }
  const std::vector<hsqp_perf>& getPerformanceIndecesBeforeStep() const { return perfBefore_; }
  /** KKT residuals {stationarity, primal} of the projected QP per instance — a DIAGNOSTIC that costs a kernel and, at 256 instances, 4.5 GB
   *  of reads per call: evaluated only after setReportKkt(true) (zeros otherwise); getBenchmarks() does not depend on it. */
  const std::vector<double>& getKktResiduals() const { return kkt_; }
  void setReportKkt(bool on) { reportKkt_ = on; }
  /** Step length and FilterLinesearch::StepType (HSQP_STEP_*) per instance of the last run. */
  const std::vector<double>& getStepSizes() const { return stepSize_; }
  const std::vector<int32_t>& getStepTypes() const { return stepType_; }
  void setLinesearchSettings(const hsqp_linesearch_settings& ls) {
    if (hsqp_set_linesearch(h_, &ls) != HSQP_OK) throw std::runtime_error(std::string("[HipSqpSolver] ") + hsqp_last_error(h_));
  }
  Benchmarks getBenchmarks() const { return bench_; }
  /** SQP iterations the last runWithReference ran, and what iteration `it` of them ended with (instance 0 .. batch-1). */
  int getNumIterations() const { return iterations_; }
  void getIterationLog(int it, std::vector<hsqp_perf>& perf, std::vector<double>& alpha, std::vector<int32_t>& stepType) const {
    perf.assign(solution_.batch, hsqp_perf{}); alpha.assign(solution_.batch, 0.0); stepType.assign(solution_.batch, HSQP_STEP_ZERO);
    if (hsqp_iteration_log(h_, it, perf.data(), alpha.data(), stepType.data()) != HSQP_OK) throw std::runtime_error("[HipSqpSolver] no such iteration in the log");
  }
  /** Live weight update (the centroidal node's gains receiver): diagonal Q / R / Qf, nullptr keeps the current one. */
  void updateWeights(const double* Q, const double* R, const double* Qf) {
    if (hsqp_update_weights(h_, Q, R, Qf) != HSQP_OK) throw std::runtime_error(std::string("[HipSqpSolver] ") + hsqp_last_error(h_));
  }
  hsqp_handle* handle() { return h_; }

 private:
  void uploadAndIterate(int nodes, double dt, const double* xInit, const double* xTraj, const double* uTraj, const hsqp_reference& ref,
                        bool takeStepWithLinesearch, const double* dtNodes, int maxIterations) {
    const int batch = ref.batch;
    hsqp_problem p{batch, nodes, dt, xInit, xTraj, uTraj, nullptr, dtNodes};
    shiftable_ = false;
    int rc = hsqp_upload_reference(h_, &p, &ref);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_upload_reference failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    rc = hsqp_iterate_device(h_, maxIterations < 1 ? 1 : maxIterations,
                             HSQP_ITER_TAKE_STEP | (reportKkt_ ? HSQP_ITER_KKT : 0) | (takeStepWithLinesearch ? HSQP_ITER_LINESEARCH : 0) | HSQP_ITER_UNTIL_CONVERGED |
                                 (keepValue_ ? HSQP_ITER_VALUE_FUNCTION : 0));
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_iterate_device failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    shiftable_ = true;
    iterations_ = hsqp_last_iterations(h_);
    solution_.batch = batch; solution_.nodes = nodes;
  }

  void download() {
    const int batch = solution_.batch, nodes = solution_.nodes;
    solution_.stateTrajectory.assign((size_t)batch * (nodes + 1) * HSQP_NX, 0.0);
    solution_.inputTrajectory.assign((size_t)batch * nodes * HSQP_NU, 0.0);
    perf_.assign(batch, hsqp_perf{}); perfBefore_.assign(batch, hsqp_perf{});
    kkt_.assign((size_t)batch * 2, 0.0); stepSize_.assign(batch, 0.0); stepType_.assign(batch, HSQP_STEP_FULL);
    hsqp_solution s{};
    s.x = solution_.stateTrajectory.data(); s.u = solution_.inputTrajectory.data();
    s.perf_before = perfBefore_.data(); s.perf_after = perf_.data(); s.kkt = reportKkt_ ? kkt_.data() : nullptr;
    s.alpha = stepSize_.data(); s.step_type = stepType_.data();
    const int rc = hsqp_download(h_, &s);
    if (rc != HSQP_OK) throw std::runtime_error("[HipSqpSolver] hsqp_download failed (" + std::to_string(rc) + "): " + hsqp_last_error(h_));
    bench_.linearQuadraticApproximationTime = s.timings.lq_approximation;
    bench_.solveQpTime = s.timings.solve_qp;
    bench_.linesearchTime = s.timings.linesearch;
    bench_.computeControllerTime = s.timings.compute_controller;
  }

  hsqp_handle* h_ = nullptr;
  PrimalSolution solution_;
  std::vector<hsqp_perf> perf_, perfBefore_;
  std::vector<double> kkt_, stepSize_;
  std::vector<int32_t> stepType_;
  Benchmarks bench_;
  int iterations_ = 0;
  bool reportKkt_ = false;
  bool keepValue_ = false;   // setKeepValueFunction
  size_t loopBatch_ = 0;     // instances of the started loop (startLoop)
  size_t loopNodes_ = 0;     // its n_nodes
  size_t gridNodes_ = 0;     // n_nodes + event_nodes of its last setLoopEventGrid (0: none since the start)
  bool shiftable_ = false;   // the handle holds the solution of a runWithReference / runRecedingHorizon: the next runRecedingHorizon shifts it
};

}  // namespace hsqp_host
