// TEST INFRASTRUCTURE: the receding-horizon loop of tests/adaptor/adaptor_driver.cpp (its WeightCompInitializer and reference manager are
// reused as they are) with sqp::Settings::useFeedbackPolicy chosen on the command line, for tests/test_gpu_feedback_policy.py.  The output has
// the lines of tests/adaptor_warm/adaptor_warm_driver.cpp; with the flag on, one more line per call:
//   <LinearController?> <max |array - hsqp_feedback_policy|> <max |computeInput(t_k, x_k) - u_k| / max(1, |u_k|) over the nodes that are
//   neither pre- nor post-event nor terminal> <entries>
//   adaptor_feedback_driver <model.json> <case.txt> <out.txt> <useFeedbackPolicy 0|1>
#include <vector>

#define main adaptor_driver_main
#include "adaptor_driver.cpp"
#undef main

int main(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: adaptor_feedback_driver model.json case.txt out.txt 0|1\n"); return 2; }
  HipSqpAdaptorConfig cfg;
  const std::string modelPath = argv[1];
  try {
    if (modelPath.size() > 5 && modelPath.substr(modelPath.size() - 5) == ".json") { cfg.model = hsqp_host::loadModelDesc(modelPath); cfg.swing = hsqp_host::loadSwingConfig(modelPath); }
    else { std::fprintf(stderr, "model.json expected\n"); return 2; }
  } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 2; }
  const bool feedback = std::atoi(argv[4]) != 0;
  std::ifstream in(argv[2]);
  int stateDim, nEvents, nKnots, calls, eventNodes, maxNodes;
  double dt, horizon, period, t0, sw[8];
  in >> stateDim >> dt >> horizon >> period >> t0 >> calls >> eventNodes >> maxNodes;
  for (double& v : sw) in >> v;
  auto rm = std::make_shared<FixedReferenceManager>();
  in >> nEvents;
  rm->ms.eventTimes.resize(nEvents); rm->ms.modeSequence.resize(nEvents + 1);
  for (auto& e : rm->ms.eventTimes) in >> e;
  for (auto& m : rm->ms.modeSequence) in >> m;
  in >> nKnots;
  rm->tt.timeTrajectory.resize(nKnots);
  for (auto& t : rm->tt.timeTrajectory) in >> t;
  for (int k = 0; k < nKnots; ++k) { vector_t s(stateDim); for (int i = 0; i < stateDim; ++i) in >> s[i]; rm->tt.stateTrajectory.push_back(s); rm->tt.inputTrajectory.push_back(vector_t::Zero(HSQP_NU)); }
  vector_t x(stateDim);
  for (int i = 0; i < stateDim; ++i) in >> x[i];
  if (!in) { std::fprintf(stderr, "malformed case file\n"); return 2; }
  cfg.stateDim = stateDim; cfg.maxNodes = maxNodes; cfg.eventNodes = eventNodes != 0;
  double mass = 0.0;
  for (const hsqp_body& b : cfg.model.bodies) mass += b.mass;   // DevModel::total_mass: the bodies in order
  mpc::Settings mpcSettings;
  mpcSettings.timeHorizon_ = horizon;
  sqp::Settings sqpSettings;
  sqpSettings.dt = dt; sqpSettings.sqpIteration = 1; sqpSettings.deltaTol = 1e-4; sqpSettings.g_max = 1e-2; sqpSettings.g_min = 1e-6;
  sqpSettings.useFeedbackPolicy = feedback;
  WeightCompInitializer initializer(&rm->ms, mass);
  try {
    HipSqpMpc mpc(mpcSettings, sqpSettings, cfg, initializer);
    mpc.getSolverPtr()->setReferenceManager(rm);
    std::FILE* out = std::fopen(argv[3], "w");
    double t = t0;
    for (int c = 0; c < calls; ++c) {
      mpc.run(t, x);
      const PrimalSolution sol = mpc.getSolverPtr()->primalSolution(t + horizon);
      const PerformanceIndex& p = mpc.getSolverPtr()->getPerformanceIndeces();
      const int n = (int)sol.timeTrajectory_.size();
      std::fprintf(out, "%d %.17g %.17g %d %.17g %.17g %.17g %zu\n", n, t, mpc.getSolverPtr()->lastStepSize(), mpc.getSolverPtr()->lastStepType(), p.cost,
                   p.dynamicsViolationSSE, p.equalityConstraintsSSE, sol.postEventIndices_.size());
      for (int k = 0; k < n; ++k) {
        std::fprintf(out, "%.17g", sol.timeTrajectory_[k]);
        for (int i = 0; i < stateDim; ++i) std::fprintf(out, " %.17g", sol.stateTrajectory_[k][i]);
        for (int i = 0; i < HSQP_NU; ++i) std::fprintf(out, " %.17g", sol.inputTrajectory_[k][i]);
        std::fprintf(out, "\n");
      }
      vector_t xs, us, tau;
      mpc.getSolverPtr()->evaluatePolicy(t + period, xs, us, tau);
      for (int j = 0; j < HSQP_NJ; ++j) std::fprintf(out, j ? " %.17g" : "%.17g", tau[j]);
      std::fprintf(out, "\n");
      if (feedback) {
        auto* lc = dynamic_cast<LinearController*>(sol.controllerPtr_.get());
        double arrDiff = -1.0, inDiff = -1.0;
        if (lc) {
          std::vector<double> K((size_t)n * HSQP_NU * HSQP_NX), uff((size_t)n * HSQP_NU);
          if (hsqp_feedback_policy(mpc.getSolverPtr()->handle(), 0, n, K.data(), uff.data()) != HSQP_OK) throw std::runtime_error("hsqp_feedback_policy failed");
          arrDiff = 0.0; inDiff = 0.0;
          for (int k = 0; k < n; ++k) {
            const matrix_t& G = lc->gainArray_[k];
            if ((int)G.rows() != HSQP_NU || (int)G.cols() != stateDim || lc->timeStamp_[k] != sol.timeTrajectory_[k]) arrDiff = 1e300;
            for (int i = 0; i < HSQP_NU; ++i) {
              arrDiff = std::max(arrDiff, std::fabs(lc->biasArray_[k][i] - uff[(size_t)k * HSQP_NU + i]));
              for (int j = 0; j < stateDim; ++j) arrDiff = std::max(arrDiff, std::fabs(G(i, j) - K[((size_t)k * HSQP_NU + i) * HSQP_NX + j]));
            }
            // (at an event stamp LinearInterpolation takes the pre-event entry, which carries the input of the node before it: the nodes
            // of an event and the terminal entry are left out)
            const bool preEvent = k + 1 < n && sol.timeTrajectory_[k + 1] == sol.timeTrajectory_[k];
            const bool postEvent = k > 0 && sol.timeTrajectory_[k - 1] == sol.timeTrajectory_[k];
            if (preEvent || postEvent || k == n - 1) continue;
            const vector_t u = lc->computeInput(sol.timeTrajectory_[k], sol.stateTrajectory_[k]);
            double scale = 1.0;
            for (int i = 0; i < HSQP_NU; ++i) scale = std::max(scale, std::fabs(sol.inputTrajectory_[k][i]));
            for (int i = 0; i < HSQP_NU; ++i) inDiff = std::max(inDiff, std::fabs(u[i] - sol.inputTrajectory_[k][i]) / scale);
          }
        }
        std::fprintf(out, "%d %.17g %.17g %d\n", lc ? 1 : 0, arrDiff, inDiff, lc ? (int)lc->timeStamp_.size() : 0);
      }
      x = xs;
      t += period;
    }
    std::fclose(out);
    std::printf("ok calls=%d useFeedbackPolicy=%d\n", calls, feedback ? 1 : 0);
    return 0;
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
}
