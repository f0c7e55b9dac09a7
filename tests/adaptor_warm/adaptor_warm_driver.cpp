// TEST INFRASTRUCTURE: the receding-horizon loop of tests/adaptor/adaptor_driver.cpp (its WeightCompInitializer and reference manager are
// reused as they are) with HipSqpAdaptorConfig::deviceWarmStart chosen on the command line, for tests/test_gpu_warm_start.py: the same
// MPC_BASE::run calls with the warm start built on the host (0) and on the device (1) write the same output.
//   adaptor_warm_driver <model.json|model.bin> <case.txt> <out.txt> <deviceWarmStart 0|1>
#define main adaptor_driver_main
#include "adaptor_driver.cpp"
#undef main

int main(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: adaptor_warm_driver model case.txt out.txt 0|1\n"); return 2; }
  HipSqpAdaptorConfig cfg;
  const std::string modelPath = argv[1];
  try {
    if (modelPath.size() > 5 && modelPath.substr(modelPath.size() - 5) == ".json") { cfg.model = hsqp_host::loadModelDesc(modelPath); cfg.swing = hsqp_host::loadSwingConfig(modelPath); }
    else { std::fprintf(stderr, "model.json expected\n"); return 2; }
  } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 2; }
  cfg.deviceWarmStart = std::atoi(argv[4]) != 0;
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
  sqpSettings.dt = dt; sqpSettings.sqpIteration = 1; sqpSettings.deltaTol = 1e-4; sqpSettings.g_max = 1e-2; sqpSettings.g_min = 1e-6; sqpSettings.useFeedbackPolicy = false;
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
      x = xs;
      for (int j = 0; j < HSQP_NJ; ++j) std::fprintf(out, j ? " %.17g" : "%.17g", tau[j]);
      std::fprintf(out, "\n");
      t += period;
    }
    std::fclose(out);
    std::printf("ok calls=%d deviceWarmStart=%d\n", calls, cfg.deviceWarmStart ? 1 : 0);
    return 0;
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
}
