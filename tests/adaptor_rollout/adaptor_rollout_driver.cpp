// TEST INFRASTRUCTURE: the receding-horizon loop of tests/adaptor/adaptor_driver.cpp (its WeightCompInitializer and reference manager are
// reused as they are) closed through HipSqpSolverAdaptor::rolloutPolicy, with sqp::Settings::useFeedbackPolicy chosen on the command line, for
// tests/test_gpu_rollout.py.  Every call: the adaptor's rolloutPolicy over one period from the measured state, and hsqp_rollout_policy on the
// adaptor's handle with the same settings; the two must agree bit for bit.  The rolled-out state is the next call's measured state.
//   adaptor_rollout_driver <model.json> <case.txt> <out.txt> <useFeedbackPolicy 0|1>
// Prints "rollout ok calls=<n> useFeedbackPolicy=<0|1>" on success; out.txt: per call, t, then the rolled-out state and input.
#include <vector>

#define main adaptor_driver_main
#include "adaptor_driver.cpp"
#undef main

int main(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: adaptor_rollout_driver model.json case.txt out.txt 0|1\n"); return 2; }
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
      vector_t xs, us;
      mpc.getSolverPtr()->rolloutPolicy(t, x, period, xs, us);
      // the same through the C ABI on the adaptor's handle
      hsqp_rollout_settings st = cfg.rollout;
      st.controller = feedback ? HSQP_ROLLOUT_FEEDBACK : HSQP_ROLLOUT_FEEDFORWARD;
      std::vector<double> s0{t - sol.timeTrajectory_.front()}, x0(HSQP_NX, 0.0), xr(HSQP_NX), ur(HSQP_NU);
      for (int i = 0; i < stateDim; ++i) x0[i] = x[i];
      int32_t status = -1, steps = 0;
      const int rc = hsqp_rollout_policy(mpc.getSolverPtr()->handle(), &st, s0.data(), x0.data(), period, 1, xr.data(), ur.data(), &status, &steps, nullptr);
      if (rc != HSQP_OK || status != HSQP_ROLLOUT_OK) throw std::runtime_error("hsqp_rollout_policy failed");
      for (int i = 0; i < stateDim; ++i) if (xs[i] != xr[i]) { std::printf("state mismatch at call %d entry %d\n", c, i); return 4; }
      for (int i = 0; i < HSQP_NU; ++i) if (us[i] != ur[i]) { std::printf("input mismatch at call %d entry %d\n", c, i); return 4; }
      std::fprintf(out, "%.17g %d", t, steps);
      for (int i = 0; i < stateDim; ++i) std::fprintf(out, " %.17g", xs[i]);
      for (int i = 0; i < HSQP_NU; ++i) std::fprintf(out, " %.17g", us[i]);
      std::fprintf(out, "\n");
      x = xs;
      t += period;
    }
    std::fclose(out);
    std::printf("rollout ok calls=%d useFeedbackPolicy=%d\n", calls, feedback ? 1 : 0);
    return 0;
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
}
