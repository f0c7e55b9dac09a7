// TEST INFRASTRUCTURE: the receding-horizon loop of tests/adaptor/adaptor_driver.cpp (its WeightCompInitializer and reference manager are
// reused as they are) with HipSqpAdaptorConfig::createValueFunction chosen on the command line, for tests/test_gpu_value.py.  The output has
// the lines of tests/adaptor_warm/adaptor_warm_driver.cpp; then one more line per call:
//   flag on:   <f> <max |getValueFunction.dfdx - hsqp_evaluate_value_function.dfdx|> <max |valueFunctionAt - the C ABI| over dV, dfdx, dfdxx>
//              <dV> <max |dfdx|> <max |dfdxx - dfdxx^T|> <getHamiltonian threw 0|1> <getStateInputEqualityConstraintLagrangian threw 0|1>
//   flag off:  threw: <the message of getValueFunction's exception>
// The query is the policy's sample time t + period at the policy's state there, moved by 0.01 in every live entry.
//   adaptor_value_driver <model.json> <case.txt> <out.txt> <createValueFunction 0|1>
#include <vector>

#define main adaptor_driver_main
#include "adaptor_driver.cpp"
#undef main

int main(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: adaptor_value_driver model.json case.txt out.txt 0|1\n"); return 2; }
  HipSqpAdaptorConfig cfg;
  const std::string modelPath = argv[1];
  try {
    if (modelPath.size() > 5 && modelPath.substr(modelPath.size() - 5) == ".json") { cfg.model = hsqp_host::loadModelDesc(modelPath); cfg.swing = hsqp_host::loadSwingConfig(modelPath); }
    else { std::fprintf(stderr, "model.json expected\n"); return 2; }
  } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 2; }
  const bool keep = std::atoi(argv[4]) != 0;
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
  cfg.createValueFunction = keep;
  double mass = 0.0;
  for (const hsqp_body& b : cfg.model.bodies) mass += b.mass;   // DevModel::total_mass: the bodies in order
  mpc::Settings mpcSettings;
  mpcSettings.timeHorizon_ = horizon;
  sqp::Settings sqpSettings;
  sqpSettings.dt = dt; sqpSettings.sqpIteration = 1; sqpSettings.deltaTol = 1e-4; sqpSettings.g_max = 1e-2; sqpSettings.g_min = 1e-6;
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
      vector_t xq = xs;
      for (int i = 0; i < stateDim; ++i) xq[i] += 0.01;
      try {
        const ScalarFunctionQuadraticApproximation q = mpc.getSolverPtr()->getValueFunction(t + period, xq);
        std::vector<double> dV, g, H;
        mpc.getSolverPtr()->valueFunctionAt(t + period, xq, dV, g, H);
        // the C ABI directly, on the handle
        std::vector<double> xr(HSQP_NX, 0.0), rV(1), rg(HSQP_NX), rH((size_t)HSQP_NX * HSQP_NX);
        std::copy_n(xq.data(), stateDim, xr.data());
        const double s = (t + period) - sol.timeTrajectory_.front();
        if (hsqp_evaluate_value_function(mpc.getSolverPtr()->handle(), 1, &s, xr.data(), rV.data(), rg.data(), rH.data()) != HSQP_OK)
          throw std::runtime_error("hsqp_evaluate_value_function failed");
        double dq = (int)q.dfdx.size() == stateDim ? 0.0 : 1e300, da = std::fabs(dV[0] - rV[0]), gmax = 0.0, asym = 0.0;
        for (int i = 0; i < stateDim; ++i) { dq = std::max(dq, std::fabs(q.dfdx[i] - rg[i])); gmax = std::max(gmax, std::fabs(rg[i])); }
        for (int i = 0; i < HSQP_NX; ++i) {
          da = std::max(da, std::fabs(g[i] - rg[i]));
          for (int j = 0; j < HSQP_NX; ++j) {
            da = std::max(da, std::fabs(H[(size_t)i * HSQP_NX + j] - rH[(size_t)i * HSQP_NX + j]));
            asym = std::max(asym, std::fabs(rH[(size_t)i * HSQP_NX + j] - rH[(size_t)j * HSQP_NX + i]));
          }
        }
        int hamThrew = 0, lagThrew = 0;
        try { mpc.getSolverPtr()->getHamiltonian(t, xq, us); } catch (const std::runtime_error&) { hamThrew = 1; }
        try { mpc.getSolverPtr()->getStateInputEqualityConstraintLagrangian(t, xq); } catch (const std::runtime_error&) { lagThrew = 1; }
        std::fprintf(out, "%.17g %.17g %.17g %.17g %.17g %.17g %d %d\n", q.f, dq, da, rV[0], gmax, asym, hamThrew, lagThrew);
      } catch (const std::runtime_error& e) {
        if (keep) throw;
        std::fprintf(out, "threw: %s\n", e.what());
      }
      x = xs;
      t += period;
    }
    std::fclose(out);
    std::printf("ok calls=%d createValueFunction=%d\n", calls, keep ? 1 : 0);
    return 0;
  } catch (const std::runtime_error& e) {
    std::printf("runtime_error: %s\n", e.what());
    return 3;
  }
}
