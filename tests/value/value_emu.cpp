// TEST INFRASTRUCTURE: the host build of the value-function kernels' source (wb_humanoid_mpc_amd/csrc/hsqp_value.h: k_value_record, k_value_eval) with a
// one-lane context, for tests/test_value.py, tests/test_gpu_value.py and tests/value/value_sanitize.cpp.  The arrays are the caller's, in the device layout:
//   val_record(B, N, k0, k1, cent, vf [B][N + 1][VF_SIZE], xbar [B][N + 1][58], S [B][n][58][58], s [B][n][58], xb [B][n][58])          n = k1 - k0 + 1
//   val_eval(B, N, dt, dts [B][N] or null, cent, n, vf, xbar, s_query [B][n], x_query [B][n][58], dV [B][n], dfdx [B][n][58], dfdxx [B][n][58][58])
//   val_vf_size()   VF_SIZE
// Any output may be null.  Built with -ffp-contract=off: the arithmetic the device evaluates unfused.
#include <cstddef>

#include "hsqp_value.h"

using namespace hsqp;

extern "C" int val_vf_size() { return VF_SIZE; }

extern "C" void val_record(int B, int N, int k0, int k1, int cent, const double* vf, const double* xbar, double* S, double* s, double* xb) {
  ValueWS* w = new ValueWS;
  const Ctx ctx{0, 1, nullptr};
  const size_t count = (size_t)(k1 - k0 + 1);
  for (int b = 0; b < B; ++b)
    for (size_t j = 0; j < count; ++j) {
      const size_t node = (size_t)b * (N + 1) + k0 + j, e = (size_t)b * count + j;
      value_record_node(ctx, vf + node * VF_SIZE, xbar + node * NX, cent, S ? S + e * NX * NX : nullptr, s ? s + e * NX : nullptr, xb ? xb + e * NX : nullptr, *w);
    }
  delete w;
}

extern "C" void val_eval(int B, int N, double dt, const double* dts, int cent, int n, const double* vf, const double* xbar, const double* s_query,
                         const double* x_query, double* dV, double* dfdx, double* dfdxx) {
  ValueWS* w = new ValueWS;
  const Ctx ctx{0, 1, nullptr};
  for (int b = 0; b < B; ++b)
    for (int q = 0; q < n; ++q) {
      const size_t e = (size_t)b * n + q;
      value_eval(ctx, vf + (size_t)b * (N + 1) * VF_SIZE, xbar + (size_t)b * (N + 1) * NX, dts ? dts + (size_t)b * N : nullptr, N, dt, cent, s_query[e], x_query + e * NX,
                 dV ? dV + e : nullptr, dfdx ? dfdx + e * NX : nullptr, dfdxx ? dfdxx + e * NX * NX : nullptr, *w);
    }
  delete w;
}
