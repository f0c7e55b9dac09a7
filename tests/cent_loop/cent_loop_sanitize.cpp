// TEST INFRASTRUCTURE: a program of its own that runs the host build of the centroidal velocity-command targets (tests/cent_loop/cent_loop_emu.cpp, compiled
// beside this file) under the address and undefined-behaviour sanitizers (tests/test_cent_loop.py): the cases of the test, recorded with the mirror's answers,
// then state rows with NaN, +-Inf and +-1e300 in the momentum, the pose and the joints.  Every array is on the heap and exactly as long as the layout says: a
// read or write past it is the sanitizer's to see.  A finite row gives finite knots with zero padding; a non-finite one may give NaN knots, never a fault.
//   cent_loop_sanitize DESC_FILE CASES_FILE
//     DESC_FILE:  the bytes of the binding's hsqp_model_desc (centroidal)
//     CASES_FILE: doubles — the default joint state [23], the case count n, then per case
//                 alpha, t0, horizon, v_cmd [4], v_filt [4], x0 [58], times [3], states [3][58], base_vel [6], v_filt after [4]
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "cent_loop_emu.h"

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: cent_loop_sanitize DESC_FILE CASES_FILE\n"); return 2; }
  std::vector<char> image(sizeof(hsqp_model_desc));
  FILE* fp = fopen(argv[1], "rb");
  if (!fp || fread(image.data(), 1, image.size(), fp) != image.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  fclose(fp);
  fp = fopen(argv[2], "rb");
  if (!fp) { fprintf(stderr, "cannot read %s\n", argv[2]); return 2; }
  std::vector<double> cases;
  for (double v; fread(&v, sizeof v, 1, fp) == 1;) cases.push_back(v);
  fclose(fp);
  constexpr int NXS = HSQP_NX, NJ = HSQP_NJ, K = HSQP_CMD_KNOTS, C = HSQP_CMD_N;
  constexpr size_t PER = 3 + C + C + NXS + K + (size_t)K * NXS + 6 + C;
  if (cases.size() < (size_t)NJ + 1) { fprintf(stderr, "short cases file\n"); return 2; }
  const int n = (int)cases[NJ];
  if (n < 1 || cases.size() != (size_t)NJ + 1 + (size_t)n * PER) { fprintf(stderr, "cases file: %zu doubles for %d cases\n", cases.size(), n); return 2; }
  char err[256] = "";
  const std::vector<double> joints(cases.begin(), cases.begin() + NJ);
  void* h = cl_create(reinterpret_cast<const hsqp_model_desc*>(image.data()), joints.data(), err, sizeof err);
  if (!h) { fprintf(stderr, "%s\n", err); return 1; }
  bool ok = true;
  double worst = 0.0;
  // 1. the recorded cases, one instance per call
  for (int c = 0; c < n && ok; ++c) {
    const double* p = cases.data() + NJ + 1 + (size_t)c * PER;
    const double alpha = p[0], t0 = p[1], horizon = p[2];
    const std::vector<double> v_cmd(p + 3, p + 3 + C), x0(p + 3 + 2 * C, p + 3 + 2 * C + NXS);
    std::vector<double> v_filt(p + 3 + C, p + 3 + 2 * C), tt(K), ts((size_t)K * NXS), bv(6);
    const double* want = p + 3 + 2 * C + NXS;
    cl_command_targets(h, alpha, 1, v_cmd.data(), v_filt.data(), x0.data(), t0, horizon, tt.data(), ts.data(), bv.data());
    for (int i = 0; i < K; ++i) ok = ok && std::fabs(tt[i] - want[i]) <= 1e-15 * std::fabs(want[i]);
    for (size_t i = 0; i < (size_t)K * NXS; ++i) { const double d = std::fabs(ts[i] - want[K + i]); worst = d > worst ? d : worst; ok = ok && d <= 1e-12; }
    for (int i = 0; i < 6; ++i) { const double d = std::fabs(bv[i] - want[K + (size_t)K * NXS + i]); worst = d > worst ? d : worst; ok = ok && d <= 1e-12; }
    for (int i = 0; i < C; ++i) ok = ok && v_filt[i] == want[K + (size_t)K * NXS + 6 + i];
    if (!ok) fprintf(stderr, "case %d differs from the mirror (worst so far %.3e)\n", c, worst);
  }
  // 2. a batch whose rows carry non-finite and huge entries: row 0 is clean and must keep the bits it has alone
  if (ok) {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double* p0 = cases.data() + NJ + 1;
    const struct { int index; double value; } edits[] = {{0, nan}, {3, inf}, {6, -inf}, {8, nan}, {9, 1e300}, {9, nan}, {10, inf}, {12, nan}, {20, -1e300}, {34, inf}, {2, -1e300}};
    const int B = 1 + (int)(sizeof edits / sizeof edits[0]);
    std::vector<double> x0((size_t)B * NXS), v_cmd((size_t)B * C), v_filt((size_t)B * C), tt((size_t)B * K), ts((size_t)B * K * NXS, -7.0), bv((size_t)B * 6);
    for (int b = 0; b < B; ++b) {
      for (int i = 0; i < NXS; ++i) x0[(size_t)b * NXS + i] = p0[3 + 2 * C + i];
      for (int i = 0; i < C; ++i) { v_cmd[(size_t)b * C + i] = p0[3 + i]; v_filt[(size_t)b * C + i] = p0[3 + C + i]; }
      if (b > 0) x0[(size_t)b * NXS + edits[b - 1].index] = edits[b - 1].value;
    }
    cl_command_targets(h, 0.8, B, v_cmd.data(), v_filt.data(), x0.data(), 0.25, 2.0, tt.data(), ts.data(), bv.data());
    std::vector<double> vf1(p0 + 3 + C, p0 + 3 + 2 * C), tt1(K), ts1((size_t)K * NXS), bv1(6);
    cl_command_targets(h, 0.8, 1, v_cmd.data(), vf1.data(), x0.data(), 0.25, 2.0, tt1.data(), ts1.data(), bv1.data());
    for (size_t i = 0; i < (size_t)K * NXS; ++i) ok = ok && ts[i] == ts1[i] && std::isfinite(ts[i]);
    for (int i = 0; i < 6; ++i) ok = ok && bv[i] == bv1[i];
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < K; ++k) {
        const double* row = ts.data() + ((size_t)b * K + k) * NXS;
        for (int i = HSQP_CNX; i < NXS; ++i) ok = ok && row[i] == 0.0;                  // the padding of every knot, whatever the row held
        ok = ok && row[10] == 0.0 && row[11] == 0.0;                                    // roll and pitch of every knot
        for (int j = 0; j < NJ; ++j) ok = ok && row[12 + j] == joints[j];
      }
    if (!ok) fprintf(stderr, "the batch with non-finite rows\n");
  }
  cl_destroy(h);
  printf(ok ? "cent loop ok %.3e\n" : "cent loop FAILED %.3e\n", worst);
  return ok ? 0 : 1;
}
