// TEST INFRASTRUCTURE: the host build of the device warm start (wb_humanoid_mpc_amd/csrc/hsqp_warm.h, k_warm_start) with a one-lane
// context, for tests/test_warm_start.py.  Compiled with -ffp-contract=off, like the device code's `fp contract(off)`.
//   warm_emu <in.bin> <out.bin>
// in.bin:  int32 {mode, B, N, N_prev, cent, has_node_times}, float64 {t0, dt, total_mass}, then float64 arrays
//          node_times [B][N+1] (if has_node_times), dts [B][N], contact flags [B][N+1][2], x_init [B][58],
//          and for N_prev > 0: x_prev [B][N_prev+1][58], u_prev [B][N_prev][35], stamps_prev [B][N_prev+1]
// out.bin: float64 x [B][N+1][58], u [B][N][35], stamps [B][N+1]
#include <cstdio>
#include <vector>

#include "hsqp_warm.h"

using namespace hsqp;

static bool rd(std::FILE* f, void* p, size_t bytes) { return bytes == 0 || std::fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: warm_emu in.bin out.bin\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hd[6];
  double sc[3];
  if (!rd(f, hd, sizeof(hd)) || !rd(f, sc, sizeof(sc))) return 2;
  const int mode = hd[0], B = hd[1], N = hd[2], Np = hd[3];
  std::vector<double> nt(hd[5] ? (size_t)B * (N + 1) : 0), dts((size_t)B * N), flags((size_t)B * (N + 1) * 2), xi((size_t)B * NX);
  std::vector<double> xp((size_t)B * (Np + 1) * NX), up((size_t)B * Np * NU), tp((size_t)B * (Np + 1));
  bool ok = rd(f, nt.data(), nt.size() * 8) && rd(f, dts.data(), dts.size() * 8) && rd(f, flags.data(), flags.size() * 8) && rd(f, xi.data(), xi.size() * 8);
  if (Np > 0) ok = ok && rd(f, xp.data(), xp.size() * 8) && rd(f, up.data(), up.size() * 8) && rd(f, tp.data(), tp.size() * 8);
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "short input\n"); return 2; }
  std::vector<double> par((size_t)B * (N + 1) * NP, 0.0);
  for (size_t r = 0; r < (size_t)B * (N + 1); ++r) { par[r * NP + HSQP_P_CONTACT] = flags[2 * r]; par[r * NP + HSQP_P_CONTACT + 1] = flags[2 * r + 1]; }
  std::vector<double> x((size_t)B * (N + 1) * NX, -1.0), u((size_t)B * N * NU, -1.0), st((size_t)B * (N + 1), -1.0);
  WarmArgs w{};
  w.mode = mode; w.B = B; w.N = N; w.N_prev = Np; w.cent = hd[4];
  w.t0 = sc[0]; w.dt = sc[1]; w.total_mass = sc[2];
  w.node_times = hd[5] ? nt.data() : nullptr; w.dts = dts.data(); w.par = par.data(); w.x_init = xi.data();
  w.x_prev = xp.data(); w.u_prev = up.data(); w.stamps_prev = tp.data();
  w.x = x.data(); w.u = u.data(); w.stamps = st.data();
  const Ctx ctx{0, 1, nullptr};
  for (int b = 0; b < B; ++b)
    for (int k = 0; k <= N; ++k) warm_node(ctx, w, tp.data() + (size_t)b * (Np + 1), b, k);
  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  std::fwrite(x.data(), 8, x.size(), o); std::fwrite(u.data(), 8, u.size(), o); std::fwrite(st.data(), 8, st.size(), o);
  std::fclose(o);
  return 0;
}
