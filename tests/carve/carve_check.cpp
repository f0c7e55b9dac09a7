// The carving helper of the handle's device buffers (wb_humanoid_mpc_amd/csrc/hsqp_carve.h) on the host: built with -fsanitize=address,undefined and run
// as a program by tests/test_carve.py.  Nothing of HIP is included.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hsqp_carve.h"

namespace {

#define CHECK(cond) \
  do { if (!(cond)) { fprintf(stderr, "carve_check.cpp:%d: %s\n", __LINE__, #cond); exit(1); } } while (0)

struct Region { const char* at; size_t bytes; };   // at == nullptr: absent

// a layout of doubles, int32 and bytes, as the handle's layout functions are written: one take per region, in order
struct Spec { size_t count; size_t elem; bool present; };

std::vector<Region> run(Carve& c, const std::vector<Spec>& specs) {
  std::vector<Region> out;
  for (const Spec& s : specs) {
    const size_t before = c.bytes();
    const char* p = s.elem == 8   ? reinterpret_cast<const char*>(c.take<double>(s.count, s.present))
                    : s.elem == 4 ? reinterpret_cast<const char*>(c.take<int32_t>(s.count, s.present))
                                  : c.take<char>(s.count, s.present);
    if (!s.present) CHECK(p == nullptr && c.bytes() == before);   // an absent region is null and moves nothing
    else CHECK(c.bytes() >= before + s.count * s.elem && c.bytes() % 256 == 0);
    out.push_back({p, s.present ? s.count * s.elem : 0});
  }
  return out;
}

void check_layout(const std::vector<Spec>& specs) {
  Carve size;
  for (const Region& r : run(size, specs)) CHECK(r.at == nullptr);   // the sizing pass hands out nothing
  const size_t total = size.bytes();
  // a buffer aligned as the device allocator's are; one byte more would be found by the address sanitizer when the regions are written
  char* base = static_cast<char*>(aligned_alloc(256, total ? total : 256));
  CHECK(base != nullptr);
  Carve bind(base);
  const std::vector<Region> got = run(bind, specs);
  CHECK(bind.bytes() == total);   // the two passes agree
  const char* last_end = base;
  for (size_t i = 0; i < got.size(); ++i) {
    if (!specs[i].present) continue;
    const Region& r = got[i];
    CHECK(r.at != nullptr && reinterpret_cast<uintptr_t>(r.at) % 256 == 0);
    CHECK(r.at >= base && r.at + r.bytes <= base + total);
    CHECK(r.at >= last_end);   // in order, no overlap
    last_end = r.at + r.bytes;
    for (size_t k = 0; k < r.bytes; ++k) const_cast<char*>(r.at)[k] = (char)i;
  }
  for (size_t i = 0; i < got.size(); ++i)   // nobody wrote into a neighbour
    for (size_t k = 0; specs[i].present && k < got[i].bytes; ++k) CHECK(got[i].at[k] == (char)i);
  free(base);
}

// The loop's thirteen regions (loop_layout, hsqp_capi.hip) at (B, E) = (5, 4) with NX = 58, NU = 35, CMD_N = 4, CMD_KNOTS = 3, every size rounded up
// to 256 bytes:
//   ne        5 int32             20 ->  256      s0        5 doubles           40 ->  256
//   seq       5 * 5 int32        100 ->  256      v_cmd     5 * 4 doubles      160 ->  256
//   bad       1 int32              4 ->  256      v_filt    2 * 5 * 4 doubles  320 ->  512
//   ro_status 5 int32             20 ->  256      x         5 * 58 doubles    2320 -> 2560
//   ev        5 * 4 doubles      160 ->  256      xs        5 * 58 doubles    2320 -> 2560
//   tt        5 * 3 doubles      120 ->  256      us        5 * 35 doubles    1400 -> 1536
//   ts        5 * 3 * 58 doubles 6960 -> 7168
//   4 * 256 + 256 + 256 + 7168 + 256 + 256 + 512 + 2560 + 2560 + 1536 = 16384
void check_loop_total() {
  const size_t B = 5, E = 4, NX = 58, NU = 35, CMD_N = 4, CMD_KNOTS = 3;
  const std::vector<Spec> loop = {{B, 4, true}, {B * (E + 1), 4, true}, {1, 4, true}, {B, 4, true}, {B * E, 8, true}, {B * CMD_KNOTS, 8, true},
                                  {B * CMD_KNOTS * NX, 8, true}, {B, 8, true}, {B * CMD_N, 8, true}, {2 * B * CMD_N, 8, true}, {B * NX, 8, true},
                                  {B * NX, 8, true}, {B * NU, 8, true}};
  Carve c;
  run(c, loop);
  CHECK(loop.size() == 13 && c.bytes() == 16384);
  check_layout(loop);
}

}  // namespace

int main() {
  check_layout({{1, 1, true}});                                             // a count of 1: one byte takes 256
  check_layout({{1, 4, true}, {1, 8, true}, {1, 1, true}});
  check_layout({{5, 4, true}, {33, 8, true}, {7, 8, true}, {257, 1, true}}); // no size a multiple of 256 bytes
  check_layout({{32, 8, true}, {64, 4, true}, {512, 1, true}});             // every size a multiple of 256 bytes
  check_layout({{5, 8, true}, {290, 8, false}, {20, 8, true}});             // an absent region between two present ones
  check_layout({{3, 4, true}, {15, 4, true}, {5, 8, false}, {290, 8, false}, {2900, 8, true}, {1750, 8, false}});   // the rollout's staging, u not asked for
  check_layout({{9, 8, false}});                                            // nothing present: zero bytes
  check_loop_total();
  printf("carve ok\n");
  return 0;
}
