// loam_lanes_open_shared's host-side capacity arithmetic (lanes.hpp lanes_shared_check), run
// stand-alone under AddressSanitizer / UBSan: every product is formed in 64 bits, so no argument
// (up to 2^32 - 1) may overflow an int on the way.  The edges of every limit and random arguments;
// the verdict is compared with a restatement in long double.
// Prints "<cases checked> <wrong verdicts>".
#include <cstdint>
#include <cstdio>

#include "../loam_velodyne-1_amd/csrc/lanes.hpp"

namespace {
uint64_t g_s = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
  g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17;
  return g_s;
}
int restated(uint32_t n, uint32_t f, uint64_t cs) {
  using namespace loam;
  if (n < 1 || n > 1024) return kSharedLanes;
  if (f < 1024 || f > 268435456u) return kSharedFromCap;
  if ((long double)n * (long double)f >= 2147483648.0L) return kSharedFromProduct;
  if ((long double)n * (long double)cs >= 2147483648.0L) return kSharedStackProduct;
  return kSharedOk;
}
}  // namespace

int main() {
  using namespace loam;
  long cases = 0, wrong = 0;
  auto check = [&](uint32_t n, uint32_t f, uint64_t cs) {
    ++cases;
    if (lanes_shared_check(n, f, cs) != restated(n, f, cs)) ++wrong;
  };
  const uint32_t ns[] = {0, 1, 2, 7, 8, 63, 64, 65, 1023, 1024, 1025, 0x7fffffffu, 0xffffffffu};
  const uint32_t fs[] = {0, 1, 1023, 1024, 1025, 1u << 20, (1u << 21) - 1, 1u << 21, (1u << 21) + 1, (1u << 28) - 1,
                         1u << 28, (1u << 28) + 1, 0x7fffffffu, 0x80000000u, 0xffffffffu};
  const uint64_t cs[] = {0, 1, 161920, (1ull << 21) - 1, 1ull << 21, (1ull << 21) + 1, (1ull << 31) - 1, 1ull << 31,
                         (1ull << 32) + 120ull * 0xffffffffull};
  for (uint32_t n : ns)
    for (uint32_t f : fs)
      for (uint64_t c : cs) check(n, f, c);
  for (int i = 0; i < 200000; ++i) {
    const uint32_t n = (uint32_t)(rnd() % (i % 4 ? 1026 : 0x100000000ull));
    const uint32_t f = (uint32_t)(rnd() % (i % 3 ? (1ull << 23) : 0x100000000ull));
    const uint64_t c = rnd() % (i % 5 ? (1ull << 23) : (1ull << 40));
    check(n, f, c);
    // on the product's edge: the largest f (and the next) that keeps n x f below 2^31
    if (n >= 1 && n <= 1024) {
      const uint32_t e = (uint32_t)(((1ull << 31) - 1) / n);
      check(n, e, 0);
      check(n, e + 1, 0);
    }
  }
  std::printf("%ld %ld\n", cases, wrong);
  return wrong == 0 ? 0 : 1;
}
