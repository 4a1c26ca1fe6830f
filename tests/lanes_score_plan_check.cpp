// loam_lanes_score's host-side launch arithmetic (score.hpp lanes_score_plan), run stand-alone under
// AddressSanitizer / UBSan: every product is formed in 64 bits, the plan array is written below n
// only and only when the verdict is kLanePlanOk.  The limits' edges (n x k = 65 536 and 65 537, a
// lane with empty clouds, counts of 1 / 1024 / 1025, capS at a large max_points) and random
// arguments; verdict, offsets, tiles and launch shape are compared with a restatement in 64-bit /
// long double arithmetic.
// Prints "<cases checked> <wrong>".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../loam_velodyne-1_amd/csrc/score.hpp"

namespace {
using namespace loam;
uint64_t g_s = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
  g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17;
  return g_s;
}

struct Case {
  uint32_t n, k, P, buf;
  int32_t capC, capS;
  std::vector<uint32_t> lane;
  std::vector<int32_t> cnt;
};

long double ceil_div_1024(long double v) {
  long long t = (long long)(v / 1024.0L);
  while ((long double)t * 1024.0L < v) ++t;
  return (long double)t;
}

int restated_verdict(const Case& c) {
  if (c.n < 1 || c.n > c.P) return kLanePlanN;
  if (c.k < 1) return kLanePlanK;
  if ((long double)c.n * (long double)c.k > 65536.0L) return kLanePlanRows;
  const long double cap_max = 2147483648.0L - 1024.0L;
  if (c.capC < 0 || c.capS < 0 || (long double)c.capC >= cap_max || (long double)c.capS >= cap_max || c.buf >= 3)
    return kLanePlanCap;
  for (uint32_t i = 0; i < c.n; ++i) {
    if (c.lane[i] >= c.P) return kLanePlanLane;
    if (c.cnt[2 * i] < 0 || c.cnt[2 * i] > c.capC || c.cnt[2 * i + 1] < 0 || c.cnt[2 * i + 1] > c.capS)
      return kLanePlanCount;
  }
  return kLanePlanOk;
}

long g_cases = 0, g_wrong = 0;

void check(const Case& c) {
  ++g_cases;
  const LaneScorePlan guard = {~0ull, ~0ull, -7, -7, -7, -7};
  // exactly n entries: a write past them is the sanitizer's to find
  std::vector<LaneScorePlan> plan(c.n <= (1u << 20) ? c.n : 0, guard);
  LaneScoreShape shape = {0xdeadbeefu, 0xdeadbeefdeadbeefull};
  const int want = restated_verdict(c);
  // (a case the restatement refuses for n may list fewer lanes than n: the function must not read them)
  const int got = lanes_score_plan(c.n, c.k, c.lane.data(), c.cnt.data(), c.P, c.buf, c.capC, c.capS, plan.data(), &shape);
  bool ok = got == want;
  if (ok && want != kLanePlanOk) {  // nothing written
    ok = shape.grid_x == 0xdeadbeefu && shape.tiles == 0xdeadbeefdeadbeefull;
    for (const LaneScorePlan& p : plan) ok = ok && p.offC == ~0ull && p.nC == -7 && p.tiles == -7;
  }
  if (ok && want == kLanePlanOk) {
    long double tiles = 0.0L;
    for (uint32_t i = 0; i < c.n && ok; ++i) {
      const LaneScorePlan& p = plan[i];
      const long double slot = (long double)c.buf * (long double)c.P + (long double)c.lane[i];
      const long double tc = ceil_div_1024((long double)c.cnt[2 * i]), ts = ceil_div_1024((long double)c.cnt[2 * i + 1]);
      ok = (long double)p.offC == slot * (long double)c.capC && (long double)p.offS == slot * (long double)c.capS &&
           p.nC == c.cnt[2 * i] && p.nS == c.cnt[2 * i + 1] && (long double)p.tiles_c == tc &&
           (long double)p.tiles == tc + ts;
      // the cloud lies inside [kOdBufs][P][cap]; the last tile's largest index is an int
      ok = ok && (long double)p.offC + (long double)c.capC <= 3.0L * (long double)c.P * (long double)c.capC &&
           (long double)p.offS + (long double)c.capS <= 3.0L * (long double)c.P * (long double)c.capS &&
           (long double)p.tiles_c * 1024.0L <= 2147483647.0L && ts * 1024.0L <= 2147483647.0L;
      tiles += tc + ts;
    }
    ok = ok && (long double)shape.grid_x == (long double)c.n * (long double)c.k && shape.grid_x <= 65536u &&
         (long double)shape.tiles == tiles * (long double)c.k;
  }
  if (!ok) ++g_wrong;
}

Case make(uint32_t n, uint32_t k, uint32_t P, uint32_t buf, int32_t capC, int32_t capS) {
  Case c{n, k, P, buf, capC, capS, {}, {}};
  const uint32_t m = n <= 65536 ? n : 1;  // (a larger n is refused before the list is read)
  c.lane.resize(m ? m : 1);
  c.cnt.assign(2 * (size_t)(m ? m : 1), 0);
  for (uint32_t i = 0; i < m; ++i) c.lane[i] = P ? (P - 1 - i % P) : 0;
  return c;
}
}  // namespace

int main() {
  // the row limit's edges
  const uint32_t nk[][2] = {{1, 65536}, {1, 65537}, {4, 16384}, {4, 16385}, {64, 1024}, {64, 1025}, {1024, 64}, {1024, 65},
                            {65536, 1}, {65537, 1}, {0, 1}, {1, 0}, {1, 0xffffffffu}, {0xffffffffu, 0xffffffffu},
                            {1024, 0x00400001u}, {65, 3}, {3, 6}};
  const int32_t counts[] = {0, 1, 1023, 1024, 1025, 2047, 2048, 2049};
  for (auto& e : nk)
    for (uint32_t P : {1u, 4u, 65u, 1024u, 65536u})
      for (uint32_t buf : {0u, 1u, 2u, 3u})
        for (int32_t cc : counts)
          for (int32_t cs : counts) {
            if (e[0] >= 65536 && cc != cs) continue;  // (the long lists: the diagonal only)
            Case c = make(e[0], e[1], P, buf, 1920, 161920);
            for (size_t i = 0; i < c.cnt.size() / 2; ++i) {
              c.cnt[2 * i] = i % 3 == 1 ? 0 : cc;          // (every third lane: empty clouds)
              c.cnt[2 * i + 1] = i % 3 == 1 ? 0 : cs;
            }
            check(c);
          }
  // capS at a large max_points, counts at and beyond the capacities, negative counts, the cap limit
  const int32_t caps[] = {0, 1, 1024, 1 << 21, (1 << 21) + 1, 0x7fffffff - 1024, 0x7fffffff - 1023, 0x7fffffff, -1};
  for (int32_t capS : caps)
    for (int32_t capC : {0, 7680, 0x7fffffff - 1024, 0x7fffffff - 1023})
      for (int32_t d : {-1, 0, 1})
        for (uint32_t P : {1u, 1024u}) {
          Case c = make(P, 3, P, 2, capC, capS);
          for (size_t i = 0; i < c.cnt.size() / 2; ++i) {
            c.cnt[2 * i] = (int32_t)((int64_t)capC + (i == c.cnt.size() / 2 - 1 ? d : 0));  // (capC < 2^31 - 1)
            c.cnt[2 * i + 1] = capS < 0 ? 0 : capS;
          }
          check(c);
        }
  // lane indices: the last lane of the list out of range
  for (uint32_t bad : {1024u, 1025u, 0x7fffffffu, 0xffffffffu}) {
    Case c = make(5, 2, 1024, 1, 1920, 161920);
    c.lane[4] = bad;
    check(c);
  }
  for (int i = 0; i < 200000; ++i) {
    const uint32_t P = 1 + (uint32_t)(rnd() % 1024);
    const uint32_t n = (uint32_t)(rnd() % (i % 7 ? P + 1 : 2 * P + 2));
    const uint32_t k = (uint32_t)(rnd() % (i % 4 ? (n ? 65536 / n + 2 : 8) : 0x100000000ull));
    const int32_t capC = (int32_t)(rnd() % (i % 5 ? 8192 : 0x80000000ull));
    const int32_t capS = (int32_t)(rnd() % (i % 3 ? (1u << 18) : 0x80000000ull));
    Case c = make(n, k, P, (uint32_t)(rnd() % (i % 11 ? 3 : 5)), capC, capS);
    for (size_t j = 0; j < c.cnt.size() / 2; ++j) {
      c.lane[j] = (uint32_t)(rnd() % (i % 13 ? P : P + 3));
      c.cnt[2 * j] = (int32_t)(rnd() % ((uint64_t)capC + (i % 17 ? 1 : 3))) - (i % 19 ? 0 : 1);
      c.cnt[2 * j + 1] = (int32_t)(rnd() % ((uint64_t)capS + (i % 23 ? 1 : 3))) - (i % 29 ? 0 : 1);
    }
    check(c);
  }
  std::printf("%ld %ld\n", g_cases, g_wrong);
  return g_wrong == 0 ? 0 : 1;
}
