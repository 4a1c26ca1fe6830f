// loam_lanes_localize's host-side planning (loc_plan.hpp lanes_localize_plan), run stand-alone under
// AddressSanitizer / UBSan: every product is formed in 64 bits, the plan array is written below n
// only and only when the verdict is kLocPlanOk.  The row limit's edges (1024 / 1025 rows in several
// n x k splits, a product that wraps in 32 bits), counts of 0 / 1 / cap / cap + 1 and negative, a
// corner count at and beyond the mapping stack's bound, a lane index at and beyond n_lanes,
// capacities up to the 2^31 limit, then random arguments; verdict, offsets, counts and the maxima are
// compared with a restatement in long double arithmetic.
// Prints "<cases checked> <wrong>".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../loam_velodyne-1_amd/csrc/loc_plan.hpp"

namespace {
using namespace loam;
uint64_t g_s = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
  g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17;
  return g_s;
}

struct Case {
  uint32_t n, k, P, buf;
  int32_t capC, capS, stackC;
  std::vector<uint32_t> lane;
  std::vector<int32_t> cnt;
};

int restated_verdict(const Case& c) {
  if (c.n < 1 || c.n > c.P) return kLocPlanN;
  if (c.k < 1) return kLocPlanK;
  if ((long double)c.n * (long double)c.k > 1024.0L) return kLocPlanTooMany;
  if (c.capC < 0 || c.capS < 0 || c.stackC < 0 || (long double)c.capC + (long double)c.capS > 2147483647.0L || c.buf >= 3)
    return kLocPlanCap;
  for (uint32_t i = 0; i < c.n; ++i) {
    if (c.lane[i] >= c.P) return kLocPlanLane;
    if (c.cnt[2 * i] < 0 || c.cnt[2 * i] > c.capC || c.cnt[2 * i + 1] < 0 || c.cnt[2 * i + 1] > c.capS)
      return kLocPlanCount;
    if (c.cnt[2 * i] > c.stackC) return kLocPlanStack;
  }
  return kLocPlanOk;
}

long g_cases = 0, g_wrong = 0, g_ok = 0;

void check(const Case& c) {
  ++g_cases;
  const LaneLocPlan guard = {~0ull, ~0ull, -7, -7, 0xdeadbeefu, 0xdeadbeefu};
  // exactly n entries: a write past them is the sanitizer's to find
  std::vector<LaneLocPlan> plan(c.n <= 1024 ? c.n : 0, guard);
  LaneLocShape shape = {0xdeadbeefu, -7, -7};
  const int want = restated_verdict(c);
  // (a case the restatement refuses for n may list fewer lanes than n: the function must not read them)
  const int got = lanes_localize_plan(c.n, c.k, c.lane.data(), c.cnt.data(), c.P, c.buf, c.capC, c.capS, c.stackC,
                                      plan.data(), &shape);
  bool ok = got == want;
  if (ok && want != kLocPlanOk) {  // nothing written
    ok = shape.rows == 0xdeadbeefu && shape.maxC == -7 && shape.maxS == -7;
    for (const LaneLocPlan& p : plan) ok = ok && p.offC == ~0ull && p.offS == ~0ull && p.nC == -7 && p.lane == 0xdeadbeefu;
  }
  if (ok && want == kLocPlanOk) {
    ++g_ok;
    int32_t maxC = 0, maxS = 0;
    for (uint32_t i = 0; i < c.n && ok; ++i) {
      const LaneLocPlan& p = plan[i];
      const long double slot = (long double)c.buf * (long double)c.P + (long double)c.lane[i];
      ok = (long double)p.offC == slot * (long double)c.capC && (long double)p.offS == slot * (long double)c.capS &&
           p.nC == c.cnt[2 * i] && p.nS == c.cnt[2 * i + 1] && p.lane == c.lane[i] && p.pad == 0;
      // the clouds lie inside [kOdBufs][P][cap]; the corner cloud fits the mapping stack
      ok = ok && (long double)p.offC + (long double)p.nC <= 3.0L * (long double)c.P * (long double)c.capC &&
           (long double)p.offS + (long double)p.nS <= 3.0L * (long double)c.P * (long double)c.capS && p.nC <= c.stackC &&
           (long double)p.nC + (long double)p.nS <= 2147483647.0L;
      if (p.nC > maxC) maxC = p.nC;
      if (p.nS > maxS) maxS = p.nS;
    }
    ok = ok && (long double)shape.rows == (long double)c.n * (long double)c.k && shape.rows <= 1024u && shape.maxC == maxC &&
         shape.maxS == maxS;
  }
  if (!ok) ++g_wrong;
}

Case make(uint32_t n, uint32_t k, uint32_t P, uint32_t buf, int32_t capC, int32_t capS, int32_t stackC) {
  Case c{n, k, P, buf, capC, capS, stackC, {}, {}};
  const uint32_t m = n <= 1024 ? n : 1;  // (a larger n is refused before the list is read)
  c.lane.resize(m ? m : 1);
  c.cnt.assign(2 * (size_t)(m ? m : 1), 0);
  for (uint32_t i = 0; i < m; ++i) c.lane[i] = P ? (P - 1 - i % P) : 0;
  return c;
}
}  // namespace

int main() {
  // the row limit's edges
  const uint32_t nk[][2] = {{1, 1024}, {1, 1025}, {4, 256}, {4, 257}, {32, 32}, {32, 33}, {33, 32}, {64, 16}, {64, 17},
                            {1024, 1}, {1025, 1}, {1024, 2}, {0, 1}, {1, 0}, {1, 0xffffffffu}, {0xffffffffu, 0xffffffffu},
                            {3, 0x55555556u}, {1024, 0x00400001u}, {65, 1}, {3, 3}};
  const int32_t counts[] = {-1, 0, 1, 1919, 1920, 1921};
  const int32_t countsS[] = {-1, 0, 1, 161919, 161920, 161921};
  for (auto& e : nk)
    for (uint32_t P : {1u, 4u, 65u, 1024u, 1025u})
      for (uint32_t buf : {0u, 1u, 2u, 3u})
        for (int32_t cc : counts)
          for (int32_t cs : countsS)
            for (int32_t stackC : {1920, 1919, 0}) {
              Case c = make(e[0], e[1], P, buf, 1920, 161920, stackC);
              for (size_t i = 0; i < c.cnt.size() / 2; ++i) {
                c.cnt[2 * i] = i % 3 == 1 ? 0 : cc;          // (every third lane: empty clouds)
                c.cnt[2 * i + 1] = i % 3 == 1 ? 0 : cs;
              }
              check(c);
            }
  // capacities up to the 2^31 limit, counts at and beyond them
  const int32_t caps[] = {0, 1, 1024, 1 << 21, 0x3fffffff, 0x40000000, 0x7fffffff - 7680, 0x7fffffff - 7679, 0x7fffffff, -1};
  for (int32_t capS : caps)
    for (int32_t capC : {0, 7680, 0x3fffffff, 0x40000000, 0x7fffffff})
      for (int32_t d : {-1, 0, 1})
        for (uint32_t P : {1u, 1024u})
          for (int32_t stackC : {capC, 0x7fffffff, -1}) {
            Case c = make(P, 1, P, 2, capC, capS, stackC);
            for (size_t i = 0; i < c.cnt.size() / 2; ++i) {
              const int64_t v = (int64_t)capC + (i == c.cnt.size() / 2 - 1 ? d : 0);
              c.cnt[2 * i] = (int32_t)(v > 0x7fffffff ? 0x7fffffff : v);
              c.cnt[2 * i + 1] = capS < 0 ? 0 : capS;
            }
            check(c);
          }
  // lane indices: the last lane of the list at and beyond n_lanes
  for (uint32_t bad : {1023u, 1024u, 1025u, 0x7fffffffu, 0xffffffffu}) {
    Case c = make(5, 2, 1024, 1, 1920, 161920, 1920);
    c.lane[4] = bad;
    check(c);
  }
  for (int i = 0; i < 300000; ++i) {
    const uint32_t P = 1 + (uint32_t)(rnd() % 1024);
    const uint32_t n = (uint32_t)(rnd() % (i % 7 ? (P < 64 ? P + 1 : 65) : 2 * P + 2));
    const uint32_t k = (uint32_t)(rnd() % (i % 4 ? (n ? 1024 / n + 2 : 8) : 0x100000000ull));
    const int32_t capC = (int32_t)(rnd() % (i % 5 ? 8192 : 0x80000000ull));
    const int32_t capS = (int32_t)(rnd() % (i % 3 ? (1u << 18) : 0x80000000ull));
    const int32_t stackC = i % 6 ? capC : (int32_t)(rnd() % ((uint64_t)capC + 2)) - (i % 31 ? 0 : 2);
    Case c = make(n, k, P, (uint32_t)(rnd() % (i % 11 ? 3 : 5)), capC, capS, stackC);
    for (size_t j = 0; j < c.cnt.size() / 2; ++j) {
      c.lane[j] = (uint32_t)(rnd() % (i % 13 ? P : P + 3));
      c.cnt[2 * j] = (int32_t)(rnd() % ((uint64_t)(i % 6 ? capC : (stackC < 0 ? 0 : stackC)) + (i % 17 ? 1 : 3))) - (i % 19 ? 0 : 1);
      c.cnt[2 * j + 1] = (int32_t)(rnd() % ((uint64_t)capS + (i % 23 ? 1 : 3))) - (i % 29 ? 0 : 1);
    }
    check(c);
  }
  std::printf("%ld %ld %ld\n", g_cases, g_wrong, g_ok);
  return g_wrong == 0 ? 0 : 1;
}
