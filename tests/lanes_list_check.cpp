// loam_lanes_map_import's host-side check of the caller's lane list (lanes.hpp lanes_list_check),
// run stand-alone under AddressSanitizer / UBSan: the list is a heap array of exactly n entries and
// the lanes' state arrays have exactly S, so a read beyond n or an index out of range is reported.
// Random lists with out-of-range indices (up to 2^32 - 1), repeats, failed and waiting lanes; the
// verdict and the offending position are compared with a plain restatement.
// Prints "<lists checked> <wrong verdicts>".
#include <cstdint>
#include <cstdio>
#include <set>
#include <vector>

#include "../loam_velodyne-1_amd/csrc/lanes.hpp"

namespace {
uint64_t g_s = 0x9e3779b97f4a7c15ull;
uint32_t rnd(uint32_t n) {  // [0, n)
  g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17;
  return (uint32_t)((g_s >> 16) % n);
}
}  // namespace

int main() {
  using namespace loam;
  long lists = 0, wrong = 0;
  for (int round = 0; round < 20000; ++round) {
    const int S = 1 + (int)rnd(round % 50 == 0 ? 1024 : 12);
    std::vector<int> fail((size_t)S, LOAM_OK);
    std::vector<LaneLife> life((size_t)S);
    for (int l = 0; l < S; ++l) {
      if (rnd(16) == 0) fail[l] = LOAM_E_INVAL;
      if (rnd(16) == 0) life[l].wait = (int)rnd(3);
    }
    const uint32_t n = 1 + rnd((uint32_t)S);
    std::vector<uint32_t> lane(n);  // exactly n entries
    std::vector<uint32_t> perm((size_t)S);
    for (int l = 0; l < S; ++l) perm[l] = (uint32_t)l;
    for (uint32_t i = 0; i < n; ++i) {  // distinct by default ...
      const uint32_t j = i + rnd((uint32_t)S - i);
      std::swap(perm[i], perm[j]);
      lane[i] = perm[i];
    }
    const uint32_t spoil = rnd(4);  // ... then one entry repeated or pushed out of range
    if (spoil == 1 && n > 1) lane[1 + rnd(n - 1)] = lane[0];
    if (spoil == 2) lane[rnd(n)] = rnd(2) ? (uint32_t)S + rnd(3) : 0xffffffffu - rnd(3);
    // the restatement
    int want = kLaneListOk;
    uint32_t want_bad = 0;
    std::set<uint32_t> seen_ref;
    for (uint32_t i = 0; i < n && want == kLaneListOk; ++i) {
      want_bad = i;
      if (lane[i] >= (uint32_t)S) want = kLaneListRange;
      else if (seen_ref.count(lane[i])) want = kLaneListTwice;
      else if (fail[lane[i]] != LOAM_OK) want = kLaneListFailed;
      else if (life[lane[i]].wait >= 0) want = kLaneListWaits;
      seen_ref.insert(lane[i]);
    }
    std::vector<char> seen;
    uint32_t bad = 0;
    const int got = lanes_list_check(lane.data(), n, S, fail.data(), life.data(), seen, &bad);
    ++lists;
    if (got != want || (want != kLaneListOk && bad != want_bad)) ++wrong;
  }
  std::printf("%ld %ld\n", lists, wrong);
  return wrong == 0 ? 0 : 1;
}
