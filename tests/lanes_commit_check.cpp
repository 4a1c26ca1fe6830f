// loam_lanes_map_commit's host-side check of the lane list (lanes.hpp lanes_commit_check), run
// stand-alone under AddressSanitizer / UBSan.  The state arrays are heap blocks of exactly S entries
// and the list one of exactly n, so a read beyond either is an error of the run.  The edges: an empty
// list, n > n_lanes (the list is then not read at all: it is a null pointer here), an index at and
// beyond the range, a duplicate of the first and of the last entry, every ineligible lane state; then
// random lists against a plain restatement, which also names the entry the verdict is about.
// Prints "<cases checked> <wrong verdicts>".
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../loam_velodyne-1_amd/csrc/lanes.hpp"

namespace {
using namespace loam;
uint64_t g_s = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
  g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17;
  return g_s;
}

struct State {
  int S;
  std::unique_ptr<int[]> fail;
  std::unique_ptr<LaneLife[]> life;
  std::unique_ptr<int32_t[]> status;
  std::unique_ptr<char[]> done;
  explicit State(int s) : S(s), fail(new int[s]), life(new LaneLife[s]), status(new int32_t[s]), done(new char[s]) {
    for (int l = 0; l < s; ++l) {
      fail[l] = LOAM_OK;
      life[l] = LaneLife();
      status[l] = LOAM_LOC_SOLVED;
      done[l] = 0;
    }
  }
};

// the rules in the header's order, one lane at a time, with a linear search for the duplicate
int restated(const State& st, const std::vector<uint32_t>& list, uint32_t n, uint32_t* bad) {
  *bad = 0;
  if (n == 0 || n > (uint32_t)st.S) return kCommitCount;
  for (uint32_t i = 0; i < n; ++i) {
    *bad = i;
    const uint32_t l = list[i];
    if (l >= (uint32_t)st.S) return kCommitRange;
    for (uint32_t j = 0; j < i; ++j)
      if (list[j] == l) return kCommitTwice;
    if (st.fail[l] != LOAM_OK) return kCommitFailed;
    if (st.life[l].wait >= 0) return kCommitWaits;
    if (st.status[l] == LOAM_LOC_OFFGRID) return kCommitOffgrid;
    if (st.status[l] != LOAM_LOC_SOLVED && st.status[l] != LOAM_LOC_NO_LM) return kCommitNoFrame;
    if (st.done[l]) return kCommitDone;
  }
  return kCommitOk;
}

long g_cases = 0, g_wrong = 0;
std::vector<char> g_seen;

// want < 0: only the restatement decides
void check(const State& st, const std::vector<uint32_t>& list, uint32_t n, int want = -1, int want_bad = -1) {
  // the list as a heap block of exactly min(n, size) entries (null where the check may not read it)
  const bool readable = n >= 1 && n <= (uint32_t)st.S;
  std::unique_ptr<uint32_t[]> blk(readable ? new uint32_t[n] : nullptr);
  for (uint32_t i = 0; readable && i < n; ++i) blk[i] = list[i];
  uint32_t bad = 0xdeadbeefu, rbad = 0;
  const int got = lanes_commit_check(blk.get(), n, st.S, st.fail.get(), st.life.get(), st.status.get(), st.done.get(),
                                     g_seen, &bad);
  const int ref = restated(st, list, n, &rbad);
  ++g_cases;
  if (got != ref || bad != rbad || (want >= 0 && got != want) || (want_bad >= 0 && bad != (uint32_t)want_bad)) ++g_wrong;
}
}  // namespace

int main() {
  {  // the count
    State st(4);
    check(st, {}, 0, kCommitCount);
    check(st, {0, 1, 2, 3, 0}, 5, kCommitCount);
    check(st, {}, 0xffffffffu, kCommitCount);
    check(st, {0, 1, 2, 3}, 4, kCommitOk);
    check(st, {3}, 1, kCommitOk);
    State one(1);
    check(one, {0}, 1, kCommitOk);
    check(one, {0, 0}, 2, kCommitCount);
    check(one, {1}, 1, kCommitRange, 0);
  }
  {  // range and duplicates at both ends
    State st(5);
    check(st, {4, 5}, 2, kCommitRange, 1);
    check(st, {0xffffffffu}, 1, kCommitRange, 0);
    check(st, {0x80000000u, 1}, 2, kCommitRange, 0);
    check(st, {2, 2}, 2, kCommitTwice, 1);
    check(st, {0, 1, 2, 3, 0}, 5, kCommitTwice, 4);
    check(st, {0, 1, 2, 4, 4}, 5, kCommitTwice, 4);
    check(st, {4, 4, 2, 1, 0}, 5, kCommitTwice, 1);
    check(st, {4, 3, 2, 1, 0}, 5, kCommitOk);
  }
  {  // every ineligible lane state, at the first and at the last entry of the list
    const int32_t statuses[] = {LOAM_LOC_SOLVED, LOAM_LOC_NO_LM, LOAM_LOC_OFFGRID, LOAM_LOC_NONE, 4, -1};
    const int verdict[] = {kCommitOk, kCommitOk, kCommitOffgrid, kCommitNoFrame, kCommitNoFrame, kCommitNoFrame};
    for (int k = 0; k < 6; ++k)
      for (int at = 0; at < 3; at += 2) {
        State st(3);
        st.status[at] = statuses[k];
        check(st, {0, 1, 2}, 3, verdict[k], verdict[k] ? at : -1);
      }
    for (int at = 0; at < 3; at += 2) {
      State a(3), b(3), c(3), d(3);
      a.fail[at] = LOAM_E_CAPACITY;
      check(a, {0, 1, 2}, 3, kCommitFailed, at);
      b.life[at].wait = 0;
      check(b, {0, 1, 2}, 3, kCommitWaits, at);
      b.life[at].wait = 3;
      check(b, {0, 1, 2}, 3, kCommitWaits, at);
      c.done[at] = 1;
      check(c, {0, 1, 2}, 3, kCommitDone, at);
      check(c, {1}, 1, kCommitOk);  // (a lane that is not listed does not matter)
      // the order of the rules: failed before waiting before the status before committed
      d.fail[at] = LOAM_E_INVAL; d.life[at].wait = 1; d.status[at] = LOAM_LOC_NONE; d.done[at] = 1;
      check(d, {0, 1, 2}, 3, kCommitFailed, at);
      d.fail[at] = LOAM_OK;
      check(d, {0, 1, 2}, 3, kCommitWaits, at);
      d.life[at].wait = -1;
      check(d, {0, 1, 2}, 3, kCommitNoFrame, at);
      d.status[at] = LOAM_LOC_NO_LM;
      check(d, {0, 1, 2}, 3, kCommitDone, at);
    }
  }
  // random states and lists: mostly eligible lanes and permutations, so that every rule is reached
  for (int it = 0; it < 200000; ++it) {
    const int S = 1 + (int)(rnd() % (it % 8 ? 12 : 1024));
    State st(S);
    for (int l = 0; l < S; ++l) {
      const uint64_t r = rnd() % 64;
      if (r == 0) st.fail[l] = LOAM_E_CAPACITY;
      if (r == 1) st.life[l].wait = (int)(rnd() % 3);
      if (r == 2) st.status[l] = LOAM_LOC_OFFGRID;
      if (r == 3) st.status[l] = LOAM_LOC_NONE;
      if (r == 4) st.done[l] = 1;
      if (r >= 32) st.status[l] = LOAM_LOC_NO_LM;
    }
    uint32_t n = (uint32_t)(rnd() % (uint64_t)(S + 2));
    std::vector<uint32_t> list(n);
    if (it % 3 == 0) {  // a prefix of a permutation: no duplicate, in range
      std::vector<uint32_t> perm((size_t)S);
      for (int l = 0; l < S; ++l) perm[l] = (uint32_t)l;
      for (int l = S - 1; l > 0; --l) std::swap(perm[l], perm[rnd() % (uint64_t)(l + 1)]);
      for (uint32_t i = 0; i < n && i < (uint32_t)S; ++i) list[i] = perm[i];
      for (uint32_t i = (uint32_t)S; i < n; ++i) list[i] = 0;
    } else {
      for (uint32_t i = 0; i < n; ++i) list[i] = (uint32_t)(rnd() % (uint64_t)(it % 5 ? S : S + 1));
    }
    check(st, list, n);
  }
  std::printf("%ld %ld\n", g_cases, g_wrong);
  return g_wrong == 0 ? 0 : 1;
}
