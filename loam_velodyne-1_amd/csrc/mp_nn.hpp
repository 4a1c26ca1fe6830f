// The mapping L-M's exact 5-NN search through the 1 m voxel hash, shared by the L-M kernels (mp.hip)
// and the diagnostic hook (mp_nn5_hook.hip).  Private to them.
#ifndef LOAM_MP_NN_HPP
#define LOAM_MP_NN_HPP

#include "mp_dev.hpp"

#pragma GCC visibility push(hidden)
namespace loam {

// (distance, index) as one ordered 64-bit key: distances are >= +0, so their bits order as they do
LOAM_D uint64_t top5_key(float d, int idx) { return ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)idx; }
// the five smallest keys so far, ascending; kept as keys, so no offer takes one apart or rebuilds it
struct Top5 {
  uint64_t K[5];
  LOAM_D float d(int k) const { return __uint_as_float((uint32_t)(K[k] >> 32)); }
  LOAM_D int i(int k) const { return (int)(uint32_t)K[k]; }
};
LOAM_D uint64_t top5_none() { return top5_key(3.4e38f, 0x7fffffff); }  // the sentinel: no point
// sorted insertion of a key below K_4 (branch-free: lt_k = key < K_k is monotone in k, so slot k
// takes K_{k-1} where lt_{k-1}, the key where lt_k alone, else keeps K_k)
LOAM_D void top5_insert(Top5& t, uint64_t key) {
  uint64_t(&K)[5] = t.K;
  const bool l0 = key < K[0], l1 = key < K[1], l2 = key < K[2], l3 = key < K[3];
  // (from the last slot down: each slot reads its lower neighbour before that one changes)
  K[4] = l3 ? K[3] : key;
  K[3] = l2 ? K[2] : (l3 ? key : K[3]);
  K[2] = l1 ? K[1] : (l2 ? key : K[2]);
  K[1] = l0 ? K[0] : (l1 ? key : K[1]);
  K[0] = l0 ? key : K[0];
}
// an offer that cannot repeat a held point (the 5-NN candidate walk: every map point is listed
// once, and a list seeded with copies of the bound B takes only keys below B)
LOAM_D void top5_offer_key(Top5& t, uint64_t key) {
  if (key < t.K[4]) top5_insert(t, key);
}
LOAM_D void top5_offer(Top5& t, uint64_t key) {
  // ascending (distance, index); a point already held is skipped (the merge of lists)
  if (key < t.K[4] && key != t.K[0] && key != t.K[1] && key != t.K[2] && key != t.K[3]) top5_insert(t, key);
}
LOAM_D void top5_offer(Top5& t, float d, int idx) { top5_offer(t, top5_key(d, idx)); }

// the 27 neighbour cells (index (dx+1) + 3(dy+1) + 9(dz+1)): centre, faces, edges, corners
// (internal linkage: a copy per code object)
namespace {
__constant__ int kCellOrder[27] = {13, 4, 10, 12, 14, 16, 22, 1, 3, 5, 7, 9, 11, 15, 17, 19, 21, 23, 25,
                                   0, 2, 6, 8, 18, 20, 24, 26};
}

// exact 5-NN within the 27 cells around q (1 m cells), as far as it matters: visited centre,
// faces, edges, corners; a cell is skipped when its box distance exceeds the current 5th
// distance or reaches the 1 m acceptance radius (the caller rejects a 5th neighbour at >= 1 m).
// Box distances are lower bounds of the float squared distances (monotone rounding of the same
// expression), so every neighbour that can be accepted is found exactly.
// t may arrive seeded with real map points (their distances to q): they bound the search from
// the start and do not change the result.
// work: candidates evaluated + (bucket ranges read << kWorkCellShift), summed per lane
constexpr int kWorkCellShift = 21;
LOAM_D void knn5(const int* start, const float4* hp, int T, float4 q, Top5& t, int& work) {
  if (T <= 0) return;
  const int cx = cell_of(q.x, 1.0f), cy = cell_of(q.y, 1.0f), cz = cell_of(q.z, 1.0f);
  const float gxl = q.x - (float)cx, gyl = q.y - (float)cy, gzl = q.z - (float)cz;
  const float gxh = (float)(cx + 1) - q.x, gyh = (float)(cy + 1) - q.y, gzh = (float)(cz + 1) - q.z;
#pragma unroll 1
  for (int o = 0; o < 27; ++o) {
    const int c = kCellOrder[o];
    const int dx = c % 3 - 1, dy = (c / 3) % 3 - 1, dz = c / 9 - 1;
    const float gx = dx < 0 ? gxl : (dx > 0 ? gxh : 0.0f);
    const float gy = dy < 0 ? gyl : (dy > 0 ? gyh : 0.0f);
    const float gz = dz < 0 ? gzl : (dz > 0 ? gzh : 0.0f);
    const float bd = sqdist(gx, gy, gz, 0.0f, 0.0f, 0.0f);
    if (bd >= 1.0f || bd > t.d(4)) continue;
    const uint32_t h = cell_hash(cx + dx, cy + dy, cz + dz) & (uint32_t)(T - 1);
    const int b0 = start[h], b1 = start[h + 1];
    work += (b1 - b0) + (1 << kWorkCellShift);
    // four independent loads in flight per step: the loop is bound by gather latency
    for (int k = b0; k < b1; k += 4) {
      float4 a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = hp[min(k + u, b1 - 1)];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (k + u < b1) top5_offer(t, sqdist(a[u].x, a[u].y, a[u].z, q.x, q.y, q.z), __builtin_bit_cast(int, a[u].w));
    }
  }
}

// batch-size launch choices (k_mp_lm_small, k_mp_nnfit<true> or + k_mp_iter): the context's Tuning
// (engine.hpp), MpBuffers::tune
constexpr int kMpQueryThreads = 256;
// lanes per query in k_mp_lm_small (streaming: the per-query search chain is the latency)
#ifndef LOAM_MP_NN_LANES
#define LOAM_MP_NN_LANES 8  // (config 3 sequential ms/sweep: 1 -> 0.972, 2 -> 1.009, 4 -> 0.943, 8 -> 0.933)
#endif
constexpr int kMpNnLanes = LOAM_MP_NN_LANES;
// k_mp_nnfit workgroup size: one wave (round 3's fit kernel, ms/step at batch 1024: 256 -> 1.27-1.29,
// 128 -> 1.16-1.20, 64 -> 1.17)
constexpr int kMpFitThreads = 64;

// The same search with the lane's work flattened: first every cell the lane may need (box
// distance below 1 m and not above the seeded 5th distance) is listed with its bucket range — 27
// independent loads in flight — then one loop runs over the concatenated candidates, so a wave
// iterates max(candidates per lane) instead of the union of its lanes' cells x buckets.  `lst` =
// the lane's LDS column (stride kMpQueryThreads).  Ranges are packed start:19 | count:13; a lane
// whose ranges do not fit falls back to knn5.
#ifndef LOAM_NN_INFLIGHT
#define LOAM_NN_INFLIGHT 8  // measured k_mp_nn ms/step: 2 -> 4.17, 4 -> 3.95, 8 -> 3.88, 16 -> 5.33
#endif
constexpr int kNnInFlight = LOAM_NN_INFLIGHT;
#ifndef LOAM_NN_LIST
#define LOAM_NN_LIST 27  // k_mp_nn list entries per lane (non-empty cells beyond it: the unlisted search)
#endif
constexpr int kNnListCap = LOAM_NN_LIST;
// cells whose bucket-range loads are in flight together
#ifndef LOAM_NN_RANGE_GROUP
#define LOAM_NN_RANGE_GROUP 27  // one-word records: all 27 in flight (ms/step: 9 -> 3.11, 27 -> 3.04; 8-byte pairs: 1 -> 3.83, 9 -> 3.51)
#endif
constexpr int kNnRangeGroup = LOAM_NN_RANGE_GROUP;
// L > 1: one of L lanes searching the same query: every lane lists the same cells, lane `sub`
// takes the candidates sub, sub + L, ... of the concatenated list (a crowded cell is shared too);
// the caller merges the L partial top-5 lists (knn5_merge)
// pending keys per lane of a deferred walk (a seeded search has 4 to 5 keys below B on average, p99
// 5 to 9, the oracle's clouds with the query moved 5 to 150 mm; more than 8 in under 2 % of queries)
constexpr int kNnPending = 8;
template <bool V>
struct NnDefer { static constexpr bool value = V; };
// diag (the test hook): which exceptional paths the lane took
constexpr int kNnDiagOverflow = 1, kNnDiagPlain = 2;
template <int S = kMpQueryThreads, int L = 1, int CAPL = 27>
LOAM_D void knn5_flat(const int* start, const uint32_t* rec, const float4* hp, int T, float4 q, Top5& t,
                      uint32_t* lst, int& work, int sub = 0, int* diag = nullptr) {
  if (T <= 0) return;
  const int cx = cell_of(q.x, 1.0f), cy = cell_of(q.y, 1.0f), cz = cell_of(q.z, 1.0f);
  const float gxl = q.x - (float)cx, gyl = q.y - (float)cy, gzl = q.z - (float)cz;
  const float gxh = (float)(cx + 1) - q.x, gyh = (float)(cy + 1) - q.y, gzh = (float)(cz + 1) - q.z;
  const float bound = t.d(4);
  int n = 0, total = 0;
  bool fits = true;
  // the range loads of a group of cells are all issued before any is used (a load whose count is
  // tested in the same block is waited for at once: one dependent round trip per cell)
#pragma unroll
  for (int g0 = 0; g0 < 27; g0 += kNnRangeGroup) {
    uint32_t rg[kNnRangeGroup];
#pragma unroll
    for (int u = 0; u < kNnRangeGroup; ++u) {
      const int o = g0 + u;
      if (o >= 27) break;
      const int c = kCellOrder[o];
      const int dx = c % 3 - 1, dy = (c / 3) % 3 - 1, dz = c / 9 - 1;
      const float gx = dx < 0 ? gxl : (dx > 0 ? gxh : 0.0f);
      const float gy = dy < 0 ? gyl : (dy > 0 ? gyh : 0.0f);
      const float gz = dz < 0 ? gzl : (dz > 0 ? gzh : 0.0f);
      const float bd = sqdist(gx, gy, gz, 0.0f, 0.0f, 0.0f);
      rg[u] = 0;
      if (bd < 1.0f && bd <= bound) {
        const uint32_t h = cell_hash(cx + dx, cy + dy, cz + dz) & (uint32_t)(T - 1);
        rg[u] = rec[h];  // the bucket's range packed in one word (hash_rec)
      }
    }
#pragma unroll
    for (int u = 0; u < kNnRangeGroup; ++u) {
      if (g0 + u >= 27) break;
      const uint32_t e = rg[u];
      if (e == kRecNone) fits = false;
      else if (e >> 19) {
        if (n < CAPL) {
          lst[n * S] = e;
          ++n;
          total += (int)(e >> 19);
        } else {
          fits = false;  // more non-empty cells than the list holds
        }
      }
    }
  }
  if (!fits) {
    if (diag) *diag |= kNnDiagPlain;
    knn5(start, hp, T, q, t, work);
    return;
  }
  work += total + (n << kWorkCellShift);
  // the list is walked one entry ahead: the LDS read of the next entry is issued when the current
  // one is taken, so its latency is not on the candidate chain
  int ci = 1, left = 0, pos = 0;
  uint32_t nx = lst[0];
  auto take = [&]() {
    pos = (int)(nx & ((1u << 19) - 1));
    left = (int)(nx >> 19);
    nx = lst[min(ci, CAPL - 1) * S];
    ++ci;
  };
  auto next = [&]() {  // index of the lane's next candidate
    if (left == 0) take();
    --left;
    return pos++;
  };
  auto skip = [&](int m) {  // pass over m candidates (the other lanes' share)
    while (m > 0) {
      if (left == 0) take();
      const int s = min(m, left);
      pos += s;
      left -= s;
      m -= s;
    }
  };
  const int mine = L == 1 ? total : (total > sub ? (total - sub + L - 1) / L : 0);
  if (L > 1 && mine > 0) skip(sub);  // (mine > 0: the list holds more than sub candidates)
  // Deferred insertion.  A seeded list is five copies of the bound B and ends as the five smallest
  // of {keys below B} and copies of B, whatever the order of the offers.  So the walk only tests
  // key < B and appends a passing key to the lane's pending list; the sorted insertions follow the
  // walk and run to the wave's largest pending count (a handful) instead of on nearly every
  // candidate step (some lane of 64 inserts at almost each).  Pending key j lies in the entries
  // CAPL - 2 - 2j (low word) and CAPL - 1 - 2j (high word) of the lane's own column, above the n
  // ranges listed; a lane whose pending list is full inserts its further keys directly, which
  // is as exact.  The wave defers when any of its lanes is seeded: an unseeded lane among them has
  // B = the sentinel, appends its first keys and inserts the rest.  A wave of unseeded lanes
  // (the first iteration) inserts directly: every candidate would pass the test there.
#ifdef LOAM_NN_NO_DEFER  // (experiment build: every walk inserts directly)
  const bool deferred = false;
#else
  const bool deferred = __builtin_amdgcn_ballot_w64(t.K[4] != top5_none()) != 0;
#endif
  constexpr int kPend0 = (CAPL - 2) * S;                                        // pending key 0 (offsets into lst)
  const int pend_full = kPend0 - 2 * S * min(kNnPending, (CAPL - n) >> 1);  // the first key that does not fit
  int pend = kPend0;
  auto walk = [&](auto defer) {
    for (int k = 0; k < mine; k += kNnInFlight) {  // independent gathers in flight per step
      int idx[kNnInFlight];
#pragma unroll
      for (int u = 0; u < kNnInFlight; ++u) {
        if (k + u < mine) {
          idx[u] = next();
          if (L > 1 && k + u + 1 < mine) skip(L - 1);
        } else {
          idx[u] = idx[0];
        }
      }
#ifdef LOAM_BOUNDS_CHECK
      for (int u = 0; u < kNnInFlight; ++u) LOAM_CHECK(idx[u] >= 0 && idx[u] < (1 << 19) + (1 << 13), idx[u], total);
#endif
      float4 a[kNnInFlight];
#pragma unroll
      for (int u = 0; u < kNnInFlight; ++u) a[u] = hp[(uint32_t)idx[u]];
#pragma unroll
      for (int u = 0; u < kNnInFlight; ++u) {
        if (k + u >= mine) continue;
        const uint64_t key = top5_key(sqdist(a[u].x, a[u].y, a[u].z, q.x, q.y, q.z), __builtin_bit_cast(int, a[u].w));
        if constexpr (decltype(defer)::value) {
          if (key < t.K[4]) {  // (= B until the lane inserts directly)
            if (pend != pend_full) {
              lst[pend] = (uint32_t)key;
              lst[pend + S] = (uint32_t)(key >> 32);
              pend -= 2 * S;
            } else {
              if (diag) *diag |= kNnDiagOverflow;
              top5_offer_key(t, key);
            }
          }
        } else {
          top5_offer_key(t, key);
        }
      }
    }
  };
  if (deferred) {
    walk(NnDefer<true>{});
    for (int pj = kPend0; pj != pend; pj -= 2 * S)  // (the wave's largest pending count)
      top5_offer_key(t, ((uint64_t)lst[pj + S] << 32) | lst[pj]);
  } else {
    walk(NnDefer<false>{});
  }
}

// the L lanes of a query group (aligned, consecutive) exchange their top-5 lists in log2(L)
// butterfly rounds; top5_offer keeps the 5 smallest (distance, index) of the union without
// duplicates, which does not depend on the order of the offers, so every lane of the group ends
// with the list a single lane's search over all the cells would have found
template <int L>
LOAM_D void knn5_merge(Top5& t) {
#pragma unroll
  for (int m = 1; m < L; m <<= 1) {
    float od[5];
    int oi[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      od[k] = __shfl_xor(t.d(k), m, 64);
      oi[k] = __shfl_xor(t.i(k), m, 64);
    }
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (oi[k] != 0x7fffffff) top5_offer(t, od[k], oi[k]);
  }
}

// an instance's search inputs, resolved once per workgroup
struct MpNnCtx {
  const float4* stack;
  const int *hcs, *hss;
  const uint32_t *hcr, *hsr;
  const float4 *hcp, *hsp, *fromC, *fromS;
  int TC, TS, nfc, nfs;
  int4* qnn;
};
LOAM_D MpNnCtx mp_nn_ctx(const MpBuffers& b, int p) {
  MpNnCtx c;
  c.stack = b.stack + (size_t)p * b.cap_stack;
  c.hcs = b.hC_start + (size_t)p * (b.tmax + 1);
  c.hss = b.hS_start + (size_t)p * (b.tmax + 1);
  c.hcr = b.hC_rec + (size_t)p * b.tmax;
  c.hsr = b.hS_rec + (size_t)p * b.tmax;
  c.hcp = b.hC_pts + (size_t)p * b.map_cap;
  c.hsp = b.hS_pts + (size_t)p * b.map_cap;
  c.TC = b.hC_T[p];
  c.TS = b.hS_T[p];
  c.nfc = b.nfrom[p * 2 + 0];
  c.nfs = b.nfrom[p * 2 + 1];
  c.fromC = b.from + (size_t)p * b.map_cap;
  c.fromS = c.fromC + c.nfc;
  c.qnn = b.q_nn + (size_t)p * b.cap_stack * 2;
  return c;
}

// the list's start: five copies of the seed bound B (see mp_nn_query), or sentinels; n0 / n1: the
// previous iteration's ordered 5-NN (i0..i3 | i4, -, distinct) when !first
LOAM_D void mp_nn_seed_from(const MpNnCtx& c, int q, bool corner, bool first, int4 n0, int4 n1, float4 sel, Top5& t,
                            int& work) {
  uint64_t start = top5_none();
  if (!first) {
    // The previous iteration's five neighbours (when they were five distinct points, n1.z) bound the
    // search: B = the largest of their (distance, index) keys at the moved query.  The list starts
    // as five copies of B and takes only keys below B, so it ends with the points below B — the
    // true 5-NN whenever they lie in the searched cells, the B point itself filling the fifth place
    // when only four lie below it (B is a real point) — and no seed needs to be offered or
    // recognised when the walk meets it again
    if (n1.z) {
      const int prev[5] = {n0.x, n0.y, n0.z, n0.w, n1.x};
      const float4* from = corner ? c.fromC : c.fromS;
      uint64_t B = 0;
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        LOAM_CHECK(prev[k] >= 0 && prev[k] < (corner ? c.nfc : c.nfs), prev[k], q);
        const float4 a = from[prev[k]];
        const uint64_t key = top5_key(sqdist(a.x, a.y, a.z, sel.x, sel.y, sel.z), prev[k]);
        B = key > B ? key : B;
      }
      work += 5;
      start = B;
    }
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) t.K[k] = start;
}

LOAM_D void mp_nn_seed(const MpNnCtx& c, int q, bool corner, bool first, float4 sel, Top5& t, int& work) {
  int4 n0 = make_int4(0, 0, 0, 0), n1 = n0;
  if (!first) { n0 = c.qnn[2 * q]; n1 = c.qnn[2 * q + 1]; }
  mp_nn_seed_from(c, q, corner, first, n0, n1, sel, t, work);
}

// the seeds for the next iteration only when the list holds five distinct map points (a rejected
// search can end with copies of B or sentinels; the list is sorted, so copies are adjacent)
LOAM_D int top5_distinct(const Top5& t) {
  return t.i(4) != 0x7fffffff && t.i(0) != t.i(1) && t.i(1) != t.i(2) && t.i(2) != t.i(3) && t.i(3) != t.i(4);
}

LOAM_D void mp_nn_store(const MpNnCtx& c, int q, const Top5& t) {
  c.qnn[2 * q] = make_int4(t.i(0), t.i(1), t.i(2), t.i(3));
  c.qnn[2 * q + 1] = make_int4(t.i(4), __float_as_int(t.d(4)), top5_distinct(t), 0);
}

template <int S = kMpQueryThreads, int L = 1, int CAPL = 27>
LOAM_D void mp_nn_query(const MpBuffers& b, const MpNnCtx& c, int q, int nsc, bool first, const loampose::MapRot& r,
                        uint32_t* lst, float4& sel, Top5& t, int& work, int sub = 0) {
  const bool corner = q < nsc;
  sel = loampose::point_to_map(r, c.stack[corner ? q : b.capC + (q - nsc)]);
  mp_nn_seed(c, q, corner, first, sel, t, work);
  if (corner) knn5_flat<S, L, CAPL>(c.hcs, c.hcr, c.hcp, c.TC, sel, t, lst, work, sub);
  else knn5_flat<S, L, CAPL>(c.hss, c.hsr, c.hsp, c.TS, sel, t, lst, work, sub);
  if constexpr (L > 1) knn5_merge<L>(t);
  LOAM_CHECK(q < b.cap_stack && (t.i(4) == 0x7fffffff || t.i(4) < (corner ? c.nfc : c.nfs)), q, t.i(4));
  if (sub == 0) mp_nn_store(c, q, t);
}

}  // namespace loam
#pragma GCC visibility pop
#endif
