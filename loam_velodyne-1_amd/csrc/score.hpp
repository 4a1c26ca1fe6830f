// loam_map_score: many candidate poses of one sweep scored against the whole streaming map
// (engine-internal).  One index of the map per call (the store packed in canonical order, each
// kind hashed into 1 m cells), shared by every candidate; per candidate and cloud the number of
// points whose nearest map point of the same kind is closer than max_dist and the truncated sum of
// squared nearest distances.
//
// The per-point search (score_nearest) is LOAM_HD: tests/score_check.cpp compiles it for the host
// and compares it with a brute-force loop.
#ifndef LOAM_SCORE_HPP
#define LOAM_SCORE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_common.hpp"
#include "mp.hpp"
#include "od.hpp"

namespace loam {

constexpr int kScoreMax = 65536;   // LOAM_SCORE_MAX
constexpr int kScoreThreads = 256, kScorePer = 4;
constexpr int kScoreTile = kScoreThreads * kScorePer;  // query points of one workgroup (of one partial sum)
constexpr int kScoreTMax = 1 << 20;                    // buckets of one kind's table at most
constexpr float kScoreCoordMax = 16777216.0f;          // a transformed coordinate beyond 2^24: no neighbour

// one kind's index: bucket b = pts[start[b] .. start[b + 1]), T a power of two >= 64 (hash_build_pair
// with 1 m cells).  A bucket holds whole cells, possibly several; the 27 cells around any cell lie
// in 27 different buckets (tests/test_cellhash.py).
struct ScoreMap {
  const int* start;
  const float4* pts;
  int T;
};

LOAM_HD bool score_finite3(const float4& p) {
  const float big = 3.402823466e+38f;
  return fabsf(p.x) <= big && fabsf(p.y) <= big && fabsf(p.z) <= big;  // (false for a NaN)
}

// lower bound of sqdist from (x, y, z) to any point of the unit cell (ix, iy, iz): the same
// expression as sqdist on the per-axis gaps, whose rounding is monotone
LOAM_HD float score_cell_d2(int ix, int iy, int iz, float x, float y, float z) {
  const float gx = fmaxf(fmaxf((float)ix - x, x - (float)(ix + 1)), 0.0f);
  const float gy = fmaxf(fmaxf((float)iy - y, y - (float)(iy + 1)), 0.0f);
  const float gz = fmaxf(fmaxf((float)iz - z, z - (float)(iz + 1)), 0.0f);
  return loamdev::sqdist(gx, gy, gz, 0.0f, 0.0f, 0.0f);
}

// min(r2, the smallest sqdist(a, q) over the indexed points a), exact for r2 <= 1: a point closer
// than 1 m lies in one of the 27 cells around q's.  The own cell first, then the other 26, a cell
// skipped when its box is not closer than the best so far.  A query with a non-finite coordinate or
// one beyond 2^24 has no neighbour (no lookup).  cand / cells count the points and buckets read.
LOAM_HD float score_nearest(const ScoreMap& m, float x, float y, float z, float r2, uint32_t& cand, uint32_t& cells) {
  float best = r2;
  if (m.T <= 0 || !(fabsf(x) <= kScoreCoordMax && fabsf(y) <= kScoreCoordMax && fabsf(z) <= kScoreCoordMax))
    return best;
  const int cx = loamdev::cell_of(x, 1.0f), cy = loamdev::cell_of(y, 1.0f), cz = loamdev::cell_of(z, 1.0f);
  const uint32_t mask = (uint32_t)m.T - 1u;
  for (int c = 0; c < 27; ++c) {
    const int k = c == 0 ? 13 : (c <= 13 ? c - 1 : c);  // 13: the own cell
    const int ix = cx + k % 3 - 1, iy = cy + (k / 3) % 3 - 1, iz = cz + k / 9 - 1;
    if (c != 0 && !(score_cell_d2(ix, iy, iz, x, y, z) < best)) continue;
    const uint32_t h = loamdev::cell_hash(ix, iy, iz) & mask;
#ifdef __HIP_DEVICE_COMPILE__
    const int2 se = loamdev::load_pair(m.start + h);  // (one 8-byte load for the bucket's two starts)
    const int s0 = se.x, s1 = se.y;
#else
    const int s0 = m.start[h], s1 = m.start[h + 1];
#endif
    ++cells;
    cand += (uint32_t)(s1 - s0);
    for (int i = s0; i < s1; ++i) {
      const float4 a = m.pts[i];
      const float d = loamdev::sqdist(a.x, a.y, a.z, x, y, z);
      if (d < best) best = d;
    }
  }
  return best;
}

// one (candidate, tile) partial: the tile's scored points, its inliers, the map points and buckets
// its searches read, the fp64 sum of its terms
struct ScorePart {
  uint32_t scored, in, cand, cells;
  double sum;
};
static_assert(sizeof(ScorePart) == 24, "ScorePart layout");

// ---- loam_lanes_score: k poses for each of n listed lanes, the lanes' Last clouds read in place
// one listed lane of a call: where its Last clouds lie (elements from OdBuffers::lastC / lastS),
// their sizes and tiles (corner tiles first, as k_mp_score has them)
struct LaneScorePlan {
  uint64_t offC, offS;
  int32_t nC, nS;
  int32_t tiles_c, tiles;
};
static_assert(sizeof(LaneScorePlan) == 32, "LaneScorePlan layout");
// the launch: one workgroup per (listed lane, pose) on x (gridDim.y stops at 65 535)
struct LaneScoreShape {
  uint32_t grid_x;   // n x k rows
  uint64_t tiles;    // tile bodies of the launch: k x the listed lanes' tiles
};
enum { kLanePlanOk = 0, kLanePlanN, kLanePlanK, kLanePlanRows, kLanePlanCap, kLanePlanLane, kLanePlanCount };
// loam_lanes_score's launch arithmetic (host only): kLanePlanOk and plan[0..n) / shape, or which
// limit the arguments break (nothing is written then).  lane[i] < P is listed lane i, cnt[2 i] /
// cnt[2 i + 1] the corner / surf count of its Last clouds in buffer buf of [kOdBufs][P][capC | capS].
// Every product is formed in 64 bits; a cloud's last tile must index below 2^31.
inline int lanes_score_plan(uint32_t n, uint32_t k, const uint32_t* lane, const int32_t* cnt, uint32_t P, uint32_t buf,
                            int32_t capC, int32_t capS, LaneScorePlan* plan, LaneScoreShape* shape) {
  if (n == 0 || n > P) return kLanePlanN;
  if (k == 0) return kLanePlanK;
  if ((uint64_t)n * (uint64_t)k > (uint64_t)kScoreMax) return kLanePlanRows;
  const int64_t cap_max = ((int64_t)1 << 31) - kScoreTile;  // (a tile's base + kScoreTile - 1 is an int)
  if (capC < 0 || capS < 0 || capC >= cap_max || capS >= cap_max || buf >= (uint32_t)kOdBufs) return kLanePlanCap;
  for (uint32_t i = 0; i < n; ++i) {
    if (lane[i] >= P) return kLanePlanLane;
    if (cnt[2 * i] < 0 || cnt[2 * i] > capC || cnt[2 * i + 1] < 0 || cnt[2 * i + 1] > capS) return kLanePlanCount;
  }
  uint64_t tiles = 0;
  for (uint32_t i = 0; i < n; ++i) {
    LaneScorePlan& p = plan[i];
    const uint64_t slot = (uint64_t)buf * P + lane[i];
    p.offC = slot * (uint64_t)capC;
    p.offS = slot * (uint64_t)capS;
    p.nC = cnt[2 * i];
    p.nS = cnt[2 * i + 1];
    p.tiles_c = (int32_t)(((int64_t)p.nC + kScoreTile - 1) / kScoreTile);
    p.tiles = p.tiles_c + (int32_t)(((int64_t)p.nS + kScoreTile - 1) / kScoreTile);
    tiles += (uint64_t)p.tiles;
  }
  shape->grid_x = n * k;
  shape->tiles = tiles * (uint64_t)k;
  return kLanePlanOk;
}

// the call's working set: allocated on demand, grown, kept until loam_destroy
struct MpScore {
  int cloud_cap = 0;        // query points per cloud q holds
  float4* q = nullptr;      // [2][cloud_cap] the corner cloud, then the surf cloud
  float* pose = nullptr;    // device [kScoreMax][6]
  loam_score_result* res = nullptr;  // device [kScoreMax]
  unsigned long long* work = nullptr;  // device [2]: points, buckets read (profiling)
  char* pin = nullptr;      // pinned: pose | res | work
  float* pose_h() const { return (float*)pin; }
  loam_score_result* res_h() const { return (loam_score_result*)(pin + (size_t)kScoreMax * 6 * sizeof(float)); }
  unsigned long long* work_h() const { return (unsigned long long*)(res_h() + kScoreMax); }
  // the map index: both kinds' tables and bucket-ordered points
  int idx_pts = 0, idx_T = 0;  // points `out` holds, buckets each table holds
  int* start = nullptr;     // [2][idx_T + 1]
  int* fill = nullptr;      // [2][idx_T]
  float4* out = nullptr;    // [idx_pts] corner points, then surf points
  int* cnt = nullptr;       // [4] corner, surf counts | their table sizes
  ScorePart* part = nullptr;  // [part_cap] a chunk of candidates x tiles
  size_t part_cap = 0;
  // loam_lanes_score's plan block (allocated by the first call, regrown when lanes with more lanes
  // are opened): pinned, the lanes' nlast words as they come down ([plan_lanes][kOdBufs][2]) and
  // the listed lanes' LaneScorePlan entries as they go up; device, those entries
  int plan_lanes = 0;
  char* plan_pin = nullptr;
  LaneScorePlan* plan = nullptr;  // device [plan_lanes]
  int* nlast_h() const { return (int*)plan_pin; }
  LaneScorePlan* plan_h() const { return (LaneScorePlan*)(plan_pin + (size_t)plan_lanes * kOdBufs * 2 * sizeof(int)); }
};
void mp_score_free(MpScore& S);
// the tables, and room for clouds of up to cloud_max points each; then the index for a map of
// nC + nS points and the partials of one chunk of the n candidates.  Both free what they replace:
// the caller's stream holds no work that reads it (the first before anything is enqueued, the
// second after the synchronisation that brought the map's sizes)
hipError_t mp_score_reserve(MpScore& S, int cloud_max);
hipError_t mp_score_reserve_map(MpScore& S, int nC, int nS, int ncorner, int nsurf, int n);
// the store of s (instance 0) packed into s.vin (the caller ran mp_map_table: nC corner points of
// `total`) and indexed; n poses (S.pose) scored on the clouds in S.q (ncorner, nsurf points) with
// r2 = max_dist^2; the results into S.res_h() (with `count` also the calls' sums of the partials'
// work counters into S.work_h()): the caller synchronises st, then reads them
hipError_t mp_score_run(MpScore& S, MpBuffers& s, MapIo& io, int nC, int total, int ncorner, int nsurf, float r2, int n,
                        bool count, hipStream_t st, Prof* prof);

// both kinds' indexes as the scoring kernels read them
struct ScoreIndex {
  const int* start[2];
  const float4* pts[2];
  const int* tsize;  // [2]
};
// the index mp_score_run and mp_lanes_score_run share: the store of s packed into s.vin in
// canonical order, both kinds hashed into 1 m cells (mp_score_reserve_map made room)
hipError_t mp_score_index(MpScore& S, MpBuffers& s, MapIo& io, int nC, int total, hipStream_t st, Prof* prof,
                          ScoreIndex* idx);
// loam_lanes_score's plan block for `lanes` lanes; frees what it replaces (nothing enqueued reads it)
hipError_t mp_score_reserve_plan(MpScore& S, int lanes);
// n listed lanes (their entries in S.plan_h()) x k poses (S.pose, row i k + j) scored on the lanes'
// Last clouds in place (lastC / lastS: OdBuffers' bases) against the store of s, indexed as
// mp_score_run does; the n k results into S.res_h(), with `count` the work counters into
// S.work_h(): the caller synchronises st, then reads them
hipError_t mp_lanes_score_run(MpScore& S, MpBuffers& s, MapIo& io, int nC, int total, const float4* lastC,
                              const float4* lastS, const LaneScoreShape& shape, int n, int k, float r2, bool count,
                              hipStream_t st, Prof* prof);

}  // namespace loam
#endif
