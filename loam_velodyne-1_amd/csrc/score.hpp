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

}  // namespace loam
#endif
