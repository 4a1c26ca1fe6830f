// loam_map_score's device code (score.hpp): the map index and the scoring kernels.
//
//  index      the store packed in canonical order into its idle vin (mp_map_pack, as the export),
//             both kinds hashed into 1 m cells by the grid-per-cloud build (hash_build_pair, spread)
//  k_mp_score one workgroup per (candidate, tile of kScoreTile query points): corner tiles first,
//             then surf tiles; a lane takes kScorePer points.  The candidate's rotation is
//             evaluated once per workgroup.  One (counts, fp64 sum) partial per workgroup.
//  k_mp_score_reduce  one lane per candidate adds its partials in tile order.
//  k_lanes_score  loam_lanes_score: one workgroup per (listed lane, pose) walks the lane's Last
//             clouds in place, tile by tile (the tile body is k_mp_score's), and writes the row.
//
// Every sum has a fixed order (lane-local over the lane's points, the wave's butterfly, the
// workgroup's waves, the tiles), so a candidate's result does not depend on the call it is part
// of.  No workgroup waits for another, and no floating-point atomic is used.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dev_common.hpp"
#include "engine.hpp"
#include "mp.hpp"
#include "od.hpp"
#include "pose_math.hpp"
#include "score.hpp"

using namespace loamdev;

namespace loam {

namespace {

constexpr size_t kScorePartBytes = (size_t)32 << 20;  // partials of one chunk of candidates at most

struct ScoreArgs {
  const float4* q[2];   // the corner / surf query cloud
  int nq[2];
  int tiles_c, tiles;   // corner tiles, all tiles
  const int* start[2];  // the two indexes
  const float4* pts[2];
  const int* tsize;     // [2] their table sizes
  const float* pose;    // [n][6]
  float r2;
  int h0;               // first candidate of this launch
  ScorePart* part;      // [candidates of the launch][tiles]
};

constexpr int kScoreWaves = kScoreThreads / 64;

// the candidate pose's map_rot, once per workgroup: the three cosines by wave 0, the sines by wave 1
// (the caller's __syncthreads follows)
__device__ __forceinline__ void score_rot_eval(const float* T, double* rot) {
  const int tid = threadIdx.x;
  if (tid < 3) rot[2 * tid] = dcos(T[tid]);
  else if (tid >= 64 && tid < 67) rot[2 * (tid - 64) + 1] = dsin(T[tid - 64]);
}
__device__ __forceinline__ loampose::MapRot score_rot_read(const float* T, const double* rot) {
  loampose::MapRot R;
  R.c0 = rot[0]; R.s0 = rot[1]; R.c1 = rot[2]; R.s1 = rot[3]; R.c2 = rot[4]; R.s2 = rot[5];
  R.t3 = T[3]; R.t4 = T[4]; R.t5 = T[5];
  return R;
}

// The tile body k_mp_score and k_lanes_score share.  The lane's kScorePer points of the tile at
// `base` of the cloud q (n >= 1 points) ...
__device__ __forceinline__ void score_tile_load(const float4* q, int n, int base, float4* p, bool* use) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int r = 0; r < kScorePer; ++r) {
    const int i = base + r * kScoreThreads + tid;
    p[r] = q[min(i, n - 1)];  // (a tile holds at least one point: n >= 1)
    use[r] = i < n && score_finite3(p[r]);
  }
}
// ... searched at R and summed: lane-local in r order, the wave's butterfly over xor 32 .. 1, then
// (behind one __syncthreads) the waves in order.  The tile's partial is returned by thread 0 (the
// other threads' value is not meaningful).  wsum / wcnt: the workgroup's LDS words of this tile; a
// caller that runs several tiles alternates between two sets, so that no wave writes a set thread 0
// still reads.
__device__ __forceinline__ ScorePart score_tile_eval(const float4* p, const bool* use, const ScoreMap& m,
                                                     const loampose::MapRot& R, float r2, double* wsum,
                                                     uint32_t (*wcnt)[4]) {
  const int tid = threadIdx.x;
  double sum = 0.0;
  uint32_t scored = 0, in = 0, cand = 0, cells = 0;
#pragma unroll
  for (int r = 0; r < kScorePer; ++r) {
    if (!use[r]) continue;
    const float4 w = loampose::point_to_map(R, p[r]);
    const float d = score_nearest(m, w.x, w.y, w.z, r2, cand, cells);
    ++scored;
    in += d < r2 ? 1u : 0u;
    sum += (double)d;
  }
  // the wave (every lane is active), then the waves in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += xor_f64(sum, o);
    scored += xor_u32(scored, o);
    in += xor_u32(in, o);
    cand += xor_u32(cand, o);
    cells += xor_u32(cells, o);
  }
  const int wv = tid >> 6;
  if ((tid & 63) == 0) {
    wsum[wv] = sum;
    wcnt[wv][0] = scored;
    wcnt[wv][1] = in;
    wcnt[wv][2] = cand;
    wcnt[wv][3] = cells;
  }
  __syncthreads();
  ScorePart o;
  o.sum = 0.0;
  o.scored = o.in = o.cand = o.cells = 0;
  if (tid == 0) {
    o.sum = wsum[0];
    o.scored = wcnt[0][0];
    o.in = wcnt[0][1];
    o.cand = wcnt[0][2];
    o.cells = wcnt[0][3];
    for (int k = 1; k < kScoreWaves; ++k) {
      o.sum += wsum[k];
      o.scored += wcnt[k][0];
      o.in += wcnt[k][1];
      o.cand += wcnt[k][2];
      o.cells += wcnt[k][3];
    }
  }
  return o;
}

__global__ __launch_bounds__(kScoreThreads) void k_mp_score(ScoreArgs a) {
  const int tid = threadIdx.x, tile = blockIdx.y;
  const int kind = tile < a.tiles_c ? 0 : 1;
  const int n = a.nq[kind], base = (kind ? tile - a.tiles_c : tile) * kScoreTile;
  // the lane's points: all loads before the rotation is waited for
  float4 p[kScorePer];
  bool use[kScorePer];
  score_tile_load(a.q[kind], n, base, p, use);
  __shared__ double rot[6];
  __shared__ double wsum[kScoreWaves];
  __shared__ uint32_t wcnt[kScoreWaves][4];
  const float* T = a.pose + (size_t)(a.h0 + blockIdx.x) * 6;
  score_rot_eval(T, rot);
  __syncthreads();
  const loampose::MapRot R = score_rot_read(T, rot);
  const ScoreMap m = {a.start[kind], a.pts[kind], a.tsize[kind]};
  const ScorePart o = score_tile_eval(p, use, m, R, a.r2, wsum, wcnt);
  if (tid == 0) a.part[(size_t)blockIdx.x * a.tiles + tile] = o;
}

struct LanesScoreArgs {
  const float4* last[2];      // OdBuffers::lastC / lastS
  const LaneScorePlan* plan;  // [n] the listed lanes
  const int* start[2];        // the two indexes
  const float4* pts[2];
  const int* tsize;           // [2] their table sizes
  const float* pose;          // [n k][6]
  float r2;
  int k;                      // poses per listed lane
  loam_score_result* res;     // [n k]
  unsigned long long* work;   // (profiling, else nullptr) [2]: the map points and buckets read are added
};

// One workgroup per (listed lane, pose): row = blockIdx.x = i k + j.  It walks lane i's tiles in
// order, corner tiles first; thread 0 adds the tiles' partials as k_mp_score_reduce does (each
// cloud's sum from 0.0, in tile order) and writes the row itself: no partial array, no second
// launch.  The sums' order is k_mp_score's throughout (score_tile_eval), so a row has the bits
// loam_map_score gives the same clouds and pose.
__global__ __launch_bounds__(kScoreThreads) void k_lanes_score(LanesScoreArgs a) {
  const int tid = threadIdx.x;
  const uint32_t row = blockIdx.x;
  const LaneScorePlan pl = a.plan[row / (uint32_t)a.k];
  __shared__ double rot[6];
  __shared__ double wsum[2][kScoreWaves];
  __shared__ uint32_t wcnt[2][kScoreWaves][4];
  const float* T = a.pose + (size_t)row * 6;
  score_rot_eval(T, rot);
  __syncthreads();
  const loampose::MapRot R = score_rot_read(T, rot);
  loam_score_result o;
  o.corner_scored = o.surf_scored = o.corner_in = o.surf_in = 0;
  o.corner_cost = o.surf_cost = 0.0;
  unsigned long long cand = 0, cells = 0;
  for (int tile = 0; tile < pl.tiles; ++tile) {
    const int kind = tile < pl.tiles_c ? 0 : 1;
    const int n = kind ? pl.nS : pl.nC, base = (kind ? tile - pl.tiles_c : tile) * kScoreTile;
    const float4* q = a.last[kind] + (kind ? pl.offS : pl.offC);
    float4 p[kScorePer];
    bool use[kScorePer];
    score_tile_load(q, n, base, p, use);
    const ScoreMap m = {a.start[kind], a.pts[kind], a.tsize[kind]};
    const ScorePart t = score_tile_eval(p, use, m, R, a.r2, wsum[tile & 1], wcnt[tile & 1]);
    if (tid == 0) {
      if (kind == 0) {
        o.corner_scored += t.scored;
        o.corner_in += t.in;
        o.corner_cost += t.sum;
      } else {
        o.surf_scored += t.scored;
        o.surf_in += t.in;
        o.surf_cost += t.sum;
      }
      cand += t.cand;
      cells += t.cells;
    }
  }
  if (tid == 0) {
    a.res[row] = o;
    if (a.work) {  // (integer sums: any order)
      atomicAdd(&a.work[0], cand);
      atomicAdd(&a.work[1], cells);
    }
  }
}

// candidates [h0, h0 + nh): the tiles' partials added in tile order, corner tiles then surf tiles.
// work (profiling, else nullptr): the launch's map points and buckets read are added to it
// (integer sums: any order)
__global__ __launch_bounds__(256) void k_mp_score_reduce(const ScorePart* part, int tiles_c, int tiles, int h0, int nh,
                                                         loam_score_result* res, unsigned long long* work) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  unsigned long long cand = 0, cells = 0;
  if (j < nh) {
    const ScorePart* p = part + (size_t)j * tiles;
    loam_score_result o;
    o.corner_scored = o.surf_scored = o.corner_in = o.surf_in = 0;
    o.corner_cost = o.surf_cost = 0.0;
    for (int t = 0; t < tiles_c; ++t) {
      o.corner_scored += p[t].scored;
      o.corner_in += p[t].in;
      o.corner_cost += p[t].sum;
    }
    for (int t = tiles_c; t < tiles; ++t) {
      o.surf_scored += p[t].scored;
      o.surf_in += p[t].in;
      o.surf_cost += p[t].sum;
    }
    res[h0 + j] = o;
    for (int t = 0; t < tiles; ++t) {
      cand += p[t].cand;
      cells += p[t].cells;
    }
  }
  if (work) {  // (wave-uniform)
    cand = wave_sum(cand);
    cells = wave_sum(cells);
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&work[0], cand);
      atomicAdd(&work[1], cells);
    }
  }
}

template <class T>
hipError_t regrow(T** p, size_t bytes) {  // the old block is released first: nothing of it is kept
  if (*p) (void)hipFree(*p);
  *p = nullptr;
  return hipMalloc((void**)p, bytes ? bytes : 16);
}

}  // namespace

void mp_score_free(MpScore& S) {
  for (void* p : {(void*)S.q, (void*)S.pose, (void*)S.res, (void*)S.work, (void*)S.start, (void*)S.fill, (void*)S.out,
                  (void*)S.cnt, (void*)S.part})
    if (p) (void)hipFree(p);
  if (S.pin) (void)hipHostFree(S.pin);
  if (S.plan_pin) (void)hipHostFree(S.plan_pin);
  if (S.plan) (void)hipFree(S.plan);
  S = MpScore();
}

hipError_t mp_score_reserve(MpScore& S, int cloud_max) {
  hipError_t e = hipSuccess;
  if (!S.pin) {
    const size_t bytes = (size_t)kScoreMax * (6 * sizeof(float) + sizeof(loam_score_result)) + 2 * sizeof(unsigned long long);
    e = hipHostMalloc((void**)&S.pin, bytes, hipHostMallocDefault);
    if (e != hipSuccess) S.pin = nullptr;
  }
  if (e == hipSuccess && !S.pose) e = hipMalloc((void**)&S.pose, (size_t)kScoreMax * 6 * sizeof(float));
  if (e == hipSuccess && !S.res) e = hipMalloc((void**)&S.res, (size_t)kScoreMax * sizeof(loam_score_result));
  if (e == hipSuccess && !S.work) e = hipMalloc((void**)&S.work, 2 * sizeof(unsigned long long));
  if (e == hipSuccess && !S.cnt) e = hipMalloc((void**)&S.cnt, 4 * sizeof(int));
  if (e == hipSuccess && (cloud_max > S.cloud_cap || !S.q)) {
    const int cap = std::max(cloud_max, 1);
    S.cloud_cap = 0;
    e = regrow(&S.q, (size_t)2 * cap * sizeof(float4));
    if (e == hipSuccess) S.cloud_cap = cap;
  }
  return e;
}

namespace {
int score_table_size(int n) { return std::min(next_pow2(std::max(n, 64)), kScoreTMax); }
int score_tiles(int n) { return (n + kScoreTile - 1) / kScoreTile; }
// candidates of one launch: their partials fit kScorePartBytes
int score_chunk(int tiles, int n) {
  if (tiles == 0) return 0;
  return (int)std::max<size_t>(1, std::min<size_t>((size_t)n, kScorePartBytes / ((size_t)tiles * sizeof(ScorePart))));
}
}  // namespace

hipError_t mp_score_reserve_map(MpScore& S, int nC, int nS, int ncorner, int nsurf, int n) {
  hipError_t e = hipSuccess;
  const int tiles = score_tiles(ncorner) + score_tiles(nsurf);
  const size_t want = (size_t)score_chunk(tiles, n) * tiles;
  if (want > S.part_cap) {
    S.part_cap = 0;
    e = regrow(&S.part, want * sizeof(ScorePart));
    if (e != hipSuccess) return e;
    S.part_cap = want;
  }
  const int T = std::max(score_table_size(nC), score_table_size(nS));
  if (T > S.idx_T || !S.start || !S.fill) {
    S.idx_T = 0;
    e = regrow(&S.start, (size_t)2 * (T + 1) * sizeof(int));
    if (e == hipSuccess) e = regrow(&S.fill, (size_t)2 * T * sizeof(int));
    if (e == hipSuccess) S.idx_T = T;
  }
  if (e == hipSuccess && (nC + nS > S.idx_pts || !S.out)) {
    const int cap = std::max(nC + nS, 1);
    S.idx_pts = 0;
    e = regrow(&S.out, (size_t)cap * sizeof(float4));
    if (e == hipSuccess) S.idx_pts = cap;
  }
  return e;
}

hipError_t mp_score_index(MpScore& S, MpBuffers& s, MapIo& io, int nC, int total, hipStream_t st, Prof* prof,
                          ScoreIndex* idx) {
  const int nS = total - nC;
  if (nC < 0 || nS < 0 || total > S.idx_pts) return hipErrorInvalidValue;
  // the store in canonical order (corner points, then surf points), then both tables
  hipError_t e = mp_map_pack(s, io, total, st, prof);
  if (e != hipSuccess) return e;
  {
    const int cnt[2] = {nC, nS};
    Xfer xp;
    xp.put(S.cnt, cnt, sizeof(cnt));
    e = xfer_launch(xp, st);
    if (e != hipSuccess) return e;
  }
  HashJob hc;
  hc.pts = s.vin; hc.pts_stride = 0; hc.pts_off = nullptr; hc.pts_off_stride = 0;
  hc.count = S.cnt; hc.count_stride_bytes = 0;
  hc.start = S.start; hc.fill = S.fill; hc.out = S.out; hc.tsize = S.cnt + 2; hc.tmax = S.idx_T;
  hc.inv_h = 1.0f;
  hc.shift = 0;  // a bucket per point up to the table limit: the search scans whole buckets
  hc.chunks = nullptr;
  HashJob hs = hc;
  hs.pts = s.vin + nC; hs.count = S.cnt + 1;
  hs.start = S.start + (S.idx_T + 1); hs.fill = S.fill + S.idx_T; hs.out = S.out + nC; hs.tsize = S.cnt + 3;
  hash_build_pair(hc, hs, 1, st, false, HashForm::kGrid);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (prof) prof->mark("score_index");
  idx->start[0] = hc.start; idx->start[1] = hs.start;
  idx->pts[0] = hc.out; idx->pts[1] = hs.out;
  idx->tsize = S.cnt + 2;
  return hipSuccess;
}

hipError_t mp_score_run(MpScore& S, MpBuffers& s, MapIo& io, int nC, int total, int ncorner, int nsurf, float r2, int n,
                        bool count, hipStream_t st, Prof* prof) {
  auto mark = [&](const char* name) { if (prof) prof->mark(name); };
  if (n < 1 || n > kScoreMax || std::max(ncorner, nsurf) > S.cloud_cap) return hipErrorInvalidValue;
  ScoreIndex ix;
  hipError_t e = mp_score_index(S, s, io, nC, total, st, prof, &ix);
  if (e != hipSuccess) return e;
  if (count) {
    e = hipMemsetAsync(S.work, 0, 2 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
  }
  ScoreArgs a;
  a.q[0] = S.q; a.q[1] = S.q + S.cloud_cap;
  a.nq[0] = ncorner; a.nq[1] = nsurf;
  a.tiles_c = score_tiles(ncorner);
  a.tiles = a.tiles_c + score_tiles(nsurf);
  a.start[0] = ix.start[0]; a.start[1] = ix.start[1];
  a.pts[0] = ix.pts[0]; a.pts[1] = ix.pts[1];
  a.tsize = ix.tsize;
  a.pose = S.pose;
  a.r2 = r2;
  if (a.tiles == 0) {  // two empty clouds: every result is zero
    e = hipMemsetAsync(S.res, 0, (size_t)n * sizeof(loam_score_result), st);
  } else {
    // candidates in chunks whose partials fit kScorePartBytes (a candidate's sums do not depend on its chunk)
    const int chunk = score_chunk(a.tiles, n);
    if ((size_t)chunk * a.tiles > S.part_cap) return hipErrorInvalidValue;
    a.part = S.part;
    for (int h0 = 0; h0 < n && e == hipSuccess; h0 += chunk) {
      const int nh = std::min(chunk, n - h0);
      a.h0 = h0;
      hipLaunchKernelGGL(k_mp_score, dim3(nh, a.tiles), dim3(kScoreThreads), 0, st, a);
      mark("k_mp_score");
      hipLaunchKernelGGL(k_mp_score_reduce, dim3((nh + 255) / 256), dim3(256), 0, st, S.part, a.tiles_c, a.tiles, h0, nh,
                         S.res, count ? S.work : nullptr);
      mark("k_mp_score_reduce");
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess)
    e = hipMemcpyAsync(S.res_h(), S.res, (size_t)n * sizeof(loam_score_result), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && count)
    e = hipMemcpyAsync(S.work_h(), S.work, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
  mark("map_score_d2h");
  return e;
}

hipError_t mp_score_reserve_plan(MpScore& S, int lanes) {
  if (lanes <= S.plan_lanes && S.plan_pin && S.plan) return hipSuccess;
  if (S.plan_pin) (void)hipHostFree(S.plan_pin);
  if (S.plan) (void)hipFree(S.plan);
  S.plan_pin = nullptr;
  S.plan = nullptr;
  S.plan_lanes = 0;
  const size_t bytes = (size_t)lanes * (kOdBufs * 2 * sizeof(int) + sizeof(LaneScorePlan));
  hipError_t e = hipHostMalloc((void**)&S.plan_pin, bytes, hipHostMallocDefault);
  if (e != hipSuccess) {
    S.plan_pin = nullptr;
    return e;
  }
  e = hipMalloc((void**)&S.plan, (size_t)lanes * sizeof(LaneScorePlan));
  if (e != hipSuccess) {
    (void)hipHostFree(S.plan_pin);
    S.plan_pin = nullptr;
    S.plan = nullptr;
    return e;
  }
  S.plan_lanes = lanes;
  return hipSuccess;
}

hipError_t mp_lanes_score_run(MpScore& S, MpBuffers& s, MapIo& io, int nC, int total, const float4* lastC,
                              const float4* lastS, const LaneScoreShape& shape, int n, int k, float r2, bool count,
                              hipStream_t st, Prof* prof) {
  auto mark = [&](const char* name) { if (prof) prof->mark(name); };
  if (n < 1 || n > S.plan_lanes || k < 1 || (uint64_t)n * (uint64_t)k != shape.grid_x || shape.grid_x > (uint32_t)kScoreMax)
    return hipErrorInvalidValue;
  mark("lanes_score_host_wait");  // (the host's planning since the sizes came down)
  hipError_t e = hipMemcpyAsync(S.plan, S.plan_h(), (size_t)n * sizeof(LaneScorePlan), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  mark("lanes_score_h2d");
  ScoreIndex ix;
  e = mp_score_index(S, s, io, nC, total, st, prof, &ix);
  if (e != hipSuccess) return e;
  if (count) {
    e = hipMemsetAsync(S.work, 0, 2 * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
  }
  LanesScoreArgs a;
  a.last[0] = lastC; a.last[1] = lastS;
  a.plan = S.plan;
  a.start[0] = ix.start[0]; a.start[1] = ix.start[1];
  a.pts[0] = ix.pts[0]; a.pts[1] = ix.pts[1];
  a.tsize = ix.tsize;
  a.pose = S.pose;
  a.r2 = r2;
  a.k = k;
  a.res = S.res;
  a.work = count ? S.work : nullptr;
  hipLaunchKernelGGL(k_lanes_score, dim3(shape.grid_x), dim3(kScoreThreads), 0, st, a);
  mark("k_lanes_score");
  e = hipGetLastError();
  if (e == hipSuccess)
    e = hipMemcpyAsync(S.res_h(), S.res, (size_t)shape.grid_x * sizeof(loam_score_result), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && count)
    e = hipMemcpyAsync(S.work_h(), S.work, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st);
  mark("lanes_score_d2h");
  return e;
}

}  // namespace loam
