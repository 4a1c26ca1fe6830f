// Map export and import of a streaming store on gfx950 (mp.hpp: MapIo, the canonical order).
#include <algorithm>

#include "mp_dev.hpp"

namespace loam {

// Export: k_mp_map_table turns the slot table (in no
// particular order after recentring) into the canonical offsets, k_mp_map_pack gathers the pool
// into vin.  Import: per uploaded chunk the kept points are compacted in input order into vin with
// a 14-bit key each (k_mp_map_keep -> k_mp_map_tile_scan -> k_mp_map_compact); the kept points are
// then sorted stably by two 7-bit LSD passes with per-tile histograms (k_mp_map_hist ->
// k_mp_map_scan -> k_mp_map_scatter, the second pass moving the points into the idle pool) and
// k_mp_map_install writes that pool's slot table.  Every placement is a prefix sum over a fixed
// order (tile, wave, lane); atomics only count.  No workgroup waits for another.
namespace {

constexpr int kMapSortTile = 4096, kMapSortThreads = 256, kMapSortPer = kMapSortTile / kMapSortThreads;
constexpr int kMapDigits = 128;

struct MapPose {
  float v[12];  // aft, bef
  int cen[3];
};

template <int NT>
__global__ __launch_bounds__(NT) void k_mp_map_table(MpBuffers b, int* tab, int inst) {
  constexpr int N = kMapKeys, E = (N + NT - 1) / NT;
  const int tid = threadIdx.x;
  const int* slots = slot_table(b, b.pool_cur, inst);
  const int* ist = b.istate + (size_t)inst * kMpStateInts;
  const float* fst = b.state + (size_t)inst * kMpStateFloats;
  __shared__ int nn[N];
  __shared__ int scratch[NT / 64 + 1];
  for (int x = tid; x < N; x += NT) {
    const int kind = x / kCubeNum, s = x % kCubeNum;
    const int2 oc = load_pair(slots + s * 4 + 2 * kind);
    nn[x] = oc.y;
    tab[kMapTabSrc + x] = oc.x;
  }
  __syncthreads();
  const int x0 = tid * E, x1 = min(N, x0 + E);
  int sum = 0;
  for (int x = x0; x < x1; ++x) sum += nn[x];
  int run;
  int off = block_excl_scan<NT>(sum, scratch, run);
  for (int x = x0; x < x1; ++x) {
    const int c = nn[x];
    nn[x] = off;
    off += c;
  }
  __syncthreads();
  for (int x = tid; x < N; x += NT) tab[kMapTabOff + x] = nn[x];
  if (tid == 0) tab[kMapTabOff + N] = run;
  if (tid < 3) tab[kMapTabInfo + tid] = ist[kMiCenW + tid];
  if (tid == 3) tab[kMapTabInfo + 3] = ist[kMiErr];
  if (tid >= 64 && tid < 76) {
    const int k = tid - 64;
    tab[kMapTabInfo + 4 + k] = __float_as_int(fst[(k < 6 ? kMpAft : kMpBef - 6) + k]);
  }
}

// output point i of the canonical order: its key by binary search over the offsets (LDS), its
// source pool[src[key] + i - off[key]].  Four points per lane, all four loads before the stores.
// inst: the instance whose store is packed, into its own map_cap points of vin
__global__ __launch_bounds__(256) void k_mp_map_pack(MpBuffers b, const int* tab, int total, int inst) {
  constexpr int N = kMapKeys;
  __shared__ int off[N + 1];
  const int tid = threadIdx.x;
  for (int x = tid; x <= N; x += 256) off[x] = tab[kMapTabOff + x];
  __syncthreads();
  const float4* pool = b.pool + ((size_t)b.pool_cur * b.P + inst) * b.map_cap;
  const int* src = tab + kMapTabSrc;
  float4* dst = b.vin + (size_t)inst * b.map_cap;
  for (int base = blockIdx.x * 1024; base < total; base += gridDim.x * 1024) {
    // the source index of output point i (clamped: the lanes past the end load a valid point)
    auto locate = [&](int i) {
      i = min(i, total - 1);
      int lo = 0;  // the last key whose offset is <= i (an empty key never is): 14 fixed steps
#pragma unroll
      for (int step = 8192; step > 0; step >>= 1) {
        const int c = lo + step;
        if (c < N && off[c] <= i) lo = c;
      }
      return src[lo] + (i - off[lo]);
    };
    const int i0 = base + tid, i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
    const int a0 = locate(i0), a1 = locate(i1), a2 = locate(i2), a3 = locate(i3);
    const float4 v0 = pool[a0], v1 = pool[a1], v2 = pool[a2], v3 = pool[a3];
    if (i0 < total) dst[i0] = v0;
    if (i1 < total) dst[i1] = v1;
    if (i2 < total) dst[i2] = v2;
    if (i3 < total) dst[i3] = v3;
  }
}

// the key of an imported point (-1: left out).  The cube is k_mp_insert's (cube_of, :983-989);
// beyond 1e9 m a point is outside every grid whose centre index is within 2^24 (and the cube
// arithmetic stays inside the int range)
LOAM_D int map_key(const float4 a, int cW, int cH, int cD, int kind) {
  if (!(fabsf(a.x) < 1e9f && fabsf(a.y) < 1e9f && fabsf(a.z) < 1e9f)) return -1;  // (NaN, inf too)
  const int ci = cube_of(a.x, cW), cj = cube_of(a.y, cH), ck = cube_of(a.z, cD);
  const bool in = ci >= 0 && ci < kCubeW && cj >= 0 && cj < kCubeH && ck >= 0 && ck < kCubeD;
  return in ? kind * kCubeNum + cube_index(ci, cj, ck) : -1;
}

// ranks of the kept elements of a kMapBinTile-point tile in element order (element r * 256 + tid):
// wave ballots, then the (r, wave) counts prefixed in that order; sh: 17 ints
LOAM_D void map_tile_rank(const bool (&keep)[4], int (&rank)[4], int* sh, int& total) {
  const int w = threadIdx.x >> 6, lane = lane_id();
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const uint64_t m = __ballot(keep[r]);
    rank[r] = __popcll(m & lanemask_lt());
    if (lane == 0) sh[r * 4 + w] = __popcll(m);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int q = 0; q < 16; ++q) {
      const int c = sh[q];
      sh[q] = run;
      run += c;
    }
    sh[16] = run;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; ++r) rank[r] += sh[r * 4 + w];
  total = sh[16];
}

__global__ __launch_bounds__(256) void k_mp_map_keep(const float4* pts, int n, int kind, MapPose ps, int* tab) {
  static_assert(kMapBinTile == 4 * 256, "four points per thread");
  __shared__ int sh[17];
  const int base = blockIdx.x * kMapBinTile;
  bool keep[4];
  int rank[4], total;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = base + r * 256 + threadIdx.x;
    keep[r] = i < n && map_key(pts[i < n ? i : 0], ps.cen[0], ps.cen[1], ps.cen[2], kind) >= 0;
  }
  map_tile_rank(keep, rank, sh, total);
  if (threadIdx.x == 0) tab[kMapTabTile + blockIdx.x] = total;
}

// the chunk's tile counts -> their offsets in vin (behind the points kept so far); one workgroup
template <int NT>
__global__ __launch_bounds__(NT) void k_mp_map_tile_scan(int* tab, int ntiles, int n, int kind) {
  static_assert(2 * NT >= kMapChunkTiles, "two tiles per thread");
  __shared__ int scratch[NT / 64 + 1];
  const int t0 = 2 * threadIdx.x;
  int* tc = tab + kMapTabTile;
  const int c0 = t0 < ntiles ? tc[t0] : 0, c1 = t0 + 1 < ntiles ? tc[t0 + 1] : 0;
  int tot;
  const int ex = block_excl_scan<NT>(c0 + c1, scratch, tot);
  const int kept = tab[kMapTabAcc];
  if (t0 < ntiles) tc[t0] = kept + ex;
  if (t0 + 1 < ntiles) tc[t0 + 1] = kept + ex + c0;
  __syncthreads();  // (every thread has read the accumulator)
  if (threadIdx.x == 0) {
    // (saturating: an offset plus a chunk stays inside the int range; beyond map_cap nothing is stored)
    const long long k = (long long)kept + tot;
    tab[kMapTabAcc] = (int)(k < 0x7fffffffll - 2 * kMapChunkPts ? k : 0x7fffffffll - 2 * kMapChunkPts);
    tab[kMapTabAcc + 1 + kind] += n - tot;
  }
}

__global__ __launch_bounds__(256) void k_mp_map_compact(const float4* pts, int n, int kind, MapPose ps, const int* tab,
                                                        float4* out, uint16_t* keys, int* cnt, int cap) {
  __shared__ int sh[17];
  const int base = blockIdx.x * kMapBinTile;
  float4 v[4];
  int key[4];
  bool keep[4];
  int rank[4], total;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = base + r * 256 + threadIdx.x;
    v[r] = pts[i < n ? i : 0];
    key[r] = i < n ? map_key(v[r], ps.cen[0], ps.cen[1], ps.cen[2], kind) : -1;
    keep[r] = key[r] >= 0;
  }
  map_tile_rank(keep, rank, sh, total);
  const int o = tab[kMapTabTile + blockIdx.x];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int d = o + rank[r];
    if (keep[r] && d < cap) {
      out[d] = v[r];
      keys[d] = (uint16_t)key[r];
      atomicAdd(&cnt[key[r]], 1);  // (a count: the placement is the scans')
    }
  }
}

template <int PASS>
LOAM_D int map_digit(int key) { return PASS == 0 ? (key & (kMapDigits - 1)) : (key >> 7); }

// hist[digit][tile]: the tile's points with that digit
template <int PASS>
__global__ __launch_bounds__(kMapSortThreads) void k_mp_map_hist(const uint16_t* keys, int n, int* hist, int ntiles) {
  static_assert(kMapKeys <= kMapDigits * kMapDigits, "two 7-bit digits");
  __shared__ int h[kMapDigits];
  const int tid = threadIdx.x, tile = blockIdx.x;
  if (tid < kMapDigits) h[tid] = 0;
  __syncthreads();
  int k[kMapSortPer];
#pragma unroll
  for (int e = 0; e < kMapSortPer; ++e) {
    const int i = tile * kMapSortTile + e * kMapSortThreads + tid;
    k[e] = i < n ? (int)keys[i] : -1;
  }
#pragma unroll
  for (int e = 0; e < kMapSortPer; ++e)
    if (k[e] >= 0) atomicAdd(&h[map_digit<PASS>(k[e])], 1);
  __syncthreads();
  if (tid < kMapDigits) hist[(size_t)tid * ntiles + tile] = h[tid];
}

// in-place exclusive prefix of a[0 .. n): one workgroup, the block scan carried over the passes
template <int NT>
__global__ __launch_bounds__(NT) void k_mp_map_scan(int* a, int n) {
  __shared__ int scratch[NT / 64 + 1];
  int carry = 0;
  for (int base = 0; base < n; base += NT * 4) {
    const int i0 = base + 4 * threadIdx.x;
    int4 v = make_int4(0, 0, 0, 0);
    if (i0 + 3 < n) v = *reinterpret_cast<const int4*>(a + i0);
    else if (i0 < n) {
      v.x = a[i0];
      if (i0 + 1 < n) v.y = a[i0 + 1];
      if (i0 + 2 < n) v.z = a[i0 + 2];
    }
    int tot;
    const int ex = carry + block_excl_scan<NT>(v.x + v.y + v.z + v.w, scratch, tot);
    const int4 o = make_int4(ex, ex + v.x, ex + v.x + v.y, ex + v.x + v.y + v.z);
    if (i0 + 3 < n) *reinterpret_cast<int4*>(a + i0) = o;
    else if (i0 < n) {
      a[i0] = o.x;
      if (i0 + 1 < n) a[i0 + 1] = o.y;
      if (i0 + 2 < n) a[i0 + 2] = o.z;
    }
    carry += tot;
  }
}

// one LSD pass over a tile: wave w takes the tile's w-th quarter in order, 64 points a round; a
// point's place = the scanned hist[digit][tile] + the digit's points in the waves before + those
// before it in its own wave (the lanes of equal digit found by seven ballots).  Pass 0 writes
// (key, index), pass 1 moves the point itself.
template <int PASS>
__global__ __launch_bounds__(kMapSortThreads) void k_mp_map_scatter(const uint16_t* keys, const uint32_t* idx, int n,
                                                                    const int* hist, int ntiles, uint16_t* keys_out,
                                                                    uint32_t* idx_out, const float4* pts, float4* pts_out) {
  constexpr int NW = kMapSortThreads / 64, PER = kMapSortTile / NW, R = PER / 64;
  __shared__ int wcnt[NW][kMapDigits];
  const int tid = threadIdx.x, tile = blockIdx.x, w = tid >> 6, lane = lane_id();
  for (int i = tid; i < NW * kMapDigits; i += kMapSortThreads) wcnt[i / kMapDigits][i % kMapDigits] = 0;
  __syncthreads();
  const int i0 = tile * kMapSortTile + w * PER + lane;
  int k[R];
  uint32_t src[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = i0 + r * 64;
    k[r] = i < n ? (int)keys[i] : -1;
    src[r] = PASS == 0 ? (uint32_t)i : (i < n ? idx[i] : 0u);
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (k[r] >= 0) atomicAdd(&wcnt[w][map_digit<PASS>(k[r])], 1);
  __syncthreads();
  if (tid < kMapDigits) {
    int run = hist[(size_t)tid * ntiles + tile];
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) {
      const int c = wcnt[ww][tid];
      wcnt[ww][tid] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const bool ok = k[r] >= 0;
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // (pass 1: gathered here, used after the ballots)
    if constexpr (PASS == 1) v = pts[ok ? src[r] : 0u];
    const int d = ok ? map_digit<PASS>(k[r]) : 0;
    uint64_t peers = __ballot(ok);
#pragma unroll
    for (int bit = 0; bit < 7; ++bit) {
      const uint64_t m = __ballot(ok && ((d >> bit) & 1));
      peers &= ((d >> bit) & 1) ? m : ~m;
    }
    const int before = __popcll(peers & lanemask_lt());
    const int pos = ok ? wcnt[w][d] + before : 0;
    __builtin_amdgcn_wave_barrier();
    if (ok && before == 0) wcnt[w][d] += __popcll(peers);  // (the digit's first lane)
    __builtin_amdgcn_wave_barrier();
    if (ok) {
      if (PASS == 0) {
        keys_out[pos] = (uint16_t)k[r];
        idx_out[pos] = src[r];
      } else {
        pts_out[pos] = v;
      }
    }
  }
}

// the slot table of the sorted points: the exclusive prefix of the per-key counts, kind-major as the
// sort placed them, into nw ([kCubeNum][4]: offC, cntC, offS, cntS); every thread of the workgroup
template <int NT>
LOAM_D void map_slots_of(const int* cnt, int* nw) {
  constexpr int N = kMapKeys, E = (N + NT - 1) / NT;
  const int tid = threadIdx.x;
  __shared__ int nn[N];
  __shared__ int scratch[NT / 64 + 1];
  for (int x = tid; x < N; x += NT) nn[x] = cnt[x];
  __syncthreads();
  const int x0 = tid * E, x1 = min(N, x0 + E);
  int sum = 0;
  for (int x = x0; x < x1; ++x) sum += nn[x];
  int run;
  int off = block_excl_scan<NT>(sum, scratch, run);
  for (int x = x0; x < x1; ++x) {
    const int c = nn[x];
    nn[x] = off;
    off += c;
  }
  __syncthreads();
  for (int x = tid; x < N; x += NT) {
    const int kind = x / kCubeNum, s = x % kCubeNum;
    nw[s * 4 + 2 * kind] = nn[x];
    nw[s * 4 + 1 + 2 * kind] = (x + 1 < N ? nn[x + 1] : run) - nn[x];
  }
}

// the imported store's slot table, centre and poses (loam_map_import: instance 0, the idle pool)
template <int NT>
__global__ __launch_bounds__(NT) void k_mp_map_install(MpBuffers b, const int* cnt, MapPose ps) {
  const int tid = threadIdx.x;
  map_slots_of<NT>(cnt, slot_table(b, 1 - b.pool_cur, 0));
  if (tid < 3) b.istate[kMiCenW + tid] = ps.cen[tid];
  if (tid >= 64 && tid < 76) {
    const int k = tid - 64;
    b.state[(k < 6 ? kMpAft : kMpBef - 6) + k] = ps.v[k];
  }
}

// the same table on its own, for a caller that installs it elsewhere (loam_lanes_map_import)
template <int NT>
__global__ __launch_bounds__(NT) void k_mp_map_slots(const int* cnt, int* nw) {
  map_slots_of<NT>(cnt, nw);
}

}  // namespace

hipError_t mp_map_ensure(MapIo& io) {
  if (io.tab && io.tab_h) return hipSuccess;
  mp_map_free(io);
  hipError_t e = hipMalloc((void**)&io.tab, (size_t)kMapTabInts * sizeof(int));
  if (e == hipSuccess) e = hipHostMalloc((void**)&io.tab_h, (size_t)kMapTabHead * sizeof(int), hipHostMallocDefault);
  if (e != hipSuccess) mp_map_free(io);
  return e;
}

void mp_map_free(MapIo& io) {
  if (io.tab) (void)hipFree(io.tab);
  if (io.tab_h) (void)hipHostFree(io.tab_h);
  io.tab = io.tab_h = nullptr;
}

hipError_t mp_map_table(MpBuffers& b, MapIo& io, hipStream_t st, Prof* prof, int inst) {
  if (inst < 0 || inst >= b.P) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_mp_map_table<1024>, dim3(1), dim3(1024), 0, st, b, io.tab, inst);
  if (prof) prof->mark("k_mp_map_table");
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    e = hipMemcpyAsync(io.tab_h, io.tab, (size_t)kMapTabHead * sizeof(int), hipMemcpyDeviceToHost, st);
  if (prof) prof->mark("map_export_table_d2h");
  return e;
}

hipError_t mp_map_pack(MpBuffers& b, MapIo& io, int total, hipStream_t st, Prof* prof, int inst) {
  if (total <= 0) return hipSuccess;
  if (total > b.map_cap || inst < 0 || inst >= b.P) return hipErrorInvalidValue;  // (vin holds map_cap points per instance)
  const int grid = std::min((total + 1023) / 1024, 2048);
  hipLaunchKernelGGL(k_mp_map_pack, dim3(grid), dim3(256), 0, st, b, io.tab, total, inst);
  if (prof) prof->mark("k_mp_map_pack");
  return hipGetLastError();
}

hipError_t mp_map_bin_begin(MpBuffers& b, MapIo& io, hipStream_t st) {
  hipError_t e = hipMemsetAsync(io.tab + kMapTabAcc, 0, 8 * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(b.app_cnt, 0, (size_t)kMapKeys * sizeof(int), st);
  return e;
}

namespace {
MapPose map_pose(const int* cen, const float* pose12) {
  MapPose ps;
  for (int k = 0; k < 12; ++k) ps.v[k] = pose12 ? pose12[k] : 0.0f;
  for (int k = 0; k < 3; ++k) ps.cen[k] = cen[k];
  return ps;
}
}  // namespace

hipError_t mp_map_bin_chunk(MpBuffers& b, MapIo& io, const float4* pts, int n, int kind, const int* cen,
                            hipStream_t st, Prof* prof) {
  if (n <= 0) return hipSuccess;
  if (n > kMapChunkPts) return hipErrorInvalidValue;
  const MapPose ps = map_pose(cen, nullptr);
  const int ntiles = (n + kMapBinTile - 1) / kMapBinTile;
  hipLaunchKernelGGL(k_mp_map_keep, dim3(ntiles), dim3(256), 0, st, pts, n, kind, ps, io.tab);
  if (prof) prof->mark("k_mp_map_keep");
  hipLaunchKernelGGL(k_mp_map_tile_scan<1024>, dim3(1), dim3(1024), 0, st, io.tab, ntiles, n, kind);
  if (prof) prof->mark("k_mp_map_tile_scan");
  hipLaunchKernelGGL(k_mp_map_compact, dim3(ntiles), dim3(256), 0, st, pts, n, kind, ps, io.tab, b.vin,
                     (uint16_t*)b.vg.keys, b.app_cnt, b.map_cap);
  if (prof) prof->mark("k_mp_map_compact");
  return hipGetLastError();
}

hipError_t mp_map_bin_result(MapIo& io, hipStream_t st) {
  return hipMemcpyAsync(io.tab_h + kMapTabAcc, io.tab + kMapTabAcc, 8 * sizeof(int), hipMemcpyDeviceToHost, st);
}

hipError_t mp_map_sort(MpBuffers& b, int kept, float4* dst, hipStream_t st, Prof* prof) {
  if (kept < 0 || kept > b.map_cap) return hipErrorInvalidValue;
  const int ntiles = (kept + kMapSortTile - 1) / kMapSortTile;
  // the histograms live in vg.vals_alt (max(map_cap, cap_stack) words, mp_alloc): 128 per 4096 points
  const size_t words = std::max((size_t)b.P * b.map_cap, (size_t)b.P * b.cap_stack);
  if ((size_t)ntiles * kMapDigits > words) return hipErrorInvalidValue;
  if (kept == 0) return hipSuccess;
  uint16_t *k0 = (uint16_t*)b.vg.keys, *k1 = (uint16_t*)b.vg.keys_alt;
  int* hist = (int*)b.vg.vals_alt;
  hipLaunchKernelGGL(k_mp_map_hist<0>, dim3(ntiles), dim3(kMapSortThreads), 0, st, k0, kept, hist, ntiles);
  if (prof) prof->mark("k_mp_map_hist");
  hipLaunchKernelGGL(k_mp_map_scan<1024>, dim3(1), dim3(1024), 0, st, hist, ntiles * kMapDigits);
  if (prof) prof->mark("k_mp_map_scan");
  hipLaunchKernelGGL(k_mp_map_scatter<0>, dim3(ntiles), dim3(kMapSortThreads), 0, st, k0, (const uint32_t*)nullptr,
                     kept, hist, ntiles, k1, b.vg.vals, (const float4*)nullptr, (float4*)nullptr);
  if (prof) prof->mark("k_mp_map_scatter");
  hipLaunchKernelGGL(k_mp_map_hist<1>, dim3(ntiles), dim3(kMapSortThreads), 0, st, k1, kept, hist, ntiles);
  if (prof) prof->mark("k_mp_map_hist");
  hipLaunchKernelGGL(k_mp_map_scan<1024>, dim3(1), dim3(1024), 0, st, hist, ntiles * kMapDigits);
  if (prof) prof->mark("k_mp_map_scan");
  hipLaunchKernelGGL(k_mp_map_scatter<1>, dim3(ntiles), dim3(kMapSortThreads), 0, st, k1, b.vg.vals, kept, hist, ntiles,
                     (uint16_t*)nullptr, (uint32_t*)nullptr, b.vin, dst);
  if (prof) prof->mark("k_mp_map_scatter");
  return hipGetLastError();
}

hipError_t mp_map_install(MpBuffers& b, MapIo& io, int kept, const int* cen, const float* pose12, hipStream_t st,
                          Prof* prof) {
  hipError_t e = mp_map_sort(b, kept, mp_map_idle_pool(b), st, prof);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mp_map_install<1024>, dim3(1), dim3(1024), 0, st, b, b.app_cnt, map_pose(cen, pose12));
  if (prof) prof->mark("k_mp_map_install");
  e = hipGetLastError();
  if (e == hipSuccess) b.pool_cur = 1 - b.pool_cur;
  return e;
}

hipError_t mp_map_slots(MpBuffers& b, MapIo& io, hipStream_t st, Prof* prof) {
  hipLaunchKernelGGL(k_mp_map_slots<1024>, dim3(1), dim3(1024), 0, st, b.app_cnt, io.tab + kMapTabSlots);
  if (prof) prof->mark("k_mp_map_slots");
  return hipGetLastError();
}

}  // namespace loam
