// Segmented PCL VoxelGrid on gfx950 (vg.hpp), used by laser mapping (mp.hip) for the stacks
// (src/laserMapping.cpp:693-701), the valid cubes (:1018-1036) and the surround map
// (:1042-1047), and by the diagnostic hook at the end of this file (dev_hooks.h).
//
//  k_vg_radix      fused LDS kernel: bbox, voxel keys, stable radix sort, per-voxel means (2048 / 12288 points)
//  k_vg_idx        the same with 8 bytes of LDS per point (16384 points)
//  k_vg_big        segments of any size through global memory
//  k_vg_split / k_vg_join   big segments as 16 key-range sub-segments through the LDS kernels
//  k_vg_merge      incremental VoxelGrid of a cube segment (old output ++ short tail)
//  vg_run          the cascade of those by segment size
//  vg_route_*      which cascade the stacks, the cubes and the surround map take
//  vg_scratch_*    the cascade's device memory (VgScratch)

#include <algorithm>
#include <vector>

#include "dev_common.hpp"
#include "dev_hooks.h"
#include "engine.hpp"
#include "vg.hpp"

using namespace loamdev;

namespace loam {
namespace {

// ---------------------------------------------------------------- segmented VoxelGrid
// PCL VoxelGrid over many segments at once: stacks (2 per instance), valid cubes (2 x
// 125 per instance), the surround map (1).  Per segment: bbox, voxel keys, a stable sort of
// (voxel, position) — the order of PCL's std::sort on (index, point) pairs with equal voxels in
// input order — and one output point per voxel, the float mean of x, y, z, intensity summed in
// sorted order.  vg_run cascades three hand-written kernels by segment size; no library sort.

// The segment's voxel frame (PCL VoxelGrid: bbox over its points, min_b = floor(min / leaf), the
// divb multipliers), or the one the job supplies (j.frame: a split parent's); false when the leaf is
// "too small" for the bbox (PCL then outputs the input unchanged; a supplied frame never is)
template <int NT>
__device__ __forceinline__ bool vg_frame_of(const VgJob& j, int s, const float4* in, int n, float inv, VgFrame& fr) {
  if (j.frame) {
    fr = j.frame[s];
    return true;
  }
  const int tid = threadIdx.x;
  float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f}, mx[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
  for (int i = tid; i < n; i += NT) {
    const float4 a = in[i];
    mn[0] = fminf(mn[0], a.x); mn[1] = fminf(mn[1], a.y); mn[2] = fminf(mn[2], a.z);
    mx[0] = fmaxf(mx[0], a.x); mx[1] = fmaxf(mx[1], a.y); mx[2] = fmaxf(mx[2], a.z);
  }
  block_bbox<NT>(mn, mx);
  if (vg_leaf_too_small(mn, mx, inv)) return false;
  fr.m0 = (int)floorf(mn[0] * inv);
  fr.m1 = (int)floorf(mn[1] * inv);
  fr.m2 = (int)floorf(mn[2] * inv);
  fr.divx = (int)floorf(mx[0] * inv) - fr.m0 + 1;
  fr.divy = (int)floorf(mx[1] * inv) - fr.m1 + 1;
  fr.pad = (int)floorf(mx[2] * inv) - fr.m2 + 1;  // (divz: the split's key range)
  return true;
}

// Fused segmented VoxelGrid with an LDS radix sort: one workgroup per segment of at most NT*E
// points does the bbox, the voxel keys, a stable radix sort of (voxel, position) pairs over the
// bits the keys can differ in, and the ordered per-voxel means.  Segments beyond NT*E are appended
// to the job's big list.
template <int NT, int E, int TAG = 0>  // TAG: which VoxelGrid job (vg_run), a distinct symbol for rocprof
__global__ __launch_bounds__(NT) void k_vg_radix(VgJob j) {
  constexpr int N = NT * E;
  __shared__ uint32_t ka[N], kb[N];
  __shared__ uint16_t va[N], vb[N];
  __shared__ uint32_t sc[(NT / 64 + 1) * 8];
  __shared__ int isc[24];
  const int tid = threadIdx.x;
  const int nl = j.list ? *j.list_n : j.nseg;
  for (int li = blockIdx.x; li < nl; li += gridDim.x) {
    const int s = j.list ? j.list[li] : li;
    if (j.skip && j.skip[s]) continue;  // (written by k_vg_merge; only the cascade's first kernel sees it)
    const int b0 = j.begin[s], b1 = j.end[s], n = b1 - b0;
    if (n <= 0) {
      if (tid == 0) j.out_count[s] = 0;
      continue;
    }
    if (n > N) {
      if (tid == 0) j.big[atomicAdd(j.big_n, 1)] = s;
      continue;
    }
    const float4* in = j.in + b0;
    const float inv = 1.0f / j.leaf[s];
    VgFrame fr;
    if (!vg_frame_of<NT>(j, s, in, n, inv, fr)) {  // "leaf size too small": output = input
      for (int i = tid; i < n; i += NT) j.out[b0 + i] = in[i];
      if (tid == 0) j.out_count[s] = n;
      continue;
    }
    const int m0 = fr.m0, m1 = fr.m1, m2 = fr.m2;
    const uint32_t mul1 = (uint32_t)fr.divx, mul2 = (uint32_t)(fr.divx * fr.divy);
    uint32_t kmax = 0;
    for (int i = tid; i < n; i += NT) {
      const float4 a = in[i];
      const int i0 = (int)(floorf(a.x * inv) - (float)m0);
      const int i1 = (int)(floorf(a.y * inv) - (float)m1);
      const int i2 = (int)(floorf(a.z * inv) - (float)m2);
      const uint32_t key = (uint32_t)i0 + (uint32_t)i1 * mul1 + (uint32_t)i2 * mul2;
      ka[i] = key;
      va[i] = (uint16_t)i;
      kmax = key > kmax ? key : kmax;
    }
    kmax = block_max_u32<NT>(kmax >> 1);
    const int nbits = kmax ? 33 - __clz((int)kmax) : (n > 1 ? 1 : 0);  // bits of the max key
    const int cur = block_radix_sort_kv<NT, E>(ka, va, kb, vb, n, nbits, sc);
    const uint32_t* ks = cur ? kb : ka;
    const uint16_t* vs = cur ? vb : va;
    // ordered per-voxel means in one pass: thread t owns sorted positions [t E, t E + E); its E
    // members are gathered at once, each run that starts in the range is summed from its head in
    // sorted order (a run reaching past the range reads on from global memory), and the runs'
    // output slots come from one block scan of the heads per thread
    {
      const int i0 = tid * E;
      uint32_t kk[E];
      float4 a[E];
      int nh = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = i0 + e;
        kk[e] = i < n ? ks[i] : 0u;
        a[e] = i < n ? in[vs[i]] : make_float4(0, 0, 0, 0);
        nh += (i < n && (i == 0 || ks[i - 1] != kk[e])) ? 1 : 0;
      }
      int tot;
      int slot = block_excl_scan<NT>(nh, isc, tot);
      bool open = false;
      uint32_t ck = 0;
      int cstart = 0;
      float sx = 0, sy = 0, sz = 0, si = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = i0 + e;
        if (i < n) {
          const bool head = i == 0 || (e > 0 ? kk[e - 1] != kk[e] : ks[i - 1] != kk[e]);
          if (head) {
            if (open) {
              const float cnt = (float)(i - cstart);
              j.out[b0 + slot++] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
            }
            open = true;
            ck = kk[e];
            cstart = i;
            sx = 0; sy = 0; sz = 0; si = 0;
          }
          if (open) { sx += a[e].x; sy += a[e].y; sz += a[e].z; si += a[e].w; }
        }
      }
      if (open) {
        int m = min(i0 + E, n);  // (the range may end past the segment)
        while (m < n && ks[m] == ck) {
          const float4 b4 = in[vs[m]];
          sx += b4.x; sy += b4.y; sz += b4.z; si += b4.w;
          ++m;
        }
        const float cnt = (float)(m - cstart);
        j.out[b0 + slot] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
      }
      if (tid == 0) j.out_count[s] = tot;
    }
    __syncthreads();  // the LDS arrays are reused by the next segment
  }
}

// The same for segments of up to NT*E = 16384 points with 8 bytes of LDS per point: the voxel
// keys stay in input order (ka[i] = key of point i) and only the 16-bit positions move between
// the two buffers, each radix pass reading its digits through them (tile_rank4 over the whole
// segment); the long surf stacks of VLP-16 sweeps fit it.
// one segment of k_vg_idx with E positions per thread (blocked: thread t owns positions [t E, t E + E)).
// (Round 4: choosing E = 4 / 8 / 16 by segment size, so that a 5k-point stack keeps 625 threads busy
// instead of 313, measured equal at batch 128 and 1024.)
template <int NT, int E>
__device__ __forceinline__ void vg_idx_segment(const VgJob& j, int s, int b0, int n, uint32_t* ka, uint16_t* va, uint16_t* vb,
                           uint32_t* sc, uint32_t* dtot, uint32_t* dbase, float* fsc, int* isc) {
  const int tid = threadIdx.x;
    const float4* in = j.in + b0;
    const float inv = 1.0f / j.leaf[s];
    VgFrame fr;
    if (!vg_frame_of<NT>(j, s, in, n, inv, fr)) {  // "leaf size too small": output = input
      for (int i = tid; i < n; i += NT) j.out[b0 + i] = in[i];
      if (tid == 0) j.out_count[s] = n;
      return;
    }
    const int m0 = fr.m0, m1 = fr.m1, m2 = fr.m2;
    const uint32_t mul1 = (uint32_t)fr.divx, mul2 = (uint32_t)(fr.divx * fr.divy);
    uint32_t kmax = 0;
    for (int i = tid; i < n; i += NT) {
      const float4 a = in[i];
      const int i0 = (int)(floorf(a.x * inv) - (float)m0);
      const int i1 = (int)(floorf(a.y * inv) - (float)m1);
      const int i2 = (int)(floorf(a.z * inv) - (float)m2);
      const uint32_t key = (uint32_t)i0 + (uint32_t)i1 * mul1 + (uint32_t)i2 * mul2;
      ka[i] = key;
      va[i] = (uint16_t)i;
      kmax = key > kmax ? key : kmax;
    }
    kmax = block_max_u32<NT>(kmax >> 1);
    const int nbits = kmax ? 33 - __clz((int)kmax) : (n > 1 ? 1 : 0);
    int cur = 0;
    for (int shift = 0; shift < nbits; shift += 4) {
      const uint16_t* vs = cur ? vb : va;
      uint16_t* vd = cur ? va : vb;
      uint32_t k[E];
      uint16_t v[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = tid * E + e;
        v[e] = i < n ? vs[i] : (uint16_t)0;
        k[e] = i < n ? ka[v[e]] : 0u;
      }
      int rank[E];
      tile_rank4<NT, E>(k, shift, n, sc, dtot, rank);
      if (tid == 0) {
        uint32_t r = 0;
        for (int d = 0; d < 16; ++d) { dbase[d] = r; r += dtot[d]; }
      }
      __syncthreads();
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (rank[e] >= 0) vd[dbase[(k[e] >> shift) & 15u] + rank[e]] = v[e];
      __syncthreads();
      cur ^= 1;
    }
    const uint16_t* vs = cur ? vb : va;
    // ordered per-voxel means (as k_vg_radix): thread t owns sorted positions [t E, t E + E),
    // gathered eight at a time
    {
      const int i0 = tid * E;
      int nh = 0;
      uint32_t prev = i0 > 0 && i0 < n ? ka[vs[i0 - 1]] : 0u;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = i0 + e;
        const uint32_t kc = i < n ? ka[vs[i]] : 0u;
        nh += (i < n && (i == 0 || prev != kc)) ? 1 : 0;
        prev = kc;
      }
      int tot;
      int slot = block_excl_scan<NT>(nh, isc, tot);
      bool open = false;
      uint32_t ck = 0;
      int cstart = 0;
      float sx = 0, sy = 0, sz = 0, si = 0;
      prev = i0 > 0 && i0 < n ? ka[vs[i0 - 1]] : 0u;
      constexpr int G = E < 8 ? E : 8;  // gathers in flight (the thread's E positions only)
#pragma unroll
      for (int e0 = 0; e0 < E; e0 += G) {
        float4 a[G];
        uint32_t kk[G];
#pragma unroll
        for (int u = 0; u < G; ++u) {
          const int i = i0 + e0 + u;
          kk[u] = i < n ? ka[vs[i]] : 0u;
          a[u] = i < n ? in[vs[i]] : make_float4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < G; ++u) {
          const int i = i0 + e0 + u;
          if (i < n) {
            if (i == 0 || prev != kk[u]) {
              if (open) {
                const float cnt = (float)(i - cstart);
                j.out[b0 + slot++] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
              }
              open = true;
              ck = kk[u];
              cstart = i;
              sx = 0; sy = 0; sz = 0; si = 0;
            }
            if (open) { sx += a[u].x; sy += a[u].y; sz += a[u].z; si += a[u].w; }
            prev = kk[u];
          }
        }
      }
      if (open) {
        int m = min(i0 + E, n);
        while (m < n && ka[vs[m]] == ck) {
          const float4 b4 = in[vs[m]];
          sx += b4.x; sy += b4.y; sz += b4.z; si += b4.w;
          ++m;
        }
        const float cnt = (float)(m - cstart);
        j.out[b0 + slot] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
      }
      if (tid == 0) j.out_count[s] = tot;
    }
}

template <int NT, int E, int TAG = 0>  // TAG: which VoxelGrid job (vg_run), a distinct symbol for rocprof
__global__ __launch_bounds__(NT) void k_vg_idx(VgJob j) {
  constexpr int N = NT * E;
  static_assert(N <= 65536, "16-bit positions");
  __shared__ uint32_t ka[N];
  __shared__ uint16_t va[N], vb[N];
  __shared__ uint32_t sc[(NT / 64 + 1) * 8];
  __shared__ uint32_t dtot[16], dbase[16];
  __shared__ float fsc[16];
  __shared__ int isc[24];
  const int tid = threadIdx.x;
  const int nl = j.list ? *j.list_n : j.nseg;
  for (int li = blockIdx.x; li < nl; li += gridDim.x) {
    const int s = j.list ? j.list[li] : li;
    const int b0 = j.begin[s], b1 = j.end[s], n = b1 - b0;
    if (n <= 0) {
      if (tid == 0) j.out_count[s] = 0;
      continue;
    }
    if (n > N) {
      if (tid == 0) j.big[atomicAdd(j.big_n, 1)] = s;
      continue;
    }
    vg_idx_segment<NT, E>(j, s, b0, n, ka, va, vb, sc, dtot, dbase, fsc, isc);
    __syncthreads();
  }
}

// Segments of any size (those beyond the LDS kernels), one workgroup each, taken from the job's list:
// bbox, voxel keys into the global key array (with the digit histograms of every pass), a stable
// LSD radix sort of (voxel, position) over the key bits through global memory — 4-bit digits, tiles
// of NT*E items ranked in registers (tile_rank4), digit bases carried from tile to tile — and the
// ordered per-voxel means over the sorted arrays.  Rare in VLP-16 batches (long surf stacks); the
// HDL-64E stack and a large surround map take it.
template <int NT, int E, int TAG = 0>  // TAG: which VoxelGrid job (vg_run), a distinct symbol for rocprof
__global__ __launch_bounds__(NT) void k_vg_big(VgJob j) {
  constexpr int TILE = NT * E;
  __shared__ uint32_t hist[8][16];
  __shared__ uint32_t dbase[16], ttot[16];
  __shared__ uint32_t sc[(NT / 64 + 1) * 8];
  __shared__ int isc[24];
  const int tid = threadIdx.x;
  const int nl = *j.list_n;
  for (int li = blockIdx.x; li < nl; li += gridDim.x) {
    const int s = j.list[li];
    const int b0 = j.begin[s], n = j.end[s] - b0;
    const float4* in = j.in + b0;
    const float inv = 1.0f / j.leaf[s];
    VgFrame fr;
    if (!vg_frame_of<NT>(j, s, in, n, inv, fr)) {  // "leaf size too small": output = input
      for (int i = tid; i < n; i += NT) j.out[b0 + i] = in[i];
      if (tid == 0) j.out_count[s] = n;
      __syncthreads();
      continue;
    }
    const int m0 = fr.m0, m1 = fr.m1, m2 = fr.m2;
    const uint32_t mul1 = (uint32_t)fr.divx, mul2 = (uint32_t)(fr.divx * fr.divy);
    for (int i = tid; i < 8 * 16; i += NT) (&hist[0][0])[i] = 0;
    __syncthreads();
    uint32_t* K = j.keys + b0;
    uint32_t* V = j.vals + b0;
    uint32_t* K2 = j.keys_alt + b0;
    uint32_t* V2 = j.vals_alt + b0;
    uint32_t kmax = 0;
    for (int i = tid; i < n; i += NT) {
      const float4 a = in[i];
      const int i0 = (int)(floorf(a.x * inv) - (float)m0);
      const int i1 = (int)(floorf(a.y * inv) - (float)m1);
      const int i2 = (int)(floorf(a.z * inv) - (float)m2);
      const uint32_t key = (uint32_t)i0 + (uint32_t)i1 * mul1 + (uint32_t)i2 * mul2;
      K[i] = key;
      V[i] = (uint32_t)i;
      kmax = key > kmax ? key : kmax;
#pragma unroll
      for (int p = 0; p < 8; ++p) atomicAdd(&hist[p][(key >> (4 * p)) & 15u], 1u);
    }
    kmax = block_max_u32<NT>(kmax >> 1);
    const int nbits = kmax ? 33 - __clz((int)kmax) : (n > 1 ? 1 : 0);
    int cur = 0;  // 0: the data is in (K, V)
    for (int pass = 0; pass * 4 < nbits; ++pass) {
      const uint32_t* ks = cur ? K2 : K;
      const uint32_t* vs = cur ? V2 : V;
      uint32_t* kd = cur ? K : K2;
      uint32_t* vd = cur ? V : V2;
      if (tid == 0) {
        uint32_t r = 0;
        for (int d = 0; d < 16; ++d) { dbase[d] = r; r += hist[pass][d]; }
      }
      __syncthreads();
      for (int t0 = 0; t0 < n; t0 += TILE) {
        const int nt = min(TILE, n - t0);
        uint32_t k[E], v[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
          const int i = tid * E + e;
          k[e] = i < nt ? ks[t0 + i] : 0u;
          v[e] = i < nt ? vs[t0 + i] : 0u;
        }
        int rank[E];
        tile_rank4<NT, E>(k, 4 * pass, nt, sc, ttot, rank);
#pragma unroll
        for (int e = 0; e < E; ++e)
          if (rank[e] >= 0) {
            const int pos = (int)dbase[(k[e] >> (4 * pass)) & 15u] + rank[e];
            kd[pos] = k[e];
            vd[pos] = v[e];
          }
        __syncthreads();
        if (tid < 16) dbase[tid] += ttot[tid];
        __syncthreads();
      }
      cur ^= 1;
    }
    const uint32_t* ks = cur ? K2 : K;
    const uint32_t* vs = cur ? V2 : V;
    // ordered per-voxel means, tile by tile: thread t's E sorted positions, heads counted by one
    // block scan per tile; each head sums its run in sorted order, reading on past its range
    int outn = 0;
    for (int t0 = 0; t0 < n; t0 += TILE) {
      const int i0 = t0 + tid * E;
      uint32_t kk[E];
      int nh = 0;
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = i0 + e;
        kk[e] = i < n ? ks[i] : 0u;
        nh += (i < n && (i == 0 || (e > 0 ? kk[e - 1] : ks[i - 1]) != kk[e])) ? 1 : 0;
      }
      int tot;
      int slot = outn + block_excl_scan<NT>(nh, isc, tot);
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = i0 + e;
        if (i < n && (i == 0 || (e > 0 ? kk[e - 1] : ks[i - 1]) != kk[e])) {
          float sx = 0, sy = 0, sz = 0, si = 0;
          int m = i;
          while (m < n && ks[m] == kk[e]) {
            const float4 b4 = in[vs[m]];
            sx += b4.x; sy += b4.y; sz += b4.z; si += b4.w;
            ++m;
          }
          const float cnt = (float)(m - i);
          j.out[b0 + slot++] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
        }
      }
      outn += tot;
    }
    if (tid == 0) j.out_count[s] = outn;
    __syncthreads();
  }
}

// The big-segment split (VgSplit, the HDL-64E surf stacks): one workgroup per parent of the job's
// big list computes the parent's frame (vg_frame_of), its voxel keys' top 4 bits (of the bit range
// the frame allows) as a bucket, the bucket sizes, and re-orders the points stably into the buckets
// (tiles ranked in registers by tile_rank4, as k_vg_big's passes): bucket d of parent li becomes
// sub-segment li * 16 + d in the parent's frame.  Equal keys share a bucket and buckets are key
// ranges in order, so the sub-segments' VoxelGrid outputs in bucket order are the parent's output,
// each voxel summed over the same points in the same (input) order.  A parent whose leaf is "too
// small" is copied to its output here (PCL) and gets empty sub-segments; list slots beyond the
// job's big list too.
template <int NT, int E>
__global__ __launch_bounds__(NT) void k_vg_split(VgJob j, VgSplit x) {
  constexpr int TILE = NT * E;
  __shared__ uint32_t sc[(NT / 64 + 1) * 8];
  __shared__ uint32_t hist[16], dbase[16], ttot[16];
  const int tid = threadIdx.x;
  const int nl = min(*j.list_n, x.npar);
  for (int li = blockIdx.x; li < nl; li += gridDim.x) {
    int* sb = x.begin + (size_t)li * 16;
    int* se = x.end + (size_t)li * 16;
    const int s = j.list[li];
    const int b0 = j.begin[s], n = j.end[s] - b0;
    const float4* in = j.in + b0;
    const float inv = 1.0f / j.leaf[s];
    // the parent's frame (vg_frame_of's, with four loads in flight per thread)
    VgFrame fr;
    {
      float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f}, mx[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
      for (int i0 = tid; i0 < n; i0 += 4 * NT) {
        float4 a[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) a[u] = in[min(i0 + u * NT, n - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          mn[0] = fminf(mn[0], a[u].x); mn[1] = fminf(mn[1], a[u].y); mn[2] = fminf(mn[2], a[u].z);
          mx[0] = fmaxf(mx[0], a[u].x); mx[1] = fmaxf(mx[1], a[u].y); mx[2] = fmaxf(mx[2], a[u].z);
        }
      }
      block_bbox<NT>(mn, mx);
      if (vg_leaf_too_small(mn, mx, inv)) {  // "leaf size too small": output = input
        for (int i = tid; i < n; i += NT) j.out[b0 + i] = in[i];
        if (tid == 0) j.out_count[s] = n;
        if (tid < 16) { sb[tid] = 0; se[tid] = 0; }
        __syncthreads();
        continue;
      }
      fr.m0 = (int)floorf(mn[0] * inv);
      fr.m1 = (int)floorf(mn[1] * inv);
      fr.m2 = (int)floorf(mn[2] * inv);
      fr.divx = (int)floorf(mx[0] * inv) - fr.m0 + 1;
      fr.divy = (int)floorf(mx[1] * inv) - fr.m1 + 1;
      fr.pad = (int)floorf(mx[2] * inv) - fr.m2 + 1;
    }
    const uint32_t mul1 = (uint32_t)fr.divx, mul2 = (uint32_t)(fr.divx * fr.divy);
    // the key range the frame allows (keys are uint32: a wider range buckets the wrapped keys by
    // their top bits, still a monotone bucket of the sorted key)
    const uint64_t kmax = (uint64_t)(fr.divx - 1) + (uint64_t)(fr.divy - 1) * (uint64_t)fr.divx +
                          (uint64_t)(fr.pad - 1) * (uint64_t)fr.divx * (uint64_t)fr.divy;
    const uint32_t km = kmax > 0xffffffffull ? 0xffffffffu : (uint32_t)kmax;
    const int bits = km ? 32 - __builtin_clz(km) : 0;
    const int shift = bits > 4 ? bits - 4 : 0;
    auto key_of = [&](const float4& a) {
      const int i0 = (int)(floorf(a.x * inv) - (float)fr.m0);
      const int i1 = (int)(floorf(a.y * inv) - (float)fr.m1);
      const int i2 = (int)(floorf(a.z * inv) - (float)fr.m2);
      return (uint32_t)i0 + (uint32_t)i1 * mul1 + (uint32_t)i2 * mul2;
    };
    if (tid < 16) hist[tid] = 0;
    __syncthreads();
    for (int i0 = tid; i0 < n; i0 += 4 * NT) {  // (four loads in flight per thread)
      float4 a[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = in[min(i0 + u * NT, n - 1)];
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (i0 + u * NT < n) atomicAdd(&hist[(key_of(a[u]) >> shift) & 15u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t r = 0;
      for (int d = 0; d < 16; ++d) { dbase[d] = r; r += hist[d]; }
    }
    __syncthreads();
    if (tid < 16) {  // the sub-segments; the non-empty ones listed for the cascade
      const int k = li * 16 + tid;
      sb[tid] = b0 + (int)dbase[tid];
      se[tid] = b0 + (int)(dbase[tid] + hist[tid]);
      x.leaf[k] = j.leaf[s];
      x.frame[k] = fr;
      x.out_count[k] = 0;
      if (hist[tid]) x.ilist[atomicAdd(&x.counts[2], 1)] = k;
    }
    float4* dst = x.pts + b0;
    for (int t0 = 0; t0 < n; t0 += TILE) {
      const int nt = min(TILE, n - t0);
      uint32_t k[E];
      float4 a[E];
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int i = tid * E + e;
        a[e] = i < nt ? in[t0 + i] : make_float4(0, 0, 0, 0);
        k[e] = i < nt ? key_of(a[e]) : 0u;
      }
      int rank[E];
      tile_rank4<NT, E>(k, shift, nt, sc, ttot, rank);
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (rank[e] >= 0) dst[dbase[(k[e] >> shift) & 15u] + rank[e]] = a[e];
      __syncthreads();
      if (tid < 16) dbase[tid] += ttot[tid];
      __syncthreads();
    }
  }
}

// the split parents' outputs: the 16 sub-segments' VoxelGrid outputs concatenated in bucket order
// into the parent's output (one workgroup per parent)
template <int NT>
__global__ __launch_bounds__(NT) void k_vg_join(VgJob j, VgSplit x) {
  __shared__ int pre[17];
  const int tid = threadIdx.x;
  const int nl = min(*j.list_n, x.npar);
  for (int li = blockIdx.x; li < nl; li += gridDim.x) {
    const int s = j.list[li];
    const int* sb = x.begin + (size_t)li * 16;
    const int* se = x.end + (size_t)li * 16;
    const int* sc = x.out_count + (size_t)li * 16;
    if (tid == 0) {
      int r = 0, any = 0;
      for (int d = 0; d < 16; ++d) {
        pre[d] = r;
        const int m = se[d] - sb[d];
        any |= m;
        r += m > 0 ? sc[d] : 0;
      }
      pre[16] = any ? r : -1;  // (-1: the parent was copied by k_vg_split)
    }
    __syncthreads();
    if (pre[16] >= 0) {  // output t of the parent: bucket d = the last with pre[d] <= t
      const int b0 = j.begin[s], tot = pre[16];
      for (int t0 = tid; t0 < tot; t0 += 4 * NT) {
        float4 v[4];
        int o[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int t = t0 + u * NT;
          int d = 0;
#pragma unroll
          for (int step = 8; step > 0; step >>= 1)
            if (d + step < 16 && pre[d + step] <= t) d += step;
          o[u] = t;
          v[u] = t < tot ? x.out[sb[d] + (t - pre[d])] : make_float4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (o[u] < tot) j.out[b0 + o[u]] = v[u];
      }
      if (tid == 0) j.out_count[s] = tot;
    }
    __syncthreads();
  }
}

// Incremental VoxelGrid of a cube segment (:1018-1036) whose first nold points are the cube's
// previous VoxelGrid output and whose tail is this frame's appended points.  A VoxelGrid output
// lists one point per voxel in voxel order; when the old points' voxel keys (under this segment's
// bounding box: the order of absolute grid cells (k, j, i) does not depend on it) are strictly
// increasing, the stable (voxel, position) sort of the whole segment is the merge of the old points
// with the sorted tail, old first within a voxel (they precede the tail in input order).  So only the
// tail is sorted (LDS bitonic, <= NEW points), and each output voxel sums its members in input
// order: its old point, then its tail points — the same float sums as the full sort.  Segments whose
// old keys are not strictly increasing (a cube appended to without a VoxelGrid since, or a mean
// rounded into a neighbouring voxel), whose keys exceed the cascade's 24 sorted bits, or whose box
// is "too small" are left to the cascade (skip[s] = 0).
// (segments beyond the cascade's LDS tiers, which k_vg_big would sort through global memory; the
// LDS tiers measured faster than the merge on 2k-12k segments)
// (Tuning::vg_merge_min: 12288 by default, the largest LDS tier)
template <int NT, int NEW>
__global__ __launch_bounds__(NT) void k_vg_merge(VgJob j) {
  static_assert((NEW & (NEW - 1)) == 0 && NEW % NT == 0 && NEW <= 65536, "bitonic sort / scan layout");
  __shared__ uint64_t nk[NEW];      // tail (key << 32 | tail position), sorted
  __shared__ uint16_t nhp[NEW];     // first entry in nk of each tail voxel that holds no old point
  __shared__ int isc[24];
  const int tid = threadIdx.x;
  const int nl = *j.mlist_n;
  for (int li = blockIdx.x; li < nl; li += gridDim.x) {
    const int s = j.mlist[li];
    const int b0 = j.begin[s], n = j.end[s] - b0, nold = j.nold[s], nnew = n - nold;
    const float4* in = j.in + b0;
    float mn[3] = {3.4e38f, 3.4e38f, 3.4e38f}, mx[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
    for (int i = tid; i < n; i += NT) {
      const float4 a = in[i];
      mn[0] = fminf(mn[0], a.x); mn[1] = fminf(mn[1], a.y); mn[2] = fminf(mn[2], a.z);
      mx[0] = fmaxf(mx[0], a.x); mx[1] = fmaxf(mx[1], a.y); mx[2] = fmaxf(mx[2], a.z);
    }
    block_bbox<NT>(mn, mx);
    const float inv = 1.0f / j.leaf[s];
    if (vg_leaf_too_small(mn, mx, inv)) {  // (the cascade copies it)
      if (tid == 0) j.skip[s] = 0;
      continue;
    }
    const int m0 = (int)floorf(mn[0] * inv), m1 = (int)floorf(mn[1] * inv), m2 = (int)floorf(mn[2] * inv);
    const int divx = (int)floorf(mx[0] * inv) - m0 + 1, divy = (int)floorf(mx[1] * inv) - m1 + 1;
    const uint32_t mul1 = (uint32_t)divx, mul2 = (uint32_t)(divx * divy);
    auto key_of = [&](const float4& a) {
      const int i0 = (int)(floorf(a.x * inv) - (float)m0);
      const int i1 = (int)(floorf(a.y * inv) - (float)m1);
      const int i2 = (int)(floorf(a.z * inv) - (float)m2);
      return (uint32_t)i0 + (uint32_t)i1 * mul1 + (uint32_t)i2 * mul2;
    };
    // the old keys (global scratch, the segment's range of the sort arrays) and their order check
    uint32_t* K = j.keys + b0;
    bool bad = false;
    for (int i = tid; i < nold; i += NT) {
      const uint32_t k = key_of(in[i]);
      K[i] = k;
      bad |= k >= (1u << 24);
    }
    // the tail's (key, position), padded to a power of two for the sort
    int P2 = 1;
    while (P2 < nnew) P2 <<= 1;
    for (int t = tid; t < P2; t += NT) {
      uint64_t e = ~0ull;
      if (t < nnew) {
        const uint32_t k = key_of(in[nold + t]);
        bad |= k >= (1u << 24);
        e = ((uint64_t)k << 32) | (uint32_t)t;
      }
      nk[t] = e;
    }
    __syncthreads();
    for (int i = tid + 1; i < nold; i += NT) bad |= K[i] <= K[i - 1];
    if (__syncthreads_or(bad)) {
      if (tid == 0) j.skip[s] = 0;
      continue;
    }
    if (P2 > 1) block_bitonic_sort<NT>(nk, P2);
    __syncthreads();
    // lower_bound of key k in the old keys (global, ascending)
    auto old_lb = [&](uint32_t k) {
      int lo = 0, hi = nold;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (K[mid] < k) lo = mid + 1; else hi = mid;
      }
      return lo;
    };
    // the tail's voxels that hold no old point, compacted in key order (NEW / NT entries per thread)
    constexpr int PT = NEW / NT;
    int fl[PT], cntf = 0;
#pragma unroll
    for (int u = 0; u < PT; ++u) {
      const int t = tid * PT + u;
      fl[u] = 0;
      if (t < nnew) {
        const uint32_t k = (uint32_t)(nk[t] >> 32);
        if (t == 0 || (uint32_t)(nk[t - 1] >> 32) != k) {
          const int at = old_lb(k);
          fl[u] = (at == nold || K[at] != k) ? 1 : 0;
        }
      }
      cntf += fl[u];
    }
    int m = 0;
    int r = block_excl_scan<NT>(cntf, isc, m);
#pragma unroll
    for (int u = 0; u < PT; ++u)
      if (fl[u]) {
        const int t = tid * PT + u;
        nhp[r] = (uint16_t)t;
        ++r;
      }
    __syncthreads();
    // sums of a voxel's tail members from tail entry e on (sorted: input order within the voxel)
    auto add_tail = [&](int e, uint32_t k, float& sx, float& sy, float& sz, float& si, int& c) {
      for (; e < nnew && (uint32_t)(nk[e] >> 32) == k; ++e) {
        const float4 a = in[nold + (int)(uint32_t)nk[e]];
        sx += a.x; sy += a.y; sz += a.z; si += a.w;
        ++c;
      }
    };
    // old voxels: slot = i + (tail-only voxels before it); members = the old point, then its tail run
    for (int i = tid; i < nold; i += NT) {
      const uint32_t k = K[i];
      int lo = 0, hi = m;  // tail-only voxels with a smaller key
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((uint32_t)(nk[nhp[mid]] >> 32) < k) lo = mid + 1; else hi = mid;
      }
      const int slot = i + lo;
      int e0 = 0, e1 = nnew;  // first tail entry with key >= k
      while (e0 < e1) {
        const int mid = (e0 + e1) >> 1;
        if ((uint32_t)(nk[mid] >> 32) < k) e0 = mid + 1; else e1 = mid;
      }
      const float4 a = in[i];
      float sx = 0, sy = 0, sz = 0, si = 0;
      sx += a.x; sy += a.y; sz += a.z; si += a.w;
      int c = 1;
      add_tail(e0, k, sx, sy, sz, si, c);
      const float cnt = (float)c;
      j.out[b0 + slot] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
    }
    // tail-only voxels: slot = r + (old voxels before it)
    for (int q = tid; q < m; q += NT) {
      const uint32_t k = (uint32_t)(nk[nhp[q]] >> 32);
      const int slot = q + old_lb(k);
      float sx = 0, sy = 0, sz = 0, si = 0;
      int c = 0;
      add_tail(nhp[q], k, sx, sy, sz, si, c);
      const float cnt = (float)c;
      j.out[b0 + slot] = make_float4(sx / cnt, sy / cnt, sz / cnt, si / cnt);
    }
    if (tid == 0) {
      j.out_count[s] = nold + m;
      j.skip[s] = 1;
    }
    __syncthreads();
  }
}

// The cascade: the fused LDS kernel at cap1 points (2048: 256 threads, for the many small cube
// segments; 12288: 1024 threads) over every segment; the segments beyond it through the 12288
// kernel (after the 2048 one), then the rest through k_vg_big.  The list-driven launches use fixed
// grids whose workgroups leave at once when their lists are short.  finish = false: the caller
// knows every segment fits cap1 (streaming stacks), only the first launch is enqueued.
// tier2_idx: the second tier is k_vg_idx (16384 points; the long surf stacks) rather than
// k_vg_radix<1024, 12> (12288; measured faster on the 2k-12k cube segments: at batch 1024 the cubes
// took 0.68 ms/step with it against 0.85 with k_vg_idx, the stacks 0.86 with k_vg_idx against 1.20)
// TAG: kVgStack / kVgCubes / kVgSurround, so a kernel trace or PMC pass tells the jobs apart
constexpr int kVgListGrid = 1024, kVgBigGrid = 256;
constexpr int kVgStack = 0, kVgCubes = 1, kVgSurround = 2;
// split (the stack job's VgSplit, when it holds every segment of the job as a parent): the segments
// the cascade's LDS kernels cannot take are split into key-range buckets (k_vg_split / k_vg_join)
// instead of k_vg_big; split_early: already the segments beyond the first kernel (instead of the
// second tier too)
template <int TAG>
hipError_t vg_run(const VgJob& j0, hipStream_t st, int cap1, bool finish = true, bool tier2_idx = false,
                  const VgSplit* split = nullptr, bool split_early = false) {
  if (j0.nseg == 0) return hipSuccess;
  if (!j0.zeroed) {
    const hipError_t e = hipMemsetAsync(j0.counts, 0, 2 * sizeof(int), st);
    if (e != hipSuccess) return e;
  }
  if (split && split->npar < j0.nseg) split = nullptr;
  // the segments of list `l` (count at j0.counts + l) through the split: 16 key-range buckets each,
  // the buckets through the cascade in their parent's frame, the outputs joined
  auto run_split = [&](int l) -> hipError_t {
    VgJob c = j0;
    c.list = j0.lists[l];
    c.list_n = j0.counts + l;
    const hipError_t ez = hipMemsetAsync(split->counts, 0, 3 * sizeof(int), st);
    if (ez != hipSuccess) return ez;
    hipLaunchKernelGGL((k_vg_split<1024, 12>), dim3(std::min(split->npar, 256)), dim3(1024), 0, st, c, *split);
    VgJob sj = j0;
    sj.in = split->pts;
    sj.out = split->out;
    sj.begin = split->begin;
    sj.end = split->end;
    sj.leaf = split->leaf;
    sj.out_count = split->out_count;
    sj.frame = split->frame;
    sj.nseg = split->npar * 16;
    sj.lists[0] = split->lists[0];
    sj.lists[1] = split->lists[1];
    sj.counts = split->counts;
    sj.zeroed = true;                  // (counts[0..1] zeroed above)
    sj.list = split->ilist;            // the non-empty sub-segments k_vg_split listed
    sj.list_n = split->counts + 2;
    sj.grid_max = 2048;                // (the list is empty unless the job had big segments)
    const hipError_t e = vg_run<TAG>(sj, st, 2048, true, true);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_vg_join<1024>), dim3(std::min(split->npar, 256)), dim3(1024), 0, st, c, *split);
    return hipGetLastError();
  };
  // the caller's input list (non-empty segments) is walked by a fixed grid
  const int grid = std::min(j0.grid_max, j0.list ? std::min(j0.nseg, 8192) : std::min(j0.nseg, 65536));
  VgJob a = j0;
  a.big = j0.lists[0];
  a.big_n = j0.counts;
  int last = 0;  // the list k_vg_big takes
  if (cap1 <= 2048) {
    hipLaunchKernelGGL((k_vg_radix<256, 8, TAG>), dim3(grid), dim3(256), 0, st, a);
    if (finish && split && split_early) return run_split(0);
    if (finish) {
      VgJob b = j0;
      b.list = j0.lists[0];
      b.list_n = j0.counts;
      b.big = j0.lists[1];
      b.big_n = j0.counts + 1;
      if (tier2_idx) hipLaunchKernelGGL((k_vg_idx<1024, 16, TAG>), dim3(std::min(j0.nseg, kVgListGrid)), dim3(1024), 0, st, b);
      else hipLaunchKernelGGL((k_vg_radix<1024, 12, TAG>), dim3(std::min(j0.nseg, kVgListGrid)), dim3(1024), 0, st, b);
      last = 1;
    }
  } else {
    hipLaunchKernelGGL((k_vg_radix<1024, 12, TAG>), dim3(grid), dim3(1024), 0, st, a);
  }
  if (finish) {
    if (split) return run_split(last);
    VgJob c = j0;
    c.list = j0.lists[last];
    c.list_n = j0.counts + last;
    hipLaunchKernelGGL((k_vg_big<1024, 12, TAG>), dim3(std::min(j0.nseg, kVgBigGrid)), dim3(1024), 0, st, c);
  }
  return hipGetLastError();
}

}  // namespace

// The three VoxelGrid routes: which cascade a job takes, from the decision inputs the product has.
// The product's call sites and the diagnostic hook (loam_dev_vg_run) both go through these.

// the stacks (:693-701), P instances: two large segments per instance (the fused 12288-point kernel
// for a few instances, the 2048-point one for batches); when the host knows every segment fits the
// first kernel (stack_max >= 0: streaming), the cascade's finish is not enqueued
hipError_t vg_route_stack(const VgJob& js, hipStream_t st, int P, int stack_max, int vg_split, int capS,
                          const VgSplit* vgs) {
  const bool fits = stack_max >= 0 && stack_max <= (P <= 4 ? 12288 : 2048);
  // (vg_split 1: the split takes the segments beyond the first kernel when a sweep can fill several
  // LDS-tier segments (HDL-64E: 64 problems 0.56 -> 0.49 ms/step), else only those beyond the LDS
  // kernels (VLP-16 at 128 / 1024 problems: splitting beyond the first kernel 0.24 -> 0.32 ms/step))
  const bool split_early = vg_split == 3 || (vg_split == 1 && capS > 4 * 16384);
  return vg_run<kVgStack>(js, st, P <= 4 ? 12288 : 2048, !fits, /*tier2_idx=*/true, vg_split ? vgs : nullptr,
                          split_early);
}

// the valid cubes (:1018-1036), P instances: with vg_merge the long segments with a short tail first
// (k_vg_merge over mlist, which sets skip), the rest by the cascade.  Most of the 2 x 125 cube
// segments per instance are small: batches start with the 2048-point kernel (many workgroups per
// CU); a few instances with the 12288-point one (one launch)
hipError_t vg_route_cubes(VgJob jv, hipStream_t st, int P, int vg_merge, const int* nold, const int* mlist,
                          const int* mlist_n, int* skip) {
  if (vg_merge) {
    jv.nold = nold; jv.mlist = mlist; jv.mlist_n = mlist_n; jv.skip = skip;
    // (its segments are rare: a small grid whose workgroups leave at once when the list is short)
    hipLaunchKernelGGL((k_vg_merge<1024, kVgMergeNew>), dim3(std::min(jv.nseg, 32)), dim3(1024), 0, st, jv);
  }
  return vg_run<kVgCubes>(jv, st, P <= 4 ? 12288 : 2048);
}

// the surround map (:1042-1047): one segment (a streaming context, the diagnostic hook), or one per
// due lane through the job's list (loam_lanes_surround); the first tier by the number of segments
// as the stack and cube routes choose it by P
hipError_t vg_route_surround(const VgJob& j, hipStream_t st) {
  return vg_run<kVgSurround>(j, st, j.nseg <= 4 ? 12288 : 2048);
}

// ---------------------------------------------------------------- scratch
hipError_t vg_scratch_alloc(VgScratch& s, size_t sort_points, size_t segments, int split_parents,
                            size_t split_points) {
  DevAlloc A;
  A(&s.keys, sort_points * sizeof(uint32_t));
  A(&s.keys_alt, sort_points * sizeof(uint32_t));
  A(&s.vals, sort_points * sizeof(uint32_t));
  A(&s.vals_alt, sort_points * sizeof(uint32_t));
  A(&s.lists[0], segments * sizeof(int));
  A(&s.lists[1], segments * sizeof(int));
  A(&s.counts, 4 * sizeof(int));
  // the split: 16 sub-segments per parent, points / outputs indexed like the job's input
  VgSplit& x = s.split;
  const size_t sub = (size_t)split_parents * 16;
  x.npar = split_parents;
  A(&x.pts, split_points * sizeof(float4));
  A(&x.out, split_points * sizeof(float4));
  A(&x.begin, sub * sizeof(int));
  A(&x.end, sub * sizeof(int));
  A(&x.out_count, sub * sizeof(int));
  A(&x.leaf, sub * sizeof(float));
  A(&x.frame, sub * sizeof(VgFrame));
  A(&x.lists[0], sub * sizeof(int));
  A(&x.lists[1], sub * sizeof(int));
  A(&x.counts, 4 * sizeof(int));
  A(&x.ilist, sub * sizeof(int));
  if (A.err != hipSuccess) vg_scratch_free(s);
  return A.err;
}

void vg_scratch_free(VgScratch& s) {
  const VgSplit& x = s.split;
  void* ptrs[] = {s.keys, s.keys_alt, s.vals, s.vals_alt, s.lists[0], s.lists[1], s.counts, x.pts, x.out, x.begin,
                  x.end, x.out_count, x.leaf, x.frame, x.lists[0], x.lists[1], x.counts, x.ilist};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  s = VgScratch();
}

}  // namespace loam

// ---------------------------------------------------------------- diagnostic hook (dev_hooks.h)
// The VoxelGrid routes on caller-supplied segments (tests/test_gpu_voxelgrid.py): host code only,
// the launches are vg_route_stack / vg_route_cubes / vg_route_surround's, the merge list is
// vg_merge_eligible's.
struct loam_dev_vg {
  int device = 0, max_total = 0, max_seg = 0;
  hipStream_t st = nullptr;
  float4 *in = nullptr, *out = nullptr;
  int *begin = nullptr, *end = nullptr, *out_count = nullptr;
  float* leaf = nullptr;
  int *lin = nullptr, *mlist = nullptr;  // input and merge lists (lengths: vg.counts[2], [3])
  int *nold = nullptr, *skip = nullptr;
  loam::VgScratch vg;                    // sort arrays, cascade lists, counters, split
};

namespace {
void dev_vg_free(loam_dev_vg* h) {
  void* ptrs[] = {h->in, h->out, h->begin, h->end, h->out_count, h->leaf, h->lin, h->mlist, h->nold, h->skip};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  loam::vg_scratch_free(h->vg);
  if (h->st) (void)hipStreamDestroy(h->st);
  delete h;
}
}  // namespace

extern "C" int loam_dev_vg_create(int device, int32_t max_total_points, int32_t max_segments, loam_dev_vg** out) {
  if (!out) return LOAM_E_INVAL;
  *out = nullptr;
  if (max_total_points < 1 || max_segments < 1 || max_segments > (1 << 24)) return LOAM_E_INVAL;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return LOAM_E_HIP;  // (no CPU path, as loam_create)
  if (device < 0 || device >= ndev) return LOAM_E_INVAL;
  if (hipSetDevice(device) != hipSuccess) return LOAM_E_HIP;
  loam_dev_vg* h = new loam_dev_vg();
  h->device = device; h->max_total = max_total_points; h->max_seg = max_segments;
  const size_t T = (size_t)max_total_points, S = (size_t)max_segments;
  loam::DevAlloc A;
  A(&h->in, T * sizeof(float4));
  A(&h->out, T * sizeof(float4));
  A(&h->begin, S * sizeof(int));
  A(&h->end, S * sizeof(int));
  A(&h->out_count, S * sizeof(int));
  A(&h->leaf, S * sizeof(float));
  A(&h->lin, S * sizeof(int));
  A(&h->mlist, S * sizeof(int));
  A(&h->nold, S * sizeof(int));
  A(&h->skip, S * sizeof(int));
  hipError_t e = A.err;
  // the split: every segment a parent (as mp_alloc's for the 2P stacks)
  if (e == hipSuccess) e = loam::vg_scratch_alloc(h->vg, T, S, max_segments, T);
  if (e == hipSuccess) e = hipStreamCreate(&h->st);
  if (e != hipSuccess) {
    dev_vg_free(h);
    return e == hipErrorOutOfMemory ? LOAM_E_NOMEM : LOAM_E_HIP;
  }
  *out = h;
  return LOAM_OK;
}

extern "C" int loam_dev_vg_run(loam_dev_vg* h, const loam_dev_vg_job* job, float* out_pts, int32_t* out_count,
                               int32_t* merged) {
  if (!h || !job || !out_pts || !out_count || !merged) return LOAM_E_INVAL;
  const int n = job->nseg, total = job->total;
  if (n < 1 || n > h->max_seg || total < 1 || total > h->max_total) return LOAM_E_INVAL;
  if (!job->pts || !job->begin || !job->end || !job->leaf || job->P < 1) return LOAM_E_INVAL;
  if (job->route < LOAM_DEV_VG_STACK || job->route > LOAM_DEV_VG_SURROUND) return LOAM_E_INVAL;
  if (job->route == LOAM_DEV_VG_SURROUND && n != 1) return LOAM_E_INVAL;
  if (job->vg_split < 0 || job->vg_split > 3 || job->vg_merge < 0 || job->vg_merge > 1 || job->vg_merge_min < 0)
    return LOAM_E_INVAL;
  int prev_end = 0;
  for (int s = 0; s < n; ++s) {  // every segment inside [0, total), in ascending order, none overlapping
    const int b0 = job->begin[s], b1 = job->end[s];
    if (b0 < prev_end || b1 < b0 || b1 > total) return LOAM_E_INVAL;
    if (!(job->leaf[s] > 0.0f) || !(job->leaf[s] < 3.0e38f)) return LOAM_E_INVAL;
    if (job->nold && (job->nold[s] < 0 || job->nold[s] > b1 - b0)) return LOAM_E_INVAL;
    prev_end = b1;
  }
  const bool cubes = job->route == LOAM_DEV_VG_CUBES, merge = cubes && job->vg_merge != 0;
  // what k_mp_vseg leaves on the cube route: the non-empty segments listed, the merge candidates
  // listed, count 0 for the empty ones, skip 0; elsewhere every count starts at -1
  std::vector<int> lin, ml, cnt0((size_t)n, -1), nold((size_t)n, 0), zero((size_t)n, 0);
  for (int s = 0; s < n; ++s) {
    const int len = job->end[s] - job->begin[s];
    if (job->nold) nold[s] = job->nold[s];
    if (!cubes) continue;
    if (len == 0) {
      cnt0[s] = 0;
      continue;
    }
    lin.push_back(s);
    if (merge && loam::vg_merge_eligible(len, nold[s], job->vg_merge_min)) ml.push_back(s);
  }
  const int cnt4[4] = {0, 0, (int)lin.size(), (int)ml.size()};
  hipStream_t st = h->st;
  auto up = [&](void* d, const void* s, size_t bytes) {
    return bytes ? hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
  };
  hipError_t e = hipSetDevice(h->device);
  if (e == hipSuccess) e = up(h->in, job->pts, (size_t)total * sizeof(float4));
  if (e == hipSuccess) e = up(h->begin, job->begin, (size_t)n * sizeof(int));
  if (e == hipSuccess) e = up(h->end, job->end, (size_t)n * sizeof(int));
  if (e == hipSuccess) e = up(h->leaf, job->leaf, (size_t)n * sizeof(float));
  if (e == hipSuccess) e = up(h->out_count, cnt0.data(), (size_t)n * sizeof(int));
  if (e == hipSuccess) e = up(h->nold, nold.data(), (size_t)n * sizeof(int));
  if (e == hipSuccess) e = up(h->skip, zero.data(), (size_t)n * sizeof(int));
  if (e == hipSuccess) e = up(h->lin, lin.data(), lin.size() * sizeof(int));
  if (e == hipSuccess) e = up(h->mlist, ml.data(), ml.size() * sizeof(int));
  if (e == hipSuccess) e = up(h->vg.counts, cnt4, sizeof(cnt4));  // (the product's earlier kernels zero the first two)
  if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)h->out, (int)LOAM_DEV_VG_SENTINEL, (size_t)total * 4, st);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    return LOAM_E_HIP;
  }
  loam::VgJob j = h->vg.job();
  j.in = h->in; j.out = h->out; j.begin = h->begin; j.end = h->end; j.leaf = h->leaf;
  j.out_count = h->out_count; j.nseg = n; j.total = total;
  j.zeroed = true;
  if (job->route == LOAM_DEV_VG_STACK) {
    h->vg.split.npar = n;
    e = loam::vg_route_stack(j, st, job->P, job->stack_max, job->vg_split, job->capS, &h->vg.split);
  } else if (cubes) {
    j.list = h->lin; j.list_n = h->vg.counts + 2;
    e = loam::vg_route_cubes(j, st, job->P, job->vg_merge, h->nold, h->mlist, h->vg.counts + 3, h->skip);
  } else {
    e = loam::vg_route_surround(j, st);
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out_pts, h->out, (size_t)total * sizeof(float4), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(out_count, h->out_count, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && merge) e = hipMemcpyAsync(merged, h->skip, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);  // (the host arrays above live until here)
  if (e == hipSuccess) e = es;
  if (!merge) std::fill(merged, merged + n, -1);
  return e == hipSuccess ? LOAM_OK : LOAM_E_HIP;
}

extern "C" int loam_dev_vg_destroy(loam_dev_vg* h) {
  if (!h) return LOAM_E_INVAL;
  (void)hipSetDevice(h->device);
  if (h->st) (void)hipStreamSynchronize(h->st);
  dev_vg_free(h);
  return LOAM_OK;
}
