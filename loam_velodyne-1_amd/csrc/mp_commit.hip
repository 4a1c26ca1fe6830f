// Shared lanes on gfx950: the listed lanes' last frames into the store (loam_lanes_map_commit;
// mp.hpp: MpCommit).
#include <algorithm>

#include "mp_dev.hpp"

namespace loam {
namespace {
// what the commit kernels write besides the commit's own buffers: the store's idle pool and slot
// table and its VoxelGrid input / output
struct CmDst {
  int* nslots;     // [kCubeNum][4] the idle slot table
  float4* npool;   // the idle pool
  float4* vin;
  const float4* vout;
};

LOAM_D bool cm_in_union(const unsigned* uni, int cube) { return (uni[cube >> 5] >> (cube & 31)) & 1u; }

// Stage 2, one workgroup per listed lane (blockIdx.x = its list position): k_mp_insert's cube slot
// of every stack point about the store's centre and its stable per-(kind, cube) ranks (the dense-key
// ballot ranking, or one wave in stack order beyond kDense keys), then instead of the instance's
// prefix and scatter: the lane's key list with its counts, every point's entry in that list, the
// lane's valid cubes OR-ed into the union, and the inserted / outside counts.
template <int NT>
__global__ __launch_bounds__(NT) void k_cm_rank(MpBuffers w, LocStore s, MpCommit c) {
  const int ip = blockIdx.x, tid = threadIdx.x, lane = lane_id();
  const int p = c.list[ip];
  if (p < 0 || p >= w.P) {
    if (tid == 0) c.lnk[ip] = 0;
    return;
  }
  const int nsc = min(max(w.sseg_cnt[p * 2 + 0], 0), w.capC), nss = min(max(w.sseg_cnt[p * 2 + 1], 0), w.capS);
  const float4* stack = w.stack + (size_t)p * w.cap_stack;
  const loampose::MapRot r = rot_load(w, p);
  const int cW = s.istate[kMiCenW], cH = s.istate[kMiCenH], cD = s.istate[kMiCenD];
  int* so = c.ent_of + (size_t)ip * c.cap_stack;
  int* ro = c.rank_of + (size_t)ip * c.cap_stack;
  __shared__ int cnt[2][kCubeNum];
  __shared__ int scratch[NT / 64 + 1];
  __shared__ int nout[2];
  constexpr int kKeyWords = (2 * kCubeNum + 31) / 32, kDense = 512, kWaves = NT / 64;
  __shared__ unsigned keybits[kKeyWords];
  __shared__ int keypre[kKeyWords + 1];
  __shared__ int wcnt[kWaves][kDense];
  for (int i = tid; i < 2 * kCubeNum; i += NT) cnt[i / kCubeNum][i % kCubeNum] = 0;
  for (int i = tid; i < kKeyWords; i += NT) keybits[i] = 0u;
  for (int i = tid; i < kWaves * kDense; i += NT) wcnt[i / kDense][i % kDense] = 0;
  if (tid < 2) nout[tid] = 0;
  __syncthreads();
  {  // the lane's valid cubes into the union
    const int nv = min(max(w.istate[(size_t)p * kMpStateInts + kMiNValid], 0), kMaxValid);
    if (tid < nv) {
      const int ind = w.valid[(size_t)p * kMaxValid + tid];
      if (ind >= 0 && ind < kCubeNum) atomicOr(c.uni() + (ind >> 5), 1u << (ind & 31));
    }
  }
  const int nst = nsc + nss;
  for (int q = tid; q < nst; q += NT) {
    const float4 a = loampose::point_to_map(r, stack[q < nsc ? q : w.capC + (q - nsc)]);
    const int ci = cube_of(a.x, cW), cj = cube_of(a.y, cH), ck = cube_of(a.z, cD);
    const bool in = ci >= 0 && ci < kCubeW && cj >= 0 && cj < kCubeH && ck >= 0 && ck < kCubeD;
    const int sl = in ? cube_index(ci, cj, ck) : -1;
    so[q] = sl;
    if (sl >= 0) {
      const int key = sl * 2 + (q < nsc ? 0 : 1);
      atomicOr(&keybits[key >> 5], 1u << (key & 31));
    } else {
      atomicAdd(&nout[q < nsc ? 0 : 1], 1);
    }
  }
  __threadfence_block();
  __syncthreads();
  {  // exclusive prefix of the words' popcounts
    constexpr int kPer = (kKeyWords + NT - 1) / NT;
    int sum = 0;
    for (int k = 0; k < kPer; ++k) {
      const int i = tid * kPer + k;
      if (i < kKeyWords) sum += __popc(keybits[i]);
    }
    int tot;
    int run = block_excl_scan<NT>(sum, scratch, tot);
    for (int k = 0; k < kPer; ++k) {
      const int i = tid * kPer + k;
      if (i < kKeyWords) {
        keypre[i] = run;
        run += __popc(keybits[i]);
      }
    }
    if (tid == 0) keypre[kKeyWords] = tot;
  }
  __syncthreads();
  const int nkeys = keypre[kKeyWords];
  if (nkeys <= kDense) {
    // stable ranks, all waves: wave wv ranks its contiguous chunk of the stack (in order, per dense
    // key), then each key's chunk counts are prefixed in wave order
    const int wv = tid >> 6, chunk = ((nst + kWaves * 64 - 1) / (kWaves * 64)) * 64;
    const int q0 = wv * chunk, q1 = min(nst, q0 + chunk);
    for (int base = q0; base < q1; base += 64) {
      const int q = base + lane;
      const bool v = q < q1;
      const int sl = v ? so[q] : -1;
      const int key = sl < 0 ? -1 : sl * 2 + (q < nsc ? 0 : 1);
      const int id = key < 0 ? -1 : keypre[key >> 5] + __popc(keybits[key >> 5] & ((1u << (key & 31)) - 1u));
      uint64_t m = __ballot(v && id >= 0);
      int rank = 0;
      while (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        const int il = __builtin_amdgcn_readlane(id, leader);
        const uint64_t mm = __ballot(v && id == il);
        const int basecnt = wcnt[wv][il];
        if (v && id == il) rank = basecnt + __popcll(mm & lanemask_lt());
        __builtin_amdgcn_wave_barrier();
        if (lane == leader) wcnt[wv][il] = basecnt + __popcll(mm);
        __builtin_amdgcn_wave_barrier();
        m &= ~mm;
      }
      if (v) ro[q] = rank;
    }
    __threadfence_block();
    __syncthreads();
    for (int i = tid; i < 2 * kCubeNum; i += NT) {
      if (!(keybits[i >> 5] & (1u << (i & 31)))) continue;
      const int id = keypre[i >> 5] + __popc(keybits[i >> 5] & ((1u << (i & 31)) - 1u));
      int run = 0;
#pragma unroll
      for (int ww = 0; ww < kWaves; ++ww) {
        const int cc = wcnt[ww][id];
        wcnt[ww][id] = run;
        run += cc;
      }
      cnt[i & 1][i >> 1] = run;
    }
    __threadfence_block();
    __syncthreads();
    for (int q = tid; q < nst; q += NT) {
      const int sl = so[q];
      if (sl < 0) continue;
      const int key = sl * 2 + (q < nsc ? 0 : 1);
      const int id = keypre[key >> 5] + __popc(keybits[key >> 5] & ((1u << (key & 31)) - 1u));
      ro[q] += wcnt[q / chunk][id];
    }
  } else if (tid < 64) {  // many keys: stable ranks by one wave, stack order
    for (int base = 0; base < nst; base += 64) {
      const int q = base + lane;
      const bool v = q < nst;
      const int kind = q < nsc ? 0 : 1;
      const int sl = v ? so[q] : -1;
      const int key = sl < 0 ? -1 : sl * 2 + kind;
      uint64_t m = __ballot(v && key >= 0);
      int rank = 0;
      while (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        const int kl = __builtin_amdgcn_readlane(key, leader);
        const uint64_t mm = __ballot(v && key == kl);
        const int basecnt = cnt[kl & 1][kl >> 1];
        if (v && key == kl) rank = basecnt + __popcll(mm & lanemask_lt());
        __builtin_amdgcn_wave_barrier();
        if (lane == leader) cnt[kl & 1][kl >> 1] = basecnt + __popcll(mm);
        __builtin_amdgcn_wave_barrier();
        m &= ~mm;
      }
      if (v) ro[q] = rank;
    }
  }
  __threadfence_block();
  __syncthreads();
  // the lane's key list (entry = the key's dense number, which is below kmax = min(cap_stack, kMapKeys))
  const int nk = min(nkeys, c.kmax);
  int* lk = c.lkey + (size_t)ip * c.kmax;
  int* lc = c.lcnt + (size_t)ip * c.kmax;
  int ins[2] = {0, 0};
  for (int i = tid; i < 2 * kCubeNum; i += NT) {
    if (!(keybits[i >> 5] & (1u << (i & 31)))) continue;
    const int id = keypre[i >> 5] + __popc(keybits[i >> 5] & ((1u << (i & 31)) - 1u));
    if (id >= nk) continue;
    lk[id] = (i & 1) * kCubeNum + (i >> 1);
    lc[id] = cnt[i & 1][i >> 1];
    ins[i & 1] += cnt[i & 1][i >> 1];
  }
  for (int q = tid; q < nst; q += NT) {
    const int sl = so[q];
    if (sl < 0) continue;
    const int key = sl * 2 + (q < nsc ? 0 : 1);
    const int id = keypre[key >> 5] + __popc(keybits[key >> 5] & ((1u << (key & 31)) - 1u));
    so[q] = id < nk ? id : -1;
  }
  const int insC = block_reduce<NT>(ins[0], scratch, [](int a, int b) { return a + b; });
  const int insS = block_reduce<NT>(ins[1], scratch, [](int a, int b) { return a + b; });
  if (tid == 0) {
    c.lnk[ip] = nk;
    atomicAdd(c.res() + kCrIns, insC);
    atomicAdd(c.res() + kCrIns + 1, insS);
    atomicAdd(c.res() + kCrOut, nout[0]);
    atomicAdd(c.res() + kCrOut + 1, nout[1]);
  }
}

// Stages 3 and 4's tables, one workgroup: the per-key counts prefixed across the listed lanes in list
// order (only the entries of the lanes' key lists are walked; the running counts of all kMapKeys keys
// sit in LDS), then per key the appended points' place in app and, for a union cube, its VoxelGrid
// segment (old ++ appended, leaf 0.2 / 0.4) by one scan each, and the list of non-empty segments.
template <int NT>
__global__ __launch_bounds__(NT) void k_cm_prefix(LocStore s, MpCommit c, int n) {
  constexpr int E = (kMapKeys + NT - 1) / NT;
  const int tid = threadIdx.x;
  __shared__ int g[kMapKeys];
  __shared__ int snk[kLocMax];
  __shared__ int scratch[NT / 64 + 1];
  __shared__ int vk[2];
  for (int x = tid; x < kMapKeys; x += NT) g[x] = 0;
  for (int i = tid; i < n; i += NT) snk[i] = min(max(c.lnk[i], 0), c.kmax);
  if (tid < 2) vk[tid] = 0;
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    const int nk = snk[i];
    int* lk = c.lkey + (size_t)i * c.kmax;
    int* lc = c.lcnt + (size_t)i * c.kmax;
    for (int e = tid; e < nk; e += NT) {  // (a lane lists a key once: no two threads share a word of g)
      const int k = lk[e];
      if (k < 0 || k >= kMapKeys) continue;
      const int cn = lc[e];
      lc[e] = g[k];
      g[k] += cn;
    }
    __syncthreads();
  }
  const int x0 = tid * E, x1 = min(kMapKeys, x0 + E);
  int sa = 0, sv = 0, ncube = 0;
  for (int x = x0; x < x1; ++x) {
    const int kind = x / kCubeNum, cube = x % kCubeNum;
    sa += g[x];
    if (cm_in_union(c.uni(), cube)) {
      sv += max(s.slots[cube * 4 + 1 + 2 * kind], 0) + g[x];
      ncube += kind == 0;
    }
  }
  int atot, vtot;
  int ao = block_excl_scan<NT>(sa, scratch, atot);
  int vo = block_excl_scan<NT>(sv, scratch, vtot);
  const bool over = vtot > s.map_cap;
  for (int x = x0; x < x1; ++x) {
    const int kind = x / kCubeNum, cube = x % kCubeNum;
    const int a = g[x], nold = max(s.slots[cube * 4 + 1 + 2 * kind], 0);
    const int nv = cm_in_union(c.uni(), cube) ? nold + a : 0;
    c.aoff[x] = ao;
    c.acnt[x] = a;
    c.seg_b[x] = over ? 0 : vo;
    c.seg_e[x] = over ? 0 : vo + nv;
    c.seg_leaf[x] = kind == 0 ? 0.2f : 0.4f;
    c.seg_cnt[x] = 0;
    if (nv > 0) {
      atomicAdd(&vk[kind], nv);
      if (!over) c.vlist[atomicAdd(c.counts() + 2, 1)] = x;
    }
    ao += a;
    vo += nv;
  }
  ncube = block_reduce<NT>(ncube, scratch, [](int a, int b) { return a + b; });
  if (tid == 0) {
    int* res = c.res();
    res[kCrCubes] = ncube;
    res[kCrVin] = vk[0];
    res[kCrVin + 1] = vk[1];
    if (over) res[kCrErr] = kCrErrVin;
  }
}

// Stage 3's scatter: listed lane blockIdx.y's stack points into the map frame (the same transform as
// k_cm_rank's, the bits k_mp_insert stores) at their key's place in app: behind the key's points of
// the earlier listed lanes, in stack order
__global__ __launch_bounds__(256) void k_cm_scatter(MpBuffers w, MpCommit c) {
  const int ip = blockIdx.y;
  const int p = c.list[ip];
  if (p < 0 || p >= w.P) return;
  const int nsc = min(max(w.sseg_cnt[p * 2 + 0], 0), w.capC), nss = min(max(w.sseg_cnt[p * 2 + 1], 0), w.capS);
  const float4* stack = w.stack + (size_t)p * w.cap_stack;
  const loampose::MapRot r = rot_load(w, p);
  const int* so = c.ent_of + (size_t)ip * c.cap_stack;
  const int* ro = c.rank_of + (size_t)ip * c.cap_stack;
  const int* lk = c.lkey + (size_t)ip * c.kmax;
  const int* lc = c.lcnt + (size_t)ip * c.kmax;
  const int nk = min(max(c.lnk[ip], 0), c.kmax);
  const size_t cap = (size_t)c.S * c.cap_stack;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < nsc + nss; q += gridDim.x * 256) {
    const int e = so[q];
    if (e < 0 || e >= nk) continue;
    const int k = lk[e];
    if (k < 0 || k >= kMapKeys) continue;
    const size_t dst = (size_t)c.aoff[k] + lc[e] + ro[q];
    if (dst < cap) c.app[dst] = loampose::point_to_map(r, stack[q < nsc ? q : w.capC + (q - nsc)]);
  }
}

// Stage 4's copy: the VoxelGrid input of every listed segment, old cube content ++ appended points;
// a workgroup per segment of the list
__global__ __launch_bounds__(256) void k_cm_vcopy(LocStore s, MpCommit c, CmDst d) {
  if (c.res()[kCrErr]) return;
  const int nl = min(c.counts()[2], kMapKeys);
  for (int it = blockIdx.x; it < nl; it += gridDim.x) {
    const int x = c.vlist[it];
    const int kind = x / kCubeNum, cube = x % kCubeNum;
    const int nold = max(s.slots[cube * 4 + 1 + 2 * kind], 0), off = s.slots[cube * 4 + 2 * kind];
    const int b0 = c.seg_b[x], n = c.seg_e[x] - b0, a0 = c.aoff[x];
    if (b0 < 0 || n < 0 || b0 + n > s.map_cap || off < 0 || off + nold > s.map_cap) continue;
    for (int t = threadIdx.x; t < n; t += 256) d.vin[b0 + t] = t < nold ? s.pool[off + t] : c.app[a0 + (t - nold)];
  }
}

// Stage 6's table, one workgroup: the new slot table (kind-major, cubes ascending, as
// k_mp_compact_table lays a store out): a union cube's key holds its VoxelGrid output, every other
// key old ++ appended; the totals and the overflow mark into the result block
template <int NT>
__global__ __launch_bounds__(NT) void k_cm_table(LocStore s, MpCommit c, CmDst d) {
  constexpr int E = (kMapKeys + NT - 1) / NT;
  const int tid = threadIdx.x;
  if (c.res()[kCrErr]) return;
  __shared__ int scratch[NT / 64 + 1];
  __shared__ int tk[2];
  if (tid < 2) tk[tid] = 0;
  __syncthreads();
  auto size_of = [&](int x) {
    const int kind = x / kCubeNum, cube = x % kCubeNum;
    return cm_in_union(c.uni(), cube) ? max(c.seg_cnt[x], 0) : max(s.slots[cube * 4 + 1 + 2 * kind], 0) + c.acnt[x];
  };
  const int x0 = tid * E, x1 = min(kMapKeys, x0 + E);
  int sum = 0;
  for (int x = x0; x < x1; ++x) sum += size_of(x);
  int run;
  int off = block_excl_scan<NT>(sum, scratch, run);
  for (int x = x0; x < x1; ++x) {
    const int kind = x / kCubeNum, cube = x % kCubeNum, nn = size_of(x);
    d.nslots[cube * 4 + 2 * kind] = off;
    d.nslots[cube * 4 + 1 + 2 * kind] = nn;
    if (nn) atomicAdd(&tk[kind], nn);
    off += nn;
  }
  __syncthreads();
  if (tid == 0) {
    int* res = c.res();
    res[kCrMap] = tk[0];
    res[kCrMap + 1] = tk[1];
    if (run > s.map_cap) res[kCrErr] = kCrErrMap;
  }
}

// Stage 6's copy into the idle pool, a workgroup per key at a time
__global__ __launch_bounds__(256) void k_cm_copy(LocStore s, MpCommit c, CmDst d) {
  if (c.res()[kCrErr]) return;
  for (int x = blockIdx.x; x < kMapKeys; x += gridDim.x) {
    const int kind = x / kCubeNum, cube = x % kCubeNum;
    const int n = d.nslots[cube * 4 + 1 + 2 * kind], dst = d.nslots[cube * 4 + 2 * kind];
    if (n <= 0 || dst < 0 || dst + n > s.map_cap) continue;
    if (cm_in_union(c.uni(), cube)) {
      const int b0 = c.seg_b[x];
      if (b0 < 0 || b0 + n > s.map_cap) continue;
      for (int t = threadIdx.x; t < n; t += 256) d.npool[dst + t] = d.vout[b0 + t];
    } else {
      const int nold = max(s.slots[cube * 4 + 1 + 2 * kind], 0), off = s.slots[cube * 4 + 2 * kind], a0 = c.aoff[x];
      if (off < 0 || off + nold > s.map_cap) continue;
      for (int t = threadIdx.x; t < n; t += 256) d.npool[dst + t] = t < nold ? s.pool[off + t] : c.app[a0 + (t - nold)];
    }
  }
}

// loam_dev_lanes_commit_input: lane p's stack in the map frame by k_cm_rank's transform, stack order
__global__ __launch_bounds__(256) void k_cm_input(MpBuffers w, int p, float4* outC, float4* outS) {
  const int nsc = min(max(w.sseg_cnt[p * 2 + 0], 0), w.capC), nss = min(max(w.sseg_cnt[p * 2 + 1], 0), w.capS);
  const float4* stack = w.stack + (size_t)p * w.cap_stack;
  const loampose::MapRot r = rot_load(w, p);
  for (int q = blockIdx.x * 256 + threadIdx.x; q < nsc + nss; q += gridDim.x * 256) {
    const float4 a = loampose::point_to_map(r, stack[q < nsc ? q : w.capC + (q - nsc)]);
    if (q < nsc) outC[q] = a; else outS[q - nsc] = a;
  }
}
}  // namespace

size_t mp_commit_bytes(int S, int cap_stack) {
  const size_t Ps = (size_t)S * cap_stack, kmax = (size_t)std::min(cap_stack, kMapKeys);
  return Ps * (2 * sizeof(int) + sizeof(float4)) + (size_t)S * kmax * 2 * sizeof(int) + (size_t)S * 2 * sizeof(int) +
         (size_t)kCmZeroInts * sizeof(int) + (size_t)kMapKeys * 9 * sizeof(int);
}

hipError_t mp_commit_alloc(MpCommit& c, int S, int cap_stack) {
  if (c.S) return hipSuccess;
  DevAlloc A;
  const size_t Ps = (size_t)S * cap_stack;
  c.cap_stack = cap_stack;
  c.kmax = std::min(cap_stack, kMapKeys);
  A(&c.ent_of, Ps * sizeof(int));
  A(&c.rank_of, Ps * sizeof(int));
  A(&c.app, Ps * sizeof(float4));
  A(&c.lkey, (size_t)S * c.kmax * sizeof(int));
  A(&c.lcnt, (size_t)S * c.kmax * sizeof(int));
  A(&c.lnk, (size_t)S * sizeof(int));
  A(&c.list, (size_t)S * sizeof(int));
  A(&c.zero, (size_t)kCmZeroInts * sizeof(int));
  int** per_key[] = {&c.aoff, &c.acnt, &c.seg_b, &c.seg_e, &c.seg_cnt, &c.vlist, &c.lists[0], &c.lists[1]};
  for (int** q : per_key) A(q, (size_t)kMapKeys * sizeof(int));
  A(&c.seg_leaf, (size_t)kMapKeys * sizeof(float));
  if (A.err == hipSuccess)
    A.err = hipHostMalloc((void**)&c.pin, ((size_t)S + kCmResWords) * sizeof(int), hipHostMallocDefault);
  if (A.err != hipSuccess) {
    mp_commit_free(c);
    return A.err;
  }
  c.S = S;
  return hipSuccess;
}

void mp_commit_free(MpCommit& c) {
  void* ptrs[] = {c.ent_of, c.rank_of, c.app, c.lkey, c.lcnt, c.lnk, c.list, c.zero, c.aoff, c.acnt, c.seg_b,
                  c.seg_e, c.seg_cnt, c.vlist, c.lists[0], c.lists[1], c.seg_leaf};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  if (c.pin) (void)hipHostFree(c.pin);
  c = MpCommit();
}

hipError_t mp_lanes_commit(MpCommit& c, const MpBuffers& w, MpBuffers& s, int n, hipStream_t st, Prof* prof) {
  static_assert(LOAM_LANES_MAX <= kLocMax, "k_cm_prefix holds a count per listed lane in LDS (snk)");
  if (n <= 0 || n > c.S || n > w.P || c.cap_stack != w.cap_stack || !s.pool || !s.vin) return hipErrorInvalidValue;
  auto mark = [&](const char* name) { if (prof) prof->mark(name); };
  mp_wait_update(s, st);  // (a deferred update of the streaming path lands first)
  hipError_t e = s.sticky != hipSuccess ? s.take_error() : hipSuccess;
  if (e == hipSuccess) e = hipMemcpyAsync(c.list, c.list_h(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(c.zero, 0, (size_t)kCmZeroInts * sizeof(int), st);
  if (e != hipSuccess) return e;
  const LocStore store = loc_store(s);
  CmDst d;
  d.nslots = s.slots + (size_t)(1 - s.pool_cur) * s.P * kCubeNum * 4;
  d.npool = s.pool + (size_t)(1 - s.pool_cur) * s.P * s.map_cap;
  d.vin = s.vin;
  d.vout = s.vout;
  hipLaunchKernelGGL(k_cm_rank<1024>, dim3(n), dim3(1024), 0, st, w, store, c);
  mark("k_cm_rank");
  hipLaunchKernelGGL(k_cm_prefix<1024>, dim3(1), dim3(1024), 0, st, store, c, n);
  mark("k_cm_prefix");
  hipLaunchKernelGGL(k_cm_scatter, dim3(8, n), dim3(256), 0, st, w, c);
  mark("k_cm_scatter");
  hipLaunchKernelGGL(k_cm_vcopy, dim3(1024), dim3(256), 0, st, store, c, d);
  mark("k_cm_vcopy");
  // the union's cubes: one VoxelGrid job over the store's input / output and sort arrays with the
  // commit's segments and lists.  Up to kMapKeys mostly small segments: the batch's cascade (the
  // 2048-point kernel first); the merge route is not taken (every route gives the same bits, §5.1)
  VgJob jv = s.vg.job();
  jv.in = s.vin; jv.out = s.vout; jv.begin = c.seg_b; jv.end = c.seg_e; jv.leaf = c.seg_leaf;
  jv.out_count = c.seg_cnt; jv.nseg = kMapKeys; jv.total = s.P * s.map_cap;
  jv.lists[0] = c.lists[0]; jv.lists[1] = c.lists[1]; jv.counts = c.counts();
  jv.list = c.vlist; jv.list_n = c.counts() + 2; jv.zeroed = true;
  e = vg_route_cubes(jv, st, /*P=*/kMapKeys, /*vg_merge=*/0, nullptr, nullptr, nullptr, nullptr);
  if (e != hipSuccess) return e;
  mark("vg_commit");
  hipLaunchKernelGGL(k_cm_table<1024>, dim3(1), dim3(1024), 0, st, store, c, d);
  hipLaunchKernelGGL(k_cm_copy, dim3(1024), dim3(256), 0, st, store, c, d);
  mark("k_cm_compact");
  e = hipGetLastError();
  if (e == hipSuccess)
    e = hipMemcpyAsync(c.res_h(), c.res(), (size_t)kCmResWords * sizeof(int), hipMemcpyDeviceToHost, st);
  return e;
}

hipError_t mp_lanes_commit_input(const MpBuffers& w, int lane, float4* outC, float4* outS, hipStream_t st) {
  if (lane < 0 || lane >= w.P) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_cm_input, dim3(16), dim3(256), 0, st, w, lane, outC, outS);
  return hipGetLastError();
}

}  // namespace loam
