// Lanes: the working set of S sequences stepped in lockstep and the kernel that gathers a step's
// per-lane results (lanes.hpp; the step itself is composed in engine_lanes.cpp from the batch kernels).
#include "lanes.hpp"

namespace loam {

namespace {
struct LaneOutSrc {
  const int* sr_err;      // [S]
  const float* od_state;  // [S][kOdStateFloats]
  const int* od_istate;   // [S][kOdStateInts]
  const float* mp_state;  // [S][kMpStateFloats]
  const int* mp_istate;   // [S][kMpStateInts]
  const int* nreg;        // [S]
  const int* loc;         // [S][kLocResWords] shared lanes on a mapping step, else null
};

// 32 lanes of a wave per lane of the step, one word each: the three error words, the two iteration
// counts, the registered cloud's size, transformSum, Aft, Bef, and whether mapping's L-M ran
// (shared lanes: a lane whose result block says LOAM_LOC_OFFGRID was not evaluated and registers nothing)
__global__ __launch_bounds__(256) void k_lanes_out(LaneOutSrc s, int* out, int S) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int l = gid >> 5, w = gid & 31;
  if (l >= S || w >= kLaneOutWords) return;
  const int* oi = s.od_istate + (size_t)l * kOdStateInts;
  const int* mi = s.mp_istate + (size_t)l * kMpStateInts;
  int v;
  if (w == kLoSrErr) v = s.sr_err[l];
  else if (w == kLoOdErr) v = oi[kIsErr];
  else if (w == kLoMpErr) v = mi[kMiErr];
  else if (w == kLoOdIters) v = oi[kIsIters];
  else if (w == kLoMpIters) v = mi[kMiIters];
  else if (w == kLoNReg) v = s.loc && s.loc[(size_t)l * kLocResWords + kLrStatus] == LOAM_LOC_OFFGRID ? 0 : s.nreg[l];
  else if (w < kLoAft) v = __float_as_int(s.od_state[(size_t)l * kOdStateFloats + kOdSum + (w - kLoOdSum)]);
  else if (w < kLoBef) v = __float_as_int(s.mp_state[(size_t)l * kMpStateFloats + kMpAft + (w - kLoAft)]);
  else if (w == kLoLmRan) v = mi[kMiLmRan];
  else v = __float_as_int(s.mp_state[(size_t)l * kMpStateFloats + kMpBef + (w - kLoBef)]);
  out[(size_t)l * kLaneOutWords + w] = v;
}

// the step's new queue entries into the lanes' device queues (thread g < nrec), and every lane's
// imuPointerLast (thread g < S)
__global__ __launch_bounds__(256) void k_lanes_imu_put(const loamimu::LaneHdr* hdr, const loamimu::LaneRec* rec, int nrec,
                                                       loamimu::SrQueue* q, int S) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g < nrec) {
    const loamimu::LaneRec r = rec[g];
    loamimu::lane_record_put(q[r.lane], r);
  }
  if (g < S) q[g].last = hdr[g].last;
}

struct LaneImuDst {
  loamimu::SrQueue* q;     // [S]
  loamimu::SrTail* tail;   // [S]
  float* od_state;         // [S][kOdStateFloats]
  float* mp_state;         // [S][kMpStateFloats]
  int* mp_istate;          // [S][kMpStateInts]
  float* trans;            // [S][12]
};

// 32 threads per lane, behind the ring sort.  A lane with a queue: the tail its sweep left
// (SrTail) becomes the queue's, /imu_trans (src/scanRegistration.cpp:614-635) goes into the
// odometry state in the order load_imu reads and into the step's result, and on the odometry's
// init frame transformSum starts from the IMU pitch / roll (src/laserOdometry.cpp:451-452).  On
// mapping steps every lane gets transformUpdate's (roll, pitch, flag).
__global__ __launch_bounds__(256) void k_lanes_imu(const loamimu::LaneHdr* hdr, LaneImuDst d, int od_init, int mapping,
                                                    int S) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int l = gid >> 5, w = gid & 31;
  const bool live = l < S;
  const loamimu::LaneHdr h = live ? hdr[l] : loamimu::LaneHdr{};
  const bool has = live && h.has != 0;
  float v = 0.0f;      // word w of the tail that holds from here on
  int front = 0, valid = 0;
  if (has) {
    valid = d.tail[l].valid;
    if (w < 24) v = valid ? d.tail[l].v[w] : (&d.q[l].rollStart)[w];
    front = d.tail[l].front;
  }
  __syncthreads();  // (every thread has read `valid` before it is cleared)
  if (has && valid) {
    if (w < 24) (&d.q[l].rollStart)[w] = v;
    if (w == 24) d.q[l].front = front;
    if (w == 25) d.tail[l].valid = 0;
  }
  // imu_trans[k] = tail word kMap[k]: pitch / yaw / roll Start, pitch / yaw / roll Cur, FromStart
  constexpr int kMap[12] = {1, 2, 0, 10, 11, 9, 18, 19, 20, 21, 22, 23};
  int src = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k)
    if (w == k) src = kMap[k];
  const float it = __shfl(v, (threadIdx.x & 32) + src, 64);
  if (live && w < 12) {
    d.trans[(size_t)l * 12 + w] = has ? it : 0.0f;
    if (has) {
      d.od_state[(size_t)l * kOdStateFloats + kOdImu + w] = it;
      if (od_init && (w == 0 || w == 2)) d.od_state[(size_t)l * kOdStateFloats + kOdSum + w] = 0.0f + it;
    }
  }
  if (live && mapping) {
    if (w == 12) d.mp_state[(size_t)l * kMpStateFloats + kMpImuRP] = h.roll;
    if (w == 13) d.mp_state[(size_t)l * kMpStateFloats + kMpImuRP + 1] = h.pitch;
    if (w == 14) d.mp_istate[(size_t)l * kMpStateInts + kMiImu] = h.mp_flag;
  }
}
struct LaneClear {
  // the odometry problem and the sweep's error word
  float* od_state;   // [S][kOdStateFloats]
  int* od_istate;    // [S][kOdStateInts]
  int* nlast;        // [S][kOdBufs][2]
  int* nfullEnd;     // [S][kOdBufs]
  int *hC_T, *hS_T;  // [kOdBufs][S]
  int* od_done;      // [S]
  int* sr_err;       // [S]
  // the mapping store
  float* mp_state;   // [S][kMpStateFloats]
  int* mp_istate;    // [S][kMpStateInts]
  int4* slots;       // [2][S][kCubeNum]
  int* mp_done;      // [S]
  int* nreg;         // [S]
  // the IMU side (null before the first loam_lanes_imu)
  int* q;            // [S][kQueWords]
  int* tail;         // [S][kTailWords]
  int* tile_key;     // [S][ntile3]
  int ntile3;
  int S;
};
constexpr int kQueWords = (int)(sizeof(loamimu::SrQueue) / 4), kTailWords = (int)(sizeof(loamimu::SrTail) / 4);
static_assert(sizeof(loamimu::SrQueue) % 4 == 0 && sizeof(loamimu::SrTail) % 4 == 0, "cleared by words");
constexpr int kRestartTiles = 10;  // workgroups per lane: each pool's 4851 slot entries in two coalesced passes

// loam_lanes_restart: lane list[blockIdx.y] as lanes_alloc (od_alloc, mp_alloc's mp_reset,
// lanes_imu_alloc) left it.  The two pools' slot tables are the bulk (an int4 per cube, coalesced
// over the workgroups of the lane); workgroup 0 also clears the lane's small blocks.  A lane
// appears once in the list and no word is shared between lanes: plain stores.
__global__ __launch_bounds__(256) void k_lanes_restart(LaneClear c, const int* list, int what) {
  const int l = list[blockIdx.y];
  if (l < 0 || l >= c.S) return;
  const int tid = threadIdx.x;
  if ((what & kClearMp) && c.slots) {  // (shared lanes have no store: slots is null)
    const int4 z = make_int4(0, 0, 0, 0);
    for (int pool = 0; pool < 2; ++pool) {
      int4* s = c.slots + ((size_t)pool * c.S + l) * kCubeNum;
      for (int i = blockIdx.x * 256 + tid; i < kCubeNum; i += gridDim.x * 256) s[i] = z;
    }
  }
  if (blockIdx.x != 0) return;
  if (what & kClearMp) {
    if (tid < kMpStateFloats) c.mp_state[(size_t)l * kMpStateFloats + tid] = 0.0f;
    if (tid < kMpStateInts)  // laserCloudCenWidth / Height / Depth (src/laserMapping.cpp:64-66), as k_mp_reset
      c.mp_istate[(size_t)l * kMpStateInts + tid] = tid == kMiCenW || tid == kMiCenD ? 10 : tid == kMiCenH ? 5 : 0;
    if (tid == 0) { c.mp_done[l] = 0; c.nreg[l] = 0; }
  }
  if (what & kClearOd) {
    if (tid < kOdStateFloats) c.od_state[(size_t)l * kOdStateFloats + tid] = 0.0f;
    if (tid < kOdStateInts) c.od_istate[(size_t)l * kOdStateInts + tid] = 0;
    if (tid < kOdBufs * 2) c.nlast[l * kOdBufs * 2 + tid] = 0;
    if (tid < kOdBufs) {
      c.nfullEnd[l * kOdBufs + tid] = 0;
      c.hC_T[tid * c.S + l] = 0;
      c.hS_T[tid * c.S + l] = 0;
    }
    if (tid == 0) { c.od_done[l] = 0; c.sr_err[l] = 0; }
  }
  if ((what & kClearImu) && c.q) {
    for (int i = tid; i < kQueWords; i += 256) c.q[(size_t)l * kQueWords + i] = 0;
    for (int i = tid; i < kTailWords; i += 256) c.tail[(size_t)l * kTailWords + i] = 0;
    for (int i = tid; i < c.ntile3; i += 256) c.tile_key[(size_t)l * c.ntile3 + i] = 0;
  }
}

// A restarted lane's init frame inside a step whose shared launches ran an ordinary frame on it
// (its odometry inactive: the cleared CornerLastNum / SurfLastNum, src/laserOdometry.cpp:465).
// Lane list[blockIdx.y] ends the step as k_od_end's mode 0 and od_frame's init frame leave a
// context (src/laserOdometry.cpp:427-456): Last[dst] = the raw lessSharp / lessFlat clouds with
// their fractional intensities, no full cloud, transform = 0, transformSum = (0 + imuPitchStart, 0,
// 0 + imuRollStart, 0, 0, 0) from the /imu_trans k_lanes_imu left in the state (zeros without IMU),
// matP and the int state zero, the overflow of a Last cloud in the error word.
__global__ __launch_bounds__(256) void k_lanes_init(OdBuffers b, FeatView f, const int* list, int dst) {
  const int p = list[blockIdx.y];
  if (p < 0 || p >= b.P) return;
  const int nl = f.count(p, 1), nf = f.count(p, 3);
  const int cl = min(nl, b.capC), cf = min(nf, b.capS);
  float4* oc = b.lastC + ((size_t)dst * b.P + p) * b.capC;
  float4* os = b.lastS + ((size_t)dst * b.P + p) * b.capS;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < cl + cf; i += gridDim.x * 256) {
    if (i < cl) oc[i] = f.lsharp[(size_t)p * f.lsharp_stride + i];
    else os[i - cl] = f.lflat[(size_t)p * f.lflat_stride + (i - cl)];
  }
  if (blockIdx.x != 0) return;
  float* st = b.state + (size_t)p * kOdStateFloats;
  int* ist = b.istate + (size_t)p * kOdStateInts;
  const int w = threadIdx.x;
  if (w < kOdImu) st[w] = w == kOdSum || w == kOdSum + 2 ? 0.0f + st[kOdImu + (w - kOdSum)] : 0.0f;
  if (w < kOdStateInts) ist[w] = w == kIsErr && (nl > b.capC || nf > b.capS) ? ERR_CAP_ROWS : 0;
  if (w == 0) {
    b.nlast[(p * kOdBufs + dst) * 2 + 0] = cl;
    b.nlast[(p * kOdBufs + dst) * 2 + 1] = cf;
    b.nfullEnd[p * kOdBufs + dst] = 0;
  }
}

// loam_lanes_set_pose: 16 threads per listed lane, one word each.  blk: the n lane indices, then n
// x 12 floats (Aft, Bef).  A lane appears once in the list and no word is shared between lanes:
// plain stores.
__global__ __launch_bounds__(256) void k_lanes_set_pose(float* mp_state, const int* blk, int n, int S) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int i = gid >> 4, w = gid & 15;
  if (i >= n || w >= 12) return;
  const int l = blk[i];
  if (l < 0 || l >= S) return;
  const float v = reinterpret_cast<const float*>(blk)[n + i * 12 + w];
  mp_state[(size_t)l * kMpStateFloats + (w < 6 ? kMpAft + w : kMpBef + (w - 6))] = v;
}

struct LaneMapDst {
  float4* pool;    // [S][map_cap] the current pool
  int4* slots;     // [S][kCubeNum] its slot tables
  float* state;    // [S][kMpStateFloats]
  int* istate;     // [S][kMpStateInts]
  int S, map_cap;
};
constexpr int kMapInstallSlotWg = 5;   // workgroups per lane that write its slot table: 4851 int4 in four coalesced passes
constexpr int kMapInstallPer = 8;      // points per thread of the point workgroups: 8 x 16 bytes in flight per lane of the wave
constexpr int kMapInstallTile = 256 * kMapInstallPer;

// loam_lanes_map_import: one sorted map into lane list[blockIdx.y]'s current pool segment and slot
// table.  Workgroups [0, kMapInstallSlotWg) of a lane copy the table (an int4 per cube), workgroup 0
// also the centre, Aft = pose blockIdx.y and Bef (mi: the call's block, kMi* of lanes.hpp); every
// other workgroup copies one tile of the points, all its loads issued before its stores.  Source and destination are 16-byte aligned and a
// wave's 64 lanes touch 1 KiB in a row on both sides.  A lane appears once in the list and no word
// is shared between lanes: plain stores, no workgroup reads what another writes.
__global__ __launch_bounds__(256) void k_lanes_map_install(LaneMapDst d, const float4* src, int kept, const int4* table,
                                                           const int* mi, int n) {
  const int l = mi[kMiList + blockIdx.y];
  if (l < 0 || l >= d.S) return;
  const int tid = threadIdx.x;
  if (blockIdx.x < kMapInstallSlotWg) {
    int4* s = d.slots + (size_t)l * kCubeNum;
    for (int i = blockIdx.x * 256 + tid; i < kCubeNum; i += kMapInstallSlotWg * 256) s[i] = table[i];
    if (blockIdx.x != 0) return;
    const float* mf = reinterpret_cast<const float*>(mi);
    if (tid < 3) d.istate[(size_t)l * kMpStateInts + kMiCenW + tid] = mi[kMiCen + tid];
    if (tid >= 64 && tid < 70) d.state[(size_t)l * kMpStateFloats + kMpAft + (tid - 64)] = mf[kMiList + n + blockIdx.y * 6 + (tid - 64)];
    if (tid >= 128 && tid < 134) d.state[(size_t)l * kMpStateFloats + kMpBef + (tid - 128)] = mf[kMiBef + (tid - 128)];
    return;
  }
  const int base = (blockIdx.x - kMapInstallSlotWg) * kMapInstallTile + tid;
  float4* dst = d.pool + (size_t)l * d.map_cap;
  static_assert(kMapInstallPer == 8, "eight points per thread, named");
  // (kept > 0 here: the grid has no point workgroups without points; the lanes past the end load point 0)
  auto at = [&](int r) { return base + r * 256 < kept ? base + r * 256 : 0; };
  const float4 v0 = src[at(0)], v1 = src[at(1)], v2 = src[at(2)], v3 = src[at(3)];
  const float4 v4 = src[at(4)], v5 = src[at(5)], v6 = src[at(6)], v7 = src[at(7)];
  if (base < kept) dst[base] = v0;
  if (base + 256 < kept) dst[base + 256] = v1;
  if (base + 512 < kept) dst[base + 512] = v2;
  if (base + 768 < kept) dst[base + 768] = v3;
  if (base + 1024 < kept) dst[base + 1024] = v4;
  if (base + 1280 < kept) dst[base + 1280] = v5;
  if (base + 1536 < kept) dst[base + 1536] = v6;
  if (base + 1792 < kept) dst[base + 1792] = v7;
}

struct LaneSur {
  const float4* pool;  // [S][map_cap] the current pool
  const int4* slots;   // [S][kCubeNum] its slot tables
  const int* istate;   // [S][kMpStateInts]
  float4* vin;         // [S][map_cap] lane l's VoxelGrid input at l * map_cap
  const float4* vout;  // [S][map_cap] ... and its output
  int *vseg_b, *vseg_e, *vseg_cnt;  // segment l = lane l
  float* vseg_leaf;
  int* vg_lin;         // the VoxelGrid's input list: the due lanes
  int* vg_counts;      // VgScratch::counts
  int S, map_cap;
};
constexpr int kSurWg = 16;   // workgroups per due lane (a 16k-point neighbourhood: one tile each)
constexpr int kSurPer = 4;   // points per thread and tile: 4 x 16 bytes in flight per lane of the wave
constexpr int kSurTile = 256 * kSurPer;
constexpr int kSurCubes = 125;  // the 5 x 5 x 5 neighbourhood (kMaxValid)

// loam_lanes_surround's gather: k_mp_surround for lane list[blockIdx.y], over kSurWg workgroups.
// Every workgroup of a lane derives the lane's 125 neighbourhood entries itself (thread t = cube
// (i, j, k) of the reference's loop order, an out-of-bounds cube an empty entry) and two block
// scans give each entry's first point and first tile; the (cube, tile) pieces are then dealt round
// robin to the lane's workgroups.  A piece is kSurTile points of one cube, corner points then surf
// points: four loads per thread issued before the four stores, a wave's 64 lanes 1 KiB in a row on
// both sides.  Workgroup 0 of a lane writes its segment (vseg_b / vseg_e / vseg_leaf = 0.2, the
// leaf of downSizeFilterCorner) and its entry of the VoxelGrid's input list; workgroup (0, 0) the
// cascade's counters.  No word is shared between lanes and none is read that another workgroup
// writes: plain stores.  Every index is checked against map_cap (a store whose last update
// overflowed is a failed lane and never listed).
__global__ __launch_bounds__(256) void k_lanes_surround(LaneSur s, const int* list, int n) {
  const int tid = threadIdx.x;
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    s.vg_counts[0] = 0;
    s.vg_counts[1] = 0;
    s.vg_counts[2] = n;
  }
  const int l = list[blockIdx.y];
  if (l < 0 || l >= s.S) return;
  __shared__ int4 sh_slot[kSurCubes];
  __shared__ int sh_pre[kSurCubes], sh_tpre[kSurCubes], sh_scan[8];
  const int* ist = s.istate + (size_t)l * kMpStateInts;
  int4 e = make_int4(0, 0, 0, 0);
  if (tid < kSurCubes) {
    const int i = ist[kMiCubeI] - 2 + tid / 25, j = ist[kMiCubeJ] - 2 + (tid / 5) % 5, k = ist[kMiCubeK] - 2 + tid % 5;
    if (i >= 0 && i < kCubeW && j >= 0 && j < kCubeH && k >= 0 && k < kCubeD)
      e = s.slots[(size_t)l * kCubeNum + (i + kCubeW * j + kCubeW * kCubeH * k)];
    e.y = min(max(e.y, 0), s.map_cap);
    e.w = min(max(e.w, 0), s.map_cap);
  }
  const int pts = e.y + e.w, tiles = (pts + kSurTile - 1) / kSurTile;
  int total, ntiles;
  const int pre = loamdev::block_excl_scan<256>(pts, sh_scan, total);
  const int tpre = loamdev::block_excl_scan<256>(tiles, sh_scan, ntiles);
  if (tid < kSurCubes) {
    sh_slot[tid] = e;
    sh_pre[tid] = pre;
    sh_tpre[tid] = tpre;
  }
  __syncthreads();
  if (blockIdx.x == 0 && tid == 0) {
    s.vseg_b[l] = l * s.map_cap;
    s.vseg_e[l] = l * s.map_cap + min(total, s.map_cap);
    s.vseg_leaf[l] = 0.2f;
    s.vg_lin[blockIdx.y] = l;
  }
  const float4* pool = s.pool + (size_t)l * s.map_cap;
  float4* dst = s.vin + (size_t)l * s.map_cap;
  static_assert(kSurPer == 4, "four points per thread, named");
  for (int p = blockIdx.x; p < ntiles; p += gridDim.x) {
    int c = 0;  // the last entry whose first tile is at or before p (it has tiles)
    for (int step = 64; step > 0; step >>= 1)
      if (c + step < kSurCubes && sh_tpre[c + step] <= p) c += step;
    const int4 q = sh_slot[c];
    const int cnt = q.y + q.w, t0 = (p - sh_tpre[c]) * kSurTile + tid, d0 = sh_pre[c];
    // (the lanes past the piece's end load point 0 and store nothing)
    auto src = [&](int t) { return t < q.y ? q.x + t : q.z + (t - q.y); };
    auto ok = [&](int t) { return t < cnt && d0 + t < s.map_cap && src(t) >= 0 && src(t) < s.map_cap; };
    const bool k0 = ok(t0), k1 = ok(t0 + 256), k2 = ok(t0 + 512), k3 = ok(t0 + 768);
    const float4 v0 = pool[k0 ? src(t0) : 0], v1 = pool[k1 ? src(t0 + 256) : 0];
    const float4 v2 = pool[k2 ? src(t0 + 512) : 0], v3 = pool[k3 ? src(t0 + 768) : 0];
    if (k0) dst[d0 + t0] = v0;
    if (k1) dst[d0 + t0 + 256] = v1;
    if (k2) dst[d0 + t0 + 512] = v2;
    if (k3) dst[d0 + t0 + 768] = v3;
  }
}

// loam_lanes_surround's pack, behind the VoxelGrid: lane list[blockIdx.y]'s output run (vout + l *
// map_cap, vseg_cnt[l] points) to its place behind the runs of the list's earlier lanes, from
// vin[0] on (vin is free again).  Every workgroup sums the earlier lanes' counts itself (a block
// scan over the list); the copy is k_lanes_surround's, four loads before four stores.
__global__ __launch_bounds__(256) void k_lanes_surround_pack(LaneSur s, const int* list) {
  const int tid = threadIdx.x;
  const int l = list[blockIdx.y];
  if (l < 0 || l >= s.S) return;
  __shared__ int sh_scan[8];
  auto count = [&](int lane) { return lane < 0 || lane >= s.S ? 0 : min(max(s.vseg_cnt[lane], 0), s.map_cap); };
  int part = 0, off;
  for (int i = tid; i < (int)blockIdx.y; i += 256) part += count(list[i]);
  (void)loamdev::block_excl_scan<256>(part, sh_scan, off);
  const int m = count(l);
  const float4* src = s.vout + (size_t)l * s.map_cap;
  float4* dst = s.vin + off;  // (off + m <= the listed lanes' map_cap together)
  for (int t0 = blockIdx.x * kSurTile + tid; t0 - tid < m; t0 += gridDim.x * kSurTile) {
    const bool k0 = t0 < m, k1 = t0 + 256 < m, k2 = t0 + 512 < m, k3 = t0 + 768 < m;
    const float4 v0 = src[k0 ? t0 : 0], v1 = src[k1 ? t0 + 256 : 0], v2 = src[k2 ? t0 + 512 : 0], v3 = src[k3 ? t0 + 768 : 0];
    if (k0) dst[t0] = v0;
    if (k1) dst[t0 + 256] = v1;
    if (k2) dst[t0 + 512] = v2;
    if (k3) dst[t0 + 768] = v3;
  }
}
}  // namespace

hipError_t lanes_surround_alloc(Lanes& L) {
  if (L.su_h) return hipSuccess;
  hipError_t e = hipHostMalloc((void**)&L.su_h, (size_t)2 * L.S * sizeof(int), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&L.su_d, (size_t)L.S * sizeof(int));
  if (e != hipSuccess) {
    if (L.su_h) (void)hipHostFree(L.su_h);
    L.su_h = nullptr;
    L.su_d = nullptr;
  }
  return e;
}

hipError_t lanes_surround_run(Lanes& L, int n, bool pack, hipStream_t st, Prof* prof) {
  MpBuffers& b = L.mp;
  if (n <= 0 || n > L.S) return hipErrorInvalidValue;
  auto mark = [&](const char* name) { if (prof) prof->mark(name); };
  hipError_t e = hipMemcpyAsync(L.su_d, L.su_h, (size_t)n * sizeof(int), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  mark("lanes_surround_h2d");
  LaneSur s;
  s.pool = b.pool + (size_t)b.pool_cur * b.P * b.map_cap;
  s.slots = (const int4*)b.slots + (size_t)b.pool_cur * b.P * kCubeNum;
  s.istate = b.istate;
  s.vin = b.vin;
  s.vout = b.vout;
  s.vseg_b = b.vseg_b; s.vseg_e = b.vseg_e; s.vseg_cnt = b.vseg_cnt; s.vseg_leaf = b.vseg_leaf;
  s.vg_lin = b.vg_lin;
  s.vg_counts = b.vg.counts;
  s.S = L.S;
  s.map_cap = b.map_cap;
  hipLaunchKernelGGL(k_lanes_surround, dim3(kSurWg, n), dim3(256), 0, st, s, (const int*)L.su_d, n);
  mark("k_lanes_surround");
  // one VoxelGrid over the due lanes' segments (segment id = lane), walked through the list
  VgJob j = b.vg.job();
  j.in = b.vin; j.out = b.vout; j.begin = b.vseg_b; j.end = b.vseg_e; j.leaf = b.vseg_leaf;
  j.out_count = b.vseg_cnt; j.nseg = n; j.total = b.P * b.map_cap;
  j.zeroed = true;  // (by k_lanes_surround)
  j.list = b.vg_lin; j.list_n = b.vg.counts + 2;
  e = vg_route_surround(j, st);
  if (e != hipSuccess) return e;
  mark("vg_lanes_surround");
  if (pack) {
    hipLaunchKernelGGL(k_lanes_surround_pack, dim3(kSurWg, n), dim3(256), 0, st, s, (const int*)L.su_d);
    mark("k_lanes_surround_pack");
  }
  e = hipGetLastError();
  if (e == hipSuccess)
    e = hipMemcpyAsync(L.su_h + L.S, b.vseg_cnt, (size_t)L.S * sizeof(int), hipMemcpyDeviceToHost, st);
  mark("lanes_surround_counts_d2h");
  return e;
}

hipError_t lanes_set_pose_alloc(Lanes& L) {
  if (L.sp_h) return hipSuccess;
  const size_t bytes = (size_t)13 * L.S * sizeof(int);
  hipError_t e = hipHostMalloc((void**)&L.sp_h, bytes, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&L.sp_d, bytes);
  if (e != hipSuccess) {
    if (L.sp_h) (void)hipHostFree(L.sp_h);
    L.sp_h = nullptr;
    L.sp_d = nullptr;
  }
  return e;
}

hipError_t lanes_set_pose(Lanes& L, int n, hipStream_t st) {
  if (n <= 0 || n > L.S) return hipErrorInvalidValue;
  hipError_t e = hipMemcpyAsync(L.sp_d, L.sp_h, (size_t)13 * n * sizeof(int), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_lanes_set_pose, dim3((n * 16 + 255) / 256), dim3(256), 0, st, L.mp.state, (const int*)L.sp_d, n, L.S);
  return hipGetLastError();
}

hipError_t lanes_map_import_alloc(Lanes& L) {
  if (L.mi_h) return hipSuccess;
  const size_t bytes = ((size_t)kMiList + 7 * (size_t)L.S) * sizeof(int);
  hipError_t e = hipHostMalloc((void**)&L.mi_h, bytes, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&L.mi_d, bytes);
  if (e != hipSuccess) {
    if (L.mi_h) (void)hipHostFree(L.mi_h);
    L.mi_h = nullptr;
    L.mi_d = nullptr;
  }
  return e;
}

hipError_t lanes_map_install(Lanes& L, const float4* src, int kept, const int* table, int n, hipStream_t st) {
  const MpBuffers& b = L.mp;
  if (n <= 0 || n > L.S || kept < 0 || kept > b.map_cap) return hipErrorInvalidValue;
  LaneMapDst d;
  d.pool = b.pool + (size_t)b.pool_cur * b.P * b.map_cap;
  d.slots = (int4*)b.slots + (size_t)b.pool_cur * b.P * kCubeNum;
  d.state = b.state;
  d.istate = b.istate;
  d.S = L.S;
  d.map_cap = b.map_cap;
  const int tiles = (kept + kMapInstallTile - 1) / kMapInstallTile;
  hipLaunchKernelGGL(k_lanes_map_install, dim3(kMapInstallSlotWg + tiles, n), dim3(256), 0, st, d, src, kept,
                     (const int4*)table, L.mi_d, n);
  return hipGetLastError();
}

hipError_t lanes_restart_alloc(Lanes& L) {
  if (L.rs_h) return hipSuccess;
  hipError_t e = hipHostMalloc((void**)&L.rs_h, (size_t)2 * L.S * sizeof(int), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&L.rs_d, (size_t)2 * L.S * sizeof(int));
  if (e != hipSuccess) {
    if (L.rs_h) (void)hipHostFree(L.rs_h);
    L.rs_h = nullptr;
    L.rs_d = nullptr;
  }
  return e;
}

hipError_t lanes_restart_clear(Lanes& L, const int* list_d, int n, int what, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  LaneClear c;
  c.od_state = L.od.state;
  c.od_istate = L.od.istate;
  c.nlast = L.od.nlast;
  c.nfullEnd = L.od.nfullEnd;
  c.hC_T = L.od.hC_T;
  c.hS_T = L.od.hS_T;
  c.od_done = L.od.done;
  c.sr_err = L.sr.err;
  c.mp_state = L.mp.state;
  c.mp_istate = L.mp.istate;
  c.slots = (int4*)L.mp.slots;
  c.mp_done = L.mp.done;
  c.nreg = L.mp.nreg;
  c.q = (int*)L.imu.q_d;
  c.tail = (int*)L.imu.tail_d;
  c.tile_key = L.imu.tile_key_d;
  c.ntile3 = L.sr.ntiles() * 3;
  c.S = L.S;
  hipLaunchKernelGGL(k_lanes_restart, dim3(kRestartTiles, n), dim3(256), 0, st, c, list_d, what);
  return hipGetLastError();
}

hipError_t lanes_init_frame(Lanes& L, const FeatView& f, const int* list_d, int n, int dst, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_lanes_init, dim3(kOdEndWg, n), dim3(256), 0, st, L.od, f, list_d, dst);
  return hipGetLastError();
}

Tuning lanes_tuning(Tuning t) {
  t.od_persist = 0;
  t.mp_persist = 0;
  t.od_moments_min = LOAM_LANES_MAX + 1;
  return t;
}

hipError_t lanes_alloc(Lanes& L, int S, int cap, int R, int map_cap, int od_max_iter, int mp_max_iter, bool shared) {
  hipError_t e = sr_alloc(L.sr, S, cap, R);
  if (e == hipSuccess) e = od_alloc(L.od, S, R, cap, od_max_iter);
  if (e == hipSuccess && !shared) e = mp_alloc(L.mp, S, R, cap, map_cap, mp_max_iter);
  if (e == hipSuccess && shared) e = mp_alloc_shared(L.mp, S, R, cap, map_cap, mp_max_iter);
  if (e == hipSuccess && shared) e = hipMalloc((void**)&L.loc_d, (size_t)S * kLocResWords * sizeof(int));
  if (e == hipSuccess && shared) e = hipHostMalloc((void**)&L.loc_h, (size_t)S * kLocResWords * sizeof(int), hipHostMallocDefault);
  const size_t pts = (size_t)S * cap;
  if (e == hipSuccess) e = hipHostMalloc((void**)&L.stage_h, pts * sizeof(float4), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&L.stage_d, pts * sizeof(float4));
  if (e == hipSuccess) e = hipHostMalloc((void**)&L.tab_h, (size_t)2 * S * sizeof(int), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&L.tab_d, (size_t)2 * S * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&L.out_d, (size_t)S * kLaneOutWords * sizeof(int));
  if (e == hipSuccess) e = hipHostMalloc((void**)&L.out_h, (size_t)S * kLaneOutWords * sizeof(int), hipHostMallocDefault);
  // (the registered clouds' sizes are read by k_lanes_out on steps before the first mapping frame)
  if (e == hipSuccess) e = hipMemset(L.mp.nreg, 0, (size_t)S * sizeof(int));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    lanes_free(L);
    return e;
  }
  L.S = S;
  L.shared = shared;
  L.loc_info.assign(shared ? S : 0, loam_localize_result());
  L.fail.assign(S, LOAM_OK);
  L.fail_new.assign(S, LOAM_OK);
  L.nreg.assign(S, 0);
  L.life.assign(S, LaneLife());
  L.committed.assign(shared ? S : 0, 0);
  return hipSuccess;
}

namespace {
// loam_lanes_push_device's gather: workgroup (., s) copies lane s's d.n points from
// the caller's device memory into raw[s * cap ..) as (x, y, z, w) words; workgroup (0, s) writes
// raw_n[s].  A 16-byte stride at a 16-byte aligned pointer is one 16-byte load and store per point
// (w as it is, as pack()'s memcpy leaves it); every other layout is three dword loads and w = 0.0f
// (a 16-byte stride at another alignment: four, w as it is).
// Words are moved as integers: NaN payloads pass unchanged.
__global__ __launch_bounds__(256) void k_lanes_gather_dev(const LaneFeedDesc* __restrict__ desc, uint4* __restrict__ raw,
                                                          int* __restrict__ raw_n, int cap) {
  const int s = blockIdx.y;
  const LaneFeedDesc d = desc[s];
  const int n = min(d.n, cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) raw_n[s] = n;
  uint4* dst = raw + (size_t)s * cap;
  const int step = gridDim.x * 256;
  if (d.stride == 16 && (d.ptr & 15) == 0) {
    const uint4* src = (const uint4*)d.ptr;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += step) dst[t] = src[t];
    return;
  }
  const char* base = (const char*)d.ptr;
  const size_t stride = (uint32_t)d.stride;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += step) {
    const uint32_t* p = (const uint32_t*)(base + (size_t)t * stride);
    dst[t] = make_uint4(p[0], p[1], p[2], d.stride == 16 ? p[3] : 0u);
  }
}

// The same with point fields (loam_set_point_fields): x, y, z as three dword loads
// and w = the point's word, as pack() forms it on the host (point_fields.hpp: one statement of the
// ring map, the conversion and the word).  A sub-dword field is read as the dword that holds it and
// shifted; an F64 time as two dwords (its address may be 4 mod 8).  The plan has checked that every
// record reaches the end of both fields inside the caller's allocation.
struct GatherFields {
  uint32_t ring_type, ring_offset, time_type, time_offset, map_n, n_rings;
  double time_scale, time_bias;
  const int16_t* map;
};
__global__ __launch_bounds__(256) void k_lanes_gather_dev_fields(const LaneFeedDesc* __restrict__ desc, uint4* __restrict__ raw,
                                                                 int* __restrict__ raw_n, int cap, GatherFields f) {
  const int s = blockIdx.y;
  const LaneFeedDesc d = desc[s];
  const int n = min(d.n, cap);
  if (blockIdx.x == 0 && threadIdx.x == 0) raw_n[s] = n;
  uint4* dst = raw + (size_t)s * cap;
  const int step = gridDim.x * 256;
  const char* base = (const char*)d.ptr;
  const size_t stride = (uint32_t)d.stride;
  const bool timed = f.time_type != LOAM_FIELD_NONE;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < n; t += step) {
    const uint32_t* p = (const uint32_t*)(base + (size_t)t * stride);
    const uint32_t v = field_uint_of_dword(p[f.ring_offset >> 2], f.ring_type, f.ring_offset);
    const int r = field_ring(v, f.map_n, f.map, f.n_rings);
    float tau = 0.0f;
    if (timed) {
      const uint32_t lo = p[f.time_offset >> 2];
      const uint32_t hi = f.time_type == LOAM_FIELD_F64 ? p[(f.time_offset >> 2) + 1] : 0u;
      tau = field_tau(field_time_of_dwords(lo, hi, f.time_type), f.time_scale, f.time_bias);
    }
    dst[t] = make_uint4(p[0], p[1], p[2], __float_as_uint(field_word(r, timed, tau)));
  }
}
}  // namespace

hipError_t lanes_gather_launch(const LaneFeedDesc* desc_d, float4* raw, int* raw_n, int cap, int S, hipStream_t st) {
  if (S <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_lanes_gather_dev, dim3(std::max(1, std::min(64, (cap + 255) / 256)), S), dim3(256), 0, st, desc_d,
                     (uint4*)raw, raw_n, cap);
  return hipGetLastError();
}

hipError_t lanes_gather_dev(Lanes& L, int cap, hipStream_t st, const PointFields* pf, const int16_t* map_d) {
  const hipError_t e = hipMemcpyAsync(L.fd_d, L.fd_h, (size_t)L.S * sizeof(LaneFeedDesc), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  if (!pf) return lanes_gather_launch(L.fd_d, L.sr.raw, L.sr.raw_n, cap, L.S, st);
  if (L.S <= 0) return hipSuccess;
  if (!map_d) return hipErrorInvalidValue;
  const GatherFields f = {pf->ring_type, pf->ring_offset, pf->time_type, pf->time_offset, pf->map_n, pf->n_rings,
                          pf->time_scale, pf->time_bias, map_d};
  hipLaunchKernelGGL(k_lanes_gather_dev_fields, dim3(std::max(1, std::min(64, (cap + 255) / 256)), L.S), dim3(256), 0, st,
                     L.fd_d, (uint4*)L.sr.raw, L.sr.raw_n, cap, f);
  return hipGetLastError();
}

hipError_t lanes_feed_alloc(Lanes& L) {
  if (L.fd_h && L.fd_d) return hipSuccess;
  hipError_t e = hipHostMalloc((void**)&L.fd_h, (size_t)L.S * sizeof(LaneFeedDesc), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&L.fd_d, (size_t)L.S * sizeof(LaneFeedDesc));
  if (e != hipSuccess) {
    if (L.fd_h) (void)hipHostFree(L.fd_h);
    if (L.fd_d) (void)hipFree(L.fd_d);
    L.fd_h = L.fd_d = nullptr;
  }
  return e;
}

hipError_t lanes_imu_alloc(Lanes& L) {
  LanesImu& I = L.imu;
  const size_t S = (size_t)L.S;
  const size_t up = S * sizeof(loamimu::LaneHdr) + S * loamimu::kQue * sizeof(loamimu::LaneRec);
  hipError_t e = hipMalloc((void**)&I.q_d, S * sizeof(loamimu::SrQueue));
  if (e == hipSuccess) e = hipMalloc((void**)&I.tail_d, S * sizeof(loamimu::SrTail));
  if (e == hipSuccess) e = hipMalloc((void**)&I.tile_key_d, S * L.sr.ntiles() * 3 * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&I.up_d, up);
  if (e == hipSuccess) e = hipHostMalloc((void**)&I.up_h, up, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&I.trans_d, S * 12 * sizeof(float));
  if (e == hipSuccess) e = hipHostMalloc((void**)&I.trans_h, S * 12 * sizeof(float), hipHostMallocDefault);
  // (an empty queue: front 0, Start / Cur / FromStart zero; `last` arrives with every IMU step)
  if (e == hipSuccess) e = hipMemset(I.q_d, 0, S * sizeof(loamimu::SrQueue));
  if (e == hipSuccess) e = hipMemset(I.tail_d, 0, S * sizeof(loamimu::SrTail));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    lanes_imu_free(L);
    return e;
  }
  loamimu::SrQueue q0;
  std::memset(&q0, 0, sizeof(q0));
  q0.last = -1;
  loamimu::MpQueue m0;
  std::memset(&m0, 0, sizeof(m0));
  m0.last = -1;
  I.sr.assign(S, q0);
  I.mp.assign(S, m0);
  I.last_stamp.assign(S, -1e300);
  I.n_new.assign(S, 0);
  I.mp_front.assign(S, 0);
  I.mp_have.assign(S, 0);
  I.on = true;
  return hipSuccess;
}

void lanes_imu_free(Lanes& L) {
  LanesImu& I = L.imu;
  if (I.q_d) (void)hipFree(I.q_d);
  if (I.tail_d) (void)hipFree(I.tail_d);
  if (I.tile_key_d) (void)hipFree(I.tile_key_d);
  if (I.up_d) (void)hipFree(I.up_d);
  if (I.up_h) (void)hipHostFree(I.up_h);
  if (I.trans_d) (void)hipFree(I.trans_d);
  if (I.trans_h) (void)hipHostFree(I.trans_h);
  I = LanesImu();
}

hipError_t lanes_imu_put(Lanes& L, size_t bytes, int nrec, hipStream_t st) {
  LanesImu& I = L.imu;
  hipError_t e = hipMemcpyAsync(I.up_d, I.up_h, bytes, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  const loamimu::LaneHdr* hdr = (const loamimu::LaneHdr*)I.up_d;
  const loamimu::LaneRec* rec = (const loamimu::LaneRec*)(I.up_d + (size_t)L.S * sizeof(loamimu::LaneHdr));
  const int n = std::max(nrec, L.S);
  hipLaunchKernelGGL(k_lanes_imu_put, dim3((n + 255) / 256), dim3(256), 0, st, hdr, rec, nrec, I.q_d, L.S);
  return hipGetLastError();
}

hipError_t lanes_imu_commit(Lanes& L, bool od_init, bool mapping, hipStream_t st) {
  LanesImu& I = L.imu;
  LaneImuDst d;
  d.q = I.q_d;
  d.tail = I.tail_d;
  d.od_state = L.od.state;
  d.mp_state = L.mp.state;
  d.mp_istate = L.mp.istate;
  d.trans = I.trans_d;
  hipLaunchKernelGGL(k_lanes_imu, dim3((L.S * 32 + 255) / 256), dim3(256), 0, st, (const loamimu::LaneHdr*)I.up_d, d,
                     od_init ? 1 : 0, mapping ? 1 : 0, L.S);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    e = hipMemcpyAsync(I.trans_h, I.trans_d, (size_t)L.S * 12 * sizeof(float), hipMemcpyDeviceToHost, st);
  return e;
}

// ---------------------------------------------------------------- loam_lanes_clouds
namespace {
constexpr int kLanePackOffThreads = 256;
// One workgroup: for each of the nine clouds the exclusive prefix sums, over the n listed lanes, of
// the lane's count where bit c of its mask word is set (else 0): table[c][j] = points of cloud c in
// entries [0, j), j = 0 .. n.  The entries go through the block scan 256 at a time with the running
// total carried in a register.  A count is clamped to its stride (a failed lane's may hold anything):
// k_lanes_pack's reads stay inside the lane's slot.  An index outside [0, S) counts nothing.
__global__ __launch_bounds__(kLanePackOffThreads) void k_lanes_pack_offsets(LanePackJob job, const int* mask,
                                                                            const int* list, int n, uint64_t* table) {
  __shared__ int scratch[kLanePackOffThreads / 64 + 1];
  const int tid = threadIdx.x;
  for (int c = 0; c < kLaneClouds; ++c) {
    const LanePackSrc s = job.c[c];
    uint64_t* row = table + (size_t)c * (n + 1);
    uint64_t carry = 0;
    for (int base = 0; base < n; base += kLanePackOffThreads) {
      const int j = base + tid;
      int m = 0;
      if (j < n) {
        const int l = list[j];
        if (l >= 0 && l < job.S && (mask[l] >> c & 1)) m = min(max(s.count[(size_t)l * s.count_stride], 0), s.stride);
      }
      int total = 0;  // (<= 256 x 2^22 points: an int holds a block's sum)
      const int excl = loamdev::block_excl_scan<kLanePackOffThreads>(m, scratch, total);
      if (j < n) row[j] = carry + (uint64_t)excl;
      carry += (uint64_t)total;
    }
    if (tid == 0) row[n] = carry;
  }
}

constexpr int kLanePackThreads = 256, kLanePackPer = 4;
static_assert(kLanePackTile == kLanePackThreads * kLanePackPer, "lanes.hpp");
constexpr int kLanePackGridMax = 2048;  // 8 workgroups for each of the 256 CUs; the rest grid-strided
struct LanePackOne {      // a wanted cloud: its slots, where point 0 of its selection goes, its table row
  const float4* src;
  float4* dst;
  int stride, cloud;
};
struct LanePackSel {
  LanePackOne w[kLaneClouds];  // the nc wanted clouds, in cloud order
  int tile0[kLaneClouds + 1];  // the first tile of each among an entry's tiles (tile0[k] = the sum for k >= nc)
  int n;                  // the table's entries (row length n + 1)
  int j0, nj;             // this launch packs entries [j0, j0 + nj)
  int nc, S;
};
// Work item = (entry, wanted cloud, kLanePackTile-point tile of the cloud's stride), k_sr_pack's shape:
// the valid points of the tile from the lane's slot to their packed place, one float4 per thread per
// access and four in flight.  A tile beyond the lane's count ends after two table reads.  Source
// (slot base + t) and destination (packed offset + t) advance by one 16-byte point per thread: both
// sides coalesced and 16-byte aligned.  The counts come from the table alone (clamped and masked by
// k_lanes_pack_offsets).  (Measured against items that each take every 8th / 32nd tile of a cloud,
// whose number does not grow with the strides, and against items read off the counts, the tiles of
// each cloud's packed range with a search of the table per point: DESIGN.md §35; this shape was the
// fastest.)
__global__ __launch_bounds__(kLanePackThreads) void k_lanes_pack(LanePackSel sel, const uint64_t* table, const int* list) {
  const uint32_t per_entry = (uint32_t)sel.tile0[kLaneClouds];
  const uint32_t items = per_entry * (uint32_t)sel.nj;  // (< 2^31: lanes_pack)
  for (uint32_t w = blockIdx.x; w < items; w += gridDim.x) {
    const int j = sel.j0 + (int)(w / per_entry), r = (int)(w % per_entry);
    int kk = 0;  // the last wanted cloud whose first tile is at or before r
    while (kk + 1 < sel.nc && r >= sel.tile0[kk + 1]) ++kk;
    const LanePackOne s = sel.w[kk];  // (a uniform index into the kernel arguments: scalar loads)
    const int t0 = (r - sel.tile0[kk]) * kLanePackTile;
    const uint64_t* row = table + (size_t)s.cloud * (sel.n + 1);
    const uint64_t o = row[j];
    const int m = (int)(row[j + 1] - o);
    const int l = list[j];
    if (t0 >= m || l < 0 || l >= sel.S) continue;
    const float4* src = s.src + (size_t)l * s.stride;
    float4* out = s.dst + o;
    float4 v[kLanePackPer];
#pragma unroll
    for (int k = 0; k < kLanePackPer; ++k) {
      const int t = t0 + k * kLanePackThreads + (int)threadIdx.x;
      v[k] = t < m ? src[t] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
#pragma unroll
    for (int k = 0; k < kLanePackPer; ++k) {
      const int t = t0 + k * kLanePackThreads + (int)threadIdx.x;
      if (t < m) out[t] = v[k];
    }
  }
}
}  // namespace

hipError_t lanes_clouds_alloc(Lanes& L) {
  if (L.cl_h) return hipSuccess;
  const size_t tab = (size_t)kLaneClouds * (L.S + 1) * sizeof(uint64_t);
  hipError_t e = hipHostMalloc((void**)&L.cl_h, (size_t)2 * L.S * sizeof(int), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&L.cl_d, (size_t)2 * L.S * sizeof(int));
  if (e == hipSuccess) e = hipHostMalloc((void**)&L.cl_tab_h, tab, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&L.cl_tab_d, tab);
  if (e != hipSuccess) {
    if (L.cl_h) (void)hipHostFree(L.cl_h);
    if (L.cl_d) (void)hipFree(L.cl_d);
    if (L.cl_tab_h) (void)hipHostFree(L.cl_tab_h);
    if (L.cl_tab_d) (void)hipFree(L.cl_tab_d);
    L.cl_h = L.cl_d = nullptr;
    L.cl_tab_h = L.cl_tab_d = nullptr;
  }
  return e;
}

LanePackJob lanes_pack_job(const Lanes& L) {
  const SrBuffers& s = L.sr;
  const OdBuffers& o = L.od;
  const int buf = L.od_last;
  LanePackJob j;
  j.S = L.S;
  j.c[0] = {s.full, s.n_full, s.cap, 1};
  j.c[1] = {s.sharp, s.cnt + 0, kSharpPerRing * s.R, 4};
  j.c[2] = {s.lsharp, s.cnt + 1, kLessSharpPerRing * s.R, 4};
  j.c[3] = {s.flat, s.cnt + 2, kFlatPerRing * s.R, 4};
  j.c[4] = {s.lflat, s.cnt + 3, s.cap, 4};
  j.c[5] = {o.lastC + (size_t)buf * o.P * o.capC, o.nlast + buf * 2 + 0, o.capC, 2 * kOdBufs};
  j.c[6] = {o.lastS + (size_t)buf * o.P * o.capS, o.nlast + buf * 2 + 1, o.capS, 2 * kOdBufs};
  j.c[7] = {o.fullEnd + (size_t)buf * o.P * o.capS, o.nfullEnd + buf, o.capS, kOdBufs};
  j.c[8] = {L.mp.reg, L.mp.nreg, L.mp.capS, 1};
  return j;
}

hipError_t lanes_pack_offsets(const LanePackJob& job, const int* mask, const int* list, int n, uint64_t* table,
                              hipStream_t st) {
  if (n <= 0 || job.S <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_lanes_pack_offsets, dim3(1), dim3(kLanePackOffThreads), 0, st, job, mask, list, n, table);
  return hipGetLastError();
}

hipError_t lanes_pack(const LanePackJob& job, const uint64_t* table, const int* list, int n, int j0, int nj,
                      unsigned clouds, const LanePackDst& d, hipStream_t st) {
  if (n <= 0 || j0 < 0 || nj <= 0 || j0 + nj > n || n > LOAM_LANES_MAX) return hipErrorInvalidValue;
  LanePackSel sel;
  std::memset(&sel, 0, sizeof(sel));
  sel.n = n; sel.j0 = j0; sel.nj = nj; sel.S = job.S;
  int tiles = 0;
  for (int c = 0; c < kLaneClouds; ++c) {
    if (!(clouds >> c & 1)) continue;
    if (job.c[c].stride <= 0) return hipErrorInvalidValue;
    sel.tile0[sel.nc] = tiles;
    // (point 0 of the selection may lie in front of the buffer: the launch's first point is T[c][j0])
    float4* dst0 = (float4*)((intptr_t)d.dst[c] + (intptr_t)d.dbase[c] * (intptr_t)sizeof(float4));
    sel.w[sel.nc++] = {job.c[c].base, dst0, job.c[c].stride, c};
    tiles += (job.c[c].stride + kLanePackTile - 1) / kLanePackTile;
  }
  if (sel.nc == 0) return hipSuccess;
  for (int k = sel.nc; k <= kLaneClouds; ++k) sel.tile0[k] = tiles;
  const long long items = (long long)tiles * nj;
  if (items > 0x7fffffffLL) return hipErrorInvalidValue;  // (the kernel counts its work items in 32 bits)
  hipLaunchKernelGGL(k_lanes_pack, dim3((unsigned)std::min<long long>(items, kLanePackGridMax)), dim3(kLanePackThreads), 0, st,
                     sel, table, list);
  return hipGetLastError();
}

void lanes_free(Lanes& L) {
  lanes_imu_free(L);
  if (L.cl_h) (void)hipHostFree(L.cl_h);
  if (L.cl_d) (void)hipFree(L.cl_d);
  if (L.cl_tab_h) (void)hipHostFree(L.cl_tab_h);
  if (L.cl_tab_d) (void)hipFree(L.cl_tab_d);
  if (L.cl_done) (void)hipEventDestroy(L.cl_done);
  sr_free(L.sr);
  od_free(L.od);
  mp_free(L.mp);
  if (L.stage_h) (void)hipHostFree(L.stage_h);
  if (L.stage_d) (void)hipFree(L.stage_d);
  if (L.tab_h) (void)hipHostFree(L.tab_h);
  if (L.tab_d) (void)hipFree(L.tab_d);
  if (L.fd_h) (void)hipHostFree(L.fd_h);
  if (L.fd_d) (void)hipFree(L.fd_d);
  if (L.feed_wait) (void)hipEventDestroy(L.feed_wait);
  if (L.feed_release) (void)hipEventDestroy(L.feed_release);
  if (L.out_d) (void)hipFree(L.out_d);
  if (L.out_h) (void)hipHostFree(L.out_h);
  if (L.rs_h) (void)hipHostFree(L.rs_h);
  if (L.rs_d) (void)hipFree(L.rs_d);
  if (L.mi_h) (void)hipHostFree(L.mi_h);
  if (L.mi_d) (void)hipFree(L.mi_d);
  if (L.su_h) (void)hipHostFree(L.su_h);
  if (L.su_d) (void)hipFree(L.su_d);
  if (L.sp_h) (void)hipHostFree(L.sp_h);
  if (L.sp_d) (void)hipFree(L.sp_d);
  if (L.loc_h) (void)hipHostFree(L.loc_h);
  if (L.loc_d) (void)hipFree(L.loc_d);
  mp_commit_free(L.cm);
  L = Lanes();
}

hipError_t lanes_out(const Lanes& L, hipStream_t st, bool loc) {
  LaneOutSrc s;
  s.loc = loc ? L.loc_d : nullptr;
  s.sr_err = L.sr.err;
  s.od_state = L.od.state;
  s.od_istate = L.od.istate;
  s.mp_state = L.mp.state;
  s.mp_istate = L.mp.istate;
  s.nreg = L.mp.nreg;
  hipLaunchKernelGGL(k_lanes_out, dim3((L.S * 32 + 255) / 256), dim3(256), 0, st, s, L.out_d, L.S);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    e = hipMemcpyAsync(L.out_h, L.out_d, (size_t)L.S * kLaneOutWords * sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && loc)
    e = hipMemcpyAsync(L.loc_h, L.loc_d, (size_t)L.S * kLocResWords * sizeof(int), hipMemcpyDeviceToHost, st);
  return e;
}

}  // namespace loam
