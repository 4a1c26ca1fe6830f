// Laser mapping on gfx950: the laserMapping loop body (/root/reference/src/laserMapping.cpp:411-1097)
// for P independent map instances (the streaming map, or one per config-4 problem).
//
//  k_mp_prepare    pose prediction (transformAssociateToMap :110-197, fed through the nav_msgs
//                  quaternion round trip :304-321), cube-grid recentring (:440-614) as slot-table
//                  shifts, FOV cube selection (:616-672), FromMap prefix.
//  k_mp_stack      stack to map frame and back (:424-434, :683-691, Q24)
//  vg_run          segmented PCL VoxelGrid for the stacks (:693-701) and the valid cubes (:1018-1036): vg.hip
//  k_mp_gather     FromMap = valid cubes concatenated (:674-681), then voxel-hashed (k_hash_build)
//  k_mp_nnfit      one L-M iteration for every instance at once, lane per stack point: the exact
//                  5-NN (:714-719, :821-826) through the 1 m hash (any point within the 1 m acceptance
//                  radius lies in the 27 cells; cells pruned by box distance), the corner PCA with the
//                  3x3 Jacobi / surface 5x3 QR plane (reused while the ordered 5-NN is unchanged),
//                  weight -> accepted row (:721-877), and (fused) the fp64 JᵀJ / Jᵀb partials with
//                  the 6x6 step in the instance's last workgroup (:879-974)
//  k_mp_iter       the step as its own launch (tuning mp_fused_max)
//  k_mp_lm_small / k_mp_lm_stream   the same for a few instances / one (streaming)
//  k_mp_lm_end     transformUpdate (:199-232)
//  k_mp_insert     stack -> cubes in stack order (:980-1016)
//  k_mp_vcopy      per valid cube: old content ++ appended points -> DS input
//  k_mp_compact    new cube store (valid cubes downsampled, others appended) into the other pool
//  k_mp_register   full cloud to the map frame (:1060-1063)
//  k_mp_loc_prepare / k_mp_loc_gather / k_mp_loc_result   loam_map_localize: n candidate poses of one
//                  sweep as the instances of a second working set against the streaming store, which
//                  is only read (prepare without recentring, FromMap per candidate, the L-M as above)
//  k_mp_loc_prepare_rows / k_mp_loc_stack_rows   loam_lanes_localize: the same with every candidate's
//                  sweep and odometry pose read in place from a listed lane (a row -> lane plan)

#include <algorithm>
#include <functional>
#include <cstring>
#include <vector>

#include "dev_common.hpp"
#include "dev_hooks.h"
#include "mp.hpp"
#include "od.hpp"
#include "pose_math.hpp"

using namespace loamdev;

namespace loam {
#ifdef LOAM_PHASES
__device__ PhaseAcc g_ph_mp = {~0ull, 0ull, 0ull, {{0}}};
#endif


namespace {

constexpr int kMpThreads = 256;

LOAM_D int cube_of(float v, int cen) {  // :446-452, :983-989
  int c = (int)((D(v) + 25.0) / 50.0) + cen;
  if (D(v) + 25.0 < 0) c--;
  return c;
}
LOAM_D int cube_index(int i, int j, int k) { return i + kCubeW * j + kCubeW * kCubeH * k; }

LOAM_D int* slot_table(const MpBuffers& b, int pool, int p) {
  return b.slots + ((size_t)pool * b.P + p) * kCubeNum * 4;
}

// ---------------------------------------------------------------- prepare
// sin / cos of the TobeMapped rotation in double (pointAssociateToMap, :240-257), kept per instance
// in b.rot beside the state: written wherever transformTobeMapped changes (prepare, each L-M
// step, the IMU blend), read by every kernel that maps points.  Per thread they were six double
// sin / cos calls, the larger part of the 5-NN kernel's instructions.
LOAM_D void rot_store(const MpBuffers& b, int p, const float* T) {
  const loampose::MapRot r = loampose::map_rot(T);
  double* d = b.rot + (size_t)p * 6;
  d[0] = r.c0; d[1] = r.s0; d[2] = r.c1; d[3] = r.s1; d[4] = r.c2; d[5] = r.s2;
}
LOAM_D loampose::MapRot rot_load(const MpBuffers& b, int p) {
  const double* d = b.rot + (size_t)p * 6;
  const float* T = b.state + (size_t)p * kMpStateFloats + kMpTobe;
  loampose::MapRot r;
  r.c0 = d[0]; r.s0 = d[1]; r.c1 = d[2]; r.s1 = d[3]; r.c2 = d[4]; r.s2 = d[5];
  r.t3 = T[3]; r.t4 = T[4]; r.t5 = T[5];
  return r;
}

// one thread: the frame's pose prediction for instance p (the odometry pose through the message
// round trip, transformAssociateToMap with the instance's Bef / Aft, :110-197), its rotation and
// the point on the Y axis of the FOV test (:616-622)
LOAM_D void prepare_pose(const MpBuffers& b, const MpInput& in, int p) {
  float* st = b.state + (size_t)p * kMpStateFloats;
  float pose[6] = {0, 0, 0, 0, 0, 0};
  if (in.pose)
    for (int k = 0; k < 6; ++k) pose[k] = in.pose[(size_t)p * in.pose_stride + k];
  loampose::pose_through_msg(pose, st + kMpSum);
  loampose::associate_to_map(st + kMpSum, st + kMpBef, st + kMpAft, st + kMpIncre, st + kMpTobe);
  const float* T = st + kMpTobe;
  const loampose::MapRot r = loampose::map_rot(T);
  rot_store(b, p, T);
  const float4 onY = loampose::point_to_map(r, make_float4(0.0f, 10.0f, 0.0f, 0.0f));
  st[kMpOnY] = onY.x; st[kMpOnY + 1] = onY.y; st[kMpOnY + 2] = onY.z;
}

// thread tid < 125: cube tid of the 5x5x5 neighbourhood of the centre cube (cI, cJ, cK) in the
// reference's i, j, k loop order: inside the grid and in the field of view (:624-672)?  ind: its index
LOAM_D bool fov_cube(const float* st, int tid, int cI, int cJ, int cK, int cW, int cH, int cD, int& ind) {
  const float* T = st + kMpTobe;
  bool inFOV = false;
  ind = 0;
  if (tid < 125) {
    const int i = cI - 2 + tid / 25, j = cJ - 2 + (tid / 5) % 5, k = cK - 2 + tid % 5;
    if (i >= 0 && i < kCubeW && j >= 0 && j < kCubeH && k >= 0 && k < kCubeD) {
      const float ox = st[kMpOnY], oy = st[kMpOnY + 1], oz = st[kMpOnY + 2];
      const float centerX = (float)(50.0 * (i - cW));
      const float centerY = (float)(50.0 * (j - cH));
      const float centerZ = (float)(50.0 * (k - cD));
      for (int ii = -1; ii <= 1; ii += 2)
        for (int jj = -1; jj <= 1; jj += 2)
          for (int kk = -1; kk <= 1; kk += 2) {
            const float cornerX = (float)(D(centerX) + 25.0 * ii);
            const float cornerY = (float)(D(centerY) + 25.0 * jj);
            const float cornerZ = (float)(D(centerZ) + 25.0 * kk);
            const float sq1 = (T[3] - cornerX) * (T[3] - cornerX) + (T[4] - cornerY) * (T[4] - cornerY) +
                              (T[5] - cornerZ) * (T[5] - cornerZ);
            const float sq2 = (ox - cornerX) * (ox - cornerX) + (oy - cornerY) * (oy - cornerY) +
                              (oz - cornerZ) * (oz - cornerZ);
            const float check1 = (float)(100.0 + D(sq1) - D(sq2) - 10.0 * sqrt(3.0) * sqrt(D(sq1)));
            const float check2 = (float)(100.0 + D(sq1) - D(sq2) + 10.0 * sqrt(3.0) * sqrt(D(sq1)));
            if (check1 < 0 && check2 > 0) inFOV = true;
          }
      ind = cube_index(i, j, k);
    }
  }
  return inFOV;
}

__global__ __launch_bounds__(kMpThreads) void k_mp_prepare(MpBuffers b, MpInput in) {
  const int p = blockIdx.x, tid = threadIdx.x;
  float* st = b.state + (size_t)p * kMpStateFloats;
  int* ist = b.istate + (size_t)p * kMpStateInts;
  int* slots = slot_table(b, b.pool_cur, p);
  __shared__ int sh_shift[3], sh_count[3];
  __shared__ int sh_nshift, sh_c[3], sh_cen[3], sh_scan[16];
  if (tid == 0) {
    prepare_pose(b, in, p);
    const float* T = st + kMpTobe;
    int cW = ist[kMiCenW], cH = ist[kMiCenH], cD = ist[kMiCenD];
    int cI = cube_of(T[3], cW), cJ = cube_of(T[4], cH), cK = cube_of(T[5], cD);
    // :454-614: each `while` moves the grid one slab per pass until the centre cube is >= 3 from
    // the edge.  The pass counts are closed-form; a line of cubes shifted by its full length (or
    // more) is entirely cleared, so at most that many slot-table shifts are replayed per axis
    // while the centre indices take every pass (ist[kMiShifts] counts the reference's passes).
    const int dim[3] = {kCubeW, kCubeH, kCubeD};
    int* c[3] = {&cI, &cJ, &cK};
    int* cen[3] = {&cW, &cH, &cD};
    int n = 0;
    long long passes = 0;
    for (int axis = 0; axis < 3; ++axis) {
      long long up = 0, down = 0;
      if (*c[axis] < 3) up = 3 - (long long)*c[axis];
      else if (*c[axis] >= dim[axis] - 3) down = (long long)*c[axis] - (dim[axis] - 4);
      const long long moves = up ? up : down;
      if (moves) {
        *c[axis] += (int)(up - down);
        *cen[axis] += (int)(up - down);
        sh_shift[n] = axis * 2 + (up ? 1 : 0);
        sh_count[n] = (int)(moves < dim[axis] ? moves : dim[axis]);
        ++n;
        passes += moves;
      }
    }
    ist[kMiShifts] = (int)(passes < 0x7fffffff ? passes : 0x7fffffff);
    sh_nshift = n;
    sh_c[0] = cI; sh_c[1] = cJ; sh_c[2] = cK;
    ist[kMiCubeI] = cI; ist[kMiCubeJ] = cJ; ist[kMiCubeK] = cK;
    ist[kMiCenW] = cW; ist[kMiCenH] = cH; ist[kMiCenD] = cD;
    sh_cen[0] = cW; sh_cen[1] = cH; sh_cen[2] = cD;
  }
  __syncthreads();
  for (int s = 0; s < sh_nshift; ++s)
  for (int rep = 0; rep < sh_count[s]; ++rep) {  // slot-table shifts: the cleared cube wraps around
    const int axis = sh_shift[s] >> 1, up = sh_shift[s] & 1;
    const int nAx = axis == 0 ? kCubeW : (axis == 1 ? kCubeH : kCubeD);
    const int na = axis == 0 ? kCubeH : kCubeW, nb = axis == 2 ? kCubeH : kCubeD;
    for (int line = tid; line < na * nb; line += kMpThreads) {
      const int a = line % na, bb = line / na;
      auto at = [&](int c) {
        if (axis == 0) return cube_index(c, a, bb);
        if (axis == 1) return cube_index(a, c, bb);
        return cube_index(a, bb, c);
      };
      int4* sl = (int4*)slots;
      if (up) {
        int4 keep = sl[at(nAx - 1)];
        for (int c = nAx - 1; c >= 1; --c) sl[at(c)] = sl[at(c - 1)];
        keep.y = 0; keep.w = 0;
        sl[at(0)] = keep;
      } else {
        int4 keep = sl[at(0)];
        for (int c = 0; c < nAx - 1; ++c) sl[at(c)] = sl[at(c + 1)];
        keep.y = 0; keep.w = 0;
        sl[at(nAx - 1)] = keep;
      }
    }
    __threadfence_block();  // (one workgroup: the next shift's lines are other threads')
    __syncthreads();
  }
  // FOV selection (:616-672) and FromMap prefix: thread c tests cube c of the 5x5x5
  // neighbourhood (the reference's i, j, k loop order), block scans keep that order
  int ind;
  const bool inFOV = fov_cube(st, tid, sh_c[0], sh_c[1], sh_c[2], sh_cen[0], sh_cen[1], sh_cen[2], ind);
  const int nC = inFOV ? slots[ind * 4 + 1] : 0, nS = inFOV ? slots[ind * 4 + 3] : 0;
  int nv, accC, accS;
  const int xv = block_excl_scan<kMpThreads>(inFOV ? 1 : 0, sh_scan, nv);
  const int xc = block_excl_scan<kMpThreads>(nC, sh_scan, accC);
  const int xs = block_excl_scan<kMpThreads>(nS, sh_scan, accS);
  int* vp = b.vpre + (size_t)p * (kMaxValid + 1) * 2;
  if (inFOV) {
    b.valid[(size_t)p * kMaxValid + xv] = ind;
    vp[xv * 2 + 0] = xc;
    vp[xv * 2 + 1] = xs;
  }
  if (tid == 0) {
    vp[nv * 2 + 0] = accC;
    vp[nv * 2 + 1] = accS;
    ist[kMiNValid] = nv;
    if (accC + accS > b.map_cap) {
      ist[kMiErr] |= ERR_CAP_MAP;
      accC = accS = 0;
      ist[kMiNValid] = 0;
    }
    b.nfrom[p * 2 + 0] = accC;
    b.nfrom[p * 2 + 1] = accS;
  }
}

// ---------------------------------------------------------------- localization (loam_map_localize)
// what the localization kernels read of the streaming store (instance 0's current pool)
struct LocStore {
  const int* slots;     // [kCubeNum][4] (offC, cntC, offS, cntS)
  const float4* pool;
  const int* istate;    // the store's instance state (grid centre, error word)
  int map_cap;
};

// The read-only half of k_mp_prepare for candidate p = blockIdx.x of the working set w: the
// candidate's Bef / Aft (cand: aft then bef) instead of a kept state, the grid centre of the shared
// store, no recentring — a candidate whose centre cube is within 3 of a grid edge (the condition
// of the reference's `while` loops, :454-614) is marked kMiLocOff and gets an empty valid set —
// then the FOV cube selection and the FromMap prefix from the shared slot table.  Writes w only;
// head: every candidate's FromMap counts and the store's error word, for the host.
//
// kLanes (shared lanes, mp_lanes_shared_frame): instance p is a lane whose Bef / Aft are its kept
// state (cand and head are null) and whose IMU flag k_lanes_imu has set for this frame.  The host
// reads no count before the gather, so the guard is the working set's: a lane whose valid cubes hold
// more than w.map_cap points, and every lane when the store's last update overflowed, gets
// ERR_CAP_MAP and an empty valid set (nothing is gathered, no L-M runs, the poses stay).
template <bool kLanes>
LOAM_D void loc_prepare(const MpBuffers& w, const MpInput& in, const LocStore& s, const float* cand, int* head) {
  const int p = blockIdx.x, tid = threadIdx.x;
  float* st = w.state + (size_t)p * kMpStateFloats;
  int* ist = w.istate + (size_t)p * kMpStateInts;
  __shared__ int sh_c[3], sh_cen[3], sh_off, sh_scan[16];
  if (tid == 0) {
    if (!kLanes)
      for (int k = 0; k < 6; ++k) {
        st[kMpAft + k] = cand[(size_t)p * 12 + k];
        st[kMpBef + k] = cand[(size_t)p * 12 + 6 + k];
      }
    prepare_pose(w, in, p);
    const float* T = st + kMpTobe;
    const int cW = s.istate[kMiCenW], cH = s.istate[kMiCenH], cD = s.istate[kMiCenD];
    const int cI = cube_of(T[3], cW), cJ = cube_of(T[4], cH), cK = cube_of(T[5], cD);
    sh_off = cI < 3 || cI >= kCubeW - 3 || cJ < 3 || cJ >= kCubeH - 3 || cK < 3 || cK >= kCubeD - 3;
    sh_c[0] = cI; sh_c[1] = cJ; sh_c[2] = cK;
    sh_cen[0] = cW; sh_cen[1] = cH; sh_cen[2] = cD;
    ist[kMiCubeI] = cI; ist[kMiCubeJ] = cJ; ist[kMiCubeK] = cK;
    ist[kMiCenW] = cW; ist[kMiCenH] = cH; ist[kMiCenD] = cD;
    ist[kMiShifts] = 0;
    ist[kMiErr] = 0;
    if (!kLanes) ist[kMiImu] = 0;  // (no IMU message: transformUpdate without the blend)
    ist[kMiDegen] = 0;
    ist[kMiLocOff] = sh_off;
    if (!kLanes && p == 0) head[2 * gridDim.x] = s.istate[kMiErr];
  }
  __syncthreads();
  int ind = 0;
  const bool inFOV = !sh_off && fov_cube(st, tid, sh_c[0], sh_c[1], sh_c[2], sh_cen[0], sh_cen[1], sh_cen[2], ind);
  const int nC = inFOV ? s.slots[ind * 4 + 1] : 0, nS = inFOV ? s.slots[ind * 4 + 3] : 0;
  int nv, accC, accS;
  const int xv = block_excl_scan<kMpThreads>(inFOV ? 1 : 0, sh_scan, nv);
  const int xc = block_excl_scan<kMpThreads>(nC, sh_scan, accC);
  const int xs = block_excl_scan<kMpThreads>(nS, sh_scan, accS);
  int* vp = w.vpre + (size_t)p * (kMaxValid + 1) * 2;
  if (inFOV) {
    w.valid[(size_t)p * kMaxValid + xv] = ind;
    vp[xv * 2 + 0] = xc;
    vp[xv * 2 + 1] = xs;
  }
  if (tid == 0) {
    bool over = accC + accS > s.map_cap;  // (k_mp_prepare's guard; a valid store never holds more)
    if (kLanes) over = over || accC + accS > w.map_cap || (s.istate[kMiErr] & ERR_CAP_MAP) != 0;
    if (over) {
      ist[kMiErr] |= ERR_CAP_MAP;
      accC = accS = 0;
      nv = 0;
    }
    vp[nv * 2 + 0] = accC;
    vp[nv * 2 + 1] = accS;
    ist[kMiNValid] = nv;
    w.nfrom[p * 2 + 0] = accC;
    w.nfrom[p * 2 + 1] = accS;
    if (!kLanes) {
      head[p * 2 + 0] = accC;
      head[p * 2 + 1] = accS;
    }
  }
}
template <bool kLanes>
__global__ __launch_bounds__(kMpThreads) void k_mp_loc_prepare(MpBuffers w, MpInput in, LocStore s,
                                                                const float* cand, int* head) {
  loc_prepare<kLanes>(w, in, s, cand, head);
}
// The rows form (loam_lanes_localize): candidate p = blockIdx.x of gridDim.x = n k rows is row p % k
// of listed lane p / k < n (rows.plan has n entries).  Bef / Aft come from the candidate table as
// <false> takes them; the odometry pose of prepare_pose is the transformSum of the row's lane, read
// in place from the lanes' odometry state (plan.lane < the lanes open: lanes_localize_plan).
__global__ __launch_bounds__(kMpThreads) void k_mp_loc_prepare_rows(MpBuffers w, LocStore s, const float* cand,
                                                                     int* head, LocRows rows) {
  const LaneLocPlan& e = rows.plan[blockIdx.x / rows.k];
  MpInput in;
  in.corner = in.surf = in.full = nullptr;
  in.corner_stride = in.surf_stride = in.full_stride = 0;
  in.ncorner = in.nsurf = in.nfull = nullptr;
  in.ncorner_stride = in.nsurf_stride = in.nfull_stride = 0;
  in.pose = rows.od_state + (size_t)e.lane * kOdStateFloats + kOdSum;
  in.pose_stride = 0;
  loc_prepare<false>(w, in, s, cand, head);
}

// FromMap of every candidate (blockIdx.y) from the shared pool: its valid cubes' corner points,
// then their surf points, cubes in valid order and points in store order (k_mp_gather's order).
// The candidate's runs (2 per valid cube: output offset, pool offset) are held in LDS; output
// point i finds its run by a fixed-step search (as k_mp_map_pack), four points per lane with all
// four loads issued before the stores, the stores fully coalesced.  The shared cubes are read by
// many candidates (L2).
constexpr int kLocRuns = 256;  // >= 2 * kMaxValid, a power of two (the search's steps)
static_assert(kLocRuns >= 2 * kMaxValid, "a candidate's runs");
__global__ __launch_bounds__(256) void k_mp_loc_gather(MpBuffers w, LocStore s) {
  const int p = blockIdx.y, tid = threadIdx.x;
  const int nv = w.istate[(size_t)p * kMpStateInts + kMiNValid];
  const int* vp = w.vpre + (size_t)p * (kMaxValid + 1) * 2;
  const int totC = vp[nv * 2 + 0], total = totC + vp[nv * 2 + 1];
  if (total <= 0 || total > w.map_cap || blockIdx.x * 1024 >= total) return;  // (uniform)
  __shared__ int off[kLocRuns], src[kLocRuns];
  {  // run tid: kind tid / nv, valid cube tid % nv; beyond 2 nv: never chosen
    const bool live = tid < 2 * nv;
    const int kind = live && tid >= nv ? 1 : 0, c = live ? tid - kind * nv : 0;
    const int ind = live ? w.valid[(size_t)p * kMaxValid + c] : 0;
    off[tid] = live ? kind * totC + vp[c * 2 + kind] : 0x7fffffff;
    src[tid] = live ? s.slots[ind * 4 + 2 * kind] : 0;
  }
  __syncthreads();
  float4* dst = w.from + (size_t)p * w.map_cap;
  for (int base = blockIdx.x * 1024; base < total; base += gridDim.x * 1024) {
    // the pool index of output point i (clamped: the lanes past the end load a valid point)
    auto locate = [&](int i) {
      i = min(i, total - 1);
      int lo = 0;  // the last run whose offset is <= i (an empty run never is the last such)
#pragma unroll
      for (int step = kLocRuns / 2; step > 0; step >>= 1)
        if (off[lo + step] <= i) lo += step;
      return src[lo] + (i - off[lo]);
    };
    const int i0 = base + tid, i1 = i0 + 256, i2 = i0 + 512, i3 = i0 + 768;
    const int a0 = locate(i0), a1 = locate(i1), a2 = locate(i2), a3 = locate(i3);
    const float4 v0 = s.pool[a0], v1 = s.pool[a1], v2 = s.pool[a2], v3 = s.pool[a3];
    if (i0 < total) dst[i0] = v0;
    if (i1 < total) dst[i1] = v1;
    if (i2 < total) dst[i2] = v2;
    if (i3 < total) dst[i3] = v3;
  }
}

// ---------------------------------------------------------------- stacks
// instance p's stacks from its two clouds (nc / ns points, clamped to capC / capS by the caller):
// every point to the map frame and back (:424-434, :683-691), corner at 0, surf at capC of the
// instance's cap_stack segment; then the segment words of the stacks' VoxelGrid.  over(): a count as
// given exceeds its capacity (ERR_CAP_STACK; asked by the one thread that writes the words)
template <class Over>
LOAM_D void stack_body(const MpBuffers& b, int p, const float4* corner, const float4* surf, int nc, int ns, Over over) {
  const loampose::MapRot r = rot_load(b, p);
  float4* out = b.stack2 + (size_t)p * b.cap_stack;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nc + ns; i += gridDim.x * 256) {
    const float4 a = i < nc ? corner[i] : surf[i - nc];
    const float4 m = loampose::point_to_map(r, a);
    out[i < nc ? i : b.capC + (i - nc)] = loampose::point_to_tobe_mapped(r, m);
  }
  if (p == 0 && blockIdx.x == 0 && threadIdx.x == 0) { b.vg.counts[0] = 0; b.vg.counts[1] = 0; }  // (vg_stack's lists)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const size_t base = (size_t)p * b.cap_stack;
    b.sseg_b[p * 2 + 0] = (int)base;
    b.sseg_e[p * 2 + 0] = (int)base + nc;
    b.sseg_b[p * 2 + 1] = (int)(base + b.capC);
    b.sseg_e[p * 2 + 1] = (int)(base + b.capC) + ns;
    b.sseg_leaf[p * 2 + 0] = 0.2f;
    b.sseg_leaf[p * 2 + 1] = 0.4f;
    if (over()) b.istate[(size_t)p * kMpStateInts + kMiErr] |= ERR_CAP_STACK;
  }
}

__global__ __launch_bounds__(256) void k_mp_stack(MpBuffers b, MpInput in) {
  const int p = blockIdx.y;
  const int nc = min(in.ncorner[p * in.ncorner_stride], b.capC);
  const int ns = min(in.nsurf[p * in.nsurf_stride], b.capS);
  stack_body(b, p, in.corner + (size_t)p * in.corner_stride, in.surf + (size_t)p * in.surf_stride, nc, ns, [&] {
    return in.ncorner[p * in.ncorner_stride] > b.capC || in.nsurf[p * in.nsurf_stride] > b.capS;
  });
}

// k_mp_stack for the rows of loam_lanes_localize: instance p = blockIdx.y of gridDim.y = n k rows
// takes the Last clouds of listed lane p / k < n (rows.plan has n entries) in place.  The plan's
// offsets lie inside [kOdBufs][lanes][cap] and its counts inside the lanes' capacities
// (lanes_localize_plan); they are clamped to the working set's capC / capS as k_mp_stack clamps its
// counts, so nothing is read past a lane's cloud or written past the row's segment.  No workgroup
// waits for another.
__global__ __launch_bounds__(256) void k_mp_loc_stack_rows(MpBuffers b, LocRows rows) {
  const int p = blockIdx.y;
  const LaneLocPlan& e = rows.plan[p / rows.k];
  stack_body(b, p, rows.lastC + e.offC, rows.lastS + e.offS, min(e.nC, b.capC), min(e.nS, b.capS),
             [&] { return e.nC > b.capC || e.nS > b.capS; });
}

// ---------------------------------------------------------------- FromMap gather
__global__ __launch_bounds__(256) void k_mp_gather(MpBuffers b) {
  const int p = blockIdx.y;
  const int nv = b.istate[(size_t)p * kMpStateInts + kMiNValid];
  const int* vp = b.vpre + (size_t)p * (kMaxValid + 1) * 2;
  const int* slots = slot_table(b, b.pool_cur, p);
  const float4* pool = b.pool + ((size_t)b.pool_cur * b.P + p) * b.map_cap;
  const int totC = vp[nv * 2 + 0], totS = vp[nv * 2 + 1];
  float4* out = b.from + (size_t)p * b.map_cap;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < totC + totS; i += gridDim.x * 256) {
    const int kind = i < totC ? 0 : 1;
    const int t = kind ? i - totC : i;
    int lo = 0, hi = nv - 1;   // last valid cube with prefix <= t
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (vp[mid * 2 + kind] <= t) lo = mid; else hi = mid - 1;
    }
    const int ind = b.valid[(size_t)p * kMaxValid + lo];
    out[i] = pool[slots[ind * 4 + 2 * kind] + (t - vp[lo * 2 + kind])];
  }
}

// ---------------------------------------------------------------- L-M
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
__constant__ int kCellOrder[27] = {13, 4, 10, 12, 14, 16, 22, 1, 3, 5, 7, 9, 11, 15, 17, 19, 21, 23, 25,
                                   0, 2, 6, 8, 18, 20, 24, 26};

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


}  // namespace

__global__ void k_mp_lm_begin(MpBuffers b) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= b.P) return;
  int* ist = b.istate + (size_t)p * kMpStateInts;
  const int nfc = b.nfrom[p * 2 + 0], nfs = b.nfrom[p * 2 + 1];
  ist[kMiStackC] = b.sseg_cnt[p * 2 + 0];
  ist[kMiStackS] = b.sseg_cnt[p * 2 + 1];
  ist[kMiFromC] = nfc;
  ist[kMiFromS] = nfs;
  ist[kMiLmRan] = (nfc > 10 && nfs > 100) ? 1 : 0;  // :706
  ist[kMiStop] = 0;
  ist[kMiIters] = 0;
  ist[kMiRows] = 0;
  ist[kMiRowsLast] = 0;
  ist[kMiFits] = 0;
  ist[kMiDegSteps] = 0;
  ist[kMiNnCand] = 0;
  ist[kMiNnCells] = 0;
  if (p == 0 && b.P == 1) ++b.ls_epoch[0];  // (k_mp_lm_stream's publication words)
}

// One L-M iteration's correspondences (:714-877), lane per stack point (corner, then surf), in
// per-query pieces shared by the batch kernel (k_mp_nnfit) and the small-batch / streaming kernels
// (k_mp_lm_small, k_mp_lm_stream).
//   mp_nn_query   the point at the current TobeMapped pose and its exact 5-NN (seeded with the
//                 previous iteration's), stored in q_nn
//   mp_fit_query  the line (corner PCA, 3x3 Jacobi) or plane (5x3 QR) through the 5 neighbours and
//                 the weighted residual.  A fit depends on nothing but the ordered 5 neighbours, so
//                 it is kept per query and reused while the ordered 5-NN is unchanged from the
//                 previous iteration (bit-identical to refitting)
//   mp_row_accum  the accepted row's J (:897-921) added in fp64
//   mp_step       the 6x6 step on the summed normal equations (:922-974)
namespace {
// the ordered 5-NN a fit was made for, and the fit: corner (x1, y1, z1, valid), (x2, y2, z2, -);
// surf (pa, pb, pc, pd), (valid, -, -, -)
struct MpFit {
  int4 n0, n1;
  float4 g0, g1;
};

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

// the line (corner: PCA of the 5 neighbours, 3x3 Jacobi, :721-760) or plane (surf: 5x3 QR, :828-850)
// through the ordered 5-NN points nb; jw: this lane's 27 words of LDS scratch for the Jacobi
LOAM_D void mp_fit_compute(bool corner, const float4 (&nb)[5], float* jw, float4& g0, float4& g1) {
  if (corner) {  // :721-760
    float cx = 0, cy = 0, cz = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) { cx += nb[k].x; cy += nb[k].y; cz += nb[k].z; }
    cx /= 5; cy /= 5; cz /= 5;
    float a11 = 0, a12 = 0, a13 = 0, a22 = 0, a23 = 0, a33 = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const float ax = nb[k].x - cx, ay = nb[k].y - cy, az = nb[k].z - cz;
      a11 += ax * ax; a12 += ax * ay; a13 += ax * az;
      a22 += ay * ay; a23 += ay * az; a33 += az * az;
    }
    a11 /= 5; a12 /= 5; a13 /= 5; a22 /= 5; a23 /= 5; a33 /= 5;
    (void)jw;
    const float A1[9] = {a11, a12, a13, a12, a22, a23, a13, a23, a33};
    float D1[3], V1[9];
    loamla::jacobi3_reg(A1, D1, V1);  // (bit-identical to jacobi<3>: tests/test_jacobi3.py)
    const bool valid = D1[0] > 3 * D1[1];
    g0 = make_float4((float)(D(cx) + 0.1 * D(V1[0])), (float)(D(cy) + 0.1 * D(V1[1])),
                     (float)(D(cz) + 0.1 * D(V1[2])), valid ? 1.0f : 0.0f);
    g1 = make_float4((float)(D(cx) - 0.1 * D(V1[0])), (float)(D(cy) - 0.1 * D(V1[1])),
                     (float)(D(cz) - 0.1 * D(V1[2])), 0.0f);
  } else {  // :828-850
    float A0[15], B0[5] = {-1, -1, -1, -1, -1}, X0[3], ws[14];
#pragma unroll
    for (int k = 0; k < 5; ++k) { A0[k * 3 + 0] = nb[k].x; A0[k * 3 + 1] = nb[k].y; A0[k * 3 + 2] = nb[k].z; }
    loamla::qr_solve(A0, B0, 5, 3, X0, ws);
    float pa = X0[0], pb = X0[1], pc = X0[2], pd = 1;
    const float ps = (float)sqrt(D(pa * pa + pb * pb + pc * pc));
    pa /= ps; pb /= ps; pc /= ps; pd /= ps;
    bool planeValid = true;
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (fabs(D(pa * nb[k].x + pb * nb[k].y + pc * nb[k].z + pd)) > 0.2) planeValid = false;
    g0 = make_float4(pa, pb, pc, pd);
    g1 = make_float4(planeValid ? 1.0f : 0.0f, 0.0f, 0.0f, 0.0f);
  }
}

// the weighted residual of the mapped point sel against a fit (:762-816 corner, :852-874 surf)
LOAM_D void mp_fit_residual(bool corner, float4 g0, float4 g1, float4 sel, float4& cf, int& ok) {
  ok = 0;
  cf = make_float4(0, 0, 0, 0);
  if (corner && g0.w != 0.0f) {  // :762-816
    const float x0 = sel.x, y0 = sel.y, z0 = sel.z;
    const float x1 = g0.x, y1 = g0.y, z1 = g0.z, x2 = g1.x, y2 = g1.y, z2 = g1.z;
    const float m11 = (x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1);
    const float m22 = (x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1);
    const float m33 = (y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1);
    const float a012 = (float)sqrt(D(m11 * m11 + m22 * m22 + m33 * m33));
    const float l12 = (float)sqrt(D((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2)));
    const float la = ((y1 - y2) * m11 + (z1 - z2) * m22) / a012 / l12;
    const float lb = -((x1 - x2) * m11 - (z1 - z2) * m33) / a012 / l12;
    const float lc = -((x1 - x2) * m22 + (y1 - y2) * m33) / a012 / l12;
    const float ld2 = a012 / l12;
    const float sw = (float)(1 - 0.9 * fabs(D(ld2)));
    cf = make_float4(sw * la, sw * lb, sw * lc, sw * ld2);
    ok = D(sw) > 0.1 ? 1 : 0;
  } else if (!corner && g1.x != 0.0f) {  // :852-874
    const float pa = g0.x, pb = g0.y, pc = g0.z, pd = g0.w;
    const float pd2 = pa * sel.x + pb * sel.y + pc * sel.z + pd;
    const float sw = (float)(1 - 0.9 * fabs(D(pd2)) / sqrt(sqrt(D(sel.x * sel.x + sel.y * sel.y + sel.z * sel.z))));
    cf = make_float4(sw * pa, sw * pb, sw * pc, sw * pd2);
    ok = D(sw) > 0.1 ? 1 : 0;
  }
}

// jw: this lane's 27 words of LDS scratch for the 3x3 Jacobi
LOAM_D void mp_fit_query(const MpBuffers& b, int p, int q, int nsc, bool first, int4 n0, int4 n1, float4 sel,
                         float* jw, int& nfits, float4& cf, int& ok) {
  const bool corner = q < nsc;
  const int nfc = b.nfrom[p * 2 + 0];
  const float4* from = b.from + (size_t)p * b.map_cap + (corner ? 0 : nfc);
  MpFit* qfit = (MpFit*)b.q_fit + (size_t)p * b.cap_stack;
  ok = 0;
  cf = make_float4(0, 0, 0, 0);
  if (n1.x != 0x7fffffff && D(__int_as_float(n1.y)) < 1.0) {  // :719, :826
    MpFit f = qfit[q];
    if (first || f.n0.x != n0.x || f.n0.y != n0.y || f.n0.z != n0.z || f.n0.w != n0.w || f.n1.x != n1.x) {
      ++nfits;
      const int idx[5] = {n0.x, n0.y, n0.z, n0.w, n1.x};
      float4 nb[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        LOAM_CHECK(idx[k] >= 0 && idx[k] < (corner ? nfc : b.nfrom[p * 2 + 1]), idx[k], q);
        nb[k] = from[idx[k]];
      }
      f.n0 = n0;
      f.n1 = make_int4(n1.x, 0, 0, 0);
      mp_fit_compute(corner, nb, jw, f.g0, f.g1);
      qfit[q] = f;
    }
    mp_fit_residual(corner, f.g0, f.g1, sel, cf, ok);
  } else if (first) {
    // no fit this iteration: drop a fit left by an earlier frame (whose map indices name other
    // points) so that a later iteration cannot take it for this frame's
    qfit[q].n0 = make_int4(-1, -1, -1, -1);
  }
}

// sin / cos of the TobeMapped rotation for the rows
struct MpTrig {
  float srx, crx, sry, cry, srz, crz;
};
LOAM_D MpTrig mp_trig_of(const float* trig) { return {trig[0], trig[1], trig[2], trig[3], trig[4], trig[5]}; }
// the same values from the stored rotation (rot_store: dsin / dcos of the same TobeMapped angles),
// without the serial double sin / cos in the kernel prologue
LOAM_D MpTrig mp_trig_of(const loampose::MapRot& r) {
  return {(float)r.s0, (float)r.c0, (float)r.s1, (float)r.c1, (float)r.s2, (float)r.c2};
}

// The six values as one place in a loop sees them: the products of them that mp_row_jac forms
// are the same for every query, and the compiler would otherwise keep each in a vector register
// across the whole loop over the queries (k_mp_nnfit has none to spare); so they are formed
// where they are used
LOAM_D MpTrig mp_trig_here(MpTrig t) {
  asm volatile("" : "+v"(t.srx), "+v"(t.crx), "+v"(t.sry), "+v"(t.cry), "+v"(t.srz), "+v"(t.crz));
  return t;
}

// the accepted row's J (:897-921): a[0..5] and b = -coefficient.w
LOAM_D void mp_row_jac(const MpTrig& tg, float4 o, float4 c, float (&a)[6], float& bb) {
  const float srx = tg.srx, crx = tg.crx, sry = tg.sry, cry = tg.cry, srz = tg.srz, crz = tg.crz;
  a[0] = (crx * sry * srz * o.x + crx * crz * sry * o.y - srx * sry * o.z) * c.x +
         (-srx * srz * o.x - crz * srx * o.y - crx * o.z) * c.y +
         (crx * cry * srz * o.x + crx * cry * crz * o.y - cry * srx * o.z) * c.z;
  a[1] = ((cry * srx * srz - crz * sry) * o.x + (sry * srz + cry * crz * srx) * o.y + crx * cry * o.z) * c.x +
         ((-cry * crz - srx * sry * srz) * o.x + (cry * srz - crz * srx * sry) * o.y - crx * sry * o.z) * c.z;
  a[2] = ((crz * srx * sry - cry * srz) * o.x + (-cry * crz - srx * sry * srz) * o.y) * c.x +
         (crx * crz * o.x - crx * srz * o.y) * c.y +
         ((sry * srz + cry * crz * srx) * o.x + (crz * sry - cry * srx * srz) * o.y) * c.z;
  a[3] = c.x;
  a[4] = c.y;
  a[5] = c.z;
  bb = -c.w;
}

LOAM_D void mp_row_accum(const MpTrig& tg, float4 o, float4 c, double (&acc)[28]) {
  float a[6], bb;
  mp_row_jac(tg, o, c, a, bb);
  int k = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int jj = i; jj < 6; ++jj) { acc[k] = loamla::dmac(acc[k], a[i], a[jj]); ++k; }
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[21 + i] = loamla::dmac(acc[21 + i], a[i], bb);
  acc[27] += 1.0;
}

struct MpStepScratch {
  float lm_ws[loamla::kLmWs];
  int lm_iws[12];
  float AtA[36], AtB[6], X[6];
  float jE[6], jV[36];  // iteration 0: jacobi6_wave's eigen decomposition of AtA
};

// the first wave of the workgroup (the iteration-0 eigen decomposition, jacobi6_wave), the rest on
// lane 0: iteration bookkeeping, the 6x6 step when there are >= 50 rows (:886-889), the update (no
// NaN guard in mapping, :956-961) and the convergence test (:972)
LOAM_D void mp_step(const MpBuffers& b, int p, const double* tot, MpStepScratch& sh) {
  const int lane = lane_id();
  int* ist = b.istate + (size_t)p * kMpStateInts;
  float* st = b.state + (size_t)p * kMpStateFloats;
  const int iter = ist[kMiIters];
  const int nrows = (int)tot[27];
  // lane 0's global reads of the step, issued together up front (round trips on the serial chain)
  int c_rows = 0, degen = 0, c_deg = 0;
  float T[6] = {0, 0, 0, 0, 0, 0};
  if (lane == 0) {
    c_rows = ist[kMiRows];
    degen = ist[kMiDegen];
    c_deg = ist[kMiDegSteps];
#pragma unroll
    for (int q = 0; q < 6; ++q) T[q] = st[kMpTobe + q];
  }
  if (nrows >= 50 && lane == 0) {
    int k = 0;
    for (int i = 0; i < 6; ++i)
      for (int jj = i; jj < 6; ++jj) {
        sh.AtA[i * 6 + jj] = (float)tot[k];
        sh.AtA[jj * 6 + i] = (float)tot[k];
        ++k;
      }
    for (int i = 0; i < 6; ++i) sh.AtB[i] = (float)tot[21 + i];
  }
  const bool solve = nrows >= 50;  // (uniform)
  bool eig = solve && iter == 0, cert = false;
  if (solve) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();  // lane 0's AtA / AtB, for the wave
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (eig) {
      cert = loamla::nondegenerate_certified(sh.AtA, 100.0f);  // every lane, the same answer
      eig = !cert;
      if (eig) loamla::jacobi6_wave(sh.AtA, sh.jE, sh.jV);
    }
    // the QR solve by the whole wave; lane 0 goes on with X
    loamla::lm_step_wave(sh.AtA, sh.AtB, iter, 100.0f, &degen, st + kMpMatP, sh.X, sh.lm_ws, sh.lm_iws,
                         eig ? sh.jE : nullptr, eig ? sh.jV : nullptr, cert);
  }
  if (lane != 0) return;
  ist[kMiIters] = iter + 1;
  ist[kMiRows] = c_rows + nrows;
  ist[kMiRowsLast] = nrows;
  if (solve) {
    ist[kMiDegen] = degen;
    if (degen) ist[kMiDegSteps] = c_deg + 1;
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      T[q] = T[q] + sh.X[q];
      st[kMpTobe + q] = T[q];
    }
    rot_store(b, p, T);
    const float dR = loamla::delta_r(sh.X), dT = loamla::delta_t(sh.X);
    if (D(dR) < 0.05 && D(dT) < 0.05) ist[kMiStop] = 1;
  }
  if (iter + 1 >= b.max_iter) ist[kMiStop] = 1;
}
}  // namespace

// the fused step of one-wave workgroups (k_mp_nnfit<true>): the wave's row sums as
// this workgroup's partial (write-through), and the last workgroup of the instance to arrive sums
// the G partials in workgroup order and runs the step
// red: the wave's sums reduce-scattered (wave_reduce_scatter_28: lanes 2v, 2v+1 hold value v)
LOAM_D void mp_store_partial_and_step(const MpBuffers& b, int p, int wg, int G, double red) {
  static_assert(kMpFitThreads == 64, "one wave per workgroup: the wave's sums are the partial");
  const int lane = lane_id();
  if ((lane & 1) == 0 && (lane >> 1) < 28)
    store_partial(&b.part[((size_t)p * kMpFitGridMax + wg) * 28 + (lane >> 1)], red);
  __shared__ int sh_last;
  __shared__ double tot[28];
  __shared__ MpStepScratch sh;
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) sh_last = arrive_last(&b.done[p], G);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (!sh_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  {  // fixed order over the workgroups: lane (half h, value v) sums half h of the partials in
     // order, sixteen loads in flight per round, then the two halves are added in order
    const int v = lane % 28, h = lane / 28, G2 = (G + 1) / 2;
    const int g0 = h == 0 ? 0 : G2, g1 = h == 0 ? G2 : G;
    const double* pp = b.part + (size_t)p * kMpFitGridMax * 28 + v;
    double sum = 0.0;
    if (h < 2) {
      for (int g = g0; g < g1; g += 16) {
        double t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u)
          t[u] = g + u < g1 ? __hip_atomic_load(&pp[(size_t)(g + u) * 28], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (g + u < g1) sum += t[u];
      }
    }
    const double upper = __shfl_down(sum, 28, 64);
    if (lane < 28) tot[lane] = sum + upper;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (lane == 0) b.done[p] = 0;
  mp_step(b, p, tot, sh);
}
// One mapping L-M iteration's correspondences in one launch: lane per query, the 5-NN search
// (knn5_flat, seeded) then the fit and row — the fit needs only the lane's own five neighbours —
// in one-wave workgroups whose 27-entry candidate lists and 27-word Jacobi scratch share one LDS
// array (the wave's search is over before its fits begin).  Rows in query order per workgroup.
// FUSED: the workgroup's partial + the last workgroup's step (mp_store_partial_and_step); else the
// rows go to q_ok / q_cf for k_mp_iter.  COUNT: the work counters.
#ifndef LOAM_NNFIT_WPE
#define LOAM_NNFIT_WPE 4
#endif
template <bool FUSED, bool COUNT>
__global__ __launch_bounds__(kMpFitThreads) __attribute__((amdgpu_waves_per_eu(LOAM_NNFIT_WPE))) void k_mp_nnfit(MpBuffers b) {
  constexpr int NT = kMpFitThreads;
  static_assert(NT == 64, "the list / scratch sharing needs one wave per workgroup");
  const XcdBlock blk = xcd_block();
  const int p = blk.y, tid = threadIdx.x;
  int* ist = b.istate + (size_t)p * kMpStateInts;
  if (!ist[kMiLmRan] || ist[kMiStop]) return;
  const bool first = ist[kMiIters] == 0;
  __shared__ uint32_t lds[kNnListCap * NT];  // candidate lists (column tid, stride NT) / Jacobi rows
  const int nsc = b.sseg_cnt[p * 2 + 0], nss = b.sseg_cnt[p * 2 + 1];
  const int nq = nsc + nss;
  int8_t* qok = b.q_ok + (size_t)p * b.cap_stack;
  float4* qcf = b.q_cf + (size_t)p * b.cap_stack;
  const loampose::MapRot r = rot_load(b, p);
  const MpNnCtx c = mp_nn_ctx(b, p);
  const MpTrig tg0 = mp_trig_of(r);
  float* jw = (float*)lds + tid * 27;
  int nfits = 0, work = 0;
  // FUSED: the rows of each pass over the queries are reduce-scattered over the wave at once (no
  // 28 fp64 sums live across the search), the passes' sums added in pass order (one pass per lane
  // for a VLP-16 stack)
  double red = 0.0;
  // FUSED: lane 2t's term t of the 28 sums (JᵀJ upper triangle row-major, Jᵀb, rows) as the
  // product of row entries term_x * term_y (mp_row_accum's order; entry 7 = 1 per accepted row)
  int term_x = -1, term_y = -1;
  if (FUSED && (tid & 1) == 0 && (tid >> 1) < 28) {
    const int t = tid >> 1;
    if (t < 21) {
      int i = 0, r0 = t;
      while (r0 >= 6 - i) { r0 -= 6 - i; ++i; }
      term_x = i;
      term_y = i + r0;
    } else if (t < 27) {
      term_x = t - 21;
      term_y = 6;
    } else {
      term_x = 7;
      term_y = 7;
    }
  }
  // one record per query (MpFit in q_fit): the 5-NN of the last iteration (i0..i3 | i4, 0,
  // distinct, fit valid) and the fit made for them — the seeds and the reuse test in one read
  MpFit* qrec = (MpFit*)b.q_fit + (size_t)p * b.cap_stack;
  for (int q0 = blk.x * NT; q0 < nq; q0 += gridDim.x * NT) {  // (wave-uniform trip count)
    const int q = q0 + tid;
    const bool corner = q < nsc;
    float4 sel = make_float4(0, 0, 0, 0), o = sel, cf = sel;
    int4 r0 = make_int4(-1, -1, -1, -1), r1 = make_int4(0, 0, 0, 0);
    bool row_ok = false;
    Top5 t;
    if (q < nq) {
      o = c.stack[corner ? q : b.capC + (q - nsc)];
      if (!first) { r0 = qrec[q].n0; r1 = qrec[q].n1; }
      sel = loampose::point_to_map(r, o);
      mp_nn_seed_from(c, q, corner, first, r0, r1, sel, t, work);
#ifdef LOAM_DIAG_OVERFLOW  // (diagnostic build: the queries that overflowed their pending list, in mp_fits >> 20)
      int dg = 0;
      int* const diag = &dg;
#else
      int* const diag = nullptr;
#endif
      if (corner) knn5_flat<NT, 1, kNnListCap>(c.hcs, c.hcr, c.hcp, c.TC, sel, t, lds + tid, work, 0, diag);
      else knn5_flat<NT, 1, kNnListCap>(c.hss, c.hsr, c.hsp, c.TS, sel, t, lds + tid, work, 0, diag);
#ifdef LOAM_DIAG_OVERFLOW
      if (dg & kNnDiagOverflow) nfits += 1 << 20;
#endif
#ifdef LOAM_DIAG_SEARCH2  // (diagnostic build: the search twice, its cost measured by the difference)
      {
        Top5 t2;
        int w2 = 0;
        asm volatile("" ::: "memory");
        mp_nn_seed_from(c, q, corner, first, r0, r1, sel, t2, w2);
        if (corner) knn5_flat<NT, 1, kNnListCap>(c.hcs, c.hcr, c.hcp, c.TC, sel, t2, lds + tid, w2, 0);
        else knn5_flat<NT, 1, kNnListCap>(c.hss, c.hsr, c.hsp, c.TS, sel, t2, lds + tid, w2, 0);
        if (t2.i(0) != t.i(0)) nfits += 1 << 20;
      }
#endif
      LOAM_CHECK(q < b.cap_stack && (t.i(4) == 0x7fffffff || t.i(4) < (corner ? c.nfc : c.nfs)), q, t.i(4));
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();  // every lane's list reads are done before the scratch reuse
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (q < nq) {
      const int4 n0 = make_int4(t.i(0), t.i(1), t.i(2), t.i(3));
      // the stored fit is this list's when the list is unchanged and the fit was made (a fit is
      // a function of the five map points alone: reusing it is bit-identical to refitting)
      bool valid = !first && r1.w && r0.x == n0.x && r0.y == n0.y && r0.z == n0.z && r0.w == n0.w &&
                   r1.x == t.i(4);
      int ok = 0;
      if (t.i(4) != 0x7fffffff && D(t.d(4)) < 1.0) {  // :719, :826
        float4 g0, g1;
        if (valid) {
          g0 = qrec[q].g0;
          g1 = qrec[q].g1;
        } else {
          ++nfits;
          const float4* from = corner ? c.fromC : c.fromS;
          float4 nb[5];
#pragma unroll
          for (int k = 0; k < 5; ++k) {
            LOAM_CHECK(t.i(k) >= 0 && t.i(k) < (corner ? c.nfc : c.nfs), t.i(k), q);
            nb[k] = from[t.i(k)];
          }
          mp_fit_compute(corner, nb, jw, g0, g1);
#ifdef LOAM_DIAG_FIT2  // (diagnostic build: every fit twice)
          {
            float4 h0, h1;
            asm volatile("" ::: "memory");
            mp_fit_compute(corner, nb, jw, h0, h1);
            if (h0.x != g0.x) nfits += 1 << 20;
          }
#endif
          qrec[q].g0 = g0;
          qrec[q].g1 = g1;
          valid = true;
        }
        mp_fit_residual(corner, g0, g1, sel, cf, ok);
      }
      // the record is written only when it changes: a reused fit's list is the stored one (the
      // next iteration's seeds and reuse test read indices and flags only)
      const int4 n1 = make_int4(t.i(4), 0, top5_distinct(t), valid ? 1 : 0);
      if (first || r0.x != n0.x || r0.y != n0.y || r0.z != n0.z || r0.w != n0.w || r1.x != n1.x || r1.z != n1.z ||
          r1.w != n1.w) {
        qrec[q].n0 = n0;
        qrec[q].n1 = n1;
      }
      if constexpr (!FUSED) {  // (k_mp_iter reads the rows back; the fused step sums them below)
        qok[q] = (int8_t)ok;
        qcf[q] = cf;
      }
      row_ok = ok != 0;
    }
    if constexpr (FUSED) {  // (outside the branch: every lane takes part)
      // the pass's rows through LDS (8 floats per lane: J, b, 1 when accepted, else zeros), then
      // lane 2t sums term t over the wave's rows in query order: no 28 fp64 sums per lane
      float a6[6] = {0, 0, 0, 0, 0, 0}, bb = 0.0f;
      const MpTrig tg = mp_trig_here(tg0);
      if (row_ok) mp_row_jac(tg, o, cf, a6, bb);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();  // the fits' scratch reads are done
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      float* rw = (float*)lds + tid * 8;
#pragma unroll
      for (int k = 0; k < 6; ++k) rw[k] = a6[k];
      rw[6] = bb;
      rw[7] = row_ok ? 1.0f : 0.0f;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (term_x >= 0) {
        const float* rows = (const float*)lds;
        double s = 0.0;
#pragma unroll 16
        for (int l = 0; l < NT; ++l) s = loamla::dmac(s, rows[l * 8 + term_x], rows[l * 8 + term_y]);
        red += s;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();  // the fits' scratch is free before the next lists
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  }
  nfits = wave_sum(nfits);
  if (lane_id() == 0 && nfits) atomicAdd(&ist[kMiFits], nfits);
  if (COUNT) {
    const int ncand = wave_sum(work & ((1 << kWorkCellShift) - 1)), ncell = wave_sum(work >> kWorkCellShift);
    if (lane_id() == 0 && ncand) {
      atomicAdd(&ist[kMiNnCand], ncand);
      atomicAdd(&ist[kMiNnCells], ncell);
    }
  }
  if constexpr (FUSED) mp_store_partial_and_step(b, p, blk.x, (int)gridDim.x, red);
}

namespace {
struct MpIterShared {
  double red[16][28];  // (up to 1024 threads)
  double tot[28];
  float trig[6];
  MpStepScratch step;
};
}  // namespace

// the normal equations of the accepted rows (:879-974) and the 6x6 step, one workgroup per
// instance; rows = the accepted correspondences of this iteration, in stack order
// NT threads per instance: 256 for large batches, 1024 for small ones (a shorter row chain per lane)
template <int NT>
__global__ __launch_bounds__(NT) void k_mp_iter(MpBuffers b) {
  const int p = blockIdx.x, tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  int* ist = b.istate + (size_t)p * kMpStateInts;
  if (!ist[kMiLmRan] || ist[kMiStop]) return;
  __shared__ MpIterShared sh;
  const int nsc = b.sseg_cnt[p * 2 + 0], nss = b.sseg_cnt[p * 2 + 1];
  const int nq = nsc + nss;
  const float4* stack = b.stack + (size_t)p * b.cap_stack;
  const int8_t* qok = b.q_ok + (size_t)p * b.cap_stack;
  const float4* qcf = b.q_cf + (size_t)p * b.cap_stack;
  const MpTrig tg = mp_trig_of(rot_load(b, p));
  const float srx = tg.srx, crx = tg.crx, sry = tg.sry, cry = tg.cry, srz = tg.srz, crz = tg.crz;
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  // four rows' loads in flight per step; the rows are still summed in the lane's q order
  for (int q0 = tid; q0 < nq; q0 += 4 * NT) {  // :897-921
    int8_t okv[4];
    float4 ov[4], cv4[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + u * NT;
      okv[u] = q < nq ? qok[q] : (int8_t)0;
      ov[u] = q < nq ? stack[q < nsc ? q : b.capC + (q - nsc)] : make_float4(0, 0, 0, 0);
      cv4[u] = q < nq ? qcf[q] : make_float4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
    if (!okv[u]) continue;
    const float4 o = ov[u], c = cv4[u];
    float a[6];
    a[0] = (crx * sry * srz * o.x + crx * crz * sry * o.y - srx * sry * o.z) * c.x +
           (-srx * srz * o.x - crz * srx * o.y - crx * o.z) * c.y +
           (crx * cry * srz * o.x + crx * cry * crz * o.y - cry * srx * o.z) * c.z;
    a[1] = ((cry * srx * srz - crz * sry) * o.x + (sry * srz + cry * crz * srx) * o.y + crx * cry * o.z) * c.x +
           ((-cry * crz - srx * sry * srz) * o.x + (cry * srz - crz * srx * sry) * o.y - crx * sry * o.z) * c.z;
    a[2] = ((crz * srx * sry - cry * srz) * o.x + (-cry * crz - srx * sry * srz) * o.y) * c.x +
           (crx * crz * o.x - crx * srz * o.y) * c.y +
           ((sry * srz + cry * crz * srx) * o.x + (crz * sry - cry * srx * srz) * o.y) * c.z;
    a[3] = c.x;
    a[4] = c.y;
    a[5] = c.z;
    const float bb = -c.w;
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int jj = i; jj < 6; ++jj) acc[k++] += (double)a[i] * (double)a[jj];  // (dmac measured slower here)
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[21 + i] += (double)a[i] * (double)bb;
    acc[27] += 1.0;
  }
  }
  wave_reduce_scatter_28(acc);  // lanes 2v, 2v+1: the wave sum of value v
  if ((lane & 1) == 0 && (lane >> 1) < 28) sh.red[w][lane >> 1] = acc[0];
  __syncthreads();
  if (tid < 28) {
    double v = sh.red[0][tid];
    for (int ww = 1; ww < NT / 64; ++ww) v += sh.red[ww][tid];
    sh.tot[tid] = v;
  }
  __syncthreads();
  if (tid < 64) mp_step(b, p, sh.tot, sh.step);  // the first wave
}


// Small batches (streaming, config 2): the whole iteration in one launch — each lane its query's
// 5-NN, fit and row, fp64 partials per workgroup, and the last workgroup of the instance to finish
// sums them in a fixed order and runs the step (three launches and a one-workgroup row pass fewer
// per iteration).
__global__ __launch_bounds__(kMpQueryThreads) void k_mp_lm_small(MpBuffers b) {
  const int p = blockIdx.y, tid = threadIdx.x, lane = lane_id(), w = tid >> 6;
  int* ist = b.istate + (size_t)p * kMpStateInts;
  if (!ist[kMiLmRan] || ist[kMiStop]) return;
  LOAM_PH(const unsigned long long ph0 = ph_now(); if (tid == 0) ph_start(&g_ph_mp, ph0);)
  __shared__ uint32_t lists[27 * kMpQueryThreads];
  __shared__ float jac[kMpQueryThreads][27];
  __shared__ double red[kMpQueryThreads / 64][28];
  const int nsc = b.sseg_cnt[p * 2 + 0], nss = b.sseg_cnt[p * 2 + 1];
  const int nq = nsc + nss;
  const float4* stack = b.stack + (size_t)p * b.cap_stack;
  int8_t* qok = b.q_ok + (size_t)p * b.cap_stack;
  float4* qcf = b.q_cf + (size_t)p * b.cap_stack;
  const bool first = ist[kMiIters] == 0;
  const loampose::MapRot r = rot_load(b, p);
  const MpNnCtx c = mp_nn_ctx(b, p);
  int work = 0, nfits = 0;  // (work: the batch kernel's profiling counter; not summed here)
  const MpTrig tg = mp_trig_of(r);
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  // each lane's row is added right after its fit (same queries, same order per lane as a
  // separate pass over the stored rows: identical sums, one reload round trip fewer)
  // kMpNnLanes lanes per query: the 5-NN search split over the group, the fit and row on its first lane
  constexpr int L = kMpNnLanes, QPB = kMpQueryThreads / L;
  const int sub = tid % L;
  for (int q = blockIdx.x * QPB + tid / L; q < nq; q += gridDim.x * QPB) {
    LOAM_PH(const unsigned long long pq0 = ph_now();)
    float4 sel;
    Top5 t;
    mp_nn_query<kMpQueryThreads, L>(b, c, q, nsc, first, r, lists + tid, sel, t, work, sub);
    LOAM_PH(asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); const unsigned long long pq1 = ph_now();)
    float4 cf = make_float4(0, 0, 0, 0);
    int ok = 0;
    if (sub == 0) {
      mp_fit_query(b, p, q, nsc, first, make_int4(t.i(0), t.i(1), t.i(2), t.i(3)),
                   make_int4(t.i(4), __float_as_int(t.d(4)), 0, 0), sel, jac[tid], nfits, cf, ok);
      qok[q] = (int8_t)ok;
      qcf[q] = cf;
      if (ok) mp_row_accum(tg, stack[q < nsc ? q : b.capC + (q - nsc)], cf, acc);
    }
    LOAM_PH(asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); const unsigned long long pq2 = ph_now();
            if (lane == 0) ph_query(&g_ph_mp, first ? 0 : 1, pq1 - pq0, pq2 - pq1);)
  }
  nfits = wave_sum(nfits);
  if (lane == 0 && nfits) atomicAdd(&ist[kMiFits], nfits);
  wave_reduce_scatter_28(acc);
  if ((lane & 1) == 0 && (lane >> 1) < 28) red[w][lane >> 1] = acc[0];
  __syncthreads();
  const int G = (int)gridDim.x;
  if (tid < 28) {
    double v = red[0][tid];
    for (int ww = 1; ww < kMpQueryThreads / 64; ++ww) v += red[ww][tid];
    store_partial(&b.part[((size_t)p * kMpSmallGrid + blockIdx.x) * 28 + tid], v);
  }
  __shared__ int sh_last;
  __shared__ double slice[8][28];
  __shared__ double tot[28];
  __shared__ MpStepScratch sh;
  __syncthreads();
  LOAM_PH(const int phk = first ? 0 : 1; const unsigned long long ph1 = ph_now();
          if (tid == 0) ph_arrive(&g_ph_mp, phk, ph0, ph1);)
  // (store_partial / arrive_last: the partials are drained write-through before the counter add;
  // the last workgroup acquires at agent scope, then reads them with sc1 loads)
  if (tid == 0)
    sh_last = arrive_last(&b.done[p], G);
  __syncthreads();
  if (!sh_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  LOAM_PH(const unsigned long long ph2 = ph_now();)
  if (tid < 8 * 28) {  // fixed-order sum: slice s holds partials s, s + 8, ... (all in flight)
    const int v = tid % 28, sl = tid / 28;
    const double* pp = b.part + (size_t)p * kMpSmallGrid * 28 + v;
    double t8[kMpSmallGrid / 8];
#pragma unroll
    for (int u = 0; u < kMpSmallGrid / 8; ++u) {
      const int g = sl + 8 * u;
      t8[u] = g < G ? __hip_atomic_load(&pp[(size_t)g * 28], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    }
    double a1 = 0.0;
#pragma unroll
    for (int u = 0; u < kMpSmallGrid / 8; ++u)
      if (sl + 8 * u < G) a1 += t8[u];
    slice[sl][v] = a1;
  }
  __syncthreads();
  if (tid < 28) {
    double v = slice[0][tid];
#pragma unroll
    for (int sl = 1; sl < 8; ++sl) v += slice[sl][tid];
    tot[tid] = v;
  }
  __syncthreads();
  LOAM_PH(const unsigned long long ph3 = ph_now();)
  if (tid < 64) {  // the first wave
    if (tid == 0) b.done[p] = 0;
    mp_step(b, p, tot, sh);
    LOAM_PH(const unsigned long long ph4 = ph_now(); if (tid == 0) ph_last(&g_ph_mp, phk, ph1, ph2, ph3, ph4);)
  }
}

// ---- the one-instance mapping L-M as one persistent launch (streaming: config 3, config 2) ----
// k_mp_lm_small's iteration (5-NN, fit, row per query group of kMpNnLanes lanes) for every
// iteration in one launch, as k_od_lm_stream does for the odometry: a query stays on the same
// lanes for the whole loop (its 5-NN seeds and fit record are read back by the lanes that wrote
// them), the partial sums are exchanged per iteration with write-through stores and a publication
// word per workgroup, and every workgroup sums all G partials in workgroup order and runs the step
// on its own copy of the state: the same transform and the same convergence decision everywhere.
struct MpLsState {
  float T[6], matP[36];
  int degen, iters, rows, deg_steps, stop;
};

// mp_step on the workgroup-local state (the first wave): the same arithmetic and decisions
LOAM_D void mp_step_ls(int max_iter, const double* tot, MpLsState& S, MpStepScratch& sh) {
  const int lane = lane_id();
  const int iter = S.iters;
  const int nrows = (int)tot[27];
  if (nrows >= 50 && lane == 0) {
    int k = 0;
    for (int i = 0; i < 6; ++i)
      for (int jj = i; jj < 6; ++jj) {
        sh.AtA[i * 6 + jj] = (float)tot[k];
        sh.AtA[jj * 6 + i] = (float)tot[k];
        ++k;
      }
    for (int i = 0; i < 6; ++i) sh.AtB[i] = (float)tot[21 + i];
  }
  const bool solve = nrows >= 50;  // (uniform)
  bool eig = solve && iter == 0, cert = false;
  int degen = S.degen;
  if (solve) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (eig) {
      cert = loamla::nondegenerate_certified(sh.AtA, 100.0f);
      eig = !cert;
      if (eig) loamla::jacobi6_wave(sh.AtA, sh.jE, sh.jV);
    }
    loamla::lm_step_wave(sh.AtA, sh.AtB, iter, 100.0f, &degen, S.matP, sh.X, sh.lm_ws, sh.lm_iws,
                         eig ? sh.jE : nullptr, eig ? sh.jV : nullptr, cert);
  }
  if (lane != 0) return;
  S.iters = iter + 1;
  S.rows += nrows;
  if (solve) {
    S.degen = degen;
    if (degen) ++S.deg_steps;
#pragma unroll
    for (int q = 0; q < 6; ++q) S.T[q] = S.T[q] + sh.X[q];
    const float dR = loamla::delta_r(sh.X), dT = loamla::delta_t(sh.X);
    if (D(dR) < 0.05 && D(dT) < 0.05) S.stop = 1;
  }
  if (iter + 1 >= max_iter) S.stop = 1;
}

__global__ __launch_bounds__(kMpQueryThreads) void k_mp_lm_stream(MpBuffers b) {
  const int g = blockIdx.x, G = gridDim.x, tid = threadIdx.x, lane = lane_id(), w = tid >> 6, p = 0;
  int* ist = b.istate;
  float* st = b.state;
  if (!ist[kMiLmRan] || ist[kMiStop]) return;  // (the same value in every workgroup)
  __shared__ uint32_t lists[27 * kMpQueryThreads];
  __shared__ float jac[kMpQueryThreads][27];
  __shared__ double red[kMpQueryThreads / 64][28], slice[8][28], tot[28];
  __shared__ MpStepScratch sh;
  __shared__ MpLsState S;
  __shared__ unsigned long long sh_epoch;
  if (tid < 6) S.T[tid] = st[kMpTobe + tid];
  if (tid < 36) S.matP[tid] = st[kMpMatP + tid];
  if (tid == 0) {
    S.degen = ist[kMiDegen];
    S.iters = ist[kMiIters];
    S.rows = ist[kMiRows];
    S.deg_steps = ist[kMiDegSteps];
    S.stop = 0;
    sh_epoch = b.ls_epoch[0];
  }
  __syncthreads();
  const int nsc = b.sseg_cnt[p * 2 + 0], nss = b.sseg_cnt[p * 2 + 1];
  const int nq = nsc + nss;
  const float4* stack = b.stack;
  int8_t* qok = b.q_ok;
  float4* qcf = b.q_cf;
  const MpNnCtx c = mp_nn_ctx(b, p);
  constexpr int L = kMpNnLanes, QPB = kMpQueryThreads / L;
  const int sub = tid % L;
  const unsigned long long tag0 = sh_epoch << 16;  // (iterations + 1 <= 1001 < 2^16: loam_create bounds max_iter)
  int nfits = 0;
  for (int it = 0; it < b.max_iter; ++it) {
    const bool first = S.iters == 0;
    const loampose::MapRot r = loampose::map_rot(S.T);  // (rot_store's values: the same dsin / dcos)
    const MpTrig tg = mp_trig_of(r);
    int work = 0;
    double acc[28];
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0.0;
    for (int q = g * QPB + tid / L; q < nq; q += G * QPB) {
      float4 sel;
      Top5 t;
      mp_nn_query<kMpQueryThreads, L>(b, c, q, nsc, first, r, lists + tid, sel, t, work, sub);
      float4 cf = make_float4(0, 0, 0, 0);
      int ok = 0;
      if (sub == 0) {
        mp_fit_query(b, p, q, nsc, first, make_int4(t.i(0), t.i(1), t.i(2), t.i(3)),
                     make_int4(t.i(4), __float_as_int(t.d(4)), 0, 0), sel, jac[tid], nfits, cf, ok);
        qok[q] = (int8_t)ok;
        qcf[q] = cf;
        if (ok) mp_row_accum(tg, stack[q < nsc ? q : b.capC + (q - nsc)], cf, acc);
      }
    }
    wave_reduce_scatter_28(acc);
    if ((lane & 1) == 0 && (lane >> 1) < 28) red[w][lane >> 1] = acc[0];
    __syncthreads();
    const int par = it & 1;
    if (tid < 28) {  // this workgroup's partial, waves in order, stored write-through
      double v = red[0][tid];
      for (int ww = 1; ww < kMpQueryThreads / 64; ++ww) v += red[ww][tid];
      store_partial(&b.ls_part[((size_t)par * kMpSmallGrid + g) * 28 + tid], v);
    }
    if (tid < 64) {
      __builtin_amdgcn_wave_barrier();  // (every lane's store drained: store_partial waits for it)
      if (tid == 0)
        __hip_atomic_store(&b.ls_flag[g], tag0 + (unsigned long long)(it + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tid < G) {  // every workgroup's partial of this iteration
      const unsigned long long want = tag0 + (unsigned long long)(it + 1);
      while (__hip_atomic_load(&b.ls_flag[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < want)
        __builtin_amdgcn_s_sleep(1);
    }
    __syncthreads();
    if (tid < 8 * 28) {  // fixed order: slice s sums partials s, s + 8, ...; the slices in order
      const int v = tid % 28, sl = tid / 28;
      const double* pp = b.ls_part + (size_t)par * kMpSmallGrid * 28 + v;
      double t8[kMpSmallGrid / 8];
#pragma unroll
      for (int u = 0; u < kMpSmallGrid / 8; ++u) {
        const int gg = sl + 8 * u;
        t8[u] = gg < G ? __hip_atomic_load(&pp[(size_t)gg * 28], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
      }
      double a1 = 0.0;
#pragma unroll
      for (int u = 0; u < kMpSmallGrid / 8; ++u)
        if (sl + 8 * u < G) a1 += t8[u];
      slice[sl][v] = a1;
    }
    __syncthreads();
    if (tid < 28) {
      double v = slice[0][tid];
#pragma unroll
      for (int sl = 1; sl < 8; ++sl) v += slice[sl][tid];
      tot[tid] = v;
    }
    __syncthreads();
    if (tid < 64) mp_step_ls(b.max_iter, tot, S, sh);
    __syncthreads();
    if (S.stop) break;
  }
  nfits = wave_sum(nfits);
  if (lane == 0 && nfits) atomicAdd(&ist[kMiFits], nfits);
  if (g == 0) {  // the state for the kernels after the loop (the same in every workgroup)
    if (tid < 6) st[kMpTobe + tid] = S.T[tid];
    if (tid < 36) st[kMpMatP + tid] = S.matP[tid];
    if (tid == 0) {
      rot_store(b, p, S.T);
      ist[kMiDegen] = S.degen;
      ist[kMiIters] = S.iters;
      ist[kMiRows] = S.rows;
      ist[kMiDegSteps] = S.deg_steps;
      ist[kMiStop] = S.stop;
    }
  }
}

// workgroups of k_mp_lm_stream (kMpSmallGrid, as k_mp_lm_small), or 0 when they could not all be
// resident at once (the per-iteration launches run instead)
int mp_lm_stream_grid() {
  static int cap[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 0;
  if (cap[dev] == 0) {
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_mp_lm_stream, kMpQueryThreads, 0) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
      per_cu = cus = 0;
    cap[dev] = std::max(1, per_cu * cus);
  }
  // (a margin of 2: other streams' kernels may hold slots a while; half the grid loops twice)
  return 2 * kMpSmallGrid <= cap[dev] ? kMpSmallGrid : (kMpSmallGrid <= cap[dev] ? kMpSmallGrid / 2 : 0);
}

// transformUpdate (:199-232) for the instances whose L-M ran; the IMU blend (:224-225) when the
// host found IMU data for the odometry stamp
__global__ void k_mp_lm_end(MpBuffers b) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p == 0) { b.vg.counts[0] = 0; b.vg.counts[1] = 0; b.vg.counts[2] = 0; b.vg.counts[3] = 0; }  // (vg_cubes' lists)
  if (p >= b.P) return;
  const int* ist = b.istate + (size_t)p * kMpStateInts;
  if (!ist[kMiLmRan]) return;
  float* st = b.state + (size_t)p * kMpStateFloats;
  if (ist[kMiImu]) {
    const float imuRollLast = st[kMpImuRP], imuPitchLast = st[kMpImuRP + 1];
    st[kMpTobe + 0] = (float)(0.998 * D(st[kMpTobe + 0]) + 0.002 * D(imuPitchLast));
    st[kMpTobe + 2] = (float)(0.998 * D(st[kMpTobe + 2]) + 0.002 * D(imuRollLast));
    rot_store(b, p, st + kMpTobe);
  }
  for (int k = 0; k < 6; ++k) {
    st[kMpBef + k] = st[kMpSum + k];
    st[kMpAft + k] = st[kMpTobe + k];
  }
}

namespace {

// ---------------------------------------------------------------- insertion (:980-1016)
// one workgroup per instance: cube slot of every stack point (corner, then surf), stable ranks by
// one wave walking the stack in order, per-cube prefix, scatter of the map-frame points.
// (k_cm_rank below restates the slot and ranking statements for loam_lanes_map_commit, whose n = 1
// result must equal this kernel's bit for bit: a change to either belongs in both.)
template <int NT>
__global__ __launch_bounds__(NT) void k_mp_insert(MpBuffers b, int* slot_of, int* rank_of) {
  const int p = blockIdx.x, tid = threadIdx.x, lane = lane_id();
  const int* ist = b.istate + (size_t)p * kMpStateInts;
  const int nsc = b.sseg_cnt[p * 2 + 0], nss = b.sseg_cnt[p * 2 + 1];
  const float4* stack = b.stack + (size_t)p * b.cap_stack;
  const loampose::MapRot r = rot_load(b, p);
  const int cW = ist[kMiCenW], cH = ist[kMiCenH], cD = ist[kMiCenD];
  int* so = slot_of + (size_t)p * b.cap_stack;
  int* ro = rank_of + (size_t)p * b.cap_stack;
  __shared__ int cnt[2][kCubeNum];
  __shared__ int scratch[NT / 64 + 1];
  // the (slot, kind) keys the stack uses, as a bitmap; their dense numbering (prefix popcounts)
  // lets every wave keep its own counts when few keys occur (the usual case: a sweep touches a
  // few dozen cubes)
  constexpr int kKeyWords = (2 * kCubeNum + 31) / 32, kDense = 512, kWaves = NT / 64;
  __shared__ unsigned keybits[kKeyWords];
  __shared__ int keypre[kKeyWords + 1];
  __shared__ int wcnt[kWaves][kDense];
  for (int i = tid; i < 2 * kCubeNum; i += NT) cnt[i / kCubeNum][i % kCubeNum] = 0;
  for (int i = tid; i < kKeyWords; i += NT) keybits[i] = 0u;
  for (int i = tid; i < kWaves * kDense; i += NT) wcnt[i / kDense][i % kDense] = 0;
  __syncthreads();
  const int nst = nsc + nss;
  for (int q = tid; q < nst; q += NT) {
    const float4 a = loampose::point_to_map(r, stack[q < nsc ? q : b.capC + (q - nsc)]);
    const int ci = cube_of(a.x, cW), cj = cube_of(a.y, cH), ck = cube_of(a.z, cD);
    const bool in = ci >= 0 && ci < kCubeW && cj >= 0 && cj < kCubeH && ck >= 0 && ck < kCubeD;
    const int s = in ? cube_index(ci, cj, ck) : -1;
    so[q] = s;
    if (s >= 0) {
      const int key = s * 2 + (q < nsc ? 0 : 1);
      atomicOr(&keybits[key >> 5], 1u << (key & 31));
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
    // stable ranks, all waves: wave w ranks its contiguous chunk of the stack (in order, per dense
    // key), then each key's chunk counts are prefixed in wave order
    const int w = tid >> 6, chunk = ((nst + kWaves * 64 - 1) / (kWaves * 64)) * 64;
    const int q0 = w * chunk, q1 = min(nst, q0 + chunk);
    constexpr int kAhead = 8;  // slot loads of eight 64-point steps in flight (the walk is load-latency bound)
    int sa[kAhead];
    for (int base = q0; base < q1; base += 64) {
      const int step = ((base - q0) >> 6) % kAhead;
      if (step == 0) {
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
          const int qq = base + u * 64 + lane;
          sa[u] = qq < q1 ? so[qq] : -1;
        }
      }
      const int q = base + lane;
      const bool v = q < q1;
      int s = -1;
#pragma unroll
      for (int u = 0; u < kAhead; ++u)
        if (u == step) s = sa[u];
      const int key = s < 0 ? -1 : s * 2 + (q < nsc ? 0 : 1);
      const int id = key < 0 ? -1 : keypre[key >> 5] + __popc(keybits[key >> 5] & ((1u << (key & 31)) - 1u));
      uint64_t m = __ballot(v && id >= 0);
      int rank = 0;
      while (m) {
        const int leader = __ffsll((unsigned long long)m) - 1;
        const int il = __builtin_amdgcn_readlane(id, leader);
        const uint64_t mm = __ballot(v && id == il);
        const int basecnt = wcnt[w][il];
        if (v && id == il) rank = basecnt + __popcll(mm & lanemask_lt());
        __builtin_amdgcn_wave_barrier();
        if (lane == leader) wcnt[w][il] = basecnt + __popcll(mm);
        __builtin_amdgcn_wave_barrier();
        m &= ~mm;
      }
      if (v) ro[q] = rank;
    }
    __threadfence_block();
    __syncthreads();
    // per dense key: chunk bases in wave order (wcnt becomes the base), total into cnt
    for (int i = tid; i < 2 * kCubeNum; i += NT) {
      if (!(keybits[i >> 5] & (1u << (i & 31)))) continue;
      const int id = keypre[i >> 5] + __popc(keybits[i >> 5] & ((1u << (i & 31)) - 1u));
      int run = 0;
#pragma unroll
      for (int ww = 0; ww < kWaves; ++ww) {
        const int c = wcnt[ww][id];
        wcnt[ww][id] = run;
        run += c;
      }
      cnt[i & 1][i >> 1] = run;
    }
    __threadfence_block();
    __syncthreads();
    for (int q = tid; q < nst; q += NT) {
      const int s = so[q];
      if (s < 0) continue;
      const int key = s * 2 + (q < nsc ? 0 : 1);
      const int id = keypre[key >> 5] + __popc(keybits[key >> 5] & ((1u << (key & 31)) - 1u));
      ro[q] += wcnt[q / chunk][id];
    }
  } else if (tid < 64) {  // many keys: stable ranks by one wave, stack order
    for (int base = 0; base < nsc + nss; base += 64) {
      const int q = base + lane;
      const bool v = q < nsc + nss;
      const int kind = q < nsc ? 0 : 1;
      const int s = v ? so[q] : -1;
      const int key = s < 0 ? -1 : s * 2 + kind;
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
  __syncthreads();
  // exclusive prefix over (kind, cube slot), kind-major: each thread owns a contiguous run of the
  // flattened counts (one block scan instead of one per 256 slots); offsets replace the counts in LDS
  int* ac = b.app_cnt + (size_t)p * kCubeNum * 2;
  int* ao = b.app_off + (size_t)p * kCubeNum * 2;
  {
    constexpr int kFlat = 2 * kCubeNum, kPer = (kFlat + NT - 1) / NT;
    int* cf = &cnt[0][0];
    int sum = 0;
    for (int k = 0; k < kPer; ++k) {
      const int i = tid * kPer + k;
      if (i < kFlat) sum += cf[i];
    }
    int tot;
    int run = block_excl_scan<NT>(sum, scratch, tot);
    for (int k = 0; k < kPer; ++k) {
      const int i = tid * kPer + k;
      if (i < kFlat) {
        const int c = cf[i];
        cf[i] = run;
        run += c;
      }
    }
    __syncthreads();
    for (int i = tid; i < kFlat; i += NT) {
      const int kind = i / kCubeNum, s = i % kCubeNum;
      const int o = cf[i], nx = i + 1 < kFlat ? cf[i + 1] : tot;
      ac[s * 2 + kind] = nx - o;
      ao[s * 2 + kind] = o;
    }
  }
  __threadfence_block();
  __syncthreads();
  float4* app = b.app + (size_t)p * b.cap_stack;
  for (int q = tid; q < nsc + nss; q += NT) {
    const int s = so[q];
    if (s < 0) continue;
    const int kind = q < nsc ? 0 : 1;
    app[ao[s * 2 + kind] + ro[q]] = loampose::point_to_map(r, stack[q < nsc ? q : b.capC + (q - nsc)]);
  }
}

// per valid cube: DS input = old cube content ++ appended points (corner region, then surf region);
// thread per (kind, valid cube) segment, one block scan for the offsets
__global__ __launch_bounds__(kMpThreads) void k_mp_vseg(MpBuffers b) {
  static_assert(2 * kMaxValid <= kMpThreads, "one thread per segment");
  const int p = blockIdx.x, tid = threadIdx.x;
  const int nv = b.istate[(size_t)p * kMpStateInts + kMiNValid];
  const int* slots = slot_table(b, b.pool_cur, p);
  const int* ac = b.app_cnt + (size_t)p * kCubeNum * 2;
  __shared__ int scratch[16];
  const int kind = tid / kMaxValid, v = tid % kMaxValid;
  int n = 0, nold = 0;
  if (tid < 2 * kMaxValid && v < nv) {
    const int ind = b.valid[(size_t)p * kMaxValid + v];
    nold = slots[ind * 4 + 1 + 2 * kind];
    n = nold + ac[ind * 2 + kind];
  }
  int tot;
  const int ex = block_excl_scan<kMpThreads>(n, scratch, tot);
  const int lim = b.map_cap;
  if (tid < 2 * kMaxValid) {
    // the reference order fills segments in (kind, v) order; a segment that would pass the
    // capacity is emptied and flags the instance (as the sequential walk did)
    const bool over = ex + n > lim;
    const int sidx = p * 2 * kMaxValid + tid;
    const int base = (int)((size_t)p * b.map_cap) + (over ? 0 : ex);
    b.vseg_b[sidx] = base;
    b.vseg_e[sidx] = base + (over ? 0 : n);
    b.vseg_leaf[sidx] = kind == 0 ? 0.2f : 0.4f;
    if (over && n > 0) b.istate[(size_t)p * kMpStateInts + kMiErr] |= ERR_CAP_MAP;
    b.vseg_nold[sidx] = nold;
    b.vseg_skip[sidx] = 0;
    if (over || n == 0) {
      b.vseg_cnt[sidx] = 0;  // (not in the VoxelGrid's list)
    } else {
      b.vg_lin[atomicAdd(b.vg.counts + 2, 1)] = sidx;
      // long segments with a short appended tail: the incremental VoxelGrid may take them
      if (b.tune.vg_merge && vg_merge_eligible(n, nold, b.tune.vg_merge_min))
        b.vg_mlist[atomicAdd(b.vg.counts + 3, 1)] = sidx;
    }
  }
}

// the DS input of every valid-cube segment, flattened over the instance's points: the segments
// are contiguous in (kind, valid cube) order, so a point finds its segment by binary search over
// their starts (LDS) and copies from the old pool or the appended stack points
__global__ __launch_bounds__(256) void k_mp_vcopy(MpBuffers b) {
  constexpr int NS = 2 * kMaxValid;
  const int p = blockIdx.y, tid = threadIdx.x;
  if (b.istate[(size_t)p * kMpStateInts + kMiErr] & ERR_CAP_MAP) return;
  const int nv = b.istate[(size_t)p * kMpStateInts + kMiNValid];
  const int* slots = slot_table(b, b.pool_cur, p);
  const float4* pool = b.pool + ((size_t)b.pool_cur * b.P + p) * b.map_cap;
  const int* ao = b.app_off + (size_t)p * kCubeNum * 2;
  const float4* app = b.app + (size_t)p * b.cap_stack;
  __shared__ int sb[NS + 1], snold[NS], soff[NS], sapp[NS];
  const int base = (int)((size_t)p * b.map_cap);
  if (tid < NS) {
    const int kind = tid / kMaxValid, v = tid % kMaxValid;
    sb[tid] = b.vseg_b[p * NS + tid] - base;
    int nold = 0, off = 0, ap = 0;
    if (v < nv) {
      const int ind = b.valid[(size_t)p * kMaxValid + v];
      nold = slots[ind * 4 + 1 + 2 * kind];
      off = slots[ind * 4 + 2 * kind];
      ap = ao[ind * 2 + kind];
    }
    snold[tid] = nold;
    soff[tid] = off;
    sapp[tid] = ap;
  }
  if (tid == 0) sb[NS] = b.vseg_e[p * NS + NS - 1] - base;
  __syncthreads();
  const int total = sb[NS];
  for (int i = blockIdx.x * 256 + tid; i < total; i += gridDim.x * 256) {
    int lo = 0, hi = NS - 1;  // last segment whose start is <= i
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (sb[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const int t = i - sb[lo];
    b.vin[base + i] = t < snold[lo] ? pool[soff[lo] + t] : app[sapp[lo] + (t - snold[lo])];
  }
}

// new cube store: valid cubes <- their DS output, every other cube <- old ++ appended.  The
// (kind, cube) sizes go to LDS in coalesced passes; each thread then owns a contiguous run of
// them, so the offsets and the non-empty list need one block scan each.
template <int NT>
__global__ __launch_bounds__(NT) void k_mp_compact_table(MpBuffers b) {
  constexpr int N = 2 * kCubeNum, E = (N + NT - 1) / NT;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int nv = b.istate[(size_t)p * kMpStateInts + kMiNValid];
  const int* old = slot_table(b, b.pool_cur, p);
  int* nw = slot_table(b, 1 - b.pool_cur, p);
  const int* ac = b.app_cnt + (size_t)p * kCubeNum * 2;
  __shared__ int16_t vidx[kCubeNum];
  __shared__ int nn[N];
  __shared__ int scratch[NT / 64 + 1];
  for (int s = tid; s < kCubeNum; s += NT) vidx[s] = -1;
  __syncthreads();
  if (tid < nv) vidx[b.valid[(size_t)p * kMaxValid + tid]] = (int16_t)tid;
  __syncthreads();
  int vpts = 0;
  for (int x = tid; x < N; x += NT) {
    const int kind = x / kCubeNum, s = x % kCubeNum, v = vidx[s];
    const int n = v >= 0 ? b.vseg_cnt[p * 2 * kMaxValid + kind * kMaxValid + v] : old[s * 4 + 1 + 2 * kind] + ac[s * 2 + kind];
    nn[x] = n;
    if (v >= 0) vpts += n;
  }
  __syncthreads();
  const int x0 = tid * E, x1 = min(N, x0 + E);
  int sum = 0;
  for (int x = x0; x < x1; ++x) sum += nn[x];
  int run;
  int off = block_excl_scan<NT>(sum, scratch, run);
  for (int x = x0; x < x1; ++x) {  // counts -> offsets, in LDS
    const int c = nn[x];
    nn[x] = off;
    off += c;
  }
  __syncthreads();
  // the table and the non-empty (kind, cube) list written (kind, cube)-consecutive across the lanes
  // (each lane's own run of entries would scatter every store): kind | cube << 1 | (valid + 1) << 14
  // (all passes at once: the non-empty entries ranked by wave ballots, the (pass, wave) counts
  // prefixed by each wave in x order — two barriers instead of three per pass)
  int* items = b.citems + (size_t)p * 2 * kCubeNum;
  constexpr int NW = NT / 64;
  static_assert(NW <= 64, "one count per lane");
  __shared__ int icnt[E][NW];
  const int lane = lane_id(), w = tid >> 6;
  int iex[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int x = e * NT + tid;
    int n = 0;
    if (x < N) {
      const int kind = x / kCubeNum, s = x % kCubeNum, o = nn[x];
      n = (x + 1 < N ? nn[x + 1] : run) - o;
      nw[s * 4 + 2 * kind] = o;
      nw[s * 4 + 1 + 2 * kind] = n;
    }
    const uint64_t m = __ballot(n > 0);
    iex[e] = n > 0 ? __popcll(m & lanemask_lt()) : -1;
    if (lane == 0) icnt[e][w] = __popcll(m);
  }
  __syncthreads();
  int nitems = 0;
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int c = lane < NW ? icnt[e][lane] : 0;
    const int incl = wave_incl_scan_x(c);
    const int base = nitems + __shfl(incl - c, w, 64);
    if (iex[e] >= 0) {
      const int x = e * NT + tid;
      items[base + iex[e]] = (x / kCubeNum) | ((x % kCubeNum) << 1) | (((int)vidx[x % kCubeNum] + 1) << 14);
    }
    nitems += __shfl(incl, NW - 1, 64);
  }
  vpts = block_reduce<NT>(vpts, scratch, [](int a, int c) { return a + c; });
  if (tid == 0) {
    b.nitems[p] = nitems;
    b.istate[(size_t)p * kMpStateInts + kMiValidPts] = vpts;
    if (run > b.map_cap) b.istate[(size_t)p * kMpStateInts + kMiErr] |= ERR_CAP_MAP;
  }
}

__global__ __launch_bounds__(256) void k_mp_compact_copy(MpBuffers b) {
  const int p = blockIdx.y;
  const int err = b.istate[(size_t)p * kMpStateInts + kMiErr];
  if (err & ERR_CAP_MAP) return;
  const int* old = slot_table(b, b.pool_cur, p);
  const int* nw = slot_table(b, 1 - b.pool_cur, p);
  const float4* pool = b.pool + ((size_t)b.pool_cur * b.P + p) * b.map_cap;
  float4* npool = b.pool + ((size_t)(1 - b.pool_cur) * b.P + p) * b.map_cap;
  const int* ao = b.app_off + (size_t)p * kCubeNum * 2;
  const float4* app = b.app + (size_t)p * b.cap_stack;
  const int* items = b.citems + (size_t)p * 2 * kCubeNum;
  const int nitems = b.nitems[p];
  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    const int code = items[it];
    const int kind = code & 1, s = (code >> 1) & 8191, v = (code >> 14) - 1;
    const int n = nw[s * 4 + 1 + 2 * kind];
    const int dst = nw[s * 4 + 2 * kind];
    if (v >= 0) {
      const int b0 = b.vseg_b[p * 2 * kMaxValid + kind * kMaxValid + v];
      for (int t = threadIdx.x; t < n; t += 256) npool[dst + t] = b.vout[b0 + t];
    } else {
      const int nold = old[s * 4 + 1 + 2 * kind], off = old[s * 4 + 2 * kind];
      for (int t = threadIdx.x; t < n; t += 256)
        npool[dst + t] = t < nold ? pool[off + t] : app[ao[s * 2 + kind] + (t - nold)];
    }
  }
}

// k_mp_register workgroups per instance (streaming and lanes; the batch registers nothing)
#ifndef LOAM_REG_WG
#define LOAM_REG_WG 8
#endif
constexpr int kMpRegWg = LOAM_REG_WG;
__global__ __launch_bounds__(256) void k_mp_register(MpBuffers b, MpInput in) {
  const int p = blockIdx.y;
  const loampose::MapRot r = rot_load(b, p);
  const int n = min(in.nfull[p * in.nfull_stride], b.capS);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256)
    b.reg[(size_t)p * b.capS + i] = loampose::point_to_map(r, in.full[(size_t)p * in.full_stride + i]);
  if (blockIdx.x == 0 && threadIdx.x == 0) b.nreg[p] = n;
}

}  // namespace

// ---------------------------------------------------------------- host side
hipError_t mp_alloc(MpBuffers& b, int P, int R, int cap_pts, int map_cap, int max_iter, bool batch) {
  DevAlloc A;
  b.P = P;
  b.capC = kLessSharpPerRing * R;
  b.capS = cap_pts;
  b.cap_stack = b.capC + b.capS;
  b.map_cap = map_cap;
  b.max_iter = max_iter;
  b.tmax = next_pow2(map_cap) > (1 << 20) ? (1 << 20) : next_pow2(map_cap);
  if (b.tmax < 64) b.tmax = 64;  // >= 64 buckets: a 3x3x3 search never lists a bucket twice (cell_hash)
  b.pool_cur = 0;
  const size_t Pm = (size_t)P * map_cap, Ps = (size_t)P * b.cap_stack;
  A(&b.state, (size_t)P * kMpStateFloats * sizeof(float));
  A(&b.istate, (size_t)P * kMpStateInts * sizeof(int));
  A(&b.slots, (size_t)2 * P * kCubeNum * 4 * sizeof(int));
  A(&b.pool, 2 * Pm * sizeof(float4));
  A(&b.valid, (size_t)P * kMaxValid * sizeof(int));
  A(&b.vpre, (size_t)P * (kMaxValid + 1) * 2 * sizeof(int));
  // (a batch set reads the odometry's Last buffers in place and registers no cloud: its inC / inS /
  // inF and reg / nreg stay null)
  if (!batch) {
    A(&b.inC, (size_t)P * b.capC * sizeof(float4));
    A(&b.inS, (size_t)P * b.capS * sizeof(float4));
    A(&b.inF, (size_t)P * b.capS * sizeof(float4));
  }
  A(&b.in_n, (size_t)P * 3 * sizeof(int));
  A(&b.in_pose, (size_t)P * 6 * sizeof(float));
  A(&b.stack2, Ps * sizeof(float4));
  A(&b.stack, Ps * sizeof(float4));
  A(&b.nstack, (size_t)P * 2 * sizeof(int));
  A(&b.from, Pm * sizeof(float4));
  A(&b.hC_start, (size_t)P * (b.tmax + 1) * sizeof(int));
  A(&b.hS_start, (size_t)P * (b.tmax + 1) * sizeof(int));
  A(&b.hC_rec, (size_t)P * b.tmax * sizeof(uint32_t));
  A(&b.hS_rec, (size_t)P * b.tmax * sizeof(uint32_t));
  // bucket counters: one set per cloud kind for small batches, whose two builds run together
  A(&b.h_fill, (size_t)2 * P * b.tmax * sizeof(int));  // (corner, surf: built concurrently)
  A(&b.hC_T, (size_t)P * sizeof(int));
  A(&b.hS_T, (size_t)P * sizeof(int));
  A(&b.hC_pts, Pm * sizeof(float4));
  A(&b.hS_pts, Pm * sizeof(float4));
  A(&b.nfrom, (size_t)P * 2 * sizeof(int));
  A(&b.q_ok, Ps * sizeof(int8_t));
  A(&b.q_cf, Ps * sizeof(float4));
  A(&b.q_nn, Ps * 2 * sizeof(int4));
  A(&b.citems, (size_t)P * 2 * kCubeNum * sizeof(int));
  A(&b.nitems, (size_t)P * sizeof(int));
  A(&b.q_fit, Ps * 4 * sizeof(float4));
  A(&b.app_cnt, (size_t)P * kCubeNum * 2 * sizeof(int));
  A(&b.app_off, (size_t)P * kCubeNum * 2 * sizeof(int));
  A(&b.app, Ps * sizeof(float4));
  A(&b.vin, Pm * sizeof(float4));
  A(&b.vout, Pm * sizeof(float4));
  A(&b.vseg_b, (size_t)P * 2 * kMaxValid * sizeof(int));
  A(&b.vseg_e, (size_t)P * 2 * kMaxValid * sizeof(int));
  A(&b.vseg_cnt, (size_t)P * 2 * kMaxValid * sizeof(int));
  A(&b.vseg_leaf, (size_t)P * 2 * kMaxValid * sizeof(float));
  A(&b.sseg_b, (size_t)P * 2 * sizeof(int));
  A(&b.sseg_e, (size_t)P * 2 * sizeof(int));
  A(&b.sseg_cnt, (size_t)P * 2 * sizeof(int));
  A(&b.sseg_leaf, (size_t)P * 2 * sizeof(float));
  A(&b.vg_lin, (size_t)P * 2 * kMaxValid * sizeof(int));
  A(&b.vg_mlist, (size_t)P * 2 * kMaxValid * sizeof(int));
  A(&b.vseg_nold, (size_t)P * 2 * kMaxValid * sizeof(int));
  A(&b.vseg_skip, (size_t)P * 2 * kMaxValid * sizeof(int));
  // the VoxelGrid scratch: sort arrays over the cube inputs or the stacks, a list entry per cube
  // segment; the stack job's big-segment split: 2P parents, points / outputs like the stacks
  if (A.err == hipSuccess) A.err = vg_scratch_alloc(b.vg, std::max(Pm, Ps), (size_t)P * 2 * kMaxValid, 2 * P, Ps);
  if (!batch) A(&b.reg, (size_t)P * b.capS * sizeof(float4));
  A(&b.part, (size_t)P * std::max(kMpSmallGrid, kMpFitGridMax) * 28 * sizeof(double));
  A(&b.rot, (size_t)P * 6 * sizeof(double));
  A(&b.done, (size_t)P * sizeof(int));
  A(&b.ls_part, (size_t)2 * kMpSmallGrid * 28 * sizeof(double));
  A(&b.ls_flag, (size_t)kMpSmallGrid * sizeof(unsigned long long));
  A(&b.ls_epoch, sizeof(unsigned long long));
  if (!batch) A(&b.nreg, (size_t)P * sizeof(int));
  if (A.err == hipSuccess) A.err = mp_reset(b, nullptr);
  if (A.err == hipSuccess) A.err = hipMemset(b.ls_flag, 0, (size_t)kMpSmallGrid * sizeof(unsigned long long));
  if (A.err == hipSuccess) A.err = hipMemset(b.ls_epoch, 0, sizeof(unsigned long long));
  if (A.err == hipSuccess) A.err = hipDeviceSynchronize();
  if (A.err != hipSuccess) mp_free(b);
  return A.err;
}

void mp_free(MpBuffers& b) {
  void* ptrs[] = {b.state, b.istate, b.slots, b.pool, b.valid, b.vpre, b.inC, b.inS, b.inF, b.in_n, b.in_pose,
                  b.stack2, b.stack, b.nstack, b.from, b.hC_start, b.hS_start, b.hC_rec, b.hS_rec, b.h_fill, b.hC_T, b.hS_T,
                  b.hC_pts, b.hS_pts, b.nfrom, b.q_ok, b.q_cf, b.q_nn, b.q_fit, b.citems, b.nitems, b.app_cnt, b.app_off, b.app, b.vin, b.vout,
                  b.vseg_b, b.vseg_e, b.vseg_cnt, b.vseg_leaf, b.sseg_b, b.sseg_e, b.sseg_cnt, b.sseg_leaf,
                  b.vg_lin, b.reg, b.nreg, b.part, b.done, b.rot, b.vg_mlist, b.vseg_nold, b.vseg_skip, b.ls_part,
                  b.ls_flag, b.ls_epoch};
  if (b.upd_pending && b.upd_done) (void)hipEventSynchronize(b.upd_done);
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  vg_scratch_free(b.vg);
  if (b.upd_fork) (void)hipEventDestroy(b.upd_fork);
  if (b.upd_done) (void)hipEventDestroy(b.upd_done);
  b = MpBuffers();
}

__global__ void k_mp_reset(MpBuffers b) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= b.P) return;
  int* ist = b.istate + (size_t)p * kMpStateInts;
  ist[kMiCenW] = 10; ist[kMiCenH] = 5; ist[kMiCenD] = 10;  // :64-66
}

hipError_t mp_reset(MpBuffers& b, hipStream_t st, bool both_tables) {
  mp_wait_update(b, st);
  b.pool_cur = 0;
  hipError_t e = hipMemsetAsync(b.state, 0, (size_t)b.P * kMpStateFloats * sizeof(float), st);
  if (e == hipSuccess) e = hipMemsetAsync(b.done, 0, (size_t)b.P * sizeof(int), st);
  if (e == hipSuccess) e = hipMemsetAsync(b.istate, 0, (size_t)b.P * kMpStateInts * sizeof(int), st);
  // (pool 0's slot table first: the one the next frame reads)
  if (e == hipSuccess) e = hipMemsetAsync(b.slots, 0, (size_t)(both_tables ? 2 : 1) * b.P * kCubeNum * 4 * sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mp_reset, dim3((b.P + 255) / 256), dim3(256), 0, st, b);
  return hipGetLastError();
}

void mp_wait_update(MpBuffers& b, hipStream_t st) {
  if (!b.upd_pending) return;
  b.note(hipStreamWaitEvent(st, b.upd_done, 0));
  b.upd_pending = false;
}

namespace {
// The middle of a mapping frame, shared by mp_frame and the localization (mp_localize_solve), for
// the P instances of b: the stack VoxelGrid, the FromMap hash builds, the L-M loop.

// the stacks' VoxelGrid (:693-701) on vs (k_mp_stack zeroed the cascade's list counters)
void mp_stack_vg(MpBuffers& b, int P, hipStream_t vs, int stack_max) {
  VgJob js = b.vg.job();
  js.in = b.stack2; js.out = b.stack; js.begin = b.sseg_b; js.end = b.sseg_e; js.leaf = b.sseg_leaf;
  js.out_count = b.sseg_cnt; js.nseg = 2 * P; js.total = P * b.cap_stack;
  // two large segments per instance (the fused 12288-point kernel); when the host knows both fit
  // (streaming), the cascade's finish is not enqueued
  // (k_mp_stack zeroed the cascade's list counters)
  js.zeroed = true;
  b.note(vg_route_stack(js, vs, P, stack_max, b.tune.vg_split, b.capS, &b.vg.split));
}

// the 1 m voxel hashes of FromMap's corner and surf parts
void mp_hash_from(MpBuffers& b, int P, hipStream_t st, bool spread = false) {
  HashJob hc;
  hc.pts = b.from; hc.pts_stride = b.map_cap; hc.pts_off = nullptr; hc.pts_off_stride = 0;
  hc.count = b.nfrom; hc.count_stride_bytes = 2 * sizeof(int);
  hc.start = b.hC_start; hc.fill = b.h_fill; hc.out = b.hC_pts; hc.tsize = b.hC_T; hc.tmax = b.tmax;
  hc.inv_h = 1.0f;
  hc.shift = 0;  // the 5-NN search scans whole buckets: keep them to single cells
  hc.chunks = nullptr;
  hc.rec = b.hC_rec;
  HashJob hs = hc;
  hs.rec = b.hS_rec;
  hs.pts_off = b.nfrom; hs.pts_off_stride = 2;
  hs.count = b.nfrom + 1; hs.start = b.hS_start; hs.out = b.hS_pts; hs.tsize = b.hS_T;
  hs.fill = b.h_fill + (size_t)P * b.tmax;  // (the two indexes are built in one launch / concurrently)
  hash_build_pair(hc, hs, P, st, false, spread ? HashForm::kGrid : HashForm::kAuto);
}

// k_mp_lm_begin, the iterations, k_mp_lm_end; persist: one instance may take the persistent launch
// (tuning mp_persist)
void mp_lm_loop(MpBuffers& b, int P, hipStream_t st, Prof* prof, bool map_empty, bool persist) {
  auto mark = [&](const char* n) { if (prof) prof->mark(n); };
  hipLaunchKernelGGL(k_mp_lm_begin, dim3((P + 255) / 256), dim3(256), 0, st, b);
  // workgroups per instance: all the stack's queries at once for a few instances; for large
  // batches about one pass over a VLP-16 stack (bigger stacks loop), fewer idle workgroups
  const int gq = std::min(P >= 64 ? 24 : 64, (b.cap_stack + kMpQueryThreads - 1) / kMpQueryThreads);
  // an empty map store (the first frame after a reset) cannot run the L-M (:706): no launches
  // one instance (streaming): the whole L-M loop as one persistent launch (tuning mp_persist)
  const int gls = persist && P == 1 && !map_empty && b.tune.mp_persist ? mp_lm_stream_grid() : 0;
  if (gls > 0) {
    hipLaunchKernelGGL(k_mp_lm_stream, dim3(gls), dim3(kMpQueryThreads), 0, st, b);
    mark("k_mp_lm_stream");
  }
  for (int it = 0; it < (map_empty || gls > 0 ? 0 : b.max_iter); ++it) {
    if (P <= b.tune.mp_small_max) {  // small batches: one launch per iteration
      hipLaunchKernelGGL(k_mp_lm_small, dim3(kMpSmallGrid, P), dim3(kMpQueryThreads), 0, st, b);
      mark("k_mp_lm_small");
      continue;
    }
    // (P >= 512: 64 workgroups, two passes per lane over a VLP-16 stack; round 6 at 1024 problems:
    // 12.28-12.32 -> 12.20-12.23 ms/step against 96; at 128 the one-pass 96 stays best)
    const int gfit_auto = P >= 512 ? 64 : gq * (kMpQueryThreads / kMpFitThreads);
    const int gfit = std::min(kMpFitGridMax, b.tune.fit_wg > 0 ? b.tune.fit_wg : gfit_auto);
    // search + fit (+ step) in one launch (round 3's separate k_mp_nn / k_mp_fit launches, and 2 / 4
    // lanes per query, measured slower and were removed in round 6)
    const bool fused = P <= b.tune.mp_fused_max;
    if (fused && prof) hipLaunchKernelGGL((k_mp_nnfit<true, true>), dim3(gfit, P), dim3(kMpFitThreads), 0, st, b);
    else if (fused) hipLaunchKernelGGL((k_mp_nnfit<true, false>), dim3(gfit, P), dim3(kMpFitThreads), 0, st, b);
    else if (prof) hipLaunchKernelGGL((k_mp_nnfit<false, true>), dim3(gfit, P), dim3(kMpFitThreads), 0, st, b);
    else hipLaunchKernelGGL((k_mp_nnfit<false, false>), dim3(gfit, P), dim3(kMpFitThreads), 0, st, b);
    mark("k_mp_nnfit");
    if (!fused) {
      hipLaunchKernelGGL(k_mp_iter<kMpThreads>, dim3(P), dim3(kMpThreads), 0, st, b);
      mark("k_mp_iter");
    }
  }
  hipLaunchKernelGGL(k_mp_lm_end, dim3((P + 255) / 256), dim3(256), 0, st, b);
}
}  // namespace

// ---- the stages of a mapping frame; every caller composes the ones whose results it hands out ----
namespace {
// front: the pose and the valid cubes, the stacks and their VoxelGrid, FromMap and its hashes.
// from_map = false: the store was just reset (batch frame 1), FromMap is empty by construction and
// neither gathered nor hashed (k_mp_prepare has set nfrom and the valid count to 0; no L-M runs)
void mp_front(MpBuffers& b, const MpInput& in, hipStream_t st, Prof* prof, int stack_max, const SideStream* side,
              bool from_map) {
  const int P = b.P;
  auto mark = [&](const char* n) { if (prof) prof->mark(n); };
  mp_wait_update(b, st);  // (the previous frame's map update, when it was deferred)
  hipLaunchKernelGGL(k_mp_prepare, dim3(P), dim3(kMpThreads), 0, st, b, in);
  mark("k_mp_prepare");
  hipLaunchKernelGGL(k_mp_stack, dim3(16, P), dim3(256), 0, st, b, in);
  mark("k_mp_stack");
  if (side && side->inputs_read) b.note(hipEventRecord(side->inputs_read, st));  // (in.corner / in.surf read)
  // the stack VoxelGrid: with a side stream it runs there, beside the FromMap gather and the map
  // hash builds (which read only the store)
  const bool fork = side && side->st && !prof && from_map;
  if (fork) {
    b.note(hipEventRecord(side->fork, st));
    b.note(hipStreamWaitEvent(side->st, side->fork, 0));
  }
  mp_stack_vg(b, P, fork ? side->st : st, stack_max);
  if (fork) b.note(hipEventRecord(side->join, side->st));
  mark("vg_stack");
  if (!from_map) return;
  hipLaunchKernelGGL(k_mp_gather, dim3(32, P), dim3(256), 0, st, b);
  mark("k_mp_gather");
  mp_hash_from(b, P, st);
  mark("k_hash_build_map");
  if (fork) b.note(hipStreamWaitEvent(st, side->join, 0));
}

// the map update on us: insertion + per-valid-cube downsampling into the other pool, which becomes
// the current one (k_mp_lm_end zeroed the cascade's list counters)
void mp_update(MpBuffers& b, hipStream_t us, Prof* prof) {
  const int P = b.P;
  auto mark = [&](const char* n) { if (prof) prof->mark(n); };
  // a few instances: 1024 threads per instance (the per-instance serial parts are the cost)
  // 1024 threads per instance also for batches (k_mp_insert 0.40 -> 0.25 ms/step at batch 1024 against 256)
  hipLaunchKernelGGL(k_mp_insert<1024>, dim3(P), dim3(1024), 0, us, b, (int*)b.vg.keys, (int*)b.vg.vals);
  mark("k_mp_insert");
  hipLaunchKernelGGL(k_mp_vseg, dim3(P), dim3(kMpThreads), 0, us, b);
  hipLaunchKernelGGL(k_mp_vcopy, dim3(32, P), dim3(256), 0, us, b);
  mark("k_mp_vseg_vcopy");
  VgJob jv = b.vg.job();
  jv.in = b.vin; jv.out = b.vout; jv.begin = b.vseg_b; jv.end = b.vseg_e; jv.leaf = b.vseg_leaf;
  jv.out_count = b.vseg_cnt; jv.nseg = 2 * kMaxValid * P; jv.total = P * b.map_cap;
  // only the non-empty segments, listed by k_mp_vseg (k_mp_lm_end zeroed the counters)
  jv.list = b.vg_lin; jv.list_n = b.vg.counts + 2; jv.zeroed = true;
  b.note(vg_route_cubes(jv, us, P, b.tune.vg_merge, b.vseg_nold, b.vg_mlist, b.vg.counts + 3, b.vseg_skip));
  mark("vg_cubes");
  hipLaunchKernelGGL(k_mp_compact_table<1024>, dim3(P), dim3(1024), 0, us, b);
  hipLaunchKernelGGL(k_mp_compact_copy, dim3(64, P), dim3(256), 0, us, b);
  mark("k_mp_compact");
  b.pool_cur = 1 - b.pool_cur;
}
}  // namespace

void mp_frame(MpBuffers& b, const MpInput& in, hipStream_t st, Prof* prof,
              const std::function<void()>& before_register, int stack_max, hipStream_t defer) {
  mp_front(b, in, st, prof, stack_max, nullptr, /*from_map=*/true);
  mp_lm_loop(b, b.P, st, prof, false, /*persist=*/true);
  // defer: the map update on the other stream, forked here; the registration stays on st
  if (defer) {
    if (!b.upd_fork) b.note(hipEventCreateWithFlags(&b.upd_fork, hipEventDisableTiming));
    if (!b.upd_done) b.note(hipEventCreateWithFlags(&b.upd_done, hipEventDisableTiming));
    b.note(hipEventRecord(b.upd_fork, st));
    b.note(hipStreamWaitEvent(defer, b.upd_fork, 0));
  }
  mp_update(b, defer ? defer : st, prof);
  if (defer) {
    b.note(hipEventRecord(b.upd_done, defer));
    b.upd_pending = true;
  }
  if (before_register) before_register();
  // (reads the final pose and the full cloud only, not the store)
  hipLaunchKernelGGL(k_mp_register, dim3(kMpRegWg, b.P), dim3(256), 0, st, b, in);
  if (prof) prof->mark("k_mp_register");
}

template <typename Hook>
int mp_stream_run(MpBuffers& b, hipStream_t st, const MpInput& in, const int* n, loam_pose6* aft, loam_pose6* bef,
                  loam_cloud_out* registered, loam_stats* stats, std::string& err, Staging& pin, const StreamIo& io,
                  bool* updated, Hook hook, hipStream_t defer);

int mp_stream_frame(MpBuffers& b, hipStream_t st, const loam_pose6& odom_sum, const loam_cloud_out& corner,
                    const loam_cloud_out& surf, const loam_cloud_out& full, loam_pose6* aft, loam_pose6* bef,
                    loam_cloud_out* registered, loam_stats* stats, std::string& err, Staging& pin, const StreamIo& io,
                    const float* imu_rp, bool* updated, hipStream_t st2, hipEvent_t ev2, hipStream_t defer) {
  if (corner.count > (uint32_t)b.capC || surf.count > (uint32_t)b.capS || full.count > (uint32_t)b.capS) {
    err = "mapping input cloud exceeds capacity";
    return LOAM_E_CAPACITY;
  }
  if ((corner.count && !corner.pts) || (surf.count && !surf.pts) || (full.count && !full.pts)) {
    err = "mapping input cloud pts is null";
    return LOAM_E_INVAL;
  }
  // host inputs: [0..2] counts, [4..9] pose, [10..11] IMU (roll, pitch), [12] IMU flag, to the
  // device in one k_xfer launch; downloads through io.xb (mp_stream_run)
  int mi[16];
  int* n = mi;
  n[0] = (int)corner.count; n[1] = (int)surf.count; n[2] = (int)full.count;
  std::memcpy(mi + 4, &odom_sum, 6 * sizeof(float));
  const float rp[2] = {imu_rp ? imu_rp[0] : 0.0f, imu_rp ? imu_rp[1] : 0.0f};
  std::memcpy(mi + 10, rp, sizeof(rp));
  mi[12] = imu_rp ? 1 : 0;
  pin.reset();
  // room for all three clouds now: the full cloud is staged later, while the kernels run
  hipError_t ue = pin.reserve((size_t)n[0] + n[1] + n[2], st);
  if (ue == hipSuccess) ue = pin.up(st, b.inC, corner.pts, (size_t)n[0]);
  if (ue == hipSuccess) ue = pin.up(st, b.inS, surf.pts, (size_t)n[1]);
  // only k_mp_register reads the full cloud: with a second stream its staging copy and DMA
  // overlap the frame's kernels (enqueued just before k_mp_register)
  const bool late = st2 != nullptr && n[2] > 0;
  if (ue == hipSuccess && !late) ue = pin.up(st, b.inF, full.pts, (size_t)n[2]);
  if (ue == hipSuccess) {
    Xfer xp;
    xp.put(b.in_n, n, 3 * sizeof(int));
    xp.put(b.in_pose, mi + 4, 6 * sizeof(float));
    xp.put(b.state + kMpImuRP, mi + 10, 2 * sizeof(float));
    xp.put(b.istate + kMiImu, mi + 12, sizeof(int));
    ue = xfer_launch(xp, st);
  }
  if (ue != hipSuccess) {
    err = std::string("mapping upload: ") + hipGetErrorString(ue);
    return LOAM_E_HIP;
  }
  MpInput in;
  in.corner = b.inC; in.surf = b.inS; in.full = b.inF;
  in.corner_stride = b.capC; in.surf_stride = b.capS; in.full_stride = b.capS;
  in.ncorner = b.in_n; in.nsurf = b.in_n + 1; in.nfull = b.in_n + 2;
  in.ncorner_stride = in.nsurf_stride = in.nfull_stride = 3;
  in.pose = b.in_pose; in.pose_stride = 6;
  return mp_stream_run(b, st, in, n, aft, bef, registered, stats, err, pin, io, updated, [&]() {
    if (!late) return hipSuccess;
    hipError_t le = pin.up(st2, b.inF, full.pts, (size_t)n[2]);
    if (le == hipSuccess) le = hipEventRecord(ev2, st2);
    if (le == hipSuccess) le = hipStreamWaitEvent(st, ev2, 0);
    return le;
  }, defer);
}

// the device-resident chain (loam_chain_sweep): the clouds are already on the device (odometry's
// published Last / full-end buffers, src, with device counts); n3: their counts on the host
int mp_stream_frame_dev(MpBuffers& b, hipStream_t st, const loam_pose6& odom_sum, const MpInput& src, const int* n3,
                        loam_pose6* aft, loam_pose6* bef, loam_cloud_out* registered, loam_stats* stats,
                        std::string& err, Staging& pin, const StreamIo& io, const float* imu_rp, bool* updated,
                        hipStream_t defer) {
  if (n3[0] > b.capC || n3[1] > b.capS || n3[2] > b.capS) {
    err = "mapping input cloud exceeds capacity";
    return LOAM_E_CAPACITY;
  }
  // as mp_stream_frame: the pose, the IMU (roll, pitch) and flag in one k_xfer launch
  const float rp[2] = {imu_rp ? imu_rp[0] : 0.0f, imu_rp ? imu_rp[1] : 0.0f};
  const int flag = imu_rp ? 1 : 0;
  Xfer xp;
  xp.put(b.in_pose, &odom_sum, 6 * sizeof(float));
  xp.put(b.state + kMpImuRP, rp, sizeof(rp));
  xp.put(b.istate + kMiImu, &flag, sizeof(int));
  const hipError_t ue = xfer_launch(xp, st);
  if (ue != hipSuccess) {
    err = std::string("mapping upload: ") + hipGetErrorString(ue);
    return LOAM_E_HIP;
  }
  MpInput in = src;
  in.pose = b.in_pose;
  in.pose_stride = 6;
  return mp_stream_run(b, st, in, n3, aft, bef, registered, stats, err, pin, io, updated,
                       []() { return hipSuccess; }, defer);
}

// the frame's kernels on `in` and the downloads (both stream entry points); hook: called just
// before k_mp_register (the late full-cloud staging); defer: the map update's stream (mp_frame),
// nullptr = in order on st
template <typename Hook>
int mp_stream_run(MpBuffers& b, hipStream_t st, const MpInput& in, const int* n, loam_pose6* aft, loam_pose6* bef,
                  loam_cloud_out* registered, loam_stats* stats, std::string& err, Staging& pin, const StreamIo& io,
                  bool* updated, Hook hook, hipStream_t defer) {
  const hipEvent_t e0 = io.e0, e1 = io.e1;
  hipError_t le = hipEventRecord(e0, st);
  mp_frame(b, in, st, nullptr, [&]() {
    if (le != hipSuccess) return;
    le = hook();
  }, std::max(n[0], n[1]), defer);
  if (le == hipSuccess) le = hipEventRecord(e1, st);
  // a deferred update's valid-point count (stats) into the mapped host block after it, one slot
  // per frame parity: this call reads the previous frame's (complete: this frame's kernels on st
  // waited for that update), while this frame's may still be writing the other slot
  const bool deferred = defer && b.upd_pending;
  if (deferred && le == hipSuccess) {
    Xfer xg;
    xg.get(io.xb.d + kXferMpUpd + 4 * (1 - b.pool_cur), b.istate + kMiValidPts, sizeof(int));
    le = xfer_launch(xg, defer);
    if (le == hipSuccess) le = hipEventRecord(b.upd_done, defer);
  }
  // state (kMpStateFloats), istate (kMpStateInts), nreg into the mapped host block, one launch
  static_assert(kXferMp + 4 * (kMpStateFloats + kMpStateInts + 1) <= kXferMpUpd, "mapping transfer region");
  static_assert(kXferMpUpd + 8 <= kXferBytes, "deferred valid-point slots");
  const float* sf = (const float*)(io.xb.h + kXferMp);
  const int* si = (const int*)(io.xb.h + kXferMp) + kMpStateFloats;
  const int* pnreg = si + kMpStateInts;
  {
    Xfer xg;
    char* d = io.xb.d + kXferMp;
    xg.get(d, b.state, kMpStateFloats * sizeof(float));
    xg.get(d + kMpStateFloats * 4, b.istate, kMpStateInts * sizeof(int));
    xg.get(d + (kMpStateFloats + kMpStateInts) * 4, b.nreg, sizeof(int));
    le = le == hipSuccess ? xfer_launch(xg, st) : le;
  }
  hipError_t he = hipGetLastError();
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  const int nreg = *pnreg;
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  if (he == hipSuccess) he = b.take_error();
  if (he == hipSuccess) he = le;
  if (he != hipSuccess) {
    err = std::string("mapping: ") + hipGetErrorString(he);
    return LOAM_E_HIP;
  }
  if (si[kMiErr]) {
    err = "mapping capacity exceeded (map store / stack)";
    return LOAM_E_CAPACITY;
  }
  std::memcpy(aft, sf + kMpAft, sizeof(loam_pose6));
  std::memcpy(bef, sf + kMpBef, sizeof(loam_pose6));
  if (updated) *updated = si[kMiLmRan] != 0;
  int rc = LOAM_OK;
  if (registered) {
    if ((uint32_t)nreg > registered->capacity) {
      registered->count = (uint32_t)nreg;
      err = "registered cloud capacity too small";
      rc = LOAM_E_CAPACITY;
    } else {
      registered->count = (uint32_t)nreg;
      pin.reset();
      he = pin.down(st, registered->pts, b.reg, (size_t)nreg);
      if (he == hipSuccess) he = hipStreamSynchronize(st);
      if (he != hipSuccess) {
        err = std::string("registered cloud download: ") + hipGetErrorString(he);
        return LOAM_E_HIP;
      }
      pin.finish();
    }
  }
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->mp_iters = si[kMiIters];
    stats->mp_rows_sum = (uint64_t)si[kMiRows];
    stats->mp_stack = (uint64_t)(si[kMiStackC] + si[kMiStackS]);
    stats->mp_stack_iters = (uint64_t)si[kMiIters] * (si[kMiStackC] + si[kMiStackS]);
    stats->mp_fits = (uint64_t)si[kMiFits];
    stats->mp_map_points = (uint64_t)(si[kMiFromC] + si[kMiFromS]);
    // (a deferred update: the previous frame's map, this frame's is not counted yet)
    stats->mp_map_valid_points =
        (uint64_t)(deferred ? *(const int*)(io.xb.h + kXferMpUpd + 4 * b.pool_cur) : si[kMiValidPts]);
    stats->mp_degenerate_steps = (uint64_t)si[kMiDegSteps];
    stats->mp_grid_shifts = (uint64_t)si[kMiShifts];
    stats->mp_nn_candidates = (uint64_t)(uint32_t)si[kMiNnCand];
    stats->mp_nn_cells = (uint64_t)(uint32_t)si[kMiNnCells];
    stats->ms_mp = ms;
  }
  return rc;
}

// /laser_cloud_surround input (:1042-1047): every in-bounds cube of the 5x5x5 neighbourhood of the
// frame's centre cube (laserCloudSurroundInd, :617-670, FOV test or not) in (i, j, k) loop order,
// each cube's corner points then its surf points, from the store the frame left; one VoxelGrid
// segment (leaf 0.2, downSizeFilterCorner) over vin.
__global__ __launch_bounds__(256) void k_mp_surround(MpBuffers b) {
  const int tid = threadIdx.x;
  if (tid == 0) { b.vg.counts[0] = 0; b.vg.counts[1] = 0; }  // (its VoxelGrid's lists)
  const int* ist = b.istate;
  const int* slots = slot_table(b, b.pool_cur, 0);
  const float4* pool = b.pool + (size_t)b.pool_cur * b.P * b.map_cap;
  __shared__ int sh_ind[kMaxValid], sh_pre[kMaxValid + 1], sh_n;
  if (tid == 0) {
    const int cI = ist[kMiCubeI], cJ = ist[kMiCubeJ], cK = ist[kMiCubeK];
    int n = 0, acc = 0;
    for (int i = cI - 2; i <= cI + 2; ++i)
      for (int j = cJ - 2; j <= cJ + 2; ++j)
        for (int k = cK - 2; k <= cK + 2; ++k) {
          if (!(i >= 0 && i < kCubeW && j >= 0 && j < kCubeH && k >= 0 && k < kCubeD)) continue;
          const int ind = cube_index(i, j, k);
          sh_ind[n] = ind;
          sh_pre[n] = acc;
          acc += slots[ind * 4 + 1] + slots[ind * 4 + 3];
          ++n;
        }
    sh_pre[n] = acc;
    sh_n = n;
    b.vseg_b[0] = 0;
    b.vseg_e[0] = acc;
    b.vseg_leaf[0] = 0.2f;
  }
  __syncthreads();
  const int n = sh_n;
  for (int c = 0; c < n; ++c) {
    const int ind = sh_ind[c], nc = slots[ind * 4 + 1], ns = slots[ind * 4 + 3];
    const int oc = slots[ind * 4 + 0], os = slots[ind * 4 + 2];
    float4* dst = b.vin + sh_pre[c];
    for (int t = tid; t < nc + ns; t += 256) dst[t] = t < nc ? pool[oc + t] : pool[os + (t - nc)];
  }
}

int mp_stream_surround(MpBuffers& b, hipStream_t st, loam_cloud_out* out, std::string& err) {
  mp_wait_update(b, st);  // (the last frame's map update, when deferred)
  hipLaunchKernelGGL(k_mp_surround, dim3(1), dim3(256), 0, st, b);
  VgJob j = b.vg.job();
  j.in = b.vin; j.out = b.vout; j.begin = b.vseg_b; j.end = b.vseg_e; j.leaf = b.vseg_leaf;
  j.out_count = b.vseg_cnt; j.nseg = 1; j.total = b.P * b.map_cap;
  j.zeroed = true;  // (by k_mp_surround)
  b.note(vg_route_surround(j, st));
  int cnt = 0;
  hipError_t he = hipMemcpyAsync(&cnt, b.vseg_cnt, sizeof(int), hipMemcpyDeviceToHost, st);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he == hipSuccess) he = b.take_error();
  if (he != hipSuccess) {
    err = std::string("surround: ") + hipGetErrorString(he);
    return LOAM_E_HIP;
  }
  if ((uint32_t)cnt > out->capacity) {
    out->count = (uint32_t)cnt;
    err = "surround cloud capacity too small";
    return LOAM_E_CAPACITY;
  }
  out->count = (uint32_t)cnt;
  if (cnt && hipMemcpy(out->pts, b.vout, (size_t)cnt * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) {
    err = "surround download failed";
    return LOAM_E_HIP;
  }
  return LOAM_OK;
}

// ---------------------------------------------------------------- map export / import
// (mp.hpp: MapIo, the canonical order).  Export: k_mp_map_table turns the slot table (in no
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

// ---------------------------------------------------------------- localization: host side
namespace {
// a candidate's result block (kLr* words): what a mapping frame at this candidate would return in
// aft (k_mp_lm_end left it in the state; untouched without an L-M) and report in its statistics
__global__ void k_mp_loc_result(MpBuffers w, int* res) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= w.P) return;
  const int* ist = w.istate + (size_t)p * kMpStateInts;
  const float* st = w.state + (size_t)p * kMpStateFloats;
  int* r = res + (size_t)p * kLocResWords;
  const bool off = ist[kMiLocOff] != 0, ran = ist[kMiLmRan] != 0;
  for (int k = 0; k < 6; ++k) r[kLrAft + k] = __float_as_int(st[kMpAft + k]);
  r[kLrStatus] = off ? 2 : (ran ? 0 : 1);  // LOAM_LOC_OFFGRID / SOLVED / NO_LM
  r[kLrIters] = ist[kMiIters];
  r[kLrDegSteps] = ist[kMiDegSteps];
  r[kLrRowsLast] = ist[kMiRowsLast];
  r[kLrRowsSum] = ist[kMiRows];
  r[kLrStackC] = off ? 0 : ist[kMiStackC];
  r[kLrStackS] = off ? 0 : ist[kMiStackS];
  r[kLrMapC] = ist[kMiFromC];
  r[kLrMapS] = ist[kMiFromS];
}

LocStore loc_store(const MpBuffers& s) {
  LocStore v;
  v.slots = s.slots + (size_t)s.pool_cur * s.P * kCubeNum * 4;
  v.pool = s.pool + (size_t)s.pool_cur * s.P * s.map_cap;
  v.istate = s.istate;
  v.map_cap = s.map_cap;
  return v;
}

void loc_free_map(MpBuffers& w) {
  void* ptrs[] = {w.from, w.hC_start, w.hS_start, w.hC_rec, w.hS_rec, w.h_fill, w.hC_pts, w.hS_pts};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  w.from = w.hC_pts = w.hS_pts = nullptr;
  w.hC_start = w.hS_start = w.h_fill = nullptr;
  w.hC_rec = w.hS_rec = nullptr;
  w.map_cap = w.tmax = 0;
}
}  // namespace

void mp_loc_free(MpLoc& L) {
  mp_free(L.w);
  if (L.cand) (void)hipFree(L.cand);
  if (L.head) (void)hipFree(L.head);
  if (L.res) (void)hipFree(L.res);
  if (L.pin) (void)hipHostFree(L.pin);
  if (L.plan) (void)hipFree(L.plan);
  if (L.plan_pin) (void)hipHostFree(L.plan_pin);
  L = MpLoc();
}

hipError_t mp_loc_reserve_rows(MpLoc& L) {
  if (L.plan_pin) return hipSuccess;
  DevAlloc A;
  A(&L.plan, (size_t)kLocMax * sizeof(LaneLocPlan));
  if (A.err == hipSuccess)
    A.err = hipHostMalloc((void**)&L.plan_pin, (size_t)kLocMax * (kOdBufs * 2 * sizeof(int) + sizeof(LaneLocPlan)),
                          hipHostMallocDefault);
  if (A.err != hipSuccess) {
    if (L.plan) (void)hipFree(L.plan);
    L.plan = nullptr;
    L.plan_pin = nullptr;
  }
  return A.err;
}

hipError_t mp_loc_reserve(MpLoc& L, const MpBuffers& s, int n, int ncorner, int nsurf) {
  if (!L.pin) {
    DevAlloc A;
    A(&L.cand, (size_t)kLocMax * 12 * sizeof(float));
    A(&L.head, (size_t)(2 * kLocMax + 4) * sizeof(int));
    A(&L.res, (size_t)kLocMax * kLocResWords * sizeof(int));
    if (A.err == hipSuccess)
      A.err = hipHostMalloc((void**)&L.pin, (size_t)kLocMax * (12 + 2 + kLocResWords) * 4 + 16, hipHostMallocDefault);
    if (A.err != hipSuccess) {
      mp_loc_free(L);
      return A.err;
    }
  }
  MpBuffers& w = L.w;
  w.tune = s.tune;
  w.max_iter = s.max_iter;
  // the stacks hold the sweep given, not the context's max_points (193 B per stack point and
  // candidate): its counts rounded up, at most the store's own capacities
  const int needC = std::min(s.capC, (std::max(ncorner, 1) + 511) / 512 * 512);
  const int needS = std::min(s.capS, (std::max(nsurf, 1) + 4095) / 4096 * 4096);
  if (n <= L.cap_n && needC <= w.capC && needS <= w.capS) return hipSuccess;
  const int capC = std::max(needC, w.capC), capS = std::max(needS, w.capS), cap_stack = capC + capS;
  // the stacks' segment bases and the VoxelGrid job's size are ints over all the candidates
  if ((size_t)n * cap_stack > (size_t)0x7fffffff) return hipErrorOutOfMemory;
  const int P = std::max(L.cap_n, n <= 4 ? 4 : std::min(kLocMax, next_pow2(n)));
  const int Pc = (size_t)P * cap_stack > (size_t)0x7fffffff ? std::max(n, L.cap_n) : P;
  mp_free(w);
  L.cap_n = L.from_cap = 0;
  DevAlloc A;
  w.P = Pc;
  w.capC = capC; w.capS = capS; w.cap_stack = cap_stack;
  w.max_iter = s.max_iter;
  w.tune = s.tune;
  const size_t Ps = (size_t)Pc * w.cap_stack;
  A(&w.state, (size_t)Pc * kMpStateFloats * sizeof(float));
  A(&w.istate, (size_t)Pc * kMpStateInts * sizeof(int));
  A(&w.valid, (size_t)Pc * kMaxValid * sizeof(int));
  A(&w.vpre, (size_t)Pc * (kMaxValid + 1) * 2 * sizeof(int));
  A(&w.nfrom, (size_t)Pc * 2 * sizeof(int));
  A(&w.hC_T, (size_t)Pc * sizeof(int));
  A(&w.hS_T, (size_t)Pc * sizeof(int));
  // the sweep's two clouds, once for every candidate
  A(&w.inC, (size_t)w.capC * sizeof(float4));
  A(&w.inS, (size_t)w.capS * sizeof(float4));
  A(&w.in_n, 3 * sizeof(int));
  A(&w.in_pose, 6 * sizeof(float));
  A(&w.stack2, Ps * sizeof(float4));
  A(&w.stack, Ps * sizeof(float4));
  A(&w.sseg_b, (size_t)Pc * 2 * sizeof(int));
  A(&w.sseg_e, (size_t)Pc * 2 * sizeof(int));
  A(&w.sseg_cnt, (size_t)Pc * 2 * sizeof(int));
  A(&w.sseg_leaf, (size_t)Pc * 2 * sizeof(float));
  // (two stack segments per candidate, each a parent of the split)
  if (A.err == hipSuccess) A.err = vg_scratch_alloc(w.vg, Ps, (size_t)Pc * 2, 2 * Pc, Ps);
  A(&w.q_ok, Ps * sizeof(int8_t));
  A(&w.q_cf, Ps * sizeof(float4));
  A(&w.q_nn, Ps * 2 * sizeof(int4));
  A(&w.q_fit, Ps * 4 * sizeof(float4));
  A(&w.part, (size_t)Pc * std::max(kMpSmallGrid, kMpFitGridMax) * 28 * sizeof(double));
  A(&w.rot, (size_t)Pc * 6 * sizeof(double));
  A(&w.done, (size_t)Pc * sizeof(int));
  A(&w.ls_epoch, sizeof(unsigned long long));  // (k_mp_lm_begin advances it for one instance)
  if (A.err == hipSuccess) A.err = hipMemset(w.state, 0, (size_t)Pc * kMpStateFloats * sizeof(float));
  if (A.err == hipSuccess) A.err = hipMemset(w.istate, 0, (size_t)Pc * kMpStateInts * sizeof(int));
  if (A.err == hipSuccess) A.err = hipMemset(w.done, 0, (size_t)Pc * sizeof(int));
  if (A.err == hipSuccess) A.err = hipMemset(w.ls_epoch, 0, sizeof(unsigned long long));
  if (A.err != hipSuccess) {
    mp_free(w);
    return A.err;
  }
  L.cap_n = Pc;
  return hipSuccess;
}

hipError_t mp_loc_reserve_map(MpLoc& L, int from_max) {
  MpBuffers& w = L.w;
  if (from_max <= L.from_cap) return hipSuccess;
  loc_free_map(w);
  L.from_cap = 0;
  // a quarter more than asked, in steps of 4096 points: later calls seldom reallocate
  const size_t want = ((size_t)from_max + from_max / 4 + 4095) / 4096 * 4096;
  const int cap = (int)std::min<size_t>(want, (size_t)1 << 28);  // (a FromMap never exceeds map_capacity <= 2^28)
  DevAlloc A;
  const int P = L.cap_n;
  w.map_cap = cap;
  w.tmax = next_pow2(cap) > (1 << 20) ? (1 << 20) : next_pow2(cap);
  if (w.tmax < 64) w.tmax = 64;
  const size_t Pm = (size_t)P * cap;
  A(&w.from, Pm * sizeof(float4));
  A(&w.hC_pts, Pm * sizeof(float4));
  A(&w.hS_pts, Pm * sizeof(float4));
  A(&w.hC_start, (size_t)P * (w.tmax + 1) * sizeof(int));
  A(&w.hS_start, (size_t)P * (w.tmax + 1) * sizeof(int));
  A(&w.hC_rec, (size_t)P * w.tmax * sizeof(uint32_t));
  A(&w.hS_rec, (size_t)P * w.tmax * sizeof(uint32_t));
  A(&w.h_fill, (size_t)2 * P * w.tmax * sizeof(int));
  if (A.err != hipSuccess) {
    loc_free_map(w);
    return A.err;
  }
  L.from_cap = cap;
  return hipSuccess;
}

hipError_t mp_localize_prepare(MpLoc& L, const MpBuffers& s, const MpInput& in, int n, hipStream_t st, Prof* prof,
                               const LocRows* rows) {
  MpBuffers& w = L.w;
  w.P = n;
  hipError_t e = hipMemcpyAsync(L.cand, L.cand_h(), (size_t)n * 12 * sizeof(float), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return e;
  if (rows) {  // (n = its listed lanes x rows->k)
    e = hipMemcpyAsync(L.plan, L.plan_h(), (size_t)(n / rows->k) * sizeof(LaneLocPlan), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return e;
    if (prof) prof->mark("lanes_localize_h2d");
    hipLaunchKernelGGL(k_mp_loc_prepare_rows, dim3(n), dim3(kMpThreads), 0, st, w, loc_store(s), L.cand, L.head, *rows);
    if (prof) prof->mark("k_mp_loc_prepare_rows");
  } else {
    hipLaunchKernelGGL(k_mp_loc_prepare<false>, dim3(n), dim3(kMpThreads), 0, st, w, in, loc_store(s), L.cand, L.head);
    if (prof) prof->mark("k_mp_loc_prepare");
  }
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(L.head_h(), L.head, (size_t)(2 * n + 1) * sizeof(int), hipMemcpyDeviceToHost, st);
}

hipError_t mp_localize_solve(MpLoc& L, const MpBuffers& s, const MpInput& in, int n, int from_max, int cloud_max,
                             int stack_max, hipStream_t st, Prof* prof, const LocRows* rows) {
  MpBuffers& w = L.w;
  w.P = n;
  auto mark = [&](const char* name) { if (prof) prof->mark(name); };
  if (rows) {
    hipLaunchKernelGGL(k_mp_loc_stack_rows, dim3(16, n), dim3(256), 0, st, w, *rows);
    mark("k_mp_loc_stack_rows");
  } else {
    hipLaunchKernelGGL(k_mp_stack, dim3(16, n), dim3(256), 0, st, w, in);
    mark("k_mp_stack");
  }
  mp_stack_vg(w, n, st, stack_max);
  mark("vg_stack");
  const bool map_empty = from_max == 0;  // no candidate can run the L-M (:706): nothing to gather or hash
  if (!map_empty) {
    // about 2048 workgroups over all the candidates, each looping over its candidate's 1024-point tiles
    const int tiles = (from_max + 1023) / 1024;
    const int gx = std::max(1, std::min(tiles, (2048 + n - 1) / n));
    hipLaunchKernelGGL(k_mp_loc_gather, dim3(gx, n), dim3(256), 0, st, w, loc_store(s));
    mark("k_mp_loc_gather");
    // a cloud beyond k_hash_build's 8192 LDS counters is a long global-atomic counting sort in its one
    // workgroup: the grid per cloud instead (1024 candidates of 8.7 k + 25 k points: 9.2 -> 3.9 ms, 64:
    // 0.47 -> 0.29; clouds inside the LDS counters are slower that way: 0.10 -> 0.68 ms at 1024)
    mp_hash_from(w, n, st, /*spread=*/cloud_max > 8192);
    mark("k_hash_build_map");
  }
  // (never the persistent one-instance L-M: it spin-waits between its workgroups)
  mp_lm_loop(w, n, st, prof, map_empty, /*persist=*/false);
  hipLaunchKernelGGL(k_mp_loc_result, dim3((n + 255) / 256), dim3(256), 0, st, w, L.res);
  mark("k_mp_loc_result");
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = w.take_error();
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(L.res_h(), L.res, (size_t)n * kLocResWords * sizeof(int), hipMemcpyDeviceToHost, st);
}

// ---------------------------------------------------------------- shared lanes
hipError_t mp_alloc_shared(MpBuffers& b, int P, int R, int cap_pts, int from_cap, int max_iter) {
  DevAlloc A;
  b.P = P;
  b.capC = kLessSharpPerRing * R;
  b.capS = cap_pts;
  b.cap_stack = b.capC + b.capS;
  b.map_cap = from_cap;
  b.max_iter = max_iter;
  b.tmax = next_pow2(from_cap) > (1 << 20) ? (1 << 20) : next_pow2(from_cap);
  if (b.tmax < 64) b.tmax = 64;
  b.pool_cur = 0;
  const size_t Pm = (size_t)P * from_cap, Ps = (size_t)P * b.cap_stack;
  // the per-lane part of mp_loc_reserve ...
  A(&b.state, (size_t)P * kMpStateFloats * sizeof(float));
  A(&b.istate, (size_t)P * kMpStateInts * sizeof(int));
  A(&b.valid, (size_t)P * kMaxValid * sizeof(int));
  A(&b.vpre, (size_t)P * (kMaxValid + 1) * 2 * sizeof(int));
  A(&b.nfrom, (size_t)P * 2 * sizeof(int));
  A(&b.hC_T, (size_t)P * sizeof(int));
  A(&b.hS_T, (size_t)P * sizeof(int));
  A(&b.stack2, Ps * sizeof(float4));
  A(&b.stack, Ps * sizeof(float4));
  A(&b.sseg_b, (size_t)P * 2 * sizeof(int));
  A(&b.sseg_e, (size_t)P * 2 * sizeof(int));
  A(&b.sseg_cnt, (size_t)P * 2 * sizeof(int));
  A(&b.sseg_leaf, (size_t)P * 2 * sizeof(float));
  if (A.err == hipSuccess) A.err = vg_scratch_alloc(b.vg, Ps, (size_t)P * 2, 2 * P, Ps);
  A(&b.q_ok, Ps * sizeof(int8_t));
  A(&b.q_cf, Ps * sizeof(float4));
  A(&b.q_nn, Ps * 2 * sizeof(int4));
  A(&b.q_fit, Ps * 4 * sizeof(float4));
  A(&b.part, (size_t)P * std::max(kMpSmallGrid, kMpFitGridMax) * 28 * sizeof(double));
  A(&b.rot, (size_t)P * 6 * sizeof(double));
  A(&b.done, (size_t)P * sizeof(int));
  A(&b.ls_epoch, sizeof(unsigned long long));  // (k_mp_lm_begin advances it for one instance)
  // ... of mp_loc_reserve_map ...
  A(&b.from, Pm * sizeof(float4));
  A(&b.hC_pts, Pm * sizeof(float4));
  A(&b.hS_pts, Pm * sizeof(float4));
  A(&b.hC_start, (size_t)P * (b.tmax + 1) * sizeof(int));
  A(&b.hS_start, (size_t)P * (b.tmax + 1) * sizeof(int));
  A(&b.hC_rec, (size_t)P * b.tmax * sizeof(uint32_t));
  A(&b.hS_rec, (size_t)P * b.tmax * sizeof(uint32_t));
  A(&b.h_fill, (size_t)2 * P * b.tmax * sizeof(int));
  // ... and the registered clouds
  A(&b.reg, (size_t)P * b.capS * sizeof(float4));
  A(&b.nreg, (size_t)P * sizeof(int));
  if (A.err == hipSuccess) A.err = hipMemset(b.state, 0, (size_t)P * kMpStateFloats * sizeof(float));
  if (A.err == hipSuccess) A.err = hipMemset(b.istate, 0, (size_t)P * kMpStateInts * sizeof(int));
  if (A.err == hipSuccess) A.err = hipMemset(b.done, 0, (size_t)P * sizeof(int));
  if (A.err == hipSuccess) A.err = hipMemset(b.ls_epoch, 0, sizeof(unsigned long long));
  if (A.err == hipSuccess) A.err = hipDeviceSynchronize();
  if (A.err != hipSuccess) mp_free(b);
  return A.err;
}

void mp_lanes_shared_frame(MpBuffers& w, MpBuffers& s, const MpInput& in, int* res, hipStream_t st, Prof* prof) {
  const int P = w.P;
  auto mark = [&](const char* name) { if (prof) prof->mark(name); };
  mp_wait_update(s, st);  // (the store's last update, when the streaming path deferred it)
  const LocStore store = loc_store(s);
  hipLaunchKernelGGL(k_mp_loc_prepare<true>, dim3(P), dim3(kMpThreads), 0, st, w, in, store, (const float*)nullptr,
                     (int*)nullptr);
  mark("k_mp_loc_prepare");
  hipLaunchKernelGGL(k_mp_stack, dim3(16, P), dim3(256), 0, st, w, in);
  mark("k_mp_stack");
  mp_stack_vg(w, P, st, /*stack_max=*/-1);
  mark("vg_stack");
  // mp_localize_solve's grid with the capacity in the place of the largest FromMap: a workgroup
  // whose first tile lies beyond its lane's FromMap returns at once
  const int tiles = (w.map_cap + 1023) / 1024;
  const int gx = std::max(1, std::min(tiles, (2048 + P - 1) / P));
  hipLaunchKernelGGL(k_mp_loc_gather, dim3(gx, P), dim3(256), 0, st, w, store);
  mark("k_mp_loc_gather");
  mp_hash_from(w, P, st, /*spread=*/w.map_cap > 8192);
  mark("k_hash_build_map");
  mp_lm_loop(w, P, st, prof, /*map_empty=*/false, /*persist=*/false);
  hipLaunchKernelGGL(k_mp_register, dim3(kMpRegWg, P), dim3(256), 0, st, w, in);
  mark("k_mp_register");
  hipLaunchKernelGGL(k_mp_loc_result, dim3((P + 255) / 256), dim3(256), 0, st, w, res);
  mark("k_mp_loc_result");
  w.note(hipGetLastError());
}

// ---------------------------------------------------------------- shared lanes: commit (loam_lanes_map_commit)
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

// A batch problem ends at cur's solved pose: no call returns its map or its registered clouds, so
// the batch frames build neither the registered clouds nor the map with cur inserted.
namespace {
// the corner / surf clouds of the odometry's Last[buf] (the batch frames read no full cloud)
MpInput batch_input(const OdBuffers& od, int buf) {
  MpInput in;
  in.corner = od.lastC + (size_t)buf * od.P * od.capC;
  in.surf = od.lastS + (size_t)buf * od.P * od.capS;
  in.full = nullptr;
  in.corner_stride = od.capC; in.surf_stride = od.capS; in.full_stride = 0;
  in.ncorner = od.nlast + buf * 2; in.nsurf = od.nlast + buf * 2 + 1; in.nfull = nullptr;
  in.ncorner_stride = 2 * kOdBufs; in.nsurf_stride = 2 * kOdBufs; in.nfull_stride = 0;
  return in;
}
}  // namespace

// frame 1 of the batch problem: reset, then prev (the seed's Last[buf]) into the empty store at
// the zero pose.  Reads only what the odometry seeding wrote, so it may run beside od_solve.
// The store is empty by construction: no FromMap gather or hash build, no L-M launches
// (k_mp_lm_begin / k_mp_lm_end still set the state frame 2 reads and zero the cascade's counters),
// then the map update, which leaves prev's map in pool 1 for frame 2.
void mp_batch_frame1(MpBuffers& b, const OdBuffers& od, int buf, hipStream_t st, Prof* prof, const SideStream* side) {
  // (only pool 0's slot table, which this frame reads, must be empty: k_mp_compact_table writes
  // every entry of pool 1's)
  b.note(mp_reset(b, st, /*both_tables=*/false));
  if (prof) prof->mark("mp_reset");
  MpInput in = batch_input(od, buf);
  in.pose = nullptr; in.pose_stride = 0;
  mp_front(b, in, st, prof, -1, side, /*from_map=*/false);
  mp_lm_loop(b, b.P, st, prof, /*map_empty=*/true, /*persist=*/true);
  mp_update(b, st, prof);
}

// frame 2: cur (TransformToEnd's Last[buf]) with the odometry transformSum, up to its solved pose
// (k_mp_lm_end); the store stays prev's map (pool 1) until the next step's reset
void mp_batch_frame2(MpBuffers& b, const OdBuffers& od, int buf, hipStream_t st, Prof* prof, const SideStream* side) {
  MpInput in = batch_input(od, buf);
  in.pose = od.state + kOdSum; in.pose_stride = kOdStateFloats;
  mp_front(b, in, st, prof, -1, side, /*from_map=*/true);
  mp_lm_loop(b, b.P, st, prof, false, /*persist=*/true);
  if (prof) prof->mark("k_mp_lm_end");  // (no later mark of the step would take it)
}

// per-instance mapping L-M iteration counts of the last frame (loam_batch_iterations)
hipError_t mp_batch_iters(MpBuffers& b, hipStream_t st, int32_t* iters) {
  std::vector<int> si((size_t)b.P * kMpStateInts);
  hipError_t he = hipStreamSynchronize(st);
  if (he == hipSuccess) he = hipMemcpy(si.data(), b.istate, si.size() * sizeof(int), hipMemcpyDeviceToHost);
  if (he == hipSuccess)
    for (int p = 0; p < b.P; ++p) iters[p] = si[(size_t)p * kMpStateInts + kMiIters];
  return he;
}

int mp_batch_download(MpBuffers& b, hipStream_t st, loam_pose6* aft, loam_stats* stats, std::string& err) {
  std::vector<float> sf((size_t)b.P * kMpStateFloats);
  std::vector<int> si((size_t)b.P * kMpStateInts);
  hipError_t he = hipStreamSynchronize(st);
  if (he == hipSuccess) he = b.take_error();
  if (he == hipSuccess) he = hipMemcpy(sf.data(), b.state, sf.size() * sizeof(float), hipMemcpyDeviceToHost);
  if (he == hipSuccess) he = hipMemcpy(si.data(), b.istate, si.size() * sizeof(int), hipMemcpyDeviceToHost);
  if (he != hipSuccess) {
    err = std::string("mapping: ") + hipGetErrorString(he);
    return LOAM_E_HIP;
  }
  for (int p = 0; p < b.P; ++p) {
    const int* q = &si[(size_t)p * kMpStateInts];
    if (q[kMiErr]) {
      err = "mapping capacity exceeded (map store / stack)";
      return LOAM_E_CAPACITY;
    }
    if (aft) std::memcpy(&aft[p], &sf[(size_t)p * kMpStateFloats + kMpAft], sizeof(loam_pose6));
    if (stats) {
      stats->mp_iters += q[kMiIters];
      stats->mp_rows_sum += (uint64_t)q[kMiRows];
      stats->mp_stack += (uint64_t)(q[kMiStackC] + q[kMiStackS]);
      stats->mp_stack_iters += (uint64_t)q[kMiIters] * (q[kMiStackC] + q[kMiStackS]);
      stats->mp_fits += (uint64_t)q[kMiFits];
      stats->mp_map_points += (uint64_t)(q[kMiFromC] + q[kMiFromS]);
      stats->mp_map_valid_points += (uint64_t)q[kMiValidPts];
      stats->mp_degenerate_steps += (uint64_t)q[kMiDegSteps];
      stats->mp_grid_shifts += (uint64_t)q[kMiShifts];
      stats->mp_nn_candidates += (uint64_t)(uint32_t)q[kMiNnCand];
      stats->mp_nn_cells += (uint64_t)(uint32_t)q[kMiNnCells];
    }
  }
  return LOAM_OK;
}

// ---------------------------------------------------------------- the 5-NN search's diagnostic hook
namespace {
struct DevNn5 {
  MpNnCtx c;           // the map as the corner cloud (fromC, hcs / hcr / hcp, TC), nfc = its size
  const float4* qs;    // [nq] queries
  const int* seeds;    // [nq][5] or nullptr
  const int* distinct; // [nq] or nullptr
  int nq;
  int4* flat;          // [nq][3]: (i0..i3), (i4, d0, d1, d2), (d3, d4, -, -)
  int4* plain;
  int* flags;          // [nq], zeroed
};
LOAM_D void dev_nn5_store(int4* out, int q, const Top5& t) {
  out[3 * q + 0] = make_int4(t.i(0), t.i(1), t.i(2), t.i(3));
  out[3 * q + 1] = make_int4(t.i(4), __float_as_int(t.d(0)), __float_as_int(t.d(1)), __float_as_int(t.d(2)));
  out[3 * q + 2] = make_int4(__float_as_int(t.d(3)), __float_as_int(t.d(4)), 0, 0);
}
// the query's start as an L-M iteration makes it: the stored previous 5-NN and their distinct flag
LOAM_D void dev_nn5_seed(const DevNn5& d, int q, float4 sel, Top5& t, int& work) {
  const bool first = d.seeds == nullptr;
  int4 n0 = make_int4(0, 0, 0, 0), n1 = n0;
  if (!first) {
    const int* s = d.seeds + 5 * q;
    n0 = make_int4(s[0], s[1], s[2], s[3]);
    n1 = make_int4(s[4], 0, d.distinct ? d.distinct[q] : 1, 0);
  }
  mp_nn_seed_from(d.c, q, true, first, n0, n1, sel, t, work);
}
// k_mp_nnfit's form: a lane per query, one-wave workgroups, the lists in the workgroup's LDS array
__global__ __launch_bounds__(kMpFitThreads) void k_dev_nn5_batch(DevNn5 d) {
  constexpr int NT = kMpFitThreads;
  __shared__ uint32_t lds[kNnListCap * NT];
  const int tid = threadIdx.x, q = blockIdx.x * NT + tid;
  if (q >= d.nq) return;
  const float4 sel = d.qs[q];
  int work = 0, diag = 0;
  Top5 t;
  dev_nn5_seed(d, q, sel, t, work);
  knn5_flat<NT, 1, kNnListCap>(d.c.hcs, d.c.hcr, d.c.hcp, d.c.TC, sel, t, lds + tid, work, 0, &diag);
  dev_nn5_store(d.flat, q, t);
  if (diag) atomicOr(&d.flags[q], diag);
  dev_nn5_seed(d, q, sel, t, work);
  knn5(d.c.hcs, d.c.hcp, d.c.TC, sel, t, work);
  dev_nn5_store(d.plain, q, t);
}
// k_mp_lm_small's form (mp_nn_query): kMpNnLanes lanes per query, their lists merged
__global__ __launch_bounds__(kMpQueryThreads) void k_dev_nn5_stream(DevNn5 d) {
  constexpr int L = kMpNnLanes, QPB = kMpQueryThreads / L;
  __shared__ uint32_t lists[27 * kMpQueryThreads];
  const int tid = threadIdx.x, sub = tid % L;
  // (whole lane groups: a group's lanes exchange their lists, so none may leave early)
  for (int q = blockIdx.x * QPB + tid / L; q < d.nq; q += gridDim.x * QPB) {
    const float4 sel = d.qs[q];
    int work = 0, diag = 0;
    Top5 t;
    dev_nn5_seed(d, q, sel, t, work);
    knn5_flat<kMpQueryThreads, L>(d.c.hcs, d.c.hcr, d.c.hcp, d.c.TC, sel, t, lists + tid, work, sub, &diag);
    if constexpr (L > 1) knn5_merge<L>(t);
    if (diag) atomicOr(&d.flags[q], diag);
    if (sub == 0) {
      dev_nn5_store(d.flat, q, t);
      dev_nn5_seed(d, q, sel, t, work);
      knn5(d.c.hcs, d.c.hcp, d.c.TC, sel, t, work);
      dev_nn5_store(d.plain, q, t);
    }
  }
}
}  // namespace

}  // namespace loam

struct loam_dev_nn5 {
  int device = 0;
  hipStream_t st = nullptr;
  float4 *map = nullptr, *hpts = nullptr, *hpts2 = nullptr, *qs = nullptr;
  int *start = nullptr, *start2 = nullptr, *fill = nullptr, *fill2 = nullptr, *count = nullptr, *tsize = nullptr;
  uint32_t *rec = nullptr, *rec2 = nullptr;
  int *seeds = nullptr, *distinct = nullptr, *flags = nullptr;
  int4 *flat = nullptr, *plain = nullptr;
};

namespace {
void dev_nn5_free(loam_dev_nn5* h) {
  void* ptrs[] = {h->map, h->hpts, h->hpts2, h->qs, h->start, h->start2, h->fill, h->fill2, h->count, h->tsize,
                  h->rec, h->rec2, h->seeds, h->distinct, h->flags, h->flat, h->plain};
  for (void* q : ptrs)
    if (q) (void)hipFree(q);
  if (h->st) (void)hipStreamDestroy(h->st);
  delete h;
}
}  // namespace

extern "C" int loam_dev_nn5_create(int device, loam_dev_nn5** out) {
  if (!out) return LOAM_E_INVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return LOAM_E_HIP;  // (no CPU path, as loam_create)
  if (device < 0 || device >= ndev) return LOAM_E_INVAL;
  if (hipSetDevice(device) != hipSuccess) return LOAM_E_HIP;
  loam_dev_nn5* h = new loam_dev_nn5();
  h->device = device;
  const size_t M = LOAM_DEV_NN5_MAX_MAP, Q = LOAM_DEV_NN5_MAX_QUERIES;
  loam::DevAlloc A;
  A(&h->map, M * sizeof(float4));
  A(&h->hpts, M * sizeof(float4));
  A(&h->hpts2, M * sizeof(float4));
  A(&h->qs, Q * sizeof(float4));
  A(&h->start, (M + 1) * sizeof(int));
  A(&h->start2, (M + 1) * sizeof(int));
  A(&h->fill, M * sizeof(int));
  A(&h->fill2, M * sizeof(int));
  A(&h->count, 2 * sizeof(int));
  A(&h->tsize, 2 * sizeof(int));
  A(&h->rec, M * sizeof(uint32_t));
  A(&h->rec2, M * sizeof(uint32_t));
  A(&h->seeds, Q * 5 * sizeof(int));
  A(&h->distinct, Q * sizeof(int));
  A(&h->flags, Q * sizeof(int));
  A(&h->flat, Q * 3 * sizeof(int4));
  A(&h->plain, Q * 3 * sizeof(int4));
  hipError_t e = A.err;
  if (e == hipSuccess) e = hipStreamCreate(&h->st);
  if (e != hipSuccess) {
    dev_nn5_free(h);
    return e == hipErrorOutOfMemory ? LOAM_E_NOMEM : LOAM_E_HIP;
  }
  *out = h;
  return LOAM_OK;
}

extern "C" int loam_dev_nn5_run(loam_dev_nn5* h, const loam_dev_nn5_job* job, int32_t* flat_idx, uint32_t* flat_dist,
                                int32_t* plain_idx, uint32_t* plain_dist, int32_t* flags, int32_t* counts) {
  using namespace loam;
  if (!h || !job || !flat_idx || !flat_dist || !plain_idx || !plain_dist || !counts) return LOAM_E_INVAL;
  const int nm = job->n_map, nq = job->n_queries;
  if (!job->map || !job->queries || nm < 1 || nm > LOAM_DEV_NN5_MAX_MAP || nq < 1 || nq > LOAM_DEV_NN5_MAX_QUERIES)
    return LOAM_E_INVAL;
  if (job->form != LOAM_DEV_NN5_BATCH && job->form != LOAM_DEV_NN5_STREAM) return LOAM_E_INVAL;
  if (job->distinct && !job->seeds) return LOAM_E_INVAL;
  if (job->seeds)
    for (int k = 0; k < 5 * nq; ++k)
      if (job->seeds[k] < 0 || job->seeds[k] >= nm) return LOAM_E_INVAL;
  hipStream_t st = h->st;
  auto up = [&](void* d, const void* s, size_t bytes) { return hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, st); };
  const int cnt2[2] = {nm, 0};  // (the hash build takes two clouds: the second one is empty)
  hipError_t e = hipSetDevice(h->device);
  if (e == hipSuccess) e = up(h->map, job->map, (size_t)nm * sizeof(float4));
  if (e == hipSuccess) e = up(h->qs, job->queries, (size_t)nq * sizeof(float4));
  if (e == hipSuccess) e = up(h->count, cnt2, sizeof(cnt2));
  if (e == hipSuccess && job->seeds) e = up(h->seeds, job->seeds, (size_t)nq * 5 * sizeof(int));
  if (e == hipSuccess && job->distinct) e = up(h->distinct, job->distinct, (size_t)nq * sizeof(int));
  if (e == hipSuccess) e = hipMemsetAsync(h->flags, 0, (size_t)nq * sizeof(int), st);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(st);
    return LOAM_E_HIP;
  }
  // the map's index as mp_hash_from builds FromMap's (1 m cells, buckets kept to single cells, packed ranges)
  HashJob hc;
  hc.pts = h->map; hc.pts_stride = LOAM_DEV_NN5_MAX_MAP; hc.pts_off = nullptr; hc.pts_off_stride = 0;
  hc.count = h->count; hc.count_stride_bytes = 2 * sizeof(int);
  hc.start = h->start; hc.fill = h->fill; hc.out = h->hpts; hc.tsize = h->tsize; hc.tmax = LOAM_DEV_NN5_MAX_MAP;
  hc.inv_h = 1.0f;
  hc.shift = 0;
  hc.chunks = nullptr;
  hc.rec = h->rec;
  HashJob hs = hc;
  hs.count = h->count + 1; hs.start = h->start2; hs.fill = h->fill2; hs.out = h->hpts2; hs.tsize = h->tsize + 1;
  hs.rec = h->rec2;
  hash_build_pair(hc, hs, 1, st, false);
  int T = 0;
  e = hipMemcpyAsync(&T, h->tsize, sizeof(int), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return LOAM_E_HIP;
  DevNn5 d;
  d.c = MpNnCtx();
  d.c.hcs = h->start; d.c.hcr = h->rec; d.c.hcp = h->hpts; d.c.TC = T;
  d.c.fromC = h->map; d.c.nfc = nm;
  d.qs = h->qs;
  d.seeds = job->seeds ? h->seeds : nullptr;
  d.distinct = job->distinct ? h->distinct : nullptr;
  d.nq = nq;
  d.flat = h->flat; d.plain = h->plain; d.flags = h->flags;
  if (job->form == LOAM_DEV_NN5_BATCH) {
    hipLaunchKernelGGL(k_dev_nn5_batch, dim3((nq + kMpFitThreads - 1) / kMpFitThreads), dim3(kMpFitThreads), 0, st, d);
  } else {
    constexpr int QPB = kMpQueryThreads / kMpNnLanes;
    hipLaunchKernelGGL(k_dev_nn5_stream, dim3((nq + QPB - 1) / QPB), dim3(kMpQueryThreads), 0, st, d);
  }
  e = hipGetLastError();
  std::vector<int4> of((size_t)nq * 3), op((size_t)nq * 3);
  std::vector<int> fl((size_t)nq);
  if (e == hipSuccess) e = hipMemcpyAsync(of.data(), h->flat, of.size() * sizeof(int4), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(op.data(), h->plain, op.size() * sizeof(int4), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(fl.data(), h->flags, fl.size() * sizeof(int), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return LOAM_E_HIP;
  auto unpack = [&](const std::vector<int4>& v, int32_t* idx, uint32_t* dist) {
    for (int q = 0; q < nq; ++q) {
      const int4 a = v[3 * q], b = v[3 * q + 1], c = v[3 * q + 2];
      const int i5[5] = {a.x, a.y, a.z, a.w, b.x}, d5[5] = {b.y, b.z, b.w, c.x, c.y};
      for (int k = 0; k < 5; ++k) {
        idx[5 * q + k] = i5[k];
        dist[5 * q + k] = (uint32_t)d5[k];
      }
    }
  };
  unpack(of, flat_idx, flat_dist);
  unpack(op, plain_idx, plain_dist);
  counts[0] = counts[1] = 0;
  for (int q = 0; q < nq; ++q) {
    if (flags) flags[q] = fl[q];
    if (fl[q] & LOAM_DEV_NN5_OVERFLOW) ++counts[0];
    if (fl[q] & LOAM_DEV_NN5_PLAIN) ++counts[1];
  }
  return LOAM_OK;
}

extern "C" int loam_dev_nn5_destroy(loam_dev_nn5* h) {
  if (!h) return LOAM_E_INVAL;
  (void)hipSetDevice(h->device);
  if (h->st) (void)hipStreamSynchronize(h->st);
  dev_nn5_free(h);
  return LOAM_OK;
}

#ifdef LOAM_PHASES
// the phase sums of the last-workgroup kernel of this file (PhaseAcc, dev_common.hpp); diagnostic
// build only (tools/phase_stream.py)
extern "C" int loam_debug_phases_mp(unsigned long long* out) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(loam::g_ph_mp), sizeof(PhaseAcc)) == hipSuccess ? 0 : -1;
}
#endif
