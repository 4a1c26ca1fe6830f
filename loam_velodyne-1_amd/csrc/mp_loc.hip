// Localization on gfx950: candidate poses (loam_map_localize, loam_lanes_localize) or the shared
// lanes as the instances of a working set against a streaming store that is only read (mp.hpp).
// The stacks' VoxelGrid, the hash builds and the L-M are the core's (mp.hip).
//  k_mp_loc_prepare / k_mp_loc_gather / k_mp_loc_result   prepare without recentring, FromMap per
//                  candidate from the shared pool, the result blocks
//  k_mp_loc_prepare_rows / k_mp_loc_stack_rows   loam_lanes_localize: every candidate's sweep and
//                  odometry pose read in place from a listed lane (a row -> lane plan)
#include <algorithm>

#include "mp_dev.hpp"

namespace loam {
namespace {

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

// ---------------------------------------------------------------- localization: host side
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
  // the sweep's two clouds, once for every candidate
  A(&w.inC, (size_t)w.capC * sizeof(float4));
  A(&w.inS, (size_t)w.capS * sizeof(float4));
  A(&w.in_n, 3 * sizeof(int));
  A(&w.in_pose, 6 * sizeof(float));
  // (the VoxelGrid scratch: two stack segments per candidate)
  mp_alloc_solve(A, w, Pc, (size_t)Pc * w.cap_stack, (size_t)Pc * 2);
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
  mp_alloc_from(A, w, L.cap_n, cap);
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

namespace {
// The middle of a localization frame for the w.P instances of w, behind their prepare kernel: the
// stacks (rows: read in place from the listed lanes), their VoxelGrid, the FromMap gather, the hash
// builds, the L-M.  from_max: the largest FromMap of an instance, or the capacity where the host reads
// no count (a workgroup beyond its instance's FromMap returns at once); cloud_max: likewise its largest part
void loc_solve(MpBuffers& w, const LocStore& store, const MpInput& in, const LocRows* rows, int from_max,
               int cloud_max, int stack_max, hipStream_t st, Prof* prof) {
  const int n = w.P;
  auto mark = [&](const char* name) { if (prof) prof->mark(name); };
  if (rows) {
    hipLaunchKernelGGL(k_mp_loc_stack_rows, dim3(16, n), dim3(256), 0, st, w, *rows);
    mark("k_mp_loc_stack_rows");
  } else {
    mp_launch_stack(w, in, st);
    mark("k_mp_stack");
  }
  mp_stack_vg(w, n, st, stack_max);
  mark("vg_stack");
  const bool map_empty = from_max == 0;  // no candidate can run the L-M (:706): nothing to gather or hash
  if (!map_empty) {
    // about 2048 workgroups over all the candidates, each looping over its candidate's 1024-point tiles
    const int tiles = (from_max + 1023) / 1024;
    const int gx = std::max(1, std::min(tiles, (2048 + n - 1) / n));
    hipLaunchKernelGGL(k_mp_loc_gather, dim3(gx, n), dim3(256), 0, st, w, store);
    mark("k_mp_loc_gather");
    // a cloud beyond k_hash_build's 8192 LDS counters is a long global-atomic counting sort in its one
    // workgroup: the grid per cloud instead (1024 candidates of 8.7 k + 25 k points: 9.2 -> 3.9 ms, 64:
    // 0.47 -> 0.29; clouds inside the LDS counters are slower that way: 0.10 -> 0.68 ms at 1024)
    mp_hash_from(w, n, st, /*spread=*/cloud_max > 8192);
    mark("k_hash_build_map");
  }
  // (never the persistent one-instance L-M: it spin-waits between its workgroups)
  mp_lm_loop(w, n, st, prof, map_empty, /*persist=*/false);
}
}  // namespace

hipError_t mp_localize_solve(MpLoc& L, const MpBuffers& s, const MpInput& in, int n, int from_max, int cloud_max,
                             int stack_max, hipStream_t st, Prof* prof, const LocRows* rows) {
  MpBuffers& w = L.w;
  w.P = n;
  loc_solve(w, loc_store(s), in, rows, from_max, cloud_max, stack_max, st, prof);
  hipLaunchKernelGGL(k_mp_loc_result, dim3((n + 255) / 256), dim3(256), 0, st, w, L.res);
  if (prof) prof->mark("k_mp_loc_result");
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
  b.max_iter = max_iter;
  b.pool_cur = 0;
  // the two groups of the localization's working set and the registered clouds
  mp_alloc_solve(A, b, P, (size_t)P * b.cap_stack, (size_t)P * 2);
  mp_alloc_from(A, b, P, from_cap);
  A(&b.reg, (size_t)P * b.capS * sizeof(float4));
  A(&b.nreg, (size_t)P * sizeof(int));
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
  // (the capacity, >= 1024, in the place of the counts the host does not read; stack_max unknown)
  loc_solve(w, store, in, nullptr, w.map_cap, w.map_cap, /*stack_max=*/-1, st, prof);
  mp_launch_register(w, in, st);
  mark("k_mp_register");
  hipLaunchKernelGGL(k_mp_loc_result, dim3((P + 255) / 256), dim3(256), 0, st, w, res);
  mark("k_mp_loc_result");
  w.note(hipGetLastError());
}

}  // namespace loam
