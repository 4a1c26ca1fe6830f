// Mapping device buffers and entry points (engine-internal).
#ifndef LOAM_MP_HPP
#define LOAM_MP_HPP

#include <hip/hip_runtime.h>

#include <functional>
#include <string>

#include "engine.hpp"
#include "loc_plan.hpp"
#include "xfer.hpp"
#include "od.hpp"
#include "vg.hpp"

namespace loam {

// cube grid of src/laserMapping.cpp:64-70
constexpr int kCubeW = 21, kCubeH = 11, kCubeD = 21, kCubeNum = kCubeW * kCubeH * kCubeD;
constexpr int kMaxValid = 125;
constexpr int kMpFitGridMax = 256;  // k_mp_fit<true> workgroups per instance (partials per instance)
constexpr int kMpSmallGrid = 256;  // workgroups per instance of the small-batch L-M iteration (multiple of 8)

// per-instance float state: Sum | Incre | TobeMapped | Bef | Aft | matP[36] | pointOnYAxis[3]
constexpr int kMpSum = 0, kMpIncre = 6, kMpTobe = 12, kMpBef = 18, kMpAft = 24, kMpMatP = 30, kMpOnY = 66,
              kMpImuRP = 69, kMpStateFloats = 72;  // kMpImuRP: IMU (roll, pitch) for transformUpdate
enum { kMiCenW = 0, kMiCenH, kMiCenD, kMiDegen, kMiNValid, kMiIters, kMiRows, kMiStackC, kMiStackS, kMiFromC,
       kMiFromS, kMiErr, kMiLmRan, kMiValidPts, kMiStop, kMiFits, kMiImu, kMiCubeI, kMiCubeJ, kMiCubeK,
       kMiDegSteps,  // L-M updates of this frame projected by the iteration-0 degeneracy analysis
       kMiShifts,    // cube-grid slab shifts of this frame's recentring (the reference's passes)
       kMiNnCand,    // map points the 5-NN evaluated this frame (seeds included)
       kMiNnCells,   // hash bucket ranges the 5-NN read this frame
       kMiRowsLast,  // rows of the last L-M iteration evaluated (mp_step; the persistent streaming L-M keeps no such count)
       kMiLocOff,    // loam_map_localize: the candidate's centre cube is within 3 of a grid edge (not evaluated)
       kMpStateInts = 28 };
static_assert(kMiLocOff < kMpStateInts, "istate layout");

// one mapping frame's inputs for every instance (device pointers)
struct MpInput {
  const float4 *corner, *surf, *full;
  size_t corner_stride, surf_stride, full_stride;
  const int *ncorner, *nsurf, *nfull;
  int ncorner_stride, nsurf_stride, nfull_stride;
  const float* pose;   // transformSum of the odometry message (nullptr = zero pose)
  int pose_stride;
  // (the batch frames register nothing: their full / nfull are null)
};

struct MpBuffers {
  int P = 0, capC = 0, capS = 0, cap_stack = 0, map_cap = 0, max_iter = 10, tmax = 0;
  int pool_cur = 0;
  float* state = nullptr;     // [P][kMpStateFloats]
  int* istate = nullptr;      // [P][kMpStateInts]
  int* slots = nullptr;       // [2][P][kCubeNum][4] (offC, cntC, offS, cntS) per pool
  float4* pool = nullptr;     // [2][P][map_cap]
  int* valid = nullptr;       // [P][kMaxValid]
  int* vpre = nullptr;        // [P][kMaxValid + 1][2] FromMap prefix (corner, surf)
  // streaming inputs (inC / inS / inF: null in a batch set, mp_alloc)
  float4 *inC = nullptr, *inS = nullptr, *inF = nullptr;
  int* in_n = nullptr;        // [P][3]
  float* in_pose = nullptr;   // [P][6]
  // stacks
  float4* stack2 = nullptr;   // [P][cap_stack] corner at 0, surf at capC
  float4* stack = nullptr;    // [P][cap_stack] voxel-grid output (same layout)
  int* nstack = nullptr;      // [P][2]
  // FromMap + hashes
  float4* from = nullptr;     // [P][map_cap] corner then surf
  int *hC_start = nullptr, *hS_start = nullptr, *h_fill = nullptr, *hC_T = nullptr, *hS_T = nullptr;
  uint32_t *hC_rec = nullptr, *hS_rec = nullptr;  // [P][tmax] packed bucket ranges (HashJob::rec)
  float4 *hC_pts = nullptr, *hS_pts = nullptr;   // [P][map_cap]
  int* nfrom = nullptr;       // [P][2]
  // per-query L-M outputs of the current iteration
  int8_t* q_ok = nullptr;     // [P][cap_stack]
  float4* q_cf = nullptr;     // [P][cap_stack]
  int4* q_nn = nullptr;       // [P][cap_stack][2] this iteration's ordered 5-NN (i0..i3 | i4, d4 bits)
  float4* q_fit = nullptr;    // [P][cap_stack][4] MpFit: the 5-NN a line / plane was fitted to + the fit
                              // (k_mp_nnfit: the last iteration's 5-NN, distinct, fit-valid + the fit)
  // insertion / per-cube downsampling
  int* app_cnt = nullptr;     // [P][kCubeNum][2] appended points per cube
  int* citems = nullptr;      // [P][2 * kCubeNum] non-empty (kind, cube, valid index) of the new store
  int* nitems = nullptr;      // [P]
  int* app_off = nullptr;     // [P][kCubeNum][2]
  float4* app = nullptr;      // [P][cap_stack] stack points grouped by cube (map frame)
  float4* vin = nullptr;      // [P][map_cap] per-valid-cube DS input (old ++ appended)
  float4* vout = nullptr;     // [P][map_cap]
  int *vseg_b = nullptr, *vseg_e = nullptr, *vseg_cnt = nullptr;  // [P][2*kMaxValid]
  float* vseg_leaf = nullptr;
  int *sseg_b = nullptr, *sseg_e = nullptr, *sseg_cnt = nullptr;  // [P][2] stack segments
  float* sseg_leaf = nullptr;
  // the VoxelGrid scratch: sort arrays [max(P map_cap, P cap_stack)], vg_run's segment lists
  // [P][2][kMaxValid], counts [4] (the lengths of its two lists, of vg_lin, of vg_mlist), the stack
  // job's big-segment split (2P parents)
  VgScratch vg;
  int* vg_lin = nullptr;                   // [P][2][kMaxValid] the non-empty cube segments (k_mp_vseg)
  int* vg_mlist = nullptr;                 // [P][2][kMaxValid] cube segments k_vg_merge may take
  int* vseg_nold = nullptr;                // [P][2][kMaxValid] leading points from the cube's last DS
  int* vseg_skip = nullptr;                // [P][2][kMaxValid] 1: k_vg_merge wrote the segment
  float4* reg = nullptr;      // [P][capS] registered full cloud (null in a batch set, as nreg)
  double* part = nullptr;     // [P][kMpSmallGrid][28] k_mp_lm_small's per-workgroup JᵀJ | Jᵀb | rows
  int* done = nullptr;        // [P] its workgroups finished (the last one runs the step)
  // the persistent one-instance L-M (k_mp_lm_stream): per workgroup and iteration parity its partial
  // sums, per workgroup its publication word (epoch << 16 | iteration + 1), the launch epoch
  // (advanced by k_mp_lm_begin)
  double* ls_part = nullptr;              // [2][kMpSmallGrid][28]
  unsigned long long* ls_flag = nullptr;  // [kMpSmallGrid]
  unsigned long long* ls_epoch = nullptr; // [1]
  double* rot = nullptr;      // [P][6] cos / sin of the TobeMapped rotation (rot_store in mp_dev.hpp)
  int* nreg = nullptr;
  // the streaming frame's map update (insertion, per-cube VoxelGrid, compaction) deferred to a side
  // stream (mp_frame's `defer`): upd_done is recorded there; the next frame, the surround cloud
  // and a reset wait for it first (upd_pending)
  hipEvent_t upd_fork = nullptr, upd_done = nullptr;
  bool upd_pending = false;
  Tuning tune;                // host-side launch choices (the frames' stages)
  hipError_t sticky = hipSuccess;  // first failed HIP call of the launch sequences
  void note(hipError_t e) {
    if (sticky == hipSuccess) sticky = e;
  }
  // returns the sticky error and clears it
  hipError_t take_error() {
    const hipError_t e = sticky;
    sticky = hipSuccess;
    return e;
  }
};

inline int mp_batch_map_capacity(int cap) { return 2 * cap; }
// on failure: freed, b empty.  batch: a set of the batch frames, which read their clouds in place and
// register nothing: inC / inS / inF and reg / nreg are not allocated
hipError_t mp_alloc(MpBuffers& b, int P, int R, int cap_pts, int map_cap, int max_iter, bool batch = false);
void mp_free(MpBuffers& b);
// both_tables = false: only pool 0's slot table is cleared (the one the next frame reads; for a
// caller whose next map update rewrites pool 1's whole table before anything reads it)
hipError_t mp_reset(MpBuffers& b, hipStream_t st, bool both_tables = true);
// One whole mapping frame (streaming, lanes): front (prepare, stacks + their VoxelGrid, FromMap
// gather + hashes), the L-M loop, the map update, the registration of the full cloud.
// before_register: called once every kernel before k_mp_register is enqueued (the streaming path
// stages the full cloud there); stack_max: the largest stack segment (corner or surf input count)
// when the host knows it, else -1
// defer: a second stream for the map update (streaming frames): the update runs there after the
// L-M, beside the registration and the caller's downloads; the frame's pose and registered cloud do
// not wait for it (b.upd_pending until the next frame's first kernel has waited for it)
void mp_frame(MpBuffers& b, const MpInput& in, hipStream_t st, Prof* prof = nullptr,
              const std::function<void()>& before_register = nullptr, int stack_max = -1,
              hipStream_t defer = nullptr);
// the batch frames' side stream: an idle second stream and a fork / join event pair for the stack
// VoxelGrid beside the FromMap gather + hash builds (st = nullptr: no branch)
struct SideStream {
  hipStream_t st = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  hipEvent_t inputs_read = nullptr;  // optional: recorded once the frame has read its input clouds
};
// the pending deferred map update (if any) before later work on st
void mp_wait_update(MpBuffers& b, hipStream_t st);
// imu_rp: the IMU (roll, pitch) transformUpdate blends in (nullptr = no IMU); *updated = whether
// transformUpdate ran (the caller then commits its IMU queue pointer)
int mp_stream_frame(MpBuffers& b, hipStream_t st, const loam_pose6& odom_sum, const loam_cloud_out& corner,
                    const loam_cloud_out& surf, const loam_cloud_out& full, loam_pose6* aft, loam_pose6* bef,
                    loam_cloud_out* registered, loam_stats* stats, std::string& err, Staging& pin, const StreamIo& io,
                    const float* imu_rp = nullptr, bool* updated = nullptr, hipStream_t st2 = nullptr,
                    hipEvent_t ev2 = nullptr, hipStream_t defer = nullptr);
// the same frame on clouds already on the device (src: pointers + device counts, n3: host counts)
int mp_stream_frame_dev(MpBuffers& b, hipStream_t st, const loam_pose6& odom_sum, const MpInput& src, const int* n3,
                        loam_pose6* aft, loam_pose6* bef, loam_cloud_out* registered, loam_stats* stats,
                        std::string& err, Staging& pin, const StreamIo& io, const float* imu_rp = nullptr,
                        bool* updated = nullptr, hipStream_t defer = nullptr);
// /laser_cloud_surround of the last streaming frame (instance 0): its 5x5x5 cube neighbourhood
// concatenated and VoxelGrid 0.2 (src/laserMapping.cpp:1038-1058)
int mp_stream_surround(MpBuffers& b, hipStream_t st, loam_cloud_out* out, std::string& err);
// The batch problem's two frames.  It ends at cur's solved pose: frame 1 (reset, prev into the empty
// store: front without FromMap, no L-M launches, the map update) and frame 2 (cur: front and L-M
// loop, nothing after k_mp_lm_end).  Neither registers a cloud, and the map with cur inserted is
// not built: no batch call returns them.
// buf: the odometry's Last buffer the frame reads (frame 1: the seed's, frame 2: TransformToEnd's)
// side: frame 1 uses only its inputs_read event (it runs on st alone)
void mp_batch_frame1(MpBuffers& b, const OdBuffers& od, int buf, hipStream_t st, Prof* prof = nullptr,
                     const SideStream* side = nullptr);
void mp_batch_frame2(MpBuffers& b, const OdBuffers& od, int buf, hipStream_t st, Prof* prof = nullptr,
                     const SideStream* side = nullptr);
int mp_batch_download(MpBuffers& b, hipStream_t st, loam_pose6* aft, loam_stats* stats, std::string& err);
hipError_t mp_batch_iters(MpBuffers& b, hipStream_t st, int32_t* iters);

// ---- map export / import of a streaming store (loam_map_export / loam_map_import: instance 0;
// loam_lanes_map_export: the export of instance `inst` of the lanes' store) ----
// Canonical order: key = kind * kCubeNum + cube (kind 0 corner, 1 surf), ascending; inside a key
// the store's own point order.  The small tables both calls need live in one device block (`tab`,
// ints) with a pinned host copy of its head; the point scratch is the store's own idle buffers
// (vin, the VoxelGrid sort arrays vg.keys .. vg.vals_alt, app_cnt: all rewritten by a frame before it reads them).
constexpr int kMapKeys = 2 * kCubeNum;
constexpr int kMapTabOff = 0;                     // [kMapKeys + 1] canonical offsets (export)
constexpr int kMapTabInfo = kMapKeys + 2;         // centre[3], istate error, aft[6], bef[6] (export)
constexpr int kMapTabAcc = kMapTabInfo + 16;      // kept points so far, dropped corner / surf (import)
constexpr int kMapTabHead = kMapTabAcc + 8;       // ints of the head (what the host reads)
constexpr int kMapTabSrc = kMapTabHead;           // [kMapKeys] pool offset of every key (export)
constexpr int kMapChunkPts = 1 << 21;             // points of one import chunk at most
constexpr int kMapBinTile = 1024;                 // points per workgroup of the chunk kernels
constexpr int kMapChunkTiles = kMapChunkPts / kMapBinTile;
constexpr int kMapTabTile = kMapTabSrc + kMapKeys + 2;  // [kMapChunkTiles] a chunk's kept points per tile, scanned in place
constexpr int kMapTabSlots = kMapTabTile + kMapChunkTiles;  // [kCubeNum][4] the sorted points' slot table (lanes import)
constexpr int kMapTabInts = kMapTabSlots + 4 * kCubeNum;
static_assert(kMapTabHead % 4 == 0 && kMapTabTile % 4 == 0 && kMapTabSlots % 4 == 0, "table regions");
struct MapIo {
  int* tab = nullptr;    // device [kMapTabInts]
  int* tab_h = nullptr;  // pinned [kMapTabHead]
};
hipError_t mp_map_ensure(MapIo& io);  // allocated by the first call
void mp_map_free(MapIo& io);
// export: the canonical offsets, the centre and the poses into io.tab (k_mp_map_table), copied to
// io.tab_h; the caller synchronises st before reading it
hipError_t mp_map_table(MpBuffers& b, MapIo& io, hipStream_t st, Prof* prof, int inst = 0);
// export: the store's points in canonical order into the instance's part of vin,
// b.vin[inst * map_cap ..) (k_mp_map_pack); total = tab_h[kMapKeys]
hipError_t mp_map_pack(MpBuffers& b, MapIo& io, int total, hipStream_t st, Prof* prof, int inst = 0);
// import: zeroes the accumulators and the per-key counts
hipError_t mp_map_bin_begin(MpBuffers& b, MapIo& io, hipStream_t st);
// import: n <= kMapChunkPts points of one kind (device memory, 16-byte aligned): the kept ones
// (in the grid about centre cen, finite) appended in input order to b.vin with their keys, at most
// map_cap of them; the accumulators count on beyond that
hipError_t mp_map_bin_chunk(MpBuffers& b, MapIo& io, const float4* pts, int n, int kind, const int* cen,
                            hipStream_t st, Prof* prof);
// import: the accumulators into io.tab_h + kMapTabAcc (the caller synchronises st)
hipError_t mp_map_bin_result(MapIo& io, hipStream_t st);
// import: the kept points (<= map_cap) sorted stably by key into dst (map_cap points, not vin)
hipError_t mp_map_sort(MpBuffers& b, int kept, float4* dst, hipStream_t st, Prof* prof);
// the idle pool from instance 0's segment on (free between two frames, as vin)
inline float4* mp_map_idle_pool(const MpBuffers& b) { return b.pool + (size_t)(1 - b.pool_cur) * b.P * b.map_cap; }
// import: mp_map_sort into the idle pool, its slot table, the centre and the Bef / Aft poses of
// instance 0 (pose12: aft then bef); on success the store switches to that pool
hipError_t mp_map_install(MpBuffers& b, MapIo& io, int kept, const int* cen, const float* pose12, hipStream_t st,
                          Prof* prof);
// import: the slot table of the sorted points into io.tab + kMapTabSlots (k_mp_map_slots); nothing
// of the store changes (loam_lanes_map_import copies the points and the table into the lanes)
hipError_t mp_map_slots(MpBuffers& b, MapIo& io, hipStream_t st, Prof* prof);

// ---- multi-hypothesis localization in a streaming store (loam_map_localize) ----
// n candidate (Aft, Bef) poses, one sweep: each candidate's laserMapping L-M against the store of `s`
// (instance 0), which is only read.  The candidates are the instances of a working set `w` (an
// MpBuffers whose pools, cube VoxelGrid, insertion and registration buffers stay unallocated: P =
// the candidates, map_cap = the largest FromMap of a candidate); the sweep's two clouds are held
// once and read by every candidate.
constexpr int kLocMax = 1024;      // LOAM_LOCALIZE_MAX
constexpr int kLocResWords = 16;   // a candidate's result block (k_mp_loc_result)
enum { kLrAft = 0, kLrStatus = 6, kLrIters, kLrDegSteps, kLrRowsLast, kLrRowsSum, kLrStackC, kLrStackS, kLrMapC,
       kLrMapS };
static_assert(kLrMapS < kLocResWords, "result block");
struct MpLoc {
  MpBuffers w;            // the working set (w.P: the candidates of the current call)
  int cap_n = 0;          // candidates it holds
  int from_cap = 0;       // FromMap points per candidate it holds (w.map_cap)
  float* cand = nullptr;  // device [kLocMax][12]: aft, bef of every candidate
  int* head = nullptr;    // device [2 * kLocMax + 4]: every candidate's FromMap counts (corner, surf), then the store's error word
  int* res = nullptr;     // device [kLocMax][kLocResWords]
  char* pin = nullptr;    // pinned host copies of cand | head | res
  float* cand_h() const { return (float*)pin; }
  int* head_h() const { return (int*)(pin + (size_t)kLocMax * 12 * 4); }
  int* res_h() const { return head_h() + 2 * kLocMax + 4; }
  // loam_lanes_localize's plan block (allocated by its first call, mp_loc_reserve_rows): pinned, the
  // lanes' nlast words as they come down ([kLocMax][kOdBufs][2]) and the listed lanes' LaneLocPlan
  // entries as they go up; device, those entries
  char* plan_pin = nullptr;
  LaneLocPlan* plan = nullptr;  // device [kLocMax]
  int* nlast_h() const { return (int*)plan_pin; }
  LaneLocPlan* plan_h() const { return (LaneLocPlan*)(plan_pin + (size_t)kLocMax * kOdBufs * 2 * sizeof(int)); }
};
// loam_lanes_localize: instance p (a row) reads the sweep of listed lane p / k in place.  plan[i], i
// < n, is listed lane i (loc_plan.hpp); lastC / lastS / od_state are the lanes' OdBuffers arrays
struct LocRows {
  const LaneLocPlan* plan;  // device [n]
  int k;                    // rows per listed lane (the launch has n k instances)
  const float4 *lastC, *lastS;
  const float* od_state;    // [lanes][kOdStateFloats]
};
void mp_loc_free(MpLoc& L);
// the candidate tables and, for n candidates and a sweep of ncorner + nsurf points, the working set's
// per-candidate part (stacks sized by the sweep's counts rounded up, L-M state); grows, never
// shrinks.  On an allocation failure the working set is freed
hipError_t mp_loc_reserve(MpLoc& L, const MpBuffers& s, int n, int ncorner, int nsurf);
// the FromMap part (from, the two hash indexes) for from_max points per candidate
hipError_t mp_loc_reserve_map(MpLoc& L, int from_max);
// the plan block of loam_lanes_localize (nothing enqueued reads it when it is made)
hipError_t mp_loc_reserve_rows(MpLoc& L);
// k_mp_loc_prepare for n candidates (L.cand) on the sweep `in` (strides 0) + the counts into
// L.head_h(); the caller synchronises st, then reads them.  rows (loam_lanes_localize): the n
// candidates are rows of L.plan (L.plan_h() goes up first), `in` is not read
hipError_t mp_localize_prepare(MpLoc& L, const MpBuffers& s, const MpInput& in, int n, hipStream_t st, Prof* prof,
                               const LocRows* rows = nullptr);
// the stacks, the FromMap gather (from_max > 0), the hash builds, the L-M and the result blocks
// into L.res_h(); the caller synchronises st, then reads them.  from_max: the largest FromMap of a
// candidate, cloud_max: its largest corner or surf part; stack_max as mp_frame's.  rows: as above
hipError_t mp_localize_solve(MpLoc& L, const MpBuffers& s, const MpInput& in, int n, int from_max, int cloud_max,
                             int stack_max, hipStream_t st, Prof* prof, const LocRows* rows = nullptr);

// ---- shared lanes (loam_lanes_open_shared): every lane's mapping frame against one streaming store ----
// The lanes' working set: an MpBuffers of P lanes built as MpLoc::w is (no pools, slot tables, cube
// VoxelGrid or insertion buffers), with from_cap FromMap points per lane (its map_cap), each lane's
// own state and the registered clouds (reg / nreg).  On failure: freed, b empty.
hipError_t mp_alloc_shared(MpBuffers& b, int P, int R, int cap_pts, int from_cap, int max_iter);
// One mapping frame of the P lanes of w against the store of s (instance 0), which is only read:
// loam_map_localize's launch sequence with the lanes' kept Bef / Aft and IMU flags (k_mp_loc_prepare<true>),
// every lane's clouds read in place (in: per-lane strides), k_mp_register behind k_mp_lm_end, then
// every lane's k_mp_loc_result block into res (device, [P][kLocResWords]).  Waits on the device for a
// deferred update of s.  No launch form depends on a count the host would have to read: stack_max
// is unknown (-1), the gather's grid covers from_cap, the hash builds take the grid-per-cloud form
// iff from_cap > 8192 (a cloud beyond k_hash_build's LDS counters is possible), and the L-M never
// takes the persistent form.
void mp_lanes_shared_frame(MpBuffers& w, MpBuffers& s, const MpInput& in, int* res, hipStream_t st, Prof* prof);

// ---- shared lanes: the listed lanes' last frames into the store (loam_lanes_map_commit) ----
// The map update of mp_update for many stacks and one store: every listed lane's stack (w.stack, read
// in place with the lane's rotation, as k_mp_register maps its cloud) appended to the store's cubes in
// list order, the cubes of the union of the lanes' valid sets through one VoxelGrid each, the result
// compacted into the store's idle pool.  A key is kind * kCubeNum + cube, the export's canonical key.
// The result block (device and pinned copy): kCrErr 0 = done; kCrErrVin: the VoxelGrid input of the
// union's cubes (kCrVin, per kind) exceeds map_cap; kCrErrMap: the new map (kCrMap, per kind) does.
constexpr int kCmResWords = 16;
enum { kCrErr = 0, kCrIns = 1, kCrOut = 3, kCrMap = 5, kCrCubes = 7, kCrVin = 8 };
enum { kCrErrVin = 1, kCrErrMap = 2 };
constexpr int kCmUniWords = (kCubeNum + 31) / 32;
// the words one memset clears in front of a commit: the union bitmap, the VoxelGrid's list counters, the result block
constexpr int kCmZeroInts = kCmUniWords + 4 + kCmResWords;
struct MpCommit {
  int S = 0, cap_stack = 0, kmax = 0;  // lanes it holds, their stack stride, key entries per lane
  // per listed lane (by list position): a stack point's entry in the lane's key list (-1: outside the
  // grid) and its stable rank among the lane's points of that key
  int* ent_of = nullptr;    // [S][cap_stack]
  int* rank_of = nullptr;   // [S][cap_stack]
  int* lkey = nullptr;      // [S][kmax] the keys the lane's stack touches
  int* lcnt = nullptr;      // [S][kmax] their counts; behind k_cm_prefix the points of earlier listed lanes in the key
  int* lnk = nullptr;       // [S] entries of the lane
  float4* app = nullptr;    // [S * cap_stack] the appended points (map frame) grouped by key, lanes in list order
  int* list = nullptr;      // [S] the call's lane list
  int* zero = nullptr;      // [kCmZeroInts] uni | counts | res
  LOAM_HD unsigned* uni() const { return (unsigned*)zero; }  // the union of the listed lanes' valid cubes, a bit per cube
  LOAM_HD int* counts() const { return zero + kCmUniWords; }  // VgJob::counts ([2]: the segment list's length)
  LOAM_HD int* res() const { return zero + kCmUniWords + 4; }
  // per key: appended points (offset in app, count); the VoxelGrid segment of a union cube's key
  int *aoff = nullptr, *acnt = nullptr;                                         // [kMapKeys]
  int *seg_b = nullptr, *seg_e = nullptr, *seg_cnt = nullptr, *vlist = nullptr;  // [kMapKeys]
  float* seg_leaf = nullptr;
  int* lists[2] = {nullptr, nullptr};  // the cascade's lists [kMapKeys]
  int* pin = nullptr;       // pinned: the lane list [S], then the result block
  int* list_h() const { return pin; }
  int* res_h() const { return pin + S; }
};
// the working set for S lanes of cap_stack stack points (the first commit); on failure nothing is kept
hipError_t mp_commit_alloc(MpCommit& c, int S, int cap_stack);
void mp_commit_free(MpCommit& c);
// bytes mp_commit_alloc asks the device for (DESIGN.md §34 derives them)
size_t mp_commit_bytes(int S, int cap_stack);
// the n lanes of c.list_h() (indices below w.P, each once) into the store s: everything up to the new
// pool and slot table and the result block's copy into c.res_h().  The caller synchronises st, reads
// the block and, where kCrErr is 0, switches the store (s.pool_cur = 1 - s.pool_cur).  Only the
// commit's buffers, the store's idle pool / slot table and its VoxelGrid scratch (vin, vout, the sort
// arrays) are written.
hipError_t mp_lanes_commit(MpCommit& c, const MpBuffers& w, MpBuffers& s, int n, hipStream_t st, Prof* prof);
// lane `lane`'s stack in the map frame by the commit's transform, in stack order (corner into outC,
// surf into outS: device, capC / capS points) — loam_dev_lanes_commit_input
hipError_t mp_lanes_commit_input(const MpBuffers& w, int lane, float4* outC, float4* outS, hipStream_t st);

}  // namespace loam
#endif
