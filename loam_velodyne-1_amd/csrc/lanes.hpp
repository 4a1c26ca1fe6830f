// Lanes (loam_lanes_*): S independent sequences in one context, advanced one sweep each per call.
// The working set is the batch's (an SrBuffers of S sweeps, an OdBuffers and an MpBuffers of S
// problems) with the streaming path's life cycle: nothing is reset between steps.  Engine-internal.
#ifndef LOAM_LANES_HPP
#define LOAM_LANES_HPP

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "engine.hpp"
#include "lanes_clouds_plan.hpp"
#include "lanes_feed_plan.hpp"
#include "point_fields.hpp"
#include "mp.hpp"
#include "od.hpp"

namespace loam {

// a lane's block of the step's result (k_lanes_out), 32-bit words
enum { kLoSrErr = 0, kLoOdErr, kLoMpErr, kLoOdIters, kLoMpIters, kLoNReg, kLoOdSum = 6, kLoAft = 12, kLoBef = 18,
       kLoLmRan = 24, kLaneOutWords = 25 };

// The lanes' IMU side (loam_lanes_imu); nothing of it exists until the first message.
// Host: a scanRegistration queue (entries and `last`) and a laserMapping queue per lane.  Device:
// the queues, whose tails (front, Start, Cur, FromStart) only the kernels write.
struct LanesImu {
  bool on = false;
  std::vector<loamimu::SrQueue> sr;  // [S] host master of the entries and of last
  std::vector<loamimu::MpQueue> mp;  // [S]
  std::vector<double> last_stamp;    // [S]
  std::vector<int> n_new;            // [S] messages since the last pushed step
  loamimu::SrQueue* q_d = nullptr;   // [S]
  loamimu::SrTail* tail_d = nullptr; // [S]
  int* tile_key_d = nullptr;         // [S][ntiles][3]
  // a step's upload: [S] LaneHdr, then the new entries as LaneRec (at most kQue per lane)
  char* up_h = nullptr;              // pinned
  char* up_d = nullptr;
  float* trans_d = nullptr;          // [S][12] /imu_trans of the step (k_lanes_imu)
  float* trans_h = nullptr;          // pinned copy
  bool step_imu = false;             // the step in flight took the IMU form
  std::vector<int> mp_front;         // [S] mp_lookup's advanced pointer of the step in flight ...
  std::vector<char> mp_have;         // ... and whether the lane had a message to look up
  size_t up_bytes = 0;               // what the last IMU step uploaded
};

// LaneLife::due: set where the pushed step wraps the lane's phase (kDuePushed), confirmed by the pull
// against the lane's status (kDueYes: what loam_lanes_surround serves), dropped by the next push, by
// loam_lanes_restart and by loam_lanes_map_import
enum { kDueNo = 0, kDuePushed, kDueYes };
// a lane's own life cycle (loam_lanes_restart); the host owns it
struct LaneLife {
  int wait = -1;   // -1: the lane follows the shared counters; >= 0: restarted, its init frame is the step after `wait` more
  int kind = 0;    // the step in flight: kLaneRuns, kLaneWaits (an empty problem, LOAM_E_NOT_READY) or kLaneInits
  int phase = 4;   // laserMapping's mapFrameCount of this lane (loam_lanes_map_export's surround_phase)
  int due = kDueNo;  // /laser_cloud_surround of the lane's last frame (loam_lanes_surround)
};
enum { kLaneRuns = 0, kLaneWaits, kLaneInits };
// words of loam_lanes_map_import's block: centre[3], Bef[6], then the list and the poses
enum { kMiCen = 0, kMiBef = 3, kMiList = 9 };
// what k_lanes_restart clears of a lane
enum { kClearOd = 1, kClearMp = 2, kClearImu = 4 };

struct Lanes {
  int S = 0;           // 0: not open
  // loam_lanes_open_shared: mp is a working set without a store (mp_alloc_shared,
  // mp.map_cap = lane_from_capacity) and a mapping frame reads the context's streaming store
  bool shared = false;
  SrBuffers sr;        // S sweeps
  OdBuffers od;        // S problems; Last buffers 0 and 1 alternate, as the streaming path's
  MpBuffers mp;        // S stores (shared lanes: S working sets, no store)
  // the step's sweeps: packed back to back in pinned memory, copied to the device staging in
  // chunks, scattered to sr.raw's stride by one kernel (as loam_batch_feed)
  float4* stage_h = nullptr;  // pinned [S * cap]
  float4* stage_d = nullptr;  // device [S * cap]
  int* tab_h = nullptr;       // pinned [2S]: sizes, then offsets
  int* tab_d = nullptr;       // device [2S]
  // loam_lanes_push_device's descriptor block (allocated by the first call) and the two events that
  // order a step's gather against the producer's stream (created by the first call that needs them)
  LaneFeedDesc* fd_h = nullptr;  // pinned [S]
  LaneFeedDesc* fd_d = nullptr;  // device [S]
  hipEvent_t feed_wait = nullptr, feed_release = nullptr;
  int* out_d = nullptr;       // device [S][kLaneOutWords]
  int* out_h = nullptr;       // pinned copy, read by loam_lanes_pull after the step's one synchronisation
  // the node state every lane shares (lockstep): scanRegistration's systemDelay counter,
  // laserOdometry's systemInited / frameCount, laserMapping's mapFrameCount
  int sr_init_count = 0;
  bool sr_inited = false, od_inited = false;
  int od_last = 0, od_frame_count = 1;
  std::vector<LaneLife> life;  // [S]
  // loam_lanes_restart's lists of a step (allocated by the first restart): the lanes to clear in
  // front of it, then the lanes whose init frame it is
  int* rs_h = nullptr;         // pinned [2S]
  int* rs_d = nullptr;         // device [2S]
  // loam_lanes_map_import's block of a call (allocated by the first import): the centre and Bef,
  // the n lane indices, then their n Aft poses of 6 floats (kMi*)
  int* mi_h = nullptr;         // pinned [kMiList + 7S]
  int* mi_d = nullptr;         // device [kMiList + 7S]
  // loam_lanes_surround's lists of a call (allocated by the first call): the due lanes up, every
  // lane's VoxelGrid output count down
  int* su_h = nullptr;         // pinned [2S]: the due list, then the counts by lane
  int* su_d = nullptr;         // device [S]: the due list
  // loam_lanes_set_pose's block of a call (allocated by the first call): the n lane indices, then
  // their n (Aft, Bef) pairs of 12 floats
  int* sp_h = nullptr;         // pinned [13S]
  int* sp_d = nullptr;         // device [13S]
  // shared lanes: every lane's k_mp_loc_result block of a mapping step, its pinned copy, and what
  // loam_lanes_localize_info hands out (filled by the pull)
  int* loc_d = nullptr;        // device [S][kLocResWords]
  int* loc_h = nullptr;        // pinned copy
  std::vector<loam_localize_result> loc_info;  // [S]
  // loam_lanes_map_commit: its working set (allocated by the first call) and which
  // lanes' last pulled frames are in the map already (cleared by every pull)
  MpCommit cm;
  std::vector<char> committed;  // [S]
  // loam_lanes_clouds, allocated by the first call: the lanes' validity masks (bit c:
  // cloud c of the lane is there) and the lane list up, the offsets table down, and the event a
  // consumer's stream waits for (created by the first call that is given one)
  int* cl_h = nullptr;            // pinned [2S]: masks by lane, then the list
  int* cl_d = nullptr;            // device [2S]
  uint64_t* cl_tab_h = nullptr;   // pinned [kLaneClouds][S + 1]
  uint64_t* cl_tab_d = nullptr;   // device [kLaneClouds][S + 1]
  hipEvent_t cl_done = nullptr;
  // the protocol: a step pushed and not yet pulled; what that step published; whether the last
  // pulled step left registered clouds
  bool in_flight = false, step_ran = false, have_reg = false;
  int step_pub = 0, step_mapped = 0;
  std::vector<int> fail;       // [S] sticky failure of a lane (LOAM_OK: live); the host owns it
  std::vector<int> fail_new;   // [S] what the host found wrong with the pushed sweep
  std::vector<uint32_t> nreg;  // [S] registered points of the last pulled step
  LanesImu imu;
  bool pulled = false;           // a step has been pulled
  std::vector<float> imu_trans;  // [S][12] /imu_trans of the last pulled step (zeros without IMU)
};

// launch choices of the lanes' L-M loops: the context's, without the two forms a lane may not take
// (the persistent one-problem kernels and the per-query moments; loam.h, loam_lanes_open)
Tuning lanes_tuning(Tuning t);
// the working set for S lanes (sweeps of cap points, R rings); on failure everything is freed
// shared: map_cap is lane_from_capacity and no lane gets a store (Lanes::shared)
hipError_t lanes_alloc(Lanes& L, int S, int cap, int R, int map_cap, int od_max_iter, int mp_max_iter,
                       bool shared = false);
void lanes_free(Lanes& L);
// k_lanes_out: every lane's block into out_d, then its copy into out_h
// loc (shared lanes, a mapping step): the step's k_mp_loc_result blocks are in loc_d: a
// LOAM_LOC_OFFGRID lane reports no registered point, and the blocks are copied into loc_h
hipError_t lanes_out(const Lanes& L, hipStream_t st, bool loc = false);
// the IMU side's buffers (the first loam_lanes_imu); on failure they are freed and imu.on stays false
hipError_t lanes_imu_alloc(Lanes& L);
void lanes_imu_free(Lanes& L);
// k_lanes_imu_put: the step's upload (imu.up_h, `bytes` of it, nrec entries behind the headers)
// to the device and the new entries and `last` into the device queues
hipError_t lanes_imu_put(Lanes& L, size_t bytes, int nrec, hipStream_t st);
// k_lanes_imu, behind the ring sort: commits the tails, writes every IMU lane's /imu_trans into the
// odometry state (od_init: and transformSum's start, src/laserOdometry.cpp:451-452) and into
// imu.trans_d, and on mapping steps every lane's (roll, pitch, flag) into the mapping state
hipError_t lanes_imu_commit(Lanes& L, bool od_init, bool mapping, hipStream_t st);

// the device feed's descriptor block (the first loam_lanes_push_device); on failure nothing is kept
hipError_t lanes_feed_alloc(Lanes& L);
// k_lanes_gather_dev: L.fd_h's S descriptors to the device, then every feeding lane's sweep from the
// caller's device memory into sr.raw at its stride and every lane's size into sr.raw_n
// pf (optional): the context's point fields and their map on the device: the gather's field form
// writes each point's word into w (point_fields.hpp)
hipError_t lanes_gather_dev(Lanes& L, int cap, hipStream_t st, const PointFields* pf = nullptr, const int16_t* map_d = nullptr);
// the kernel alone on device descriptors (loam_dev_lanes_gather)
hipError_t lanes_gather_launch(const LaneFeedDesc* desc_d, float4* raw, int* raw_n, int cap, int S, hipStream_t st);

// the restart lists' buffers (the first loam_lanes_restart)
hipError_t lanes_restart_alloc(Lanes& L);
// k_lanes_restart: one launch that leaves the n lanes of list_d (device) as lanes_alloc left them,
// in the parts `what` names (kClear*)
hipError_t lanes_restart_clear(Lanes& L, const int* list_d, int n, int what, hipStream_t st);
// k_lanes_init, behind the step's shared k_od_end and in front of its hash build: the n lanes of
// list_d end the step as the odometry's init frame leaves a context: Last[dst] = the raw lessSharp
// / lessFlat clouds, transform zero, transformSum zero or the IMU start pitch / roll, istate zero
hipError_t lanes_init_frame(Lanes& L, const FeatView& f, const int* list_d, int n, int dst, hipStream_t st);


// loam_lanes_map_import's argument check of the lane list (host only): 0, or which rule lane[*bad]
// breaks.  n in [1, S] is the caller's to check; lane[] is read below n only, and fail / wait (S
// entries: a lane's sticky failure, LaneLife::wait) only at indices below S
enum { kLaneListOk = 0, kLaneListRange, kLaneListTwice, kLaneListFailed, kLaneListWaits };
inline int lanes_list_check(const uint32_t* lane, uint32_t n, int S, const int* fail, const LaneLife* life,
                            std::vector<char>& seen, uint32_t* bad) {
  seen.assign((size_t)S, 0);
  for (uint32_t i = 0; i < n; ++i) {
    *bad = i;
    const uint32_t l = lane[i];
    if (l >= (uint32_t)S) return kLaneListRange;
    if (seen[l]) return kLaneListTwice;
    seen[l] = 1;
    if (fail[l] != LOAM_OK) return kLaneListFailed;
    if (life[l].wait >= 0) return kLaneListWaits;
  }
  return kLaneListOk;
}

// loam_lanes_map_commit's argument check of the lane list (host only): 0, or which rule the count or
// lane[*bad] breaks.  lane[] is read below n only, and only when n is in [1, S]; fail / life / status /
// committed have S entries and are read at indices below S: a lane's sticky failure, its life cycle,
// the LOAM_LOC_* status of its last pulled step (LOAM_LOC_NONE where it ran no mapping frame of its
// own) and whether that frame was committed since
enum { kCommitOk = 0, kCommitCount, kCommitRange, kCommitTwice, kCommitFailed, kCommitWaits, kCommitNoFrame,
       kCommitOffgrid, kCommitDone };
inline int lanes_commit_check(const uint32_t* lane, uint32_t n, int S, const int* fail, const LaneLife* life,
                              const int32_t* status, const char* committed, std::vector<char>& seen, uint32_t* bad) {
  *bad = 0;
  if (S <= 0 || n == 0 || n > (uint32_t)S) return kCommitCount;
  seen.assign((size_t)S, 0);
  for (uint32_t i = 0; i < n; ++i) {
    *bad = i;
    const uint32_t l = lane[i];
    if (l >= (uint32_t)S) return kCommitRange;
    if (seen[l]) return kCommitTwice;
    seen[l] = 1;
    if (fail[l] != LOAM_OK) return kCommitFailed;
    if (life[l].wait >= 0) return kCommitWaits;
    if (status[l] == LOAM_LOC_OFFGRID) return kCommitOffgrid;
    if (status[l] != LOAM_LOC_SOLVED && status[l] != LOAM_LOC_NO_LM) return kCommitNoFrame;
    if (committed[l]) return kCommitDone;
  }
  return kCommitOk;
}

// loam_lanes_open_shared's capacity arithmetic (host only): LOAM_OK, or which limit the arguments
// break.  cap_stack = max_points + 120 n_rings; the products are the int bases of the lanes' FromMap
// and stack segments (VgJob::total, MpBuffers' strides)
enum { kSharedOk = 0, kSharedLanes, kSharedFromCap, kSharedFromProduct, kSharedStackProduct };
inline int lanes_shared_check(uint32_t n_lanes, uint32_t from_cap, uint64_t cap_stack) {
  if (n_lanes == 0 || n_lanes > LOAM_LANES_MAX) return kSharedLanes;
  if (from_cap < 1024 || from_cap > (1u << 28)) return kSharedFromCap;
  if ((uint64_t)n_lanes * from_cap >= ((uint64_t)1 << 31)) return kSharedFromProduct;
  if ((uint64_t)n_lanes * cap_stack >= ((uint64_t)1 << 31)) return kSharedStackProduct;
  return kSharedOk;
}

// the set-pose block's buffers (the first loam_lanes_set_pose)
hipError_t lanes_set_pose_alloc(Lanes& L);
// k_lanes_set_pose: one launch that writes Aft and Bef of the n lanes of L.sp_h's block (uploaded
// here) into their mapping state; the caller synchronises st before it refills the block
hipError_t lanes_set_pose(Lanes& L, int n, hipStream_t st);

// the import lists' buffers (the first loam_lanes_map_import)
hipError_t lanes_map_import_alloc(Lanes& L);
// k_lanes_map_install: one launch that copies `kept` sorted points (src) and their slot table
// (table, [kCubeNum] int4) into the current pool segment and slot table of each of the n lanes
// of L.mi_d's block, and writes each lane's centre, Aft and Bef from that block.  src and table are
// not part of any lane's live data.
hipError_t lanes_map_install(Lanes& L, const float4* src, int kept, const int* table, int n, hipStream_t st);


// the surround lists' buffers (the first loam_lanes_surround)
hipError_t lanes_surround_alloc(Lanes& L);
// /laser_cloud_surround of the n due lanes listed in L.su_h (ascending): the list's upload,
// k_lanes_surround (each lane's 5x5x5 cube neighbourhood gathered from its current pool into its part
// of vin, its VoxelGrid segment and list entry), one VoxelGrid over the listed segments (lane l's
// output at vout + l * map_cap, its count at vseg_cnt[l]), with `pack` k_lanes_surround_pack (the
// outputs back to back in list order from vin[0] on), and every lane's count into L.su_h + S.  The
// caller synchronises st, then reads the counts (lanes_surround_count).  Only scratch is written.
hipError_t lanes_surround_run(Lanes& L, int n, bool pack, hipStream_t st, Prof* prof);
// a lane's output count as the pack kernel reads it
inline int lanes_surround_count(const Lanes& L, int lane) {
  return std::min(std::max(L.su_h[L.S + lane], 0), L.mp.map_cap);
}


// ---- loam_lanes_clouds: the lanes' clouds packed back to back over a list of lanes
// cloud c of lane l: count[l * count_stride] points (clamped to [0, stride]) from base + l * stride
struct LanePackSrc {
  const float4* base;
  const int* count;
  int stride, count_stride;
};
struct LanePackJob {
  LanePackSrc c[kLaneClouds];
  int S;
};
// where a launch puts cloud c: point k of its selection over the list at dst[c][dbase[c] + k]
struct LanePackDst {
  float4* dst[kLaneClouds];
  long long dbase[kLaneClouds];
};
constexpr int kLanePackTile = 1024;  // points a workgroup moves per pass (dev_hooks.h LOAM_DEV_LANES_PACK_TILE)
// the masks / list block, the table and its pinned copy (the first loam_lanes_clouds)
hipError_t lanes_clouds_alloc(Lanes& L);
// the nine clouds of the last step where they lie: L.sr, the odometry's buffer L.od_last, mp.reg
LanePackJob lanes_pack_job(const Lanes& L);
// k_lanes_pack_offsets: table [kLaneClouds][n + 1] (device), table[c][j] = points of cloud c in list
// entries [0, j), an entry counting where bit c of mask[list[j]] is set.  mask [job.S], list [n]: device.
hipError_t lanes_pack_offsets(const LanePackJob& job, const int* mask, const int* list, int n, uint64_t* table,
                              hipStream_t st);
// k_lanes_pack: entries [j0, j0 + nj) of that table, the clouds in the bit mask `clouds`
hipError_t lanes_pack(const LanePackJob& job, const uint64_t* table, const int* list, int n, int j0, int nj,
                      unsigned clouds, const LanePackDst& d, hipStream_t st);

}  // namespace loam
#endif
