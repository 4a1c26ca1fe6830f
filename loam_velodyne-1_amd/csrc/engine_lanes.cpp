// libloam_hip host engine: loam_lanes_* and the loam_dev_lanes_* hooks.
#include <cmath>

#include "engine_ctx.hpp"

// ------------------------------------------------------------------ lanes
// S sequences in lockstep (loam.h): a step is the batch's launch sequences on the
// lanes' own working set, with the streaming path's life cycle.  What loam_chain_sweep keeps in the
// context per sequence (system_delay, the odometry's init frame and frame counter, the surround
// phase) is kept once for all lanes; what it keeps on the device (the odometry state, the Last
// clouds, the map store) is the batch buffers' per-problem state, never cleared between steps.
namespace {
// what is wrong with a lane's pushed sweep before any kernel sees it (LOAM_OK: nothing)
// (fields_end: the end of the context's point fields in a record, 0 without them)
int lane_sweep_code(const loam_cloud_in& c, int cap, uint32_t fields_end) {
  if (c.count == 0) return LOAM_E_INVAL;
  if (c.data == nullptr || c.stride_bytes < 12 || c.stride_bytes % 4 != 0 || c.stride_bytes < fields_end) return LOAM_E_INVAL;
  if (c.count > (uint32_t)cap) return LOAM_E_CAPACITY;
  return LOAM_OK;
}

// whether the step about to be enqueued runs laserMapping (lanes_enqueue's `pub`)
bool lanes_will_map(const loam_ctx* x) {
  const Lanes& L = x->lanes;
  return L.od_inited && L.od_frame_count + 1 >= (int)x->cfg.skip_frame_num + 1;
}

// one step's device work on x->st, behind the sweeps' upload; sets L.step_pub / L.step_mapped
// imu: the step's LaneHdr block and new queue entries are on the device (lanes_imu_put): the ring
// sort takes the tile-parallel IMU form and k_lanes_imu follows it
// n_init: the lanes whose own init frame this step is (loam_lanes_restart), listed at L.rs_d + S
hipError_t lanes_enqueue(loam_ctx* x, Prof* pf, bool imu, int n_init) {
  Lanes& L = x->lanes;
  const int S = L.S;
  hipStream_t st = x->st;
  OdBuffers& o = L.od;
  hipError_t e = hipSuccess;
  auto T = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  SrParams prm = sr_params(x);
  if (imu) {
    prm.imu = L.imu.q_d;
    prm.imu_lane = (const loamimu::LaneHdr*)L.imu.up_d;
    prm.imu_tail = L.imu.tail_d;
    prm.imu_tile_key = L.imu.tile_key_d;
  }
  sr_launch(L.sr, prm, st, pf);
  if (imu) {
    T(lanes_imu_commit(L, !L.od_inited, lanes_will_map(x), st));
    x->prof.mark("k_lanes_imu");
  }
  const FeatView f = feat_view(L.sr, 0, 1);
  L.step_pub = 0;
  L.step_mapped = 0;
  if (!L.od_inited) {  // src/laserOdometry.cpp:427-456: Last = raw lessSharp / lessFlat, no L-M (od_frame's init frame)
    hipLaunchKernelGGL(k_od_end, dim3(kOdEndWg, S), dim3(256), 0, st, o, f, 0, 0, 0);
    x->prof.mark("k_od_end");
    od_build_hashes(o, 0, st);
    x->prof.mark("k_hash_build_last");
    L.od_last = 0;
    L.od_inited = true;
    L.step_pub = LOAM_PUB_CLOUDS;
  } else {
    const int cur = L.od_last, nxt = 1 - cur;
    od_solve(o, f, cur, st, pf, /*device_fini=*/true);
    x->prof.mark("k_od_fini");
    L.od_frame_count++;
    const bool pub = L.od_frame_count >= (int)x->cfg.skip_frame_num + 1;
    hipLaunchKernelGGL(k_od_end, dim3(kOdEndWg, S), dim3(256), 0, st, o, f, nxt, 2, pub ? 1 : 0);
    x->prof.mark("k_od_end");
    if (n_init) {  // restarted lanes: the init frame's Last clouds and state over the ordinary frame's
      T(lanes_init_frame(L, f, L.rs_d + S, n_init, nxt, st));
      x->prof.mark("k_lanes_init");
    }
    od_build_hashes(o, nxt, st);
    x->prof.mark("k_hash_build_last");
    L.od_last = nxt;
    L.step_pub = LOAM_PUB_POSE;
    if (pub) {
      L.od_frame_count = 0;
      L.step_pub |= LOAM_PUB_CLOUDS | LOAM_PUB_FULL;
      // laserMapping on the published clouds in place, as the device chain reads them: fullEnd is
      // already at the sweep's end, the pose is the transformSum the odometry left on the device
      MpInput in;
      in.corner = o.lastC + (size_t)nxt * o.P * o.capC;
      in.surf = o.lastS + (size_t)nxt * o.P * o.capS;
      in.full = o.fullEnd + (size_t)nxt * o.P * o.capS;
      in.corner_stride = o.capC; in.surf_stride = o.capS; in.full_stride = o.capS;
      in.ncorner = o.nlast + nxt * 2; in.nsurf = o.nlast + nxt * 2 + 1; in.nfull = o.nfullEnd + nxt;
      in.ncorner_stride = in.nsurf_stride = 2 * kOdBufs; in.nfull_stride = kOdBufs;
      in.pose = o.state + kOdSum; in.pose_stride = kOdStateFloats;
      // shared lanes: loam_map_localize's sequence over the lanes against the context's store, read only
      if (L.shared) mp_lanes_shared_frame(L.mp, x->mp1, in, L.loc_d, st, pf);
      else mp_frame(L.mp, in, st, pf);
      L.step_mapped = 1;
      for (int l = 0; l < S; ++l)  // :1038-1040, for the lanes this was a mapping frame for
        if (L.life[l].kind == kLaneRuns && ++L.life[l].phase >= 5) {
          L.life[l].phase = 0;
          L.life[l].due = kDuePushed;  // (/laser_cloud_surround, once the pull has seen the lane's status)
        }
      if (n_init) {  // (skip_frame_num = 0) an init frame does not map: the lane's store is empty again
        T(lanes_restart_clear(L, L.rs_d + S, n_init, kClearMp, st));
        x->prof.mark("k_lanes_restart");
      }
    }
  }
  T(lanes_out(L, st, L.shared && L.step_mapped));
  x->prof.mark("k_lanes_out");
  T(hipGetLastError());
  return e;
}

// The three refusals of the lanes' state every entry point words alike, in this order: of `need`,
// the first that does not hold.  LOAM_OK, or the failure.
enum { kLanesOpen = 1, kLanesIdle = 2, kLanesPulled = 4 };
int lanes_state_refused(const std::string& who, const Lanes& L, int need) {
  if ((need & kLanesOpen) && !L.S) return fail(LOAM_E_INVAL, who + ": lanes are not open");
  if ((need & kLanesIdle) && L.in_flight) return fail(LOAM_E_INVAL, who + ": a step is in flight (loam_lanes_pull first)");
  if ((need & kLanesPulled) && !L.pulled) return fail(LOAM_E_INVAL, who + ": no step was pulled");
  return LOAM_OK;
}

// loam_lanes_open / loam_lanes_open_shared behind their argument checks
int lanes_open_tail(loam_ctx* x, const std::string& who, uint32_t n_lanes, uint32_t capacity, bool shared) {
  HIP_TRY(hipSetDevice(x->device));
  const hipError_t he = lanes_alloc(x->lanes, (int)n_lanes, x->cap, x->R, (int)capacity, (int)x->cfg.od_max_iter,
                                    (int)x->cfg.mp_max_iter, shared);
  if (he != hipSuccess) return nomem(who + ": allocation failed: " + hipGetErrorString(he));
  Lanes& L = x->lanes;
  L.od.tune = L.mp.tune = lanes_tuning(x->tune);
  L.od_frame_count = (int)x->cfg.skip_frame_num;  // frameCount = skipFrameNum (src/laserOdometry.cpp:407)
  x->seen_sweep = true;  // (loam_set_ring_table: the lanes' sweeps take the context's ring model as it is now)
  return LOAM_OK;
}
}  // namespace

extern "C" int loam_lanes_open(loam_ctx* x, uint32_t n_lanes, uint32_t lane_map_capacity) {
  if (!x) return fail(LOAM_E_INVAL, "null argument");
  if (x->lanes.S) return fail(LOAM_E_INVAL, "loam_lanes_open: lanes are open (loam_lanes_close first)");
  if (n_lanes == 0 || n_lanes > LOAM_LANES_MAX)
    return fail(LOAM_E_INVAL, "loam_lanes_open: n_lanes must be in [1, LOAM_LANES_MAX]");
  if (lane_map_capacity < 1024 || lane_map_capacity > (1u << 28))
    return fail(LOAM_E_INVAL, "loam_lanes_open: lane_map_capacity must be in [1024, 2^28] points");
  // (the stores' and stacks' segment bases and VgJob::total are ints)
  const uint64_t cap_stack = (uint64_t)x->cap + (uint64_t)kLessSharpPerRing * x->R;
  if ((uint64_t)n_lanes * lane_map_capacity >= ((uint64_t)1 << 31))
    return fail(LOAM_E_INVAL, "loam_lanes_open: n_lanes x lane_map_capacity reaches 2^31 points");
  if ((uint64_t)n_lanes * cap_stack >= ((uint64_t)1 << 31))
    return fail(LOAM_E_INVAL, "loam_lanes_open: n_lanes x stack capacity (max_points + 120 n_rings) reaches 2^31 points");
  return lanes_open_tail(x, "loam_lanes_open", n_lanes, lane_map_capacity, /*shared=*/false);
}

// Shared lanes (loam.h): the lanes' mapping working set holds no store, a mapping
// step reads x->mp1's.
extern "C" int loam_lanes_open_shared(loam_ctx* x, uint32_t n_lanes, uint32_t lane_from_capacity) {
  if (!x) return fail(LOAM_E_INVAL, "null argument");
  const std::string who = "loam_lanes_open_shared";
  if (x->lanes.S) return fail(LOAM_E_INVAL, who + ": lanes are open (loam_lanes_close first)");
  const uint64_t cap_stack = (uint64_t)x->cap + (uint64_t)kLessSharpPerRing * x->R;
  switch (lanes_shared_check(n_lanes, lane_from_capacity, cap_stack)) {
    case kSharedLanes: return fail(LOAM_E_INVAL, who + ": n_lanes must be in [1, LOAM_LANES_MAX]");
    case kSharedFromCap: return fail(LOAM_E_INVAL, who + ": lane_from_capacity must be in [1024, 2^28] points");
    case kSharedFromProduct: return fail(LOAM_E_INVAL, who + ": n_lanes x lane_from_capacity reaches 2^31 points");
    case kSharedStackProduct:
      return fail(LOAM_E_INVAL, who + ": n_lanes x stack capacity (max_points + 120 n_rings) reaches 2^31 points");
    default: break;
  }
  return lanes_open_tail(x, who, n_lanes, lane_from_capacity, /*shared=*/true);
}

namespace {
// lanes_list_check's four rules with their messages: LOAM_OK, or the failure.  for_import: in
// loam_lanes_map_import's words (no value behind an index out of range, its own advice to a waiting lane)
int lanes_list_refused(const std::string& who, const Lanes& L, const uint32_t* lane, uint32_t n, bool for_import = false) {
  std::vector<char> seen;
  uint32_t bad = 0;
  const int why = lanes_list_check(lane, n, L.S, L.fail.data(), L.life.data(), seen, &bad);
  if (why == kLaneListOk) return LOAM_OK;
  const std::string at = who + ": lane[" + std::to_string(bad) + "]" +
                         (for_import && why == kLaneListRange ? "" : " = " + std::to_string(lane[bad]));
  if (why == kLaneListRange) return fail(LOAM_E_INVAL, at + " is out of range");
  if (why == kLaneListTwice) return fail(LOAM_E_INVAL, at + " is listed twice");
  if (why == kLaneListFailed) return fail(LOAM_E_INVAL, at + " has failed (loam_lanes_restart first)");
  if (for_import)
    return fail(LOAM_E_INVAL, at + " was restarted and waits for its init step: import after the lane's init step");
  return fail(LOAM_E_INVAL, at + " waits for its init step (the restart's clear would overwrite the pose)");
}
}  // namespace

extern "C" int loam_lanes_set_pose(loam_ctx* x, uint32_t n, const uint32_t* lane, const loam_pose6* aft,
                                   const loam_pose6* bef) {
  if (!x || !lane || !aft) return fail(LOAM_E_INVAL, "null argument");
  const std::string who = "loam_lanes_set_pose";
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused(who, L, kLanesOpen)) return rc;
  if (!L.shared) return fail(LOAM_E_INVAL, who + ": the lanes have their own maps (loam_lanes_open); use loam_lanes_map_import");
  if (const int rc = lanes_state_refused(who, L, kLanesIdle)) return rc;
  if (n == 0 || n > (uint32_t)L.S) return fail(LOAM_E_INVAL, who + ": n must be in [1, n_lanes]");
  if (const int rc = lanes_list_refused(who, L, lane, n)) return rc;
  HIP_TRY(hipSetDevice(x->device));
  if (lanes_set_pose_alloc(L) != hipSuccess) return nomem(who + ": allocation failed");
  for (uint32_t i = 0; i < n; ++i) L.sp_h[i] = (int)lane[i];
  cand_rows((float*)(L.sp_h + n), n, aft, bef);
  hipError_t he = lanes_set_pose(L, (int)n, x->st);
  const hipError_t se = hipStreamSynchronize(x->st);
  if (he == hipSuccess) he = se;
  if (he != hipSuccess) return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
  return LOAM_OK;
}

extern "C" int loam_lanes_localize_info(loam_ctx* x, loam_localize_result* out) {
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  const std::string who = "loam_lanes_localize_info";
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused(who, L, kLanesOpen)) return rc;
  if (!L.shared) return fail(LOAM_E_INVAL, who + ": the lanes have their own maps (loam_lanes_open)");
  if (const int rc = lanes_state_refused(who, L, kLanesIdle | kLanesPulled)) return rc;
  std::memcpy(out, L.loc_info.data(), (size_t)L.S * sizeof(loam_localize_result));
  return LOAM_OK;
}

namespace {
// loam_lanes_map_commit's refusals of the call itself and of the lane list (lanes_commit_check's
// rules with their messages): LOAM_OK, or the failure
int lanes_commit_refused(const std::string& who, loam_ctx* x, const uint32_t* lane, uint32_t n) {
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused(who, L, kLanesOpen)) return rc;
  if (!L.shared)
    return fail(LOAM_E_INVAL, who + ": the lanes have their own maps (loam_lanes_open), which they write themselves");
  if (const int rc = lanes_state_refused(who, L, kLanesIdle | kLanesPulled)) return rc;
  std::vector<char> seen;
  std::vector<int32_t> status((size_t)L.S);
  for (int l = 0; l < L.S; ++l) status[l] = L.loc_info[l].status;
  uint32_t bad = 0;
  const int why = lanes_commit_check(lane, n, L.S, L.fail.data(), L.life.data(), status.data(), L.committed.data(), seen, &bad);
  if (why == kCommitOk) return LOAM_OK;
  if (why == kCommitCount) return fail(LOAM_E_INVAL, who + ": n must be in [1, n_lanes]");
  const std::string at = who + ": lane[" + std::to_string(bad) + "] = " + std::to_string(lane[bad]);
  if (why == kCommitRange) return fail(LOAM_E_INVAL, at + " is out of range");
  if (why == kCommitTwice) return fail(LOAM_E_INVAL, at + " is listed twice");
  if (why == kCommitFailed) return fail(LOAM_E_INVAL, at + " has failed (loam_lanes_restart first)");
  if (why == kCommitWaits) return fail(LOAM_E_INVAL, at + " waits for its init step");
  if (why == kCommitOffgrid)
    return fail(LOAM_E_INVAL, at + " was not evaluated (LOAM_LOC_OFFGRID: the frame would recentre the grid)");
  if (why == kCommitDone) return fail(LOAM_E_INVAL, at + ": its last frame is in the map already (a frame enters the map once)");
  return fail(LOAM_E_INVAL, at + " ran no mapping frame on the last pulled step");
}
// the store's error word after the context's queued work has been drained
int store_overflowed(loam_ctx* x, const std::string& who) {
  int err = 0;
  HIP_TRY(hipMemcpy(&err, x->mp1.istate + kMiErr, sizeof(int), hipMemcpyDeviceToHost));
  if (err & ERR_CAP_MAP) return store_invalid(who);
  return LOAM_OK;
}
}  // namespace

// The listed lanes' last frames into the context's streaming store (mp_lanes_commit):
// built in the store's idle pool, which becomes the current one after the result block says it fits.
extern "C" int loam_lanes_map_commit(loam_ctx* x, uint32_t n, const uint32_t* lane, loam_commit_result* out) {
  if (!x || !lane || !out) return fail(LOAM_E_INVAL, "null argument");
  const std::string who = "loam_lanes_map_commit";
  if (const int rc = lanes_commit_refused(who, x, lane, n)) return rc;
  Lanes& L = x->lanes;
  if (const int rc = map_drain(x)) return rc;
  if (const int rc = store_overflowed(x, who)) return rc;
  if (mp_commit_alloc(L.cm, L.S, L.mp.cap_stack) != hipSuccess) return nomem(who + ": allocation failed");
  MpBuffers& s = x->mp1;
  for (uint32_t i = 0; i < n; ++i) L.cm.list_h()[i] = (int)lane[i];
  hipStream_t st = x->st;
  x->prof.begin(st);
  hipError_t he = mp_lanes_commit(L.cm, L.mp, s, (int)n, st, &x->prof);
  const hipError_t se = hipStreamSynchronize(st);
  if (he == hipSuccess) he = se;
  x->prof.collect();
  if (he != hipSuccess) return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
  const int* r = L.cm.res_h();
  if (r[kCrErr]) {
    const int at = r[kCrErr] == kCrErrVin ? kCrVin : kCrMap;
    out->map_points[0] = (uint64_t)r[at];
    out->map_points[1] = (uint64_t)r[at + 1];
    return fail(LOAM_E_CAPACITY, who + (r[kCrErr] == kCrErrVin ? ": the VoxelGrid input of the union's cubes exceeds map_capacity"
                                                                 : ": the map after the commit exceeds map_capacity"));
  }
  s.pool_cur = 1 - s.pool_cur;
  // (statistics only, as loam_map_import: no frame of the context built this store)
  *(int*)(x->xb.h + kXferMpUpd + 4 * (1 - s.pool_cur)) = 0;
  x->surround_due = false;
  for (uint32_t i = 0; i < n; ++i) L.committed[lane[i]] = 1;
  for (int k = 0; k < 2; ++k) {
    out->inserted[k] = (uint64_t)r[kCrIns + k];
    out->outside[k] = (uint64_t)r[kCrOut + k];
    out->map_points[k] = (uint64_t)r[kCrMap + k];
  }
  out->cubes = (uint32_t)r[kCrCubes];
  return LOAM_OK;
}

// the hook of dev_hooks.h: a lane's stack in the map frame and its valid set, as the commit reads them
extern "C" int loam_dev_lanes_commit_input(loam_ctx* x, uint32_t lane, float* corner_out, float* surf_out,
                                           uint32_t* n_out, int32_t* valid_out, uint32_t* n_valid) {
  if (!x || !corner_out || !surf_out || !n_out || !valid_out || !n_valid) return fail(LOAM_E_INVAL, "null argument");
  const std::string who = "loam_dev_lanes_commit_input";
  if (const int rc = lanes_commit_refused(who, x, &lane, 1)) return rc;
  Lanes& L = x->lanes;
  const MpBuffers& w = L.mp;
  if (const int rc = map_drain(x)) return rc;
  float4 *dC = nullptr, *dS = nullptr;
  hipError_t he = hipMalloc((void**)&dC, (size_t)w.capC * sizeof(float4));
  if (he == hipSuccess) he = hipMalloc((void**)&dS, (size_t)w.capS * sizeof(float4));
  int cnt[2] = {0, 0}, nv = 0;
  if (he == hipSuccess) he = mp_lanes_commit_input(w, (int)lane, dC, dS, x->st);
  if (he == hipSuccess) he = hipStreamSynchronize(x->st);
  if (he == hipSuccess) he = hipMemcpy(cnt, w.sseg_cnt + (size_t)lane * 2, sizeof(cnt), hipMemcpyDeviceToHost);
  if (he == hipSuccess)
    he = hipMemcpy(&nv, w.istate + (size_t)lane * kMpStateInts + kMiNValid, sizeof(int), hipMemcpyDeviceToHost);
  cnt[0] = std::min(std::max(cnt[0], 0), w.capC);
  cnt[1] = std::min(std::max(cnt[1], 0), w.capS);
  nv = std::min(std::max(nv, 0), kMaxValid);
  if (he == hipSuccess && cnt[0]) he = hipMemcpy(corner_out, dC, (size_t)cnt[0] * sizeof(float4), hipMemcpyDeviceToHost);
  if (he == hipSuccess && cnt[1]) he = hipMemcpy(surf_out, dS, (size_t)cnt[1] * sizeof(float4), hipMemcpyDeviceToHost);
  if (he == hipSuccess && nv)
    he = hipMemcpy(valid_out, w.valid + (size_t)lane * kMaxValid, (size_t)nv * sizeof(int), hipMemcpyDeviceToHost);
  if (dC) (void)hipFree(dC);
  if (dS) (void)hipFree(dS);
  if (he != hipSuccess) {
    (void)hipGetLastError();
    return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
  }
  n_out[0] = (uint32_t)cnt[0];
  n_out[1] = (uint32_t)cnt[1];
  *n_valid = (uint32_t)nv;
  return LOAM_OK;
}

// k pose guesses for each of n listed lanes against the whole streaming map (score.hpp, DESIGN.md
// §31): loam_map_score's sequence with the lanes' Last clouds read in place.  The lanes' nlast
// words come down with the map's sizes; the host then knows every listed lane's tiles.
extern "C" int loam_lanes_score(loam_ctx* x, uint32_t n, const uint32_t* lane, float max_dist, uint32_t k,
                                const loam_pose6* pose, loam_score_result* out) {
  if (!x || !lane || !pose || !out) return fail(LOAM_E_INVAL, "null argument");
  const std::string who = "loam_lanes_score";
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused(who, L, kLanesOpen | kLanesIdle)) return rc;
  if (!L.pulled || !L.od_inited)
    return fail(LOAM_E_INVAL, who + ": no step was pulled on which the odometry was initialised (no Last clouds yet)");
  if (n == 0 || n > (uint32_t)L.S) return fail(LOAM_E_INVAL, who + ": n must be in [1, n_lanes]");
  if (k == 0) return fail(LOAM_E_INVAL, who + ": k must be at least 1");
  if ((uint64_t)n * (uint64_t)k > (uint64_t)LOAM_SCORE_MAX)
    return fail(LOAM_E_INVAL, who + ": n x k must not exceed LOAM_SCORE_MAX");
  if (const int rc = score_max_dist_refused(who, max_dist)) return rc;
  if (const int rc = lanes_list_refused(who, L, lane, n)) return rc;
  int rc = map_drain(x);
  if (rc) return rc;
  MpBuffers& b = x->mp1;
  MpScore& S = x->score;
  const OdBuffers& o = L.od;
  hipError_t he = mp_map_ensure(x->mio);
  if (he == hipSuccess) he = mp_score_reserve(S, 0);
  if (he == hipSuccess) he = mp_score_reserve_plan(S, L.S);
  if (he != hipSuccess) return nomem(who + ": working set allocation failed: " + hipGetErrorString(he));
  hipStream_t st = x->st;
  const size_t rows = (size_t)n * k;
  std::memcpy(S.pose_h(), pose, rows * sizeof(loam_pose6));
  x->prof.begin(st);
  he = mp_map_table(b, x->mio, st, &x->prof);
  if (he == hipSuccess) he = hipMemcpyAsync(S.pose, S.pose_h(), rows * sizeof(loam_pose6), hipMemcpyHostToDevice, st);
  x->prof.mark("lanes_score_h2d");
  if (he == hipSuccess)
    he = hipMemcpyAsync(S.nlast_h(), o.nlast, (size_t)L.S * kOdBufs * 2 * sizeof(int), hipMemcpyDeviceToHost, st);
  x->prof.mark("lanes_score_d2h");
  if ((rc = sync_or_fail(x, he, who))) return rc;
  int nC = 0, total = 0;
  if ((rc = score_map_sizes(x, who, &nC, &total))) return rc;
  std::vector<int32_t> cnt((size_t)2 * n);
  for (uint32_t i = 0; i < n; ++i) {
    const int* w = S.nlast_h() + ((size_t)lane[i] * kOdBufs + L.od_last) * 2;
    cnt[2 * i] = w[0];
    cnt[2 * i + 1] = w[1];
  }
  LaneScoreShape shape;
  const int plan = lanes_score_plan(n, k, lane, cnt.data(), (uint32_t)L.S, (uint32_t)L.od_last, o.capC, o.capS,
                                    S.plan_h(), &shape);
  if (plan != kLanePlanOk) {
    x->prof.collect();
    return fail(LOAM_E_HIP, who + ": a lane's Last cloud sizes are not valid (plan code " + std::to_string(plan) + ")");
  }
  if ((rc = score_reserve_index(x, who, nC, total, 0, 0, (int)rows))) return rc;
  const bool count = x->prof.on;  // (with profiling the kernel also adds up the points and buckets the searches read)
  he = mp_lanes_score_run(S, b, x->mio, nC, total, o.lastC, o.lastS, shape, (int)n, (int)k, max_dist * max_dist, count,
                          st, &x->prof);
  if ((rc = sync_or_fail(x, he, who))) return rc;
  x->prof.collect();
  if (count) {
    double queries = 0.0;
    for (size_t r = 0; r < rows; ++r) queries += (double)S.res_h()[r].corner_scored + (double)S.res_h()[r].surf_scored;
    score_count_work(x, queries);
  }
  std::memcpy(out, S.res_h(), rows * sizeof(loam_score_result));
  return LOAM_OK;
}

// k candidate poses for each of n listed lanes refined for the lane's own last sweep:
// loam_map_localize's sequence with every row's clouds and transformSum read in place from the row's
// lane.  Three synchronisations: the lanes' nlast words (they size the rows' stacks), the rows'
// FromMap counts (they size the FromMap part), the results.
extern "C" int loam_lanes_localize(loam_ctx* x, uint32_t n, const uint32_t* lane, uint32_t k, const loam_pose6* aft,
                                   const loam_pose6* bef, loam_localize_result* out) {
  static_assert(kLocPlanRows == (uint32_t)kLocMax && kLocPlanBufs == (uint32_t)kOdBufs, "loc_plan.hpp and mp.hpp / od.hpp");
  static_assert(LOAM_LANES_MAX <= kLocMax, "MpLoc's plan block holds every lane's nlast words");
  if (!x || !lane || !aft || !out) return fail(LOAM_E_INVAL, "null argument");
  const std::string who = "loam_lanes_localize";
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused(who, L, kLanesOpen | kLanesIdle)) return rc;
  if (!L.pulled || !L.od_inited)
    return fail(LOAM_E_INVAL, who + ": no step was pulled on which the odometry was initialised (no Last clouds yet)");
  if (n == 0 || n > (uint32_t)L.S) return fail(LOAM_E_INVAL, who + ": n must be in [1, n_lanes]");
  if (k == 0) return fail(LOAM_E_INVAL, who + ": k must be at least 1");
  if ((uint64_t)n * (uint64_t)k > (uint64_t)LOAM_LOCALIZE_MAX)
    return fail(LOAM_E_INVAL, who + ": n x k must not exceed LOAM_LOCALIZE_MAX");
  if (const int rc = lanes_list_refused(who, L, lane, n)) return rc;
  int rc = map_drain(x);
  if (rc) return rc;
  const MpBuffers& s = x->mp1;
  MpLoc& Lc = x->loc;
  const OdBuffers& o = L.od;
  hipStream_t st = x->st;
  hipError_t he = mp_loc_reserve_rows(Lc);
  if (he != hipSuccess) return nomem(who + ": working set allocation failed: " + hipGetErrorString(he));
  x->prof.begin(st);
  he = hipMemcpyAsync(Lc.nlast_h(), o.nlast, (size_t)L.S * kOdBufs * 2 * sizeof(int), hipMemcpyDeviceToHost, st);
  x->prof.mark("lanes_localize_d2h");
  if ((rc = sync_or_fail(x, he, who))) return rc;
  std::vector<int32_t> cnt((size_t)2 * n);
  for (uint32_t i = 0; i < n; ++i) {
    const int* w = Lc.nlast_h() + ((size_t)lane[i] * kOdBufs + L.od_last) * 2;
    cnt[2 * i] = w[0];
    cnt[2 * i + 1] = w[1];
  }
  LaneLocShape shape;
  const int plan = lanes_localize_plan(n, k, lane, cnt.data(), (uint32_t)L.S, (uint32_t)L.od_last, o.capC, o.capS, s.capC,
                                       Lc.plan_h(), &shape);
  if (plan != kLocPlanOk) {
    x->prof.collect();
    if (plan == kLocPlanStack)
      return fail(LOAM_E_INVAL, who + ": a listed lane's corner cloud exceeds the mapping stack (120 points per ring)");
    return fail(LOAM_E_HIP, who + ": a lane's Last cloud sizes are not valid (plan code " + std::to_string(plan) + ")");
  }
  const int rows = (int)shape.rows;
  he = mp_loc_reserve(Lc, s, rows, shape.maxC, shape.maxS);
  if (he != hipSuccess) {
    x->prof.collect();
    return nomem(who + ": working set allocation failed: " + hipGetErrorString(he));
  }
  Prof* pf = x->prof.on ? &x->prof : nullptr;  // (with profiling the L-M kernels also count their work)
  cand_rows(Lc.cand_h(), (size_t)rows, aft, bef);
  LocRows lr;
  lr.plan = Lc.plan;
  lr.k = (int)k;
  lr.lastC = o.lastC;
  lr.lastS = o.lastS;
  lr.od_state = o.state;
  const MpInput none = {};  // (the rows kernels read the lanes' clouds through the plan)
  he = mp_localize_prepare(Lc, s, none, rows, st, pf, &lr);
  if ((rc = sync_or_fail(x, he, who))) return rc;
  return localize_finish(x, who, none, rows, std::max(shape.maxC, shape.maxS), &lr, "lanes_localize_d2h", out);
}

extern "C" int loam_lanes_close(loam_ctx* x) {
  if (!x) return fail(LOAM_E_INVAL, "null argument");
  if (const int rc = lanes_state_refused("loam_lanes_close", x->lanes, kLanesOpen)) return rc;
  HIP_TRY(hipSetDevice(x->device));
  (void)hipStreamSynchronize(x->st);
  (void)x->lanes.mp.take_error();
  lanes_free(x->lanes);
  return LOAM_OK;
}

namespace {
// Every push: what is refused before anything is enqueued, counted or changed.  Lane l's sweep stamp
// is stamps ? stamps[l] : stamp.
int lanes_push_check(loam_ctx* x, const double* stamps, double stamp, const std::string& who) {
  const Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused(who, L, kLanesOpen | kLanesIdle)) return rc;
  for (int l = 0; l < L.S; ++l)
    if (!std::isfinite(stamps ? stamps[l] : stamp)) return fail(LOAM_E_INVAL, who + ": a sweep stamp is not finite");
  return LOAM_OK;
}

// Every push, behind its checks: drops what the last step left; false inside system_delay, where the
// step is counted and nothing is enqueued
bool lanes_push_begin(loam_ctx* x) {
  Lanes& L = x->lanes;
  L.imu.step_imu = false;
  L.have_reg = false;
  for (int l = 0; l < L.S; ++l) L.life[l].due = kDueNo;  // (the last step's /laser_cloud_surround)
  if (L.sr_inited) return true;
  // src/scanRegistration.cpp:213-219 (Q1): the sweeps are not looked at
  L.sr_init_count++;
  if (L.sr_init_count >= (int)x->cfg.system_delay) L.sr_inited = true;
  L.in_flight = true;
  L.step_ran = false;
  return false;
}

// the lanes' kinds on this step and loam_lanes_restart's lists of it
// a restarted lane: an empty problem until its init frame, and raw[l] is not looked at
void lanes_push_kinds(Lanes& L, int& n_clear, int& n_init) {
  const int S = L.S;
  n_clear = n_init = 0;
  for (int l = 0; l < S; ++l) {
    LaneLife& f = L.life[l];
    f.kind = kLaneRuns;
    if (f.wait < 0) continue;
    f.kind = f.wait == 0 ? kLaneInits : kLaneWaits;
    L.rs_h[n_clear++] = l;
    if (f.kind == kLaneInits) L.rs_h[S + n_init++] = l;
  }
}

// opens the step's timeline; the restarted lanes as lanes_alloc left them, in front of everything
// the step does
int lanes_push_clear(loam_ctx* x, int n_clear) {
  Lanes& L = x->lanes;
  hipStream_t st = x->st;
  x->prof.begin(st);
  if (n_clear) {
    HIP_TRY(hipMemcpyAsync(L.rs_d, L.rs_h, (size_t)2 * L.S * sizeof(int), hipMemcpyHostToDevice, st));
    x->prof.mark("lanes_h2d");
    HIP_TRY(lanes_restart_clear(L, L.rs_d, n_clear, kClearOd | kClearMp | (L.imu.on ? kClearImu : 0), st));
    x->prof.mark("k_lanes_restart");
  }
  return LOAM_OK;
}

// Every push, behind the sweeps in sr.raw / sr.raw_n: the step's IMU block, its kernels and the
// life counters
int lanes_push_finish(loam_ctx* x, const double* stamps, double stamp, int n_clear, int n_init, const std::string& who) {
  Lanes& L = x->lanes;
  LanesImu& I = L.imu;
  const int S = L.S;
  hipStream_t st = x->st;
  Prof* pf = x->prof.on ? &x->prof : nullptr;
  // IMU: any live lane with a message makes this an IMU step for all lanes
  bool imu = false;
  if (I.on) {
    auto live = [&](int l) {
      return L.fail[l] == LOAM_OK && L.fail_new[l] == LOAM_OK && L.life[l].kind != kLaneWaits;
    };
    for (int l = 0; l < S && !imu; ++l) imu = live(l) && I.sr[l].last >= 0;
    if (imu) {
      const bool will_map = lanes_will_map(x);
      loamimu::LaneHdr* hdr = (loamimu::LaneHdr*)I.up_h;
      loamimu::LaneRec* rec = (loamimu::LaneRec*)(I.up_h + (size_t)S * sizeof(loamimu::LaneHdr));
      int nrec = 0;
      for (int l = 0; l < S; ++l) {
        const loamimu::SrQueue& q = I.sr[l];
        loamimu::LaneHdr& h = hdr[l];
        std::memset(&h, 0, sizeof(h));
        h.time_scan = stamps ? stamps[l] : stamp;
        h.last = q.last;
        h.has = live(l) && q.last >= 0 ? 1 : 0;
        I.mp_have[l] = 0;
        if (!h.has) continue;
        // transformUpdate's blend (src/laserMapping.cpp:199-226) at this lane's stamp, from its
        // committed pointer; the pull commits the advanced one when the lane's L-M ran
        // (not on the lane's own init frame, which does not map)
        if (will_map && L.life[l].kind == kLaneRuns &&
            loamimu::mp_lookup(I.mp[l], h.time_scan, h.roll, h.pitch, I.mp_front[l])) {
          h.mp_flag = 1;
          I.mp_have[l] = 1;
        }
        // the entries pushed since the last step (the ring holds the last kQue of them)
        nrec += loamimu::lane_records(q, I.n_new[l], l, rec + nrec);
        I.n_new[l] = 0;
      }
      I.up_bytes = (size_t)S * sizeof(loamimu::LaneHdr) + (size_t)nrec * sizeof(loamimu::LaneRec);
      HIP_TRY(lanes_imu_put(L, I.up_bytes, nrec, st));
    }
  }
  x->prof.mark("lanes_h2d");
  const hipError_t he = lanes_enqueue(x, pf, imu, n_init);
  for (int l = 0; l < n_clear; ++l) L.life[L.rs_h[l]].wait--;  // (an init frame ends the restart: -1)
  L.in_flight = true;
  L.step_ran = true;
  I.step_imu = imu;
  if (he != hipSuccess) return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
  return LOAM_OK;
}

// loam_lanes_push / loam_lanes_push_stamped
int lanes_push(loam_ctx* x, const double* stamps, double stamp, const loam_cloud_in* raw) {
  const std::string who = "loam_lanes_push";
  Lanes& L = x->lanes;
  if (const int rc = lanes_push_check(x, stamps, stamp, who)) return rc;
  const int S = L.S;
  if (!lanes_push_begin(x)) return LOAM_OK;
  HIP_TRY(hipSetDevice(x->device));
  // a lane whose sweep cannot be uploaded, and a lane that failed before, is an empty sweep on the
  // device: its slot goes through the kernels as an empty problem of a batch does
  int n_clear = 0, n_init = 0;
  lanes_push_kinds(L, n_clear, n_init);
  std::vector<loam_cloud_in> eff((size_t)S);
  int* nn = L.tab_h;
  int* off = nn + S;
  size_t run = 0;
  for (int l = 0; l < S; ++l) {
    const bool waits = L.life[l].kind == kLaneWaits;
    L.fail_new[l] = waits ? LOAM_OK : lane_sweep_code(raw[l], x->cap, x->pf.on ? x->pf.end : 0);
    eff[l] = raw[l];
    if (waits || L.fail_new[l] != LOAM_OK || L.fail[l] != LOAM_OK) eff[l].count = 0;
    nn[l] = (int)eff[l].count;
    off[l] = (int)run;
    run += eff[l].count;
  }
  hipStream_t st = x->st;
  if (const int rc = lanes_push_clear(x, n_clear)) return rc;
  // packed in chunks of sweeps, each chunk's copy enqueued before the next is packed
  constexpr int kPushChunk = 128;  // sweeps
  for (int s0 = 0; s0 < S; s0 += kPushChunk) {
    const int s1 = std::min(S, s0 + kPushChunk);
    pack_tight_of([&](size_t s) -> const loam_cloud_in& { return eff[s]; }, (size_t)s0, (size_t)s1, off, L.stage_h, x->pf);
    const size_t a = (size_t)off[s0], b = (size_t)off[s1 - 1] + (size_t)nn[s1 - 1];
    if (b > a)
      HIP_TRY(hipMemcpyAsync(L.stage_d + a, L.stage_h + a, (b - a) * sizeof(float4), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipMemcpyAsync(L.tab_d, nn, (size_t)2 * S * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(sr_scatter_packed(L.stage_d, L.tab_d + S, L.tab_d, L.sr.raw, x->cap, S, st));
  HIP_TRY(hipMemcpyAsync(L.sr.raw_n, L.tab_d, (size_t)S * sizeof(int), hipMemcpyDeviceToDevice, st));
  return lanes_push_finish(x, stamps, stamp, n_clear, n_init, who);
}

// what HIP knows of a caller's pointer: the allocation around it, and whether that is plain device
// memory of `device` (pinned, registered, managed and peer memory are not)
void lanes_feed_lookup(const void* p, int device, LaneFeedIn& q) {
  q.on_device = 0;
  q.base = 0;
  q.size = 0;
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof(at));
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice || at.isManaged ||
      at.device != device || hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
    (void)hipGetLastError();  // (a pointer HIP does not know is an error of the query, not of the context)
    return;
  }
  q.on_device = 1;
  q.base = (uintptr_t)base;
  q.size = (uint64_t)size;
}

// raw[0..S) and the lanes' states into the plan's input, with HIP's answer for every pointer the
// step would read.  A pointer inside the allocation found for the previous lane of this call takes
// that answer; nothing is kept between calls (the memory may have been freed).
void lanes_feed_inputs(const loam_cloud_in* raw, int S, int cap, int device, const int* state, std::vector<LaneFeedIn>& in,
                       uint32_t fields_end = 0) {
  in.resize((size_t)S);
  const LaneFeedIn* prev = nullptr;
  for (int l = 0; l < S; ++l) {
    LaneFeedIn& q = in[l];
    std::memset(&q, 0, sizeof(q));
    q.state = state[l];
    if (q.state != kFeedRuns) continue;  // (raw[l] is not looked at)
    q.ptr = (uintptr_t)raw[l].data;
    q.count = raw[l].count;
    q.stride = raw[l].stride_bytes;
    if (!lanes_feed_looks(q, cap, fields_end)) continue;
    if (prev && q.ptr >= prev->base && (uint64_t)(q.ptr - prev->base) < prev->size) {
      q.on_device = 1;
      q.base = prev->base;
      q.size = prev->size;
    } else {
      lanes_feed_lookup(raw[l].data, device, q);
    }
    if (q.on_device) prev = &q;
  }
}
}  // namespace

extern "C" int loam_lanes_push(loam_ctx* x, double stamp, const loam_cloud_in* raw) {
  if (!x || !raw) return fail(LOAM_E_INVAL, "null argument");
  return lanes_push(x, nullptr, stamp, raw);
}

extern "C" int loam_lanes_push_stamped(loam_ctx* x, const double* stamp, const loam_cloud_in* raw) {
  if (!x || !stamp || !raw) return fail(LOAM_E_INVAL, "null argument");
  return lanes_push(x, stamp, 0.0, raw);
}

extern "C" int loam_lanes_push_device(loam_ctx* x, const double* stamp, const loam_cloud_in* raw, void* producer_stream,
                                      uint32_t flags) {
  static_assert(kFeedLaneOk == LOAM_OK && kFeedLaneInval == LOAM_E_INVAL && kFeedLaneCapacity == LOAM_E_CAPACITY,
                "lanes_feed_plan.hpp");
  const std::string who = "loam_lanes_push_device";
  if (!x || !stamp || !raw) return fail(LOAM_E_INVAL, "null argument");
  if (flags & ~(uint32_t)(LOAM_FEED_WAIT | LOAM_FEED_RELEASE)) return fail(LOAM_E_INVAL, who + ": unknown flag bits");
  Lanes& L = x->lanes;
  if (const int rc = lanes_push_check(x, stamp, 0.0, who)) return rc;
  const int S = L.S;
  HIP_TRY(hipSetDevice(x->device));
  if (lanes_feed_alloc(L) != hipSuccess) return nomem(who + ": the descriptor block's allocation failed");
  hipStream_t prod = (hipStream_t)producer_stream;
  bool feeds = false;
  if (L.sr_inited) {  // (inside system_delay the sweeps are not looked at)
    std::vector<int> state((size_t)S);
    for (int l = 0; l < S; ++l) state[l] = L.fail[l] != LOAM_OK ? kFeedFailed : L.life[l].wait > 0 ? kFeedWaits : kFeedRuns;
    std::vector<LaneFeedIn> in;
    const uint32_t fields_end = x->pf.on ? x->pf.end : 0;
    lanes_feed_inputs(raw, S, x->cap, x->device, state.data(), in, fields_end);
    // (the last step was pulled: its copy of the descriptor block is done; the lanes' codes go into
    // fail_new only when nothing can refuse the call any more)
    std::vector<int32_t> code((size_t)S);
    uint32_t bad = 0;
    const int verdict = lanes_feed_plan(in.data(), (uint32_t)S, x->cap, L.fd_h, code.data(), &bad, fields_end);
    if (verdict != kFeedOk) {
      char msg[128];
      lanes_feed_message(verdict, bad, msg, sizeof(msg));
      return fail(LOAM_E_INVAL, who + ": " + msg);
    }
    for (int l = 0; l < S && !feeds; ++l) feeds = L.fd_h[l].n > 0;
    if (feeds && (flags & LOAM_FEED_WAIT) && !L.feed_wait) HIP_TRY(hipEventCreateWithFlags(&L.feed_wait, hipEventDisableTiming));
    if (feeds && (flags & LOAM_FEED_RELEASE) && !L.feed_release)
      HIP_TRY(hipEventCreateWithFlags(&L.feed_release, hipEventDisableTiming));
    std::copy(code.begin(), code.end(), L.fail_new.begin());
  }
  if (!lanes_push_begin(x)) return LOAM_OK;
  int n_clear = 0, n_init = 0;
  lanes_push_kinds(L, n_clear, n_init);
  hipStream_t st = x->st;
  if (const int rc = lanes_push_clear(x, n_clear)) return rc;
  if (feeds && (flags & LOAM_FEED_WAIT)) {  // the gather behind the work enqueued so far on the producer's stream
    HIP_TRY(hipEventRecord(L.feed_wait, prod));
    HIP_TRY(hipStreamWaitEvent(st, L.feed_wait, 0));
  }
  HIP_TRY(lanes_gather_dev(L, x->cap, st, x->pf.on ? &x->pf : nullptr, x->pf_map_d));
  x->prof.mark("k_lanes_gather_dev");
  if (feeds && (flags & LOAM_FEED_RELEASE)) {  // the producer's later work behind the gather
    HIP_TRY(hipEventRecord(L.feed_release, st));
    HIP_TRY(hipStreamWaitEvent(prod, L.feed_release, 0));
  }
  return lanes_push_finish(x, stamp, 0.0, n_clear, n_init, who);
}

// dev_hooks.h: the device feed's validation and gather on caller-supplied device sweeps
extern "C" int loam_dev_lanes_gather(int device, int32_t S, int32_t cap, const void* raw_in, uint32_t* out_raw,
                                     int32_t* out_n) {
  const loam_cloud_in* raw = (const loam_cloud_in*)raw_in;
  if (!raw || !out_raw || !out_n || S < 1 || S > LOAM_LANES_MAX || cap < 1 || cap > LOAM_DEV_LANES_GATHER_MAX_CAP)
    return fail(LOAM_E_INVAL, "loam_dev_lanes_gather: bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LOAM_E_HIP, "no HIP device");  // (no CPU path)
  if (device < 0 || device >= ndev) return fail(LOAM_E_INVAL, "loam_dev_lanes_gather: no such device");
  HIP_TRY(hipSetDevice(device));
  const std::vector<int> state((size_t)S, kFeedRuns);
  std::vector<LaneFeedIn> in;
  lanes_feed_inputs(raw, S, cap, device, state.data(), in);
  std::vector<LaneFeedDesc> desc((size_t)S);
  std::vector<int32_t> code((size_t)S);
  uint32_t bad = 0;
  const int verdict = lanes_feed_plan(in.data(), (uint32_t)S, cap, desc.data(), code.data(), &bad);
  if (verdict != kFeedOk) {
    char msg[128];
    lanes_feed_message(verdict, bad, msg, sizeof(msg));
    return fail(LOAM_E_INVAL, std::string("loam_dev_lanes_gather: ") + msg);
  }
  const size_t words = (size_t)S * cap * 4;
  LaneFeedDesc* desc_d = nullptr;
  float4* raw_d = nullptr;
  int* n_d = nullptr;
  hipError_t e = hipMalloc((void**)&desc_d, (size_t)S * sizeof(LaneFeedDesc));
  if (e == hipSuccess) e = hipMalloc((void**)&raw_d, words * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMalloc((void**)&n_d, (size_t)S * sizeof(int));
  const bool nomem = e != hipSuccess;
  if (e == hipSuccess) e = hipMemcpy(desc_d, desc.data(), (size_t)S * sizeof(LaneFeedDesc), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemsetD32((hipDeviceptr_t)raw_d, (int)LOAM_DEV_VG_SENTINEL, words);
  if (e == hipSuccess) e = hipMemsetD32((hipDeviceptr_t)n_d, -1, (size_t)S);
  if (e == hipSuccess) e = lanes_gather_launch(desc_d, raw_d, n_d, cap, S, nullptr);
  if (e == hipSuccess) e = hipMemcpy(out_raw, raw_d, words * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out_n, n_d, (size_t)S * sizeof(int), hipMemcpyDeviceToHost);
  if (desc_d) (void)hipFree(desc_d);
  if (raw_d) (void)hipFree(raw_d);
  if (n_d) (void)hipFree(n_d);
  if (e == hipSuccess) return LOAM_OK;
  (void)hipGetLastError();
  return nomem ? fail(LOAM_E_NOMEM, "loam_dev_lanes_gather: allocation failed")
               : fail(LOAM_E_HIP, std::string("loam_dev_lanes_gather: ") + hipGetErrorString(e));
}

extern "C" int loam_lanes_imu(loam_ctx* x, uint32_t lane, double stamp, const double* quat_xyzw,
                              const double* lin_acc_xyz) {
  if (!x || !quat_xyzw || !lin_acc_xyz) return fail(LOAM_E_INVAL, "null argument");
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused("loam_lanes_imu", L, kLanesOpen)) return rc;
  if (lane >= (uint32_t)L.S) return fail(LOAM_E_INVAL, "loam_lanes_imu: lane index out of range");
  // (the queues a push copied and the pointers a pull commits do not change in between)
  if (const int rc = lanes_state_refused("loam_lanes_imu", L, kLanesIdle)) return rc;
  if (L.fail[lane] != LOAM_OK) return fail(LOAM_E_INVAL, "loam_lanes_imu: the lane has failed");
  LanesImu& I = L.imu;
  if (!(stamp >= (I.on ? I.last_stamp[lane] : -1e300)))
    return fail(LOAM_E_INVAL, "loam_lanes_imu: IMU stamps of a lane must be non-decreasing");
  if (!I.on) {  // the first message of any lane: the queues, host and device
    HIP_TRY(hipSetDevice(x->device));
    const hipError_t he = lanes_imu_alloc(L);
    if (he != hipSuccess) return nomem(std::string("loam_lanes_imu: allocation failed: ") + hipGetErrorString(he));
  }
  I.last_stamp[lane] = stamp;
  double roll, pitch, yaw;
  loampose::rpy_from_quat(quat_xyzw, roll, pitch, yaw);  // tf::Matrix3x3(q).getRPY
  loamimu::sr_push(I.sr[lane], stamp, roll, pitch, yaw, lin_acc_xyz);  // scanRegistration.cpp:638-660
  loamimu::mp_push(I.mp[lane], stamp, roll, pitch);                     // laserMapping.cpp:323-335
  I.n_new[lane]++;
  return LOAM_OK;
}

extern "C" int loam_lanes_restart(loam_ctx* x, uint32_t lane, uint32_t* wait_steps) {
  if (!x || !wait_steps) return fail(LOAM_E_INVAL, "null argument");
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused("loam_lanes_restart", L, kLanesOpen)) return rc;
  if (lane >= (uint32_t)L.S) return fail(LOAM_E_INVAL, "loam_lanes_restart: lane index out of range");
  if (const int rc = lanes_state_refused("loam_lanes_restart", L, kLanesIdle)) return rc;
  const int s = (int)x->cfg.skip_frame_num;
  LaneLife& f = L.life[lane];
  if (L.od_inited) {
    if (!L.rs_h) {  // the first restart: the steps' lane lists
      HIP_TRY(hipSetDevice(x->device));
      const hipError_t he = lanes_restart_alloc(L);
      if (he != hipSuccess) return nomem(std::string("loam_lanes_restart: allocation failed: ") + hipGetErrorString(he));
    }
    // The lane's init frame is the step before a mapping step of the shared phase (a fresh context
    // maps on the frame after its init frame: od_frame_count = s, and the init frame does not
    // count).  Step j from here maps when od_frame_count + j reaches s + 1 (mod s + 1), so the init
    // frame is step j = s - od_frame_count (mod s + 1), in 1..s+1, and j - 1 steps are waited.
    f.wait = (2 * s - L.od_frame_count) % (s + 1);
    *wait_steps = (uint32_t)f.wait;
  } else {
    // before the shared init frame nothing of the lane is on the device yet: it takes that frame
    // with the others, after what is left of system_delay (Q1: one step at least)
    *wait_steps = L.sr_inited ? 0u : (uint32_t)std::max(1, (int)x->cfg.system_delay - L.sr_init_count);
    if (L.mi_h) {  // ... but for a map a loam_lanes_map_import may have put there: cleared here and now
      HIP_TRY(hipSetDevice(x->device));
      L.mi_h[kMiList] = (int)lane;
      HIP_TRY(hipMemcpyAsync(L.mi_d + kMiList, L.mi_h + kMiList, sizeof(int), hipMemcpyHostToDevice, x->st));
      HIP_TRY(lanes_restart_clear(L, L.mi_d + kMiList, 1, kClearMp, x->st));
      HIP_TRY(hipStreamSynchronize(x->st));
    }
    if (L.sp_h) {  // ... and for the poses a loam_lanes_set_pose may have put there (shared lanes)
      HIP_TRY(hipSetDevice(x->device));
      L.sp_h[0] = (int)lane;
      HIP_TRY(hipMemcpyAsync(L.sp_d, L.sp_h, sizeof(int), hipMemcpyHostToDevice, x->st));
      HIP_TRY(lanes_restart_clear(L, L.sp_d, 1, kClearMp, x->st));
      HIP_TRY(hipStreamSynchronize(x->st));
    }
  }
  f.phase = 4;  // mapFrameCount = mapFrameNum - 1 (src/laserMapping.cpp:405)
  f.due = kDueNo;
  L.fail[lane] = LOAM_OK;
  L.fail_new[lane] = LOAM_OK;
  L.nreg[lane] = 0;
  LanesImu& I = L.imu;
  if (I.on) {  // the lane's queues as lanes_imu_alloc left them (the device's: k_lanes_restart)
    std::memset(&I.sr[lane], 0, sizeof(I.sr[lane]));
    std::memset(&I.mp[lane], 0, sizeof(I.mp[lane]));
    I.sr[lane].last = I.mp[lane].last = -1;
    I.last_stamp[lane] = -1e300;
    I.n_new[lane] = 0;
    I.mp_front[lane] = 0;
    I.mp_have[lane] = 0;
  }
  return LOAM_OK;
}

extern "C" int loam_lanes_imu_trans(loam_ctx* x, float* out) {
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused("loam_lanes_imu_trans", L, kLanesOpen | kLanesIdle | kLanesPulled)) return rc;
  std::memcpy(out, L.imu_trans.data(), (size_t)L.S * 12 * sizeof(float));
  return LOAM_OK;
}

extern "C" int loam_lanes_pull(loam_ctx* x, loam_lane_out* out) {
  static_assert(sizeof(loam_lane_out) == 96, "loam_lane_out layout");
  static_assert(LOAM_LANES_MAX == 1024, "loam.h");
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused("loam_lanes_pull", L, kLanesOpen)) return rc;
  if (!L.in_flight) return fail(LOAM_E_INVAL, "loam_lanes_pull: no step was pushed");
  const int S = L.S;
  L.imu_trans.assign((size_t)S * 12, 0.0f);
  if (L.shared) {  // (LOAM_LOC_NONE with zeros until a lane's mapping frame is found below)
    loam_localize_result none;
    std::memset(&none, 0, sizeof(none));
    none.status = LOAM_LOC_NONE;
    L.loc_info.assign((size_t)S, none);
    L.committed.assign((size_t)S, 0);  // (loam_lanes_map_commit: the frames of this pull are new)
  }
  if (!L.step_ran) {  // inside system_delay: nothing was enqueued
    L.in_flight = false;
    L.pulled = true;
    std::memset(out, 0, (size_t)S * sizeof(loam_lane_out));
    for (int l = 0; l < S; ++l) out[l].status = LOAM_E_NOT_READY;
    return LOAM_OK;
  }
  HIP_TRY(hipSetDevice(x->device));
  hipError_t he = hipStreamSynchronize(x->st);
  L.in_flight = false;
  if (he == hipSuccess) he = L.mp.take_error();
  x->prof.collect();
  if (he != hipSuccess) return fail(LOAM_E_HIP, std::string("loam_lanes_pull: ") + hipGetErrorString(he));
  std::memset(out, 0, (size_t)S * sizeof(loam_lane_out));
  for (int l = 0; l < S; ++l) {
    const int* w = L.out_h + (size_t)l * kLaneOutWords;
    loam_lane_out& q = out[l];
    const int kind = L.life[l].kind;
    if (kind == kLaneWaits) {  // restarted, before its init frame: its sweep was not looked at
      L.nreg[l] = 0;
      q.status = LOAM_E_NOT_READY;
      continue;
    }
    const bool mapped = L.step_mapped && kind == kLaneRuns;
    if (L.fail[l] == LOAM_OK) {  // this step's failure, the host's finding first
      int code = L.fail_new[l];
      if (code == LOAM_OK && (w[kLoSrErr] & ERR_EMPTY)) code = LOAM_E_INVAL;
      if (code == LOAM_OK && (w[kLoSrErr] & ERR_CAP_RING)) code = LOAM_E_CAPACITY;
      if (code == LOAM_OK && w[kLoOdErr]) code = LOAM_E_CAPACITY;
      if (code == LOAM_OK && mapped && w[kLoMpErr]) code = LOAM_E_CAPACITY;
      L.fail[l] = code;
    }
    L.nreg[l] = 0;
    if (L.fail[l] != LOAM_OK) {
      q.status = L.fail[l];
      continue;
    }
    q.status = LOAM_OK;
    q.published = kind == kLaneInits ? LOAM_PUB_CLOUDS : L.step_pub;
    q.mapped = mapped ? 1 : 0;
    if (q.published & LOAM_PUB_POSE) {
      q.od_iters = w[kLoOdIters];
      std::memcpy(&q.od_sum, w + kLoOdSum, sizeof(loam_pose6));
    }
    if (mapped) {
      q.mp_iters = w[kLoMpIters];
      std::memcpy(&q.aft, w + kLoAft, sizeof(loam_pose6));
      std::memcpy(&q.bef, w + kLoBef, sizeof(loam_pose6));
      q.n_registered = (uint32_t)w[kLoNReg];
      L.nreg[l] = q.n_registered;
      // laserMapping's queue pointer walks inside transformUpdate, i.e. only when the L-M ran
      if (L.imu.step_imu && L.imu.mp_have[l] && w[kLoLmRan]) L.imu.mp[l].front = L.imu.mp_front[l];
      if (L.shared) {
        loc_result_of(L.loc_h + (size_t)l * kLocResWords, L.loc_info[l]);
      }
    }
    if (L.imu.step_imu) std::memcpy(&L.imu_trans[(size_t)l * 12], L.imu.trans_h + (size_t)l * 12, 12 * sizeof(float));
  }
  // /laser_cloud_surround: a lane whose phase this step wrapped publishes when the frame mapped it
  for (int l = 0; l < S; ++l)
    L.life[l].due = L.life[l].due == kDuePushed && out[l].status == LOAM_OK && out[l].mapped ? kDueYes : kDueNo;
  L.pulled = true;
  L.have_reg = L.step_mapped != 0;
  return LOAM_OK;
}

extern "C" int loam_lanes_registered(loam_ctx* x, uint32_t lane, loam_cloud_out* out) {
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused("loam_lanes_registered", L, kLanesOpen)) return rc;
  if (lane >= (uint32_t)L.S) return fail(LOAM_E_INVAL, "loam_lanes_registered: lane index out of range");
  if (L.in_flight || !L.have_reg)
    return fail(LOAM_E_INVAL, "loam_lanes_registered: the last pulled step did not map (or a step is in flight)");
  if (L.fail[lane] != LOAM_OK) return fail(LOAM_E_INVAL, "loam_lanes_registered: the lane has failed");
  const int n = (int)L.nreg[lane];
  if (n > 0 && (uint32_t)n <= out->capacity && !out->pts)
    return fail(LOAM_E_INVAL, "loam_lanes_registered: out->pts is null");
  HIP_TRY(hipSetDevice(x->device));
  x->pin.reset();
  const int rc = copy_out(x->st, x->pin, L.mp.reg + (size_t)lane * L.mp.capS, n, out);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(x->st));
  x->pin.finish();
  return LOAM_OK;
}

// ------------------------------------------------------------------ loam_lanes_clouds
namespace {
// Which of the nine clouds lane l holds from the last pulled step (bit c: cloud c of
// loam_lanes_clouds_out).  The host owns the lane states; the device's counts are stale where a bit
// is clear: k_od_end leaves fullEnd / nfullEnd alone on frames that do not publish it and writes an
// ordinary frame's into a lane whose own init frame the step was, and a failed lane's counts may
// hold anything.
int lanes_clouds_mask(const Lanes& L, int l) {
  const LaneLife& f = L.life[l];
  if (!L.pulled || !L.step_ran || L.fail[l] != LOAM_OK || f.wait >= 0 || f.kind == kLaneWaits) return 0;
  int m = 0x7f;  // scanRegistration's five and the Last clouds: every frame of a live lane
  if (f.kind == kLaneRuns && (L.step_pub & LOAM_PUB_FULL)) m |= 1 << 7;
  if (f.kind == kLaneRuns && L.step_mapped && L.nreg[l] > 0) m |= 1 << 8;  // (a LOAM_LOC_OFFGRID lane registered nothing)
  return m;
}

int lanes_clouds(loam_ctx* x, uint32_t n, const uint32_t* lane, loam_lanes_clouds_out* out, bool device,
                 void* consumer_stream) {
  static_assert(sizeof(loam_lanes_clouds_out) == LOAM_LANE_CLOUDS * 32 && LOAM_LANE_CLOUDS == kLaneClouds, "loam.h");
  const std::string who = device ? "loam_lanes_clouds_device" : "loam_lanes_clouds";
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused(who, L, kLanesOpen | kLanesIdle)) return rc;
  const int S = L.S;
  if (n == 0 || n > (uint32_t)S) return fail(LOAM_E_INVAL, who + ": n must be in [1, n_lanes]");
  if (!lane && n != (uint32_t)S) return fail(LOAM_E_INVAL, who + ": lane == NULL lists every lane: n must be n_lanes");
  if (lane) {
    std::vector<char> seen((size_t)S, 0);
    for (uint32_t i = 0; i < n; ++i) {
      const std::string at = who + ": lane[" + std::to_string(i) + "] = " + std::to_string(lane[i]);
      if (lane[i] >= (uint32_t)S) return fail(LOAM_E_INVAL, at + " is out of range");
      if (seen[lane[i]]) return fail(LOAM_E_INVAL, at + " is listed twice");
      seen[lane[i]] = 1;
    }
  }
  loam_batch_cloud* cl[kLaneClouds] = {&out->full, &out->sharp, &out->less_sharp, &out->flat, &out->less_flat,
                                       &out->corner_last, &out->surf_last, &out->full_end, &out->registered};
  static const char* const kName[kLaneClouds] = {"full", "sharp", "less_sharp", "flat", "less_flat",
                                                 "corner_last", "surf_last", "full_end", "registered"};
  unsigned wanted = 0, with_pts = 0;
  for (int c = 0; c < kLaneClouds; ++c) {
    if (cl[c]->pts || cl[c]->offset) wanted |= 1u << c;
    if (cl[c]->pts) with_pts |= 1u << c;
  }
  HIP_TRY(hipSetDevice(x->device));
  if (device) {  // every destination as loam_lanes_push_device validates its sources
    for (int c = 0; c < kLaneClouds; ++c) {
      if (!(with_pts >> c & 1)) continue;
      const uintptr_t p = (uintptr_t)cl[c]->pts;
      LaneFeedIn q;
      std::memset(&q, 0, sizeof(q));
      lanes_feed_lookup(cl[c]->pts, x->device, q);
      const std::string at = who + ": " + kName[c] + ".pts";
      if (!q.on_device) return fail(LOAM_E_INVAL, at + " is not plain device memory of the context's device");
      if (p & 15) return fail(LOAM_E_INVAL, at + " is not 16-byte aligned");
      const uint64_t room = q.size - (uint64_t)(p - q.base);
      if (cl[c]->capacity > room / sizeof(float4))
        return fail(LOAM_E_INVAL, at + ": capacity x 16 bytes leaves the pointer's allocation");
    }
  } else {
    const uint64_t lane_max = (uint64_t)pack_sweep_max(x) + L.od.capC + 2 * (uint64_t)L.od.capS + L.mp.capS;
    if (with_pts && lane_max > kPackStagePts)
      return fail(LOAM_E_INVAL, who + ": max_points is too large for the download staging (one lane's nine clouds "
                                "must fit " + std::to_string(kPackStagePts) + " points)");
  }
  // the masks, on the host: when no wanted cloud of any listed lane is there, nothing is launched
  std::vector<int> mask((size_t)S, 0);
  unsigned any = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const int l = lane ? (int)lane[i] : (int)i;
    mask[l] = lanes_clouds_mask(L, l);
    any |= (unsigned)mask[l];
  }
  if (!(any & wanted)) {
    for (int c = 0; c < kLaneClouds; ++c) {
      if (!(wanted >> c & 1)) continue;
      cl[c]->count = 0;
      if (cl[c]->offset) std::fill(cl[c]->offset, cl[c]->offset + n + 1, 0u);
    }
    return LOAM_OK;
  }
  if (lanes_clouds_alloc(L) != hipSuccess) return nomem(who + ": the mask / table block's allocation failed");
  hipStream_t st = x->st;
  std::copy(mask.begin(), mask.end(), L.cl_h);
  for (uint32_t i = 0; i < n; ++i) L.cl_h[S + i] = lane ? (int)lane[i] : (int)i;
  const int* mask_d = L.cl_d;
  const int* list_d = L.cl_d + S;
  const LanePackJob job = lanes_pack_job(L);
  x->prof.begin(st);
  HIP_TRY(hipMemcpyAsync(L.cl_d, L.cl_h, (size_t)2 * S * sizeof(int), hipMemcpyHostToDevice, st));
  x->prof.mark("lanes_clouds_h2d");
  HIP_TRY(lanes_pack_offsets(job, mask_d, list_d, (int)n, L.cl_tab_d, st));
  x->prof.mark("k_lanes_pack_offsets");
  const size_t row = (size_t)n + 1;
  HIP_TRY(hipMemcpyAsync(L.cl_tab_h, L.cl_tab_d, kLaneClouds * row * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  x->prof.mark("lanes_clouds_table_d2h");
  HIP_TRY(hipStreamSynchronize(st));
  const uint64_t* T = L.cl_tab_h;  // T[c * row + j]
  for (int c = 0; c < kLaneClouds; ++c)
    if ((wanted >> c & 1) && T[c * row + n] > 0xffffffffull) {
      x->prof.collect();
      return fail(LOAM_E_INVAL, who + ": a cloud of this list has more points than a uint32_t offset holds; ask for fewer lanes");
    }
  bool fits = true;
  unsigned pmask = 0;
  for (int c = 0; c < kLaneClouds; ++c) {
    if (!(wanted >> c & 1)) continue;
    const uint64_t total = T[c * row + n];
    cl[c]->count = total;
    if (cl[c]->offset)
      for (size_t j = 0; j < row; ++j) cl[c]->offset[j] = (uint32_t)T[c * row + j];
    if (!cl[c]->pts) continue;
    if (cl[c]->capacity < total) fits = false;
    else if (total > 0) pmask |= 1u << c;
  }
  if (!fits) {
    x->prof.collect();
    return fail(LOAM_E_CAPACITY, who + ": a cloud's capacity is too small (count holds the required size)");
  }
  if (!pmask) {
    x->prof.collect();
    return LOAM_OK;
  }
  LanePackDst d;
  if (device) {  // straight into the caller's buffers
    for (int c = 0; c < kLaneClouds; ++c) {
      d.dst[c] = (float4*)cl[c]->pts;
      d.dbase[c] = 0;
    }
    hipStream_t cons = (hipStream_t)consumer_stream;
    if (cons && !L.cl_done) HIP_TRY(hipEventCreateWithFlags(&L.cl_done, hipEventDisableTiming));
    HIP_TRY(lanes_pack(job, L.cl_tab_d, list_d, (int)n, 0, (int)n, pmask, d, st));
    x->prof.mark("k_lanes_pack");
    if (cons) {  // the consumer's later work behind the pack; the marks are folded in by the next timeline
      HIP_TRY(hipEventRecord(L.cl_done, st));
      HIP_TRY(hipStreamWaitEvent(cons, L.cl_done, 0));
      return LOAM_OK;
    }
    HIP_TRY(hipStreamSynchronize(st));
    x->prof.collect();
    return LOAM_OK;
  }
  std::vector<LaneCloudsChunk> chunks;
  uint32_t bad = 0;
  if (!lanes_clouds_plan(T, n, pmask, kPackStagePts, chunks, &bad)) {  // (cannot happen: lane_max above)
    x->prof.collect();
    return fail(LOAM_E_INVAL, who + ": a lane's clouds exceed the download staging");
  }
  if (const int rc = ensure_pack_stage(x, "lanes clouds download")) {
    x->prof.collect();
    return rc;
  }
  // chunk k: packed into device buffer k & 1 and DMA'd into pinned buffer k & 1; while the host
  // copies chunk k into the caller's arrays, chunk k + 1 is packed and transferred (loam_batch_features)
  auto enqueue = [&](size_t k) -> hipError_t {
    const LaneCloudsChunk& ch = chunks[k];
    const int i = (int)(k & 1);
    for (int c = 0; c < kLaneClouds; ++c) {
      d.dst[c] = x->pack_dev[i];
      d.dbase[c] = (long long)ch.cbase[c] - (long long)T[c * row + ch.j0];
    }
    x->prof.mark("lanes_clouds_host_wait");
    hipError_t e = lanes_pack(job, L.cl_tab_d, list_d, (int)n, (int)ch.j0, (int)(ch.j1 - ch.j0), pmask, d, st);
    x->prof.mark("k_lanes_pack");
    if (e == hipSuccess)
      e = hipMemcpyAsync(x->pack_pin[i], x->pack_dev[i], ch.pts * sizeof(float4), hipMemcpyDeviceToHost, st);
    x->prof.mark("lanes_clouds_d2h");
    if (e == hipSuccess) e = hipEventRecord(x->pack_done[i], st);
    return e;
  };
  hipError_t he = hipSuccess;
  for (size_t k = 0; k < chunks.size() && k < 2 && he == hipSuccess; ++k) he = enqueue(k);
  for (size_t k = 0; k < chunks.size() && he == hipSuccess; ++k) {
    const LaneCloudsChunk& ch = chunks[k];
    he = hipEventSynchronize(x->pack_done[k & 1]);
    if (he != hipSuccess) break;
    for (int c = 0; c < kLaneClouds; ++c) {
      if (!(pmask >> c & 1)) continue;
      const uint64_t a = T[c * row + ch.j0], b = T[c * row + ch.j1];
      if (b > a) copy_wide(cl[c]->pts + a, x->pack_pin[k & 1] + ch.cbase[c], (size_t)(b - a) * sizeof(float4));
    }
    if (k + 2 < chunks.size()) he = enqueue(k + 2);
  }
  if (he != hipSuccess) {  // (drain what was enqueued before reporting)
    (void)hipStreamSynchronize(st);
    return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
  }
  x->prof.collect();
  return LOAM_OK;
}
}  // namespace

extern "C" int loam_lanes_clouds(loam_ctx* x, uint32_t n, const uint32_t* lane, loam_lanes_clouds_out* out) {
  return lanes_clouds(x, n, lane, out, false, nullptr);
}

extern "C" int loam_lanes_clouds_device(loam_ctx* x, uint32_t n, const uint32_t* lane, loam_lanes_clouds_out* out,
                                        void* consumer_stream) {
  return lanes_clouds(x, n, lane, out, true, consumer_stream);
}

// dev_hooks.h: the two pack kernels on caller-made clouds
extern "C" int loam_dev_lanes_pack(int device, int32_t S, const int32_t* strides, const int32_t* counts, const int32_t* mask,
                                   const uint32_t* list, int32_t n, const float* const* src, float* dst, uint64_t dst_points,
                                   uint64_t* table_out) {
  static_assert(LOAM_DEV_LANES_PACK_TILE == kLanePackTile, "dev_hooks.h");
  const std::string who = "loam_dev_lanes_pack";
  if (!strides || !counts || !mask || !list || !src || !dst || !table_out || S < 1 || S > LOAM_LANES_MAX || n < 1 || n > S)
    return fail(LOAM_E_INVAL, who + ": bad argument");
  size_t src_pts[kLaneClouds], all = 0;
  for (int c = 0; c < kLaneClouds; ++c) {
    if (!src[c] || strides[c] < 1 || strides[c] > LOAM_DEV_LANES_PACK_MAX_STRIDE) return fail(LOAM_E_INVAL, who + ": bad cloud");
    src_pts[c] = (size_t)S * strides[c];
    all += src_pts[c];
  }
  for (int32_t i = 0; i < n; ++i)
    if (list[i] >= (uint32_t)S) return fail(LOAM_E_INVAL, who + ": a lane index is out of range");
  // what the kernels will count, restated: the destination must hold it
  uint64_t need = 0;
  for (int c = 0; c < kLaneClouds; ++c)
    for (int32_t i = 0; i < n; ++i)
      if (mask[list[i]] >> c & 1) need += (uint64_t)std::min(std::max(counts[(size_t)c * S + list[i]], 0), strides[c]);
  if (need > dst_points) return fail(LOAM_E_CAPACITY, who + ": dst is too small for the selection");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(LOAM_E_HIP, "no HIP device");  // (no CPU path)
  if (device < 0 || device >= ndev) return fail(LOAM_E_INVAL, who + ": no such device");
  HIP_TRY(hipSetDevice(device));
  float4 *src_d = nullptr, *dst_d = nullptr;
  int* ints_d = nullptr;  // counts [9][S], mask [S], list [n]
  uint64_t* tab_d = nullptr;
  const size_t nints = (size_t)kLaneClouds * S + S + n, tab = (size_t)kLaneClouds * (n + 1);
  hipError_t e = hipMalloc((void**)&src_d, all * sizeof(float4));
  if (e == hipSuccess) e = hipMalloc((void**)&dst_d, std::max<uint64_t>(dst_points, 1) * sizeof(float4));
  if (e == hipSuccess) e = hipMalloc((void**)&ints_d, nints * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&tab_d, tab * sizeof(uint64_t));
  const bool nomem = e != hipSuccess;
  LanePackJob job;
  LanePackDst d;
  job.S = S;
  size_t at = 0;
  for (int c = 0; c < kLaneClouds && e == hipSuccess; ++c) {
    e = hipMemcpy(src_d + at, src[c], src_pts[c] * sizeof(float4), hipMemcpyHostToDevice);
    job.c[c] = {src_d + at, ints_d + (size_t)c * S, strides[c], 1};
    at += src_pts[c];
    d.dst[c] = dst_d;  // cloud c's selection behind cloud c - 1's (dbase below, from the table)
    d.dbase[c] = 0;
  }
  if (e == hipSuccess) e = hipMemcpy(ints_d, counts, (size_t)kLaneClouds * S * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ints_d + (size_t)kLaneClouds * S, mask, (size_t)S * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ints_d + (size_t)kLaneClouds * S + S, list, (size_t)n * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dst_d, dst, dst_points * sizeof(float4), hipMemcpyHostToDevice);
  const int* mask_d = ints_d + (size_t)kLaneClouds * S;
  const int* list_d = mask_d + S;
  if (e == hipSuccess) e = lanes_pack_offsets(job, mask_d, list_d, n, tab_d, nullptr);
  if (e == hipSuccess) e = hipMemcpy(table_out, tab_d, tab * sizeof(uint64_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) {
    uint64_t run = 0, total = 0;
    for (int c = 0; c < kLaneClouds; ++c) total += table_out[(size_t)c * (n + 1) + n];
    if (total != need) {  // (the kernel and the restatement above disagree: nothing is packed)
      e = hipErrorUnknown;
    } else {
      for (int c = 0; c < kLaneClouds; ++c) {
        d.dbase[c] = (long long)run;
        run += table_out[(size_t)c * (n + 1) + n];
      }
      e = lanes_pack(job, tab_d, list_d, n, 0, n, (1u << kLaneClouds) - 1, d, nullptr);
    }
  }
  if (e == hipSuccess) e = hipMemcpy(dst, dst_d, dst_points * sizeof(float4), hipMemcpyDeviceToHost);
  if (src_d) (void)hipFree(src_d);
  if (dst_d) (void)hipFree(dst_d);
  if (ints_d) (void)hipFree(ints_d);
  if (tab_d) (void)hipFree(tab_d);
  if (e == hipSuccess) return LOAM_OK;
  (void)hipGetLastError();
  return nomem ? fail(LOAM_E_NOMEM, who + ": allocation failed") : fail(LOAM_E_HIP, who + ": " + hipGetErrorString(e));
}

extern "C" int loam_lanes_map_export(loam_ctx* x, uint32_t lane, loam_map* out) {
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused("loam_lanes_map_export", L, kLanesOpen)) return rc;
  if (L.shared)
    return fail(LOAM_E_INVAL, "loam_lanes_map_export: shared lanes have no lane map (loam_map_export gives the context's)");
  if (lane >= (uint32_t)L.S) return fail(LOAM_E_INVAL, "loam_lanes_map_export: lane index out of range");
  if (const int rc = lanes_state_refused("loam_lanes_map_export", L, kLanesIdle)) return rc;
  if (L.fail[lane] != LOAM_OK) return fail(LOAM_E_INVAL, "loam_lanes_map_export: the lane has failed");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipStreamSynchronize(x->st));
  return map_export_of(x, L.mp, (int)lane, L.life[lane].phase, out);
}

// One map into n lanes between two steps (loam.h).  The stream is idle (the pull
// drained it), so the import's scratch (vin, the sort arrays, app_cnt, the idle pool) is free; the
// map is binned and sorted once into the idle pool's first segment, and one launch copies it into
// the listed lanes' current pool segments and slot tables.  pool_cur does not move.
extern "C" int loam_lanes_map_import(loam_ctx* x, uint32_t n, const uint32_t* lane, const loam_map* in,
                                     const loam_pose6* aft, uint64_t* dropped) {
  if (!x || !lane || !in) return fail(LOAM_E_INVAL, "null argument");
  const std::string who = "loam_lanes_map_import";
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused(who, L, kLanesOpen)) return rc;
  if (L.shared)
    return fail(LOAM_E_INVAL, who + ": shared lanes have no lane map (loam_map_import changes the context's, "
                                    "loam_lanes_set_pose a lane's poses)");
  if (const int rc = lanes_state_refused(who, L, kLanesIdle)) return rc;
  if (n == 0 || n > (uint32_t)L.S) return fail(LOAM_E_INVAL, who + ": n must be in [1, n_lanes]");
  int rc = lanes_list_refused(who, L, lane, n, /*for_import=*/true);
  if (rc) return rc;
  rc = map_import_args(in, who);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipStreamSynchronize(x->st));
  if (!L.mi_h) {
    const hipError_t ae = lanes_map_import_alloc(L);
    if (ae != hipSuccess) return nomem(who + ": allocation failed: " + hipGetErrorString(ae));
  }
  MpBuffers& b = L.mp;
  hipStream_t st = x->st;
  int kept = 0;
  rc = map_import_bin(x, b, in, who, dropped, &kept);
  if (rc) return rc;
  if (kept > b.map_cap) {
    x->prof.collect();
    return fail(LOAM_E_CAPACITY, who + ": the points inside the grid exceed lane_map_capacity");
  }
  // everything so far wrote scratch only, and so do the sort and the table; the lanes change in the
  // one launch behind them
  for (int k = 0; k < 3; ++k) L.mi_h[kMiCen + k] = in->center[k];
  std::memcpy(L.mi_h + kMiBef, &in->bef, sizeof(loam_pose6));
  for (uint32_t i = 0; i < n; ++i) {
    L.mi_h[kMiList + i] = (int)lane[i];
    std::memcpy(L.mi_h + kMiList + n + 6 * (size_t)i, aft ? &aft[i] : &in->aft, sizeof(loam_pose6));
  }
  float4* sorted = mp_map_idle_pool(b);
  hipError_t he = hipMemcpyAsync(L.mi_d, L.mi_h, ((size_t)kMiList + 7 * (size_t)n) * sizeof(int), hipMemcpyHostToDevice, st);
  x->prof.mark("lanes_map_import_h2d");
  if (he == hipSuccess) he = mp_map_sort(b, kept, sorted, st, &x->prof);
  if (he == hipSuccess) he = mp_map_slots(b, x->mio, st, &x->prof);
  if (he == hipSuccess) he = lanes_map_install(L, sorted, kept, x->mio.tab + kMapTabSlots, (int)n, st);
  x->prof.mark("k_lanes_map_install");
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    (void)hipStreamSynchronize(st);
    return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
  }
  x->prof.collect();
  for (uint32_t i = 0; i < n; ++i) {  // (as loam_map_import: a pending surround publication is dropped)
    L.life[lane[i]].phase = in->surround_phase;
    L.life[lane[i]].due = kDueNo;
  }
  return LOAM_OK;
}

// /laser_cloud_surround of every due lane (loam.h).  The stream is idle (the pull
// drained it) and the lanes' vin / vout / VoxelGrid arrays are free until the next push: one launch
// sequence gathers, filters and packs the due lanes' clouds there, the counts come back in one copy
// behind one synchronisation, and the packed points leave through the shared download staging.
extern "C" int loam_lanes_surround(loam_ctx* x, loam_lanes_cloud* out) {
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  Lanes& L = x->lanes;
  if (const int rc = lanes_state_refused("loam_lanes_surround", L, kLanesOpen)) return rc;
  if (L.shared)
    return fail(LOAM_E_INVAL, "loam_lanes_surround: shared lanes have no lane map (loam_mapping_surround gives the context's)");
  if (const int rc = lanes_state_refused("loam_lanes_surround", L, kLanesIdle)) return rc;
  const int S = L.S;
  int n = 0;
  for (int l = 0; l < S; ++l) n += L.life[l].due == kDueYes;
  auto fill = [&](const int* cnt) {  // cnt: the due lanes' counts by lane (null: nothing is due)
    uint64_t run = 0;
    for (int l = 0; l < S; ++l) {
      const bool due = cnt && L.life[l].due == kDueYes;
      if (out->offset) out->offset[l] = (uint32_t)run;
      if (out->published) out->published[l] = due ? 1 : 0;
      if (due) run += (uint64_t)cnt[l];
    }
    if (out->offset) out->offset[S] = (uint32_t)run;
    out->count = run;
  };
  if (n == 0) {
    fill(nullptr);
    return LOAM_OK;
  }
  HIP_TRY(hipSetDevice(x->device));
  const bool want = out->pts != nullptr;
  if (lanes_surround_alloc(L) != hipSuccess) return nomem("loam_lanes_surround: allocation failed");
  if (want) {
    const int rc = ensure_pack_stage(x, "surround download");
    if (rc) return rc;
  }
  n = 0;
  for (int l = 0; l < S; ++l)
    if (L.life[l].due == kDueYes) L.su_h[n++] = l;
  hipStream_t st = x->st;
  x->prof.begin(st);
  hipError_t he = lanes_surround_run(L, n, want, st, x->prof.on ? &x->prof : nullptr);
  const hipError_t se = hipStreamSynchronize(st);
  if (he == hipSuccess) he = se;
  if (he == hipSuccess) he = L.mp.take_error();
  if (he != hipSuccess) return fail(LOAM_E_HIP, std::string("loam_lanes_surround: ") + hipGetErrorString(he));
  std::vector<int> cnt((size_t)S, 0);
  for (int i = 0; i < n; ++i) cnt[L.su_h[i]] = lanes_surround_count(L, L.su_h[i]);
  fill(cnt.data());
  const uint64_t total = out->count;
  if (!want || total == 0) {
    x->prof.collect();
    return LOAM_OK;
  }
  if (total > out->capacity) {
    x->prof.collect();
    return fail(LOAM_E_CAPACITY, "loam_lanes_surround: capacity is too small (count holds the required size)");
  }
  // the packed runs (vin from 0 on) in chunks of one pinned buffer: chunk k is DMA'd into buffer
  // k & 1 while the host copies chunk k - 1 into the caller's array (as loam_map_export)
  const float4* packed = L.mp.vin;
  const size_t nchunk = (size_t)((total + kPackStagePts - 1) / kPackStagePts);
  auto enqueue = [&](size_t k) -> hipError_t {
    const size_t a = k * kPackStagePts, m = std::min(kPackStagePts, (size_t)total - a);
    hipError_t e = hipMemcpyAsync(x->pack_pin[k & 1], packed + a, m * sizeof(float4), hipMemcpyDeviceToHost, st);
    x->prof.mark("lanes_surround_d2h");
    if (e == hipSuccess) e = hipEventRecord(x->pack_done[k & 1], st);
    return e;
  };
  for (size_t k = 0; k < nchunk && k < 2 && he == hipSuccess; ++k) he = enqueue(k);
  for (size_t k = 0; k < nchunk && he == hipSuccess; ++k) {
    const size_t a = k * kPackStagePts, m = std::min(kPackStagePts, (size_t)total - a);
    he = hipEventSynchronize(x->pack_done[k & 1]);
    if (he != hipSuccess) break;
    copy_wide(out->pts + a, x->pack_pin[k & 1], m * sizeof(float4));
    if (k + 2 < nchunk) he = enqueue(k + 2);
  }
  if (he != hipSuccess) {  // (drain what was enqueued before reporting)
    (void)hipStreamSynchronize(st);
    return fail(LOAM_E_HIP, std::string("loam_lanes_surround: ") + hipGetErrorString(he));
  }
  x->prof.collect();
  return LOAM_OK;
}
