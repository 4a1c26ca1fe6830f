// libloam_hip host engine: the map services on the context's streaming store: export / import,
// multi-hypothesis localization, scoring, and the parts of those sequences that the lanes' forms
// (engine_lanes.cpp) run too.
#include "engine_ctx.hpp"

namespace loam {
namespace eng {

int sync_or_fail(loam_ctx* x, hipError_t he, const std::string& who) {
  if (he == hipSuccess) he = hipStreamSynchronize(x->st);
  if (he == hipSuccess) return LOAM_OK;
  (void)hipStreamSynchronize(x->st);
  x->prof.collect();
  return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
}

int nomem(const std::string& msg) {
  (void)hipGetLastError();
  return fail(LOAM_E_NOMEM, msg);
}

int store_invalid(const std::string& who) {
  return fail(LOAM_E_INVAL, who + ": the last map update exceeded map_capacity, the store is not valid");
}

void cand_rows(float* dst, size_t rows, const loam_pose6* aft, const loam_pose6* bef) {
  for (size_t h = 0; h < rows; ++h) {
    std::memcpy(dst + h * 12, &aft[h], sizeof(loam_pose6));
    if (bef) std::memcpy(dst + h * 12 + 6, &bef[h], sizeof(loam_pose6));
    else std::memset(dst + h * 12 + 6, 0, sizeof(loam_pose6));
  }
}

// ------------------------------------------------------------------ map export / import
// a context's queued work: the node calls' stream and the side stream a deferred update runs on
int map_drain(loam_ctx* x) {
  HIP_TRY(hipSetDevice(x->device));
  mp_wait_update(x->mp1, x->st);
  HIP_TRY(hipStreamSynchronize(x->st));
  if (x->st2) HIP_TRY(hipStreamSynchronize(x->st2));
  const hipError_t he = x->mp1.take_error();
  if (he != hipSuccess) return fail(LOAM_E_HIP, std::string("mapping: ") + hipGetErrorString(he));
  return LOAM_OK;
}

// loam_map_export's body for instance `inst` of the store b, whose queued work has been drained
// (loam_map_export: the streaming store; loam_lanes_map_export: a lane); phase: its mapFrameCount
int map_export_of(loam_ctx* x, MpBuffers& b, int inst, int phase, loam_map* out) {
  int rc = LOAM_OK;
  HIP_TRY(mp_map_ensure(x->mio));
  hipStream_t st = x->st;
  x->prof.begin(st);
  HIP_TRY(mp_map_table(b, x->mio, st, &x->prof, inst));
  HIP_TRY(hipStreamSynchronize(st));
  const int* T = x->mio.tab_h;
  const int nC = T[kMapTabOff + kCubeNum], total = T[kMapTabOff + kMapKeys];
  if ((T[kMapTabInfo + 3] & ERR_CAP_MAP) || nC < 0 || total < nC || total > b.map_cap) {
    x->prof.collect();
    return store_invalid("loam_map_export");
  }
  loam_map_cloud* cl[2] = {&out->corner, &out->surf};
  const int first[2] = {0, nC}, count[2] = {nC, total - nC};
  bool fits = true, want = false;
  for (int k = 0; k < 2; ++k) {
    cl[k]->count = (uint64_t)count[k];
    if (cl[k]->cube_offset)
      for (int c = 0; c <= kCubeNum; ++c) cl[k]->cube_offset[c] = (uint32_t)(T[kMapTabOff + k * kCubeNum + c] - first[k]);
    if (!cl[k]->pts) continue;
    if (cl[k]->capacity < (uint64_t)count[k]) fits = false;
    else if (count[k] > 0) want = true;
  }
  for (int k = 0; k < 3; ++k) out->center[k] = T[kMapTabInfo + k];
  out->surround_phase = phase;
  std::memcpy(&out->aft, T + kMapTabInfo + 4, sizeof(loam_pose6));
  std::memcpy(&out->bef, T + kMapTabInfo + 10, sizeof(loam_pose6));
  if (!fits) {
    x->prof.collect();
    return fail(LOAM_E_CAPACITY, "loam_map_export: a cloud's capacity is too small (count holds the required size)");
  }
  if (!want) {
    x->prof.collect();
    return LOAM_OK;
  }
  rc = ensure_pack_stage(x, "map export");
  if (rc) return rc;
  HIP_TRY(mp_map_pack(b, x->mio, total, st, &x->prof, inst));
  const float4* packed = b.vin + (size_t)inst * b.map_cap;
  // the wanted clouds' runs of vin in chunks of one pinned buffer: chunk k is DMA'd into buffer
  // k & 1 while the host copies chunk k - 1 into the caller's array
  struct Chunk {
    int kind;
    size_t a, n;  // points [a, a + n) of the cloud
  };
  std::vector<Chunk> chunks;
  for (int k = 0; k < 2; ++k)
    if (cl[k]->pts)
      for (size_t a = 0; a < (size_t)count[k]; a += kPackStagePts)
        chunks.push_back({k, a, std::min(kPackStagePts, (size_t)count[k] - a)});
  auto enqueue = [&](size_t k) -> hipError_t {
    const Chunk& ch = chunks[k];
    x->prof.mark("map_export_host_wait");
    hipError_t e = hipMemcpyAsync(x->pack_pin[k & 1], packed + first[ch.kind] + ch.a, ch.n * sizeof(float4),
                                  hipMemcpyDeviceToHost, st);
    x->prof.mark("map_export_d2h");
    if (e == hipSuccess) e = hipEventRecord(x->pack_done[k & 1], st);
    return e;
  };
  hipError_t he = hipSuccess;
  for (size_t k = 0; k < chunks.size() && k < 2 && he == hipSuccess; ++k) he = enqueue(k);
  for (size_t k = 0; k < chunks.size() && he == hipSuccess; ++k) {
    const Chunk& ch = chunks[k];
    he = hipEventSynchronize(x->pack_done[k & 1]);
    if (he != hipSuccess) break;
    copy_wide(cl[ch.kind]->pts + ch.a, x->pack_pin[k & 1], ch.n * sizeof(float4));
    if (k + 2 < chunks.size()) he = enqueue(k + 2);
  }
  if (he != hipSuccess) {  // (drain what was enqueued before reporting)
    (void)hipStreamSynchronize(st);
    return fail(LOAM_E_HIP, std::string("loam_map_export: ") + hipGetErrorString(he));
  }
  x->prof.collect();
  return LOAM_OK;
}

// what loam_map_import and loam_lanes_map_import (who: the call's name) refuse of `in`
int map_import_args(const loam_map* in, const std::string& who) {
  const loam_map_cloud* cl[2] = {&in->corner, &in->surf};
  for (int k = 0; k < 2; ++k)
    if (cl[k]->count > 0 && !cl[k]->pts) return fail(LOAM_E_INVAL, who + ": a cloud's pts is null");
  if (in->surround_phase < 0 || in->surround_phase > 4)
    return fail(LOAM_E_INVAL, who + ": surround_phase must be 0..4");
  for (int k = 0; k < 3; ++k)
    if (in->center[k] > (1 << 24) || in->center[k] < -(1 << 24))
      return fail(LOAM_E_INVAL, who + ": a center component is beyond 2^24");
  const uint64_t kMaxIn = ((uint64_t)1 << 31) - ((uint64_t)1 << 23);
  if (cl[0]->count > kMaxIn || cl[1]->count > kMaxIn || cl[0]->count + cl[1]->count > kMaxIn)
    return fail(LOAM_E_INVAL, who + ": more than 2^31 - 2^23 points");
  return LOAM_OK;
}

// The two clouds of `in` uploaded and binned into the scratch of the store b, whose queued work has
// been drained: the kept points in input order in b.vin with their keys and per-key counts
// (mp_map_bin_chunk); nothing of the store changes.  Begins the profile interval, fills dropped
// (when given) and *kept (which may exceed b.map_cap: the caller's LOAM_E_CAPACITY).
int map_import_bin(loam_ctx* x, MpBuffers& b, const loam_map* in, const std::string& who, uint64_t* dropped, int* kept) {
  const loam_map_cloud* cl[2] = {&in->corner, &in->surf};
  HIP_TRY(mp_map_ensure(x->mio));
  if (cl[0]->count + cl[1]->count > 0) {
    const int rc = ensure_pack_stage(x, "map import");
    if (rc) return rc;
  }
  static_assert(kMapChunkPts <= (int)kPackStagePts, "an import chunk fits one staging buffer");
  hipStream_t st = x->st;
  const int cen[3] = {in->center[0], in->center[1], in->center[2]};
  x->prof.begin(st);
  hipError_t he = mp_map_bin_begin(b, x->mio, st);
  // chunk k: copied into pinned buffer k & 1, DMA'd into device buffer k & 1 and binned there, while
  // the host copies chunk k + 1 into the other pinned buffer
  size_t k = 0;
  for (int kind = 0; kind < 2 && he == hipSuccess; ++kind)
    for (uint64_t a = 0; a < cl[kind]->count && he == hipSuccess; a += kMapChunkPts, ++k) {
      const size_t n = (size_t)std::min<uint64_t>(kMapChunkPts, cl[kind]->count - a);
      const int i = (int)(k & 1);
      if (k >= 2) he = hipEventSynchronize(x->pack_done[i]);  // (the chunk two back has left both buffers)
      if (he != hipSuccess) break;
      copy_wide(x->pack_pin[i], cl[kind]->pts + a, n * sizeof(float4));
      x->prof.mark("map_import_host_wait");
      he = hipMemcpyAsync(x->pack_dev[i], x->pack_pin[i], n * sizeof(float4), hipMemcpyHostToDevice, st);
      x->prof.mark("map_import_h2d");
      if (he == hipSuccess) he = mp_map_bin_chunk(b, x->mio, x->pack_dev[i], (int)n, kind, cen, st, &x->prof);
      if (he == hipSuccess) he = hipEventRecord(x->pack_done[i], st);
    }
  if (he == hipSuccess) he = mp_map_bin_result(x->mio, st);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    (void)hipStreamSynchronize(st);
    return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
  }
  const int* acc = x->mio.tab_h + kMapTabAcc;
  if (dropped) {
    dropped[0] = (uint64_t)acc[1];
    dropped[1] = (uint64_t)acc[2];
  }
  *kept = acc[0];
  return LOAM_OK;
}

// a k_mp_loc_result block as the C-ABI hands it out
void loc_result_of(const int* r, loam_localize_result& o) {
  std::memcpy(&o.aft, r + kLrAft, sizeof(loam_pose6));
  o.status = r[kLrStatus];
  o.iters = r[kLrIters];
  o.degenerate_steps = r[kLrDegSteps];
  o.rows_last = (uint32_t)r[kLrRowsLast];
  o.rows_sum = (uint32_t)r[kLrRowsSum];
  o.stack_corner = (uint32_t)r[kLrStackC];
  o.stack_surf = (uint32_t)r[kLrStackS];
  o.map_corner = (uint32_t)r[kLrMapC];
  o.map_surf = (uint32_t)r[kLrMapS];
}

int localize_finish(loam_ctx* x, const std::string& who, const MpInput& in, int rows, int in_max, const LocRows* lr,
                    const char* mark, loam_localize_result* out) {
  MpLoc& L = x->loc;
  const MpBuffers& s = x->mp1;
  hipStream_t st = x->st;
  Prof* pf = x->prof.on ? &x->prof : nullptr;  // (with profiling the L-M kernels also count their work)
  const int* head = L.head_h();
  if (head[2 * rows] & ERR_CAP_MAP) {
    x->prof.collect();
    return store_invalid(who);
  }
  int from_max = 0, cloud_max = 0;
  for (int h = 0; h < rows; ++h) {
    from_max = std::max(from_max, head[2 * h] + head[2 * h + 1]);
    cloud_max = std::max(cloud_max, std::max(head[2 * h], head[2 * h + 1]));
  }
  hipError_t he = mp_loc_reserve_map(L, from_max);
  if (he != hipSuccess) {
    x->prof.collect();
    return nomem(who + ": FromMap allocation failed (" + std::to_string(rows) + " x " + std::to_string(from_max) +
                 " points): " + hipGetErrorString(he));
  }
  he = mp_localize_solve(L, s, in, rows, from_max, cloud_max, in_max, st, pf, lr);
  x->prof.mark(mark);
  if (const int rc = sync_or_fail(x, he, who)) return rc;
  x->prof.collect();
  const int* R = L.res_h();
  for (int h = 0; h < rows; ++h) loc_result_of(R + (size_t)h * kLocResWords, out[h]);
  return LOAM_OK;
}

int score_max_dist_refused(const std::string& who, float max_dist) {
  if (max_dist > 0.0f && max_dist <= 1.0f) return LOAM_OK;
  return fail(LOAM_E_INVAL, who + ": max_dist must be in (0, 1] (the map index has 1 m cells)");
}

int score_map_sizes(loam_ctx* x, const std::string& who, int* nC, int* total) {
  const int* T = x->mio.tab_h;
  *nC = T[kMapTabOff + kCubeNum];
  *total = T[kMapTabOff + kMapKeys];
  if ((T[kMapTabInfo + 3] & ERR_CAP_MAP) || *nC < 0 || *total < *nC || *total > x->mp1.map_cap) {
    x->prof.collect();
    return store_invalid(who);
  }
  return LOAM_OK;
}

int score_reserve_index(loam_ctx* x, const std::string& who, int nC, int total, int cnt_c, int cnt_s, int rows) {
  const hipError_t he = mp_score_reserve_map(x->score, nC, total - nC, cnt_c, cnt_s, rows);
  if (he == hipSuccess) return LOAM_OK;
  x->prof.collect();
  return nomem(who + ": index allocation failed (" + std::to_string(total) + " map points): " + hipGetErrorString(he));
}

void score_count_work(loam_ctx* x, double queries) {  // work counters beside the kernel times: (count, calls)
  const char* names[3] = {"score_nn_candidates", "score_nn_cells", "score_queries"};
  const double v[3] = {(double)x->score.work_h()[0], (double)x->score.work_h()[1], queries};
  for (int k = 0; k < 3; ++k) {
    auto& a = x->prof.acc[names[k]];
    a.first += v[k];
    a.second += 1;
  }
}

}  // namespace eng
}  // namespace loam

extern "C" int loam_map_export(loam_ctx* x, loam_map* out) {
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  const int rc = map_drain(x);
  if (rc) return rc;
  return map_export_of(x, x->mp1, 0, x->map_frame_count, out);
}

extern "C" int loam_map_import(loam_ctx* x, const loam_map* in, uint64_t* dropped) {
  if (!x || !in) return fail(LOAM_E_INVAL, "null argument");
  int rc = map_import_args(in, "loam_map_import");
  if (rc) return rc;
  rc = map_drain(x);
  if (rc) return rc;
  MpBuffers& b = x->mp1;
  hipStream_t st = x->st;
  const int cen[3] = {in->center[0], in->center[1], in->center[2]};
  int kept = 0;
  rc = map_import_bin(x, b, in, "loam_map_import", dropped, &kept);
  if (rc) return rc;
  if (kept > b.map_cap) {
    x->prof.collect();
    return fail(LOAM_E_CAPACITY, "loam_map_import: the points inside the grid exceed map_capacity");
  }
  // everything so far wrote scratch only; the sort fills the idle pool and its slot table, and the
  // store switches to them once they are enqueued without error
  float pose12[12];
  std::memcpy(pose12, &in->aft, sizeof(loam_pose6));
  std::memcpy(pose12 + 6, &in->bef, sizeof(loam_pose6));
  hipError_t he = mp_map_install(b, x->mio, kept, cen, pose12, st, &x->prof);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) return fail(LOAM_E_HIP, std::string("loam_map_import: ") + hipGetErrorString(he));
  x->prof.collect();
  // (statistics only: the valid-point slot a deferred update's next frame reads as "the previous
  // frame's", mp_stream_run; no frame built this store)
  *(int*)(x->xb.h + kXferMpUpd + 4 * (1 - b.pool_cur)) = 0;
  x->map_frame_count = in->surround_phase;
  x->surround_due = false;
  return LOAM_OK;
}

// ------------------------------------------------------------------ multi-hypothesis localization
// n candidate (Aft, Bef) poses of one sweep against the streaming map, which is only read: every
// candidate is an instance of the context's second mapping working set (MpLoc, mp.hpp).  The host
// reads the candidates' FromMap counts once (to size the set), then the results.
extern "C" int loam_map_localize(loam_ctx* x, const loam_pose6* odom_sum, const loam_cloud_out* corner_last,
                                 const loam_cloud_out* surf_last, uint32_t n, const loam_pose6* aft,
                                 const loam_pose6* bef, loam_localize_result* out) {
  static_assert(LOAM_LOCALIZE_MAX == kLocMax, "loam.h and mp.hpp");
  static_assert(sizeof(loam_localize_result) == 60, "loam_localize_result layout");
  if (!x || !odom_sum || !corner_last || !surf_last || !aft || !out) return fail(LOAM_E_INVAL, "null argument");
  const std::string who = "loam_map_localize";
  if (n == 0 || n > LOAM_LOCALIZE_MAX) return fail(LOAM_E_INVAL, who + ": n must be in [1, LOAM_LOCALIZE_MAX]");
  if ((corner_last->count && !corner_last->pts) || (surf_last->count && !surf_last->pts))
    return fail(LOAM_E_INVAL, who + ": a cloud's pts is null");
  const MpBuffers& s = x->mp1;
  // (corner_last: also the mapping stack's own bound, 120 picks per ring, as loam_mapping has it)
  if (corner_last->count > (uint32_t)x->cap || surf_last->count > (uint32_t)x->cap ||
      corner_last->count > (uint32_t)s.capC)
    return fail(LOAM_E_INVAL, who + ": a cloud exceeds max_points (corner_last: 120 points per ring)");
  int rc = map_drain(x);
  if (rc) return rc;
  MpLoc& L = x->loc;
  hipError_t he = mp_loc_reserve(L, s, (int)n, (int)corner_last->count, (int)surf_last->count);
  if (he != hipSuccess) return nomem(who + ": working set allocation failed: " + hipGetErrorString(he));
  hipStream_t st = x->st;
  Prof* pf = x->prof.on ? &x->prof : nullptr;  // (with profiling the L-M kernels also count their work)
  MpBuffers& w = L.w;
  cand_rows(L.cand_h(), n, aft, bef);
  const int cnt[3] = {(int)corner_last->count, (int)surf_last->count, 0};
  x->prof.begin(st);
  x->pin.reset();
  he = x->pin.reserve((size_t)cnt[0] + cnt[1], st);
  if (he == hipSuccess) he = x->pin.up(st, w.inC, corner_last->pts, (size_t)cnt[0]);
  if (he == hipSuccess) he = x->pin.up(st, w.inS, surf_last->pts, (size_t)cnt[1]);
  if (he == hipSuccess) {
    Xfer xp;
    xp.put(w.in_n, cnt, 3 * sizeof(int));
    xp.put(w.in_pose, odom_sum, 6 * sizeof(float));
    he = xfer_launch(xp, st);
  }
  x->prof.mark("map_localize_h2d");
  MpInput in;  // the one sweep, read by every candidate
  in.corner = w.inC; in.surf = w.inS; in.full = nullptr;
  in.corner_stride = in.surf_stride = in.full_stride = 0;
  in.ncorner = w.in_n; in.nsurf = w.in_n + 1; in.nfull = w.in_n + 2;
  in.ncorner_stride = in.nsurf_stride = in.nfull_stride = 0;
  in.pose = w.in_pose; in.pose_stride = 0;
  if (he == hipSuccess) he = mp_localize_prepare(L, s, in, (int)n, st, pf);
  if ((rc = sync_or_fail(x, he, who))) return rc;
  return localize_finish(x, who, in, (int)n, std::max(cnt[0], cnt[1]), nullptr, "map_localize_d2h", out);
}

// ------------------------------------------------------------------ scoring pose guesses
// n poses of one sweep against the whole streaming map, which is only read (score.hpp).  The host
// reads the map's sizes once (to size the index), then the results.
extern "C" int loam_map_score(loam_ctx* x, const loam_cloud_out* corner, const loam_cloud_out* surf, float max_dist,
                              uint32_t n, const loam_pose6* pose, loam_score_result* out) {
  static_assert(LOAM_SCORE_MAX == kScoreMax, "loam.h and score.hpp");
  static_assert(sizeof(loam_score_result) == 32, "loam_score_result layout");
  if (!x || !corner || !surf || !pose || !out) return fail(LOAM_E_INVAL, "null argument");
  const std::string who = "loam_map_score";
  if (n == 0 || n > LOAM_SCORE_MAX) return fail(LOAM_E_INVAL, who + ": n must be in [1, LOAM_SCORE_MAX]");
  int rc = score_max_dist_refused(who, max_dist);
  if (rc) return rc;
  if ((corner->count && !corner->pts) || (surf->count && !surf->pts))
    return fail(LOAM_E_INVAL, who + ": a cloud's pts is null");
  if (corner->count > (uint32_t)x->cap || surf->count > (uint32_t)x->cap)
    return fail(LOAM_E_INVAL, who + ": a cloud exceeds max_points");
  if ((rc = map_drain(x))) return rc;
  MpBuffers& b = x->mp1;
  MpScore& S = x->score;
  const int cnt[2] = {(int)corner->count, (int)surf->count};
  hipError_t he = mp_map_ensure(x->mio);
  if (he == hipSuccess) he = mp_score_reserve(S, std::max(cnt[0], cnt[1]));
  if (he != hipSuccess) return nomem(who + ": working set allocation failed: " + hipGetErrorString(he));
  hipStream_t st = x->st;
  std::memcpy(S.pose_h(), pose, (size_t)n * sizeof(loam_pose6));
  x->prof.begin(st);
  he = mp_map_table(b, x->mio, st, &x->prof);
  x->pin.reset();
  if (he == hipSuccess) he = x->pin.reserve((size_t)cnt[0] + cnt[1], st);
  if (he == hipSuccess) he = x->pin.up(st, S.q, corner->pts, (size_t)cnt[0]);
  if (he == hipSuccess) he = x->pin.up(st, S.q + S.cloud_cap, surf->pts, (size_t)cnt[1]);
  if (he == hipSuccess) he = hipMemcpyAsync(S.pose, S.pose_h(), (size_t)n * sizeof(loam_pose6), hipMemcpyHostToDevice, st);
  x->prof.mark("map_score_h2d");
  if ((rc = sync_or_fail(x, he, who))) return rc;
  int nC = 0, total = 0;
  if ((rc = score_map_sizes(x, who, &nC, &total))) return rc;
  if ((rc = score_reserve_index(x, who, nC, total, cnt[0], cnt[1], (int)n))) return rc;
  const bool count = x->prof.on;  // (with profiling the reduction also adds up the points and buckets the searches read)
  he = mp_score_run(S, b, x->mio, nC, total, cnt[0], cnt[1], max_dist * max_dist, (int)n, count, st, &x->prof);
  if ((rc = sync_or_fail(x, he, who))) return rc;
  x->prof.collect();
  if (count) score_count_work(x, (double)n * ((double)S.res_h()[0].corner_scored + (double)S.res_h()[0].surf_scored));
  std::memcpy(out, S.res_h(), (size_t)n * sizeof(loam_score_result));
  return LOAM_OK;
}
