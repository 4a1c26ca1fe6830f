// The host engine's private header: struct loam_ctx and the host helpers that more than one of the
// engine's translation units needs.  Included only by engine.cpp (create / destroy, tuning, the
// streaming nodes, k_xfer), engine_batch.cpp (loam_batch_*), engine_map.cpp (export / import,
// localize, score) and engine_lanes.cpp (loam_lanes_*); never by a kernel file or a caller.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/loam/loam.h"
#include "dev_hooks.h"
#include "engine.hpp"
#include "lanes.hpp"
#include "mp.hpp"
#include "od.hpp"
#include "point_fields.hpp"
#include "pose_math.hpp"
#include "score.hpp"

using namespace loam;  // (as the engine's files have it: loam_ctx names the kernels' types unqualified)

constexpr size_t kMetaBytes = 8192;  // (loam_ctx::meta)

struct loam_ctx {
  loam_config cfg;
  int device = 0;
  hipStream_t st = nullptr;
  int R = 16, cap = 40000;
  // scan registration (streaming)
  int sr_init_count = 0;
  bool sr_inited = false;
  SrBuffers sr1;        // one sweep
  SrRingTab ring_tab;   // the ring model's tangent thresholds (sr_params)
  // loam_set_ring_table: the table that replaced cfg.ring_model (tb_n = 0: none), allowed until the
  // context has seen a sweep
  int tb_n = 0;
  float tb_bound[LOAM_RING_TABLE_MAX + 1];
  int32_t tb_ring[LOAM_RING_TABLE_MAX];
  bool seen_sweep = false;
  // loam_set_point_fields: ring, or ring and time, from the records' own fields
  // (pf.on = 0: none, the ring model or table rules); pf_map_d: the map for the device push's gather
  PointFields pf;
  int16_t* pf_map_d = nullptr;
  SrBuffers odin;       // odometry input feature set (host topics uploaded here)
  OdBuffers od1;        // one odometry problem
  bool od_inited = false;
  int od_last = 0, od_frame_count = 1;  // frameCount = skipFrameNum (src/laserOdometry.cpp:407)
  float od_sum[6] = {0, 0, 0, 0, 0, 0};  // transformSum: the streaming path accumulates it on the host
  MpBuffers mp1;        // streaming map
  int map_frame_count = 4;    // mapFrameCount = mapFrameNum - 1 (src/laserMapping.cpp:405)
  bool surround_due = false;  // the last loam_mapping frame publishes /laser_cloud_surround
  // IMU (loam_imu): scanRegistration's queue (host master copy, uploaded per sweep) and
  // laserMapping's queue
  loamimu::SrQueue* sr_imu = nullptr;     // host
  loamimu::SrQueue* sr_imu_dev = nullptr; // device
  loamimu::MpQueue mp_imu;
  double imu_last_stamp = -1e300;
  // batch (config 4)
  int P = 0;
  SrBuffers srb;
  // tune.sr_ahead: the next step's scan registration runs one step ahead on st3, into the other of
  // two buffer sets, as soon as the step that last read that set has finished (step_done); the
  // step that consumes it waits on sr_done.  The raw sweeps are uploaded into both sets.
  SrBuffers srb2;
  hipStream_t st3 = nullptr;
  hipEvent_t sr_done = nullptr, step_done[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ahead_at = nullptr;  // the point of this step after which it may start (tune.sr_ahead_at)
  // ... followed by the next step's odometry seed (Last[0] and its hashes, into the other istate
  // set), once this step's second mapping frame begins (the odometry no longer reads Last[0])
  hipEvent_t seed_at = nullptr, seed_done = nullptr;
  bool seed_ready = false;
  // tune.step_pipe: consecutive steps overlap — the odometry of a step (st) beside the mapping of the
  // previous one (st4), the scan registration + seed of the next (st3); hand-offs by events (batch_enqueue_pipe)
  hipStream_t st4 = nullptr;
  hipEvent_t od_done = nullptr, mp1_done = nullptr, a_start = nullptr, b_last = nullptr;
  hipEvent_t mp1_read = nullptr;  // frame 1 has read Last[s] (after its k_mp_stack)
  // per SR set (slot) of the step pipeline: frame 2 of the step reading set i has read Last[e]; that
  // step's mapping is done (the set's last reader)
  hipEvent_t inputs_read[3] = {nullptr, nullptr, nullptr};
  hipEvent_t mp_done[3] = {nullptr, nullptr, nullptr};
  bool mp_done_rec[3] = {false, false, false}, inputs_read_rec[3] = {false, false, false}, b_used = false;
  // the Last buffers (OdBuffers, kOdBufs of them) of the next step: its seed's (od_s, the odometry's
  // Last) and its TransformToEnd's (od_e, frame 2's input).  The step pipeline rotates (s, e) ->
  // (3 - s - e, s), so the next seed writes the buffer no running step reads and never waits for the
  // odometry; batch_enqueue keeps them.  od_s_last: the seed buffer of the last enqueued step.
  int od_s = 0, od_e = 1, od_s_last = 0;
  bool step_done_rec[3] = {false, false, false};
  int sr_idx = 0;         // the set the next step reads
  bool sr_ready = false;  // its scan registration is already enqueued (st3, sr_done)
  int srb_last = 0;       // the set of the last enqueued step (loam_batch_download)
  // tune.pipe_sr_sets = 3: the step pipeline rotates three SR sets (and odometry state sets), so a
  // step's scan registration waits for the mapping of the step three back, not two
  SrBuffers srb3;
  SrBuffers& srbuf(int i) { return i == 2 ? srb3 : (i ? srb2 : srb); }
  int pipe_k = 0;         // pipelined steps since the last drain (their mapping sets alternate by parity)
  MpBuffers mpb2;         // the second mapping set: the step pipeline's steps alternate (mpbuf)
  MpBuffers& mpbuf(int i) { return i ? mpb2 : mpb; }
  int mp_last = 0;        // the mapping set of the last enqueued step (loam_batch_download)
  // loam_batch_feed: each pipelined step's sweeps arrive from the host through the SR set the step
  // reads (copied on st3 behind that set's previous reader, then its scan registration + seed
  // there); a fed context enqueues nothing ahead at the end of a run (the feed does)
  bool fed = false;
  float4* feed_pin[3] = {nullptr, nullptr, nullptr};  // pinned staging per SR set: the sweeps back to back
  int* feed_n[3] = {nullptr, nullptr, nullptr};       // pinned sweep sizes per SR set, [2P], then offsets [2P]
  float4* feed_dev = nullptr;                         // device staging of the packed sweeps, [2P][cap] points
  int* feed_doff = nullptr;                           // device sizes + offsets, [4P]
  hipEvent_t feed_copied[3] = {nullptr, nullptr, nullptr};
  bool feed_rec[3] = {false, false, false};
  void free_feed() {
    for (int i = 0; i < 3; ++i) {
      if (feed_rec[i]) (void)hipEventSynchronize(feed_copied[i]);
      if (feed_pin[i]) (void)hipHostFree(feed_pin[i]);
      if (feed_n[i]) (void)hipHostFree(feed_n[i]);
      feed_pin[i] = nullptr;
      feed_n[i] = nullptr;
      feed_rec[i] = false;
    }
    if (feed_dev) (void)hipFree(feed_dev);
    if (feed_doff) (void)hipFree(feed_doff);
    feed_dev = nullptr;
    feed_doff = nullptr;
  }
  bool batch_ran = false;  // a loam_batch_run since the last loam_batch_upload (loam_batch_features)
  // loam_batch_features: the offset table of the selected sweeps (device, and its pinned host copy)
  // and the bounded staging its packed chunks go through, two device pack buffers and two pinned
  // host buffers of kPackStagePts points used alternately.  Allocated by the first call for the
  // uploaded batch size (pack_S sweeps), freed with the batch's other buffers.
  uint64_t* pack_table = nullptr;
  uint64_t* pack_table_h = nullptr;
  float4* pack_dev[2] = {nullptr, nullptr};
  float4* pack_pin[2] = {nullptr, nullptr};
  hipEvent_t pack_done[2] = {nullptr, nullptr};
  int pack_S = 0;
  MapIo mio;  // loam_map_export / loam_map_import: their small tables (the points go through pack_dev / pack_pin)
  MpLoc loc;  // loam_map_localize: the candidates' working set, allocated by the first call, kept until loam_destroy
  MpScore score;  // loam_map_score: the query clouds, the pose / result tables and the map index, likewise
  Lanes lanes;    // loam_lanes_*: S sequences in lockstep, their own working set (lanes.hpp); S = 0 until loam_lanes_open
  void free_pack_table() {
    if (pack_table) (void)hipFree(pack_table);
    if (pack_table_h) (void)hipHostFree(pack_table_h);
    pack_table = pack_table_h = nullptr;
    pack_S = 0;
  }
  void free_pack() {  // (the call that used them has drained its work)
    free_pack_table();
    for (int i = 0; i < 2; ++i) {
      if (pack_dev[i]) (void)hipFree(pack_dev[i]);
      if (pack_pin[i]) (void)hipHostFree(pack_pin[i]);
      if (pack_done[i]) (void)hipEventDestroy(pack_done[i]);
      pack_dev[i] = pack_pin[i] = nullptr;
      pack_done[i] = nullptr;
    }
    pack_S = 0;
  }
  void reset_ahead() {    // (after draining st3 / st4)
    sr_ready = false;
    seed_ready = false;
    for (int i = 0; i < 3; ++i) mp_done_rec[i] = inputs_read_rec[i] = false;
    b_used = false;
    sr_idx = srb_last = pipe_k = 0;
    batch_ran = false;  // (srb_last no longer names the set of the last run: loam_batch_features waits for the next)
    step_done_rec[0] = step_done_rec[1] = step_done_rec[2] = false;
  }
  OdBuffers odb;
  MpBuffers mpb;
  std::vector<float4> stage;
  Staging pin;                  // pinned staging of the node calls' host clouds
  // pinned scratch (8 KB) for the node calls' host-side small values, as ints:
  //   odometry           [8..19] imu_trans, [24..27]
  //                      init-frame Last counts (downloaded), [32 ..) the host copy of the
  //                      state / istate / nlast / nfullEnd download (from xb)
  // Every other small transfer of a node call goes through k_xfer (xfer.hpp): host values in its
  // arguments, device values into xb (scan registration, odometry and mapping regions)
  char* meta = nullptr;
  XferBuf xb;          // mapped, coherent host block for k_xfer's downloads (xfer.hpp regions)
  StreamIo io() { StreamIo s; s.meta = meta; s.xb = xb; s.e0 = ev[4]; s.e1 = ev[5]; return s; }
  loam_stats stats;
  Prof prof;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipStream_t st2 = nullptr;                 // batch: mapping frame 1 beside the odometry solve
  hipEvent_t fork = nullptr, join = nullptr, fork2 = nullptr, join2 = nullptr;
  Tuning tune;                               // launch choices by batch size (loam_set_tuning)
  int prio = 0;                              // HIP priority of the context's streams (loam_set_stream_priority)
  // tune.graph: the batch step captured once as a HIP graph (for this P / these buffers) and replayed
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  int graph_P = 0;
  void drop_graph() {
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    if (graph) (void)hipGraphDestroy(graph);
    graph_exec = nullptr;
    graph = nullptr;
    graph_P = 0;
    for (int i = 0; i < 2; ++i) {
      if (od_graph_exec[i]) (void)hipGraphExecDestroy(od_graph_exec[i]);
      if (od_graph[i]) (void)hipGraphDestroy(od_graph[i]);
      od_graph_exec[i] = nullptr;
      od_graph[i] = nullptr;
    }
  }
  // tune.od_graph: the streaming odometry's L-M launches (od_solve) captured once per Last-buffer
  // parity and replayed (one host call instead of ~35 launches per frame)
  hipGraph_t od_graph[2] = {nullptr, nullptr};
  hipGraphExec_t od_graph_exec[2] = {nullptr, nullptr};
};

// The helpers live in loam::eng and are hidden: the shared library exports none of them.
#pragma GCC visibility push(hidden)
namespace loam {
namespace eng {

// sets the thread's loam_last_error() text (engine.cpp keeps it) and returns code
int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess)                                                          \
      return fail(LOAM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));  \
  } while (0)

inline FeatView feat_view(const SrBuffers& b, int first, int step) {
  FeatView v;
  const size_t R = b.R;
  v.sharp = b.sharp + (size_t)first * kSharpPerRing * R;
  v.lsharp = b.lsharp + (size_t)first * kLessSharpPerRing * R;
  v.flat = b.flat + (size_t)first * kFlatPerRing * R;
  v.lflat = b.lflat + (size_t)first * b.cap;
  v.full = b.full + (size_t)first * b.cap;
  v.sharp_stride = (size_t)step * kSharpPerRing * R;
  v.lsharp_stride = (size_t)step * kLessSharpPerRing * R;
  v.flat_stride = (size_t)step * kFlatPerRing * R;
  v.lflat_stride = (size_t)step * b.cap;
  v.full_stride = (size_t)step * b.cap;
  v.cnt = b.cnt + (size_t)first * 4;
  v.cnt_stride = 4 * step;
  v.nfull_p = b.n_full + first;
  v.nfull_stride = step;
  return v;
}

inline SrParams sr_params(const loam_ctx* c) {
  SrParams p;
  p.R = c->R;
  // (any cfg.ring_model but LOAM_RING_LINEAR has always meant the VLP-16 rule; a table comes only
  // through loam_set_ring_table)
  p.ring_model = c->tb_n ? LOAM_RING_TABLE : (c->cfg.ring_model == LOAM_RING_LINEAR ? LOAM_RING_LINEAR : LOAM_RING_VLP16);
  p.ring_lo = c->cfg.ring_lo_deg;
  p.ring_hi = c->cfg.ring_hi_deg;
  c->ring_tab.fill(p);  // (a table's bounds and rings too: the device copies)
  // (fields set: the model or table above is kept but not consulted; the ring kernels' field
  // instantiations read the word pack() or the device push's gather left in raw's w)
  if (c->pf.on) p.ring_model = c->pf.time_type != LOAM_FIELD_NONE ? kRingSrcFieldTime : kRingSrcField;
  return p;
}

// ---- engine.cpp
// pf: the context's point fields (every record must reach the end of both)
int check_cloud_in(const loam_cloud_in& c, int cap, const PointFields& pf);
// points [i0, i1) of c into dst[i0 ..) as float4; with fields set, w is the point's word (point_fields.hpp)
void pack(const loam_cloud_in& c, float4* dst, size_t i0, size_t i1, const PointFields& pf);
// device cloud -> caller storage through the pinned arena (completed by pin.finish() after a sync)
int copy_out(hipStream_t st, Staging& pin, const float4* dev, int n, loam_cloud_out* o);
int sr_errors(int e);
void count_bytes(loam_stats& s);

// sweeps [s0, s1) (sweep s = sweep(s)) packed back to back (sweep s at off[s]) into dst, on up to eight threads
template <class Sweep>
void pack_tight_of(Sweep sweep, size_t s0, size_t s1, const int* off, float4* dst, const PointFields& pf) {
  auto run = [&](size_t a, size_t b) {
    for (size_t s = a; s < b; ++s) {
      const loam_cloud_in& c = sweep(s);
      pack(c, dst + off[s], 0, c.count, pf);
    }
  };
  const size_t S = s1 - s0;
  const unsigned hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
  const size_t nt = S >= 64 ? hw : 1;
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; ++t) th.emplace_back(run, s0 + S * t / nt, s0 + S * (t + 1) / nt);
  run(s0, s0 + S / nt);
  for (auto& t : th) t.join();
}

// ---- engine_batch.cpp: the bounded download / upload staging (pack_dev / pack_pin), shared by
// loam_batch_features, the map export / import and the lanes' cloud downloads
// points of one staging buffer (32 MiB): a chunk of the packed clouds is at most this large
constexpr size_t kPackStagePts = (size_t)1 << 21;
size_t pack_sweep_max(const loam_ctx* x);
int ensure_pack_stage(loam_ctx* x, const char* what);
void copy_wide(void* dst, const void* src, size_t bytes);

// ---- engine_map.cpp
int map_drain(loam_ctx* x);
int map_export_of(loam_ctx* x, MpBuffers& b, int inst, int phase, loam_map* out);
int map_import_args(const loam_map* in, const std::string& who);
int map_import_bin(loam_ctx* x, MpBuffers& b, const loam_map* in, const std::string& who, uint64_t* dropped, int* kept);
void loc_result_of(const int* r, loam_localize_result& o);
// he, or the result of synchronising x->st when he is hipSuccess; on an error the stream is
// synchronised (again), the profile interval collected and the call fails with who + ": " + HIP's text
int sync_or_fail(loam_ctx* x, hipError_t he, const std::string& who);
// a failed allocation or reservation: LOAM_E_NOMEM with msg, and HIP's last error cleared (left set,
// the hipGetLastError that ends an unrelated later step would report it)
int nomem(const std::string& msg);
// the refusal of a store whose last update overflowed (ERR_CAP_MAP)
int store_invalid(const std::string& who);
// rows candidate rows of 12 floats at dst: (aft[h], bef ? bef[h] : zeros)
void cand_rows(float* dst, size_t rows, const loam_pose6* aft, const loam_pose6* bef);
// loam_map_localize / loam_lanes_localize behind the synchronised mp_localize_prepare: the head
// check, the FromMap part's reservation, mp_localize_solve (lr: the lanes' rows, null for the one
// sweep `in`), the results into out[0..rows).  in_max: the largest input cloud; mark: the profile
// segment the solve's tail is booked under
int localize_finish(loam_ctx* x, const std::string& who, const MpInput& in, int rows, int in_max, const LocRows* lr,
                    const char* mark, loam_localize_result* out);
// loam_map_score / loam_lanes_score: the max_dist rule; the map table mp_map_table left in
// x->mio.tab_h (nC corner points of total, or the store's refusal); the index reservation; with
// profiling, the three work counters (queries: the scored points over all poses)
int score_max_dist_refused(const std::string& who, float max_dist);
int score_map_sizes(loam_ctx* x, const std::string& who, int* nC, int* total);
int score_reserve_index(loam_ctx* x, const std::string& who, int nC, int total, int cnt_c, int cnt_s, int rows);
void score_count_work(loam_ctx* x, double queries);

}  // namespace eng
}  // namespace loam
#pragma GCC visibility pop

using namespace loam::eng;
