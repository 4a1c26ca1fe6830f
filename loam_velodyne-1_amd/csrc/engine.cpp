// libloam_hip: host engine behind the C-ABI of include/loam/loam.h.
//
// A context owns one HIP device, one stream and the device-resident state the four reference
// nodes keep in globals: the scan-registration delay counter, the odometry transform / Last
// clouds / their voxel hashes, and the mapping cube store.  Every entry point uploads the
// caller's host cloud(s), runs the kernels of sr.hip / od.hip / mp.hip on the context stream and
// copies the results back; nothing here computes a point on the CPU (a missing GPU or kernel
// image fails loudly with LOAM_E_HIP).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstddef>
#include <algorithm>
#include <cmath>
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
#include "pose_math.hpp"
#include "score.hpp"

#ifdef LOAM_PIPE_TRACE
// Diagnostic builds only (tools/build_variant.sh NAME -DLOAM_PIPE_TRACE): device timestamps of the
// step pipeline's stages (events recorded on the stage's stream), printed by loam_batch_sync as
// "step stage start_us end_us" relative to the first event, to see which hand-off paces the steps.
namespace {
struct PipeTrace {
  struct Mark { int step; const char* stage; hipEvent_t a, b; };
  std::vector<Mark> marks;
  int step = 0;
  void begin(const char* stage, hipStream_t st) {
    Mark m{step, stage, nullptr, nullptr};
    (void)hipEventCreate(&m.a);
    (void)hipEventCreate(&m.b);
    (void)hipEventRecord(m.a, st);
    marks.push_back(m);
  }
  void end(const char* stage, hipStream_t st) {
    for (auto it = marks.rbegin(); it != marks.rend(); ++it)
      if (!std::strcmp(it->stage, stage) && it->step == step) { (void)hipEventRecord(it->b, st); return; }
  }
  void dump() {
    if (marks.empty()) return;
    for (auto& m : marks) {
      float a = 0, b = 0;
      if (!m.a || !m.b) continue;
      (void)hipEventElapsedTime(&a, marks[0].a, m.a);
      (void)hipEventElapsedTime(&b, marks[0].a, m.b);
      std::fprintf(stderr, "PIPE %d %s %.1f %.1f\n", m.step, m.stage, 1e3 * a, 1e3 * b);
    }
    for (auto& m : marks) {
      if (m.a) (void)hipEventDestroy(m.a);
      if (m.b) (void)hipEventDestroy(m.b);
    }
    marks.clear();
  }
};
PipeTrace g_pt;
}  // namespace
#define PT_BEGIN(s, st) g_pt.begin(s, st)
#define PT_END(s, st) g_pt.end(s, st)
#else
#define PT_BEGIN(s, st) ((void)0)
#define PT_END(s, st) ((void)0)
#endif

using namespace loam;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess)                                                          \
      return fail(LOAM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));  \
  } while (0)

FeatView feat_view(const SrBuffers& b, int first, int step) {
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

}  // namespace

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

namespace {

int check_cloud_in(const loam_cloud_in& c, int cap) {
  if (c.count > 0 && c.data == nullptr) return fail(LOAM_E_INVAL, "cloud data is null");
  if (c.stride_bytes < 12 || c.stride_bytes % 4 != 0) return fail(LOAM_E_INVAL, "bad stride_bytes");
  if (c.count > (uint32_t)cap) return fail(LOAM_E_CAPACITY, "cloud exceeds max_points");
  return LOAM_OK;
}

// (records need not be 4-byte aligned: a PointCloud2's data follows a variable-length header in
// the message, and loam_pc2_cloud hands it over in place)
// points [i0, i1) of c into dst[i0 ..) as float4 (w is not read by the device: a 16-byte stride
// is copied as is)
void pack(const loam_cloud_in& c, float4* dst, size_t i0, size_t i1) {
  const char* base = (const char*)c.data;
  if (c.stride_bytes == 16) {
    std::memcpy(dst + i0, base + i0 * 16, (i1 - i0) * 16);
    return;
  }
  for (size_t i = i0; i < i1; ++i) {
    float q[3];
    std::memcpy(q, base + i * c.stride_bytes, sizeof(q));
    dst[i] = make_float4(q[0], q[1], q[2], 0.0f);
  }
}

// sweeps [s0, s1) (sweep s = sweep(s)) packed back to back (sweep s at off[s]) into dst, on up to eight threads
template <class Sweep>
void pack_tight_of(Sweep sweep, size_t s0, size_t s1, const int* off, float4* dst) {
  auto run = [&](size_t a, size_t b) {
    for (size_t s = a; s < b; ++s) {
      const loam_cloud_in& c = sweep(s);
      pack(c, dst + off[s], 0, c.count);
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

// device cloud -> caller storage through the pinned arena (completed by pin.finish() after a sync)
int copy_out(hipStream_t st, Staging& pin, const float4* dev, int n, loam_cloud_out* o) {
  if (o == nullptr) return LOAM_OK;
  if ((uint32_t)n > o->capacity) {
    o->count = (uint32_t)n;
    return fail(LOAM_E_CAPACITY, "output cloud capacity too small");
  }
  o->count = (uint32_t)n;
  if (n > 0) HIP_TRY(pin.down(st, o->pts, dev, (size_t)n));
  return LOAM_OK;
}

int upload_cloud(hipStream_t st, Staging& pin, const loam_cloud_out& c, float4* dev, int cap) {
  if (c.count > (uint32_t)cap) return fail(LOAM_E_CAPACITY, "input feature cloud exceeds capacity");
  if (c.count > 0) {
    if (c.pts == nullptr) return fail(LOAM_E_INVAL, "feature cloud pts is null");
    HIP_TRY(pin.up(st, dev, c.pts, (size_t)c.count));
  }
  return LOAM_OK;
}

int sr_errors(int e) {
  if (e & ERR_EMPTY) return fail(LOAM_E_INVAL, "sweep has no finite point");
  if (e & ERR_CAP_RING) return fail(LOAM_E_CAPACITY, "a ring span exceeds the per-ring capacity");
  return LOAM_OK;
}

SrParams sr_params(const loam_ctx* c) {
  SrParams p;
  p.R = c->R;
  p.ring_model = (int)c->cfg.ring_model;
  p.ring_lo = c->cfg.ring_lo_deg;
  p.ring_hi = c->cfg.ring_hi_deg;
  c->ring_tab.fill(p);
  return p;
}

void count_bytes(loam_stats& s) {
  // algorithmic bytes, SURVEY.md §8(d)
  s.bytes_sr = 16 * s.n_raw + 32 * s.n_ring + 16 * (s.n_sharp + s.n_less_sharp + s.n_flat + s.n_less_flat);
  s.bytes_od = 16 * s.od_assoc_points + 16 * s.od_queries + 12 * s.od_queries + 32 * s.od_rows_sum;
  s.bytes_mp = 16 * s.mp_map_points + 96 * s.mp_stack_iters + 64 * s.mp_rows_sum + 32 * s.mp_stack +
               32 * s.mp_map_valid_points;
}

}  // namespace

namespace loam {
void set_last_error(const std::string& msg) { g_err = msg; }
}  // namespace loam

extern "C" {

const char* loam_last_error(void) { return g_err.c_str(); }

void loam_config_default(loam_config* d) {
  std::memset(d, 0, sizeof(*d));
  d->n_rings = 16;
  d->ring_model = LOAM_RING_VLP16;
  d->ring_lo_deg = -24.8f;
  d->ring_hi_deg = 2.0f;
  d->system_delay = 20;
  d->max_points = 40000;
  d->od_max_iter = 25;
  d->mp_max_iter = 10;
  d->skip_frame_num = 1;
  d->map_capacity = 1u << 21;
}

int loam_create(loam_ctx** out, const loam_config* cfg, int device) {
  if (out == nullptr) return fail(LOAM_E_INVAL, "out is null");
  *out = nullptr;
  loam_config c;
  if (cfg) c = *cfg;
  else loam_config_default(&c);
  if (c.n_rings < 2 || c.n_rings > 64) return fail(LOAM_E_INVAL, "n_rings must be in [2, 64]");
  if (c.max_points < 64 || c.max_points > (1u << 22)) return fail(LOAM_E_INVAL, "bad max_points");
  if (c.od_max_iter < 1 || c.od_max_iter > 1000 || c.mp_max_iter < 1 || c.mp_max_iter > 1000)
    return fail(LOAM_E_INVAL, "bad iteration limits");
  if (c.map_capacity < 1024 || c.map_capacity > (1u << 28))
    return fail(LOAM_E_INVAL, "map_capacity must be in [1024, 2^28] points");
  if (c.skip_frame_num > (1u << 20)) return fail(LOAM_E_INVAL, "bad skip_frame_num");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(LOAM_E_HIP, "no HIP device available (the engine has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(LOAM_E_INVAL, "bad device index");
  HIP_TRY(hipSetDevice(device));
  loam_ctx* x = new loam_ctx();
  x->cfg = c;
  x->device = device;
  x->R = (int)c.n_rings;
  x->cap = (int)c.max_points;
  x->od_frame_count = (int)c.skip_frame_num;
  std::memset(&x->stats, 0, sizeof(x->stats));
  if (hipStreamCreateWithFlags(&x->st, hipStreamNonBlocking) != hipSuccess) {
    delete x;
    return fail(LOAM_E_HIP, "hipStreamCreate failed");
  }
  hipError_t he = hipSuccess;
  for (auto& e : x->ev)
    if (he == hipSuccess) he = hipEventCreate(&e);
  if (he == hipSuccess && hipStreamCreateWithFlags(&x->st2, hipStreamNonBlocking) != hipSuccess) x->st2 = nullptr;
  // the batch pipeline's streams, created here with the first two: streams take the process's
  // GPU_MAX_HW_QUEUES hardware queues in creation order, and the four created together measured
  // 2.42 ms/step at the 8-GPU share against 3.13 when st3 / st4 came with the first batch (two
  // stages then shared a queue).  A context that never runs batches drops them (tuning
  // batch_streams = 0, the node pipeline's contexts), leaving the queues to the other contexts.
  if (he == hipSuccess && hipStreamCreateWithFlags(&x->st3, hipStreamNonBlocking) != hipSuccess) x->st3 = nullptr;
  if (he == hipSuccess && hipStreamCreateWithFlags(&x->st4, hipStreamNonBlocking) != hipSuccess) x->st4 = nullptr;
  if (he == hipSuccess) he = hipEventCreateWithFlags(&x->sr_done, hipEventDisableTiming);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&x->ahead_at, hipEventDisableTiming);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&x->seed_at, hipEventDisableTiming);
  for (hipEvent_t* e : {&x->od_done, &x->mp1_done, &x->inputs_read[0], &x->inputs_read[1], &x->inputs_read[2],
                        &x->a_start, &x->b_last, &x->mp_done[0], &x->mp_done[1], &x->mp_done[2], &x->mp1_read})
    if (he == hipSuccess) he = hipEventCreateWithFlags(e, hipEventDisableTiming);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&x->seed_done, hipEventDisableTiming);
  for (auto& e : x->step_done)
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e, hipEventDisableTiming);
  for (auto& e : x->feed_copied)
    if (he == hipSuccess) he = hipEventCreateWithFlags(&e, hipEventDisableTiming);
  x->pin.streams[0] = x->st;
  x->pin.streams[1] = x->st2;
  if (he == hipSuccess) he = hipEventCreateWithFlags(&x->fork, hipEventDisableTiming);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&x->join, hipEventDisableTiming);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&x->fork2, hipEventDisableTiming);
  if (he == hipSuccess) he = hipEventCreateWithFlags(&x->join2, hipEventDisableTiming);
  if (he != hipSuccess) {
    loam_destroy(x);
    return fail(LOAM_E_HIP, std::string("event creation failed: ") + hipGetErrorString(he));
  }
  if (he == hipSuccess) he = sr_ring_tab_alloc(x->ring_tab, sr_params(x));
  if (he == hipSuccess) he = sr_alloc(x->sr1, 1, x->cap, x->R);
  if (he == hipSuccess) he = sr_alloc(x->odin, 1, x->cap, x->R);
  if (he == hipSuccess) he = od_alloc(x->od1, 1, x->R, x->cap, (int)c.od_max_iter);
  if (he == hipSuccess) he = mp_alloc(x->mp1, 1, x->R, x->cap, (int)c.map_capacity, (int)c.mp_max_iter);
  x->od1.tune = x->mp1.tune = x->tune;
  if (he == hipSuccess) he = hipMalloc(&x->sr_imu_dev, sizeof(loamimu::SrQueue));
  if (he != hipSuccess) x->sr_imu_dev = nullptr;
  if (he == hipSuccess) he = hipHostMalloc((void**)&x->meta, kMetaBytes, hipHostMallocDefault);
  if (he != hipSuccess) x->meta = nullptr;
  if (he == hipSuccess) he = hipHostMalloc((void**)&x->xb.h, kXferBytes, hipHostMallocCoherent | hipHostMallocMapped);
  if (he != hipSuccess) x->xb.h = nullptr;
  else std::memset(x->xb.h, 0, kXferBytes);  // (the deferred valid-point slots are read before written)
  if (he == hipSuccess) he = hipHostGetDevicePointer((void**)&x->xb.d, x->xb.h, 0);
  x->sr_imu = new loamimu::SrQueue();
  std::memset(x->sr_imu, 0, sizeof(loamimu::SrQueue));
  x->sr_imu->last = -1;
  std::memset(&x->mp_imu, 0, sizeof(x->mp_imu));
  x->mp_imu.last = -1;
  if (he == hipSuccess) he = hipDeviceSynchronize();
  if (he != hipSuccess) {
    loam_destroy(x);
    return fail(LOAM_E_NOMEM, std::string("device allocation failed: ") + hipGetErrorString(he));
  }
  *out = x;
  return LOAM_OK;
}

void loam_destroy(loam_ctx* x) {
  if (!x) return;
  (void)hipSetDevice(x->device);
  if (x->st) (void)hipStreamSynchronize(x->st);
  if (x->st2) (void)hipStreamSynchronize(x->st2);  // (a pipelined step's mapping set runs there)
  if (x->st3) (void)hipStreamSynchronize(x->st3);
  if (x->st4) (void)hipStreamSynchronize(x->st4);
  sr_ring_tab_free(x->ring_tab);
  sr_free(x->sr1);
  sr_free(x->odin);
  od_free(x->od1);
  mp_free(x->mp1);
  sr_free(x->srb);
  sr_free(x->srb2);
  sr_free(x->srb3);
  od_free(x->odb);
  mp_free(x->mpb);
  mp_free(x->mpb2);
  x->free_feed();
  x->free_pack();
  mp_map_free(x->mio);
  mp_loc_free(x->loc);
  mp_score_free(x->score);
  lanes_free(x->lanes);
  for (auto& e : x->feed_copied)
    if (e) (void)hipEventDestroy(e);
  if (x->sr_imu_dev) (void)hipFree(x->sr_imu_dev);
  if (x->meta) (void)hipHostFree(x->meta);
  if (x->xb.h) (void)hipHostFree(x->xb.h);
  x->pin.release();
  delete x->sr_imu;
  for (auto& e : x->ev)
    if (e) (void)hipEventDestroy(e);
  if (x->st2) (void)hipStreamSynchronize(x->st2);
  x->drop_graph();
  if (x->fork) (void)hipEventDestroy(x->fork);
  if (x->join) (void)hipEventDestroy(x->join);
  if (x->fork2) (void)hipEventDestroy(x->fork2);
  if (x->join2) (void)hipEventDestroy(x->join2);
  if (x->sr_done) (void)hipEventDestroy(x->sr_done);
  if (x->ahead_at) (void)hipEventDestroy(x->ahead_at);
  if (x->seed_at) (void)hipEventDestroy(x->seed_at);
  for (hipEvent_t e : {x->od_done, x->mp1_done, x->inputs_read[0], x->inputs_read[1], x->inputs_read[2], x->a_start,
                       x->b_last, x->mp_done[0], x->mp_done[1], x->mp_done[2], x->mp1_read})
    if (e) (void)hipEventDestroy(e);
  if (x->st4) (void)hipStreamDestroy(x->st4);
  if (x->seed_done) (void)hipEventDestroy(x->seed_done);
  for (auto& e : x->step_done)
    if (e) (void)hipEventDestroy(e);
  if (x->st3) (void)hipStreamDestroy(x->st3);
  if (x->st2) (void)hipStreamDestroy(x->st2);
  if (x->st) (void)hipStreamDestroy(x->st);
  delete x;
}

namespace {
// the context's streams recreated at priority prio, in loam_create's order (st, st2, st3, st4: streams take the process's
// hardware queues in creation order); the batch pipeline's two only when the context keeps them
// (tuning batch_streams).  Drains the old streams first: a failure leaves the context on them.
int remake_streams(loam_ctx* x, int prio) {
  HIP_TRY(hipStreamSynchronize(x->st));
  if (x->st2) HIP_TRY(hipStreamSynchronize(x->st2));
  if (x->st3) HIP_TRY(hipStreamSynchronize(x->st3));
  if (x->st4) HIP_TRY(hipStreamSynchronize(x->st4));
  const bool batch = x->st3 != nullptr || x->st4 != nullptr;
  hipStream_t ns[4] = {nullptr, nullptr, nullptr, nullptr};
  hipError_t he = hipSuccess;
  for (int i = 0; i < (batch ? 4 : 2) && he == hipSuccess; ++i)
    he = hipStreamCreateWithPriority(&ns[i], hipStreamNonBlocking, prio);
  if (he != hipSuccess) {
    for (hipStream_t s : ns)
      if (s) (void)hipStreamDestroy(s);
    return fail(LOAM_E_HIP, "hipStreamCreateWithPriority failed (context keeps its old streams)");
  }
  for (hipStream_t s : {x->st, x->st2, x->st3, x->st4})
    if (s) (void)hipStreamDestroy(s);
  x->st = ns[0];
  x->st2 = ns[1];
  x->st3 = ns[2];
  x->st4 = ns[3];
  x->prio = prio;
  x->reset_ahead();
  x->drop_graph();  // (captured on the old streams)
  x->pin.streams[0] = x->st;
  x->pin.streams[1] = x->st2;
  return LOAM_OK;
}
}  // namespace

int loam_set_stream_priority(loam_ctx* x, int priority) {
  if (!x) return fail(LOAM_E_INVAL, "null argument");
  HIP_TRY(hipSetDevice(x->device));
  int least = 0, greatest = 0;  // HIP: a numerically lower value is a higher priority
  HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
  return remake_streams(x, priority > 0 ? greatest : priority < 0 ? least : 0);
}

int loam_set_tuning(loam_ctx* x, const char* key, long long value) {
  if (!x || !key) return fail(LOAM_E_INVAL, "null argument");
  Tuning t = x->tune;
  if (!t.set(key, value)) return fail(LOAM_E_INVAL, std::string("unknown tuning key or value out of range: ") + key);
  // (the streams below are created on the context's device, whatever device is current)
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipStreamSynchronize(x->st));
  if (x->st2) HIP_TRY(hipStreamSynchronize(x->st2));
  if (x->st3) HIP_TRY(hipStreamSynchronize(x->st3));
  if (x->st4) HIP_TRY(hipStreamSynchronize(x->st4));
  if (t.batch_streams) {
    // created before anything changes (at the context's stream priority, as
    // loam_set_stream_priority creates them): a failure leaves the context as it was
    hipStream_t n3 = x->st3, n4 = x->st4;
    if (!n3) HIP_TRY(hipStreamCreateWithPriority(&n3, hipStreamNonBlocking, x->prio));
    if (!n4) {
      const hipError_t e = hipStreamCreateWithPriority(&n4, hipStreamNonBlocking, x->prio);
      if (e != hipSuccess) {
        if (n3 != x->st3) (void)hipStreamDestroy(n3);
        return fail(LOAM_E_HIP, std::string("hipStreamCreateWithPriority: ") + hipGetErrorString(e));
      }
    }
    x->st3 = n3;
    x->st4 = n4;
  } else {  // (the batch then runs on st / st2 alone)
    if (x->st3) (void)hipStreamDestroy(x->st3);
    if (x->st4) (void)hipStreamDestroy(x->st4);
    x->st3 = x->st4 = nullptr;
  }
  x->tune = t;
  x->reset_ahead();
  x->drop_graph();  // (captured with the old choices)
  x->od1.tune = x->odb.tune = t;
  x->mp1.tune = x->mpb.tune = x->mpb2.tune = t;
  x->lanes.od.tune = x->lanes.mp.tune = lanes_tuning(t);
  return LOAM_OK;
}

int loam_get_tuning(loam_ctx* x, const char* key, long long* value) {
  if (!x || !key || !value) return fail(LOAM_E_INVAL, "null argument");
  if (!x->tune.get(key, value)) return fail(LOAM_E_INVAL, std::string("unknown tuning key: ") + key);
  return LOAM_OK;
}

int loam_set_profiling(loam_ctx* x, int on) {
  if (!x) return fail(LOAM_E_INVAL, "null argument");
  x->prof.on = on != 0;
  x->prof.acc.clear();
  return LOAM_OK;
}

int loam_get_kernel_times(loam_ctx* x, char* buf, uint32_t cap) {
  if (!x || !buf || cap == 0) return fail(LOAM_E_INVAL, "null argument");
  std::string s;
  for (auto& kv : x->prof.acc) {
    char line[256];
    std::snprintf(line, sizeof(line), "%s %.6f %ld\n", kv.first.c_str(), kv.second.first, kv.second.second);
    s += line;
  }
  if (s.size() + 1 > cap) return fail(LOAM_E_CAPACITY, "buffer too small");
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return LOAM_OK;
}

int loam_get_stats(loam_ctx* x, loam_stats* s) {
  if (!x || !s) return fail(LOAM_E_INVAL, "null argument");
  *s = x->stats;
  return LOAM_OK;
}

}  // extern "C"

namespace {
// ------------------------------------------------------------------ scanRegistration
// The laserCloudHandler body on ctx->sr1.  out == nullptr (the device-resident chain): the topics
// stay in sr1 for the odometry that follows; cnt5 (sharp, lessSharp, flat, lessFlat, full counts)
// and imu12 (/imu_trans) are returned either way.
// pending (the chain, optional): when the sweep needs no host work between the scan registration
// and the odometry (no IMU queue, no host outputs), the call returns once the kernels and the
// counts' download are enqueued, *pending = true: cnt5 are then read after the odometry's sync
// (sr_collect), and an error the scan registration reports is returned there (the odometry
// kernels it fed are undone: od_frame)
int sr_frame(loam_ctx* x, double stamp, const loam_cloud_in& raw, loam_features* out, int* cnt5, float* imu12,
             bool* pending = nullptr) {
  if (!x->sr_inited) {  // src/scanRegistration.cpp:213-219 (Q1)
    x->sr_init_count++;
    if (x->sr_init_count >= (int)x->cfg.system_delay) x->sr_inited = true;
    return fail(LOAM_E_NOT_READY, "inside systemDelay");
  }
  int rc = check_cloud_in(raw, x->cap);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(x->device));
  SrBuffers& b = x->sr1;
  const int n = (int)raw.count;
  x->pin.reset();
  HIP_TRY(x->pin.reserve((size_t)2 * n, x->st));
  float4* praw = x->pin.buf;  // the sweep packed straight into pinned memory
  float4* pfull = x->pin.buf + n;  // the early download of the full cloud (below)
  x->pin.off = (size_t)2 * n;
  // packed in chunks, each chunk's DMA overlapping the packing of the next
  constexpr size_t kPackChunk = 8192;
  for (size_t i0 = 0; i0 < (size_t)n; i0 += kPackChunk) {
    const size_t i1 = std::min((size_t)n, i0 + kPackChunk);
    pack(raw, praw, i0, i1);
    HIP_TRY(hipMemcpyAsync(b.raw + i0, praw + i0, (i1 - i0) * sizeof(float4), hipMemcpyHostToDevice, x->st));
  }
  {
    Xfer xp;
    xp.put(b.raw_n, &n, sizeof(int));
    HIP_TRY(xfer_launch(xp, x->st));
  }
  SrParams prm = sr_params(x);
  loamimu::SrQueue* q = x->sr_imu;
  const size_t tail = offsetof(loamimu::SrQueue, front);  // pointers, Start, Cur, FromStart
  if (q->last >= 0) {  // IMU de-skew (:286-349) with the queue as loam_imu left it
    HIP_TRY(hipMemcpyAsync(x->sr_imu_dev, q, sizeof(*q), hipMemcpyHostToDevice, x->st));
    prm.imu = x->sr_imu_dev;
    prm.time_scan = stamp;
  }
  HIP_TRY(hipEventRecord(x->ev[0], x->st));
  // /velodyne_cloud_2 is final once the rings are sorted: its n (>= the kept points) points come
  // down on the second stream, and reach the caller's buffer on the host, while the curvature /
  // pick / VoxelGrid kernels run
  // (only when the caller's buffer holds all n points: nfull <= n can then not fail on capacity)
  const bool early = out && x->st2 != nullptr && n > 0 && out->full.pts && (uint32_t)n <= out->full.capacity;
  sr_launch(b, prm, x->st, nullptr, early ? x->fork : nullptr);
  HIP_TRY(hipEventRecord(x->ev[1], x->st));
  HIP_TRY(hipGetLastError());
  if (early) {
    HIP_TRY(hipStreamWaitEvent(x->st2, x->fork, 0));
    HIP_TRY(hipMemcpyAsync(pfull, b.full, (size_t)n * sizeof(float4), hipMemcpyDeviceToHost, x->st2));
    HIP_TRY(hipEventRecord(x->join, x->st2));
  }
  if (q->last >= 0)
    HIP_TRY(hipMemcpyAsync((char*)q + tail, (const char*)x->sr_imu_dev + tail, sizeof(*q) - tail,
                           hipMemcpyDeviceToHost, x->st));
  // [1..4] counts, [5] nfull, [6] err into the mapped host block, one launch
  const int* mi = (const int*)(x->xb.h + kXferSr) - 1;
  {
    Xfer xg;
    xg.get(x->xb.d + kXferSr, b.cnt, 4 * sizeof(int));
    xg.get(x->xb.d + kXferSr + 16, b.n_full, sizeof(int));
    xg.get(x->xb.d + kXferSr + 20, b.err, sizeof(int));
    HIP_TRY(xfer_launch(xg, x->st));
  }
  HIP_TRY(hipGetLastError());
  if (pending && !out && q->last < 0) {  // (the chain: no sync here, sr_collect after the odometry)
    const float it[12] = {q->pitchStart, q->yawStart, q->rollStart, q->pitchCur, q->yawCur, q->rollCur,
                          q->shiftFSX,   q->shiftFSY, q->shiftFSZ,  q->veloFSX,  q->veloFSY, q->veloFSZ};
    std::memcpy(imu12, it, sizeof(it));
    for (int k = 0; k < 5; ++k) cnt5[k] = 0;
    *pending = true;
    return LOAM_OK;
  }
  HIP_TRY(hipStreamSynchronize(x->st));
  int cnt[4] = {mi[1], mi[2], mi[3], mi[4]};
  const int nfull = mi[5];
  rc = sr_errors(mi[6]);
  if (rc) {
    if (early) HIP_TRY(hipEventSynchronize(x->join));  // the arena is reused by the next call
    return rc;  // (nothing written to the caller's buffers)
  }
  if (early) {
    HIP_TRY(hipEventSynchronize(x->join));
    std::memcpy(out->full.pts, pfull, (size_t)nfull * sizeof(float4));
  }
  int e = 0;
  x->pin.reset();
  if (out) {
    if (early) {
      out->full.count = (uint32_t)nfull;
      if ((uint32_t)nfull > out->full.capacity) e |= fail(LOAM_E_CAPACITY, "output cloud capacity too small");
    } else {
      e |= copy_out(x->st, x->pin, b.full, nfull, &out->full);
    }
    e |= copy_out(x->st, x->pin, b.sharp, cnt[0], &out->sharp);
    e |= copy_out(x->st, x->pin, b.lsharp, cnt[1], &out->less_sharp);
    e |= copy_out(x->st, x->pin, b.flat, cnt[2], &out->flat);
    e |= copy_out(x->st, x->pin, b.lflat, cnt[3], &out->less_flat);
    HIP_TRY(hipStreamSynchronize(x->st));
    x->pin.finish();
  }
  // /imu_trans (:614-635)
  const float it[12] = {q->pitchStart, q->yawStart, q->rollStart, q->pitchCur, q->yawCur, q->rollCur,
                        q->shiftFSX,   q->shiftFSY, q->shiftFSZ,  q->veloFSX,  q->veloFSY, q->veloFSZ};
  if (out) std::memcpy(out->imu_trans, it, sizeof(it));
  std::memcpy(imu12, it, sizeof(it));
  for (int k = 0; k < 4; ++k) cnt5[k] = cnt[k];
  cnt5[4] = nfull;
  float ms = 0;
  (void)hipEventElapsedTime(&ms, x->ev[0], x->ev[1]);
  std::memset(&x->stats, 0, sizeof(x->stats));
  x->stats.n_raw = (uint64_t)n;
  x->stats.n_ring = (uint64_t)nfull;
  x->stats.n_sharp = cnt[0]; x->stats.n_less_sharp = cnt[1];
  x->stats.n_flat = cnt[2]; x->stats.n_less_flat = cnt[3];
  x->stats.ms_sr = ms;
  count_bytes(x->stats);
  return e ? LOAM_E_CAPACITY : LOAM_OK;
}

// a pending scan registration's results (sr_frame's pending mode), once the stream has been
// synchronised past them: its error code; cnt5 filled
int sr_collect(loam_ctx* x, int* cnt5) {
  const int* mi = (const int*)(x->xb.h + kXferSr) - 1;
  for (int k = 0; k < 4; ++k) cnt5[k] = mi[1 + k];
  cnt5[4] = mi[5];
  return sr_errors(mi[6]);
}

// ------------------------------------------------------------------ laserOdometry
// The laserOdometry loop body on the features fv (cnt: sharp, lessSharp, flat, lessFlat, full
// counts; imu: /imu_trans).  late_full: the full cloud is still on the host (message mode) and is
// staged while the L-M runs; nullptr when fv's full cloud is already on the device.  nl3 (optional):
// the published CornerLast / SurfLast / full-cloud counts, for a mapping on the device copies.
int od_frame(loam_ctx* x, const FeatView& fv, const int* cnt, const float* imu, const loam_cloud_out* late_full,
             loam_pose6* sum_out, loam_cloud_out* corner_last, loam_cloud_out* surf_last, loam_cloud_out* full_end,
             int* published, int* nl3, bool defer = false, bool sr_pending = false);
}  // namespace

extern "C" {
int loam_scan_registration(loam_ctx* x, double stamp, loam_cloud_in raw, loam_features* out) {
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  int cnt5[5];
  float imu12[12];
  return sr_frame(x, stamp, raw, out, cnt5, imu12);
}

int loam_odometry(loam_ctx* x, double stamp, const loam_features* in, loam_pose6* sum_out,
                  loam_cloud_out* corner_last, loam_cloud_out* surf_last, loam_cloud_out* full_end,
                  int* published) {
  (void)stamp;
  if (!x || !in || !published) return fail(LOAM_E_INVAL, "null argument");
  HIP_TRY(hipSetDevice(x->device));
  *published = 0;
  SrBuffers& fi = x->odin;
  const int R = x->R;
  if (in->sharp.count > (uint32_t)(kSharpPerRing * R) || in->flat.count > (uint32_t)(kFlatPerRing * R) ||
      in->less_sharp.count > (uint32_t)(kLessSharpPerRing * R))
    return fail(LOAM_E_CAPACITY, "feature cloud larger than scan registration can produce");
  if (in->full.count > (uint32_t)x->cap) return fail(LOAM_E_CAPACITY, "input feature cloud exceeds capacity");
  if (in->full.count > 0 && in->full.pts == nullptr) return fail(LOAM_E_INVAL, "feature cloud pts is null");
  int rc = 0;
  x->pin.reset();
  HIP_TRY(x->pin.reserve((size_t)in->sharp.count + in->less_sharp.count + in->flat.count + in->less_flat.count +
                             in->full.count, x->st));
  // only k_od_end reads the full cloud: after the first frame, with a second stream, it is staged
  // while the L-M kernels run (late_full below)
  const bool late = x->od_inited && x->st2 != nullptr && in->full.count > 0;
  if ((rc = upload_cloud(x->st, x->pin, in->sharp, fi.sharp, kSharpPerRing * R)) ||
      (rc = upload_cloud(x->st, x->pin, in->less_sharp, fi.lsharp, kLessSharpPerRing * R)) ||
      (rc = upload_cloud(x->st, x->pin, in->flat, fi.flat, kFlatPerRing * R)) ||
      (rc = upload_cloud(x->st, x->pin, in->less_flat, fi.lflat, x->cap)) ||
      (!late && (rc = upload_cloud(x->st, x->pin, in->full, fi.full, x->cap))))
    return rc;
  int cnt[5] = {(int)in->sharp.count, (int)in->less_sharp.count, (int)in->flat.count,
                (int)in->less_flat.count, (int)in->full.count};
  {
    Xfer xp;
    xp.put(fi.cnt, cnt, 4 * sizeof(int));
    xp.put(fi.n_full, &cnt[4], sizeof(int));
    HIP_TRY(xfer_launch(xp, x->st));
    HIP_TRY(hipGetLastError());
  }
  return od_frame(x, feat_view(fi, 0, 1), cnt, in->imu_trans, late ? &in->full : nullptr, sum_out, corner_last,
                  surf_last, full_end, published, nullptr);
}
}  // extern "C"

namespace {
int od_frame(loam_ctx* x, const FeatView& fv, const int* cnt, const float* imu_in, const loam_cloud_out* late_full,
             loam_pose6* sum_out, loam_cloud_out* corner_last, loam_cloud_out* surf_last, loam_cloud_out* full_end,
             int* published, int* nl3, bool defer, bool sr_pending) {
  *published = 0;
  OdBuffers& o = x->od1;
  SrBuffers& fi = x->odin;
  int* mi = (int*)x->meta;  // [8..19] imu_trans, [24..] downloads below
  std::memcpy(mi + 8, imu_in, 12 * sizeof(float));
  const bool late = late_full != nullptr;
  std::memset(&x->stats, 0, sizeof(x->stats));
  // imuTransHandler (:330-351): this sweep's /imu_trans, in the state order load_imu reads
  {
    Xfer xp;
    xp.put(o.state + kOdImu, mi + 8, 12 * sizeof(float));
    HIP_TRY(xfer_launch(xp, x->st));
  }
  HIP_TRY(od_wait_hashes(o, x->st));  // (the previous frame's hash build, when deferred)
  if (!x->od_inited) {  // src/laserOdometry.cpp:427-456: Last = raw lessSharp / lessFlat, no L-M
    // :451-452 transformSum[0] += imuPitchStart; transformSum[2] += imuRollStart (from zero)
    const float sum0[3] = {0.0f + imu_in[0], 0.0f, 0.0f + imu_in[2]};
    HIP_TRY(hipMemcpyAsync(o.state + kOdSum, sum0, sizeof(sum0), hipMemcpyHostToDevice, x->st));
    x->od_sum[0] = sum0[0];
    x->od_sum[2] = sum0[2];
    hipLaunchKernelGGL(k_od_end, dim3(16, 1), dim3(256), 0, x->st, o, fv, 0, 0, 0);
    od_build_hashes(o, 0, x->st);
    HIP_TRY(hipGetLastError());
    x->od_last = 0;
    x->od_inited = true;
    int* nl = mi + 24;
    HIP_TRY(hipMemcpyAsync(nl, o.nlast, 2 * sizeof(int), hipMemcpyDeviceToHost, x->st));
    HIP_TRY(hipStreamSynchronize(x->st));
    *published = LOAM_PUB_CLOUDS;
    if (nl3) { nl3[0] = nl[0]; nl3[1] = nl[1]; nl3[2] = 0; }
    x->pin.reset();
    int e = copy_out(x->st, x->pin, o.lastC, nl[0], corner_last) | copy_out(x->st, x->pin, o.lastS, nl[1], surf_last);
    HIP_TRY(hipStreamSynchronize(x->st));
    x->pin.finish();
    return e ? LOAM_E_CAPACITY : LOAM_OK;
  }
  const int cur = x->od_last, nxt = 1 - cur;
  HIP_TRY(hipEventRecord(x->ev[0], x->st));
  // the pose accumulation (:830-856) runs on the host after the download: one scalar chain of
  // double trig, which a one-thread kernel took ~16 us for (the batch path keeps it on the device)
  // sr_pending: k_od_begin keeps a copy of the state to undo this frame with (the third state slot,
  // unused by the one-problem context)
  OdBuffers ob = o;
  const bool graph = x->tune.od_graph && defer;  // (the chain: fv is the context's own sr1)
  if (sr_pending || graph) {  // (a graph bakes the copy in: every replayed frame keeps it)
    ob.bk_state = o.state_set[2];
    ob.bk_istate = o.istate_set[2];
  }
  if (graph) {
    if (!x->od_graph_exec[cur]) {
      HIP_TRY(hipStreamBeginCapture(x->st, hipStreamCaptureModeThreadLocal));
      od_solve(ob, fv, cur, x->st, nullptr, /*device_fini=*/false);
      hipGraph_t g = nullptr;
      const hipError_t ce = hipGetLastError(), ee = hipStreamEndCapture(x->st, &g);
      if (ce != hipSuccess || ee != hipSuccess) {
        if (g) (void)hipGraphDestroy(g);
        return fail(LOAM_E_HIP, std::string("odometry graph capture: ") + hipGetErrorString(ce != hipSuccess ? ce : ee));
      }
      x->od_graph[cur] = g;
      HIP_TRY(hipGraphInstantiate(&x->od_graph_exec[cur], g, nullptr, nullptr, 0));
    }
    HIP_TRY(hipGraphLaunch(x->od_graph_exec[cur], x->st));
  } else {
    od_solve(ob, fv, cur, x->st, nullptr, /*device_fini=*/false);
  }
  if (late) {  // late_full: host copy + DMA on the second stream, overlapping the L-M above
    HIP_TRY(x->pin.up(x->st2, fi.full, late_full->pts, (size_t)late_full->count));
    HIP_TRY(hipEventRecord(x->join, x->st2));
    HIP_TRY(hipStreamWaitEvent(x->st, x->join, 0));
  }
  const int frame_count0 = x->od_frame_count;
  x->od_frame_count++;
  const bool pub = x->od_frame_count >= (int)x->cfg.skip_frame_num + 1;
  hipLaunchKernelGGL(k_od_end, dim3(64, 1), dim3(256), 0, x->st, o, fv, nxt, 2, pub ? 1 : 0);  // one sweep: a wider grid
  // the new Last clouds' hash tables are read by the next frame's association only: with
  // stream_defer they are built on the second stream while this frame's results go out (and the
  // mapping runs)
  if (defer && x->tune.stream_defer && x->st2) HIP_TRY(od_build_hashes_deferred(o, nxt, x->st, x->st2));
  else od_build_hashes(o, nxt, x->st);
  HIP_TRY(hipEventRecord(x->ev[1], x->st));
  HIP_TRY(hipGetLastError());
  x->od_last = nxt;
  // state (kOdStateFloats), istate (kOdStateInts), nlast (4: problem 0's buffers 0 and 1, the two the
  // streaming path alternates), nfullEnd (2) into the mapped host
  // block in one launch, then copied out (the host edits st / ist below)
  static_assert(kXferOd + 4 * (kOdStateFloats + kOdStateInts + 6) <= kXferMp, "odometry transfer region");
  {
    Xfer xg;
    char* d = x->xb.d + kXferOd;
    xg.get(d, o.state, kOdStateFloats * sizeof(float));
    xg.get(d + 4 * kOdStateFloats, o.istate, kOdStateInts * sizeof(int));
    xg.get(d + 4 * (kOdStateFloats + kOdStateInts), o.nlast, 4 * sizeof(int));
    xg.get(d + 4 * (kOdStateFloats + kOdStateInts + 4), o.nfullEnd, 2 * sizeof(int));
    HIP_TRY(xfer_launch(xg, x->st));
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(x->st));
  int cnt_l[5];
  if (sr_pending) {  // the scan registration's result is known now
    const int src = sr_collect(x, cnt_l);
    cnt = cnt_l;
    if (src) {  // undo this frame: the state from k_od_begin's copy, the host counters (Last[nxt] unused)
      HIP_TRY(hipMemcpyAsync(o.state, o.state_set[2], kOdStateFloats * sizeof(float), hipMemcpyDeviceToDevice, x->st));
      HIP_TRY(hipMemcpyAsync(o.istate, o.istate_set[2], kOdStateInts * sizeof(int), hipMemcpyDeviceToDevice, x->st));
      HIP_TRY(hipStreamSynchronize(x->st));
      x->od_last = cur;
      x->od_frame_count = frame_count0;
      return src;
    }
  }
  float* st = (float*)(mi + 32);                  // kOdStateFloats
  int* ist = mi + 32 + kOdStateFloats;             // kOdStateInts
  int* nl = ist + kOdStateInts;                    // 4
  int* nfe = nl + 4;                               // 2
  std::memcpy(st, x->xb.h + kXferOd, 4 * (kOdStateFloats + kOdStateInts + 6));
  if (ist[kIsErr]) return fail(LOAM_E_CAPACITY, "odometry capacity exceeded");
  {  // :830-856 (k_od_fini's body, host side): transformSum from this frame's transform
    const float* q = imu_in;
    loampose::Imu m;
    m.pitchStart = q[0]; m.yawStart = q[1]; m.rollStart = q[2];
    m.pitchLast = q[3]; m.yawLast = q[4]; m.rollLast = q[5];
    m.shiftX = q[6]; m.shiftY = q[7]; m.shiftZ = q[8];
    m.veloX = q[9]; m.veloY = q[10]; m.veloZ = q[11];
    loampose::accumulate_pose(st, m, x->od_sum);
    ist[kIsQueries] = ist[kIsAssoc] * (cnt[0] + cnt[2]);
    // keep the device copy of transformSum current (it is seeded only on the init frame): the
    // host result goes back in k_xfer's arguments, ordered before the next frame's kernels
    Xfer xp;
    xp.put(o.state + kOdSum, x->od_sum, sizeof(loam_pose6));
    HIP_TRY(xfer_launch(xp, x->st));
    HIP_TRY(hipGetLastError());
  }
  if (sum_out) std::memcpy(sum_out, x->od_sum, sizeof(loam_pose6));
  *published = LOAM_PUB_POSE;
  int e = 0;
  if (pub) {
    x->od_frame_count = 0;
    *published |= LOAM_PUB_CLOUDS | LOAM_PUB_FULL;
    if (nl3) { nl3[0] = nl[nxt * 2 + 0]; nl3[1] = nl[nxt * 2 + 1]; nl3[2] = nfe[nxt]; }
    x->pin.reset();
    e |= copy_out(x->st, x->pin, o.lastC + (size_t)nxt * o.P * o.capC, nl[nxt * 2 + 0], corner_last);
    e |= copy_out(x->st, x->pin, o.lastS + (size_t)nxt * o.P * o.capS, nl[nxt * 2 + 1], surf_last);
    e |= copy_out(x->st, x->pin, o.fullEnd + (size_t)nxt * o.P * o.capS, nfe[nxt], full_end);
    HIP_TRY(hipStreamSynchronize(x->st));
    x->pin.finish();
  }
  float ms = 0;
  (void)hipEventElapsedTime(&ms, x->ev[0], x->ev[1]);
  x->stats.ms_od = ms;
  x->stats.od_iters = ist[kIsIters];
  x->stats.od_assoc_rounds = ist[kIsAssoc];
  x->stats.od_rows_sum = (uint64_t)ist[kIsRows];
  x->stats.od_queries = ist[kIsQueries];
  x->stats.od_degenerate_steps = (uint64_t)ist[kIsDegSteps];
  x->stats.od_nan_skips = (uint64_t)ist[kIsNanSkips];
  x->stats.od_assoc_gathered = (uint64_t)(uint32_t)ist[kIsGathered];
  x->stats.od_assoc_boxes = (uint64_t)(uint32_t)ist[kIsBoxes];
  {
    const uint64_t nq = ist[kIsAssoc] ? (uint64_t)(ist[kIsQueries] / ist[kIsAssoc]) : 0, it = (uint64_t)ist[kIsIters];
    x->stats.od_query_iters = nq * it;
    x->stats.od_row_evals = nq * it * (it + 1) / 2;
  }
  x->stats.od_corner_last = nl[cur * 2 + 0];
  x->stats.od_surf_last = nl[cur * 2 + 1];
  x->stats.od_assoc_points = (uint64_t)ist[kIsAssoc] * (nl[cur * 2 + 0] + nl[cur * 2 + 1]);
  count_bytes(x->stats);
  return e ? LOAM_E_CAPACITY : LOAM_OK;
}
}  // namespace

extern "C" {

// ------------------------------------------------------------------ laserMapping
int loam_mapping(loam_ctx* x, double stamp, const loam_pose6* odom_sum, const loam_cloud_out* corner_last,
                 const loam_cloud_out* surf_last, const loam_cloud_out* full_end, loam_pose6* aft,
                 loam_pose6* bef, loam_cloud_out* registered) {
  if (!x || !odom_sum || !corner_last || !surf_last || !full_end || !aft || !bef)
    return fail(LOAM_E_INVAL, "null argument");
  HIP_TRY(hipSetDevice(x->device));
  // transformUpdate's IMU blend (:199-226): roll / pitch at the odometry stamp + scanPeriod
  float rp[2];
  int front = 0;
  const bool have_imu = loamimu::mp_lookup(x->mp_imu, stamp, rp[0], rp[1], front);
  bool updated = false;
  const int rc = mp_stream_frame(x->mp1, x->st, *odom_sum, *corner_last, *surf_last, *full_end, aft, bef,
                                 registered, &x->stats, g_err, x->pin, x->io(), have_imu ? rp : nullptr, &updated,
                                 x->st2, x->join);
  if (have_imu && updated) x->mp_imu.front = front;  // the pointer walk happens inside transformUpdate
  x->surround_due = false;
  if (rc == LOAM_OK && ++x->map_frame_count >= 5) {  // :1038-1040
    x->map_frame_count = 0;
    x->surround_due = true;
  }
  return rc;
}

// ------------------------------------------------------------------ device-resident node chain
// scanRegistration -> laserOdometry -> laserMapping on one sweep with the intermediate topics left
// in device memory: odometry reads scanRegistration's buffers (sr1) in place and mapping reads
// odometry's published CornerLast / SurfLast / full-end buffers in place.  The arithmetic is the
// three node calls' own (the same kernels on the same values); only the host round trips of the
// intermediate clouds are gone, as in an intra-process (nodelet) deployment.
int loam_chain_sweep(loam_ctx* x, double stamp, loam_cloud_in raw, loam_chain_out* out) {
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  HIP_TRY(hipSetDevice(x->device));
  out->published = 0;
  out->mapped = 0;
  int cnt5[5];
  float imu12[12];
  // (stream_defer, after the odometry's first frame: the odometry is enqueued behind the scan
  // registration without a host round trip; sr_frame's pending mode)
  bool sr_pending = false;
  int rc = sr_frame(x, stamp, raw, nullptr, cnt5, imu12, x->od_inited && x->tune.stream_defer ? &sr_pending : nullptr);
  if (rc) return rc;
  int nl3[3] = {0, 0, 0};
  rc = od_frame(x, feat_view(x->sr1, 0, 1), cnt5, imu12, nullptr, &out->od_sum, nullptr, nullptr, nullptr,
                &out->published, nl3, /*defer=*/true, sr_pending);
  if (rc) return rc;
  if (out->published != (LOAM_PUB_POSE | LOAM_PUB_CLOUDS | LOAM_PUB_FULL)) return LOAM_OK;
  const OdBuffers& o = x->od1;
  const int nxt = x->od_last;  // od_frame swapped: the published Last is the current one
  MpInput in;
  in.corner = o.lastC + (size_t)nxt * o.P * o.capC;
  in.surf = o.lastS + (size_t)nxt * o.P * o.capS;
  in.full = o.fullEnd + (size_t)nxt * o.P * o.capS;
  in.corner_stride = o.capC; in.surf_stride = o.capS; in.full_stride = o.capS;
  in.ncorner = o.nlast + nxt * 2; in.nsurf = o.nlast + nxt * 2 + 1; in.nfull = o.nfullEnd + nxt;
  in.ncorner_stride = in.nsurf_stride = 2 * kOdBufs; in.nfull_stride = kOdBufs;
  in.pose = nullptr; in.pose_stride = 6;
  float rp[2];
  int front = 0;
  const bool have_imu = loamimu::mp_lookup(x->mp_imu, stamp, rp[0], rp[1], front);
  bool updated = false;
  loam_cloud_out* reg = out->registered.capacity ? &out->registered : nullptr;
  if (!reg) out->registered.count = 0;
  rc = mp_stream_frame_dev(x->mp1, x->st, out->od_sum, in, nl3, &out->aft, &out->bef, reg, &x->stats, g_err,
                           x->pin, x->io(), have_imu ? rp : nullptr, &updated, x->tune.stream_defer ? x->st2 : nullptr);
  if (have_imu && updated) x->mp_imu.front = front;
  x->surround_due = false;
  if (rc == LOAM_OK && ++x->map_frame_count >= 5) {  // :1038-1040
    x->map_frame_count = 0;
    x->surround_due = true;
  }
  if (rc == LOAM_OK) out->mapped = 1;
  return rc;
}

int loam_mapping_surround(loam_ctx* x, loam_cloud_out* out, int* published) {
  if (!x || !out || !published) return fail(LOAM_E_INVAL, "null argument");
  *published = 0;
  if (!x->surround_due) {
    out->count = 0;
    return LOAM_OK;
  }
  if (out->capacity && !out->pts) return fail(LOAM_E_INVAL, "surround cloud pts is null");
  HIP_TRY(hipSetDevice(x->device));
  const int rc = mp_stream_surround(x->mp1, x->st, out, g_err);
  if (rc == LOAM_OK) *published = 1;
  return rc;
}

// ------------------------------------------------------------------ IMU
int loam_imu(loam_ctx* x, double stamp, const double* quat_xyzw, const double* lin_acc_xyz) {
  if (!x || !quat_xyzw || !lin_acc_xyz) return fail(LOAM_E_INVAL, "null argument");
  if (!(stamp >= x->imu_last_stamp)) return fail(LOAM_E_INVAL, "IMU stamps must be non-decreasing");
  x->imu_last_stamp = stamp;
  double roll, pitch, yaw;
  loampose::rpy_from_quat(quat_xyzw, roll, pitch, yaw);  // tf::Matrix3x3(q).getRPY
  loamimu::sr_push(*x->sr_imu, stamp, roll, pitch, yaw, lin_acc_xyz);  // scanRegistration.cpp:638-660
  loamimu::mp_push(x->mp_imu, stamp, roll, pitch);                     // laserMapping.cpp:323-335
  return LOAM_OK;
}

// ------------------------------------------------------------------ transformMaintenance
int loam_maintenance(const loam_pose6* odom_sum, const loam_pose6* bef, const loam_pose6* aft,
                     loam_pose6* integrated) {
  if (!odom_sum || !bef || !aft || !integrated) return fail(LOAM_E_INVAL, "null argument");
  // src/transformMaintenance.cpp:147-203: Sum and Aft arrive as quaternion messages, Bef through
  // the twist fields; then transformAssociateToMap (:60-145).  Scalar host algebra, no kernel.
  float S[6], A[6], B[6], incre[6] = {0, 0, 0, 0, 0, 0}, T[6];
  loampose::pose_through_msg((const float*)odom_sum, S);
  loampose::pose_through_msg((const float*)aft, A);
  std::memcpy(B, bef, sizeof(B));
  loampose::associate_to_map(S, B, A, incre, T);
  std::memcpy(integrated, T, sizeof(T));
  return LOAM_OK;
}

// ------------------------------------------------------------------ batch (config 4)
int loam_batch_upload(loam_ctx* x, uint32_t n, const loam_cloud_in* prev, const loam_cloud_in* cur) {
  if (!x || !prev || !cur || n == 0) return fail(LOAM_E_INVAL, "bad batch arguments");
  HIP_TRY(hipSetDevice(x->device));
  for (uint32_t i = 0; i < n; ++i) {
    int rc = check_cloud_in(prev[i], x->cap);
    if (!rc) rc = check_cloud_in(cur[i], x->cap);
    if (rc) return rc;
  }
  // (a step ahead may still read the raw sweeps or write its buffer set)
  HIP_TRY(hipStreamSynchronize(x->st));
  if (x->st2) HIP_TRY(hipStreamSynchronize(x->st2));
  if (x->st3) HIP_TRY(hipStreamSynchronize(x->st3));
  if (x->st4) HIP_TRY(hipStreamSynchronize(x->st4));
  x->reset_ahead();
  x->fed = false;
  if ((int)n != x->P) {
    if (x->st2) HIP_TRY(hipStreamSynchronize(x->st2));
    x->drop_graph();  // (its kernels' arguments name the old buffers)
    x->free_feed();   // (sized for the old batch)
    x->free_pack();
    sr_free(x->srb);
    sr_free(x->srb2);
    sr_free(x->srb3);
    od_free(x->odb);
    mp_free(x->mpb);
    mp_free(x->mpb2);
    x->P = 0;  // no batch until every buffer of the new size exists
    // (the second SR / mapping sets only when a mode that alternates them runs: ensure_second_sets)
    hipError_t he = sr_alloc(x->srb, 2 * (int)n, x->cap, x->R);
    if (he == hipSuccess) he = od_alloc(x->odb, (int)n, x->R, x->cap, (int)x->cfg.od_max_iter);
    if (he == hipSuccess)
      he = mp_alloc(x->mpb, (int)n, x->R, x->cap, mp_batch_map_capacity(x->cap), (int)x->cfg.mp_max_iter, /*batch=*/true);
    if (he != hipSuccess) {
      sr_free(x->srb);
      sr_free(x->srb2);
      sr_free(x->srb3);
      od_free(x->odb);
      mp_free(x->mpb);
      mp_free(x->mpb2);
      return fail(LOAM_E_NOMEM, std::string("batch allocation failed: ") + hipGetErrorString(he));
    }
    x->P = (int)n;
  }
  x->odb.tune = x->tune;
  x->mpb.tune = x->mpb2.tune = x->tune;
  std::vector<float4> h((size_t)x->cap);
  std::vector<int> counts(2 * n);
  for (uint32_t i = 0; i < n; ++i)
    for (int k = 0; k < 2; ++k) {
      const loam_cloud_in& c = k == 0 ? prev[i] : cur[i];
      pack(c, h.data(), 0, c.count);
      counts[2 * i + k] = (int)c.count;
      HIP_TRY(hipMemcpy(x->srb.raw + (size_t)(2 * i + k) * x->cap, h.data(), (size_t)c.count * sizeof(float4),
                        hipMemcpyHostToDevice));
    }
  HIP_TRY(hipMemcpy(x->srb.raw_n, counts.data(), counts.size() * sizeof(int), hipMemcpyHostToDevice));
  for (SrBuffers* o : {&x->srb2, &x->srb3})
    if (o->S) {  // the other sets' raw sweeps (tune.sr_ahead / step_pipe)
      HIP_TRY(hipMemcpy(o->raw, x->srb.raw, (size_t)2 * n * x->cap * sizeof(float4), hipMemcpyDeviceToDevice));
      HIP_TRY(hipMemcpy(o->raw_n, x->srb.raw_n, counts.size() * sizeof(int), hipMemcpyDeviceToDevice));
    }
  return LOAM_OK;
}

namespace {
// sweeps [s0, s1) of a batch (sweep 2i = prev[i], 2i + 1 = cur[i]) packed back to back (pack_tight_of)
void pack_tight(const loam_cloud_in* prev, const loam_cloud_in* cur, size_t s0, size_t s1, const int* off, float4* dst) {
  pack_tight_of([&](size_t s) -> const loam_cloud_in& { return (s & 1) ? cur[s / 2] : prev[s / 2]; }, s0, s1, off, dst);
}

// The second scan-registration set and the second mapping set, which only the modes that alternate
// the sets between steps use (tune.sr_ahead, tune.step_pipe): allocated on the first step that
// needs them, the uploaded raw sweeps copied from the first set.  The sets of the batch are then
// kept until an upload of another size.
// the SR sets the step pipeline rotates (tune.pipe_sr_sets when pipelined, else 2)
int pipe_slots(const loam_ctx* x, bool pipe) { return pipe ? x->tune.pipe_sr_sets : 2; }

int ensure_second_sets(loam_ctx* x, int slots) {
  const int P = x->P;
  if (slots > 2 && !x->srb3.S) {  // the third SR set (tune.pipe_sr_sets = 3)
    const hipError_t he = sr_alloc(x->srb3, 2 * P, x->cap, x->R);
    if (he != hipSuccess) {
      sr_free(x->srb3);
      return fail(LOAM_E_NOMEM, std::string("third batch set allocation failed: ") + hipGetErrorString(he));
    }
    HIP_TRY(hipMemcpy(x->srb3.raw, x->srb.raw, (size_t)2 * P * x->cap * sizeof(float4), hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(x->srb3.raw_n, x->srb.raw_n, (size_t)2 * P * sizeof(int), hipMemcpyDeviceToDevice));
  }
  if (x->srb2.S) return LOAM_OK;
  hipError_t he = sr_alloc(x->srb2, 2 * P, x->cap, x->R);
  if (he == hipSuccess)
    he = mp_alloc(x->mpb2, P, x->R, x->cap, mp_batch_map_capacity(x->cap), (int)x->cfg.mp_max_iter, /*batch=*/true);
  if (he != hipSuccess) {
    sr_free(x->srb2);
    sr_free(x->srb3);
    mp_free(x->mpb2);
    return fail(LOAM_E_NOMEM, std::string("second batch set allocation failed: ") + hipGetErrorString(he));
  }
  x->mpb2.tune = x->tune;
  // (the raw sweeps are only read by the kernels, so the first set's may be copied while steps run)
  HIP_TRY(hipMemcpy(x->srb2.raw, x->srb.raw, (size_t)2 * P * x->cap * sizeof(float4), hipMemcpyDeviceToDevice));
  HIP_TRY(hipMemcpy(x->srb2.raw_n, x->srb.raw_n, (size_t)2 * P * sizeof(int), hipMemcpyDeviceToDevice));
  return LOAM_OK;
}
}  // namespace

namespace {
// one batch step's device work on x->st (+ x->st2 for mapping frame 1); timing events only when
// `events` (a captured graph records none: its stage times are not split)
hipError_t batch_enqueue(loam_ctx* x, Prof* pf, bool events) {
  const int P = x->P;
  OdBuffers& o = x->odb;
  hipError_t e = hipSuccess;
  auto T = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  // scan registration of this step: already enqueued one step ahead (st3), or here
  const int idx = x->sr_idx;
  SrBuffers& sb = x->srbuf(idx);
  const int ls = x->od_s, le = x->od_e;  // (Last buffers: the seed's, TransformToEnd's)
  x->od_s_last = ls;
  if (events) T(hipEventRecord(x->ev[0], x->st));
  x->prof.begin(x->st);
  if (x->b_used) {  // pipelined steps' mappings may still run on st4 / st2 (batch_enqueue_pipe)
    for (int i = 0; i < 3; ++i)
      if (x->mp_done_rec[i]) T(hipStreamWaitEvent(x->st, x->mp_done[i], 0));
    x->b_used = false;
  }
  if (x->sr_ready) {
    T(hipStreamWaitEvent(x->st, x->sr_done, 0));
    x->sr_ready = false;
  } else {
    sr_launch(sb, sr_params(x), x->st, pf);
  }
  if (events) T(hipEventRecord(x->ev[1], x->st));
  o.istate = o.istate_set[idx];  // (this step's; the kernels take the buffers by value)
  o.state = o.state_set[idx];
  T(hipMemsetAsync(o.state, 0, (size_t)P * kOdStateFloats * sizeof(float), x->st));
  const FeatView fprev = feat_view(sb, 0, 2), fcur = feat_view(sb, 1, 2);
  const bool ahead = x->st3 && x->tune.sr_ahead > 0 && P >= x->tune.sr_ahead && events && !pf;
  const int ahead_at = x->tune.sr_ahead_at >= 0 ? x->tune.sr_ahead_at : (P <= 256 ? 2 : 1);
  auto ahead_point = [&](int at) {
    if (ahead && ahead_at == at) T(hipEventRecord(x->ahead_at, x->st));
  };
  ahead_point(0);
  // odometry seeded from prev as a solved zero-increment frame, then one loop body on cur
  if (x->seed_ready) {  // enqueued one step ahead (st3, seed_done)
    T(hipStreamWaitEvent(x->st, x->seed_done, 0));
    x->seed_ready = false;
  } else {
    T(hipMemsetAsync(o.istate, 0, (size_t)P * kOdStateInts * sizeof(int), x->st));
    hipLaunchKernelGGL(k_od_end, dim3(kOdEndWg, P), dim3(256), 0, x->st, o, fprev, ls, 1, 0);
    x->prof.mark("k_od_end_seed");
    od_build_hashes(o, ls, x->st);
    x->prof.mark("k_hash_build_last");
  }
  ahead_point(1);
  // mapping frame 1 (prev into an empty map at the origin) reads only the seeding's Last[s]: it runs on a second stream beside the odometry solve, whose L-M iterations are
  // chains of small latency-bound launches that leave most of the chip idle.  The profiling pass
  // keeps one stream so that its per-kernel event times stay attributable.
  const bool overlap = x->st2 && !pf;
  if (overlap) {
    T(hipEventRecord(x->fork, x->st));
    T(hipStreamWaitEvent(x->st2, x->fork, 0));
    mp_batch_frame1(x->mpbuf(idx), o, ls, x->st2, nullptr);
    T(hipEventRecord(x->join, x->st2));
  }
  // the pose accumulation (k_od_fini, one serial double-trig chain per problem) beside
  // TransformToEnd on the second stream: both only read the solved transform
  od_solve(o, fcur, ls, x->st, pf, /*device_fini=*/!overlap);
  if (overlap) {
    T(hipEventRecord(x->fork2, x->st));
    T(hipStreamWaitEvent(x->st2, x->fork2, 0));
    od_fini(o, fcur, x->st2);
    T(hipEventRecord(x->join2, x->st2));
  }
  hipLaunchKernelGGL(k_od_end, dim3(kOdEndWg, P), dim3(256), 0, x->st, o, fcur, le, 2, 0);
  x->prof.mark("k_od_end");
  if (overlap) T(hipStreamWaitEvent(x->st, x->join2, 0));
  if (events) T(hipEventRecord(x->ev[2], x->st));
  // mapping: (frame 1 unless overlapped) then cur with the odometry pose
  if (overlap) {
    T(hipStreamWaitEvent(x->st, x->join, 0));
  } else {
    mp_batch_frame1(x->mpbuf(idx), o, ls, x->st, pf);
  }
  ahead_point(2);
  if (ahead) T(hipEventRecord(x->seed_at, x->st));
  // (frame 1 is done: the second stream is free for frame 2's stack VoxelGrid)
  SideStream side;
  side.st = x->st2;
  side.fork = x->fork; side.join = x->join;
  mp_batch_frame2(x->mpbuf(idx), o, le, x->st, pf, overlap ? &side : nullptr);
  x->mp_last = idx;
  if (events) T(hipEventRecord(x->ev[3], x->st));
  x->srb_last = idx;
  // the next step's scan registration into the other set, once the step that last read it is done
  // (not in a captured graph, whose replays would all reuse one set, nor in the profiling pass)
  if (ahead) {
    T(hipEventRecord(x->step_done[idx], x->st));
    x->step_done_rec[idx] = true;
    const int nx = idx == 0 ? 1 : 0;  // (two sets here; a slot 2 left by pipelined runs goes back to 0)
    if (x->step_done_rec[nx]) T(hipStreamWaitEvent(x->st3, x->step_done[nx], 0));
    T(hipStreamWaitEvent(x->st3, x->ahead_at, 0));
    sr_launch(x->srbuf(nx), sr_params(x), x->st3, nullptr);
    T(hipEventRecord(x->sr_done, x->st3));
    x->sr_ready = true;
    x->sr_idx = nx;
    // the next step's odometry seed: Last[s] / its hashes are free once this step's odometry is
    // done (the second mapping frame reads Last[e] and the state only); its counts go to the other
    // istate set, which the next step reads
    T(hipStreamWaitEvent(x->st3, x->seed_at, 0));
    OdBuffers on = o;
    on.istate = o.istate_set[nx];
    T(hipMemsetAsync(on.istate, 0, (size_t)P * kOdStateInts * sizeof(int), x->st3));
    hipLaunchKernelGGL(k_od_end, dim3(kOdEndWg, P), dim3(256), 0, x->st3, on, feat_view(x->srbuf(nx), 0, 2), ls, 1, 0);
    od_build_hashes(on, ls, x->st3);
    T(hipEventRecord(x->seed_done, x->st3));
    x->seed_ready = true;
  }
  T(hipGetLastError());
  return e;
}
// The scan registration of the step reading buffer set i and its odometry seed (Last[ls], its
// hashes, the counts in istate set i), on st3.  Waits: the set's previous step is done with it
// (mp_done[i]: its mapping, the last reader, after that step's odometry), and, when `free_last` is
// recorded, Last[ls]'s last reader: frame 2 of the step before the current one (the rotation of
// batch_enqueue_pipe leaves Last[ls] to no running step's odometry or frame 1).
// the event after which the seed of the step reading SR slot j may rewrite its Last buffer: frame 2
// of the step two before it (slot j - 2 of n) read that buffer last (its inputs_read), if recorded
hipEvent_t seed_free_last(const loam_ctx* x, int j, int n) {
  const int k = (j + n - 2) % n;
  return x->inputs_read_rec[k] ? x->inputs_read[k] : nullptr;
}
hipError_t enqueue_ahead(loam_ctx* x, int i, int ls, hipEvent_t free_last) {
  const int P = x->P;
  OdBuffers on = x->odb;
  hipError_t e = hipSuccess;
  auto T = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  if (x->mp_done_rec[i]) T(hipStreamWaitEvent(x->st3, x->mp_done[i], 0));
  T(hipStreamWaitEvent(x->st3, x->a_start, 0));  // (whatever ran on st before this call)
  PT_BEGIN("sr", x->st3);
  sr_launch(x->srbuf(i), sr_params(x), x->st3, nullptr);
  PT_END("sr", x->st3);
  T(hipEventRecord(x->sr_done, x->st3));
  if (free_last) T(hipStreamWaitEvent(x->st3, free_last, 0));
  on.istate = on.istate_set[i];
  T(hipMemsetAsync(on.istate, 0, (size_t)P * kOdStateInts * sizeof(int), x->st3));
  hipLaunchKernelGGL(k_od_end, dim3(kOdEndWg, P), dim3(256), 0, x->st3, on, feat_view(x->srbuf(i), 0, 2), ls, 1, 0);
  od_build_hashes(on, ls, x->st3);
  T(hipEventRecord(x->seed_done, x->st3));
  x->sr_ready = x->seed_ready = true;
  return e;
}

// One batch step as a stage of a software pipeline over consecutive steps (tune.step_pipe):
//   st3  scan registration + odometry seed of step k + 1 (enqueue_ahead)
//   st   odometry of step k (L-M against Last[s], pose accumulation, TransformToEnd into Last[e])
//   st4 / st2  mapping of step k: frame 1 (reads Last[s]), frame 2 (reads Last[e], after the
//        odometry); with two mapping sets (tune.pipe_mp_sets = 2) the steps alternate st4 / st2
// so the odometry of step k + 1 runs beside the mapping of step k and the seed of step k + 2 beside
// both.  Buffers shared between steps: the SR set, the odometry state / istate sets and the mapping
// sets alternate; the three Last buffers rotate (s, e) -> (3 - s - e, s): step k + 1 seeds the one
// step k - 1's frame 2 read last (inputs_read of that parity), and step k + 1's TransformToEnd
// rewrites step k's Last[s] once frame 1 of step k has read it (mp1_read; the odometry of step k is
// ahead on st).  Every step does the same work as batch_enqueue's; loam_batch_sync waits for all
// four streams.
hipError_t batch_enqueue_pipe(loam_ctx* x) {
  const int P = x->P;
  OdBuffers& o = x->odb;
  hipError_t e = hipSuccess;
  auto T = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  const int n = pipe_slots(x, true), idx = x->sr_idx, nx = (idx + 1) % n;
  const int ls = x->od_s, le = x->od_e, lf = kOdBufs - ls - le;
  static_assert(kOdBufs == 3, "the rotation takes three Last buffers");
  SrBuffers& sb = x->srbuf(idx);
  T(hipEventRecord(x->a_start, x->st));
  T(hipEventRecord(x->ev[0], x->st));
  // (not enqueued ahead: the first pipelined step, or a fed context's step without a feed, which
  // re-runs the set's resident sweeps; Last[ls]'s last reader as for the trailing call below)
  if (!x->sr_ready || !x->seed_ready) T(enqueue_ahead(x, idx, ls, seed_free_last(x, idx, n)));
  x->sr_ready = x->seed_ready = false;
  x->od_s_last = ls;
  const FeatView fcur = feat_view(sb, 1, 2);
  // odometry (st)
  o.istate = o.istate_set[idx];
  o.state = o.state_set[idx];
  T(hipStreamWaitEvent(x->st, x->sr_done, 0));
  T(hipStreamWaitEvent(x->st, x->seed_done, 0));
  T(hipEventRecord(x->ev[1], x->st));
  PT_BEGIN("od", x->st);
  T(hipMemsetAsync(o.state, 0, (size_t)P * kOdStateFloats * sizeof(float), x->st));
  od_solve(o, fcur, ls, x->st, nullptr, /*device_fini=*/true);
  // Last[le] was the previous step's Last[s]: its frame 1 has read it (its odometry is ahead on st);
  // before that, frame 2 of the step before read it, which the previous seed waited for
  if (x->b_used) T(hipStreamWaitEvent(x->st, x->mp1_read, 0));
  hipLaunchKernelGGL(k_od_end, dim3(kOdEndWg, P), dim3(256), 0, x->st, o, fcur, le, 2, 0);
  PT_END("od", x->st);
  T(hipEventRecord(x->od_done, x->st));
  T(hipEventRecord(x->ev[2], x->st));
  // mapping: frame 1 once the seed (and this call's earlier work on st) is there, frame 2 once the
  // odometry is.  tune.pipe_mp_sets = 2: the steps alternate between two mapping sets on st4 / st2,
  // so the next step's frame 1 runs beside this step's frame 2 (no side branch then); 1: one set
  // on st4, frame 2's stack VoxelGrid on st2
  const bool two = x->tune.pipe_mp_sets == 2;
  const int m = x->pipe_k++ & 1;  // (the mapping sets alternate by step, whatever the SR slots)
  hipStream_t ms = two && m ? x->st2 : x->st4;
  MpBuffers& mb = two ? x->mpbuf(m) : x->mpb;
  T(hipStreamWaitEvent(ms, x->a_start, 0));
  T(hipStreamWaitEvent(ms, x->seed_done, 0));
  SideStream side1;  // (no branches: only the event once Last[ls] is read)
  side1.inputs_read = x->mp1_read;
  PT_BEGIN("mp1", ms);
  mp_batch_frame1(mb, o, ls, ms, nullptr, &side1);
  PT_END("mp1", ms);
  T(hipEventRecord(x->mp1_done, ms));
  T(hipStreamWaitEvent(ms, x->od_done, 0));
  PT_BEGIN("mp2", ms);
  SideStream side;
  side.st = two ? nullptr : x->st2;
  side.fork = x->fork; side.join = x->join;
  side.inputs_read = x->inputs_read[idx];
  mp_batch_frame2(mb, o, le, ms, nullptr, &side);
  PT_END("mp2", ms);
#ifdef LOAM_PIPE_TRACE
  ++g_pt.step;
#endif
  T(hipEventRecord(x->mp_done[idx], ms));
  x->mp_done_rec[idx] = true;
  x->b_used = true;
  x->mp_last = two ? m : 0;
  T(hipEventRecord(x->ev[3], ms));
  x->srb_last = idx;
  // the next step's scan registration + seed (st3) into Last[lf], which frame 2 of the previous
  // step (SR set nx) read last; a fed context's next loam_batch_feed enqueues them instead, after
  // copying its sweeps into set nx
  if (!x->fed) T(enqueue_ahead(x, nx, lf, seed_free_last(x, nx, n)));
  x->inputs_read_rec[idx] = true;
  x->od_s = lf;
  x->od_e = ls;
  x->sr_idx = nx;
  T(hipGetLastError());
  return e;
}
}  // namespace

int loam_batch_run(loam_ctx* x) {
  if (!x || x->P == 0) return fail(LOAM_E_INVAL, "no batch uploaded");
  HIP_TRY(hipSetDevice(x->device));
  Prof* pf = x->prof.on ? &x->prof : nullptr;
  const bool pipe = !pf && !x->tune.graph && x->st2 && x->st3 && x->st4 && x->tune.step_pipe > 0 && x->P >= x->tune.step_pipe;
  const bool ahead = !pf && !x->tune.graph && x->st3 && x->tune.sr_ahead > 0 && x->P >= x->tune.sr_ahead;
  if (pipe || ahead) {
    const int rc = ensure_second_sets(x, pipe_slots(x, pipe));
    if (rc) return rc;
  }
  if (pipe) {
    HIP_TRY(batch_enqueue_pipe(x));
    x->batch_ran = true;
    return LOAM_OK;
  }
  if (!x->tune.graph || pf) {
    HIP_TRY(batch_enqueue(x, pf, true));
    x->batch_ran = true;
    return LOAM_OK;
  }
  // graph replay: captured on the first call for this batch (the kernels' arguments are the
  // batch's buffers, which stay put until the next loam_batch_upload of another size)
  if (!x->graph_exec || x->graph_P != x->P) {
    x->drop_graph();
    HIP_TRY(hipStreamBeginCapture(x->st, hipStreamCaptureModeThreadLocal));
    const hipError_t ce = batch_enqueue(x, nullptr, false);
    hipGraph_t g = nullptr;
    const hipError_t ee = hipStreamEndCapture(x->st, &g);
    if (ce != hipSuccess || ee != hipSuccess) {
      if (g) (void)hipGraphDestroy(g);
      return fail(LOAM_E_HIP, std::string("batch graph capture: ") + hipGetErrorString(ce != hipSuccess ? ce : ee));
    }
    x->graph = g;
    HIP_TRY(hipGraphInstantiate(&x->graph_exec, g, nullptr, nullptr, 0));
    x->graph_P = x->P;
  }
  HIP_TRY(hipEventRecord(x->ev[0], x->st));
  HIP_TRY(hipEventRecord(x->ev[1], x->st));
  HIP_TRY(hipEventRecord(x->ev[2], x->st));
  HIP_TRY(hipGraphLaunch(x->graph_exec, x->st));
  HIP_TRY(hipEventRecord(x->ev[3], x->st));
  x->batch_ran = true;
  return LOAM_OK;
}

int loam_batch_feed(loam_ctx* x, uint32_t n, const loam_cloud_in* prev, const loam_cloud_in* cur) {
  if (!x || !prev || !cur || n == 0) return fail(LOAM_E_INVAL, "bad batch arguments");
  if (x->P == 0 || (int)n != x->P)
    return fail(LOAM_E_INVAL, "loam_batch_feed: n must equal the uploaded batch size (loam_batch_upload first)");
  HIP_TRY(hipSetDevice(x->device));
  for (uint32_t i = 0; i < n; ++i) {
    int rc = check_cloud_in(prev[i], x->cap);
    if (!rc) rc = check_cloud_in(cur[i], x->cap);
    if (rc) return rc;
  }
  const int P = x->P;
  const bool pipe = !x->prof.on && !x->tune.graph && x->st2 && x->st3 && x->st4 && x->tune.step_pipe > 0 &&
                    P >= x->tune.step_pipe;
  if (!pipe) {  // sequential steps: the next step's sweeps replace the resident ones (as an upload)
    return loam_batch_upload(x, n, prev, cur);
  }
  int rc = ensure_second_sets(x, pipe_slots(x, true));
  if (rc) return rc;
  const int i = x->sr_idx;  // the set the next step reads
  if (x->sr_ready || x->seed_ready) {
    // (enqueued ahead on the set's resident sweeps by a run before the context was fed: discarded,
    // the feed's scan registration rewrites the set)
    HIP_TRY(hipStreamSynchronize(x->st3));
    x->sr_ready = x->seed_ready = false;
  }
  const size_t per = (size_t)2 * P * x->cap;
  if (!x->feed_pin[i]) {
    HIP_TRY(hipHostMalloc((void**)&x->feed_pin[i], per * sizeof(float4), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)&x->feed_n[i], (size_t)4 * P * sizeof(int), hipHostMallocDefault));
  }
  if (!x->feed_dev) {
    HIP_TRY(hipMalloc((void**)&x->feed_dev, per * sizeof(float4)));
    HIP_TRY(hipMalloc((void**)&x->feed_doff, (size_t)4 * P * sizeof(int)));
  }
  if (x->feed_rec[i]) HIP_TRY(hipEventSynchronize(x->feed_copied[i]));  // (the staging's last copy is out)
  SrBuffers& sb = x->srbuf(i);
  // behind the set's last reader (the step that used it: its mapping, after its scan registration)
  if (x->mp_done_rec[i]) HIP_TRY(hipStreamWaitEvent(x->st3, x->mp_done[i], 0));
  // the sweeps packed back to back in chunks, each chunk one copy into the device staging enqueued
  // before the next is packed (the host packing overlaps the DMA of the chunk before); then one
  // kernel puts every sweep at its stride in the set's raw array
  const size_t S = (size_t)2 * P;
  int* nn = x->feed_n[i];
  int* off = nn + S;
  {
    size_t run = 0;
    for (size_t s = 0; s < S; ++s) {
      const loam_cloud_in& c = (s & 1) ? cur[s / 2] : prev[s / 2];
      nn[s] = (int)c.count;
      off[s] = (int)run;
      run += c.count;
    }
  }
  constexpr size_t kFeedChunk = 128;  // sweeps
  for (size_t s0 = 0; s0 < S; s0 += kFeedChunk) {
    const size_t s1 = std::min(S, s0 + kFeedChunk);
    pack_tight(prev, cur, s0, s1, off, x->feed_pin[i]);
    const size_t a = (size_t)off[s0], b = (size_t)off[s1 - 1] + (size_t)nn[s1 - 1];
    if (b > a)
      HIP_TRY(hipMemcpyAsync(x->feed_dev + a, x->feed_pin[i] + a, (b - a) * sizeof(float4), hipMemcpyHostToDevice, x->st3));
  }
  HIP_TRY(hipMemcpyAsync(x->feed_doff, nn, 2 * S * sizeof(int), hipMemcpyHostToDevice, x->st3));
  HIP_TRY(sr_scatter_packed(x->feed_dev, x->feed_doff + S, x->feed_doff, sb.raw, x->cap, (int)S, x->st3));
  HIP_TRY(hipMemcpyAsync(sb.raw_n, x->feed_doff, S * sizeof(int), hipMemcpyDeviceToDevice, x->st3));
  HIP_TRY(hipEventRecord(x->feed_copied[i], x->st3));
  x->feed_rec[i] = true;
  HIP_TRY(enqueue_ahead(x, i, x->od_s, seed_free_last(x, i, pipe_slots(x, true))));
  x->fed = true;
  return LOAM_OK;
}

int loam_batch_sync(loam_ctx* x) {
  if (!x) return fail(LOAM_E_INVAL, "null argument");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipStreamSynchronize(x->st));
  // (a step's work includes its mapping on st4 and the scan registration it enqueued for the next
  // step on st3)
  if (x->st4) HIP_TRY(hipStreamSynchronize(x->st4));
  if (x->st2) HIP_TRY(hipStreamSynchronize(x->st2));
  if (x->st3) HIP_TRY(hipStreamSynchronize(x->st3));
  // launch errors of either mapping set (the step pipeline alternates them), reported by this call
  for (int i = 0; i < 2; ++i) HIP_TRY(x->mpbuf(i).take_error());
#ifdef LOAM_PIPE_TRACE
  g_pt.dump();
#endif
  return LOAM_OK;
}

int loam_batch_lm_info(loam_ctx* x, int32_t* od_iters, int32_t* mp_iters, loam_pose6* od_transform) {
  if (!x || x->P == 0) return fail(LOAM_E_INVAL, "no batch");
  HIP_TRY(hipSetDevice(x->device));
  const int P = x->P;
  for (hipStream_t s : {x->st, x->st2, x->st3, x->st4})
    if (s) HIP_TRY(hipStreamSynchronize(s));
  if (od_iters) {
    std::vector<int> ist((size_t)P * kOdStateInts);
    HIP_TRY(hipMemcpy(ist.data(), x->odb.istate, ist.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < P; ++i) od_iters[i] = ist[(size_t)i * kOdStateInts + kIsIters];
  }
  if (od_transform) {  // (state floats 0..5: the L-M transform, kOdSum the accumulated pose)
    std::vector<float> st((size_t)P * kOdStateFloats);
    HIP_TRY(hipMemcpy(st.data(), x->odb.state, st.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int i = 0; i < P; ++i) std::memcpy(&od_transform[i], &st[(size_t)i * kOdStateFloats], sizeof(loam_pose6));
  }
  if (mp_iters) HIP_TRY(mp_batch_iters(x->mpbuf(x->mp_last), x->st, mp_iters));
  return LOAM_OK;
}

int loam_batch_download(loam_ctx* x, loam_pose6* od_sum, loam_pose6* aft, loam_stats* stats) {
  if (!x || x->P == 0) return fail(LOAM_E_INVAL, "no batch");
  HIP_TRY(hipSetDevice(x->device));
  const int P = x->P;
  HIP_TRY(hipStreamSynchronize(x->st));
  if (x->st4) HIP_TRY(hipStreamSynchronize(x->st4));
  if (x->st2) HIP_TRY(hipStreamSynchronize(x->st2));
  if (x->st3) HIP_TRY(hipStreamSynchronize(x->st3));  // (the work enqueued ahead rewrites Last[0] alike)
  std::vector<float> st((size_t)P * kOdStateFloats);
  std::vector<int> ist((size_t)P * kOdStateInts), srerr(2 * P), cnt(8 * P), nfull(2 * P), nl((size_t)kOdBufs * 2 * P);
  HIP_TRY(hipMemcpy(st.data(), x->odb.state, st.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ist.data(), x->odb.istate, ist.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(srerr.data(), x->srbuf(x->srb_last).err, srerr.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(cnt.data(), x->srbuf(x->srb_last).cnt, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(nfull.data(), x->srbuf(x->srb_last).n_full, nfull.size() * sizeof(int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(nl.data(), x->odb.nlast, nl.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int i = 0; i < 2 * P; ++i) {
    int rc = sr_errors(srerr[i]);
    if (rc) return rc;
  }
  if (od_sum)
    for (int i = 0; i < P; ++i) std::memcpy(&od_sum[i], &st[(size_t)i * kOdStateFloats + kOdSum], sizeof(loam_pose6));
  loam_stats s;
  std::memset(&s, 0, sizeof(s));
  // (a launch error recorded on the other mapping set during an earlier pipelined step fails this
  // call too, not a later unrelated one)
  HIP_TRY(x->mpbuf(1 - x->mp_last).take_error());
  int rc = mp_batch_download(x->mpbuf(x->mp_last), x->st, aft, &s, g_err);
  if (rc) return rc;
  for (int i = 0; i < 2 * P; ++i) {
    s.n_ring += nfull[i];
    s.n_sharp += cnt[4 * i]; s.n_less_sharp += cnt[4 * i + 1];
    s.n_flat += cnt[4 * i + 2]; s.n_less_flat += cnt[4 * i + 3];
  }
  int raw_n[2];
  (void)raw_n;
  std::vector<int> rn(2 * P);
  HIP_TRY(hipMemcpy(rn.data(), x->srbuf(x->srb_last).raw_n, rn.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int i = 0; i < 2 * P; ++i) s.n_raw += rn[i];
  const int ls = x->od_s_last;  // (the last step's Last[s]; every step reads the same counts)
  for (int i = 0; i < P; ++i) {
    const int* q = &ist[(size_t)i * kOdStateInts];
    if (q[kIsErr]) return fail(LOAM_E_CAPACITY, "odometry capacity exceeded");
    s.od_iters += q[kIsIters];
    s.od_assoc_rounds += q[kIsAssoc];
    s.od_rows_sum += (uint64_t)q[kIsRows];
    s.od_queries += q[kIsQueries];
    s.od_degenerate_steps += (uint64_t)q[kIsDegSteps];
    s.od_nan_skips += (uint64_t)q[kIsNanSkips];
    s.od_assoc_gathered += (uint64_t)(uint32_t)q[kIsGathered];
    s.od_assoc_boxes += (uint64_t)(uint32_t)q[kIsBoxes];
    const uint64_t nq = q[kIsAssoc] ? (uint64_t)(q[kIsQueries] / q[kIsAssoc]) : 0, it = (uint64_t)q[kIsIters];
    s.od_query_iters += nq * it;
    s.od_row_evals += nq * it * (it + 1) / 2;
    const int* n = &nl[((size_t)i * kOdBufs + ls) * 2];
    s.od_corner_last += n[0];
    s.od_surf_last += n[1];
    s.od_assoc_points += (uint64_t)q[kIsAssoc] * (n[0] + n[1]);
  }
  count_bytes(s);
  x->prof.collect();
  float ms_sr = 0, ms_od = 0, ms_mp = 0;
  (void)hipEventElapsedTime(&ms_sr, x->ev[0], x->ev[1]);
  (void)hipEventElapsedTime(&ms_od, x->ev[1], x->ev[2]);
  (void)hipEventElapsedTime(&ms_mp, x->ev[2], x->ev[3]);
  s.ms_sr = ms_sr;
  s.ms_od = ms_od;
  s.ms_mp = ms_mp;
  x->stats = s;
  if (stats) *stats = s;
  return LOAM_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ batch feature download
namespace {
// points of one staging buffer (32 MiB): a chunk of the packed clouds is at most this large
constexpr size_t kPackStagePts = (size_t)1 << 21;

// a sweep's clouds at their strides (full and less_flat up to max_points, 12 + 120 + 24 picks per ring)
size_t pack_sweep_max(const loam_ctx* x) {
  return (size_t)2 * x->cap + (size_t)(kSharpPerRing + kLessSharpPerRing + kFlatPerRing) * x->R;
}

// the staging itself: shared by loam_batch_features and the map export / import, kept until loam_destroy
int ensure_pack_stage(loam_ctx* x, const char* what) {
  if (x->pack_pin[1] && x->pack_dev[1] && x->pack_done[1]) return LOAM_OK;
  hipError_t he = hipSuccess;
  for (int i = 0; i < 2; ++i) {
    if (he == hipSuccess && !x->pack_dev[i]) he = hipMalloc((void**)&x->pack_dev[i], kPackStagePts * sizeof(float4));
    if (he == hipSuccess && !x->pack_pin[i])
      he = hipHostMalloc((void**)&x->pack_pin[i], kPackStagePts * sizeof(float4), hipHostMallocDefault);
    if (he == hipSuccess && !x->pack_done[i]) he = hipEventCreateWithFlags(&x->pack_done[i], hipEventDisableTiming);
  }
  if (he != hipSuccess) {
    x->free_pack();
    return fail(LOAM_E_NOMEM, std::string(what) + " staging allocation failed: " + hipGetErrorString(he));
  }
  return LOAM_OK;
}

int ensure_pack(loam_ctx* x) {
  const int S = 2 * x->P;
  if (x->pack_S == S) return LOAM_OK;
  if (pack_sweep_max(x) > kPackStagePts)
    return fail(LOAM_E_INVAL, "loam_batch_features: max_points is too large for the download staging (one sweep's "
                              "clouds must fit " + std::to_string(kPackStagePts) + " points)");
  x->free_pack_table();
  hipError_t he = hipMalloc((void**)&x->pack_table, (size_t)kPackClouds * (S + 1) * sizeof(uint64_t));
  if (he == hipSuccess)
    he = hipHostMalloc((void**)&x->pack_table_h, (size_t)kPackClouds * (S + 1) * sizeof(uint64_t), hipHostMallocDefault);
  if (he != hipSuccess) {
    x->free_pack();
    return fail(LOAM_E_NOMEM, std::string("feature download staging allocation failed: ") + hipGetErrorString(he));
  }
  const int rc = ensure_pack_stage(x, "feature download");
  if (rc) {
    x->free_pack();
    return rc;
  }
  x->pack_S = S;
  return LOAM_OK;
}

// pinned staging -> caller storage, large runs on up to eight threads (as pack_tight)
void copy_wide(void* dst, const void* src, size_t bytes) {
  constexpr size_t kMin = (size_t)4 << 20;  // per thread
  const size_t hw = std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
  const size_t nt = std::max<size_t>(1, std::min(hw, bytes / kMin));
  std::vector<std::thread> th;
  auto part = [&](size_t t) {
    const size_t a = bytes * t / nt / 16 * 16, b = t + 1 == nt ? bytes : bytes * (t + 1) / nt / 16 * 16;
    std::memcpy((char*)dst + a, (const char*)src + a, b - a);
  };
  for (size_t t = 1; t < nt; ++t) th.emplace_back(part, t);
  part(0);
  for (auto& t : th) t.join();
}
}  // namespace

extern "C" int loam_batch_features(loam_ctx* x, uint32_t first, uint32_t n, loam_batch_clouds* out) {
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  if (x->P == 0) return fail(LOAM_E_INVAL, "no batch uploaded");
  if (!x->batch_ran) return fail(LOAM_E_INVAL, "loam_batch_features: no loam_batch_run since the last loam_batch_upload");
  const uint32_t P = (uint32_t)x->P;
  if (n == 0 || first >= P || n > P - first)
    return fail(LOAM_E_INVAL, "loam_batch_features: problems [first, first + n) must be a non-empty range of the batch");
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipStreamSynchronize(x->st));
  if (x->st4) HIP_TRY(hipStreamSynchronize(x->st4));
  if (x->st2) HIP_TRY(hipStreamSynchronize(x->st2));
  if (x->st3) HIP_TRY(hipStreamSynchronize(x->st3));
  // the set of the last enqueued step, not the set the next step reads: the work enqueued ahead (or
  // a feed) has already rewritten that one.  Nothing after k_sr_compact writes a set's clouds (the
  // odometry and the mapping read them through FeatView's const pointers), so they are as the scan
  // registration of that step left them.
  const SrBuffers& sb = x->srbuf(x->srb_last);
  {
    std::vector<int> srerr(2 * (size_t)P);
    HIP_TRY(hipMemcpy(srerr.data(), sb.err, srerr.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int e : srerr) {
      const int rc = sr_errors(e);
      if (rc) return rc;
    }
  }
  int rc = ensure_pack(x);
  if (rc) return rc;
  loam_batch_cloud* cl[kPackClouds] = {&out->full, &out->sharp, &out->less_sharp, &out->flat, &out->less_flat};
  const int s0 = 2 * (int)first, ns = 2 * (int)n;
  // Everything below runs on st and is complete when the call returns: a later run waits behind
  // none of it.  (One stream: the chunks' pack kernels are ~3 % of their transfers, and alternating
  // the chunks between st and st2 measured no faster at 1024 VLP-16 problems and slower at 64
  // HDL-64E ones)
  hipStream_t st = x->st;
  x->prof.begin(x->st);
  HIP_TRY(sr_pack_offsets(sb, s0, ns, x->pack_table, x->st));
  x->prof.mark("k_sr_pack_offsets");
  const size_t row = (size_t)ns + 1;
  HIP_TRY(hipMemcpyAsync(x->pack_table_h, x->pack_table, kPackClouds * row * sizeof(uint64_t), hipMemcpyDeviceToHost, x->st));
  x->prof.mark("batch_features_table_d2h");
  HIP_TRY(hipStreamSynchronize(x->st));
  const uint64_t* T = x->pack_table_h;  // T[c * row + j]
  unsigned wanted = 0, mask = 0;
  for (int c = 0; c < kPackClouds; ++c) {
    if (!cl[c]->pts && !cl[c]->offset) continue;
    wanted |= 1u << c;
    if (T[c * row + ns] > 0xffffffffull) {
      x->prof.collect();
      return fail(LOAM_E_INVAL, "loam_batch_features: a cloud of this range has more points than a uint32_t offset holds; "
                                "ask for a smaller range of problems");
    }
  }
  bool fits = true;
  for (int c = 0; c < kPackClouds; ++c) {
    if (!(wanted >> c & 1)) continue;
    const uint64_t total = T[c * row + ns];
    cl[c]->count = total;
    if (cl[c]->offset)
      for (size_t j = 0; j < row; ++j) cl[c]->offset[j] = (uint32_t)T[c * row + j];
    if (!cl[c]->pts) continue;
    if (cl[c]->capacity < total) fits = false;
    else if (total > 0) mask |= 1u << c;
  }
  if (!fits) {
    x->prof.collect();
    return fail(LOAM_E_CAPACITY, "loam_batch_features: a cloud's capacity is too small (count holds the required size)");
  }
  // the sweep range in chunks whose packed size fits one staging buffer (a sweep always does:
  // ensure_pack), each cloud's run of a chunk contiguous at cbase[c]
  struct Chunk {
    int j0, j1;
    size_t cbase[kPackClouds], pts;
  };
  std::vector<Chunk> chunks;
  auto span = [&](int a, int b) {
    size_t s = 0;
    for (int c = 0; c < kPackClouds; ++c)
      if (mask >> c & 1) s += (size_t)(T[c * row + b] - T[c * row + a]);
    return s;
  };
  for (int j0 = 0; mask && j0 < ns;) {
    int j1 = j0 + 1;
    while (j1 < ns && span(j0, j1 + 1) <= kPackStagePts) ++j1;
    Chunk ch;
    ch.j0 = j0;
    ch.j1 = j1;
    ch.pts = 0;
    for (int c = 0; c < kPackClouds; ++c) {
      ch.cbase[c] = ch.pts;
      if (mask >> c & 1) ch.pts += (size_t)(T[c * row + j1] - T[c * row + j0]);
    }
    if (ch.pts > kPackStagePts) {  // (cannot happen: counts are clamped to the strides ensure_pack sized for)
      x->prof.collect();
      return fail(LOAM_E_INVAL, "loam_batch_features: a sweep's clouds exceed the download staging");
    }
    if (ch.pts) chunks.push_back(ch);
    j0 = j1;
  }
  // chunk k: packed into device buffer k & 1 and DMA'd into pinned buffer k & 1; while the host
  // copies chunk k into the caller's arrays, chunk k + 1 is packed and transferred
  auto enqueue = [&](size_t k) -> hipError_t {
    const Chunk& ch = chunks[k];
    const int i = (int)(k & 1);
    long long dbase[kPackClouds];
    for (int c = 0; c < kPackClouds; ++c) dbase[c] = (long long)ch.cbase[c] - (long long)T[c * row + ch.j0];
    // (profiling: the time the stream sat empty while the host copied the chunk before, kept out of
    // the kernel's segment)
    x->prof.mark("batch_features_host_wait");
    hipError_t e = sr_pack(sb, x->pack_table, s0, ns, ch.j0, ch.j1 - ch.j0, mask, dbase, x->pack_dev[i], st);
    x->prof.mark("k_sr_pack");
    if (e == hipSuccess)
      e = hipMemcpyAsync(x->pack_pin[i], x->pack_dev[i], ch.pts * sizeof(float4), hipMemcpyDeviceToHost, st);
    x->prof.mark("batch_features_d2h");
    if (e == hipSuccess) e = hipEventRecord(x->pack_done[i], st);
    return e;
  };
  hipError_t he = hipSuccess;
  for (size_t k = 0; k < chunks.size() && k < 2 && he == hipSuccess; ++k) he = enqueue(k);
  for (size_t k = 0; k < chunks.size() && he == hipSuccess; ++k) {
    const Chunk& ch = chunks[k];
    he = hipEventSynchronize(x->pack_done[k & 1]);
    if (he != hipSuccess) break;
    for (int c = 0; c < kPackClouds; ++c) {
      if (!(mask >> c & 1)) continue;
      const uint64_t a = T[c * row + ch.j0], b = T[c * row + ch.j1];
      if (b > a) copy_wide(cl[c]->pts + a, x->pack_pin[k & 1] + ch.cbase[c], (size_t)(b - a) * sizeof(float4));
    }
    if (k + 2 < chunks.size()) he = enqueue(k + 2);
  }
  if (he != hipSuccess) {  // (drain what was enqueued before reporting)
    (void)hipStreamSynchronize(st);
    return fail(LOAM_E_HIP, std::string("loam_batch_features: ") + hipGetErrorString(he));
  }
  x->prof.collect();
  return LOAM_OK;
}

// ------------------------------------------------------------------ map export / import
namespace {
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
}  // namespace

namespace {
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
    return fail(LOAM_E_INVAL, "loam_map_export: the last map update exceeded map_capacity, the store is not valid");
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
}  // namespace

extern "C" int loam_map_export(loam_ctx* x, loam_map* out) {
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  const int rc = map_drain(x);
  if (rc) return rc;
  return map_export_of(x, x->mp1, 0, x->map_frame_count, out);
}

namespace {
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
}  // namespace

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
namespace {
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
}  // namespace

// n candidate (Aft, Bef) poses of one sweep against the streaming map, which is only read: every
// candidate is an instance of the context's second mapping working set (MpLoc, mp.hpp).  The host
// reads the candidates' FromMap counts once (to size the set), then the results.
extern "C" int loam_map_localize(loam_ctx* x, const loam_pose6* odom_sum, const loam_cloud_out* corner_last,
                                 const loam_cloud_out* surf_last, uint32_t n, const loam_pose6* aft,
                                 const loam_pose6* bef, loam_localize_result* out) {
  static_assert(LOAM_LOCALIZE_MAX == kLocMax, "loam.h and mp.hpp");
  static_assert(sizeof(loam_localize_result) == 60, "loam_localize_result layout");
  if (!x || !odom_sum || !corner_last || !surf_last || !aft || !out) return fail(LOAM_E_INVAL, "null argument");
  if (n == 0 || n > LOAM_LOCALIZE_MAX)
    return fail(LOAM_E_INVAL, "loam_map_localize: n must be in [1, LOAM_LOCALIZE_MAX]");
  if ((corner_last->count && !corner_last->pts) || (surf_last->count && !surf_last->pts))
    return fail(LOAM_E_INVAL, "loam_map_localize: a cloud's pts is null");
  const MpBuffers& s = x->mp1;
  // (corner_last: also the mapping stack's own bound, 120 picks per ring, as loam_mapping has it)
  if (corner_last->count > (uint32_t)x->cap || surf_last->count > (uint32_t)x->cap ||
      corner_last->count > (uint32_t)s.capC)
    return fail(LOAM_E_INVAL, "loam_map_localize: a cloud exceeds max_points (corner_last: 120 points per ring)");
  int rc = map_drain(x);
  if (rc) return rc;
  MpLoc& L = x->loc;
  hipError_t he = mp_loc_reserve(L, s, (int)n, (int)corner_last->count, (int)surf_last->count);
  if (he != hipSuccess)
    return fail(LOAM_E_NOMEM, std::string("loam_map_localize: working set allocation failed: ") + hipGetErrorString(he));
  hipStream_t st = x->st;
  Prof* pf = x->prof.on ? &x->prof : nullptr;  // (with profiling the L-M kernels also count their work)
  MpBuffers& w = L.w;
  float* ch = L.cand_h();
  for (uint32_t h = 0; h < n; ++h) {
    std::memcpy(ch + (size_t)h * 12, &aft[h], sizeof(loam_pose6));
    if (bef) std::memcpy(ch + (size_t)h * 12 + 6, &bef[h], sizeof(loam_pose6));
    else std::memset(ch + (size_t)h * 12 + 6, 0, sizeof(loam_pose6));
  }
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
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    (void)hipStreamSynchronize(st);
    x->prof.collect();
    return fail(LOAM_E_HIP, std::string("loam_map_localize: ") + hipGetErrorString(he));
  }
  const int* head = L.head_h();
  if (head[2 * n] & ERR_CAP_MAP) {
    x->prof.collect();
    return fail(LOAM_E_INVAL, "loam_map_localize: the last map update exceeded map_capacity, the store is not valid");
  }
  int from_max = 0, cloud_max = 0;
  for (uint32_t h = 0; h < n; ++h) {
    from_max = std::max(from_max, head[2 * h] + head[2 * h + 1]);
    cloud_max = std::max(cloud_max, std::max(head[2 * h], head[2 * h + 1]));
  }
  he = mp_loc_reserve_map(L, from_max);
  if (he != hipSuccess) {
    x->prof.collect();
    return fail(LOAM_E_NOMEM, std::string("loam_map_localize: FromMap allocation failed (") + std::to_string(n) + " x " +
                                  std::to_string(from_max) + " points): " + hipGetErrorString(he));
  }
  he = mp_localize_solve(L, s, in, (int)n, from_max, cloud_max, std::max(cnt[0], cnt[1]), st, pf);
  x->prof.mark("map_localize_d2h");
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    (void)hipStreamSynchronize(st);
    x->prof.collect();
    return fail(LOAM_E_HIP, std::string("loam_map_localize: ") + hipGetErrorString(he));
  }
  x->prof.collect();
  const int* R = L.res_h();
  for (uint32_t h = 0; h < n; ++h) loc_result_of(R + (size_t)h * kLocResWords, out[h]);
  return LOAM_OK;
}

// ------------------------------------------------------------------ scoring pose guesses
// n poses of one sweep against the whole streaming map, which is only read (score.hpp).  The host
// reads the map's sizes once (to size the index), then the results.
extern "C" int loam_map_score(loam_ctx* x, const loam_cloud_out* corner, const loam_cloud_out* surf, float max_dist,
                              uint32_t n, const loam_pose6* pose, loam_score_result* out) {
  static_assert(LOAM_SCORE_MAX == kScoreMax, "loam.h and score.hpp");
  static_assert(sizeof(loam_score_result) == 32, "loam_score_result layout");
  if (!x || !corner || !surf || !pose || !out) return fail(LOAM_E_INVAL, "null argument");
  if (n == 0 || n > LOAM_SCORE_MAX) return fail(LOAM_E_INVAL, "loam_map_score: n must be in [1, LOAM_SCORE_MAX]");
  if (!(max_dist > 0.0f && max_dist <= 1.0f))
    return fail(LOAM_E_INVAL, "loam_map_score: max_dist must be in (0, 1] (the map index has 1 m cells)");
  if ((corner->count && !corner->pts) || (surf->count && !surf->pts))
    return fail(LOAM_E_INVAL, "loam_map_score: a cloud's pts is null");
  if (corner->count > (uint32_t)x->cap || surf->count > (uint32_t)x->cap)
    return fail(LOAM_E_INVAL, "loam_map_score: a cloud exceeds max_points");
  int rc = map_drain(x);
  if (rc) return rc;
  MpBuffers& b = x->mp1;
  MpScore& S = x->score;
  const int cnt[2] = {(int)corner->count, (int)surf->count};
  hipError_t he = mp_map_ensure(x->mio);
  if (he == hipSuccess) he = mp_score_reserve(S, std::max(cnt[0], cnt[1]));
  if (he != hipSuccess)
    return fail(LOAM_E_NOMEM, std::string("loam_map_score: working set allocation failed: ") + hipGetErrorString(he));
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
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    (void)hipStreamSynchronize(st);
    x->prof.collect();
    return fail(LOAM_E_HIP, std::string("loam_map_score: ") + hipGetErrorString(he));
  }
  const int* T = x->mio.tab_h;
  const int nC = T[kMapTabOff + kCubeNum], total = T[kMapTabOff + kMapKeys];
  if ((T[kMapTabInfo + 3] & ERR_CAP_MAP) || nC < 0 || total < nC || total > b.map_cap) {
    x->prof.collect();
    return fail(LOAM_E_INVAL, "loam_map_score: the last map update exceeded map_capacity, the store is not valid");
  }
  he = mp_score_reserve_map(S, nC, total - nC, cnt[0], cnt[1], (int)n);
  if (he != hipSuccess) {
    x->prof.collect();
    return fail(LOAM_E_NOMEM, std::string("loam_map_score: index allocation failed (") + std::to_string(total) +
                                  " map points): " + hipGetErrorString(he));
  }
  const bool count = x->prof.on;  // (with profiling the reduction also adds up the points and buckets the searches read)
  he = mp_score_run(S, b, x->mio, nC, total, cnt[0], cnt[1], max_dist * max_dist, (int)n, count, st, &x->prof);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    (void)hipStreamSynchronize(st);
    x->prof.collect();
    return fail(LOAM_E_HIP, std::string("loam_map_score: ") + hipGetErrorString(he));
  }
  x->prof.collect();
  if (count) {  // work counters beside the kernel times: (count, calls)
    const char* names[3] = {"score_nn_candidates", "score_nn_cells", "score_queries"};
    const double v[3] = {(double)S.work_h()[0], (double)S.work_h()[1],
                         (double)n * ((double)S.res_h()[0].corner_scored + (double)S.res_h()[0].surf_scored)};
    for (int k = 0; k < 3; ++k) {
      auto& a = x->prof.acc[names[k]];
      a.first += v[k];
      a.second += 1;
    }
  }
  std::memcpy(out, S.res_h(), (size_t)n * sizeof(loam_score_result));
  return LOAM_OK;
}

// ------------------------------------------------------------------ lanes
// S sequences in lockstep (loam.h): a step is the batch's launch sequences on the
// lanes' own working set, with the streaming path's life cycle.  What loam_chain_sweep keeps in the
// context per sequence (system_delay, the odometry's init frame and frame counter, the surround
// phase) is kept once for all lanes; what it keeps on the device (the odometry state, the Last
// clouds, the map store) is the batch buffers' per-problem state, never cleared between steps.
namespace {
// what is wrong with a lane's pushed sweep before any kernel sees it (LOAM_OK: nothing)
int lane_sweep_code(const loam_cloud_in& c, int cap) {
  if (c.count == 0) return LOAM_E_INVAL;
  if (c.data == nullptr || c.stride_bytes < 12 || c.stride_bytes % 4 != 0) return LOAM_E_INVAL;
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
  HIP_TRY(hipSetDevice(x->device));
  const hipError_t he = lanes_alloc(x->lanes, (int)n_lanes, x->cap, x->R, (int)lane_map_capacity,
                                    (int)x->cfg.od_max_iter, (int)x->cfg.mp_max_iter);
  if (he != hipSuccess) {
    (void)hipGetLastError();
    return fail(LOAM_E_NOMEM, std::string("loam_lanes_open: allocation failed: ") + hipGetErrorString(he));
  }
  Lanes& L = x->lanes;
  L.od.tune = L.mp.tune = lanes_tuning(x->tune);
  L.od_frame_count = (int)x->cfg.skip_frame_num;  // frameCount = skipFrameNum (src/laserOdometry.cpp:407)
  return LOAM_OK;
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
  HIP_TRY(hipSetDevice(x->device));
  const hipError_t he = lanes_alloc(x->lanes, (int)n_lanes, x->cap, x->R, (int)lane_from_capacity,
                                    (int)x->cfg.od_max_iter, (int)x->cfg.mp_max_iter, /*shared=*/true);
  if (he != hipSuccess) {
    (void)hipGetLastError();
    return fail(LOAM_E_NOMEM, who + ": allocation failed: " + hipGetErrorString(he));
  }
  Lanes& L = x->lanes;
  L.od.tune = L.mp.tune = lanes_tuning(x->tune);
  L.od_frame_count = (int)x->cfg.skip_frame_num;  // frameCount = skipFrameNum (src/laserOdometry.cpp:407)
  return LOAM_OK;
}

namespace {
// lanes_list_check's four rules with their messages: LOAM_OK, or the failure
int lanes_list_refused(const std::string& who, const Lanes& L, const uint32_t* lane, uint32_t n) {
  std::vector<char> seen;
  uint32_t bad = 0;
  const int why = lanes_list_check(lane, n, L.S, L.fail.data(), L.life.data(), seen, &bad);
  if (why != kLaneListOk) {
    const std::string at = who + ": lane[" + std::to_string(bad) + "] = " + std::to_string(lane[bad]);
    if (why == kLaneListRange) return fail(LOAM_E_INVAL, at + " is out of range");
    if (why == kLaneListTwice) return fail(LOAM_E_INVAL, at + " is listed twice");
    if (why == kLaneListFailed) return fail(LOAM_E_INVAL, at + " has failed (loam_lanes_restart first)");
    return fail(LOAM_E_INVAL, at + " waits for its init step (the restart's clear would overwrite the pose)");
  }
  return LOAM_OK;
}
}  // namespace

extern "C" int loam_lanes_set_pose(loam_ctx* x, uint32_t n, const uint32_t* lane, const loam_pose6* aft,
                                   const loam_pose6* bef) {
  if (!x || !lane || !aft) return fail(LOAM_E_INVAL, "null argument");
  const std::string who = "loam_lanes_set_pose";
  Lanes& L = x->lanes;
  if (!L.S) return fail(LOAM_E_INVAL, who + ": lanes are not open");
  if (!L.shared) return fail(LOAM_E_INVAL, who + ": the lanes have their own maps (loam_lanes_open); use loam_lanes_map_import");
  if (L.in_flight) return fail(LOAM_E_INVAL, who + ": a step is in flight (loam_lanes_pull first)");
  if (n == 0 || n > (uint32_t)L.S) return fail(LOAM_E_INVAL, who + ": n must be in [1, n_lanes]");
  if (const int rc = lanes_list_refused(who, L, lane, n)) return rc;
  HIP_TRY(hipSetDevice(x->device));
  if (lanes_set_pose_alloc(L) != hipSuccess) {
    (void)hipGetLastError();
    return fail(LOAM_E_NOMEM, who + ": allocation failed");
  }
  for (uint32_t i = 0; i < n; ++i) {
    L.sp_h[i] = (int)lane[i];
    std::memcpy(L.sp_h + n + (size_t)i * 12, &aft[i], sizeof(loam_pose6));
    if (bef) std::memcpy(L.sp_h + n + (size_t)i * 12 + 6, &bef[i], sizeof(loam_pose6));
    else std::memset(L.sp_h + n + (size_t)i * 12 + 6, 0, sizeof(loam_pose6));
  }
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
  if (!L.S) return fail(LOAM_E_INVAL, who + ": lanes are not open");
  if (!L.shared) return fail(LOAM_E_INVAL, who + ": the lanes have their own maps (loam_lanes_open)");
  if (L.in_flight) return fail(LOAM_E_INVAL, who + ": a step is in flight (loam_lanes_pull first)");
  if (!L.pulled) return fail(LOAM_E_INVAL, who + ": no step was pulled");
  std::memcpy(out, L.loc_info.data(), (size_t)L.S * sizeof(loam_localize_result));
  return LOAM_OK;
}

namespace {
// loam_lanes_map_commit's refusals of the call itself and of the lane list (lanes_commit_check's
// rules with their messages): LOAM_OK, or the failure
int lanes_commit_refused(const std::string& who, loam_ctx* x, const uint32_t* lane, uint32_t n) {
  Lanes& L = x->lanes;
  if (!L.S) return fail(LOAM_E_INVAL, who + ": lanes are not open");
  if (!L.shared)
    return fail(LOAM_E_INVAL, who + ": the lanes have their own maps (loam_lanes_open), which they write themselves");
  if (L.in_flight) return fail(LOAM_E_INVAL, who + ": a step is in flight (loam_lanes_pull first)");
  if (!L.pulled) return fail(LOAM_E_INVAL, who + ": no step was pulled");
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
  if (err & ERR_CAP_MAP) return fail(LOAM_E_INVAL, who + ": the last map update exceeded map_capacity, the store is not valid");
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
  if (mp_commit_alloc(L.cm, L.S, L.mp.cap_stack) != hipSuccess) {
    (void)hipGetLastError();
    return fail(LOAM_E_NOMEM, who + ": allocation failed");
  }
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
  if (!L.S) return fail(LOAM_E_INVAL, who + ": lanes are not open");
  if (L.in_flight) return fail(LOAM_E_INVAL, who + ": a step is in flight (loam_lanes_pull first)");
  if (!L.pulled || !L.od_inited)
    return fail(LOAM_E_INVAL, who + ": no step was pulled on which the odometry was initialised (no Last clouds yet)");
  if (n == 0 || n > (uint32_t)L.S) return fail(LOAM_E_INVAL, who + ": n must be in [1, n_lanes]");
  if (k == 0) return fail(LOAM_E_INVAL, who + ": k must be at least 1");
  if ((uint64_t)n * (uint64_t)k > (uint64_t)LOAM_SCORE_MAX)
    return fail(LOAM_E_INVAL, who + ": n x k must not exceed LOAM_SCORE_MAX");
  if (!(max_dist > 0.0f && max_dist <= 1.0f))
    return fail(LOAM_E_INVAL, who + ": max_dist must be in (0, 1] (the map index has 1 m cells)");
  if (const int rc = lanes_list_refused(who, L, lane, n)) return rc;
  int rc = map_drain(x);
  if (rc) return rc;
  MpBuffers& b = x->mp1;
  MpScore& S = x->score;
  const OdBuffers& o = L.od;
  hipError_t he = mp_map_ensure(x->mio);
  if (he == hipSuccess) he = mp_score_reserve(S, 0);
  if (he == hipSuccess) he = mp_score_reserve_plan(S, L.S);
  if (he != hipSuccess) {
    (void)hipGetLastError();
    return fail(LOAM_E_NOMEM, who + ": working set allocation failed: " + hipGetErrorString(he));
  }
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
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    (void)hipStreamSynchronize(st);
    x->prof.collect();
    return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
  }
  const int* T = x->mio.tab_h;
  const int nC = T[kMapTabOff + kCubeNum], total = T[kMapTabOff + kMapKeys];
  if ((T[kMapTabInfo + 3] & ERR_CAP_MAP) || nC < 0 || total < nC || total > b.map_cap) {
    x->prof.collect();
    return fail(LOAM_E_INVAL, who + ": the last map update exceeded map_capacity, the store is not valid");
  }
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
  he = mp_score_reserve_map(S, nC, total - nC, 0, 0, (int)rows);
  if (he != hipSuccess) {
    x->prof.collect();
    return fail(LOAM_E_NOMEM, who + ": index allocation failed (" + std::to_string(total) + " map points): " +
                                  hipGetErrorString(he));
  }
  const bool count = x->prof.on;  // (with profiling the kernel also adds up the points and buckets the searches read)
  he = mp_lanes_score_run(S, b, x->mio, nC, total, o.lastC, o.lastS, shape, (int)n, (int)k, max_dist * max_dist, count,
                          st, &x->prof);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    (void)hipStreamSynchronize(st);
    x->prof.collect();
    return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
  }
  x->prof.collect();
  if (count) {  // work counters beside the kernel times: (count, calls)
    double queries = 0.0;
    for (size_t r = 0; r < rows; ++r) queries += (double)S.res_h()[r].corner_scored + (double)S.res_h()[r].surf_scored;
    const char* names[3] = {"score_nn_candidates", "score_nn_cells", "score_queries"};
    const double v[3] = {(double)S.work_h()[0], (double)S.work_h()[1], queries};
    for (int c = 0; c < 3; ++c) {
      auto& a = x->prof.acc[names[c]];
      a.first += v[c];
      a.second += 1;
    }
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
  if (!L.S) return fail(LOAM_E_INVAL, who + ": lanes are not open");
  if (L.in_flight) return fail(LOAM_E_INVAL, who + ": a step is in flight (loam_lanes_pull first)");
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
  if (he != hipSuccess) {
    (void)hipGetLastError();
    return fail(LOAM_E_NOMEM, who + ": working set allocation failed: " + hipGetErrorString(he));
  }
  x->prof.begin(st);
  he = hipMemcpyAsync(Lc.nlast_h(), o.nlast, (size_t)L.S * kOdBufs * 2 * sizeof(int), hipMemcpyDeviceToHost, st);
  x->prof.mark("lanes_localize_d2h");
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    (void)hipStreamSynchronize(st);
    x->prof.collect();
    return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
  }
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
    (void)hipGetLastError();
    x->prof.collect();
    return fail(LOAM_E_NOMEM, who + ": working set allocation failed: " + hipGetErrorString(he));
  }
  Prof* pf = x->prof.on ? &x->prof : nullptr;  // (with profiling the L-M kernels also count their work)
  float* ch = Lc.cand_h();
  for (int h = 0; h < rows; ++h) {
    std::memcpy(ch + (size_t)h * 12, &aft[h], sizeof(loam_pose6));
    if (bef) std::memcpy(ch + (size_t)h * 12 + 6, &bef[h], sizeof(loam_pose6));
    else std::memset(ch + (size_t)h * 12 + 6, 0, sizeof(loam_pose6));
  }
  LocRows lr;
  lr.plan = Lc.plan;
  lr.k = (int)k;
  lr.lastC = o.lastC;
  lr.lastS = o.lastS;
  lr.od_state = o.state;
  const MpInput none = {};  // (the rows kernels read the lanes' clouds through the plan)
  he = mp_localize_prepare(Lc, s, none, rows, st, pf, &lr);
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    (void)hipStreamSynchronize(st);
    x->prof.collect();
    return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
  }
  const int* head = Lc.head_h();
  if (head[2 * rows] & ERR_CAP_MAP) {
    x->prof.collect();
    return fail(LOAM_E_INVAL, who + ": the last map update exceeded map_capacity, the store is not valid");
  }
  int from_max = 0, cloud_max = 0;
  for (int h = 0; h < rows; ++h) {
    from_max = std::max(from_max, head[2 * h] + head[2 * h + 1]);
    cloud_max = std::max(cloud_max, std::max(head[2 * h], head[2 * h + 1]));
  }
  he = mp_loc_reserve_map(Lc, from_max);
  if (he != hipSuccess) {
    (void)hipGetLastError();
    x->prof.collect();
    return fail(LOAM_E_NOMEM, who + ": FromMap allocation failed (" + std::to_string(rows) + " x " +
                                  std::to_string(from_max) + " points): " + hipGetErrorString(he));
  }
  he = mp_localize_solve(Lc, s, none, rows, from_max, cloud_max, std::max(shape.maxC, shape.maxS), st, pf, &lr);
  x->prof.mark("lanes_localize_d2h");
  if (he == hipSuccess) he = hipStreamSynchronize(st);
  if (he != hipSuccess) {
    (void)hipStreamSynchronize(st);
    x->prof.collect();
    return fail(LOAM_E_HIP, who + ": " + hipGetErrorString(he));
  }
  x->prof.collect();
  const int* R = Lc.res_h();
  for (int h = 0; h < rows; ++h) loc_result_of(R + (size_t)h * kLocResWords, out[h]);
  return LOAM_OK;
}

extern "C" int loam_lanes_close(loam_ctx* x) {
  if (!x) return fail(LOAM_E_INVAL, "null argument");
  if (!x->lanes.S) return fail(LOAM_E_INVAL, "loam_lanes_close: lanes are not open");
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
  if (!L.S) return fail(LOAM_E_INVAL, who + ": lanes are not open");
  if (L.in_flight) return fail(LOAM_E_INVAL, who + ": a step is in flight (loam_lanes_pull first)");
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
    L.fail_new[l] = waits ? LOAM_OK : lane_sweep_code(raw[l], x->cap);
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
    pack_tight_of([&](size_t s) -> const loam_cloud_in& { return eff[s]; }, (size_t)s0, (size_t)s1, off, L.stage_h);
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
void lanes_feed_inputs(const loam_cloud_in* raw, int S, int cap, int device, const int* state, std::vector<LaneFeedIn>& in) {
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
    if (!lanes_feed_looks(q, cap)) continue;
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
  if (lanes_feed_alloc(L) != hipSuccess) {
    (void)hipGetLastError();
    return fail(LOAM_E_NOMEM, who + ": the descriptor block's allocation failed");
  }
  hipStream_t prod = (hipStream_t)producer_stream;
  bool feeds = false;
  if (L.sr_inited) {  // (inside system_delay the sweeps are not looked at)
    std::vector<int> state((size_t)S);
    for (int l = 0; l < S; ++l) state[l] = L.fail[l] != LOAM_OK ? kFeedFailed : L.life[l].wait > 0 ? kFeedWaits : kFeedRuns;
    std::vector<LaneFeedIn> in;
    lanes_feed_inputs(raw, S, x->cap, x->device, state.data(), in);
    // (the last step was pulled: its copy of the descriptor block is done; the lanes' codes go into
    // fail_new only when nothing can refuse the call any more)
    std::vector<int32_t> code((size_t)S);
    uint32_t bad = 0;
    const int verdict = lanes_feed_plan(in.data(), (uint32_t)S, x->cap, L.fd_h, code.data(), &bad);
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
  HIP_TRY(lanes_gather_dev(L, x->cap, st));
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
  if (!L.S) return fail(LOAM_E_INVAL, "loam_lanes_imu: lanes are not open");
  if (lane >= (uint32_t)L.S) return fail(LOAM_E_INVAL, "loam_lanes_imu: lane index out of range");
  // (the queues a push copied and the pointers a pull commits do not change in between)
  if (L.in_flight) return fail(LOAM_E_INVAL, "loam_lanes_imu: a step is in flight (loam_lanes_pull first)");
  if (L.fail[lane] != LOAM_OK) return fail(LOAM_E_INVAL, "loam_lanes_imu: the lane has failed");
  LanesImu& I = L.imu;
  if (!(stamp >= (I.on ? I.last_stamp[lane] : -1e300)))
    return fail(LOAM_E_INVAL, "loam_lanes_imu: IMU stamps of a lane must be non-decreasing");
  if (!I.on) {  // the first message of any lane: the queues, host and device
    HIP_TRY(hipSetDevice(x->device));
    const hipError_t he = lanes_imu_alloc(L);
    if (he != hipSuccess) {
      (void)hipGetLastError();
      return fail(LOAM_E_NOMEM, std::string("loam_lanes_imu: allocation failed: ") + hipGetErrorString(he));
    }
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
  if (!L.S) return fail(LOAM_E_INVAL, "loam_lanes_restart: lanes are not open");
  if (lane >= (uint32_t)L.S) return fail(LOAM_E_INVAL, "loam_lanes_restart: lane index out of range");
  if (L.in_flight) return fail(LOAM_E_INVAL, "loam_lanes_restart: a step is in flight (loam_lanes_pull first)");
  const int s = (int)x->cfg.skip_frame_num;
  LaneLife& f = L.life[lane];
  if (L.od_inited) {
    if (!L.rs_h) {  // the first restart: the steps' lane lists
      HIP_TRY(hipSetDevice(x->device));
      const hipError_t he = lanes_restart_alloc(L);
      if (he != hipSuccess) {
        (void)hipGetLastError();
        return fail(LOAM_E_NOMEM, std::string("loam_lanes_restart: allocation failed: ") + hipGetErrorString(he));
      }
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
  if (!L.S) return fail(LOAM_E_INVAL, "loam_lanes_imu_trans: lanes are not open");
  if (L.in_flight) return fail(LOAM_E_INVAL, "loam_lanes_imu_trans: a step is in flight (loam_lanes_pull first)");
  if (!L.pulled) return fail(LOAM_E_INVAL, "loam_lanes_imu_trans: no step was pulled");
  std::memcpy(out, L.imu_trans.data(), (size_t)L.S * 12 * sizeof(float));
  return LOAM_OK;
}

extern "C" int loam_lanes_pull(loam_ctx* x, loam_lane_out* out) {
  static_assert(sizeof(loam_lane_out) == 96, "loam_lane_out layout");
  static_assert(LOAM_LANES_MAX == 1024, "loam.h");
  if (!x || !out) return fail(LOAM_E_INVAL, "null argument");
  Lanes& L = x->lanes;
  if (!L.S) return fail(LOAM_E_INVAL, "loam_lanes_pull: lanes are not open");
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
  if (!L.S) return fail(LOAM_E_INVAL, "loam_lanes_registered: lanes are not open");
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
  if (!L.S) return fail(LOAM_E_INVAL, who + ": lanes are not open");
  if (L.in_flight) return fail(LOAM_E_INVAL, who + ": a step is in flight (loam_lanes_pull first)");
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
  if (lanes_clouds_alloc(L) != hipSuccess) {
    (void)hipGetLastError();
    return fail(LOAM_E_NOMEM, who + ": the mask / table block's allocation failed");
  }
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
  if (!L.S) return fail(LOAM_E_INVAL, "loam_lanes_map_export: lanes are not open");
  if (L.shared)
    return fail(LOAM_E_INVAL, "loam_lanes_map_export: shared lanes have no lane map (loam_map_export gives the context's)");
  if (lane >= (uint32_t)L.S) return fail(LOAM_E_INVAL, "loam_lanes_map_export: lane index out of range");
  if (L.in_flight) return fail(LOAM_E_INVAL, "loam_lanes_map_export: a step is in flight (loam_lanes_pull first)");
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
  if (!L.S) return fail(LOAM_E_INVAL, who + ": lanes are not open");
  if (L.shared)
    return fail(LOAM_E_INVAL, who + ": shared lanes have no lane map (loam_map_import changes the context's, "
                                    "loam_lanes_set_pose a lane's poses)");
  if (L.in_flight) return fail(LOAM_E_INVAL, who + ": a step is in flight (loam_lanes_pull first)");
  if (n == 0 || n > (uint32_t)L.S) return fail(LOAM_E_INVAL, who + ": n must be in [1, n_lanes]");
  std::vector<char> seen;
  uint32_t bad = 0;
  const int why = lanes_list_check(lane, n, L.S, L.fail.data(), L.life.data(), seen, &bad);
  if (why != kLaneListOk) {
    const std::string at = who + ": lane[" + std::to_string(bad) + "]" +
                           (why == kLaneListRange ? "" : " = " + std::to_string(lane[bad]));
    if (why == kLaneListRange) return fail(LOAM_E_INVAL, at + " is out of range");
    if (why == kLaneListTwice) return fail(LOAM_E_INVAL, at + " is listed twice");
    if (why == kLaneListFailed) return fail(LOAM_E_INVAL, at + " has failed (loam_lanes_restart first)");
    return fail(LOAM_E_INVAL, at + " was restarted and waits for its init step: import after the lane's init step");
  }
  int rc = map_import_args(in, who);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(x->device));
  HIP_TRY(hipStreamSynchronize(x->st));
  if (!L.mi_h) {
    const hipError_t ae = lanes_map_import_alloc(L);
    if (ae != hipSuccess) {
      (void)hipGetLastError();
      return fail(LOAM_E_NOMEM, who + ": allocation failed: " + hipGetErrorString(ae));
    }
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
  if (!L.S) return fail(LOAM_E_INVAL, "loam_lanes_surround: lanes are not open");
  if (L.shared)
    return fail(LOAM_E_INVAL, "loam_lanes_surround: shared lanes have no lane map (loam_mapping_surround gives the context's)");
  if (L.in_flight) return fail(LOAM_E_INVAL, "loam_lanes_surround: a step is in flight (loam_lanes_pull first)");
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
  if (lanes_surround_alloc(L) != hipSuccess) {
    (void)hipGetLastError();
    return fail(LOAM_E_NOMEM, "loam_lanes_surround: allocation failed");
  }
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

namespace loam {
__global__ __launch_bounds__(256) void k_xfer(Xfer x) {
  for (int e = 0; e < x.n; ++e) {
    uint32_t* d = x.dst[e];
    const uint32_t* s = x.src[e];
    for (int w = threadIdx.x; w < x.words[e]; w += 256) d[w] = s ? s[w] : x.imm[x.imm_off[e] + w];
  }
}
hipError_t xfer_launch(const Xfer& x, hipStream_t st) {
  if (x.overflow) return hipErrorInvalidValue;
  if (x.n) hipLaunchKernelGGL(k_xfer, dim3(1), dim3(256), 0, st, x);
  return hipGetLastError();
}
}  // namespace loam
