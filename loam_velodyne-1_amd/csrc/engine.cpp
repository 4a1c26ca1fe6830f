// libloam_hip: host engine behind the C-ABI of include/loam/loam.h.
//
// A context owns one HIP device, one stream and the device-resident state the four reference
// nodes keep in globals: the scan-registration delay counter, the odometry transform / Last
// clouds / their voxel hashes, and the mapping cube store.  Every entry point uploads the
// caller's host cloud(s), runs the kernels of sr.hip / od.hip / mp.hip on the context stream and
// copies the results back; nothing here computes a point on the CPU (a missing GPU or kernel
// image fails loudly with LOAM_E_HIP).
//
// This file: the context's life cycle, tuning, profiling, the streaming nodes and k_xfer.  The
// batch step is in engine_batch.cpp, the map services in engine_map.cpp, the lanes in
// engine_lanes.cpp; struct loam_ctx and the helpers they share are in engine_ctx.hpp.
#include <cmath>
#include <cstddef>
#include <cstdio>

#include "engine_ctx.hpp"
#include "ring_table.hpp"

namespace {
thread_local std::string g_err;
}  // namespace

namespace loam {
void set_last_error(const std::string& msg) { g_err = msg; }

namespace eng {

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int check_cloud_in(const loam_cloud_in& c, int cap, const PointFields& pf) {
  if (c.count > 0 && c.data == nullptr) return fail(LOAM_E_INVAL, "cloud data is null");
  if (c.stride_bytes < 12 || c.stride_bytes % 4 != 0) return fail(LOAM_E_INVAL, "bad stride_bytes");
  if (pf.on && c.stride_bytes < pf.end) return fail(LOAM_E_INVAL, "bad stride_bytes: a record ends before the context's point fields do");
  if (c.count > (uint32_t)cap) return fail(LOAM_E_CAPACITY, "cloud exceeds max_points");
  return LOAM_OK;
}

// (records need not be 4-byte aligned: a PointCloud2's data follows a variable-length header in
// the message, and loam_pc2_cloud hands it over in place)
// points [i0, i1) of c into dst[i0 ..) as float4.  Without point fields w is not read by the
// device: a 16-byte stride is copied as is.  With them w is the point's word (its ring, or ring +
// tau, negative = dropped: point_fields.hpp), which the ring kernels' field instantiations read;
// the caller's own fourth word never reaches it.
void pack(const loam_cloud_in& c, float4* dst, size_t i0, size_t i1, const PointFields& pf) {
  const char* base = (const char*)c.data;
  if (pf.on) {
    for (size_t i = i0; i < i1; ++i) {
      const unsigned char* rec = (const unsigned char*)base + i * c.stride_bytes;
      float q[3];
      std::memcpy(q, rec, sizeof(q));
      dst[i] = make_float4(q[0], q[1], q[2], field_word_of_record(pf, rec));
    }
    return;
  }
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

int sr_errors(int e) {
  if (e & ERR_EMPTY) return fail(LOAM_E_INVAL, "sweep has no finite point");
  if (e & ERR_CAP_RING) return fail(LOAM_E_CAPACITY, "a ring span exceeds the per-ring capacity");
  return LOAM_OK;
}

void count_bytes(loam_stats& s) {
  // algorithmic bytes, SURVEY.md §8(d)
  s.bytes_sr = 16 * s.n_raw + 32 * s.n_ring + 16 * (s.n_sharp + s.n_less_sharp + s.n_flat + s.n_less_flat);
  s.bytes_od = 16 * s.od_assoc_points + 16 * s.od_queries + 12 * s.od_queries + 32 * s.od_rows_sum;
  s.bytes_mp = 16 * s.mp_map_points + 96 * s.mp_stack_iters + 64 * s.mp_rows_sum + 32 * s.mp_stack +
               32 * s.mp_map_valid_points;
}

}  // namespace eng
}  // namespace loam

namespace {
int upload_cloud(hipStream_t st, Staging& pin, const loam_cloud_out& c, float4* dev, int cap) {
  if (c.count > (uint32_t)cap) return fail(LOAM_E_CAPACITY, "input feature cloud exceeds capacity");
  if (c.count > 0) {
    if (c.pts == nullptr) return fail(LOAM_E_INVAL, "feature cloud pts is null");
    HIP_TRY(pin.up(st, dev, c.pts, (size_t)c.count));
  }
  return LOAM_OK;
}
}  // namespace

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

// ------------------------------------------------------------------ ring tables (ring_table.hpp)
int loam_ring_table_check(uint32_t n_rings, uint32_t n, const float* bound_deg, const int32_t* ring) {
  const int why = ring_table_check_why(n_rings, n, bound_deg, ring);
  if (why != kRingTableOk) return fail(LOAM_E_INVAL, std::string("loam_ring_table_check: ") + ring_table_why_text(why));
  return LOAM_OK;
}

int loam_ring_table_of_model(const loam_config* cfg, uint32_t* n, float* bound_deg, int32_t* ring) {
  const std::string who = "loam_ring_table_of_model: ";
  if (!cfg) return fail(LOAM_E_INVAL, who + "null argument");
  if (cfg->n_rings < 2 || cfg->n_rings > 64) return fail(LOAM_E_INVAL, who + ring_table_why_text(kRingTableRings));
  const int why = ring_table_of_model_why((int)cfg->ring_model, (int)cfg->n_rings, cfg->ring_lo_deg, cfg->ring_hi_deg, n,
                                          bound_deg, ring);
  if (why != kRingTableOk) return fail(LOAM_E_INVAL, who + ring_table_why_text(why));
  return LOAM_OK;
}

int loam_set_ring_table(loam_ctx* x, uint32_t n, const float* bound_deg, const int32_t* ring) {
  const std::string who = "loam_set_ring_table: ";
  if (!x) return fail(LOAM_E_INVAL, who + "null argument");
  if (x->seen_sweep)
    return fail(LOAM_E_INVAL, who + "the context has seen a sweep (the ring model is set before the first one)");
  const int why = ring_table_check_why((uint32_t)x->R, n, bound_deg, ring);
  if (why != kRingTableOk) return fail(LOAM_E_INVAL, who + ring_table_why_text(why));
  HIP_TRY(hipSetDevice(x->device));
  SrParams p;
  p.R = x->R;
  p.ring_model = LOAM_RING_TABLE;
  SrRingTab t;
  const hipError_t he = sr_ring_tab_alloc(t, p, bound_deg, ring, (int)n);  // (synchronous copies: nothing of the caller's is read later)
  if (he == hipErrorOutOfMemory) return nomem(who + "allocation failed");
  if (he != hipSuccess) return fail(LOAM_E_HIP, who + hipGetErrorString(he));
  sr_ring_tab_free(x->ring_tab);  // (no launch has read it: the context has seen no sweep)
  x->ring_tab = t;
  x->tb_n = (int)n;
  std::memcpy(x->tb_bound, bound_deg, ((size_t)n + 1) * sizeof(float));
  std::memcpy(x->tb_ring, ring, (size_t)n * sizeof(int32_t));
  return LOAM_OK;
}

// ------------------------------------------------------------------ point fields (point_fields.hpp)
int loam_point_fields_check(uint32_t n_rings, const loam_point_fields* f) {
  const int why = point_fields_check_why(n_rings, f);
  if (why != kFieldsOk) return fail(LOAM_E_INVAL, std::string("loam_point_fields_check: ") + point_fields_why_text(why));
  return LOAM_OK;
}

int loam_set_point_fields(loam_ctx* x, const loam_point_fields* f) {
  const std::string who = "loam_set_point_fields: ";
  if (!x) return fail(LOAM_E_INVAL, who + "null argument");
  if (x->seen_sweep)
    return fail(LOAM_E_INVAL, who + "the context has seen a sweep (the point fields are set before the first one)");
  if (!f) {  // back to the ring model or table
    x->pf = PointFields();
    return LOAM_OK;
  }
  const int why = point_fields_check_why((uint32_t)x->R, f);
  if (why != kFieldsOk) return fail(LOAM_E_INVAL, who + point_fields_why_text(why));
  HIP_TRY(hipSetDevice(x->device));
  const PointFields pf = point_fields_of((uint32_t)x->R, *f);
  if (!x->pf_map_d) {
    const hipError_t he = hipMalloc((void**)&x->pf_map_d, sizeof(pf.map));
    if (he != hipSuccess) {
      x->pf_map_d = nullptr;
      if (he == hipErrorOutOfMemory) return nomem(who + "allocation failed");
      return fail(LOAM_E_HIP, who + hipGetErrorString(he));
    }
  }
  // (a synchronous copy, and no launch reads the map: the context has seen no sweep)
  HIP_TRY(hipMemcpy(x->pf_map_d, pf.map, sizeof(pf.map), hipMemcpyHostToDevice));
  x->pf = pf;
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
  if (x->pf_map_d) (void)hipFree(x->pf_map_d);
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
  int rc = check_cloud_in(raw, x->cap, x->pf);
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
    pack(raw, praw, i0, i1, x->pf);
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
  const int rc = sr_frame(x, stamp, raw, out, cnt5, imu12);
  if (rc == LOAM_OK) x->seen_sweep = true;  // (loam_set_ring_table)
  return rc;
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
  x->seen_sweep = true;  // (loam_set_ring_table: the sweep's rings are the model's from here on)
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
}  // extern "C"

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
