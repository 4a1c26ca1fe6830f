// libloam_hip host engine: the batch step (config 4) and its three pipelines (sequential, scan
// registration ahead, the step pipeline), the feed, the downloads, and the bounded pack staging
// that loam_batch_features shares with the map and lanes downloads (engine_ctx.hpp).
#include <cstdio>

#include "engine_ctx.hpp"

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

extern "C" {

// ------------------------------------------------------------------ batch (config 4)
int loam_batch_upload(loam_ctx* x, uint32_t n, const loam_cloud_in* prev, const loam_cloud_in* cur) {
  if (!x || !prev || !cur || n == 0) return fail(LOAM_E_INVAL, "bad batch arguments");
  HIP_TRY(hipSetDevice(x->device));
  for (uint32_t i = 0; i < n; ++i) {
    int rc = check_cloud_in(prev[i], x->cap, x->pf);
    if (!rc) rc = check_cloud_in(cur[i], x->cap, x->pf);
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
      pack(c, h.data(), 0, c.count, x->pf);
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
  x->seen_sweep = true;  // (loam_set_ring_table)
  return LOAM_OK;
}

namespace {
// sweeps [s0, s1) of a batch (sweep 2i = prev[i], 2i + 1 = cur[i]) packed back to back (pack_tight_of)
void pack_tight(const loam_cloud_in* prev, const loam_cloud_in* cur, size_t s0, size_t s1, const int* off, float4* dst,
                const PointFields& pf) {
  pack_tight_of([&](size_t s) -> const loam_cloud_in& { return (s & 1) ? cur[s / 2] : prev[s / 2]; }, s0, s1, off, dst, pf);
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
    int rc = check_cloud_in(prev[i], x->cap, x->pf);
    if (!rc) rc = check_cloud_in(cur[i], x->cap, x->pf);
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
    pack_tight(prev, cur, s0, s1, off, x->feed_pin[i], x->pf);
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
  x->seen_sweep = true;  // (loam_set_ring_table)
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
  std::string err;  // (written only with a failure's code)
  int rc = mp_batch_download(x->mpbuf(x->mp_last), x->st, aft, &s, err);
  if (rc) return fail(rc, err);
  for (int i = 0; i < 2 * P; ++i) {
    s.n_ring += nfull[i];
    s.n_sharp += cnt[4 * i]; s.n_less_sharp += cnt[4 * i + 1];
    s.n_flat += cnt[4 * i + 2]; s.n_less_flat += cnt[4 * i + 3];
  }
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
namespace loam {
namespace eng {
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
}  // namespace eng
}  // namespace loam

namespace {
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
