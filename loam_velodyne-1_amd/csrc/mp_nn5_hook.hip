// The mapping 5-NN search's diagnostic hook (dev_hooks.h: loam_dev_nn5_*): knn5_flat in the batch
// and the streaming kernels' forms beside the unlisted search knn5, on a map and queries given.
#include <vector>

#include "dev_hooks.h"
#include "mp_nn.hpp"

namespace loam {
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
