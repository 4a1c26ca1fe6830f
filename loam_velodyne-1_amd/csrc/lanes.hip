// Lanes: the working set of S sequences stepped in lockstep and the kernel that gathers a step's
// per-lane results (lanes.hpp; the step itself is composed in engine.cpp from the batch kernels).
#include "lanes.hpp"

namespace loam {

namespace {
struct LaneOutSrc {
  const int* sr_err;      // [S]
  const float* od_state;  // [S][kOdStateFloats]
  const int* od_istate;   // [S][kOdStateInts]
  const float* mp_state;  // [S][kMpStateFloats]
  const int* mp_istate;   // [S][kMpStateInts]
  const int* nreg;        // [S]
};

// 32 lanes of a wave per lane of the step, one word each: the three error words, the two iteration
// counts, the registered cloud's size, transformSum, Aft, Bef
__global__ __launch_bounds__(256) void k_lanes_out(LaneOutSrc s, int* out, int S) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  const int l = gid >> 5, w = gid & 31;
  if (l >= S || w >= kLaneOutWords) return;
  const int* oi = s.od_istate + (size_t)l * kOdStateInts;
  const int* mi = s.mp_istate + (size_t)l * kMpStateInts;
  int v;
  if (w == kLoSrErr) v = s.sr_err[l];
  else if (w == kLoOdErr) v = oi[kIsErr];
  else if (w == kLoMpErr) v = mi[kMiErr];
  else if (w == kLoOdIters) v = oi[kIsIters];
  else if (w == kLoMpIters) v = mi[kMiIters];
  else if (w == kLoNReg) v = s.nreg[l];
  else if (w < kLoAft) v = __float_as_int(s.od_state[(size_t)l * kOdStateFloats + kOdSum + (w - kLoOdSum)]);
  else if (w < kLoBef) v = __float_as_int(s.mp_state[(size_t)l * kMpStateFloats + kMpAft + (w - kLoAft)]);
  else v = __float_as_int(s.mp_state[(size_t)l * kMpStateFloats + kMpBef + (w - kLoBef)]);
  out[(size_t)l * kLaneOutWords + w] = v;
}
}  // namespace

Tuning lanes_tuning(Tuning t) {
  t.od_persist = 0;
  t.mp_persist = 0;
  t.od_moments_min = LOAM_LANES_MAX + 1;
  return t;
}

hipError_t lanes_alloc(Lanes& L, int S, int cap, int R, int map_cap, int od_max_iter, int mp_max_iter) {
  hipError_t e = sr_alloc(L.sr, S, cap, R);
  if (e == hipSuccess) e = od_alloc(L.od, S, R, cap, od_max_iter);
  if (e == hipSuccess) e = mp_alloc(L.mp, S, R, cap, map_cap, mp_max_iter);
  const size_t pts = (size_t)S * cap;
  if (e == hipSuccess) e = hipHostMalloc((void**)&L.stage_h, pts * sizeof(float4), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&L.stage_d, pts * sizeof(float4));
  if (e == hipSuccess) e = hipHostMalloc((void**)&L.tab_h, (size_t)2 * S * sizeof(int), hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&L.tab_d, (size_t)2 * S * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&L.out_d, (size_t)S * kLaneOutWords * sizeof(int));
  if (e == hipSuccess) e = hipHostMalloc((void**)&L.out_h, (size_t)S * kLaneOutWords * sizeof(int), hipHostMallocDefault);
  // (the registered clouds' sizes are read by k_lanes_out on steps before the first mapping frame)
  if (e == hipSuccess) e = hipMemset(L.mp.nreg, 0, (size_t)S * sizeof(int));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    lanes_free(L);
    return e;
  }
  L.S = S;
  L.fail.assign(S, LOAM_OK);
  L.fail_new.assign(S, LOAM_OK);
  L.nreg.assign(S, 0);
  return hipSuccess;
}

void lanes_free(Lanes& L) {
  sr_free(L.sr);
  od_free(L.od);
  mp_free(L.mp);
  if (L.stage_h) (void)hipHostFree(L.stage_h);
  if (L.stage_d) (void)hipFree(L.stage_d);
  if (L.tab_h) (void)hipHostFree(L.tab_h);
  if (L.tab_d) (void)hipFree(L.tab_d);
  if (L.out_d) (void)hipFree(L.out_d);
  if (L.out_h) (void)hipHostFree(L.out_h);
  L = Lanes();
}

hipError_t lanes_out(const Lanes& L, hipStream_t st) {
  LaneOutSrc s;
  s.sr_err = L.sr.err;
  s.od_state = L.od.state;
  s.od_istate = L.od.istate;
  s.mp_state = L.mp.state;
  s.mp_istate = L.mp.istate;
  s.nreg = L.mp.nreg;
  hipLaunchKernelGGL(k_lanes_out, dim3((L.S * 32 + 255) / 256), dim3(256), 0, st, s, L.out_d, L.S);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess)
    e = hipMemcpyAsync(L.out_h, L.out_d, (size_t)L.S * kLaneOutWords * sizeof(int), hipMemcpyDeviceToHost, st);
  return e;
}

}  // namespace loam
