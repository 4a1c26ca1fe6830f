// Lanes (loam_lanes_*): S independent sequences in one context, advanced one sweep each per call.
// The working set is the batch's (an SrBuffers of S sweeps, an OdBuffers and an MpBuffers of S
// problems) with the streaming path's life cycle: nothing is reset between steps.  Engine-internal.
#ifndef LOAM_LANES_HPP
#define LOAM_LANES_HPP

#include <hip/hip_runtime.h>

#include <vector>

#include "engine.hpp"
#include "mp.hpp"
#include "od.hpp"

namespace loam {

// a lane's block of the step's result (k_lanes_out), 32-bit words
enum { kLoSrErr = 0, kLoOdErr, kLoMpErr, kLoOdIters, kLoMpIters, kLoNReg, kLoOdSum = 6, kLoAft = 12, kLoBef = 18,
       kLaneOutWords = 24 };

struct Lanes {
  int S = 0;           // 0: not open
  SrBuffers sr;        // S sweeps
  OdBuffers od;        // S problems; Last buffers 0 and 1 alternate, as the streaming path's
  MpBuffers mp;        // S stores
  // the step's sweeps: packed back to back in pinned memory, copied to the device staging in
  // chunks, scattered to sr.raw's stride by one kernel (as loam_batch_feed)
  float4* stage_h = nullptr;  // pinned [S * cap]
  float4* stage_d = nullptr;  // device [S * cap]
  int* tab_h = nullptr;       // pinned [2S]: sizes, then offsets
  int* tab_d = nullptr;       // device [2S]
  int* out_d = nullptr;       // device [S][kLaneOutWords]
  int* out_h = nullptr;       // pinned copy, read by loam_lanes_pull after the step's one synchronisation
  // the node state every lane shares (lockstep): scanRegistration's systemDelay counter,
  // laserOdometry's systemInited / frameCount, laserMapping's mapFrameCount
  int sr_init_count = 0;
  bool sr_inited = false, od_inited = false;
  int od_last = 0, od_frame_count = 1, map_frame_count = 4;
  // the protocol: a step pushed and not yet pulled; what that step published; whether the last
  // pulled step left registered clouds
  bool in_flight = false, step_ran = false, have_reg = false;
  int step_pub = 0, step_mapped = 0;
  std::vector<int> fail;       // [S] sticky failure of a lane (LOAM_OK: live); the host owns it
  std::vector<int> fail_new;   // [S] what the host found wrong with the pushed sweep
  std::vector<uint32_t> nreg;  // [S] registered points of the last pulled step
};

// launch choices of the lanes' L-M loops: the context's, without the two forms a lane may not take
// (the persistent one-problem kernels and the per-query moments; loam.h, loam_lanes_open)
Tuning lanes_tuning(Tuning t);
// the working set for S lanes (sweeps of cap points, R rings); on failure everything is freed
hipError_t lanes_alloc(Lanes& L, int S, int cap, int R, int map_cap, int od_max_iter, int mp_max_iter);
void lanes_free(Lanes& L);
// k_lanes_out: every lane's block into out_d, then its copy into out_h
hipError_t lanes_out(const Lanes& L, hipStream_t st);

}  // namespace loam
#endif
