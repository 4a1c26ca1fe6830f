// loam_lanes_localize's host-side planning: host only, no HIP.
#ifndef LOAM_LOC_PLAN_HPP
#define LOAM_LOC_PLAN_HPP

#include <cstdint>

namespace loam {

constexpr uint32_t kLocPlanRows = 1024;  // LOAM_LOCALIZE_MAX (mp.hpp kLocMax)
constexpr uint32_t kLocPlanBufs = 3;     // od.hpp kOdBufs

// one listed lane of a call, as the rows kernels read it: where its Last clouds lie (elements from
// OdBuffers::lastC / lastS), their sizes, and the lane itself (its transformSum in the odometry state)
struct LaneLocPlan {
  uint64_t offC, offS;
  int32_t nC, nS;
  uint32_t lane;
  uint32_t pad;
};
static_assert(sizeof(LaneLocPlan) == 32, "LaneLocPlan layout");
// the call: n x k rows, and the largest listed corner / surf cloud (what sizes the rows' stacks)
struct LaneLocShape {
  uint32_t rows;
  int32_t maxC, maxS;
};
enum { kLocPlanOk = 0, kLocPlanN, kLocPlanK, kLocPlanTooMany, kLocPlanCap, kLocPlanLane, kLocPlanCount, kLocPlanStack };
// loam_lanes_localize's arithmetic: kLocPlanOk and plan[0..n) / shape, or which limit the arguments
// break (nothing is written then).  lane[i] < P is listed lane i, cnt[2 i] / cnt[2 i + 1] the corner
// / surf count of its Last clouds in buffer buf of [kOdBufs][P][capC | capS]; stack_capC is the
// mapping stack's corner bound (loam_map_localize refuses a larger corner cloud).  Every product is
// formed in 64 bits; capC + capS must be an int (a stack segment's length is one).
inline int lanes_localize_plan(uint32_t n, uint32_t k, const uint32_t* lane, const int32_t* cnt, uint32_t P, uint32_t buf,
                               int32_t capC, int32_t capS, int32_t stack_capC, LaneLocPlan* plan, LaneLocShape* shape) {
  if (n == 0 || n > P) return kLocPlanN;
  if (k == 0) return kLocPlanK;
  if ((uint64_t)n * (uint64_t)k > (uint64_t)kLocPlanRows) return kLocPlanTooMany;
  if (capC < 0 || capS < 0 || stack_capC < 0 || (int64_t)capC + (int64_t)capS > (int64_t)0x7fffffff || buf >= kLocPlanBufs)
    return kLocPlanCap;
  for (uint32_t i = 0; i < n; ++i) {
    if (lane[i] >= P) return kLocPlanLane;
    if (cnt[2 * i] < 0 || cnt[2 * i] > capC || cnt[2 * i + 1] < 0 || cnt[2 * i + 1] > capS) return kLocPlanCount;
    if (cnt[2 * i] > stack_capC) return kLocPlanStack;
  }
  int32_t maxC = 0, maxS = 0;
  for (uint32_t i = 0; i < n; ++i) {
    LaneLocPlan& p = plan[i];
    const uint64_t slot = (uint64_t)buf * P + lane[i];
    p.offC = slot * (uint64_t)capC;
    p.offS = slot * (uint64_t)capS;
    p.nC = cnt[2 * i];
    p.nS = cnt[2 * i + 1];
    p.lane = lane[i];
    p.pad = 0;
    if (p.nC > maxC) maxC = p.nC;
    if (p.nS > maxS) maxS = p.nS;
  }
  shape->rows = n * k;
  shape->maxC = maxC;
  shape->maxS = maxS;
  return kLocPlanOk;
}

}  // namespace loam
#endif
