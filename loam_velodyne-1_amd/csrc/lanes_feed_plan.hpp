// loam_lanes_push_device's host-side planning: host only, no HIP.
#ifndef LOAM_LANES_FEED_PLAN_HPP
#define LOAM_LANES_FEED_PLAN_HPP

#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace loam {

// what k_lanes_gather_dev reads of a lane: where its sweep lies, its points (0: the lane does not
// feed) and the records' stride in bytes
struct LaneFeedDesc {
  uint64_t ptr;
  int32_t n;
  int32_t stride;
};
static_assert(sizeof(LaneFeedDesc) == 16, "LaneFeedDesc layout");

// a lane on the step about to be enqueued
enum { kFeedRuns = 0, kFeedWaits, kFeedFailed };
// a lane's failure code, with loam.h's values (LOAM_OK, LOAM_E_INVAL, LOAM_E_CAPACITY)
enum { kFeedLaneOk = 0, kFeedLaneInval = -1, kFeedLaneCapacity = -2 };
// the call's verdict
enum { kFeedOk = 0, kFeedNotDevice, kFeedRange };

// one lane as the caller handed it over, and what the entry point found out about its pointer:
// the allocation around it (base, size) and whether that is device memory of the context's device.
// base / size / on_device are read only where lanes_feed_looks() holds.
struct LaneFeedIn {
  uintptr_t ptr;
  uint32_t count;
  uint32_t stride;
  int32_t state;  // kFeed{Runs, Waits, Failed}
  int32_t on_device;
  uintptr_t base;
  uint64_t size;
};

// lane_sweep_code's rules and the device form's own (a 4-byte aligned pointer): what is wrong with
// the lane's sweep before its memory is looked at
// fields_end (here and below): the end of the context's point fields in a record
// (loam_set_point_fields), 0 without them
inline int lanes_feed_lane_code(uintptr_t ptr, uint32_t count, uint32_t stride, int32_t cap, uint32_t fields_end = 0) {
  if (count == 0) return kFeedLaneInval;
  if (ptr == 0 || stride < 12 || stride % 4 != 0 || ptr % 4 != 0 || stride < fields_end) return kFeedLaneInval;
  if (cap < 0 || count > (uint32_t)cap) return kFeedLaneCapacity;
  return kFeedLaneOk;
}

// whether the lane's sweep is read this step: only then is its pointer looked up
inline bool lanes_feed_looks(const LaneFeedIn& in, int32_t cap, uint32_t fields_end = 0) {
  return in.state == kFeedRuns && lanes_feed_lane_code(in.ptr, in.count, in.stride, cap, fields_end) == kFeedLaneOk;
}

// the bytes read of a record: x, y, z; a 16-byte stride is read whole (w is copied, as the host
// form's memcpy copies it); with point fields, each field to its end as well, rounded up to the
// dword the gather reads it in (a U8 / U16 field is read as the aligned dword that holds it)
inline uint32_t lanes_feed_record(uint32_t stride, uint32_t fields_end = 0) {
  const uint32_t xyz = stride == 16 ? 16u : 12u;
  const uint32_t end4 = (fields_end + 3u) & ~3u;
  return end4 > xyz ? end4 : xyz;
}

// whether the lane's bytes [ptr, ptr + (count - 1) stride + record) lie inside [base, base + size);
// count >= 1.  Nothing is added to a pointer: the span is formed in 64 bits (count < 2^31 and stride
// < 2^32: below 2^63) and compared with what the allocation has left behind ptr.
inline bool lanes_feed_in_range(uintptr_t ptr, uint32_t count, uint32_t stride, uintptr_t base, uint64_t size,
                                uint32_t fields_end = 0) {
  if (ptr < base) return false;
  const uint64_t lead = (uint64_t)ptr - (uint64_t)base;
  if (lead > size) return false;
  const uint64_t span = (uint64_t)(count - 1) * (uint64_t)stride + lanes_feed_record(stride, fields_end);
  return span <= size - lead;
}

// The call: kFeedOk with desc[0..S) and code[0..S) written, or the rule lane *bad breaks, with
// nothing written.  A lane that waits or has failed gets n = 0 and kFeedLaneOk whatever it holds; a
// lane whose sweep fails lanes_feed_lane_code gets n = 0 and that code; every other lane must lie in
// device memory of the context's device (kFeedNotDevice) and inside its allocation (kFeedRange).
inline int lanes_feed_plan(const LaneFeedIn* in, uint32_t S, int32_t cap, LaneFeedDesc* desc, int32_t* code,
                           uint32_t* bad, uint32_t fields_end = 0) {
  for (uint32_t l = 0; l < S; ++l) {
    const LaneFeedIn& q = in[l];
    if (!lanes_feed_looks(q, cap, fields_end)) continue;
    *bad = l;
    if (!q.on_device) return kFeedNotDevice;
    if (!lanes_feed_in_range(q.ptr, q.count, q.stride, q.base, q.size, fields_end)) return kFeedRange;
  }
  for (uint32_t l = 0; l < S; ++l) {
    const LaneFeedIn& q = in[l];
    const bool looks = lanes_feed_looks(q, cap, fields_end);
    code[l] = q.state == kFeedRuns ? lanes_feed_lane_code(q.ptr, q.count, q.stride, cap, fields_end) : kFeedLaneOk;
    desc[l].ptr = looks ? (uint64_t)q.ptr : 0;
    desc[l].n = looks ? (int32_t)q.count : 0;
    desc[l].stride = looks ? (int32_t)q.stride : 0;
  }
  return kFeedOk;
}

// the refusal's message (verdict != kFeedOk)
inline void lanes_feed_message(int verdict, uint32_t lane, char* buf, size_t len) {
  const char* what = verdict == kFeedNotDevice ? "data is not device memory of the context's device"
                                               : "the sweep leaves its allocation";
  std::snprintf(buf, len, "lane %u: %s", (unsigned)lane, what);
}

}  // namespace loam
#endif
