// Segmented PCL VoxelGrid (vg.hip): job descriptions, the cascade's scratch memory and the three
// routes the mapping code and the diagnostic hook (dev_hooks.h) launch it through (engine-internal).
#ifndef LOAM_VG_HPP
#define LOAM_VG_HPP

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "dev_common.hpp"

namespace loam {

// the voxel frame of a segment (PCL VoxelGrid's min_b and divb multipliers), for sub-segments that
// take their parent's (vg_run's big-segment split)
struct VgFrame {
  int m0, m1, m2, divx, divy, pad;
};

// segmented PCL VoxelGrid job (segment s: input in[begin[s] .. end[s]), output out[begin[s] ..))
struct VgJob {
  const float4* in;
  float4* out;
  const int* begin;
  const int* end;
  const float* leaf;     // per segment
  int* out_count;        // per segment
  uint32_t *keys, *keys_alt, *vals, *vals_alt;  // k_vg_big's global sort arrays (indexed like in)
  int nseg;
  int total;             // size of in / out / keys arrays
  // vg_run's cascade: lists[0] / lists[1] ([nseg] segment ids) and their lengths counts[0] / [1]
  // (device); a kernel processes every segment, or the ids of list / *list_n, and appends the
  // segments beyond its capacity to big / *big_n
  int* lists[2] = {nullptr, nullptr};
  int* counts = nullptr;   // [3]: the two lists' lengths, and the length of the caller's input list
  // set by the caller: counts[0] / counts[1] already zeroed by an earlier kernel on the stream
  bool zeroed = false;
  const int* list = nullptr;
  const int* list_n = nullptr;
  int* big = nullptr;
  int* big_n = nullptr;
  // incremental cube VoxelGrid (k_vg_merge): per segment the count of its leading points that are the
  // cube's previous VoxelGrid output, the candidate list, and the per-segment "done" flags the
  // cascade's first kernel skips
  const int* nold = nullptr;
  const int* mlist = nullptr;
  const int* mlist_n = nullptr;
  int* skip = nullptr;
  // per segment: the voxel frame to use instead of the segment's own bounding box (sub-segments of a
  // split parent); nullptr: every segment computes its own
  const VgFrame* frame = nullptr;
  int grid_max = 1 << 30;  // the first kernel's grid at most (the split's sub-job)
};

// vg_run's split of the segments beyond the LDS tiers (the HDL-64E surf stacks): each parent's
// points re-ordered stably into 16 buckets by the top bits of their voxel key (k_vg_split), the
// buckets VoxelGridded as sub-segments in the parent's frame by the LDS cascade, their outputs
// concatenated in bucket order (k_vg_join).  Sub-segment li * 16 + d; pts / out indexed like the
// job's input
struct VgSplit {
  float4* pts = nullptr;
  float4* out = nullptr;
  int *begin = nullptr, *end = nullptr, *out_count = nullptr;
  float* leaf = nullptr;
  VgFrame* frame = nullptr;
  int* lists[2] = {nullptr, nullptr};
  int* ilist = nullptr;   // the non-empty sub-segments (the cascade's input list)
  int* counts = nullptr;  // [3]: the cascade's two lists, ilist
  int npar = 0;           // parents it holds (list entries beyond go to k_vg_big)
};

// The cascade's device memory, owned in one place: the global sort arrays, the two cascade lists,
// the list counters and the big-segment split.  counts is [4]: the two cascade lists, then the
// caller's input list and the caller's merge list (the lists themselves are the caller's).
struct VgScratch {
  uint32_t *keys = nullptr, *keys_alt = nullptr, *vals = nullptr, *vals_alt = nullptr;  // [sort_points]
  int* lists[2] = {nullptr, nullptr};  // [segments]
  int* counts = nullptr;               // [4]
  VgSplit split;
  // a job on this scratch (sort arrays, lists, counts); the caller fills in its segments
  VgJob job() const {
    VgJob j;
    j.keys = keys; j.keys_alt = keys_alt; j.vals = vals; j.vals_alt = vals_alt;
    j.lists[0] = lists[0]; j.lists[1] = lists[1]; j.counts = counts;
    return j;
  }
};
// sort_points: entries of each sort array; segments: entries of each cascade list; the split holds
// split_parents parents (16 sub-segments each) and split_points points.  On failure: freed, s empty
hipError_t vg_scratch_alloc(VgScratch& s, size_t sort_points, size_t segments, int split_parents,
                            size_t split_points);
void vg_scratch_free(VgScratch& s);

constexpr int kVgMergeNew = 8192;  // appended points k_vg_merge sorts at most (vg.hip)
// a cube segment of n points whose first nold are its previous VoxelGrid output goes on the merge list
// (k_mp_vseg; the diagnostic hook loam_dev_vg_run)
LOAM_HD bool vg_merge_eligible(int n, int nold, int merge_min) {
  return n > merge_min && nold > 0 && n - nold <= kVgMergeNew;
}

// The three VoxelGrid routes: which cascade a job takes, from the decision inputs the product has.
// The product's call sites and the diagnostic hook (loam_dev_vg_run) both go through these.
hipError_t vg_route_stack(const VgJob& js, hipStream_t st, int P, int stack_max, int vg_split, int capS,
                          const VgSplit* vgs);
hipError_t vg_route_cubes(VgJob jv, hipStream_t st, int P, int vg_merge, const int* nold, const int* mlist,
                          const int* mlist_n, int* skip);
// (the surround map: one segment, or the due lanes' segments through j.list; first tier by j.nseg)
hipError_t vg_route_surround(const VgJob& j, hipStream_t st);

}  // namespace loam
#endif
