/* Diagnostic entries of libloam_hip.so that are not part of the public C-ABI (include/loam/): they run
 * internal routines of the engine on caller-supplied data, for the test suite.  Exported, undocumented
 * for users, free to change.  Return LOAM_OK or a negative LOAM_E_* code (include/loam/loam.h). */
#ifndef LOAM_DEV_HOOKS_H
#define LOAM_DEV_HOOKS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The segmented VoxelGrid (vg.hip vg_run) through the product's three routes.  A handle owns the
 * device scratch a mapping instance would (sort arrays, cascade lists and counters, input / merge
 * lists, nold / skip, the split's buffers); consecutive jobs reuse it as consecutive frames do. */
typedef struct loam_dev_vg loam_dev_vg;

#define LOAM_DEV_VG_STACK 0    /* mp_stack_vg: the stacks of P instances */
#define LOAM_DEV_VG_CUBES 1    /* the map update's valid-cube segments of P instances */
#define LOAM_DEV_VG_SURROUND 2 /* mp_stream_surround: one segment */

typedef struct {
  const float* pts;     /* [total][4] x, y, z, intensity */
  int32_t total;
  int32_t nseg;
  const int32_t* begin; /* [nseg] segment s is pts[begin[s] .. end[s]); ascending, gaps and empty ones allowed */
  const int32_t* end;   /* [nseg] */
  const float* leaf;    /* [nseg] */
  const int32_t* nold;  /* [nseg] or NULL (= 0): leading points that are a previous VoxelGrid output (cubes) */
  /* the route, by the product's own decision inputs */
  int32_t route;        /* LOAM_DEV_VG_* */
  int32_t P;            /* instance count (P <= 4 against P > 4 chooses the first kernel) */
  int32_t vg_split, vg_merge, vg_merge_min; /* the tuning values of loam_set_tuning */
  int32_t capS;         /* the surf capacity (vg_split 1's rule) */
  int32_t stack_max;    /* the longest stack the host knows of, or -1 (stack route) */
} loam_dev_vg_job;

/* LOAM_E_HIP without a GPU (no CPU path), LOAM_E_INVAL for bad arguments, LOAM_E_NOMEM */
int loam_dev_vg_create(int device, int32_t max_total_points, int32_t max_segments, loam_dev_vg** out);

/* out_pts [total][4]: first filled with the sentinel LOAM_DEV_VG_SENTINEL (every word), then segment
 * s's output at begin[s]; out_count [nseg]: -1 where no kernel wrote a count; merged [nseg]: the
 * segment's skip flag (1: k_vg_merge wrote it) on the cube route with vg_merge, else -1.
 * LOAM_E_INVAL for a job beyond the handle's sizes, segments out of range or overlapping, a leaf
 * that is not positive, nold outside [0, n], an unknown route, more than one surround segment. */
#define LOAM_DEV_VG_SENTINEL 0x7fc5a5a5u /* a quiet NaN */
int loam_dev_vg_run(loam_dev_vg* h, const loam_dev_vg_job* job, float* out_pts, int32_t* out_count, int32_t* merged);

int loam_dev_vg_destroy(loam_dev_vg* h);

#ifdef __cplusplus
}
#endif
#endif
