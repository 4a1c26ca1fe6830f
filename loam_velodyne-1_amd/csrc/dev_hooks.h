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

/* The mapping 5-NN search (mp_nn.hpp: mp_nn_seed_from + knn5_flat, and the plain knn5) on a caller's
 * map points and queries: the map's 1 m voxel hash is built by the product's hash build, then one
 * kernel runs both searches on every query from the same start. */
typedef struct loam_dev_nn5 loam_dev_nn5;

#define LOAM_DEV_NN5_MAX_MAP 16384
#define LOAM_DEV_NN5_MAX_QUERIES 4096
#define LOAM_DEV_NN5_BATCH 0  /* a lane per query, one-wave workgroups (k_mp_nnfit's form) */
#define LOAM_DEV_NN5_STREAM 1 /* a lane group per query, lists merged (k_mp_lm_small / k_mp_lm_stream's form) */
#define LOAM_DEV_NN5_OVERFLOW 1 /* flags: a lane of the query filled its pending list and inserted directly */
#define LOAM_DEV_NN5_PLAIN 2    /* flags: the flat search fell back to the plain one */

typedef struct {
  const float* map;        /* [n_map][4] x, y, z, - */
  int32_t n_map;           /* 1 .. LOAM_DEV_NN5_MAX_MAP */
  const float* queries;    /* [n_queries][4] x, y, z, - (map frame) */
  int32_t n_queries;       /* 1 .. LOAM_DEV_NN5_MAX_QUERIES */
  const int32_t* seeds;    /* NULL: unseeded (a first iteration); else [n_queries][5] map indices */
  const int32_t* distinct; /* NULL (every query's seeds count) or [n_queries]: 0 = that query starts unseeded */
  int32_t form;            /* LOAM_DEV_NN5_* */
} loam_dev_nn5_job;

/* LOAM_E_HIP without a GPU, LOAM_E_NOMEM */
int loam_dev_nn5_create(int device, loam_dev_nn5** out);

/* flat_idx / flat_dist, plain_idx / plain_dist [n_queries][5]: the list of knn5_flat and of knn5,
 * ascending: the map index (0x7fffffff: none) and the bits of the float squared distance.
 * flags [n_queries] or NULL: LOAM_DEV_NN5_OVERFLOW | LOAM_DEV_NN5_PLAIN; counts [2]: the queries
 * with each flag.  LOAM_E_INVAL for sizes out of range, a seed outside the map, an unknown form. */
int loam_dev_nn5_run(loam_dev_nn5* h, const loam_dev_nn5_job* job, int32_t* flat_idx, uint32_t* flat_dist,
                     int32_t* plain_idx, uint32_t* plain_dist, int32_t* flags, int32_t* counts);

int loam_dev_nn5_destroy(loam_dev_nn5* h);

/* The odometry association's nearest neighbour (od.hip) on a caller's Last cloud and queries: the
 * cloud's 1 m voxel hash and chunk boxes are built by the product's hash build (the odometry form),
 * then every query is searched by the lane-per-query first stage (lane_hash_nn, k_od_sel_nn's) and by
 * the wave-per-query search (wave_hash_nn, k_od_assoc's). */
typedef struct loam_dev_od_nn loam_dev_od_nn;

#define LOAM_DEV_OD_NN_MAX_CLOUD 16384
#define LOAM_DEV_OD_NN_MAX_QUERIES 4096

typedef struct {
  const float* cloud;   /* [n_cloud][4] x, y, z, intensity: its integer part is the ring, 0 .. 255 */
  int32_t n_cloud;      /* 1 .. LOAM_DEV_OD_NN_MAX_CLOUD */
  const float* queries; /* [n_queries][4] x, y, z, - (the cloud's frame) */
  int32_t n_queries;    /* 1 .. LOAM_DEV_OD_NN_MAX_QUERIES */
  const int32_t* seeds; /* NULL: every query unseeded; else [n_queries] cloud indices, -1 = unseeded */
} loam_dev_od_nn_job;

/* LOAM_E_HIP without a GPU, LOAM_E_NOMEM */
int loam_dev_od_nn_create(int device, loam_dev_od_nn** out);

/* Keys are (bits of the float squared distance << 32 | cloud index << 8 | ring); ~0: none.
 * lane_key [n_queries]: the lane search's word (~0 where it left the query to the wave: no point of
 * its cells below 1 m2); wave_key: wave_hash_nn's result (its chunk stage included); chunk_key (or
 * NULL): wave_chunk_nn alone, what k_od_assoc runs for a query the lane left; left [n_queries]: 1
 * where lane_key is ~0.  LOAM_E_INVAL for sizes out of range, a seed outside [-1, n_cloud), a ring
 * outside 0 .. 255, null pointers. */
int loam_dev_od_nn_run(loam_dev_od_nn* h, const loam_dev_od_nn_job* job, uint64_t* lane_key, uint64_t* wave_key,
                       uint64_t* chunk_key, int32_t* left);

int loam_dev_od_nn_destroy(loam_dev_od_nn* h);

/* One association round of the odometry (od.hip od_assoc_round: k_od_sel / k_od_sel_nn and k_od_assoc,
 * the launches od_solve makes every fifth iteration) on up to LOAM_DEV_OD_ASSOC_MAX_P caller-made
 * problems.  A handle owns an OdBuffers of the product's od_alloc and the feature buffers of a FeatView;
 * consecutive jobs reuse it.  The transform is zero, so TransformToStart leaves the queries as given. */
typedef struct loam_dev_od_assoc loam_dev_od_assoc;

#define LOAM_DEV_OD_ASSOC_MAX_P 4
#define LOAM_DEV_OD_ASSOC_MAX_CLOUD 16384
#define LOAM_DEV_OD_ASSOC_MAX_QUERIES 8192 /* per kind: the forward walk ends at min(queries of the kind, cloud
                                              size) (Q11), so a walk past 4096 points takes as many queries */
#define LOAM_DEV_OD_ASSOC_MAX_GRID 16384
#define LOAM_DEV_OD_ASSOC_SENTINEL (-0x5a5a5a5b) /* neither -1 nor an index */

typedef struct {
  const float* corner_last;    /* [n_corner_last][4] x, y, z, intensity: its integer part is the ring, 0 .. 63 */
  int32_t n_corner_last;       /* 1 .. LOAM_DEV_OD_ASSOC_MAX_CLOUD */
  const float* surf_last;      /* [n_surf_last][4] */
  int32_t n_surf_last;         /* 1 .. LOAM_DEV_OD_ASSOC_MAX_CLOUD */
  const float* corner_q;       /* [n_corner_q][4] raw sharp points (w: a whole number), NULL when there are none */
  int32_t n_corner_q;          /* 0 .. LOAM_DEV_OD_ASSOC_MAX_QUERIES */
  const float* surf_q;         /* [n_surf_q][4] raw flat points */
  int32_t n_surf_q;            /* 0 .. LOAM_DEV_OD_ASSOC_MAX_QUERIES; n_corner_q + n_surf_q >= 1 */
  const int32_t* corner_seeds; /* NULL or [n_corner_q][3]: the previous round's ind1, ind2, ind3 (indices of */
  const int32_t* surf_seeds;   /* the kind's Last cloud, -1: none); [n_surf_q][3] */
} loam_dev_od_assoc_problem;

typedef struct {
  const loam_dev_od_assoc_problem* prob; /* [P] */
  int32_t P;                             /* 1 .. LOAM_DEV_OD_ASSOC_MAX_P */
  /* the tuning values od_assoc_round and the kernels read (loam_set_tuning's ranges) */
  int32_t od_sel_min, od_nn_lane, od_nn_lane_min, od_win_mono, od_win_mono_min;
  int32_t grid;      /* k_od_assoc's workgroups per problem, 0 .. LOAM_DEV_OD_ASSOC_MAX_GRID; 0: the product's rule */
  int32_t count;     /* 1: the COUNT instantiations (the work counters), 0: the plain ones */
  int32_t hash_form; /* od_build_hashes' form: 0 the product's rule (a grid per cloud for P <= 4), 1 the grid
                        per cloud, 2 a workgroup per cloud */
} loam_dev_od_assoc_job;

/* LOAM_E_HIP without a GPU (no CPU path), LOAM_E_NOMEM */
int loam_dev_od_assoc_create(int device, loam_dev_od_assoc** out);

/* A job with any seeds runs as a seeded round (kIsIters > 0, iteration 5; a problem or kind without
 * seeds then has -1 everywhere), one without as the first round (iteration 0).
 * ind [P][3][Q], Q = the job's largest n_corner_q + n_surf_q: problem p's ind1 / ind2 / ind3 of its
 * corner queries, then of its surface queries; the device array is first filled with
 * LOAM_DEV_OD_ASSOC_SENTINEL and then holds the seeds, so in an unseeded job an entry no kernel wrote
 * shows (in a seeded one it shows as its seed); entries beyond a problem's queries are the sentinel.
 * mono [P][2], rstart [P][2][66]: the hash build's ring-monotone flags and ring start tables of the
 * corner and the surface Last cloud; counters [P][2]: kIsGathered, kIsBoxes (zero unless count).
 * LOAM_E_HIP also when a kernel raised a problem's error flags (kIsErr).
 * LOAM_E_INVAL, before the handle is touched, for null pointers, sizes, tuning values, grid, count or
 * hash_form out of range, a ring outside 0 .. 63, a query w with a fraction, a seed outside [-1, n). */
int loam_dev_od_assoc_run(loam_dev_od_assoc* h, const loam_dev_od_assoc_job* job, int32_t* ind, int32_t* mono,
                          int32_t* rstart, int32_t* counters);

int loam_dev_od_assoc_destroy(loam_dev_od_assoc* h);

/* Scan registration's ring ID (sr.hip) of n caller points (sensor frame: x, y, z, -) under a ring
 * model (n_rings in [2, 64], ring_model LOAM_RING_*, the linear model's two angles; what loam_create
 * takes from its loam_config): ring [n] from the production ring_of (tangent thresholds, falling
 * back to the exact evaluation), exact [n] from ring_of_exact alone, fast [n] 1 where the thresholds
 * decided.  Rings outside 0 .. n_rings - 1 are those of dropped points.  n in 1 .. LOAM_DEV_SR_RING_MAX.
 * LOAM_E_HIP without a GPU, LOAM_E_INVAL for bad arguments, LOAM_E_NOMEM. */
#define LOAM_DEV_SR_RING_MAX (1 << 22)
int loam_dev_sr_ring_of(int device, int32_t n_rings, int32_t ring_model, float ring_lo_deg, float ring_hi_deg,
                        const float* pts, int32_t n, int32_t* ring, int32_t* exact, int32_t* fast);

/* The same under a ring table (include/loam/loam.h loam_set_ring_table: n_tab intervals,
 * bound_deg [n_tab + 1], ring_tab [n_tab]) in place of the model arguments; ring, exact and fast as
 * above.  LOAM_E_INVAL also for a table loam_ring_table_check refuses. */
int loam_dev_sr_ring_of_table(int device, int32_t n_rings, uint32_t n_tab, const float* bound_deg,
                              const int32_t* ring_tab, const float* pts, int32_t n, int32_t* ring, int32_t* exact,
                              int32_t* fast);

/* loam_lanes_push_device's validation and gather (lanes_feed_plan.hpp, lanes.hip k_lanes_gather_dev) on
 * S caller sweeps in device memory: raw [S] is a loam_cloud_in array (include/loam/loam.h) whose data
 * are device pointers; every lane counts as running.  out_raw [S][cap][4] words: first filled with
 * LOAM_DEV_VG_SENTINEL (every word), then lane s's points at [s][0 .. out_n[s]); out_n [S]: what the
 * kernel wrote into scan registration's sizes (0 for a lane the product would fail: count 0 or beyond
 * cap, null or misaligned data, a bad stride).  S in 1 .. LOAM_LANES_MAX, cap in 1 ..
 * LOAM_DEV_LANES_GATHER_MAX_CAP.  LOAM_E_INVAL for bad arguments and for what the product refuses at
 * call level (a pointer that is not device memory of `device`, a sweep that leaves its allocation),
 * before anything is launched; LOAM_E_HIP without a GPU; LOAM_E_NOMEM. */
#define LOAM_DEV_LANES_GATHER_MAX_CAP (1 << 22)
int loam_dev_lanes_gather(int device, int32_t S, int32_t cap, const void* raw /* loam_cloud_in [S] */, uint32_t* out_raw,
                          int32_t* out_n);

/* What loam_lanes_map_commit reads of one shared lane (include/loam/loam.h): the lane's
 * downsampled CornerStack / SurfStack of its last pulled mapping frame in the map frame, computed by
 * the commit's own transform, in stack order, the points outside the cube grid included
 * (corner_out: 120 n_rings x 4 floats, surf_out: max_points x 4 floats at most; n_out: the two
 * counts), and the frame's valid cubes (valid_out [125], *n_valid).  So that a test can restate a
 * commit of several lanes on the host.  LOAM_E_INVAL where the commit would
 * refuse the lane. */
struct loam_ctx;
int loam_dev_lanes_commit_input(struct loam_ctx* ctx, uint32_t lane, float* corner_out, float* surf_out,
                                uint32_t* n_out /* [2] */, int32_t* valid_out /* [125] */, uint32_t* n_valid);

/* loam_lanes_clouds' two kernels (lanes.hip k_lanes_pack_offsets / k_lanes_pack) on nine
 * caller-made clouds of S lanes: cloud c has strides[c] points of room per lane at src[c] ([S][strides[c]][4]
 * floats, host memory) and counts[c * S + l] points in lane l (any value: the kernel clamps it to [0,
 * strides[c]]); mask [S]: bit c of mask[l] = cloud c of lane l counts; list [n]: the lanes to pack, in
 * order.  table_out [9][n + 1]: the offsets kernel's table.  dst [dst_points][4] floats goes to the device
 * as it is, cloud c's selection is packed behind cloud c - 1's from dst[0] on, and dst comes back: what
 * lies behind the selection is as the caller left it.  LOAM_DEV_LANES_PACK_TILE is the pack kernel's
 * tile in points.  LOAM_E_INVAL for bad arguments (S outside 1 .. LOAM_LANES_MAX, n outside 1 .. S, a
 * stride outside 1 .. LOAM_DEV_LANES_PACK_MAX_STRIDE, an index >= S), LOAM_E_CAPACITY when dst_points is
 * less than the selection (checked on the host, before anything is launched), LOAM_E_HIP without a GPU,
 * LOAM_E_NOMEM. */
#define LOAM_DEV_LANES_PACK_TILE 1024
#define LOAM_DEV_LANES_PACK_MAX_STRIDE (1 << 22)
int loam_dev_lanes_pack(int device, int32_t S, const int32_t* strides /* [9] */, const int32_t* counts /* [9][S] */,
                        const int32_t* mask /* [S] */, const uint32_t* list /* [n] */, int32_t n,
                        const float* const* src /* [9] */, float* dst, uint64_t dst_points, uint64_t* table_out);

#ifdef __cplusplus
}
#endif
#endif
