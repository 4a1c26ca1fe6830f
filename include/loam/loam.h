/* loam.h — C-ABI of the MI355X LOAM scan-matching engine (libloam_hip.so).
 *
 * Drop-in for the compute bodies of the four ROS nodes of the reference
 * (/root/reference = Maofei/loam_velodyne-1).  Each entry point replaces one node callback:
 *
 *   loam_scan_registration  <- laserCloudHandler        src/scanRegistration.cpp:211-636
 *   loam_imu                <- imuHandler               src/scanRegistration.cpp:638-660 and
 *                              laserMapping imuHandler  src/laserMapping.cpp:323-335
 *   loam_odometry           <- laserOdometry loop body  src/laserOdometry.cpp:413-931
 *                              (inputs = what handlers :275-354 store)
 *   loam_mapping            <- laserMapping loop body   src/laserMapping.cpp:411-1097
 *                              (inputs = what handlers :274-321 store)
 *   loam_mapping_surround   <- /laser_cloud_surround    src/laserMapping.cpp:1038-1058
 *   loam_maintenance        <- transformMaintenance     src/transformMaintenance.cpp:147-203
 *   loam_batch_*            <- config 4 of BASELINE.json (independent problems, no reference
 *                              equivalent: one problem = the bodies above composed)
 *
 * Conventions: no C++ types cross the boundary; all host storage is caller-owned and never
 * retained after a call; a context owns its device memory, one HIP device and its HIP streams
 * (the node bodies run on one; a batch step spreads over up to four, loam_batch_sync drains them
 * all); a context is not thread-safe, distinct contexts may run concurrently.  Every function returns
 * LOAM_OK (0) or a negative LOAM_E_* code; loam_last_error() describes the last failure on the
 * calling thread.  LOAM_E_CAPACITY writes the required size back into the cloud's `count`.
 */
#ifndef LOAM_LOAM_H
#define LOAM_LOAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LOAM_OK 0
#define LOAM_E_INVAL (-1)
#define LOAM_E_CAPACITY (-2)
#define LOAM_E_HIP (-3)
#define LOAM_E_NOT_READY (-4) /* scan registration inside systemDelay (Q1) */
#define LOAM_E_NOMEM (-5)

/* published-flag bits of loam_odometry (the topics laserOdometry publishes on this call) */
#define LOAM_PUB_POSE 1   /* /laser_odom_to_init  (src/laserOdometry.cpp:858-873) */
#define LOAM_PUB_CLOUDS 2 /* /laser_cloud_corner_last + /laser_cloud_surf_last (:439-449, :913-923) */
#define LOAM_PUB_FULL 4   /* /velodyne_cloud_3    (:925-929) */

/* ring-ID models for scan registration */
#define LOAM_RING_VLP16 0  /* reference: round(angle) -> r>0 ? r : r+(N-1)  src/scanRegistration.cpp:248-260 */
#define LOAM_RING_LINEAR 1 /* bk HDL-64E hint: int((angle-lo)/step + 0.5f), bk src/scanRegistration.cpp:268-275 */
#define LOAM_RING_TABLE 2  /* a table of elevation intervals (loam_set_ring_table), not a value of loam_config::ring_model */
#define LOAM_RING_TABLE_MAX 64 /* intervals of a ring table */

/* PCL PointXYZI payload in a 16-byte record (PCL's in-memory PointXYZI is 32 B with padding).
 * intensity = ring + 0.1*relTime out of scan registration (src/scanRegistration.cpp:283-284),
 * the integer ring after TransformToEnd (src/laserOdometry.cpp:193). */
typedef struct { float x, y, z, intensity; } loam_point;

/* the reference's float transform[6] layout: (rx, ry, rz, tx, ty, tz) in the camera frame
 * (x left, y up, z forward), e.g. transformSum src/laserOdometry.cpp:94 */
typedef struct { float rx, ry, rz, tx, ty, tz; } loam_pose6;

/* caller-owned input cloud; x, y, z floats at byte offsets 0, 4, 8 of each record
 * (accepts 16-B PointXYZ/loam_point and 32-B PointXYZI / velodyne XYZIR records); stride_bytes a
 * multiple of 4, data at any alignment (e.g. a PointCloud2 message's own buffer, loam_pc2_cloud) */
typedef struct { const void *data; uint32_t count; uint32_t stride_bytes; } loam_cloud_in;

/* caller-owned output storage; count = points written (or required, on LOAM_E_CAPACITY) */
typedef struct { loam_point *pts; uint32_t count; uint32_t capacity; } loam_cloud_out;

/* the six topics scanRegistration publishes (src/scanRegistration.cpp:584-635) */
typedef struct {
  loam_cloud_out full;       /* /velodyne_cloud_2 */
  loam_cloud_out sharp;      /* /laser_cloud_sharp */
  loam_cloud_out less_sharp; /* /laser_cloud_less_sharp */
  loam_cloud_out flat;       /* /laser_cloud_flat */
  loam_cloud_out less_flat;  /* /laser_cloud_less_flat */
  float imu_trans[12];       /* /imu_trans: start RPY, cur RPY, shift, velo (zeros without IMU) */
} loam_features;

typedef struct {
  uint32_t n_rings;        /* N_SCANS (16)                                  scanRegistration.cpp:61 */
  uint32_t ring_model;     /* LOAM_RING_VLP16 | LOAM_RING_LINEAR */
  float ring_lo_deg;       /* LOAM_RING_LINEAR lower bound (-24.8) */
  float ring_hi_deg;       /* LOAM_RING_LINEAR upper bound (2.0) */
  uint32_t system_delay;   /* 20                                            scanRegistration.cpp:57 */
  uint32_t max_points;     /* per-sweep capacity (40000 in the reference)   scanRegistration.cpp:63 */
  uint32_t od_max_iter;    /* 25                                            laserOdometry.cpp:470 */
  uint32_t mp_max_iter;    /* 10                                            laserMapping.cpp:710 */
  uint32_t skip_frame_num; /* 1                                             laserOdometry.cpp:51 */
  uint32_t map_capacity;   /* device map-store capacity in points (per map instance) */
} loam_config;

/* per-call counters; feed the algorithmic-byte formula of SURVEY.md §8(d) */
typedef struct {
  uint64_t n_raw, n_ring;                       /* SR input points, ring-sorted points */
  uint64_t n_sharp, n_less_sharp, n_flat, n_less_flat;
  uint64_t od_iters, od_assoc_rounds, od_rows_sum, od_corner_last, od_surf_last, od_queries;
  uint64_t od_assoc_points;                     /* sum over problems of rounds x (C + S) */
  uint64_t mp_iters, mp_rows_sum, mp_stack, mp_map_points;
  uint64_t mp_map_valid_points;                 /* points of the valid cubes after the last map update (a batch: prev's, its only one) */
  uint64_t mp_stack_iters;                      /* sum over problems of iterations x stack size */
  uint64_t mp_fits;                             /* line / plane fits computed (the rest reused: same ordered 5-NN) */
  uint64_t od_query_iters;                      /* sum over problems of L-M iterations x queries (sharp + flat) */
  uint64_t od_row_evals;                        /* Jacobian rows evaluated: sum of queries x it(it+1)/2 (Q12) */
  uint64_t bytes_sr, bytes_od, bytes_mp;        /* algorithmic bytes, SURVEY.md §8(d) */
  double ms_sr, ms_od, ms_mp;                   /* device time per stage (HIP events) */
  /* reference branches taken (batch: summed over problems) */
  uint64_t od_degenerate_steps; /* odometry L-M updates projected by the iteration-0 degeneracy
                                   analysis (src/laserOdometry.cpp:770-797, Q15) */
  uint64_t od_nan_skips;        /* odometry L-M updates skipped by the NaN guard (:799-811, Q16) */
  uint64_t mp_degenerate_steps; /* mapping L-M updates projected (src/laserMapping.cpp:927-954) */
  uint64_t mp_grid_shifts;      /* cube-grid slab shifts of the recentring (:454-614, Q23) */
  /* memory work the search kernels actually did (the bench's gathered-byte roofline) */
  uint64_t mp_nn_candidates;    /* map points whose distance the 5-NN evaluated (incl. the seeds) */
  uint64_t mp_nn_cells;         /* hash bucket ranges the 5-NN read */
  uint64_t od_assoc_gathered;   /* Last-cloud points the association loaded (cells, fallback, windows) */
  uint64_t od_assoc_boxes;      /* 64-point chunk boxes the association loaded */
} loam_stats;

typedef struct loam_ctx loam_ctx;

void loam_config_default(loam_config *cfg);               /* reference constants (VLP-16) */
int loam_create(loam_ctx **out, const loam_config *cfg, int device);
void loam_destroy(loam_ctx *ctx);
const char *loam_last_error(void);

/* ---- ring tables: a ring model stated as data, for lidars whose beams are not evenly spaced
 * (VLP-32C, Pandar40/64, calibrated elevations) ----
 * A table is n intervals, 1 <= n <= LOAM_RING_TABLE_MAX, given as bound_deg[n + 1] (strictly
 * ascending) and ring[n].  With a = the reference's float vertical angle
 * (atan(y / sqrt(x^2 + z^2)) * 180 / pi in the camera frame, src/scanRegistration.cpp:241-247), a
 * point's ring is ring[i] for the i with bound_deg[i] <= a < bound_deg[i + 1], compared as floats.
 * The point is dropped (the reference's scanID < 0 || scanID > N_SCANS - 1 skip, :262-265) when a is
 * below bound_deg[0], at or above bound_deg[n] or NaN, and when ring[i] == -1.  Ring order should
 * follow elevation: the odometry associates across neighbouring rings (+-2.5).
 *
 * loam_ring_table_check (host only, no context): LOAM_OK, or LOAM_E_INVAL with the rule broken in
 * loam_last_error(): pointers non-null; n_rings in [2, 64]; n in range; every bound finite and
 * inside (-89, 89); bounds strictly ascending; every interval at least 1/32 degree wide; every
 * ring[i] in [-1, n_rings); at least one ring[i] not -1.
 *
 * loam_ring_table_of_model (host only): the table that restates cfg's built-in model (cfg->n_rings,
 * ring_model, ring_lo_deg, ring_hi_deg): the intervals from the first to the last valid ring, each
 * bound the first float at which the new ring holds, so the table gives the model's ring on every
 * float in [bound_deg[0], bound_deg[*n]).  bound_deg holds LOAM_RING_TABLE_MAX + 1 floats, ring
 * LOAM_RING_TABLE_MAX.  LOAM_E_INVAL (nothing written) for a model that needs more than
 * LOAM_RING_TABLE_MAX intervals or whose table the check refuses.
 *
 * loam_set_ring_table: the context's ring model becomes a copy of the table, whatever
 * cfg.ring_model said; n_rings (loam_create) still sizes everything.  Every service of the context
 * then uses it: the node calls, the chain, the batch, the lanes.  Allowed only while the context has
 * seen no sweep: after a successful loam_scan_registration, loam_chain_sweep, loam_batch_upload,
 * loam_batch_feed, loam_lanes_open or loam_lanes_open_shared it returns LOAM_E_INVAL and changes
 * nothing (a sensor does not change during a context's life).  Argument errors are the check's
 * (against the context's n_rings); LOAM_E_NOMEM / LOAM_E_HIP leave the old model intact. */
int loam_ring_table_check(uint32_t n_rings, uint32_t n, const float *bound_deg, const int32_t *ring);
int loam_ring_table_of_model(const loam_config *cfg, uint32_t *n, float *bound_deg, int32_t *ring);
int loam_set_ring_table(loam_ctx *ctx, uint32_t n, const float *bound_deg, const int32_t *ring);

/* ---- ring and time from the sweep's own fields (velodyne PointXYZIRT, Ouster, Hesai) ----
 * A context may read each point's ring, or its ring and its time, from fields of the caller's
 * records instead of reconstructing them from the geometry.  r = the ring, v = the ring field's
 * value read unsigned, t = the time field's value.
 *
 * A point is kept only if x, y, z are finite; v < ring_map_n (v < n_rings without a map);
 * r = ring_map[v] (r = v without a map) is not negative; and, with a time field,
 * tau = (float)((double)t * time_scale + time_bias) is finite with 0 <= tau <= 0.5 (the product and
 * the sum rounded to double, the result to float).  Every other point is dropped as the reference
 * drops a point whose scanID is out of range (src/scanRegistration.cpp:257-260).
 *
 * Ring only (time_type == LOAM_FIELD_NONE): the ring from the field, the time from the azimuth as
 * under a ring model: intensity = (float)(r + 0.1 * relTime).
 * Ring and time: intensity = (float)r + tau (one float addition), and the point's time for the IMU
 * de-skew is intensity - (float)r, which is tau again: the time the odometry reads back out of the
 * point (src/laserOdometry.cpp:103, s = 10 * tau for the reference's 0.1 s scan period).  Azimuth,
 * the sweep's ends and halfPassed are not computed.  A time field without a ring field is not offered.
 *
 * loam_point_fields_check (host only, no context): LOAM_OK, or LOAM_E_INVAL with the rule broken in
 * loam_last_error(): f non-null; ring_type U8 | U16 | U32; time_type NONE | F32 | U32 | F64; each
 * offset at least 12 and a multiple of its field's size; each field ends at or below byte 65536;
 * the fields do not overlap; with a time field time_scale and time_bias finite and time_scale != 0;
 * ring_map == NULL requires ring_map_n == 0; a given map has 1 .. LOAM_RING_MAP_MAX entries, each
 * in [-1, n_rings), at least one of them >= 0.
 *
 * loam_set_point_fields: the context copies the fields and the map; f == NULL returns to the ring
 * model (or table), which is kept but not consulted while fields are set.  Allowed only while the
 * context has seen no sweep, as loam_set_ring_table is, and in either order with it; n_rings still
 * sizes everything.  LOAM_E_NOMEM / LOAM_E_HIP leave the previous state intact.  Every cloud then
 * handed to the context needs stride_bytes at or above the end of both fields (else the call's or
 * the lane's LOAM_E_INVAL, as for a bad stride); host clouds are read at any alignment;
 * loam_lanes_push_device keeps its alignment rules, and its range check covers each field's end. */
#define LOAM_FIELD_NONE 0
#define LOAM_FIELD_U8   1
#define LOAM_FIELD_U16  2
#define LOAM_FIELD_U32  3
#define LOAM_FIELD_F32  4
#define LOAM_FIELD_F64  5
#define LOAM_RING_MAP_MAX 256

typedef struct {
  uint32_t ring_type, ring_offset;    /* U8 | U16 | U32; byte offset inside a record */
  uint32_t time_type, time_offset;    /* NONE | F32 | U32 | F64 */
  double   time_scale, time_bias;     /* tau = (float)((double)t * time_scale + time_bias), seconds after the sweep's stamp */
  const int32_t *ring_map;            /* NULL = identity; else ring_map[v] = ring of field value v, or -1 = drop */
  uint32_t ring_map_n;                /* entries, <= LOAM_RING_MAP_MAX */
} loam_point_fields;

int loam_point_fields_check(uint32_t n_rings, const loam_point_fields *f);
int loam_set_point_fields(loam_ctx *ctx, const loam_point_fields *f);

/* = the /imu/data handlers of scanRegistration (src/scanRegistration.cpp:638-660: queue entry, gravity
 * removal, AccumulateIMUShift) and laserMapping (src/laserMapping.cpp:323-335).  quat_xyzw = the
 * sensor_msgs/Imu orientation (x, y, z, w), lin_acc_xyz = linear_acceleration, both float64 as in the
 * message.  Stamps must be non-decreasing (LOAM_E_INVAL otherwise).  With IMU data, scan registration
 * de-skews each point with it (:286-349) and fills imu_trans; odometry and mapping use it through
 * imu_trans and the mapping queue (src/laserOdometry.cpp:330-351, src/laserMapping.cpp:199-226). */
int loam_imu(loam_ctx *ctx, double stamp, const double quat_xyzw[4], const double lin_acc_xyz[3]);

/* = laserCloudHandler.  Returns LOAM_E_NOT_READY for the first system_delay sweeps (Q1). */
int loam_scan_registration(loam_ctx *ctx, double stamp, loam_cloud_in raw, loam_features *out);

/* = laserOdometry loop body for one synchronised set of the six scanRegistration topics.
 * sum_out receives transformSum when LOAM_PUB_POSE is set; the three clouds are written when
 * their flag is set in *published. */
int loam_odometry(loam_ctx *ctx, double stamp, const loam_features *in, loam_pose6 *sum_out,
                  loam_cloud_out *corner_last, loam_cloud_out *surf_last, loam_cloud_out *full_end,
                  int *published);

/* = laserMapping loop body for one synchronised (corner_last, surf_last, full, odometry) set.
 * odom_sum goes through the reference's nav_msgs quaternion round trip.  aft / bef are
 * transformAftMapped / transformBefMapped (the Bef pose the reference smuggles in the twist
 * fields, src/laserMapping.cpp:1082-1087); registered = full cloud in the map frame. */
int loam_mapping(loam_ctx *ctx, double stamp, const loam_pose6 *odom_sum,
                 const loam_cloud_out *corner_last, const loam_cloud_out *surf_last,
                 const loam_cloud_out *full_end, loam_pose6 *aft, loam_pose6 *bef,
                 loam_cloud_out *registered);

/* = the /laser_cloud_surround publish of the laserMapping loop body (src/laserMapping.cpp:1038-1058,
 * mapFrameNum = 5, :52, :405): the map store's 5x5x5 cube neighbourhood of the last mapping frame
 * (laserCloudSurroundInd, :617-670), corner then surf points per cube, VoxelGrid 0.2.  The
 * reference publishes it on the 1st successful loam_mapping frame and every 5th after it: on
 * those frames *published = 1 and out is filled; otherwise *published = 0 and out->count = 0.
 * Call between a loam_mapping and the next (the cloud is computed on demand from the store that
 * frame left; a LOAM_E_CAPACITY call may be repeated with more capacity). */
int loam_mapping_surround(loam_ctx *ctx, loam_cloud_out *out, int *published);

/* ---- device-resident node chain (no reference equivalent: the reference's nodes exchange ROS
 * messages; this is the intra-process / nodelet deployment of the same three bodies) ----
 * One sweep through loam_scan_registration -> loam_odometry -> loam_mapping (on the frames odometry
 * publishes all three clouds, as the node graph does) on one context, the intermediate topics left
 * in device memory: odometry reads scan registration's output buffers in place, mapping reads
 * odometry's published CornerLast / SurfLast / full-end buffers in place.  Same kernels, same values
 * as the three message calls; loam_mapping_surround works after it as after loam_mapping.
 * Returns LOAM_E_NOT_READY inside system_delay.  registered: capacity 0 = not downloaded.
 * (Tuning stream_defer, default on, for this call: the bookkeeping only the next sweep reads —
 * mapping's map update, odometry's hash tables of the new Last clouds — runs on the context's second
 * stream after the call has its results; the next call waits for it on the device.  A map-update
 * capacity error is then reported by the next call.) */
typedef struct {
  int32_t published;          /* loam_odometry's LOAM_PUB_* flags for this sweep */
  int32_t mapped;             /* 1 when laserMapping ran on this sweep */
  loam_pose6 od_sum;          /* /laser_odom_to_init (transformSum), when LOAM_PUB_POSE */
  loam_pose6 aft, bef;        /* transformAftMapped / transformBefMapped, when mapped */
  loam_cloud_out registered;  /* /velodyne_cloud_registered, when mapped and capacity > 0 */
} loam_chain_out;
int loam_chain_sweep(loam_ctx *ctx, double stamp, loam_cloud_in raw, loam_chain_out *out);

/* = transformMaintenance laserOdometryHandler with the last odomAftMappedHandler state.
 * Pure host function (scalar pose algebra, no kernel). */
int loam_maintenance(const loam_pose6 *odom_sum, const loam_pose6 *bef, const loam_pose6 *aft,
                     loam_pose6 *integrated);

/* ---- batched independent problems (config 4) ----
 * problem i = scan registration of (prev_i, cur_i), odometry seeded from prev_i and solved on
 * cur_i, mapping of prev_i into an empty map then solved for cur_i.
 * upload copies the host sweeps into device memory; run executes every problem on the device
 * with all inputs resident in HBM; download copies the poses back.  run only enqueues: for
 * n >= 64 (tunings step_pipe / sr_ahead) consecutive runs overlap as a software pipeline — a run's
 * odometry beside the previous run's mapping, the next run's scan registration and odometry seed
 * enqueued ahead (they re-run the same uploaded problems, unless loam_batch_feed supplies each run's
 * sweeps) — and sync waits for all of it.  download returns the last run's results.
 * A problem ends at cur's solved pose: the map with cur inserted and the registered clouds
 * (/velodyne_cloud_registered) are not built, since no batch call returns them.  So in a batch's
 * stats mp_map_valid_points is the figure of prev's map update (the only one that runs), and the
 * map-store overflow that only inserting cur could raise (LOAM_E_CAPACITY from download) is not
 * raised; an overflow while mapping prev, or of a stack, still is. */
int loam_batch_upload(loam_ctx *ctx, uint32_t n, const loam_cloud_in *prev,
                      const loam_cloud_in *cur);
int loam_batch_run(loam_ctx *ctx);
/* the sweeps of the NEXT loam_batch_run: n independent problems of the uploaded batch size (a new
 * batch arriving over time).  In the step pipeline (n >= tuning step_pipe) the sweeps are copied from
 * pinned staging into the scan-registration set that step reads, on the pipeline's own stream behind
 * that set's previous reader, and that step's scan registration + odometry seed are enqueued there
 * at once, so fresh batches overlap the running steps; a fed context no longer re-runs the resident
 * sweeps ahead (a run without a feed re-runs that set's last sweeps).  Otherwise (sequential steps)
 * the same as loam_batch_upload.  The call packs the sweeps on the calling thread and returns once
 * the copies are enqueued; the caller's buffers are free on return. */
int loam_batch_feed(loam_ctx *ctx, uint32_t n, const loam_cloud_in *prev, const loam_cloud_in *cur);
int loam_batch_sync(loam_ctx *ctx);   /* waits for the work enqueued by loam_batch_run */
int loam_batch_download(loam_ctx *ctx, loam_pose6 *od_sum, loam_pose6 *aft, loam_stats *stats);
/* per-problem L-M results of the last run behind loam_batch_download's poses, for parity checks
 * (any pointer may be NULL): the odometry and mapping iteration counts (the convergence decisions)
 * and the odometry's solved increment transform[6] (src/laserOdometry.cpp:93, :811; the pose the
 * accumulation and TransformToEnd use) */
int loam_batch_lm_info(loam_ctx *ctx, int32_t *od_iters, int32_t *mp_iters, loam_pose6 *od_transform);

/* ---- the scan-registration clouds of a batch ----
 * One of the five scanRegistration clouds of every selected sweep, packed back to back in
 * caller-owned storage.  Problems [first, first + n) select 2n sweeps in the order
 * sweep j = 2*(i - first) + (0: prev_i, 1: cur_i); sweep j's points are pts[offset[j] .. offset[j+1])
 * and offset[2n] = count.  Points are the records loam_scan_registration writes: ring-major,
 * intensity = ring + 0.1*relTime. */
typedef struct {
  loam_point *pts;      /* caller-owned, NULL = the points are not wanted (count / offsets still filled) */
  uint64_t capacity;    /* points pts holds */
  uint64_t count;       /* points of the selection (written, or required on LOAM_E_CAPACITY) */
  uint32_t *offset;     /* caller-owned [2*n + 1], NULL = not wanted */
} loam_batch_cloud;
typedef struct { loam_batch_cloud full, sharp, less_sharp, flat, less_flat; } loam_batch_clouds;

/* The clouds of the run whose poses loam_batch_download reports (the last loam_batch_run), after
 * waiting for the context's queued work as loam_batch_download does.  A cloud whose pts and offset
 * are both NULL is not wanted and its struct is left untouched; for every other cloud count and
 * (when given) offset are always filled, the points when pts is given.  Passing every pts as NULL
 * is the sizes-only query.  The pipeline is left as found: a following loam_batch_run behaves as
 * if this call had not happened.  The points are packed on the device and transferred through a
 * fixed-size staging (allocated by the first call, released by loam_destroy), chunk by chunk.
 * Errors: LOAM_E_INVAL for a null argument, no uploaded batch, no loam_batch_run since the last
 * loam_batch_upload (or since a loam_set_tuning / loam_set_stream_priority, which restart the
 * pipeline), n == 0, first + n beyond the batch, a wanted cloud of the range exceeding
 * 2^32 - 1 points (ask for a smaller range), or a max_points too large for the staging; a sweep's
 * scan-registration error as loam_batch_download reports it; LOAM_E_CAPACITY when a wanted
 * cloud's points do not fit its capacity: no points are written, every wanted count / offset is
 * filled, and the call may be repeated with more room. */
int loam_batch_features(loam_ctx *ctx, uint32_t first, uint32_t n, loam_batch_clouds *out);

/* ---- the map: save it, load it (no reference equivalent: the reference never hands its map over) ----
 * The streaming context's cube map, laserCloudCornerArray / laserCloudSurfArray
 * (src/laserMapping.cpp:64-70, :96-99, :980-1036): 21 x 11 x 21 cubes of 50 m.  Each cloud is in
 * canonical order: cubes in ascending cube index (i + 21*j + 231*k, the reference's cubeInd),
 * inside a cube the store's own point order (FLANN ties by index and PCL's VoxelGrid sums in input
 * order, so that order is part of the map).  Points are in the map frame.  Batch maps have no
 * export. */
#define LOAM_MAP_CUBES 4851 /* 21 * 11 * 21 */

typedef struct {
  loam_point *pts;        /* caller-owned; export: NULL = the points are not wanted; import: the points */
  uint64_t capacity;      /* export: points pts holds; import: ignored */
  uint64_t count;         /* export: points of the cloud (written, or required on LOAM_E_CAPACITY); import: points given */
  uint32_t *cube_offset;  /* export: caller-owned [LOAM_MAP_CUBES + 1] or NULL: cube c = pts[cube_offset[c] .. cube_offset[c+1]); import: ignored */
} loam_map_cloud;

typedef struct {
  loam_map_cloud corner;   /* laserCloudCornerArray */
  loam_map_cloud surf;     /* laserCloudSurfArray */
  int32_t center[3];       /* laserCloudCenWidth / CenHeight / CenDepth (10, 5, 10 at start) */
  int32_t surround_phase;  /* mapFrameCount, 0..4 (4 = the next mapping frame publishes surround) */
  loam_pose6 aft;          /* transformAftMapped */
  loam_pose6 bef;          /* transformBefMapped */
} loam_map;

/* Writes the context's streaming map and mapping pose state, after waiting for the context's
 * queued work (a loam_chain_sweep's deferred map update included).  For each cloud count and (when
 * given) cube_offset are always filled, the points when pts is given; every pts NULL is the
 * sizes-only query.  LOAM_E_CAPACITY (a cloud's points do not fit its capacity) writes no point
 * and fills every count and offset, so the call can be repeated with more room.  The call changes
 * nothing: a mapping frame after it behaves as if it had not happened.  The points are packed on
 * the device and transferred through loam_batch_features' fixed-size staging, chunk by chunk.
 * LOAM_E_INVAL for a null argument, or when the last map update overflowed map_capacity. */
int loam_map_export(loam_ctx *ctx, loam_map *out);

/* Replaces the context's streaming map and mapping pose state: center, bef, aft and
 * surround_phase are set, a pending surround publication is dropped; odometry, scan registration
 * and the IMU queues are left alone.  The points need not be sorted: each goes to the cube the
 * reference's insertion would choose for it with the given center (:983-989) and keeps its input
 * order inside that cube.  Points outside the grid or with a non-finite coordinate are left out
 * and counted per cloud in dropped[0] (corner) / dropped[1] (surf) when dropped is given.  Nothing
 * is downsampled here: as in the reference, a cube is downsampled when it next falls into a
 * frame's valid set (:1018-1036).  An import of two empty clouds is a map reset that keeps the
 * given poses.  The two intended uses:
 *   resume    import exactly what loam_map_export gave; the stream continues bit for bit;
 *   localize  in a prior map with a fresh odometry: bef = zeros, aft = the initial pose guess
 *             (the first mapping frame then applies the whole odometry pose on top of aft).
 * Errors: LOAM_E_INVAL for a null argument (a cloud with count > 0 and pts NULL included),
 * surround_phase outside 0..4, a |center| component above 2^24, or more than 2^31 - 2^23 points in
 * all; LOAM_E_CAPACITY when the kept points exceed map_capacity (dropped is filled).  In every
 * error case the old map and poses are left exactly as they were. */
int loam_map_import(loam_ctx *ctx, const loam_map *in, uint64_t dropped[2]);

/* ---- multi-hypothesis localization in the map (no reference equivalent) ----
 * One sweep's feature clouds and n candidate poses: laserMapping's sweep-to-map refinement
 * (src/laserMapping.cpp:411-974 without the map update) for every candidate at once against the
 * context's streaming map, which is only read. */
#define LOAM_LOC_SOLVED  0  /* the L-M ran; aft is the refined pose */
#define LOAM_LOC_NO_LM   1  /* <= 10 corner or <= 100 surf map points in the candidate's valid cubes
                               (src/laserMapping.cpp:706): no L-M, aft = the candidate's aft as given */
#define LOAM_LOC_OFFGRID 2  /* a mapping frame at this guess would recentre the cube grid (:454-614);
                               not evaluated, aft = the candidate's aft as given, the counts are 0 */
#define LOAM_LOCALIZE_MAX 1024

typedef struct {
  loam_pose6 aft;            /* transformAftMapped a mapping frame would leave */
  int32_t status;            /* LOAM_LOC_* */
  int32_t iters;             /* L-M iterations run */
  int32_t degenerate_steps;  /* updates projected by the iteration-0 degeneracy analysis */
  uint32_t rows_last;        /* rows (accepted correspondences) of the last iteration evaluated */
  uint32_t rows_sum;         /* rows summed over the iterations (loam_stats.mp_rows_sum) */
  uint32_t stack_corner, stack_surf;  /* the sweep's stacks after their VoxelGrid (0.2 / 0.4) */
  uint32_t map_corner, map_surf;      /* FromMap points of the candidate's valid cubes */
} loam_localize_result;

/* out[h], h < n, is what one loam_mapping(ctx', stamp, odom_sum, corner_last, surf_last, ...) would
 * return in aft and report in its statistics, where ctx' holds this context's map and grid centre
 * as they are now, transformBefMapped = bef[h] (zeros when bef is NULL), transformAftMapped =
 * aft[h], and has received no IMU message: odom_sum through the nav_msgs quaternion round trip,
 * transformAssociateToMap, the candidate's centre cube and FOV-tested 5x5x5 valid set, FromMap in
 * the reference's order, the stacks' round trip and VoxelGrid, up to mp_max_iter L-M iterations,
 * transformUpdate without IMU.  Without an L-M (LOAM_LOC_NO_LM) that frame leaves
 * transformAftMapped alone, so aft = aft[h].  A candidate whose centre cube is within 3 of a grid
 * edge (the frame would first recentre the grid, which this call never does) is LOAM_LOC_OFFGRID:
 * import the map with another centre to evaluate it.  No residual score is returned; rank by
 * status, rows_last / (stack_corner + stack_surf) and iters < mp_max_iter.
 * The call waits for the context's queued work (a deferred map update included) and changes
 * nothing in the context: the map, the grid centre, Bef / Aft, the surround phase and a pending
 * surround publication, odometry, scan registration, the IMU queues and the last frame's statistics
 * stay as they were, and every later call behaves as if this one had not happened.  Its working
 * set (sized by n, the sweep's counts and the largest FromMap) is allocated on demand and kept until
 * loam_destroy.
 * Errors: LOAM_E_INVAL for a null argument (bef may be NULL), n == 0 or n > LOAM_LOCALIZE_MAX, a
 * cloud with count > 0 and pts NULL, a cloud larger than max_points (corner_last: than the mapping
 * stack's 120 points per ring), or a map whose last update overflowed map_capacity; LOAM_E_NOMEM
 * when the working set cannot be allocated; LOAM_E_HIP for a failed HIP call.  In every error
 * case out is untouched and the context is as it was. */
int loam_map_localize(loam_ctx *ctx, const loam_pose6 *odom_sum,
                      const loam_cloud_out *corner_last, const loam_cloud_out *surf_last,
                      uint32_t n, const loam_pose6 *aft, const loam_pose6 *bef,
                      loam_localize_result *out);

/* ---- scoring pose guesses against the map (no reference equivalent) ----
 * loam_map_localize's missing score (score its refined aft) and its pre-filter (score a grid of
 * tens of thousands of guesses, refine the best few hundred): no L-M, no per-candidate working set. */
#define LOAM_SCORE_MAX 65536

typedef struct {
  uint32_t corner_scored, surf_scored; /* points of each cloud with three finite coordinates (same for every candidate) */
  uint32_t corner_in, surf_in;         /* of them: nearest map point of the same kind at d2 < max_dist^2 */
  double corner_cost, surf_cost;       /* sum over the scored points of (inlier ? d2 : max_dist^2) */
} loam_score_result;                   /* 32 bytes */

/* out[h], h < n: every scored point p of the two clouds is put into the map frame by
 * pointAssociateToMap (src/laserMapping.cpp:234-252) with transformTobeMapped = pose[h]; d2 is the
 * smallest float squared distance (dx*dx + dy*dy + dz*dz, no contraction) to any point of the same
 * kind in the context's streaming map: the whole map, not a candidate's valid cubes, so the grid
 * centre plays no part.  With r2 = max_dist * max_dist (float) the point is an inlier iff d2 < r2
 * (false for a NaN and for an empty map) and contributes d2, else r2, to its cloud's cost, a
 * double sum of these float terms.  A transformed coordinate that is non-finite or beyond 2^24 has
 * no neighbour.  Nothing is downsampled.  pose[h] is a map pose of the sweep (what aft is after a
 * mapping frame): loam_map_localize's returned aft, or a grid of guesses, with the sweep's
 * corner_last / surf_last.  Rank by corner_in + surf_in (more is better), then by corner_cost +
 * surf_cost (less is better).
 * out[h] depends on the map, the clouds, max_dist and pose[h] only: bit for bit the same whatever
 * n is, wherever h sits in the call, and from run to run (partial sums are combined in a fixed
 * order given by the clouds' sizes; no floating-point atomics).
 * The call waits for the context's queued work (a deferred map update included) and changes
 * nothing in the context.  The map's index (a 1 m cell hash of every map point: 16 bytes per point
 * and 16 per bucket) is rebuilt by every call and shared by all candidates; the working set is allocated on
 * demand and kept until loam_destroy.  An empty map is no error: every count is 0 and every cost
 * is scored * r2.
 * Errors: LOAM_E_INVAL for a null argument, n == 0 or n > LOAM_SCORE_MAX, max_dist not in (0, 1]
 * (the index has 1 m cells: the 27 cells around a point hold every neighbour closer than 1 m), a
 * cloud with count > 0 and pts NULL, a cloud larger than max_points, or a map whose last update
 * overflowed map_capacity; LOAM_E_NOMEM when the working set cannot be allocated; LOAM_E_HIP for
 * a failed HIP call.  In every error case out is untouched and the context is as it was. */
int loam_map_score(loam_ctx *ctx, const loam_cloud_out *corner, const loam_cloud_out *surf,
                   float max_dist, uint32_t n, const loam_pose6 *pose, loam_score_result *out);

/* ---- lanes: many independent sequences in lockstep (no reference equivalent) ----
 * n_lanes sequences in one context, each advanced by one sweep per step.  Lane l behaves exactly as
 * a fresh context that receives lane l's IMU messages through loam_imu (loam_lanes_imu) and lane l's
 * sweeps through loam_chain_sweep at lane l's stamps, in the same interleaving: the same poses,
 * registered clouds, map and /imu_trans, bit for bit, whatever the other lanes do and whether or
 * not they have an IMU.  A step runs the
 * batch's kernels on all lanes at once (one launch sequence per step, not per sequence) and keeps
 * what the streaming path keeps from sweep to sweep: the Last clouds, transformSum, the cube maps,
 * Bef / Aft.  system_delay, the odometry's init frame and skip_frame_num advance identically in every
 * lane, so published and mapped are the same for every live lane of a step that was never restarted.
 * A restarted lane (loam_lanes_restart) reports LOAM_E_NOT_READY on its wait steps and published =
 * LOAM_PUB_CLOUDS, mapped = 0 on its own init step, whatever the others report; its mapped can be 0
 * where theirs is 1 only on those steps, and is never 1 where theirs is 0.
 * The lanes never take the two launch forms loam_set_tuning's od_persist / mp_persist and
 * od_moments_min select, at any n_lanes (1 included), and no tuning turns them on:
 *   - the per-query moments are not bit-identical to the other forms, and a sequence compounds a
 *     difference that was validated for one two-sweep problem only;
 *   - the persistent L-M kernels' workgroups wait on each other, and more than two of them running
 *     at once on one GPU can hang: a lanes step is safe beside any other context's work.
 * The streaming nodes, the batch and the context's own IMU queues (loam_imu) are separate state and untouched;
 * their entry points may be called whenever no lanes step is in flight. */
#define LOAM_LANES_MAX 1024

typedef struct {
  int32_t status;     /* LOAM_OK, LOAM_E_NOT_READY inside system_delay and on a restarted lane's wait steps, or the lane's sticky failure */
  int32_t published;  /* loam_odometry's LOAM_PUB_* flags of this lane's frame */
  int32_t mapped;     /* 1 when laserMapping ran on this sweep */
  int32_t od_iters, mp_iters;   /* L-M iterations of this frame's odometry / mapping (0 when none ran) */
  loam_pose6 od_sum;  /* transformSum, when LOAM_PUB_POSE */
  loam_pose6 aft, bef;/* transformAftMapped / transformBefMapped, when mapped */
  uint32_t n_registered; /* points of /velodyne_cloud_registered of this frame, when mapped */
} loam_lane_out;

/* Allocates the lanes' working set (scan registration for n_lanes sweeps, odometry and mapping for
 * n_lanes problems, lane_map_capacity points of map store per lane, pinned staging for one step's
 * sweeps; DESIGN.md §21 has the bytes per lane).  Every lane starts as a fresh context: empty map,
 * centre (10, 5, 10), zero poses, odometry not initialised, system_delay not yet consumed.
 * LOAM_E_INVAL: null context, lanes already open (close first), n_lanes == 0 or > LOAM_LANES_MAX,
 * lane_map_capacity outside loam_create's [1024, 2^28], or n_lanes x lane_map_capacity or n_lanes x
 * (max_points + 120 n_rings) reaching 2^31 (the message names the product).  LOAM_E_NOMEM when an
 * allocation fails: everything is freed and the context is as it was.  loam_destroy closes. */
int loam_lanes_open(loam_ctx *ctx, uint32_t n_lanes, uint32_t lane_map_capacity);
/* One step: raw[l] is lane l's next sweep.  Packs the sweeps on the calling thread, enqueues the
 * whole step and returns; the caller's buffers are free on return.  One step may be in flight: a
 * second push before a pull is LOAM_E_INVAL.  Returns LOAM_OK when the step was enqueued, whatever
 * the individual lanes will report.
 * A lane fails when its sweep fails scan registration as the node call would (count == 0 or no
 * finite point: LOAM_E_INVAL; more than max_points: LOAM_E_CAPACITY; null data or a bad stride:
 * LOAM_E_INVAL) or when its map store or stack overflows (LOAM_E_CAPACITY).  The failure is sticky:
 * the lane reports that code in status on this step and every later one, its other fields are not
 * meaningful and its map cannot be exported; no other lane is affected, bit for bit.  Feeding
 * count = 0 is therefore how a lane that has run out of sweeps is retired.  Inside system_delay the
 * sweeps are not looked at, as in the node. */
int loam_lanes_push(loam_ctx *ctx, double stamp, const loam_cloud_in *raw /* [n_lanes] */);
/* loam_lanes_push with one sweep stamp per lane (recorded sequences do not share a clock);
 * loam_lanes_push is the case of equal stamps.  The stamps matter only to lanes with IMU messages:
 * the de-skew and mapping's roll / pitch blend look the queues up by them.  A null stamp array or
 * a stamp that is not finite (either call): LOAM_E_INVAL, nothing is enqueued or counted. */
int loam_lanes_push_stamped(loam_ctx *ctx, const double *stamp /* [n_lanes] */, const loam_cloud_in *raw /* [n_lanes] */);
/* loam_lanes_push_stamped for sweeps that are already in device memory: raw[l].data
 * is a device pointer, and one kernel gathers every lane's sweep straight into scan registration's
 * input.  No host packing, no pinned staging and no bulk copy takes place; the call never
 * synchronises with the host.  It enqueues the step loam_lanes_push_stamped(ctx, stamp, raw_host)
 * enqueues for raw_host[l] holding the same bytes in host memory: every later output (the pull
 * records, registered clouds, /imu_trans, exported maps, surround clouds, score and localize rows)
 * is bit for bit that of the host push, and the two kinds of push may alternate from step to step.
 * raw[l].data is plain device memory of the context's device (hipMalloc; a framework's tensor), x, y,
 * z floats at byte offsets 0, 4, 8 of each record, stride_bytes at least 12 and a multiple of 4, and
 * data 4-byte aligned (the one rule the host form does not have: the device reads dwords).
 * A lane fails, sticky, with the host push's codes: count == 0 (how a lane retires), null data, a
 * bad stride or data % 4 != 0: LOAM_E_INVAL; count > max_points: LOAM_E_CAPACITY; a sweep without a
 * finite point is found by scan registration.  Of a failed lane, a waiting lane (loam_lanes_restart)
 * and every lane inside system_delay raw[l] is not looked at: not the pointer, its memory or its range.
 * LOAM_E_INVAL with nothing enqueued, nothing counted and no lane changed: a null ctx, stamp or raw;
 * lanes not open; a step in flight; a stamp that is not finite; unknown flag bits; a live lane's
 * non-null, aligned pointer that HIP does not report as device memory of the context's device
 * (pinned or registered host memory, managed memory and another device's memory are refused); a live
 * lane's range [data, data + (count - 1) stride_bytes + 12) that leaves its allocation (+ 16 at a
 * 16-byte stride, whose fourth word is copied as the host form copies it).
 * LOAM_E_NOMEM, and nothing changed, when the first call's descriptor block (32 bytes per lane)
 * cannot be allocated.
 * Ordering against the producer of the sweeps, by flags:
 *   0: the sweeps are visible to the device already (the caller synchronised) and stay untouched
 *      until loam_lanes_pull of this step returns; producer_stream is not read.
 *   LOAM_FEED_WAIT: the gather waits for the work enqueued so far on producer_stream (an event
 *      recorded there, waited for on the context's stream).
 *   LOAM_FEED_RELEASE: work enqueued on producer_stream after this call waits for the gather (an
 *      event recorded behind it, waited for on producer_stream) and may overwrite the sweeps.
 * The two events are created, timing disabled, by the first call that needs them and live until
 * loam_lanes_close; none is recorded on a step that reads no sweep (inside system_delay, or every
 * lane failed, waiting or retiring). */
#define LOAM_FEED_WAIT    1
#define LOAM_FEED_RELEASE 2
int loam_lanes_push_device(loam_ctx *ctx, const double *stamp /* [n_lanes] */,
                           const loam_cloud_in *raw /* [n_lanes], data = device pointers */,
                           void *producer_stream /* a hipStream_t, read only when flags != 0 */,
                           uint32_t flags);
/* loam_imu for one lane: the message enters the lane's scanRegistration and laserMapping queues
 * (on the host; the next push uploads the new entries).  A lane that never got a message runs
 * without IMU; a lane may get its first message before any step.  From the first message of any
 * lane on, a step in which some live lane has a message de-skews with the tile-parallel IMU form of
 * the ring sort and runs k_lanes_imu; nothing of this is allocated or launched before.
 * LOAM_E_INVAL: a null argument, lanes not open, lane >= n_lanes, a failed lane, a stamp below the
 * lane's last one (the other lanes are unaffected), or a step in flight.  LOAM_E_NOMEM when the
 * first message's allocation fails.  As with loam_imu, more than 200 messages between a lane's
 * consumed pointer and its last message lap the queue and are outside the contract. */
int loam_lanes_imu(loam_ctx *ctx, uint32_t lane, double stamp, const double quat_xyzw[4], const double lin_acc_xyz[3]);
/* /imu_trans of every lane from the last pulled step, 12 floats per lane in loam_features.imu_trans
 * order; zeros for a lane without IMU messages, a failed lane and a step inside system_delay.
 * LOAM_E_INVAL while a step is in flight and before the first pull. */
int loam_lanes_imu_trans(loam_ctx *ctx, float *out /* [n_lanes][12] */);
/* Waits for the pushed step (its only synchronisation) and fills out[l] for every lane.  LOAM_OK
 * when the step ran, whatever the lanes report; LOAM_E_INVAL with nothing pushed. */
int loam_lanes_pull(loam_ctx *ctx, loam_lane_out *out /* [n_lanes] */);
/* /velodyne_cloud_registered of one lane from the last pulled step: valid while that step's mapped
 * is set and until the next push (LOAM_E_INVAL otherwise, for a failed lane and for lane >=
 * n_lanes).  LOAM_E_CAPACITY writes the required size into out->count. */
int loam_lanes_registered(loam_ctx *ctx, uint32_t lane, loam_cloud_out *out);
/* loam_map_export for one lane's map: canonical cube order, centre, Aft / Bef; surround_phase is
 * the lane's own mapping frame counter (4 at open and at a restart, advanced on each of the lane's
 * mapping frames; the same in every lane that was never restarted).  LOAM_E_INVAL while a step is in flight, for a failed
 * lane and for lane >= n_lanes. */
int loam_lanes_map_export(loam_ctx *ctx, uint32_t lane, loam_map *out);
/* Lane `lane` becomes a fresh sequence: empty map, centre (10, 5, 10), zero transformSum / Bef / Aft,
 * odometry not initialised, empty IMU queues (host and device; loam_lanes_imu accepts any first
 * stamp again), surround_phase 4, sticky failure cleared.  From its first consumed sweep on, the
 * lane behaves exactly as a fresh context created with system_delay = 0 that receives the lane's
 * IMU messages (those sent after this call) through loam_imu and its sweeps through
 * loam_chain_sweep: bit for bit, whatever the other lanes do.  No other lane changes by a bit.
 * A live lane may be restarted (a parameter sweep over one recording), and so may a failed or a
 * retired one; a second restart before the lane's init step only recomputes the wait.
 * Phase rule: the lanes keep one launch sequence per step, so mapping runs on the same steps for
 * every lane.  The lane's init frame (Last = the raw lessSharp / lessFlat clouds, no L-M, published
 * = LOAM_PUB_CLOUDS) is taken on the step before a mapping step of the shared phase, as a fresh
 * context maps on the frame after its init frame.  With s = skip_frame_num and c = the shared
 * odometry frame counter (s at the shared init frame, 0 after a mapping step, + 1 per other step)
 *     *wait_steps = (2 s - c) mod (s + 1),   in 0..s:
 * the number of coming steps on which raw[lane] is not looked at and the lane reports status =
 * LOAM_E_NOT_READY and zero /imu_trans.  The caller offers the sequence's first sweep on the step
 * after them; that step is the lane's init step (mapped = 0 even where the other lanes map).
 * Called inside system_delay or before the shared init frame, the lane is cleared and takes the
 * shared init frame with the others; *wait_steps is then the number of steps until that frame.
 * A restarted lane consumes no system_delay of its own: the caller drops the sweeps its node would
 * not have looked at (the node never looks at them either).
 * The clear is one kernel launch for all lanes restarted between two steps, in front of the next
 * step; the first call allocates two lane lists (n_lanes ints each, pinned and device).
 * LOAM_E_INVAL, and nothing is changed: null context or wait_steps, lanes not open, lane >=
 * n_lanes, a step in flight.  LOAM_E_NOMEM when the first call's allocation fails. */
int loam_lanes_restart(loam_ctx *ctx, uint32_t lane, uint32_t *wait_steps);
/* One map into n lanes of the open lanes, between two steps: loam_map_import for lanes.  lane[i],
 * i < n, are distinct lane indices.  Every listed lane's cube map, grid centre, Bef / Aft and
 * surround_phase are replaced as loam_map_import replaces a context's: centre = in->center, Bef =
 * in->bef, surround_phase = in->surround_phase, Aft = aft[i] (in->aft for every lane when aft is
 * NULL); points in any order, each to the cube the reference's insertion would choose, input order
 * kept inside a cube, nothing downsampled, two empty clouds = a map reset that keeps the poses.
 * dropped as in loam_map_import (the same for every lane: one map, one centre).
 * A listed lane behaves from here on, bit for bit, as a context would that received
 * loam_map_import(in with aft = aft[i]) at the same point of its call sequence; its odometry, scan
 * registration, IMU queues and sticky state are not touched, and no unlisted lane changes by a bit.
 * The map is uploaded and sorted once and copied on the device into every listed lane.
 * May be called whenever lanes are open and no step is in flight (before the first push and inside
 * system_delay too), except for a lane between loam_lanes_restart and the pull of its init step:
 * import after the lane's init step (that frame neither reads nor writes the map, and the restart
 * clears the lane's store up to and including that step).  A restart clears an imported map.
 * LOAM_E_INVAL, and nothing changes in any lane and dropped is not written: a null ctx / lane / in,
 * lanes not open, a step in flight, n == 0 or n > n_lanes, a lane index >= n_lanes, a lane listed
 * twice, a failed lane (restart it first), a lane waiting for its init step, and loam_map_import's
 * own argument errors.  LOAM_E_CAPACITY, and nothing changes in any lane: the kept points exceed
 * lane_map_capacity (dropped is filled).  LOAM_E_NOMEM when the first call's allocation (two blocks
 * of 9 + 7 n_lanes words) fails. */
int loam_lanes_map_import(loam_ctx *ctx, uint32_t n, const uint32_t *lane /* [n] */,
                          const loam_map *in, const loam_pose6 *aft /* [n] or NULL */,
                          uint64_t dropped[2]);
/* /laser_cloud_surround of every lane whose last pulled frame publishes it, in one call. */
typedef struct {
  loam_point *pts;      /* caller-owned; NULL = the points are not wanted */
  uint64_t capacity;    /* points pts holds */
  uint64_t count;       /* points of all publishing lanes (written, or required on LOAM_E_CAPACITY) */
  uint32_t *offset;     /* caller-owned [n_lanes + 1] or NULL: lane l = pts[offset[l] .. offset[l+1]) */
  int32_t *published;   /* caller-owned [n_lanes] or NULL: 1 = lane l's last frame publishes the topic */
} loam_lanes_cloud;
/* loam_mapping_surround for the lanes (src/laserMapping.cpp:1038-1058).
 * When a lane is due: lane l is due after a pulled step on which the lane mapped (mapped = 1, status
 * = LOAM_OK) and its own mapFrameCount wrapped (its surround_phase went 4 -> 0): the lane's 1st
 * mapping frame since open, since a restart or since a surround_phase = 4 import, and every 5th
 * after that.  A lane is not due on its wait steps, on its init step, while it has failed or
 * retired, inside system_delay, or on a step that did not map.
 * Equality with a context: for a due lane the cloud is, bit for bit and in point order, what
 * loam_mapping_surround returns on the context that lane equals (a fresh context fed through
 * loam_imu + loam_chain_sweep; after a restart a fresh system_delay = 0 context; after
 * loam_lanes_map_import a context that received loam_map_import at that point): the in-bounds cubes
 * of the 5 x 5 x 5 neighbourhood of the frame's centre cube in (i, j, k) loop order, each cube's
 * corner points then its surf points from the store the frame left, through one VoxelGrid of leaf
 * 0.2.  A lane that is not due has published[l] = 0 and an empty range.
 * The result is valid from the pull of a step until the next loam_lanes_push /
 * loam_lanes_push_stamped.  loam_lanes_restart and loam_lanes_map_import drop the flag of the lanes
 * they touch (as loam_map_import does for a context); no other lane's flag changes.
 * The clouds are computed on demand: the call waits for nothing but its own work and changes
 * nothing in any lane (later steps, registered clouds and exported maps are bit-identical to a run
 * that never called it); it may be repeated, and repeated calls return the same bits.  One launch
 * sequence serves every due lane, the counts reach the host in one copy, and the points come back
 * packed in lane order through the download staging loam_batch_features and loam_map_export share.
 * When nothing is due (before the first pull too): LOAM_OK, every published = 0, every offset = 0,
 * count = 0, and nothing is launched.
 * pts == NULL is the sizes-only query; count, offset and published are always filled when given.
 * LOAM_E_CAPACITY (count > capacity) writes no point and fills count, offset and published, so the
 * call can be repeated with more room.
 * LOAM_E_INVAL, and nothing of out is written: a null ctx / out, lanes not open, a step in flight.
 * LOAM_E_HIP for a failed HIP call.  LOAM_E_NOMEM when the first call's allocation (two lane lists,
 * and the shared download staging if no call made it before) fails.  No allocation is sized by the
 * call: the scratch is the lanes' own VoxelGrid input / output arrays, idle between a pull and the
 * next push (loam_lanes_map_export uses them the same way). */
int loam_lanes_surround(loam_ctx *ctx, loam_lanes_cloud *out);

/* ---- every topic cloud of the last pulled step, for a list of lanes in one call ----
 * A loam_batch_cloud per topic, packed over the listed lanes: lane lane[i]'s points of a cloud are
 * pts[offset[i] .. offset[i+1]) and offset[n] = count (offset has n + 1 entries here). */
#define LOAM_LANE_CLOUDS 9
typedef struct {
  loam_batch_cloud full, sharp, less_sharp, flat, less_flat;   /* scanRegistration's five */
  loam_batch_cloud corner_last, surf_last;                     /* laserCloudCornerLast / SurfLast */
  loam_batch_cloud full_end;                                   /* /velodyne_cloud_3 */
  loam_batch_cloud registered;                                 /* /velodyne_cloud_registered */
} loam_lanes_clouds_out;

/* Valid between a pull and the next push, in both lane modes; lane = NULL lists lanes 0 .. n - 1
 * and needs n == n_lanes.  The protocol is loam_batch_features': a cloud whose pts and offset are
 * both NULL is not wanted and its struct is left untouched; for every other cloud count and (when
 * given) offset[0 .. n] are always filled, the points when pts is given; every pts NULL is the
 * sizes-only query; LOAM_E_CAPACITY (a wanted cloud's points do not fit its capacity) writes no
 * point, fills every wanted count / offset, and the call may be repeated.  The call changes nothing
 * in any lane and may be repeated with the same bits.
 * Contents, for a lane whose status on the last pulled step was LOAM_OK, bit for bit and in order:
 *   full .. less_flat   what loam_scan_registration writes for the lane's sweep (de-skewed where the
 *                       lane has IMU messages);
 *   corner_last, surf_last   the lane's Last clouds as that frame left them, the clouds
 *                       loam_lanes_score / loam_lanes_localize read: what loam_odometry writes on a
 *                       frame with LOAM_PUB_CLOUDS, the raw lessSharp / lessFlat clouds on the lane's
 *                       init frame; filled on frames that do not publish them too;
 *   full_end            on a frame whose pull record has LOAM_PUB_FULL, as loam_odometry writes it;
 *                       an empty range otherwise;
 *   registered          when the pull reported mapped = 1: n_registered points, what
 *                       loam_lanes_registered returns (0 for a LOAM_LOC_OFFGRID shared lane).
 * Every cloud is an empty range, without an error, for a failed or retired lane, a lane on a wait
 * step, a lane between loam_lanes_restart and the pull of its init step, every lane inside
 * system_delay and before the first pull.  When every range is empty nothing is launched.
 * LOAM_E_INVAL with out untouched: null ctx / out, lanes not open, a step in flight, n == 0 or
 * n > n_lanes, lane == NULL with n != n_lanes, an index >= n_lanes, a lane listed twice, a wanted
 * cloud of the list exceeding 2^32 - 1 points, or (the host form) a max_points so large that one
 * lane's nine clouds at their strides (5 max_points + 276 n_rings points) exceed the download
 * staging of 2^21 points.  That limit holds whichever clouds are wanted, for every call that gives a
 * pts; the sizes-only query and the device form use no staging and have no such limit.
 * LOAM_E_NOMEM when the first call's allocation fails, LOAM_E_HIP for a failed HIP call. */
int loam_lanes_clouds(loam_ctx *ctx, uint32_t n, const uint32_t *lane /* [n] or NULL */, loam_lanes_clouds_out *out);
/* The same with every pts in plain device memory of the context's device, 16-byte aligned, and
 * capacity * 16 bytes inside its allocation (anything else: LOAM_E_INVAL, nothing written).  The
 * points are packed straight into the caller's buffers: no staging, no device-to-host copy.  offset
 * and count stay host-side and are filled before return (the call's one small synchronisation).
 * consumer_stream (a hipStream_t) non-NULL: the stream is made to wait for the pack and the call
 * returns without waiting; NULL: the call synchronises before it returns.  Same bits as the host form.
 * The pack runs on the context's own stream and is ordered behind nothing of the caller's: whatever
 * still reads or writes the destination buffers, on consumer_stream or any other stream, must have
 * finished (or been synchronised with) before the call.  The lanes' own buffers need no such care: the
 * next push starts on the same stream, behind the pack. */
int loam_lanes_clouds_device(loam_ctx *ctx, uint32_t n, const uint32_t *lane, loam_lanes_clouds_out *out,
                             void *consumer_stream);

/* ---- shared lanes: every lane localizes in the context's one map, which a step only reads ----
 * Opens n_lanes lanes whose laserMapping refines against the context's streaming map (the store
 * loam_map_import / loam_mapping / loam_chain_sweep maintain), which a lanes step only reads.
 * No per-lane store exists.  lane_from_capacity = FromMap points one lane may gather per frame
 * (the points of its FOV-tested 5 x 5 x 5 valid cubes; 48 bytes each and 24 per hash bucket, DESIGN.md
 * §30, against 152 per point of lane_map_capacity).
 * Scan registration, the odometry, the IMU queues, the restart phase rule and every call not named
 * below work as on loam_lanes_open's lanes.  A context holds one set of lanes of one mode at a time.
 * A lane's mapping frame.  Let M be the context's map as loam_map_export would give it at the push
 * and (Aft, Bef) the lane's poses before the step.  The lane's aft, bef, mp_iters and registered
 * cloud are, bit for bit and in point order, what loam_mapping returns on a context that has just
 * received loam_map_import(M with aft = Aft, bef = Bef), has received the lane's IMU messages, and is
 * given the lane's od_sum, corner_last, surf_last and full_end.  Nothing is inserted, downsampled,
 * compacted or recentred: no bit of the map, its grid centre or the context's own Bef / Aft changes.
 *   - A lane whose centre cube is within 3 of a grid edge (a sequential frame would recentre the
 *     grid first) is not evaluated: mapped = 1, mp_iters = 0, n_registered = 0, Aft / Bef as they
 *     were, LOAM_LOC_OFFGRID in loam_lanes_localize_info.  Remedy: loam_map_import with another centre.
 *   - LOAM_LOC_NO_LM is the reference's own branch (src/laserMapping.cpp:706): the poses are left
 *     alone and the cloud is registered with transformTobeMapped.
 *   - A lane whose valid cubes hold more than lane_from_capacity points fails with the sticky
 *     LOAM_E_CAPACITY (found on the device: a push waits for nothing); no other lane is affected.  A
 *     map whose last update overflowed map_capacity fails every lane's mapping frame the same way.
 * The map may change between steps: loam_map_import, loam_mapping and loam_chain_sweep on this
 * context are allowed whenever no step is in flight, and the next step reads the store they left
 * (it waits on the device for a deferred map update).  One context can keep mapping while its lanes
 * localize in that map.
 * loam_lanes_map_import, loam_lanes_map_export and loam_lanes_surround are LOAM_E_INVAL on shared
 * lanes (there is no lane map): use loam_map_import, loam_map_export and loam_mapping_surround.
 * Errors: loam_lanes_open's, with lane_from_capacity in [1024, 2^28] and the 2^31 limits on n_lanes
 * x lane_from_capacity and n_lanes x (max_points + 120 n_rings).  LOAM_E_NOMEM frees everything. */
int loam_lanes_open_shared(loam_ctx *ctx, uint32_t n_lanes, uint32_t lane_from_capacity);

/* Aft / Bef of the listed lanes (bef NULL = zeros), between two steps; shared lanes only.  One
 * kernel launch writes every listed lane's poses.  The two uses:
 *   - at start or after a restart: bef = zeros, aft = the guess of the lane's pose in the map;
 *   - re-seeding a running lane (a better pose from loam_map_localize / loam_map_score): bef = the
 *     lane's last od_sum, so that only later odometry increments are applied on top of aft.
 * LOAM_E_INVAL, and nothing changes in any lane: a null ctx / lane / aft, lanes not open or opened
 * with loam_lanes_open, a step in flight, n == 0 or n > n_lanes, a lane index >= n_lanes, a lane
 * listed twice, a failed lane, a lane between loam_lanes_restart and the pull of its init step (the
 * restart's deferred clear would overwrite the pose).  LOAM_E_NOMEM when the first call's allocation
 * (two blocks of 13 n_lanes words) fails. */
int loam_lanes_set_pose(loam_ctx *ctx, uint32_t n, const uint32_t *lane, const loam_pose6 *aft, const loam_pose6 *bef);

/* loam_localize_result of every lane's mapping frame of the last pulled step; shared lanes only.
 * For a lane without IMU messages out[l] equals, field for field, loam_map_localize(n = 1, aft =
 * Aft, bef = Bef) with the lane's od_sum, corner_last and surf_last on a context holding M.
 * LOAM_LOC_NONE with zeros: the lane ran no mapping frame on that step (a step that did not map,
 * a wait or init step of a restarted lane, inside system_delay) or has failed.
 * LOAM_E_INVAL: a null argument, lanes not open or not shared, a step in flight, before the first pull. */
#define LOAM_LOC_NONE (LOAM_LOC_OFFGRID + 1)   /* = 3, behind loam_map_localize's statuses: the lane ran no mapping frame on that step */
int loam_lanes_localize_info(loam_ctx *ctx, loam_localize_result *out /* [n_lanes] */);

/* loam_map_score for the lanes, between two steps, in both lane modes: k pose guesses for each of n
 * listed lanes in one call, one index of the map and one synchronisation for all of them.
 * out[i*k + j], i < n, j < k, is bit for bit (all 32 bytes) what loam_map_score(ctx, C, S, max_dist,
 * 1, &pose[i*k + j], ..) returns on this context, where C / S are lane lane[i]'s
 * laserCloudCornerLast / laserCloudSurfLast as its last pulled frame left them: what loam_odometry
 * writes into corner_last / surf_last on the context the lane equals (the raw lessSharp / lessFlat
 * clouds on the lane's init frame, src/laserOdometry.cpp:427-434, the TransformToEnd clouds on every
 * later frame, :875-902), whether or not that frame publishes them.  They are read in place on the
 * device, in their stored order.  A row depends on the map, the lane's clouds, max_dist and its own
 * pose only: not on n, k, its position in the call, or the run.
 * The map is the context's streaming map: on shared lanes the map the lanes localize in, on
 * loam_lanes_open lanes whatever loam_map_import put into the context (the prior map a caller is
 * about to hand to loam_lanes_map_import with aft = the best guess); a lane's own store is not read.
 * The call waits for the context's queued work (a deferred map update included), changes nothing
 * in the context or in any lane, and may be repeated.  An empty map is no error: every count is 0
 * and every cost is scored * r2.
 * LOAM_E_INVAL, with out untouched: a null argument, lanes not open, a step in flight, no pulled
 * step yet on which the odometry was initialised (inside system_delay), n == 0 or n > n_lanes,
 * k == 0, n x k > LOAM_SCORE_MAX, max_dist not in (0, 1], a lane index >= n_lanes, a lane listed
 * twice, a failed lane, a lane between loam_lanes_restart and the pull of its init step, a map whose
 * last update overflowed map_capacity.  LOAM_E_NOMEM / LOAM_E_HIP as loam_map_score. */
int loam_lanes_score(loam_ctx *ctx, uint32_t n, const uint32_t *lane /* [n] */, float max_dist,
                     uint32_t k, const loam_pose6 *pose /* [n][k] */, loam_score_result *out /* [n][k] */);

/* loam_map_localize for the lanes, between two steps, in both lane modes: k candidate poses for each
 * of n listed lanes, each lane's candidates refined for that lane's own last sweep, all n x k in one
 * launch sequence.  out[i*k + j], i < n, j < k, is bit for bit (all 60 bytes) what
 * loam_map_localize(ctx, &Sum, C, S, 1, &aft[i*k + j], bef ? &bef[i*k + j] : NULL, ..) returns on
 * this context, where C / S are lane lane[i]'s laserCloudCornerLast / laserCloudSurfLast as its last
 * pulled frame left them (the clouds loam_lanes_score reads) and Sum is the lane's transformSum: the
 * od_sum the pull reported on a frame with LOAM_PUB_POSE.  All three are read in place on the device.
 * A row depends on the map, the lane's clouds and Sum, and its own (aft, bef) only: not on n, k, its
 * position in the call, or the run.  The map is the context's streaming map, as for loam_lanes_score.
 * As in loam_map_localize no IMU blend is applied: for a lane that receives IMU messages a row is
 * therefore not what the lane's own shared step computes from the same poses.  Only the batch forms
 * of the L-M run, never the persistent one-instance kernels.
 * The call waits for the context's queued work (a deferred map update included), writes nothing but
 * the localization working set it shares with loam_map_localize (grown on demand, kept until
 * loam_destroy), changes nothing in the map or in any lane, and may be repeated.  To use a result,
 * hand its aft to loam_lanes_set_pose with bef = the lane's od_sum.
 * LOAM_E_INVAL, with out untouched: a null ctx / lane / aft / out (bef may be NULL = zeros), lanes
 * not open, a step in flight, no pulled step yet on which the odometry was initialised, n == 0 or
 * n > n_lanes, k == 0, n x k > LOAM_LOCALIZE_MAX, a lane index >= n_lanes, a lane listed twice, a
 * failed lane, a lane between loam_lanes_restart and the pull of its init step, a listed lane whose
 * corner cloud exceeds the mapping stack's 120 points per ring, a map whose last update overflowed
 * map_capacity.  LOAM_E_NOMEM / LOAM_E_HIP as loam_map_localize.  In every error case the context
 * and the lanes are as they were. */
int loam_lanes_localize(loam_ctx *ctx, uint32_t n, const uint32_t *lane /* [n] */, uint32_t k,
                        const loam_pose6 *aft /* [n][k] */, const loam_pose6 *bef /* [n][k] or NULL = zeros */,
                        loam_localize_result *out /* [n][k] */);
/* The write-back half of the shared mode, between two steps, shared lanes only: the listed lanes'
 * last pulled mapping frames enter the context's map in one call.  It is laserMapping's
 * map update (src/laserMapping.cpp:980-1036: insertion, then the VoxelGrid of the frame's valid
 * cubes) for all listed lanes at once.  Let M be the map as loam_map_export gives it before the call.
 * A listed lane's stack is the downsampled CornerStack / SurfStack of its last pulled mapping frame,
 * taken into the map frame with the pose the frame registered its cloud with (transformTobeMapped
 * after the L-M and the IMU blend, or the predicted pose of a LOAM_LOC_NO_LM frame); its valid set is
 * that frame's laserCloudValidInd.  Both are read in place on the device.  After the call, per kind
 * (corner, surf) and cube c:
 *   content(c) = M(c) ++ the stack points of lane[0] that fall into c ++ those of lane[1] ++ ...
 * (each lane's points in stack order, c by the reference's cube formula about the map's centre); if c
 * is in the union of the listed lanes' valid sets, content(c) goes through one PCL VoxelGrid (leaf
 * 0.2 corner, 0.4 surf), otherwise it stays the concatenation.  The result depends on M, the listed
 * lanes' frames and the order of the list only.  With n = 1 it is, bit for bit, the map a context
 * holds that imported M with the lane's Aft / Bef and was given the lane's sweep by loam_mapping.
 * No lane state, no pose, not the context's Bef / Aft or surround_phase and not the grid centre
 * change, and the grid is never recentred; /laser_cloud_surround of the context's last own frame is
 * no longer due (as after loam_map_import).  The next step reads the new map; loam_mapping /
 * loam_chain_sweep on the context continue in it.  The call synchronises.
 * Commit before anything moves the map's centre (a loam_map_import with another centre, a
 * loam_mapping / loam_chain_sweep on the context that recentres the grid): the lanes' valid sets are
 * cube indices about the centre their frames ran with, and this is not checked.
 * LOAM_E_INVAL, with nothing changed and out unwritten: a null argument, lanes not open or opened
 * with loam_lanes_open, a step in flight, n == 0 or n > n_lanes, a lane index >= n_lanes, a lane
 * listed twice, a failed lane, a lane between loam_lanes_restart and the pull of its init step, a
 * lane whose last pulled step was not a mapping frame of its own with LOAM_LOC_SOLVED or
 * LOAM_LOC_NO_LM (LOAM_LOC_NONE, LOAM_LOC_OFFGRID, inside system_delay), a lane whose frame was
 * committed since that pull (a frame enters the map once), a map whose last update overflowed
 * map_capacity.
 * LOAM_E_CAPACITY, with the map unchanged bit for bit and only out->map_points written: the VoxelGrid
 * input of the union's cubes (old content and appended points, both kinds) or the map after the
 * commit exceeds map_capacity.  map_points then holds, per kind, the points of the one that did not
 * fit (the VoxelGrid input is found first); their sum is the map_capacity that part needs.
 * LOAM_E_NOMEM when the first call's working set (sized by n_lanes and the stack capacity, 24 bytes
 * per stack point and lane) cannot be allocated; LOAM_E_HIP. */
typedef struct {
  uint64_t inserted[2];   /* corner, surf points appended (inside the grid) */
  uint64_t outside[2];    /* stack points outside the cube grid, dropped as the reference drops them */
  uint64_t map_points[2]; /* the map's corner / surf points after the commit */
  uint32_t cubes;         /* cubes of the union of the listed lanes' valid sets */
} loam_commit_result;
int loam_lanes_map_commit(loam_ctx *ctx, uint32_t n, const uint32_t *lane /* [n] */, loam_commit_result *out);

/* Frees the lanes' working set (waits for a step in flight).  LOAM_E_INVAL when not open. */
int loam_lanes_close(loam_ctx *ctx);

/* scheduling (no reference equivalent; the reference's nodes are OS processes): priority of the
 * context's HIP streams.  priority > 0 = the device's highest stream priority, 0 = normal,
 * < 0 = lowest.  Used by a node pipeline to favour its critical node (laserMapping) when several
 * contexts share one GPU.  Waits for the context's queued work, then replaces its streams. */
int loam_set_stream_priority(loam_ctx *ctx, int priority);

/* launch-shape choices of the batch / streaming L-M loops by batch size (no reference equivalent):
 * key = one of od_small_max, od_fused_max, mp_small_max, mp_fused_max, od_assoc_wg, fit_wg, graph,
 * vg_merge, vg_merge_min, vg_split, sr_ahead, sr_ahead_at, step_pipe, batch_streams, pipe_mp_sets, od_sel_min, od_win_mono,
 * od_win_mono_min, od_moments_min, od_persist, mp_persist, stream_defer, od_graph, pipe_sr_sets, od_nn_lane,
 * od_nn_lane_min (loam_velodyne-1_amd/csrc/engine.hpp, struct Tuning).  od_nn_lane: the odometry association's
 * nearest neighbour on a lane per query in the TransformToStart launch, for batches of od_nn_lane_min (and
 * od_sel_min) problems or more: 0 off (a wave per query), 1 in the seeded association rounds, 2 in every
 * round.  Every choice computes the same results bit for bit except od_moments_min (the odometry's
 * stored rows as per-query fp64 moments: within the north star's 1e-4 of the reference);
 * the defaults are the measured fastest.  LOAM_E_INVAL for an unknown key or a value out of range.
 * Takes effect from the next call (waits for the context's queued work). */
int loam_set_tuning(loam_ctx *ctx, const char *key, long long value);
/* the current value of a launch choice (LOAM_E_INVAL for an unknown key) */
int loam_get_tuning(loam_ctx *ctx, const char *key, long long *value);

/* last-call statistics of a context (stage device times, counts, algorithmic bytes) */
int loam_get_stats(loam_ctx *ctx, loam_stats *stats);

/* diagnostics (no reference equivalent): per-kernel device time of the batch path, measured with
 * HIP events on the context stream.  loam_get_kernel_times writes "name total_ms launches\n" lines. */
int loam_set_profiling(loam_ctx *ctx, int on);
int loam_get_kernel_times(loam_ctx *ctx, char *buf, uint32_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LOAM_LOAM_H */
