"""ctypes binding of libloam_hip.so, the MI355X LOAM scan-matching engine (C-ABI in
include/loam/loam.h).  One `Engine` = one loam_ctx = the four reference ROS nodes' compute bodies
on one GPU:

    scan_registration(raw)          laserCloudHandler    src/scanRegistration.cpp:211-636
    odometry(features)              laserOdometry body   src/laserOdometry.cpp:413-931
    mapping(pose, corner, surf, full) laserMapping body  src/laserMapping.cpp:411-1097
    maintenance(sum, bef, aft)      transformMaintenance src/transformMaintenance.cpp:147-203
    batch_*                         config 4 (independent problems)
    lanes_*                         many sequences in lockstep (with IMU §23)

There is no CPU path: without a GPU (or without the built library) every call raises.
The package directory name contains '-', so import it with
importlib.import_module("loam_velodyne-1_amd")."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LOAM_HIP_LIB") or os.path.join(_HERE, "libloam_hip.so")
_LIB = None

LOAM_OK, LOAM_E_INVAL, LOAM_E_CAPACITY, LOAM_E_HIP, LOAM_E_NOT_READY, LOAM_E_NOMEM = 0, -1, -2, -3, -4, -5
PUB_POSE, PUB_CLOUDS, PUB_FULL = 1, 2, 4
RING_VLP16, RING_LINEAR = 0, 1
RING_TABLE_MAX = 64  # LOAM_RING_TABLE_MAX: intervals of a ring table (Engine.set_ring_table)
# LOAM_FIELD_*: the type of a record's ring or time field (Engine.set_point_fields)
FIELD_NONE, FIELD_U8, FIELD_U16, FIELD_U32, FIELD_F32, FIELD_F64 = 0, 1, 2, 3, 4, 5
RING_MAP_MAX = 256   # LOAM_RING_MAP_MAX: entries of a ring map


class LoamError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"loam error {code}: {msg}")
        self.code = code


class CloudIn(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("count", ctypes.c_uint32), ("stride_bytes", ctypes.c_uint32)]


class PointFields(ctypes.Structure):
    """include/loam/loam.h loam_point_fields: where a record keeps its ring and its time"""
    _fields_ = [("ring_type", ctypes.c_uint32), ("ring_offset", ctypes.c_uint32),
                ("time_type", ctypes.c_uint32), ("time_offset", ctypes.c_uint32),
                ("time_scale", ctypes.c_double), ("time_bias", ctypes.c_double),
                ("ring_map", ctypes.POINTER(ctypes.c_int32)), ("ring_map_n", ctypes.c_uint32)]

    @staticmethod
    def of(ring, time=None, ring_map=None):
        """ring = (type, offset); time = None or (type, offset, scale, bias); ring_map = None or ints
        (-1 = drop).  The structure keeps the map's storage alive."""
        f = PointFields()
        f.ring_type, f.ring_offset = int(ring[0]), int(ring[1])
        f.time_scale = 1.0
        if time is not None:
            f.time_type, f.time_offset = int(time[0]), int(time[1])
            f.time_scale, f.time_bias = float(time[2]), float(time[3])
        if ring_map is not None:
            m = np.ascontiguousarray(ring_map, np.int32).reshape(-1)
            f._map = m
            f.ring_map = m.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
            f.ring_map_n = len(m)
        return f


class CloudOut(ctypes.Structure):
    _fields_ = [("pts", ctypes.c_void_p), ("count", ctypes.c_uint32), ("capacity", ctypes.c_uint32)]


class Features(ctypes.Structure):
    _fields_ = [("full", CloudOut), ("sharp", CloudOut), ("less_sharp", CloudOut),
                ("flat", CloudOut), ("less_flat", CloudOut), ("imu_trans", ctypes.c_float * 12)]


class Pose6(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("rx", "ry", "rz", "tx", "ty", "tz")]

    def arr(self):
        return np.array([self.rx, self.ry, self.rz, self.tx, self.ty, self.tz], np.float32)

    @staticmethod
    def of(a):
        p = Pose6()
        p.rx, p.ry, p.rz, p.tx, p.ty, p.tz = [float(v) for v in a]
        return p


class OdometryMsg(ctypes.Structure):
    """include/loam/loam_msg.h loam_odometry_msg (nav_msgs/Odometry fields the reference writes)"""
    _fields_ = [("stamp", ctypes.c_double), ("frame_id", ctypes.c_char_p), ("child_frame_id", ctypes.c_char_p),
                ("orientation", ctypes.c_double * 4), ("position", ctypes.c_double * 3),
                ("twist_angular", ctypes.c_double * 3), ("twist_linear", ctypes.c_double * 3)]


class TfMsg(ctypes.Structure):
    _fields_ = [("stamp", ctypes.c_double), ("frame_id", ctypes.c_char_p), ("child_frame_id", ctypes.c_char_p),
                ("rotation", ctypes.c_double * 4), ("origin", ctypes.c_double * 3)]


MSG_LASER_ODOM, MSG_AFT_MAPPED, MSG_INTEGRATED = 0, 1, 2


class Config(ctypes.Structure):
    _fields_ = [("n_rings", ctypes.c_uint32), ("ring_model", ctypes.c_uint32),
                ("ring_lo_deg", ctypes.c_float), ("ring_hi_deg", ctypes.c_float),
                ("system_delay", ctypes.c_uint32), ("max_points", ctypes.c_uint32),
                ("od_max_iter", ctypes.c_uint32), ("mp_max_iter", ctypes.c_uint32),
                ("skip_frame_num", ctypes.c_uint32), ("map_capacity", ctypes.c_uint32)]


STAT_U64 = ("n_raw", "n_ring", "n_sharp", "n_less_sharp", "n_flat", "n_less_flat",
            "od_iters", "od_assoc_rounds", "od_rows_sum", "od_corner_last", "od_surf_last", "od_queries",
            "od_assoc_points",
            "mp_iters", "mp_rows_sum", "mp_stack", "mp_map_points", "mp_map_valid_points", "mp_stack_iters",
            "mp_fits", "od_query_iters", "od_row_evals",
            "bytes_sr", "bytes_od", "bytes_mp")


STAT_BRANCH = ("od_degenerate_steps", "od_nan_skips", "mp_degenerate_steps", "mp_grid_shifts")
STAT_WORK = ("mp_nn_candidates", "mp_nn_cells", "od_assoc_gathered", "od_assoc_boxes")


class ChainOut(ctypes.Structure):
    _fields_ = [("published", ctypes.c_int32), ("mapped", ctypes.c_int32), ("od_sum", Pose6),
                ("aft", Pose6), ("bef", Pose6), ("registered", CloudOut)]


class Stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in STAT_U64] + \
               [(n, ctypes.c_double) for n in ("ms_sr", "ms_od", "ms_mp")] + \
               [(n, ctypes.c_uint64) for n in STAT_BRANCH + STAT_WORK]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class BatchCloud(ctypes.Structure):
    """include/loam/loam.h loam_batch_cloud: one cloud of every selected sweep, packed back to back"""
    _fields_ = [("pts", ctypes.c_void_p), ("capacity", ctypes.c_uint64), ("count", ctypes.c_uint64),
                ("offset", ctypes.c_void_p)]


BATCH_CLOUDS = ("full", "sharp", "less_sharp", "flat", "less_flat")


class BatchClouds(ctypes.Structure):
    _fields_ = [(n, BatchCloud) for n in BATCH_CLOUDS]


MAP_CUBES = 4851  # LOAM_MAP_CUBES: 21 * 11 * 21 (src/laserMapping.cpp:64-70)


class MapCloud(ctypes.Structure):
    """include/loam/loam.h loam_map_cloud: one cloud of the cube map in canonical order"""
    _fields_ = [("pts", ctypes.c_void_p), ("capacity", ctypes.c_uint64), ("count", ctypes.c_uint64),
                ("cube_offset", ctypes.c_void_p)]


class Map(ctypes.Structure):
    """include/loam/loam.h loam_map"""
    _fields_ = [("corner", MapCloud), ("surf", MapCloud), ("center", ctypes.c_int32 * 3),
                ("surround_phase", ctypes.c_int32), ("aft", Pose6), ("bef", Pose6)]


MAP_KEYS = ("corner", "surf", "corner_offset", "surf_offset", "center", "surround_phase", "aft", "bef")

LOC_SOLVED, LOC_NO_LM, LOC_OFFGRID = 0, 1, 2  # LOAM_LOC_*: a candidate's status
LOCALIZE_MAX = 1024  # LOAM_LOCALIZE_MAX: candidates of one loam_map_localize call


class LocalizeResult(ctypes.Structure):
    """include/loam/loam.h loam_localize_result: one candidate of loam_map_localize"""
    _fields_ = [("aft", Pose6), ("status", ctypes.c_int32), ("iters", ctypes.c_int32),
                ("degenerate_steps", ctypes.c_int32), ("rows_last", ctypes.c_uint32), ("rows_sum", ctypes.c_uint32),
                ("stack_corner", ctypes.c_uint32), ("stack_surf", ctypes.c_uint32),
                ("map_corner", ctypes.c_uint32), ("map_surf", ctypes.c_uint32)]


LOCALIZE_KEYS = tuple(n for n, _ in LocalizeResult._fields_)
LOC_NONE = 3  # LOAM_LOC_NONE (loam_lanes_localize_info): the lane ran no mapping frame on that step
_LOC_DTYPE = np.dtype([(n, np.float32, (6,)) if t is Pose6 else (n, np.uint32 if t is ctypes.c_uint32 else np.int32)
                       for n, t in LocalizeResult._fields_])

SCORE_MAX = 65536  # LOAM_SCORE_MAX: poses of one loam_map_score call


class ScoreResult(ctypes.Structure):
    """include/loam/loam.h loam_score_result: one pose of loam_map_score"""
    _fields_ = [("corner_scored", ctypes.c_uint32), ("surf_scored", ctypes.c_uint32),
                ("corner_in", ctypes.c_uint32), ("surf_in", ctypes.c_uint32),
                ("corner_cost", ctypes.c_double), ("surf_cost", ctypes.c_double)]


SCORE_KEYS = tuple(n for n, _ in ScoreResult._fields_)
_SCORE_DTYPE = np.dtype([(n, np.float64 if t is ctypes.c_double else np.uint32) for n, t in ScoreResult._fields_])


LANES_MAX = 1024  # LOAM_LANES_MAX: lanes of one context


class CommitResult(ctypes.Structure):
    """include/loam/loam.h loam_commit_result: what loam_lanes_map_commit did to the map"""
    _fields_ = [("inserted", ctypes.c_uint64 * 2), ("outside", ctypes.c_uint64 * 2),
                ("map_points", ctypes.c_uint64 * 2), ("cubes", ctypes.c_uint32)]


FEED_WAIT, FEED_RELEASE = 1, 2  # LOAM_FEED_*: loam_lanes_push_device's ordering against the producer's stream


class LaneOut(ctypes.Structure):
    """include/loam/loam.h loam_lane_out: one lane of a lanes step"""
    _fields_ = [("status", ctypes.c_int32), ("published", ctypes.c_int32), ("mapped", ctypes.c_int32),
                ("od_iters", ctypes.c_int32), ("mp_iters", ctypes.c_int32), ("od_sum", Pose6), ("aft", Pose6),
                ("bef", Pose6), ("n_registered", ctypes.c_uint32)]


LANE_KEYS = tuple(n for n, _ in LaneOut._fields_)
_LANE_DTYPE = np.dtype([(n, np.float32, (6,)) if t is Pose6 else (n, np.uint32 if t is ctypes.c_uint32 else np.int32)
                        for n, t in LaneOut._fields_])


class LanesCloud(ctypes.Structure):
    """include/loam/loam.h loam_lanes_cloud: /laser_cloud_surround of every publishing lane, packed"""
    _fields_ = [("pts", ctypes.c_void_p), ("capacity", ctypes.c_uint64), ("count", ctypes.c_uint64),
                ("offset", ctypes.c_void_p), ("published", ctypes.c_void_p)]


LANE_CLOUDS = BATCH_CLOUDS + ("corner_last", "surf_last", "full_end", "registered")  # LOAM_LANE_CLOUDS, in order


class LanesCloudsOut(ctypes.Structure):
    """include/loam/loam.h loam_lanes_clouds_out: every topic cloud of the listed lanes, packed per topic"""
    _fields_ = [(n, BatchCloud) for n in LANE_CLOUDS]


EXPORTS = ("loam_config_default", "loam_create", "loam_destroy", "loam_last_error", "loam_imu",
           "loam_scan_registration", "loam_odometry", "loam_mapping", "loam_mapping_surround",
           "loam_maintenance", "loam_chain_sweep",
           "loam_ring_table_check", "loam_ring_table_of_model", "loam_set_ring_table",
           "loam_point_fields_check", "loam_set_point_fields",
           "loam_batch_upload", "loam_batch_feed", "loam_batch_run", "loam_batch_sync", "loam_batch_download", "loam_batch_lm_info", "loam_batch_features", "loam_map_export", "loam_map_import", "loam_map_localize", "loam_map_score", "loam_get_stats",
           "loam_lanes_open", "loam_lanes_push", "loam_lanes_pull", "loam_lanes_registered", "loam_lanes_map_export",
           "loam_lanes_close", "loam_lanes_imu", "loam_lanes_push_stamped", "loam_lanes_imu_trans",
           "loam_lanes_restart", "loam_lanes_map_import", "loam_lanes_surround",
           "loam_lanes_open_shared", "loam_lanes_set_pose", "loam_lanes_localize_info", "loam_lanes_score",
           "loam_lanes_localize", "loam_lanes_push_device", "loam_lanes_map_commit",
           "loam_lanes_clouds", "loam_lanes_clouds_device",
           "loam_set_profiling", "loam_get_kernel_times", "loam_set_stream_priority", "loam_set_tuning",
           "loam_get_tuning",
           # include/loam/loam_bag.h: recorded-sweep ingest (rosbag v2, PointCloud2, Imu)
           "loam_bag_open", "loam_bag_close", "loam_bag_next", "loam_pc2_parse", "loam_pc2_cloud", "loam_pc2_point_fields",
           "loam_imu_parse",
           # include/loam/loam_msg.h: the reference's pose message conventions
           "loam_msg_from_pose", "loam_pose_from_msg")


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is not built (run __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        P, PP = ctypes.POINTER, ctypes.c_void_p
        L.loam_config_default.argtypes = [P(Config)]
        L.loam_create.argtypes = [P(PP), P(Config), ctypes.c_int]
        L.loam_destroy.argtypes = [PP]
        L.loam_last_error.restype = ctypes.c_char_p
        L.loam_scan_registration.argtypes = [PP, ctypes.c_double, CloudIn, P(Features)]
        L.loam_imu.argtypes = [PP, ctypes.c_double, P(ctypes.c_double), P(ctypes.c_double)]
        L.loam_odometry.argtypes = [PP, ctypes.c_double, P(Features), P(Pose6), P(CloudOut), P(CloudOut),
                                    P(CloudOut), P(ctypes.c_int)]
        L.loam_mapping.argtypes = [PP, ctypes.c_double, P(Pose6), P(CloudOut), P(CloudOut), P(CloudOut),
                                   P(Pose6), P(Pose6), P(CloudOut)]
        L.loam_mapping_surround.argtypes = [PP, P(CloudOut), P(ctypes.c_int)]
        L.loam_chain_sweep.argtypes = [PP, ctypes.c_double, CloudIn, P(ChainOut)]
        L.loam_maintenance.argtypes = [P(Pose6)] * 4
        L.loam_ring_table_check.argtypes = [ctypes.c_uint32, ctypes.c_uint32, P(ctypes.c_float), P(ctypes.c_int32)]
        L.loam_ring_table_of_model.argtypes = [P(Config), P(ctypes.c_uint32), P(ctypes.c_float), P(ctypes.c_int32)]
        L.loam_set_ring_table.argtypes = [PP, ctypes.c_uint32, P(ctypes.c_float), P(ctypes.c_int32)]
        L.loam_point_fields_check.argtypes = [ctypes.c_uint32, P(PointFields)]
        L.loam_set_point_fields.argtypes = [PP, P(PointFields)]
        L.loam_batch_upload.argtypes = [PP, ctypes.c_uint32, P(CloudIn), P(CloudIn)]
        L.loam_batch_feed.argtypes = [PP, ctypes.c_uint32, P(CloudIn), P(CloudIn)]
        L.loam_batch_run.argtypes = [PP]
        L.loam_batch_sync.argtypes = [PP]
        L.loam_set_profiling.argtypes = [PP, ctypes.c_int]
        L.loam_set_stream_priority.argtypes = [PP, ctypes.c_int]
        L.loam_set_tuning.argtypes = [PP, ctypes.c_char_p, ctypes.c_longlong]
        L.loam_get_tuning.argtypes = [PP, ctypes.c_char_p, P(ctypes.c_longlong)]
        L.loam_get_kernel_times.argtypes = [PP, ctypes.c_char_p, ctypes.c_uint32]
        L.loam_batch_download.argtypes = [PP, P(Pose6), P(Pose6), P(Stats)]
        L.loam_batch_lm_info.argtypes = [PP, P(ctypes.c_int32), P(ctypes.c_int32), P(Pose6)]
        L.loam_batch_features.argtypes = [PP, ctypes.c_uint32, ctypes.c_uint32, P(BatchClouds)]
        L.loam_map_export.argtypes = [PP, P(Map)]
        L.loam_map_import.argtypes = [PP, P(Map), P(ctypes.c_uint64)]
        L.loam_map_localize.argtypes = [PP, P(Pose6), P(CloudOut), P(CloudOut), ctypes.c_uint32, P(Pose6), P(Pose6),
                                        P(LocalizeResult)]
        L.loam_map_score.argtypes = [PP, P(CloudOut), P(CloudOut), ctypes.c_float, ctypes.c_uint32, P(Pose6),
                                     P(ScoreResult)]
        L.loam_get_stats.argtypes = [PP, P(Stats)]
        L.loam_lanes_open.argtypes = [PP, ctypes.c_uint32, ctypes.c_uint32]
        L.loam_lanes_push.argtypes = [PP, ctypes.c_double, P(CloudIn)]
        L.loam_lanes_pull.argtypes = [PP, P(LaneOut)]
        L.loam_lanes_registered.argtypes = [PP, ctypes.c_uint32, P(CloudOut)]
        L.loam_lanes_map_export.argtypes = [PP, ctypes.c_uint32, P(Map)]
        L.loam_lanes_close.argtypes = [PP]
        L.loam_lanes_imu.argtypes = [PP, ctypes.c_uint32, ctypes.c_double, P(ctypes.c_double), P(ctypes.c_double)]
        L.loam_lanes_push_stamped.argtypes = [PP, P(ctypes.c_double), P(CloudIn)]
        L.loam_lanes_imu_trans.argtypes = [PP, P(ctypes.c_float)]
        L.loam_lanes_restart.argtypes = [PP, ctypes.c_uint32, P(ctypes.c_uint32)]
        L.loam_lanes_map_import.argtypes = [PP, ctypes.c_uint32, P(ctypes.c_uint32), P(Map), P(Pose6),
                                            P(ctypes.c_uint64)]
        L.loam_lanes_surround.argtypes = [PP, P(LanesCloud)]
        L.loam_lanes_open_shared.argtypes = [PP, ctypes.c_uint32, ctypes.c_uint32]
        L.loam_lanes_set_pose.argtypes = [PP, ctypes.c_uint32, P(ctypes.c_uint32), P(Pose6), P(Pose6)]
        L.loam_lanes_localize_info.argtypes = [PP, P(LocalizeResult)]
        L.loam_lanes_score.argtypes = [PP, ctypes.c_uint32, P(ctypes.c_uint32), ctypes.c_float, ctypes.c_uint32, P(Pose6),
                                       P(ScoreResult)]
        L.loam_lanes_localize.argtypes = [PP, ctypes.c_uint32, P(ctypes.c_uint32), ctypes.c_uint32, P(Pose6), P(Pose6),
                                          P(LocalizeResult)]
        L.loam_lanes_push_device.argtypes = [PP, P(ctypes.c_double), P(CloudIn), ctypes.c_void_p, ctypes.c_uint32]
        L.loam_lanes_map_commit.argtypes = [PP, ctypes.c_uint32, P(ctypes.c_uint32), P(CommitResult)]
        L.loam_lanes_clouds.argtypes = [PP, ctypes.c_uint32, P(ctypes.c_uint32), P(LanesCloudsOut)]
        L.loam_lanes_clouds_device.argtypes = [PP, ctypes.c_uint32, P(ctypes.c_uint32), P(LanesCloudsOut),
                                               ctypes.c_void_p]
        L.loam_msg_from_pose.argtypes = [ctypes.c_int, ctypes.c_double, P(Pose6), P(Pose6), P(OdometryMsg), P(TfMsg)]
        L.loam_pose_from_msg.argtypes = [P(OdometryMsg), P(Pose6), P(Pose6)]
        _LIB = L
    return _LIB


def _check(rc):
    if rc != LOAM_OK:
        raise LoamError(rc, lib().loam_last_error().decode())
    return rc


def default_config(**kw):
    c = Config()
    lib().loam_config_default(ctypes.byref(c))
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _ring_table_args(bounds, rings):
    b = np.ascontiguousarray(bounds, np.float32).reshape(-1)
    r = np.ascontiguousarray(rings, np.int32).reshape(-1)
    if len(b) != len(r) + 1:
        raise ValueError("a ring table of n intervals has n + 1 bounds and n rings")
    return (b.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            len(r), (b, r))


def ring_table_check(n_rings, bounds, rings):
    """loam_ring_table_check: raises LoamError with the rule a table (bounds [n + 1] degrees, rings [n]) breaks"""
    pb, pr, n, _keep = _ring_table_args(bounds, rings)
    _check(lib().loam_ring_table_check(n_rings, n, pb, pr))


def ring_table_of_model(cfg):
    """loam_ring_table_of_model: (bounds float32 [n + 1], rings int32 [n]) restating cfg's built-in ring model"""
    b = np.zeros(RING_TABLE_MAX + 1, np.float32)
    r = np.zeros(RING_TABLE_MAX, np.int32)
    n = ctypes.c_uint32(0)
    _check(lib().loam_ring_table_of_model(ctypes.byref(cfg), ctypes.byref(n),
                                          b.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                          r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
    return b[:n.value + 1].copy(), r[:n.value].copy()


def ring_table_from_elevations(elev_deg):
    """the ring table of a lidar from its beams' elevations (degrees, any order, 2 .. 64 distinct values; ValueError otherwise):
    the beams sorted by ascending elevation are rings 0 .. R - 1 (the odometry's neighbouring-ring test
    needs ring order to follow elevation), the bounds are the midpoints between neighbouring beams,
    and each outer bound lies half the nearest spacing beyond its end beam.
    Returns (bounds float32 [R + 1], rings int32 [R]); ring i is beam np.argsort(elev_deg)[i]."""
    e = np.sort(np.asarray(elev_deg, np.float64).reshape(-1))
    if not 2 <= len(e) <= RING_TABLE_MAX:
        raise ValueError(f"2 .. {RING_TABLE_MAX} beams, not {len(e)}")
    if not np.all(np.isfinite(e)) or np.any(np.diff(e) <= 0):
        raise ValueError("the elevations must be finite and distinct")
    mid = 0.5 * (e[:-1] + e[1:])
    bounds = np.concatenate([[e[0] - 0.5 * (e[1] - e[0])], mid, [e[-1] + 0.5 * (e[-1] - e[-2])]])
    return bounds.astype(np.float32), np.arange(len(e), dtype=np.int32)


def point_fields_check(n_rings, fields):
    """loam_point_fields_check: raises LoamError with the rule a PointFields breaks"""
    _check(lib().loam_point_fields_check(n_rings, ctypes.byref(fields) if fields is not None else None))


def records(xyz, ring, time=None):
    """velodyne-layout (PointXYZIRT) records of a sweep: 32 bytes each, x, y, z float32 at 0 / 4 / 8,
    ring uint16 at 20, time float32 at 24 (0 when time is None), everything else 0.  Returns
    (CloudIn, keep-alive); the fields are ring=(FIELD_U16, 20), time=(FIELD_F32, 24, 1.0, 0.0)."""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    rec = np.zeros((max(n, 1), 32), np.uint8)
    rec[:n, 0:12] = np.ascontiguousarray(xyz).view(np.uint8).reshape(n, 12)
    rec[:n, 20:22] = np.ascontiguousarray(ring, np.uint16).reshape(n, 1).view(np.uint8)
    if time is not None:
        rec[:n, 24:28] = np.ascontiguousarray(time, np.float32).reshape(n, 1).view(np.uint8)
    return CloudIn(rec.ctypes.data, n, 32), rec


def _cloud_in(a):
    """an (n, >= 3) float array, or a ready loam_cloud_in (a strided view of caller memory, e.g. a
    PointCloud2 message's records: rosbag.pc2_cloud_in) passed through as is"""
    if isinstance(a, CloudIn):
        return a, None
    a = np.ascontiguousarray(a, np.float32)
    return CloudIn(a.ctypes.data, a.shape[0], a.shape[1] * 4), a


def _cloud_in_device(r):
    """a sweep in device memory as a loam_cloud_in: a ready CloudIn, a (ptr, count, stride_bytes)
    tuple, or an object with __cuda_array_interface__ (a torch tensor on the GPU): 2-D float32, at
    least 3 columns, unit column stride"""
    if isinstance(r, CloudIn):
        return r
    if isinstance(r, tuple):
        ptr, count, stride = r
        return CloudIn(int(ptr) or None, int(count), int(stride))
    cai = getattr(r, "__cuda_array_interface__", None)
    if cai is None:
        raise ValueError("a device sweep is a CloudIn, a (ptr, count, stride_bytes) tuple or an object with "
                         "__cuda_array_interface__")
    shape, strides = tuple(cai["shape"]), cai.get("strides")
    if np.dtype(cai["typestr"]) != np.dtype(np.float32):
        raise ValueError("a device sweep must be float32")
    if len(shape) != 2 or shape[1] < 3:
        raise ValueError("a device sweep must be 2-D with at least 3 columns")
    row, col = (shape[1] * 4, 4) if strides is None else (int(strides[0]), int(strides[1]))
    if col != 4 or not 0 <= row < 1 << 32:
        raise ValueError("a device sweep needs unit column stride and a row stride that is not negative")
    return CloudIn(int(cai["data"][0]) or None, int(shape[0]), row)


class _Out:
    def __init__(self, cap):
        self.arr = np.empty((max(cap, 1), 4), np.float32)
        self.c = CloudOut(self.arr.ctypes.data, 0, cap)

    def get(self, count=None):
        return self.arr[:self.c.count if count is None else count].copy()


def _cloud_ref(a):
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 4)
    return CloudOut(a.ctypes.data if a.shape[0] else None, a.shape[0], a.shape[0]), a


class Engine:
    # scan_registration / chain_sweep accept a loam_cloud_in view as the raw sweep (rosbag.replay)
    takes_cloud_in = True

    def __init__(self, cfg=None, device=0, cap=None):
        self.cfg = cfg or default_config()
        self.h = ctypes.c_void_p()
        _check(lib().loam_create(ctypes.byref(self.h), ctypes.byref(self.cfg), device))
        self.cap = cap or int(self.cfg.max_points)
        # output storage reused by every call (the results are copied out of it)
        self._sr_outs = [_Out(self.cap) for _ in range(5)]
        self._od_outs = [_Out(self.cap) for _ in range(3)]

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            lib().loam_destroy(self.h)
            self.h = ctypes.c_void_p()

    def __del__(self):
        self.close()

    def stats(self):
        s = Stats()
        _check(lib().loam_get_stats(self.h, ctypes.byref(s)))
        return s.as_dict()

    def set_ring_table(self, bounds, rings):
        """loam_set_ring_table: the context's ring model becomes the table (bounds [n + 1] degrees,
        rings [n]; ring_table_from_elevations builds one), before the context's first sweep"""
        pb, pr, n, _keep = _ring_table_args(bounds, rings)
        _check(lib().loam_set_ring_table(self.h, n, pb, pr))

    def set_point_fields(self, ring=None, time=None, ring_map=None, fields=None):
        """loam_set_point_fields, before the context's first sweep: ring = (type, offset), time =
        None or (type, offset, scale, bias), ring_map = None or ints (-1 = drop); or a ready
        PointFields as `fields`.  Neither ring nor fields: back to the ring model."""
        if fields is None and ring is not None:
            fields = PointFields.of(ring, time, ring_map)
        _check(lib().loam_set_point_fields(self.h, ctypes.byref(fields) if fields is not None else None))

    # --- the node bodies
    def imu(self, stamp, quat_xyzw, lin_acc):
        """/imu/data (scanRegistration and laserMapping imuHandlers)"""
        q = (ctypes.c_double * 4)(*[float(v) for v in quat_xyzw])
        a = (ctypes.c_double * 3)(*[float(v) for v in lin_acc])
        _check(lib().loam_imu(self.h, stamp, q, a))

    def scan_registration(self, raw, stamp=0.0):
        ci, keep = _cloud_in(raw)
        outs = self._sr_outs
        f = Features(*[o.c for o in outs])
        rc = lib().loam_scan_registration(self.h, stamp, ci, ctypes.byref(f))
        if rc == LOAM_E_NOT_READY:
            return rc, None
        _check(rc)
        names = ["full", "sharp", "less_sharp", "flat", "less_flat"]
        res = {n: o.get(getattr(f, n).count) for n, o in zip(names, outs)}
        res["imu_trans"] = np.array(f.imu_trans[:], np.float32)
        return 0, res

    def odometry(self, feats, stamp=0.0):
        refs = [_cloud_ref(feats[n]) for n in ("full", "sharp", "less_sharp", "flat", "less_flat")]
        f = Features(*[r[0] for r in refs])
        if "imu_trans" in feats:
            f.imu_trans[:] = [float(v) for v in feats["imu_trans"]]
        pose = Pose6()
        outs = self._od_outs
        for o in outs:
            o.c.count = 0
        pub = ctypes.c_int(0)
        _check(lib().loam_odometry(self.h, stamp, ctypes.byref(f), ctypes.byref(pose), ctypes.byref(outs[0].c),
                                   ctypes.byref(outs[1].c), ctypes.byref(outs[2].c), ctypes.byref(pub)))
        return pub.value, pose.arr(), outs[0].get(), outs[1].get(), outs[2].get()

    def mapping(self, odom_sum, corner, surf, full, stamp=0.0):
        refs = [_cloud_ref(a) for a in (corner, surf, full)]
        aft, bef = Pose6(), Pose6()
        reg = _Out(max(int(np.asarray(full).shape[0]), 1))
        _check(lib().loam_mapping(self.h, stamp, ctypes.byref(Pose6.of(odom_sum)), ctypes.byref(refs[0][0]),
                                  ctypes.byref(refs[1][0]), ctypes.byref(refs[2][0]), ctypes.byref(aft),
                                  ctypes.byref(bef), ctypes.byref(reg.c)))
        return aft.arr(), bef.arr(), reg.get()

    def chain_sweep(self, raw, stamp=0.0, registered=False):
        """one sweep through the three node bodies with the intermediate topics kept on the device
        (loam_chain_sweep): (rc, published, od_sum, aft, bef, registered) -- aft / bef None when
        mapping did not run on this sweep, registered None unless requested"""
        ci, keep = _cloud_in(raw)
        out = ChainOut()
        # (the registered cloud has one point per input point: a CloudIn view carries its count)
        reg = _Out(max(int(ci.count), 1)) if registered else None
        if reg is not None:
            out.registered = reg.c
        rc = lib().loam_chain_sweep(self.h, stamp, ci, ctypes.byref(out))
        if rc == LOAM_E_NOT_READY:
            return rc, 0, None, None, None, None
        _check(rc)
        if not out.mapped:
            return 0, out.published, out.od_sum.arr(), None, None, None
        r = None
        if reg is not None:
            reg.c = out.registered
            r = reg.get()
        return 0, out.published, out.od_sum.arr(), out.aft.arr(), out.bef.arr(), r

    def mapping_surround(self, cap=1 << 16):
        """/laser_cloud_surround of the last mapping frame (laserMapping.cpp:1038-1058): an (n, 4)
        array on the frames the reference publishes it (1st, then every 5th), else None"""
        pub = ctypes.c_int(0)
        out = _Out(cap)
        rc = lib().loam_mapping_surround(self.h, ctypes.byref(out.c), ctypes.byref(pub))
        if rc == LOAM_E_CAPACITY:
            out = _Out(int(out.c.count))
            rc = lib().loam_mapping_surround(self.h, ctypes.byref(out.c), ctypes.byref(pub))
        _check(rc)
        return out.get() if pub.value else None

    # --- config 4
    @staticmethod
    def prepare_batch(prevs, curs):
        """the loam_cloud_in arrays of a batch (kept with the arrays they view), built once for
        repeated batch_feed calls"""
        n = len(prevs)
        keep = []
        a = (CloudIn * n)()
        b = (CloudIn * n)()
        for i in range(n):
            a[i], k1 = _cloud_in(prevs[i])
            b[i], k2 = _cloud_in(curs[i])
            keep += [k1, k2]
        return n, a, b, keep

    def batch_upload(self, prevs, curs):
        n, a, b, _keep = self.prepare_batch(prevs, curs)
        _check(lib().loam_batch_upload(self.h, n, a, b))
        self.n = n

    def batch_feed(self, prevs, curs=None):
        """the sweeps of the next batch_run (loam_batch_feed): (prevs, curs) lists, or a
        prepare_batch result as the only argument"""
        n, a, b, _keep = prevs if curs is None else self.prepare_batch(prevs, curs)
        _check(lib().loam_batch_feed(self.h, n, a, b))

    def batch_run(self):
        _check(lib().loam_batch_run(self.h))

    def sync(self):
        _check(lib().loam_batch_sync(self.h))

    def set_stream_priority(self, priority):
        """> 0 highest, 0 normal, < 0 lowest device stream priority for this context's streams"""
        _check(lib().loam_set_stream_priority(self.h, int(priority)))

    def set_tuning(self, **kv):
        """launch-shape choices by batch size (include/loam/loam.h loam_set_tuning), e.g.
        set_tuning(od_fused_max=0); every choice computes the same results"""
        for k, v in kv.items():
            _check(lib().loam_set_tuning(self.h, k.encode(), int(v)))

    def get_tuning(self, key):
        """the current value of a launch choice (include/loam/loam.h loam_get_tuning)"""
        v = ctypes.c_longlong(0)
        _check(lib().loam_get_tuning(self.h, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def set_profiling(self, on):
        _check(lib().loam_set_profiling(self.h, 1 if on else 0))

    def kernel_times(self):
        """{kernel: (total_ms, launches)} accumulated since profiling was enabled"""
        buf = ctypes.create_string_buffer(1 << 16)
        _check(lib().loam_get_kernel_times(self.h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, ms, n = line.split()
            out[name] = (float(ms), int(n))
        return out

    def batch_download(self):
        od = (Pose6 * self.n)()
        aft = (Pose6 * self.n)()
        st = Stats()
        _check(lib().loam_batch_download(self.h, od, aft, ctypes.byref(st)))
        return (np.array([p.arr() for p in od]), np.array([p.arr() for p in aft]), st.as_dict())

    def batch_lm_info(self):
        """per-problem L-M results of the last run: (odometry iterations, mapping iterations, the
        odometry's solved transform [n, 6])"""
        od = np.zeros(self.n, np.int32)
        mp = np.zeros(self.n, np.int32)
        tr = (Pose6 * self.n)()
        P = ctypes.POINTER(ctypes.c_int32)
        _check(lib().loam_batch_lm_info(self.h, od.ctypes.data_as(P), mp.ctypes.data_as(P), tr))
        return od, mp, np.array([p.arr() for p in tr])

    def batch_features(self, first=0, n=None, clouds=BATCH_CLOUDS):
        """the scan-registration clouds of problems [first, first + n) of the last batch_run
        (loam_batch_features): {name: (points [N, 4] float32, offsets [2n + 1] uint32)}, sweep
        j = 2 * (i - first) + (0: prev_i, 1: cur_i) at points[offsets[j]:offsets[j + 1]]"""
        n = max(getattr(self, "n", 0) - first, 0) if n is None else n
        for c in clouds:
            if c not in BATCH_CLOUDS:
                raise ValueError(f"unknown cloud {c!r}")
        if n < 0 or first < 0:
            raise ValueError("first and n must not be negative")
        bc = BatchClouds()
        offs = {c: np.zeros(2 * n + 1, np.uint32) for c in clouds}
        for c in clouds:
            getattr(bc, c).offset = offs[c].ctypes.data
        _check(lib().loam_batch_features(self.h, first, n, ctypes.byref(bc)))  # sizes only
        pts = {c: np.empty((int(getattr(bc, c).count), 4), np.float32) for c in clouds}
        for c in clouds:
            b = getattr(bc, c)
            b.pts, b.capacity = pts[c].ctypes.data, pts[c].shape[0]
        if clouds:
            _check(lib().loam_batch_features(self.h, first, n, ctypes.byref(bc)))
        return {c: (pts[c], offs[c]) for c in clouds}

    # --- the map
    def map_export(self):
        """the streaming context's cube map and mapping pose state (loam_map_export): a dict of
        corner / surf ([N, 4] float32, canonical order: cube index ascending, the store's order
        inside a cube), corner_offset / surf_offset ([MAP_CUBES + 1] uint32: cube c is
        points[offset[c]:offset[c + 1]]), center ([3] int32), surround_phase, aft, bef"""
        return self._map_export(lambda m: lib().loam_map_export(self.h, ctypes.byref(m)))

    @staticmethod
    def _map_export(call):
        m = Map()
        offs = [np.zeros(MAP_CUBES + 1, np.uint32) for _ in range(2)]
        m.corner.cube_offset, m.surf.cube_offset = offs[0].ctypes.data, offs[1].ctypes.data
        _check(call(m))  # sizes only
        pts = [np.empty((int(c.count), 4), np.float32) for c in (m.corner, m.surf)]
        for c, a in zip((m.corner, m.surf), pts):
            c.pts, c.capacity = a.ctypes.data, a.shape[0]
        _check(call(m))
        return {"corner": pts[0], "surf": pts[1], "corner_offset": offs[0], "surf_offset": offs[1],
                "center": np.array(m.center[:], np.int32), "surround_phase": int(m.surround_phase),
                "aft": m.aft.arr(), "bef": m.bef.arr()}

    @staticmethod
    def _map_in(corner, surf, center, surround_phase, aft, bef):
        """a loam_map over the caller's arrays (and the arrays, to be kept alive over the call)"""
        m = Map()
        keep = []
        for c, a in ((m.corner, corner), (m.surf, surf)):
            a = np.ascontiguousarray(a, np.float32).reshape(-1, 4)
            keep.append(a)
            c.pts, c.count, c.capacity = (a.ctypes.data if a.shape[0] else None), a.shape[0], a.shape[0]
        m.center[:] = [int(v) for v in center]
        m.surround_phase = int(surround_phase)
        m.aft = Pose6.of(np.zeros(6) if aft is None else aft)
        m.bef = Pose6.of(np.zeros(6) if bef is None else bef)
        return m, keep

    def map_import(self, corner, surf, center=(10, 5, 10), surround_phase=4, aft=None, bef=None):
        """replaces the context's map and mapping pose state (loam_map_import): corner / surf [N, 4]
        map-frame points in any order; returns the (corner, surf) counts of the points left out
        (outside the grid about `center`, or non-finite).  Resume: pass what map_export gave.
        Localize in a prior map with a fresh odometry: bef = None (zeros), aft = the pose guess."""
        m, keep = self._map_in(corner, surf, center, surround_phase, aft, bef)
        dropped = (ctypes.c_uint64 * 2)(0, 0)
        _check(lib().loam_map_import(self.h, ctypes.byref(m), dropped))
        return int(dropped[0]), int(dropped[1])

    # --- lanes: many sequences in lockstep
    def lanes_open(self, n, map_capacity):
        """n independent sequences in this context, map_capacity points of map store each
        (loam_lanes_open); every lane starts as a fresh Engine does"""
        _check(lib().loam_lanes_open(self.h, int(n), int(map_capacity)))
        self.n_lanes = int(n)

    def lanes_push(self, raws, stamp=0.0):
        """one step: raws[l] is lane l's next sweep ((n, >= 3) float array or a loam_cloud_in; an
        empty array retires the lane).  stamp: the sweeps' stamp, or a sequence of one stamp per
        lane.  Enqueues the step and returns (loam_lanes_push / loam_lanes_push_stamped)."""
        if len(raws) != self.n_lanes:
            raise ValueError("one sweep per lane")
        a = (CloudIn * self.n_lanes)()
        keep = []
        for l, r in enumerate(raws):
            a[l], k = _cloud_in(r)
            keep.append(k)
        if np.ndim(stamp) == 0:
            _check(lib().loam_lanes_push(self.h, float(stamp), a))
            return
        if len(stamp) != self.n_lanes:
            raise ValueError("one stamp per lane")
        t = (ctypes.c_double * self.n_lanes)(*[float(v) for v in stamp])
        _check(lib().loam_lanes_push_stamped(self.h, t, a))

    def lanes_push_device(self, raws, stamp=0.0, stream=None, wait=False, release=False):
        """lanes_push for sweeps that are already in device memory (loam_lanes_push_device): raws[l]
        is a CloudIn, a (ptr, count, stride_bytes) tuple or an object with __cuda_array_interface__
        (a torch tensor on this GPU: 2-D float32, at least 3 columns).  stream: the producer's HIP
        stream as an integer handle (torch.cuda.current_stream().cuda_stream); wait: the gather waits
        for the work enqueued on it so far; release: its later work waits for the gather and may
        overwrite the sweeps.  Without either the caller has synchronised and leaves the sweeps
        untouched until lanes_pull returns."""
        if len(raws) != self.n_lanes:
            raise ValueError("one sweep per lane")
        if (wait or release) and stream is None:
            raise ValueError("wait / release need the producer's stream")
        a = (CloudIn * self.n_lanes)()
        for l, r in enumerate(raws):
            a[l] = _cloud_in_device(r)
        if np.ndim(stamp) == 0:
            stamp = [stamp] * self.n_lanes
        if len(stamp) != self.n_lanes:
            raise ValueError("one stamp per lane")
        t = (ctypes.c_double * self.n_lanes)(*[float(v) for v in stamp])
        flags = (FEED_WAIT if wait else 0) | (FEED_RELEASE if release else 0)
        _check(lib().loam_lanes_push_device(self.h, t, a, ctypes.c_void_p(stream if stream is not None else 0), flags))

    def lanes_step_device(self, raws, stamp=0.0, stream=None, wait=False, release=False):
        """lanes_push_device followed by lanes_pull"""
        self.lanes_push_device(raws, stamp, stream, wait, release)
        return self.lanes_pull()

    def lanes_imu(self, lane, stamp, quat_xyzw, lin_acc):
        """/imu/data of one lane (loam_lanes_imu): loam_imu for that lane's sequence"""
        q = (ctypes.c_double * 4)(*[float(v) for v in quat_xyzw])
        a = (ctypes.c_double * 3)(*[float(v) for v in lin_acc])
        _check(lib().loam_lanes_imu(self.h, int(lane), stamp, q, a))

    def lanes_restart(self, lane):
        """lane `lane` becomes a fresh sequence (loam_lanes_restart).  Returns wait_steps: the number
        of coming steps on which the lane's sweep is not looked at (status LOAM_E_NOT_READY); the
        sequence's first sweep goes in on the step after them, the lane's init step.  With s =
        skip_frame_num and c the shared odometry frame counter it is (2 s - c) mod (s + 1)."""
        w = ctypes.c_uint32(0)
        _check(lib().loam_lanes_restart(self.h, int(lane), ctypes.byref(w)))
        return int(w.value)

    def lanes_imu_trans(self):
        """/imu_trans of every lane from the last pulled step (loam_lanes_imu_trans): an
        (n_lanes, 12) float32 array, zero rows for lanes without IMU"""
        out = np.zeros((self.n_lanes, 12), np.float32)
        _check(lib().loam_lanes_imu_trans(self.h, out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return out

    def lanes_pull(self):
        """waits for the pushed step (loam_lanes_pull): a dict of numpy arrays, one row per lane:
        status (LOAM_OK, LOAM_E_NOT_READY inside system_delay, or the lane's sticky failure code),
        published, mapped, od_iters, mp_iters, od_sum / aft / bef (n, 6), n_registered"""
        rec = np.zeros(self.n_lanes, _LANE_DTYPE)
        _check(lib().loam_lanes_pull(self.h, rec.ctypes.data_as(ctypes.POINTER(LaneOut))))
        return {k: rec[k].copy() for k in LANE_KEYS}

    def lanes_step(self, raws, stamp=0.0):
        """lanes_push followed by lanes_pull"""
        self.lanes_push(raws, stamp)
        return self.lanes_pull()

    def lanes_registered(self, lane):
        """/velodyne_cloud_registered of one lane from the last pulled step, which mapped
        (loam_lanes_registered): an (n, 4) array"""
        out = _Out(0)
        rc = lib().loam_lanes_registered(self.h, int(lane), ctypes.byref(out.c))
        if rc == LOAM_E_CAPACITY:
            out = _Out(int(out.c.count))
            rc = lib().loam_lanes_registered(self.h, int(lane), ctypes.byref(out.c))
        _check(rc)
        return out.get()

    def _lanes_list(self, lanes):
        """(n, the ctypes index array or None for every lane) of a lanes_clouds list"""
        if lanes is None:
            return self.n_lanes, None
        lanes = [int(l) for l in np.atleast_1d(lanes)]
        return len(lanes), (ctypes.c_uint32 * max(len(lanes), 1))(*lanes)

    def lanes_clouds(self, lanes=None, clouds=None):
        """the topic clouds of the last pulled step for the listed lanes (loam_lanes_clouds; lanes
        None = every lane, clouds None = all nine of LANE_CLOUDS): {name: [an (n, 4) float32 array
        per listed lane]}, an empty array where the lane's frame has no such cloud.  Valid until the
        next lanes_push; the sizes-only call first, then one call with room."""
        clouds = LANE_CLOUDS if clouds is None else tuple(clouds)
        for c in clouds:
            if c not in LANE_CLOUDS:
                raise ValueError(f"unknown cloud {c!r}")
        n, idx = self._lanes_list(lanes)
        lc = LanesCloudsOut()
        offs = {c: np.zeros(n + 1, np.uint32) for c in clouds}
        for c in clouds:
            getattr(lc, c).offset = offs[c].ctypes.data
        if clouds:
            _check(lib().loam_lanes_clouds(self.h, n, idx, ctypes.byref(lc)))  # sizes only
        pts = {c: np.empty((int(getattr(lc, c).count), 4), np.float32) for c in clouds}
        for c in clouds:
            b = getattr(lc, c)
            b.pts, b.capacity = pts[c].ctypes.data, pts[c].shape[0]
        if any(p.shape[0] for p in pts.values()):
            _check(lib().loam_lanes_clouds(self.h, n, idx, ctypes.byref(lc)))
        return {c: [pts[c][offs[c][i]:offs[c][i + 1]].copy() for i in range(n)] for c in clouds}

    def lanes_clouds_device(self, dst, lanes=None, stream=None):
        """lanes_clouds into device memory (loam_lanes_clouds_device): dst = {name: an object with
        __cuda_array_interface__ (a torch tensor on this GPU: float32, contiguous, 4 floats per point,
        16-byte aligned)}; the points are packed straight into it.  stream: the consumer's HIP stream as
        an integer handle: its later work waits for the pack and the call does not; None: the call
        waits.  Earlier work that still uses the buffers must have finished before the call (the pack
        waits for nothing of the caller's).  Returns {name: offsets [n + 1] uint32}: listed lane i's points of a cloud are rows
        offsets[i] .. offsets[i + 1] of its buffer."""
        n, idx = self._lanes_list(lanes)
        lc = LanesCloudsOut()
        offs = {}
        for c, buf in dst.items():
            if c not in LANE_CLOUDS:
                raise ValueError(f"unknown cloud {c!r}")
            cai = buf.__cuda_array_interface__
            if np.dtype(cai["typestr"]) != np.dtype(np.float32) or cai.get("strides") is not None:
                raise ValueError("a destination must be contiguous float32")
            offs[c] = np.zeros(n + 1, np.uint32)
            b = getattr(lc, c)
            b.pts, b.capacity = int(cai["data"][0]) or None, int(np.prod(cai["shape"])) // 4
            b.offset = offs[c].ctypes.data
        _check(lib().loam_lanes_clouds_device(self.h, n, idx, ctypes.byref(lc),
                                              ctypes.c_void_p(stream if stream is not None else 0)))
        return offs

    def lanes_map_export(self, lane):
        """one lane's cube map and mapping pose state (loam_lanes_map_export): the dict map_export
        returns, so save_map takes it"""
        return self._map_export(lambda m: lib().loam_lanes_map_export(self.h, int(lane), ctypes.byref(m)))

    def lanes_map_import(self, lanes, corner, surf, center=(10, 5, 10), surround_phase=4, aft=None, bef=None,
                         corner_offset=None, surf_offset=None):
        """one map into the listed lanes between two steps (loam_lanes_map_import): map_import's
        arguments, uploaded and sorted once and copied on the device into every lane of `lanes`
        (distinct indices).  aft: one pose for every lane, or an [n, 6] array of one pose guess per
        listed lane; None = zeros.  Returns the (corner, surf) counts of the points left out.
        load_map's dict can be splatted in: lanes_map_import(lanes, **load_map(path)); its cube
        offsets are not needed (the points are binned again)."""
        lanes = [int(l) for l in np.atleast_1d(lanes)]
        n = len(lanes)
        a = np.zeros(6, np.float32) if aft is None else np.ascontiguousarray(aft, np.float32)
        per_lane = a.ndim == 2
        if per_lane and a.shape != (n, 6):
            raise ValueError("aft: one pose, or one pose per listed lane ([n, 6])")
        m, keep = self._map_in(corner, surf, center, surround_phase, None if per_lane else a, bef)
        idx = (ctypes.c_uint32 * max(n, 1))(*lanes)
        poses = a.ctypes.data_as(ctypes.POINTER(Pose6)) if per_lane else None
        dropped = (ctypes.c_uint64 * 2)(0, 0)
        _check(lib().loam_lanes_map_import(self.h, n, idx, ctypes.byref(m), poses, dropped))
        return int(dropped[0]), int(dropped[1])

    def lanes_surround(self):
        """/laser_cloud_surround of every lane from the last pulled step (loam_lanes_surround): a
        list with one entry per lane, an (n, 4) float32 array where the lane's frame publishes the
        topic (its 1st mapping frame and every 5th after it) and None where it does not.  Valid
        until the next lanes_push; the sizes-only call first, then one call with room."""
        S = self.n_lanes
        off = np.zeros(S + 1, np.uint32)
        pub = np.zeros(S, np.int32)
        c = LanesCloud()
        c.offset, c.published = off.ctypes.data, pub.ctypes.data
        _check(lib().loam_lanes_surround(self.h, ctypes.byref(c)))  # sizes only
        pts = np.empty((int(c.count), 4), np.float32)
        if pts.shape[0]:
            c.pts, c.capacity = pts.ctypes.data, pts.shape[0]
            _check(lib().loam_lanes_surround(self.h, ctypes.byref(c)))
        return [pts[off[l]:off[l + 1]].copy() if pub[l] else None for l in range(S)]

    def lanes_open_shared(self, n, from_capacity):
        """n lanes that localize in this context's own map, which their steps only read
        (loam_lanes_open_shared): no lane holds a map; from_capacity = the map points one lane's
        frame may gather from its valid cubes.  map_import / mapping / chain_sweep on this Engine
        change the map between steps; lanes_set_pose gives a lane its pose in it."""
        _check(lib().loam_lanes_open_shared(self.h, int(n), int(from_capacity)))
        self.n_lanes = int(n)

    def lanes_set_pose(self, lanes, aft, bef=None):
        """Aft / Bef of the listed shared lanes between two steps (loam_lanes_set_pose): aft one pose
        or an [n, 6] array of one per listed lane, bef likewise (None = zeros).  At start or after
        a restart: bef = None, aft = the pose guess.  Re-seeding a running lane: bef = the lane's
        last od_sum, aft = the better pose."""
        lanes = [int(l) for l in np.atleast_1d(lanes)]
        n = len(lanes)
        P = ctypes.POINTER(Pose6)

        def poses(v):
            a = np.ascontiguousarray(v, np.float32)
            a = np.ascontiguousarray(np.broadcast_to(a, (n, 6))) if a.ndim == 1 else a
            if a.shape != (n, 6):
                raise ValueError("one pose, or one pose per listed lane ([n, 6])")
            return a
        a = poses(aft)
        b = None if bef is None else poses(bef)
        idx = (ctypes.c_uint32 * max(n, 1))(*lanes)
        _check(lib().loam_lanes_set_pose(self.h, n, idx, a.ctypes.data_as(P), None if b is None else b.ctypes.data_as(P)))

    def lanes_map_commit(self, lanes):
        """the listed shared lanes' last pulled mapping frames into this context's map in one call
        (loam_lanes_map_commit): per cube the map's content, then each listed lane's stack points in
        list order, the cubes of the lanes' valid sets downsampled once.  Returns a dict of
        loam_commit_result's fields (inserted / outside / map_points as (corner, surf) pairs, cubes).
        LoamError with LOAM_E_CAPACITY leaves the map as it was; only that error carries a `commit`
        attribute, whose map_points are the points that did not fit."""
        lanes = [int(l) for l in np.atleast_1d(lanes)]
        idx = (ctypes.c_uint32 * max(len(lanes), 1))(*lanes)
        r = CommitResult()
        rc = lib().loam_lanes_map_commit(self.h, len(lanes), idx, ctypes.byref(r))
        out = {"inserted": (int(r.inserted[0]), int(r.inserted[1])), "outside": (int(r.outside[0]), int(r.outside[1])),
               "map_points": (int(r.map_points[0]), int(r.map_points[1])), "cubes": int(r.cubes)}
        if rc != LOAM_OK:
            err = LoamError(rc, lib().loam_last_error().decode())
            if rc == LOAM_E_CAPACITY:
                err.commit = out
            raise err
        return out

    def lanes_localize_info(self):
        """every shared lane's mapping frame of the last pulled step as map_localize reports a
        candidate (loam_lanes_localize_info): a structured array of n_lanes records with
        LOCALIZE_KEYS' fields; status LOC_NONE (and zeros) where the lane ran no mapping frame"""
        rec = np.zeros(self.n_lanes, _LOC_DTYPE)
        _check(lib().loam_lanes_localize_info(self.h, rec.ctypes.data_as(ctypes.POINTER(LocalizeResult))))
        return rec

    def lanes_score(self, lanes, poses, max_dist=1.0):
        """pose guesses for the listed lanes' own last sweeps scored against the context's whole map
        in one call (loam_lanes_score): poses (n, k, 6), or (k, 6) used for every listed lane.
        Returns map_score's dict with arrays of shape (n, k): row [i, j] is what map_score gives
        lane lanes[i]'s corner_last / surf_last at poses[i, j].  n x k <= SCORE_MAX."""
        lanes = [int(l) for l in np.atleast_1d(lanes)]
        n = len(lanes)
        p = _lane_poses(n, poses)
        k = p.shape[1]
        idx = (ctypes.c_uint32 * max(n, 1))(*lanes)
        rec = np.empty(max(n * k, 1), _SCORE_DTYPE)
        _check(lib().loam_lanes_score(self.h, n, idx, float(max_dist), k, p.ctypes.data_as(ctypes.POINTER(Pose6)),
                                      rec.ctypes.data_as(ctypes.POINTER(ScoreResult))))
        return {key: rec[key][:n * k].reshape(n, k).copy() for key in SCORE_KEYS}

    def lanes_localize(self, lanes, aft, bef=None):
        """candidate poses for the listed lanes' own last sweeps refined against the context's map in
        one call (loam_lanes_localize): aft (n, k, 6), or (k, 6) used for every listed lane; bef the
        same shapes, or None = zeros.  Returns map_localize's dict with arrays of shape (n, k), and
        (n, k, 6) for aft: row [i, j] is what map_localize gives lane lanes[i]'s od_sum, corner_last
        and surf_last at (aft[i, j], bef[i, j]).  n x k <= LOCALIZE_MAX."""
        lanes = [int(l) for l in np.atleast_1d(lanes)]
        n = len(lanes)
        a = _lane_poses(n, aft)
        k = a.shape[1]
        P = ctypes.POINTER(Pose6)
        pb = None
        if bef is not None:
            b = _lane_poses(n, bef)
            if b.shape != a.shape:
                raise ValueError("aft and bef must hold the same number of candidates per lane")
            pb = b.ctypes.data_as(P)
        idx = (ctypes.c_uint32 * max(n, 1))(*lanes)
        rec = np.zeros(max(n * k, 1), _LOC_DTYPE)
        _check(lib().loam_lanes_localize(self.h, n, idx, k, a.ctypes.data_as(P), pb,
                                         rec.ctypes.data_as(ctypes.POINTER(LocalizeResult))))
        return {key: rec[key][:n * k].reshape((n, k) + rec[key].shape[1:]).copy() for key in LOCALIZE_KEYS}

    def lanes_relocalize(self, lanes, poses, od_sum, max_dist=1.0, refine=0):
        """re-seeds the listed shared lanes in the map: scores the guesses (lanes_score), takes each
        lane's best row by score_order and gives it to the lane with lanes_set_pose(aft = the chosen
        guess, bef = od_sum[lane]), od_sum being the last lanes_pull / lanes_step output's (n_lanes,
        6) array, so that only later odometry increments are applied on top.  Returns a dict: index
        (n,) the chosen rows, aft (n, 6) the chosen guesses, score (map_score's keys, (n,) each).
        refine = m >= 1 (m x n <= LOCALIZE_MAX): relocalize's chain per lane.  Each lane's best m
        guesses by score_order are refined with lanes_localize(aft = the guesses, bef =
        od_sum[lane]), the LOC_SOLVED refined poses are scored again (a row that was not solved
        keeps its coarse score), and the lane gets the refined aft of its best fine row.  index is
        then (n,) that row of `poses`, aft its refined pose, score its fine score, and the dict also
        holds localize (lanes_localize's result), coarse and fine (map_score's keys), each (n, m)
        in the lanes' coarse order, with rows (n, m) = their rows of `poses`."""
        lanes = [int(l) for l in np.atleast_1d(lanes)]
        n = len(lanes)
        p = _lane_poses(n, poses)
        od_sum = np.asarray(od_sum, np.float32)
        if od_sum.ndim != 2 or od_sum.shape != (self.n_lanes, 6):
            raise ValueError("od_sum: the (n_lanes, 6) array of the last pulled step")
        m = int(refine)
        if m < 0 or m * n > LOCALIZE_MAX:
            raise ValueError("refine x the listed lanes must be in [0, LOCALIZE_MAX]")
        score = self.lanes_score(lanes, p, max_dist)
        order = [score_order({key: v[i] for key, v in score.items()}) for i in range(n)]
        bef = np.ascontiguousarray(od_sum[lanes])
        ar = np.arange(n)
        if m == 0:
            index = np.array([o[0] for o in order], np.int64)
            aft = np.ascontiguousarray(p[ar, index])
            self.lanes_set_pose(lanes, aft, bef)
            return {"index": index, "aft": aft, "score": {key: v[ar, index] for key, v in score.items()}}
        m = min(m, p.shape[1])
        rows = np.stack([o[:m] for o in order])  # (n, m)
        guess = np.ascontiguousarray(p[ar[:, None], rows])
        loc = self.lanes_localize(lanes, guess, np.ascontiguousarray(np.broadcast_to(bef[:, None, :], guess.shape)))
        coarse = {key: v[ar[:, None], rows] for key, v in score.items()}
        fine = {key: v.copy() for key, v in coarse.items()}
        ok = loc["status"] == LOC_SOLVED
        if ok.any():  # (one call scores every row; the rows that were not solved keep their coarse score)
            s = self.lanes_score(lanes, loc["aft"], max_dist)
            for key in SCORE_KEYS:
                fine[key][ok] = s[key][ok]
        best = np.array([score_order({key: v[i] for key, v in fine.items()}, rows[i])[0] for i in range(n)], np.int64)
        aft = np.ascontiguousarray(loc["aft"][ar, best])
        self.lanes_set_pose(lanes, aft, bef)
        return {"index": rows[ar, best], "aft": aft, "score": {key: v[ar, best] for key, v in fine.items()},
                "rows": rows, "localize": loc, "coarse": coarse, "fine": fine}

    def lanes_close(self):
        _check(lib().loam_lanes_close(self.h))
        self.n_lanes = 0

    def map_localize(self, odom_sum, corner, surf, aft, bef=None):
        """n candidate poses of one sweep against the context's map, which is left untouched
        (loam_map_localize): aft / bef (n, 6) float32 (bef None = zeros).  Returns a dict of numpy
        arrays, one entry per candidate: aft (n, 6), the pose a mapping frame started from
        (bef[h], aft[h]) would leave, status (LOC_SOLVED / LOC_NO_LM / LOC_OFFGRID), iters,
        degenerate_steps, rows_last, rows_sum, stack_corner, stack_surf, map_corner, map_surf.
        Rank by status == LOC_SOLVED, then rows_last / (stack_corner + stack_surf)."""
        aft = np.ascontiguousarray(aft, np.float32).reshape(-1, 6)
        n = aft.shape[0]
        P = ctypes.POINTER(Pose6)
        pb = None
        if bef is not None:
            bef = np.ascontiguousarray(bef, np.float32).reshape(-1, 6)
            if bef.shape[0] != n:
                raise ValueError("aft and bef must hold the same number of candidates")
            pb = bef.ctypes.data_as(P)
        refs = [_cloud_ref(a) for a in (corner, surf)]
        out = (LocalizeResult * max(n, 1))()
        _check(lib().loam_map_localize(self.h, ctypes.byref(Pose6.of(odom_sum)), ctypes.byref(refs[0][0]),
                                       ctypes.byref(refs[1][0]), n, aft.ctypes.data_as(P), pb, out))
        rec = np.frombuffer(out, dtype=np.dtype([(k, np.float32, (6,)) if k == "aft" else
                                                 (k, np.int32 if k in ("status", "iters", "degenerate_steps") else np.uint32)
                                                 for k in LOCALIZE_KEYS]), count=n)
        return {k: rec[k].copy() for k in LOCALIZE_KEYS}

    def map_score(self, corner, surf, poses, max_dist=1.0):
        """poses (n, 6) float32 of one sweep scored against the context's whole map, which is left
        untouched (loam_map_score): a dict of numpy arrays, one entry per pose: corner_scored /
        surf_scored (the clouds' finite points), corner_in / surf_in (those whose nearest map point
        of the same kind is closer than max_dist <= 1 m), corner_cost / surf_cost (float64: the sum
        of the squared nearest distances, max_dist^2 for a point without such a neighbour).  A pose's
        entries do not depend on the other poses of the call.  Any number of poses: more than
        SCORE_MAX go in several calls."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        n = poses.shape[0]
        refs = [_cloud_ref(a) for a in (corner, surf)]
        rec = np.empty(n, _SCORE_DTYPE)
        for a in range(0, n, SCORE_MAX):
            m = min(SCORE_MAX, n - a)
            _check(lib().loam_map_score(self.h, ctypes.byref(refs[0][0]), ctypes.byref(refs[1][0]), float(max_dist), m,
                                        poses[a:a + m].ctypes.data_as(ctypes.POINTER(Pose6)),
                                        rec[a:a + m].ctypes.data_as(ctypes.POINTER(ScoreResult))))
        return {k: rec[k].copy() for k in SCORE_KEYS}

    def relocalize(self, corner, surf, poses, keep=64, max_dist=1.0):
        """where in the loaded map is this sweep: scores every pose guess (map_score), refines the
        best `keep` (<= LOCALIZE_MAX) with map_localize (odom_sum = zeros, bef = None, aft = the
        guess) and scores the refined poses of the LOC_SOLVED ones.  Returns a dict: index (the kept
        guesses' rows of `poses`), localize (map_localize's result for them), coarse (their first
        scores), fine (the scores of their refined aft; a guess that was not LOC_SOLVED keeps its
        coarse score), all ordered best first by the fine score: most corner_in + surf_in, then
        least corner_cost + surf_cost, then lowest index.  The kept guesses are chosen by the same key
        on the coarse scores."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 6)
        if not 1 <= keep <= LOCALIZE_MAX:
            raise ValueError("keep must be in [1, LOCALIZE_MAX]")
        coarse = self.map_score(corner, surf, poses, max_dist)
        idx = score_order(coarse)[:keep]
        loc = self.map_localize(np.zeros(6, np.float32), corner, surf, poses[idx])
        fine = {k: coarse[k][idx].copy() for k in SCORE_KEYS}
        ok = np.flatnonzero(loc["status"] == LOC_SOLVED)
        if ok.size:
            s = self.map_score(corner, surf, loc["aft"][ok], max_dist)
            for k in SCORE_KEYS:
                fine[k][ok] = s[k]
        o = score_order(fine, idx)
        return {"index": idx[o], "localize": {k: v[o] for k, v in loc.items()},
                "coarse": {k: coarse[k][idx][o] for k in SCORE_KEYS}, "fine": {k: v[o] for k, v in fine.items()}}


def _lane_poses(n, poses):
    """lanes_score's poses as a contiguous (n, k, 6) float32 array"""
    p = np.asarray(poses, np.float32)
    if p.ndim == 2 and p.shape[1:] == (6,):
        p = np.broadcast_to(p, (n,) + p.shape)
    if p.ndim != 3 or p.shape[0] != n or p.shape[1] == 0 or p.shape[2] != 6:
        raise ValueError("poses: (n, k, 6) with one block per listed lane, or (k, 6) for every lane")
    return np.ascontiguousarray(p)


def score_order(score, index=None):
    """the rows of a map_score result best first: most corner_in + surf_in, then least corner_cost +
    surf_cost, then lowest index (the row number, or the given one)"""
    n_in = score["corner_in"].astype(np.int64) + score["surf_in"]
    cost = score["corner_cost"] + score["surf_cost"]
    index = np.arange(n_in.shape[0]) if index is None else np.asarray(index)
    return np.lexsort((index, cost, -n_in))


def save_map(path, m):
    """a map_export dict as an .npz file (numpy only)"""
    np.savez(path, **{k: np.asarray(m[k]) for k in MAP_KEYS})


def load_map(path):
    """the dict save_map wrote; Engine.map_import(m["corner"], m["surf"], m["center"],
    m["surround_phase"], m["aft"], m["bef"]) resumes from it"""
    with np.load(path) as z:
        m = {k: z[k] for k in MAP_KEYS}
    m["surround_phase"] = int(m["surround_phase"])
    return m


def maintenance(odom_sum, bef, aft):
    out = Pose6()
    _check(lib().loam_maintenance(ctypes.byref(Pose6.of(odom_sum)), ctypes.byref(Pose6.of(bef)),
                                  ctypes.byref(Pose6.of(aft)), ctypes.byref(out)))
    return out.arr()


def msg_from_pose(kind, pose, bef=None, stamp=0.0):
    """pose (+ bef for MSG_AFT_MAPPED) -> (OdometryMsg, TfMsg) as the reference publishes them"""
    m, t = OdometryMsg(), TfMsg()
    b = ctypes.byref(Pose6.of(bef)) if bef is not None else None
    _check(lib().loam_msg_from_pose(kind, stamp, ctypes.byref(Pose6.of(pose)), b, ctypes.byref(m), ctypes.byref(t)))
    return m, t


def pose_from_msg(m):
    """OdometryMsg -> (pose, bef) as the receiving handlers read it"""
    p, b = Pose6(), Pose6()
    _check(lib().loam_pose_from_msg(ctypes.byref(m), ctypes.byref(p), ctypes.byref(b)))
    return p.arr(), b.arr()
