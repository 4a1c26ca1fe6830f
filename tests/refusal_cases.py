"""What the lanes entry points and the map services refuse before any kernel runs: the return code
and the whole loam_last_error() text, by entry point, lanes state and arguments.

Written by hand from the engine's source as it stood before the host engine was split into
engine.cpp / engine_batch.cpp / engine_map.cpp / engine_lanes.cpp; tests/test_gpu_refusals.py ran
against a library built from that source first (LOAM_HIP_LIB), unchanged, so the table records
that engine and not the one that composes the texts from shared helpers.

The context: the smallest configuration loam_create accepts with system_delay = 1, S = 3 lanes of
1024 points (own maps: lane_map_capacity, shared lanes: lane_from_capacity).  The states need no
kernel: with system_delay = 1 the first push is only counted, so the lanes are "in flight" with
nothing enqueued, and the pull that follows leaves them "pulled" with the odometry not initialised.

A row: (entry point, arguments, who, {kind: {state: expectation}}).  An expectation is the text
behind `who` of a LOAM_E_INVAL refusal, OK for a call the state accepts and that changes nothing
(it is made, and must return LOAM_OK), or ACCEPTS for a call the state accepts and that would
enqueue work or move the state (it is not made).  The arguments are plain values; the test builds
the C call from them.  Lists of lanes are `lanes`, and `n` where the count differs from the list."""
import math

OK, ACCEPTS = "ok", "accepts"
INVAL = -1  # LOAM_E_INVAL
S = 3
LANE_CAP = 1024
CLOSED, IDLE, IN_FLIGHT, PULLED = "closed", "idle", "in_flight", "pulled"
STATES = (CLOSED, IDLE, IN_FLIGHT, PULLED)
KINDS = ("own", "shared")
CONFIG = dict(n_rings=2, system_delay=1, max_points=64, od_max_iter=1, mp_max_iter=1, skip_frame_num=0, map_capacity=1024)

LOCALIZE_MAX, SCORE_MAX, LANES_MAX = 1024, 65536, 1024

NOT_OPEN = ": lanes are not open"
FLIES = ": a step is in flight (loam_lanes_pull first)"
NOT_PULLED = ": no step was pulled"
IS_OPEN = ": lanes are open (loam_lanes_close first)"
N_RANGE = ": n must be in [1, n_lanes]"
NO_LAST = ": no step was pulled on which the odometry was initialised (no Last clouds yet)"


def st(closed, idle, in_flight, pulled):
    return {CLOSED: closed, IDLE: idle, IN_FLIGHT: in_flight, PULLED: pulled}


def both(states):
    return {"own": states, "shared": states}


def every(text):
    return both(st(text, text, text, text))


ROWS = []


def row(call, args, expect, who=None):
    ROWS.append((call, args, who or call, expect))


# ---- loam_lanes_open(n_lanes, lane_map_capacity): open first, then the arguments in order
for a, closed in ((dict(n=S, cap=LANE_CAP), ACCEPTS),
                  (dict(n=0, cap=LANE_CAP), ": n_lanes must be in [1, LOAM_LANES_MAX]"),
                  (dict(n=LANES_MAX + 1, cap=LANE_CAP), ": n_lanes must be in [1, LOAM_LANES_MAX]"),
                  (dict(n=S, cap=1023), ": lane_map_capacity must be in [1024, 2^28] points"),
                  (dict(n=S, cap=(1 << 28) + 1), ": lane_map_capacity must be in [1024, 2^28] points"),
                  (dict(n=8, cap=1 << 28), ": n_lanes x lane_map_capacity reaches 2^31 points")):
    row("loam_lanes_open", a, both(st(closed, IS_OPEN, IS_OPEN, IS_OPEN)))

# ---- loam_lanes_open_shared(n_lanes, lane_from_capacity)
for a, closed in ((dict(n=S, cap=LANE_CAP), ACCEPTS),
                  (dict(n=0, cap=LANE_CAP), ": n_lanes must be in [1, LOAM_LANES_MAX]"),
                  (dict(n=LANES_MAX + 1, cap=LANE_CAP), ": n_lanes must be in [1, LOAM_LANES_MAX]"),
                  (dict(n=S, cap=1023), ": lane_from_capacity must be in [1024, 2^28] points"),
                  (dict(n=S, cap=(1 << 28) + 1), ": lane_from_capacity must be in [1024, 2^28] points"),
                  (dict(n=8, cap=1 << 28), ": n_lanes x lane_from_capacity reaches 2^31 points")):
    row("loam_lanes_open_shared", a, both(st(closed, IS_OPEN, IS_OPEN, IS_OPEN)))

# ---- loam_lanes_close
row("loam_lanes_close", {}, both(st(NOT_OPEN, ACCEPTS, ACCEPTS, ACCEPTS)))

# ---- the lane lists the calls below share
LISTS = (("valid", dict(lanes=[0, 2])),
         ("n0", dict(lanes=[0, 2], n=0)),
         ("n_over", dict(lanes=[0, 1, 2, 0], n=S + 1)),
         ("range", dict(lanes=[0, S])),
         ("twice", dict(lanes=[1, 1])))

# ---- loam_lanes_set_pose: open, shared lanes only, idle, n, the list
OWN_SET_POSE = ": the lanes have their own maps (loam_lanes_open); use loam_lanes_map_import"
for name, a in LISTS:
    idle = {"valid": ACCEPTS, "n0": N_RANGE, "n_over": N_RANGE, "range": ": lane[1] = 3 is out of range",
            "twice": ": lane[1] = 1 is listed twice"}[name]
    row("loam_lanes_set_pose", a, {"own": st(NOT_OPEN, OWN_SET_POSE, OWN_SET_POSE, OWN_SET_POSE),
                                   "shared": st(NOT_OPEN, idle, FLIES, idle)})

# ---- loam_lanes_localize_info: open, shared lanes only, idle, pulled
OWN_INFO = ": the lanes have their own maps (loam_lanes_open)"
row("loam_lanes_localize_info", {}, {"own": st(NOT_OPEN, OWN_INFO, OWN_INFO, OWN_INFO),
                                     "shared": st(NOT_OPEN, NOT_PULLED, FLIES, OK)})

# ---- loam_lanes_map_commit and its hook loam_dev_lanes_commit_input: open, shared lanes only, idle,
# pulled, n, the list; a lane pulled inside system_delay ran no mapping frame
OWN_COMMIT = ": the lanes have their own maps (loam_lanes_open), which they write themselves"
for name, a in LISTS:
    pulled = {"valid": ": lane[0] = 0 ran no mapping frame on the last pulled step", "n0": N_RANGE, "n_over": N_RANGE,
              "range": ": lane[0] = 0 ran no mapping frame on the last pulled step",  # (lane[0] is judged first)
              "twice": ": lane[0] = 1 ran no mapping frame on the last pulled step"}[name]
    row("loam_lanes_map_commit", a, {"own": st(NOT_OPEN, OWN_COMMIT, OWN_COMMIT, OWN_COMMIT),
                                     "shared": st(NOT_OPEN, NOT_PULLED, FLIES, pulled)})
for lane, pulled in ((0, ": lane[0] = 0 ran no mapping frame on the last pulled step"),
                     (S, ": lane[0] = 3 is out of range")):
    row("loam_dev_lanes_commit_input", dict(lane=lane), {"own": st(NOT_OPEN, OWN_COMMIT, OWN_COMMIT, OWN_COMMIT),
                                                         "shared": st(NOT_OPEN, NOT_PULLED, FLIES, pulled)})

# ---- loam_lanes_score / loam_lanes_localize: open, idle, a pulled step with Last clouds, and only
# then n, k, n x k, max_dist and the list: none of the four states has Last clouds, so every
# argument meets the state's refusal
ROWS_ARGS = [dict(a, k=2) for _, a in LISTS] + [dict(lanes=[0, 2], k=0)]
for a in ROWS_ARGS + [dict(lanes=[0, 2], k=SCORE_MAX // 2 + 1)]:
    for max_dist in (1.0, 0.0, 1.5, math.nan):
        row("loam_lanes_score", dict(a, max_dist=max_dist), both(st(NOT_OPEN, NO_LAST, FLIES, NO_LAST)))
for a in ROWS_ARGS + [dict(lanes=[0, 2], k=LOCALIZE_MAX // 2 + 1)]:
    row("loam_lanes_localize", a, both(st(NOT_OPEN, NO_LAST, FLIES, NO_LAST)))

# ---- the pushes: open, idle, finite stamps (loam_lanes_push_stamped speaks as loam_lanes_push);
# loam_lanes_push_device looks at its flag bits before the lanes
BAD_STAMP = ": a sweep stamp is not finite"
row("loam_lanes_push", dict(stamp=0.0), both(st(NOT_OPEN, ACCEPTS, FLIES, ACCEPTS)))
row("loam_lanes_push", dict(stamp=math.nan), both(st(NOT_OPEN, BAD_STAMP, FLIES, BAD_STAMP)))
row("loam_lanes_push_stamped", dict(stamps=[0.0, 0.0, 0.0]), both(st(NOT_OPEN, ACCEPTS, FLIES, ACCEPTS)), who="loam_lanes_push")
row("loam_lanes_push_stamped", dict(stamps=[0.0, 0.0, math.inf]), both(st(NOT_OPEN, BAD_STAMP, FLIES, BAD_STAMP)),
    who="loam_lanes_push")
row("loam_lanes_push_device", dict(stamps=[0.0, 0.0, 0.0], flags=3), both(st(NOT_OPEN, ACCEPTS, FLIES, ACCEPTS)))
row("loam_lanes_push_device", dict(stamps=[0.0, -math.inf, 0.0], flags=0), both(st(NOT_OPEN, BAD_STAMP, FLIES, BAD_STAMP)))
for flags in (4, 0x80000001):
    row("loam_lanes_push_device", dict(stamps=[0.0, 0.0, 0.0], flags=flags), every(": unknown flag bits"))

# ---- loam_lanes_imu: open, the lane, idle, the lane's stamps (NaN is not "non-decreasing")
IMU_RANGE = ": lane index out of range"
row("loam_lanes_imu", dict(lane=1, stamp=1.0), both(st(NOT_OPEN, ACCEPTS, FLIES, ACCEPTS)))
row("loam_lanes_imu", dict(lane=S, stamp=1.0), both(st(NOT_OPEN, IMU_RANGE, IMU_RANGE, IMU_RANGE)))
row("loam_lanes_imu", dict(lane=1, stamp=math.nan),
    both(st(NOT_OPEN, ": IMU stamps of a lane must be non-decreasing", FLIES, ": IMU stamps of a lane must be non-decreasing")))

# ---- loam_lanes_restart: open, the lane, idle
row("loam_lanes_restart", dict(lane=1), both(st(NOT_OPEN, ACCEPTS, FLIES, ACCEPTS)))
row("loam_lanes_restart", dict(lane=S), both(st(NOT_OPEN, IMU_RANGE, IMU_RANGE, IMU_RANGE)))

# ---- loam_lanes_imu_trans, loam_lanes_pull
row("loam_lanes_imu_trans", {}, both(st(NOT_OPEN, NOT_PULLED, FLIES, OK)))
row("loam_lanes_pull", {}, both(st(NOT_OPEN, ": no step was pushed", ACCEPTS, ": no step was pushed")))

# ---- loam_lanes_registered: open, the lane, a pulled step that mapped
NO_REG = ": the last pulled step did not map (or a step is in flight)"
row("loam_lanes_registered", dict(lane=1), both(st(NOT_OPEN, NO_REG, NO_REG, NO_REG)))
row("loam_lanes_registered", dict(lane=S), both(st(NOT_OPEN, IMU_RANGE, IMU_RANGE, IMU_RANGE)))

# ---- loam_lanes_clouds / loam_lanes_clouds_device (no cloud asked for: nothing to launch): open,
# idle, n, lane == NULL, the list
for call in ("loam_lanes_clouds", "loam_lanes_clouds_device"):
    for name, a in LISTS + (("all", dict(lanes=None, n=S)), ("null_n", dict(lanes=None, n=2))):
        idle = {"valid": OK, "all": OK, "n0": N_RANGE, "n_over": N_RANGE,
                "null_n": ": lane == NULL lists every lane: n must be n_lanes",
                "range": ": lane[1] = 3 is out of range", "twice": ": lane[1] = 1 is listed twice"}[name]
        row(call, a, both(st(NOT_OPEN, idle, FLIES, idle)))

# ---- loam_lanes_map_export: open, own maps only, the lane, idle
SHARED_EXPORT = ": shared lanes have no lane map (loam_map_export gives the context's)"
row("loam_lanes_map_export", dict(lane=1), {"own": st(NOT_OPEN, ACCEPTS, FLIES, ACCEPTS),
                                            "shared": st(NOT_OPEN, SHARED_EXPORT, SHARED_EXPORT, SHARED_EXPORT)})
row("loam_lanes_map_export", dict(lane=S), {"own": st(NOT_OPEN, IMU_RANGE, IMU_RANGE, IMU_RANGE),
                                            "shared": st(NOT_OPEN, SHARED_EXPORT, SHARED_EXPORT, SHARED_EXPORT)})

# ---- loam_lanes_map_import: open, own maps only, idle, n, the list (in its own words), the map
SHARED_IMPORT = (": shared lanes have no lane map (loam_map_import changes the context's, "
                 "loam_lanes_set_pose a lane's poses)")
for name, a in LISTS + (("phase", dict(lanes=[0, 2], surround_phase=5)), ("null_pts", dict(lanes=[0, 2], null_pts=True)),
                        ("center", dict(lanes=[0, 2], center=(10, (1 << 24) + 1, 10)))):
    idle = {"valid": ACCEPTS, "n0": N_RANGE, "n_over": N_RANGE, "range": ": lane[1] is out of range",
            "twice": ": lane[1] = 1 is listed twice", "phase": ": surround_phase must be 0..4",
            "null_pts": ": a cloud's pts is null", "center": ": a center component is beyond 2^24"}[name]
    row("loam_lanes_map_import", a, {"own": st(NOT_OPEN, idle, FLIES, idle),
                                     "shared": st(NOT_OPEN, SHARED_IMPORT, SHARED_IMPORT, SHARED_IMPORT)})

# ---- loam_lanes_surround: open, own maps only, idle; no lane is due: nothing to launch
SHARED_SURROUND = ": shared lanes have no lane map (loam_mapping_surround gives the context's)"
row("loam_lanes_surround", {}, {"own": st(NOT_OPEN, OK, FLIES, OK),
                                "shared": st(NOT_OPEN, SHARED_SURROUND, SHARED_SURROUND, SHARED_SURROUND)})


def expand(kind, state):
    """the calls of a (kind, state): (entry point, arguments, LOAM_OK or LOAM_E_INVAL, whole message or None)"""
    out = []
    for call, args, who, expect in ROWS:
        e = expect[kind][state]
        if e == ACCEPTS:
            continue
        out.append((call, args, 0, None) if e == OK else (call, args, INVAL, who + e))
    return out


# ---- loam_map_localize / loam_map_score on a context without lanes: the argument refusals, in the
# order the calls make them (counts are of CONFIG's max_points = 64)
MAP_ROWS = [
    ("loam_map_localize", dict(n=0), "loam_map_localize: n must be in [1, LOAM_LOCALIZE_MAX]"),
    ("loam_map_localize", dict(n=LOCALIZE_MAX + 1), "loam_map_localize: n must be in [1, LOAM_LOCALIZE_MAX]"),
    ("loam_map_localize", dict(n=0, corner_null=True), "loam_map_localize: n must be in [1, LOAM_LOCALIZE_MAX]"),
    ("loam_map_localize", dict(n=1, corner_null=True), "loam_map_localize: a cloud's pts is null"),
    ("loam_map_localize", dict(n=1, surf_null=True), "loam_map_localize: a cloud's pts is null"),
    ("loam_map_localize", dict(n=1, corner=65),
     "loam_map_localize: a cloud exceeds max_points (corner_last: 120 points per ring)"),
    ("loam_map_localize", dict(n=1, surf=65),
     "loam_map_localize: a cloud exceeds max_points (corner_last: 120 points per ring)"),
    ("loam_map_score", dict(n=0), "loam_map_score: n must be in [1, LOAM_SCORE_MAX]"),
    ("loam_map_score", dict(n=SCORE_MAX + 1), "loam_map_score: n must be in [1, LOAM_SCORE_MAX]"),
    ("loam_map_score", dict(n=0, max_dist=0.0), "loam_map_score: n must be in [1, LOAM_SCORE_MAX]"),
    ("loam_map_score", dict(n=1, max_dist=0.0), "loam_map_score: max_dist must be in (0, 1] (the map index has 1 m cells)"),
    ("loam_map_score", dict(n=1, max_dist=1.5), "loam_map_score: max_dist must be in (0, 1] (the map index has 1 m cells)"),
    ("loam_map_score", dict(n=1, max_dist=math.nan),
     "loam_map_score: max_dist must be in (0, 1] (the map index has 1 m cells)"),
    ("loam_map_score", dict(n=1, max_dist=-1.0, corner_null=True),
     "loam_map_score: max_dist must be in (0, 1] (the map index has 1 m cells)"),
    ("loam_map_score", dict(n=1, corner_null=True), "loam_map_score: a cloud's pts is null"),
    ("loam_map_score", dict(n=1, surf_null=True), "loam_map_score: a cloud's pts is null"),
    ("loam_map_score", dict(n=1, corner=65), "loam_map_score: a cloud exceeds max_points"),
    ("loam_map_score", dict(n=1, surf=65), "loam_map_score: a cloud exceeds max_points"),
]
