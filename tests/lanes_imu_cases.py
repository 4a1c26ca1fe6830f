"""Inputs of tests/test_gpu_lanes_imu.py (built without a GPU; tests/test_lanes_imu_cases.py checks
the conditions they must meet).

A feed is one lane's sequence: its sweeps, its sweep stamps and, per sweep, the /imu/data messages
delivered before that sweep (the messages up to the sweep's end, as tests/test_gpu_parity.py's
_stream_imu delivers them)."""
import math

import numpy as np

PERIOD = 0.1       # scanPeriod
QUE = 200          # imuQueLength
TILE = 2048        # points of a ring-sort tile (kSrThreads x kRingE)
DELAY = 2          # system_delay of every stream here
K = 12             # sweeps of a stream unless a case says otherwise


def schedule(imus, t0, n, first_k=0):
    """per sweep k, the messages with stamp <= t0 + 0.1 (k + 1) not delivered before; nothing is
    delivered before sweep first_k, which then gets everything due"""
    out, j = [], 0
    for k in range(n):
        due = []
        if k >= first_k:
            while j < len(imus) and imus[j][0] <= t0 + PERIOD * (k + 1):
                due.append(imus[j])
                j += 1
        out.append(due)
    return out


class Feed:
    def __init__(self, sweeps, t0, sched=None):
        self.sweeps = list(sweeps)
        self.t0 = t0
        self.stamps = [t0 + PERIOD * k for k in range(len(self.sweeps))]
        self.sched = sched if sched is not None else [[] for _ in self.sweeps]

    def without_imu(self):
        return Feed(self.sweeps, self.t0)

    @property
    def has_imu(self):
        return any(self.sched)


def max_backlog(feed, delay=DELAY):
    """an upper bound of the messages between a queue's consumed pointer and its last message, over
    the stream, for scanRegistration's queue and laserMapping's: scanRegistration's pointer ends a
    processed sweep at the first message later than the sweep's last point, which is no earlier
    than the last message before the sweep's start; laserMapping's pointer moves to the message
    after stamp + 0.1 on the mapping frames whose L-M runs, which are every second processed sweep
    from the fourth on (skip_frame_num 1; the first mapping frame has an empty map)."""
    stamps = [m[0] for due in feed.sched for m in due]
    delivered, sr_used, mp_used, worst = 0, 0, 0, 0
    for k, due in enumerate(feed.sched):
        delivered += len(due)
        worst = max(worst, delivered - sr_used, delivered - mp_used)
        if k < delay or delivered == 0:
            continue
        before = sum(1 for t in stamps[:delivered] if t < feed.stamps[k])
        sr_used = max(sr_used, before - 1)
        if k >= delay + 3 and (k - delay) % 2 == 1:
            mp_used = max(mp_used, before - 1)
    return worst


def crafted_head(sweep):
    """the sweep behind 3 NaN points and one finite point at 40 degrees elevation in the direction
    of the sweep's first point: the first finite point then fails the VLP-16 ring filter"""
    x, y = float(sweep[0, 0]), float(sweep[0, 1])
    head = np.full((4, sweep.shape[1]), np.nan, np.float32)
    head[3] = 0.0
    head[3, 0], head[3, 1], head[3, 2] = x, y, math.hypot(x, y) * math.tan(math.radians(40.0))
    return np.ascontiguousarray(np.vstack([head, sweep]))


def head_elevation(sweep):
    """the VLP-16 ring of the sweep's first finite point from its rounded elevation in degrees
    (src/scanRegistration.cpp:241-256); the ring filter keeps 0..15"""
    i = int(np.flatnonzero(np.all(np.isfinite(sweep[:, :3]), axis=1))[0])
    x, y, z = (float(v) for v in sweep[i, :3])
    a = math.degrees(math.atan(z / math.hypot(x, y)))
    r = int(a + (-0.5 if a < 0 else 0.5))
    return r if r > 0 else r + 15


NAN_TAIL = 2100


def nan_tail(sweep):
    tail = np.full((NAN_TAIL, sweep.shape[1]), np.nan, np.float32)
    return np.ascontiguousarray(np.vstack([sweep, tail]))


def trailing_nans(sweep):
    ok = np.all(np.isfinite(sweep[:, :3]), axis=1)
    return int(sweep.shape[0] - 1 - np.flatnonzero(ok)[-1])


def case_mixed(sg):
    """S = 3: an IMU lane, a lane without, and a lane on another clock (+100 s) with a 250 Hz IMU
    whose first message is withheld until after the fourth sweep"""
    a = Feed(sg.stream_sweeps(K, 1), 0.0)
    a.sched = schedule(sg.imu_stream(-0.5, PERIOD * K + 0.1, seed=1), 0.0, K)
    b = Feed(sg.stream_sweeps(K, 2), 0.0)
    t0 = 100.0
    c = Feed(sg.stream_sweeps(K, 3, t0=t0), t0)
    # (a 0.2 s lead before the first sweep the messages are delivered for)
    c.sched = schedule(sg.imu_stream(t0 + 4 * PERIOD - 0.2, t0 + PERIOD * K + 0.1, rate=250.0, seed=3), t0, K, first_k=4)
    return [a, b, c]


def case_tiles(sg):
    """S = 2, both with IMU: crafted heads (Start persists) / NaN tails longer than a tile (the last
    processed point sits in an earlier tile), and a lane whose messages end before its last sweep
    starts (that sweep takes every point's state from the last entry, without interpolation)"""
    a = Feed([crafted_head(s) for s in sg.stream_sweeps(K, 4)], 0.0)
    a.sched = schedule(sg.imu_stream(-0.5, PERIOD * K + 0.1, seed=4), 0.0, K)
    b = Feed([nan_tail(s) for s in sg.stream_sweeps(K, 5)], 0.0)
    b.sched = schedule(sg.imu_stream(-0.5, PERIOD * (K - 1) - 0.05, seed=5), 0.0, K)
    return [a, b]


BACK_SRC, BACK_DST, BACK_N = 12000, 2500, 5


def backward_block(sweep):
    """copies of BACK_N points from index BACK_SRC (before the sweep's half-way flip) inserted at
    BACK_DST, four tiles earlier: the forward-only queue pointer they leave is ahead of every
    point's own entry until BACK_SRC, through whole tiles, so those tiles' points depend on the
    pointer carried in from the tiles before (100 Hz messages: the entries are 10 ms apart, the
    two positions about 33 ms)"""
    return np.ascontiguousarray(np.vstack([sweep[:BACK_DST], sweep[BACK_SRC:BACK_SRC + BACK_N], sweep[BACK_DST:]]))


def case_backward(sg, n=8):
    """S = 2: a lane with IMU whose sweeps step backwards in time across tiles, and a plain lane"""
    a = Feed([backward_block(s) for s in sg.stream_sweeps(n, 6)], 0.0)
    a.sched = schedule(sg.imu_stream(-0.5, PERIOD * n + 0.1, seed=6), 0.0, n)
    return [a, Feed(sg.stream_sweeps(n, 2), 0.0)]


def case_wide(sg, n=7):
    """S = 65: lanes 0 and 64 with IMU, the others cycle two streams without"""
    a = Feed(sg.stream_sweeps(n, 1), 0.0)
    a.sched = schedule(sg.imu_stream(-0.5, PERIOD * n + 0.1, seed=1), 0.0, n)
    z = Feed(sg.stream_sweeps(n, 5), 0.0)
    z.sched = schedule(sg.imu_stream(-0.3, PERIOD * n + 0.1, seed=5), 0.0, n)
    p, q = Feed(sg.stream_sweeps(n, 2), 0.0), Feed(sg.stream_sweeps(n, 3), 0.0)
    return [a] + [(p, q)[l % 2] for l in range(63)] + [z]
