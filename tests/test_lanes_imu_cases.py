"""The conditions the inputs of tests/test_gpu_lanes_imu.py must meet (no GPU): no message schedule
laps an IMU queue (200 or more messages between a lane's consumed pointer and its last message are
outside loam_imu's contract), the crafted first point fails the VLP-16 ring filter, the NaN tails
are longer than a ring-sort tile, and the schedules do what the cases say."""
import numpy as np

import lanes_imu_cases as lc


def _feeds(sg):
    return {"mixed": lc.case_mixed(sg), "tiles": lc.case_tiles(sg), "backward": lc.case_backward(sg), "wide": [lc.case_wide(sg)[l] for l in (0, 1, 2, 64)]}


def test_no_schedule_laps_a_queue(sg):
    for name, feeds in _feeds(sg).items():
        for l, f in enumerate(feeds):
            assert lc.max_backlog(f) < lc.QUE, (name, l)
            stamps = [m[0] for due in f.sched for m in due]
            assert stamps == sorted(stamps), (name, l)


def test_backlog_bound_sees_a_lapped_queue(sg):
    f = lc.Feed(sg.stream_sweeps(4, 1), 0.0)
    f.sched = lc.schedule(sg.imu_stream(-1.0, 0.5, rate=250.0, seed=1), 0.0, 4)
    assert lc.max_backlog(f) >= lc.QUE


def test_mixed_case_schedules(sg):
    a, b, c = lc.case_mixed(sg)
    assert a.has_imu and not b.has_imu and c.has_imu
    assert len(a.sweeps) == len(b.sweeps) == len(c.sweeps) == lc.K == 12
    # lane 2: nothing before the fifth sweep, another clock, and more messages than the queue holds
    assert [len(d) for d in c.sched[:4]] == [0, 0, 0, 0] and len(c.sched[4]) > 0
    assert sum(len(d) for d in c.sched) > lc.QUE
    assert c.stamps[0] == 100.0 and a.stamps[0] == 0.0
    assert all(len(d) > 0 for d in a.sched)
    assert not np.array_equal(a.sweeps[0], c.sweeps[0])


def test_tile_case_inputs(sg):
    a, b = lc.case_tiles(sg)
    for s in a.sweeps:
        assert np.all(np.isnan(s[:3, :3])) and np.all(np.isfinite(s[3, :3]))
        assert not 0 <= lc.head_elevation(s) <= 15
        assert s.shape[0] > 7 * lc.TILE and s.shape[0] % lc.TILE != 0
    plain = sg.stream_sweeps(1, 4)[0]
    assert 0 <= lc.head_elevation(plain) <= 15
    for s in b.sweeps:
        assert lc.trailing_nans(s) == lc.NAN_TAIL > lc.TILE
        # the last finite point is not in the last tile
        assert (s.shape[0] - 1) // lc.TILE > (s.shape[0] - 1 - lc.NAN_TAIL) // lc.TILE
    # lane b's messages all precede its last sweep's start, and not the sweep's before
    last = max(m[0] for due in b.sched for m in due)
    assert b.stamps[-2] < last < b.stamps[-1]
    assert len(b.sched[-1]) == 0


def test_backward_case_inputs(sg):
    a, b = lc.case_backward(sg)
    assert a.has_imu and not b.has_imu
    plain = sg.stream_sweeps(len(a.sweeps), 6)
    for s, p in zip(a.sweeps, plain):
        assert s.shape[0] == p.shape[0] + lc.BACK_N
        np.testing.assert_array_equal(s[lc.BACK_DST:lc.BACK_DST + lc.BACK_N], p[lc.BACK_SRC:lc.BACK_SRC + lc.BACK_N])
        # whole tiles lie between the two positions, and the block comes from before the half-way flip
        assert lc.BACK_SRC // lc.TILE - lc.BACK_DST // lc.TILE >= 3
        assert lc.BACK_SRC + lc.BACK_N < p.shape[0] // 2 - 1000
        az = np.unwrap(-np.arctan2(p[:, 1], p[:, 0]))  # the sweep's orientation, increasing with time
        dt = (az[lc.BACK_SRC] - az[lc.BACK_DST]) / (az[-1] - az[0]) * lc.PERIOD
        assert dt > 0.02  # two 100 Hz entries and more


def test_wide_case_layout(sg):
    feeds = lc.case_wide(sg)
    assert len(feeds) == 65 and len(feeds[0].sweeps) == 7
    assert [l for l, f in enumerate(feeds) if f.has_imu] == [0, 64]
    assert feeds[1] is feeds[3] and feeds[2] is feeds[4] and feeds[1] is not feeds[2]
