"""Lanes with IMU (loam_lanes_imu, loam_lanes_push_stamped, loam_lanes_imu_trans).

The specification: lane l behaves exactly as a fresh context that receives lane l's IMU messages
through loam_imu and lane l's sweeps through loam_chain_sweep at lane l's stamps, in the same
interleaving, bit for bit (poses, registered clouds, the exported map, /imu_trans), whatever the
other lanes do and whether or not they have an IMU.

  1. S = 3: an IMU lane, a lane without, a lane on another clock with a 250 Hz IMU that starts late
  2. lane 0 of it against the CPU oracle within POSE_TOL
  3. S = 2: a first finite point that fails the ring filter, NaN tails longer than a tile, a sweep
     behind all IMU stamps
  4. S = 65 with two IMU lanes (the plain lanes take the fused ring sort there, an IMU step must not)
  5. every LOAM_E_INVAL, each leaving the lanes as they were
  6. sweeps that step backwards in time across tiles: the forward-only queue pointer carried from
     tile to tile decides whole tiles' entries

/imu_trans of a context comes from a second context fed the same messages and the sweeps through
loam_scan_registration (loam_chain_sweep does not return it; the scan registration is the same call).
Inputs: tests/lanes_imu_cases.py (their conditions: tests/test_lanes_imu_cases.py)."""
import ctypes

import numpy as np
import pytest

import lanes_imu_cases as lc

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4  # as tests/test_gpu_parity.py
MAP_CAP = 1 << 17


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, msg):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _map_eq(a, b, msg):
    for k in ("corner", "surf", "aft", "bef"):
        _same(a[k], b[k], f"{msg} {k}")
    for k in ("corner_offset", "surf_offset", "center"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{msg} {k}")
    assert a["surround_phase"] == b["surround_phase"], msg


def _cfg(loam):
    return loam.default_config(system_delay=lc.DELAY)


@pytest.fixture(scope="module")
def context(loam):
    """a feed through a fresh context: loam_imu + chain_sweep; one record per sweep, the final map"""
    cache = {}

    def run(feed, n=None):
        key = (id(feed), n)
        if key in cache:
            return cache[key][1:]
        e, s = loam.Engine(_cfg(loam)), loam.Engine(_cfg(loam))
        recs = []
        for k, sw in enumerate(feed.sweeps[:n]):
            for m in feed.sched[k]:
                e.imu(*m)
                s.imu(*m)
            rc, pub, od, aft, bef, reg = e.chain_sweep(sw, stamp=feed.stamps[k], registered=True)
            rec = {"rc": rc, "pub": pub, "od_sum": od, "aft": aft, "bef": bef, "reg": reg}
            if aft is not None:
                rec["mp_iters"] = e.stats()["mp_iters"]
            src, f = s.scan_registration(sw, stamp=feed.stamps[k])
            assert src == rc
            rec["imu_trans"] = f["imu_trans"] if src == 0 else np.zeros(12, np.float32)
            recs.append(rec)
        out = (recs, e.map_export())
        e.close()
        s.close()
        cache[key] = (feed,) + out  # (the feed is kept: its id is the key)
        return out
    return run


def _lanes_run(loam, feeds, n=None, eng=None, stamped=True):
    """the feeds as lanes: per-step pull dicts, per-step {lane: registered cloud}, per-step
    /imu_trans, per-lane final maps"""
    S = len(feeds)
    n = len(feeds[0].sweeps) if n is None else n
    e = eng or loam.Engine(_cfg(loam))
    e.lanes_open(S, MAP_CAP)
    outs, regs, trans = [], [], []
    for k in range(n):
        for l, f in enumerate(feeds):
            for m in f.sched[k]:
                e.lanes_imu(l, *m)
        stamp = [f.stamps[k] for f in feeds] if stamped else feeds[0].stamps[k]
        o = e.lanes_step([f.sweeps[k] for f in feeds], stamp=stamp)
        outs.append(o)
        trans.append(e.lanes_imu_trans())
        regs.append({l: e.lanes_registered(l) for l in range(S) if o["mapped"][l] and o["status"][l] == 0} if S <= 8
                    else {})
    return e, outs, regs, trans


def _lane_eq_context(loam, outs, regs, trans, l, recs, msg, check_reg=True):
    assert len(outs) == len(recs)
    mapped = 0
    for k, (o, r) in enumerate(zip(outs, recs)):
        m = f"{msg} lane {l} step {k}"
        assert o["status"][l] == r["rc"], m
        _same(trans[k][l], r["imu_trans"], m + " imu_trans")
        if r["rc"] != 0:
            assert r["rc"] == loam.LOAM_E_NOT_READY and o["published"][l] == 0 and o["mapped"][l] == 0, m
            continue
        assert o["published"][l] == r["pub"], m
        assert o["mapped"][l] == (1 if r["aft"] is not None else 0), m
        _same(o["od_sum"][l], r["od_sum"], m + " od_sum")
        if r["aft"] is None:
            continue
        mapped += 1
        _same(o["aft"][l], r["aft"], m + " aft")
        _same(o["bef"][l], r["bef"], m + " bef")
        assert o["mp_iters"][l] == r["mp_iters"], m
        assert o["n_registered"][l] == r["reg"].shape[0] > 0, m
        if check_reg:
            _same(regs[k][l], r["reg"], m + " registered")
    return mapped


@pytest.fixture(scope="module")
def mixed(loam, sg):
    feeds = lc.case_mixed(sg)
    e, outs, regs, trans = _lanes_run(loam, feeds)
    maps = [e.lanes_map_export(l) for l in range(3)]
    e.close()
    return feeds, outs, regs, trans, maps


def test_mixed_lanes_equal_contexts(loam, mixed, context):
    feeds, outs, regs, trans, maps = mixed
    for l, f in enumerate(feeds):
        recs, cmap = context(f)
        assert _lane_eq_context(loam, outs, regs, trans, l, recs, "S=3") >= 4
        _map_eq(maps[l], cmap, f"lane {l} map")
    # the first mapping frame has an empty map: no L-M there (the mapping pointer stays)
    first = next(k for k, o in enumerate(outs) if o["mapped"][0])
    assert all(outs[first]["mp_iters"] == 0)
    assert any(o["mapped"][0] and o["mp_iters"][0] > 0 for o in outs)
    # the IMU took effect
    last = trans[-1]
    assert np.abs(last[0]).max() > 0 and np.abs(last[2]).max() > 0 and not last[1].any()
    assert not trans[3][2].any() and trans[4][2].any()  # lane 2's first message: before the fifth sweep
    plain, _ = context(feeds[0].without_imu())
    assert not np.array_equal(_bits(outs[-1]["aft"][0]), _bits(plain[-1]["aft"]))


def test_mixed_lane_equals_oracle(mixed, oc):
    feeds, outs, _, trans, _ = mixed
    f = feeds[0]
    o = oc.Oracle(oc.default_config(system_delay=lc.DELAY))
    poses = maps = 0
    for k, sw in enumerate(f.sweeps):
        for m in f.sched[k]:
            o.imu(*m)
        rc, ft = o.scan_registration(sw, stamp=f.stamps[k])
        assert (rc != 0) == (outs[k]["status"][0] != 0), k
        if rc != 0:
            continue
        np.testing.assert_array_equal(trans[k][0], ft["imu_trans"], err_msg=f"step {k} imu_trans")
        pub, pose, cl, sl, full = o.odometry(ft, stamp=f.stamps[k])
        assert outs[k]["published"][0] == pub, k
        if pub & 1:
            poses += 1
            assert np.max(np.abs(outs[k]["od_sum"][0] - pose)) <= POSE_TOL, k
        assert outs[k]["mapped"][0] == (1 if pub == 7 else 0), k
        if pub == 7:
            maps += 1
            aft, bef, _ = o.mapping(pose, cl, sl, full, stamp=f.stamps[k])
            assert np.max(np.abs(outs[k]["aft"][0] - aft)) <= POSE_TOL, k
            assert np.max(np.abs(outs[k]["bef"][0] - bef)) <= POSE_TOL, k
    assert poses >= 8 and maps >= 4


def test_tile_edges(loam, sg, context):
    feeds = lc.case_tiles(sg)
    e, outs, regs, trans = _lanes_run(loam, feeds)
    maps = [e.lanes_map_export(l) for l in range(2)]
    e.close()
    for l, f in enumerate(feeds):
        recs, cmap = context(f)
        assert _lane_eq_context(loam, outs, regs, trans, l, recs, "tiles") >= 4
        _map_eq(maps[l], cmap, f"lane {l} map")
        assert trans[-1][l].any()
    # lane 0's first processed sweep: its first finite point fails the ring filter, so Start is the
    # (zero) Start of before; later sweeps keep the Start of the sweep before
    assert not trans[lc.DELAY][0][:3].any()


def test_backward_steps_across_tiles(loam, sg, context):
    feeds = lc.case_backward(sg)
    e, outs, regs, trans = _lanes_run(loam, feeds)
    maps = [e.lanes_map_export(l) for l in range(2)]
    e.close()
    for l, f in enumerate(feeds):
        recs, cmap = context(f)
        assert _lane_eq_context(loam, outs, regs, trans, l, recs, "backward") >= 2
        _map_eq(maps[l], cmap, f"lane {l} map")
    assert trans[-1][0].any() and not trans[-1][1].any()


def test_wide_step_with_two_imu_lanes(loam, sg, context):
    feeds = lc.case_wide(sg)
    n = len(feeds[0].sweeps)
    e, outs, _, trans = _lanes_run(loam, feeds)
    imu_maps = {l: e.lanes_map_export(l) for l in (0, 1, 64)}
    e.close()
    for l in (0, 1, 64):
        recs, cmap = context(feeds[l])
        assert _lane_eq_context(loam, outs, None, trans, l, recs, "S=65", check_reg=False) == 2
        _map_eq(imu_maps[l], cmap, f"lane {l} map")
    assert trans[-1][0].any() and trans[-1][64].any() and not trans[-1][1:64].any()
    # the same feeds without a message: today's path (the fused ring sort), lane for lane
    bare = [f.without_imu() for f in feeds[:1]] + feeds[1:64] + [feeds[64].without_imu()]
    e, bouts, _, btrans = _lanes_run(loam, bare, stamped=False)
    bmaps = {l: e.lanes_map_export(l) for l in (0, 1, 64)}
    e.close()
    assert not np.any(btrans)
    for l in (0, 64):
        recs, cmap = context(bare[l])
        assert _lane_eq_context(loam, bouts, None, btrans, l, recs, "S=65 bare", check_reg=False) == 2
        _map_eq(bmaps[l], cmap, f"bare lane {l} map")
    # a lane without IMU computes the same in an IMU step (two-kernel ring sort) and a plain one
    for k in range(n):
        for key, v in outs[k].items():
            for l in range(1, 64):
                if v.dtype == np.float32:
                    _same(v[l], bouts[k][key][l], f"step {k} {key} lane {l}")
                else:
                    assert v[l] == bouts[k][key][l], (k, key, l)
    _map_eq(imu_maps[1], bmaps[1], "lane 1 map, IMU step against plain step")


def test_errors_leave_the_lanes_as_they_were(loam, sg, context):
    feeds = lc.case_mixed(sg)[:2]
    feeds[1] = lc.Feed(feeds[1].sweeps, 0.0, lc.schedule(sg.imu_stream(-0.5, lc.PERIOD * lc.K + 0.1, seed=2), 0.0, lc.K))
    n = 6
    L = loam.lib()
    inval = loam.LOAM_E_INVAL
    eng = loam.Engine(_cfg(loam))
    h = eng.h
    q = (ctypes.c_double * 4)(0, 0, 0, 1)
    a = (ctypes.c_double * 3)(0, 0, 9.81)
    out24 = (ctypes.c_float * 24)(*([7.0] * 24))
    raw2 = (loam.CloudIn * 2)()
    t2 = (ctypes.c_double * 2)(0.0, 0.0)
    # lanes not open
    assert L.loam_lanes_imu(h, 0, 0.0, q, a) == inval
    assert L.loam_lanes_push_stamped(h, t2, raw2) == inval
    assert L.loam_lanes_imu_trans(h, out24) == inval
    eng.lanes_open(2, MAP_CAP)
    assert L.loam_lanes_imu_trans(h, out24) == inval  # before the first pull
    assert list(out24) == [7.0] * 24
    outs, regs, trans = [], [], []
    for k in range(n):
        for l, f in enumerate(feeds):
            for m in f.sched[k]:
                eng.lanes_imu(l, *m)
        # refused calls before the step: null arguments, the lane index, a decreasing stamp on
        # lane 1, a null / non-finite stamp array
        assert L.loam_lanes_imu(h, 0, 1e9, None, a) == inval
        assert L.loam_lanes_imu(h, 0, 1e9, q, None) == inval
        assert L.loam_lanes_imu(h, 2, 1e9, q, a) == inval
        assert L.loam_lanes_imu(h, 1, feeds[1].sched[k][-1][0] - 1e-3, q, a) == inval
        assert b"non-decreasing" in L.loam_last_error()
        sw = [f.sweeps[k] for f in feeds]
        raws = (loam.CloudIn * 2)(*[loam.CloudIn(s.ctypes.data, s.shape[0], 16) for s in sw])
        assert L.loam_lanes_push_stamped(h, None, raws) == inval
        for bad in (float("nan"), float("inf")):
            assert L.loam_lanes_push_stamped(h, (ctypes.c_double * 2)(feeds[0].stamps[k], bad), raws) == inval
            assert L.loam_lanes_push(h, bad, raws) == inval
        eng.lanes_push(sw, stamp=[f.stamps[k] for f in feeds])
        # refused while the step is in flight
        assert L.loam_lanes_imu(h, 0, 1e9, q, a) == inval
        assert b"in flight" in L.loam_last_error()
        assert L.loam_lanes_imu_trans(h, out24) == inval
        assert L.loam_lanes_push_stamped(h, (ctypes.c_double * 2)(0.0, 0.0), raws) == inval
        o = eng.lanes_pull()
        outs.append(o)
        trans.append(eng.lanes_imu_trans())
        regs.append({l: eng.lanes_registered(l) for l in range(2) if o["mapped"][l]})
    # none of it disturbed either lane (the refused stamp on lane 1 included)
    for l, f in enumerate(feeds):
        recs, _ = context(f, n)
        assert _lane_eq_context(loam, outs, regs, trans, l, recs, "errors") >= 1
    # a failed lane takes no message; the other lane goes on as its context
    k = n
    for l, f in enumerate(feeds):
        for m in f.sched[k]:
            eng.lanes_imu(l, *m)
    o = eng.lanes_step([feeds[0].sweeps[k], np.zeros((0, 4), np.float32)], stamp=feeds[0].stamps[k])
    assert list(o["status"]) == [0, inval]
    assert L.loam_lanes_imu(h, 1, 1e9, q, a) == inval
    assert b"failed" in L.loam_last_error()
    t = eng.lanes_imu_trans()
    assert t[0].any() and not t[1].any()
    recs, _ = context(feeds[0], n + 1)
    _same(o["od_sum"][0], recs[k]["od_sum"], "lane 0 beside the failed lane")
    _same(t[0], recs[k]["imu_trans"], "lane 0 imu_trans beside the failed lane")
    eng.close()
