"""loam_lanes_surround: /laser_cloud_surround for every lane in one call.

The specification: for a due lane the cloud is, bit for bit and in point order, what
loam_mapping_surround returns on the context that lane equals; a lane that is not due publishes
nothing; the call changes nothing in any lane.  Every yardstick cloud comes from a streaming
context (loam_chain_sweep + loam_mapping_surround), never from a second lanes run.

  1. S = 3 against three contexts, step by step; the run's poses, registered clouds and maps equal
     those of a run that never called lanes_surround
  2. lanes due on different steps (imports with surround_phase 2 and 4), one segment beyond the
     largest LDS tier
  3. restart, failure, retirement
  4. the sizes-only query and the LOAM_E_CAPACITY protocol
  5. protocol: closed lanes, a step in flight, nothing due, an import into a due lane
  6. S = 65: the 2048-point first tier, one lane fed a decimated sweep that stays below it

Streams: VLP-16 synthetic loops (synthgen.stream_sweeps), system_delay = 0, skip_frame_num = 1.  A
context with system_delay = 0 still does not look at its first sweep, so sweep 0 is not ready,
sweep 1 is the odometry's init frame and sweeps 2, 4, ..., 12 map: 13 sweeps hold the 1st mapping
frame (sweep 2) and the 5th after it (sweep 12), the two frames that publish."""
import ctypes

import numpy as np
import pytest

from test_gpu_lanes_restart import _map_eq, _same, _step_eq
from test_gpu_map import _surround_input

pytestmark = pytest.mark.gpu

MAP_CAP = 1 << 17
N_SWEEPS = 13
TIER_SMALL, TIER_LDS = 2048, 12288  # the VoxelGrid cascade's LDS tiers (csrc/vg.hip)


def _cfg(loam):
    return loam.default_config(system_delay=0, skip_frame_num=1)


@pytest.fixture(scope="module")
def sweeps(sg):
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = sg.stream_sweeps(N_SWEEPS, seed)
        return cache[seed]
    return get


@pytest.fixture(scope="module")
def ctx(loam):
    """a fresh context over a list of sweeps (chain_sweep), with map_import calls in front of the
    sweeps `imports` names ({k: keywords, or a function of the context's export at that point}).
    One record per sweep, with "sur": mapping_surround() straight after a sweep that mapped (None
    where it does not publish, and after a sweep that did not map), and the final map"""
    cache = {}

    def run(key, seq, imports=None):
        key = (key, len(seq))
        if key in cache:
            return cache[key]
        e = loam.Engine(_cfg(loam))
        recs = []
        for k, sw in enumerate(seq):
            if imports and k in imports:
                kw = imports[k]
                e.map_import(**(kw(e.map_export()) if callable(kw) else kw))
            rc, pub, od, aft, bef, reg = e.chain_sweep(sw, stamp=0.1 * k, registered=True)
            rec = {"rc": rc, "pub": pub, "od_sum": od, "aft": aft, "bef": bef, "reg": reg, "sur": None}
            if rc == 0 and aft is None:
                rec["od_iters"] = e.stats()["od_iters"]
            if aft is not None:
                rec["mp_iters"] = e.stats()["mp_iters"]
                rec["sur"] = e.mapping_surround()
            recs.append(rec)
        cache[key] = (recs, e.map_export())
        e.close()
        return cache[key]
    return run


def _sur_eq(sur, l, rec, msg):
    """lane l of lanes_surround()'s list against a context's record: None exactly where the context
    publishes nothing, else the same bits in the same order"""
    assert (sur[l] is None) == (rec["sur"] is None), msg
    if rec["sur"] is not None:
        assert sur[l].dtype == np.float32 and sur[l].shape[0] > 0, msg
        _same(sur[l], rec["sur"], msg + " surround")


def _kw(m, **over):
    kw = {k: m[k] for k in ("corner", "surf", "center", "surround_phase", "aft", "bef")}
    kw.update(over)
    return kw


def _run(loam, feeds, surround=True, before=None, lanes=None):
    """feeds[k][l]: lane l's sweep of step k; before(k, engine, outs) runs in front of step k.
    Returns per step: the pull, {lane: registered}, lanes_surround() (None when not called); and
    the final maps of the live lanes"""
    S = len(feeds[0])
    e = loam.Engine(_cfg(loam))
    e.lanes_open(S, MAP_CAP)
    lanes = range(S) if lanes is None else lanes
    outs, regs, surs = [], [], []
    for k, raws in enumerate(feeds):
        if before:
            before(k, e, outs)
        o = e.lanes_step(raws, stamp=0.1 * k)
        outs.append(o)
        surs.append(e.lanes_surround() if surround else None)
        regs.append({l: e.lanes_registered(l) for l in lanes if o["mapped"][l] and o["status"][l] == 0})
    maps = {l: e.lanes_map_export(l) for l in lanes if outs[-1]["status"][l] == 0}
    e.close()
    return outs, regs, surs, maps


def test_lanes_equal_contexts(loam, sweeps, ctx):
    seeds = (1, 2, 3)
    feeds = [[sweeps(s)[k] for s in seeds] for k in range(N_SWEEPS)]
    outs, regs, surs, maps = _run(loam, feeds)
    pubs = []
    for l, s in enumerate(seeds):
        recs, cmap = ctx(f"s{s}", sweeps(s))
        for k in range(N_SWEEPS):
            _step_eq(loam, outs[k], regs[k], l, recs[k], f"lane {l} step {k}")
            _sur_eq(surs[k], l, recs[k], f"lane {l} step {k}")
        pubs.append([k for k in range(N_SWEEPS) if surs[k][l] is not None])
        _map_eq(maps[l], cmap, f"lane {l} map")
    assert pubs == [[2, 12]] * 3  # the 1st mapping frame and the 5th after it
    # a run that never asked: every step and the final maps are the same bits
    o2, r2, _, m2 = _run(loam, feeds, surround=False)
    for k in range(N_SWEEPS):
        for f in outs[k]:
            np.testing.assert_array_equal(outs[k][f].view(np.uint32), o2[k][f].view(np.uint32), err_msg=f"step {k} {f}")
        assert regs[k].keys() == r2[k].keys()
        for l in regs[k]:
            _same(regs[k][l], r2[k][l], f"step {k} lane {l} registered")
    for l in range(3):
        _map_eq(maps[l], m2[l], f"lane {l} map, with and without lanes_surround")


def _filler():
    """30 000 seeded uniform points in a 40 m box above the scene (y: up), inside the centre cube's
    5 x 5 x 5 neighbourhood (50 m cubes about (10, 5, 10): |x|, |z| < 125, y < 125)"""
    rng = np.random.default_rng(2029)
    p = np.zeros((30000, 4), np.float32)
    p[:, 0] = rng.uniform(-20, 20, 30000)
    p[:, 1] = rng.uniform(30, 70, 30000)
    p[:, 2] = rng.uniform(-20, 20, 30000)
    p[:, 3] = rng.uniform(0, 1, 30000)
    return p


def test_lanes_due_on_different_steps(loam, sweeps, ctx):
    """before step 5 (mapping frames 2 and 4 done: phase 1) lane 0 gets its own map back with
    surround_phase 2 (due on sweep 10), lane 1 its own map plus the filler with surround_phase 4
    (due on sweep 6); lane 2 is left alone (due on sweeps 2 and 12)"""
    seeds = (1, 2, 3)
    at = 5
    feeds = [[sweeps(s)[k] for s in seeds] for k in range(N_SWEEPS)]
    fill = _filler()
    # (CPU) the filler alone keeps more than the largest LDS tier under a 0.4 m VoxelGrid, so the
    # lane's published cloud (leaf 0.2, behind its surf cubes' 0.4) stays beyond it whatever else is there
    vox = np.floor(fill[:, :3].astype(np.float64) / 0.4).astype(np.int64)
    assert np.unique(vox, axis=0).shape[0] > TIER_LDS
    kws = {0: lambda m: _kw(m, surround_phase=2),
           1: lambda m: _kw(m, surf=np.concatenate([m["surf"], fill]), surround_phase=4)}
    sizes = {}

    def before(k, e, outs):
        if k == at:
            for l in (0, 1):
                assert e.lanes_map_import([l], **kws[l](e.lanes_map_export(l))) == (0, 0)
            assert e.lanes_surround() == [None] * 3

    S = 3
    e = loam.Engine(_cfg(loam))
    e.lanes_open(S, MAP_CAP)
    outs, regs, surs = [], [], []
    for k in range(N_SWEEPS):
        before(k, e, outs)
        o = e.lanes_step(feeds[k], stamp=0.1 * k)
        outs.append(o)
        surs.append(e.lanes_surround())
        regs.append({l: e.lanes_registered(l) for l in range(S) if o["mapped"][l]})
        for l in range(S):
            if surs[k][l] is not None:  # the segment's input, rebuilt from the lane's export
                src = _surround_input(e.lanes_map_export(l), o["aft"][l][3:])
                sizes[(k, l)] = (src.shape[0], surs[k][l].shape[0])
                print(f"step {k} lane {l}: surround input {src.shape[0]} points, published {surs[k][l].shape[0]}")
    maps = {l: e.lanes_map_export(l) for l in range(S)}
    e.close()
    for l, s in enumerate(seeds):
        recs, cmap = ctx(f"s{s}+import{l}@{at}" if l in kws else f"s{s}", sweeps(s), {at: kws[l]} if l in kws else None)
        for k in range(N_SWEEPS):
            _step_eq(loam, outs[k], regs[k], l, recs[k], f"lane {l} step {k}")
            _sur_eq(surs[k], l, recs[k], f"lane {l} step {k}")
        _map_eq(maps[l], cmap, f"lane {l} map")
    pubs = {k: [l for l in range(S) if surs[k][l] is not None] for k in range(N_SWEEPS)}
    assert {k: v for k, v in pubs.items() if v} == {2: [0, 1, 2], 6: [1], 10: [0], 12: [2]}
    assert any(0 < len(v) < S for v in pubs.values())  # a proper subset of the lanes
    # at most 4 segments: the route starts at the 12288-point tier; some lane is served by it, and
    # lane 1's segment lies beyond every LDS tier (k_vg_big)
    assert sizes[(6, 1)][0] > TIER_LDS and sizes[(6, 1)][1] > TIER_LDS
    assert any(n <= TIER_LDS for (n, _) in sizes.values())


def test_restart_failure_retirement(loam, sweeps, ctx):
    """lane 1 is restarted behind step 2 (where it was due) onto stream 4; lane 2 is fed a NaN sweep
    and lane 3 count = 0 on step 3; lane 0 runs undisturbed"""
    n = N_SWEEPS
    seeds = (1, 2, 3, 5)
    empty = np.zeros((0, 4), np.float32)
    D = sweeps(4)
    state = {}

    def before(k, e, outs):
        if k == 3:
            sur = e.lanes_surround()
            assert all(s is not None for s in sur)
            state["wait"] = e.lanes_restart(1)
            after = e.lanes_surround()
            assert after[1] is None  # the restart dropped the lane's flag, and only that one
            for l in (0, 2, 3):
                _same(after[l], sur[l], f"lane {l} after lane 1's restart")

    feeds = [[sweeps(s)[k] for s in seeds] for k in range(n)]
    for k in range(3, n):
        feeds[k][1] = D[k - 2]  # wait_steps == 0: step 3 is the lane's init step and takes D[1]
        feeds[k][3] = empty
    feeds[3][2] = np.full_like(feeds[3][2], np.nan)
    outs, regs, surs, maps = _run(loam, feeds, before=before, lanes=(0, 1))
    assert state["wait"] == 0
    inval = loam.LOAM_E_INVAL
    for k in range(3, n):
        assert outs[k]["status"][2] == inval and outs[k]["status"][3] == inval, k
        assert surs[k][2] is None and surs[k][3] is None, k  # (step 12 would have been their 6th frame)
    # the restarted lane: a fresh system_delay = 0 context over D (D[0]: the sweep the caller drops)
    recs, cmap = ctx("s4", D[:n - 2])
    for j, k in enumerate(range(3, n)):
        _step_eq(loam, outs[k], regs[k], 1, recs[1 + j], f"restarted lane step {k}")
        _sur_eq(surs[k], 1, recs[1 + j], f"restarted lane step {k}")
    assert [k for k in range(n) if surs[k][1] is not None] == [2, 4]  # its own 1st mapping frame: step 4
    assert [l for l in range(4) if surs[4][l] is not None] == [1]
    _map_eq(maps[1], cmap, "restarted lane map")
    # the undisturbed lane, and the others up to their failure, equal their S = 1 runs
    for l, upto in ((0, n), (2, 3), (3, 3)):
        so, sr, ss, sm = _run(loam, [[sweeps(seeds[l])[k]] for k in range(upto)])
        for k in range(upto):
            assert (surs[k][l] is None) == (ss[k][0] is None), (l, k)
            if ss[k][0] is not None:
                _same(surs[k][l], ss[k][0], f"lane {l} step {k} vs S=1")
        if l == 0:
            _map_eq(maps[0], sm[0], "lane 0 map vs S=1")
            assert [k for k in range(n) if surs[k][0] is not None] == [2, 12]


def _raw_call(loam, e, S, pts=None, capacity=0):
    off = np.full(S + 1, 0xDEAD, np.uint32)
    pub = np.full(S, -7, np.int32)
    c = loam.LanesCloud(pts.ctypes.data if pts is not None else None, capacity, 0xBEEF, off.ctypes.data, pub.ctypes.data)
    rc = loam.lib().loam_lanes_surround(e.h, ctypes.byref(c))
    return rc, int(c.count), off, pub


def test_capacity_protocol(loam, sweeps):
    S = 2
    e = loam.Engine(_cfg(loam))
    e.lanes_open(S, MAP_CAP)
    for k in range(3):
        o = e.lanes_step([sweeps(1)[k], sweeps(2)[k]], stamp=0.1 * k)
    assert list(o["mapped"]) == [1, 1]
    direct = e.lanes_surround()
    n0, n1 = direct[0].shape[0], direct[1].shape[0]
    rc, count, off, pub = _raw_call(loam, e, S)  # sizes only
    assert rc == loam.LOAM_OK and count == n0 + n1 and list(off) == [0, n0, n0 + n1] and list(pub) == [1, 1]
    guard = np.full((count, 4), 7.0, np.float32)
    rc, c2, off2, pub2 = _raw_call(loam, e, S, guard, count - 1)
    assert rc == loam.LOAM_E_CAPACITY and loam.lib().loam_last_error()
    assert c2 == count and list(off2) == list(off) and list(pub2) == [1, 1]
    assert np.all(guard == 7.0)  # no point was written
    rc, c3, off3, _ = _raw_call(loam, e, S, guard, count)
    assert rc == loam.LOAM_OK and c3 == count and list(off3) == list(off)
    _same(guard[:n0], direct[0], "lane 0, the call with room")
    _same(guard[n0:], direct[1], "lane 1, the call with room")
    again = np.zeros((count + 5, 4), np.float32)
    rc, c4, _, _ = _raw_call(loam, e, S, again, count + 5)
    assert rc == loam.LOAM_OK and c4 == count
    _same(again[:count], guard, "two calls in a row")
    assert np.all(again[count:] == 0)
    # without offset / published arrays the count alone is filled
    c = loam.LanesCloud(None, 0, 0, None, None)
    assert loam.lib().loam_lanes_surround(e.h, ctypes.byref(c)) == loam.LOAM_OK and c.count == count
    e.close()


def test_protocol(loam, sweeps):
    L = loam.lib()
    inval = loam.LOAM_E_INVAL
    S = 2
    e = loam.Engine(_cfg(loam))
    c = loam.LanesCloud(None, 3, 5, None, None)
    assert L.loam_lanes_surround(e.h, ctypes.byref(c)) == inval and b"not open" in L.loam_last_error()
    assert (c.capacity, c.count) == (3, 5)
    e.lanes_open(S, MAP_CAP)
    a, b = sweeps(1), sweeps(2)

    def nothing():
        rc, count, off, pub = _raw_call(loam, e, S)
        return rc == loam.LOAM_OK and count == 0 and list(off) == [0] * (S + 1) and list(pub) == [0] * S

    assert nothing()  # before the first pull
    e.lanes_push([a[0], b[0]])
    off = np.full(S + 1, 9, np.uint32)
    c = loam.LanesCloud(None, 3, 5, off.ctypes.data, None)
    assert L.loam_lanes_surround(e.h, ctypes.byref(c)) == inval and b"in flight" in L.loam_last_error()
    assert (c.capacity, c.count) == (3, 5) and list(off) == [9] * (S + 1)
    e.lanes_pull()
    assert nothing()  # the sweep that is not looked at
    e.lanes_step([a[1], b[1]], stamp=0.1)
    assert nothing()  # the init frame: a step that did not map
    o = e.lanes_step([a[2], b[2]], stamp=0.2)
    assert list(o["mapped"]) == [1, 1]
    sur = e.lanes_surround()
    assert sur[0] is not None and sur[1] is not None
    # an import into a due lane drops that lane's flag only
    m = e.lanes_map_export(0)
    e.lanes_map_import([0], **{k: m[k] for k in ("corner", "surf", "center", "surround_phase", "aft", "bef")})
    after = e.lanes_surround()
    assert after[0] is None
    _same(after[1], sur[1], "lane 1 after lane 0's import")
    e.lanes_push([a[3], b[3]], stamp=0.3)
    assert L.loam_lanes_surround(e.h, ctypes.byref(c)) == inval  # in flight again
    o = e.lanes_pull()
    assert list(o["mapped"]) == [0, 0] and list(o["status"]) == [0, 0]
    assert nothing()  # the next push dropped the flags, and this step did not map
    e.lanes_close()
    assert L.loam_lanes_surround(e.h, ctypes.byref(c)) == inval  # closed again
    e.close()


def test_sixty_five_lanes(loam, sweeps, ctx):
    """S = 65, the sweep that is not looked at, the init frame and the first mapping frame: all 65
    lanes are due, so the VoxelGrid starts at its 2048-point tier.  Lanes 0 .. 63 repeat streams 1-3;
    lane 64 is fed every 16th point of stream 1, whose neighbourhood stays below that tier"""
    S, K = 65, 3
    dec = [sw[::16].copy() for sw in sweeps(1)[:K]]
    feed_of = [sweeps(1 + l % 3) for l in range(64)] + [dec]
    e = loam.Engine(_cfg(loam))
    e.lanes_open(S, MAP_CAP)
    for k in range(K):
        o = e.lanes_step([f[k] for f in feed_of], stamp=0.1 * k)
    assert np.all(o["status"] == 0) and np.all(o["mapped"] == 1)
    rc, count, off, pub = _raw_call(loam, e, S)
    sur = e.lanes_surround()
    assert rc == loam.LOAM_OK and list(pub) == [1] * S
    assert list(off) == list(np.concatenate([[0], np.cumsum([s.shape[0] for s in sur])])) and count == off[S]
    sizes = {l: _surround_input(e.lanes_map_export(l), o["aft"][l][3:]).shape[0] for l in (0, 1, 2, 64)}
    print("surround input points of lanes 0, 1, 2, 64:", sizes, "published:", {l: sur[l].shape[0] for l in sizes})
    e.close()
    for l in range(64):
        recs, _ = ctx(f"s{1 + l % 3}", sweeps(1 + l % 3)[:K])
        _sur_eq(sur, l, recs[K - 1], f"lane {l}")
    recs, _ = ctx("s1/16", dec)
    _sur_eq(sur, 64, recs[K - 1], "the decimated lane")
    # the route's first tier takes the decimated lane; the whole sweeps' segments pass it on
    assert sizes[64] <= TIER_SMALL < min(sizes[l] for l in (0, 1, 2))
