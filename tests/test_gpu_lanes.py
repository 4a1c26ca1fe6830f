"""loam_lanes_*: S sequences in one context, stepped in lockstep.

The specification is one sentence: lane l behaves exactly as a fresh context fed lane l's sweeps
through loam_chain_sweep, with no IMU message.  So every comparison against such a context is bit
for bit (poses, registered clouds, the exported map); the oracle comparison uses the suite's
north-star tolerance.

  1. lanes == separate contexts (S = 3), step by step and in the final maps
  2. lanes == the CPU oracle within POSE_TOL
  3. a failed lane (NaN sweep) and a retired lane (count = 0) fail alone and for good; the other
     lanes equal their S = 1 runs; the context's own stream is untouched by the lanes
  4. S = 65: the launch forms only a large batch takes (and the per-query moments it must not take)
  5. protocol and argument errors leave the lanes as they were

Streams: VLP-16 synthetic loops (synthgen.stream_sweeps), skip_frame_num = 1, so after the
system_delay sweeps and the odometry's init frame every second sweep is a mapping frame."""
import ctypes

import numpy as np
import pytest

import scenarios

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4  # as tests/test_gpu_parity.py
MAP_CAP = 1 << 17
FULL = 7  # LOAM_PUB_POSE | LOAM_PUB_CLOUDS | LOAM_PUB_FULL


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


@pytest.fixture(scope="module")
def sweeps(sg):
    cache = {}

    def get(seed, n=10):
        if seed not in cache:
            cache[seed] = sg.stream_sweeps(10, seed)
        return cache[seed][:n]
    return get


@pytest.fixture(scope="module")
def chain(loam, sweeps):
    """a fresh context fed a stream through chain_sweep: one record per sweep and the final map"""
    cache = {}

    def run(seed, n, delay, eng=None):
        key = (seed, n, delay)
        if key in cache and eng is None:
            return cache[key]
        e = eng or loam.Engine(loam.default_config(system_delay=delay))
        recs = []
        for k, sw in enumerate(sweeps(seed, n)):
            rc, pub, od, aft, bef, reg = e.chain_sweep(sw, stamp=0.1 * k, registered=True)
            rec = {"rc": rc, "pub": pub, "od_sum": od, "aft": aft, "bef": bef, "reg": reg}
            if aft is not None:
                rec["mp_iters"] = e.stats()["mp_iters"]
            recs.append(rec)
        out = (recs, e.map_export())
        if eng is None:
            e.close()
            cache[key] = out
        return out
    return run


def _lanes_run(loam, feeds, delay, eng=None, export=True, before_close=None):
    """feeds[k][l]: lane l's sweep of step k.  Returns (per-step pull dicts, per-step {lane: registered
    cloud} of the live lanes, per-lane final map or None for a failed lane); before_close(engine) is
    called with the lanes still open"""
    S = len(feeds[0])
    e = eng or loam.Engine(loam.default_config(system_delay=delay))
    e.lanes_open(S, MAP_CAP)
    outs, regs = [], []
    for k, raws in enumerate(feeds):
        o = e.lanes_step(raws, stamp=0.1 * k)
        outs.append(o)
        regs.append({l: e.lanes_registered(l) for l in range(S) if o["mapped"][l] and o["status"][l] == 0})
    maps = [e.lanes_map_export(l) if export and outs[-1]["status"][l] == 0 else None for l in range(S)]
    if before_close:
        before_close(e)
    e.lanes_close()
    if eng is None:
        e.close()
    return outs, regs, maps


def _lane_eq_chain(loam, outs, regs, l, recs, msg):
    """lane l of a lanes run against a chain_sweep context's records, step by step, bit for bit"""
    assert len(outs) == len(recs)
    mapped = 0
    for k, (o, r) in enumerate(zip(outs, recs)):
        m = f"{msg} lane {l} step {k}"
        assert o["status"][l] == r["rc"], m
        if r["rc"] != 0:
            assert r["rc"] == loam.LOAM_E_NOT_READY and o["published"][l] == 0 and o["mapped"][l] == 0, m
            continue
        assert o["published"][l] == r["pub"], m
        assert o["mapped"][l] == (1 if r["aft"] is not None else 0), m
        _same(o["od_sum"][l], r["od_sum"], m + " od_sum")
        if r["aft"] is None:
            assert l not in regs[k], m
            continue
        mapped += 1
        _same(o["aft"][l], r["aft"], m + " aft")
        _same(o["bef"][l], r["bef"], m + " bef")
        assert o["mp_iters"][l] == r["mp_iters"], m
        assert o["n_registered"][l] == r["reg"].shape[0] > 0, m
        _same(regs[k][l], r["reg"], m + " registered")
    return mapped


def _lane_eq_lane(a, ra, la, b, rb, lb, msg, steps=None):
    """lane la of run a against lane lb of run b in every field, bit for bit"""
    for k in range(len(a) if steps is None else steps):
        for f in a[k]:
            va, vb = a[k][f][la], b[k][f][lb]
            m = f"{msg} step {k} {f}"
            if va.dtype == np.float32:
                _same(va, vb, m)
            else:
                assert va == vb, m
        assert (la in ra[k]) == (lb in rb[k]), msg
        if la in ra[k]:
            _same(ra[k][la], rb[k][lb], f"{msg} step {k} registered")


@pytest.fixture(scope="module")
def three(loam, sweeps):
    """S = 3, seeds 1-3, 10 sweeps, system_delay 2 (tests 1 and 2)"""
    feeds = [[sweeps(s)[k] for s in (1, 2, 3)] for k in range(10)]
    return _lanes_run(loam, feeds, delay=2)


def test_lanes_equal_separate_contexts(loam, three, chain):
    outs, regs, maps = three
    for l, seed in enumerate((1, 2, 3)):
        recs, cmap = chain(seed, 10, 2)
        assert _lane_eq_chain(loam, outs, regs, l, recs, "S=3") >= 3
        _map_eq(maps[l], cmap, f"lane {l} map")
        assert maps[l]["corner"].shape[0] > 0 and maps[l]["surf"].shape[0] > 0
    for o in outs:  # lockstep: the same frame kind in every lane
        assert len(set(o["published"])) == 1 and len(set(o["mapped"])) == 1


def test_lanes_equal_oracle(three, sweeps, oc):
    outs, _, _ = three
    for l, seed in enumerate((1, 2, 3)):
        ro = scenarios.run_stream(oc.Oracle(oc.default_config(system_delay=2)), sweeps(seed), stats=False)
        mapped = 0
        assert [r["k"] for r in ro] == [k for k, o in enumerate(outs) if o["status"][l] == 0]
        for r in ro:
            o, m = outs[r["k"]], f"lane {l} step {r['k']}"
            assert o["published"][l] == r["pub"], m
            if r["pub"] & 1:
                assert np.max(np.abs(o["od_sum"][l] - r["pose"])) <= POSE_TOL, m
            assert o["mapped"][l] == (1 if "aft" in r else 0), m
            if "aft" in r:
                mapped += 1
                assert np.max(np.abs(o["aft"][l] - r["aft"])) <= POSE_TOL, m
                assert np.max(np.abs(o["bef"][l] - r["bef"])) <= POSE_TOL, m
        assert mapped >= 3


def test_independence_and_retirement(loam, sweeps, chain):
    K = 8
    empty = np.zeros((0, 4), np.float32)
    seeds = (1, 2, 3, 4, 5)
    feeds = [[sweeps(s)[k] for s in seeds] for k in range(K)]
    feeds[3][4] = np.full_like(feeds[3][4], np.nan)
    for k in range(5, K):
        feeds[k][2] = empty
    eng = loam.Engine(loam.default_config(system_delay=1))
    inval = loam.LOAM_E_INVAL

    def refused(e):  # a failed lane's map is not exported
        for l in (4, 2):
            with pytest.raises(loam.LoamError) as ei:
                e.lanes_map_export(l)
            assert ei.value.code == inval
    outs, regs, maps = _lanes_run(loam, feeds, delay=1, eng=eng, before_close=refused)
    for k, o in enumerate(outs):
        want = [loam.LOAM_E_NOT_READY] * 5 if k == 0 else [0, 0, inval if k >= 5 else 0, 0, inval if k >= 3 else 0]
        assert list(o["status"]) == want, k
    for l, seed in ((0, 1), (1, 2), (3, 4)):
        so, sr, sm = _lanes_run(loam, [[sweeps(seed)[k]] for k in range(K)], delay=1)
        _lane_eq_lane(outs, regs, l, so, sr, 0, f"lane {l} vs S=1")
        _map_eq(maps[l], sm[0], f"lane {l} map vs S=1")
        assert sum(int(o["mapped"][0]) for o in so) == 3
    # the retired lane ran like its S = 1 self until it was retired
    so, sr, _ = _lanes_run(loam, [[sweeps(3)[k]] for k in range(5)], delay=1, export=False)
    _lane_eq_lane(outs, regs, 2, so, sr, 0, "lane 2 before retirement", steps=5)
    # the context's own streaming state was not touched by the lanes
    recs, cmap = chain(1, 4, 1)
    mine, mmap = chain(1, 4, 1, eng=eng)
    for k, (a, b) in enumerate(zip(mine, recs)):
        assert (a["rc"], a["pub"]) == (b["rc"], b["pub"]), k
        for f in ("od_sum", "aft", "bef", "reg"):
            assert (a[f] is None) == (b[f] is None), (k, f)
            if a[f] is not None:
                _same(a[f], b[f], f"own stream step {k} {f}")
    _map_eq(mmap, cmap, "own stream map")
    eng.close()


def test_failed_lane_export_refused(loam, sweeps):
    eng = loam.Engine(loam.default_config(system_delay=1))
    eng.lanes_open(2, MAP_CAP)
    for k in range(3):
        raws = [sweeps(1)[k], sweeps(2)[k]]
        if k == 2:
            raws[1] = np.full_like(raws[1], np.nan)
        o = eng.lanes_step(raws)
    assert list(o["status"]) == [0, loam.LOAM_E_INVAL] and o["mapped"][0] == 1
    with pytest.raises(loam.LoamError) as ei:
        eng.lanes_map_export(1)
    assert ei.value.code == loam.LOAM_E_INVAL
    with pytest.raises(loam.LoamError) as ei:
        eng.lanes_registered(1)
    assert ei.value.code == loam.LOAM_E_INVAL
    assert eng.lanes_map_export(0)["surf"].shape[0] > 0
    # a sweep beyond max_points fails its lane with LOAM_E_CAPACITY and is not uploaded
    big = np.ones((int(eng.cfg.max_points) + 1, 4), np.float32)
    o = eng.lanes_step([big, sweeps(2)[3]])
    assert list(o["status"]) == [loam.LOAM_E_CAPACITY, loam.LOAM_E_INVAL]
    eng.close()


def test_large_batch_launch_shapes(loam, sweeps, chain):
    """S = 65 switches the ring sort to the fused kernel (>= 64 sweeps), the odometry to k_od_sel and
    the many-problem association grid, the hash builds to a workgroup per cloud, and would switch
    the odometry rows to the per-query moments, which are not bit-identical: the comparison with
    the chain_sweep contexts fails if the lanes leave them on."""
    K, S = 6, 65
    seed_of = [1 + l % 4 for l in range(64)] + [5]
    feeds = [[sweeps(s)[k] for s in seed_of] for k in range(K)]
    eng = loam.Engine(loam.default_config(system_delay=1))
    eng.lanes_open(S, MAP_CAP)
    outs, regs = [], []
    for k, raws in enumerate(feeds):
        o = eng.lanes_step(raws, stamp=0.1 * k)
        outs.append(o)
        # (the registered clouds of the lanes compared below: the first two copies of each stream)
        regs.append({l: eng.lanes_registered(l) for l in (0, 1, 2, 3, 4, 5, 6, 7, 64) if o["mapped"][l]})
    for k, o in enumerate(outs):
        assert np.all(o["status"] == (loam.LOAM_E_NOT_READY if k == 0 else 0)), k
        for f, v in o.items():  # every copy of a stream agrees in every field
            for l in range(4, 64):
                if v.dtype == np.float32:
                    _same(v[l], v[l % 4], f"step {k} {f} lane {l}")
                else:
                    assert v[l] == v[l % 4], (k, f, l)
        for l in (4, 5, 6, 7):
            if o["mapped"][l]:
                _same(regs[k][l], regs[k][l - 4], f"step {k} registered lane {l}")
    for l in (0, 1, 2, 3, 64):
        recs, cmap = chain(seed_of[l], K, 1)
        assert _lane_eq_chain(loam, outs, regs, l, recs, "S=65") == 2
        if l in (1, 64):
            _map_eq(eng.lanes_map_export(l), cmap, f"lane {l} map")
    _map_eq(eng.lanes_map_export(61), eng.lanes_map_export(1), "copies' maps")
    eng.close()


def test_protocol_and_errors(loam, sweeps):
    L = loam.lib()
    inval = loam.LOAM_E_INVAL
    eng = loam.Engine(loam.default_config(system_delay=1))
    h = eng.h
    raw2 = (loam.CloudIn * 2)()
    out2 = (loam.LaneOut * 2)()
    cloud = loam.CloudOut(None, 0, 0)
    m = loam.Map()
    # before open
    assert L.loam_lanes_push(h, 0.0, raw2) == inval
    assert L.loam_lanes_pull(h, out2) == inval
    assert L.loam_lanes_registered(h, 0, ctypes.byref(cloud)) == inval
    assert L.loam_lanes_map_export(h, 0, ctypes.byref(m)) == inval
    assert L.loam_lanes_close(h) == inval
    # open's arguments
    assert L.loam_lanes_open(h, 0, MAP_CAP) == inval
    assert L.loam_lanes_open(h, 1025, MAP_CAP) == inval
    assert L.loam_lanes_open(h, 2, 1023) == inval
    assert L.loam_lanes_open(h, 2, (1 << 28) + 1) == inval
    assert L.loam_lanes_open(h, 1024, 1 << 21) == inval
    assert b"lane_map_capacity" in L.loam_last_error()
    with pytest.raises(loam.LoamError):  # (nothing was opened by the refused calls)
        eng.lanes_close()
    eng.lanes_open(2, MAP_CAP)
    assert L.loam_lanes_open(h, 2, MAP_CAP) == inval  # open twice
    assert L.loam_lanes_pull(h, out2) == inval  # nothing pushed
    a, b = sweeps(1), sweeps(2)
    o = eng.lanes_step([a[0], b[0]])  # inside system_delay
    assert list(o["status"]) == [loam.LOAM_E_NOT_READY] * 2
    eng.lanes_push([a[1], b[1]])  # the init frame
    raws = (loam.CloudIn * 2)(loam.CloudIn(a[2].ctypes.data, a[2].shape[0], 16),
                              loam.CloudIn(b[2].ctypes.data, b[2].shape[0], 16))
    assert L.loam_lanes_push(h, 0.0, raws) == inval  # push twice
    assert L.loam_lanes_map_export(h, 0, ctypes.byref(m)) == inval  # export while in flight
    assert L.loam_lanes_registered(h, 0, ctypes.byref(cloud)) == inval
    o = eng.lanes_pull()
    assert list(o["status"]) == [0, 0] and list(o["published"]) == [loam.PUB_CLOUDS] * 2 and list(o["mapped"]) == [0, 0]
    assert L.loam_lanes_pull(h, out2) == inval  # pull twice
    assert L.loam_lanes_registered(h, 0, ctypes.byref(cloud)) == inval  # a step that did not map
    assert L.loam_lanes_registered(h, 2, ctypes.byref(cloud)) == inval  # lane index
    assert L.loam_lanes_map_export(h, 2, ctypes.byref(m)) == inval
    o = eng.lanes_step([a[2], b[2]])  # the refused calls changed nothing: the step maps as it should
    assert list(o["published"]) == [FULL] * 2 and list(o["mapped"]) == [1, 1]
    n = int(o["n_registered"][1])
    assert n > 0
    small = np.full((n, 4), 7.0, np.float32)
    c = loam.CloudOut(small.ctypes.data, 0, n - 1)
    assert L.loam_lanes_registered(h, 1, ctypes.byref(c)) == loam.LOAM_E_CAPACITY
    assert c.count == n and np.all(small == 7.0)
    c.capacity = n
    assert L.loam_lanes_registered(h, 1, ctypes.byref(c)) == loam.LOAM_OK and c.count == n
    _same(small, eng.lanes_registered(1), "registered, repeated with room")
    # the two lanes are what an undisturbed run gives
    ref = loam.Engine(loam.default_config(system_delay=1))
    for k in range(3):
        rc, pub, od, aft, bef, reg = ref.chain_sweep(b[k], stamp=0.1 * k, registered=True)
    _same(o["aft"][1], aft, "aft after the refused calls")
    _same(small, reg, "registered after the refused calls")
    _map_eq(eng.lanes_map_export(1), ref.map_export(), "map after the refused calls")
    eng.lanes_close()
    eng.lanes_open(1, 1024)  # (open after close; the smallest store)
    eng.lanes_close()
    ref.close()
    eng.close()
