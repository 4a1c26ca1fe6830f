"""Shared lanes (loam_lanes_open_shared): every lane localizes in the context's one
map, which a step only reads.

The specification: on a mapping step, lane l's aft, bef, mp_iters and registered cloud are what
loam_mapping returns on a scratch context that has just received loam_map_import(M with aft = the
lane's Aft, bef = its Bef), M being the context's map at the push.  The yardstick of a lane is
therefore a streaming context fed the lane's sweeps through loam_chain_sweep with that import in
front of every sweep (`_scratch`), never a second lanes run.  The prior map M is a fresh context
over stream 1, exported.

  1. S = 3 against scratch contexts, two pose guesses and a lane left at zero
  2. loam_lanes_localize_info against loam_map_localize(n = 1)
  3. the map is only read; the context's own streaming calls go on as if no lanes had been opened
  4. LOAM_LOC_NO_LM and LOAM_LOC_OFFGRID lanes beside an ordinary one
  5. lane_from_capacity exactly reached, and one point short (the sticky LOAM_E_CAPACITY)
  6. the context imports another map between two steps
  7. a lane with /imu/data beside one without
  8. a restart: loam_lanes_set_pose refused until the init step is pulled
  9. S = 65 (the batch launch forms)
 10. every LOAM_E_INVAL, each leaving the lanes as they were

Streams: VLP-16 synthetic loops (synthgen.stream_sweeps), as tests/test_gpu_lanes.py."""
import ctypes

import numpy as np
import pytest

import lanes_imu_cases as lc
from test_gpu_lanes_restart import _same, _step_eq

pytestmark = pytest.mark.gpu

FROM_CAP = 1 << 17
N_SWEEPS = 12
GUESS = np.array([[0, 0, 0, 0, 0, 0], [0.01, -0.02, 0.015, 0.05, -0.03, 0.04], [-0.015, 0.01, 0.02, -0.04, 0.02, 0.06]],
                 np.float32)  # Aft guesses: M's start pose (zero) and small offsets from it (test_gpu_lanes_map_import.py)
ZERO = np.zeros(6, np.float32)
FAR = np.array([0, 0, 0, 300.0, 0, 0], np.float32)   # centre cube 16: empty cubes, inside the grid (§19)
OFF = np.array([0, 0, 0, 450.0, 0, 0], np.float32)   # centre cube 19 of 21: within 3 of the edge


@pytest.fixture(scope="module")
def sweeps(sg):
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = sg.stream_sweeps(N_SWEEPS, seed)
        return cache[seed]
    return get


def _kw(m, **over):
    kw = {k: m[k] for k in ("corner", "surf", "center", "surround_phase", "aft", "bef")}
    kw.update(over)
    return kw


@pytest.fixture(scope="module")
def prior(loam, sweeps):
    """M: the map a fresh context built over stream 1"""
    e = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    for k, sw in enumerate(sweeps(1)):
        e.chain_sweep(sw, stamp=0.1 * k)
    m = e.map_export()
    e.close()
    assert m["corner"].shape[0] > 1000 and m["surf"].shape[0] > 1000
    return m


@pytest.fixture(scope="module")
def prior2(prior):
    """M shuffled, about another centre (the context's second map of test 6)"""
    rng = np.random.default_rng(6)
    out = dict(prior, center=np.array([11, 5, 9], np.int32))
    for name in ("corner", "surf"):
        out[name] = prior[name][rng.permutation(prior[name].shape[0])]
    return out


@pytest.fixture(scope="module")
def scratch(loam):
    """the yardstick of one lane: a context fed `seq` through chain_sweep with map_import(the map of
    step k, aft = the context's current Aft, bef = its current Bef) in front of every sweep.
    maps: {first step: map}; pose: {step: (aft, bef)} poses set in front of that step (a lane's
    set_pose); imus: per step the /imu/data messages delivered before it.  One record per sweep,
    with `pre` = the (Aft, Bef) the frame started from.  Cached by key."""
    cache = {}

    def run(key, seq, maps, pose=None, delay=1, skip=1, stamps=None, imus=None):
        key = (key, len(seq), delay, skip)
        if key in cache:
            return cache[key]
        e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
        aft, bef, m, recs = ZERO, ZERO, None, []
        for k, sw in enumerate(seq):
            if pose and k in pose:
                aft, bef = pose[k]
            m = maps.get(k, m)
            for msg in (imus[k] if imus else ()):
                e.imu(*msg)
            if m is not None:
                e.map_import(**_kw(m, aft=aft, bef=bef))
            rc, pub, od, a, b, reg = e.chain_sweep(sw, stamp=stamps[k] if stamps else 0.1 * k, registered=True)
            rec = {"rc": rc, "pub": pub, "od_sum": od, "aft": a, "bef": b, "reg": reg, "pre": (aft, bef)}
            if rc == 0 and a is None:
                rec["od_iters"] = e.stats()["od_iters"]
            if a is not None:
                rec["mp_iters"] = e.stats()["mp_iters"]
                aft, bef = a, b
            recs.append(rec)
        e.close()
        cache[key] = recs
        return recs
    return run


def _open(loam, S, m, from_cap=FROM_CAP, delay=1, skip=1):
    e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
    if m is not None:
        assert e.map_import(**_kw(m)) == (0, 0)
    e.lanes_open_shared(S, from_cap)
    return e


def _step(e, raws, k, lanes, stamp=None):
    o = e.lanes_step(raws, stamp=0.1 * k if stamp is None else stamp)
    info = e.lanes_localize_info()
    return o, {l: e.lanes_registered(l) for l in lanes if o["mapped"][l] and o["status"][l] == 0}, info


def _run(e, raws_of, n, lanes, hooks=None):
    outs, regs, infos = [], [], []
    for k in range(n):
        if hooks and k in hooks:
            hooks[k](e)
        o, r, i = _step(e, raws_of(k), k, lanes)
        outs.append(o)
        regs.append(r)
        infos.append(i)
    return outs, regs, infos


def _check_lane(loam, outs, regs, l, recs, first=0, shift=0, upto=None):
    mapped = 0
    for k in range(first, len(outs) if upto is None else upto):
        mapped += _step_eq(loam, outs[k], regs[k], l, recs[k + shift], f"lane {l} step {k}")
    return mapped


def _outs_eq(a, b, la, lb, msg):
    """lane la of run a = lane lb of run b, every pulled field and the registered clouds"""
    (oa, ra, ia), (ob, rb, ib) = a, b
    assert len(oa) == len(ob)
    for k in range(len(oa)):
        for f in oa[k]:
            _same(oa[k][f][la], ob[k][f][lb], f"{msg} step {k} {f}")
        assert ia[k][la].tobytes() == ib[k][lb].tobytes(), f"{msg} step {k} info"
        assert (la in ra[k]) == (lb in rb[k]), f"{msg} step {k}"
        if la in ra[k]:
            _same(ra[k][la], rb[k][lb], f"{msg} step {k} registered")


SEEDS3 = (1, 2, 1)
POSE3 = {0: GUESS[1], 2: GUESS[2]}


@pytest.fixture(scope="module")
def three(loam, sweeps, prior):
    """test 1's run: S = 3, seeds (1, 2, 1), lanes 0 and 2 set to two guesses, lane 1 left at zero"""
    def run(from_cap):
        e = _open(loam, 3, prior, from_cap)
        before = e.map_export()
        e.lanes_set_pose([2, 0], np.stack([POSE3[2], POSE3[0]]))
        res = _run(e, lambda k: [sweeps(s)[k] for s in SEEDS3], 10, range(3))
        after = e.map_export()
        return e, res, before, after
    e, res, before, after = run(FROM_CAP)
    yield {"e": e, "res": res, "before": before, "after": after, "run": run}
    e.close()


def _yard3(scratch, sweeps, prior, l, n=10):
    return scratch(f"s{SEEDS3[l]}+M g{l}", sweeps(SEEDS3[l])[:n], {0: prior}, {0: (POSE3.get(l, ZERO), ZERO)})


def test_three_lanes_against_scratch_contexts(loam, sweeps, prior, scratch, three):
    outs, regs, infos = three["res"]
    plain = scratch("s1 no map", sweeps(1)[:10], {})
    for l in range(3):
        recs = _yard3(scratch, sweeps, prior, l)
        assert _check_lane(loam, outs, regs, l, recs) >= 3
        km = [k for k, r in enumerate(recs) if r["aft"] is not None]
        assert all(recs[k]["mp_iters"] > 0 for k in km)  # the L-M ran in M
        assert all(infos[k]["status"][l] == loam.LOC_SOLVED for k in km)
    recs = _yard3(scratch, sweeps, prior, 0)
    km = next(k for k, r in enumerate(recs) if r["aft"] is not None)
    assert not np.array_equal(recs[km]["aft"].view(np.uint32), plain[km]["aft"].view(np.uint32))


def test_info_against_map_localize(loam, sweeps, prior, scratch, three):
    outs, regs, infos = three["res"]
    E = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    assert E.map_import(**_kw(prior)) == (0, 0)
    checked = 0
    for l in range(3):
        recs = _yard3(scratch, sweeps, prior, l)  # (`pre`: the poses the lane's frame started from, checked by test 1)
        A = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))  # the lane's clouds by node calls
        for k, sw in enumerate(sweeps(SEEDS3[l])[:10]):
            rc, f = A.scan_registration(sw, stamp=0.1 * k)
            pub = 0
            if rc == 0:
                pub, pose, cl, sl, full = A.odometry(f, stamp=0.1 * k)
            if pub != 7:
                for m in range(3):
                    assert infos[k]["status"][m] == loam.LOC_NONE and not infos[k]["aft"][m].any()
                    assert infos[k]["iters"][m] == 0 and infos[k]["map_surf"][m] == 0
                continue
            _same(outs[k]["od_sum"][l], pose, f"lane {l} step {k} od_sum")
            aft, bef = recs[k]["pre"]
            res = E.map_localize(pose, cl, sl, aft[None, :], bef[None, :])
            for key in loam.LOCALIZE_KEYS:
                _same(infos[k][key][l], res[key][0], f"lane {l} step {k} {key}")
            assert res["status"][0] == loam.LOC_SOLVED and res["map_surf"][0] > 100
            checked += 1
        A.close()
    E.close()
    assert checked >= 9


def _map_same(a, b, msg):
    for k in ("corner", "surf", "aft", "bef"):
        _same(a[k], b[k], f"{msg} {k}")
    for k in ("corner_offset", "surf_offset", "center"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{msg} {k}")
    assert a["surround_phase"] == b["surround_phase"], msg


def test_the_map_is_only_read(loam, sweeps, prior, three):
    _map_same(three["after"], three["before"], "the context's map after 10 steps")
    e = three["e"]
    K = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))  # never opened lanes
    assert K.map_import(**_kw(prior)) == (0, 0)
    _map_same(three["before"], K.map_export(), "the context's map")
    a, b = e.mapping_surround(), K.mapping_surround()
    assert (a is None) == (b is None)
    for k, sw in enumerate(sweeps(3)[:6]):
        ra, rb = e.chain_sweep(sw, stamp=0.1 * k, registered=True), K.chain_sweep(sw, stamp=0.1 * k, registered=True)
        for x, y in zip(ra, rb):
            assert (x is None) == (y is None), k
            if x is not None:
                _same(np.asarray(x, np.float32), np.asarray(y, np.float32), f"chain_sweep {k}")
        a, b = e.mapping_surround(), K.mapping_surround()
        assert (a is None) == (b is None), k
        if a is not None:
            _same(a, b, f"surround {k}")
    _map_same(e.map_export(), K.map_export(), "the maps after the later sweeps")
    K.close()
    # ... and the lanes go on in the map those sweeps left (one more step runs)
    o = e.lanes_step([sweeps(s)[10] for s in SEEDS3], stamp=1.0)
    assert list(o["status"]) == [0, 0, 0] and list(o["mapped"]) == [1, 1, 1]


def test_statuses(loam, sweeps, prior, scratch):
    n = 8
    e = _open(loam, 3, prior)
    e.lanes_set_pose([0, 1, 2], np.stack([FAR, OFF, GUESS[1]]))
    three_ = _run(e, lambda k: [sweeps(1)[k], sweeps(2)[k], sweeps(1)[k]], n, range(3))
    e.close()
    e = _open(loam, 1, prior)
    e.lanes_set_pose([0], GUESS[1])
    alone = _run(e, lambda k: [sweeps(1)[k]], n, range(1))
    e.close()
    outs, regs, infos = three_
    _outs_eq(three_, alone, 2, 0, "lane 2 beside the special lanes / alone")
    far = scratch("s1+M far", sweeps(1)[:n], {0: prior}, {0: (FAR, ZERO)})
    assert _check_lane(loam, outs, regs, 0, far) >= 3
    mapped = [k for k in range(n) if outs[k]["mapped"][0]]
    assert len(mapped) >= 3 and all(outs[k]["mapped"][1] == 1 and outs[k]["status"][1] == 0 for k in mapped)
    for k in mapped:
        i = infos[k]
        assert i["status"][0] == loam.LOC_NO_LM and i["iters"][0] == 0
        assert i["map_corner"][0] <= 10 or i["map_surf"][0] <= 100
        _same(outs[k]["aft"][0], FAR, "far aft")
        _same(outs[k]["bef"][0], ZERO, "far bef")
        assert outs[k]["mp_iters"][0] == 0 and outs[k]["n_registered"][0] > 0
        assert i["status"][1] == loam.LOC_OFFGRID
        _same(i["aft"][1], OFF, "off info aft")
        for key in loam.LOCALIZE_KEYS[2:]:
            assert i[key][1] == 0, key
        _same(outs[k]["aft"][1], OFF, "off aft")
        _same(outs[k]["bef"][1], ZERO, "off bef")
        assert outs[k]["mp_iters"][1] == 0 and outs[k]["n_registered"][1] == 0
        assert regs[k][1].shape[0] == 0
        assert i["status"][2] == loam.LOC_SOLVED


def test_from_capacity(loam, sweeps, prior, scratch, three):
    outs, regs, infos = three["res"]
    tot = np.stack([i["map_corner"].astype(np.int64) + i["map_surf"] for i in infos])  # [step][lane]
    F = int(tot.max())
    print("largest FromMap", F, tot.max(axis=0).tolist())
    assert F >= 1024  # (lane_from_capacity's lower bound)
    e, exact, _, _ = three["run"](F)
    e.close()
    for l in range(3):
        _outs_eq(exact, three["res"], l, l, f"lane {l} at lane_from_capacity = the largest FromMap")
    # one point less.  (Every lane of test 1 sees all of M, so all three reach F; a fourth lane at
    # the 300 m guess, whose valid cubes are empty, is the lane that must not notice.)
    n = len(outs)
    e = _open(loam, 4, prior, F - 1)
    before = e.map_export()
    e.lanes_set_pose([2, 0, 3], np.stack([POSE3[2], POSE3[0], FAR]))
    o, r, i = _run(e, lambda k: [sweeps(s)[k] for s in SEEDS3 + (1,)], n, range(4))
    _map_same(e.map_export(), before, "the context's map after the overflows")
    e.close()
    for l in range(3):
        first = next(k for k in range(n) if tot[k][l] > F - 1)  # the lane's first frame beyond the capacity
        _check_lane(loam, o, r, l, _yard3(scratch, sweeps, prior, l), upto=first)
        for k in range(first, n):
            assert o[k]["status"][l] == loam.LOAM_E_CAPACITY, (k, l)
            assert i[k]["status"][l] == loam.LOC_NONE and not i[k]["aft"][l].any()
    far = scratch("s1+M far", sweeps(1)[:n], {0: prior}, {0: (FAR, ZERO)})
    assert _check_lane(loam, o, r, 3, far) >= 3


def test_the_map_changes_between_steps(loam, sweeps, prior, prior2, scratch):
    n, at = 10, 5
    e = _open(loam, 3, prior)
    e.lanes_set_pose([2, 0], np.stack([POSE3[2], POSE3[0]]))

    def swap(eng):
        assert eng.map_import(**_kw(prior2)) == (0, 0)
    outs, regs, infos = _run(e, lambda k: [sweeps(s)[k] for s in SEEDS3], n, range(3), {at: swap})
    e.close()
    for l in range(3):
        recs = scratch(f"s{SEEDS3[l]}+M,M2@{at} g{l}", sweeps(SEEDS3[l])[:n], {0: prior, at: prior2},
                       {0: (POSE3.get(l, ZERO), ZERO)})
        assert _check_lane(loam, outs, regs, l, recs) >= 4
        late = [k for k in range(at, n) if recs[k]["aft"] is not None]
        assert len(late) >= 2
        for k in late:  # the L-M ran in the second map
            assert infos[k]["status"][l] == loam.LOC_SOLVED and infos[k]["map_surf"][l] > 100 and recs[k]["mp_iters"] > 0


def test_imu_lane(loam, sg, prior, scratch):
    feeds = lc.case_mixed(sg)[:2]  # lane 0 with /imu/data, lane 1 without
    n = lc.K
    e = loam.Engine(loam.default_config(system_delay=lc.DELAY))
    assert e.map_import(**_kw(prior)) == (0, 0)
    e.lanes_open_shared(2, FROM_CAP)
    e.lanes_set_pose([0, 1], GUESS[1])
    outs, regs = [], []
    for k in range(n):
        for l, f in enumerate(feeds):
            for m in f.sched[k]:
                e.lanes_imu(l, *m)
        o, r, _ = _step(e, [f.sweeps[k] for f in feeds], k, range(2), stamp=[f.stamps[k] for f in feeds])
        outs.append(o)
        regs.append(r)
    e.close()
    skip = int(loam.default_config().skip_frame_num)
    for l, f in enumerate(feeds):
        recs = scratch(f"imu case_mixed {l}", f.sweeps, {0: prior}, {0: (GUESS[1], ZERO)}, lc.DELAY, skip, f.stamps,
                       f.sched)
        assert _check_lane(loam, outs, regs, l, recs) >= 3
        assert all(r["mp_iters"] > 0 for r in recs if r["aft"] is not None)
    # the blend matters: the same sweeps without the messages end elsewhere
    f = feeds[0]
    with_imu = scratch("imu case_mixed 0", f.sweeps, {0: prior}, {0: (GUESS[1], ZERO)}, lc.DELAY, skip, f.stamps, f.sched)
    without = scratch("imu case_mixed 0, no messages", f.sweeps, {0: prior}, {0: (GUESS[1], ZERO)}, lc.DELAY, skip, f.stamps)
    assert f.has_imu
    assert any(a["aft"] is not None and not np.array_equal(a["aft"].view(np.uint32), b["aft"].view(np.uint32))
               for a, b in zip(with_imu, without))


def test_restart(loam, sweeps, prior, scratch):
    n, after = 12, 5
    e = _open(loam, 3, prior)
    e.lanes_set_pose([0, 2], np.stack([POSE3[0], POSE3[2]]))
    outs, regs = [], []
    init_step = None
    P = ctypes.POINTER(loam.Pose6)
    one = (ctypes.c_uint32 * 1)(1)
    g = np.ascontiguousarray(GUESS[1][None, :])
    for k in range(n):
        if k == after:
            assert e.lanes_restart(1) == 0
            init_step = after
        if init_step is not None and k <= init_step:  # up to and including the push of the init step
            assert loam.lib().loam_lanes_set_pose(e.h, 1, one, g.ctypes.data_as(P), None) == loam.LOAM_E_INVAL
            assert b"init step" in loam.lib().loam_last_error()
        if init_step is not None and k == init_step + 1:
            e.lanes_set_pose([1], GUESS[1])
        raws = [sweeps(1)[k], sweeps(2)[k], sweeps(1)[k]]
        if init_step is not None:
            raws[1] = sweeps(1)[0] if k < init_step else sweeps(1)[1 + k - init_step]
        o, r, _ = _step(e, raws, k, range(3))
        outs.append(o)
        regs.append(r)
    e.close()
    recs = scratch("s1+M fresh g1", sweeps(1)[:1 + n - init_step], {0: prior}, {0: (GUESS[1], ZERO)}, delay=0)
    assert recs[0]["rc"] == loam.LOAM_E_NOT_READY and recs[1]["pub"] == loam.PUB_CLOUDS
    assert _check_lane(loam, outs, regs, 1, recs, first=init_step, shift=1 - init_step) >= 2
    before = scratch("s2+M g1", sweeps(2)[:after], {0: prior})
    _check_lane(loam, outs, regs, 1, before, upto=after)
    for l in (0, 2):
        assert _check_lane(loam, outs, regs, l, _yard3(scratch, sweeps, prior, l, n)) >= 4


@pytest.mark.parametrize("from_cap", [FROM_CAP, 8192])
def test_65_lanes(loam, sweeps, prior, scratch, from_cap):
    """S = 65: the batch forms of the L-M; lane_from_capacity above / at 8192: the grid-per-cloud hash
    build / the workgroup-per-cloud one.  The second case runs in M thinned to at most 8192 points,
    so that no FromMap can exceed the capacity."""
    S, n = 65, 6
    seeds = (1, 2, 3)
    aft = (np.arange(S, dtype=np.float32)[:, None] * np.array([1, -1, 1, 2, -2, 2], np.float32) * np.float32(1e-3))
    sample = (0, 31, 64)
    if from_cap == 8192:
        step = -(-(prior["corner"].shape[0] + prior["surf"].shape[0]) // 8192)
        prior = dict(prior, corner=prior["corner"][::step], surf=prior["surf"][::step])
        assert prior["corner"].shape[0] + prior["surf"].shape[0] <= 8192 and prior["surf"].shape[0] > 1000
    e = _open(loam, S, prior, from_cap)
    e.lanes_set_pose(list(range(S)), aft)
    outs, regs, infos = _run(e, lambda k: [sweeps(seeds[l % 3])[k] for l in range(S)], n, sample)
    e.close()
    for l in sample:
        recs = scratch(f"s{seeds[l % 3]}+M a{l} {from_cap}", sweeps(seeds[l % 3])[:n], {0: prior}, {0: (aft[l], ZERO)})
        assert _check_lane(loam, outs, regs, l, recs) >= 2
        assert all(r["mp_iters"] > 0 for r in recs if r["aft"] is not None)
    assert all((o["status"] == 0).all() for o in outs[1:])


def test_every_invalid_call_changes_nothing(loam, sweeps, prior, scratch):
    n, at = 8, 5
    INVAL = loam.LOAM_E_INVAL
    L = loam.lib()
    P = ctypes.POINTER(loam.Pose6)
    g = np.ascontiguousarray(np.tile(GUESS[2], (4, 1)))
    info = (loam.LocalizeResult * 3)()

    def set_pose(eng, lanes, count=None, aft=g, lane_null=False):
        idx = (ctypes.c_uint32 * max(len(lanes), 1))(*lanes)
        return L.loam_lanes_set_pose(eng.h, len(lanes) if count is None else count, None if lane_null else idx,
                                     None if aft is None else aft.ctypes.data_as(P), None)
    closed = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    assert set_pose(closed, [0]) == INVAL and L.loam_lanes_localize_info(closed.h, info) == INVAL  # not open
    for bad in ((0, 4096), (loam.LANES_MAX + 1, 4096), (2, 1023), (2, (1 << 28) + 1), (1024, 1 << 21)):
        assert L.loam_lanes_open_shared(closed.h, *bad) == INVAL, bad
    closed.lanes_open(2, 4096)  # own-store lanes refuse both calls
    assert set_pose(closed, [0]) == INVAL and b"loam_lanes_open" in L.loam_last_error()
    assert L.loam_lanes_localize_info(closed.h, info) == INVAL
    assert L.loam_lanes_open_shared(closed.h, 2, 4096) == INVAL  # one set of lanes at a time
    closed.close()
    e = _open(loam, 3, prior)
    assert L.loam_lanes_localize_info(e.h, info) == INVAL  # before the first pull
    assert L.loam_lanes_open(e.h, 2, 4096) == INVAL
    e.lanes_set_pose([0, 1], np.stack([POSE3[0], GUESS[2]]))
    outs, regs = [], []
    for k in range(n):
        raws = [sweeps(1)[k], sweeps(2)[k], sweeps(3)[k] if k != 3 else np.zeros((0, 4), np.float32)]
        if k == at:
            assert outs[-1]["status"][2] == INVAL  # lane 2 has failed (the empty sweep)
            for lanes, kw in (([0], dict(count=0)), ([0, 1, 2, 0], dict(count=4)), ([0, 3], {}), ([1, 0xffffffff], {}),
                              ([1, 0, 1], {}), ([0, 2], {}), ([0], dict(aft=None)), ([0], dict(lane_null=True))):
                assert set_pose(e, lanes, **kw) == INVAL, (lanes, kw)
                assert L.loam_last_error()
            assert L.loam_lanes_localize_info(e.h, None) == INVAL
            for call in (lambda: e.lanes_map_export(0), lambda: e.lanes_surround(),
                         lambda: e.lanes_map_import([0], **_kw(prior))):
                with pytest.raises(loam.LoamError) as err:
                    call()
                assert err.value.code == INVAL and "no lane map" in str(err.value)
            e.lanes_push(raws, stamp=0.1 * k)
            assert set_pose(e, [0]) == INVAL and L.loam_lanes_localize_info(e.h, info) == INVAL  # a step in flight
            o = e.lanes_pull()
            r = {l: e.lanes_registered(l) for l in range(2) if o["mapped"][l]}
        else:
            o, r, _ = _step(e, raws, k, range(2))
        outs.append(o)
        regs.append(r)
    e.close()
    for l, s, a in ((0, 1, POSE3[0]), (1, 2, GUESS[2])):
        recs = scratch(f"s{s}+M inval {l}", sweeps(s)[:n], {0: prior}, {0: (a, ZERO)})
        assert _check_lane(loam, outs, regs, l, recs) >= 3
