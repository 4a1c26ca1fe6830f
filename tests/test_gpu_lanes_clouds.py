"""loam_lanes_clouds / loam_lanes_clouds_device: every topic cloud of a step for a list of lanes in one
call.

The specification: for a live lane the nine clouds are, bit for bit and in point order, what the node
calls (loam_scan_registration -> loam_odometry -> loam_mapping) hand out on the context that lane
equals; a cloud the lane's frame does not have is an empty range; the call changes nothing in any lane.
Every yardstick cloud comes from contexts driven through the node calls, never from a second lanes run.

  1. the two kernels alone (loam_dev_lanes_pack) on the smallest shapes, against a numpy restatement
  2. S = 3 own-map lanes against three contexts, every step; the Last clouds on non-publishing steps
     against contexts with skip_frame_num = 0 and through loam_map_score; no side effect
  3. the same with lane IMU messages
  4. lists and states: unequal counts, a retired lane, a lane whose init step is a mapping step, the
     sizes-only query, LOAM_E_CAPACITY
  5. shared lanes: registered, an OFFGRID lane, the downloaded frame through loam_mapping elsewhere
  6. S = 65, all nine clouds: more than two staging buffers
  7. the device form: same bits, with and without a consumer stream; refused destinations
  8. every LOAM_E_INVAL with out untouched; a step in flight; before the first pull

Streams: VLP-16 synthetic loops (synthgen.stream_sweeps), system_delay = 0 (sweep 0 is still not looked
at, sweep 1 is the odometry's init frame), skip_frame_num = 1 unless a test says otherwise."""
import ctypes

import numpy as np
import pytest

import hipmem
import lanes_imu_cases as lc
from test_gpu_lanes_restart import _map_eq, _same

pytestmark = pytest.mark.gpu

MAP_CAP = 1 << 17
N_SWEEPS = 13
SR = ("full", "sharp", "less_sharp", "flat", "less_flat")
CLOUDS = SR + ("corner_last", "surf_last", "full_end", "registered")
TILE = 1024            # LOAM_DEV_LANES_PACK_TILE: points a workgroup of k_lanes_pack moves per pass
STAGE = 1 << 21        # points of one download staging buffer
EMPTY = np.zeros((0, 4), np.float32)
HOOK = "loam_dev_lanes_pack"
ZERO = np.zeros(6, np.float32)
OFF = np.array([0, 0, 0, 450.0, 0, 0], np.float32)   # centre cube 19 of 21: LOAM_LOC_OFFGRID
MD = 0.5


def _cfg(loam, skip=1, delay=0):
    return loam.default_config(system_delay=delay, skip_frame_num=skip)


@pytest.fixture(scope="module")
def sweeps(sg):
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = sg.stream_sweeps(N_SWEEPS, seed)
        return cache[seed]
    return get


@pytest.fixture(scope="module")
def nodes(loam):
    """a sequence through a fresh context's node calls: per sweep {"rc"} or the five scanRegistration
    clouds ("sr"), loam_odometry's published flags, transformSum and three clouds, and (mapping: on
    the frames that publish /velodyne_cloud_3) loam_mapping's aft, bef and registered cloud.
    imus: per sweep the /imu/data messages delivered before it.  Cached by key."""
    cache = {}

    def run(key, seq, skip=1, delay=0, mapping=True, imus=None, stamps=None):
        key = (key, len(seq), skip, delay, mapping)
        if key in cache:
            return cache[key]
        e = loam.Engine(_cfg(loam, skip, delay))
        recs = []
        for k, sw in enumerate(seq):
            t = stamps[k] if stamps else 0.1 * k
            for m in (imus[k] if imus else ()):
                e.imu(*m)
            rc, f = e.scan_registration(sw, stamp=t)
            if rc != 0:
                assert rc == loam.LOAM_E_NOT_READY
                recs.append({"rc": rc})
                continue
            pub, od, cl, sl, fe = e.odometry(f, stamp=t)
            rec = {"rc": 0, "sr": f, "pub": pub, "od_sum": od, "corner_last": cl, "surf_last": sl, "full_end": fe,
                   "aft": None}
            if mapping and pub & loam.PUB_FULL:
                rec["aft"], rec["bef"], rec["reg"] = e.mapping(od, cl, sl, fe, stamp=t)
            recs.append(rec)
        e.close()
        cache[key] = recs
        return recs
    return run


def _expect(loam, rec, rec0=None):
    """the nine clouds of a lane after the step whose node-call record is rec; rec0: the same sweep on
    a context with skip_frame_num = 0, which publishes the Last clouds on every frame"""
    if rec["rc"] != 0:
        return {c: EMPTY for c in CLOUDS}
    out = {c: rec["sr"][c] for c in SR}
    src = rec if rec["pub"] & loam.PUB_CLOUDS else rec0
    if src is not None:
        assert src["pub"] & loam.PUB_CLOUDS
        out["corner_last"], out["surf_last"] = src["corner_last"], src["surf_last"]
    out["full_end"] = rec["full_end"] if rec["pub"] & loam.PUB_FULL else EMPTY
    out["registered"] = rec["reg"] if rec["aft"] is not None else EMPTY
    return out


def _lane_eq(got, i, want, msg):
    for c, w in want.items():
        assert got[c][i].dtype == np.float32, msg
        _same(got[c][i], w, f"{msg} {c}")


# ---------------------------------------------------------------- 1. the kernels alone
def _hook(loam):
    P = ctypes.POINTER
    f = getattr(loam.lib(), HOOK)
    f.argtypes = [ctypes.c_int, ctypes.c_int32, P(ctypes.c_int32), P(ctypes.c_int32), P(ctypes.c_int32), P(ctypes.c_uint32),
                  ctypes.c_int32, P(ctypes.c_void_p), ctypes.c_void_p, ctypes.c_uint64, P(ctypes.c_uint64)]
    return f


def _pack_case(loam, S, strides, counts, mask, lanes, slack=7):
    """the hook on seeded clouds against the restatement: the table, every packed point, and dst behind
    the selection as it was"""
    rng = np.random.default_rng(35)
    src = [rng.integers(0, 1 << 32, (S, st, 4), dtype=np.uint64).astype(np.uint32) for st in strides]
    n = len(lanes)
    table = np.zeros((9, n + 1), np.uint64)
    packed = []
    for c in range(9):
        for j, l in enumerate(lanes):
            m = min(max(int(counts[c][l]), 0), strides[c]) if mask[l] >> c & 1 else 0
            table[c, j + 1] = table[c, j] + m
            packed.append(src[c][l, :m])
    packed = np.concatenate(packed)
    total = packed.shape[0]
    assert total == int(table[:, n].sum())
    dst = np.full((total + slack, 4), 0x7fc5a5a5, np.uint32)
    got = np.full((9, n + 1), 0xdead, np.uint64)
    P = ctypes.POINTER
    ptrs = (ctypes.c_void_p * 9)(*[s.ctypes.data for s in src])
    cnt = np.ascontiguousarray(counts, np.int32)
    args = (np.asarray(strides, np.int32), cnt, np.asarray(mask, np.int32), np.asarray(lanes, np.uint32))
    call = lambda room: _hook(loam)(0, S, args[0].ctypes.data_as(P(ctypes.c_int32)), args[1].ctypes.data_as(P(ctypes.c_int32)),
                                     args[2].ctypes.data_as(P(ctypes.c_int32)), args[3].ctypes.data_as(P(ctypes.c_uint32)),
                                     n, ptrs, dst.ctypes.data, room, got.ctypes.data_as(P(ctypes.c_uint64)))
    if total:
        assert call(total - 1) == loam.LOAM_E_CAPACITY  # (checked on the host: nothing runs)
        assert np.all(dst == 0x7fc5a5a5) and np.all(got == 0xdead)
    assert call(total + slack) == loam.LOAM_OK, loam.lib().loam_last_error()
    np.testing.assert_array_equal(got, table)
    np.testing.assert_array_equal(dst[:total], packed)
    assert np.all(dst[total:] == 0x7fc5a5a5)
    return table


def test_pack_kernels_smallest_shapes(loam):
    T = TILE
    big = 2 * T + 3
    far = 5 * T + 5  # one cloud of six tiles
    strides = [far, 12, 200, 33, big, 200, big, big, big]
    S = 5
    # counts of the listed lanes 3, 0, 4 cover 0, 1, T - 1, T, T + 1, the stride, stride + 5 (clamped),
    # a negative one (clamped to 0) and a cloud of several tiles; lane 1 is masked with large counts, lane 2
    # is not listed
    counts = np.zeros((9, S), np.int32)
    counts[:, 1] = 1 << 20
    counts[:, 2] = 5
    counts[:, 3] = [far, 0, 1, 33 + 5, T - 1, 200, T, T + 1, big]
    counts[:, 0] = [far + 5, 12, 200 + 5, -3, big + 5, 0, 2 * T, 1, T - 1]
    counts[:, 4] = [3 * T, 1, 0, 1, T + 1, 1, big, 5, 9]
    full = (1 << 9) - 1
    mask = [full, 0, full, full, full & ~(1 << 7 | 1 << 8)]  # lane 4: no full_end, no registered
    t = _pack_case(loam, S, strides, counts, mask, [3, 0, 4])
    assert int(t[7, 3] - t[7, 2]) == 0 and int(t[0, 2] - t[0, 1]) == far and int(t[3, 2] - t[3, 1]) == 0
    # listing the masked lane adds nothing; the default order
    t = _pack_case(loam, S, strides, counts, mask, [0, 1, 2, 3, 4])
    assert np.all(t[:, 2] == t[:, 1])
    # every lane masked: an all-zero table and nothing written
    t = _pack_case(loam, S, strides, counts, [0] * S, [3, 0, 4])
    assert not t.any()


def test_pack_offsets_beyond_one_block_scan(loam):
    """n = 300 listed lanes: the offsets kernel's second pass of 256 with the carried total"""
    S = 300
    rng = np.random.default_rng(36)
    strides = [5, 3, 4, 2, 5, 4, 5, 5, 5]
    counts = rng.integers(-1, 8, (9, S)).astype(np.int32)
    mask = rng.integers(0, 1 << 9, S).astype(np.int32)
    t = _pack_case(loam, S, strides, counts, mask, list(rng.permutation(S)))
    assert t[:, 300].min() > 0 and t[:, 256].min() > 0  # the second pass starts from a carried total


# ---------------------------------------------------------------- 2. own-map lanes against contexts
def _kw(m, **over):
    kw = {k: m[k] for k in ("corner", "surf", "center", "surround_phase", "aft", "bef")}
    kw.update(over)
    return kw


@pytest.fixture(scope="module")
def prior(loam, sweeps):
    """M: the map a fresh context built over stream 1"""
    e = loam.Engine(_cfg(loam, delay=1))
    for k, sw in enumerate(sweeps(1)[:12]):
        e.chain_sweep(sw, stamp=0.1 * k)
    m = e.map_export()
    e.close()
    assert m["corner"].shape[0] > 1000 and m["surf"].shape[0] > 1000
    return m


def _score_rec(loam, d):
    r = np.zeros(d["corner_in"].shape, loam._SCORE_DTYPE)
    assert r.dtype.itemsize == 32
    for k in loam.SCORE_KEYS:
        r[k] = d[k]
    return r


POSES = np.array([[0, 0, 0, 0, 0, 0], [0.01, -0.02, 0.015, 0.05, -0.03, 0.04]], np.float32)


def _own_run(loam, feeds, prior, clouds):
    """S own-map lanes in a context that holds M; per step the pull, lanes_clouds() (when asked), the
    lanes_score rows and lanes_surround(); the final maps"""
    S = len(feeds[0])
    e = loam.Engine(_cfg(loam))
    assert e.map_import(**_kw(prior)) == (0, 0)
    e.lanes_open(S, MAP_CAP)
    outs, got, scores, surs = [], [], [], []
    for k, raws in enumerate(feeds):
        o = e.lanes_step(raws, stamp=0.1 * k)
        outs.append(o)
        if clouds:
            got.append(e.lanes_clouds())
            again = e.lanes_clouds()
            for c in CLOUDS:
                for l in range(S):
                    _same(again[c][l], got[k][c][l], f"step {k} lane {l} {c}: a repeated call")
        scores.append(_score_rec(loam, e.lanes_score(list(range(S)), POSES, MD)) if k >= 1 else None)
        surs.append(e.lanes_surround())
    maps = [e.lanes_map_export(l) for l in range(S)]
    e.close()
    return outs, got, scores, surs, maps


def test_own_map_lanes_equal_contexts(loam, sweeps, nodes, prior):
    seeds = (1, 2, 3)
    feeds = [[sweeps(s)[k] for s in seeds] for k in range(N_SWEEPS)]
    outs, got, scores, surs, maps = _own_run(loam, feeds, prior, True)
    yard = loam.Engine(_cfg(loam))
    assert yard.map_import(**_kw(prior)) == (0, 0)
    kinds = set()
    for l, s in enumerate(seeds):
        recs = nodes(f"s{s}", sweeps(s))
        recs0 = nodes(f"s{s}", sweeps(s), skip=0, mapping=False)
        for k in range(N_SWEEPS):
            r, m = recs[k], f"lane {l} step {k}"
            assert outs[k]["status"][l] == r["rc"], m
            _lane_eq(got[k], l, _expect(loam, r, recs0[k]), m)
            if r["rc"] != 0:
                continue
            assert outs[k]["published"][l] == r["pub"] and outs[k]["mapped"][l] == (r["aft"] is not None), m
            kinds.add((bool(r["pub"] & loam.PUB_CLOUDS), bool(r["pub"] & loam.PUB_FULL), r["aft"] is not None))
            # full_end / registered are empty exactly where the context publishes none
            assert (got[k]["full_end"][l].shape[0] > 0) == bool(r["pub"] & loam.PUB_FULL), m
            assert (got[k]["registered"][l].shape[0] > 0) == (r["aft"] is not None), m
            assert got[k]["registered"][l].shape[0] == outs[k]["n_registered"][l], m
            assert got[k]["corner_last"][l].shape[0] > 0 and got[k]["surf_last"][l].shape[0] > TILE, m
            # the downloaded Last clouds are the clouds loam_lanes_score read: the same 32 bytes per row
            want = _score_rec(loam, yard.map_score(got[k]["corner_last"][l], got[k]["surf_last"][l], POSES, MD))
            for j in range(POSES.shape[0]):
                assert scores[k][l, j].tobytes() == want[j].tobytes(), (m, j)
    yard.close()
    # the init frame, mapping frames and frames that publish the pose alone
    assert kinds == {(True, False, False), (True, True, True), (False, False, False)}
    # a run that never asked: poses, surround clouds and maps are the same bits
    o2, _, s2, u2, m2 = _own_run(loam, feeds, prior, False)
    for k in range(N_SWEEPS):
        for f in outs[k]:
            np.testing.assert_array_equal(outs[k][f].view(np.uint32), o2[k][f].view(np.uint32), err_msg=f"step {k} {f}")
        for l in range(3):
            assert (surs[k][l] is None) == (u2[k][l] is None), (k, l)
            if surs[k][l] is not None:
                _same(surs[k][l], u2[k][l], f"step {k} lane {l} surround")
            if scores[k] is not None:
                assert scores[k][l].tobytes() == s2[k][l].tobytes(), (k, l)
    assert any(s is not None for sur in surs for s in sur)
    for l in range(3):
        _map_eq(maps[l], m2[l], f"lane {l} map, with and without lanes_clouds")


# ---------------------------------------------------------------- 3. lane IMU
def test_imu_lanes_equal_contexts(loam, sg, nodes):
    feeds = lc.case_mixed(sg)
    assert any(f.has_imu for f in feeds) and not all(f.has_imu for f in feeds)
    S, n = len(feeds), len(feeds[0].sweeps)
    e = loam.Engine(loam.default_config(system_delay=lc.DELAY))
    skip = int(e.cfg.skip_frame_num)
    e.lanes_open(S, MAP_CAP)
    outs, got = [], []
    for k in range(n):
        for l, f in enumerate(feeds):
            for m in f.sched[k]:
                e.lanes_imu(l, *m)
        outs.append(e.lanes_step([f.sweeps[k] for f in feeds], stamp=[f.stamps[k] for f in feeds]))
        got.append(e.lanes_clouds())
    e.close()
    mapped = 0
    for l, f in enumerate(feeds):
        recs = nodes(f"imu{l}", f.sweeps, skip=skip, delay=lc.DELAY, imus=f.sched, stamps=f.stamps)
        recs0 = nodes(f"imu{l}", f.sweeps, skip=0, delay=lc.DELAY, mapping=False, imus=f.sched, stamps=f.stamps)
        for k in range(n):
            assert outs[k]["status"][l] == recs[k]["rc"], (l, k)
            _lane_eq(got[k], l, _expect(loam, recs[k], recs0[k]), f"imu lane {l} step {k}")
            mapped += recs[k]["rc"] == 0 and recs[k]["aft"] is not None
    assert mapped >= 3 * S
    # the IMU took effect on the clouds: the de-skewed full cloud differs from the plain one
    l = next(l for l, f in enumerate(feeds) if f.has_imu)
    plain = nodes(f"imu{l} plain", feeds[l].sweeps, skip=skip, delay=lc.DELAY, mapping=False, stamps=feeds[l].stamps)
    assert not np.array_equal(got[-1]["full"][l].view(np.uint32), plain[-1]["sr"]["full"].view(np.uint32))


# ---------------------------------------------------------------- 4. lists and states
def _raw(loam, e, n, lanes, want=CLOUDS, pts=None, caps=None, offsets=True):
    """loam_lanes_clouds through ctypes with sentinels in count / offset: (rc, the struct, offsets)"""
    o = loam.LanesCloudsOut()
    offs = {}
    for c in want:
        b = getattr(o, c)
        b.count = 0xBEEF
        if offsets:
            offs[c] = np.full(n + 1, 0xDEAD, np.uint32)
            b.offset = offs[c].ctypes.data
        if pts is not None and c in pts:
            b.pts = pts[c].ctypes.data
            b.capacity = caps[c] if caps and c in caps else pts[c].shape[0]
    idx = None if lanes is None else (ctypes.c_uint32 * max(len(lanes), 1))(*lanes)
    rc = loam.lib().loam_lanes_clouds(e.h, n, idx, ctypes.byref(o))
    return rc, o, offs


def test_lists_and_states(loam, sweeps, nodes):
    """skip_frame_num = 0 (every frame from sweep 2 on publishes and maps, so a restarted lane's init step
    is a mapping step).  Lane 0: stream 1; lane 1: every 4th point of stream 2; lane 2: retired with
    count = 0 from step 3 on; lane 3: stream 3, restarted behind step 3 onto stream 4; lane 4: stream 3"""
    S, n = 5, 6
    D = sweeps(4)
    dec = [sw[::4].copy() for sw in sweeps(2)]
    e = loam.Engine(_cfg(loam, skip=0))
    e.lanes_open(S, MAP_CAP)
    got, outs = [], []
    for k in range(n):
        raws = [sweeps(1)[k], dec[k], sweeps(2)[k] if k < 3 else EMPTY, sweeps(3)[k] if k < 4 else D[k - 3], sweeps(3)[k]]
        if k == 4:
            assert e.lanes_restart(3) == 0  # its init step is the next one
            c = e.lanes_clouds([3, 0], ["full", "corner_last"])
            assert c["full"][0].shape[0] == 0 and c["corner_last"][0].shape[0] == 0  # between the restart and its init step's pull
            assert c["full"][1].shape[0] > 0
        outs.append(e.lanes_step(raws, stamp=0.1 * k))
        got.append(e.lanes_clouds())
    o = outs[4]
    assert o["published"][3] == loam.PUB_CLOUDS and o["mapped"][3] == 0 and o["mapped"][0] == 1
    yard = {0: nodes("s1", sweeps(1)[:n], skip=0), 1: nodes("s2/4", dec[:n], skip=0), 2: nodes("s2", sweeps(2)[:n], skip=0),
            3: nodes("s3", sweeps(3)[:n], skip=0), 4: nodes("s3", sweeps(3)[:n], skip=0)}
    fresh = nodes("s4", D[:n], skip=0)
    for k in range(n):
        for l in range(S):
            m = f"lane {l} step {k}"
            if l == 2 and k >= 3:
                assert outs[k]["status"][l] == loam.LOAM_E_INVAL, m
                want = {c: EMPTY for c in CLOUDS}
            elif l == 3 and k >= 4:
                want = _expect(loam, fresh[k - 3])
            else:
                want = _expect(loam, yard[l][k])
            _lane_eq(got[k], l, want, m)
    # the restarted lane's init step on a mapping step: no full_end, no registered, the raw lessSharp /
    # lessFlat clouds as its Last clouds, while the others have everything
    g = got[4]
    assert g["full_end"][3].shape[0] == 0 and g["registered"][3].shape[0] == 0
    _same(g["corner_last"][3], fresh[1]["sr"]["less_sharp"], "init step corner_last")
    _same(g["surf_last"][3], fresh[1]["sr"]["less_flat"], "init step surf_last")
    assert all(g["full_end"][l].shape[0] > 0 and g["registered"][l].shape[0] > 0 for l in (0, 1, 4))
    assert g["full"][1].shape[0] * 3 < g["full"][0].shape[0]  # unequal counts
    # a list in another order, a subset of the clouds
    last = got[n - 1]
    sub = e.lanes_clouds([2, 0], ["registered", "sharp"])
    assert sorted(sub) == ["registered", "sharp"]
    for c in sub:
        _same(sub[c][0], last[c][2], f"list [2, 0] {c}")
        _same(sub[c][1], last[c][0], f"list [2, 0] {c}")
    mid = e.lanes_clouds([4, 2, 1])  # the retired lane in the middle of the list
    for c in CLOUDS:
        assert mid[c][1].shape[0] == 0
        _same(mid[c][0], last[c][4], c)
        _same(mid[c][2], last[c][1], c)
    # the sizes-only query
    rc, s, offs = _raw(loam, e, S, None)
    assert rc == loam.LOAM_OK
    for c in CLOUDS:
        sizes = [last[c][l].shape[0] for l in range(S)]
        assert list(offs[c]) == list(np.concatenate([[0], np.cumsum(sizes)])) and getattr(s, c).count == sum(sizes), c
    # an unwanted cloud's struct is left untouched; count alone without an offset array
    rc, s2, _ = _raw(loam, e, S, None, want=("flat",), offsets=False)
    assert rc == loam.LOAM_OK and s2.flat.count == 0xBEEF  # (neither pts nor offset: not wanted)
    lone = np.zeros(S + 1, np.uint32)
    s3 = loam.LanesCloudsOut()
    s3.flat.offset = lone.ctypes.data
    s3.full.capacity, s3.full.count = 77, 0x1234
    untouched = bytes(s3.full)
    assert loam.lib().loam_lanes_clouds(e.h, S, None, ctypes.byref(s3)) == loam.LOAM_OK
    assert s3.flat.count == s.flat.count and list(lone) == list(offs["flat"]) and bytes(s3.full) == untouched
    # LOAM_E_CAPACITY: one point too few on one cloud: no byte of any pts written, every count / offset
    # filled, and the repeat succeeds
    bufs = {c: np.full((int(getattr(s, c).count) + 3, 4), 7.0, np.float32) for c in CLOUDS}
    caps = {c: int(getattr(s, c).count) for c in CLOUDS}
    rc, s4, o4 = _raw(loam, e, S, None, pts=bufs, caps=dict(caps, surf_last=caps["surf_last"] - 1))
    assert rc == loam.LOAM_E_CAPACITY and loam.lib().loam_last_error()
    for c in CLOUDS:
        assert np.all(bufs[c] == 7.0), c
        assert getattr(s4, c).count == getattr(s, c).count and list(o4[c]) == list(offs[c]), c
    rc, s5, o5 = _raw(loam, e, S, None, pts=bufs, caps=caps)
    assert rc == loam.LOAM_OK
    for c in CLOUDS:
        assert np.all(bufs[c][caps[c]:] == 7.0), c  # nothing behind the selection
        for l in range(S):
            _same(bufs[c][o5[c][l]:o5[c][l + 1]], last[c][l], f"the call with room, lane {l} {c}")
    e.close()


# ---------------------------------------------------------------- 5. shared lanes
def test_shared_lanes(loam, sweeps, prior):
    S, n = 3, 7
    seeds = (1, 2, 1)
    guess = np.array([0.01, -0.02, 0.015, 0.05, -0.03, 0.04], np.float32)
    e = loam.Engine(_cfg(loam, delay=1))
    assert e.map_import(**_kw(prior)) == (0, 0)
    e.lanes_open_shared(S, 1 << 17)
    e.lanes_set_pose([0, 2], np.stack([guess, OFF]))
    scratch = loam.Engine(_cfg(loam, delay=1))
    pose = {0: (guess, ZERO), 1: (ZERO, ZERO), 2: (OFF, ZERO)}
    mapped = offgrid = 0
    for k in range(n):
        o = e.lanes_step([sweeps(s)[k] for s in seeds], stamp=0.1 * k)
        info = e.lanes_localize_info()
        got = e.lanes_clouds()
        for l in range(S):
            m = f"shared lane {l} step {k}"
            if o["status"][l] != 0:
                assert all(got[c][l].shape[0] == 0 for c in CLOUDS), m
                continue
            assert got["full"][l].shape[0] > 0 and got["corner_last"][l].shape[0] > 0, m
            if not o["mapped"][l]:
                assert got["registered"][l].shape[0] == 0, m
                continue
            _same(got["registered"][l], e.lanes_registered(l), m + " registered")
            assert got["registered"][l].shape[0] == o["n_registered"][l], m
            if info["status"][l] == loam.LOC_OFFGRID:
                offgrid += 1
                assert got["registered"][l].shape[0] == 0 and got["full_end"][l].shape[0] > 0, m
                continue
            # the lane's frame, taken to loam_mapping on another context that holds the map with the
            # lane's Aft / Bef: the lane's own result
            assert scratch.map_import(**_kw(prior, aft=pose[l][0], bef=pose[l][1])) == (0, 0)
            aft, bef, reg = scratch.mapping(o["od_sum"][l], got["corner_last"][l], got["surf_last"][l], got["full_end"][l],
                                            stamp=0.1 * k)
            _same(aft, o["aft"][l], m + " aft through loam_mapping")
            _same(bef, o["bef"][l], m + " bef through loam_mapping")
            _same(reg, got["registered"][l], m + " registered through loam_mapping")
            pose[l] = (o["aft"][l].copy(), o["bef"][l].copy())
            mapped += 1
    e.close()
    scratch.close()
    assert mapped >= 4 and offgrid >= 2


# ---------------------------------------------------------------- 6. S = 65
def test_sixty_five_lanes(loam, sweeps, nodes):
    S, K = 65, 3
    e = loam.Engine(_cfg(loam))
    e.lanes_open(S, MAP_CAP)
    for k in range(K):
        o = e.lanes_step([sweeps(1 + l % 3)[k] for l in range(S)], stamp=0.1 * k)
    assert np.all(o["status"] == 0) and np.all(o["mapped"] == 1)
    got = e.lanes_clouds()
    total = sum(got[c][l].shape[0] for c in CLOUDS for l in range(S))
    biggest = max(sum(got[c][l].shape[0] for c in CLOUDS) for l in range(S))
    print(f"S = 65: {total} points, the largest lane {biggest}")
    assert total > 2 * STAGE and biggest < STAGE  # at least three staging chunks, a lane always fits one
    for l in range(S):
        _same(got["registered"][l], e.lanes_registered(l), f"lane {l} registered")
    e.close()
    for l in (0, 31, 64):
        rec = nodes(f"s{1 + l % 3}", sweeps(1 + l % 3)[:K])[K - 1]
        _lane_eq(got, l, _expect(loam, rec), f"lane {l} of 65")


# ---------------------------------------------------------------- 7. the device form
class _Dev:
    """a device buffer of `rows` points as lanes_clouds_device takes it"""

    def __init__(self, ptr, rows):
        self.ptr, self.rows = ptr, rows
        self.__cuda_array_interface__ = {"shape": (rows, 4), "typestr": "<f4", "data": (ptr, False), "version": 3}


def test_device_form(loam, sweeps):
    hip = hipmem.Hip(loam)
    S = 3
    engines = [loam.Engine(_cfg(loam)) for _ in range(2)]  # the second: a twin that sees no refused call
    for e in engines:
        e.lanes_open(S, MAP_CAP)
        for k in range(3):
            o = e.lanes_step([sweeps(s)[k] for s in (1, 2, 3)], stamp=0.1 * k)
        assert list(o["mapped"]) == [1, 1, 1]
    e, twin = engines
    lanes = [2, 0, 1]
    host = e.lanes_clouds(lanes)
    sizes = {c: sum(a.shape[0] for a in host[c]) for c in CLOUDS}
    slack = 5
    fill = np.full(4, 3.0, np.float32)

    def fresh():
        bufs = {}
        for c in CLOUDS:
            rows = sizes[c] + slack
            bufs[c] = _Dev(hip.upload(np.tile(fill, (rows, 1))), rows)
        return bufs

    def check(bufs, offs, msg):
        for c in CLOUDS:
            a = hip.get(bufs[c].ptr, bufs[c].rows * 16).view(np.float32).reshape(-1, 4)
            assert list(offs[c]) == list(np.concatenate([[0], np.cumsum([h.shape[0] for h in host[c]])])), (msg, c)
            for i in range(len(lanes)):
                _same(a[offs[c][i]:offs[c][i + 1]], host[c][i], f"{msg} {c} entry {i}")
            assert np.all(a[sizes[c]:] == 3.0), (msg, c)

    bufs = fresh()
    check(bufs, e.lanes_clouds_device(bufs, lanes), "no consumer stream")
    st = hip.stream()
    bufs = fresh()
    offs = e.lanes_clouds_device(bufs, lanes, stream=st)
    # the consumer's copy is ordered behind the pack by the stream alone
    pin = {c: hip.host_malloc(bufs[c].rows * 16) for c in CLOUDS}
    for c in CLOUDS:
        hip._ok(hip.L.hipMemcpyAsync(pin[c][0], bufs[c].ptr, bufs[c].rows * 16, hipmem.D2H, st), "hipMemcpyAsync")
    hip.sync(st)
    for c in CLOUDS:
        a = pin[c][1].view(np.float32).reshape(-1, 4)
        for i in range(len(lanes)):
            _same(a[offs[c][i]:offs[c][i + 1]], host[c][i], f"consumer stream {c} entry {i}")
        assert np.all(a[sizes[c]:] == 3.0), c
    check(bufs, offs, "consumer stream, read back")
    # refused destinations: nothing written anywhere
    bufs = fresh()
    hostmem = np.full((sizes["flat"] + slack, 4), 3.0, np.float32)
    refusals = {"a host pointer": dict(bufs, flat=_Dev(hostmem.ctypes.data, hostmem.shape[0])),
                "a misaligned pointer": dict(bufs, surf_last=_Dev(bufs["surf_last"].ptr + 4, bufs["surf_last"].rows - 1)),
                "a capacity that leaves the allocation": dict(bufs, full=_Dev(bufs["full"].ptr + 16, bufs["full"].rows))}
    for what, dst in refusals.items():
        with pytest.raises(loam.LoamError) as err:
            e.lanes_clouds_device(dst, lanes)
        assert err.value.code == loam.LOAM_E_INVAL, what
        assert np.all(hostmem == 3.0), what
        for c in CLOUDS:
            assert np.all(hip.get(bufs[c].ptr, bufs[c].rows * 16).view(np.float32) == 3.0), (what, c)
    # ... and the next step equals the twin's
    raws = [sweeps(s)[3] for s in (1, 2, 3)]
    oa, ob = e.lanes_step(raws, stamp=0.3), twin.lanes_step(raws, stamp=0.3)
    for f in oa:
        np.testing.assert_array_equal(oa[f].view(np.uint32), ob[f].view(np.uint32), err_msg=f)
    ca, cb = e.lanes_clouds(), twin.lanes_clouds()
    for c in CLOUDS:
        for l in range(S):
            _same(ca[c][l], cb[c][l], f"the step after the refusals, lane {l} {c}")
    for x in engines:
        x.close()
    hip.release()


# ---------------------------------------------------------------- 8. protocol
def test_protocol(loam, sweeps):
    L = loam.lib()
    inval = loam.LOAM_E_INVAL
    S = 3
    e = loam.Engine(_cfg(loam))

    def refused(n, lanes, word):
        o = loam.LanesCloudsOut()
        ctypes.memset(ctypes.byref(o), 0xa5, ctypes.sizeof(o))
        o.full.pts, o.full.offset = None, None  # (two clouds look wanted, one does not)
        before = bytes(o)
        idx = None if lanes is None else (ctypes.c_uint32 * max(len(lanes), 1))(*lanes)
        for call in (lambda: L.loam_lanes_clouds(e.h, n, idx, ctypes.byref(o)),
                     lambda: L.loam_lanes_clouds_device(e.h, n, idx, ctypes.byref(o), None)):
            assert call() == inval and word in L.loam_last_error(), (n, lanes, L.loam_last_error())
            assert bytes(o) == before, (n, lanes)

    refused(S, None, b"not open")
    e.lanes_open(S, MAP_CAP)
    refused(0, [0], b"n must be")
    refused(S + 1, [0, 1, 2, 0], b"n must be")
    refused(2, None, b"n_lanes")
    refused(2, [0, S], b"out of range")
    refused(3, [1, 2, 1], b"twice")

    def all_empty():
        rc, s, offs = _raw(loam, e, S, None)
        return rc == loam.LOAM_OK and all(getattr(s, c).count == 0 and list(offs[c]) == [0] * (S + 1) for c in CLOUDS)

    assert all_empty()  # before the first pull
    raws = lambda k: [sweeps(s)[k] for s in (1, 2, 3)]
    e.lanes_push(raws(0))
    refused(S, None, b"in flight")
    e.lanes_pull()
    assert all_empty()  # the sweep that is not looked at
    e.lanes_step(raws(1), stamp=0.1)
    assert not all_empty()
    e.lanes_push(raws(2), stamp=0.2)
    refused(1, [1], b"in flight")
    o = e.lanes_pull()
    assert list(o["mapped"]) == [1, 1, 1]
    got = e.lanes_clouds([1])
    assert got["registered"][0].shape[0] == o["n_registered"][1] > 0
    e.lanes_close()
    refused(S, None, b"not open")
    e.close()
    _staging_limit(loam)


def _staging_limit(loam):
    """the host form's refusal of a max_points whose nine strides (5 max_points + 276 rings) exceed the
    2^21-point staging, whichever clouds are wanted: checked before the mask, so straight behind the
    open.  The sizes-only query and the device form have no staging and stay LOAM_OK."""
    L = loam.lib()
    e = loam.Engine(loam.default_config(system_delay=0, skip_frame_num=1, max_points=1 << 19), cap=1)
    assert 5 * (1 << 19) > STAGE
    e.lanes_open(1, MAP_CAP)
    room = np.full((8, 4), 3.0, np.float32)
    o = loam.LanesCloudsOut()
    ctypes.memset(ctypes.byref(o), 0xa5, ctypes.sizeof(o))
    for c in CLOUDS:
        b = getattr(o, c)
        b.pts, b.offset = None, None
    o.registered.pts, o.registered.capacity = room.ctypes.data, room.shape[0]
    before = bytes(o)
    assert L.loam_lanes_clouds(e.h, 1, None, ctypes.byref(o)) == loam.LOAM_E_INVAL
    msg = L.loam_last_error()
    assert b"2097152" in msg and b"staging" in msg, msg
    assert bytes(o) == before and np.all(room == 3.0)
    rc, s, offs = _raw(loam, e, 1, None)  # sizes only
    assert rc == loam.LOAM_OK and all(getattr(s, c).count == 0 and list(offs[c]) == [0, 0] for c in CLOUDS)
    hip = hipmem.Hip(loam)
    dev = _Dev(hip.upload(room), room.shape[0])
    offs = e.lanes_clouds_device({"registered": dev}, [0])
    assert list(offs["registered"]) == [0, 0]
    assert np.all(hip.get(dev.ptr, room.nbytes).view(np.float32) == 3.0)
    e.lanes_close()
    e.close()
    hip.release()
