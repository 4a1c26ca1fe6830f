"""loam_lanes_score: pose guesses for every listed lane's own last sweep scored
against the context's whole map in one call.

The specification: row (i, j) is, bit for bit (all 32 bytes), what loam_map_score returns for lane
lane[i]'s laserCloudCornerLast / laserCloudSurfLast at pose[i][j].  The yardstick is therefore always
Engine.map_score on a second context holding the map, with the clouds of a node-call context
(scan_registration + odometry, skip_frame_num = 0: loam_odometry publishes the Last clouds on every
frame, and neither node depends on that setting) fed the lane's sweeps; never a second lanes_score.

  1. S = 3 shared lanes, ragged (one lane's sweeps decimated), list [2, 0, 1], six poses per lane,
     after the init step, pose-only steps and mapping steps
  2. a row alone, a repeated call, and a run that never scores
  3. own-store lanes with the map imported into the context; an empty context map
  4. a restart: refused until the init step is pulled, then the init frame's raw clouds
  5. the context imports another map between two calls
  6. S = 65, every lane listed in descending order
  7. n x k = LOAM_SCORE_MAX, and one row more
  8. every LOAM_E_INVAL, each leaving `out` and the lanes as they were
  9. Engine.lanes_relocalize: a lane seeded 300 m off comes back

Streams: VLP-16 synthetic loops (synthgen.stream_sweeps), the prior map M and the scratch contexts
as tests/test_gpu_lanes_shared.py has them."""
import ctypes

import numpy as np
import pytest

from test_gpu_lanes_shared import (FAR, FROM_CAP, GUESS, POSE3, ZERO, _check_lane, _kw, _map_same, _open, _outs_eq, _step,
                                   prior, prior2, scratch, sweeps)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

MD = 0.5           # max_dist of most calls: r2 = 0.25 exactly
TILE = 1024        # query points of one tile (score.hpp kScoreTile)
STREAMS3 = ("1", "2", "1d")
LIST3 = [2, 0, 1]
N3 = 6


def _stream(sweeps, name):
    """stream "<seed>" of the shared test, "<seed>d" the same sweeps with every second point"""
    seq = sweeps(int(name[0]))
    return [sw[::2] for sw in seq] if name.endswith("d") else seq


def _rec(loam, d):
    """a score dict as one structured array: a row's 32 bytes are r[i].tobytes()"""
    r = np.zeros(d["corner_in"].shape, loam._SCORE_DTYPE)
    assert r.dtype.itemsize == 32
    for k in loam.SCORE_KEYS:
        r[k] = d[k]
    return r


def _rows_eq(a, b, msg):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    for i in range(a.shape[0]):
        assert a[i].tobytes() == b[i].tobytes(), (msg, i, a[i], b[i])


def _poses(l):
    """six poses, different per lane: zero, two small offsets, 300 m off, a NaN in tx, about 1 rad"""
    d = np.float32(0.002 * l)
    nan = np.array([0, 0, 0, np.nan, 0, 0], np.float32)
    rot = np.array([0.3, 1.0 + 0.1 * l, -0.2, 0.5, 0.1, -0.3], np.float32)
    return np.stack([ZERO, GUESS[1] + d, GUESS[2] - d, FAR, nan, rot]).astype(np.float32)


def _tiles(c):
    return -(-c["corner"].shape[0] // TILE) + -(-c["surf"].shape[0] // TILE)


@pytest.fixture(scope="module")
def clouds(loam, sweeps):
    """the yardstick's clouds: per sweep of a stream what loam_odometry leaves in corner_last /
    surf_last on a node-call context (None inside system_delay).  Cached by (stream, delay)."""
    cache = {}

    def get(stream, delay=1, n=N3):
        key = (stream, delay)
        if key not in cache or len(cache[key]) < n:
            A = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=0))
            recs = []
            for k, sw in enumerate(_stream(sweeps, stream)[:n]):
                rc, f = A.scan_registration(sw, stamp=0.1 * k)
                if rc != 0:
                    assert rc == loam.LOAM_E_NOT_READY
                    recs.append(None)
                    continue
                pub, pose, cl, sl, full = A.odometry(f, stamp=0.1 * k)
                assert pub & loam.PUB_CLOUDS  # (skip_frame_num = 0: every frame publishes them)
                recs.append({"corner": cl, "surf": sl, "full": full, "od_sum": pose})
            A.close()
            cache[key] = recs
        return cache[key]
    return get


@pytest.fixture(scope="module")
def yard(loam, prior, prior2):
    """Engine.map_score on a second context holding M (which = 2: the shuffled M of test 5)"""
    eng = {}

    def score(c, poses, max_dist=MD, which=1):
        if which not in eng:
            eng[which] = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
            assert eng[which].map_import(**_kw(prior if which == 1 else prior2)) == (0, 0)
        return _rec(loam, eng[which].map_score(c["corner"], c["surf"], np.asarray(poses, np.float32).reshape(-1, 6), max_dist))
    yield score
    for e in eng.values():
        e.close()


ALONE = ((0, 1), (1, 5), (2, 2), (0, 4), (1, 3))  # (position in the list, pose) of the rows scored alone


@pytest.fixture(scope="module")
def run3(loam, sweeps, prior):
    """S = 3 shared lanes over streams 1, 2 and the decimated 1; score: lanes_score after every
    pulled step from the init step on (and the extra calls of test 2 after the last)"""
    P = np.stack([_poses(l) for l in LIST3])

    def run(score):
        e = _open(loam, 3, prior)
        e.lanes_set_pose([2, 0], np.stack([POSE3[2], POSE3[0]]))
        outs, regs, infos, scores = [], [], [], {}
        for k in range(N3):
            o, r, i = _step(e, [_stream(sweeps, s)[k] for s in STREAMS3], k, range(3))
            outs.append(o)
            regs.append(r)
            infos.append(i)
            if score and k >= 1:
                scores[k] = _rec(loam, e.lanes_score(LIST3, P, MD))
        extra = {}
        if score:
            extra["again"] = _rec(loam, e.lanes_score(LIST3, P, MD))
            extra["alone"] = {(i, j): _rec(loam, e.lanes_score([LIST3[i]], P[i:i + 1, j:j + 1], MD)) for i, j in ALONE}
            extra["moved"] = _rec(loam, e.lanes_score([1, 2], P[[2, 0]][:, ::-1], MD))  # other n, k, positions
        m = e.map_export()
        e.close()
        return {"res": (outs, regs, infos), "scores": scores, "map": m, "P": P, **extra}
    return run


@pytest.fixture(scope="module")
def scored3(run3):
    return run3(True)


def test_every_kind_of_step(loam, clouds, yard, scored3):
    outs = scored3["res"][0]
    P, scores = scored3["P"], scored3["scores"]
    assert outs[0]["status"][0] == loam.LOAM_E_NOT_READY and outs[1]["published"][0] == loam.PUB_CLOUDS  # the init step
    kinds = {("map" if outs[k]["mapped"][0] else "pose") for k in range(2, N3)}
    assert kinds == {"map", "pose"} and sorted(scores) == list(range(1, N3))
    for k in range(1, N3):
        cl = {l: clouds(STREAMS3[l])[k] for l in range(3)}
        # ragged lanes, and a cloud of several tiles
        assert _tiles(cl[2]) != _tiles(cl[0]) and max(c["surf"].shape[0] for c in cl.values()) > 2 * TILE
        for i, l in enumerate(LIST3):
            want = yard(cl[l], P[i])
            _rows_eq(scores[k][i], want, f"step {k} lane {l}")
            got = scores[k][i]
            n_c, n_s = cl[l]["corner"].shape[0], cl[l]["surf"].shape[0]
            assert (got["corner_scored"] == n_c).all() and (got["surf_scored"] == n_s).all()
            for j in (3, 4):  # 300 m off, NaN: no inlier, cost = scored x r2
                assert got["corner_in"][j] == 0 and got["surf_in"][j] == 0
                assert got["corner_cost"][j] == n_c * 0.25 and got["surf_cost"][j] == n_s * 0.25
            assert got["surf_in"][0] > 100  # the zero pose lies in M


def test_independence_and_no_side_effect(loam, run3, scored3):
    last = scored3["scores"][N3 - 1]
    _rows_eq(scored3["again"].reshape(-1), last.reshape(-1), "a repeated call")
    for (i, j), alone in scored3["alone"].items():
        assert alone.shape == (1, 1)
        _rows_eq(alone[0], last[i, j:j + 1], f"row ({i}, {j}) alone")
    moved = scored3["moved"]  # lanes [1, 2] = list positions 2, 0, poses reversed
    _rows_eq(moved[0], last[2][::-1], "lane 1 in another call")
    _rows_eq(moved[1], last[0][::-1], "lane 2 in another call")
    plain = run3(False)
    for l in range(3):
        _outs_eq(scored3["res"], plain["res"], l, l, f"lane {l} with / without scoring")
    _map_same(scored3["map"], plain["map"], "the context's map with / without scoring")


def test_own_store_lanes(loam, sweeps, prior, clouds, yard):
    P = np.stack([_poses(1)[:3], _poses(0)[:3]])
    e = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    assert e.map_import(**_kw(prior)) == (0, 0)
    e.lanes_open(2, 1 << 17)
    for k in range(3):
        o = e.lanes_step([sweeps(1)[k], sweeps(2)[k]], stamp=0.1 * k)
    assert list(o["mapped"]) == [1, 1]
    got = _rec(loam, e.lanes_score([1, 0], P, MD))
    e.close()
    _rows_eq(got[0], yard(clouds("2")[2], P[0]), "own-store lane 1")
    _rows_eq(got[1], yard(clouds("1")[2], P[1]), "own-store lane 0")
    # an empty context map
    e = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    e.lanes_open(1, 1 << 17)
    for k in range(2):
        e.lanes_step([sweeps(1)[k]], stamp=0.1 * k)
    got = e.lanes_score([0], _poses(0), 1.0)
    e.close()
    c = clouds("1")[1]
    for kind in ("corner", "surf"):
        assert (got[kind + "_scored"] == c[kind].shape[0]).all() and c[kind].shape[0] > 0
        assert (got[kind + "_in"] == 0).all()
        assert (got[kind + "_cost"] == c[kind].shape[0] * 1.0).all()


def _raw_score(loam, e, lanes, poses, k, out, n=None, max_dist=MD, lane_null=False, pose_null=False, out_null=False):
    """the C call itself: poses an (n k, 6) float32 array"""
    idx = (ctypes.c_uint32 * max(len(lanes), 1))(*lanes)
    return loam.lib().loam_lanes_score(
        e.h, len(lanes) if n is None else n, None if lane_null else idx, max_dist, k,
        None if pose_null else poses.ctypes.data_as(ctypes.POINTER(loam.Pose6)), None if out_null else out)


def _sentinel(loam, rows):
    out = (loam.ScoreResult * rows)()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    return out, bytes(out)


def test_restart(loam, sweeps, prior, clouds, yard):
    after = 3
    e = _open(loam, 2, prior)
    P = _poses(1)
    out, pattern = _sentinel(loam, 6)
    init_step = None
    for k in range(8):
        if k == after:
            init_step = after + e.lanes_restart(1)
        if init_step is not None and k <= init_step:  # up to and including the push of the init step
            assert _raw_score(loam, e, [1], P, 6, out) == loam.LOAM_E_INVAL
            assert b"init step" in loam.lib().loam_last_error() and bytes(out) == pattern
            assert _raw_score(loam, e, [0], P, 6, out) == loam.LOAM_OK  # the other lane is served
            ctypes.memset(out, 0xA5, ctypes.sizeof(out))
        raws = [sweeps(2)[k], sweeps(2)[k]]
        if init_step is not None:
            raws[1] = sweeps(1)[0] if k < init_step else sweeps(1)[1 + k - init_step]
        o = e.lanes_step(raws, stamp=0.1 * k)
        if init_step is not None and k >= init_step:
            assert o["status"][1] == 0
            fresh = clouds("1", delay=0)[1 + k - init_step]  # (the fresh context's sweep 0 is not looked at)
            _rows_eq(_rec(loam, e.lanes_score([1], P, MD))[0], yard(fresh, P), f"restarted lane, step {k}")
            if k == init_step:
                assert o["published"][1] == loam.PUB_CLOUDS
            if k > init_step + 1:
                break
    assert init_step is not None and k > init_step
    e.close()


def test_the_map_changes_between_two_calls(loam, sweeps, prior, prior2, clouds, yard):
    e = _open(loam, 2, prior)
    for k in range(3):
        e.lanes_step([sweeps(1)[k], sweeps(2)[k]], stamp=0.1 * k)
    P = np.stack([_poses(0), _poses(1)])
    first = _rec(loam, e.lanes_score([0, 1], P, MD))
    assert e.map_import(**_kw(prior2)) == (0, 0)
    second = _rec(loam, e.lanes_score([0, 1], P, MD))
    e.close()
    for i, s in enumerate(("1", "2")):
        _rows_eq(first[i], yard(clouds(s)[2], P[i]), f"lane {i} in M")
        _rows_eq(second[i], yard(clouds(s)[2], P[i], which=2), f"lane {i} in the second map")
    # (the same points in another order: the nearest distances stay, the index differs)
    assert (first["surf_in"] == second["surf_in"]).all()


def test_65_lanes(loam, sweeps, prior, clouds, yard):
    S = 65
    names = ("1", "2", "3")
    e = _open(loam, S, prior)
    for k in range(3):
        o = e.lanes_step([sweeps(int(names[l % 3]))[k] for l in range(S)], stamp=0.1 * k)
    assert (o["status"] == 0).all()
    P = _poses(0)[[0, 1, 5]]
    lanes = list(range(S - 1, -1, -1))
    got = _rec(loam, e.lanes_score(lanes, P, MD))
    e.close()
    assert got.shape == (S, 3)
    for l in (0, 31, 64):
        _rows_eq(got[lanes.index(l)], yard(clouds(names[l % 3])[2], P), f"lane {l}")
    for l in range(3, S):  # lanes that share a stream and the poses
        _rows_eq(got[lanes.index(l)], got[lanes.index(l % 3)], f"lanes {l} and {l % 3}")
    assert got[lanes.index(0)].tobytes() != got[lanes.index(1)].tobytes()


def test_the_size_limit(loam, sweeps, prior, clouds, yard):
    S, k = 4, loam.SCORE_MAX // 4
    names = ("1", "2", "1d", "2")
    rng = np.random.default_rng(31)
    P = (rng.uniform(-1, 1, (k, 6)) * np.array([0.05, 0.05, 0.05, 0.5, 0.5, 0.5])).astype(np.float32)
    e = _open(loam, S, prior)
    for s in range(3):
        o = e.lanes_step([_stream(sweeps, nm)[s] for nm in names], stamp=0.1 * s)
    assert (o["status"] == 0).all()
    got = _rec(loam, e.lanes_score([3, 2, 1, 0], P, MD))
    assert got.shape == (S, k)
    for i, l in enumerate([3, 2, 1, 0]):
        _rows_eq(got[i][[0, k - 1]], yard(clouds(names[l])[2], P[[0, k - 1]]), f"lane {l}")
    big = np.zeros((loam.SCORE_MAX + 1, 6), np.float32)
    out, pattern = _sentinel(loam, 4)
    assert _raw_score(loam, e, [0], big, loam.SCORE_MAX + 1, out) == loam.LOAM_E_INVAL
    assert _raw_score(loam, e, [0, 1], big, loam.SCORE_MAX // 2 + 1, out) == loam.LOAM_E_INVAL
    assert _raw_score(loam, e, [0, 1, 2], big, 0x55555556, out) == loam.LOAM_E_INVAL  # (n x k wraps to 2 in 32 bits)
    assert bytes(out) == pattern
    e.close()


def test_every_invalid_call_changes_nothing(loam, sweeps, prior, scratch, clouds):
    n, at = 8, 5
    INVAL = loam.LOAM_E_INVAL
    L = loam.lib()
    P = np.ascontiguousarray(np.tile(_poses(0), (4, 1)))
    out, pattern = _sentinel(loam, 24)

    def refused(eng, lanes, k=2, **kw):
        rc = _raw_score(loam, eng, lanes, P, k, out, **kw)
        assert rc == INVAL and L.loam_last_error() and bytes(out) == pattern, (lanes, k, kw)

    closed = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    refused(closed, [0])  # lanes not open
    closed.close()
    e = _open(loam, 3, prior)
    refused(e, [0])  # before the first pull
    e.lanes_set_pose([0, 1], np.stack([POSE3[0], GUESS[2]]))
    outs, regs = [], []
    for k in range(n):
        raws = [sweeps(1)[k], sweeps(2)[k], sweeps(3)[k] if k != 3 else np.zeros((0, 4), np.float32)]
        if k == 1:
            assert outs[0]["status"][0] == loam.LOAM_E_NOT_READY
            refused(e, [0])  # inside system_delay: pulled steps, none of them the init step
        if k == at:
            assert outs[-1]["status"][2] == INVAL  # lane 2 has failed (the empty sweep)
            for lanes, kw in (([0], dict(n=0)), ([0, 1, 2, 0], dict(n=4)), ([0], dict(k=0)), ([0, 1], dict(k=32769)),
                              ([0, 3], {}), ([1, 0xffffffff], {}), ([1, 0, 1], {}), ([0, 2], {}),
                              ([0], dict(max_dist=0.0)), ([0], dict(max_dist=-0.5)), ([0], dict(max_dist=1.5)),
                              ([0], dict(max_dist=float("nan"))), ([0], dict(lane_null=True)), ([0], dict(pose_null=True))):
                refused(e, lanes, **kw)
            assert _raw_score(loam, e, [0], P, 2, out, out_null=True) == INVAL
            assert e.lanes_restart(2) >= 0
            refused(e, [0, 2])  # lane 2 waits for its init step
            assert b"init step" in L.loam_last_error()
            e.lanes_push(raws, stamp=0.1 * k)
            refused(e, [0])  # a step in flight
            o = e.lanes_pull()
            r = {l: e.lanes_registered(l) for l in range(2) if o["mapped"][l]}
        else:
            o, r, _ = _step(e, raws, k, range(2))
        outs.append(o)
        regs.append(r)
    # the calls above were refused, this one (max_dist exactly 1, the list's upper bounds) is not
    assert _raw_score(loam, e, [1, 0], P, 12, out, max_dist=1.0) == loam.LOAM_OK and bytes(out) != pattern
    e.close()
    for l, s, a in ((0, 1, POSE3[0]), (1, 2, GUESS[2])):
        recs = scratch(f"s{s}+M inval {l}", sweeps(s)[:n], {0: prior}, {0: (a, ZERO)})
        assert _check_lane(loam, outs, regs, l, recs) >= 3
    # a map whose last update overflowed map_capacity
    small = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1, map_capacity=1024))
    small.lanes_open(1, 4096)
    for k in range(2):
        small.lanes_step([sweeps(1)[k]], stamp=0.1 * k)
    c = clouds("1")[1]
    assert _raw_score(loam, small, [0], P, 2, out) == loam.LOAM_OK  # (the empty map is served)
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    with pytest.raises(loam.LoamError) as ei:  # the frame's map update does not fit 1024 points
        small.mapping(c["od_sum"], c["corner"], c["surf"], c["full"])
    assert ei.value.code == loam.LOAM_E_CAPACITY
    refused(small, [0])
    assert b"map_capacity" in L.loam_last_error()
    small.close()


def test_lanes_relocalize(loam, sweeps, prior, scratch, clouds, yard):
    n, at = 7, 2
    grid = np.stack([GUESS[2], np.array([0, 0, 0, 0.5, 0, 0], np.float32), ZERO, GUESS[1],
                     np.array([0, 0.05, 0, 0, -0.5, 0], np.float32), np.array([0, 0, 0, 0, 0, 0.6], np.float32)])
    e = _open(loam, 2, prior)
    e.lanes_set_pose([0, 1], np.stack([GUESS[1], FAR]))
    outs, regs, infos = [], [], []
    rel = None
    for k in range(n):
        o, r, i = _step(e, [sweeps(2)[k], sweeps(1)[k]], k, range(2))
        outs.append(o)
        regs.append(r)
        infos.append(i)
        if k == at:
            assert o["mapped"][1] == 1 and i["status"][1] == loam.LOC_NO_LM
            rel = e.lanes_relocalize([1], grid, o["od_sum"], MD)
    e.close()
    want = yard(clouds("1")[at], grid)
    order = loam.score_order({key: want[key] for key in loam.SCORE_KEYS})
    assert rel["index"].tolist() == [int(order[0])]
    chosen = grid[order[0]]
    assert rel["aft"].tobytes() == chosen[None, :].tobytes()
    assert _rec(loam, rel["score"])[0].tobytes() == want[order[0]].tobytes()
    later = [k for k in range(at + 1, n) if outs[k]["mapped"][1]]
    assert len(later) >= 2 and all(infos[k]["status"][1] == loam.LOC_SOLVED for k in later)
    recs = scratch("s1+M far, relocalized", sweeps(1)[:n], {0: prior},
                   {0: (FAR, ZERO), at + 1: (chosen, outs[at]["od_sum"][1])})
    assert _check_lane(loam, outs, regs, 1, recs) >= 3
    assert all(recs[k]["mp_iters"] > 0 for k in later)
