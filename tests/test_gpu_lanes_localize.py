"""loam_lanes_localize: candidate poses for every listed lane's own last sweep refined
against the context's map in one call.

The specification: row (i, j) is, bit for bit (all 60 bytes), what loam_map_localize(n = 1) returns
for lane lane[i]'s transformSum, laserCloudCornerLast and laserCloudSurfLast at (aft[i][j],
bef[i][j]).  The yardstick is therefore always Engine.map_localize on a second context holding the
map, with the clouds and od_sum of a node-call context (the `clouds` fixture of
tests/test_gpu_lanes_score.py); never a second lanes_localize.

  1. S = 3 shared lanes, ragged (one lane's sweeps decimated), list [2, 0, 1], k = 3 (9 rows in a
     working set of 16), after the init step, mapping steps and pose-only steps; bef = NULL
  2. the same rows alone, at other n / k and positions, repeated, and at row counts on both sides of
     mp_small_max and mp_fused_max
  3. a run that never calls lanes_localize gives the same steps and map; map_localize on the same
     context gives the same bytes before and after
  4. own-store lanes with the map imported into the context; an empty context map
  5. a restart: refused until the init step is pulled, then the fresh context's clouds
  6. S = 65, every lane listed in descending order, k = 1
  7. 4 x 256 = LOAM_LOCALIZE_MAX rows, and more
  8. every LOAM_E_INVAL a call can be given (the mapping stack's corner bound equals the lanes' own
     capacity, so that refusal is lanes_localize_plan's to show: tests/lanes_localize_plan_check.cpp),
     each leaving `out` and the later steps as they were; a store that overflowed map_capacity
  9. Engine.lanes_relocalize(refine = 4): the lane seeded 300 m off gets the pose the same chain of
     map_score / map_localize / score_order chooses

Streams: VLP-16 synthetic loops (synthgen.stream_sweeps), the prior map M and the scratch contexts
as tests/test_gpu_lanes_shared.py has them."""
import ctypes

import numpy as np
import pytest

from test_gpu_lanes_score import _stream, clouds, yard  # noqa: F401 (fixtures)
from test_gpu_lanes_shared import (FAR, GUESS, OFF, POSE3, ZERO, _check_lane, _kw, _map_same, _open, _outs_eq, _step, prior,
                                   prior2, scratch, sweeps)  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

MD = 0.5
STREAMS3 = ("1", "2", "1d")
LIST3 = [2, 0, 1]
N3 = 6
NC = 6  # candidates of a lane: three with bef (call A), three with bef = zeros (call B: bef = NULL)


def _rec(loam, d):
    """a localize dict as one structured array: a row's 60 bytes are r[i].tobytes()"""
    r = np.zeros(d["status"].shape, loam._LOC_DTYPE)
    assert r.dtype.itemsize == 60
    for k in loam.LOCALIZE_KEYS:
        r[k] = d[k]
    return r


def _rows_eq(a, b, msg):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    for i in range(a.shape[0]):
        assert a[i].tobytes() == b[i].tobytes(), (msg, i, a[i], b[i])


def _cands(l, pulled_aft, od_sum):
    """lane l's six (aft, bef): zero, a small offset with bef = od_sum, the lane's pulled aft with
    bef = od_sum | another small offset, 300 m off (NO_LM), 450 m off (OFFGRID), these with bef zero"""
    d = np.float32(0.002 * l)
    aft = np.stack([ZERO, GUESS[1] + d, pulled_aft, GUESS[2] - d, FAR, OFF]).astype(np.float32)
    bef = np.stack([ZERO, od_sum, od_sum, ZERO, ZERO, ZERO]).astype(np.float32)
    return aft, bef


@pytest.fixture(scope="module")
def yloc(loam, prior):
    """Engine.map_localize on a second context holding M, one candidate per call"""
    eng = []

    def run(c, aft, bef=None):
        if not eng:
            eng.append(loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1)))
            assert eng[0].map_import(**_kw(prior)) == (0, 0)
        aft = np.asarray(aft, np.float32).reshape(-1, 6)
        bef = None if bef is None else np.asarray(bef, np.float32).reshape(-1, 6)
        rows = [_rec(loam, eng[0].map_localize(c["od_sum"], c["corner"], c["surf"], aft[j:j + 1],
                                               None if bef is None else bef[j:j + 1])) for j in range(aft.shape[0])]
        return np.concatenate(rows)
    yield run
    for e in eng:
        e.close()


ALONE = ((0, 1), (1, 5), (2, 2), (0, 4), (1, 0))  # (position in the list, candidate) of the rows refined alone


def _tile(A, B, i, count):
    """`count` candidates of list position i: its six, cycled"""
    j = np.arange(count) % NC
    return A[i][j][None], B[i][j][None]


@pytest.fixture(scope="module")
def run3(loam, sweeps, prior, clouds):
    """S = 3 shared lanes over streams 1, 2 and the decimated 1; localize: lanes_localize twice after
    every pulled step from the init step on (and the extra calls of tests 2 and 3 after the last)"""
    def run(localize):
        e = _open(loam, 3, prior)
        e.lanes_set_pose([2, 0], np.stack([POSE3[2], POSE3[0]]))
        outs, regs, infos, rows, cands = [], [], [], {}, {}
        extra = {}
        probe = clouds("1")[2]
        pa = np.stack([ZERO, GUESS[1]])
        for k in range(N3):
            o, r, i = _step(e, [_stream(sweeps, s)[k] for s in STREAMS3], k, range(3))
            outs.append(o)
            regs.append(r)
            infos.append(i)
            if localize and k >= 1:
                if k == 1:  # the shared working set, before lanes_localize grows it
                    extra["ml_before"] = _rec(loam, e.map_localize(probe["od_sum"], probe["corner"], probe["surf"], pa))
                ab = [_cands(l, o["aft"][l], clouds(STREAMS3[l])[k]["od_sum"]) for l in LIST3]
                A, B = np.stack([a for a, _ in ab]), np.stack([b for _, b in ab])
                first = _rec(loam, e.lanes_localize(LIST3, A[:, :3], B[:, :3]))
                second = _rec(loam, e.lanes_localize(LIST3, A[:, 3:]))
                rows[k] = np.concatenate([first, second], axis=1)
                cands[k] = (A, B)
        if localize:
            A, B = cands[N3 - 1]
            extra["ml_after"] = _rec(loam, e.map_localize(probe["od_sum"], probe["corner"], probe["surf"], pa))
            extra["again"] = _rec(loam, e.lanes_localize(LIST3, A[:, :3], B[:, :3]))
            extra["alone"] = {(i, j): _rec(loam, e.lanes_localize([LIST3[i]], A[i:i + 1, j:j + 1], B[i:i + 1, j:j + 1]))
                              for i, j in ALONE}
            extra["moved"] = _rec(loam, e.lanes_localize([1, 2], A[[2, 0]][:, 1::-1], B[[2, 0]][:, 1::-1]))  # 4 rows
            sm = e.get_tuning("mp_small_max")
            extra["small_max"] = sm
            extra["sized"] = {}
            for count in (1, sm, sm + 1, 64):
                extra["sized"][count] = _rec(loam, e.lanes_localize([LIST3[1]], *_tile(A, B, 1, count)))
            # the fused fit below and above its threshold (the default lies beyond LOAM_LOCALIZE_MAX)
            fm = sm + 2
            e.set_tuning(mp_fused_max=fm)
            assert e.get_tuning("mp_fused_max") == fm
            extra["fused"] = {count: _rec(loam, e.lanes_localize([LIST3[2]], *_tile(A, B, 2, count))) for count in (fm, fm + 1)}
        m = e.map_export()
        e.close()
        return {"res": (outs, regs, infos), "rows": rows, "cands": cands, "map": m, **extra}
    return run


@pytest.fixture(scope="module")
def done3(run3):
    return run3(True)


def test_every_kind_of_step(loam, clouds, yloc, done3):
    outs = done3["res"][0]
    rows = done3["rows"]
    assert outs[0]["status"][0] == loam.LOAM_E_NOT_READY and outs[1]["published"][0] == loam.PUB_CLOUDS  # the init step
    kinds = {("map" if outs[k]["mapped"][0] else "pose") for k in range(2, N3)}
    assert kinds == {"map", "pose"} and sorted(rows) == list(range(1, N3))
    for k in range(1, N3):
        A, B = done3["cands"][k]
        cl = {l: clouds(STREAMS3[l])[k] for l in range(3)}
        # ragged lanes: the rows' stacks are sized by the largest listed cloud, not by the row's own
        assert len({(c["corner"].shape[0], c["surf"].shape[0]) for c in cl.values()}) == 3
        for i, l in enumerate(LIST3):
            got = rows[k][i]
            _rows_eq(got[:3], yloc(cl[l], A[i, :3], B[i, :3]), f"step {k} lane {l} with bef")
            _rows_eq(got[3:], yloc(cl[l], A[i, 3:], None), f"step {k} lane {l} bef = NULL")
            assert got["status"][0] == loam.LOC_SOLVED and got["map_surf"][0] > 100 and got["iters"][0] > 0
            assert got["status"][4] == loam.LOC_NO_LM and got["aft"][4].tobytes() == FAR.tobytes()
            assert got["status"][5] == loam.LOC_OFFGRID and got["aft"][5].tobytes() == OFF.tobytes()
            for key in ("stack_corner", "stack_surf", "map_corner", "map_surf"):
                assert got[key][5] == 0, key
            assert got["stack_surf"][0] > 0 and got["stack_corner"][0] > 0
    # the lanes differ: a row is its own lane's
    last = rows[N3 - 1]
    assert last[0][0].tobytes() != last[1][0].tobytes() != last[2][0].tobytes()


def test_rows_do_not_depend_on_the_call(loam, done3):
    last = done3["rows"][N3 - 1]
    _rows_eq(done3["again"].reshape(-1), last[:, :3].reshape(-1), "a repeated call")
    for (i, j), alone in done3["alone"].items():
        assert alone.shape == (1, 1)
        _rows_eq(alone[0], last[i, j:j + 1], f"row ({i}, {j}) alone")
    moved = done3["moved"]  # lanes [1, 2] = list positions 2, 0; candidates 1, 0
    _rows_eq(moved[0], last[2][1::-1], "lane 1 in another call")
    _rows_eq(moved[1], last[0][1::-1], "lane 2 in another call")
    sm = done3["small_max"]
    assert 1 <= sm < 63  # 1 and sm take k_mp_lm_small, sm + 1 and 64 the batch fit
    for count, got in done3["sized"].items():
        assert got.shape == (1, count)
        _rows_eq(got[0], last[1][np.arange(count) % NC], f"{count} rows of one lane")
    for count, got in done3["fused"].items():
        _rows_eq(got[0], last[2][np.arange(count) % NC], f"{count} rows about mp_fused_max")


def test_nothing_is_mutated(loam, run3, done3):
    plain = run3(False)
    for l in range(3):
        _outs_eq(done3["res"], plain["res"], l, l, f"lane {l} with / without lanes_localize")
    _map_same(done3["map"], plain["map"], "the context's map with / without lanes_localize")
    assert done3["ml_before"].shape == (2,) and done3["ml_before"]["status"][0] == loam.LOC_SOLVED
    _rows_eq(done3["ml_after"], done3["ml_before"], "map_localize on the shared working set")


def test_other_maps(loam, sweeps, prior, clouds, yloc):
    ab = [_cands(l, GUESS[2], clouds(s)[2]["od_sum"]) for l, s in ((1, "2"), (0, "1"))]
    A, B = np.stack([a for a, _ in ab]), np.stack([b for _, b in ab])
    e = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    assert e.map_import(**_kw(prior)) == (0, 0)
    e.lanes_open(2, 1 << 17)
    for k in range(3):
        o = e.lanes_step([sweeps(1)[k], sweeps(2)[k]], stamp=0.1 * k)
    assert list(o["mapped"]) == [1, 1]
    got = _rec(loam, e.lanes_localize([1, 0], A, B))
    e.close()
    _rows_eq(got[0], yloc(clouds("2")[2], A[0], B[0]), "own-store lane 1")
    _rows_eq(got[1], yloc(clouds("1")[2], A[1], B[1]), "own-store lane 0")
    assert got["status"][0][0] == loam.LOC_SOLVED
    # an empty context map: no L-M anywhere, aft as given (OFFGRID where the grid ends)
    e = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    e.lanes_open(1, 1 << 17)
    for k in range(2):
        e.lanes_step([sweeps(1)[k]], stamp=0.1 * k)
    got = _rec(loam, e.lanes_localize([0], A[1][:5]))
    e.close()
    assert (got["status"] == loam.LOC_NO_LM).all() and got["aft"].tobytes() == A[1][:5].tobytes()
    assert (got["map_corner"] == 0).all() and (got["map_surf"] == 0).all()


def _raw(loam, e, lanes, aft, k, out, n=None, bef=None, lane_null=False, aft_null=False, out_null=False):
    """the C call itself: aft / bef (n k, 6) float32 arrays"""
    idx = (ctypes.c_uint32 * max(len(lanes), 1))(*lanes)
    P = ctypes.POINTER(loam.Pose6)
    return loam.lib().loam_lanes_localize(
        e.h, len(lanes) if n is None else n, None if lane_null else idx, k, None if aft_null else aft.ctypes.data_as(P),
        None if bef is None else bef.ctypes.data_as(P), None if out_null else out)


def _sentinel(loam, rows):
    out = (loam.LocalizeResult * rows)()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    return out, bytes(out)


def test_restart(loam, sweeps, prior, clouds, yloc):
    after = 3
    e = _open(loam, 2, prior)
    A = np.ascontiguousarray(np.stack([ZERO, GUESS[1], FAR]))
    out, pattern = _sentinel(loam, 3)
    init_step = None
    for k in range(8):
        if k == after:
            init_step = after + e.lanes_restart(1)
        if init_step is not None and k <= init_step:  # up to and including the push of the init step
            assert _raw(loam, e, [1], A, 3, out) == loam.LOAM_E_INVAL
            assert b"init step" in loam.lib().loam_last_error() and bytes(out) == pattern
            assert _raw(loam, e, [0], A, 3, out) == loam.LOAM_OK  # the other lane is served
            ctypes.memset(out, 0xA5, ctypes.sizeof(out))
        raws = [sweeps(2)[k], sweeps(2)[k]]
        if init_step is not None:
            raws[1] = sweeps(1)[0] if k < init_step else sweeps(1)[1 + k - init_step]
        o = e.lanes_step(raws, stamp=0.1 * k)
        if init_step is not None and k >= init_step:
            assert o["status"][1] == 0
            fresh = clouds("1", delay=0)[1 + k - init_step]  # (the fresh context's sweep 0 is not looked at)
            _rows_eq(_rec(loam, e.lanes_localize([1], A))[0], yloc(fresh, A), f"restarted lane, step {k}")
            if k > init_step + 1:
                break
    assert init_step is not None and k > init_step
    e.close()


def test_65_lanes(loam, sweeps, prior, clouds, yloc):
    S = 65
    names = ("1", "2", "3")
    e = _open(loam, S, prior)
    for k in range(3):
        o = e.lanes_step([sweeps(int(names[l % 3]))[k] for l in range(S)], stamp=0.1 * k)
    assert (o["status"] == 0).all()
    lanes = list(range(S - 1, -1, -1))
    A = np.stack([GUESS[1 + l % 2] + np.float32(0.001 * (l % 3)) for l in lanes])[:, None, :].astype(np.float32)
    B = np.stack([clouds(names[l % 3])[2]["od_sum"] for l in lanes])[:, None, :].astype(np.float32)
    got = _rec(loam, e.lanes_localize(lanes, A, B))
    e.close()
    assert got.shape == (S, 1)
    for l in (0, 31, 64):
        i = lanes.index(l)
        _rows_eq(got[i], yloc(clouds(names[l % 3])[2], A[i], B[i]), f"lane {l}")
        assert got["status"][i][0] == loam.LOC_SOLVED
    for l in range(6, S):  # lanes that share a stream and the candidate
        _rows_eq(got[lanes.index(l)], got[lanes.index(l % 6)], f"lanes {l} and {l % 6}")
    assert got[lanes.index(0)].tobytes() != got[lanes.index(1)].tobytes()


def test_the_row_limit(loam, sweeps, prior, clouds, yloc):
    S, k = 4, loam.LOCALIZE_MAX // 4
    names = ("1", "2", "1d", "2")
    rng = np.random.default_rng(32)
    A = (rng.uniform(-1, 1, (k, 6)) * np.array([0.03, 0.03, 0.03, 0.2, 0.2, 0.2])).astype(np.float32)
    e = _open(loam, S, prior)
    for s in range(3):
        o = e.lanes_step([_stream(sweeps, nm)[s] for nm in names], stamp=0.1 * s)
    assert (o["status"] == 0).all()
    got = _rec(loam, e.lanes_localize([3, 2, 1, 0], A))  # (k, 6): the same candidates for every lane
    assert got.shape == (S, k)
    for i, l in enumerate([3, 2, 1, 0]):
        _rows_eq(got[i][[0, k - 1]], yloc(clouds(names[l])[2], A[[0, k - 1]]), f"lane {l}")
    assert (got["status"] == loam.LOC_SOLVED).all()
    big = np.zeros((loam.LOCALIZE_MAX + 4, 6), np.float32)
    out, pattern = _sentinel(loam, 4)
    assert _raw(loam, e, [0], big, loam.LOCALIZE_MAX + 1, out) == loam.LOAM_E_INVAL
    assert _raw(loam, e, [0, 1], big, loam.LOCALIZE_MAX // 2 + 1, out) == loam.LOAM_E_INVAL
    assert _raw(loam, e, [0, 1, 2, 3], big, k + 1, out) == loam.LOAM_E_INVAL
    assert _raw(loam, e, [0, 1, 2], big, 0x55555556, out) == loam.LOAM_E_INVAL  # (n x k wraps to 2 in 32 bits)
    assert b"LOAM_LOCALIZE_MAX" in loam.lib().loam_last_error()
    assert bytes(out) == pattern
    e.close()


def test_every_invalid_call_changes_nothing(loam, sweeps, prior, clouds):
    n, at = 8, 5
    INVAL = loam.LOAM_E_INVAL
    L = loam.lib()
    A = np.ascontiguousarray(np.tile(np.stack([ZERO, GUESS[1], GUESS[2], FAR]), (6, 1)))
    out, pattern = _sentinel(loam, 24)

    def refused(eng, lanes, k=2, **kw):
        rc = _raw(loam, eng, lanes, A, k, out, **kw)
        assert rc == INVAL and L.loam_last_error() and bytes(out) == pattern, (lanes, k, kw)

    closed = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    refused(closed, [0])  # lanes not open
    closed.close()

    def run(calls):
        e = _open(loam, 3, prior)
        if calls:
            refused(e, [0])  # before the first pull
        e.lanes_set_pose([0, 1], np.stack([POSE3[0], GUESS[2]]))
        outs, regs, infos = [], [], []
        for k in range(n):
            raws = [sweeps(1)[k], sweeps(2)[k], sweeps(3)[k] if k != 3 else np.zeros((0, 4), np.float32)]
            if k == 1 and calls:
                assert outs[0]["status"][0] == loam.LOAM_E_NOT_READY
                refused(e, [0])  # inside system_delay: pulled steps, none of them the init step
            if k == at:
                assert outs[-1]["status"][2] == INVAL  # lane 2 has failed (the empty sweep)
                if calls:
                    for lanes, kw in (([0], dict(n=0)), ([0, 1, 2, 0], dict(n=4)), ([0], dict(k=0)), ([0, 1], dict(k=513)),
                                      ([0, 3], {}), ([1, 0xffffffff], {}), ([1, 0, 1], {}), ([0, 2], {}),
                                      ([0], dict(lane_null=True)), ([0], dict(aft_null=True)), ([0, 1], dict(bef=A, k=513))):
                        refused(e, lanes, **kw)
                    assert _raw(loam, e, [0], A, 2, out, out_null=True) == INVAL
                assert e.lanes_restart(2) >= 0
                if calls:
                    refused(e, [0, 2])  # lane 2 waits for its init step
                    assert b"init step" in L.loam_last_error()
                e.lanes_push(raws, stamp=0.1 * k)
                if calls:
                    refused(e, [0])  # a step in flight
                    assert b"in flight" in L.loam_last_error()
                o = e.lanes_pull()
                r = {l: e.lanes_registered(l) for l in range(2) if o["mapped"][l]}
                i = e.lanes_localize_info()
            else:
                o, r, i = _step(e, raws, k, range(2))
            outs.append(o)
            regs.append(r)
            infos.append(i)
        if calls:  # the calls above were refused, this one (the list's upper bounds, bef given) is not
            assert _raw(loam, e, [1, 0], A, 12, out, bef=A) == loam.LOAM_OK and bytes(out) != pattern
            ctypes.memset(out, 0xA5, ctypes.sizeof(out))
        e.close()
        return outs, regs, infos

    with_calls, without = run(True), run(False)
    assert sum(int(o["mapped"][0]) for o in without[0]) >= 3
    for l in range(2):
        _outs_eq(with_calls, without, l, l, f"lane {l} with / without the refused calls")
    # a map whose last update overflowed map_capacity
    small = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1, map_capacity=1024))
    small.lanes_open(1, 4096)
    for k in range(2):
        small.lanes_step([sweeps(1)[k]], stamp=0.1 * k)
    c = clouds("1")[1]
    assert _raw(loam, small, [0], A, 2, out) == loam.LOAM_OK  # (the empty map is served)
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    with pytest.raises(loam.LoamError) as ei:  # the frame's map update does not fit 1024 points
        small.mapping(c["od_sum"], c["corner"], c["surf"], c["full"])
    assert ei.value.code == loam.LOAM_E_CAPACITY
    refused(small, [0])
    assert b"map_capacity" in L.loam_last_error()
    small.close()


def test_lanes_relocalize_refined(loam, sweeps, prior, scratch, clouds, yard, yloc):
    n, at, m = 7, 2, 4
    grid = np.stack([GUESS[2], np.array([0, 0, 0, 0.5, 0, 0], np.float32), ZERO, GUESS[1],
                     np.array([0, 0.05, 0, 0, -0.5, 0], np.float32), np.array([0, 0, 0, 0, 0, 0.6], np.float32)])
    e = _open(loam, 2, prior)
    e.lanes_set_pose([0, 1], np.stack([GUESS[1], FAR]))
    outs, regs, infos = [], [], []
    for k in range(n):
        o, r, i = _step(e, [sweeps(2)[k], sweeps(1)[k]], k, range(2))
        outs.append(o)
        regs.append(r)
        infos.append(i)
        if k == at:
            assert o["mapped"][1] == 1 and i["status"][1] == loam.LOC_NO_LM
            rel0 = e.lanes_relocalize([1], grid, o["od_sum"], MD)  # refine = 0: the unrefined function
            rel = e.lanes_relocalize([1], grid, o["od_sum"], MD, refine=m)
    e.close()
    c = clouds("1")[at]
    od_sum = outs[at]["od_sum"][1]
    assert od_sum.tobytes() == c["od_sum"].tobytes()
    # the same chain on the yardstick contexts
    coarse = yard(c, grid)
    order = loam.score_order({key: coarse[key] for key in loam.SCORE_KEYS})
    assert sorted(rel0) == ["aft", "index", "score"] and rel0["index"].tolist() == [int(order[0])]
    assert rel0["aft"].tobytes() == grid[order[0]][None, :].tobytes()
    assert _srec(loam, rel0["score"])[0].tobytes() == coarse[order[0]].tobytes()
    idx = order[:m]
    loc = yloc(c, grid[idx], np.tile(od_sum, (m, 1)))
    fine = coarse[idx].copy()
    ok = np.flatnonzero(loc["status"] == loam.LOC_SOLVED)
    assert ok.size >= 2
    fine[ok] = yard(c, loc["aft"][ok])
    best = loam.score_order({key: fine[key] for key in loam.SCORE_KEYS}, idx)[0]
    assert rel["rows"].tolist() == [idx.tolist()] and rel["index"].tolist() == [int(idx[best])]
    _rows_eq(_rec(loam, rel["localize"])[0], loc, "the refined rows")
    _rows_eq(_srec(loam, rel["coarse"])[0], coarse[idx], "coarse")
    _rows_eq(_srec(loam, rel["fine"])[0], fine, "fine")
    chosen = loc["aft"][best]
    assert rel["aft"].tobytes() == chosen[None, :].tobytes()
    assert loc["status"][best] == loam.LOC_SOLVED and chosen.tobytes() != grid[idx[best]].tobytes()
    assert _srec(loam, rel["score"])[0].tobytes() == fine[best].tobytes()
    later = [k for k in range(at + 1, n) if outs[k]["mapped"][1]]
    assert len(later) >= 2 and all(infos[k]["status"][1] == loam.LOC_SOLVED for k in later)
    recs = scratch("s1+M far, relocalized and refined", sweeps(1)[:n], {0: prior},
                   {0: (FAR, ZERO), at + 1: (chosen, od_sum)})
    assert _check_lane(loam, outs, regs, 1, recs) >= 3
    assert all(recs[k]["mp_iters"] > 0 for k in later)


def _srec(loam, d):
    """a score dict as one structured array (32-byte rows)"""
    r = np.zeros(d["corner_in"].shape, loam._SCORE_DTYPE)
    for k in loam.SCORE_KEYS:
        r[k] = d[k]
    return r
