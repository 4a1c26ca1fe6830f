"""loam_lanes_map_commit: the listed shared lanes' last frames enter the context's map.

The specification: per kind and cube, content = M's ++ the stack points of the listed lanes in list
order; the cubes of the union of the lanes' valid sets go through one PCL VoxelGrid.  Two yardsticks,
both independent of the commit kernels: the scratch context of tests/test_gpu_lanes_shared.py (a
streaming context that imported M with the lane's poses and was given the lane's sweeps: what n = 1
must leave), and a host restatement (`_restate`: cube_keys of tests/test_gpu_map.py, concatenation,
the oracle's voxel_grid per union cube) on the lanes' stacks as the hook loam_dev_lanes_commit_input
returns them; test 2 pins the restatement to the scratch context.  Everything is compared bit for bit.

  1. n = 1 against the scratch context
  2. the restatement against the scratch context
  3. overlapping lanes: [2, 0, 1] and [0, 1, 2] against their restatements, and they differ
  4. disjoint lanes commute
  5. the lanes, then the context's own chain_sweep, go on in the new map
  6. map_capacity exactly reached, and one point short (nothing changes)
  7. S = 65: all 65 lanes in one commit, and a 3-lane sublist (both hash forms of lane_from_capacity)
  8. every LOAM_E_INVAL, each leaving the map and the next step as they were
"""
import ctypes

import numpy as np
import pytest

from test_gpu_lanes_restart import _same
from test_gpu_lanes_shared import (FAR, FROM_CAP, GUESS, OFF, POSE3, SEEDS3, ZERO, _check_lane, _kw, _map_same,  # noqa: F401
                                   _step, prior, scratch, sweeps)
from test_gpu_map import cube_keys
from vg_cases import oracle_vg

pytestmark = pytest.mark.gpu

CUBES = 21 * 11 * 21
LEAF = {"corner": 0.2, "surf": 0.4}
KINDS = ("corner", "surf")


def _engine(loam, S, m, from_cap=FROM_CAP, **cfg):
    e = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1, **cfg))
    assert e.map_import(**_kw(m)) == (0, 0)
    e.lanes_open_shared(S, from_cap)
    return e


def _to_map_step(e, raws_of, lanes, outs, regs, k0=0):
    """steps from k0 on up to and including the next mapping step; returns its index"""
    for k in range(k0, 12):
        o, r, _ = _step(e, raws_of(k), k, lanes)
        outs.append(o)
        regs.append(r)
        if o["mapped"].any():
            return k
    raise AssertionError("no mapping step")


def _hook(loam, e, lane):
    """(corner [nC, 4], surf [nS, 4], valid cubes) of a lane: loam_dev_lanes_commit_input"""
    f = loam.lib().loam_dev_lanes_commit_input
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 5
    c = np.zeros((120 * int(e.cfg.n_rings), 4), np.float32)
    s = np.zeros((int(e.cap), 4), np.float32)
    n = np.zeros(2, np.uint32)
    v = np.full(125, -1, np.int32)
    nv = ctypes.c_uint32(0)
    rc = f(e.h, lane, c.ctypes.data, s.ctypes.data, n.ctypes.data, v.ctypes.data, ctypes.addressof(nv))
    assert rc == 0, loam.lib().loam_last_error()
    return {"corner": c[:n[0]].copy(), "surf": s[:n[1]].copy(), "valid": v[:nv.value].copy()}


def _restate(m, inputs, vg):
    """the commit of `inputs` (hook outputs, in list order) into the export m, on the host.  Returns the
    new corner / surf clouds with their cube offsets, the loam_commit_result counts and the largest
    VoxelGrid input (`vin`: the points of the union's cubes before downsampling, both kinds)"""
    union = sorted({int(c) for i in inputs for c in i["valid"]})
    out = {"center": m["center"], "vin": 0, "inserted": [], "outside": [], "map_points": [], "cubes": len(union)}
    for kind in KINDS:
        off = m[kind + "_offset"].astype(np.int64)
        content = {c: [m[kind][off[c]:off[c + 1]]] for c in range(CUBES) if off[c + 1] > off[c]}
        ins = outs = 0
        for i in inputs:
            key = cube_keys(i[kind], m["center"])
            ins += int((key >= 0).sum())
            outs += int((key < 0).sum())
            for c in np.unique(key[key >= 0]):
                content.setdefault(int(c), []).append(i[kind][key == c])  # (stack order inside the cube)
        parts, noff = [], np.zeros(CUBES + 1, np.int64)
        for c in range(CUBES):
            pts = np.concatenate(content[c]) if c in content else np.zeros((0, 4), np.float32)
            if c in union and len(pts):
                out["vin"] += len(pts)
                pts = vg(pts, LEAF[kind])
            parts.append(pts)
            noff[c + 1] = noff[c] + len(pts)
        out[kind] = np.concatenate(parts).astype(np.float32).reshape(-1, 4)
        out[kind + "_offset"] = noff.astype(np.uint32)
        out["inserted"].append(ins)
        out["outside"].append(outs)
        out["map_points"].append(int(noff[-1]))
    return out


def _points_same(a, b, msg):
    """the clouds, the cube offsets and the centre of two maps (an export or a restatement)"""
    for kind in KINDS:
        np.testing.assert_array_equal(a[kind + "_offset"], b[kind + "_offset"], err_msg=f"{msg} {kind} offsets")
        _same(a[kind], b[kind], f"{msg} {kind}")
    np.testing.assert_array_equal(a["center"], b["center"], err_msg=msg)


def _result_same(r, want, msg):
    for f in ("inserted", "outside", "map_points"):
        assert tuple(r[f]) == tuple(want[f]), (msg, f, r[f], want[f])
    assert r["cubes"] == want["cubes"], msg


def _scratch_map(loam, seq, m, aft0):
    """the scratch context of a lane (import of m with the lane's current poses in front of every
    sweep), exported behind its first mapping sweep: m with that one sweep committed"""
    e = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    aft, bef = aft0, ZERO
    for k, sw in enumerate(seq):
        e.map_import(**_kw(m, aft=aft, bef=bef))
        rc, pub, od, a, b, _ = e.chain_sweep(sw, stamp=0.1 * k)
        if a is not None:
            out = e.map_export()
            e.close()
            return k, out
    raise AssertionError("no mapping sweep")


def _raws3(sweeps):
    return lambda k: [sweeps(s)[k] for s in SEEDS3]


def _open3(loam, sweeps, prior, **cfg):
    """test_gpu_lanes_shared's three lanes (seeds 1, 2, 1, two guesses and a lane at zero) up to and
    including their first mapping step"""
    e = _engine(loam, 3, prior, **cfg)
    e.lanes_set_pose([2, 0], np.stack([POSE3[2], POSE3[0]]))
    run = {"e": e, "outs": [], "regs": []}
    run["km"] = _to_map_step(e, _raws3(sweeps), range(3), run["outs"], run["regs"])
    assert list(run["outs"][-1]["mapped"]) == [1, 1, 1] and list(run["outs"][-1]["status"]) == [0, 0, 0]
    return run


@pytest.fixture(scope="module")
def vg(oc):
    return oracle_vg(oc)


@pytest.fixture(scope="module")
def single(loam, sweeps, prior):
    """tests 1 and 2: lane 1 committed alone behind the first mapping step"""
    run = _open3(loam, sweeps, prior)
    e = run["e"]
    run["before"] = e.map_export()
    run["in1"] = _hook(loam, e, 1)
    run["res"] = e.lanes_map_commit([1])
    run["after"] = e.map_export()
    e.close()
    km, run["yard"] = _scratch_map(loam, sweeps(SEEDS3[1]), prior, ZERO)
    assert km == run["km"]
    return run


def test_one_lane_against_its_scratch_context(loam, single):
    before, after, yard = single["before"], single["after"], single["yard"]
    _points_same(after, yard, "commit([1]) against lane 1's scratch context")
    for f in ("aft", "bef"):
        _same(after[f], before[f], f"the context's {f}")
    assert after["surround_phase"] == before["surround_phase"]
    assert not np.array_equal(after["surf_offset"], before["surf_offset"])  # (the map did change)
    i = single["in1"]
    keys = [cube_keys(i[k], before["center"]) for k in KINDS]
    want = {"inserted": [int((q >= 0).sum()) for q in keys], "outside": [int((q < 0).sum()) for q in keys],
            "map_points": [after[k].shape[0] for k in KINDS], "cubes": len(set(i["valid"].tolist()))}
    _result_same(single["res"], want, "loam_commit_result")
    assert want["inserted"][1] > 100 and want["cubes"] > 0 and len(i["valid"]) == want["cubes"]


def test_the_restatement_against_the_scratch_context(single, vg):
    re = _restate(single["before"], [single["in1"]], vg)
    _points_same(re, single["yard"], "the restatement of commit([1]) against lane 1's scratch context")
    _result_same(single["res"], re, "loam_commit_result against the restatement")


@pytest.fixture(scope="module")
def overlap(loam, sweeps, prior, vg):
    """test 3's first run, kept open for test 5: commit([2, 0, 1]) behind the first mapping step"""
    run = _open3(loam, sweeps, prior)
    e = run["e"]
    run["before"] = e.map_export()
    run["inputs"] = [_hook(loam, e, l) for l in range(3)]
    run["res"] = e.lanes_map_commit([2, 0, 1])
    run["after"] = e.map_export()
    run["restated"] = _restate(run["before"], [run["inputs"][l] for l in (2, 0, 1)], vg)
    yield run
    e.close()


def test_overlapping_lanes_in_list_order(loam, sweeps, prior, vg, overlap):
    _points_same(overlap["after"], overlap["restated"], "commit([2, 0, 1])")
    _result_same(overlap["res"], overlap["restated"], "commit([2, 0, 1])")
    _map_same(dict(overlap["after"], corner=overlap["before"]["corner"], surf=overlap["before"]["surf"],
                   corner_offset=overlap["before"]["corner_offset"], surf_offset=overlap["before"]["surf_offset"]),
              overlap["before"], "everything but the points")
    run = _open3(loam, sweeps, prior)
    e = run["e"]
    inputs = [_hook(loam, e, l) for l in range(3)]
    for a, b in zip(inputs, overlap["inputs"]):  # (the same frames in both runs)
        for f in a:
            _same(a[f], b[f], f)
    res = e.lanes_map_commit([0, 1, 2])
    after = e.map_export()
    e.close()
    re = _restate(overlap["before"], inputs, vg)
    _points_same(after, re, "commit([0, 1, 2])")
    _result_same(res, re, "commit([0, 1, 2])")
    # the list's order is the order inside a cube: the lanes share cubes, so the two maps differ
    assert any(after[k].shape != overlap["after"][k].shape or
               not np.array_equal(after[k].view(np.uint32), overlap["after"][k].view(np.uint32)) for k in KINDS)


def test_disjoint_lanes_commute(loam, sweeps, prior, vg):
    def run():
        e = _engine(loam, 2, prior)
        e.lanes_set_pose([0, 1], np.stack([GUESS[1], FAR]))
        outs, regs = [], []
        _to_map_step(e, lambda k: [sweeps(1)[k], sweeps(2)[k]], range(2), outs, regs)
        return e
    e = run()
    info = e.lanes_localize_info()
    assert info["status"][0] == loam.LOC_SOLVED and info["status"][1] == loam.LOC_NO_LM
    before = e.map_export()
    near, far = _hook(loam, e, 0), _hook(loam, e, 1)
    touched = [set(np.concatenate([cube_keys(i[k], before["center"]) for k in KINDS]).tolist()) - {-1} for i in (near, far)]
    sets = [set(i["valid"].tolist()) | t for i, t in zip((near, far), touched)]
    assert touched[0] and touched[1] and len(far["valid"]) > 0
    assert not (sets[0] & sets[1])  # valid sets and touched cubes are disjoint
    both = e.lanes_map_commit([0, 1])
    after = e.map_export()
    e.close()
    e = run()
    first = e.lanes_map_commit([0])
    second = e.lanes_map_commit([1])
    after2 = e.map_export()
    e.close()
    re = _restate(before, [near, far], vg)
    _points_same(after, re, "commit([near, far])")
    _points_same(after2, after, "commit([near]) then commit([far])")
    _result_same(both, re, "commit([near, far])")
    assert second["map_points"] == both["map_points"] and first["cubes"] + second["cubes"] == both["cubes"]
    assert tuple(np.add(first["inserted"], second["inserted"])) == both["inserted"]


def test_the_lanes_go_on_in_the_new_map(loam, sweeps, prior, scratch, overlap):
    e, km, outs, regs = overlap["e"], overlap["km"], overlap["outs"], overlap["regs"]
    n = km + 5
    for k in range(km + 1, n):
        o, r, _ = _step(e, _raws3(sweeps)(k), k, range(3))
        outs.append(o)
        regs.append(r)
    for l in range(3):
        recs = scratch(f"s{SEEDS3[l]}+M g{l}, committed@{km + 1}", sweeps(SEEDS3[l])[:n], {0: prior, km + 1: overlap["after"]},
                       {0: (POSE3.get(l, ZERO), ZERO)})
        assert _check_lane(loam, outs, regs, l, recs) >= 3
        assert any(r["aft"] is not None and r["mp_iters"] > 0 for r in recs[km + 1:])
    _map_same(e.map_export(), overlap["after"], "the map after four more steps")
    K = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    assert K.map_import(**_kw(overlap["after"])) == (0, 0)
    mapped = 0
    for k, sw in enumerate(sweeps(3)[:5]):
        ra, rb = e.chain_sweep(sw, stamp=0.1 * k, registered=True), K.chain_sweep(sw, stamp=0.1 * k, registered=True)
        for x, y in zip(ra, rb):
            assert (x is None) == (y is None), k
            if x is not None:
                _same(np.asarray(x, np.float32), np.asarray(y, np.float32), f"chain_sweep {k}")
        mapped += ra[3] is not None
    assert mapped >= 1
    _map_same(e.map_export(), K.map_export(), "the maps after the context's own sweeps")
    K.close()


def test_capacity(loam, sweeps, prior, overlap):
    re = overlap["restated"]
    need = max(re["vin"], sum(re["map_points"]))
    print("required map_capacity", need, "VoxelGrid input", re["vin"], "new map", re["map_points"])
    run = _open3(loam, sweeps, prior, map_capacity=need)
    res = run["e"].lanes_map_commit([2, 0, 1])
    _points_same(run["e"].map_export(), overlap["after"], "map_capacity = the required size")
    _result_same(res, re, "map_capacity = the required size")
    run["e"].close()
    # one point less: nothing changes
    plain = _open3(loam, sweeps, prior, map_capacity=need - 1)  # the uncommitted run
    run = _open3(loam, sweeps, prior, map_capacity=need - 1)
    e = run["e"]
    before = e.map_export()
    with pytest.raises(loam.LoamError) as err:
        e.lanes_map_commit([2, 0, 1])
    assert err.value.code == loam.LOAM_E_CAPACITY
    assert sum(err.value.commit["map_points"]) == need
    _map_same(e.map_export(), before, "the map after LOAM_E_CAPACITY")
    k = run["km"] + 1
    a, b = _step(e, _raws3(sweeps)(k), k, range(3)), _step(plain["e"], _raws3(sweeps)(k), k, range(3))
    assert list(a[0]["status"]) == [0, 0, 0]
    for f in a[0]:
        _same(a[0][f], b[0][f], f"the step behind LOAM_E_CAPACITY {f}")
    assert a[2].tobytes() == b[2].tobytes()
    for l in a[1]:
        _same(a[1][l], b[1][l], f"registered {l}")
    e.close()
    plain["e"].close()


@pytest.mark.parametrize("from_cap", [FROM_CAP, 8192])
def test_65_lanes(loam, sweeps, prior, vg, from_cap):
    """more listed lanes than a wave, more lanes than a wave's dense keys: all 65 lanes in one commit,
    and a 3-lane sublist of the same frames on a second run; lane_from_capacity above / at 8192 (the
    lanes' frames under both hash forms, the second in M thinned to at most 8192 points)"""
    S, seeds = 65, (1, 2, 3)
    aft = (np.arange(S, dtype=np.float32)[:, None] * np.array([1, -1, 1, 2, -2, 2], np.float32) * np.float32(1e-3))
    if from_cap == 8192:
        step = -(-(prior["corner"].shape[0] + prior["surf"].shape[0]) // 8192)
        prior = dict(prior, corner=prior["corner"][::step], surf=prior["surf"][::step])
        assert prior["corner"].shape[0] + prior["surf"].shape[0] <= 8192 and prior["surf"].shape[0] > 1000

    def run():
        e = _engine(loam, S, prior, from_cap)
        e.lanes_set_pose(list(range(S)), aft)
        outs = []
        _to_map_step(e, lambda k: [sweeps(seeds[l % 3])[k] for l in range(S)], (), outs, [])
        assert (outs[-1]["status"] == 0).all() and (outs[-1]["mapped"] == 1).all()
        return e, e.map_export()
    e, before = run()
    order = list(range(S - 1, S - 33, -1)) + list(range(S - 32))  # every lane once, not ascending
    assert sorted(order) == list(range(S))
    inputs = {l: _hook(loam, e, l) for l in range(S)}
    res = e.lanes_map_commit(order)
    after = e.map_export()
    e.close()
    re = _restate(before, [inputs[l] for l in order], vg)
    _points_same(after, re, "all 65 lanes")
    _result_same(res, re, "all 65 lanes")
    assert res["inserted"][1] > 65 * 100
    e, before2 = run()
    _points_same(before2, before, "the second run's map")
    sub = [64, 3, 31]
    res = e.lanes_map_commit(sub)
    after = e.map_export()
    e.close()
    re = _restate(before, [inputs[l] for l in sub], vg)
    _points_same(after, re, "the sublist")
    _result_same(res, re, "the sublist")


def test_every_invalid_call_changes_nothing(loam, sweeps, prior):
    INVAL = loam.LOAM_E_INVAL
    L = loam.lib()
    out = loam.CommitResult()
    ctypes.memset(ctypes.byref(out), 0xa5, ctypes.sizeof(out))
    untouched = bytes(out)

    def commit(eng, lanes, count=None, lane_null=False, out_null=False):
        idx = (ctypes.c_uint32 * max(len(lanes), 1))(*lanes)
        rc = L.loam_lanes_map_commit(eng.h, len(lanes) if count is None else count, None if lane_null else idx,
                                     None if out_null else ctypes.byref(out))
        assert bytes(out) == untouched
        return rc

    def refused(eng, lanes, word, **kw):
        assert commit(eng, lanes, **kw) == INVAL, (lanes, kw)
        assert word.encode() in L.loam_last_error(), (lanes, kw, L.loam_last_error())
    closed = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    refused(closed, [0], "not open")
    closed.lanes_open(2, 4096)  # own-store lanes write their maps themselves
    refused(closed, [0], "loam_lanes_open")
    closed.close()
    raws = lambda k: [sweeps(1)[k], sweeps(2)[k], sweeps(1)[k], sweeps(3)[k]]  # noqa: E731

    def start():
        """lanes 0 (a guess) and 2 (zero) map, lane 1 stands where a frame would recentre the grid,
        lane 3 fails on its second sweep"""
        e = _engine(loam, 4, prior)
        e.lanes_set_pose([0, 1], np.stack([GUESS[1], OFF]))
        return e
    e, twin = start(), start()
    refused(e, [0], "no step was pulled")
    km = None
    for k in range(12):
        rk = raws(k)
        if k == 1:
            rk[3] = np.zeros((0, 4), np.float32)
        e.lanes_push(rk, stamp=0.1 * k)
        refused(e, [0], "in flight")
        o = e.lanes_pull()
        twin.lanes_step(rk, stamp=0.1 * k)
        if o["mapped"].any():
            km = k
            break
        refused(e, [0], "ran no mapping frame")  # inside system_delay, the init step, a step that does not map
    assert km is not None and o["status"][3] == INVAL
    info = e.lanes_localize_info()
    assert list(info["status"][:3]) == [loam.LOC_SOLVED, loam.LOC_OFFGRID, loam.LOC_SOLVED]
    before = e.map_export()
    refused(e, [0], "null", lane_null=True)
    refused(e, [0], "null", out_null=True)
    refused(e, [0], "n must be", count=0)
    refused(e, [0, 2, 1, 3, 0], "n must be")
    refused(e, [0, 4], "out of range")
    refused(e, [2, 0xffffffff], "out of range")
    refused(e, [0, 2, 0], "listed twice")
    refused(e, [2, 2], "listed twice")
    refused(e, [0, 3], "has failed")
    refused(e, [0, 1], "LOAM_LOC_OFFGRID")
    hook = L.loam_dev_lanes_commit_input
    hook.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 5
    buf = np.zeros((int(e.cap), 4), np.float32)
    w = np.zeros(128, np.int32)
    for lane in (1, 3, 4):  # the hook refuses what the commit refuses
        assert hook(e.h, lane, buf.ctypes.data, buf.ctypes.data, w.ctypes.data, w.ctypes.data, w.ctypes.data) == INVAL
    _map_same(e.map_export(), before, "the map after the refusals")
    # a frame enters the map once (checked on a second pair of engines, since the commit changes the map)
    c = start()
    for k in range(km + 1):
        rk = raws(k)
        if k == 1:
            rk[3] = np.zeros((0, 4), np.float32)
        c.lanes_step(rk, stamp=0.1 * k)
    c.lanes_map_commit([2])
    once = c.map_export()
    refused(c, [2], "enters the map once")
    refused(c, [0, 2], "enters the map once")
    assert hook(c.h, 2, buf.ctypes.data, buf.ctypes.data, w.ctypes.data, w.ctypes.data, w.ctypes.data) == INVAL
    _map_same(c.map_export(), once, "the map after the second commit of a frame")
    c.lanes_map_commit([0])  # (lane 0's frame is still new)
    c.close()
    # a restarted lane waits for its init step
    e.lanes_restart(2)
    twin.lanes_restart(2)
    refused(e, [2], "init step")
    _map_same(e.map_export(), before, "the map after the refusals")
    for k in range(km + 1, km + 3):
        a, b = _step(e, raws(k), k, range(3)), _step(twin, raws(k), k, range(3))
        for f in a[0]:
            _same(a[0][f], b[0][f], f"step {k} behind the refusals {f}")
        assert a[2].tobytes() == b[2].tobytes()
        for l in a[1]:
            _same(a[1][l], b[1][l], f"step {k} registered {l}")
    e.close()
    twin.close()


def test_an_overflowed_store_is_refused(loam, sweeps, prior):
    """the context's own update overflows map_capacity behind the lanes' mapping step: the store is not
    valid (loam_map_export refuses it too), and so is a commit into it"""
    total = prior["corner"].shape[0] + prior["surf"].shape[0]
    e = _engine(loam, 1, prior, map_capacity=total + 64)
    e.lanes_set_pose([0], GUESS[1])
    outs, regs = [], []
    _to_map_step(e, lambda k: [sweeps(1)[k]], range(1), outs, regs)
    assert outs[-1]["status"][0] == 0
    for k, sw in enumerate(sweeps(3)[:4]):
        try:
            e.chain_sweep(sw, stamp=0.1 * k)
        except loam.LoamError as err:  # (a deferred update overflows behind the call that enqueued it:
            assert err.code == loam.LOAM_E_CAPACITY  # the refused export below is the precondition)
    with pytest.raises(loam.LoamError) as err:
        e.map_export()
    assert err.value.code == loam.LOAM_E_INVAL
    with pytest.raises(loam.LoamError) as err:
        e.lanes_map_commit([0])
    assert err.value.code == loam.LOAM_E_INVAL and "exceeded map_capacity" in str(err.value)
    e.close()
