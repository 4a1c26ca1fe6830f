"""loam_lanes_map_import: one saved map into n lanes between two steps.

The specification: a listed lane behaves from the call on exactly as the context of the lanes'
equivalence (a fresh context fed the lane's sweeps through loam_chain_sweep) would, had that context
received loam_map_import(in with aft = aft[i]) at the same point of its call sequence: every later
step's status, flags, poses, iteration counts and registered cloud, and the exported map, bit for
bit; no unlisted lane changes by a bit.  Every yardstick is such a streaming context, never a second
lanes run.  The prior map M is made here: a fresh context over stream 1, exported.

  1. before the first push, two lanes with two pose guesses in one call
  2. mid-run with pool_cur 1 and 0, right after a mapping and after a non-mapping step; a shuffled
     cloud with points outside the grid and NaNs, another centre
  3. after a restart: refused until the lane's init step is pulled, then equal to a fresh
     system_delay = 0 context that imported before its first sweep; a restart before the shared init
     frame clears an imported map
  4. one call for three lanes / for all 65 lanes (the batch launch forms) against single contexts
  5. lane_map_capacity exactly reached, and exceeded by one point
  6. a cloud of more than one upload chunk
  7. two empty clouds: a map reset that keeps the given poses
  8. every LOAM_E_INVAL, each leaving the lanes as they were

Streams: VLP-16 synthetic loops (synthgen.stream_sweeps), as tests/test_gpu_lanes.py."""
import ctypes

import numpy as np
import pytest

from test_gpu_lanes_restart import _map_eq, _same, _step_eq

pytestmark = pytest.mark.gpu

MAP_CAP = 1 << 17
N_SWEEPS = 12
GUESS = np.array([[0, 0, 0, 0, 0, 0], [0.01, -0.02, 0.015, 0.05, -0.03, 0.04], [-0.015, 0.01, 0.02, -0.04, 0.02, 0.06]],
                 np.float32)  # Aft guesses: M's start pose (zero) and small offsets from it
ZERO = np.zeros(6, np.float32)


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
    sweeps `imports` names ({k: map_import's keywords}; k = len(seq): behind the last sweep).
    Returns one record per sweep, the final map and {k: (dropped, the map exported straight after)}.
    Cached by `key`, which names the sweeps and the imports."""
    cache = {}

    def run(key, seq, delay, skip, imports=None):
        key = (key, len(seq), delay, skip)
        if key in cache:
            return cache[key]
        e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
        recs, imp = [], {}
        for k in range(len(seq) + 1):
            if imports and k in imports:
                dropped = e.map_import(**imports[k])
                imp[k] = (dropped, e.map_export())
            if k == len(seq):
                break
            rc, pub, od, aft, bef, reg = e.chain_sweep(seq[k], stamp=0.1 * k, registered=True)
            rec = {"rc": rc, "pub": pub, "od_sum": od, "aft": aft, "bef": bef, "reg": reg}
            if rc == 0 and aft is None:
                rec["od_iters"] = e.stats()["od_iters"]
            if aft is not None:
                rec["mp_iters"] = e.stats()["mp_iters"]
            recs.append(rec)
        cache[key] = (recs, e.map_export(), imp)
        e.close()
        return cache[key]
    return run


@pytest.fixture(scope="module")
def prior(sweeps, ctx):
    """M: the map a fresh context built over stream 1"""
    m = ctx("s1", sweeps(1), 1, 1)[1]
    assert m["corner"].shape[0] > 1000 and m["surf"].shape[0] > 1000
    return m


def _kw(m, **over):
    kw = {k: m[k] for k in ("corner", "surf", "center", "surround_phase", "aft", "bef")}
    kw.update(over)
    return kw


def _step(e, raws, k, lanes):
    o = e.lanes_step(raws, stamp=0.1 * k)
    return o, {l: e.lanes_registered(l) for l in lanes if o["mapped"][l] and o["status"][l] == 0}


def _raw(loam, e, lanes, kw, n=None, mutate=None):
    """loam_lanes_map_import through ctypes: (rc, dropped), dropped preset to (7, 8)"""
    m, keep = e._map_in(kw["corner"], kw["surf"], kw["center"], kw["surround_phase"], kw["aft"], kw["bef"])
    if mutate:
        mutate(m)
    idx = (ctypes.c_uint32 * max(len(lanes), 1))(*lanes)
    dropped = (ctypes.c_uint64 * 2)(7, 8)
    rc = loam.lib().loam_lanes_map_import(e.h, len(lanes) if n is None else n, idx, ctypes.byref(m), None, dropped)
    return rc, (int(dropped[0]), int(dropped[1]))


def _check_lane(loam, outs, regs, l, recs, first=0, shift=0, upto=None):
    """lane l's steps [first, upto) against recs[k + shift]; returns the number that mapped"""
    mapped = 0
    for k in range(first, len(outs) if upto is None else upto):
        mapped += _step_eq(loam, outs[k], regs[k], l, recs[k + shift], f"lane {l} step {k}")
    return mapped


def test_before_the_first_push(loam, sweeps, ctx, prior):
    """S = 3: M into lanes [2, 0] with two guesses before anything was pushed; lane 1 gets nothing"""
    n, delay, skip = 8, 1, 1
    seeds = (1, 2, 1)
    e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
    e.lanes_open(3, MAP_CAP)
    dropped = e.lanes_map_import([2, 0], **_kw(prior, aft=GUESS[[0, 1]], bef=ZERO))
    first = {l: e.lanes_map_export(l) for l in range(3)}
    outs, regs = [], []
    for k in range(n):
        o, r = _step(e, [sweeps(s)[k] for s in seeds], k, range(3))
        outs.append(o)
        regs.append(r)
    maps = {l: e.lanes_map_export(l) for l in range(3)}
    e.close()
    plain, _, _ = ctx("s1", sweeps(1)[:n], delay, skip)
    for l, g in ((2, 0), (0, 1)):
        recs, cmap, imp = ctx(f"s1+M@0g{g}", sweeps(1)[:n], delay, skip, {0: _kw(prior, aft=GUESS[g], bef=ZERO)})
        # not vacuous: the first mapping frame in the imported map ran its L-M, and not to the pose
        # the same context reaches without the map
        km = next(k for k, r in enumerate(recs) if r["aft"] is not None)
        assert recs[km]["mp_iters"] > 0
        assert not np.array_equal(recs[km]["aft"].view(np.uint32), plain[km]["aft"].view(np.uint32))
        assert dropped == imp[0][0]
        _map_eq(first[l], imp[0][1], f"lane {l} straight after the import")
        assert _check_lane(loam, outs, regs, l, recs) >= 3
        _map_eq(maps[l], cmap, f"lane {l} map")
    recs, cmap, _ = ctx("s2", sweeps(2)[:n], delay, skip)
    assert first[1]["corner"].shape[0] == 0 and first[1]["surf"].shape[0] == 0
    _check_lane(loam, outs, regs, 1, recs)
    _map_eq(maps[1], cmap, "lane 1 map")


def _spoiled(m, seed):
    """M shuffled, with points outside every grid and points with a NaN coordinate mixed in"""
    rng = np.random.default_rng(seed)
    out = {}
    for name, far, nan in (("corner", 37, 11), ("surf", 53, 17)):
        a = m[name].copy()
        f = rng.uniform(-20, 20, (far, 4)).astype(np.float32)
        f[:, rng.integers(0, 3)] = 1e5
        q = a[rng.integers(0, a.shape[0], nan)].copy()
        q[np.arange(nan), rng.integers(0, 3, nan)] = np.nan
        a = np.concatenate([a, f, q])
        out[name] = a[rng.permutation(a.shape[0])]
    return out


@pytest.mark.parametrize("at", [3, 6])
def test_mid_run_both_pools(loam, sweeps, ctx, prior, at):
    """system_delay = 1, skip_frame_num = 1: steps 2, 4, 6, ... map.  at = 3: one mapping step done
    (pool_cur = 1), straight behind it; at = 6: two done (pool_cur = 0), behind a step that did not map"""
    n, delay, skip = 10, 1, 1
    seeds = (2, 1, 3)
    kw = _kw(prior, center=(11, 5, 9), **_spoiled(prior, at))
    recs, cmap, imp = ctx(f"s1+spoiled@{at}", sweeps(1)[:n], delay, skip, {at: kw})
    assert imp[at][0] == (37 + 11, 53 + 17)
    e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
    e.lanes_open(3, MAP_CAP)
    outs, regs = [], []
    for k in range(n):
        if k == at:
            assert outs[k - 1]["mapped"][1] == (1 if at == 3 else 0)
            assert e.lanes_map_import([1], **kw) == imp[at][0]
            _map_eq(e.lanes_map_export(1), imp[at][1], "lane 1 straight after the import")
        o, r = _step(e, [sweeps(s)[k] for s in seeds], k, range(3))
        outs.append(o)
        regs.append(r)
    maps = {l: e.lanes_map_export(l) for l in range(3)}
    e.close()
    assert _check_lane(loam, outs, regs, 1, recs, first=at) >= 2
    _check_lane(loam, outs, regs, 1, recs, upto=at)
    _map_eq(maps[1], cmap, "lane 1 map")
    for l in (0, 2):
        recs, cmap, _ = ctx(f"s{seeds[l]}", sweeps(seeds[l])[:n], delay, skip)
        _check_lane(loam, outs, regs, l, recs)
        _map_eq(maps[l], cmap, f"lane {l} map")


@pytest.mark.parametrize("skip,after", [(1, 5), (1, 6), (0, 5)])
def test_after_a_restart(loam, sweeps, ctx, prior, skip, after):
    """lane 1 (stream 2) is restarted before step `after` and then runs stream 1 from D[1] on.  The
    import is refused until the lane's init step has been pulled; from then on the lane is a fresh
    system_delay = 0 context that imported before its first sweep"""
    n, delay = 12, 1
    kw = _kw(prior, aft=GUESS[1], bef=ZERO)
    e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
    e.lanes_open(3, MAP_CAP)
    outs, regs = [], []
    init_step = None
    for k in range(n):
        if k == after:
            wait = e.lanes_restart(1)
            assert wait == (0 if (skip, after) != (1, 6) else 1)
            init_step = after + wait
        if init_step is not None and k <= init_step:  # up to and including the push of the init step
            before = e.lanes_map_export(1)
            rc, dropped = _raw(loam, e, [1], kw)
            assert rc == loam.LOAM_E_INVAL and dropped == (7, 8)
            assert b"init step" in loam.lib().loam_last_error()
            _map_eq(e.lanes_map_export(1), before, f"lane 1 after the refused import of step {k}")
        if init_step is not None and k == init_step + 1:
            assert e.lanes_map_import([1], **kw) == (0, 0)
        raws = [sweeps(2)[k], sweeps(2)[k], sweeps(3)[k]]
        if init_step is not None:
            raws[1] = sweeps(1)[0] if k < init_step else sweeps(1)[1 + k - init_step]
        o, r = _step(e, raws, k, range(3))
        outs.append(o)
        regs.append(r)
    maps = {l: e.lanes_map_export(l) for l in range(3)}
    e.close()
    recs, cmap, _ = ctx("s1+M@0g1", sweeps(1)[:1 + n - init_step], 0, skip, {0: kw})
    assert recs[0]["rc"] == loam.LOAM_E_NOT_READY and recs[1]["pub"] == loam.PUB_CLOUDS
    for k in range(after, init_step):
        assert outs[k]["status"][1] == loam.LOAM_E_NOT_READY
    assert _check_lane(loam, outs, regs, 1, recs, first=init_step, shift=1 - init_step) >= 2
    _map_eq(maps[1], cmap, "lane 1 map")
    for l, s in ((0, 2), (2, 3)):
        recs, cmap, _ = ctx(f"s{s}", sweeps(s)[:n], delay, skip)
        _check_lane(loam, outs, regs, l, recs)
        _map_eq(maps[l], cmap, f"lane {l} map")


def test_restart_before_the_shared_init_clears_an_import(loam, sweeps, ctx, prior):
    """inside system_delay a restart has nothing to wait for; the map an import put there goes"""
    n, delay, skip = 6, 2, 1
    e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
    e.lanes_open(2, MAP_CAP)
    e.lanes_map_import([0, 1], **_kw(prior, aft=GUESS[1], bef=ZERO))
    assert e.lanes_restart(1) == 2
    m = e.lanes_map_export(1)
    assert m["corner"].shape[0] == 0 and m["surf"].shape[0] == 0 and list(m["center"]) == [10, 5, 10]
    assert not m["aft"].any() and not m["bef"].any() and m["surround_phase"] == 4
    outs, regs = [], []
    for k in range(n):
        o, r = _step(e, [sweeps(1)[k], sweeps(2)[k]], k, range(2))
        outs.append(o)
        regs.append(r)
    maps = {l: e.lanes_map_export(l) for l in range(2)}
    e.close()
    recs, cmap, _ = ctx("s1+M@0g1", sweeps(1)[:n], delay, skip, {0: _kw(prior, aft=GUESS[1], bef=ZERO)})
    _check_lane(loam, outs, regs, 0, recs)
    _map_eq(maps[0], cmap, "lane 0 map")
    recs, cmap, _ = ctx("s2", sweeps(2)[:n], delay, skip)
    _check_lane(loam, outs, regs, 1, recs)
    _map_eq(maps[1], cmap, "lane 1 map")


def test_three_lanes_in_one_call(loam, sweeps, ctx, prior):
    """S = 5: lanes [4, 1, 3] with three guesses in one call against three contexts"""
    n, delay, skip = 8, 1, 1
    listed = [4, 1, 3]
    seeds = (2, 1, 3, 1, 1)
    e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
    e.lanes_open(5, MAP_CAP)
    e.lanes_map_import(listed, **_kw(prior, aft=GUESS, bef=ZERO))
    outs, regs = [], []
    for k in range(n):
        o, r = _step(e, [sweeps(s)[k] for s in seeds], k, range(5))
        outs.append(o)
        regs.append(r)
    maps = {l: e.lanes_map_export(l) for l in range(5)}
    e.close()
    for g, l in enumerate(listed):
        recs, cmap, _ = ctx(f"s1+M@0g{g}", sweeps(1)[:n], delay, skip, {0: _kw(prior, aft=GUESS[g], bef=ZERO)})
        assert _check_lane(loam, outs, regs, l, recs) >= 3
        _map_eq(maps[l], cmap, f"lane {l} map")
    for l in (0, 2):
        recs, cmap, _ = ctx(f"s{seeds[l]}", sweeps(seeds[l])[:n], delay, skip)
        _check_lane(loam, outs, regs, l, recs)
        _map_eq(maps[l], cmap, f"lane {l} map")


def test_all_of_65_lanes(loam, sweeps, ctx, prior):
    """S = 65 (the launch forms change at 64): one call for every lane, each with its own guess"""
    S, n, delay, skip = 65, 4, 1, 0
    aft = (np.arange(S, dtype=np.float32)[:, None] * np.array([1, -1, 1, 2, -2, 2], np.float32) * np.float32(1e-3))
    sample = (0, 31, 64)
    e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
    e.lanes_open(S, MAP_CAP)
    e.lanes_map_import(list(range(S)), **_kw(prior, aft=aft, bef=ZERO))
    first = [e.lanes_map_export(l) for l in range(S)]
    for l in range(S):
        _same(first[l]["aft"], aft[l], f"lane {l} aft")
        _map_eq(dict(first[l], aft=first[0]["aft"]), first[0], f"lane {l} against lane 0 straight after the import")
    outs, regs = [], []
    for k in range(n):
        o, r = _step(e, [sweeps(1)[k]] * S, k, sample)
        outs.append(o)
        regs.append(r)
    maps = {l: e.lanes_map_export(l) for l in sample}
    e.close()
    for l in sample:
        recs, cmap, imp = ctx(f"s1+M@0a{l}", sweeps(1)[:n], delay, skip, {0: _kw(prior, aft=aft[l], bef=ZERO)})
        _map_eq(first[l], imp[0][1], f"lane {l} straight after the import")
        assert _check_lane(loam, outs, regs, l, recs) >= 2
        _map_eq(maps[l], cmap, f"lane {l} map")


def _in_grid(rng, n):
    """n points well inside the default grid (cubes of 50 m, 21 x 11 x 21 about (10, 5, 10))"""
    a = rng.uniform(-100, 100, (n, 4)).astype(np.float32)
    a[:, 3] = rng.uniform(0, 16, n).astype(np.float32)
    return a


def _far(rng, n):
    a = _in_grid(rng, n)
    a[:, 0] = 1e5
    return a


def test_capacity_edge(loam, ctx):
    """lane_map_capacity = 4096: exactly 4096 kept points fit, 4097 are LOAM_E_CAPACITY and nothing changes"""
    rng = np.random.default_rng(5)
    corner = np.concatenate([_in_grid(rng, 1500), _far(rng, 40)])
    surf = np.concatenate([_far(rng, 60), _in_grid(rng, 2596)])
    kw = dict(corner=corner, surf=surf, center=(10, 5, 10), surround_phase=2, aft=GUESS[1], bef=GUESS[2])
    _, _, imp = ctx("cap4096", [], 1, 1, {0: kw})
    e = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    e.lanes_open(2, 4096)
    assert e.lanes_map_import([1, 0], **kw) == imp[0][0] == (40, 60)
    maps = [e.lanes_map_export(l) for l in range(2)]
    for l in range(2):
        assert maps[l]["corner"].shape[0] + maps[l]["surf"].shape[0] == 4096
        _map_eq(maps[l], imp[0][1], f"lane {l}")
    over = dict(kw, corner=np.concatenate([corner, _in_grid(rng, 1)]), aft=ZERO, surround_phase=0)
    rc, dropped = _raw(loam, e, [0, 1], over)
    assert rc == loam.LOAM_E_CAPACITY and dropped == (40, 60)
    for l in range(2):
        _map_eq(e.lanes_map_export(l), maps[l], f"lane {l} after LOAM_E_CAPACITY")
    e.close()


def test_chunk_boundary(loam, ctx):
    """2^21 + 1500 corner points (two upload chunks), about 3000 of them inside the grid, in both chunks"""
    rng = np.random.default_rng(6)
    n = (1 << 21) + 1500
    corner = np.empty((n, 4), np.float32)
    corner[:] = _far(rng, 1)[0]
    inside = np.concatenate([rng.choice(1 << 21, 2300, replace=False), (1 << 21) + rng.choice(1500, 700, replace=False)])
    corner[inside] = _in_grid(rng, inside.shape[0])
    kw = dict(corner=corner, surf=_in_grid(rng, 500), center=(10, 5, 10), surround_phase=4, aft=GUESS[2], bef=ZERO)
    _, _, imp = ctx("chunks", [], 1, 1, {0: kw})
    assert imp[0][0] == (n - 3000, 0) and imp[0][1]["corner"].shape[0] == 3000
    e = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    e.lanes_open(2, MAP_CAP)
    assert e.lanes_map_import([1], **kw) == imp[0][0]
    _map_eq(e.lanes_map_export(1), imp[0][1], "lane 1")
    assert e.lanes_map_export(0)["corner"].shape[0] == 0
    e.close()


def test_reset(loam, sweeps, ctx):
    """two empty clouds into a running lane: an empty map, the given poses, and on as the context"""
    n, delay, skip, at = 10, 1, 1, 6
    empty = np.zeros((0, 4), np.float32)
    kw = dict(corner=empty, surf=empty, center=(10, 5, 10), surround_phase=1, aft=GUESS[1], bef=GUESS[2])
    recs, cmap, imp = ctx(f"s1+reset@{at}", sweeps(1)[:n], delay, skip, {at: kw})
    e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
    e.lanes_open(2, MAP_CAP)
    outs, regs = [], []
    for k in range(n):
        if k == at:
            assert e.lanes_map_export(0)["surf"].shape[0] > 0
            assert e.lanes_map_import([0], **kw) == (0, 0)
            m = e.lanes_map_export(0)
            assert m["corner"].shape[0] == 0 and m["surf"].shape[0] == 0 and m["surround_phase"] == 1
            _same(m["aft"], GUESS[1], "aft")
            _same(m["bef"], GUESS[2], "bef")
            _map_eq(m, imp[at][1], "lane 0 straight after the reset")
        o, r = _step(e, [sweeps(1)[k], sweeps(2)[k]], k, range(2))
        outs.append(o)
        regs.append(r)
    maps = {l: e.lanes_map_export(l) for l in range(2)}
    e.close()
    assert _check_lane(loam, outs, regs, 0, recs) >= 4
    _map_eq(maps[0], cmap, "lane 0 map")
    recs, cmap, _ = ctx("s2", sweeps(2)[:n], delay, skip)
    _check_lane(loam, outs, regs, 1, recs)
    _map_eq(maps[1], cmap, "lane 1 map")


def test_every_invalid_call_changes_nothing(loam, sweeps, ctx, prior):
    """S = 3; lane 2 has failed (an empty sweep).  Every refused call leaves `dropped` alone and the
    live lanes' maps and later steps as they would have been"""
    n, delay, skip, at = 8, 1, 1, 5
    kw = _kw(prior, aft=GUESS[1], bef=ZERO)
    INVAL = loam.LOAM_E_INVAL
    closed = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
    assert _raw(loam, closed, [0], kw) == (INVAL, (7, 8))  # lanes not open
    closed.close()
    e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
    e.lanes_open(3, MAP_CAP)
    outs, regs = [], []
    big = np.zeros((4, 4), np.float32)

    def corner_count(c):
        def f(m):
            m.corner.count = c
        return f

    def null_pts(m):
        m.surf.pts = None

    def phase(m):
        m.surround_phase = 5

    def centre(m):
        m.center[1] = -(1 << 24) - 1
    for k in range(n):
        raws = [sweeps(1)[k], sweeps(2)[k], sweeps(3)[k] if k != 3 else np.zeros((0, 4), np.float32)]
        if k == at:
            assert outs[-1]["status"][2] == INVAL
            before = [e.lanes_map_export(l) for l in range(2)]
            bad = [dict(lanes=[0], n=0), dict(lanes=[0, 1, 2, 0], n=4), dict(lanes=[0, 3]), dict(lanes=[1, 0xffffffff]),
                   dict(lanes=[1, 0, 1]), dict(lanes=[0, 2]), dict(lanes=[0], mutate=null_pts), dict(lanes=[0], mutate=phase),
                   dict(lanes=[0], mutate=centre), dict(lanes=[0], kw=dict(kw, corner=big), mutate=corner_count(1 << 31))]
            for b in bad:
                assert _raw(loam, e, b["lanes"], b.get("kw", kw), b.get("n"), b.get("mutate")) == (INVAL, (7, 8)), b
                assert loam.lib().loam_last_error()
            for l in range(2):
                _map_eq(e.lanes_map_export(l), before[l], f"lane {l} after the refused calls")
            e.lanes_push(raws, stamp=0.1 * k)
            assert _raw(loam, e, [0], kw) == (INVAL, (7, 8))  # a step in flight
            o = e.lanes_pull()
            r = {l: e.lanes_registered(l) for l in range(2) if o["mapped"][l]}
        else:
            o, r = _step(e, raws, k, range(2))
        outs.append(o)
        regs.append(r)
    maps = {l: e.lanes_map_export(l) for l in range(2)}
    e.close()
    for l, s in ((0, 1), (1, 2)):
        recs, cmap, _ = ctx(f"s{s}", sweeps(s)[:n], delay, skip)
        assert _check_lane(loam, outs, regs, l, recs) >= 3
        _map_eq(maps[l], cmap, f"lane {l} map")
