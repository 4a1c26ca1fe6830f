"""loam_lanes_restart: one lane becomes a fresh sequence while the others run.

The specification: from its first consumed sweep on, a restarted lane behaves exactly as a fresh
context created with system_delay = 0 that receives the lane's IMU messages through loam_imu and its
sweeps through loam_chain_sweep, bit for bit, and no other lane changes by a bit.  The yardstick is
always such a context (never a second lanes run).  A context with system_delay = 0 still does not
look at its first sweep (Q1), so a sequence D is offered to a restarted lane from D[1] on (D[0] is
the sweep "the caller drops") and the yardstick's record of D[1 + j] is the lane's j-th step.

  1. S = 3, skip_frame_num = 1: wait_steps == 0 and wait_steps == 1
  2. skip_frame_num = 0 (the lane's init step is a mapping step of the others) and = 2
  3. a failed and a retired lane revived
  4. a restart inside system_delay: the lane takes the shared init frame
  5. a lane with IMU restarted onto an earlier clock
  6. S = 65: the batch launch forms
  7. three lanes restarted between the same two steps, in two orders
  8. every LOAM_E_INVAL, each leaving the lanes as they were

Streams: VLP-16 synthetic loops (synthgen.stream_sweeps), as tests/test_gpu_lanes.py."""
import ctypes

import numpy as np
import pytest

import lanes_imu_cases as lc

pytestmark = pytest.mark.gpu

MAP_CAP = 1 << 17
N_SWEEPS = 12


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, msg):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _words(v):
    """a pulled field as comparable words: floats by their bits"""
    return _bits(v) if np.asarray(v).dtype == np.float32 else np.asarray(v)


def _map_eq(a, b, msg):
    for k in ("corner", "surf", "aft", "bef"):
        _same(a[k], b[k], f"{msg} {k}")
    for k in ("corner_offset", "surf_offset", "center"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{msg} {k}")
    assert a["surround_phase"] == b["surround_phase"], msg


def expected_wait(delay, skip, steps_done):
    """wait_steps by walking the shared counters of lanes.hpp (not by the formula): the number of
    coming steps before the lane's init step, which is the first coming step that is not the
    shared init frame or earlier and is followed by a mapping step"""
    sr_count, sr_inited, od_inited, c = 0, False, False, skip
    kinds = []  # per step: "skip", "init", "map", "pose"
    for _ in range(steps_done + 2 * skip + 4):
        if not sr_inited:
            sr_count += 1
            sr_inited = sr_count >= delay
            kinds.append("skip")
        elif not od_inited:
            od_inited = True
            kinds.append("init")
        else:
            c += 1
            kinds.append("map" if c >= skip + 1 else "pose")
            if c >= skip + 1:
                c = 0
    if "init" not in kinds[:steps_done]:  # the lane takes the shared init frame
        return kinds.index("init") - steps_done
    j = steps_done
    while kinds[j + 1] != "map":
        j += 1
    return j - steps_done


@pytest.fixture(scope="module")
def sweeps(sg):
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = sg.stream_sweeps(N_SWEEPS, seed)
        return cache[seed]
    return get


@pytest.fixture(scope="module")
def chain(loam):
    """a list of sweeps through a fresh context's chain_sweep: one record per sweep, the final map"""
    cache = {}

    def run(key, seq, delay, skip):
        key = (key, len(seq), delay, skip)
        if key not in cache:
            e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
            recs = []
            for k, sw in enumerate(seq):
                rc, pub, od, aft, bef, reg = e.chain_sweep(sw, stamp=0.1 * k, registered=True)
                rec = {"rc": rc, "pub": pub, "od_sum": od, "aft": aft, "bef": bef, "reg": reg}
                # (loam_get_stats holds the last node body's frame: the odometry's count is there
                # only after a sweep that did not map)
                if rc == 0 and aft is None:
                    rec["od_iters"] = e.stats()["od_iters"]
                if aft is not None:
                    rec["mp_iters"] = e.stats()["mp_iters"]
                recs.append(rec)
            cache[key] = (recs, e.map_export())
            e.close()
        return cache[key]
    return run


def _step_eq(loam, o, reg, l, r, m, trans=None):
    """lane l of one pulled step against one record of a context, bit for bit; returns mapped"""
    assert o["status"][l] == r["rc"], m
    if trans is not None:
        _same(trans[l], r["imu_trans"], m + " imu_trans")
    if r["rc"] != 0:
        assert r["rc"] == loam.LOAM_E_NOT_READY and o["published"][l] == 0 and o["mapped"][l] == 0, m
        return 0
    assert o["published"][l] == r["pub"], m
    assert o["mapped"][l] == (1 if r["aft"] is not None else 0), m
    if r["pub"] & loam.PUB_POSE:
        _same(o["od_sum"][l], r["od_sum"], m + " od_sum")
        if "od_iters" in r:
            assert o["od_iters"][l] == r["od_iters"], m + " od_iters"
    if r["aft"] is None:
        assert l not in reg, m
        return 0
    _same(o["aft"][l], r["aft"], m + " aft")
    _same(o["bef"][l], r["bef"], m + " bef")
    assert o["mp_iters"][l] == r["mp_iters"], m
    assert o["n_registered"][l] == r["reg"].shape[0] > 0, m
    _same(reg[l], r["reg"], m + " registered")
    return 1


class Plan:
    """lane `lane` is restarted after `after` steps and then runs stream `seed`"""

    def __init__(self, lane, after, seed):
        self.lane, self.after, self.seed = lane, after, seed
        self.wait = self.init_step = None


def _run(loam, sweeps, seeds, delay, skip, n, plans, sample=None, feed=None, order=None):
    """S = len(seeds) lanes for n steps; lane l runs stream seeds[l] until a plan restarts it.  A
    restarted lane is offered its new stream's sweep 0 on its wait steps (not looked at) and sweeps
    1, 2, ... from its init step on.  feed(k, l): an override of lane l's sweep of step k, or None.
    Returns the per-step pull dicts, the per-step {lane: registered cloud} and the final {lane: map}
    of the live lanes (of `sample` when given)"""
    S = len(seeds)
    e = loam.Engine(loam.default_config(system_delay=delay, skip_frame_num=skip))
    e.lanes_open(S, MAP_CAP)
    cur = [(s, 0, 0) for s in seeds]  # stream, its sweep index at step `first`, first
    wait_until = [0] * S
    outs, regs = [], []
    lanes = range(S) if sample is None else sample
    for k in range(n):
        due = [p for p in plans if p.after == k]
        for p in ([due[i] for i in order] if due and order else due):
            p.wait = e.lanes_restart(p.lane)
            p.init_step = k + p.wait
            wait_until[p.lane] = p.init_step
            cur[p.lane] = (p.seed, 1, p.init_step)
        raws = []
        for l in range(S):
            seed, i0, first = cur[l]
            sw = sweeps(seed)[0] if k < wait_until[l] else sweeps(seed)[i0 + k - first]
            over = feed(k, l) if feed else None
            raws.append(sw if over is None else over)
        o = e.lanes_step(raws, stamp=0.1 * k)
        outs.append(o)
        regs.append({l: e.lanes_registered(l) for l in lanes if o["mapped"][l] and o["status"][l] == 0})
    maps = {l: e.lanes_map_export(l) for l in lanes if outs[-1]["status"][l] == 0}
    e.close()
    return outs, regs, maps


def _check_restarted(loam, sweeps, chain, outs, regs, maps, p, skip, min_mapped):
    """the plan's lane from its wait steps on: LOAM_E_NOT_READY, then the fresh context's records"""
    n = len(outs)
    l = p.lane
    for k in range(p.after, p.init_step):
        o = outs[k]
        m = f"lane {l} wait step {k}"
        assert o["status"][l] == loam.LOAM_E_NOT_READY and o["published"][l] == 0 and o["mapped"][l] == 0, m
        assert l not in regs[k], m
    seq = sweeps(p.seed)[:1 + n - p.init_step]
    recs, cmap = chain(p.seed, seq, 0, skip)
    assert recs[0]["rc"] == loam.LOAM_E_NOT_READY and recs[1]["pub"] == loam.PUB_CLOUDS
    mapped = 0
    for j, k in enumerate(range(p.init_step, n)):
        mapped += _step_eq(loam, outs[k], regs[k], l, recs[1 + j], f"restarted lane {l} step {k}")
    assert outs[p.init_step]["published"][l] == loam.PUB_CLOUDS and outs[p.init_step]["mapped"][l] == 0
    assert mapped >= min_mapped, (l, mapped)
    _map_eq(maps[l], cmap, f"restarted lane {l} map")
    assert maps[l]["corner"].shape[0] > 0 and maps[l]["surf"].shape[0] > 0


def _check_whole(loam, sweeps, chain, outs, regs, maps, l, seed, delay, skip, upto=None):
    """lane l ran stream `seed` undisturbed for the whole run (or its first `upto` steps)"""
    n = len(outs) if upto is None else upto
    recs, cmap = chain(seed, sweeps(seed)[:n], delay, skip)
    for k in range(n):
        _step_eq(loam, outs[k], regs[k], l, recs[k], f"lane {l} step {k}")
    if upto is None:
        _map_eq(maps[l], cmap, f"lane {l} map")


@pytest.mark.parametrize("after,wait", [(5, 0), (6, 1)])
def test_restart_between_running_lanes(loam, sweeps, chain, after, wait):
    """lane 1 runs stream 2 for 5 steps (and, for wait_steps == 1, one step more), then stream 4"""
    n = 10 + wait * 2
    p = Plan(1, after, 4)
    outs, regs, maps = _run(loam, sweeps, (1, 2, 3), 1, 1, n, [p])
    assert p.wait == wait == expected_wait(1, 1, after)
    _check_whole(loam, sweeps, chain, outs, regs, maps, 1, 2, 1, 1, upto=after)
    _check_restarted(loam, sweeps, chain, outs, regs, maps, p, 1, min_mapped=2)
    for l, seed in ((0, 1), (2, 3)):
        _check_whole(loam, sweeps, chain, outs, regs, maps, l, seed, 1, 1)
    # the others mapped on a step the restarted lane did not (its wait or init step) and never the reverse
    for o in outs:
        assert o["mapped"][1] <= o["mapped"][0] == o["mapped"][2]


@pytest.mark.parametrize("skip,after", [(0, 4), (2, 5), (2, 6), (2, 7)])
def test_other_skip_frame_nums(loam, sweeps, chain, skip, after):
    n = 12 if skip else 9
    p = Plan(0, after, 5)
    outs, regs, maps = _run(loam, sweeps, (2, 3), 1, skip, n, [p])
    # the documented formula: c = the shared frame counter after `after` steps
    c = skip
    for _ in range(after - 2):
        c = c + 1 if c + 1 < skip + 1 else 0
    assert p.wait == (2 * skip - c) % (skip + 1) == expected_wait(1, skip, after)
    assert 0 <= p.wait <= skip
    if skip == 0:
        assert p.wait == 0 and outs[p.init_step]["mapped"][1] == 1  # the others map on the lane's init step
    _check_restarted(loam, sweeps, chain, outs, regs, maps, p, skip, min_mapped=2)
    _check_whole(loam, sweeps, chain, outs, regs, maps, 1, 3, 1, skip)


def test_revive_failed_and_retired(loam, sweeps, chain):
    empty = np.zeros((0, 4), np.float32)
    plans = [Plan(0, 5, 4), Plan(1, 5, 5)]

    def feed(k, l):
        if l == 0 and k == 3:
            return np.full_like(sweeps(1)[3], np.nan)
        return empty if l == 1 and k in (3, 4) else None
    outs, regs, maps = _run(loam, sweeps, (1, 2, 3), 1, 1, 10, plans, feed=feed)
    inval = loam.LOAM_E_INVAL
    assert [int(o["status"][0]) for o in outs[:5]] == [loam.LOAM_E_NOT_READY, 0, 0, inval, inval]
    assert [int(o["status"][1]) for o in outs[:5]] == [loam.LOAM_E_NOT_READY, 0, 0, inval, inval]
    for p in plans:
        assert p.wait == 0
        _check_restarted(loam, sweeps, chain, outs, regs, maps, p, 1, min_mapped=2)
    _check_whole(loam, sweeps, chain, outs, regs, maps, 2, 3, 1, 1)


def test_restart_inside_system_delay(loam, sweeps, chain):
    delay, n = 3, 10
    p = Plan(1, 1, 4)
    # the lane is offered stream 4's sweep k on step k throughout; the shared init frame is step 3
    outs, regs, maps = _run(loam, sweeps, (1, 2), delay, 1, n, [p], feed=lambda k, l: sweeps(4)[k] if l == 1 else None)
    assert p.wait == 2 == expected_wait(delay, 1, 1) and p.init_step == delay
    recs, cmap = chain("offered", [sweeps(4)[0]] + sweeps(4)[delay:n], 0, 1)
    for k in range(delay):
        assert outs[k]["status"][1] == loam.LOAM_E_NOT_READY
    mapped = sum(_step_eq(loam, outs[k], regs[k], 1, recs[1 + k - delay], f"lane 1 step {k}") for k in range(delay, n))
    assert mapped >= 3
    _map_eq(maps[1], cmap, "lane 1 map")
    _check_whole(loam, sweeps, chain, outs, regs, maps, 0, 1, delay, 1)


@pytest.fixture(scope="module")
def context(loam):
    """a lanes_imu_cases feed through a fresh context: loam_imu + chain_sweep, and /imu_trans from a
    second context's scan registration (as tests/test_gpu_lanes_imu.py)"""
    def run(feed, delay):
        cfg = loam.default_config(system_delay=delay)
        e, s = loam.Engine(cfg), loam.Engine(cfg)
        recs = []
        for k, sw in enumerate(feed.sweeps):
            for m in feed.sched[k]:
                e.imu(*m)
                s.imu(*m)
            rc, pub, od, aft, bef, reg = e.chain_sweep(sw, stamp=feed.stamps[k], registered=True)
            rec = {"rc": rc, "pub": pub, "od_sum": od, "aft": aft, "bef": bef, "reg": reg}
            if rc == 0 and aft is None:
                rec["od_iters"] = e.stats()["od_iters"]
            if aft is not None:
                rec["mp_iters"] = e.stats()["mp_iters"]
            src, f = s.scan_registration(sw, stamp=feed.stamps[k])
            assert src == rc
            rec["imu_trans"] = f["imu_trans"] if src == 0 else np.zeros(12, np.float32)
            recs.append(rec)
        out = (recs, e.map_export())
        e.close()
        s.close()
        return out
    return run


def test_restart_with_imu(loam, sg, context):
    K, after = lc.K, 6
    a, b, c = lc.case_mixed(sg)
    # the new sequence of lane 0: another stream and IMU on a clock 50 s before lane 0's first one
    t0 = -50.0
    d = lc.Feed(sg.stream_sweeps(K - after + 1, 4, t0=t0), t0)
    d.sched = lc.schedule(sg.imu_stream(t0 - 0.5, t0 + lc.PERIOD * len(d.sweeps) + 0.1, seed=7), t0, len(d.sweeps))
    assert d.sched[0][0][0] < a.sched[after - 1][-1][0]  # earlier than the lane's last stamp before the restart
    e = loam.Engine(loam.default_config(system_delay=lc.DELAY))
    e.lanes_open(3, MAP_CAP)
    outs, regs, trans = [], [], []
    for k in range(K):
        if k == after:
            assert e.lanes_restart(0) == 0 == expected_wait(lc.DELAY, 1, after)
            for m in d.sched[0]:  # (those of the sweep the caller drops)
                e.lanes_imu(0, *m)
        f0, j = (a, k) if k < after else (d, 1 + k - after)
        for l, (f, i) in enumerate(((f0, j), (b, k), (c, k))):
            for m in f.sched[i]:
                e.lanes_imu(l, *m)
        o = e.lanes_step([f0.sweeps[j], b.sweeps[k], c.sweeps[k]], stamp=[f0.stamps[j], b.stamps[k], c.stamps[k]])
        outs.append(o)
        trans.append(e.lanes_imu_trans())
        regs.append({l: e.lanes_registered(l) for l in range(3) if o["mapped"][l] and o["status"][l] == 0})
    maps = [e.lanes_map_export(l) for l in range(3)]
    e.close()
    recs, cmap = context(d, 0)
    mapped = 0
    for k in range(after, K):
        mapped += _step_eq(loam, outs[k], regs[k], 0, recs[1 + k - after], f"restarted lane 0 step {k}", trans=trans[k])
    assert mapped >= 3 and trans[after][0].any() and trans[-1][0].any()
    _map_eq(maps[0], cmap, "restarted lane 0 map")
    ra, _ = context(lc.Feed(a.sweeps[:after], a.t0, a.sched[:after]), lc.DELAY)
    for k in range(after):
        _step_eq(loam, outs[k], regs[k], 0, ra[k], f"lane 0 step {k}", trans=trans[k])
    for l, f in ((1, b), (2, c)):
        recs, cmap = context(f, lc.DELAY)
        for k in range(K):
            _step_eq(loam, outs[k], regs[k], l, recs[k], f"lane {l} step {k}", trans=trans[k])
        _map_eq(maps[l], cmap, f"lane {l} map")


def test_large_batch_restart(loam, sweeps, chain):
    """S = 65 (the launch forms of a large batch), lane 7 restarted after 3 of 8 steps"""
    seed_of = [1 + l % 3 for l in range(64)] + [5]
    p = Plan(7, 3, 4)
    outs, regs, maps = _run(loam, sweeps, seed_of, 1, 1, 8, [p], sample=(0, 7, 64))
    assert p.wait == 0
    _check_restarted(loam, sweeps, chain, outs, regs, maps, p, 1, min_mapped=2)
    for l in (0, 64):
        _check_whole(loam, sweeps, chain, outs, regs, maps, l, seed_of[l], 1, 1)
    for k, o in enumerate(outs):  # every other lane of lane 7's old stream goes on as lane 1
        for f, v in o.items():
            for l in (4, 10, 61):
                assert np.array_equal(_words(v[l]), _words(v[1])), (k, f, l)


def test_list_of_lanes_in_any_order(loam, sweeps, chain):
    """lanes 1, 3 and 4 of 5 restarted between the same two steps: one clear, and the order of the
    calls is immaterial"""
    seeds = (1, 2, 3, 1, 2)
    runs = []
    for order in ((0, 1, 2), (2, 0, 1)):
        plans = [Plan(1, 4, 4), Plan(3, 4, 5), Plan(4, 4, 3)]
        outs, regs, maps = _run(loam, sweeps, seeds, 1, 1, 9, plans, order=order)
        for p in plans:
            assert p.wait == 1
            _check_restarted(loam, sweeps, chain, outs, regs, maps, p, 1, min_mapped=2)
        for l in (0, 2):
            _check_whole(loam, sweeps, chain, outs, regs, maps, l, seeds[l], 1, 1)
        runs.append((outs, regs, maps))
    (oa, ra, ma), (ob, rb, mb) = runs
    for k in range(len(oa)):
        for f in oa[k]:
            np.testing.assert_array_equal(_words(oa[k][f]), _words(ob[k][f]), err_msg=f"step {k} {f}")
        assert ra[k].keys() == rb[k].keys()
        for l in ra[k]:
            _same(ra[k][l], rb[k][l], f"step {k} registered lane {l}")
    for l in range(5):
        _map_eq(ma[l], mb[l], f"lane {l} map, either order")


def test_errors_leave_the_lanes_as_they_were(loam, sweeps, chain):
    L = loam.lib()
    inval = loam.LOAM_E_INVAL
    eng = loam.Engine(loam.default_config(system_delay=1))
    h = eng.h
    w = ctypes.c_uint32(77)
    assert L.loam_lanes_restart(h, 0, ctypes.byref(w)) == inval  # lanes not open
    assert b"not open" in L.loam_last_error()
    eng.lanes_open(2, MAP_CAP)
    a, b = sweeps(1), sweeps(2)
    recs, _ = chain(2, b[:8], 1, 1)
    n = 0

    def step():
        nonlocal n
        o = eng.lanes_step([a[n], b[n]], stamp=0.1 * n)
        reg = {1: eng.lanes_registered(1)} if o["mapped"][1] else {}
        _step_eq(loam, o, reg, 1, recs[n], f"control lane step {n}")
        n += 1
    for _ in range(3):
        step()
    assert L.loam_lanes_restart(None, 0, ctypes.byref(w)) == inval
    step()
    assert L.loam_lanes_restart(h, 0, None) == inval
    step()
    assert L.loam_lanes_restart(h, 2, ctypes.byref(w)) == inval
    assert b"lane index" in L.loam_last_error()
    step()
    eng.lanes_push([a[n], b[n]], stamp=0.1 * n)
    assert L.loam_lanes_restart(h, 0, ctypes.byref(w)) == inval  # a step in flight
    assert b"in flight" in L.loam_last_error()
    o = eng.lanes_pull()
    _step_eq(loam, o, {1: eng.lanes_registered(1)} if o["mapped"][1] else {}, 1, recs[n], "control lane, in flight")
    n += 1
    assert w.value == 77
    # none of the refused calls restarted lane 0 either
    ra, _ = chain(1, a[:8], 1, 1)
    o = eng.lanes_step([a[n], b[n]], stamp=0.1 * n)
    _step_eq(loam, o, {l: eng.lanes_registered(l) for l in (0, 1) if o["mapped"][l]}, 0, ra[n], "lane 0")
    # a restart twice before the init step only recomputes the wait
    w1, w2 = eng.lanes_restart(0), eng.lanes_restart(0)
    assert w1 == w2 == expected_wait(1, 1, n + 1)
    eng.close()
