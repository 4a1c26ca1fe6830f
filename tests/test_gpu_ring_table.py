"""Ring tables on the GPU (loam_set_ring_table): a ring model stated as data.

Hook (loam_dev_sr_ring_of_table), on the uneven 32-beam sensor cut from the synthetic HDL-64 sweep
(ring_table_cases.py): (i) around every bound at 0.5 / 5 / 50 m, every consecutive float within 4e-3
degrees: the production ring equals the exact one, both deciders present; (ii) on the 32-beam sweep
(no point within 0.05 degrees of a bound, asserted) the thresholds decide every point and the ring
is the numpy table rule's; (iii) degenerate points take the exact evaluation, elevations outside
the table and inside a -1 interval are dropped.

Built-in models restated: a context given loam_ring_table_of_model of its own config equals a
context left on the built-in model bit for bit: a node call on test_gpu_sr_ring_id.py's moved sweep,
that sweep first and last in a 32-problem batch (k_sr_ring_fused), and (VLP-16) 8 sweeps through
loam_chain_sweep with the exported map.

Uneven sensor through the product: the node call's full cloud is the input stably sorted by the
numpy ring; the batch returns the same clouds; two lanes (host and device push) equal two
loam_chain_sweep contexts.

Refusals: loam_set_ring_table after each call that shows the context a sweep, each of the check's
errors through a context, and a refused call leaving the built-in model's outputs unchanged."""
import ctypes

import numpy as np
import pytest

import hipmem
import ring_table_cases as rt
import sr_ring_hook as rh

pytestmark = pytest.mark.gpu

CLOUDS = ("full", "sharp", "less_sharp", "flat", "less_flat")
WINDOW_DEG = 4e-3
MAP_CAP = 1 << 19
MARGIN_DEG = 0.05


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, msg):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


# ---------------------------------------------------------------- the uneven sensor
@pytest.fixture(scope="module")
def uneven(loam, sg):
    """the table, two 6-sweep 32-beam streams, the sweeps' capacity and the numpy ring of stream 0's sweep 1"""
    bounds, rings = rt.uneven_table(loam)
    loam.ring_table_check(rt.N_RINGS, bounds, rings)
    streams = [[rt.uneven_sweep(s) for s in sg.stream_sweeps(6, seed, lidar=sg.HDL64)] for seed in (2, 3)]
    cap = max(len(s) for st in streams for s in st)
    for st in streams:
        for s in st:   # no kept point within 0.05 degrees of a bound: the numpy rule and the device rule agree
            ang = rt.vertical_angle(s[:, :3])
            assert np.min(rt.margin_to_bounds(bounds, ang)) > MARGIN_DEG
            want = np.searchsorted(np.array(rt.KEEP_LASERS), s[:, 3].astype(np.int64))
            np.testing.assert_array_equal(rt.table_rule(bounds, rings, ang.astype(np.float32)), want)
    return dict(bounds=bounds, rings=rings, streams=streams, cap=int(cap),
                cfg=dict(n_rings=rt.N_RINGS, max_points=int(cap)))


def _engine(loam, u, **kw):
    e = loam.Engine(loam.default_config(**dict(u["cfg"], **kw)))
    e.set_ring_table(u["bounds"], u["rings"])
    return e


def _node_call(e, raw):
    assert e.scan_registration(raw)[0] == -4   # LOAM_E_NOT_READY: the first sweep is inside systemDelay
    rc, f = e.scan_registration(raw)
    assert rc == 0
    return f


# ---------------------------------------------------------------- 3. the hook
def test_hook_ring_equals_exact_at_every_bound(loam, uneven):
    b, r = uneven["bounds"], uneven["rings"]
    parts = []
    for k, hr in enumerate((0.5, 5.0, 50.0)):
        az = 0.3 + 1.1 * k
        x, y = np.float32(hr * np.cos(az)), np.float32(hr * np.sin(az))
        rad = np.sqrt(np.float64(np.float32(np.float32(x * x) + np.float32(y * y))))
        for bd in b.astype(np.float64):
            z = rh.consecutive_floats(rad * np.tan(np.radians(bd - WINDOW_DEG)), rad * np.tan(np.radians(bd + WINDOW_DEG)))
            p = np.empty((len(z), 3), np.float32)
            p[:, 0], p[:, 1], p[:, 2] = x, y, z
            parts.append(p)
    pts = np.concatenate(parts)
    ring, exact, fast = rt.ring_of(loam.lib(), rt.N_RINGS, b, r, pts)
    nfast = int(fast.sum())
    print(f"{len(pts)} points, {nfast} decided by the thresholds, {len(pts) - nfast} by the exact evaluation")
    bad = np.nonzero(ring != exact)[0]
    assert bad.size == 0, (bad[:5], pts[bad[:5]], ring[bad[:5]], exact[bad[:5]])
    assert 0 < nfast < len(pts)
    assert set(np.unique(exact)) == set(range(-1, rt.N_RINGS))   # every ring's bounds, and the drop beyond the ends


def test_hook_thresholds_decide_the_uneven_sweep(loam, uneven):
    b, r = uneven["bounds"], uneven["rings"]
    pts = uneven["streams"][0][1][:, :3]
    ring, exact, fast = rt.ring_of(loam.lib(), rt.N_RINGS, b, r, pts)
    np.testing.assert_array_equal(ring, exact)
    assert int(fast.sum()) == len(pts), np.nonzero(fast == 0)[0][:10]
    np.testing.assert_array_equal(ring, rt.table_rule(b, r, rt.vertical_angle(pts).astype(np.float32)))
    assert set(np.unique(ring)) == set(range(rt.N_RINGS))


def test_hook_degenerate_and_dropped_points(loam, uneven):
    b = uneven["bounds"]
    r = uneven["rings"].copy()
    r[10] = -1                                    # a dropped interval inside the table
    hole = 0.5 * (float(b[10]) + float(b[11]))
    pts = []
    for z in (0.0, -0.0, 1e-3, -1e-3, 200.0, -200.0):
        for h in (0.0, -0.0):
            pts.append((h, h, z))
            pts.append((h, -h, z))
    n_zero = len(pts)
    outside = (float(b[0]) - 0.3, float(b[0]) - 5.0, float(b[-1]) + 0.3, float(b[-1]) + 10.0, 30.0, 45.0, 60.0, 89.0,
               -45.0, -60.0, -89.0, hole, hole + 0.1, hole - 0.1)
    for mag in (1e-3, 200.0):
        for elev in outside:
            pts.append((mag * np.cos(np.radians(elev)), 0.0, mag * np.sin(np.radians(elev))))
            pts.append((0.0, -mag * np.cos(np.radians(elev)), mag * np.sin(np.radians(elev))))
    pts = np.array(pts, np.float32)
    ring, exact, fast = rt.ring_of(loam.lib(), rt.N_RINGS, b, r, pts)
    np.testing.assert_array_equal(ring, exact)
    assert np.all(fast[:n_zero] == 0)             # px = pz = 0: the exact evaluation
    assert np.all(ring[n_zero:] == -1)            # beyond the table or inside the -1 interval: dropped
    # the rest of the table is untouched by the hole
    sw = uneven["streams"][0][1][::7, :3]
    ring2, exact2, _ = rt.ring_of(loam.lib(), rt.N_RINGS, b, r, sw)
    want = rt.table_rule(b, r, rt.vertical_angle(sw).astype(np.float32))
    np.testing.assert_array_equal(ring2, want)
    np.testing.assert_array_equal(exact2, want)
    assert np.any(want == -1) and np.any(want == 9) and np.any(want == 11)


# ---------------------------------------------------------------- 4. the built-in models restated
_MODELS = {"vlp16": (dict(), rh.VLP16, None), "linear64": (dict(n_rings=64, ring_model=1, max_points=160000), rh.HDL64, 1)}
_RESTATED = {}


def _restated_case(loam, sg, name):
    if name not in _RESTATED:
        kw, model, lidar = _MODELS[name]
        prevs, curs = sg.batch_problems(2, base_seed=4100) if lidar is None else \
            sg.batch_problems(2, base_seed=4100, lidar=sg.HDL64)
        _RESTATED[name] = (kw, list(prevs), list(curs), rt.moved_sweep(curs[0], rh.all_boundaries(model), 5))
    return _RESTATED[name]


def _pair(loam, kw):
    """(a context on the built-in model, one given the model's own table)"""
    cfg = loam.default_config(**kw)
    a, b = loam.Engine(loam.default_config(**kw)), loam.Engine(loam.default_config(**kw))
    b.set_ring_table(*loam.ring_table_of_model(cfg))
    return a, b


@pytest.mark.parametrize("name", sorted(_MODELS))
def test_restated_model_node_call(loam, sg, name):
    kw, _, _, moved = _restated_case(loam, sg, name)
    a, b = _pair(loam, dict(kw, system_delay=1))
    fa, fb = _node_call(a, moved), _node_call(b, moved)
    a.close()
    b.close()
    assert fa["full"].shape[0] > 1000
    for c in CLOUDS:
        _same(fa[c], fb[c], f"{name} node call {c}")


@pytest.mark.parametrize("name", sorted(_MODELS))
def test_restated_model_fused_batch(loam, sg, name):
    kw, prevs, curs, moved = _restated_case(loam, sg, name)
    bp = [moved] + [prevs[i % 2] for i in range(1, 32)]
    bc = [curs[i % 2] for i in range(31)] + [moved]
    res = []
    for e in _pair(loam, kw):
        e.batch_upload(bp, bc)
        e.batch_run()
        res.append(e.batch_features())
        e.close()
    for c in CLOUDS:
        np.testing.assert_array_equal(res[0][c][1], res[1][c][1], err_msg=f"{name} batch {c} offsets")
        _same(res[0][c][0], res[1][c][0], f"{name} batch {c}")
    assert int(res[0]["full"][1][1]) > 1000 and int(res[0]["full"][1][64] - res[0]["full"][1][63]) > 1000


def test_restated_model_chain(loam, sg):
    sweeps = sg.stream_sweeps(8, 1)
    runs = []
    for e in _pair(loam, dict(system_delay=0)):
        recs = [e.chain_sweep(sw, stamp=0.1 * k, registered=True) for k, sw in enumerate(sweeps)]
        runs.append((recs, e.map_export()))
        e.close()
    (ra, ma), (rb, mb) = runs
    mapped = 0
    for k, (x, y) in enumerate(zip(ra, rb)):
        assert x[0] == y[0] and x[1] == y[1], k
        for i, what in ((2, "od_sum"), (3, "aft"), (4, "bef"), (5, "registered")):
            assert (x[i] is None) == (y[i] is None), (k, what)
            if x[i] is not None:
                _same(x[i], y[i], f"chain sweep {k} {what}")
        mapped += x[3] is not None
    assert mapped >= 3
    for key in ("corner", "surf", "aft", "bef"):
        _same(ma[key], mb[key], f"chain map {key}")
    for key in ("corner_offset", "surf_offset", "center"):
        np.testing.assert_array_equal(ma[key], mb[key], err_msg=f"chain map {key}")
    assert ma["corner"].shape[0] > 100 and ma["surf"].shape[0] > 1000


# ---------------------------------------------------------------- 5. the uneven sensor through the product
@pytest.fixture(scope="module")
def uneven_node(loam, uneven):
    """the five clouds of a node call on stream 0's sweep 1"""
    e = _engine(loam, uneven, system_delay=1)
    f = _node_call(e, uneven["streams"][0][1])
    e.close()
    return f


def test_uneven_node_call_sorts_by_the_table(loam, uneven, uneven_node):
    raw = uneven["streams"][0][1]
    ring = rt.table_rule(uneven["bounds"], uneven["rings"], rt.vertical_angle(raw[:, :3]).astype(np.float32))
    assert np.all(ring >= 0)
    order = np.argsort(ring, kind="stable")
    full = uneven_node["full"]
    assert full.shape[0] == raw.shape[0]
    _same(full[:, 0], raw[order, 1], "full x = the sensor's y")     # the axis swap of src/scanRegistration.cpp:225-229
    _same(full[:, 1], raw[order, 2], "full y = the sensor's z")
    _same(full[:, 2], raw[order, 0], "full z = the sensor's x")
    np.testing.assert_array_equal(np.floor(full[:, 3]).astype(np.int64), ring[order])
    assert set(np.unique(ring)) == set(range(rt.N_RINGS))
    for c in CLOUDS[1:]:
        assert uneven_node[c].shape[0] > 0, c
        assert np.all((uneven_node[c][:, 3] >= 0) & (uneven_node[c][:, 3] < rt.N_RINGS)), c


def test_uneven_fused_batch_returns_the_node_calls_clouds(loam, uneven, uneven_node):
    s = uneven["streams"][0]
    sweep = s[1]
    bp = [sweep] + [s[2 + i % 2] for i in range(1, 32)]
    bc = [s[4 + i % 2] for i in range(31)] + [sweep]
    e = _engine(loam, uneven)
    e.batch_upload(bp, bc)
    e.batch_run()
    res = e.batch_features()
    e.close()
    for j in (0, 63):
        for c in CLOUDS:
            got, want = res[c][0][int(res[c][1][j]):int(res[c][1][j + 1])], uneven_node[c]
            _same(got, want, f"batch sweep {j} {c}")   # the same clouds: x, y, z and intensity bit for bit


@pytest.fixture(scope="module")
def uneven_chain(loam, uneven):
    """each stream through its own loam_chain_sweep context: per sweep the record and the five clouds of
    a node call on it (scan registration keeps no state without IMU)"""
    out = []
    node = _engine(loam, uneven, system_delay=1)
    assert node.scan_registration(uneven["streams"][0][0])[0] == loam.LOAM_E_NOT_READY
    for st in uneven["streams"]:
        e = _engine(loam, uneven, system_delay=1)
        recs = []
        for k, sw in enumerate(st):
            rc, pub, od, aft, bef, reg = e.chain_sweep(sw, stamp=0.1 * k, registered=True)
            rec = {"rc": rc, "pub": pub, "od_sum": od, "aft": aft, "bef": bef, "reg": reg}
            if rc == 0:
                rc2, f = node.scan_registration(sw)
                assert rc2 == 0
                rec["sr"] = f
            recs.append(rec)
        e.close()
        out.append(recs)
    node.close()
    return out


@pytest.mark.parametrize("push", ["host", "device"])
def test_uneven_lanes_equal_chain_contexts(loam, uneven, uneven_chain, push):
    streams = uneven["streams"]
    e = _engine(loam, uneven, system_delay=1)
    e.lanes_open(2, MAP_CAP)
    hip = hipmem.Hip(loam) if push == "device" else None
    mapped = 0
    try:
        for k in range(6):
            raws = [np.ascontiguousarray(streams[l][k]) for l in range(2)]
            if hip is None:
                e.lanes_push(raws, stamp=0.1 * k)
            else:
                e.lanes_push_device([(hip.upload(r), r.shape[0], r.shape[1] * 4) for r in raws], stamp=0.1 * k)
            o = e.lanes_pull()
            cl = e.lanes_clouds() if np.any(o["status"] == 0) else None
            for l in range(2):
                r, m = uneven_chain[l][k], f"{push} push lane {l} step {k}"
                assert o["status"][l] == r["rc"], m
                if r["rc"] != 0:
                    continue
                assert o["published"][l] == r["pub"], m
                _same(o["od_sum"][l], r["od_sum"], m + " od_sum")
                for c in CLOUDS:
                    _same(cl[c][l], r["sr"][c], f"{m} {c}")
                assert o["mapped"][l] == (1 if r["aft"] is not None else 0), m
                if r["aft"] is not None:
                    mapped += 1
                    _same(o["aft"][l], r["aft"], m + " aft")
                    _same(o["bef"][l], r["bef"], m + " bef")
                    _same(cl["registered"][l], r["reg"], m + " registered")
    finally:
        e.lanes_close()
        e.close()
        if hip is not None:
            hip.release()
    assert mapped >= 4


# ---------------------------------------------------------------- 6. refusals
def _set(loam, e, bounds, rings):
    b = np.ascontiguousarray(bounds, np.float32)
    r = np.ascontiguousarray(rings, np.int32)
    return loam.lib().loam_set_ring_table(e.h, len(r), b.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                          r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))


@pytest.mark.parametrize("after", ["scan_registration", "chain_sweep", "batch_upload", "batch_feed", "lanes_open",
                                   "lanes_open_shared"])
def test_set_ring_table_is_refused_after_a_sweep(loam, sg, after):
    prev, cur = sg.single_problem(0)
    e = loam.Engine(loam.default_config(system_delay=1))
    table = loam.ring_table_of_model(e.cfg)
    if after == "scan_registration":
        assert e.scan_registration(cur)[0] == loam.LOAM_E_NOT_READY
        assert _set(loam, e, *table) == 0          # (a sweep inside systemDelay is discarded unseen)
        assert e.scan_registration(cur)[0] == 0
    elif after == "chain_sweep":
        assert e.chain_sweep(cur)[0] == loam.LOAM_E_NOT_READY
        assert e.chain_sweep(cur)[0] == 0
    elif after == "batch_upload":
        e.batch_upload([prev], [cur])
    elif after == "batch_feed":
        e.batch_upload([prev], [cur])
        e.batch_feed([prev], [cur])
    elif after == "lanes_open":
        e.lanes_open(1, 1024)
    else:
        e.lanes_open_shared(1, 1024)
    assert _set(loam, e, *table) == loam.LOAM_E_INVAL
    assert b"seen a sweep" in loam.lib().loam_last_error()
    e.close()


def test_refused_tables_leave_the_model_as_it_was(loam, sg):
    _, cur = sg.single_problem(0)
    ref = loam.Engine(loam.default_config(system_delay=1))
    want = _node_call(ref, cur)
    ref.close()
    e = loam.Engine(loam.default_config(system_delay=1))
    b = np.arange(-2.0, 3.0, dtype=np.float32)
    r = np.array([0, 1, -1, 15], np.int32)
    L = loam.lib()
    pf, pi = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    inval = loam.LOAM_E_INVAL
    assert L.loam_set_ring_table(e.h, 4, None, r.ctypes.data_as(pi)) == inval
    assert L.loam_set_ring_table(e.h, 4, b.ctypes.data_as(pf), None) == inval
    assert L.loam_set_ring_table(e.h, 0, b.ctypes.data_as(pf), r.ctypes.data_as(pi)) == inval
    assert L.loam_set_ring_table(e.h, 65, b.ctypes.data_as(pf), r.ctypes.data_as(pi)) == inval
    for bb, rr, word in (([-2.0, -1.0, np.nan, 1.0, 2.0], r, b"(-89, 89)"), ([-2.0, -1.0, 0.0, 1.0, 89.5], r, b"(-89, 89)"),
                         ([-2.0, -1.0, -1.0, 1.0, 2.0], r, b"ascending"), ([-2.0, -1.0, -0.99, 1.0, 2.0], r, b"1/32"),
                         (b, [0, 1, -1, 16], b"[-1, n_rings)"), (b, [0, 1, -2, 15], b"[-1, n_rings)"),
                         (b, [-1, -1, -1, -1], b"not be -1")):
        assert _set(loam, e, bb, rr) == inval
        assert word in L.loam_last_error(), (word, L.loam_last_error())
    got = _node_call(e, cur)
    for c in CLOUDS:
        _same(got[c], want[c], f"after the refusals {c}")
    assert _set(loam, e, b, r) == inval            # and now the context has seen a sweep
    e.close()
