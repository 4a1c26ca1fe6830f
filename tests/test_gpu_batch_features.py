"""loam_batch_features: the scan-registration clouds of every problem of a batch run, against the
CPU oracle's scanRegistration of the same sweeps.

Every selected sweep and all five clouds are compared, with the tolerances of test_gpu_parity.py:
shapes and x, y, z bit-exact, intensity (ring + 0.1 * relTime, float atan2: ocml / glibc) within
2e-6.  The shapes are the smallest that reach each launch shape of the batch scan registration: 6
sweeps (two-kernel ring sort), 64 sweeps (k_sr_ring_fused), a pipelined and fed 64-problem batch
(three / two rotating SR sets), the mixed selection routes, and HDL-64E sweeps."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT_TOL = 2e-6
CLOUDS = ("full", "sharp", "less_sharp", "flat", "less_flat")

_SWEEPS = {}   # (base_seed, lidar) -> (prevs, curs), the longest batch asked for so far
_ORACLE = {}   # id of a sweep array -> (the array, the oracle's feature clouds of it)


def _problems(sg, n, base_seed, lidar=None):
    """the first n problems of a seeded batch.  Problem i depends on base_seed + i alone, so a
    shorter batch is a prefix of a longer one: the arrays already generated are kept (their oracle
    results are shared between the tests through _ORACLE)"""
    key = (base_seed, lidar)
    old = _SWEEPS.get(key, ([], []))
    if len(old[0]) < n:
        kw = {} if lidar is None else dict(lidar=lidar)
        p, c = sg.batch_problems(n, base_seed=base_seed, **kw)
        p, c = list(p), list(c)
        p[:len(old[0])] = old[0]
        c[:len(old[1])] = old[1]
        _SWEEPS[key] = (p, c)
    p, c = _SWEEPS[key]
    return list(p[:n]), list(c[:n])


def _oracle_sr(oc, raw, cfg_kw=None):
    """the oracle's scanRegistration of one sweep, computed once per sweep array and shared"""
    hit = _ORACLE.get(id(raw))
    if hit is not None and hit[0] is raw:
        return hit[1]
    kw = dict(cfg_kw or {})
    kw.setdefault("system_delay", 1)
    o = oc.Oracle(oc.default_config(**kw), cap=int(kw.get("max_points", 40000)))
    assert o.scan_registration(raw)[0] != 0      # inside systemDelay
    rc, f = o.scan_registration(raw)
    assert rc == 0
    _ORACLE[id(raw)] = (raw, f)
    return f


def _oracle_all(oc, raws, cfg_kw=None):
    """the sweeps not yet in _ORACLE on eight threads (an Oracle per sweep, no shared state; the
    library call releases the GIL)"""
    from concurrent.futures import ThreadPoolExecutor
    todo = [r for r in {id(r): r for r in raws}.values() if _ORACLE.get(id(r), (None,))[0] is not r]
    oc.lib()
    with ThreadPoolExecutor(8) as pool:
        list(pool.map(lambda r: _oracle_sr(oc, r, cfg_kw), todo))


def _cmp_cloud(a, b, name):
    assert a.shape == b.shape, f"{name}: {a.shape} vs {b.shape}"
    np.testing.assert_array_equal(a[:, :3], b[:, :3], err_msg=name)
    if a.shape[0]:
        assert np.max(np.abs(a[:, 3] - b[:, 3])) <= INT_TOL, name


def _sweep(res, name, j):
    pts, off = res[name]
    return pts[int(off[j]):int(off[j + 1])]


def _check_layout(res, n):
    for name in CLOUDS:
        pts, off = res[name]
        assert off.shape == (2 * n + 1,) and off.dtype == np.uint32
        assert off[0] == 0 and off[-1] == pts.shape[0] and np.all(np.diff(off.astype(np.int64)) >= 0), name
        assert pts.dtype == np.float32 and pts.shape[1] == 4


def _check_against_oracle(oc, res, prevs, curs, cfg_kw=None, what=""):
    """every sweep (2i: prev_i, 2i + 1: cur_i) and every cloud of a whole-batch download"""
    n = len(prevs)
    _check_layout(res, n)
    _oracle_all(oc, list(prevs) + list(curs), cfg_kw)
    for i in range(n):
        for k, raw in enumerate((prevs[i], curs[i])):
            fo = _oracle_sr(oc, raw, cfg_kw)
            for name in CLOUDS:
                _cmp_cloud(_sweep(res, name, 2 * i + k), fo[name], f"{what} problem {i} sweep {k} {name}")


def _small_batch(sg):
    """P = 3: plain problems, one sweep ragged (20 011 points) with non-finite returns"""
    key = "small"
    if key not in _SWEEPS:
        prevs, curs = _problems(sg, 3, 1896)
        raw = curs[1].copy()
        raw[::97, 0] = np.nan
        curs[1] = raw[:20011]
        _SWEEPS[key] = (prevs, curs)
    return _SWEEPS[key]


def _run(loam, prevs, curs, cfg_kw=None):
    e = loam.Engine(loam.default_config(**(cfg_kw or {})))
    e.batch_upload(prevs, curs)
    e.batch_run()
    return e


# ---------------------------------------------------------------- parity shapes
def test_features_small_batch(loam, oc, sg):
    """6 sweeps: the two-kernel ring sort, a sequential step"""
    prevs, curs = _small_batch(sg)
    e = _run(loam, prevs, curs)
    res = e.batch_features()
    e.close()
    assert res["full"][1][4] - res["full"][1][3] < 20011  # the ragged sweep lost its NaN returns
    _check_against_oracle(oc, res, prevs, curs, what="P=3")


def test_features_ring_fused(loam, oc, sg):
    """64 sweeps: the smallest launch that takes k_sr_ring_fused (sequential step, P < step_pipe)"""
    prevs, curs = _problems(sg, 32, 1896)
    e = _run(loam, prevs, curs)
    res = e.batch_features()
    e.close()
    _check_against_oracle(oc, res, prevs, curs, what="P=32")


@pytest.mark.parametrize("sets", [3, 2])
def test_features_pipelined_and_fed(loam, oc, sg, sets):
    """P = 64 runs as the step pipeline; with feeds the rotating SR sets hold different batches, so
    reading any set but the last step's returns the wrong sweeps"""
    A, B = _problems(sg, 64, 1896), _problems(sg, 64, 3000)
    e = loam.Engine()
    e.set_tuning(pipe_sr_sets=sets)
    e.batch_upload(*A)
    pa, pb = e.prepare_batch(*A), e.prepare_batch(*B)
    e.batch_feed(pa)
    e.batch_run()
    e.batch_feed(pb)
    e.batch_run()
    e.sync()
    _check_against_oracle(oc, e.batch_features(), *B, what=f"sets={sets} fed B")
    e.batch_feed(pa)
    e.batch_run()
    _check_against_oracle(oc, e.batch_features(), *A, what=f"sets={sets} fed A")
    e.close()


def test_features_selection_routes(loam, oc, sg):
    """the mixed-route batch of test_gpu_parity.test_sr_batch_selection_routes: dropped rings,
    doubled sweeps and both, more routed sweeps than the fallback kernels' workgroup rows"""
    P = 48
    prevs, curs = _problems(sg, P + 1, 3000)

    def drop_ring(a):
        elev = np.degrees(np.arctan2(a[:, 2], np.hypot(a[:, 0], a[:, 1])))
        return a[np.abs(elev - 3.0) > 0.5]

    bp, bc = [], []
    for i in range(P):
        p, c = prevs[i], curs[i]
        if i % 4 in (1, 3):  # two sweeps per message
            p, c = np.concatenate([prevs[i + 1], p]), np.concatenate([p, c])
        if i % 4 in (0, 3):
            p, c = drop_ring(p), drop_ring(c)
        bp.append(p)
        bc.append(c)
    kw = dict(max_points=80000)
    e = _run(loam, bp, bc, kw)
    res = e.batch_features()
    e.close()
    _check_against_oracle(oc, res, bp, bc, kw, what="routes")


def test_features_hdl64(loam, oc, sg):
    """64 HDL-64E sweeps (64 rings, 160 000-point slots): four distinct problems eight times over,
    every downloaded sweep against its source's oracle result"""
    p4, c4 = _problems(sg, 4, 5000, lidar=sg.HDL64)
    prevs, curs = [p4[i % 4] for i in range(32)], [c4[i % 4] for i in range(32)]
    kw = dict(n_rings=64, ring_model=loam.RING_LINEAR, max_points=160000)
    e = _run(loam, prevs, curs, kw)
    res = e.batch_features()
    e.close()
    _check_against_oracle(oc, res, prevs, curs, kw, what="HDL-64E")


# ---------------------------------------------------------------- semantics
def _raw_call(loam, e, first, n, bufs, count0=0):
    """loam_batch_features through ctypes: bufs = {cloud: (points array or None, capacity, offsets
    array or None)}, every struct's count preset to count0; returns (rc, the struct)"""
    bc = loam.BatchClouds()
    for name in CLOUDS:
        getattr(bc, name).count = count0
    for name, (pts, cap, off) in bufs.items():
        b = getattr(bc, name)
        b.pts = pts.ctypes.data if pts is not None else None
        b.capacity = cap
        b.offset = off.ctypes.data if off is not None else None
    return loam.lib().loam_batch_features(e.h, first, n, ctypes.byref(bc)), bc


def test_features_semantics(loam, sg):
    prevs, curs = _small_batch(sg)
    e = loam.Engine()
    e.batch_upload(prevs, curs)
    with pytest.raises(loam.LoamError) as ei:     # no run since the upload
        e.batch_features()
    assert ei.value.code == loam.LOAM_E_INVAL
    e.batch_run()
    whole = e.batch_features()
    _check_layout(whole, 3)
    for first, n in ((3, 1), (2, 2), (0, 4), (0, 0)):
        with pytest.raises(loam.LoamError) as ei:
            e.batch_features(first, n)
        assert ei.value.code == loam.LOAM_E_INVAL, (first, n)
    # a sub-range is the matching slice of the whole
    part = e.batch_features(1, 2)
    _check_layout(part, 2)
    for name in CLOUDS:
        pts, off = whole[name]
        np.testing.assert_array_equal(part[name][0], pts[int(off[2]):int(off[6])], err_msg=name)
        np.testing.assert_array_equal(part[name][1], off[2:7] - off[2], err_msg=name)
    # a subset of the clouds: the same arrays, the other structs untouched
    sub = e.batch_features(clouds=("flat", "full"))
    assert sorted(sub) == ["flat", "full"]
    for name in sub:
        np.testing.assert_array_equal(sub[name][0], whole[name][0])
        np.testing.assert_array_equal(sub[name][1], whole[name][1])
    off_f = np.zeros(7, np.uint32)
    rc, bc = _raw_call(loam, e, 0, 3, {"sharp": (None, 0, off_f)}, count0=77)
    assert rc == 0 and bc.sharp.count == whole["sharp"][0].shape[0]
    np.testing.assert_array_equal(off_f, whole["sharp"][1])
    for name in ("full", "less_sharp", "flat", "less_flat"):
        b = getattr(bc, name)
        assert (b.pts, b.capacity, b.count, b.offset) == (None, 0, 77, None), name
    # sizes only: every count and offset, no points
    offs = {name: np.zeros(7, np.uint32) for name in CLOUDS}
    rc, bc = _raw_call(loam, e, 0, 3, {name: (None, 0, offs[name]) for name in CLOUDS})
    assert rc == 0
    for name in CLOUDS:
        assert getattr(bc, name).count == whole[name][0].shape[0]
        np.testing.assert_array_equal(offs[name], whole[name][1])
    # one cloud a point short: LOAM_E_CAPACITY, the required counts, nothing written past any buffer
    GUARD = np.float32(-12345.5)
    for short in ("less_flat", "sharp"):
        bufs, offs = {}, {}
        for name in CLOUDS:
            need = whole[name][0].shape[0]
            cap = need - 1 if name == short else need
            arr = np.full((need + 8, 4), GUARD, np.float32)
            offs[name] = np.zeros(7, np.uint32)
            bufs[name] = (arr, cap, offs[name])
        rc, bc = _raw_call(loam, e, 0, 3, bufs)
        assert rc == loam.LOAM_E_CAPACITY, short
        for name in CLOUDS:
            need = whole[name][0].shape[0]
            assert getattr(bc, name).count == need, (short, name)
            np.testing.assert_array_equal(offs[name], whole[name][1])
            assert np.all(bufs[name][0][bufs[name][1]:] == GUARD), (short, name)
        # ... and the call may be repeated with more room: guards behind the points stay intact
        for name in CLOUDS:
            bufs[name] = (bufs[name][0], whole[name][0].shape[0], offs[name])
        rc, bc = _raw_call(loam, e, 0, 3, bufs)
        assert rc == 0
        for name in CLOUDS:
            need = whole[name][0].shape[0]
            np.testing.assert_array_equal(bufs[name][0][:need], whole[name][0], err_msg=name)
            assert np.all(bufs[name][0][need:] == GUARD), name
    # null arguments
    assert loam.lib().loam_batch_features(e.h, 0, 3, None) == loam.LOAM_E_INVAL
    # a new upload needs a new run
    e.batch_upload(prevs, curs)
    with pytest.raises(loam.LoamError):
        e.batch_features()
    e.close()
    fresh = loam.Engine()
    fresh.n = 3
    with pytest.raises(loam.LoamError) as ei:     # no batch uploaded
        fresh.batch_features()
    assert ei.value.code == loam.LOAM_E_INVAL
    fresh.close()


def test_features_leave_the_pipeline_alone(loam, sg):
    """run, batch_features, run, download == run, run, download, bit for bit (P = 64: pipelined
    steps with work enqueued ahead when the call arrives)"""
    A = _problems(sg, 64, 1896)

    def go(with_features):
        e = loam.Engine()
        e.batch_upload(*A)
        e.batch_run()
        if with_features:
            res = e.batch_features()
            assert res["full"][0].shape[0] > 64 * 2 * 10000
        e.batch_run()
        od, aft, st = e.batch_download()
        oi, mi, tr = e.batch_lm_info()
        e.close()
        return od, aft, st, oi, mi, tr

    x, y = go(True), go(False)
    np.testing.assert_array_equal(x[0], y[0])
    np.testing.assert_array_equal(x[1], y[1])
    assert x[2]["od_iters"] == y[2]["od_iters"] and x[2]["mp_iters"] == y[2]["mp_iters"]
    np.testing.assert_array_equal(x[3], y[3])
    np.testing.assert_array_equal(x[4], y[4])
    np.testing.assert_array_equal(x[5], y[5])


def test_features_equal_node_call(loam, sg):
    """each sweep's batch clouds equal loam_scan_registration on the same sweep, intensity
    included, bit for bit: the launch shape (batch grid or one sweep) does not change results"""
    prevs, curs = _small_batch(sg)
    e = _run(loam, prevs, curs)
    res = e.batch_features()
    e.close()
    for i in range(3):
        for k, raw in enumerate((prevs[i], curs[i])):
            node = loam.Engine(loam.default_config(system_delay=1))
            assert node.scan_registration(raw)[0] == loam.LOAM_E_NOT_READY
            rc, f = node.scan_registration(raw)
            node.close()
            assert rc == 0
            for name in CLOUDS:
                got = _sweep(res, name, 2 * i + k)
                assert got.shape == f[name].shape, (i, k, name)
                np.testing.assert_array_equal(got[:, :3], f[name][:, :3], err_msg=f"{i} {k} {name}")
                assert np.max(np.abs(got[:, 3] - f[name][:, 3]), initial=0.0) <= INT_TOL, (i, k, name)
                assert np.array_equal(got.view(np.uint32), f[name].view(np.uint32)), (i, k, name)
