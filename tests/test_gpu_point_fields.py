"""Ring and time from the sweep's own fields on the GPU (loam_set_point_fields).

The yardstick is the oracle-pinned model path wherever the fields say what the model would say, and
a numpy statement (point_fields_cases.py) where they say something no model can.

1. Ring only equals the model: the ring recovered from the model's full cloud, fed back as a U16
   field, gives the five clouds and imu_trans bit for bit (a stream sweep, the sweep with NaN and
   30-60 degree points, and cuts of 1 / 2047 / 2048 / 2049 points around the 2048-point tile).
2. Ring and time equals the model: tau' = I - ring as an F32 field; node call, 8 sweeps through
   loam_chain_sweep with the exported map, and an HDL-64 node call with 64 rings.
3. Fields no model can state, against numpy: a decimating ring map, two swapped lasers, U32
   nanosecond times with a bias, times outside [0, 0.5]; every type and stride gives the same bits.
4. The services agree on test 3's sensor: the fused batch, and host- and device-pushed lanes
   against loam_chain_sweep contexts.
5. IMU: ring only equals the model (chain and lane); jittered times agree between the chain, the
   host-pushed and the device-pushed lane; unjittered times stay within 1e-3 m of the model.
6. Refusals."""
import ctypes

import numpy as np
import pytest

import hipmem
import lanes_imu_cases as lc
import point_fields_cases as pc

pytestmark = pytest.mark.gpu

CLOUDS = ("full", "sharp", "less_sharp", "flat", "less_flat")
MAP_CAP = 1 << 19
HDL = dict(n_rings=64, ring_model=1, max_points=160000)
RING_ONLY = pc.Layout((pc.U16, 20), None, 32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b, msg):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _node_call(e, raw, stamp=0.0):
    assert e.scan_registration(raw, stamp=stamp)[0] == -4   # LOAM_E_NOT_READY: the first sweep is inside systemDelay
    rc, f = e.scan_registration(raw, stamp=stamp)
    assert rc == 0
    return f


def _engine(loam, layout=None, scale=1.0, bias=0.0, ring_map=None, **kw):
    e = loam.Engine(loam.default_config(**kw))
    if layout is not None:
        e.set_point_fields(fields=pc.fields(loam, layout, scale, bias, ring_map))
    return e


def _preconditions(sweep, full):
    """what the tests lean on (checked on the CPU oracle when they were written): every point kept,
    unique coordinate bit patterns, intensity - int(intensity) in [0, 0.1000004], no negative value"""
    assert full.shape[0] == sweep.shape[0]
    assert len(set(pc.xyz_keys(sweep[:, :3]))) == sweep.shape[0]
    frac = full[:, 3] - np.floor(full[:, 3])
    assert not np.any(np.signbit(full[:, 3])) and not np.any(np.signbit(frac))
    assert float(frac.max()) <= 0.1000004


def _tau_of_model(ring, inten):
    """tau' = I_A - ring (exact), for the model's kept points; 0 for the absent ones"""
    r = np.where(ring == 65535, 0, ring).astype(np.float32)
    tau = (inten - r).astype(np.float32)
    assert np.array_equal(_bits(r + tau), _bits(inten))       # ring + tau' == I_A exactly
    return tau


# ---------------------------------------------------------------- the VLP-16 sweeps and the model's answers
@pytest.fixture(scope="module")
def vlp(loam, sg):
    sweeps = sg.stream_sweeps(8, 1)
    assert all(s.shape[0] == 28800 for s in sweeps)
    node = _engine(loam, system_delay=1)
    fulls = [_node_call(node, sweeps[0])] + [node.scan_registration(s)[1] for s in sweeps[1:]]
    node.close()
    for s, f in zip(sweeps, fulls):
        _preconditions(s, f["full"])
    return dict(sweeps=sweeps, model=fulls)


def _cases_of(vlp):
    base = vlp["sweeps"][1]
    crafted, high, nan = pc.with_nans_and_high_points(base)
    out = {"stream": base, "nan_high": crafted}
    for n in (1, 2047, 2048, 2049):
        out[f"cut{n}"] = np.ascontiguousarray(base[:n])
    return out


@pytest.mark.parametrize("case", ["stream", "nan_high", "cut1", "cut2047", "cut2048", "cut2049"])
@pytest.mark.parametrize("mode", ["ring", "ring_time"])
def test_fields_equal_the_model_on_a_node_call(loam, vlp, case, mode):
    raw = _cases_of(vlp)[case]
    a = _engine(loam, system_delay=1)
    fa = _node_call(a, raw)
    a.close()
    ring, inten = pc.rings_from_full(raw[:, :3], fa["full"])
    if case == "nan_high":
        assert np.count_nonzero(ring == 65535) == 128 and ring[0] == 65535 and ring[-1] == 65535
        assert fa["full"].shape[0] == raw.shape[0] - 128
    else:
        assert not np.any(ring == 65535)
    if mode == "ring":
        ci, keep = pc.cloud_in(loam, RING_ONLY, raw[:, :3], ring)
        b = _engine(loam, RING_ONLY, system_delay=1)
    else:
        ci, keep = pc.cloud_in(loam, pc.VELODYNE, raw[:, :3], ring, _tau_of_model(ring, inten))
        b = _engine(loam, pc.VELODYNE, system_delay=1)
    fb = _node_call(b, ci)
    b.close()
    for c in CLOUDS:
        _same(fa[c], fb[c], f"{case} {mode} {c}")
    _same(fa["imu_trans"], fb["imu_trans"], f"{case} {mode} imu_trans")
    if case in ("stream", "nan_high"):
        assert fb["less_flat"].shape[0] > 1000 and fb["sharp"].shape[0] > 20


def _timed_clouds(loam, vlp):
    out = []
    for s, f in zip(vlp["sweeps"], vlp["model"]):
        ring, inten = pc.rings_from_full(s[:, :3], f["full"])
        out.append(pc.cloud_in(loam, pc.VELODYNE, s[:, :3], ring, _tau_of_model(ring, inten)))
    return out


def test_ring_and_time_equals_the_model_through_the_chain(loam, vlp):
    timed = _timed_clouds(loam, vlp)
    runs = []
    for layout, feed in ((None, vlp["sweeps"]), (pc.VELODYNE, [ci for ci, _ in timed])):
        e = _engine(loam, layout, system_delay=0)
        recs = [e.chain_sweep(sw, stamp=0.1 * k, registered=True) for k, sw in enumerate(feed)]
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


def test_ring_and_time_equals_the_linear_model_with_64_rings(loam, sg):
    raw = sg.stream_sweeps(2, 2, lidar=sg.HDL64)[1]
    assert raw.shape[0] == 131072
    a = _engine(loam, system_delay=1, **HDL)
    fa = _node_call(a, raw)
    a.close()
    _preconditions(raw, fa["full"])
    ring, inten = pc.rings_from_full(raw[:, :3], fa["full"])
    assert set(np.unique(ring)) == set(range(64))
    ci, keep = pc.cloud_in(loam, pc.VELODYNE, raw[:, :3], ring, _tau_of_model(ring, inten))
    b = _engine(loam, pc.VELODYNE, system_delay=1, **HDL)
    fb = _node_call(b, ci)
    b.close()
    for c in CLOUDS:
        _same(fa[c], fb[c], f"HDL-64 {c}")


# ---------------------------------------------------------------- 3. fields no model can state
N32 = 32
RING_MAP = [l // 2 if l % 2 == 0 else -1 for l in range(64)]     # a 64-beam unit decimated to 32 rings
SWAP = (10, 20)                                                  # two lasers whose field values are swapped
BIAS = -0.01
SCALE = 1e-9


def _sensor_values(sweep, seed):
    """the ring field's values, the U32 nanosecond times and their tau for one HDL-64 sweep"""
    laser = sweep[:, 3].astype(np.int64)
    v = laser.copy()
    v[laser == SWAP[0]], v[laser == SWAP[1]] = SWAP[1], SWAP[0]
    n = sweep.shape[0]
    want = np.arange(n) / n * 0.095 + laser * 2e-6                # the firing column plus a per-laser offset
    ns = np.round((want - BIAS) / SCALE).astype(np.uint32)
    rng = np.random.default_rng(seed)
    bad = rng.choice(n, 300, replace=False)
    ns[bad[:150]] = rng.integers(0, 9_000_000, 150)               # before the sweep: tau < 0
    ns[bad[150:]] = rng.integers(520_000_000, 4_000_000_000, 150)  # beyond 0.5 s
    tau = pc.tau_of(ns, SCALE, BIAS)
    return v, ns, tau


@pytest.fixture(scope="module")
def sensor(loam, sg):
    streams = [sg.stream_sweeps(6, seed, lidar=sg.HDL64) for seed in (2, 3)]
    vals = [[_sensor_values(s, 100 * i + k) for k, s in enumerate(st)] for i, st in enumerate(streams)]
    return dict(streams=streams, vals=vals, cfg=dict(n_rings=N32, max_points=160000))


U32_LAYOUT = pc.Layout((pc.U16, 20), (pc.U32, 24), 32)


def _sensor_engine(loam, sensor, layout=U32_LAYOUT, scale=SCALE, bias=BIAS, **kw):
    return _engine(loam, layout, scale, bias, RING_MAP, **dict(sensor["cfg"], **kw))


def _sensor_cloud(loam, sensor, i, k, layout=U32_LAYOUT, lead=0):
    s = sensor["streams"][i][k]
    v, ns, tau = sensor["vals"][i][k]
    t = ns if layout.time[0] == pc.U32 else tau      # F32 / F64 carry tau itself (scale 1, bias 0): the same value
    return pc.cloud_in(loam, layout, s[:, :3], v, t, lead)


@pytest.fixture(scope="module")
def sensor_node(loam, sensor):
    """the five clouds of a node call on stream 0's sweep 1"""
    e = _sensor_engine(loam, sensor, system_delay=1)
    ci, keep = _sensor_cloud(loam, sensor, 0, 1)
    f = _node_call(e, ci)
    e.close()
    return f


def test_sensor_node_call_against_numpy(loam, sensor, sensor_node):
    s = sensor["streams"][0][1]
    v, ns, tau = sensor["vals"][0][1]
    r = pc.ring_of(v, N32, RING_MAP)
    ok = pc.kept(s[:, :3], r, tau)
    assert 100 <= np.count_nonzero((r >= 0) & ~ok) <= 200 and np.count_nonzero(r < 0) > s.shape[0] // 4
    want = pc.expected_full(s[:, :3], r, tau)
    full = sensor_node["full"]
    _same(full, want, "full = the kept points stably sorted by ring, (y, z, x), float32(r) + tau")
    assert set(np.unique(full[:, 3].astype(np.int64))) == set(range(N32))
    # the field contradicts the elevation: laser 20's points sit in ring 5, laser 10's in ring 10
    laser_of = {k: int(l) for k, l in zip(pc.xyz_keys(s[:, :3]), s[:, 3])}
    lasers = np.array([laser_of[k] for k in pc.xyz_keys(full[:, [2, 0, 1]])])
    rings = full[:, 3].astype(np.int64)
    assert set(lasers[rings == 5]) == {20} and set(lasers[rings == 10]) == {10} and set(lasers[rings == 6]) == {12}
    rows = {row.tobytes() for row in np.ascontiguousarray(full)}
    for c in ("sharp", "less_sharp", "flat"):
        assert sensor_node[c].shape[0] > 0, c
        assert all(row.tobytes() in rows for row in np.ascontiguousarray(sensor_node[c])), c
    lf = sensor_node["less_flat"][:, 3]
    assert lf.shape[0] > 1000
    assert np.all((lf >= 0) & (lf.astype(np.int64) < N32) & (lf - np.floor(lf) <= 0.5))


@pytest.mark.parametrize("ring_t,time_t,stride,lead", [(pc.U8, pc.F32, 24, 0), (pc.U16, pc.F64, 28, 0), (pc.U32, pc.U32, 32, 0),
                                                        (pc.U8, pc.F64, 48, 0), (pc.U32, pc.F32, 24, 0), (pc.U16, pc.U32, 28, 1)])
def test_sensor_every_type_and_stride_gives_the_same_bits(loam, sensor, sensor_node, ring_t, time_t, stride, lead):
    # ring at 12 (its type's size is a divisor), time at 16; F64 ends at 24, the smallest stride here
    layout = pc.Layout((ring_t, 12), (time_t, 16), stride)
    assert layout.end() <= stride
    scale, bias = (SCALE, BIAS) if time_t == pc.U32 else (1.0, 0.0)
    e = _sensor_engine(loam, sensor, layout, scale, bias, system_delay=1)
    ci, keep = _sensor_cloud(loam, sensor, 0, 1, layout, lead)
    assert ci.data % 4 == lead
    f = _node_call(e, ci)
    e.close()
    for c in CLOUDS:
        _same(f[c], sensor_node[c], f"{layout.ring} {layout.time} stride {stride} lead {lead} {c}")


# ---------------------------------------------------------------- 4. the services agree
def test_sensor_fused_batch_returns_the_node_calls_clouds(loam, sensor, sensor_node):
    clouds = [[_sensor_cloud(loam, sensor, 0, k) for k in range(6)]]
    ci = [c for c, _ in clouds[0]]
    bp = [ci[1]] + [ci[2 + i % 2] for i in range(1, 32)]
    bc = [ci[4 + i % 2] for i in range(31)] + [ci[1]]
    e = _sensor_engine(loam, sensor)
    e.batch_upload(bp, bc)
    e.batch_run()
    res = e.batch_features()
    e.close()
    for j in (0, 63):
        for c in CLOUDS:
            got = res[c][0][int(res[c][1][j]):int(res[c][1][j + 1])]
            _same(got, sensor_node[c], f"batch sweep {j} {c}")


@pytest.fixture(scope="module")
def sensor_chain(loam, sensor):
    """each stream through its own loam_chain_sweep context, with the node call's clouds per sweep"""
    out = []
    node = _sensor_engine(loam, sensor, system_delay=1)
    assert node.scan_registration(_sensor_cloud(loam, sensor, 0, 0)[0])[0] == loam.LOAM_E_NOT_READY
    for i in range(2):
        e = _sensor_engine(loam, sensor, system_delay=1)
        recs = []
        for k in range(6):
            ci, keep = _sensor_cloud(loam, sensor, i, k)
            rc, pub, od, aft, bef, reg = e.chain_sweep(ci, stamp=0.1 * k, registered=True)
            rec = {"rc": rc, "pub": pub, "od_sum": od, "aft": aft, "bef": bef, "reg": reg}
            if rc == 0:
                rc2, f = node.scan_registration(ci)
                assert rc2 == 0
                rec["sr"] = f
            recs.append(rec)
        out.append((recs, e.map_export()))
        e.close()
    node.close()
    return out


# the device push's layout: ring u16 in the high half of its dword, an F64 time whose address is 4 mod 8
DEV_LAYOUT = pc.Layout((pc.U16, 22), (pc.F64, 24), 40)


@pytest.mark.parametrize("push", ["host", "device"])
def test_sensor_lanes_equal_chain_contexts(loam, sensor, sensor_chain, push):
    hip = hipmem.Hip(loam) if push == "device" else None
    layout, scale, bias = (DEV_LAYOUT, 1.0, 0.0) if hip else (U32_LAYOUT, SCALE, BIAS)
    e = _sensor_engine(loam, sensor, layout, scale, bias, system_delay=1)
    e.lanes_open(2, MAP_CAP)
    mapped = 0
    try:
        for k in range(6):
            clouds = [_sensor_cloud(loam, sensor, l, k, layout) for l in range(2)]
            if hip is None:
                e.lanes_push([c for c, _ in clouds], stamp=0.1 * k)
            else:
                dev = []
                for c, buf in clouds:
                    base = hip.malloc(buf.nbytes + 8)
                    assert base % 8 == 0
                    hip.put(base + 4, buf)                   # records at 4 mod 8: time at 4 + 40 i + 24
                    dev.append((base + 4, c.count, layout.stride))
                e.lanes_push_device(dev, stamp=0.1 * k)
            o = e.lanes_pull()
            cl = e.lanes_clouds() if np.any(o["status"] == 0) else None
            for l in range(2):
                r, m = sensor_chain[l][0][k], f"{push} push lane {l} step {k}"
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
        for l in range(2):
            ml, mc = e.lanes_map_export(l), sensor_chain[l][1]
            for key in ("corner", "surf"):
                _same(ml[key], mc[key], f"{push} push lane {l} map {key}")
    finally:
        e.lanes_close()
        e.close()
        if hip is not None:
            hip.release()
    assert mapped >= 4


# ---------------------------------------------------------------- 5. IMU
K_IMU = 6


@pytest.fixture(scope="module")
def imu_case(loam, sg, vlp):
    """6 VLP-16 sweeps with the loop's IMU stream, and the model's run of them: per sweep the node
    call's clouds and imu_trans, and the chain's record"""
    sweeps = vlp["sweeps"][:K_IMU]
    sched = lc.schedule(sg.imu_stream(-0.5, lc.PERIOD * K_IMU + 0.1, seed=1), 0.0, K_IMU)
    return dict(sweeps=sweeps, sched=sched, model=_imu_run_chain(loam, None, sweeps, sched))


def _imu_run_chain(loam, layout, feed, sched):
    e, s = _engine(loam, layout, system_delay=1), _engine(loam, layout, system_delay=1)
    recs = []
    for k, sw in enumerate(feed):
        for m in sched[k]:
            e.imu(*m)
            s.imu(*m)
        rc, pub, od, aft, bef, reg = e.chain_sweep(sw, stamp=0.1 * k, registered=True)
        src, f = s.scan_registration(sw, stamp=0.1 * k)
        assert rc == src
        recs.append({"rc": rc, "pub": pub, "od_sum": od, "aft": aft, "bef": bef, "reg": reg, "sr": f})
    e.close()
    s.close()
    return recs


def _imu_run_lane(loam, layout, feed, sched, hip=None):
    """the same stream on the one lane of a lanes context, pushed from the host or (hip) from the device"""
    e = _engine(loam, layout, system_delay=1)
    e.lanes_open(1, MAP_CAP)
    recs = []
    try:
        for k, sw in enumerate(feed):
            for m in sched[k]:
                e.lanes_imu(0, *m)
            if hip is None:
                e.lanes_push([sw], stamp=0.1 * k)
            else:
                ci, buf = sw
                e.lanes_push_device([(hip.upload(buf), ci.count, ci.stride_bytes)], stamp=0.1 * k)
            o = e.lanes_pull()
            rec = {"rc": int(o["status"][0])}
            if rec["rc"] == 0:
                cl = e.lanes_clouds()
                rec.update(pub=int(o["published"][0]), od_sum=o["od_sum"][0].copy(), mapped=int(o["mapped"][0]),
                           aft=o["aft"][0].copy(), bef=o["bef"][0].copy(), reg=cl["registered"][0],
                           sr={c: cl[c][0] for c in CLOUDS}, imu_trans=e.lanes_imu_trans()[0].copy())
            recs.append(rec)
    finally:
        e.lanes_close()
        e.close()
    return recs


def _same_run(a, b, msg, lane_b=False):
    """two runs bit for bit: full, imu_trans, poses, registered clouds (b may be a lane's records)"""
    n = 0
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["rc"] == y["rc"], (msg, k)
        if x["rc"] != 0:
            continue
        n += 1
        for c in CLOUDS:
            _same(x["sr"][c], y["sr"][c], f"{msg} sweep {k} {c}")
        xt = x["imu_trans"] if "imu_trans" in x else x["sr"]["imu_trans"]
        yt = y["imu_trans"] if "imu_trans" in y else y["sr"]["imu_trans"]
        _same(xt, yt, f"{msg} sweep {k} imu_trans")
        assert x["pub"] == y["pub"], (msg, k)
        _same(x["od_sum"], y["od_sum"], f"{msg} sweep {k} od_sum")
        xm = x["mapped"] if "mapped" in x else (x["aft"] is not None)
        ym = y["mapped"] if "mapped" in y else (y["aft"] is not None)
        assert bool(xm) == bool(ym), (msg, k)
        if xm:
            _same(x["aft"], y["aft"], f"{msg} sweep {k} aft")
            _same(x["bef"], y["bef"], f"{msg} sweep {k} bef")
            _same(x["reg"], y["reg"], f"{msg} sweep {k} registered")
    assert n >= 4


def _imu_fields(loam, imu_case, timed, jitter_seed=None):
    """the stream's sweeps as records: the ring (and tau') recovered from a context without IMU"""
    out = []
    for k, s in enumerate(imu_case["sweeps"]):
        ring, inten = pc.rings_from_full(s[:, :3], imu_case["plain"][k]["full"])
        if not timed:
            out.append(pc.cloud_in(loam, RING_ONLY, s[:, :3], ring))
            continue
        tau = _tau_of_model(ring, inten)
        if jitter_seed is not None:   # +-2 ms, clipped at 0: times cross between neighbours and across tiles
            rng = np.random.default_rng(jitter_seed + k)
            tau = np.maximum(tau + rng.uniform(-2e-3, 2e-3, len(tau)).astype(np.float32), np.float32(0))
        out.append(pc.cloud_in(loam, pc.VELODYNE, s[:, :3], ring, tau))
    return out


@pytest.fixture(scope="module")
def imu_plain(imu_case, vlp):
    imu_case["plain"] = vlp["model"][:K_IMU]      # the model without IMU: the rings and the times of the points
    return imu_case


def test_imu_ring_only_equals_the_model(loam, imu_plain):
    feed = _imu_fields(loam, imu_plain, timed=False)
    assert np.any(np.abs(imu_plain["model"][2]["sr"]["imu_trans"]) > 0)      # the de-skew is live
    got = _imu_run_chain(loam, RING_ONLY, [ci for ci, _ in feed], imu_plain["sched"])       # k_sr_ring_sort<true>
    _same_run(imu_plain["model"], got, "chain, ring only")
    lane = _imu_run_lane(loam, RING_ONLY, [ci for ci, _ in feed], imu_plain["sched"])       # count / scatter<true>
    _same_run(imu_plain["model"], lane, "lane, ring only")


def test_imu_jittered_times_agree_between_the_services(loam, imu_plain):
    feed = _imu_fields(loam, imu_plain, timed=True, jitter_seed=77)
    tau = feed[2][1][:28800 * 32].reshape(-1, 32)[:, 24:28].copy().view(np.float32).reshape(-1)
    d = np.diff(tau)
    assert np.count_nonzero(d < 0) > 5000                                    # times are not monotone along the sweep
    tile_max = np.maximum.accumulate([tau[i:i + pc.TILE].max() for i in range(0, len(tau), pc.TILE)])
    assert any(tau[i:i + pc.TILE].min() < tile_max[j - 1] for j, i in enumerate(range(0, len(tau), pc.TILE)) if j > 0)
    chain = _imu_run_chain(loam, pc.VELODYNE, [ci for ci, _ in feed], imu_plain["sched"])
    host = _imu_run_lane(loam, pc.VELODYNE, [ci for ci, _ in feed], imu_plain["sched"])
    _same_run(chain, host, "chain against the host-pushed lane, jittered times")
    hip = hipmem.Hip(loam)
    try:
        dev = _imu_run_lane(loam, pc.VELODYNE, feed, imu_plain["sched"], hip)
    finally:
        hip.release()
    _same_run(chain, dev, "chain against the device-pushed lane, jittered times")


def test_imu_unjittered_times_stay_next_to_the_model(loam, imu_plain):
    """A guard against a wrong queue entry or unit, not a precision claim: the time differs from the
    model's by at most half an ulp of the intensity (2 us at ring 15), which at the stream's 1 m/s
    and 0.17 rad/s moves a 30 m point by about 2e-5 m; a wrong entry moves it by centimetres."""
    feed = _imu_fields(loam, imu_plain, timed=True)
    got = _imu_run_chain(loam, pc.VELODYNE, [ci for ci, _ in feed], imu_plain["sched"])
    worst = 0.0
    for k, (x, y) in enumerate(zip(imu_plain["model"], got)):
        assert x["rc"] == y["rc"]
        if x["rc"] != 0:
            continue
        a, b = x["sr"]["full"], y["sr"]["full"]
        assert a.shape == b.shape
        _same(a[:, 3], b[:, 3], f"sweep {k} intensity")                     # ring + tau' == I exactly
        worst = max(worst, float(np.abs(a[:, :3] - b[:, :3]).max()))
    print(f"largest |delta| over full's coordinates, fields against the model with the same IMU: {worst:.3g} m")
    assert worst < 1e-3


# ---------------------------------------------------------------- bag replay
@pytest.mark.parametrize("fields", ["auto", "ring_only"])
def test_bag_replay_with_fields_equals_the_model(loam, vlp, tmp_path, fields):
    """the stream as a bag of velodyne PointXYZIRT messages whose ring and time are the model's own:
    replay(fields="auto") (ring and time from the first message's field list) and replay(fields=a
    ring-only PointFields) give the poses of a replay on the ring model, bit for bit"""
    import importlib
    import bagwriter as bw
    rb = importlib.import_module("loam_velodyne-1_amd.rosbag")
    msgs = []
    for k, (s, f) in enumerate(zip(vlp["sweeps"], vlp["model"])):
        ring, inten = pc.rings_from_full(s[:, :3], f["full"])
        buf, _ = pc.records(pc.VELODYNE, s[:, :3], ring, _tau_of_model(ring, inten), fill=0)
        msg = pc.pointcloud2(pc.PC2_VELODYNE, 32, buf[:s.shape[0] * 32].tobytes(), stamp=0.1 * k)
        msgs.append(("/velodyne_points", "sensor_msgs/PointCloud2", 0.1 * k + 0.05, msg))
    path = tmp_path / "fields.bag"
    bw.write_bag(path, msgs, chunk_messages=4)
    cfg = dict(system_delay=1)
    want = rb.replay(path, loam.Engine(loam.default_config(**cfg)))
    arg = "auto" if fields == "auto" else loam.PointFields.of((loam.FIELD_U16, 20))
    got = rb.replay(path, loam.Engine(loam.default_config(**cfg)), fields=arg)
    assert got["sweeps"] == want["sweeps"] == 8 and len(want["odometry"]) >= 5 and len(want["mapping"]) >= 2
    for key in ("odometry", "mapping"):
        assert len(got[key]) == len(want[key]), key
        for (ta, pa), (tb, pb) in zip(got[key], want[key]):
            assert ta == tb
            _same(pa, pb, f"replay {fields} {key} at {ta}")
    with pytest.raises(ValueError):
        rb.replay(path, loam.Engine(loam.default_config(**cfg)), fields="ring")


# ---------------------------------------------------------------- 6. refusals
def _set(loam, e, f):
    return loam.lib().loam_set_point_fields(e.h, ctypes.byref(f) if f is not None else None)


@pytest.mark.parametrize("after", ["scan_registration", "chain_sweep", "batch_upload", "batch_feed", "lanes_open",
                                   "lanes_open_shared"])
def test_set_point_fields_is_refused_after_a_sweep(loam, sg, after):
    prev, cur = sg.single_problem(0)
    e = loam.Engine(loam.default_config(system_delay=1))
    f = pc.fields(loam, pc.VELODYNE)
    if after == "scan_registration":
        assert e.scan_registration(cur)[0] == loam.LOAM_E_NOT_READY
        assert _set(loam, e, f) == 0 and _set(loam, e, None) == 0      # (a sweep inside systemDelay is discarded unseen)
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
    assert _set(loam, e, f) == loam.LOAM_E_INVAL
    assert b"seen a sweep" in loam.lib().loam_last_error()
    assert _set(loam, e, None) == loam.LOAM_E_INVAL
    e.close()


def test_refused_fields_leave_the_model_as_it_was(loam, sg):
    _, cur = sg.single_problem(0)
    ref = loam.Engine(loam.default_config(system_delay=1))
    want = _node_call(ref, cur)
    ref.close()
    e = loam.Engine(loam.default_config(system_delay=1))
    P = loam.PointFields.of
    L = loam.lib()
    for f, word in ((P((pc.F32, 20)), b"ring_type"), (P((pc.U16, 20), (pc.U16, 24, 1.0, 0.0)), b"time_type"),
                    (P((pc.U16, 8)), b"at least 12"), (P((pc.U16, 21)), b"multiple"), (P((pc.U32, 65536)), b"65536"),
                    (P((pc.U16, 26), (pc.F32, 24, 1.0, 0.0)), b"overlap"), (P((pc.U16, 20), (pc.F32, 24, 0.0, 0.0)), b"time_scale"),
                    (P((pc.U16, 20), (pc.F32, 24, 1.0, np.inf)), b"time_bias"), (P((pc.U16, 20), None, [0] * 257), b"ring_map_n"),
                    (P((pc.U16, 20), None, [0, 16]), b"[-1, n_rings)"), (P((pc.U16, 20), None, [-1, -1]), b"not be -1")):
        assert _set(loam, e, f) == loam.LOAM_E_INVAL
        assert word in L.loam_last_error() and b"loam_set_point_fields" in L.loam_last_error(), (word, L.loam_last_error())
    f = P((pc.U16, 20))
    f.ring_map_n = 2
    assert _set(loam, e, f) == loam.LOAM_E_INVAL and b"ring_map is null" in L.loam_last_error()
    # set, then back to the model, then a table and fields in either order: the model's outputs again
    assert _set(loam, e, pc.fields(loam, pc.VELODYNE)) == 0 and _set(loam, e, None) == 0
    got = _node_call(e, cur)
    for c in CLOUDS:
        _same(got[c], want[c], f"after the refusals {c}")
    assert _set(loam, e, pc.fields(loam, pc.VELODYNE)) == loam.LOAM_E_INVAL     # and now the context has seen a sweep
    e.close()


def test_fields_and_ring_table_in_either_order(loam, vlp):
    raw = vlp["sweeps"][1]
    ring, inten = pc.rings_from_full(raw[:, :3], vlp["model"][1]["full"])
    ci, keep = pc.cloud_in(loam, pc.VELODYNE, raw[:, :3], ring, _tau_of_model(ring, inten))
    table = loam.ring_table_of_model(loam.default_config())
    for order in ("table_first", "fields_first"):
        e = loam.Engine(loam.default_config(system_delay=1))
        if order == "table_first":
            e.set_ring_table(*table)
        e.set_point_fields(fields=pc.fields(loam, pc.VELODYNE))
        if order == "fields_first":
            e.set_ring_table(*table)
        f = _node_call(e, ci)
        e.close()
        for c in CLOUDS:
            _same(f[c], vlp["model"][1][c], f"{order} {c}")


def test_a_sweep_without_a_kept_point_is_a_sweep_the_model_rejects(loam, vlp):
    """every point finite but none kept: what the ring model does with a sweep whose every point it
    rejects (here: 40 degrees elevation under the VLP-16 rule), call by call"""
    raw = np.array(vlp["sweeps"][1][:3000], np.float32, copy=True)
    high = raw.copy()
    high[:, 2] = (np.hypot(high[:, 0].astype(np.float64), high[:, 1].astype(np.float64)) * np.tan(np.radians(40.0))).astype(np.float32)
    outs = []
    for layout, feed in ((None, high),
                         (RING_ONLY, pc.cloud_in(loam, RING_ONLY, raw[:, :3], np.full(3000, 65535))[0:2]),
                         (pc.VELODYNE, pc.cloud_in(loam, pc.VELODYNE, raw[:, :3], np.zeros(3000), np.full(3000, 0.7))[0:2])):
        e = _engine(loam, layout, system_delay=1)
        sw = feed if layout is None else feed[0]
        assert e.scan_registration(sw)[0] == loam.LOAM_E_NOT_READY
        try:
            rc, f = e.scan_registration(sw)
            outs.append((rc, None if f is None else {c: f[c].shape[0] for c in CLOUDS}, ""))
        except loam.LoamError as err:
            outs.append((err.code, None, str(err).split(": ", 1)[-1]))
        e.close()
    assert outs[1] == outs[0] and outs[2] == outs[0], outs


def _short_stride_cloud(loam, n=64):
    xyz = np.random.default_rng(5).normal(size=(n, 6)).astype(np.float32) * 5
    return loam.CloudIn(xyz.ctypes.data, n, 24), xyz              # 24 < the velodyne fields' end (28)


def test_a_stride_below_a_fields_end_is_refused_per_service(loam, vlp):
    cur = vlp["sweeps"][1]
    short, keep = _short_stride_cloud(loam)
    ring, inten = pc.rings_from_full(cur[:, :3], vlp["model"][1]["full"])
    ok, keep2 = loam.records(cur[:, :3], ring, _tau_of_model(ring, inten))
    L = loam.lib()

    def inval(call):
        with pytest.raises(loam.LoamError) as err:
            call()
        assert err.value.code == loam.LOAM_E_INVAL and "stride" in str(err.value), str(err.value)

    e = _engine(loam, pc.VELODYNE, system_delay=1)
    assert e.scan_registration(short)[0] == loam.LOAM_E_NOT_READY      # (a sweep inside systemDelay is not looked at)
    inval(lambda: e.scan_registration(short))
    inval(lambda: e.chain_sweep(short))
    inval(lambda: e.batch_upload([ok], [short]))
    inval(lambda: e.batch_upload([short], [ok]))
    e.batch_upload([ok], [ok])
    inval(lambda: e.batch_feed([ok], [short]))
    e.close()
    # the lanes: the lane's own sticky LOAM_E_INVAL, the other lane runs on
    hip = hipmem.Hip(loam)
    try:
        for push in ("host", "device"):
            e = _engine(loam, pc.VELODYNE, system_delay=1)
            e.lanes_open(2, 1 << 16)
            d_ok, d_short = hip.upload(keep2), hip.upload(keep)
            for k in range(3):     # step 0 is inside systemDelay; lane 1's short stride comes on step 1 and sticks
                if push == "host":
                    e.lanes_push([ok, short if k == 1 else ok], stamp=0.1 * k)
                else:
                    e.lanes_push_device([(d_ok, ok.count, 32), (d_short, short.count, 24) if k == 1 else (d_ok, ok.count, 32)],
                                        stamp=0.1 * k)
                o = e.lanes_pull()
                want = [loam.LOAM_E_NOT_READY] * 2 if k == 0 else [0, loam.LOAM_E_INVAL]
                assert list(o["status"]) == want, (push, k, o["status"])
            # the device-push range: x, y, z fit, the time field's end does not -> the call is refused, nothing enqueued
            if push == "device":
                n = 100
                need = (n - 1) * 32 + 28
                buf = hip.malloc(need - 1)
                a = (loam.CloudIn * 2)(loam.CloudIn(buf, n, 32), loam.CloudIn(d_ok, ok.count, 32))
                st = (ctypes.c_double * 2)(0.3, 0.3)
                assert L.loam_lanes_push_device(e.h, st, a, None, 0) == loam.LOAM_E_INVAL
                assert b"leaves its allocation" in L.loam_last_error()
                exact = hip.malloc(need)
                hip.put(exact, keep2[:n].reshape(-1)[:need])
                a[0] = loam.CloudIn(exact, n, 32)
                assert L.loam_lanes_push_device(e.h, st, a, None, 0) == 0     # the field's end just inside
                e.lanes_pull()
            e.lanes_close()
            e.close()
    finally:
        hip.release()
