"""loam_map_export / loam_map_import on the GPU: the streaming cube map leaves the engine in
canonical order (cube index ascending, the store's point order inside a cube) and comes back.

  1. the export rebuilds the oracle's /laser_cloud_surround bit for bit (the recentring stream of
     test_gpu_branches.py: slot table permuted, lines cleared, pools ping-ponged); the surround's
     centre cube is that of transformTobeMapped as in the reference (:446-452), not of the frame's
     Aft, which stays put on the frames that jump into empty space (_frame_position)
  2. a fresh engine that imports the export continues the stream bit for bit
  3. the import's binning of an arbitrary cloud = numpy's stable sort by (kind, cube)
  4. errors leave the map alone
  5. a deferred map update (loam_chain_sweep) is waited for

Rules of comparison as in test_gpu_branches.py: clouds bit-exact (intensity within 2e-6), poses
within the north-star 1e-4."""
import ctypes

import numpy as np
import pytest

import scenarios

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4
INT_TOL = 2e-6
W, H, D = 21, 11, 21
NCUBE = W * H * D
SPLIT_AT = 7  # the mapping frame after which engine B takes over engine A's map (+x, back, +y done)


def cube_of(v, cen):
    """src/laserMapping.cpp:446-452 / :983-989 in float64: int((v + 25) / 50) + cen, one less below zero"""
    v = np.asarray(v, np.float32).astype(np.float64) + 25.0
    ok = np.isfinite(v) & (np.abs(v) < 1e12)
    c = np.trunc(np.where(ok, v, 0.0) / 50.0).astype(np.int64) + cen
    c = np.where(v < 0, c - 1, c)
    return np.where(ok, c, -(1 << 40))


def cube_keys(pts, center):
    """cube index i + 21 j + 231 k of every point, -1 outside the grid or non-finite"""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    i, j, k = (cube_of(pts[:, a], int(center[a])) for a in range(3))
    ok = (i >= 0) & (i < W) & (j >= 0) & (j < H) & (k >= 0) & (k < D)
    return np.where(ok, i + W * j + W * H * k, -1)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _map_eq(a, b, msg=""):
    for k in ("corner", "surf", "aft", "bef"):
        assert a[k].shape == b[k].shape, (msg, k, a[k].shape, b[k].shape)
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{msg} {k}")
    for k in ("corner_offset", "surf_offset", "center"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{msg} {k}")
    assert a["surround_phase"] == b["surround_phase"], msg


def _check_offsets(m):
    for kind in ("corner", "surf"):
        off = m[kind + "_offset"].astype(np.int64)
        assert off.shape == (NCUBE + 1,) and off[0] == 0 and np.all(np.diff(off) >= 0), kind
        assert off[NCUBE] == m[kind].shape[0], kind


def _cloud_eq(a, b, name):
    assert a.shape == b.shape, f"{name}: {a.shape} vs {b.shape}"
    np.testing.assert_array_equal(a[:, :3], b[:, :3], err_msg=name)
    if a.shape[0]:
        assert np.max(np.abs(a[:, 3] - b[:, 3])) <= INT_TOL, name


def _surround_input(m, pos):
    """/laser_cloud_surround's VoxelGrid input (:1042-1047) rebuilt from an export: the in-bounds
    cubes of the 5x5x5 neighbourhood of the frame's centre cube (of position pos) in i, j, k loop
    order, each cube's corner points then its surf points"""
    ci, cj, ck = (int(cube_of(pos[a], int(m["center"][a]))) for a in range(3))
    parts = []
    for i in range(ci - 2, ci + 3):
        for j in range(cj - 2, cj + 3):
            for k in range(ck - 2, ck + 3):
                if not (0 <= i < W and 0 <= j < H and 0 <= k < D):
                    continue
                c = i + W * j + W * H * k
                for kind in ("corner", "surf"):
                    off = m[kind + "_offset"]
                    parts.append(m[kind][off[c]:off[c + 1]])
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 4), np.float32)


def _frame_position(prev, o, jump):
    """the translation of transformTobeMapped the frame starts from, which the reference takes the
    centre cube of (:446-452): the previous Aft plus the odometry's move since the previous Bef
    (transformAssociateToMap with its rotation of that move left out: under a metre on the 1100 m
    jump, and every frame of this stream is more than 5 m from a cube boundary).  It is not the
    frame's Aft: a frame that jumped into empty space runs no L-M and leaves Aft / Bef as they were."""
    if prev is None:
        return (o["pose"][3:] + np.float32(jump)).astype(np.float64)
    return prev["aft"][3:].astype(np.float64) + (o["pose"][3:] + np.float32(jump) - prev["bef"][3:])


def _recentre(pos, center):
    """the reference's recentring passes (:454-614) for a frame at pos: (new centre, passes)"""
    center = list(center)
    n = 0
    for a, dim in enumerate((W, H, D)):
        c = int(cube_of(pos[a], center[a]))
        up = max(0, 3 - c)
        down = max(0, c - (dim - 4))
        center[a] += up - down
        n += up + down
    return center, n


def _map_frame(eng, rec, jump):
    p = rec["pose"].copy()
    p[3:] += np.float32(jump)
    aft, bef, reg = eng.mapping(p, rec["corner_last"], rec["surf_last"], rec["full_end"], stamp=0.1 * rec["k"])
    s = eng.stats()
    return {"aft": aft, "bef": bef, "registered": reg, "surround": eng.mapping_surround(),
            "mp_shifts": s["mp_grid_shifts"], "mp_iters": s["mp_iters"]}


@pytest.fixture(scope="module")
def stream(loam, oc, sg):
    """the recentring stream on the oracle (uninterrupted) and on engine A; A's map is exported on
    every frame the oracle publishes a surround cloud; after mapping frame SPLIT_AT a fresh engine
    B imports A's export, and both take the remaining frames from the oracle's recorded odometry"""
    sweeps = sg.stream_sweeps(34, 1)
    jumps = scenarios.GRID_JUMPS
    cfg = dict(system_delay=1)
    ro = scenarios.run_stream(oc.Oracle(oc.default_config(**cfg)), sweeps, jumps=jumps)
    A = loam.Engine(loam.default_config(**cfg))
    out = {"ro": [r for r in ro if "aft" in r], "A": [], "B": {}, "exports": {}}
    m = 0
    for k, sw in enumerate(sweeps):  # scenarios.run_stream's loop, with the export hooks
        rc, f = A.scan_registration(sw, stamp=0.1 * k)
        if rc != 0:
            continue
        pub, pose, cl, sl, full = A.odometry(f, stamp=0.1 * k)
        if pub != 7:
            continue
        rec = _map_frame(A, {"pose": pose, "corner_last": cl, "surf_last": sl, "full_end": full, "k": k},
                         jumps[m] if m < len(jumps) else (0, 0, 0))
        out["A"].append(rec)
        if out["ro"][m]["surround"] is not None:
            out["exports"][m] = A.map_export()
        m += 1
        if m == SPLIT_AT + 1:
            break
    B = loam.Engine(loam.default_config(**cfg))
    mA = A.map_export()
    out["dropped"] = B.map_import(mA["corner"], mA["surf"], mA["center"], mA["surround_phase"], mA["aft"], mA["bef"])
    out["split"] = (mA, B.map_export())
    for m in range(SPLIT_AT + 1, len(out["ro"])):
        o = out["ro"][m]
        jump = jumps[m] if m < len(jumps) else (0, 0, 0)
        out["A"].append(_map_frame(A, o, jump))
        out["B"][m] = _map_frame(B, o, jump)
        if o["surround"] is not None:
            out["exports"][m] = A.map_export()
    return out


def test_export_rebuilds_oracle_surround(stream, oc):
    ro, exports = stream["ro"], stream["exports"]
    frames = sorted(exports)
    assert len(frames) >= 3, frames
    center, shifted, after_shift = [10, 5, 10], False, 0
    for m, o in enumerate(ro):
        jump = scenarios.GRID_JUMPS[m] if m < len(scenarios.GRID_JUMPS) else (0, 0, 0)
        pos = _frame_position(ro[m - 1] if m else None, o, jump)
        center, n = _recentre(pos, center)
        assert n == o["mp_shifts"], (m, n, o["mp_shifts"])  # the numpy restatement agrees with the oracle
        shifted = shifted or n > 0
        if m not in exports:
            continue
        e = exports[m]
        after_shift += shifted
        _check_offsets(e)
        np.testing.assert_array_equal(e["center"], center, err_msg=f"center@{m}")
        np.testing.assert_array_equal(_bits(e["aft"]), _bits(stream["A"][m]["aft"]), err_msg=f"aft@{m}")
        np.testing.assert_array_equal(_bits(e["bef"]), _bits(stream["A"][m]["bef"]), err_msg=f"bef@{m}")
        assert e["surround_phase"] == 0, m  # (the frame just published)
        src = _surround_input(e, pos)
        outb = np.empty((max(src.shape[0], 1), 4), np.float32)
        n = oc.lib().oracle_voxel_grid(src.ctypes.data, src.shape[0], 0.2, outb.ctypes.data, outb.shape[0])
        print(f"frame {m}: map {e['corner'].shape[0]} + {e['surf'].shape[0]} points, surround input {src.shape[0]}, "
              f"surround {n} (oracle {o['surround'].shape[0]})")
        np.testing.assert_array_equal(outb[:n], o["surround"], err_msg=f"surround@{m}")
    assert after_shift >= 1


def test_round_trip_continues_stream(stream):
    mA, mB = stream["split"]
    assert stream["dropped"] == (0, 0)
    _check_offsets(mA)
    assert mA["corner"].shape[0] > 0 and mA["surf"].shape[0] > 0
    _map_eq(mA, mB, "B's export after the import")
    assert len(stream["B"]) >= 8
    assert max(stream["B"][m]["mp_shifts"] for m in stream["B"]) == 16  # the -1100 m jump
    for m, b in stream["B"].items():
        a, o = stream["A"][m], stream["ro"][m]
        for k in ("aft", "bef", "registered"):
            np.testing.assert_array_equal(_bits(b[k]), _bits(a[k]), err_msg=f"{k}@{m}")
        assert (b["surround"] is None) == (a["surround"] is None) == (o["surround"] is None), m
        if o["surround"] is not None:
            np.testing.assert_array_equal(_bits(b["surround"]), _bits(a["surround"]), err_msg=f"surround@{m}")
            np.testing.assert_array_equal(b["surround"], o["surround"], err_msg=f"surround@{m} (oracle)")
        assert (b["mp_shifts"], b["mp_iters"]) == (a["mp_shifts"], a["mp_iters"]) == (o["mp_shifts"], o["mp_iters"]), m
        assert np.abs(b["aft"] - o["aft"]).max() <= POSE_TOL, (m, b["aft"], o["aft"])
        assert np.abs(b["bef"] - o["bef"]).max() <= POSE_TOL, m
        _cloud_eq(b["registered"], o["registered"], f"registered@{m}")


CENTER3 = (12, 4, 9)
EDGES = np.array([25.0, -25.0, np.nextafter(np.float32(-25), np.float32(-np.inf)),
                  np.nextafter(np.float32(25), np.float32(-np.inf)), 525.0, -525.0, 524.99, -524.99, -75.0], np.float32)


def _bin_clouds():
    rng = np.random.default_rng(20261019)
    mid = np.array([50.0 * (10 - CENTER3[0]), 50.0 * (5 - CENTER3[1]), 50.0 * (10 - CENTER3[2])])
    half = np.array([546.0, 286.0, 546.0])

    def uniform(n):
        p = np.empty((n, 4), np.float32)
        p[:, :3] = (mid + rng.uniform(-1.0, 1.0, (n, 3)) * half).astype(np.float32)
        p[:, 3] = rng.uniform(0, 16, n).astype(np.float32)
        return p

    corner, surf = uniform(70001), uniform(200003)
    one = np.empty((50000, 4), np.float32)  # one cube: a single run across many tiles
    one[:, :3] = rng.uniform(-20.0, 20.0, (50000, 3)).astype(np.float32)
    one[:, 3] = np.arange(50000, dtype=np.float32)
    edge = np.zeros((3 * len(EDGES), 4), np.float32)  # the cube boundaries, on every axis
    for a in range(3):
        edge[a * len(EDGES):(a + 1) * len(EDGES), a] = EDGES
    edge[:, 3] = np.arange(edge.shape[0])
    bad = np.array([[np.nan, 0, 0, 1], [0, np.inf, 0, 2], [0, 0, -np.inf, 3], [np.nan, np.nan, np.nan, 4],
                    [1, 2, 3, np.nan]], np.float32)  # (the last one is kept: its coordinates are finite)
    return corner, np.concatenate([surf, one, edge, bad]), np.concatenate([edge, bad, corner[:5]])


def test_cube_formula_edges():
    # the issue's table for a centre index of 10 on the axis (21 = out above, -1 = out below)
    assert list(cube_of(EDGES, 10)) == [11, 10, 9, 10, 21, -1, 20, 0, 8]


def _expect(pts, center):
    key = cube_keys(pts, center)
    keep = key >= 0
    order = np.argsort(key[keep], kind="stable")
    off = np.concatenate([[0], np.cumsum(np.bincount(key[keep], minlength=NCUBE))]).astype(np.uint32)
    return pts[keep][order], off, int((~keep).sum())


def test_import_bins_like_stable_sort(loam):
    corner, surf, extra = _bin_clouds()
    corner = np.concatenate([corner, extra])
    for pts in (corner[:70001], surf[:200003]):  # the conditions on the drawn inputs
        key = cube_keys(pts, CENTER3)
        assert (key >= 0).mean() >= 0.85 and np.unique(key[key >= 0]).size >= 4000
    eng = loam.Engine(loam.default_config(map_capacity=1 << 19))
    aft = np.array([0.01, 0.02, 0.03, 1, 2, 3], np.float32)
    bef = np.array([0.04, 0.05, 0.06, 4, 5, 6], np.float32)
    empty = np.zeros((0, 4), np.float32)
    for c, s in ((corner, surf), (empty, surf), (corner, empty), (empty, empty)):
        dropped = eng.map_import(c, s, CENTER3, 2, aft, bef)
        m = eng.map_export()
        ec, es = _expect(c, CENTER3), _expect(s, CENTER3)
        print(f"import {c.shape[0]} + {s.shape[0]} points: kept {m['corner'].shape[0]} + {m['surf'].shape[0]}, "
              f"dropped {dropped}, largest cube {np.diff(es[1].astype(np.int64)).max()}")
        assert dropped == (ec[2], es[2])
        for kind, e in (("corner", ec), ("surf", es)):
            np.testing.assert_array_equal(m[kind + "_offset"], e[1], err_msg=kind)
            assert m[kind].shape == e[0].shape, kind
            np.testing.assert_array_equal(_bits(m[kind]), _bits(e[0]), err_msg=kind)
        np.testing.assert_array_equal(m["center"], CENTER3)
        assert m["surround_phase"] == 2
        np.testing.assert_array_equal(m["aft"], aft)
        np.testing.assert_array_equal(m["bef"], bef)


def test_errors_leave_map_alone(loam):
    rng = np.random.default_rng(5)
    eng = loam.Engine(loam.default_config(map_capacity=1024))

    def cloud(n):
        p = rng.uniform(-200, 200, (n, 4)).astype(np.float32)
        p[:, 1] *= 0.5
        return p

    aft = np.arange(6, dtype=np.float32)
    assert eng.map_import(cloud(300), cloud(500), (10, 5, 10), 1, aft, -aft) == (0, 0)
    before = eng.map_export()
    assert before["corner"].shape[0] == 300 and before["surf"].shape[0] == 500
    for c, s in ((cloud(2000), cloud(0)), (cloud(600), cloud(600))):  # 2000 in-grid points into 1024
        with pytest.raises(loam.LoamError) as ei:
            eng.map_import(c, s, (9, 5, 11), 3, -aft, aft)
        assert ei.value.code == loam.LOAM_E_CAPACITY
        _map_eq(before, eng.map_export(), "after a refused import")
    for kw in (dict(surround_phase=5), dict(surround_phase=-1), dict(center=(10, 5, (1 << 24) + 1)),
               dict(center=(-(1 << 24) - 1, 5, 10))):
        with pytest.raises(loam.LoamError) as ei:
            eng.map_import(cloud(10), cloud(10), **kw)
        assert ei.value.code == loam.LOAM_E_INVAL, kw
    _map_eq(before, eng.map_export(), "after invalid imports")
    # the sizes-only query, then too little room: counts and offsets filled, no point written
    L = loam.lib()
    m = loam.Map()
    assert L.loam_map_export(eng.h, ctypes.byref(m)) == loam.LOAM_OK
    assert (m.corner.count, m.surf.count, m.surround_phase) == (300, 500, 1)
    assert list(m.center) == [10, 5, 10]
    sent = np.full((500, 4), -7.5, np.float32)
    small = np.full((299, 4), -7.5, np.float32)
    offs = [np.full(NCUBE + 1, 0xFFFFFFFF, np.uint32) for _ in range(2)]
    m = loam.Map()
    m.corner.pts, m.corner.capacity, m.corner.cube_offset = small.ctypes.data, 299, offs[0].ctypes.data
    m.surf.pts, m.surf.capacity, m.surf.cube_offset = sent.ctypes.data, 500, offs[1].ctypes.data
    assert L.loam_map_export(eng.h, ctypes.byref(m)) == loam.LOAM_E_CAPACITY
    assert L.loam_last_error()
    assert (m.corner.count, m.surf.count) == (300, 500)
    np.testing.assert_array_equal(offs[0], before["corner_offset"])
    np.testing.assert_array_equal(offs[1], before["surf_offset"])
    assert np.all(sent == -7.5) and np.all(small == -7.5)
    _map_eq(before, eng.map_export(), "after a refused export")


def test_export_waits_for_deferred_update(loam, sg):
    sweeps = sg.stream_sweeps(10, 1)
    cfg = dict(system_delay=1)
    chain = loam.Engine(loam.default_config(**cfg))
    assert chain.get_tuning("stream_defer") == 1
    mapped = 0
    for k, sw in enumerate(sweeps):
        rc, pub, od, aft, bef, reg = chain.chain_sweep(sw, stamp=0.1 * k)
        mapped += aft is not None
    assert mapped >= 4
    nodes = loam.Engine(loam.default_config(**cfg))
    scenarios.run_stream(nodes, sweeps, stats=False)
    mc, mn = chain.map_export(), nodes.map_export()
    assert mc["corner"].shape[0] > 0 and mc["surf"].shape[0] > 0
    _check_offsets(mc)
    _map_eq(mc, mn, "chain_sweep against the node calls")
