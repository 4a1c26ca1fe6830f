"""loam_map_score on the GPU: many poses of one sweep scored against the whole streaming map in one
call, the context untouched.

The map is made in numpy and imported, never exported, so the reference (tests/score_ref.py: a
windowed brute force in numpy) does not depend on the code under test: the oracle's corner_last /
surf_last of mapping frames 0..3 of the 14-sweep synthetic stream, each put into the map frame with
its oracle aft in float64 and cast to float32.  The queries are frame 4's clouds.  Every
coordinate is below 128 m.

  1. exact tier: rotation zero (the queries pre-rotated on the host by frame 4's oracle rotation,
     the candidates translations of up to +-2 m about its position), where numpy restates the
     device's float arithmetic bit for bit: counts equal, costs within the bound of an fp64 sum
  2. rotated tier: +-4 deg / +-0.6 m about frame 4's oracle aft against a float64 reference, with
     the tolerance of a position error of DELTA (worked out below) and no more
  3. a pose's 32 bytes do not depend on n or on its place in the call (n = 1, 513, 65536)
  4. tile edges (cloud sizes 0, 1, T - 1, T, T + 1) and non-finite query points
  5. a large map (both tables beyond the hash build's LDS counters)
  6. the empty map
  7. the context is untouched: export, statistics, the rest of the stream, a pending deferred update
  8. errors leave out and the map alone
  9. relocalize = its steps composed by hand
"""
import ctypes

import numpy as np
import pytest

import scenarios
import score_ref as sr

pytestmark = pytest.mark.gpu

CFG = dict(system_delay=1)
POSE_TOL = 1e-4   # test_gpu_map.POSE_TOL (engine against oracle)
INT_TOL = 2e-6
TILE = 1024       # score.hpp kScoreTile: query points of one workgroup
# Rotated tier.  The device rounds to float seven times on the way from a query point to its map
# position (pose_math.hpp point_to_map: x1, y1, y2, z2, then x, y, z), each at most half an ulp of
# a value below 128 m (2^-17 m = 7.6e-6 m): a position error below 7 * 0.5 * 2^-17 * sqrt(3) =
# 4.7e-5 m; DELTA takes a margin of two.  The map points are the same floats on both sides.
DELTA = 1e-4
ROT_DIST = 0.5    # (the reference alone: at 0.3 / 0.5 / 1.0 m at most 0.18 % / 0.18 % / 0.04 % of a cloud's
                  # points lie within DELTA of the radius for these candidates, far below the 1 % allowed)
KEYS = ("corner_scored", "surf_scored", "corner_in", "surf_in", "corner_cost", "surf_cost")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _rows(res, idx=None):
    """rows idx of a map_score result as the 32 bytes loam_score_result holds, one row each"""
    n = res["corner_in"].shape[0]
    rec = np.empty(n, np.dtype([(k, np.float64 if k.endswith("cost") else np.uint32) for k in KEYS]))
    for k in KEYS:
        rec[k] = res[k]
    rec = rec if idx is None else rec[np.asarray(idx)]
    return rec.view(np.uint8).reshape(rec.shape[0], 32)


def _map_eq(a, b, msg=""):
    for k in ("corner", "surf", "aft", "bef"):
        assert a[k].shape == b[k].shape, (msg, k, a[k].shape, b[k].shape)
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{msg} {k}")
    for k in ("corner_offset", "surf_offset", "center"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{msg} {k}")
    assert a["surround_phase"] == b["surround_phase"], msg


def _candidates(base, n, seed):
    """test_gpu_localize._candidates: base pose + a seeded perturbation of up to +-4 deg / +-0.6 m,
    scaled by (h % 8 + 1) / 8"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1.0, 1.0, (n, 6)) * np.array([np.deg2rad(4.0)] * 3 + [0.6] * 3)
    d *= ((np.arange(n) % 8 + 1) / 8.0)[:, None]
    return (np.asarray(base, np.float64)[None, :] + d).astype(np.float32)


def _translations(base_t, n, seed):
    """poses (0, 0, 0, t): t = base_t + a seeded offset of up to +-2 m per axis scaled by
    (h % 8 + 1) / 8 (candidate 0: no offset), so that a call holds near and far guesses"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-2.0, 2.0, (n, 3)) * ((np.arange(n) % 8 + 1) / 8.0)[:, None]
    d[0] = 0.0
    p = np.zeros((n, 6), np.float32)
    p[:, 3:] = (np.asarray(base_t, np.float64)[None, :] + d).astype(np.float32)
    return p


def _subset(n):
    """the candidates checked against the reference: all up to 64; beyond, the first 8, the last 8
    and every 64th"""
    if n <= 64:
        return list(range(n))
    return sorted(set(range(8)) | set(range(n - 8, n)) | set(range(0, n, 64)))


def _with_w(xyz, w):
    return np.ascontiguousarray(np.c_[np.asarray(xyz, np.float32), np.asarray(w, np.float32)], np.float32)


@pytest.fixture(scope="module")
def world(loam, oc, sg):
    sweeps = sg.stream_sweeps(14, 1)
    ro = scenarios.run_stream(oc.Oracle(oc.default_config(**CFG)), sweeps)
    frames = [r for r in ro if "aft" in r]
    assert len(frames) >= 6, [r["k"] for r in frames]
    corner = np.concatenate([_with_w(sr.to_map64(f["aft"], f["corner_last"]), f["corner_last"][:, 3]) for f in frames[:4]])
    surf = np.concatenate([_with_w(sr.to_map64(f["aft"], f["surf_last"]), f["surf_last"][:, 3]) for f in frames[:4]])
    q = frames[4]
    qc, qs = np.ascontiguousarray(q["corner_last"], np.float32), np.ascontiguousarray(q["surf_last"], np.float32)
    assert max(np.abs(a[:, :3]).max() for a in (corner, surf, qc, qs)) < 126.0  # (+ 2 m of translation: below 128)
    E = loam.Engine(loam.default_config(**CFG))
    assert E.map_import(corner, surf) == (0, 0)
    # the exact tier's queries: frame 4's clouds under its oracle rotation alone
    rot = np.array(list(q["aft"][:3]) + [0.0, 0.0, 0.0], np.float32)
    qc0, qs0 = _with_w(sr.to_map64(rot, qc), qc[:, 3]), _with_w(sr.to_map64(rot, qs), qs[:, 3])
    return dict(sweeps=sweeps, frames=frames, corner=corner, surf=surf, qc=qc, qs=qs, qc0=qc0, qs0=qs0, E=E,
                smaps=(sr.SortedMap(corner), sr.SortedMap(surf)), trans=_translations(q["aft"][3:], 513, 20261101),
                near=_candidates(q["aft"], 513, 20261102), d2_cache={})


def _check_exact(res, h, ref, tag):
    """candidate h of a call's result against the float32 restatement: counts equal, each cost
    within N * 2^-52 * max(ref, 1) of the exactly rounded sum of the reference terms"""
    got = {k: res[k][h] for k in KEYS}
    print(f"{tag}[{h}]: got {({k: (float(v) if k.endswith('cost') else int(v)) for k, v in got.items()})} ref {ref}")
    for kind in ("corner", "surf"):
        assert int(got[kind + "_scored"]) == ref[kind + "_scored"], (tag, h, kind)
        assert int(got[kind + "_in"]) == ref[kind + "_in"], (tag, h, kind)
        c = ref[kind + "_cost"]
        bound = ref[kind + "_scored"] * 2.0 ** -52 * max(c, 1.0)
        assert abs(float(got[kind + "_cost"]) - c) <= bound, (tag, h, kind, float(got[kind + "_cost"]), c, bound)


@pytest.mark.parametrize("max_dist", [0.25, 1.0])
@pytest.mark.parametrize("n", [1, 5, 64, 513])
def test_exact_tier(world, n, max_dist):
    E, poses = world["E"], world["trans"][:n]
    res = E.map_score(world["qc0"], world["qs0"], poses, max_dist)
    assert all(res[k].shape == (n,) for k in KEYS)
    ins = []
    for h in _subset(n):
        ref = sr.exact_score(world["smaps"], (world["qc0"], world["qs0"]), poses[h][3:], max_dist, world["d2_cache"])
        _check_exact(res, h, ref, f"exact@{n}/{max_dist}")
        ins.append(ref["corner_in"] + ref["surf_in"])
    total = world["qc0"].shape[0] + world["qs0"].shape[0]
    assert np.all(res["corner_scored"] == world["qc0"].shape[0]) and np.all(res["surf_scored"] == world["qs0"].shape[0])
    if n >= 64:  # the compared candidates hold good and bad guesses
        assert max(ins) > 0.9 * total and min(ins) < 0.5 * total, (min(ins), max(ins), total)


@pytest.mark.parametrize("n", [5, 64])
def test_rotated_tier(world, n):
    E, poses = world["E"], world["near"][:n]
    res = E.map_score(world["qc"], world["qs"], poses, ROT_DIST)
    for h in _subset(n):
        ref = sr.float64_score(world["smaps"], (world["qc"], world["qs"]), poses[h], ROT_DIST, DELTA)
        print(f"rotated@{n}[{h}]: got {({k: (float(res[k][h]) if k.endswith('cost') else int(res[k][h])) for k in KEYS})} "
              f"ref {ref}")
        for kind in ("corner", "surf"):
            N, B = ref[kind + "_scored"], ref[kind + "_border"]
            assert int(res[kind + "_scored"][h]) == N, (h, kind)
            assert B <= 0.01 * N, (h, kind, B, N)  # (the tolerance below cannot hide a failure)
            assert abs(int(res[kind + "_in"][h]) - ref[kind + "_in"]) <= B, (h, kind, int(res[kind + "_in"][h]), ref)
            tol = N * (2.0 * ROT_DIST * DELTA + DELTA * DELTA + 2.0 ** -22 * ROT_DIST * ROT_DIST)
            assert abs(float(res[kind + "_cost"][h]) - ref[kind + "_cost"]) <= tol, (h, kind, float(res[kind + "_cost"][h]), ref, tol)


def test_independent_of_the_call(world, loam):
    E, C = world["E"], world["near"][:64]
    qc, qs = world["qc"], world["qs"]
    # the full clouds: alone, and inside n = 513 at both ends and in the middle
    p513 = world["near"].copy()
    picks = {0: 0, 255: 17, 512: 63}
    for pos, h in picks.items():
        p513[pos] = C[h]
    r513 = E.map_score(qc, qs, p513, ROT_DIST)
    for pos, h in picks.items():
        alone = E.map_score(qc, qs, C[h:h + 1], ROT_DIST)
        np.testing.assert_array_equal(_rows(alone), _rows(r513, [pos]), err_msg=f"candidate {h} alone / at {pos} of 513")
    np.testing.assert_array_equal(_rows(r513), _rows(E.map_score(qc, qs, p513, ROT_DIST)), err_msg="two identical calls")
    # every 8th query point: n = 65536 (the 64 poses 1024 times), 513 and alone
    qc8, qs8 = np.ascontiguousarray(qc[::8]), np.ascontiguousarray(qs[::8])
    assert loam.SCORE_MAX == 65536
    big = E.map_score(qc8, qs8, np.tile(C, (1024, 1)), ROT_DIST)
    rows = _rows(big).reshape(1024, 64, 32)
    np.testing.assert_array_equal(rows, np.broadcast_to(rows[:1], rows.shape), err_msg="the 1024 repeats of the 64 poses")
    r64 = E.map_score(qc8, qs8, C, ROT_DIST)
    np.testing.assert_array_equal(_rows(r64), rows[0], err_msg="n = 64 against the first 64 of 65536")
    np.testing.assert_array_equal(_rows(r64), rows[1023], err_msg="n = 64 against the last 64 of 65536")
    for h in (0, 17, 63):
        alone = E.map_score(qc8, qs8, C[h:h + 1], ROT_DIST)
        np.testing.assert_array_equal(_rows(alone), rows[511, h:h + 1], err_msg=f"candidate {h} alone / inside 65536")
    assert len({bytes(r) for r in rows[0]}) == 64  # (64 different results: the comparison is no trivial one)
    # more poses than one call takes: the binding loops
    over = E.map_score(qc8, qs8, np.tile(C, (1025, 1)), ROT_DIST)
    np.testing.assert_array_equal(_rows(over)[-64:], rows[0], err_msg="the poses beyond SCORE_MAX")


@pytest.mark.parametrize("sizes", [(0, TILE + 1), (1, TILE), (TILE - 1, 1), (TILE, 0), (TILE + 1, TILE - 1), (0, 0)])
def test_tile_edges(world, sizes):
    """cloud sizes around the workgroup's tile, corner and surf independently (the corner queries
    are surf points here: frame 4 has fewer corner points than a tile)"""
    E, poses = world["E"], world["trans"][[0, 9, 23]]
    qc, qs = world["qs0"][1000:1000 + sizes[0]], world["qs0"][3000:3000 + sizes[1]]
    res = E.map_score(qc, qs, poses, 1.0)
    for h in range(3):
        _check_exact(res, h, sr.exact_score(world["smaps"], (qc, qs), poses[h][3:], 1.0), f"sizes {sizes}")
    assert np.all(res["corner_scored"] == sizes[0]) and np.all(res["surf_scored"] == sizes[1])


def test_non_finite_points_are_not_scored(world):
    E, poses = world["E"], world["trans"][[0, 9, 23]]
    qc, qs = world["qc0"].copy(), world["qs0"][:2 * TILE + 100].copy()
    bad_c, bad_s = [0, 100, 545], [0, 1, TILE - 1, TILE, TILE + 500, 2 * TILE + 99]
    for k, i in enumerate(bad_c):
        qc[i, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    for k, i in enumerate(bad_s):
        qs[i, k % 3] = (np.inf, -np.inf, np.nan)[k % 3]
    qs[5, 3] = np.nan  # (the fourth component is not a coordinate: the point is scored)
    res = E.map_score(qc, qs, poses, 1.0)
    assert np.all(res["corner_scored"] == qc.shape[0] - len(bad_c)) and np.all(res["surf_scored"] == qs.shape[0] - len(bad_s))
    clean_c, clean_s = np.delete(qc, bad_c, axis=0), np.delete(qs, bad_s, axis=0)
    clean = E.map_score(clean_c, clean_s, poses, 1.0)
    for h in range(3):
        _check_exact(res, h, sr.exact_score(world["smaps"], (qc, qs), poses[h][3:], 1.0), "non-finite")
        for k in ("corner_scored", "surf_scored", "corner_in", "surf_in"):  # the rest unchanged
            assert res[k][h] == clean[k][h], (k, h)


@pytest.mark.parametrize("n", [5, 64])
def test_large_map(world, loam, n):
    """the same map plus uniform noise points, as test_gpu_localize's dense map: both kinds' tables
    are beyond the hash build's 8192 LDS counters (counters in global memory)"""
    if "large" not in world:
        rng = np.random.default_rng(20261021)

        def noise(k):
            p = np.empty((k, 4), np.float32)
            p[:, :3] = (rng.uniform(-1.0, 1.0, (k, 3)) * np.array([120.0, 70.0, 120.0])).astype(np.float32)
            p[:, 3] = rng.uniform(0, 16, k).astype(np.float32)
            return p

        corner, surf = np.concatenate([world["corner"], noise(30000)]), np.concatenate([world["surf"], noise(150000)])
        L = loam.Engine(loam.default_config(**CFG))
        assert L.map_import(corner, surf) == (0, 0)
        world["large"] = (L, (sr.SortedMap(corner), sr.SortedMap(surf)), {})
    L, smaps, cache = world["large"]
    assert min(s.x.shape[0] for s in smaps) > 8192
    qc, qs = np.ascontiguousarray(world["qc0"][::4]), np.ascontiguousarray(world["qs0"][::8])
    poses = world["trans"][:n]
    res = L.map_score(qc, qs, poses, 1.0)
    for h in range(n):
        _check_exact(res, h, sr.exact_score(smaps, (qc, qs), poses[h][3:], 1.0, cache), f"large@{n}")


def test_empty_map(world, loam):
    eng = loam.Engine(loam.default_config(**CFG))
    for max_dist in (0.25, 1.0, 0.3):
        res = eng.map_score(world["qc"], world["qs"], world["near"][:5], max_dist)
        r2 = float(np.float32(max_dist) * np.float32(max_dist))
        assert np.all(res["corner_in"] == 0) and np.all(res["surf_in"] == 0)
        assert np.all(res["corner_scored"] == world["qc"].shape[0]) and np.all(res["surf_scored"] == world["qs"].shape[0])
        assert np.all(res["corner_cost"] == world["qc"].shape[0] * r2), (res["corner_cost"], r2)
        assert np.all(res["surf_cost"] == world["qs"].shape[0] * r2), (res["surf_cost"], r2)
    e = eng.map_export()
    assert e["corner"].shape[0] == 0 and e["surf"].shape[0] == 0 and e["surround_phase"] == 4


def _map_frame(eng, o):
    aft, bef, reg = eng.mapping(o["pose"], o["corner_last"], o["surf_last"], o["full_end"], stamp=0.1 * o["k"])
    s = eng.stats()
    return {"aft": aft, "bef": bef, "registered": reg, "surround": eng.mapping_surround(), "mp_iters": s["mp_iters"]}


def _stream_engine(loam, sweeps, frames_wanted):
    """an engine after `frames_wanted` mapping frames of the stream through the node calls"""
    A = loam.Engine(loam.default_config(**CFG))
    m = 0
    for k, sw in enumerate(sweeps):
        rc, f = A.scan_registration(sw, stamp=0.1 * k)
        if rc != 0:
            continue
        pub, pose, cl, sl, full = A.odometry(f, stamp=0.1 * k)
        if pub != 7:
            continue
        A.mapping(pose, cl, sl, full, stamp=0.1 * k)
        A.mapping_surround()
        m += 1
        if m == frames_wanted:
            break
    return A


def test_context_untouched_and_stream_continues(world, loam):
    sweeps, frames = world["sweeps"], world["frames"]
    A = _stream_engine(loam, sweeps, 4)  # the map after the frame of sweep 8
    M = A.map_export()
    K = loam.Engine(loam.default_config(**CFG))  # the control: the same map, no score call
    K.map_import(M["corner"], M["surf"], M["center"], M["surround_phase"], M["aft"], M["bef"])
    poses = world["near"][:64]
    stats0 = A.stats()
    r1 = A.map_score(world["qc"], world["qs"], poses, ROT_DIST)
    r2 = A.map_score(world["qc"], world["qs"], poses, ROT_DIST)
    np.testing.assert_array_equal(_rows(r1), _rows(r2), err_msg="two identical calls")
    np.testing.assert_array_equal(_rows(r1), _rows(K.map_score(world["qc"], world["qs"], poses, ROT_DIST)),
                                  err_msg="the stream's engine against the one that imported its map")
    assert r1["surf_in"].max() > 0.5 * world["qs"].shape[0]
    K.map_import(M["corner"], M["surf"], M["center"], M["surround_phase"], M["aft"], M["bef"])  # (K: no call before the frames)
    _map_eq(M, A.map_export(), "after two 64-pose calls")
    assert A.stats() == stats0
    for m in range(4, len(frames)):
        o = frames[m]
        a, k = _map_frame(A, o), _map_frame(K, o)
        for key in ("aft", "bef", "registered"):
            np.testing.assert_array_equal(_bits(a[key]), _bits(k[key]), err_msg=f"{key}@{m}")
        assert (a["surround"] is None) == (k["surround"] is None) == (o["surround"] is None), m
        if o["surround"] is not None:
            np.testing.assert_array_equal(_bits(a["surround"]), _bits(k["surround"]), err_msg=f"surround@{m}")
        assert a["mp_iters"] == k["mp_iters"] == o["mp_iters"], m
        assert np.abs(a["aft"] - o["aft"]).max() <= POSE_TOL, (m, a["aft"], o["aft"])
        np.testing.assert_array_equal(a["registered"][:, :3], o["registered"][:, :3], err_msg=f"registered@{m}")
        assert np.max(np.abs(a["registered"][:, 3] - o["registered"][:, 3])) <= INT_TOL, m
        if m == 4:  # between two frames as well
            A.map_score(world["qc"], world["qs"], poses[:5], 1.0)
    _map_eq(A.map_export(), K.map_export(), "at the end of the stream")


def test_waits_for_deferred_update(world, loam):
    sweeps = world["sweeps"]
    poses = world["near"][:5]
    res, maps = [], []
    for drain in (False, True):
        ch = loam.Engine(loam.default_config(**CFG))
        assert ch.get_tuning("stream_defer") == 1
        mapped = 0
        for k, sw in enumerate(sweeps[:9]):  # through sweep 8 = the fourth mapping frame, its map update deferred
            rc, pub, od, a, b, reg = ch.chain_sweep(sw, stamp=0.1 * k)
            mapped += a is not None
        assert mapped == 4
        if drain:
            maps.append(ch.map_export())  # (waits for the update)
        res.append(ch.map_score(world["qc"], world["qs"], poses, ROT_DIST))
        maps.append(ch.map_export())
    np.testing.assert_array_equal(_rows(res[0]), _rows(res[1]), err_msg="right after chain_sweep against after a drain")
    _map_eq(maps[0], maps[1], "the map after the call against the drained one")
    _map_eq(maps[1], maps[2], "the drained map before and after the call")
    # the same map through the node calls
    A = _stream_engine(loam, sweeps, 4)
    _map_eq(maps[0], A.map_export(), "chain_sweep's map against the node calls'")
    np.testing.assert_array_equal(_rows(res[0]), _rows(A.map_score(world["qc"], world["qs"], poses, ROT_DIST)))


def test_errors_leave_out_and_map_alone(world, loam):
    L, E = loam.lib(), world["E"]
    M = E.map_export()
    P = ctypes.POINTER(loam.Pose6)
    n = 3
    poses = np.ascontiguousarray(world["near"][:n])
    cl, sl = world["qc"], world["qs"]
    big = np.zeros((int(E.cfg.max_points) + 1, 4), np.float32)

    def cloud(a, null=False):
        return loam.CloudOut(None if null else a.ctypes.data, a.shape[0], a.shape[0])

    good = dict(ctx=E.h, corner=ctypes.byref(cloud(cl)), surf=ctypes.byref(cloud(sl)), max_dist=0.5, n=n,
                pose=poses.ctypes.data_as(P))
    cases = {
        "null corner": dict(corner=None),
        "null surf": dict(surf=None),
        "null pose": dict(pose=None),
        "n == 0": dict(n=0),
        "n > LOAM_SCORE_MAX": dict(n=loam.SCORE_MAX + 1),
        "max_dist 0": dict(max_dist=0.0),
        "max_dist < 0": dict(max_dist=-0.5),
        "max_dist just above 1": dict(max_dist=float(np.nextafter(np.float32(1.0), np.float32(2.0)))),
        "max_dist NaN": dict(max_dist=float("nan")),
        "max_dist inf": dict(max_dist=float("inf")),
        "corner pts null": dict(corner=ctypes.byref(cloud(cl, null=True))),
        "surf pts null": dict(surf=ctypes.byref(cloud(sl, null=True))),
        "corner beyond max_points": dict(corner=ctypes.byref(cloud(big))),
        "surf beyond max_points": dict(surf=ctypes.byref(cloud(big))),
    }
    out = (loam.ScoreResult * (loam.SCORE_MAX + 1))()
    pattern = bytes([0xA5]) * ctypes.sizeof(out)
    for name, kw in cases.items():
        a = dict(good, **kw)
        ctypes.memmove(out, pattern, len(pattern))
        rc = L.loam_map_score(a["ctx"], a["corner"], a["surf"], a["max_dist"], a["n"], a["pose"], out)
        assert rc == loam.LOAM_E_INVAL, (name, rc)
        assert L.loam_last_error(), name
        assert bytes(out) == pattern, name
        _map_eq(M, E.map_export(), f"after {name}")
    assert L.loam_map_score(E.h, good["corner"], good["surf"], 0.5, n, good["pose"], None) == loam.LOAM_E_INVAL
    _map_eq(M, E.map_export(), "after a null out")
    # the calls above were refused, this one (max_dist exactly 1) is not
    ctypes.memmove(out, pattern, len(pattern))
    assert L.loam_map_score(E.h, good["corner"], good["surf"], 1.0, n, good["pose"], out) == loam.LOAM_OK
    assert all(out[h].surf_scored == sl.shape[0] and out[h].surf_in > 0 for h in range(n))
    assert bytes(out)[n * 32:] == pattern[n * 32:]


def test_overflowed_store_is_refused(world, loam):
    rec = world["frames"][4]
    small = loam.Engine(loam.default_config(map_capacity=1024, **CFG))
    with pytest.raises(loam.LoamError) as ei:  # the frame's map update does not fit 1024 points
        small.mapping(rec["pose"], rec["corner_last"], rec["surf_last"], rec["full_end"])
    assert ei.value.code == loam.LOAM_E_CAPACITY
    L, P = loam.lib(), ctypes.POINTER(loam.Pose6)
    poses = np.ascontiguousarray(world["near"][:2])
    cl, sl = world["qc"], world["qs"]
    out = (loam.ScoreResult * 2)()
    pattern = bytes([0xA5]) * ctypes.sizeof(out)
    ctypes.memmove(out, pattern, len(pattern))
    rc = L.loam_map_score(small.h, ctypes.byref(loam.CloudOut(cl.ctypes.data, cl.shape[0], cl.shape[0])),
                          ctypes.byref(loam.CloudOut(sl.ctypes.data, sl.shape[0], sl.shape[0])), 0.5, 2,
                          poses.ctypes.data_as(P), out)
    assert rc == loam.LOAM_E_INVAL and L.loam_last_error()
    assert bytes(out) == pattern


def test_relocalize_equals_its_steps(world, loam):
    """a yaw x x x z grid about frame 4's pose (ry is the yaw: y is the vertical axis)"""
    E, o = world["E"], world["frames"][4]
    qc, qs = world["qc"], world["qs"]
    yaw = np.deg2rad(np.arange(-7, 8, 1.0))
    step = np.arange(-7, 8) * 0.2
    g = np.array([(dy, dx, dz) for dy in yaw for dx in step for dz in step])
    grid = np.tile(np.asarray(o["aft"], np.float64), (g.shape[0], 1))
    grid[:, 1] += g[:, 0]
    grid[:, 3] += g[:, 1]
    grid[:, 5] += g[:, 2]
    grid = grid.astype(np.float32)
    assert grid.shape[0] == 3375
    keep = 64
    got = E.relocalize(qc, qs, grid, keep=keep, max_dist=ROT_DIST)

    def order(s, index):
        n_in = s["corner_in"].astype(np.int64) + s["surf_in"]
        cost = s["corner_cost"] + s["surf_cost"]
        return sorted(range(len(index)), key=lambda i: (-int(n_in[i]), float(cost[i]), int(index[i])))

    coarse = E.map_score(qc, qs, grid, ROT_DIST)
    idx = np.array(order(coarse, np.arange(grid.shape[0]))[:keep])
    loc = E.map_localize(np.zeros(6, np.float32), qc, qs, grid[idx])
    fine = {k: coarse[k][idx].copy() for k in KEYS}
    ok = np.flatnonzero(loc["status"] == loam.LOC_SOLVED)
    s = E.map_score(qc, qs, loc["aft"][ok], ROT_DIST)
    for k in KEYS:
        fine[k][ok] = s[k]
    fo = np.array(order(fine, idx))
    np.testing.assert_array_equal(got["index"], idx[fo])
    for k in loc:
        np.testing.assert_array_equal(_bits(got["localize"][k]) if k == "aft" else got["localize"][k],
                                      _bits(loc[k][fo]) if k == "aft" else loc[k][fo], err_msg=k)
    np.testing.assert_array_equal(_rows(got["coarse"]), _rows(coarse, idx[fo]))
    np.testing.assert_array_equal(_rows(got["fine"]), _rows(fine, fo))
    assert len(ok) > 0
    best = got["localize"]["aft"][0]
    print(f"relocalize: {grid.shape[0]} guesses, kept {keep}, {len(ok)} solved; best guess {grid[got['index'][0]]} "
          f"-> refined {best}; oracle aft {o['aft']}; |refined - oracle| rot {np.abs(best[:3] - o['aft'][:3]).max():.3g} rad, "
          f"trans {np.linalg.norm(best[3:] - o['aft'][3:]):.3g} m; coarse in {int(got['coarse']['corner_in'][0]) + int(got['coarse']['surf_in'][0])} "
          f"fine in {int(got['fine']['corner_in'][0]) + int(got['fine']['surf_in'][0])} of {qc.shape[0] + qs.shape[0]}")
    with pytest.raises(ValueError):
        E.relocalize(qc, qs, grid, keep=loam.LOCALIZE_MAX + 1)
