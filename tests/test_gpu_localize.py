"""loam_map_localize on the GPU: n candidate poses of one sweep against the streaming map in one
call, the context untouched.

The specification under test: out[h] is what one loam_mapping on a context holding the same map,
transformBefMapped = bef[h] and transformAftMapped = aft[h] would return in aft and report in its
statistics.  The comparator is exactly that, built from entry points that predate the call: one
engine, map_import(M, aft, bef) then mapping(rec) and stats(), once per candidate.

The map M is engine A's after mapping frame M0 of the 14-sweep synthetic stream (the frame of sweep
8; this stream maps every second sweep, 6 frames in all); rec is the oracle's record of frame
M0 + 1 (its odometry pose and clouds).

  1. n = 1 at M's own (aft, bef) = the oracle's frame M0 + 1
  2. seeded perturbed candidates (up to +-0.6 m, +-4 deg; a second set with bef = NULL) at n = 1, 4,
     5, 64, 513 (the launch shapes: mp_small_max 4 | 5, the query grid at 64, the fit grid at 512)
     = the comparator, bit for bit in aft and equal in every count; the same at n = 5, 64 on a dense
     map (FromMap beyond the hash build's LDS counters, several gather tiles per workgroup)
  3. an empty-cube guess (NO_LM) and an off-grid guess (OFFGRID) beside ordinary candidates
  4. the context is untouched: export, statistics, the rest of the stream, a pending deferred update
  5. errors leave out and the map alone
"""
import ctypes

import numpy as np
import pytest

import scenarios

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4   # test_gpu_map.POSE_TOL (engine against oracle)
INT_TOL = 2e-6
M0 = 3            # the mapping frame of sweep 8
CFG = dict(system_delay=1)
MAX_ITER = 10     # loam_config_default's mp_max_iter
COUNTS = ("status", "iters", "degenerate_steps", "rows_last", "rows_sum", "stack_corner", "stack_surf",
          "map_corner", "map_surf")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _map_eq(a, b, msg=""):
    for k in ("corner", "surf", "aft", "bef"):
        assert a[k].shape == b[k].shape, (msg, k, a[k].shape, b[k].shape)
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{msg} {k}")
    for k in ("corner_offset", "surf_offset", "center"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{msg} {k}")
    assert a["surround_phase"] == b["surround_phase"], msg


def _res_eq(a, b, msg="", idx_a=None, idx_b=None):
    """two map_localize results (or rows idx_a of a against rows idx_b of b), byte for byte"""
    for k in a:
        x = a[k] if idx_a is None else a[k][idx_a]
        y = b[k] if idx_b is None else b[k][idx_b]
        np.testing.assert_array_equal(_bits(x) if k == "aft" else x, _bits(y) if k == "aft" else y, err_msg=f"{msg} {k}")


def _import(eng, m, aft=None, bef=None):
    return eng.map_import(m["corner"], m["surf"], m["center"], m["surround_phase"],
                          m["aft"] if aft is None else aft, bef)


def _map_frame(eng, o):
    aft, bef, reg = eng.mapping(o["pose"], o["corner_last"], o["surf_last"], o["full_end"], stamp=0.1 * o["k"])
    s = eng.stats()
    return {"aft": aft, "bef": bef, "registered": reg, "surround": eng.mapping_surround(), "mp_iters": s["mp_iters"]}


def _candidates(base, n, seed):
    """base pose + a seeded perturbation of up to +-4 deg / +-0.6 m, scaled by (h % 8 + 1) / 8 so that
    every call holds guesses that converge early and guesses that use every iteration"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1.0, 1.0, (n, 6)) * np.array([np.deg2rad(4.0)] * 3 + [0.6] * 3)
    d *= ((np.arange(n) % 8 + 1) / 8.0)[:, None]
    return (np.asarray(base, np.float64)[None, :] + d).astype(np.float32)


def _subset(n):
    """the candidates checked against the comparator: all up to 64; beyond, the first 40, the last 8
    and every 16th"""
    if n <= 64:
        return list(range(n))
    return sorted(set(range(40)) | set(range(n - 8, n)) | set(range(0, n, 16)))


@pytest.fixture(scope="module")
def world(loam, oc, sg):
    sweeps = sg.stream_sweeps(14, 1)
    ro = scenarios.run_stream(oc.Oracle(oc.default_config(**CFG)), sweeps)
    frames = [r for r in ro if "aft" in r]
    assert len(frames) >= M0 + 3 and frames[M0]["k"] == 8, [r["k"] for r in frames]
    A = loam.Engine(loam.default_config(**CFG))
    m = 0
    for k, sw in enumerate(sweeps):  # scenarios.run_stream's loop, stopped after mapping frame M0
        rc, f = A.scan_registration(sw, stamp=0.1 * k)
        if rc != 0:
            continue
        pub, pose, cl, sl, full = A.odometry(f, stamp=0.1 * k)
        if pub != 7:
            continue
        A.mapping(pose, cl, sl, full, stamp=0.1 * k)
        A.mapping_surround()
        m += 1
        if m == M0 + 1:
            break
    M = A.map_export()
    assert M["corner"].shape[0] > 100 and M["surf"].shape[0] > 1000
    rec = frames[M0 + 1]
    # the engine the localization calls run on: M imported (test 4 keeps A for itself)
    E = loam.Engine(loam.default_config(**CFG))
    assert _import(E, M, bef=M["bef"]) == (0, 0)
    C = loam.Engine(loam.default_config(**CFG))  # the comparator's engine, re-imported per candidate

    def comparator(m):
        """the comparator on map m: (aft, bef) -> one sequential frame's aft and statistics"""
        cache = {}

        def compare(aft, bef):
            aft = np.ascontiguousarray(aft, np.float32)
            key = (aft.tobytes(), None if bef is None else np.ascontiguousarray(bef, np.float32).tobytes())
            if key not in cache:
                _import(C, m, aft=aft, bef=bef)
                a, b, _ = C.mapping(rec["pose"], rec["corner_last"], rec["surf_last"], rec["full_end"])
                cache[key] = (a, C.stats())
            return cache[key]
        return compare

    compare = comparator(M)

    def localize(eng, aft, bef=None):
        return eng.map_localize(rec["pose"], rec["corner_last"], rec["surf_last"], aft, bef)

    near = _candidates(M["aft"], 513, 20261019)         # bef = M's
    fresh = _candidates(rec["aft"], 513, 20261020)      # bef = NULL, aft near rec's map pose
    return dict(sweeps=sweeps, frames=frames, A=A, M=M, rec=rec, E=E, compare=compare, comparator=comparator,
                localize=localize, near=near, fresh=fresh)


def _check_against_comparator(world, res, aft, bef, idx, tag, compare=None):
    """the candidates idx of a call's result = the comparator's frames (on the stream map, or the given
    comparator's); returns their iteration counts"""
    iters = []
    for h in idx:
        ca, cs = (compare or world["compare"])(aft[h], None if bef is None else bef[h])
        got = {k: int(res[k][h]) for k in COUNTS}
        print(f"{tag}[{h}]: {got}  sequential: iters {cs['mp_iters']} rows {cs['mp_rows_sum']} "
              f"stack {cs['mp_stack']} map {cs['mp_map_points']}  |aft - sequential| "
              f"{np.abs(res['aft'][h] - ca).max():.3g}")
        np.testing.assert_array_equal(_bits(res["aft"][h]), _bits(ca), err_msg=f"{tag} aft[{h}]")
        assert got["iters"] == cs["mp_iters"], (tag, h)
        assert got["rows_sum"] == cs["mp_rows_sum"], (tag, h)
        assert got["degenerate_steps"] == cs["mp_degenerate_steps"], (tag, h)
        assert got["stack_corner"] + got["stack_surf"] == cs["mp_stack"], (tag, h)
        assert got["map_corner"] + got["map_surf"] == cs["mp_map_points"], (tag, h)
        assert got["status"] == (0 if got["map_corner"] > 10 and got["map_surf"] > 100 else 1), (tag, h)
        assert got["rows_last"] <= got["rows_sum"] and (got["iters"] > 1 or got["rows_last"] == got["rows_sum"]), (tag, h)
        iters.append(got["iters"])
    return iters


def test_anchor_to_oracle(world, loam):
    M, o = world["M"], world["frames"][M0 + 1]
    res = world["localize"](world["E"], M["aft"][None, :], M["bef"][None, :])
    print(f"anchor: status {res['status'][0]} iters {res['iters'][0]} (oracle {o['mp_iters']}) rows_last "
          f"{res['rows_last'][0]} |aft - oracle| {np.abs(res['aft'][0] - o['aft']).max():.3g}")
    assert res["status"][0] == loam.LOC_SOLVED
    assert res["iters"][0] == o["mp_iters"]
    assert np.abs(res["aft"][0] - o["aft"]).max() <= POSE_TOL
    np.testing.assert_array_equal(_bits(res["aft"][0]), _bits(o["aft"]))  # (0 on this stream: bit for bit)
    _check_against_comparator(world, res, M["aft"][None, :], M["bef"][None, :], [0], "anchor")


@pytest.mark.parametrize("n", [1, 4, 5, 64, 513])
def test_equals_sequential_frames(world, loam, n):
    M = world["M"]
    bef = np.tile(M["bef"], (n, 1))
    for tag, aft, b in (("near", world["near"][:n], bef), ("fresh", world["fresh"][:n], None)):
        res = world["localize"](world["E"], aft, b)
        assert res["aft"].shape == (n, 6) and all(res[k].shape == (n,) for k in COUNTS)
        iters = _check_against_comparator(world, res, aft, b, _subset(n), f"{tag}@{n}")
        assert np.all(res["status"] == loam.LOC_SOLVED), tag
        assert np.all((res["iters"] >= 1) & (res["iters"] <= MAX_ITER)), tag
        print(f"{tag}@{n}: compared candidates' iterations {sorted(iters)}")
        # the compared candidates of either set are no trivial ones: some use every iteration, some
        # converge before (asserted where the set holds every perturbation scale several times)
        if n >= 64:
            assert max(iters) == MAX_ITER and min(iters) < MAX_ITER, (tag, iters)


@pytest.mark.parametrize("n", [5, 64])
def test_dense_map_equals_sequential_frames(world, loam, n):
    """a map whose candidates hold tens of thousands of FromMap points: the surf part is beyond the hash
    build's 8192 LDS counters (the grid-per-cloud build the call then asks for, tables in global
    memory), and a gather workgroup takes several 1024-point tiles.  The map: the stream map plus
    uniform points about the origin (too sparse to enter a 5-NN within 1 m often)"""
    M = world["M"]
    rng = np.random.default_rng(20261021)

    def noise(k):
        p = np.empty((k, 4), np.float32)
        p[:, :3] = (rng.uniform(-1.0, 1.0, (k, 3)) * np.array([120.0, 70.0, 120.0])).astype(np.float32)
        p[:, 3] = rng.uniform(0, 16, k).astype(np.float32)
        return p

    D = dict(M, corner=np.concatenate([M["corner"], noise(30000)]), surf=np.concatenate([M["surf"], noise(150000)]))
    E = loam.Engine(loam.default_config(**CFG))
    assert _import(E, D, bef=M["bef"]) == (0, 0)
    aft, bef = world["near"][:n], np.tile(M["bef"], (n, 1))
    res = world["localize"](E, aft, bef)
    total = res["map_corner"].astype(np.int64) + res["map_surf"]
    print(f"dense@{n}: FromMap corner {res['map_corner'].min()}-{res['map_corner'].max()}, surf "
          f"{res['map_surf'].min()}-{res['map_surf'].max()}")
    assert res["map_surf"].min() > 8192              # every candidate's surf index is built by the grid form
    assert total.min() > 32 * 1024                   # at n = 64 (32 workgroups per candidate) every workgroup loops
    assert np.all(res["status"] == loam.LOC_SOLVED)
    iters = _check_against_comparator(world, res, aft, bef, range(n), f"dense@{n}", compare=world["comparator"](D))
    assert min(iters) < MAX_ITER, iters


def test_one_iteration_rows_last_is_rows_sum(world, loam):
    M = world["M"]
    E1 = loam.Engine(loam.default_config(mp_max_iter=1, **CFG))
    _import(E1, M, bef=M["bef"])
    for n in (4, 5):
        res = world["localize"](E1, world["near"][:n], np.tile(M["bef"], (n, 1)))
        assert np.all(res["status"] == loam.LOC_SOLVED) and np.all(res["iters"] == 1)
        assert np.all(res["rows_last"] > 0)
        np.testing.assert_array_equal(res["rows_last"], res["rows_sum"])


def test_special_candidates_beside_ordinary_ones(world, loam):
    M, E = world["M"], world["E"]
    assert list(M["center"]) == [10, 5, 10]
    # inside the grid, among cubes no frame has filled: centre cube 16, its 5x5x5 neighbourhood 14..18
    # (at 120 m the centre cube is 12, whose neighbourhood 10..14 still holds the origin's cubes:
    # measured 1128 + 5587 FromMap points there, an L-M of 10 iterations with no accepted row)
    far = M["aft"].copy()
    far[3] += np.float32(300.0)
    off = M["aft"].copy()
    off[3] = np.float32(450.0)        # centre cube 19 of 21: within 3 of the edge
    far120 = M["aft"].copy()
    far120[3] += np.float32(120.0)    # (an L-M on the origin's cubes seen from afar: as the sequential frame)
    aft = np.stack([world["near"][7], far, world["near"][2], off, world["near"][12], far120])
    bef = np.tile(M["bef"], (6, 1))
    res = world["localize"](E, aft, bef)
    print({k: res[k].tolist() for k in COUNTS})
    assert res["status"].tolist()[:5] == [loam.LOC_SOLVED, loam.LOC_NO_LM, loam.LOC_SOLVED, loam.LOC_OFFGRID,
                                          loam.LOC_SOLVED]
    # NO_LM: the sequential frame's aft and counts
    _check_against_comparator(world, res, aft, bef, [1], "far")
    assert res["iters"][1] == 0 and res["rows_sum"][1] == 0 and res["rows_last"][1] == 0
    assert res["map_corner"][1] <= 10 or res["map_surf"][1] <= 100
    assert res["stack_corner"][1] > 0 and res["stack_surf"][1] > 0
    # OFFGRID: the guess back, every count 0
    np.testing.assert_array_equal(_bits(res["aft"][3]), _bits(off))
    for k in COUNTS[1:]:
        assert res[k][3] == 0, k
    # the ordinary ones: as when run alone
    for h in (0, 2, 4):
        alone = world["localize"](E, aft[h][None, :], bef[h][None, :])
        _res_eq(res, alone, f"candidate {h} alone", idx_a=[h], idx_b=[0])
    _check_against_comparator(world, res, aft, bef, [0, 2, 4, 5], "ordinary")


def test_context_untouched_and_stream_continues(world, loam):
    A, M, frames = world["A"], world["M"], world["frames"]
    K = loam.Engine(loam.default_config(**CFG))  # the control: the same map, no localization call
    _import(K, M, bef=M["bef"])
    bef = np.tile(M["bef"], (64, 1))
    stats0 = A.stats()
    r1 = world["localize"](A, world["near"][:64], bef)
    r2 = world["localize"](A, world["near"][:64], bef)
    _res_eq(r1, r2, "two identical calls")
    _res_eq(r1, world["localize"](world["E"], world["near"][:64], bef), "A against the engine that imported M")
    _map_eq(M, A.map_export(), "after a 64-candidate call")
    assert A.stats() == stats0
    published = 0
    for m in range(M0 + 1, len(frames)):
        o = frames[m]
        a, k = _map_frame(A, o), _map_frame(K, o)
        for key in ("aft", "bef", "registered"):
            np.testing.assert_array_equal(_bits(a[key]), _bits(k[key]), err_msg=f"{key}@{m}")
        assert (a["surround"] is None) == (k["surround"] is None) == (o["surround"] is None), m
        if o["surround"] is not None:
            published += 1
            np.testing.assert_array_equal(_bits(a["surround"]), _bits(k["surround"]), err_msg=f"surround@{m}")
            np.testing.assert_array_equal(a["surround"], o["surround"], err_msg=f"surround@{m} (oracle)")
        assert a["mp_iters"] == k["mp_iters"] == o["mp_iters"], m
        assert np.abs(a["aft"] - o["aft"]).max() <= POSE_TOL, (m, a["aft"], o["aft"])
        assert np.abs(a["bef"] - o["bef"]).max() <= POSE_TOL, m
        assert a["registered"].shape == o["registered"].shape, m
        np.testing.assert_array_equal(a["registered"][:, :3], o["registered"][:, :3], err_msg=f"registered@{m}")
        assert np.max(np.abs(a["registered"][:, 3] - o["registered"][:, 3])) <= INT_TOL, m
    assert published >= 1  # (the surround phase went on counting across the call)
    _map_eq(A.map_export(), K.map_export(), "at the end of the stream")


def test_waits_for_deferred_update(world, loam):
    sweeps, M = world["sweeps"], world["M"]
    aft, bef = world["near"][:5], np.tile(M["bef"], (5, 1))
    res = []
    for drain in (False, True):
        ch = loam.Engine(loam.default_config(**CFG))
        assert ch.get_tuning("stream_defer") == 1
        mapped = 0
        for k, sw in enumerate(sweeps[:9]):  # through sweep 8 = mapping frame M0, its map update deferred
            rc, pub, od, a, b, reg = ch.chain_sweep(sw, stamp=0.1 * k)
            mapped += a is not None
        assert mapped == M0 + 1
        if drain:
            _map_eq(M, ch.map_export(), "chain_sweep's map")  # (waits for the update, as loam_batch_sync's drain)
        res.append(world["localize"](ch, aft, bef))
    _res_eq(res[0], res[1], "right after chain_sweep against after a drain")
    _res_eq(res[0], world["localize"](world["E"], aft, bef), "chain_sweep's map against the node calls'")


def test_errors_leave_out_and_map_alone(world, loam):
    L, E, M, rec = loam.lib(), world["E"], world["M"], world["rec"]
    P = ctypes.POINTER(loam.Pose6)
    n = 3
    aft = np.ascontiguousarray(world["near"][:n])
    pose = loam.Pose6.of(rec["pose"])
    cl = np.ascontiguousarray(rec["corner_last"], np.float32)
    sl = np.ascontiguousarray(rec["surf_last"], np.float32)
    big = np.zeros((int(E.cfg.max_points) + 1, 4), np.float32)

    def cloud(a, count=None, null=False):
        return loam.CloudOut(None if null else a.ctypes.data, a.shape[0] if count is None else count, a.shape[0])

    good = dict(ctx=E.h, odom=ctypes.byref(pose), corner=ctypes.byref(cloud(cl)), surf=ctypes.byref(cloud(sl)), n=n,
                aft=aft.ctypes.data_as(P), bef=None)
    cases = {
        "null odom_sum": dict(odom=None),
        "null corner_last": dict(corner=None),
        "null surf_last": dict(surf=None),
        "null aft": dict(aft=None),
        "n == 0": dict(n=0),
        "n > LOAM_LOCALIZE_MAX": dict(n=loam.LOCALIZE_MAX + 1),
        "corner pts null": dict(corner=ctypes.byref(cloud(cl, null=True))),
        "surf pts null": dict(surf=ctypes.byref(cloud(sl, null=True))),
        "surf beyond max_points": dict(surf=ctypes.byref(cloud(big))),
        "corner beyond max_points": dict(corner=ctypes.byref(cloud(big))),
    }
    out = (loam.LocalizeResult * (loam.LOCALIZE_MAX + 1))()
    pattern = bytes([0xA5]) * ctypes.sizeof(out)
    for name, kw in cases.items():
        a = dict(good, **kw)
        ctypes.memmove(out, pattern, len(pattern))
        rc = L.loam_map_localize(a["ctx"], a["odom"], a["corner"], a["surf"], a["n"], a["aft"], a["bef"], out)
        assert rc == loam.LOAM_E_INVAL, (name, rc)
        assert L.loam_last_error(), name
        assert bytes(out) == pattern, name
        _map_eq(M, E.map_export(), f"after {name}")
    assert L.loam_map_localize(E.h, good["odom"], good["corner"], good["surf"], n, good["aft"], None, None) == loam.LOAM_E_INVAL
    _map_eq(M, E.map_export(), "after a null out")
    # the calls above were refused, this one is not
    ctypes.memmove(out, pattern, len(pattern))
    assert L.loam_map_localize(E.h, good["odom"], good["corner"], good["surf"], n, good["aft"], None, out) == loam.LOAM_OK
    assert all(out[h].status == loam.LOC_SOLVED for h in range(n))
    assert bytes(out)[n * ctypes.sizeof(loam.LocalizeResult):] == pattern[n * ctypes.sizeof(loam.LocalizeResult):]


def test_overflowed_store_is_refused(world, loam):
    rec = world["rec"]
    small = loam.Engine(loam.default_config(map_capacity=1024, **CFG))
    with pytest.raises(loam.LoamError) as ei:  # the frame's map update does not fit 1024 points
        small.mapping(rec["pose"], rec["corner_last"], rec["surf_last"], rec["full_end"])
    assert ei.value.code == loam.LOAM_E_CAPACITY
    with pytest.raises(loam.LoamError) as ei:
        small.map_export()
    assert ei.value.code == loam.LOAM_E_INVAL
    # through the C-ABI: the code, and out (pre-filled) unchanged
    L, P = loam.lib(), ctypes.POINTER(loam.Pose6)
    aft = np.ascontiguousarray(world["near"][:2])
    cl = np.ascontiguousarray(rec["corner_last"], np.float32)
    sl = np.ascontiguousarray(rec["surf_last"], np.float32)
    out = (loam.LocalizeResult * 2)()
    pattern = bytes([0xA5]) * ctypes.sizeof(out)
    ctypes.memmove(out, pattern, len(pattern))
    rc = L.loam_map_localize(small.h, ctypes.byref(loam.Pose6.of(rec["pose"])),
                             ctypes.byref(loam.CloudOut(cl.ctypes.data, cl.shape[0], cl.shape[0])),
                             ctypes.byref(loam.CloudOut(sl.ctypes.data, sl.shape[0], sl.shape[0])), 2,
                             aft.ctypes.data_as(P), None, out)
    assert rc == loam.LOAM_E_INVAL and L.loam_last_error()
    assert bytes(out) == pattern


def test_empty_map_is_no_lm(world, loam):
    eng = loam.Engine(loam.default_config(**CFG))
    aft = world["near"][:6]
    res = world["localize"](eng, aft)
    assert np.all(res["status"] == loam.LOC_NO_LM)
    np.testing.assert_array_equal(_bits(res["aft"]), _bits(aft))
    for k in ("iters", "rows_last", "rows_sum", "degenerate_steps", "map_corner", "map_surf"):
        assert np.all(res[k] == 0), k
    assert np.all(res["stack_corner"] > 0) and np.all(res["stack_surf"] > 0)
    e = eng.map_export()
    assert e["corner"].shape[0] == 0 and e["surf"].shape[0] == 0 and e["surround_phase"] == 4


def test_working_set_regrowth_equals_fresh_context(world, loam):
    """The working set of the call grows and is then reused (it never shrinks): on one context, 1
    candidate on a small sweep, 5 candidates (beyond the floor of 4 the set starts with), 1 candidate
    on the whole sweep (larger stacks: the sweep's counts are rounded up to 512 corner / 4096 surf
    points), the small sweep again (the set is kept), then a map with a larger FromMap (its part of the
    set grows alone: a quarter more than asked, in steps of 4096 points).  Every call = the same call
    as the first one of a fresh context, bit for bit."""
    M, rec = world["M"], world["rec"]
    small_map = dict(M, corner=M["corner"][::4], surf=M["surf"][::4])
    rng = np.random.default_rng(20261022)
    near = np.empty((8000, 4), np.float32)  # inside the centre cube, which holds the sensor
    near[:, :3] = rng.uniform(-20.0, 20.0, (8000, 3)).astype(np.float32)
    near[:, 3] = rng.uniform(0, 16, 8000).astype(np.float32)
    big_map = dict(M, surf=np.concatenate([M["surf"], near]))
    whole = (rec["corner_last"], rec["surf_last"])
    part = (np.ascontiguousarray(rec["corner_last"][::3]), np.ascontiguousarray(rec["surf_last"][::5]))
    assert part[0].shape[0] <= 512 < whole[0].shape[0] and part[1].shape[0] <= 4096 < whole[1].shape[0]
    bef = M["bef"]

    def call(eng, sweep, n):
        return eng.map_localize(rec["pose"], sweep[0], sweep[1], world["near"][:n], np.tile(bef, (n, 1)))

    def fresh(m):
        eng = loam.Engine(loam.default_config(**CFG))
        assert _import(eng, m, bef=bef) == (0, 0)
        return eng

    G = fresh(small_map)
    from_small = 0
    for tag, sweep, n in (("first", part, 1), ("more candidates", part, 5), ("larger sweep", whole, 1),
                          ("smaller sweep, set kept", part, 1)):
        got = call(G, sweep, n)
        _res_eq(got, call(fresh(small_map), sweep, n), tag)
        assert np.all(got["status"] == loam.LOC_SOLVED), tag
        from_small = max(from_small, int((got["map_corner"] + got["map_surf"]).max()))
    assert _import(G, big_map, bef=bef) == (0, 0)
    got = call(G, whole, 1)
    from_big = int(got["map_corner"][0] + got["map_surf"][0])
    print(f"regrowth: FromMap {from_small} -> {from_big} points, iterations {got['iters'][0]}")
    assert 0 < from_small and from_small + from_small // 4 <= 4096 < from_big  # the FromMap part had to grow
    _res_eq(got, call(fresh(big_map), whole, 1), "larger FromMap")
    assert got["status"][0] == loam.LOC_SOLVED
