"""The odometry association's nearest neighbour on a lane per query (csrc/od.hip lane_hash_nn, the
k_od_sel_nn launch, tuning od_nn_lane) through the diagnostic hook loam_dev_od_nn_run (csrc/
dev_hooks.h): bit for bit against the wave-per-query search (wave_hash_nn) wherever the lane
settled its query, and against a numpy brute force over (float32 (dx*dx + dy*dy) + dz*dz bits,
index) wherever that minimum lies below 1 m2; then the whole batch step bit for bit across
od_nn_lane 0 / 1 / 2."""
import numpy as np
import pytest

import od_nn_hook
from od_nn_hook import NONE

ONE_BITS = int(np.float32(1.0).view(np.uint32))
D25_BITS = int(np.float32(25.0).view(np.uint32))
EXACT_ROWS = 1 << 30  # tuning od_moments_min: no batch size keeps the odometry rows as moments


# ------------------------------------------------------------------ the reference
def brute(cloud, rings, queries):
    """the smallest (distance bits << 32 | index << 8 | ring) of every query over the whole cloud"""
    m = np.asarray(cloud, np.float32)
    rings = np.asarray(rings, np.uint64)
    out = np.zeros(len(queries), np.uint64)
    low = (np.arange(len(m), dtype=np.uint64) << np.uint64(8)) | rings
    for i, q in enumerate(np.asarray(queries, np.float32)):
        d = m - q[None, :3]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == np.float32
        out[i] = ((d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | low).min()
    return out


def dist_bits(keys):
    return (np.asarray(keys, np.uint64) >> np.uint64(32)).astype(np.int64)


def check(hook, cloud, rings, queries, seeds=None):
    """the properties every case must hold; returns (result, brute keys)"""
    r = hook.run(cloud, rings, queries, seeds)
    ref = brute(cloud, rings, queries)
    near = dist_bits(ref) < ONE_BITS
    settled = r.left == 0
    print(f"queries {len(ref)}, settled {int(settled.sum())}, brute below 1 m2 {int(near.sum())}")
    np.testing.assert_array_equal(r.left == 1, r.lane == np.uint64(NONE))
    # the lane settles exactly the queries whose nearest point lies below 1 m2, with that point
    np.testing.assert_array_equal(settled, near)
    np.testing.assert_array_equal(r.lane[near], ref[near])
    # lane == wave wherever the lane settled
    np.testing.assert_array_equal(r.lane[settled], r.wave[settled])
    # a query the lane left: the wave's cell stage found nothing below 1 m2 either, so its result is
    # its chunk stage's, which is what k_od_assoc runs for such a query
    left = ~settled
    assert np.all((r.wave[left] == np.uint64(NONE)) | (dist_bits(r.wave[left]) >= ONE_BITS))
    np.testing.assert_array_equal(r.wave[left], r.chunk[left])
    # both wave searches are exact below 25 m2 (the chunk stage alone covers the whole cloud)
    in5 = dist_bits(ref) < D25_BITS
    np.testing.assert_array_equal(r.wave[in5], ref[in5])
    np.testing.assert_array_equal(r.chunk[in5], ref[in5])
    return r, ref


# ------------------------------------------------------------------ the inputs (built once)
def make_spread(n=400, nq=300, span=30.0, seed=5):
    """a few hundred points over tens of metres (several cells share a bucket of the 256-entry table),
    queries near points and in empty space"""
    g = np.random.default_rng(seed)
    cloud = g.uniform(-span, span, (n, 3)).astype(np.float32)
    cloud[:, 2] = g.uniform(-3, 3, n)
    rings = g.integers(0, 16, n)
    near = cloud[g.integers(0, n, nq * 2 // 3)] + g.normal(0, 0.4, (nq * 2 // 3, 3)).astype(np.float32)
    far = g.uniform(-span, span, (nq - len(near), 3)).astype(np.float32)
    return cloud, rings, np.concatenate([near, far]).astype(np.float32)


def make_lattice():
    """a 0.5 m lattice, every point twice (indices i and i + n): a query at a cell's centre is
    equally far from 8 points and their copies; the lowest index wins"""
    ax = np.arange(-2, 3, dtype=np.float32) * np.float32(0.5)
    p = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    cloud = np.concatenate([p, p])
    rings = np.concatenate([np.arange(len(p)) % 16, (np.arange(len(p)) + 3) % 16])
    centres = p[(p < 1.0).all(1)] + np.float32(0.25)
    return cloud, rings, np.concatenate([centres, p[:40]]).astype(np.float32)


def make_faces():
    """queries on cell faces and at negative coordinates, the nearest point across the face"""
    cloud, queries = [], []
    for k, (x, y, z) in enumerate([(0.0, 0.5, 0.5), (-3.0, -2.5, 1.5), (4.0, -7.0, -1.0), (-6.0, -6.0, -6.0)]):
        base = np.array([x, y, z], np.float32) + np.float32(20 * k) * np.array([1, 0, 0], np.float32)
        for ax in range(3):
            e = np.zeros(3, np.float32)
            e[ax] = 1
            cloud.append(base - np.float32(0.05) * e)          # just below the face
            cloud.append(base + np.float32(0.7) * e)           # farther, in the query's own cell
            queries += [base, base + np.float32(0.02) * e, base - np.float32(1e-6) * e]
    cloud = np.array(cloud, np.float32)
    return cloud, np.arange(len(cloud)) % 16, np.array(queries, np.float32)


def make_radius():
    """lone points (20 m apart) with queries just under, at and just over 1 m from them"""
    cloud = np.array([[20.0 * k + 0.5, 0.5, 0.5] for k in range(6)], np.float32)
    queries = []
    for k, d in enumerate([0.99, 0.9999, 1.0, 1.0001, 1.2, 3.0]):
        for e in ([1, 0, 0], [0, -1, 0], [0, 0, 1]):
            queries.append(cloud[k] + np.float32(d) * np.array(e, np.float32))
    return cloud, np.arange(6), np.array(queries, np.float32)


def make_crowded(n_in):
    """n_in points in one cell beside sparse neighbours: the lanes of the crowded cell walk
    thousands of candidates, the others a handful"""
    g = np.random.default_rng(11)
    crowd = (np.array([10, 10, 10]) + g.uniform(0.01, 0.99, (n_in, 3))).astype(np.float32)
    sparse = g.uniform(5, 16, (200, 3)).astype(np.float32)
    cloud = np.concatenate([sparse, crowd])
    rings = g.integers(0, 64, len(cloud))
    queries = np.concatenate([crowd[:20] + np.float32(0.01), sparse[:40] + np.float32(0.2),
                              g.uniform(5, 16, (40, 3)).astype(np.float32)])
    return cloud, rings, queries.astype(np.float32)


@pytest.fixture(scope="module")
def cases():
    made = {}

    def get(name, *a):
        if (name, a) not in made:
            made[(name, a)] = globals()["make_" + name](*a)
        return made[(name, a)]
    return get


@pytest.fixture(scope="module")
def hook(loam):
    h = od_nn_hook.Handle(loam.lib())
    yield h
    h.close()


# ------------------------------------------------------------------ the hook cases
@pytest.mark.gpu
def test_three_points(hook):
    """3 points (the table clamps to 64 buckets), 5 queries"""
    cloud = np.array([[0.2, 0.2, 0.2], [0.9, 0.1, 0.3], [-0.4, 0.3, 0.1]], np.float32)
    queries = np.array([[0.25, 0.2, 0.2], [0.8, 0.1, 0.3], [-0.5, 0.3, 0.0], [0.5, 1.5, 0.2], [9, 9, 9]], np.float32)
    r, _ = check(hook, cloud, [0, 1, 2], queries)
    assert list(r.left) == [0, 0, 0, 1, 1]


@pytest.mark.gpu
@pytest.mark.parametrize("nq", [1, 65])
def test_partial_waves(hook, cases, nq):
    cloud, rings, queries = cases("spread")
    check(hook, cloud, rings, queries[:nq])


@pytest.mark.gpu
def test_spread_shared_buckets(hook, cases):
    cloud, rings, queries = cases("spread")
    r, _ = check(hook, cloud, rings, queries)
    assert 0 < r.left.sum() < len(queries)


@pytest.mark.gpu
def test_lattice_ties(hook, cases):
    cloud, rings, queries = cases("lattice")
    r, ref = check(hook, cloud, rings, queries)
    n = len(cloud) // 2
    assert np.all(((r.lane >> np.uint64(8)) & np.uint64(0xffffff)) < np.uint64(n))  # never the copy


@pytest.mark.gpu
def test_cell_faces_negative(hook, cases):
    cloud, rings, queries = cases("faces")
    r, _ = check(hook, cloud, rings, queries)
    assert not r.left.any()


@pytest.mark.gpu
def test_one_metre_radius(hook, cases):
    cloud, rings, queries = cases("radius")
    r, ref = check(hook, cloud, rings, queries)
    # (the construction: both sides of the radius occur)
    assert (dist_bits(ref) < ONE_BITS).any() and (dist_bits(ref) >= ONE_BITS).any()


@pytest.mark.gpu
def test_seeds(hook, cases):
    """seeds that are the true neighbour (the inclusive bound), stale seeds several metres off, and
    unseeded lanes mixed in one wave"""
    cloud, rings, queries = cases("spread")
    ref = brute(cloud, rings, queries)
    true = ((ref >> np.uint64(8)) & np.uint64(0xffffff)).astype(np.int32)
    check(hook, cloud, rings, queries, true)
    g = np.random.default_rng(3)
    stale = g.integers(0, len(cloud), len(queries)).astype(np.int32)
    check(hook, cloud, rings, queries, stale)
    mixed = np.where(np.arange(len(queries)) % 3 == 0, -1, np.where(np.arange(len(queries)) % 3 == 1, true, stale))
    check(hook, cloud, rings, queries, mixed.astype(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("n_in", [3000, 9000])
def test_crowded_cell(hook, cases, n_in):
    """3000 points in one cell (a packed range) and 9000 (beyond the packed count: the lane walks its
    cells one by one)"""
    cloud, rings, queries = cases("crowded", n_in)
    check(hook, cloud, rings, queries)
    ref = brute(cloud, rings, queries)
    seeds = ((ref >> np.uint64(8)) & np.uint64(0xffffff)).astype(np.int32)
    check(hook, cloud, rings, queries, seeds)


# ------------------------------------------------------------------ end to end
def _run(loam, prevs, curs, cfg, nn_lane, profiling=False):
    e = loam.Engine(cfg) if cfg is not None else loam.Engine()
    e.set_tuning(od_sel_min=1, od_nn_lane_min=1, od_moments_min=EXACT_ROWS, od_persist=0, od_nn_lane=nn_lane)
    if profiling:
        e.set_profiling(True)
    e.batch_upload(prevs, curs)
    e.batch_run()
    try:
        od, aft, st = e.batch_download()
        info = e.batch_lm_info()
    finally:
        e.close()
    return od, aft, st, info


def _same(a, b):
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    for x, y in zip(a[3], b[3]):
        np.testing.assert_array_equal(x, y)


@pytest.mark.gpu
def test_batch_vlp16_modes(loam, sg):
    prevs, curs = sg.batch_problems(4, base_seed=8100)
    runs = [_run(loam, prevs, curs, None, m, profiling=True) for m in (0, 1, 2)]
    print("odometry iterations", runs[0][3][0], "gathered", [r[2]["od_assoc_gathered"] for r in runs])
    assert runs[0][3][0].max() > 5  # (seeded association rounds ran)
    for r in runs[1:]:
        _same(runs[0], r)
        # the work counter means the same: the cells' candidates, the chunks, the windows
        assert r[2]["od_assoc_gathered"] == runs[0][2]["od_assoc_gathered"] > 0


@pytest.mark.gpu
def test_batch_hdl64_modes(loam, sg):
    prev, cur = sg.single_problem(2, lidar=sg.HDL64)
    cfg = loam.default_config(n_rings=64, ring_model=loam.RING_LINEAR, max_points=160000)
    runs = [_run(loam, [prev], [cur], cfg, m) for m in (0, 1, 2)]
    for r in runs[1:]:
        _same(runs[0], r)


@pytest.mark.gpu
def test_batch_empty_and_tiny_modes(loam, sg):
    prevs, curs = sg.batch_problems(8, base_seed=4100)
    bad = list(curs)
    bad[2] = np.full((100, 4), np.nan, np.float32)
    tiny = list(prevs)
    tiny[5] = prevs[5][:300]
    for m in (0, 1, 2):
        with pytest.raises(loam.LoamError) as ei:
            _run(loam, prevs, bad, None, m)
        assert ei.value.code == loam.LOAM_E_INVAL
    runs = [_run(loam, tiny, curs, None, m) for m in (0, 1, 2)]
    for r in runs[1:]:
        _same(runs[0], r)
