"""The mapping 5-NN search (csrc/mp_nn.hpp: mp_nn_seed_from + knn5_flat, with its deferred top-5
insertion, pending-list overflow and fallback) through the diagnostic hook loam_dev_nn5_run
(csrc/dev_hooks.h), in the batch form (a lane per query) and the streaming form (a lane group per
query): bit for bit against the plain knn5 on every query, and against a numpy brute force (float32
dx*dx + dy*dy + dz*dz, ties broken by index) wherever the fifth distance is below 1 m.  The inputs
are built once; the properties a case relies on are checked on the CPU (test_case_constructions)."""
import numpy as np
import pytest

import nn5_hook
from nn5_hook import BATCH, NONE, OVERFLOW, PLAIN, STREAM

FORMS = [pytest.param(BATCH, id="batch"), pytest.param(STREAM, id="stream")]
PENDING = 8          # kNnPending: a lane's pending keys
LANES = 8            # kMpNnLanes: the streaming form's lanes per query
FAR_BITS = int(np.float32(3.4e38).view(np.uint32))   # the distance of an empty place
ONE_BITS = int(np.float32(1.0).view(np.uint32))


# ------------------------------------------------------------------ the reference
def keys_of(map_xyz, q):
    """(distance bits << 32 | index) of every map point for one query, as the kernels form it"""
    m = np.asarray(map_xyz, np.float32)
    d = m - np.asarray(q, np.float32)[None, :]
    d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    assert d2.dtype == np.float32
    return (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(len(m), dtype=np.uint64)


def brute5(map_xyz, queries):
    """(idx int32 [nq][5], dist bits uint32 [nq][5]) of the five smallest keys (map of >= 5 points)"""
    nq = len(queries)
    idx, dist = np.zeros((nq, 5), np.int32), np.zeros((nq, 5), np.uint32)
    for i in range(nq):
        k = keys_of(map_xyz, queries[i])
        k = np.sort(np.partition(k, 4)[:5])
        idx[i] = (k & np.uint64(0xffffffff)).astype(np.int64)
        dist[i] = (k >> np.uint64(32)).astype(np.uint32)
    return idx, dist


def below_bound(map_xyz, q, seeds):
    """how many keys lie below the seed bound B = the largest seed key"""
    k = keys_of(map_xyz, q)
    return int((k < k[np.asarray(seeds)].max()).sum())


def cell_hash(c):
    """dev_common.hpp cell_hash of integer cells [n][3]"""
    c = np.asarray(c, np.int64)
    m = np.uint64(0xffffffff)
    u = lambda v: v.astype(np.uint64) & m   # (two's complement, 32 bits)
    h = ((u(c[:, 0] >> 2) * np.uint64(73856093)) ^ (u(c[:, 1] >> 2) * np.uint64(19349663)) ^
         (u(c[:, 2] >> 2) * np.uint64(83492791))) & m
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7feb352d)) & m
    h ^= h >> np.uint64(15)
    return ((h << np.uint64(6)) & m) | u(c[:, 0] & 3) | (u(c[:, 1] & 3) << np.uint64(2)) | (u(c[:, 2] & 3) << np.uint64(4))


def listed_buckets(q, T):
    """the buckets an unseeded search of q lists: the cells at a box distance below 1 m (in float32)"""
    q = np.asarray(q, np.float32)
    c = np.floor(q).astype(np.int64)
    lo, hi = q - c.astype(np.float32), (c + 1).astype(np.float32) - q
    out = set()
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                g = [np.float32(0) if d == 0 else (lo[a] if d < 0 else hi[a]) for a, d in enumerate((dx, dy, dz))]
                if g[0] * g[0] + g[1] * g[1] + g[2] * g[2] < np.float32(1):
                    out.add(int(cell_hash([c + [dx, dy, dz]])[0]) & (T - 1))
    return out


def table_size(n):
    """the hash table of a map of n points: a power of two >= max(n, 64), at most the hook's 16384"""
    return min(1 << max(int(n) - 1, 63).bit_length(), 16384)


def candidates(map_xyz, q):
    """the map points (mask) in the buckets an unseeded search of q lists: all it can meet"""
    T = table_size(len(map_xyz))
    mine = np.array(sorted(listed_buckets(q, T)), np.uint64)
    return np.isin(cell_hash(np.floor(map_xyz).astype(np.int64)) & np.uint64(T - 1), mine)


class Case:
    def __init__(self, map_xyz, queries, seeds=None, distinct=None):
        self.map = np.ascontiguousarray(map_xyz, np.float32)
        self.queries = np.ascontiguousarray(queries, np.float32)
        self.seeds, self.distinct = seeds, distinct
        self.ref = brute5(self.map, self.queries)

    def run(self, hook, form):
        return hook.run(self.map, self.queries, form, seeds=self.seeds, distinct=self.distinct)

    def check(self, res, what):
        """flat == plain on every query; == the brute force wherever a fifth distance is below 1 m"""
        (fi, fd), (pi, pd) = res.flat, res.plain
        bad = np.flatnonzero((fi != pi).any(1) | (fd != pd).any(1))
        assert len(bad) == 0, (what, "flat != plain", bad[:8], fi[bad[:2]], pi[bad[:2]], fd[bad[:2]], pd[bad[:2]])
        ri, rd = self.ref
        near = (fd[:, 4] < ONE_BITS) | (rd[:, 4] < ONE_BITS)
        bad = np.flatnonzero(near & ((fi != ri).any(1) | (fd != rd).any(1)))
        assert len(bad) == 0, (what, "flat != brute force", bad[:8], fi[bad[:2]], ri[bad[:2]], fd[bad[:2]], rd[bad[:2]])
        # ascending keys on every query
        k = (fd.astype(np.uint64) << np.uint64(32)) | fi.astype(np.uint32).astype(np.uint64)
        assert (k[:, 1:] >= k[:, :-1]).all(), what
        return int(near.sum())


# ------------------------------------------------------------------ the inputs
def uneven_map(rng):
    """a sparse background and clusters of very different density in a 12 m box"""
    parts = [rng.uniform(-6, 6, (2500, 3))]
    for n, s in ((600, 0.15), (300, 0.4), (1200, 0.6), (60, 0.05), (900, 1.2)):
        parts.append(rng.uniform(-5, 5, 3) + rng.normal(0, s, (n, 3)))
    return np.concatenate(parts).astype(np.float32)


def uneven_queries(rng, m):
    near = m[rng.choice(len(m), 1300, replace=False)] + rng.normal(0, 0.05, (1300, 3)).astype(np.float32)
    return np.concatenate([near, rng.uniform(-6.5, 6.5, (237, 3))]).astype(np.float32)   # (no multiple of 64)


def make_uneven():
    rng = np.random.default_rng(71)
    m = uneven_map(rng)
    return Case(m, uneven_queries(rng, m))


def make_seeded(distinct=False):
    """the uneven case's queries moved a few centimetres, seeded with their previous true 5-NN"""
    rng = np.random.default_rng(71)
    m = uneven_map(rng)
    q0 = uneven_queries(rng, m)
    seeds = brute5(m, q0)[0]
    q1 = (q0 + rng.normal(0, 0.03, q0.shape)).astype(np.float32)
    flags = (rng.random(len(q1)) < 0.5).astype(np.int32) if distinct else None
    return Case(m, q1, seeds=seeds, distinct=flags)


CLUSTER, SITES = 120, 40


def make_overflow():
    """per site: a query, 120 points within 0.3 m of it and five stale seeds about 0.9 m away"""
    rng = np.random.default_rng(5)
    pts, queries, seeds = [], [], []
    for s in range(SITES):
        c = np.array([(s % 7) * 5.0 + 0.5, (s // 7) * 5.0 + 0.5, 0.5]) + rng.uniform(-0.2, 0.2, 3)
        v = rng.normal(0, 1, (CLUSTER, 3))
        v *= (rng.uniform(0.02, 0.3, CLUSTER) / np.linalg.norm(v, axis=1))[:, None]
        w = rng.normal(0, 1, (5, 3))
        w *= (rng.uniform(0.88, 0.92, 5) / np.linalg.norm(w, axis=1))[:, None]
        base = sum(len(p) for p in pts)
        pts += [c + v, c + w]
        seeds.append(base + CLUSTER + np.arange(5))
        queries.append(c)
    return Case(np.concatenate(pts), np.array(queries), seeds=np.array(seeds, np.int32))


def make_lattice(seeded):
    """a 0.25 m lattice with exact duplicates; queries on points, cell centres and edge midpoints:
    equal distances at every rank, decided by the index"""
    rng = np.random.default_rng(9)
    g = np.arange(13, dtype=np.float32) * np.float32(0.25)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    m = np.concatenate([lat, lat[rng.choice(len(lat), 300, replace=False)]]).astype(np.float32)
    on = lat[rng.choice(len(lat), 200, replace=False)]
    centre = lat[rng.choice(len(lat), 200, replace=False)] + np.float32(0.125)
    edge = lat[rng.choice(len(lat), 200, replace=False)] + np.array([0.125, 0, 0], np.float32)
    q = np.concatenate([on, centre, edge]).astype(np.float32)
    return Case(m, q, seeds=brute5(m, q)[0] if seeded else None)


def make_sparse():
    """clumps of one to four points 8 m apart, and a dense blob far away that makes the table large
    enough for few clumps to share buckets: fewer than five candidates for nearly every query"""
    rng = np.random.default_rng(3)
    pts, queries = [], []
    for s in range(60):
        c = np.array([(s % 8) * 8.0, (s // 8) * 8.0, 0.0]) + rng.uniform(0, 1, 3)
        pts.append(c + rng.uniform(-0.4, 0.4, (1 + s % 4, 3)))
        queries += [c, c + rng.uniform(-0.3, 0.3, 3)]
    pts.append(np.array([300.0, 300.0, 300.0]) + rng.uniform(0, 3, (4000, 3)))
    return Case(np.concatenate(pts), np.array(queries))


CROWD = 9000


def make_crowded():
    """one 1 m cell with more than 8,191 points (its packed range does not fit: the plain search)"""
    rng = np.random.default_rng(13)
    crowd = np.array([10.0, 10.0, 10.0]) + rng.uniform(0.1, 0.9, (CROWD, 3))
    rest = rng.uniform(0, 9, (1500, 3))
    m = np.concatenate([crowd, rest]).astype(np.float32)
    near = np.array([10.5, 10.5, 10.5]) + rng.uniform(-0.9, 0.9, (70, 3))
    far = rest[rng.choice(len(rest), 70, replace=False)] + rng.normal(0, 0.05, (70, 3))
    return Case(m, np.concatenate([near, far]).astype(np.float32))


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
    h = nn5_hook.Handle(loam.lib())
    yield h
    h.close()


# ------------------------------------------------------------------ the constructions (CPU)
def test_case_constructions(cases):
    # overflow: every site has far more keys below its stale seeds' bound than a pending list
    # holds, enough for every lane of a streaming group (a lane takes every 8th candidate, at
    # most five of a lane's are not below B), and the bound lies within 1 m
    c = cases("overflow")
    for q, s in zip(c.queries, c.seeds):
        n = below_bound(c.map, q, s)
        assert n >= CLUSTER and n > PENDING and n // LANES - 5 > PENDING
        assert keys_of(c.map, q)[s].max() >> np.uint64(32) < ONE_BITS
    # seeded: most queries have at most a pending list's keys below the bound (the deferred path
    # without overflow), and the true previous 5-NN are five distinct points
    c = cases("seeded")
    n = np.array([below_bound(c.map, q, s) for q, s in zip(c.queries[:300], c.seeds[:300])])
    assert (n <= PENDING).mean() > 0.5 and n.min() >= 4
    assert all(len(set(s)) == 5 for s in c.seeds)
    # lattice: ties at the fifth place between different indices, and duplicates at distance zero
    c = cases("lattice", False)
    ri, rd = c.ref
    k = np.array([np.sort(keys_of(c.map, q))[:6] >> np.uint64(32) for q in c.queries[:100]])
    assert (k[:, 4] == k[:, 5]).any() and ((rd[:, 0] == 0) & (rd[:, 1] == 0)).any()
    # sparse: fewer than five map points in the buckets of the 27 cells around any query
    c = cases("sparse")
    assert table_size(len(c.map)) == 8192
    n = np.array([candidates(c.map, q).sum() for q in c.queries])
    assert (n >= 1).all() and (n < 5).sum() >= 60   # (half of the queries)
    # crowded: the cell's count does not fit the 13 bits of a packed range
    c = cases("crowded")
    cell = np.floor(c.map).astype(int)
    assert (cell == [10, 10, 10]).all(1).sum() == CROWD > 8191


# ------------------------------------------------------------------ the searches (GPU)
@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_uneven_unseeded(hook, cases, form):
    c = cases("uneven")
    res = c.run(hook, form)
    assert c.check(res, "uneven") > 1000
    assert res.plain_count == 0 and res.overflow == 0   # (no wave of an unseeded job defers)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_seeded_moved(hook, cases, form):
    c = cases("seeded")
    res = c.run(hook, form)
    assert c.check(res, "seeded") > 1000
    assert res.plain_count == 0


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_stale_seeds_overflow(hook, cases, form):
    c = cases("overflow")
    res = c.run(hook, form)
    assert c.check(res, "overflow") == SITES
    assert res.overflow > 0, "the pending-overflow path did not run"
    assert res.overflow == SITES and ((res.flags & OVERFLOW) != 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("seeded", [False, True], ids=["unseeded", "seeded"])
def test_lattice_ties(hook, cases, form, seeded):
    c = cases("lattice", seeded)
    res = c.run(hook, form)
    assert c.check(res, "lattice") == len(c.queries)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_fewer_than_five(hook, cases, form):
    c = cases("sparse")
    res = c.run(hook, form)
    c.check(res, "sparse")
    fi, fd = res.flat
    assert ((fi == NONE) == (fd == FAR_BITS)).all()
    few = 0
    for i, q in enumerate(c.queries):   # fewer than five candidates: all of them in key order, then empty places
        k = np.sort(keys_of(c.map, q)[candidates(c.map, q)])
        if len(k) >= 5:
            continue
        few += 1
        np.testing.assert_array_equal(fi[i, :len(k)], (k & np.uint64(0xffffffff)).astype(np.int64))
        np.testing.assert_array_equal(fd[i, :len(k)], (k >> np.uint64(32)).astype(np.uint32))
        assert (fi[i, len(k):] == NONE).all() and (fd[i, len(k):] == FAR_BITS).all()
    assert few >= 60


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_seeds_not_distinct(hook, cases, form):
    c = cases("seeded", True)
    res = c.run(hook, form)
    assert c.check(res, "distinct off") > 1000
    # a query whose flag is off starts unseeded: the unseeded job's list
    un = hook.run(c.map, c.queries, form)
    off = c.distinct == 0
    assert off.sum() > 100
    np.testing.assert_array_equal(res.flat[0][off], un.flat[0][off])
    np.testing.assert_array_equal(res.flat[1][off], un.flat[1][off])


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_crowded_cell_falls_back(hook, cases, form):
    c = cases("crowded")
    res = c.run(hook, form)
    assert c.check(res, "crowded") >= 100
    assert res.plain_count > 0, "the knn5 fallback did not run"
    # exactly the queries that list the crowded cell's bucket (the first 70 at least)
    T = table_size(len(c.map))
    bucket = int(cell_hash([[10, 10, 10]])[0]) & (T - 1)
    want = np.array([bucket in listed_buckets(q, T) for q in c.queries])
    assert want[:70].all()
    np.testing.assert_array_equal((res.flags & PLAIN) != 0, want)
