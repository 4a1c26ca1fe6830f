"""The odometry association's ring windows case by case: a plain restatement of the
reference's two association passages, and the clouds and queries that reach each mechanism of the
engine's window search (csrc/od.hip wave_window, wave_window_mono, mono_seed_key, od_assoc_wave).

A case is one Last cloud and one query list, used for both kinds (as CornerLast with sharp queries
and as SurfLast with flat ones).  The forward walk ends at min(queries, cloud size) (Q11), so a case
that wants whole windows pads its queries with far ones up to the cloud size.

Sizes the cases are built around: a chunk is 64 points, a sub-chunk 32; one box step covers 64
chunks = 4096 points in the walks and 64 sub-chunks = 2048 points in the index-range form."""
import numpy as np

CORNER, SURF = 0, 1
F32 = np.float32


# ------------------------------------------------------------------ the restatement
def sqdist(cloud, q):
    """float32 (dx*dx + dy*dy) + dz*dz of every cloud point to q"""
    d = np.asarray(cloud, F32)[:, :3] - np.asarray(q, F32)[None, :3]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert d2.dtype == F32
    return d2


def assoc_one(d2, ring, kind, fwd_end, last_tie=False):
    """src/laserOdometry.cpp:478-527 (corner) / :590-650 (surf) for one query whose squared distances to
    the Last cloud are d2 (a list) and whose rings are ring (a list of ints).  Returns (ind1, ind2,
    ind3, points the two walks examined).  last_tie (not the reference: for making seeds): `<=` in
    place of `<`, i.e. the last of equally distant points in walk order."""
    n = len(d2)
    c = min(range(n), key=d2.__getitem__) if n < 64 else int(np.argmin(np.asarray(d2)))
    if not d2[c] < 25:
        return -1, -1, -1, 0
    scan = ring[c]
    m2, m3, i2, i3 = 25.0, 25.0, -1, -1
    visited = 0
    better = (lambda a, b: a <= b) if last_tie else (lambda a, b: a < b)
    j = c + 1
    while j < fwd_end:
        if ring[j] > scan + 2.5:
            break
        visited += 1
        if kind == CORNER:
            if ring[j] > scan and better(d2[j], m2):
                m2, i2 = d2[j], j
        elif ring[j] <= scan:
            if better(d2[j], m2):
                m2, i2 = d2[j], j
        elif better(d2[j], m3):
            m3, i3 = d2[j], j
        j += 1
    j = c - 1
    while j >= 0:
        if ring[j] < scan - 2.5:
            break
        visited += 1
        if kind == CORNER:
            if ring[j] < scan and better(d2[j], m2):
                m2, i2 = d2[j], j
        elif ring[j] >= scan:
            if better(d2[j], m2):
                m2, i2 = d2[j], j
        elif better(d2[j], m3):
            m3, i3 = d2[j], j
        j -= 1
    if last_tie:  # `<=` also accepts a point at exactly 25, which is no member
        i2 = i2 if m2 < 25 else -1
        i3 = i3 if m3 < 25 else -1
    return c, i2, i3, visited


def assoc_ref(cloud, queries, kind, fwd_end, last_tie=False, with_visited=False):
    """ind [nq, 3] int32 of every query: the nearest point by brute force, then the two walks"""
    cloud = np.asarray(cloud, F32)
    ring = cloud[:, 3].astype(np.int32).tolist()
    out = np.full((len(queries), 3), -1, np.int32)
    vis = np.zeros(len(queries), np.int64)
    for i, q in enumerate(np.asarray(queries, F32)):
        d2 = sqdist(cloud, q)
        if not d2.min() < 25:
            continue
        a = assoc_one(d2.tolist(), ring, kind, fwd_end, last_tie)
        out[i] = a[:3]
        vis[i] = a[3]
    return (out, vis) if with_visited else out


# ------------------------------------------------------------------ a case
class Case:
    def __init__(self, name, cloud, queries, pad=True, note=""):
        """cloud [n, 4] (w: ring + a fraction), queries [nq, 3 or 4]; pad: far queries appended until
        there are as many queries as points, so that the forward walks end at the cloud's end"""
        self.name, self.note = name, note
        self.cloud = np.ascontiguousarray(cloud, F32)
        q = np.zeros((len(queries), 4), F32)
        q[:, :3] = np.asarray(queries, F32)[:, :3]
        self.n_real = len(q)
        if pad and len(q) < len(self.cloud):
            k = np.arange(len(self.cloud) - len(q) + 3, dtype=F32)
            far = np.zeros((len(k), 4), F32)
            far[:, 0] = self.cloud[:, 0].max() + F32(40) + F32(7) * k   # beyond every point, each alone
            far[:, 1] = self.cloud[:, 1].max() + F32(40) + F32(0.37) * k
            far[:, 2] = F32(-3.3)
            q = np.concatenate([q, far])
        self.queries = q
        self.fwd_end = min(len(q), len(self.cloud))
        self.rings = self.cloud[:, 3].astype(np.int32)
        self.mono = bool(np.all(np.diff(self.rings) >= 0))
        self._ref = {}

    def ref(self, kind):
        if kind not in self._ref:
            self._ref[kind] = assoc_ref(self.cloud, self.queries, kind, self.fwd_end, with_visited=True)
        return self._ref[kind][0]

    def visited(self, kind):
        self.ref(kind)
        return self._ref[kind][1]

    def problem(self, seeds=None):
        d = dict(corner_last=self.cloud, surf_last=self.cloud, corner_q=self.queries, surf_q=self.queries)
        if seeds is not None:
            d["corner_seeds"], d["surf_seeds"] = seeds
        return d

    def ring_starts(self):
        """the ring start table of a ring-monotone cloud: first index whose ring >= r, r in [0, 66)"""
        return np.searchsorted(self.rings, np.arange(66), side="left").astype(np.int32)


def with_ring(xyz, ring):
    out = np.zeros((len(xyz), 4), F32)
    out[:, :3] = xyz
    out[:, 3] = np.asarray(ring, F32) + F32(0.25)
    return out


# ------------------------------------------------------------------ rings, clamp, nonmono
RING_IDS = (0, 1, 4, 5, 6, 9, 62, 63)
PER_RING = 112   # 896 points: ring k of RING_IDS is [112 k, 112 k + 112), a chunk boundary inside every ring


def rings_cloud(seed=11):
    """a lidar-like ring-major cloud: ring id r on a circle of 8 m at height 0.3 r, 112 points a ring
    (0.45 m apart), the groups {0, 1}, {4, 5, 6}, {9}, {62, 63} more than two rings apart"""
    g = np.random.default_rng(seed)
    pts, ring = [], []
    for r in RING_IDS:
        az = (np.arange(PER_RING) + g.uniform(-0.3, 0.3, PER_RING)) * (2 * np.pi / PER_RING)
        rad = 8.0 + g.uniform(-0.2, 0.2, PER_RING)
        pts.append(np.stack([rad * np.cos(az), rad * np.sin(az), 0.3 * r + g.uniform(-0.05, 0.05, PER_RING)], 1))
        ring += [r] * PER_RING
    return with_ring(np.concatenate(pts).astype(F32), ring)


def near(cloud, idx, seed, sigma=0.08):
    g = np.random.default_rng(seed)
    return (cloud[idx, :3] + g.normal(0, sigma, (len(idx), 3))).astype(F32)


def rings_case():
    c = rings_cloud()
    g = np.random.default_rng(12)
    q = np.concatenate([near(c, np.arange(len(c)), 13),            # next to every point of every ring
                        g.uniform(-12, 12, (60, 3)).astype(F32),   # anywhere, some beyond 5 m of everything
                        near(c, np.array([0, len(c) - 1]), 14, 0.02)])
    return Case("rings", c, q, note="ring 0, the top ring, gaps of more than two rings, a lone ring")


def clamp_cases():
    """the rings cloud with fewer queries than points: the forward end (the query count) inside ring
    `scan`, inside the next ring, at c + 1, at and before c"""
    c = rings_cloud()
    out = []
    for nq in (300, 400):  # inside ring id 4 (indices 224 .. 335), inside ring id 5 (336 .. 447)
        g = np.random.default_rng(nq)
        edge = np.arange(nq - 6, nq + 6)                       # c around the forward end: c + 1 == end, c >= end
        rest = g.choice(len(c), nq - len(edge), replace=False)
        idx = np.concatenate([edge, rest])
        out.append(Case(f"clamp{nq}", c, near(c, idx, nq + 1), pad=False, note=f"forward end {nq}"))
    return out


def nonmono_case():
    """the rings cloud with its ring blocks in the order 0, 4, 1, 5, 6, 9, 62, 63 and two single points
    swapped: from ring 0 the forward walk stops at the ring 4 block although ring 1 follows"""
    c = rings_cloud()
    order = np.concatenate([np.arange(k * PER_RING, (k + 1) * PER_RING) for k in (0, 2, 1, 3, 4, 5, 6, 7)])
    order[[400, 500]] = order[[500, 400]]
    c2 = c[order]
    q = np.concatenate([near(c2, np.arange(len(c2)), 23), near(c2, np.array([0, len(c2) - 1]), 24, 0.02)])
    return Case("nonmono", c2, q, note="rings decrease in index order")


def small_cases():
    """a lone ring, and clouds of 1, 2, 64 and 65 points (the last one point into a second chunk), the
    nearest point at index 0 and at n - 1"""
    out = []
    x = np.arange(100, dtype=F32) * F32(0.3)
    line = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)
    c = with_ring(line, [7] * 100)
    out.append(Case("onering", c, near(c, np.arange(100), 31, 0.05), note="a single ring: no other-ring point"))
    for n, rings in ((1, [5]), (2, [3, 4]), (64, [0] * 20 + [1] * 20 + [2] * 24), (65, [61] * 30 + [62] * 34 + [63])):
        c = with_ring(line[:n], rings)
        q = np.concatenate([near(c, np.arange(n), 40 + n, 0.05), near(c, np.array([0, n - 1]), 41 + n, 0.02),
                            np.array([[-1.0, 0.1, 0.05], [x[n - 1] + 1.0, 0.1, 0.05]], F32)])
        out.append(Case(f"n{n}", c, q, note=f"{n} points"))
    return out


# ------------------------------------------------------------------ long
LONG_N = 2200


def long_case():
    """rings 10, 11, 12 of 2200 points each, 0.25 m apart on lines, between a 40-point ring 7 and a
    40-point ring 14 far away (the walks' stops).  Ring 10 runs x = 0 .. 550 at y = 0, ring 11 goes on
    x = 550 .. 1100 at y = 1, ring 12 runs x = -550 .. 0 at y = 2: its end lies beside ring 10's start.
      F1: beside an early point of ring 10.  The forward window is 6590 points; apart from the query's
          own chunk, the only points below 5 m are ring 12's last, in the last chunk before the stop.
      B1: beside a late point of ring 12: the backward window mirrors it (ring 10's first points lie
          in the chunk of the backward stop).
      F2 / B2: beside the ring 10 / 11 boundary: the other ring starts in the first chunk walked.
    Every chunk between is at least 5 m from the query."""
    k = np.arange(LONG_N, dtype=np.float64)
    z = np.zeros(LONG_N)
    r10 = np.stack([0.25 * k, z, z], 1)
    r11 = np.stack([550.0 + 0.25 * k, z + 1.0, z], 1)
    r12 = np.stack([-0.25 * (LONG_N - 1 - k), z + 2.0, z], 1)
    k40 = np.arange(40, dtype=np.float64)
    r7 = np.stack([0.5 * k40, np.full(40, -100.0), np.zeros(40)], 1)
    r14 = np.stack([0.5 * k40, np.full(40, -120.0), np.zeros(40)], 1)
    c = with_ring(np.concatenate([r7, r10, r11, r12, r14]).astype(F32),
                  [7] * 40 + [10] * LONG_N + [11] * LONG_N + [12] * LONG_N + [14] * 40)
    b10, b11, b12 = 40, 40 + LONG_N, 40 + 2 * LONG_N
    idx = np.array([b10 + 2, b12 + LONG_N - 6, b10 + LONG_N - 10, b11 + 8,   # F1, B1, F2, B2
                    b10 + 70, b12 + LONG_N - 70, b11 + 1100])
    off = np.array([0.03, 0.02, 0.01], F32)
    return Case("long", c, c[idx, :3] + off, note="windows beyond one box step, all but one chunk skipped")


# ------------------------------------------------------------------ ties
def ties_cloud(k_tie, mirror):
    """Three chunks, every coordinate a multiple of 1/8, the query at the origin.
      chunk 0: ring 4 (32 points) and ring 5 (32): the nearest point N = (0, 0, 1/8) at index 40; K =
               (-1, 0, 0) in ring 4 (at (-2, 0, 0) unless k_tie); S1 = (0, 2, 0) before N and S2 =
               (0, -2, 0) after it in ring 5; the rest beyond 5 m
      chunk 1: ring 6 on the plane x = 1, around F1 = (1, 0, 0): the chunk's box is exactly 1 away
      chunk 2: ring 6 on the plane y = 1, around F2 = (0, 1, 0)
    F1 and F2 are equally distant forward (the earlier, F1, wins); with k_tie K is as distant
    backward (forward wins).  mirror: the index order reversed and ring r -> 10 - r, which swaps
    forward and backward."""
    far = lambda i: (40.0 + i / 8.0, 40.0, 0.0)
    pts, ring = [], []
    for i in range(32):
        pts.append(((-1.0 if k_tie else -2.0), 0.0, 0.0) if i == 20 else far(i))
        ring.append(4)
    for i in range(32, 64):
        pts.append({36: (0.0, 2.0, 0.0), 40: (0.0, 0.0, 0.125), 44: (0.0, -2.0, 0.0)}.get(i, far(i)))
        ring.append(5)
    grid = [(a / 8.0, b / 8.0) for a in range(-4, 4) for b in range(-4, 4)]  # 64 pairs, (0, 0) among them
    for a, b in grid:
        pts.append((1.0, a, b))
        ring.append(6)
    for a, b in grid:
        pts.append((a, 1.0, b))
        ring.append(6)
    c = with_ring(np.array(pts, F32), ring)
    if mirror:
        c = c[::-1].copy()
        c[:, 3] = F32(10.25) - c[:, 3].astype(np.int32).astype(F32)
    return c


def ties_cases():
    out = []
    for k_tie in (False, True):
        for mirror in (False, True):
            name = "ties" + ("_k" if k_tie else "") + ("_m" if mirror else "")
            out.append(Case(name, ties_cloud(k_tie, mirror), np.zeros((1, 3), F32),
                            note="equal distances: forward before backward, earlier before later"))
    # the 25 m2 threshold: three clusters 100 m apart, each with its query at the cluster's origin
    pts = [((0, 0, 0.125), 5), ((3, 4, 0), 6), ((-3, -4, 0), 5), ((-3, 4, 0), 4),         # exactly 25: not taken
           ((100, 0, 0.125), 5), ((103, 3.875, 0), 6), ((97, -3.875, 0), 5), ((97, 3.875, 0), 4),  # just below
           ((203, 4, 0), 5), ((206, 0, 0), 6), ((200, -6, 0), 5)]                          # the nearest at 25
    pts.sort(key=lambda t: t[1])
    c = with_ring(np.array([p for p, _ in pts], F32), [r for _, r in pts])
    q = np.array([[0, 0, 0], [100, 0, 0], [200, 0, 0]], F32)
    out.append(Case("ties_25", c, q, note="exactly 25 m2 (not taken), just below, the nearest at 25 m2"))
    return out


# ------------------------------------------------------------------ random
def random_case(name, n_rings, n, nq, seed):
    """a ring-major lidar-like cloud (ring r at elevation -15 + 30 r / n_rings degrees, ranges 4 .. 25 m)
    and nq queries in 30 clusters around cloud points; the forward end is nq (Q11)"""
    g = np.random.default_rng(seed)
    ring = np.sort(np.arange(n) % n_rings)
    az = g.uniform(0, 2 * np.pi, n)
    key = np.lexsort((az, ring))
    ring, az = ring[key], az[key]
    rng = 4.0 + 21.0 * (0.5 + 0.5 * np.sin(3 * az)) * g.uniform(0.9, 1.0, n)
    el = np.deg2rad(-15.0 + 30.0 * ring / n_rings)
    xyz = np.stack([rng * np.cos(el) * np.cos(az), rng * np.cos(el) * np.sin(az), rng * np.sin(el)], 1)
    c = with_ring(xyz.astype(F32), ring)
    centres = g.choice(n, 30, replace=False)
    centres[:6] = [3, n - 4, nq - 2, nq + 40, n // 2, n // 3]  # both ends of the cloud, around the forward end
    q = (c[np.repeat(centres, nq // 30), :3] + g.normal(0, 0.5, (nq, 3))).astype(F32)
    return Case(name, c, q, pad=False, note=f"{n_rings} rings, {n} points, {nq} queries in clusters")


def random_cases():
    return [random_case("random16", 16, 5000, 1500, 51), random_case("random64", 64, 16384, 1500, 52)]


# ------------------------------------------------------------------ all of them, built once
_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = [rings_case()] + clamp_cases() + [nonmono_case()] + small_cases() + [long_case()] + ties_cases() + \
            random_cases()
    return _ALL


def by_name(name):
    return next(c for c in all_cases() if c.name == name)


NAMES = ["rings", "clamp300", "clamp400", "nonmono", "onering", "n1", "n2", "n64", "n65", "long",
         "ties", "ties_m", "ties_k", "ties_k_m", "ties_25", "random16", "random64"]


# ------------------------------------------------------------------ seeds
def seed_sets(case, kind, oracle_od_assoc):
    """the previous round's ind1, ind2, ind3 in four ways; seeds only bound the searches, so every one
    of them leaves the unseeded answer.  oracle_od_assoc: oracle_ctypes.od_assoc (any association
    will do for `moved`: a seed need not be right)"""
    n, nq = len(case.cloud), len(case.queries)
    g = np.random.default_rng(7 + kind)
    moved = case.queries.copy()
    moved[:, :3] += g.normal(0, 0.03, (nq, 3)).astype(F32)
    sets = {"moved": oracle_od_assoc(case.cloud, moved, kind, case.fwd_end)}
    rnd = g.integers(-1, n, (nq, 3)).astype(np.int32)
    ref = case.ref(kind)
    rnd[::5, 1] = ref[::5, 0]  # equal to c
    rnd[1::5, 2] = ref[1::5, 0]
    rnd[2::7] = -1
    sets["random"] = rnd
    far = np.full((nq, 3), -1, np.int32)
    for i in range(min(nq, case.n_real if case.n_real < 400 else 400)):  # (the padding queries keep -1)
        beyond = np.nonzero(sqdist(case.cloud, case.queries[i]) >= 25)[0]
        if len(beyond):
            far[i] = g.choice(beyond, 3)
    sets["far"] = far
    if case.name.startswith("ties"):  # the last of equally distant points in walk order
        sets["last_tie"] = assoc_ref(case.cloud, case.queries, kind, case.fwd_end, last_tie=True)
    return sets
