"""Input segments for the VoxelGrid cascade's edges (tests/test_vg_cases.py checks that the drawn
inputs have the properties they are meant to have; tests/test_gpu_voxelgrid.py runs them), and a
numpy restatement of the voxel key computation (csrc/vg.hip vg_frame_of and the kernels' key
lines, as pcl_voxel_grid in tests/test_oracle_components.py) that tells, per segment, how many bits
its largest key needs, how k_vg_split would bucket it and whether k_vg_merge may take it.

Every generator returns a float32 [n][4] array (x, y, z, intensity)."""
import numpy as np

F = np.float32
INT_MAX = 2 ** 31 - 1
KEY_BITS = (4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 31)
LEAVES = (0.2, 0.4)


# ---------------------------------------------------------------- the key computation, restated
def leaf_too_small(pts, leaf):
    """vg_leaf_too_small (csrc/dev_common.hpp) on the segment's bounding box"""
    inv = F(1.0) / F(leaf)
    mn, mx = pts[:, :3].min(0), pts[:, :3].max(0)
    e = []
    for d in range(3):
        sp, lo, hi = F((mx[d] - mn[d]) * inv), F(mn[d] * inv), F(mx[d] * inv)
        if not sp < F(2147483648.0) or not lo >= F(-2147483648.0) or not hi < F(2147483648.0):
            return True
        e.append(int(sp) + 1)
    xy = e[0] * e[1]
    return xy > INT_MAX or xy * e[2] > INT_MAX


def axis_extents(pts, leaf):
    """the three factors of the "too small" product"""
    inv = F(1.0) / F(leaf)
    mn, mx = pts[:, :3].min(0), pts[:, :3].max(0)
    return [int(F((mx[d] - mn[d]) * inv)) + 1 for d in range(3)]


def seg_keys(pts, leaf):
    """(keys as int64 [n], div [3]) of a segment whose leaf is not too small"""
    inv = F(1.0) / F(leaf)
    xyz = np.ascontiguousarray(pts[:, :3], F)
    mn, mx = xyz.min(0), xyz.max(0)
    minb = np.floor(mn * inv).astype(np.int64)
    maxb = np.floor(mx * inv).astype(np.int64)
    div = maxb - minb + 1
    ijk = (np.floor(xyz * inv) - minb.astype(F)).astype(np.int64)
    key = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    return key, div


def key_bits(pts, leaf):
    """bits the segment's largest voxel key needs (0: one voxel); None when the leaf is too small"""
    if leaf_too_small(pts, leaf):
        return None
    key, _ = seg_keys(pts, leaf)
    return int(key.max()).bit_length()


def split_buckets(pts, leaf):
    """k_vg_split's 16 bucket sizes: the top 4 of the bits the frame's largest possible key needs;
    None when the leaf is too small (the parent is copied)"""
    if leaf_too_small(pts, leaf):
        return None
    key, div = seg_keys(pts, leaf)
    kmax = int(div[0] - 1) + int(div[1] - 1) * int(div[0]) + int(div[2] - 1) * int(div[0]) * int(div[1])
    bits = min(kmax, 2 ** 32 - 1).bit_length()
    shift = bits - 4 if bits > 4 else 0
    return np.bincount((key >> shift) & 15, minlength=16)


def merge_precondition(pts, leaf, nold):
    """k_vg_merge takes the segment: the leaf is not too small, every key is below 2^24 and the
    keys of the first nold points are strictly increasing"""
    if leaf_too_small(pts, leaf):
        return False
    key, _ = seg_keys(pts, leaf)
    if int(key.max()) >= 1 << 24:
        return False
    return bool(np.all(np.diff(key[:nold]) > 0))


def merge_eligible(n, nold, merge_min, new_max=8192):
    """vg_merge_eligible (csrc/vg.hpp), restated"""
    return n > merge_min and nold > 0 and n - nold <= new_max


# ---------------------------------------------------------------- distributions
def _intensity(rng, n):
    return rng.uniform(0.0, 16.0, n)


def _pack(xyz, inten):
    return np.ascontiguousarray(np.concatenate([xyz, np.asarray(inten)[:, None]], 1), F)


def _in_voxels(rng, ijk, leaf):
    """one point inside each voxel ijk (away from its faces, so float rounding keeps it there)"""
    return (ijk + rng.uniform(0.1, 0.9, ijk.shape)) * leaf


def uniform(n, leaf, seed):
    """(a) uniform in a voxel-aligned cube of about n / 2.5 voxels around the origin"""
    rng = np.random.default_rng(seed)
    k = max(1, int(round((n / 2.5) ** (1.0 / 3.0))))
    lo = -(k // 2) * leaf
    return _pack(lo + rng.uniform(0.0, k * leaf, (n, 3)), _intensity(rng, n))


def one_voxel(n, leaf, seed):
    """(b) every point in one voxel; intensities over seven decades"""
    rng = np.random.default_rng(seed)
    ijk = np.tile(np.array([[-3.0, 7.0, 2.0]]), (n, 1))
    return _pack(_in_voxels(rng, ijk, leaf), 10.0 ** rng.uniform(-3.0, 4.0, n))


def one_per_voxel(n, leaf, seed, descending=False):
    """(c) point i alone in voxel i of a W x W x . lattice: keys ascending (or descending) in input order"""
    rng = np.random.default_rng(seed)
    w = max(1, int(np.ceil(n ** (1.0 / 3.0))))
    i = np.arange(n)
    ijk = np.stack([i % w, (i // w) % w, i // (w * w)], 1).astype(np.float64) - (w // 2)
    p = _pack(_in_voxels(rng, ijk, leaf), _intensity(rng, n))
    return np.ascontiguousarray(p[::-1]) if descending else p


def two_voxels(n, leaf, seed):
    """(d) two voxels next to each other in x, alternating: keys {0, 1}"""
    rng = np.random.default_rng(seed)
    ijk = np.zeros((n, 3))
    ijk[:, 0] = np.arange(n) % 2
    ijk += np.array([-1.0, 4.0, -2.0])
    return _pack(_in_voxels(rng, ijk, leaf), 10.0 ** rng.uniform(-3.0, 4.0, n))


def span_dims(bits):
    """box dimensions in voxels whose largest key needs exactly `bits` bits"""
    d = max(1, int(np.floor(2.0 ** ((bits - 1) / 3.0))))
    dz = -(-(2 ** (bits - 1) + 1) // (d * d))
    assert 2 ** (bits - 1) <= d * d * dz - 1 < 2 ** bits and d * d * dz <= INT_MAX
    return d, d, dz


def key_span(n, leaf, seed, bits):
    """(e) a box whose largest key needs exactly `bits` bits: one point in the box's minimum voxel,
    one in its maximum voxel (n >= 2), the rest in random voxels"""
    rng = np.random.default_rng(seed)
    div = np.array(span_dims(bits))
    ijk = rng.integers(0, div, (n, 3)).astype(np.float64)
    where = rng.permutation(n)[:2]
    ijk[where[0]] = 0
    if n >= 2:
        ijk[where[1]] = div - 1
    ijk -= div // 2
    return _pack(_in_voxels(rng, ijk, leaf), _intensity(rng, n))


def too_small(n, leaf, seed, kind="xy"):
    """(f) the voxel counts of the bounding box multiply beyond INT_MAX: output = input.
    kind "xy": already x times y does; "xyz": only the product of all three (2000^3)"""
    rng = np.random.default_rng(seed)
    side = {"xy": 100000, "xyz": 2000}[kind]
    ijk = rng.integers(0, side, (n, 3)).astype(np.float64)
    where = rng.permutation(n)[:2]
    ijk[where[0]] = 0
    if n >= 2:
        ijk[where[1]] = side - 1
    ijk -= side // 2
    return _pack(_in_voxels(rng, ijk, leaf), _intensity(rng, n))


def boundaries(n, leaf, seed):
    """(g) negative coordinates, points exactly on voxel faces (k * leaf rounded to float), -0.0,
    exact duplicates"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-6.0 * leaf, 6.0 * leaf, (n, 3)).astype(F)
    lat = (rng.integers(-6, 7, (n, 3)).astype(F) * F(leaf)).astype(F)
    on_face = rng.random((n, 3)) < 0.5
    xyz[on_face] = lat[on_face]
    xyz[rng.random((n, 3)) < 0.05] = F(-0.0)
    p = _pack(xyz, _intensity(rng, n))
    if n >= 2:
        dup = rng.random(n) < 0.2
        p[dup] = p[rng.integers(0, n, int(dup.sum()))]
    return p


SKEWS = ("one_bucket", "low16", "ends", "mid", "huge")


def split_skew(n, leaf, seed, kind):
    """(h) bucket populations of the 16-way split.  The frame is 32 x 32 x 16 voxels (14 key bits), so
    a point's bucket is its z layer.  A point in the minimum and one in the maximum voxel fix the frame,
    which puts one point in the last bucket whatever the kind; "one_bucket" is the case without them
    (a single voxel: bucket 0 is the parent).
      low16: every other point in bucket 0       ends: buckets 0 and 15 only
      mid:   bucket 5 holds 2049..16384 points   huge: bucket 5 holds more than 16384 points"""
    if kind == "one_bucket":
        return one_voxel(n, leaf, seed)
    rng = np.random.default_rng(seed)
    div = np.array([32, 32, 16])
    ijk = rng.integers(0, div, (n, 3)).astype(np.float64)
    if kind == "low16":
        ijk[:, 2] = 0
    elif kind == "ends":
        ijk[:, 2] = 15 * rng.integers(0, 2, n)
    else:
        m = {"mid": min(n - 2, max(2049, n // 4)), "huge": min(n - 2, max(16385, n // 2))}[kind]
        ijk[:m, 2] = 5
        ijk[m:, 2] = rng.choice([0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], n - m)
        ijk = ijk[rng.permutation(n)]
    ijk[0] = 0
    ijk[n - 1] = div - 1
    ijk -= div // 2
    return _pack(_in_voxels(rng, ijk, leaf), _intensity(rng, n))


MERGE_TAKEN = ("taken", "taken_bbox")
MERGE_FALLBACK = ("raw_prefix", "key24", "too_small")


def merge_segment(vg, nold, ntail, leaf, seed, kind="taken"):
    """(i) a cube segment: nold old points, then ntail appended ones.
    vg(pts, leaf) is the reference VoxelGrid (oracle_voxel_grid): the old prefix is its output on a
    random cloud in a 50 m cube (1..3 points per voxel), cut to nold points.  The tail cycles through
    points in voxels that hold an old point, points in new voxels among the old ones, and points in the
    bounding box's minimum / maximum corner voxels (before the first and after the last old voxel).
      taken_bbox: the last tail point lies 3 voxels below the minimum on every axis (every key shifts)
      raw_prefix: the old points are a raw cloud (keys not increasing)
      key24:      the last tail point lies 60 m beyond the cube on every axis (leaf 0.2: keys >= 2^24)
      too_small:  the last tail point lies 100 km away"""
    rng = np.random.default_rng(seed)
    side = int(round(50.0 / leaf))
    if kind == "raw_prefix":
        old = _pack(rng.uniform(-25.0, 25.0, (nold, 3)), _intensity(rng, nold))
    else:
        m = nold + nold // 4 + 8
        ijk = rng.integers(0, side, (m, 3))
        ijk = np.repeat(ijk, rng.integers(1, 4, m), 0).astype(np.float64) - side // 2
        cloud = _pack(_in_voxels(rng, ijk, leaf), _intensity(rng, len(ijk)))
        cloud = cloud[rng.permutation(len(cloud))]
        old = vg(cloud, leaf)
        assert len(old) >= nold
        old = old[:nold]
    inv = F(1.0) / F(leaf)
    cell = np.floor(old[:, :3] * inv).astype(np.float64)
    lo, hi = cell.min(0), cell.max(0)
    t = np.arange(ntail)
    tail_ijk = np.where((t % 4 == 0)[:, None], cell[rng.integers(0, nold, ntail)],
                        np.where((t % 4 == 1)[:, None],
                                 rng.integers(lo.astype(np.int64), hi.astype(np.int64) + 1, (ntail, 3)).astype(np.float64),
                                 np.where((t % 4 == 2)[:, None], lo, hi)))
    tail = _pack(_in_voxels(rng, tail_ijk, leaf), _intensity(rng, ntail))
    if ntail:
        if kind == "taken_bbox":
            tail[-1, :3] = ((lo - 3.0 + 0.5) * leaf).astype(F)
        elif kind == "key24":
            tail[-1, :3] = F(25.0 + 60.0)
        elif kind == "too_small":
            tail[-1, :3] = F(1.0e5)
    return np.ascontiguousarray(np.concatenate([old, tail]), F), nold


# ---------------------------------------------------------------- jobs
def pack_job(segments, leaves, gap=3, nolds=None):
    """segments (arrays, possibly empty) laid out with `gap` unused points between them (filled with
    points that would change any bounding box they leaked into) -> pts, begin, end, leaf[, nold]"""
    total = sum(len(s) for s in segments) + gap * (len(segments) + 1)
    pts = np.full((max(total, 1), 4), F(-7.5e3), F)
    begin, end = [], []
    at = gap
    for s in segments:
        begin.append(at)
        pts[at:at + len(s)] = s
        at += len(s)
        end.append(at)
        at += gap
    out = [pts, np.array(begin, np.int32), np.array(end, np.int32), np.array(leaves, F)]
    if nolds is not None:
        out.append(np.array(nolds, np.int32))
    return out


# ---------------------------------------------------------------- references
def oracle_vg(oc):
    """vg(pts, leaf) -> oracle_voxel_grid's output (oracle/oracle_math.hpp voxel_grid)"""
    lib = oc.lib()

    def vg(pts, leaf):
        pts = np.ascontiguousarray(pts, F)
        n = len(pts)
        if n == 0:
            return np.zeros((0, 4), F)
        out = np.zeros((n, 4), F)
        m = lib.oracle_voxel_grid(pts.ctypes.data, n, float(leaf), out.ctypes.data, n)
        assert 0 <= m <= n
        return out[:m].copy()
    return vg


def f64_voxel_means(pts, leaf):
    """the float64 statement: voxels in key order, members by the restated keys; per voxel the mean of
    its members, their count and the largest |value| among them, per field.  None: leaf too small"""
    if leaf_too_small(pts, leaf):
        return None
    key, _ = seg_keys(pts, leaf)
    order = np.lexsort((np.arange(len(pts)), key))
    _, start, cnt = np.unique(key[order], return_index=True, return_counts=True)
    p = pts[order].astype(np.float64)
    mean = np.add.reduceat(p, start, 0) / cnt[:, None]
    vmax = np.maximum.reduceat(np.abs(p), start, 0)
    return mean, cnt, vmax
