"""The reference of loam_map_score's tests, in numpy only: for one pose, every query point's
squared distance to its nearest map point by brute force, then the counts and costs as
include/loam/loam.h defines them.

The brute force is chunked and windowed: the map is sorted by x, the (transformed) queries are grouped
by squares of (x, z); a group of queries meets the map points whose x and z lie
within WINDOW of the group's x and z ranges (a contiguous run in x, a mask in z), and every pair of
that block is evaluated.  A map point left out is farther than WINDOW > max_dist from every query
of the group along one axis alone, so it can be neither an inlier's neighbour nor change a
truncated term: the result is that of the loop over the whole map wherever d2 < WINDOW^2, and "no
neighbour within WINDOW" (inf) elsewhere.  No spatial structure beyond the two sorts
(tests/test_score_search.py::test_reference_equals_plain_loop compares it with the plain loop).

  exact tier    rotation zero: the device's arithmetic restated in float32 (the transform of
                pose_math.hpp point_to_map with sin = 0, cos = 1; sqdist's order), bit for bit
  float64 tier  any pose: transform and distances in float64
"""
import math

import numpy as np

WINDOW = 1.0625  # > 1 m = the largest max_dist, with room for the float64 tier's position error
CHUNK = 128  # queries of one dense block at most
TILE = 3.0    # metres: the queries are grouped by squares of this size in (x, z)


def to_map64(pose, pts):
    """pointAssociateToMap (src/laserMapping.cpp:234-252) in float64, no intermediate rounding"""
    rx, ry, rz, tx, ty, tz = [float(v) for v in pose]
    x, y, z = (np.asarray(pts[:, k], np.float64) for k in range(3))
    x1 = math.cos(rz) * x - math.sin(rz) * y
    y1 = math.sin(rz) * x + math.cos(rz) * y
    z1 = z
    x2 = x1
    y2 = math.cos(rx) * y1 - math.sin(rx) * z1
    z2 = math.sin(rx) * y1 + math.cos(rx) * z1
    out = np.empty((x.shape[0], 3), np.float64)
    out[:, 0] = math.cos(ry) * x2 + math.sin(ry) * z2 + tx
    out[:, 1] = y2 + ty
    out[:, 2] = -math.sin(ry) * x2 + math.cos(ry) * z2 + tz
    return out


def translate32(t, pts):
    """point_to_map for a pose (0, 0, 0, t) as the device rounds it: x and z added in double and
    rounded once, y added in float"""
    t = np.asarray(t, np.float32)
    p = np.asarray(pts, np.float32)
    out = np.empty((p.shape[0], 3), np.float32)
    out[:, 0] = (p[:, 0].astype(np.float64) + np.float64(t[0])).astype(np.float32)
    out[:, 1] = p[:, 1] + t[1]
    out[:, 2] = (p[:, 2].astype(np.float64) + np.float64(t[2])).astype(np.float32)
    return out


def scored_mask(pts):
    """the points with three finite coordinates"""
    return np.isfinite(np.asarray(pts)[:, :3]).all(axis=1)


class SortedMap:
    """one kind's map points sorted by x, in float32 and float64"""

    def __init__(self, pts):
        p = np.ascontiguousarray(np.asarray(pts, np.float32)[:, :3])
        o = np.argsort(p[:, 0], kind="stable")
        self.p32 = np.ascontiguousarray(p[o])
        self.p64 = self.p32.astype(np.float64)
        self.x = self.p64[:, 0].copy()


def nearest_d2(smap, q, dtype):
    """min over the map of the squared distance to each row of q ([n, 3], finite, dtype float32:
    sqdist's float arithmetic and order, float64: plain), inf where no map point lies within WINDOW
    of the query in x and in z"""
    n = q.shape[0]
    out = np.full(n, np.inf, dtype)
    if n == 0 or smap.x.shape[0] == 0:
        return out
    m = smap.p32 if dtype == np.float32 else smap.p64
    # the queries grouped by TILE x TILE squares of (x, z): dense regions give large groups
    tx, tz = np.floor(q[:, 0].astype(np.float64) / TILE), np.floor(q[:, 2].astype(np.float64) / TILE)
    o = np.lexsort((tz, tx))
    qs, tx, tz = q[o], tx[o], tz[o]
    best = np.full(n, np.inf, dtype)
    cuts = np.flatnonzero((np.diff(tx) != 0) | (np.diff(tz) != 0)) + 1
    for s0, s1 in zip(np.r_[0, cuts], np.r_[cuts, n]):
        g = qs[s0:s1]
        lo = np.searchsorted(smap.x, float(g[:, 0].min()) - WINDOW, side="left")
        hi = np.searchsorted(smap.x, float(g[:, 0].max()) + WINDOW, side="right")
        blk = m[lo:hi]
        blk = blk[(blk[:, 2] >= float(g[:, 2].min()) - WINDOW) & (blk[:, 2] <= float(g[:, 2].max()) + WINDOW)]
        if blk.shape[0] == 0:
            continue
        for a in range(s0, s1, CHUNK):
            c = qs[a:min(a + CHUNK, s1)]
            dx = blk[None, :, 0] - c[:, None, 0]
            dy = blk[None, :, 1] - c[:, None, 1]
            dz = blk[None, :, 2] - c[:, None, 2]
            d2 = dx * dx + dy * dy + dz * dz  # ((dx*dx + dy*dy) + dz*dz, every operation rounded in dtype)
            best[a:a + c.shape[0]] = d2.min(axis=1)
    out[o] = best
    return out


def score_terms(d2, max_dist, dtype):
    """(inlier mask, terms) of the scored points' nearest squared distances"""
    r2 = dtype(max_dist) * dtype(max_dist)
    inl = d2 < r2
    return inl, np.where(inl, d2, r2).astype(dtype)


def exact_score(smaps, clouds, t, max_dist, d2_cache=None):
    """loam_score_result of the pose (0, 0, 0, t) restated in float32: a dict with the counts (equal
    to the device's) and, per cloud, math.fsum of the float terms.  d2_cache: a dict that keeps the
    nearest distances of (t, cloud) across max_dist values"""
    res = {}
    for name, smap, cl in (("corner", smaps[0], clouds[0]), ("surf", smaps[1], clouds[1])):
        key = (np.asarray(t, np.float32).tobytes(), name)
        if d2_cache is not None and key in d2_cache:
            d2 = d2_cache[key]
        else:
            ok = scored_mask(cl)
            d2 = nearest_d2(smap, translate32(t, np.asarray(cl, np.float32)[ok]), np.float32)
            if d2_cache is not None:
                d2_cache[key] = d2
        inl, terms = score_terms(d2, max_dist, np.float32)
        res[name + "_scored"] = int(d2.shape[0])
        res[name + "_in"] = int(inl.sum())
        res[name + "_cost"] = math.fsum(float(v) for v in terms)
    return res


def float64_score(smaps, clouds, pose, max_dist, delta):
    """the float64 reference of any pose: counts, costs, and per cloud the number of scored points
    whose nearest distance lies within delta of max_dist (the points a position error of delta may
    flip)"""
    res = {}
    for name, smap, cl in (("corner", smaps[0], clouds[0]), ("surf", smaps[1], clouds[1])):
        ok = scored_mask(cl)
        d2 = nearest_d2(smap, to_map64(pose, np.asarray(cl, np.float64)[ok]), np.float64)
        inl, terms = score_terms(d2, max_dist, np.float64)
        d = np.sqrt(d2)
        res[name + "_scored"] = int(d2.shape[0])
        res[name + "_in"] = int(inl.sum())
        res[name + "_cost"] = math.fsum(float(v) for v in terms)
        res[name + "_border"] = int((np.abs(d - max_dist) <= delta).sum())
    return res
