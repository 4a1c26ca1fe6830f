"""Mapping-frame sequences that reach the map update's branches no scene of the suite reaches
(tests/test_map_cases.py checks, on the oracle alone, that every case has the properties it is meant
to have; tests/test_gpu_map_parity.py gives the identical frames to the engine and compares the whole
cube map with the oracle's after every frame).

A case is a list of mapping frames, each a dict of pose (the odometry pose laserMapping receives),
corner_last, surf_last, full_end and stamp, plus odom / jump (pose = odom + jump on the translation).
The frames are either recorded from the oracle's own scan registration and odometry over raw sweeps
(`recorded`) or crafted directly, so a difference upstream of mapping cannot enter.

  wide      sweeps whose returns are moved along their rays to 40..520 m: every frame inserts into
            more than 512 (cube, kind) keys (k_mp_insert's one-wave ranking) and lets cubes outside
            the frame's 5x5x5 neighbourhood grow raw (k_mp_compact_copy's old ++ appended)
  wide_out  the same to 540 m: part of every stack lies outside the grid (slot -1)
  below     to 500 m with a phase that does not depend on the ring: 300..512 keys, the dense
            ranking near its capacity
  edge511 / edge512 / edge513   crafted: exactly that many keys on a fresh map, then 5..9 points
            into each of the same cubes, cubes interleaved along the cloud
  order     crafted: five keys of more than 1000 points each outside the neighbourhood, the surf
            keys changing with every stack point, three frames onto the same cubes
  shifted   two wide frames, then scenarios.GRID_JUMPS[4:] on ordinary sweeps' frames: the far
            cubes' content moves through the slot table, lines are cleared and wrapped
"""
import numpy as np

import scenarios

F = np.float32
W, H, D = 21, 11, 21
NCUBE = W * H * D
CFG = dict(system_delay=1)
K_DENSE = 512  # k_mp_insert's kDense: more keys than this take the one-wave ranking
N_RINGS, MAX_POINTS = 16, 40000  # the default config's: 120 * N_RINGS corner points, MAX_POINTS surf points

# (rmax, f, phi): a return on ring `ring` at azimuth az goes to 40 + (rmax - 40)(0.5 + 0.5 sin(f az + phi ring)) m
PUSH = {"wide": (520.0, 7, 0.8), "wide_out": (540.0, 9, 1.0), "below": (500.0, 3, 0.0)}
RECORDED = ("wide", "wide_out", "below", "shifted")
EDGES = {"edge511": 511, "edge512": 512, "edge513": 513}
CRAFTED = tuple(EDGES) + ("order",)
CASES = RECORDED[:3] + CRAFTED + ("shifted",)
N_SWEEPS = 8
SHIFT_WIDE_FRAMES = 2
SHIFT_JUMPS = [(0, 0, 0)] * SHIFT_WIDE_FRAMES + list(scenarios.GRID_JUMPS[4:])


def push_out(raw, rmax, f, phi):
    """every return of a raw sweep (x, y, z, ring) moved along its ray to the range above"""
    raw = np.array(raw, F)
    xyz = raw[:, :3].astype(np.float64)
    r = np.linalg.norm(xyz, axis=1)
    az = np.arctan2(xyz[:, 1], xyz[:, 0])
    rng = 40.0 + (rmax - 40.0) * (0.5 + 0.5 * np.sin(f * az + phi * raw[:, 3].astype(np.float64)))
    raw[:, :3] = (xyz / r[:, None] * rng[:, None]).astype(F)
    return raw


def raw_sweeps(sg, name):
    """the raw sweeps of a recorded case (what chain_sweep and the lanes are given)"""
    if name == "plain":
        return [np.array(s, F) for s in sg.stream_sweeps(N_SWEEPS, 1)]
    if name == "shifted":
        n = 2 * len(SHIFT_JUMPS) + 2
        sw = sg.stream_sweeps(n, 1)
        wide = 2 * SHIFT_WIDE_FRAMES + 1  # the sweeps behind the first two mapping frames
        return [push_out(s, *PUSH["wide"]) if k <= wide else np.array(s, F) for k, s in enumerate(sw)]
    return [push_out(s, *PUSH[name]) for s in sg.stream_sweeps(N_SWEEPS, 1)]


def record(oc, sweeps, jumps=()):
    """the mapping frames the oracle's scan registration and odometry publish over `sweeps`"""
    o = oc.Oracle(oc.default_config(**CFG))
    frames = []
    for k, sw in enumerate(sweeps):
        rc, f = o.scan_registration(sw, stamp=0.1 * k)
        if rc != 0:
            continue
        pub, pose, cl, sl, full = o.odometry(f, stamp=0.1 * k)
        if pub != 7:
            continue
        m = len(frames)
        jump = np.array(jumps[m] if m < len(jumps) else (0, 0, 0), F)
        p = pose.copy()
        p[3:] += jump
        frames.append({"pose": p, "odom": pose, "jump": jump, "corner_last": cl, "surf_last": sl, "full_end": full,
                       "stamp": 0.1 * k, "k": k})
    return frames


# ---------------------------------------------------------------- crafted frames
def cube_centre(c):
    c = np.asarray(c)
    return np.stack([50.0 * (c % W - 10), 50.0 * (c // W % H - 5), 50.0 * (c // (W * H) - 10)], -1)


def cheb(c, center=(10, 5, 10)):
    """a cube's distance from the centre cube, in cubes (the 5x5x5 neighbourhood is cheb <= 2)"""
    c = np.asarray(c)
    return np.maximum(np.maximum(np.abs(c % W - center[0]), np.abs(c // W % H - center[1])),
                      np.abs(c // (W * H) - center[2]))


def _frame(corner, surf, t):
    zero = np.zeros(6, F)
    return {"pose": zero, "odom": zero, "jump": np.zeros(3, F), "corner_last": corner, "surf_last": surf,
            "full_end": surf.copy(), "stamp": 0.1 * t, "k": t}


def _cloud(xyz, first):
    """points with a running number as intensity (every point of a case is told apart)"""
    p = np.empty((len(xyz), 4), F)
    p[:, :3] = np.asarray(xyz, np.float64).reshape(-1, 3)
    p[:, 3] = first + np.arange(len(xyz))
    return p


N_CORNER_KEYS = 8
LATTICE = np.array([(x, y, z) for x in (-8.0, 0.0, 8.0) for y in (-8.0, 0.0, 8.0) for z in (-8.0, 0.0, 8.0)])


def edge_frames(nkeys):
    """frame 0: one surf point at the centre of each of nkeys - 8 cubes at least 3 cubes from the
    sensor's, one corner point at the centre of each of 8 further ones; frame 1: 5..9 points, 8 m
    apart, into each of the same cubes, one point per cube in turn"""
    rng = np.random.default_rng(nkeys)
    far = np.flatnonzero(cheb(np.arange(NCUBE)) >= 3)
    pick = rng.permutation(far)[:nkeys]
    cubes = {"surf": pick[:nkeys - N_CORNER_KEYS], "corner": pick[nkeys - N_CORNER_KEYS:]}
    first = {k: _cloud(cube_centre(c), 0) for k, c in cubes.items()}
    second = {}
    for k, c in cubes.items():
        m = rng.integers(5, 10, len(c))
        m[:2] = 9  # (every turn holds two cubes or more: no two neighbours of the cloud share a cube)
        which = [rng.permutation(len(LATTICE))[:n] for n in m]
        xyz = [cube_centre(c[i]) + LATTICE[which[i][r]] for r in range(9) for i in range(len(c)) if r < m[i]]
        second[k] = _cloud(xyz, 10000)
    return [_frame(first["corner"], first["surf"], 0), _frame(second["corner"], second["surf"], 1)], cubes


ORDER_CORNER = 13 + W * 5 + W * H * 13
ORDER_SURF = [i + W * 5 + W * H * 10 for i in (13, 14, 15, 16)]
ORDER_SIDE = 34  # a 34 x 34 lattice of (y, z) rows, 1.4 m apart: 1156 points per key, each in a voxel of its own


def order_frames():
    """three frames onto one corner cube and four surf cubes in a row along x, all outside the
    neighbourhood.  Every (y, z) row of the lattice holds one point per cube, so the stack's
    VoxelGrid (which sorts by z, y, x voxel) leaves the surf keys changing with every point.
    1156 corner + 4624 surf points: neither a multiple of 64."""
    rng = np.random.default_rng(34)
    a = np.arange(ORDER_SIDE)
    rows = np.stack(np.meshgrid(a, a, indexing="ij"), -1).reshape(-1, 2) * 1.4 - 23.1
    frames = []
    for t in range(3):
        clouds = []
        for cubes in ([ORDER_CORNER], ORDER_SURF):
            xyz = []
            for r in rng.permutation(len(rows)):  # (the input order is not the stack's)
                for c in cubes:
                    ctr = cube_centre(c)
                    xyz.append((ctr[0] + rng.uniform(-20, 20), ctr[1] + rows[r, 0] + 0.45 * t, ctr[2] + rows[r, 1] + 0.45 * t))
            clouds.append(_cloud(xyz, 100000 * t))
        frames.append(_frame(clouds[0], clouds[1], t))
    return frames


# ---------------------------------------------------------------- the cases and the oracle's run of them
_cache = {}


def frames(name, oc, sg):
    key = ("frames", name)
    if key not in _cache:
        if name in EDGES:
            _cache[key] = edge_frames(EDGES[name])[0]
        elif name == "order":
            _cache[key] = order_frames()
        elif name == "shifted":
            _cache[key] = record(oc, raw_sweeps(sg, name), SHIFT_JUMPS)[:len(SHIFT_JUMPS)]
        else:
            _cache[key] = record(oc, raw_sweeps(sg, name))
    return _cache[key]


def map_frame(impl, fr):
    """one mapping frame on the oracle or an engine: everything the parity test compares"""
    aft, bef, reg = impl.mapping(fr["pose"], fr["corner_last"], fr["surf_last"], fr["full_end"], stamp=fr["stamp"])
    s = impl.stats()
    return {"aft": aft, "bef": bef, "registered": reg, "surround": impl.mapping_surround(),
            "mp_shifts": s["mp_grid_shifts"], "mp_iters": s["mp_iters"], "mp_stack": s["mp_stack"],
            "map": impl.map_export()}


def oracle_run(name, oc, sg):
    """the oracle's record of every frame of a case (computed once, read only)"""
    key = ("oracle", name)
    if key not in _cache:
        o = oc.Oracle(oc.default_config(**CFG))
        _cache[key] = [map_frame(o, fr) for fr in frames(name, oc, sg)]
    return _cache[key]


def oracle_pipeline(name, oc, sg):
    """the oracle's whole pipeline over a recorded case's raw sweeps: per sweep None, or the mapping
    frame's record (the deferred-update and lanes routes' yardstick)"""
    key = ("pipeline", name)
    if key not in _cache:
        o = oc.Oracle(oc.default_config(**CFG))
        out = []
        for k, sw in enumerate(raw_sweeps(sg, name)):
            rec = None
            rc, f = o.scan_registration(sw, stamp=0.1 * k)
            if rc == 0:
                pub, pose, cl, sl, full = o.odometry(f, stamp=0.1 * k)
                if pub == 7:
                    rec = map_frame(o, {"pose": pose, "corner_last": cl, "surf_last": sl, "full_end": full,
                                        "stamp": 0.1 * k})
                    rec["od_sum"] = pose
            out.append(rec)
        _cache[key] = out
    return _cache[key]


def keys_of(rec):
    """the (cube, kind) keys a frame inserted into, from the oracle's export"""
    return int(np.count_nonzero(rec["map"]["inserted"]))


def cube_sizes(m):
    """[2, NCUBE] points per cube of an export"""
    return np.stack([np.diff(m[k + "_offset"].astype(np.int64)) for k in ("corner", "surf")])


def frame_cube(prev, fr):
    """the frame's centre cube (i, j, k) in the grid as the frame leaves it: of the position the
    reference takes it of (test_gpu_map._frame_position), after the recentring"""
    from test_gpu_map import _frame_position, _recentre, cube_of
    pos = _frame_position(prev, {"pose": fr["odom"]}, fr["jump"])
    center, n = _recentre(pos, prev["map"]["center"] if prev else [10, 5, 10])
    return [int(cube_of(pos[a], center[a])) for a in range(3)], center, n
