"""Hand-built VLP-16 sweeps for the ring sort's and the ring VoxelGrid's edge cases
(test_sr_chain_cases.py checks on the CPU that each sweep produces its case, test_gpu_sr_chain.py runs
them on the GPU), and a numpy restatement of what the ring VoxelGrid sees of a ring: its lessFlat
candidates, their voxel runs and the width of its sort key.

A sweep is K azimuth steps; at every step each ring with a return fires once, in ring order.  The
point of ring r at step k lies at elevation ELEV[r] and orientation -pi + 0.01 + (2 pi - 0.02) k /
(K - 1) (scanRegistration's -atan2(y, x), increasing over the sweep), at the range the design gives
(NaN: no return, no point).  Non-finite points are separate rows put in afterwards."""
import numpy as np

R = 16
TILE = 2048                                   # k_sr_ring_fused's tile (kSrThreads * kRingE points)
# ring r of the VLP-16 model: the rounded elevation e is ring e when positive, e + 15 otherwise
ELEV = np.array([r if r % 2 else r - 15 for r in range(R)], np.float64)
LEAF = np.float32(5.0)                        # 1 / 0.2f in float


def room(K, half=6.0, seed=0, sigma=0.01):
    """ranges [K, R] of a square room of half-width `half` m around the sensor, with a little noise"""
    ori = -np.pi + 0.01 + (2 * np.pi - 0.02) * np.arange(K) / (K - 1)
    rxy = half / np.maximum(np.abs(np.cos(ori)), np.abs(np.sin(ori)))
    rng = rxy[:, None] / np.cos(np.radians(ELEV))[None, :]
    return rng + np.random.default_rng(seed).normal(0.0, sigma, rng.shape)


def sweep(rng):
    """the raw sweep (sensor frame x, y, z, 0) [n, 4] float32 of ranges [K, R]: a row per finite range"""
    K = rng.shape[0]
    ori = -np.pi + 0.01 + (2 * np.pi - 0.02) * np.arange(K) / (K - 1)
    el = np.radians(ELEV)
    x = rng * np.cos(el)[None, :] * np.cos(-ori)[:, None]
    y = rng * np.cos(el)[None, :] * np.sin(-ori)[:, None]
    z = rng * np.sin(el)[None, :]
    p = np.stack([x, y, z, np.zeros_like(x)], -1).reshape(-1, 4)
    return np.ascontiguousarray(p[np.isfinite(rng).reshape(-1)], np.float32)


def with_nans(raw, at):
    """raw with an all-NaN row put in before each of the (ascending, original) row indices `at`"""
    return np.ascontiguousarray(np.insert(raw, np.asarray(at, np.int64), np.nan, axis=0), np.float32)


def padded_to(raw, n, seed):
    """raw with NaN rows scattered over its middle so that it has exactly n rows; the ends stay finite"""
    need = n - raw.shape[0]
    assert need >= 0
    at = np.sort(np.random.default_rng(seed).integers(100, raw.shape[0] - 100, need))
    return with_nans(raw, at)


# ---------------------------------------------------------------- the ring sort's sweeps
def ring_sort_sweeps():
    """{name: raw}: where the sweep's ends lie and how n sits against the 2048-point tile"""
    base = sweep(room(250, seed=1))            # 4000 points
    out = {}
    out["first_late"] = with_nans(base, [0] * 70)                     # first finite point at 70 (> 64)
    out["last_early"] = with_nans(base, [base.shape[0]] * 80)         # last finite point 80 before the end
    out["tile_multiple"] = padded_to(base, 2 * TILE, seed=2)          # n == 2 tiles
    out["tile_plus_one"] = padded_to(base, 2 * TILE + 1, seed=3)      # n == 2 tiles + 1
    out["below_tile"] = sweep(room(93, seed=4))                       # 1488 points: one partial tile
    return out


def bad_sweeps():
    """{name: raw}: sweeps scan registration refuses (no finite point)"""
    return {"all_nan": np.full((100, 4), np.nan, np.float32), "empty": np.zeros((0, 4), np.float32)}


# ---------------------------------------------------------------- the ring VoxelGrid's sweeps
WALL_RING, ONE_VOXEL_RING, SHORT_RING, ONE_CAND_RING = 14, 1, 5, 7
OWN_VOXEL_RING, WIDE_RING = 0, 15


def vg_sweep_near():
    """a wall at about 1 m on WALL_RING, seen at 1100 steps (voxels of several dozen members; the range
    alternates by 0.25 m over stretches of it, so consecutive candidates leave a voxel and come back:
    voxels re-entered by non-adjacent runs); ONE_VOXEL_RING's returns all within one 0.2 m cell;
    SHORT_RING: 8 points (no selectable span: 0 candidates); ONE_CAND_RING: 11 smooth points (a span of
    one point: 1 candidate);
    the other rings see the room at every fourth step"""
    K = 1100
    rng = np.full((K, R), np.nan)
    rm = room(K, seed=5)
    for r in range(R):
        rng[::4, r] = rm[::4, r]
    k = np.arange(K)
    wall = 1.0 / np.cos(np.radians(ELEV[WALL_RING])) + 0.0 * k
    zig = ((k // 200) % 2 == 1) & (k % 2 == 1)
    wall[zig] += 0.25
    rng[:, WALL_RING] = wall
    rng[:, ONE_VOXEL_RING] = np.nan
    rng[340:370, ONE_VOXEL_RING] = 0.3         # 30 returns on an arc of 0.05 m
    for ring, cnt in ((SHORT_RING, 8), (ONE_CAND_RING, 11)):
        rng[:, ring] = np.nan
        rng[500:500 + cnt, ring] = 4.0
    return sweep(rng)


def vg_sweep_far():
    """OWN_VOXEL_RING: 1100 returns alternating between 30 and 31.5 m (0.34 m apart along either circle),
    every candidate alone in its voxel (more than 1024 runs, and a voxel index narrow enough for the
    32-bit key next to 11 run bits);
    WIDE_RING (elevation 15 degrees): ranges swinging between 2 and 150 m, a bounding box of some
    2^29 cells, too wide for the 32-bit key; the other rings see the room at every fourth step"""
    K = 1100
    rng = np.full((K, R), np.nan)
    rm = room(K, seed=6)
    for r in range(R):
        rng[::4, r] = rm[::4, r]
    k = np.arange(K)
    rng[:, OWN_VOXEL_RING] = np.where(k % 2 == 0, 30.0, 31.5)
    rng[::2, WIDE_RING] = 76.0 + 74.0 * np.sin(2 * np.pi * k[::2] / K * 3)
    return sweep(rng)


def vg_sweeps():
    return {"vg_near": vg_sweep_near(), "vg_far": vg_sweep_far()}


# ---------------------------------------------------------------- what the ring VoxelGrid sees
def ring_vg_cases(f):
    """per ring of an oracle scan-registration result f: dict(ncand, nruns, nvox, max_members, rb,
    cells, fits32, nout): the lessFlat candidates (the points of the ring's selectable span
    [start + 5, end - 5) that are not in less_sharp), the runs of consecutive candidates in one 0.2 m
    voxel of the candidates' bounding box, the distinct voxels, the largest voxel's members, the run
    number's bits, the box's cells, whether (voxel << rb) | run fits 32 bits, and the oracle's own
    count of downsampled points of the ring (nout; nvox must equal it)"""
    full = f["full"]
    ring = full[:, 3].astype(np.int64)
    assert np.all(np.diff(ring) >= 0)
    sharpish = {row.tobytes() for row in f["less_sharp"]}
    lf_ring = f["less_flat"][:, 3].astype(np.int64)
    out = {}
    for q in range(R):
        idx = np.nonzero(ring == q)[0]
        assert idx.size, "every ring of these sweeps has points"
        lo, en = int(idx[0]) + 5, int(idx[-1]) + 1 - 5
        cand = [i for i in range(lo, en) if full[i].tobytes() not in sharpish]
        c = dict(ncand=len(cand), nruns=0, nvox=0, max_members=0, rb=0, cells=0, fits32=True,
                 nout=int(np.sum(lf_ring == q)))
        if cand:
            P = full[cand, :3].astype(np.float32)
            minb = np.floor(P.min(0) * LEAF)
            div = (np.floor(P.max(0) * LEAF) - minb + 1).astype(np.int64)
            ijk = (np.floor(P * LEAF) - minb).astype(np.int64)
            vox = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
            c["nruns"] = 1 + int(np.sum(vox[1:] != vox[:-1]))
            c["nvox"] = int(np.unique(vox).size)
            c["max_members"] = int(np.bincount(np.unique(vox, return_inverse=True)[1]).max())
            c["rb"] = int(c["nruns"] - 1).bit_length()
            c["cells"] = int(div[0] * div[1] * div[2])
            c["fits32"] = c["cells"] <= 1 << (32 - c["rb"])
        out[q] = c
    return out


def check_vg_cases(near, far):
    """the cases vg_sweep_near / vg_sweep_far are there for, on ring_vg_cases of their oracle results"""
    for name, cases in (("near", near), ("far", far)):
        for q, c in cases.items():
            assert c["nvox"] == c["nout"], (name, q, c)        # the restatement agrees with the oracle
            assert c["ncand"] <= TILE, (name, q, c)
    w = near[WALL_RING]
    assert w["max_members"] > 32 and w["nruns"] > w["nvox"] + 50 and w["fits32"], w
    o = near[ONE_VOXEL_RING]
    assert o["ncand"] >= 10 and o["nvox"] == 1 and o["nruns"] == 1, o
    assert near[SHORT_RING]["ncand"] == 0, near[SHORT_RING]
    assert near[ONE_CAND_RING]["ncand"] == 1 and near[ONE_CAND_RING]["nvox"] == 1, near[ONE_CAND_RING]
    v = far[OWN_VOXEL_RING]
    assert v["nruns"] > 1024 and v["nruns"] == v["ncand"] == v["nvox"] and v["rb"] == 11 and v["fits32"], v
    x = far[WIDE_RING]
    assert x["nruns"] > 256 and not x["fits32"], x
    # the ordinary rings: a few hundred runs on 32-bit keys
    assert all(c["fits32"] for q, c in far.items() if q != WIDE_RING)
