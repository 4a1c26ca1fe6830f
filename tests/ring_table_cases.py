"""Ring tables (include/loam/loam.h loam_set_ring_table) for the tests: a numpy restatement of the
table rule, the table hook (csrc/dev_hooks.h loam_dev_sr_ring_of_table), the VLP-32C's published
elevations, and an unevenly spaced 32-beam sensor cut from the synthetic HDL-64 sweep.  Test
infrastructure: the package binds the product calls, not the hook."""
import ctypes

import numpy as np

HOOK = "loam_dev_sr_ring_of_table"
MAX_N = 1 << 22

# Velodyne VLP-32C, elevation of laser 0 .. 31 in firing order (degrees, the user manual's table)
VLP32C_ELEV = (-25.0, -1.0, -1.667, -15.639, -11.31, 0.0, -0.667, -8.843, -7.254, 0.333, -0.333, -6.148, -5.333,
               1.333, 0.667, -4.0, -4.667, 1.667, 1.0, -3.667, -3.333, 3.333, 2.333, -2.667, -3.0, 7.0, 4.667,
               -2.333, -2.0, 15.0, 10.333, -1.333)

# the uneven sensor: 32 of the synthetic HDL-64's lasers (elevation -24.8 + 26.8 k / 63 degrees):
# every laser of a dense middle band, every third outside it
KEEP_LASERS = tuple(range(0, 24, 3)) + tuple(range(24, 41)) + tuple(range(43, 64, 3))
assert len(KEEP_LASERS) == 32 and len(set(KEEP_LASERS)) == 32
N_RINGS = 32


def hdl64_elevation(k):
    return -24.8 + (2.0 + 24.8) * np.asarray(k, np.float64) / 63.0


def uneven_sweep(raw):
    """the points of the kept lasers of a synthetic HDL-64 sweep (x, y, z, laser), order kept: true
    rays of the scene"""
    return np.ascontiguousarray(raw[np.isin(raw[:, 3].astype(np.int64), KEEP_LASERS)])


def uneven_table(loam):
    """(bounds, rings) of the kept beams' nominal elevations"""
    return loam.ring_table_from_elevations(hdl64_elevation(KEEP_LASERS))


def vertical_angle(xyz):
    """the reference's vertical angle (degrees, float64) of sensor-frame points: atan(z / hypot(x, y))"""
    p = np.asarray(xyz, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.degrees(np.arctan(p[:, 2] / np.hypot(p[:, 0], p[:, 1])))


def table_rule(bounds, rings, angle):
    """the table rule on float32 angles: ring[i] for bound[i] <= a < bound[i + 1]; -1 outside, for a
    NaN and where ring[i] is -1"""
    b = np.asarray(bounds, np.float32)
    r = np.asarray(rings, np.int64)
    a = np.asarray(angle, np.float32)
    i = np.clip(np.searchsorted(b, a, side="right") - 1, 0, len(r) - 1)
    with np.errstate(invalid="ignore"):
        inside = (a >= b[0]) & (a < b[-1])
    return np.where(inside, r[i], -1)


def margin_to_bounds(bounds, angle):
    """the distance (degrees) of each angle to its nearest bound"""
    b = np.asarray(bounds, np.float64)
    return np.min(np.abs(np.asarray(angle, np.float64)[:, None] - b[None, :]), axis=1)


def moved_sweep(raw, bounds, seed):
    """test_gpu_sr_ring_id.py's moved sweep: every third point to 1e-7 .. 3e-3 degrees (log-uniform, either
    side) from its nearest bound (bounds: sr_ring_hook.all_boundaries of the model)"""
    rng = np.random.default_rng(seed)
    out = raw.copy()
    idx = np.arange(0, len(raw), 3)
    idx = idx[np.all(np.isfinite(raw[idx, :3]), axis=1)]
    hr = np.hypot(raw[idx, 0].astype(np.float64), raw[idx, 1].astype(np.float64))
    elev = np.degrees(np.arctan2(raw[idx, 2].astype(np.float64), hr))
    b = np.asarray(bounds, np.float64)
    near = b[np.argmin(np.abs(elev[:, None] - b[None, :]), axis=1)]
    off = 10.0 ** rng.uniform(-7.0, np.log10(3e-3), len(idx)) * rng.choice([-1.0, 1.0], len(idx))
    out[idx, 2] = (hr * np.tan(np.radians(near + off))).astype(np.float32)
    frac = float(np.mean(np.abs(off) < 1e-3))
    assert 0.85 < frac < 0.93, frac
    return out


def bind(lib):
    f = getattr(lib, HOOK)
    f.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                  ctypes.c_int32] + [ctypes.c_void_p] * 3
    f.restype = ctypes.c_int
    return f


def ring_of(lib, n_rings, bounds, rings, xyz, device=0):
    """xyz [n, 3] sensor-frame points -> (ring, exact, fast) int32 [n] each under the table"""
    f = bind(lib)
    b = np.ascontiguousarray(bounds, np.float32)
    r = np.ascontiguousarray(rings, np.int32)
    assert len(b) == len(r) + 1
    xyz = np.asarray(xyz, np.float32)
    outs = [np.zeros(len(xyz), np.int32) for _ in range(3)]
    for s in range(0, len(xyz), MAX_N):
        p = np.zeros((min(MAX_N, len(xyz) - s), 4), np.float32)
        p[:, :3] = xyz[s:s + len(p)]
        o = [np.zeros(len(p), np.int32) for _ in range(3)]
        rc = f(device, n_rings, len(r), b.ctypes.data, r.ctypes.data, p.ctypes.data, len(p), *[a.ctypes.data for a in o])
        if rc != 0:
            raise RuntimeError(f"{HOOK}: {rc}")
        for a, c in zip(outs, o):
            a[s:s + len(p)] = c
    return outs
