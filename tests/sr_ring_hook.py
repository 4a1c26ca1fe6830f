"""The diagnostic ring-ID hook (loam_velodyne-1_amd/csrc/dev_hooks.h: loam_dev_sr_ring_of) and a
numpy restatement of scan registration's ring_id with its true boundaries.  Test infrastructure:
the package does not bind the hook."""
import ctypes

import numpy as np

NAME = "loam_dev_sr_ring_of"
MAX_N = 1 << 22
VLP16 = dict(n_rings=16, ring_model=0, ring_lo_deg=-24.8, ring_hi_deg=2.0)
HDL64 = dict(n_rings=64, ring_model=1, ring_lo_deg=-24.8, ring_hi_deg=2.0)


def bind(lib):
    f = getattr(lib, NAME)
    f.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                  ctypes.c_int32] + [ctypes.c_void_p] * 3
    f.restype = ctypes.c_int
    return f


def ring_of(lib, model, xyz, device=0):
    """xyz [n, 3] sensor-frame points -> (ring, exact, fast) int32 [n] each, in chunks the hook takes"""
    f = bind(lib)
    xyz = np.asarray(xyz, np.float32)
    outs = [np.zeros(len(xyz), np.int32) for _ in range(3)]
    for s in range(0, len(xyz), MAX_N):
        p = np.zeros((min(MAX_N, len(xyz) - s), 4), np.float32)
        p[:, :3] = xyz[s:s + len(p)]
        o = [np.zeros(len(p), np.int32) for _ in range(3)]
        rc = f(device, model["n_rings"], model["ring_model"], model["ring_lo_deg"], model["ring_hi_deg"],
               p.ctypes.data, len(p), *[a.ctypes.data for a in o])
        if rc != 0:
            raise RuntimeError(f"{NAME}: {rc}")
        for a, b in zip(outs, o):
            a[s:s + len(p)] = b
    return outs


def ring_id(model, angle):
    """ring_id of float32 angles (degrees), as sr.hip / the reference evaluate it"""
    a = np.asarray(angle, np.float32)
    R = model["n_rings"]
    if model["ring_model"] == 1:
        lo, hi = np.float32(model["ring_lo_deg"]), np.float32(model["ring_hi_deg"])
        step = np.float32((hi - lo) / np.float32(R - 1))
        aid = ((a - lo) / step).astype(np.float32)
        return np.trunc((aid + np.float32(0.5)).astype(np.float32)).astype(np.int64)
    d = a.astype(np.float64)
    r = np.trunc(d + np.where(d < 0.0, -0.5, 0.5)).astype(np.int64)
    return np.where(r > 0, r, r + (R - 1))


def true_boundaries(model):
    """the angles (float64, degrees) at which ring_id changes, around every valid ring: found from
    ring_id itself on a 1/512-degree grid over (-40, 40), each refined to the first float32 that holds
    the new value"""
    g = (np.arange(-40 * 512, 40 * 512 + 1) / 512.0).astype(np.float32)
    v = ring_id(model, g)
    out = []
    for k in np.nonzero(v[1:] != v[:-1])[0]:
        lo, hi = g[k], g[k + 1]
        valid = [x for x in (v[k], v[k + 1]) if 0 <= x < model["n_rings"]]
        if not valid:
            continue
        while True:
            mid = np.float32(lo + (hi - lo) * np.float32(0.5))
            if not (lo < mid < hi):
                break
            if ring_id(model, mid) == v[k]:
                lo = mid
            else:
                hi = mid
        out.append(float(hi))
    return np.array(out, np.float64)


def stated_boundaries(model):
    """the boundaries as the models' formulas state them: every half-integer degree from -15.5 to
    15.5 (VLP-16); lo + (j + 0.5) step, j = -1 .. R - 1 (linear)"""
    R = model["n_rings"]
    if model["ring_model"] == 1:
        lo, hi = model["ring_lo_deg"], model["ring_hi_deg"]
        step = (hi - lo) / (R - 1)
        return lo + (np.arange(-1, R) + 0.5) * step
    return np.arange(-15.5, 15.6, 1.0)


def all_boundaries(model):
    b = np.concatenate([true_boundaries(model), stated_boundaries(model)])
    b = np.sort(b)
    return b[np.concatenate([[True], np.diff(b) > 1e-4])]   # (a stated one within 1e-4 of a found one is the same)


def consecutive_floats(lo, hi):
    """every float32 in [lo, hi], both of one sign and not zero"""
    lo, hi = np.float32(lo), np.float32(hi)
    assert lo <= hi and (lo > 0 or hi < 0)
    a, b = int(np.abs(lo).view(np.uint32)), int(np.abs(hi).view(np.uint32))
    m = np.arange(min(a, b), max(a, b) + 1, dtype=np.uint32).view(np.float32)
    return m if lo > 0 else -m[::-1]
