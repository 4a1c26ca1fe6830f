"""Scan registration's ring ID from tangent thresholds (sr.hip ring_of) against the exact
evaluation it replaces on the common path (ring_of_exact), for the VLP-16 and the 64-ring linear
model, through the hook loam_dev_sr_ring_of and through the product against the CPU oracle.

Hook, per model: (i) for every true boundary of ring_id (found from ring_id itself, plus the
half-integer / lo + (j + 0.5) step lists the models state) and horizontal ranges 0.5 m, 5 m and
50 m, every consecutive float py within 4e-3 degrees of the boundary: the production ring equals
the exact one; (ii) an unmodified synthetic sweep: the thresholds decide every point; (iii)
degenerate points (px = pz = 0, +-0, 1e-3 m and 200 m, elevations beyond +-16 degrees): the
exact evaluation, or a ring outside 0 .. R - 1 that agrees with it.

Product: a sweep with every third point moved to 1e-7 .. 3e-3 degrees (log-uniform: about 89 %
inside the 1e-3 degree guard) from its nearest boundary, as a single node call (the two-kernel
ring sort) and in a batch of 32 problems (k_sr_ring_fused); all five clouds against the oracle
with test_gpu_batch_features.py's tolerances: x, y, z bit-exact, intensity within 2e-6."""
import numpy as np
import pytest

import sr_ring_hook as rh

pytestmark = pytest.mark.gpu

INT_TOL = 2e-6
CLOUDS = ("full", "sharp", "less_sharp", "flat", "less_flat")
MODELS = {"vlp16": rh.VLP16, "linear64": rh.HDL64}
WINDOW_DEG = 4e-3


def _near_boundary_points(model):
    """set (i): sensor-frame points (x, y horizontal at a fixed azimuth per range, z = py)"""
    parts = []
    for k, hr in enumerate((0.5, 5.0, 50.0)):
        az = 0.3 + 1.1 * k
        x, y = np.float32(hr * np.cos(az)), np.float32(hr * np.sin(az))
        r = np.sqrt(np.float64(np.float32(np.float32(x * x) + np.float32(y * y))))   # sqrt of the kernel's float r2
        for b in rh.all_boundaries(model):
            lo, hi = r * np.tan(np.radians(b - WINDOW_DEG)), r * np.tan(np.radians(b + WINDOW_DEG))
            z = rh.consecutive_floats(lo, hi)
            p = np.empty((len(z), 3), np.float32)
            p[:, 0], p[:, 1], p[:, 2] = x, y, z
            parts.append(p)
    return np.concatenate(parts)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_ring_equals_exact_at_every_boundary(loam, name):
    model = MODELS[name]
    b = rh.all_boundaries(model)
    assert len(b) >= (32 if name == "vlp16" else 65), b
    pts = _near_boundary_points(model)
    ring, exact, fast = rh.ring_of(loam.lib(), model, pts)
    nfast = int(fast.sum())
    print(f"{name}: {len(pts)} points, {nfast} decided by the thresholds, {len(pts) - nfast} by the exact evaluation")
    bad = np.nonzero(ring != exact)[0]
    assert bad.size == 0, (bad[:5], pts[bad[:5]], ring[bad[:5]], exact[bad[:5]])
    assert 0 < nfast < len(pts)      # both sides of the guard are in the set
    R = model["n_rings"]
    assert set(np.unique(exact[(exact >= 0) & (exact < R)])) == set(range(R))   # every ring's boundaries were reached


@pytest.mark.parametrize("name", sorted(MODELS))
def test_thresholds_decide_a_plain_sweep(loam, sg, name):
    """set (ii): no point of a synthetic sweep lies within 0.2 degrees of a boundary, so none may take
    the exact evaluation (the fast path is not dead code)"""
    model = MODELS[name]
    _, cur = sg.single_problem(0) if name == "vlp16" else sg.single_problem(2, lidar=sg.HDL64)
    pts = cur[np.all(np.isfinite(cur[:, :3]), axis=1)][:, :3]
    ring, exact, fast = rh.ring_of(loam.lib(), model, pts)
    np.testing.assert_array_equal(ring, exact)
    assert int(fast.sum()) == len(pts), np.nonzero(fast == 0)[0][:10]
    assert np.all((ring >= 0) & (ring < model["n_rings"]))


@pytest.mark.parametrize("name", sorted(MODELS))
def test_degenerate_points_take_the_exact_evaluation(loam, name):
    """set (iii)"""
    model = MODELS[name]
    R = model["n_rings"]
    pts = []
    for z in (0.0, -0.0, 1e-3, -1e-3, 200.0, -200.0):
        for h in (0.0, -0.0):
            pts.append((h, h, z))          # px = pz = 0 (the sensor's x, y), py zero or not
            pts.append((h, -h, z))
    # elevations beyond the model's rings: +-16 degrees for VLP-16; the linear model's own ends
    # (its ring 0 reaches down to lo - 1.5 step = -25.44, its ring 63 up to hi + 0.5 step = 2.21)
    elevs = ((16.5, -16.5, 17.2, -25.9, 30.0, -30.0, 45.0, -60.0, 89.0, -89.0) if name == "vlp16" else
             (2.5, 3.0, 16.5, 30.0, 89.0, -25.6, -25.9, -30.0, -60.0, -89.0))
    for mag in (1e-3, 200.0):
        for elev in elevs:
            pts.append((mag * np.cos(np.radians(elev)), 0.0, mag * np.sin(np.radians(elev))))
            pts.append((0.0, -mag * np.cos(np.radians(elev)), mag * np.sin(np.radians(elev))))
    pts = np.array(pts, np.float32)
    ring, exact, fast = rh.ring_of(loam.lib(), model, pts)
    np.testing.assert_array_equal(ring, exact)
    inside = (ring >= 0) & (ring < R)
    horizontal_zero = (pts[:, 0] == 0) & (pts[:, 1] == 0)
    assert np.all(fast[horizontal_zero] == 0)
    assert np.all(~inside[~horizontal_zero])                  # (the elevations are beyond the rings)
    assert np.all((fast == 0) | (~inside & (ring == exact)))


# ---------------------------------------------------------------- through the product
def _moved_sweep(raw, model, seed):
    """every third point to 1e-7 .. 3e-3 degrees (log-uniform, either side) from its nearest boundary"""
    rng = np.random.default_rng(seed)
    out = raw.copy()
    idx = np.arange(0, len(raw), 3)
    idx = idx[np.all(np.isfinite(raw[idx, :3]), axis=1)]
    hr = np.hypot(raw[idx, 0].astype(np.float64), raw[idx, 1].astype(np.float64))
    elev = np.degrees(np.arctan2(raw[idx, 2].astype(np.float64), hr))
    b = rh.all_boundaries(model)
    near = b[np.argmin(np.abs(elev[:, None] - b[None, :]), axis=1)]
    off = 10.0 ** rng.uniform(-7.0, np.log10(3e-3), len(idx)) * rng.choice([-1.0, 1.0], len(idx))
    out[idx, 2] = (hr * np.tan(np.radians(near + off))).astype(np.float32)
    frac = float(np.mean(np.abs(off) < 1e-3))
    assert 0.85 < frac < 0.93, frac
    return out


def _oracle(oc, raw, kw):
    kw = dict(kw, system_delay=1)
    o = oc.Oracle(oc.default_config(**kw), cap=int(kw.get("max_points", 40000)))
    assert o.scan_registration(raw)[0] != 0
    rc, f = o.scan_registration(raw)
    assert rc == 0
    return f


def _cmp(got, want, what):
    for name in CLOUDS:
        a, b = got[name], want[name]
        assert a.shape == b.shape, f"{what} {name}: {a.shape} vs {b.shape}"
        np.testing.assert_array_equal(a[:, :3], b[:, :3], err_msg=f"{what} {name}")
        if a.shape[0]:
            assert np.max(np.abs(a[:, 3] - b[:, 3])) <= INT_TOL, f"{what} {name}"


_CASES = {}


def _case(sg, oc, loam, name):
    """the moved sweep of a model, its oracle clouds and the engine configuration (computed once)"""
    if name not in _CASES:
        if name == "vlp16":
            kw, model = {}, rh.VLP16
            prevs, curs = sg.batch_problems(2, base_seed=4100)
        else:
            kw, model = dict(n_rings=64, ring_model=loam.RING_LINEAR, max_points=160000), rh.HDL64
            prevs, curs = sg.batch_problems(2, base_seed=4100, lidar=sg.HDL64)
        moved = _moved_sweep(curs[0], model, 5)
        _CASES[name] = (kw, list(prevs), list(curs), moved, _oracle(oc, moved, kw))
    return _CASES[name]


@pytest.mark.parametrize("name", sorted(MODELS))
def test_moved_sweep_single_call(loam, oc, sg, name):
    kw, _, _, moved, want = _case(sg, oc, loam, name)
    node = loam.Engine(loam.default_config(system_delay=1, **kw))
    assert node.scan_registration(moved)[0] == loam.LOAM_E_NOT_READY
    rc, f = node.scan_registration(moved)
    node.close()
    assert rc == 0
    _cmp(f, want, f"{name} node call")


@pytest.mark.parametrize("name", sorted(MODELS))
def test_moved_sweep_in_a_fused_batch(loam, oc, sg, name):
    """32 problems = 64 sweeps: the smallest launch that takes k_sr_ring_fused; the moved sweep is
    the first and the last sweep of the batch"""
    kw, prevs, curs, moved, want = _case(sg, oc, loam, name)
    bp = [moved] + [prevs[i % 2] for i in range(1, 32)]
    bc = [curs[i % 2] for i in range(31)] + [moved]
    e = loam.Engine(loam.default_config(**kw))
    e.batch_upload(bp, bc)
    e.batch_run()
    res = e.batch_features()
    e.close()
    for j in (0, 63):
        got = {n: res[n][0][int(res[n][1][j]):int(res[n][1][j + 1])] for n in CLOUDS}
        _cmp(got, want, f"{name} batch sweep {j}")
