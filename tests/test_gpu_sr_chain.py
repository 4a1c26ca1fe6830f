"""The fused ring sort's chain (sweep ends found once per sweep by k_sr_ring_prep, tile loads issued
ahead of raw_n) and the ring VoxelGrid's two sort-key widths, on the hand-built sweeps of
sr_chain_cases.py: 32 problems (64 sweeps, the smallest launch that takes k_sr_ring_fused) against
the CPU oracle's scanRegistration, bit for bit, and against the same sweeps as 31 problems (the
two-kernel ring sort), bit for bit.

Intensity (ring + 0.1 * relTime) included; the oracle comparison prints the largest intensity difference
before it asserts."""
import numpy as np
import pytest

import sr_chain_cases as sc

pytestmark = pytest.mark.gpu

CLOUDS = ("full", "sharp", "less_sharp", "flat", "less_flat")
_CACHE = {}


def _designs():
    if "designs" not in _CACHE:
        d = dict(sc.ring_sort_sweeps())
        d.update(sc.vg_sweeps())
        _CACHE["designs"] = d
    return _CACHE["designs"]


def _batch(P):
    """P problems whose 2 P sweeps cycle through the designs (every design at both the prev and the cur
    position, since their number is odd); the names of the sweeps in download order"""
    names = sorted(_designs())
    assert len(names) % 2 == 1
    order = [names[j % len(names)] for j in range(2 * P)]
    d = _designs()
    return [d[order[2 * i]] for i in range(P)], [d[order[2 * i + 1]] for i in range(P)], order


def _oracle(oc, name):
    key = ("oracle", name)
    if key not in _CACHE:
        o = oc.Oracle(oc.default_config(system_delay=1), cap=40000)
        raw = _designs()[name]
        assert o.scan_registration(raw)[0] != 0      # inside systemDelay
        rc, f = o.scan_registration(raw)
        assert rc == 0, name
        _CACHE[key] = f
    return _CACHE[key]


def _features(loam, P):
    """the five clouds and the counts of a P-problem run of the designs, computed once per P"""
    key = ("gpu", P)
    if key not in _CACHE:
        prevs, curs, _ = _batch(P)
        e = loam.Engine()
        e.batch_upload(prevs, curs)
        e.batch_run()
        res = e.batch_features()
        _, _, st = e.batch_download()
        e.close()
        _CACHE[key] = (res, st)
    return _CACHE[key]


def _sweep(res, name, j):
    pts, off = res[name]
    return pts[int(off[j]):int(off[j + 1])]


def test_designs_produce_their_cases(oc):
    """the crafted sweeps really are the cases (the CPU check of test_sr_chain_cases.py, repeated here so
    that a generator change cannot hollow this file out)"""
    d = _designs()
    fin = {k: np.nonzero(np.isfinite(v[:, :3]).all(1))[0] for k, v in d.items()}
    assert fin["first_late"][0] > 64
    assert d["last_early"].shape[0] - 1 - fin["last_early"][-1] > 64
    assert d["tile_multiple"].shape[0] == 2 * sc.TILE and fin["tile_multiple"][-1] == 2 * sc.TILE - 1
    assert d["tile_plus_one"].shape[0] == 2 * sc.TILE + 1 and fin["tile_plus_one"][-1] == 2 * sc.TILE
    assert 0 < d["below_tile"].shape[0] < sc.TILE
    sc.check_vg_cases(sc.ring_vg_cases(_oracle(oc, "vg_near")), sc.ring_vg_cases(_oracle(oc, "vg_far")))


def test_fused_chain_equals_oracle(loam, oc):
    """64 sweeps (k_sr_ring_fused, k_sr_ringvg): every sweep's five clouds, bit for bit"""
    res, _ = _features(loam, 32)
    _, _, order = _batch(32)
    worst = 0.0
    for j, name in enumerate(order):
        fo = _oracle(oc, name)
        for c in CLOUDS:
            got = _sweep(res, c, j)
            assert got.shape == fo[c].shape, (j, name, c, got.shape, fo[c].shape)
            if got.size:
                worst = max(worst, float(np.max(np.abs(got[:, 3] - fo[c][:, 3]))))
    print(f"largest intensity difference to the oracle: {worst:.3g}")
    for j, name in enumerate(order):
        fo = _oracle(oc, name)
        for c in CLOUDS:
            got = _sweep(res, c, j)
            assert np.array_equal(got.view(np.uint32), fo[c].view(np.uint32)), (j, name, c)


def test_fused_chain_equals_two_kernel_form(loam):
    """the same sweeps as 31 problems (62 sweeps: k_sr_ring_count / k_sr_ring_scatter): clouds and counts"""
    res32, st32 = _features(loam, 32)
    res31, st31 = _features(loam, 31)
    for c in CLOUDS:
        p32, o32 = res32[c]
        p31, o31 = res31[c]
        np.testing.assert_array_equal(o31, o32[:63], err_msg=c)
        assert np.array_equal(p31.view(np.uint32), p32[:int(o32[62])].view(np.uint32)), c
    # the counts of the two sweeps the shorter batch lacks, from the longer one's own clouds
    for stat, c in (("n_ring", "full"), ("n_sharp", "sharp"), ("n_less_sharp", "less_sharp"), ("n_flat", "flat"),
                    ("n_less_flat", "less_flat")):
        assert st32[stat] == int(res32[c][1][64]) and st31[stat] == int(res31[c][1][62]), stat


@pytest.mark.parametrize("P", [32, 31])
def test_refused_sweeps_ride_along(loam, P):
    """an all-NaN sweep and an empty one among valid ones: both ring-sort forms flag them (the batch
    calls report LOAM_E_INVAL, "sweep has no finite point") and, with the two sweeps replaced, the same
    engine runs the batch as ever"""
    prevs, curs, _ = _batch(P)
    bad = sc.bad_sweeps()
    bp, bc = list(prevs), list(curs)
    bp[3], bc[17] = bad["all_nan"], bad["empty"]
    e = loam.Engine()
    e.batch_upload(bp, bc)
    e.batch_run()
    with pytest.raises(loam.LoamError) as ei:
        e.batch_features()
    assert ei.value.code == loam.LOAM_E_INVAL
    e.batch_upload(prevs, curs)
    e.batch_run()
    res = e.batch_features()
    e.close()
    want, _ = _features(loam, P)
    for c in CLOUDS:
        np.testing.assert_array_equal(res[c][1], want[c][1], err_msg=c)
        assert np.array_equal(res[c][0].view(np.uint32), want[c][0].view(np.uint32)), c
