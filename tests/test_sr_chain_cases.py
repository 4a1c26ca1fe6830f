"""The hand-built sweeps of sr_chain_cases.py on the CPU: each produces the case it is there for, by
the oracle's scanRegistration and the numpy restatement of the ring VoxelGrid's view of a ring."""
import numpy as np

import sr_chain_cases as sc


def _sr(oc, raw):
    o = oc.Oracle(oc.default_config(system_delay=1), cap=40000)
    assert o.scan_registration(raw)[0] != 0      # inside systemDelay
    return o.scan_registration(raw)


def test_ring_sort_sweeps(oc):
    d = sc.ring_sort_sweeps()
    fin = {k: np.nonzero(np.isfinite(v[:, :3]).all(1))[0] for k, v in d.items()}
    assert fin["first_late"][0] > 64
    assert d["last_early"].shape[0] - 1 - fin["last_early"][-1] > 64
    assert d["tile_multiple"].shape[0] == 2 * sc.TILE and fin["tile_multiple"][-1] == 2 * sc.TILE - 1
    assert d["tile_plus_one"].shape[0] == 2 * sc.TILE + 1 and fin["tile_plus_one"][-1] == 2 * sc.TILE
    assert 0 < d["below_tile"].shape[0] < sc.TILE
    for name, raw in d.items():
        rc, f = _sr(oc, raw)
        assert rc == 0 and f["full"].shape[0] == fin[name].size, name   # every finite point lies on a ring
        assert np.unique(f["full"][:, 3].astype(int)).size == sc.R, name
    for name, raw in sc.bad_sweeps().items():
        assert _sr(oc, raw)[0] != 0, name


def test_ring_vg_sweeps(oc):
    res = {}
    for name, raw in sc.vg_sweeps().items():
        rc, f = _sr(oc, raw)
        assert rc == 0, name
        res[name] = sc.ring_vg_cases(f)
    sc.check_vg_cases(res["vg_near"], res["vg_far"])
