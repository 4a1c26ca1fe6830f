"""k_sr_features at the edges of its tiles: sweeps of 11, 12 and 13 points (the first lengths with
a curvature at all: 5 neighbours either side), 1023, 1024 and 1025 (a kFeatSpan tile's end and its
6-point halo) and 2060 (a second tile that is mostly halo), plus one full sweep.  All five clouds
against the CPU oracle, as a single node call and as the sweeps of one batch, with
test_gpu_batch_features.py's tolerances: x, y, z bit-exact, intensity within 2e-6."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

INT_TOL = 2e-6
CLOUDS = ("full", "sharp", "less_sharp", "flat", "less_flat")
LENGTHS = (11, 12, 13, 1023, 1024, 1025, 2060, None)

_SWEEPS = []


def _sweeps(sg, oc):
    """the eight sweeps (windows of one synthetic sweep) and their oracle clouds, computed once"""
    if not _SWEEPS:
        prev, cur = sg.batch_problems(1, base_seed=4300)
        for k, n in enumerate(LENGTHS):
            raw = cur[0] if n is None else cur[0][700 * k:700 * k + n].copy()
            o = oc.Oracle(oc.default_config(system_delay=1), cap=40000)
            assert o.scan_registration(raw)[0] != 0
            rc, f = o.scan_registration(raw)
            assert rc == 0
            _SWEEPS.append((raw, f))
    return _SWEEPS


def _cmp(got, want, what):
    for name in CLOUDS:
        a, b = got[name], want[name]
        assert a.shape == b.shape, f"{what} {name}: {a.shape} vs {b.shape}"
        np.testing.assert_array_equal(a[:, :3], b[:, :3], err_msg=f"{what} {name}")
        if a.shape[0]:
            assert np.max(np.abs(a[:, 3] - b[:, 3])) <= INT_TOL, f"{what} {name}"


@pytest.mark.parametrize("k", range(len(LENGTHS)))
def test_single_sweep(loam, oc, sg, k):
    raw, want = _sweeps(sg, oc)[k]
    node = loam.Engine(loam.default_config(system_delay=1))
    assert node.scan_registration(raw)[0] == loam.LOAM_E_NOT_READY
    rc, f = node.scan_registration(raw)
    node.close()
    assert rc == 0
    _cmp(f, want, f"{len(raw)} points, node call")


def test_batch(loam, oc, sg):
    sw = _sweeps(sg, oc)
    e = loam.Engine()
    e.batch_upload([s[0] for s in sw[0::2]], [s[0] for s in sw[1::2]])
    e.batch_run()
    res = e.batch_features()
    e.close()
    for j, (raw, want) in enumerate(sw):
        got = {n: res[n][0][int(res[n][1][j]):int(res[n][1][j + 1])] for n in CLOUDS}
        _cmp(got, want, f"{len(raw)} points, batch sweep {j}")
