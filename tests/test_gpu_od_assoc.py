"""One association round of the odometry (csrc/od.hip od_assoc_round: k_od_sel / k_od_sel_nn,
k_od_assoc, od_assoc_wave, wave_window, wave_window_mono) through the diagnostic hook
loam_dev_od_assoc_run (csrc/dev_hooks.h) on the cases of tests/od_assoc_cases.py: ind1, ind2, ind3 of
every query as integers against the plain restatement assoc_ref (which tests/test_od_assoc_cases.py
ties to the oracle), in every launch form, with both window algorithms, both hash build forms, the
counting instantiations, unseeded and seeded.  DESIGN.md §5.3."""
import numpy as np
import pytest

import od_assoc_cases as ac
import od_assoc_hook as hook
from od_assoc_cases import CORNER, SURF

pytestmark = pytest.mark.gpu

SMALL = [n for n in ac.NAMES if not n.startswith("random")]
MONO = (0, 3)  # od_win_mono: the walks, the index ranges (od_win_mono_min = 1)


@pytest.fixture(scope="module")
def h(loam):
    handle = hook.Handle(loam.lib())
    yield handle
    handle.close()


_SEEDS = {}


def seeds_of(case, oc):
    """{set name: (corner seeds, surf seeds)}, made once per case"""
    if case.name not in _SEEDS:
        c, s = ac.seed_sets(case, CORNER, oc.od_assoc), ac.seed_sets(case, SURF, oc.od_assoc)
        _SEEDS[case.name] = {k: (c[k], s[k]) for k in c}
    return _SEEDS[case.name]


def assert_ind(case, res, p, what):
    for kind, got in ((CORNER, res.corner[p]), (SURF, res.surf[p])):
        ref = case.ref(kind)
        bad = np.nonzero((ref != got).any(1))[0]
        assert len(bad) == 0, (case.name, what, "corner" if kind == CORNER else "surf", bad[:5].tolist(),
                               ref[bad[:5]].tolist(), got[bad[:5]].tolist())


def assert_tables(case, res, p):
    """the hash build's mono flags and ring start tables (meaningful for a ring-monotone cloud)"""
    assert res.mono[p].tolist() == [int(case.mono)] * 2, case.name
    if case.mono:
        for k in range(2):
            np.testing.assert_array_equal(res.rstart[p, k], case.ring_starts())


def run_forms(h, case, launch, mono, seeds=None, what=""):
    """both hash build forms, COUNT off and on; returns the counting runs' counters"""
    counters = []
    for hash_form in (hook.HASH_GRID, hook.HASH_SINGLE):
        first = None
        for count in (0, 1):
            res = h.run([case.problem(seeds)], launch=hook.LAUNCHES[launch], od_win_mono=mono, count=count,
                        hash_form=hash_form)
            assert_ind(case, res, 0, f"{what} {launch} mono {mono} hash {hash_form} count {count}")
            assert_tables(case, res, 0)
            if count == 0:
                first = res.raw
                assert res.counters.tolist() == [[0, 0]]
            else:
                np.testing.assert_array_equal(res.raw, first)
                counters.append(res.counters[0].copy())
    return counters


@pytest.mark.parametrize("mono", MONO)
@pytest.mark.parametrize("launch", list(hook.LAUNCHES))
@pytest.mark.parametrize("name", SMALL)
def test_first_round(h, name, launch, mono):
    run_forms(h, ac.by_name(name), launch, mono, what="unseeded")


@pytest.mark.parametrize("mono", MONO)
@pytest.mark.parametrize("launch", list(hook.LAUNCHES))
@pytest.mark.parametrize("name", SMALL)
def test_seeded_round(h, oc, name, launch, mono):
    """seeds only bound the searches: the moved query's answer, random indices, points beyond 5 m, and
    (ties) the last of equally distant points in walk order all leave the unseeded answer"""
    case = ac.by_name(name)
    sets = seeds_of(case, oc)
    assert ("last_tie" in sets) == name.startswith("ties")
    for k, seeds in sets.items():
        run_forms(h, case, launch, mono, seeds, what=f"seeds {k}")


@pytest.mark.parametrize("mono", MONO)
@pytest.mark.parametrize("launch", list(hook.LAUNCHES))
@pytest.mark.parametrize("name", ["random16", "random64"])
def test_random(h, oc, name, launch, mono):
    """the large clouds, also with 16 (and 32) workgroups: a wave then stages its 3000 / 16 = 188 queries
    as two full batches of 64 and one of 60 (94: one full and one of 30)"""
    case = ac.by_name(name)
    sets = seeds_of(case, oc)
    for seeds, what in ((None, "unseeded"), (sets["moved"], "seeds moved"), (sets["random"], "seeds random")):
        for grid in (0, 16, 32):
            for hash_form, count in ((hook.HASH_GRID, 0), (hook.HASH_SINGLE, 1)):
                res = h.run([case.problem(seeds)], launch=hook.LAUNCHES[launch], od_win_mono=mono, grid=grid,
                            count=count, hash_form=hash_form)
                assert_ind(case, res, 0, f"{what} {launch} mono {mono} grid {grid} hash {hash_form}")
                assert_tables(case, res, 0)


@pytest.mark.parametrize("mono", MONO)
def test_long_skips_chunks(h, mono):
    """on `long` the windows of the seven built queries hold tens of thousands of points; the search
    loads far fewer (its nearest neighbour cells included): the skip is taken, not bypassed.  The
    padding queries have no point below 25 m2, so no windows, but their 27 hash buckets hold points:
    what they gather is measured by a job of the padding queries alone and taken off."""
    case = ac.by_name("long")
    window = int(case.visited(CORNER).sum() + case.visited(SURF).sum())
    pads = case.queries[case.n_real:]
    pad_job = dict(corner_last=case.cloud, surf_last=case.cloud, corner_q=pads, surf_q=pads)
    for launch in hook.LAUNCHES:
        res = h.run([pad_job], launch=hook.LAUNCHES[launch], od_win_mono=mono, count=1)
        assert np.all(res.corner[0] == -1) and np.all(res.surf[0] == -1)
        for gathered, boxes in run_forms(h, case, launch, mono, what="long"):
            built = int(gathered) - int(res.counters[0, 0])
            print(f"long {launch} mono {mono}: window points {window}, gathered {gathered}, of the padding "
                  f"{res.counters[0, 0]}, of the built queries {built}, boxes {boxes}")
            assert 0 < built < window and boxes > 0


def test_three_problems_in_one_call(h, oc):
    """P = 3 with three different cases: each problem's result is its own P = 1 result"""
    cases = [ac.by_name(n) for n in ("rings", "n1", "ties_k")]
    for seeded in (False, True):
        probs = [c.problem(seeds_of(c, oc)["random"] if seeded else None) for c in cases]
        for launch in hook.LAUNCHES:
            for mono in MONO:
                for hash_form in (hook.HASH_GRID, hook.HASH_SINGLE):
                    res = h.run(probs, launch=hook.LAUNCHES[launch], od_win_mono=mono, hash_form=hash_form, count=1)
                    for p, c in enumerate(cases):
                        assert_ind(c, res, p, f"P = 3 {launch} mono {mono} hash {hash_form} seeded {seeded}")
                        assert_tables(c, res, p)
                        one = h.run([probs[p]], launch=hook.LAUNCHES[launch], od_win_mono=mono, hash_form=hash_form,
                                    count=1)
                        np.testing.assert_array_equal(one.corner[0], res.corner[p])
                        np.testing.assert_array_equal(one.surf[0], res.surf[p])
                        np.testing.assert_array_equal(one.counters[0], res.counters[p])


def test_handle_reuse(h):
    """long, then the one-point cloud, then long again on one handle: nothing of a job survives"""
    a, b = ac.by_name("long"), ac.by_name("n1")
    for mono in MONO:
        first = h.run([a.problem()], od_win_mono=mono, count=1)
        small = h.run([b.problem()], od_win_mono=mono, count=1)
        again = h.run([a.problem()], od_win_mono=mono, count=1)
        assert_ind(a, first, 0, "long")
        assert_ind(b, small, 0, "n1 after long")
        assert_tables(b, small, 0)
        np.testing.assert_array_equal(first.raw, again.raw)
        np.testing.assert_array_equal(first.counters, again.counters)
        np.testing.assert_array_equal(first.rstart, again.rstart)


@pytest.mark.parametrize("mono", MONO)
@pytest.mark.parametrize("launch", list(hook.LAUNCHES))
def test_unwritten_entries_show(h, launch, mono):
    """an unseeded job leaves the sentinel wherever no kernel wrote: none within the queries, in
    every launch form, with the default grid and with 16 workgroups"""
    for name in ("clamp300", "n1", "random16"):
        case = ac.by_name(name)
        for grid in (0, 16):
            res = h.run([case.problem()], launch=hook.LAUNCHES[launch], od_win_mono=mono, grid=grid)
            assert not np.any(res.raw[:, :, :2 * len(case.queries)] == hook.SENTINEL), (name, grid)
