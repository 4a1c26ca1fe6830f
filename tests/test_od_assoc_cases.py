"""The association cases (tests/od_assoc_cases.py) without a GPU: their preconditions, that every
situation they are built for occurs, and the plain restatement assoc_ref against the oracle's
association (oracle_od_assoc: oracle.cpp od_assoc_corner / od_assoc_surf) index for index."""
import numpy as np
import pytest

import od_assoc_cases as ac
from od_assoc_cases import CORNER, SURF

KINDS = ((CORNER, "corner"), (SURF, "surf"))


def nearest(case):
    """(c, its squared distance, how many points lie at that distance) of every query"""
    out = []
    for q in case.queries:
        d2 = ac.sqdist(case.cloud, q)
        c = int(np.argmin(d2))
        out.append((c, float(d2[c]), int(np.sum(d2 == d2[c]))))
    return out


@pytest.mark.parametrize("name", ac.NAMES)
def test_preconditions(name):
    case = ac.by_name(name)
    assert [c.name for c in ac.all_cases()] == ac.NAMES
    assert 1 <= len(case.cloud) <= 16384 and 1 <= len(case.queries) <= 8192
    assert case.rings.min() >= 0 and case.rings.max() <= 63
    assert np.all(case.queries[:, 3] == np.floor(case.queries[:, 3]))
    assert case.mono == (name != "nonmono")
    # FLANN's tie order is not the subject: every query has one nearest point
    multi = [(i, nn) for i, nn in enumerate(nearest(case)) if nn[2] != 1]
    assert not multi, multi[:5]


@pytest.mark.parametrize("name", ac.NAMES)
def test_restatement_equals_oracle(name, oc):
    case = ac.by_name(name)
    for kind, kn in KINDS:
        ref = case.ref(kind)
        got = oc.od_assoc(case.cloud, case.queries, kind, case.fwd_end)
        bad = np.nonzero((ref != got).any(1))[0]
        assert len(bad) == 0, (kn, bad[:5], ref[bad[:5]], got[bad[:5]])
        f = ref[ref[:, 0] >= 0]
        print(f"{name} {kn}: n {len(case.cloud)} queries {len(case.queries)} (built {case.n_real}) forward end "
              f"{case.fwd_end} | ind1 found {len(f)} none {len(ref) - len(f)} | ind2 found {int((f[:, 1] >= 0).sum())} "
              f"none {int((f[:, 1] < 0).sum())} | ind3 found {int((f[:, 2] >= 0).sum())} none {int((f[:, 2] < 0).sum())}"
              f" | longest window {int(case.visited(kind).max())}")


def test_found_and_not_found_everywhere():
    """ind2 and ind3, each found and not found behind a found ind1; a corner has no ind3"""
    seen = set()
    for case in ac.all_cases():
        c, s = case.ref(CORNER), case.ref(SURF)
        assert np.all(c[:, 2] == -1)
        for what, col, r in (("corner ind2", 1, c), ("surf ind2", 1, s), ("surf ind3", 2, s)):
            has = r[:, 0] >= 0
            if np.any(has & (r[:, col] >= 0)):
                seen.add((case.name, what, "found"))
            if np.any(has & (r[:, col] < 0)):
                seen.add((case.name, what, "none"))
        if np.any(c[:, 0] < 0):
            seen.add((case.name, "ind1", "none"))  # a query with no point below 25 m2
    for what in ("corner ind2", "surf ind2", "surf ind3"):
        for state in ("found", "none"):
            # in a case with whole windows, in one with the forward end clamped, and in the large clouds
            for names in (("rings", "n65"), ("clamp300", "clamp400"), ("random16", "random64")):
                if (what, state) == ("corner ind2", "none") and names[0] == "random16":
                    continue  # (the large clouds have a neighbour ring below 5 m everywhere)
                if (what, state) == ("surf ind3", "none") and names[0] == "random16":
                    continue
                assert any((n, what, state) in seen for n in names), (what, state, names)
    assert ("rings", "ind1", "none") in seen


def test_rings_situations():
    case = ac.by_name("rings")
    rings = case.rings
    c, s = case.ref(CORNER), case.ref(SURF)
    scan = np.where(c[:, 0] >= 0, rings[np.maximum(c[:, 0], 0)], -1)
    for r in ac.RING_IDS:
        assert np.any(scan == r), r  # a nearest point on every ring
    # the lone ring 9: every neighbour ring is more than two away, so the walks stop at once
    assert np.all(c[scan == 9, 1] == -1) and np.all(s[scan == 9, 2] == -1) and np.any(s[scan == 9, 1] >= 0)
    # rings 0 and 63: an other-ring point exists on one side only, and is found there
    assert np.any(c[scan == 0, 1] >= 0) and np.all(rings[c[(scan == 0) & (c[:, 1] >= 0), 1]] == 1)
    assert np.any(c[scan == 63, 1] >= 0) and np.all(rings[c[(scan == 63) & (c[:, 1] >= 0), 1]] == 62)
    assert np.any(c[:, 0] == 0) and np.any(c[:, 0] == len(case.cloud) - 1)
    one = ac.by_name("onering")
    assert np.all(one.ref(CORNER)[:, 1] == -1) and np.all(one.ref(SURF)[:, 2] == -1)
    assert np.any(one.ref(SURF)[:, 1] >= 0)
    for n in (1, 2, 64, 65):
        k = ac.by_name(f"n{n}")
        assert len(k.cloud) == n and k.fwd_end == n
        r = k.ref(SURF)
        assert np.any(r[:, 0] == 0) and np.any(r[:, 0] == n - 1)
    assert np.all(ac.by_name("n1").ref(SURF)[:, 1:] == -1)


def test_clamp_situations():
    """the forward end inside ring `scan`, inside the next ring of the window, at c + 1 and at or before
    c (the last two: an empty forward window)"""
    seen = set()
    for name in ("clamp300", "clamp400"):
        case = ac.by_name(name)
        e, rings = case.fwd_end, case.rings
        assert e == len(case.queries) < len(case.cloud)
        for c in case.ref(SURF)[:, 0]:
            if c < 0:
                continue
            scan = rings[c]
            if c + 1 == e:
                seen.add("at c + 1")
            elif c >= e:
                seen.add("at or before c")
            elif rings[e] == scan:
                seen.add("inside ring scan")
            elif scan < rings[e] <= scan + 2:
                seen.add("inside the next ring")
    assert seen == {"at c + 1", "at or before c", "inside ring scan", "inside the next ring"}, seen


def test_long_windows():
    case = ac.by_name("long")
    for kind, _ in KINDS:
        v, r = case.visited(kind), case.ref(kind)
        # F1 and B1: a walk of more than one box step (4096 points), the other-ring point at its far end
        assert v[0] > 4096 + 2048 and v[1] > 4096 + 2048
        other = r[:, 2] if kind == SURF else r[:, 1]
        assert other[0] - r[0, 0] > 4096 + 2048 and r[1, 0] - other[1] > 4096 + 2048
        assert 0 < other[2] - r[2, 0] < 128 and 0 < r[3, 0] - other[3] < 128  # F2, B2: the first chunks walked
    # every chunk strictly between the query's own and the one found is at least 5 m away
    c = case.cloud
    for q, lo, hi in ((0, case.ref(CORNER)[0, 0], case.ref(CORNER)[0, 1]), (1, case.ref(CORNER)[1, 1], case.ref(CORNER)[1, 0])):
        k0, k1 = lo // 64 + 1, hi // 64
        d2 = ac.sqdist(c[k0 * 64:k1 * 64], case.queries[q])
        assert k1 - k0 > 64 and d2.min() >= 25


def test_ties_are_exact():
    for name, fwd_wins in (("ties", None), ("ties_m", None), ("ties_k", True), ("ties_k_m", True)):
        case = ac.by_name(name)
        d2 = ac.sqdist(case.cloud, case.queries[0])
        for kind, _ in KINDS:
            r = case.ref(kind)[0]
            last = ac.assoc_ref(case.cloud, case.queries[:1], kind, case.fwd_end, last_tie=True)[0]
            c = r[0]
            for col in ((1,) if kind == CORNER else (1, 2)):
                assert r[col] >= 0 and last[col] >= 0 and r[col] != last[col] and d2[r[col]] == d2[last[col]], (name, col)
                # walk order: forward before backward, then by distance from c
                pos = lambda j: (0, j - c) if j > c else (1, c - j)
                assert pos(r[col]) < pos(last[col])
            if fwd_wins:  # K is as distant backward as F1 forward (mirrored: the other way round)
                other = 1 if kind == CORNER else 2
                assert r[other] > c > last[other]
    t = ac.by_name("ties_25")
    d2 = [ac.sqdist(t.cloud, q) for q in t.queries[:3]]
    assert np.sum(d2[0] == 25) == 3 and np.sum(d2[0] < 25) == 1     # only the nearest is below 25
    assert np.all(t.ref(CORNER)[0] == (t.ref(CORNER)[0, 0], -1, -1)) and np.all(t.ref(SURF)[0, 1:] == -1)
    assert np.all(t.ref(SURF)[1] >= 0) and t.ref(CORNER)[1, 1] >= 0  # just below 25: taken
    assert 24 < np.sort(d2[1])[1] < 25
    assert d2[2].min() == 25 and np.all(t.ref(SURF)[2] == -1) and np.all(t.ref(CORNER)[2] == -1)


def test_nonmono_walk_stops_early():
    """from a nearest point in the ring 0 block the forward walk meets the ring 4 block first and
    stops, although ring 1 points below 5 m follow"""
    case = ac.by_name("nonmono")
    r = case.ref(CORNER)
    hits = 0
    for i in np.nonzero((r[:, 0] >= 0) & (r[:, 0] < ac.PER_RING))[0]:
        d2 = ac.sqdist(case.cloud, case.queries[i])
        assert r[i, 1] == -1
        hits += int(np.any((case.rings == 1) & (d2 < 25)))
    assert hits > 50


def test_seed_sets_are_valid(oc):
    for name in ("rings", "ties_k", "n1", "long"):
        case = ac.by_name(name)
        for kind, _ in KINDS:
            sets = ac.seed_sets(case, kind, oc.od_assoc)
            assert {"moved", "random", "far"} <= set(sets)
            for k, s in sets.items():
                assert s.shape == (len(case.queries), 3) and s.dtype == np.int32
                assert s.min() >= -1 and s.max() < len(case.cloud), k
            far = sets["far"][:case.n_real]
            for i in np.nonzero(far[:, 0] >= 0)[0][:50]:
                assert np.all(ac.sqdist(case.cloud, case.queries[i])[far[i]] >= 25)
            ref = case.ref(kind)
            assert np.any(sets["random"][:, 1] == ref[:, 0])  # a seed equal to c
