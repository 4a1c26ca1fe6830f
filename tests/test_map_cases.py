"""The preconditions of tests/map_cases.py, on the oracle alone (no GPU): every case reaches the
branch of the map update it is meant to reach, told from what Oracle.map_export() reports about each
frame's insertion (src/laserMapping.cpp:980-1016), not from the engine.  And the oracle's export
itself: it rebuilds the oracle's own /laser_cloud_surround, its insertion counts add up to the stack,
and oracle_map_export answers the sizes-only query and refuses too little room as loam_map_export does."""
import ctypes

import numpy as np
import pytest

import map_cases as mc
from test_gpu_map import _bits, _check_offsets, _frame_position, _surround_input, cube_keys
from vg_cases import oracle_vg

KINDS = ("corner", "surf")


def _cube(m, kind, c):
    off = m[kind + "_offset"]
    return m[kind][off[c]:off[c + 1]]


@pytest.fixture(scope="module")
def vg(oc):
    return oracle_vg(oc)


@pytest.mark.parametrize("name", mc.CASES)
def test_insertion_counts_add_up_to_the_stack(oc, sg, name):
    run = mc.oracle_run(name, oc, sg)
    assert len(run) == len(mc.frames(name, oc, sg)) >= 2
    for m, r in enumerate(run):
        e = r["map"]
        _check_offsets(e)
        assert e["inserted"].shape == (2, mc.NCUBE) and e["inserted"].min() >= 0
        assert int(e["inserted"].sum()) + sum(e["dropped"]) == r["mp_stack"], (name, m)
        np.testing.assert_array_equal(_bits(e["aft"]), _bits(r["aft"]))
        np.testing.assert_array_equal(_bits(e["bef"]), _bits(r["bef"]))


@pytest.mark.parametrize("name", mc.CASES)
def test_export_rebuilds_the_oracles_surround(oc, sg, vg, name):
    fr, run = mc.frames(name, oc, sg), mc.oracle_run(name, oc, sg)
    published = 0
    for m, (f, r) in enumerate(zip(fr, run)):
        assert (r["surround"] is not None) == (m % 5 == 0) == (r["map"]["surround_phase"] == 0), (name, m)
        if r["surround"] is None:
            continue
        pos = _frame_position(run[m - 1] if m else None, {"pose": f["odom"]}, f["jump"])
        src = _surround_input(r["map"], pos)
        out = vg(src, 0.2) if len(src) else src
        assert out.shape == r["surround"].shape, (name, m)
        np.testing.assert_array_equal(_bits(out), _bits(r["surround"]), err_msg=f"{name} surround@{m}")
        published += 1
    assert published >= 1
    if name in ("wide", "shifted"):
        assert any(r["surround"] is not None and len(r["surround"]) > 1000 for r in run)


def test_sizes_only_query_and_capacity_refusal(oc, sg):
    o = oc.Oracle(oc.default_config(**mc.CFG))
    full = mc.map_frame(o, mc.frames("edge513", oc, sg)[0])["map"]
    assert full["corner"].shape[0] == 8 and full["surf"].shape[0] == 505
    L = oc.lib()
    m = oc.Map()
    assert L.oracle_map_export(o.h, ctypes.byref(m), None, None) == 0  # sizes only, no offsets
    assert (m.corner.count, m.surf.count, m.surround_phase) == (8, 505, 0) and list(m.center) == [10, 5, 10]
    sent = np.full((505, 4), -7.5, np.float32)
    small = np.full((7, 4), -7.5, np.float32)
    offs = [np.full(mc.NCUBE + 1, 0xFFFFFFFF, np.uint32) for _ in range(2)]
    ins = np.full((2, mc.NCUBE), -1, np.int32)
    m = oc.Map()
    m.corner.pts, m.corner.capacity, m.corner.cube_offset = small.ctypes.data, 7, offs[0].ctypes.data
    m.surf.pts, m.surf.capacity, m.surf.cube_offset = sent.ctypes.data, 505, offs[1].ctypes.data
    assert L.oracle_map_export(o.h, ctypes.byref(m), ins.ctypes.data, None) == -2  # LOAM_E_CAPACITY
    assert (m.corner.count, m.surf.count) == (8, 505)
    np.testing.assert_array_equal(offs[0], full["corner_offset"])
    np.testing.assert_array_equal(offs[1], full["surf_offset"])
    np.testing.assert_array_equal(ins, full["inserted"])
    assert np.all(sent == -7.5) and np.all(small == -7.5)  # no point written
    assert L.oracle_map_export(o.h, None, None, None) == -1
    again = o.map_export()  # the export changes nothing
    for k in again:
        np.testing.assert_array_equal(again[k], full[k], err_msg=k)


def _grown_far(prev, f, r):
    """cubes outside the frame's 5x5x5 neighbourhood that held points and got more (raw old ++ appended)"""
    cube, _, n = mc.frame_cube(prev, f)
    assert n == 0
    far = mc.cheb(np.arange(mc.NCUBE), cube) > 2
    return int(((mc.cube_sizes(prev["map"]) > 0) & (r["map"]["inserted"] > 0) & far[None, :]).any(axis=0).sum())


@pytest.mark.parametrize("name", ("wide", "wide_out"))
def test_wide_frames_take_the_one_wave_ranking(oc, sg, name):
    fr, run = mc.frames(name, oc, sg), mc.oracle_run(name, oc, sg)
    assert len(run) >= 3
    for m, (f, r) in enumerate(zip(fr, run)):
        grown = _grown_far(run[m - 1], f, r) if m else 0
        print(f"{name} frame {m}: {len(f['corner_last'])} + {len(f['surf_last'])} points, keys {mc.keys_of(r)}, "
              f"dropped {r['map']['dropped']}, cubes outside the neighbourhood grown raw {grown}")
        assert len(f["corner_last"]) <= 120 * mc.N_RINGS and len(f["surf_last"]) <= 29000
        assert mc.keys_of(r) > mc.K_DENSE
        if m:
            assert grown >= 100
        if name == "wide_out":
            assert sum(r["map"]["dropped"]) > 0
        else:
            assert r["map"]["dropped"] == (0, 0)


def test_below_stays_on_the_dense_ranking(oc, sg):
    fr, run = mc.frames("below", oc, sg), mc.oracle_run("below", oc, sg)
    assert len(run) >= 3
    for m, r in enumerate(run):
        print(f"below frame {m}: keys {mc.keys_of(r)}, cubes outside the neighbourhood grown raw "
              f"{_grown_far(run[m - 1], fr[m], r) if m else 0}")
        assert 300 < mc.keys_of(r) < mc.K_DENSE


@pytest.mark.parametrize("name", sorted(mc.EDGES))
def test_edge_cases_hold_exactly_their_keys(oc, sg, name):
    n = mc.EDGES[name]
    fr, cubes = mc.edge_frames(n)
    run = mc.oracle_run(name, oc, sg)
    assert len(fr) == 2 and mc.cheb(np.concatenate(list(cubes.values()))).min() >= 3
    assert len(set(cubes["corner"]) | set(cubes["surf"])) == n  # (the corner cubes are further ones)
    for k, kind in enumerate(KINDS):
        for f in fr:
            assert len(f[kind + "_last"]) <= (120 * mc.N_RINGS, mc.MAX_POINTS)[k]
        # frame 0: one point at each cube's centre
        np.testing.assert_array_equal(cube_keys(fr[0][kind + "_last"], (10, 5, 10)), cubes[kind])
        np.testing.assert_array_equal(fr[0][kind + "_last"][:, :3], mc.cube_centre(cubes[kind]).astype(np.float32))
        # frame 1: 5..9 points into each of the same cubes, one cube after the other, at least 1 m apart
        key = cube_keys(fr[1][kind + "_last"], (10, 5, 10))
        cnt = np.bincount(key, minlength=mc.NCUBE)
        assert set(np.flatnonzero(cnt)) == set(cubes[kind]) and cnt[cubes[kind]].min() >= 5 and cnt[cubes[kind]].max() <= 9
        assert np.all(key[1:] != key[:-1])
        for c in cubes[kind]:
            p = fr[1][kind + "_last"][key == c, :3].astype(np.float64)
            d = np.linalg.norm(p[:, None] - p[None], axis=2) + 1e9 * np.eye(len(p))
            assert d.min() >= 1.0
    for m, r in enumerate(run):
        print(f"{name} frame {m}: keys {mc.keys_of(r)}, stack {r['mp_stack']}")
        assert mc.keys_of(r) == n and r["map"]["dropped"] == (0, 0) and r["mp_iters"] == 0
        for k, kind in enumerate(KINDS):
            assert set(np.flatnonzero(r["map"]["inserted"][k])) == set(cubes[kind])
    assert run[1]["map"]["inserted"].max() <= 9 and run[1]["map"]["inserted"][run[1]["map"]["inserted"] > 0].min() >= 5


def test_order_case(oc, sg, vg):
    fr, run = mc.frames("order", oc, sg), mc.oracle_run("order", oc, sg)
    assert len(run) == 3
    cubes = [mc.ORDER_CORNER] + mc.ORDER_SURF
    assert mc.cheb(np.array(cubes)).min() > 2
    for m, (f, r) in enumerate(zip(fr, run)):
        ins = r["map"]["inserted"]
        assert 3 <= mc.keys_of(r) <= 8 and ins[ins > 0].min() > 1000 and r["map"]["dropped"] == (0, 0)
        nsc, nst = int(ins[0].sum()), int(ins.sum())
        assert nst % 64 != 0 and nsc % 64 != 0  # the corner / surf boundary falls inside a 64-point step
        assert len(f["corner_last"]) <= 120 * mc.N_RINGS
        # the surf stack as the reference builds it (identity pose: VoxelGrid 0.4 of surf_last)
        stack = vg(f["surf_last"], 0.4)
        assert len(stack) == int(ins[1].sum())
        assert not np.array_equal(_bits(stack), _bits(f["surf_last"]))  # (the VoxelGrid reorders the input)
        key = cube_keys(stack, (10, 5, 10))
        assert np.all(key[1:] != key[:-1])  # keys change with every point
        # the map holds the stack's points of every cube in stack order
        for c in mc.ORDER_SURF:
            np.testing.assert_array_equal(_bits(_cube(r["map"], "surf", c)[-ins[1][c]:]), _bits(stack[key == c]))
    # the exported map holds points of two and more frames in raw order: old ++ appended
    raw = 0
    for k, kind in enumerate(KINDS):
        for c in ([mc.ORDER_CORNER], mc.ORDER_SURF)[k]:
            a, b, d = (_cube(run[t]["map"], kind, c) for t in range(3))
            assert len(b) == len(a) + run[1]["map"]["inserted"][k][c] and len(d) == len(b) + run[2]["map"]["inserted"][k][c]
            assert np.array_equal(_bits(d[:len(b)]), _bits(b)) and np.array_equal(_bits(b[:len(a)]), _bits(a))
            assert np.unique(d[:, 3] // 100000).size == 3  # (the intensity tells the frame)
            raw += 1
    assert raw >= 3


def test_shifted_case(oc, sg):
    fr, run = mc.frames("shifted", oc, sg), mc.oracle_run("shifted", oc, sg)
    assert len(run) == len(mc.SHIFT_JUMPS)
    for m in range(mc.SHIFT_WIDE_FRAMES):
        assert mc.keys_of(run[m]) > mc.K_DENSE
    cleared_frames = moved_frames = 0
    idx = np.arange(mc.NCUBE)
    ijk = np.stack([idx % mc.W, idx // mc.W % mc.H, idx // (mc.W * mc.H)], 1)
    dims = np.array([mc.W, mc.H, mc.D])
    for m, (f, r) in enumerate(zip(fr, run)):
        prev = run[m - 1] if m else None
        cube, center, n = mc.frame_cube(prev, f)
        assert n == r["mp_shifts"], (m, n, r["mp_shifts"])  # test_gpu_map's _recentre
        np.testing.assert_array_equal(r["map"]["center"], center)
        if not n:
            continue
        d = np.array(center) - prev["map"]["center"]
        before, after, ins = mc.cube_sizes(prev["map"]), mc.cube_sizes(r["map"]), r["map"]["inserted"]
        to = ijk + d
        inside = np.all((to >= 0) & (to < dims), axis=1)
        # lines cleared and wrapped: cubes that held points leave the grid, and the lines that come in
        # at the other end hold nothing but this frame's points
        cleared = int((before[:, ~inside] > 0).sum())
        fresh = ~np.all((ijk - d >= 0) & (ijk - d < dims), axis=1)
        assert np.array_equal(after[:, fresh] > 0, ins[:, fresh] > 0)
        # non-empty cubes more than two from the centre move, content unchanged
        tgt = (to[:, 0] + mc.W * to[:, 1] + mc.W * mc.H * to[:, 2])[inside]
        src = idx[inside]
        far = mc.cheb(tgt, cube) > 2
        moved = 0
        for k, kind in enumerate(KINDS):
            for s, t in zip(src[far], tgt[far]):
                if before[k][s] and not ins[k][t]:
                    assert np.array_equal(_bits(_cube(prev["map"], kind, s)), _bits(_cube(r["map"], kind, t))), (m, kind, s, t)
                    moved += 1
        print(f"shifted frame {m}: {n} shifts, centre {center}, (cube, kind) entries cleared {cleared}, moved far from the centre {moved}")
        cleared_frames += cleared > 0
        moved_frames += moved > 0
    assert cleared_frames >= 1 and moved_frames >= 1
