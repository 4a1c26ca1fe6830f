"""The VoxelGrid edge inputs (tests/vg_cases.py) have the properties the GPU tests rely on, so none
of those can pass vacuously; the reference they compare with (oracle_voxel_grid) agrees with a
float64 statement on these inputs; the diagnostic hook is exported and has no CPU path.  No GPU."""
import numpy as np
import pytest

import vg_cases as vc
import vg_hook

MERGE_TABLE = ((4000, 0), (4000, 1), (4000, 2), (4000, 1023), (4000, 1024), (4000, 1025), (3000, 8191), (3000, 8192),
               (3000, 8193), (2000, 100))
MERGE_MIN = 2500


@pytest.fixture(scope="module")
def vg(oc):
    return vc.oracle_vg(oc)


@pytest.mark.parametrize("leaf", vc.LEAVES)
def test_key_span_hits_every_bit_count(leaf):
    seen = set()
    for bits in vc.KEY_BITS:
        for n in (2, 2047, 2049, 12289):
            p = vc.key_span(n, leaf, 100 + bits, bits)
            assert not vc.leaf_too_small(p, leaf)
            assert vc.key_bits(p, leaf) == bits, (bits, n)
            seen.add(bits)
    assert seen == set(vc.KEY_BITS)


@pytest.mark.parametrize("leaf", vc.LEAVES)
def test_small_key_ranges(leaf):
    for n in (1, 2, 7, 2049, 12289):
        assert vc.key_bits(vc.one_voxel(n, leaf, 1), leaf) == 0
        key, _ = vc.seg_keys(vc.two_voxels(n, leaf, 2), leaf)
        assert set(key.tolist()) == ({0, 1} if n > 1 else {0})   # the kmax >> 1 == 0 branch
        if n > 1:
            np.testing.assert_array_equal(key, np.arange(n) % 2)


@pytest.mark.parametrize("leaf", vc.LEAVES)
def test_one_per_voxel_is_sorted_and_keeps_every_point(vg, leaf):
    for n in (1, 2, 9, 2048, 12289, 24577):
        up = vc.one_per_voxel(n, leaf, 3)
        down = vc.one_per_voxel(n, leaf, 3, descending=True)
        ku, _ = vc.seg_keys(up, leaf)
        kd, _ = vc.seg_keys(down, leaf)
        assert np.all(np.diff(ku) > 0) and np.all(np.diff(kd) < 0)
        assert len(vg(up, leaf)) == n and len(vg(down, leaf)) == n


@pytest.mark.parametrize("leaf", vc.LEAVES)
def test_uniform_density(leaf):
    # (below a few hundred points the cube is one to four voxels a side and the ratio is no average)
    for n in (2047, 2048, 2049, 12287, 12288, 12289, 16384, 24577, 30000, 40000):
        key, _ = vc.seg_keys(vc.uniform(n, leaf, 4), leaf)
        per_voxel = n / len(np.unique(key))
        assert 1.5 <= per_voxel <= 4.0, (n, per_voxel)


@pytest.mark.parametrize("leaf", vc.LEAVES)
def test_too_small_cases(vg, leaf):
    for n in (2, 2049, 12289):
        for kind in ("xy", "xyz"):
            p = vc.too_small(n, leaf, 5, kind)
            assert vc.leaf_too_small(p, leaf)
            e = vc.axis_extents(p, leaf)
            # "xyz": no two axes overflow, only all three
            assert (max(e[0] * e[1], e[0] * e[2], e[1] * e[2]) > vc.INT_MAX) == (kind == "xy")
            np.testing.assert_array_equal(vg(p, leaf).view(np.uint32), p.view(np.uint32))


@pytest.mark.parametrize("leaf", vc.LEAVES)
def test_boundary_cases_hold_what_they_name(leaf):
    p = vc.boundaries(12289, leaf, 6)
    xyz = p[:, :3]
    assert (xyz < 0).any() and np.signbit(xyz[xyz == 0]).any()
    on_face = xyz == (np.round(xyz / np.float32(leaf)) * np.float32(leaf)).astype(np.float32)
    assert on_face.mean() > 0.3
    assert len(np.unique(p, axis=0)) < len(p)


@pytest.mark.parametrize("leaf", vc.LEAVES)
def test_split_skew_classes(leaf):
    n = 40000
    b = {k: vc.split_buckets(vc.split_skew(n, leaf, 7, k), leaf) for k in vc.SKEWS}
    assert b["one_bucket"].max() == n                       # a bucket as large as its parent
    assert b["low16"][0] == n - 1 and b["low16"][15] == 1   # ... but for the point that spans the frame
    assert (b["ends"] == 0).sum() == 14 and b["ends"][0] > 0 and b["ends"][15] > 0
    assert 2049 <= b["mid"][5] <= 16384 and b["mid"].max() == b["mid"][5]
    assert b["huge"][5] > 16384
    assert all(v.sum() == n for v in b.values())
    for k in ("low16", "ends"):   # the small parents of the early split
        for m in (2049, 16385):
            v = vc.split_buckets(vc.split_skew(m, leaf, 8, k), leaf)
            assert (v == 0).sum() == 14 and v.sum() == m


def test_merge_classes(vg):
    for li, (nold, ntail) in enumerate(MERGE_TABLE):
        leaf = vc.LEAVES[li % 2]
        elig = vc.merge_eligible(nold + ntail, nold, MERGE_MIN)
        assert elig == ((nold, ntail) not in ((3000, 8193), (2000, 100)))
        for kind in vc.MERGE_TAKEN:
            p, no = vc.merge_segment(vg, nold, ntail, leaf, 9 + li, kind)
            assert no == nold and len(p) == nold + ntail
            assert vc.merge_precondition(p, leaf, nold), (nold, ntail, kind)
            key, _ = vc.seg_keys(p, leaf)
            old, tail = key[:nold], key[nold:]
            if ntail >= 8:   # the four kinds of tail point
                assert np.isin(tail, old).any() and (~np.isin(tail, old)).any()
                assert (tail < old[0]).any() and (tail > old[-1]).any()
                inside = (~np.isin(tail, old)) & (tail > old[0]) & (tail < old[-1])
                assert inside.any()
            if kind == "taken_bbox" and ntail:   # the last tail point alone moves the box: every key shifts
                k0, _ = vc.seg_keys(p[:-1], leaf)
                assert (key[:-1] != k0).all()
    for kind in vc.MERGE_FALLBACK:
        p, no = vc.merge_segment(vg, 4000, 1024, 0.2, 20, kind)
        assert vc.merge_eligible(len(p), no, MERGE_MIN)
        assert not vc.merge_precondition(p, 0.2, no), kind
    p, no = vc.merge_segment(vg, 4000, 1024, 0.2, 20, "raw_prefix")
    assert not vc.leaf_too_small(p, 0.2) and vc.seg_keys(p, 0.2)[0].max() < 1 << 24
    p, no = vc.merge_segment(vg, 4000, 1024, 0.2, 20, "key24")
    key, _ = vc.seg_keys(p, 0.2)
    assert not vc.leaf_too_small(p, 0.2) and key.max() >= 1 << 24 and np.all(np.diff(key[:no]) > 0)
    p, no = vc.merge_segment(vg, 4000, 1024, 0.2, 20, "too_small")
    assert vc.leaf_too_small(p, 0.2)


def _anchor_cases(vg):
    for leaf in vc.LEAVES:
        for n in (1, 2, 9, 2049, 12289, 20000):
            yield "uniform", vc.uniform(n, leaf, 30), leaf
            yield "one_voxel", vc.one_voxel(n, leaf, 31), leaf
            yield "ascending", vc.one_per_voxel(n, leaf, 32), leaf
            yield "descending", vc.one_per_voxel(n, leaf, 32, descending=True), leaf
            yield "two_voxels", vc.two_voxels(n, leaf, 33), leaf
            yield "boundaries", vc.boundaries(n, leaf, 34), leaf
        for bits in vc.KEY_BITS:
            yield f"span{bits}", vc.key_span(12289, leaf, 35, bits), leaf
        for kind in ("xy", "xyz"):
            yield "too_small_" + kind, vc.too_small(2049, leaf, 36, kind), leaf
        for kind in vc.SKEWS:
            yield "skew_" + kind, vc.split_skew(20000, leaf, 37, kind), leaf
        for kind in vc.MERGE_TAKEN + vc.MERGE_FALLBACK:
            yield "merge_" + kind, vc.merge_segment(vg, 4000, 1025, leaf, 38, kind)[0], leaf


def test_oracle_against_float64_statement(vg):
    """oracle_voxel_grid on the edge inputs: the voxels of the restated keys in key order, each mean
    within cnt * 2^-23 * max|v| (cnt float additions and one division, each within 2^-24 relative)
    of the float64 mean; a too-small leaf returns the input"""
    count = 0
    for name, p, leaf in _anchor_cases(vg):
        out = vg(p, leaf)
        ref = vc.f64_voxel_means(p, leaf)
        if ref is None:
            np.testing.assert_array_equal(out.view(np.uint32), p.view(np.uint32), err_msg=name)
        else:
            mean, cnt, vmax = ref
            assert len(out) == len(mean), name
            bound = cnt[:, None] * 2.0 ** -23 * vmax
            assert (np.abs(out.astype(np.float64) - mean) <= bound).all(), name
        count += 1
    assert count == 2 * (6 * 6 + len(vc.KEY_BITS) + 2 + len(vc.SKEWS) + 5)


def test_hook_symbols_exported(loam):
    lib = loam.lib()
    for n in vg_hook.NAMES:
        assert hasattr(lib, n), n
        assert n not in loam.EXPORTS


def test_hook_has_no_cpu_path(loam):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    rc, h = vg_hook.create(loam.lib(), 1000, 4)
    assert rc == loam.LOAM_E_HIP and not h
