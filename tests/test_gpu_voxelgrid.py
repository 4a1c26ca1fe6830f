"""The segmented VoxelGrid cascade (csrc/vg.hip vg_run and its seven kernels) tier by tier, through
the product's own three routes (the diagnostic hook loam_dev_vg_run, csrc/dev_hooks.h), against
oracle_voxel_grid per segment: the counts and every output float bit for bit, the sentinel intact
between the segments.  The sizes are the kernels' capacity edges; tests/test_vg_cases.py shows that
the inputs (tests/vg_cases.py) have the key ranges, bucket populations and merge classes meant."""
import numpy as np
import pytest

import vg_cases as vc
import vg_hook
from vg_hook import CUBES, STACK, SURROUND

pytestmark = pytest.mark.gpu

MAX_TOTAL, MAX_SEG = 3_300_000, 8400
FEW, MANY = 2, 8   # instance counts on the two sides of the routes' P <= 4 test
MERGE_MIN = 2500


@pytest.fixture(scope="module")
def vg(oc):
    return vc.oracle_vg(oc)


@pytest.fixture(scope="module")
def hook(loam):
    h = vg_hook.Handle(loam.lib(), MAX_TOTAL, MAX_SEG)
    yield h
    h.close()


class Job:
    """segments laid out with gaps, and their reference outputs (computed once)"""

    def __init__(self, vg, segments, leaves, nolds=None):
        assert len(segments) == len(leaves)
        self.segments, self.leaves, self.nolds = segments, [float(v) for v in leaves], nolds
        packed = vc.pack_job(segments, leaves, nolds=nolds)
        self.pts, self.begin, self.end, self.leaf = packed[:4]
        self.nold = packed[4] if nolds is not None else None
        self.ref = [vg(s, l) for s, l in zip(segments, self.leaves)]
        self.longest = max(len(s) for s in segments)

    def run(self, hook, route, P, **kw):
        res = hook.run(self.pts, self.begin, self.end, self.leaf, route, P, nold=self.nold, **kw)
        self.check(res, (route, P, kw))
        return res

    def check(self, res, what):
        out, cnt, merged = res
        assert not (cnt == -1).any(), (what, np.flatnonzero(cnt == -1))
        np.testing.assert_array_equal(cnt, [len(r) for r in self.ref], err_msg=str(what))
        u = out.view(np.uint32)
        gap = np.ones(len(out), bool)
        for s, r in enumerate(self.ref):
            b = int(self.begin[s])
            gap[b:int(self.end[s])] = False
            got = u[b:b + len(r)]
            if not np.array_equal(got, r.view(np.uint32)):
                bad = np.flatnonzero((got != r.view(np.uint32)).any(1))
                raise AssertionError(f"{what}: segment {s} ({len(self.segments[s])} points, leaf {self.leaves[s]}): "
                                     f"{len(bad)} of {len(r)} outputs differ, first at {bad[0]}: "
                                     f"{out[b + bad[0]]} != {r[bad[0]]}")
        assert (u[gap] == vg_hook.SENTINEL).all(), (what, "a write outside the segments")


def shapes(n, seed):
    """distributions (a), (b), (c) both ways, (g) and (d) at one size: makers that take the leaf"""
    return [lambda l: vc.uniform(n, l, seed), lambda l: vc.one_voxel(n, l, seed + 1),
            lambda l: vc.one_per_voxel(n, l, seed + 2), lambda l: vc.one_per_voxel(n, l, seed + 2, descending=True),
            lambda l: vc.boundaries(n, l, seed + 3), lambda l: vc.two_voxels(n, l, seed + 4)]


def mixed_jobs(vg, n, seed):
    """two jobs of 8 segments (6 distributions at size n, two empty segments between them), the leaves
    0.2 / 0.4 alternating in the first and swapped in the second, as the stack and cube jobs mix them"""
    empty = np.zeros((0, 4), np.float32)
    jobs = []
    for swap in (0, 1):
        segs, leaves = [], []
        for i, mk in enumerate(shapes(n, seed)):
            leaf = vc.LEAVES[(i + swap) % 2]
            segs.append(mk(leaf))
            leaves.append(leaf)
            if i in (0, 3):
                segs.append(empty)
                leaves.append(vc.LEAVES[swap])
        jobs.append(Job(vg, segs, leaves))
    return jobs


def span_jobs(vg, n, seed):
    """distribution (e) at size n: every targeted key bit count with both leaves, 7 or 8 segments a job"""
    jobs = []
    for swap in (0, 1):
        for part in (vc.KEY_BITS[:8], vc.KEY_BITS[8:]):
            leaves = [vc.LEAVES[(i + swap) % 2] for i in range(len(part))]
            jobs.append(Job(vg, [vc.key_span(n, l, seed + b, b) for b, l in zip(part, leaves)], leaves))
    return jobs


def too_small_job(vg, n, seed):
    """distribution (f) at size n, both kinds and both leaves, beside an ordinary segment"""
    return Job(vg, [vc.too_small(n, 0.2, seed, "xy"), vc.uniform(n, 0.4, seed), vc.too_small(n, 0.4, seed, "xyz"),
                    vc.too_small(n, 0.2, seed, "xyz"), vc.too_small(n, 0.4, seed, "xy")], [0.2, 0.4, 0.4, 0.2, 0.4])


def test_hook_rejects_jobs_it_cannot_run_safely(hook):
    p = vc.uniform(100, 0.2, 1)
    ok = dict(pts=p, begin=[0, 50], end=[50, 100], leaf=[0.2, 0.4], route=CUBES, P=1)
    hook.run(**ok)
    for bad in (dict(end=[60, 100]),                 # overlapping segments
                dict(end=[50, 101]),                 # past the points
                dict(begin=[-1, 50]),
                dict(begin=[50, 0], end=[100, 50]),  # not ascending
                dict(leaf=[0.2, 0.0]), dict(leaf=[0.2, float("nan")]),
                dict(nold=[51, 0]), dict(nold=[-1, 0]),
                dict(route=3), dict(P=0), dict(vg_split=4), dict(vg_merge=2),
                dict(route=SURROUND),                # two segments
                dict(begin=np.zeros(MAX_SEG + 1, np.int32), end=np.zeros(MAX_SEG + 1, np.int32),
                     leaf=np.full(MAX_SEG + 1, 0.2)),
                dict(pts=np.zeros((MAX_TOTAL + 1, 4), np.float32))):
        with pytest.raises(RuntimeError, match="loam_dev_vg_run: -1"):
            hook.run(**dict(ok, **bad))


# ---------------------------------------------------------------- surround: one segment
SURROUND_SIZES = (1, 2, 12287, 12288, 12289, 24576, 24577, 30000)


@pytest.mark.parametrize("n", SURROUND_SIZES)
def test_surround_sizes(hook, vg, n):
    for leaf in vc.LEAVES:   # (the product's surround leaf is 0.2; the route takes the segment's)
        for mk in shapes(n, 1000 + n):
            _, _, merged = Job(vg, [mk(leaf)], [leaf]).run(hook, SURROUND, 1)
            assert (merged == -1).all()


@pytest.mark.parametrize("n", (12288, 12289))
def test_surround_key_spans_and_too_small(hook, vg, n):
    for leaf in vc.LEAVES:
        for bits in vc.KEY_BITS:
            Job(vg, [vc.key_span(n, leaf, 1100 + bits, bits)], [leaf]).run(hook, SURROUND, 1)
        for kind in ("xy", "xyz"):
            Job(vg, [vc.too_small(n, leaf, 1200, kind)], [leaf]).run(hook, SURROUND, 1)


# ---------------------------------------------------------------- cubes, merge off
@pytest.mark.parametrize("n", SURROUND_SIZES)
def test_cubes_few_instances(hook, vg, n):
    for job in mixed_jobs(vg, n, 2000 + n):
        job.run(hook, CUBES, FEW, vg_merge=0)


CUBE_BATCH_SIZES = (1, 2, 7, 8, 9, 2047, 2048, 2049, 12287, 12288, 12289, 24577)


@pytest.mark.parametrize("n", CUBE_BATCH_SIZES)
def test_cubes_batch(hook, vg, n):
    for job in mixed_jobs(vg, n, 3000 + n):
        job.run(hook, CUBES, MANY, vg_merge=0)


@pytest.mark.parametrize("P,n", [(FEW, 12288), (FEW, 12289), (MANY, 2048), (MANY, 2049), (MANY, 12288), (MANY, 12289)])
def test_cubes_key_spans(hook, vg, P, n):
    for job in span_jobs(vg, n, 3500 + n):
        job.run(hook, CUBES, P, vg_merge=0)


@pytest.mark.parametrize("P,n", [(FEW, 12288), (FEW, 12289), (MANY, 2048), (MANY, 12288), (MANY, 24577)])
def test_cubes_too_small(hook, vg, P, n):
    too_small_job(vg, n, 3600 + n).run(hook, CUBES, P, vg_merge=0)


# ---------------------------------------------------------------- cubes, merge on
MERGE_TABLE = ((4000, 0), (4000, 1), (4000, 2), (4000, 1023), (4000, 1024), (4000, 1025), (3000, 8191), (3000, 8192),
               (3000, 8193), (2000, 100))


def check_merged(job, merged, what):
    want = [int(vc.merge_eligible(len(s), no, MERGE_MIN) and vc.merge_precondition(s, l, no)) if len(s) else 0
            for s, l, no in zip(job.segments, job.leaves, job.nolds)]
    np.testing.assert_array_equal(merged, want, err_msg=str(what))
    return want


@pytest.mark.parametrize("P", (FEW, MANY))
@pytest.mark.parametrize("kind", vc.MERGE_TAKEN)
def test_cubes_merge_table(hook, vg, P, kind):
    for swap in (0, 1):
        leaves = [vc.LEAVES[(i + swap) % 2] for i in range(len(MERGE_TABLE))]
        segs = [vc.merge_segment(vg, no, nt, l, 4000 + i, kind) for i, ((no, nt), l) in enumerate(zip(MERGE_TABLE, leaves))]
        job = Job(vg, [s for s, _ in segs], leaves, nolds=[no for _, no in segs])
        _, _, merged = job.run(hook, CUBES, P, vg_merge=1, vg_merge_min=MERGE_MIN)
        want = check_merged(job, merged, (P, kind, swap))
        assert want == [1] * 8 + [0, 0]   # the tail of 8193 and the segment of 2100 points go to the cascade
        # merge off: the same output by the cascade alone
        _, _, off = job.run(hook, CUBES, P, vg_merge=0, vg_merge_min=MERGE_MIN)
        assert (off == -1).all()


@pytest.mark.parametrize("P", (FEW, MANY))
def test_cubes_merge_fallbacks(hook, vg, P):
    segs, leaves = [], []
    for i, kind in enumerate(("taken",) + vc.MERGE_FALLBACK + ("taken_bbox",)):
        for leaf in ((0.2,) if kind == "key24" else vc.LEAVES):   # (at leaf 0.4 the far point's key stays below 2^24)
            segs.append(vc.merge_segment(vg, 4000, 1025, leaf, 4100 + i, kind))
            leaves.append(leaf)
    segs.append((np.zeros((0, 4), np.float32), 0))
    leaves.append(0.2)
    job = Job(vg, [s for s, _ in segs], leaves, nolds=[no for _, no in segs])
    _, _, merged = job.run(hook, CUBES, P, vg_merge=1, vg_merge_min=MERGE_MIN)
    want = check_merged(job, merged, P)
    assert want == [1, 1, 0, 0, 0, 0, 0, 1, 1, 0]


# ---------------------------------------------------------------- stacks
def stack_variants(P, longest):
    """the tuning values and host knowledge of the stack route for this P class"""
    if P <= 4:
        tunes = [dict(vg_split=0), dict(vg_split=2), dict(vg_split=1, capS=40000), dict(vg_split=1, capS=70000)]
    else:
        tunes = [dict(vg_split=0), dict(vg_split=2), dict(vg_split=3), dict(vg_split=1, capS=40000),
                 dict(vg_split=1, capS=70000)]
    return [dict(t, stack_max=m) for t in tunes for m in (-1, longest)]


STACK_SIZES = {FEW: (12287, 12288, 12289, 20000, 40000), MANY: (2047, 2048, 2049, 16383, 16384, 16385, 40000)}
STACK_EDGES = {FEW: (12288, 12289), MANY: (2048, 2049, 16384, 16385)}


@pytest.mark.parametrize("P,n", [(P, n) for P in (FEW, MANY) for n in STACK_SIZES[P]])
def test_stack_sizes(hook, vg, P, n):
    for job in mixed_jobs(vg, n, 5000 + n):
        for kw in stack_variants(P, job.longest):
            job.run(hook, STACK, P, **kw)


@pytest.mark.parametrize("P,n", [(P, n) for P in (FEW, MANY) for n in STACK_EDGES[P]])
def test_stack_key_spans(hook, vg, P, n):
    for job in span_jobs(vg, n, 5500 + n):
        for kw in stack_variants(P, job.longest):
            job.run(hook, STACK, P, **kw)


@pytest.mark.parametrize("P,n", [(FEW, 40000), (MANY, 2049), (MANY, 16385), (MANY, 40000)])
def test_stack_split_skew(hook, vg, P, n):
    kinds = [k for k in vc.SKEWS if n >= 40000 or k not in ("mid", "huge")]
    for swap in (0, 1):
        leaves = [vc.LEAVES[(i + swap) % 2] for i in range(len(kinds))]
        job = Job(vg, [vc.split_skew(n, l, 5600 + i, k) for i, (k, l) in enumerate(zip(kinds, leaves))], leaves)
        for kw in stack_variants(P, job.longest):
            job.run(hook, STACK, P, **kw)


@pytest.mark.parametrize("P,n", [(FEW, 12288), (FEW, 12289), (FEW, 40000), (MANY, 2048), (MANY, 2049), (MANY, 16385),
                                 (MANY, 40000)])
def test_stack_too_small(hook, vg, P, n):
    job = too_small_job(vg, n, 5700 + n)
    for kw in stack_variants(P, job.longest):
        job.run(hook, STACK, P, **kw)


# ---------------------------------------------------------------- a workgroup's second segment
def stride_job(vg, nseg, lo, hi, seed):
    """nseg segments of lo..hi points: uniform, single-voxel, a 17-bit key span and two-voxel content in
    turn, so that what one segment leaves in LDS differs from what the next needs"""
    rng = np.random.default_rng(seed)
    segs, leaves = [], []
    for s in range(nseg):
        n, leaf = int(rng.integers(lo, hi + 1)), vc.LEAVES[(s // 4) % 2]
        segs.append((vc.uniform, vc.one_voxel, lambda n, l, sd: vc.key_span(n, l, sd, 17), vc.two_voxels)[s % 4](n, leaf, seed + s))
        leaves.append(leaf)
    return Job(vg, segs, leaves)


@pytest.mark.parametrize("P", (FEW, MANY))
def test_second_segment_first_kernel(hook, vg, P):
    # the first kernel walks the cube route's input list with at most 8192 workgroups (k_vg_radix<1024, 12>
    # for a few instances, k_vg_radix<256, 8> for batches): 8300 small segments, some at its capacity,
    # a few beyond it
    rng = np.random.default_rng(5900 + P)
    cap = 12288 if P <= 4 else 2048
    sizes = rng.integers(1, 200, 8300)
    sizes[rng.permutation(8300)[:24]] = np.repeat([cap - 1, cap, cap + 1], 8)
    makers = (vc.uniform, vc.one_voxel, lambda n, l, sd: vc.key_span(n, l, sd, 13), vc.two_voxels, vc.boundaries)
    leaves = [vc.LEAVES[(s // 5) % 2] for s in range(8300)]
    job = Job(vg, [makers[s % 5](int(n), l, 5900 + s) for s, (n, l) in enumerate(zip(sizes, leaves))], leaves)
    job.run(hook, CUBES, P, vg_merge=0)


def test_second_segment_big(hook, vg):
    # k_vg_big's grid is 256 workgroups: 260 segments beyond the 12288-point kernel
    stride_job(vg, 260, 12289, 12300, 6000).run(hook, CUBES, FEW, vg_merge=0)


def test_second_segment_second_tier(hook, vg):
    # the second tier's grid is 1024 workgroups: k_vg_radix<1024, 12> on the cube route, k_vg_idx on the stack route
    job = stride_job(vg, 1030, 2049, 2060, 6100)
    job.run(hook, CUBES, MANY, vg_merge=0)
    job.run(hook, STACK, MANY, vg_split=0)


def test_second_segment_split_join(hook, vg):
    # k_vg_split / k_vg_join run 256 workgroups: 260 parents beyond the first kernel, split early
    stride_job(vg, 260, 2049, 2100, 6200).run(hook, STACK, MANY, vg_split=3)


def test_second_segment_merge(hook, vg):
    # k_vg_merge's grid is 32 workgroups: 40 eligible segments
    rng = np.random.default_rng(6300)
    leaves = [vc.LEAVES[s % 2] for s in range(40)]
    segs = [vc.merge_segment(vg, int(rng.integers(2600, 2700)), int(rng.integers(300, 500)), l, 6300 + s,
                             vc.MERGE_TAKEN[(s // 2) % 2]) for s, l in enumerate(leaves)]
    job = Job(vg, [s for s, _ in segs], leaves, nolds=[no for _, no in segs])
    _, _, merged = job.run(hook, CUBES, MANY, vg_merge=1, vg_merge_min=MERGE_MIN)
    assert check_merged(job, merged, "grid") == [1] * 40


# ---------------------------------------------------------------- scratch reuse, determinism
def test_scratch_reuse_and_determinism(hook, vg):
    """consecutive jobs on one handle share the sort arrays, lists and split buffers, as consecutive
    frames do: a job through the split and k_vg_big (a bucket of 20000 points), a job of tiny segments,
    the first again; each compared with the reference, the two runs of the first with each other"""
    big = Job(vg, [vc.split_skew(40000, 0.2, 7000, "huge"), vc.uniform(40000, 0.4, 7001),
                   vc.split_skew(30000, 0.4, 7002, "ends"), vc.boundaries(13000, 0.2, 7003)], [0.2, 0.4, 0.4, 0.2])
    assert vc.split_buckets(big.segments[0], 0.2).max() > 16384
    tiny = Job(vg, [mk(vc.LEAVES[i % 2]) for i, mk in enumerate(shapes(9, 7100) + shapes(1, 7200))],
               [vc.LEAVES[i % 2] for i in range(12)])
    kw = dict(vg_split=2, stack_max=-1)
    out1, cnt1, _ = big.run(hook, STACK, FEW, **kw)
    tiny.run(hook, STACK, FEW, **kw)
    tiny.run(hook, CUBES, MANY, vg_merge=0)
    out2, cnt2, _ = big.run(hook, STACK, FEW, **kw)
    np.testing.assert_array_equal(cnt1, cnt2)
    for s in range(len(cnt1)):
        b = int(big.begin[s])
        np.testing.assert_array_equal(out1[b:b + cnt1[s]].view(np.uint32), out2[b:b + cnt2[s]].view(np.uint32))
