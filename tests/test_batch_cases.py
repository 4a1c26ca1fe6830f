"""The conditions the inputs of tests/test_gpu_batch_branches.py must meet (no GPU): asserted on the
oracle alone, so that a GPU test that compares against it is not vacuous.  The bounds are what the
oracle does on the nine crops of synthgen.batch_problems(12, base_seed=9100); a
bound that fails means the fixture changed, not that the bound is too high."""
import numpy as np

import batch_cases as bc


def test_layout(sg):
    cs = bc.cases(sg)
    for name in "AB":
        bt = cs[name]
        assert len(bt.prevs) == len(bt.curs) == bc.P == 64
        assert bt.variant[0] in bc.ABNORMAL and bt.variant[-1] in bc.ABNORMAL
        assert sum(bt.fill) == 4
        assert sorted(set(bt.seed) - {bt.seed[i] for i in range(bc.P) if bt.fill[i]}) == \
            [bc.BASE_SEED + 6 * "AB".index(name) + k for k in range(6)]
        for v, _ in bc.VARIANTS:
            assert sum(1 for i in range(bc.P) if bt.variant[i] == v and not bt.fill[i]) == 6, v
        # interleaved: no whole problem beside another, the NaN-guard variant directly before one
        for i in range(bc.P):
            if bt.variant[i] == bc.WHOLE:
                assert bt.variant[i - 1] in bc.ABNORMAL and bt.variant[i + 1] in bc.ABNORMAL, i
            if bt.variant[i] == "ground_prev":
                assert bt.variant[i + 1] == bc.WHOLE and bt.seed[i + 1] == bt.seed[i]
    prevs, curs, at = bc.fill_batch(sg)
    for name in "AB":
        assert len(at[name]) == 4
        for i, j in at[name]:
            np.testing.assert_array_equal(cs[name].prevs[i], prevs[j])
            np.testing.assert_array_equal(cs[name].curs[i], curs[j])


def test_oracle_reaches_every_branch(oc, sg):
    cs = bc.cases(sg)
    total = {k: 0 for k in bc.CLASS_MIN}
    for name in "AB":
        bt = cs[name]
        od, aft, od_it, mp_it, stats = bc.oracle_batch(oc, sg, name)
        assert np.all(np.isfinite(od)) and np.all(np.isfinite(aft)), name
        cl = bc.classes(bt, stats)
        print(f"batch {name}: " + ", ".join(f"{k} {len(v)}" for k, v in cl.items()))
        for k, v in cl.items():
            assert len(v) >= 1, (name, k)
            total[k] += len(v)
        # a NaN-guard problem directly beside a whole one that the oracle solves normally
        assert any(bt.variant[i + 1] == bc.WHOLE and stats[i + 1]["od_nan_skips"] == 0
                   and stats[i + 1]["od_degenerate_steps"] == 0 for i in cl["nan_guard"]), name
        # the NaN guard leaves the odometry pose zero
        for i in cl["nan_guard"]:
            assert not od[i].any(), bt.label(i)
        # the fill problems and the seeds' whole problems are ordinary ones
        for i in range(bc.P):
            if bt.variant[i] == bc.WHOLE:
                s = stats[i]
                assert s["od_iters"] > 0 and s["mp_iters"] > 0 and s["od_nan_skips"] == 0, bt.label(i)
    for k, n in bc.CLASS_MIN.items():
        assert total[k] >= n, (k, total[k], n)


def test_oracle_is_deterministic_on_the_cases(oc, sg):
    bt = bc.cases(sg)["A"]
    od, aft, od_it, mp_it, _ = bc.oracle_batch(oc, sg, "A")
    od2, aft2, od_it2, mp_it2, _ = bc.oracle_all(oc, bt.prevs, bt.curs)
    np.testing.assert_array_equal(od, od2)
    np.testing.assert_array_equal(aft, aft2)
    np.testing.assert_array_equal(od_it, od_it2)
    np.testing.assert_array_equal(mp_it, mp_it2)


def test_long_loops_run_to_their_limits(oc, sg):
    """with od_max_iter=100, mp_max_iter=20 (test_long_loops): the NaN guard skips 100 of 100 steps,
    a degenerate odometry runs past 25 iterations, and mapping reaches 20"""
    bt = bc.cases(sg)["A"]
    _, _, od_it, mp_it, stats = bc.oracle_batch(oc, sg, "A", 100, 20)
    assert sum(1 for s in stats if s["od_nan_skips"] == s["od_iters"] == 100) >= 4
    assert sum(1 for s in stats if s["od_degenerate_steps"] == s["od_iters"] > 25) >= 1
    assert sum(1 for i, s in enumerate(stats) if bt.variant[i] == "thin4_prev" and s["od_iters"] == 100
               and s["mp_iters"] == 20) >= 1
