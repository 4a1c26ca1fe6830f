"""The batch step ends at cur's solved pose: frame 1 maps prev into the empty store
(no FromMap gather or hash build), frame 2 stops after its L-M; no registered cloud and no map with
cur inserted are built, because no batch call returns them.

  launch composition   the per-kernel profile of one step holds exactly the launches that remain
  step after step      the un-flipped pool, the shortened event chains and the one-table reset give
                       the same bits on every consecutive step, under every way the steps overlap
  fresh batches        nothing of one step's store reaches the next step's other batch
  empty first map      a problem whose prev yields no features skips frame 2's L-M, with no stale
                       FromMap counts or hash sizes from the step before

Shapes: 6 problems (the smallest batch that takes k_mp_nnfit: above mp_small_max 4); 64 only where
the default step pipeline has to engage on its own.  Poses against the oracle within the north-star
1e-4 m / 1e-4 rad (BASELINE.json), everything else bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4
EXACT_ROWS = 1 << 30  # tuning od_moments_min above any batch: the reference's row accumulation
P6 = 6
_C = {}


def _six(sg, oc):
    """the 6 problems and their oracle poses, computed once"""
    if "six" not in _C:
        prevs, curs = sg.batch_problems(P6, base_seed=3100)
        ref = [oc.problem(p, c)[:2] for p, c in zip(prevs, curs)]
        _C["six"] = (prevs, curs, np.array([r[0] for r in ref]), np.array([r[1] for r in ref]))
    return _C["six"]


def test_launch_composition(loam, oc, sg):
    """one profiled step: no registration, one map update (prev's), one FromMap gather + hash build
    (cur's), mp_max_iter search + fit launches (cur's L-M; prev's runs none)"""
    prevs, curs, _, _ = _six(sg, oc)
    e = loam.Engine()
    e.set_profiling(True)
    e.batch_upload(prevs, curs)
    e.batch_run()
    e.batch_download()
    kt = e.kernel_times()
    e.close()
    launches = {k: v[1] for k, v in kt.items()}
    print(launches)
    assert "k_mp_register" not in launches
    for name in ("k_mp_insert", "vg_cubes", "k_mp_compact", "k_mp_gather", "k_hash_build_map"):
        assert launches.get(name) == 1, (name, launches)
    assert launches.get("k_mp_nnfit") == loam.default_config().mp_max_iter, launches


@pytest.mark.parametrize("tune", [
    {},
    {"sr_ahead": 1},
    {"step_pipe": 1},
    {"step_pipe": 1, "pipe_mp_sets": 1},
    {"graph": 1},
], ids=lambda t: ",".join(f"{k}={v}" for k, v in t.items()) or "default")
def test_step_after_step(loam, oc, sg, tune):
    """four consecutive steps of one resident batch: poses and per-problem L-M results of every step
    equal step 1's bit for bit, and step 1's poses the oracle's"""
    prevs, curs, od_o, aft_o = _six(sg, oc)
    e = loam.Engine()
    e.set_tuning(**{"od_moments_min": EXACT_ROWS, **tune})
    e.batch_upload(prevs, curs)
    first = None
    for step in range(4):
        e.batch_run()
        od, aft, _ = e.batch_download()
        info = e.batch_lm_info()
        if first is None:
            first = (od, aft, info)
            err = max(np.abs(od - od_o).max(), np.abs(aft - aft_o).max())
            print(tune, "step 1 |gpu - oracle| =", err)
            assert err <= POSE_TOL, (tune, err)
            assert info[1].min() > 0  # (every problem's frame 2 ran its L-M)
        np.testing.assert_array_equal(od, first[0], err_msg=f"{tune} step {step + 1}")
        np.testing.assert_array_equal(aft, first[1], err_msg=f"{tune} step {step + 1}")
        for a, b in zip(info, first[2]):
            np.testing.assert_array_equal(a, b, err_msg=f"{tune} step {step + 1}")
    e.close()


def test_fresh_batches(loam, sg):
    """two different 64-problem batches fed alternately through the default step pipeline: every
    step's poses equal those of a fresh context that ran only that batch"""
    P = 64
    batches = [sg.batch_problems(P, base_seed=s) for s in (3200, 4700)]

    def once(b):
        e = loam.Engine()
        e.batch_upload(*b)
        e.batch_run()
        od, aft, _ = e.batch_download()
        e.close()
        return od, aft

    want = [once(b) for b in batches]
    assert not np.array_equal(want[0][1], want[1][1])
    e = loam.Engine()
    assert e.get_tuning("step_pipe") <= P  # (the pipeline engages on its own)
    e.batch_upload(*batches[0])
    fed = [e.prepare_batch(*b) for b in batches]
    for step in range(5):
        k = step & 1
        e.batch_feed(fed[k])
        e.batch_run()
        od, aft, _ = e.batch_download()
        np.testing.assert_array_equal(od, want[k][0], err_msg=f"step {step + 1}")
        np.testing.assert_array_equal(aft, want[k][1], err_msg=f"step {step + 1}")
    e.close()


def test_empty_first_map(loam, oc, sg):
    """one problem of the six whose prev is a single return (no features: nothing seeds the odometry,
    nothing enters the map): its frame 2 finds an empty FromMap and skips the L-M as the oracle does,
    on a context whose step before left that problem a full map's FromMap counts and hash sizes"""
    prevs, curs, od_o, aft_o = _six(sg, oc)
    k = 2
    sparse = list(prevs)
    sparse[k] = prevs[k][::len(prevs[k])].copy()
    assert len(sparse[k]) == 1
    od_k, aft_k, st_k = oc.problem(sparse[k], curs[k])
    assert st_k["mp_iters"] == 0 and st_k["mp_map_points"] == 0
    e = loam.Engine()
    e.set_tuning(od_moments_min=EXACT_ROWS)
    e.batch_upload(prevs, curs)
    e.batch_run()
    e.batch_download()
    assert e.batch_lm_info()[1][k] > 0
    e.batch_upload(sparse, curs)  # (the same size: the buffers stay)
    for step in range(2):
        e.batch_run()
        od, aft, st = e.batch_download()
        od_it, mp_it, _ = e.batch_lm_info()
        assert mp_it[k] == st_k["mp_iters"] == 0, (step, od_it, mp_it)
        err = max(np.abs(od[k] - od_k).max(), np.abs(aft[k] - aft_k).max())
        print("sparse problem |gpu - oracle| =", err)
        assert err <= POSE_TOL, (step, od[k], aft[k])
        for i in range(P6):  # (the other five: as the oracle, untouched by their neighbour)
            if i != k:
                assert max(np.abs(od[i] - od_o[i]).max(), np.abs(aft[i] - aft_o[i]).max()) <= POSE_TOL, (step, i)
        assert np.all(mp_it[np.arange(P6) != k] > 0)
    e.close()
