"""The batch forms of the L-M kernels (P >= 64: k_od_sel + k_od_assoc<., false>, k_od_sel_nn,
k_od_rows<true / false> + k_od_step, k_od_rows_mom<true / false>, k_mp_nnfit<true / false> +
k_mp_iter) on abnormal problems, against the oracle.

tests/batch_cases.py builds two batches of exactly 64 problems (od_small_max is 63; od_sel_min,
od_moments_min and step_pipe are 64) in which whole problems sit between crops of raw sweeps that
drive the reference's abnormal branches; tests/test_batch_cases.py asserts on the oracle alone that
they are reached:
  * the iteration-0 degeneracy projection (src/laserOdometry.cpp:770-797, src/laserMapping.cpp:927-954)
    in odometry, in mapping, in both, and in mapping after an odometry that never was degenerate;
  * the NaN guard (:799-811) on every one of the 25 (or 100) iterations.  In ground_prev the NaN is
    the plane normalisation `pa /= ps` (:666-670) with ps = sqrt(pa² + pb² + pc²) = 0: a ground-only
    sweep's SurfLast holds one point twice (same coordinates, same ring), so for the flat queries
    whose closest point it is the second plane point (minPointInd2, the nearest on the same or a
    lower ring) is its copy, (t2 - t1) x (t3 - t1) is exactly zero and pa, pb, pc, pd2 are 0 / 0.
    NaN passes `s > 0.1 && pd2 != 0` while s = 1 (iterations 0..4); from iteration 5 on s is NaN and
    the row is rejected, but the rows stored by then are re-evaluated on every later iteration (Q12),
    so matAtA is NaN and matX is skipped to the end;
  * the Q11 window clamp (:486, :598), the L-M gate (:465), fewer than 10 rows on every odometry
    iteration (no step is ever taken), fewer than 50 on every mapping iteration, loops that stop
    early and loops that run to their limit.
The kernels under test share per-batch buffers (the partial sums under `part`, the per-problem
stop / degenerate / NaN-skip state) and let a problem's last workgroup sum the partials and run
the step: a problem's NaN, stop flag or projection must not reach its neighbours, and must not
survive into the next run on the same context."""
import numpy as np
import pytest

import batch_cases as bc
import test_gpu_moments as tm

pytestmark = pytest.mark.gpu

EXACT_ROWS = 1 << 30  # tuning od_moments_min: no batch size keeps the odometry rows as moments
TOL, ATTRIB = tm.TOL, tm.ATTRIB
_CACHE = {}


def _download(e):
    od, aft, st = e.batch_download()
    od_it, mp_it, tr = e.batch_lm_info()
    return {"od": od, "aft": aft, "st": st, "od_it": od_it.astype(np.int64), "mp_it": mp_it.astype(np.int64), "tr": tr}


def _run(loam, prevs, curs, cfg=None, runs=1, **tune):
    e = loam.Engine(cfg) if cfg is not None else loam.Engine()
    e.set_tuning(**tune)
    e.batch_upload(prevs, curs)
    out = []
    for _ in range(runs):
        e.batch_run()
        out.append(_download(e))
    e.close()
    return out


def _same(r, ref, what, rows=slice(None), totals=True):
    np.testing.assert_array_equal(r["od"], ref["od"][rows], err_msg=f"{what}: odometry pose")
    np.testing.assert_array_equal(r["aft"], ref["aft"][rows], err_msg=f"{what}: mapping pose")
    np.testing.assert_array_equal(r["od_it"], ref["od_it"][rows], err_msg=f"{what}: odometry iterations")
    np.testing.assert_array_equal(r["mp_it"], ref["mp_it"][rows], err_msg=f"{what}: mapping iterations")
    if totals:
        for k in bc.TOTALS:
            assert r["st"][k] == ref["st"][k], (what, k, r["st"][k], ref["st"][k])


def _against_oracle(r, oracle, what):
    od_o, aft_o, od_it_o, mp_it_o, stats = oracle
    np.testing.assert_array_equal(r["od"], od_o, err_msg=f"{what}: odometry pose")
    np.testing.assert_array_equal(r["aft"], aft_o, err_msg=f"{what}: mapping pose")
    np.testing.assert_array_equal(r["od_it"], od_it_o, err_msg=f"{what}: odometry iterations")
    np.testing.assert_array_equal(r["mp_it"], mp_it_o, err_msg=f"{what}: mapping iterations")
    for k, v in bc.totals(stats).items():
        assert r["st"][k] == v, (what, k, r["st"][k], v)


def _exact(loam, oc, sg, name):
    """(a)'s two runs of batch `name` on one context, checked against the oracle, shared"""
    if name not in _CACHE:
        bt = bc.cases(sg)[name]
        oracle = bc.oracle_batch(oc, sg, name)
        runs = _run(loam, bt.prevs, bt.curs, runs=2, od_moments_min=EXACT_ROWS)
        _against_oracle(runs[0], oracle, f"batch {name}")
        # the same context again: no stop, degenerate or NaN-skip state left from the first run
        _against_oracle(runs[1], oracle, f"batch {name}, second run")
        _CACHE[name] = runs[0]
    return _CACHE[name]


@pytest.mark.parametrize("name", ["A", "B"])
def test_exact_rows(loam, oc, sg, name):
    """(a) the reference's row re-evaluation at the default launch shapes of P = 64: poses bit-equal
    to the oracle on all 64 problems, per-problem iteration counts equal, the five counter totals
    equal the oracle's sums; and the same on a second run of the same context"""
    _exact(loam, oc, sg, name)


LAUNCH_FORMS = [
    ({"od_fused_max": 0}, 1),                        # k_od_rows<false> + k_od_step
    ({"mp_fused_max": 0}, 1),                        # k_mp_nnfit<false> + k_mp_iter
    ({"od_nn_lane_min": 1, "od_nn_lane": 2}, 1),     # k_od_sel_nn on tiny and sector Last clouds, every round
    ({"od_nn_lane_min": 1, "od_nn_lane": 1}, 1),     # ... the seeded rounds
    ({"od_sel_min": 1024}, 1),                       # TransformToStart inside the association wave
    ({"od_assoc_wg": 16}, 1),                        # fewer association waves per problem (queries looped)
    ({"fit_wg": 7}, 1),                              # fewer k_mp_nnfit workgroups per problem
    ({"od_win_mono": 0}, 1),                         # the ring windows by the walks
    ({"graph": 1}, 2),                               # the step captured as a HIP graph, then replayed
    ({"step_pipe": 0, "sr_ahead": 0}, 1),            # sequential steps
    ({}, 3),                                         # the default step pipeline for three steps
]


@pytest.mark.parametrize("tune,runs", LAUNCH_FORMS,
                         ids=lambda v: (",".join(f"{k}={x}" for k, x in v.items()) or "default") if isinstance(v, dict)
                         else f"{v}runs")
def test_launch_forms(loam, oc, sg, tune, runs):
    """(b) every launch form a batch of 64 can take, on batch A: bit-equal to (a) in poses,
    per-problem iteration counts and the five totals, on every run"""
    ref = _exact(loam, oc, sg, "A")
    bt = bc.cases(sg)["A"]
    for n, r in enumerate(_run(loam, bt.prevs, bt.curs, runs=runs, **{"od_moments_min": EXACT_ROWS, **tune})):
        _same(r, ref, f"{tune} run {n}")


@pytest.mark.parametrize("P", [63, 4])
def test_batch_size_independence(loam, oc, sg, P):
    """(c) batch A's first 63 and first 4 problems as their own batches (k_od_rows_small with
    k_od_assoc<., true>, k_mp_nnfit / k_mp_lm_small): the rows of (a) bit for bit"""
    ref = _exact(loam, oc, sg, "A")
    prevs, curs = bc.cases(sg)["A"].head(P)
    (r,) = _run(loam, prevs, curs)
    _same(r, ref, f"P={P}", rows=slice(0, P), totals=False)
    _, _, _, _, stats = bc.oracle_batch(oc, sg, "A")
    for k, v in bc.totals(stats[:P]).items():
        assert r["st"][k] == v, (P, k, r["st"][k], v)


def test_long_loops(loam, oc, sg):
    """(d) od_max_iter = 100, mp_max_iter = 20 on batch A, exact rows: the NaN guard 100 times, the
    Q12 rows of 100 iterations stored and re-evaluated, mapping to 20 iterations"""
    bt = bc.cases(sg)["A"]
    oracle = bc.oracle_batch(oc, sg, "A", 100, 20)
    assert oracle[2].max() == 100 and oracle[3].max() == 20
    cfg = loam.default_config(od_max_iter=100, mp_max_iter=20)
    (r,) = _run(loam, bt.prevs, bt.curs, cfg, od_moments_min=EXACT_ROWS)
    _against_oracle(r, oracle, "long loops")


def _whole64(loam, sg):
    if "whole64" not in _CACHE:
        prevs, curs, _ = bc.fill_batch(sg)
        (_CACHE["whole64"],) = _run(loam, prevs, curs)
    return _CACHE["whole64"]


@pytest.mark.parametrize("name", ["A", "B"])
def test_moments(loam, oc, sg, name):
    """(e) the per-query fp64 moments, the default at P = 64 (k_od_rows_mom<true>; with
    od_fused_max = 0 k_od_rows_mom<false> + k_od_step, the same bits).  Every problem within the
    north star's 1e-4 of the oracle; a problem whose every step the NaN guard skips has the oracle's
    odometry pose bit for bit, a problem under the L-M gate both poses; the NaN-skip and row totals
    equal the oracle's (a rejected row is not counted, a NaN row is); the whole problems follow
    tests/test_gpu_moments.py's attribution rule and do not depend on their neighbours (bit-equal
    to the same problems inside a batch of 64 whole ones).  Measured maxima per variant:
    DESIGN.md §15."""
    bt = bc.cases(sg)[name]
    od_o, aft_o, od_it_o, mp_it_o, stats = bc.oracle_batch(oc, sg, name)
    (r,) = _run(loam, bt.prevs, bt.curs)
    (r2,) = _run(loam, bt.prevs, bt.curs, od_fused_max=0)
    _same(r2, r, "k_od_rows_mom<false> + k_od_step against the fused step")

    e_od = np.abs(r["od"] - od_o).max(axis=1)
    e_mp = np.abs(r["aft"] - aft_o).max(axis=1)
    err = np.maximum(e_od, e_mp)
    abn = np.array([v != bc.WHOLE for v in bt.variant])
    edges = [0.0, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, TOL, np.inf]
    hist = {"== 0": int(np.sum(err[abn] == 0))}
    for lo, hi in zip(edges[:-1], edges[1:]):
        hist[f"<= {hi:.0e}"] = int(np.sum((err[abn] > lo) & (err[abn] <= hi)))
    print(f"moments, batch {name}: {int(abn.sum())} abnormal problems, max |d odometry| {e_od[abn].max():.3g}, "
          f"max |d mapping| {e_mp[abn].max():.3g}; error histogram {hist}")
    for v in bc.ABNORMAL:
        m = np.array([x == v for x in bt.variant])
        print(f"  {v}: max |d odometry| {e_od[m].max():.3g}, max |d mapping| {e_mp[m].max():.3g}, "
              f"iteration flips odometry {int(np.sum(r['od_it'][m] != od_it_o[m]))} "
              f"mapping {int(np.sum(r['mp_it'][m] != mp_it_o[m]))}")
    for i in np.flatnonzero(abn & (err > ATTRIB)):
        s = stats[i]
        print(f"  {bt.label(i)}: |d odometry| {e_od[i]:.3g} |d mapping| {e_mp[i]:.3g}; odometry iterations "
              f"{r['od_it'][i]} (oracle {od_it_o[i]}), mapping {r['mp_it'][i]} (oracle {mp_it_o[i]}); oracle "
              f"degenerate steps {s['od_degenerate_steps']} / {s['mp_degenerate_steps']}, NaN skips "
              f"{s['od_nan_skips']}, rows {s['od_rows_sum']} / {s['mp_rows_sum']}")
    assert err.max() <= TOL, bt.label(int(np.argmax(err)))

    cl = bc.classes(bt, stats)
    skipped = [i for i, s in enumerate(stats) if s["od_iters"] > 0 and s["od_nan_skips"] == s["od_iters"]]
    assert len(skipped) >= len(cl["nan_guard"]) >= 1
    for i in skipped:  # no step is ever applied
        np.testing.assert_array_equal(r["od"][i], od_o[i], err_msg=bt.label(i))
        assert r["od_it"][i] == od_it_o[i], bt.label(i)
    for i in cl["under_gate"]:
        np.testing.assert_array_equal(r["od"][i], od_o[i], err_msg=bt.label(i))
        np.testing.assert_array_equal(r["aft"][i], aft_o[i], err_msg=bt.label(i))
        assert r["od_it"][i] == 0 and r["mp_it"][i] == 0, bt.label(i)
    want = bc.totals(stats)
    for k in ("od_nan_skips", "od_rows_sum"):
        assert r["st"][k] == want[k], (k, r["st"][k], want[k])

    # the whole problems: test_gpu_moments' rule (an error above ATTRIB comes with a convergence
    # flip or is the reference's own mapping for the engine's odometry result)
    w = np.flatnonzero(~abn)
    print(f"  whole problems {[bt.label(i) for i in w]}:")
    tm.attribute(oc, [bt.prevs[i] for i in w], [bt.curs[i] for i in w], None,
                 (r["od"][w], r["aft"][w], r["st"], r["od_it"][w], r["mp_it"][w], r["tr"][w]),
                 (od_o[w], aft_o[w], od_it_o[w], mp_it_o[w]))
    # ... and per-problem sums that do not depend on the neighbours
    ref = _whole64(loam, sg)
    _, _, at = bc.fill_batch(sg)
    for i, j in at[name]:
        np.testing.assert_array_equal(r["od"][i], ref["od"][j], err_msg=bt.label(i))
        np.testing.assert_array_equal(r["aft"][i], ref["aft"][j], err_msg=bt.label(i))
        assert r["od_it"][i] == ref["od_it"][j] and r["mp_it"][i] == ref["mp_it"][j], bt.label(i)
