"""Inputs of tests/test_gpu_batch_branches.py (built without a GPU; tests/test_batch_cases.py checks
on the oracle alone that they reach the branches they are meant to reach).

Two batches of exactly 64 config-4 problems (the smallest batch that takes the batch forms of the
L-M kernels), built from the raw sweeps of synthgen.batch_problems(12, base_seed=9100): each seed's
(prev, cur) whole and in nine crops that drive the reference's abnormal branches — the iteration-0
degeneracy projection (src/laserOdometry.cpp:770-797, src/laserMapping.cpp:927-954), the NaN guard
(:799-811), the Q11 window clamp (:486, :598), the L-M gate, fewer than 10 / 50 rows, loops that
never converge.  Batch A holds seeds 0..5 and four whole problems of further seeds, batch B seeds
6..11 and four more; DESIGN.md §15 lists what the oracle does on each variant."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import scenarios

BASE_SEED = 9100
N_SEEDS = 12
N_FILL = 8
P = 64
WHOLE = "whole"


def _sector(raw, deg):
    """the returns of a sweep with azimuth in [0, deg)"""
    az = np.degrees(np.arctan2(raw[:, 1], raw[:, 0])) % 360.0
    return np.ascontiguousarray(raw[az < deg])


def ground_both(prev, cur):
    return scenarios.ground_only(prev), scenarios.ground_only(cur)


def ground_both_12(prev, cur):
    return scenarios.ground_only(prev, -1.2), scenarios.ground_only(cur, -1.2)


def ground_prev(prev, cur):
    return scenarios.ground_only(prev), cur


def ground_cur(prev, cur):
    return prev, scenarios.ground_only(cur)


def sector40_prev(prev, cur):
    return _sector(prev, 40.0), cur


def sector20_prev(prev, cur):
    return _sector(prev, 20.0), cur


def thin4_prev(prev, cur):
    return np.ascontiguousarray(prev[::4]), cur


def head300_cur(prev, cur):
    return prev, np.ascontiguousarray(cur[:300])


def head3000_prev(prev, cur):
    return np.ascontiguousarray(prev[:3000]), cur


def whole(prev, cur):
    return prev, cur


# a seed's ten problems in batch order: the NaN-guard variant (ground_prev) directly before the
# whole problem, an abnormal one first and last
VARIANTS = (("ground_both", ground_both), ("ground_prev", ground_prev), (WHOLE, whole),
            ("ground_cur", ground_cur), ("sector40_prev", sector40_prev), ("thin4_prev", thin4_prev),
            ("sector20_prev", sector20_prev), ("head300_cur", head300_cur),
            ("ground_both_-1.2", ground_both_12), ("head3000_prev", head3000_prev))
ABNORMAL = tuple(n for n, _ in VARIANTS if n != WHOLE)


class Batch:
    """64 problems: prevs / curs, and per problem its variant name, its seed and whether it is one
    of the four whole problems of further seeds ("fill")"""

    def __init__(self, name):
        self.name = name
        self.prevs, self.curs, self.variant, self.seed, self.fill = [], [], [], [], []

    def add(self, pc, variant, seed, fill=False):
        self.prevs.append(pc[0])
        self.curs.append(pc[1])
        self.variant.append(variant)
        self.seed.append(seed)
        self.fill.append(fill)

    def label(self, i):
        return f"{self.name}[{i}] {self.variant[i]} seed {self.seed[i]}" + (" (fill)" if self.fill[i] else "")

    def head(self, n):
        return self.prevs[:n], self.curs[:n]


_CASES = {}
_ORACLE = {}


def cases(sg):
    """{"A": Batch, "B": Batch}: a batch is six seeds' blocks of ten (VARIANTS' order), with one fill
    problem after each of the first four blocks, so problems 0 and 63 are abnormal, every whole
    problem has abnormal neighbours and the first four problems are three abnormal ones and a whole
    one"""
    if not _CASES:
        prevs, curs = sg.batch_problems(N_SEEDS + N_FILL, base_seed=BASE_SEED)
        for b, name in enumerate("AB"):
            bt = Batch(name)
            for k in range(6):
                s = 6 * b + k
                for vname, fn in VARIANTS:
                    bt.add(fn(prevs[s], curs[s]), vname, BASE_SEED + s)
                if k < 4:
                    f = N_SEEDS + 4 * b + k
                    bt.add((prevs[f], curs[f]), WHOLE, BASE_SEED + f, fill=True)
            assert len(bt.prevs) == P
            _CASES[name] = bt
    return _CASES


def fill_batch(sg):
    """64 whole problems (seeds BASE_SEED ...) and, per batch name, where its four fill problems sit
    among them: {"A": [(index in A, index here), ...], "B": ...}"""
    if "fill" not in _CASES:
        cs = cases(sg)
        prevs, curs = sg.batch_problems(P, base_seed=BASE_SEED)
        at = {n: [(i, cs[n].seed[i] - BASE_SEED) for i in range(P) if cs[n].fill[i]] for n in "AB"}
        _CASES["fill"] = (prevs, curs, at)
    return _CASES["fill"]


def oracle_all(oc, prevs, curs, cfg=None):
    """the oracle on every problem, on a thread pool (ctypes releases the GIL; the oracle keeps no
    global state): (od [n, 6], aft [n, 6], od_iters [n], mp_iters [n], [stats dict] * n)"""
    n = min(16, os.cpu_count() or 1)
    with ThreadPoolExecutor(n) as ex:
        outs = list(ex.map(lambda pc: oc.problem(pc[0], pc[1], cfg), zip(prevs, curs)))
    od = np.array([o[0] for o in outs])
    aft = np.array([o[1] for o in outs])
    od_it = np.array([o[2]["od_iters"] for o in outs], np.int64)
    mp_it = np.array([o[2]["mp_iters"] for o in outs], np.int64)
    return od, aft, od_it, mp_it, [o[2] for o in outs]


def oracle_batch(oc, sg, name, od_max_iter=None, mp_max_iter=None):
    """oracle_all of batch `name`, run once per (batch, iteration limits) and shared: read-only"""
    key = (name, od_max_iter, mp_max_iter)
    if key not in _ORACLE:
        kw = {k: v for k, v in (("od_max_iter", od_max_iter), ("mp_max_iter", mp_max_iter)) if v is not None}
        bt = cases(sg)[name]
        out = oracle_all(oc, bt.prevs, bt.curs, oc.default_config(**kw) if kw else None)
        for a in out[:4]:
            a.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


TOTALS = ("od_degenerate_steps", "mp_degenerate_steps", "od_nan_skips", "od_rows_sum", "mp_rows_sum")


def totals(stats):
    """the batch totals of the counters batch_download returns, from the oracle's per-problem stats"""
    return {k: int(sum(s[k] for s in stats)) for k in TOTALS}


# ---------------------------------------------------------------- the classes of abnormal problem
def classes(bt, stats):
    """{class: [problem indices]} of a batch by what the oracle does on each problem (default
    iteration limits 25 / 10)"""
    c = {k: [] for k in ("nan_guard", "od_degenerate", "od_clean_mp_degenerate", "mp_degenerate", "under_gate",
                         "row_starved", "mp_never_solves", "q11_clamp", "od_early_stop")}
    for i, s in enumerate(stats):
        if s["od_nan_skips"] == s["od_iters"] == 25:
            c["nan_guard"].append(i)
        if s["od_degenerate_steps"] == s["od_iters"] > 0:
            c["od_degenerate"].append(i)
        # (a ground problem whose odometry takes 25 real steps: the NaN guard's problems, which also
        # have no degenerate step, are their own class)
        if (bt.variant[i].startswith("ground") and s["od_iters"] == 25 and s["od_degenerate_steps"] == 0
                and s["od_nan_skips"] == 0 and s["mp_degenerate_steps"] > 0):
            c["od_clean_mp_degenerate"].append(i)
        if s["mp_degenerate_steps"] == s["mp_iters"] > 0:
            c["mp_degenerate"].append(i)
        if s["od_iters"] == 0 and s["mp_iters"] == 0:
            c["under_gate"].append(i)
        if s["od_iters"] == 25 and s["od_rows_sum"] == 0:
            c["row_starved"].append(i)
        if s["mp_iters"] == 10 and s["mp_rows_sum"] < 500:
            c["mp_never_solves"].append(i)
        if 0 < s["od_corner_last"] < s["n_sharp"] and s["od_iters"] > 0:
            c["q11_clamp"].append(i)
        if 0 < s["od_iters"] < 25:
            c["od_early_stop"].append(i)
    return c


# the least number of problems of each class over A and B together (what the oracle was seen to do
# on these inputs); each batch alone holds at least one of every class
CLASS_MIN = {"nan_guard": 10, "od_degenerate": 40, "od_clean_mp_degenerate": 2, "mp_degenerate": 60,
             "under_gate": 8, "row_starved": 8, "mp_never_solves": 10, "q11_clamp": 20, "od_early_stop": 10}
