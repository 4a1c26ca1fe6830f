"""loam_map_score against the only other way to judge a pose guess, loam_map_localize, through the
C-ABI on one GPU.

  python tools/score_bench.py --map stream|big [--n 1,1024,65536] [--max-dist 0.5] [--out FILE]

stream: the map of the 14-sweep synthetic stream after the mapping frame of sweep 8, the sweep of
        the next mapping frame (tools/localize_bench.py's set-up)
big:    tools/localize_bench.py's uniform 1.5 M point map; same sweep

Per n: the whole-call wall time (median and range of --reps calls after a warm-up call that
allocates the working set), then one call with profiling on: the device time of the index build, the
scoring kernel and the reduction, the points and buckets the kernel read per query (counted by its
work-counting variant) and the gathered bytes / time against the measured HBM copy rate.  Then the
yardstick on the same map in the same process: loam_map_localize at n = 1024 with the default
mp_max_iter and on a context created with mp_max_iter = 1, as time per candidate.  One JSON line
per n, one for the yardstick.  Run each --map as its own process under a time limit."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
loam = importlib.import_module("loam_velodyne-1_amd")
import localize_bench as lb  # noqa: E402  (the maps, the sweep, the candidates)

CFG = lb.CFG


def timed(call, reps):
    t0 = time.perf_counter()
    res = call()  # (allocates or grows the working set)
    first = (time.perf_counter() - t0) * 1e3
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    return res, first, lb.spread(wall)


def profiled(eng, call):
    """one call with profiling on: {name: (value, launches)} of what it added"""
    eng.set_profiling(True)
    before = eng.kernel_times()
    call()
    after = eng.kernel_times()
    eng.set_profiling(False)
    return {k: (v[0] - before.get(k, (0.0, 0))[0], v[1] - before.get(k, (0.0, 0))[1]) for k, v in after.items()
            if v[1] != before.get(k, (0.0, 0))[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", choices=("stream", "big"), default="stream")
    ap.add_argument("--n", default="1,1024,65536")
    ap.add_argument("--max-dist", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    M, sw = lb.stream_map_and_sweep()
    if a.map == "big":
        M = lb.big_map(M)
    engs = {it: loam.Engine(loam.default_config(mp_max_iter=it, **CFG)) for it in (10, 1)}
    for e in engs.values():
        dropped = e.map_import(M["corner"], M["surf"], M["center"], M["surround_phase"], M["aft"], M["bef"])
    eng = engs[10]
    kept = eng.map_export()
    map_points = [int(kept["corner"].shape[0]), int(kept["surf"].shape[0])]
    queries = int(sw["corner"].shape[0] + sw["surf"].shape[0])
    lines = []
    # the sweep's map pose: loam_map_localize's refined aft of the map's own pose pair
    aft0 = eng.map_localize(sw["pose"], sw["corner"], sw["surf"], M["aft"][None, :], M["bef"][None, :])["aft"][0]
    for n in [int(v) for v in a.n.split(",")]:
        poses = lb.candidates(aft0, n)
        call = lambda: eng.map_score(sw["corner"], sw["surf"], poses, a.max_dist)
        res, first_ms, w = timed(call, a.reps)
        p = profiled(eng, call)
        ms = {k: round(p[k][0], 4) for k in ("score_index", "k_mp_map_table", "k_mp_map_pack", "k_mp_score", "k_mp_score_reduce",
                                            "map_score_h2d", "map_score_d2h") if k in p}
        cand, cells, q = (p.get(k, (0.0, 0))[0] for k in ("score_nn_candidates", "score_nn_cells", "score_queries"))
        k_ms = p.get("k_mp_score", (0.0, 0))[0]
        gathered = 16.0 * cand + 8.0 * cells  # a float4 per point read, a bucket's two starts
        build_ms = sum(p.get(k, (0.0, 0))[0] for k in ("score_index", "k_mp_map_pack", "k_mp_map_table"))
        line = dict(what="score", map=a.map, map_points=map_points, dropped=dropped, queries=queries, n=n, max_dist=a.max_dist,
                    first_call_ms=round(first_ms, 3), call_ms=w, us_per_pose=round(1e3 * w["median"] / n, 4), device_ms=ms,
                    index_build_share_of_call=round(build_ms / w["median"], 4),
                    candidates_per_query=round(cand / q, 3) if q else None, cells_per_query=round(cells / q, 3) if q else None,
                    gathered_gb_s=round(gathered / (k_ms * 1e-3) / 1e9, 1) if k_ms > 0 else None,
                    gathered_frac_hbm_copy=round(gathered / (k_ms * 1e-3) / (lb.HBM_COPY_TBS * 1e12), 4) if k_ms > 0 else None,
                    inlier_share=[round(float((res["corner_in"] + res["surf_in"]).min()) / queries, 4),
                                  round(float((res["corner_in"] + res["surf_in"]).max()) / queries, 4)])
        print(json.dumps(line), flush=True)
        lines.append(line)
    # the yardstick: loam_map_localize on the same map, 1024 candidates
    n = 1024
    aft, bef = lb.candidates(M["aft"], n), np.tile(M["bef"], (n, 1))
    poses = lb.candidates(aft0, n)
    yard = {}
    for it, e in engs.items():
        r, first_ms, w = timed(lambda: e.map_localize(sw["pose"], sw["corner"], sw["surf"], aft, bef), a.reps)
        yard[f"localize_iter{it}"] = dict(call_ms=w, us_per_candidate=round(1e3 * w["median"] / n, 4),
                                         iters_mean=round(float(r["iters"].mean()), 2))
    _, _, w = timed(lambda: eng.map_score(sw["corner"], sw["surf"], poses, a.max_dist), a.reps)
    yard["score"] = dict(call_ms=w, us_per_pose=round(1e3 * w["median"] / n, 4))
    yard["score_over_one_iteration"] = round(w["median"] / yard["localize_iter1"]["call_ms"]["median"], 4)
    yard["score_over_localize"] = round(w["median"] / yard["localize_iter10"]["call_ms"]["median"], 4)
    line = dict(what="yardstick", map=a.map, n=n, **yard)
    print(json.dumps(line), flush=True)
    lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
