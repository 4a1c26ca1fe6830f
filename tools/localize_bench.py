"""loam_map_localize against the only other way to do the same work, n x (loam_map_import +
loam_mapping), through the C-ABI on one GPU.

  python tools/localize_bench.py --map stream|big [--n 1,64,1024] [--out FILE]

stream: the map of the 14-sweep synthetic stream after the mapping frame of sweep 8, the sweep
        of the next mapping frame (tests/test_gpu_localize.py's set-up, from the engine's own odometry)
big:    tests/test_gpu_map.py's uniform cloud scaled to 1.5 M points, imported as a map; same sweep

Per n: the whole-call wall time (median and range of --reps calls after a warm-up call that
allocates the working set), the device time of every kernel of one call with profiling on, the
gather's bytes written / time, then the sequential yardstick on the same candidates and the
mapping frame's time alone.  One JSON line per n.  Run each --map as its own process under a time
limit."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
loam = importlib.import_module("loam_velodyne-1_amd")
sg = importlib.import_module("loam_velodyne-1_amd.synthgen")

HBM_COPY_TBS = 6.29  # measured float4 copy rate of the MI355X (the figure the gather is held against)
CFG = dict(system_delay=1)


def stream_map_and_sweep():
    """(map export after the mapping frame of sweep 8, the next mapping frame's inputs)"""
    eng = loam.Engine(loam.default_config(**CFG))
    m, M = 0, None
    for k, sw in enumerate(sg.stream_sweeps(14, 1)):
        rc, f = eng.scan_registration(sw, stamp=0.1 * k)
        if rc != 0:
            continue
        pub, pose, cl, sl, full = eng.odometry(f, stamp=0.1 * k)
        if pub != 7:
            continue
        if M is not None:
            return M, dict(pose=pose, corner=cl, surf=sl, full=full)
        eng.mapping(pose, cl, sl, full, stamp=0.1 * k)
        m += 1
        if m == 4:
            M = eng.map_export()
    raise RuntimeError("the stream ended before the frame after the map")


def big_map(M):
    """the uniform cloud of tests/test_gpu_map.py's import test at 1.5 M points, M's poses"""
    rng = np.random.default_rng(20261019)
    half = np.array([546.0, 286.0, 546.0])

    def uniform(n):
        p = np.empty((n, 4), np.float32)
        p[:, :3] = (rng.uniform(-1.0, 1.0, (n, 3)) * half).astype(np.float32)
        p[:, 3] = rng.uniform(0, 16, n).astype(np.float32)
        return p

    return dict(M, corner=uniform(388894), surf=uniform(1111106), center=np.array([10, 5, 10], np.int32))


def candidates(base, n):
    rng = np.random.default_rng(7)
    d = rng.uniform(-1.0, 1.0, (n, 6)) * np.array([np.deg2rad(4.0)] * 3 + [0.6] * 3)
    d *= ((np.arange(n) % 8 + 1) / 8.0)[:, None]
    return (np.asarray(base, np.float64)[None, :] + d).astype(np.float32)


def spread(ts):
    ts = sorted(ts)
    return dict(median=round(ts[len(ts) // 2], 4), min=round(ts[0], 4), max=round(ts[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", choices=("stream", "big"), default="stream")
    ap.add_argument("--n", default="1,64,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    M, sw = stream_map_and_sweep()
    if a.map == "big":
        M = big_map(M)
    eng = loam.Engine(loam.default_config(**CFG))
    seq = loam.Engine(loam.default_config(**CFG))

    def imp(e, aft=None):
        return e.map_import(M["corner"], M["surf"], M["center"], M["surround_phase"], M["aft"] if aft is None else aft,
                            M["bef"])

    dropped = imp(eng)
    kept = eng.map_export()
    lines = []
    for n in [int(v) for v in a.n.split(",")]:
        aft, bef = candidates(M["aft"], n), np.tile(M["bef"], (n, 1))
        call = lambda: eng.map_localize(sw["pose"], sw["corner"], sw["surf"], aft, bef)
        t0 = time.perf_counter()
        res = call()  # (allocates or grows the working set)
        first_ms = (time.perf_counter() - t0) * 1e3
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e3)
        eng.set_profiling(True)
        before = eng.kernel_times()
        call()
        after = eng.kernel_times()
        eng.set_profiling(False)
        kern = {k: round(v[0] - before.get(k, (0.0, 0))[0], 4) for k, v in after.items()
                if v[1] != before.get(k, (0.0, 0))[1]}
        from_pts = int(res["map_corner"].astype(np.int64).sum() + res["map_surf"].astype(np.int64).sum())
        g_ms = kern.get("k_mp_loc_gather", 0.0)
        # the yardstick: the same candidates one at a time (import + frame), and the frames alone
        t_seq, t_frame, aft_seq = [], [], np.empty_like(aft)
        imp(seq, aft[0])
        seq.mapping(sw["pose"], sw["corner"], sw["surf"], sw["full"])  # (warm-up)
        t_all = time.perf_counter()
        for h in range(n):
            t0 = time.perf_counter()
            imp(seq, aft[h])
            t1 = time.perf_counter()
            aft_seq[h] = seq.mapping(sw["pose"], sw["corner"], sw["surf"], sw["full"])[0]
            t2 = time.perf_counter()
            t_seq.append((t2 - t0) * 1e3)
            t_frame.append((t2 - t1) * 1e3)
        seq_total = (time.perf_counter() - t_all) * 1e3
        same = bool(np.array_equal(aft_seq.view(np.uint32), res["aft"].view(np.uint32)))
        w = spread(wall)
        line = dict(map=a.map, map_points=[int(kept["corner"].shape[0]), int(kept["surf"].shape[0])], dropped=dropped,
                    n=n, first_call_ms=round(first_ms, 3), call_ms=w, kernels_ms=kern,
                    from_points_sum=from_pts, from_points_max=int((res["map_corner"] + res["map_surf"]).max()),
                    gather_gb_s=round(from_pts * 16 / (g_ms * 1e-3) / 1e9, 1) if g_ms > 0 else None,
                    gather_frac_hbm_copy=round(from_pts * 16 / (g_ms * 1e-3) / (HBM_COPY_TBS * 1e12), 4) if g_ms > 0 else None,
                    status=np.bincount(res["status"], minlength=3).tolist(),
                    iters_mean=round(float(res["iters"].mean()), 2),
                    sequential_total_ms=round(seq_total, 3), sequential_each_ms=spread(t_seq),
                    frame_alone_ms=spread(t_frame), frames_alone_total_ms=round(float(np.sum(t_frame)), 3),
                    call_over_sequential=round(w["median"] / seq_total, 4),
                    call_over_n_frames=round(w["median"] / float(np.sum(t_frame)), 4),
                    aft_equal_sequential=same)
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
