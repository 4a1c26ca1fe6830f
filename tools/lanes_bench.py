"""loam_lanes_* against the only other way to advance many sequences, one context per sequence
stepped by loam_chain_sweep from one thread, through the C-ABI on one GPU.

  python tools/lanes_bench.py [--s 1,16,64] [--sweeps 27] [--map-cap 131072] [--yard-max 1024]
                              [--profile-s 64] [--imu] [--out FILE]

Per S: S lanes over eight distinct VLP-16 synthetic streams laid out cyclically.  The wall time of
lanes_step (push + pull), and of the push alone (host packing + enqueue), median and range over the
steps after a warm-up of four, mapping steps and the others separately (skip_frame_num = 1: they
alternate).  Then the yardstick on the same streams in the same process: min(S, --yard-max)
contexts with the lanes' map capacity, each stepped by chain_sweep in turn; with fewer contexts
than lanes the time is scaled by S / contexts and the line says so.  The last od_sum / aft of lane 0
are compared with its yardstick context bit for bit.  --profile-s: one more run at that S with
loam_set_profiling on, the device time per kernel and step.  --imu: every lane is also fed
synthgen.imu_stream of its stream (100 Hz, the messages up to each sweep's end before the sweep)
through loam_lanes_imu, and the yardstick contexts get the same messages through loam_imu before
their chain_sweep; the time of those calls is reported on its own (imu_feed_ms, per
step) and is not part of the step times on either side.  One JSON line per S.  Run under a time
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

N_STREAMS = 8
WARM = 4  # steps after the init frame left out of the medians


def spread(ts):
    ts = sorted(ts)
    if not ts:
        return None
    return dict(median=round(ts[len(ts) // 2], 4), min=round(ts[0], 4), max=round(ts[-1], 4), n=len(ts))


def imu_schedules(K):
    """per stream, per sweep k: the messages with stamp <= 0.1 (k + 1) not delivered before"""
    out = []
    for i in range(N_STREAMS):
        imus, j, sched = sg.imu_stream(-0.5, 0.1 * K + 0.1, seed=1 + i), 0, []
        for k in range(K):
            due = []
            while j < len(imus) and imus[j][0] <= 0.1 * (k + 1):
                due.append(imus[j])
                j += 1
            sched.append(due)
        out.append(sched)
    return out


def run_lanes(S, streams, K, map_cap, profile=False, imu=None):
    eng = loam.Engine(loam.default_config(system_delay=1))
    t0 = time.perf_counter()
    eng.lanes_open(S, map_cap)
    open_ms = (time.perf_counter() - t0) * 1e3
    step = {0: [], 1: []}
    push = {0: [], 1: []}
    last = None
    n_prof = [0, 0]
    feed = []
    for k in range(K):
        raws = [streams[l % N_STREAMS][k] for l in range(S)]
        if profile and k == 2 + WARM:
            eng.set_profiling(True)
        if imu:
            t0 = time.perf_counter()
            for l in range(S):
                for m in imu[l % N_STREAMS][k]:
                    eng.lanes_imu(l, *m)
            feed.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        eng.lanes_push(raws, stamp=0.1 * k)
        t1 = time.perf_counter()
        o = eng.lanes_pull()
        t2 = time.perf_counter()
        if k >= 2 and not np.all(o["status"] == 0):
            raise RuntimeError(f"step {k}: lane status {np.unique(o['status'])}")
        if k >= 2 + WARM:
            m = int(o["mapped"][0])
            step[m].append((t2 - t0) * 1e3)
            push[m].append((t1 - t0) * 1e3)
            n_prof[m] += 1
        last = o
    kern = None
    if profile:
        n = n_prof[0] + n_prof[1]
        kern = {k: round(v[0] / n, 4) for k, v in sorted(eng.kernel_times().items(), key=lambda kv: -kv[1][0])}
        eng.set_profiling(False)
    trans = eng.lanes_imu_trans() if imu else None
    eng.lanes_close()
    eng.close()
    res = dict(open_ms=round(open_ms, 1), step_mapped_ms=spread(step[1]), step_unmapped_ms=spread(step[0]),
               push_mapped_ms=spread(push[1]), push_unmapped_ms=spread(push[0]))
    if imu:
        res["imu_feed_ms"] = spread(feed[2 + WARM:])
        res["imu_trans_nonzero_lanes"] = int(np.count_nonzero(np.any(trans != 0, axis=1)))
    return res, last, kern, n_prof


def run_yardstick(n, streams, K, map_cap, imu=None):
    engs = []
    t0 = time.perf_counter()
    for _ in range(n):
        e = loam.Engine(loam.default_config(system_delay=1, map_capacity=map_cap))
        e.set_tuning(batch_streams=0)  # (a context that runs no batch keeps two streams)
        engs.append(e)
    create_ms = (time.perf_counter() - t0) * 1e3
    step = {0: [], 1: []}
    last = None
    feed = []
    for k in range(K):
        if imu:
            t0 = time.perf_counter()
            for l, e in enumerate(engs):
                for m in imu[l % N_STREAMS][k]:
                    e.imu(*m)
            feed.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        for l, e in enumerate(engs):
            r = e.chain_sweep(streams[l % N_STREAMS][k], stamp=0.1 * k)
            if l == 0:
                last = r
        t1 = time.perf_counter()
        if k >= 2 + WARM:
            step[1 if last[3] is not None else 0].append((t1 - t0) * 1e3)
    for e in engs:
        e.close()
    res = dict(create_ms=round(create_ms, 1), step_mapped_ms=spread(step[1]), step_unmapped_ms=spread(step[0]))
    if imu:
        res["imu_feed_ms"] = spread(feed[2 + WARM:])
    return res, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", default="1,16,64")
    ap.add_argument("--sweeps", type=int, default=27)
    ap.add_argument("--map-cap", type=int, default=1 << 17)
    ap.add_argument("--yard-max", type=int, default=1024)
    ap.add_argument("--profile-s", type=int, default=0)
    ap.add_argument("--imu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    K = a.sweeps
    streams = [sg.stream_sweeps(K, 1 + i) for i in range(N_STREAMS)]
    imu = imu_schedules(K) if a.imu else None
    pts = int(np.mean([sw.shape[0] for sw in streams[0]]))
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                for ln in lines:
                    f.write(json.dumps(ln) + "\n")

    for S in [int(v) for v in a.s.split(",") if v]:
        res, last, _, _ = run_lanes(S, streams, K, a.map_cap, imu=imu)
        ny = min(S, a.yard_max)
        yard, ylast = run_yardstick(ny, streams, K, a.map_cap, imu=imu)
        scale = S / ny
        line = dict(S=S, imu=bool(a.imu), sweeps=K, points_per_sweep=pts, map_cap=a.map_cap, lanes=res, yardstick_contexts=ny,
                    yardstick_scaled=ny != S, yardstick=yard)
        for kind in ("mapped", "unmapped"):
            lm, ym = res[f"step_{kind}_ms"], yard[f"step_{kind}_ms"]
            if lm and ym:
                line[f"yardstick_over_lanes_{kind}"] = round(ym["median"] * scale / lm["median"], 3)
                line[f"lanes_sweeps_per_s_{kind}"] = round(S / lm["median"] * 1e3, 1)
        same = ylast[3] is not None and \
            np.array_equal(last["aft"][0].view(np.uint32), np.asarray(ylast[3], np.float32).view(np.uint32))
        line["lane0_equals_context"] = bool(np.array_equal(last["od_sum"][0].view(np.uint32),
                                                           np.asarray(ylast[2], np.float32).view(np.uint32))
                                            and (same or ylast[3] is None))
        emit(line)
    if a.profile_s:
        res, _, kern, n_prof = run_lanes(a.profile_s, streams, K, a.map_cap, profile=True, imu=imu)
        total = round(sum(kern.values()), 4)
        emit(dict(profile_S=a.profile_s, imu=bool(a.imu), steps=n_prof[0] + n_prof[1], mapped_steps=n_prof[1],
                  device_ms_per_step=kern, device_ms_per_step_total=total,
                  h2d_and_packing_share=round(kern.get("lanes_h2d", 0.0) / total, 4) if total else None,
                  step_ms_profiled=res))


if __name__ == "__main__":
    main()
