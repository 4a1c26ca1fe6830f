"""loam_lanes_* against the only other way to advance many sequences, one context per sequence
stepped by loam_chain_sweep from one thread, through the C-ABI on one GPU.

  python tools/lanes_bench.py [--s 1,16,64] [--sweeps 27] [--map-cap 131072] [--yard-max 1024]
                              [--profile-s 64] [--imu] [--restart K,M] [--occupancy N] [--map-import N]
                              [--surround] [--shared stream|big [--from-cap F]]
                              [--score stream|big [--k K1,K2]] [--localize stream|big [--k K1,K2]]
                              [--commit stream|big] [--feed device [--pairs 3]] [--out FILE]

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
limit.

--feed device (instead of the above): per S, the same steps fed from host memory
(loam_lanes_push) and from device memory (loam_lanes_push_device; the sweeps uploaded once per stream
into hipMalloc'd buffers before timing), --pairs times alternating in one process, the host feed
first: step and push times as above for each feed, the ratios of the medians, whether the device
feed's last pull equals the host feed's bit for bit, and the device feed once more with every sweep
in one allocation, whose push needs one pointer query instead of one per lane (pointer_queries_ms =
the difference of the two pushes).  --profile-s: one profiled run of each feed (the lanes_h2d /
k_lanes_gather_dev marks).

--restart K,M (instead of the above): per S, one lanes run of --sweeps steps whose
first half has no restart and whose second half restarts K lanes (K = 0: S / 4) before every M-th
step through loam_lanes_restart: the wall time of lanes_step in both halves (mapping steps and the
others apart), of the restart calls per event, and the parent's only alternative measured in the
same process, loam_lanes_close + loam_lanes_open; then the same run once more with
loam_set_profiling on in the second half for k_lanes_restart's and k_lanes_init's device time per
launch (the profiled run's wall times are not reported: the events cost time).
A restarted lane goes on with its stream's next sweeps (as a fresh sequence).

--occupancy N (instead of the above): a directory of N synthetic recordings of 10..40 sweeps over
S = 16 lanes, (a) recycled: a lane whose recording has ended is restarted onto the next one, (b)
retired and left dead: waves of 16 recordings, each wave a loam_lanes_open ... loam_lanes_close that
lasts as long as its longest recording.  Total sweeps per second both ways, open / close included.

--map-import N (instead of the above): per S and for two maps (the map a context
builds over stream 1 in --sweeps sweeps, and N synthetic points inside the grid, half corner half
surf), in one process: the wall time of one loam_lanes_map_import into all S lanes and into lane 0
alone, of loam_map_import into one streaming context, and of the parent's only way to give S
sequences the map, min(S, --yard-max) contexts (made as the yardstick's) each receiving
loam_map_import (scaled by S / contexts when fewer).  Every figure is a median with its range over
seven calls after two warm-up calls; the sides alternate call by call.  Then the same calls under
loam_set_profiling for the device time per launch of every import kernel, k_lanes_map_install's
bytes written (n kept 16 + n 4851 16) over its device time, and a hipMemcpyDtoD of as many bytes
timed with events in the same process (median of seven after two warm-up copies).

--surround (instead of the above): per S, S lanes over 23 sweeps (system_delay = 1:
sweep 22 is the 11th mapping frame, on which every lane publishes /laser_cloud_surround), then the
wall time of one loam_lanes_surround call with room for every lane's cloud, the median and range of
seven calls after two warm-up calls.  The baseline in the same process: min(S, --yard-max) streaming
contexts that hold the same maps and are due on the same frame (each was fed its lane's sweeps
through loam_chain_sweep for the odometry's state, received loam_map_import of its lane's export in
front of the last sweep and then ran that one mapping frame), each calling loam_mapping_surround
one after the other into its own preallocated array, timed the same way, the sides alternating call
by call.  Both sides go through ctypes with nothing allocated
inside the timed region.  Every lane's cloud is compared with its context's bit for bit.  Then
seven more calls of loam_lanes_surround under loam_set_profiling for its device time per call and
kernel (loam_mapping_surround records none).

--shared stream|big (instead of the above): per S, a fleet localizing in one map both
ways in one process, alternating three times: shared lanes (loam_lanes_open_shared, the context
imports the map, every lane set to the zero pose) and the parent's only way, own-store lanes with the
map imported into all S lanes (lane_map_capacity = the smallest power of two that holds it).  The
map: what a context builds over stream 1 in --sweeps sweeps, or tools/localize_bench.py's big map
(1.5 M uniform points).  Per run: the device memory the open took (hipMemGetInfo before and after),
the wall time of lanes_step after the warm-up, mapping steps and the others apart, the lanes that
failed, and on the shared side the largest FromMap a lane gathered.  An open that fails is reported
(opens = false), not an error.  --profile-s S: one more shared run at that S under
loam_set_profiling, the device time per kernel and step and per launch.

--score stream|big (instead of the above): shared lanes in that map; S from --s and k
from --k are paired by position (64,1024 with 256,64: the shapes 64 x 256 and 1024 x 64).  Per shape,
k pose guesses for every lane's last sweep scored both ways on the same context, alternating three
times: one loam_lanes_score call, and the parent's only way, S loam_map_score calls of k poses each
with the lane's Last clouds handed in from host memory (obtained from node-call contexts, which is
not timed).  max_dist 0.5; wall time per way, median and range of 5 after a warm-up; one more call of
each under loam_set_profiling for the device time per kernel; sampled rows of both ways compared bit
for bit.

--localize stream|big (instead of the above): the same fleet and shapes (--s and --k
paired by position: 64,1024 with 16,1).  Per shape, k candidate poses near every lane's pose (the
score mode's distribution as aft, the lane's od_sum as bef) refined both ways on the same context,
alternating three times: one loam_lanes_localize call, and the parent's only way, S loam_map_localize
calls of k candidates each with the lane's Last clouds and od_sum handed in from host memory (from
node-call contexts, not timed).  Wall time per way, median and range of 5 after a warm-up; one more
call of each under loam_set_profiling for the device time per kernel and the share of the two rows
kernels; sampled rows of both ways compared bit for bit in every pair.

--commit stream|big (instead of the above): S shared lanes in that map with
map_capacity = the power of two that holds the map and S stacks of 4096 points.  Behind every mapping
step one loam_lanes_map_commit of all live lanes: its wall time, median and range over the mapping
steps after the warm-up, --pairs times alternating with the yardstick, the parent's way to the same
effect: S loam_mapping calls per mapping step on a context holding the map, fed each stream's
CornerLast / SurfLast / fullEnd of that step from host memory (from node calls, not timed; shared
lanes hand out no feature clouds, so the cost of S downloads is reported from loam_lanes_registered).
Also: hipMemGetInfo around the first commit against the derived working set, the map's size after
every commit, and the mapping steps' wall time with commits against one more run without.
--profile-s S: one more fleet at that S with every timed commit under loam_set_profiling (device ms per
stage, summed over the commits).

--clouds (instead of the above): S own-store lanes over 33 sweeps (15 mapping steps: a
warm-up of four, eleven timed).  Behind every mapping step, each call into room made beforehand: --pairs
times alternating the yardstick (the parent's only way: S loam_lanes_registered calls) and one
loam_lanes_clouds of the registered cloud alone; then one loam_lanes_clouds of all nine clouds and one
loam_lanes_clouds_device of all nine (no consumer stream: the call waits).  Wall ms of each, median and
range over the timed steps; GB/s of the nine clouds' packed bytes beside hipMemcpy device-to-host of one
pinned 32 MiB block in the same process; the last timed step once more under loam_set_profiling (device
ms per stage; the device form's traffic = read + written bytes over k_lanes_pack's time).  One process
per row: --s 64, --s 1024."""
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


class DeviceSweeps:
    """every stream's sweeps uploaded once into hipMalloc'd memory (--feed device): one buffer per
    stream (consecutive lanes lie in different allocations: the push queries HIP for every lane), or
    all of them in one arena (one query per push)"""

    def __init__(self, streams, K, arena=False):
        import ctypes
        loam.lib()
        self.hip = hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
        hip.hipFree.argtypes = [ctypes.c_void_p]
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        packed = [np.ascontiguousarray(np.concatenate(st[:K]), np.float32) for st in streams]
        sizes = [(a.nbytes + 255) // 256 * 256 for a in packed]
        self.bufs = []
        for n in [sum(sizes)] if arena else sizes:
            p = ctypes.c_void_p()
            if hip.hipMalloc(ctypes.byref(p), n) != 0:
                raise RuntimeError("hipMalloc failed")
            self.bufs.append(p.value)
        starts = np.concatenate([[0], np.cumsum(sizes)])
        bases = [self.bufs[0] + int(starts[i]) if arena else self.bufs[i] for i in range(len(packed))]
        for base, a in zip(bases, packed):
            if hip.hipMemcpy(base, a.ctypes.data, a.nbytes, 1) != 0:
                raise RuntimeError("hipMemcpy failed")
        self.raws = []  # [stream][k] = (ptr, count, stride)
        for i, st in enumerate(streams):
            off, row = 0, []
            for sw in st[:K]:
                row.append((bases[i] + off, sw.shape[0], sw.shape[1] * 4))
                off += sw.shape[0] * sw.shape[1] * 4
            self.raws.append(row)

    def free(self):
        for p in self.bufs:
            self.hip.hipFree(p)


def run_lanes(S, streams, K, map_cap, profile=False, imu=None, dev=None):
    """dev: a DeviceSweeps: the steps go through lanes_push_device (flags 0: the uploads were synchronous)"""
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
        raws = [(dev.raws if dev else streams)[l % N_STREAMS][k] for l in range(S)]
        if profile and k == 2 + WARM:
            eng.set_profiling(True)
        if imu:
            t0 = time.perf_counter()
            for l in range(S):
                for m in imu[l % N_STREAMS][k]:
                    eng.lanes_imu(l, *m)
            feed.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        (eng.lanes_push_device if dev else eng.lanes_push)(raws, stamp=0.1 * k)
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


def run_feed(S, streams, K, map_cap, pairs=3, profile=False):
    """--feed device: the same steps fed from host memory (lanes_push) and from device memory
    (lanes_push_device), alternating in one process, the host feed first; the device feed once more
    from one arena, where one pointer query serves every lane"""
    devs = {"device": DeviceSweeps(streams, K), "device_arena": DeviceSweeps(streams, K, arena=True)}
    runs = []
    equal = True
    for p in range(pairs):
        pair = {}
        for feed in ("host", "device", "device_arena"):
            res, last, _, _ = run_lanes(S, streams, K, map_cap, dev=devs.get(feed))
            pair[feed] = res
            if feed == "host":
                ref = last
            else:
                equal = equal and all(np.array_equal(np.ascontiguousarray(last[k]).view(np.uint32),
                                                     np.ascontiguousarray(ref[k]).view(np.uint32)) for k in last)
        runs.append(pair)
    line = dict(S=S, sweeps=K, pairs=runs, device_last_pull_equals_host=bool(equal))
    for kind in ("mapped", "unmapped"):
        ratios = [r["host"][f"step_{kind}_ms"]["median"] / r["device"][f"step_{kind}_ms"]["median"] for r in runs]
        line[f"host_over_device_{kind}"] = [round(v, 3) for v in ratios]
        line[f"device_below_host_{kind}"] = bool(min(ratios) > 1.0)
    # what the per-lane pointer queries cost: the push with a query for every lane against the push
    # whose lanes all lie in one allocation (one query)
    q = [r["device"]["push_mapped_ms"]["median"] - r["device_arena"]["push_mapped_ms"]["median"] for r in runs]
    line["pointer_queries_ms"] = [round(v, 4) for v in q]
    line["push_device_ms"] = [r["device"]["push_mapped_ms"]["median"] for r in runs]
    if profile:
        kerns = {}
        for feed in ("host", "device"):
            _, _, kern, n_prof = run_lanes(S, streams, K, map_cap, profile=True, dev=devs.get(feed))
            kerns[feed] = dict(device_ms_per_step=kern, device_ms_per_step_total=round(sum(kern.values()), 4),
                               steps=n_prof[0] + n_prof[1])
        line["profiled"] = kerns
    for d in devs.values():
        d.free()
    return line


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


def run_restart(S, streams, K, map_cap, k_lanes, every, profile):
    eng = loam.Engine(loam.default_config(system_delay=1))
    t0 = time.perf_counter()
    eng.lanes_open(S, map_cap)
    open_ms = (time.perf_counter() - t0) * 1e3
    half = K // 2
    step = {(on, m): [] for on in (False, True) for m in (0, 1)}
    calls, nxt, events = [], 0, 0
    for k in range(K):
        raws = [streams[l % N_STREAMS][k] for l in range(S)]
        on = k >= half
        if k == half and profile:
            eng.set_profiling(True)
        if on and (k - half) % every == 0:
            t0 = time.perf_counter()
            for _ in range(k_lanes):
                eng.lanes_restart(nxt % S)
                nxt += 1
            calls.append((time.perf_counter() - t0) * 1e3)
            events += 1
        t0 = time.perf_counter()
        eng.lanes_push(raws, stamp=0.1 * k)
        o = eng.lanes_pull()
        if k >= 2 + WARM:
            step[(on, int(o["mapped"].max()))].append((time.perf_counter() - t0) * 1e3)
    if profile:
        kt = eng.kernel_times()
        eng.close()
        return dict(device_ms_per_launch={n: round(kt[n][0] / kt[n][1], 4) for n in ("k_lanes_restart", "k_lanes_init")
                                          if n in kt and kt[n][1]},
                    launches={n: kt[n][1] for n in ("k_lanes_restart", "k_lanes_init") if n in kt})
    t0 = time.perf_counter()
    eng.lanes_close()
    t1 = time.perf_counter()
    eng.lanes_open(S, map_cap)
    t2 = time.perf_counter()
    eng.lanes_close()
    eng.close()
    return dict(S=S, restart_lanes=k_lanes, every=every, sweeps=K, first_open_ms=round(open_ms, 1),
                step_mapped_ms_without=spread(step[(False, 1)]), step_mapped_ms_with=spread(step[(True, 1)]),
                step_unmapped_ms_without=spread(step[(False, 0)]), step_unmapped_ms_with=spread(step[(True, 0)]),
                restart_events=events, restart_calls_ms_per_event=spread(calls),
                close_ms=round((t1 - t0) * 1e3, 2), reopen_ms=round((t2 - t1) * 1e3, 2),
                close_plus_open_ms=round((t2 - t0) * 1e3, 2))


def run_occupancy(n_rec, streams, map_cap, S=16):
    rng = np.random.default_rng(0)
    lens = [int(v) for v in rng.integers(10, 41, size=n_rec)]
    recs = [(i % N_STREAMS, lens[i]) for i in range(n_rec)]
    empty = np.zeros((0, 4), np.float32)
    # (a) recycled with loam_lanes_restart; a recording's sweep 0 is the one system_delay drops
    eng = loam.Engine(loam.default_config(system_delay=1))
    t0 = time.perf_counter()
    eng.lanes_open(S, map_cap)
    todo = list(range(n_rec))
    lane = [None] * S  # (recording, next sweep, steps to wait)
    for l in range(S):
        lane[l] = (todo.pop(0), 0, 0) if todo else None
    steps = restarts = 0
    while any(v is not None for v in lane):
        raws = []
        for l in range(S):
            if lane[l] is not None and lane[l][2] == 0 and lane[l][1] >= recs[lane[l][0]][1]:
                lane[l] = None  # the recording has ended: the next one, or the lane is retired
                if todo:
                    lane[l] = (todo.pop(0), 1, eng.lanes_restart(l))
                    restarts += 1
            if lane[l] is None:
                raws.append(empty)
                continue
            r, j, w = lane[l]
            raws.append(streams[recs[r][0]][j if w == 0 else 0])
            lane[l] = (r, j + 1, 0) if w == 0 else (r, j, w - 1)
        if any(v is not None for v in lane):
            eng.lanes_step(raws, stamp=0.1 * steps)
            steps += 1
    eng.lanes_close()
    recycled_s = time.perf_counter() - t0
    # (b) waves of S recordings, an ended one fed count = 0 until the wave's longest has ended
    t0 = time.perf_counter()
    wsteps = 0
    for w0 in range(0, n_rec, S):
        wave = recs[w0:w0 + S]
        eng.lanes_open(len(wave), map_cap)
        for k in range(max(n for _, n in wave)):
            eng.lanes_step([streams[i][k] if k < n else empty for i, n in wave], stamp=0.1 * k)
            wsteps += 1
        eng.lanes_close()
    waves_s = time.perf_counter() - t0
    eng.close()
    total = sum(lens)
    return dict(occupancy_recordings=n_rec, S=S, sweeps_total=total, lengths_min_max=[min(lens), max(lens)],
                recycled=dict(steps=steps, restarts=restarts, wall_s=round(recycled_s, 3),
                              sweeps_per_s=round(total / recycled_s, 1), occupancy=round(total / (steps * S), 3)),
                left_dead=dict(steps=wsteps, waves=(n_rec + S - 1) // S, wall_s=round(waves_s, 3),
                               sweeps_per_s=round(total / waves_s, 1), occupancy=round(total / (wsteps * S), 3)),
                recycled_over_left_dead=round(waves_s / recycled_s, 3))


def _dtod_ms(nbytes, reps=7, warm=2):
    """hipMemcpyDtoD of nbytes between two fresh device buffers: event times in ms"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    vp = ctypes.c_void_p

    def ok(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")
    a, b, e0, e1 = vp(), vp(), vp(), vp()
    ok(hip.hipMalloc(ctypes.byref(a), ctypes.c_size_t(nbytes)))
    ok(hip.hipMalloc(ctypes.byref(b), ctypes.c_size_t(nbytes)))
    ok(hip.hipMemset(a, 1, ctypes.c_size_t(nbytes)))
    ok(hip.hipEventCreate(ctypes.byref(e0)))
    ok(hip.hipEventCreate(ctypes.byref(e1)))
    ts = []
    for r in range(warm + reps):
        ok(hip.hipEventRecord(e0, None))
        ok(hip.hipMemcpyDtoDAsync(b, a, ctypes.c_size_t(nbytes), None))
        ok(hip.hipEventRecord(e1, None))
        ok(hip.hipEventSynchronize(e1))
        ms = ctypes.c_float(0)
        ok(hip.hipEventElapsedTime(ctypes.byref(ms), e0, e1))
        if r >= warm:
            ts.append(ms.value)
    for ev in (e0, e1):
        ok(hip.hipEventDestroy(ev))
    ok(hip.hipFree(a))
    ok(hip.hipFree(b))
    return ts


def run_map_import(S, maps, map_cap, yard_max, reps=7, warm=2):
    """one JSON line per map: see the module text"""
    ny = min(S, yard_max)
    eng = loam.Engine(loam.default_config(system_delay=1))
    eng.lanes_open(S, map_cap)
    yard = []
    for _ in range(ny):
        e = loam.Engine(loam.default_config(system_delay=1, map_capacity=map_cap))
        e.set_tuning(batch_streams=0)
        yard.append(e)
    every = list(range(S))
    out = []
    for name, m in maps:
        kw = dict(corner=m["corner"], surf=m["surf"], center=m["center"], surround_phase=4)
        wall = {"lanes_all": [], "lanes_one": [], "context_one": [], "contexts_all": []}

        def timed(key, f, r):
            t0 = time.perf_counter()
            f()
            if r >= warm:
                wall[key].append((time.perf_counter() - t0) * 1e3)
        dropped = None
        for r in range(warm + reps):  # (every call ends in its own synchronisation)
            timed("lanes_all", lambda: eng.lanes_map_import(every, **kw), r)
            timed("contexts_all", lambda: [e.map_import(**kw) for e in yard], r)
            timed("lanes_one", lambda: eng.lanes_map_import([0], **kw), r)
            timed("context_one", lambda: yard[0].map_import(**kw), r)
        dropped = eng.lanes_map_import(every, **kw)
        lm, cm = eng.lanes_map_export(S - 1), yard[-1].map_export()
        same = all(np.array_equal(lm[k], cm[k]) for k in ("corner", "surf", "corner_offset", "surf_offset"))
        kept = int(lm["corner"].shape[0] + lm["surf"].shape[0])
        # device time per launch, in runs of their own (the events cost host time)
        dev = {}
        for key, f in (("lanes_all", lambda: eng.lanes_map_import(every, **kw)),
                       ("lanes_one", lambda: eng.lanes_map_import([0], **kw))):
            eng.set_profiling(True)
            for _ in range(reps):
                f()
            dev[key] = {k: [round(v[0] / v[1], 4), v[1]] for k, v in sorted(eng.kernel_times().items()) if v[1]}
            eng.set_profiling(False)
        yard[0].set_profiling(True)
        for _ in range(reps):
            yard[0].map_import(**kw)
        dev["context_one"] = {k: [round(v[0] / v[1], 4), v[1]] for k, v in sorted(yard[0].kernel_times().items()) if v[1]}
        yard[0].set_profiling(False)
        line = dict(map_import=name, S=S, map_cap=map_cap, points_in=int(m["corner"].shape[0] + m["surf"].shape[0]),
                    kept=kept, dropped=list(dropped), lane_equals_context=bool(same), contexts=ny,
                    contexts_scaled=ny != S, wall_ms={k: spread(v) for k, v in wall.items()},
                    device_ms_per_launch_and_launches=dev)
        line["contexts_over_lanes"] = round(line["wall_ms"]["contexts_all"]["median"] * (S / ny) /
                                            line["wall_ms"]["lanes_all"]["median"], 2)
        line["lanes_one_minus_context_one_ms"] = round(line["wall_ms"]["lanes_one"]["median"] -
                                                       line["wall_ms"]["context_one"]["median"], 4)
        for key in ("lanes_all", "lanes_one"):
            n = S if key == "lanes_all" else 1
            nbytes = n * (kept + 4851) * 16
            ms = dev[key].get("k_lanes_map_install", [0, 0])[0]
            copy = spread(_dtod_ms(nbytes))
            line[f"install_{key}"] = dict(bytes_written=nbytes, device_ms=ms,
                                          gb_per_s=round(nbytes / ms / 1e6, 1) if ms else None, dtod_ms=copy,
                                          dtod_gb_per_s=round(nbytes / copy["median"] / 1e6, 1))
        out.append(line)
    for e in yard:
        e.close()
    eng.lanes_close()
    eng.close()
    return out


def run_surround(S, streams, map_cap, yard_max, reps=7, warm=2):
    """one JSON line: see the module text"""
    import ctypes
    K = 23
    L = loam.lib()
    ny = min(S, yard_max)
    eng = loam.Engine(loam.default_config(system_delay=1))
    eng.lanes_open(S, map_cap)
    yard = []
    for _ in range(ny):
        e = loam.Engine(loam.default_config(system_delay=1, map_capacity=map_cap))
        e.set_tuning(batch_streams=0)
        yard.append(e)
    for k in range(K):
        if k == K - 1:  # each context takes its lane's map (surround_phase 4 here) in front of the last frame
            for l, e in enumerate(yard):
                m = eng.lanes_map_export(l)
                if m["surround_phase"] != 4:
                    raise RuntimeError("the last frame is not the lanes' publishing frame")
                e.map_import(**{f: m[f] for f in ("corner", "surf", "center", "surround_phase", "aft", "bef")})
        o = eng.lanes_step([streams[l % N_STREAMS][k] for l in range(S)], stamp=0.1 * k)
        for l, e in enumerate(yard):
            e.chain_sweep(streams[l % N_STREAMS][k], stamp=0.1 * k)
    if not (np.all(o["status"] == 0) and np.all(o["mapped"] == 1)):
        raise RuntimeError("the last step did not map every lane")
    ref = eng.lanes_surround()
    if any(c is None for c in ref):
        raise RuntimeError("a lane is not due on the last step")
    total = sum(c.shape[0] for c in ref)
    pts = np.zeros((total, 4), np.float32)
    off = np.zeros(S + 1, np.uint32)
    pub = np.zeros(S, np.int32)
    lc = loam.LanesCloud(pts.ctypes.data, total, 0, off.ctypes.data, pub.ctypes.data)
    outs = [np.zeros((ref[l].shape[0], 4), np.float32) for l in range(ny)]
    cos = [loam.CloudOut(a.ctypes.data, 0, a.shape[0]) for a in outs]
    flag = ctypes.c_int(0)

    def lanes_call():
        if L.loam_lanes_surround(eng.h, ctypes.byref(lc)) != 0:
            raise RuntimeError(L.loam_last_error().decode())

    def contexts_call():
        for e, c in zip(yard, cos):
            if L.loam_mapping_surround(e.h, ctypes.byref(c), ctypes.byref(flag)) != 0 or not flag.value:
                raise RuntimeError("a context did not publish: " + L.loam_last_error().decode())

    wall = {"lanes": [], "contexts": []}
    for r in range(warm + reps):
        for key, f in (("lanes", lanes_call), ("contexts", contexts_call)):
            t0 = time.perf_counter()
            f()
            if r >= warm:
                wall[key].append((time.perf_counter() - t0) * 1e3)
    same = all(np.array_equal(pts[off[l]:off[l + 1]].view(np.uint32), outs[l].view(np.uint32)) for l in range(ny))
    # (loam_mapping_surround records no per-kernel times: the lanes' call alone)
    eng.set_profiling(True)
    for _ in range(reps):
        lanes_call()
    dev = {k: round(v[0] / reps, 4) for k, v in sorted(eng.kernel_times().items()) if v[1]}
    eng.set_profiling(False)
    for e in yard:
        e.close()
    eng.lanes_close()
    eng.close()
    line = dict(surround=True, S=S, map_cap=map_cap, sweeps=K, points_out=int(total),
                points_out_per_lane=[int(min(c.shape[0] for c in ref)), int(max(c.shape[0] for c in ref))],
                contexts=ny, contexts_scaled=ny != S, lanes_equal_contexts=bool(same),
                wall_ms={k: spread(v) for k, v in wall.items()}, device_ms_per_call=dev)
    lm, cm = line["wall_ms"]["lanes"], line["wall_ms"]["contexts"]
    line["contexts_over_lanes"] = round(cm["median"] * (S / ny) / lm["median"], 2)
    # the call beats the serial contexts by more than the spread of the repetitions
    line["lanes_max_below_contexts_min"] = bool(lm["max"] < cm["min"] * (S / ny))
    return line


def _mem_free():
    """free device memory in bytes (hipMemGetInfo)"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
    if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) != 0:
        raise RuntimeError("hipMemGetInfo failed")
    return int(free.value)


def shared_big_map(M):
    """tools/localize_bench.py's big map: 1.5 M uniform points about M's centre"""
    rng = np.random.default_rng(20261019)
    half = np.array([546.0, 286.0, 546.0])

    def uniform(n):
        p = np.empty((n, 4), np.float32)
        p[:, :3] = (rng.uniform(-1.0, 1.0, (n, 3)) * half).astype(np.float32)
        p[:, 3] = rng.uniform(0, 16, n).astype(np.float32)
        return p
    return dict(M, corner=uniform(388894), surf=uniform(1111106), center=np.array([10, 5, 10], np.int32))


def run_fleet(S, streams, K, M, cap, shared, profile=False):
    """S lanes over K steps in the map M: shared lanes of lane_from_capacity cap in a context that
    imported M, or own-store lanes of lane_map_capacity cap with M imported into every lane.  The
    device memory the open (and, own-store, nothing else) took, the wall time of the steps after
    the warm-up, and every lane's last status."""
    kw = dict(corner=M["corner"], surf=M["surf"], center=M["center"], surround_phase=4)
    total = int(M["corner"].shape[0] + M["surf"].shape[0])
    free_ctx = _mem_free()
    # (the context's own store holds M on the shared side and stays empty on the other)
    eng = loam.Engine(loam.default_config(system_delay=1, map_capacity=max(1 << 17, 1 << int(np.ceil(np.log2(total))))
                                          if shared else 1 << 17))
    eng.set_tuning(batch_streams=0)
    if shared:
        eng.map_import(**kw)
    free0 = _mem_free()
    t0 = time.perf_counter()
    try:
        (eng.lanes_open_shared if shared else eng.lanes_open)(S, cap)
    except loam.LoamError as err:
        eng.close()
        return dict(opens=False, error=str(err)[:160])
    open_ms = (time.perf_counter() - t0) * 1e3
    held = free0 - _mem_free()
    t0 = time.perf_counter()
    if shared:
        eng.lanes_set_pose(list(range(S)), np.zeros(6, np.float32))
    else:
        eng.lanes_map_import(list(range(S)), **kw)
    seed_ms = (time.perf_counter() - t0) * 1e3
    step = {0: [], 1: []}
    n_prof = 0
    status = None
    frm = 0
    for k in range(K):
        raws = [streams[l % N_STREAMS][k] for l in range(S)]
        if profile and k == 2 + WARM:
            eng.set_profiling(True)
        t0 = time.perf_counter()
        eng.lanes_push(raws, stamp=0.1 * k)
        o = eng.lanes_pull()
        t1 = time.perf_counter()
        status = o["status"]
        if k >= 2 + WARM:
            step[int(o["mapped"].max())].append((t1 - t0) * 1e3)
            n_prof += 1
        if shared and o["mapped"].max():
            i = eng.lanes_localize_info()
            frm = max(frm, int((i["map_corner"].astype(np.int64) + i["map_surf"]).max()))
    res = dict(opens=True, open_ms=round(open_ms, 1), held_bytes=held, context_bytes=free_ctx - free0,
               seed_ms=round(seed_ms, 2),
               step_mapped_ms=spread(step[1]), step_unmapped_ms=spread(step[0]),
               lanes_failed=int(np.count_nonzero(status != 0)))
    if shared:
        res["from_map_max"] = frm
    if profile:
        res["device_ms_per_step"] = {k: round(v[0] / n_prof, 4)
                                     for k, v in sorted(eng.kernel_times().items(), key=lambda kv: -kv[1][0])}
        res["device_ms_per_launch"] = {k: round(v[0] / v[1], 4) for k, v in sorted(eng.kernel_times().items()) if v[1]}
        res["profiled_steps"] = n_prof
        eng.set_profiling(False)
    eng.lanes_close()
    eng.close()
    return res


def run_shared(S, streams, K, name, M, from_cap, pairs=3, profile=False):
    """one JSON line: `pairs` alternating (shared, own-store) runs of S lanes in the map M"""
    total = int(M["corner"].shape[0] + M["surf"].shape[0])
    C = 1 << int(np.ceil(np.log2(max(total, 1024))))
    runs = []
    grown = []  # own-store capacities at which a lane's store overflowed while it mapped into it
    for _ in range(pairs):
        sh = run_fleet(S, streams, K, M, from_cap, True)
        own = run_fleet(S, streams, K, M, C, False)
        while own["opens"] and own["lanes_failed"] and C < (1 << 24):  # (the yardstick's maps grow: the next power of two)
            grown.append(C)
            C *= 2
            own = run_fleet(S, streams, K, M, C, False)
        runs.append(dict(shared=sh, own_store=own))
        if not own["opens"] or not sh["opens"]:
            break  # (an open that fails fails every time)
    line = dict(shared_leg=name, S=S, sweeps=K, map_points=total, lane_map_capacity=C, lane_from_capacity=from_cap,
                own_store_overflowed_at=grown, pairs=runs)
    both = [r for r in runs if r["shared"]["opens"] and r["own_store"]["opens"]]
    if both:
        line["shared_not_above_own_mapped"] = [bool(r["shared"]["step_mapped_ms"]["median"] <=
                                                    r["own_store"]["step_mapped_ms"]["median"]) for r in both]
        saved = both[0]["own_store"]["held_bytes"] - both[0]["shared"]["held_bytes"]
        line["held_bytes_saved"] = saved
        line["held_bytes_saved_bound"] = S * 112 * (C - from_cap)
        line["memory_accepted"] = bool(saved >= S * 112 * (C - from_cap))
    if profile:
        line["profile_shared"] = run_fleet(S, streams, K, M, from_cap, True, profile=True)
    return line


def commit_bytes(S, cap_stack):
    """device bytes of loam_lanes_map_commit's working set as DESIGN.md §34 derives them"""
    keys = 2 * 21 * 11 * 21
    return S * cap_stack * 24 + S * min(cap_stack, keys) * 8 + S * 8 + (152 + 4 + 16) * 4 + keys * 9 * 4


def run_commit(S, streams, K, name, M, from_cap, pairs=3, profile=False):
    """one JSON line: S shared lanes in the map M; behind every mapping step after the
    warm-up one loam_lanes_map_commit of all S lanes, against the parent's way to the same effect: S
    loam_mapping calls on a context holding M, one lane's clouds after the other.  The yardstick's
    clouds are each stream's CornerLast / SurfLast / fullEnd of that step from node calls (shared
    lanes hand out no feature clouds; what a download would cost is reported from
    loam_lanes_registered).  `pairs` alternating (commit, yardstick) runs; the first commit's device
    memory; the mapping steps of a run with commits against the same run without."""
    kw = dict(corner=M["corner"], surf=M["surf"], center=M["center"], surround_phase=4)
    total = int(M["corner"].shape[0] + M["surf"].shape[0])
    cfg = loam.default_config()
    pts_cap = int(cfg.max_points) + 120 * int(cfg.n_rings)  # a lane's stack capacity
    # the VoxelGrid input of a commit holds the union's cubes and every lane's stack before it shrinks
    cap = 1 << int(np.ceil(np.log2(total + S * 4096)))
    cap = max(cap, 1 << 17)

    def fleet(commit, prof=False):
        eng = loam.Engine(loam.default_config(system_delay=1, map_capacity=cap))
        eng.set_tuning(batch_streams=0)
        eng.map_import(**kw)
        eng.lanes_open_shared(S, from_cap)
        eng.lanes_set_pose(list(range(S)), np.zeros(6, np.float32))
        lanes = list(range(S))
        steps, commits, downloads, grown, ws = [], [], [], [], None
        res = refused = None
        device = {}
        committing = commit
        for k in range(K):
            raws = [streams[l % N_STREAMS][k] for l in range(S)]
            t0 = time.perf_counter()
            eng.lanes_push(raws, stamp=0.1 * k)
            o = eng.lanes_pull()
            t1 = time.perf_counter()
            if not o["mapped"].max():
                continue
            if k >= 2 + WARM:
                steps.append((t1 - t0) * 1e3)
            if not commit:
                continue
            # the lanes a commit takes: live, and their frame ran (LOAM_LOC_SOLVED or LOAM_LOC_NO_LM)
            st = eng.lanes_localize_info()["status"]
            ok = [l for l in lanes if o["status"][l] == 0 and o["mapped"][l] and st[l] in (loam.LOC_SOLVED, loam.LOC_NO_LM)]
            if not ok:
                continue
            if k >= 2 + WARM:  # (what downloading one cloud per lane costs: the registered clouds)
                t0 = time.perf_counter()
                for l in ok:
                    eng.lanes_registered(l)
                downloads.append((time.perf_counter() - t0) * 1e3)
            free0 = _mem_free()
            t0 = time.perf_counter()
            try:
                if prof and k >= 2 + WARM:  # (device ms per launch between the marks, summed over the timed commits)
                    for name_, ms in _profiled(eng, lambda: eng.lanes_map_commit(ok)).items():
                        device[name_] = round(device.get(name_, 0.0) + ms, 4)
                    device["commits"] = device.get("commits", 0) + 1
                    continue
                res = eng.lanes_map_commit(ok)
            except loam.LoamError as err:  # (reported, and the run goes on without further commits)
                refused = str(err)[:160]
                commit = False
                continue
            t1 = time.perf_counter()
            if ws is None:
                ws = free0 - _mem_free()
            if k >= 2 + WARM:
                commits.append((t1 - t0) * 1e3)
            grown.append(sum(res["map_points"]))
        out = dict(step_mapped_ms=spread(steps), lanes_failed=int(np.count_nonzero(o["status"] != 0)))
        if committing:
            out.update(commit_ms=spread(commits), registered_download_ms=spread(downloads), working_set_bytes=ws,
                       map_points_after_commits=grown, last_commit=res, commit_refused=refused)
        if prof:
            out["device_ms"] = device
        eng.lanes_close()
        eng.close()
        return out

    # the yardstick's clouds: per stream and step what loam_odometry publishes for laserMapping
    feats = []
    for i in range(min(S, N_STREAMS)):
        A = loam.Engine(loam.default_config(system_delay=1))
        per = {}
        for k in range(K):
            rc, f = A.scan_registration(streams[i][k], stamp=0.1 * k)
            if rc == 0:
                pub, pose, cl, sl, full = A.odometry(f, stamp=0.1 * k)
                if pub == 7:
                    per[k] = (pose, cl, sl, full)
        A.close()
        feats.append(per)

    def yard():
        Y = loam.Engine(loam.default_config(system_delay=1, map_capacity=cap))
        Y.map_import(**kw)
        ts, failed = [], None
        for k in sorted(set.intersection(*[set(f) for f in feats])):
            t0 = time.perf_counter()
            try:
                for l in range(S):
                    Y.mapping(*feats[l % len(feats)][k], stamp=0.1 * k)
            except loam.LoamError as err:
                failed = str(err)[:160]
                break
            if k >= 2 + WARM:
                ts.append((time.perf_counter() - t0) * 1e3)
        Y.close()
        return dict(mapping_calls_ms=spread(ts), mapping_failed=failed)
    runs = [dict(commit=fleet(True), yardstick=yard()) for _ in range(pairs)]
    plain = fleet(False)
    line = dict(commit_leg=name, S=S, sweeps=K, map_points=total, map_capacity=cap, lane_from_capacity=from_cap,
                working_set_bytes_derived=commit_bytes(S, pts_cap), pairs=runs, steps_without_commits=plain)
    both = [(r["commit"]["commit_ms"], r["yardstick"]["mapping_calls_ms"]) for r in runs]
    both = [(c, y) for c, y in both if c and y]  # (a side without a timed mapping step has no figure)
    line["pairs_timed"] = len(both)
    line["commit_below_yardstick"] = [bool(c["median"] < y["median"]) for c, y in both]
    line["ranges_apart"] = [bool(c["max"] < y["min"]) for c, y in both]
    line["yardstick_over_commit"] = [round(y["median"] / c["median"], 1) for c, y in both]
    if profile:
        line["profile_commit"] = fleet(True, prof=True)
    return line


def _profiled(eng, call):
    """device ms per kernel and the work counters of one call under loam_set_profiling"""
    eng.set_profiling(True)
    before = eng.kernel_times()
    call()
    after = eng.kernel_times()
    eng.set_profiling(False)
    return {k: round(v[0] - before.get(k, (0.0, 0))[0], 4) for k, v in sorted(after.items())
            if v[1] != before.get(k, (0.0, 0))[1]}


def run_score(S, k, streams, name, M, from_cap, pairs=3, reps=5):
    """one JSON line: k poses for each of S shared lanes in the map M, loam_lanes_score against S
    loam_map_score calls on the same context, `pairs` alternating timings"""
    kw = dict(corner=M["corner"], surf=M["surf"], center=M["center"], surround_phase=4)
    total = int(M["corner"].shape[0] + M["surf"].shape[0])
    eng = loam.Engine(loam.default_config(system_delay=1, map_capacity=max(1 << 17, 1 << int(np.ceil(np.log2(total))))))
    eng.set_tuning(batch_streams=0)
    eng.map_import(**kw)
    eng.lanes_open_shared(S, from_cap)
    eng.lanes_set_pose(list(range(S)), np.zeros(6, np.float32))
    n_steps = 3
    for j in range(n_steps):
        o = eng.lanes_step([streams[l % N_STREAMS][j] for l in range(S)], stamp=0.1 * j)
    # the yardstick's clouds (not timed): every stream's Last clouds of that step from a node-call context
    last = []
    for i in range(min(S, N_STREAMS)):
        A = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=0))
        for j in range(n_steps):
            rc, f = A.scan_registration(streams[i][j], stamp=0.1 * j)
            if rc == 0:
                _, _, cl, sl, _ = A.odometry(f, stamp=0.1 * j)
        A.close()
        last.append((cl, sl))
    rng = np.random.default_rng(31)
    P = (rng.uniform(-1, 1, (k, 6)) * np.array([0.05, 0.05, 0.05, 0.5, 0.5, 0.5])).astype(np.float32)
    lanes = list(range(S))

    def new():
        return eng.lanes_score(lanes, P, 0.5)

    def yard():
        return [eng.map_score(*last[l % N_STREAMS], P, 0.5) for l in lanes]

    def timed(call):
        call()  # warm-up
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return spread(ts)
    runs = [dict(lanes_score_ms=timed(new), map_score_calls_ms=timed(yard)) for _ in range(pairs)]
    got, want = new(), yard()
    same = all(np.array_equal(got[key][l].view(np.uint64 if got[key].dtype == np.float64 else np.uint32),
                              want[l][key].view(np.uint64 if got[key].dtype == np.float64 else np.uint32))
               for key in loam.SCORE_KEYS for l in sorted({0, S // 2, S - 1}))
    line = dict(score_leg=name, S=S, k=k, rows=S * k, map_points=total, max_dist=0.5,
                lanes_failed=int(np.count_nonzero(o["status"] != 0)),
                query_points_per_lane=int(np.mean([c.shape[0] + s_.shape[0] for c, s_ in last])), pairs=runs,
                new_below_yardstick=[bool(r["lanes_score_ms"]["median"] < r["map_score_calls_ms"]["median"]) for r in runs],
                yardstick_over_new=[round(r["map_score_calls_ms"]["median"] / r["lanes_score_ms"]["median"], 2) for r in runs],
                sampled_rows_equal=bool(same))
    line["device_ms_lanes_score"] = _profiled(eng, new)
    line["device_ms_map_score_calls"] = _profiled(eng, yard)
    dn, dy = line["device_ms_lanes_score"], line["device_ms_map_score_calls"]
    idx = ("score_index", "k_mp_map_pack", "k_mp_map_table")
    line["index_ms_new"] = round(sum(dn.get(n, 0.0) for n in idx), 4)
    line["index_ms_yardstick"] = round(sum(dy.get(n, 0.0) for n in idx), 4)
    line["index_share_of_yardstick_wall"] = round(line["index_ms_yardstick"] / runs[-1]["map_score_calls_ms"]["median"], 3)
    eng.lanes_close()
    eng.close()
    return line


def run_localize(S, k, streams, name, M, from_cap, pairs=3, reps=5):
    """one JSON line: k candidates for each of S shared lanes in the map M, loam_lanes_localize against
    S loam_map_localize calls on the same context, `pairs` alternating timings"""
    kw = dict(corner=M["corner"], surf=M["surf"], center=M["center"], surround_phase=4)
    total = int(M["corner"].shape[0] + M["surf"].shape[0])
    eng = loam.Engine(loam.default_config(system_delay=1, map_capacity=max(1 << 17, 1 << int(np.ceil(np.log2(total))))))
    eng.set_tuning(batch_streams=0)
    eng.map_import(**kw)
    eng.lanes_open_shared(S, from_cap)
    eng.lanes_set_pose(list(range(S)), np.zeros(6, np.float32))
    n_steps = 3
    for j in range(n_steps):
        o = eng.lanes_step([streams[l % N_STREAMS][j] for l in range(S)], stamp=0.1 * j)
    # the yardstick's inputs (not timed): every stream's Last clouds and od_sum of that step from a node-call context
    last = []
    for i in range(min(S, N_STREAMS)):
        A = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=0))
        for j in range(n_steps):
            rc, f = A.scan_registration(streams[i][j], stamp=0.1 * j)
            if rc == 0:
                _, od, cl, sl, _ = A.odometry(f, stamp=0.1 * j)
        A.close()
        last.append((np.asarray(od, np.float32), cl, sl))
    rng = np.random.default_rng(31)
    P = (rng.uniform(-1, 1, (k, 6)) * np.array([0.05, 0.05, 0.05, 0.5, 0.5, 0.5])).astype(np.float32)
    lanes = list(range(S))
    bef = np.ascontiguousarray(np.stack([np.broadcast_to(last[l % N_STREAMS][0], (k, 6)) for l in lanes]))
    aft = np.ascontiguousarray(np.broadcast_to(P, (S, k, 6)))

    def new():
        return eng.lanes_localize(lanes, aft, bef)

    def yard():
        return [eng.map_localize(*last[l % N_STREAMS], P, bef[l]) for l in lanes]

    def timed(call):
        call()  # warm-up
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
        return spread(ts)

    def same_rows():
        got, want = new(), yard()
        return all(np.array_equal(got[key][l].view(np.uint32), want[l][key].view(np.uint32))
                   for key in loam.LOCALIZE_KEYS for l in sorted({0, S // 2, S - 1}))
    runs, same = [], []
    for _ in range(pairs):
        runs.append(dict(lanes_localize_ms=timed(new), map_localize_calls_ms=timed(yard)))
        same.append(bool(same_rows()))
    got = new()
    line = dict(localize_leg=name, S=S, k=k, rows=S * k, map_points=total,
                lanes_failed=int(np.count_nonzero(o["status"] != 0)),
                rows_solved=int(np.count_nonzero(got["status"] == loam.LOC_SOLVED)),
                from_map_points_per_row=int(np.mean(got["map_corner"].astype(np.int64) + got["map_surf"])),
                stack_points_per_lane=int(np.mean([c.shape[0] + s_.shape[0] for _, c, s_ in last])), pairs=runs,
                new_below_yardstick=[bool(r["lanes_localize_ms"]["median"] < r["map_localize_calls_ms"]["median"]) for r in runs],
                yardstick_over_new=[round(r["map_localize_calls_ms"]["median"] / r["lanes_localize_ms"]["median"], 2)
                                    for r in runs],
                sampled_rows_equal=same)
    line["device_ms_lanes_localize"] = dn = _profiled(eng, new)
    line["device_ms_map_localize_calls"] = _profiled(eng, yard)
    dev = sum(v for key, v in dn.items() if key.startswith(("k_", "vg_", "lanes_localize")))
    line["rows_kernels_share_of_device_ms"] = round((dn.get("k_mp_loc_prepare_rows", 0.0) + dn.get("k_mp_loc_stack_rows", 0.0)) /
                                                    dev, 4) if dev else None
    eng.lanes_close()
    eng.close()
    return line


def _d2h_ceiling_gbs(nbytes=32 << 20, reps=5, warm=2):
    """hipMemcpy device-to-host of one pinned block of nbytes: GB/s, median of reps"""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    hip.hipMemcpy.argtypes = [vp, vp, sz, ctypes.c_int]
    hip.hipHostMalloc.argtypes = [ctypes.POINTER(vp), sz, ctypes.c_uint]
    hip.hipMalloc.argtypes = [ctypes.POINTER(vp), sz]
    hip.hipMemset.argtypes = [vp, ctypes.c_int, sz]
    hip.hipFree.argtypes = [vp]
    hip.hipHostFree.argtypes = [vp]
    d, h = vp(), vp()
    if hip.hipMalloc(ctypes.byref(d), nbytes) or hip.hipHostMalloc(ctypes.byref(h), nbytes, 0) or hip.hipMemset(d, 1, nbytes):
        raise RuntimeError("HIP allocation failed")
    ts = []
    for r in range(warm + reps):
        t0 = time.perf_counter()
        if hip.hipMemcpy(h, d, nbytes, 2):
            raise RuntimeError("hipMemcpy failed")
        if r >= warm:
            ts.append(time.perf_counter() - t0)
    hip.hipFree(d)
    hip.hipHostFree(h)
    return round(nbytes / sorted(ts)[len(ts) // 2] / 1e9, 2)


def run_clouds(S, streams, K, map_cap, pairs=3, measured=11):
    """one JSON line: see --clouds in the module text"""
    import ctypes
    L = loam.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    eng = loam.Engine(loam.default_config(system_delay=1))
    eng.lanes_open(S, map_cap)
    yard = [[] for _ in range(pairs)]
    one = [[] for _ in range(pairs)]
    nine, dev, nine_bytes, reg_bytes = [], [], [], []
    host = {c: np.empty((0, 4), np.float32) for c in loam.LANE_CLOUDS}
    dbuf = {c: [None, 0] for c in loam.LANE_CLOUDS}  # device pointer, points
    offs = {c: np.zeros(S + 1, np.uint32) for c in loam.LANE_CLOUDS}
    prof, n_map = None, 0

    def sizes():
        o = loam.LanesCloudsOut()
        for c in loam.LANE_CLOUDS:
            getattr(o, c).offset = offs[c].ctypes.data
        loam._check(L.loam_lanes_clouds(eng.h, S, None, ctypes.byref(o)))
        return {c: int(getattr(o, c).count) for c in loam.LANE_CLOUDS}

    def call_host(clouds):
        o = loam.LanesCloudsOut()
        for c in clouds:
            b = getattr(o, c)
            b.pts, b.capacity, b.offset = host[c].ctypes.data, host[c].shape[0], offs[c].ctypes.data
        t0 = time.perf_counter()
        rc = L.loam_lanes_clouds(eng.h, S, None, ctypes.byref(o))
        dt = (time.perf_counter() - t0) * 1e3
        loam._check(rc)
        return dt

    def call_dev():
        o = loam.LanesCloudsOut()
        for c in loam.LANE_CLOUDS:
            b = getattr(o, c)
            b.pts, b.capacity, b.offset = dbuf[c][0], dbuf[c][1], offs[c].ctypes.data
        t0 = time.perf_counter()
        rc = L.loam_lanes_clouds_device(eng.h, S, None, ctypes.byref(o), None)
        dt = (time.perf_counter() - t0) * 1e3
        loam._check(rc)
        return dt

    for k in range(K):
        o = eng.lanes_step([streams[l % N_STREAMS][k] for l in range(S)], stamp=0.1 * k)
        if k >= 2 and not np.all(o["status"] == 0):
            raise RuntimeError(f"step {k}: lane status {np.unique(o['status'])}")
        if not o["mapped"][0]:
            continue
        n_map += 1
        if n_map > WARM + measured:
            continue
        # room for this step's clouds, outside the timed calls
        need = sizes()
        for c, n in need.items():
            if host[c].shape[0] < n:
                host[c] = np.empty((n + n // 8, 4), np.float32)
                host[c][:] = 0  # (touched: no page faults inside the timed copy)
            if dbuf[c][1] < n:
                if dbuf[c][0]:
                    hip.hipFree(dbuf[c][0])
                p = ctypes.c_void_p()
                if hip.hipMalloc(ctypes.byref(p), (n + n // 8) * 16) != 0:
                    raise RuntimeError("hipMalloc failed")
                dbuf[c] = [p.value, n + n // 8]
        # the parent's way: S loam_lanes_registered calls, each into its own room
        nreg = o["n_registered"].astype(np.int64)
        start = np.concatenate([[0], np.cumsum(nreg)])
        outs = [loam.CloudOut(host["registered"].ctypes.data + int(start[l]) * 16, 0, int(nreg[l])) for l in range(S)]
        ty, ta = [], []
        for p in range(pairs):
            t0 = time.perf_counter()
            for l in range(S):
                rc = L.loam_lanes_registered(eng.h, l, ctypes.byref(outs[l]))
                if rc:
                    loam._check(rc)
            ty.append((time.perf_counter() - t0) * 1e3)
            ta.append(call_host(("registered",)))
        tb = call_host(loam.LANE_CLOUDS)
        tc = call_dev()
        if n_map == WARM + measured:  # the last timed step once more under profiling (not timed)
            prof = dict(host_all=_profiled(eng, lambda: call_host(loam.LANE_CLOUDS)), device_all=_profiled(eng, call_dev))
        if n_map > WARM:
            for p in range(pairs):
                yard[p].append(ty[p])
                one[p].append(ta[p])
            nine.append(tb)
            dev.append(tc)
            nine_bytes.append(sum(need.values()) * 16)
            reg_bytes.append(need["registered"] * 16)
    for c in dbuf:
        if dbuf[c][0]:
            hip.hipFree(dbuf[c][0])
    eng.lanes_close()
    eng.close()
    nb = float(np.median(nine_bytes))
    line = dict(clouds_S=S, sweeps=K, mapping_steps_timed=len(nine), warm_up=WARM,
                yardstick_registered_calls_ms=[spread(t) for t in yard], registered_one_call_ms=[spread(t) for t in one],
                registered_bytes=int(np.median(reg_bytes)), all_nine_host_ms=spread(nine), all_nine_bytes=int(nb),
                all_nine_host_gbs=round(nb / spread(nine)["median"] / 1e6, 2),
                d2h_pinned_32mib_gbs=_d2h_ceiling_gbs(), all_nine_device_wall_ms=spread(dev), profiled_device_ms=prof)
    line["one_call_below_yardstick_every_pair"] = all(a["max"] < y["min"] for a, y in zip(line["registered_one_call_ms"],
                                                                                        line["yardstick_registered_calls_ms"]))
    if prof and prof["device_all"].get("k_lanes_pack"):
        ms = prof["device_all"]["k_lanes_pack"]
        line["all_nine_device_pack_ms"] = ms
        line["all_nine_device_traffic_gbs"] = round(2 * nb / ms / 1e6, 1)  # read + written
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", default="1,16,64")
    ap.add_argument("--sweeps", type=int, default=27)
    ap.add_argument("--map-cap", type=int, default=1 << 17)
    ap.add_argument("--yard-max", type=int, default=1024)
    ap.add_argument("--profile-s", type=int, default=0)
    ap.add_argument("--imu", action="store_true")
    ap.add_argument("--restart", default=None, help="K,M: restart K lanes (0: S / 4) before every M-th step")
    ap.add_argument("--occupancy", type=int, default=0, help="recordings of 10..40 sweeps over 16 lanes")
    ap.add_argument("--map-import", type=int, default=0, help="points of the synthetic map (and the stream map)")
    ap.add_argument("--surround", action="store_true", help="loam_lanes_surround against serial contexts")
    ap.add_argument("--shared", default=None, help="stream|big: shared lanes against own-store lanes in that map")
    ap.add_argument("--from-cap", type=int, default=0,
                    help="--shared: lane_from_capacity (0: the power of two that holds the stream map, 65536 in the big map)")
    ap.add_argument("--score", default=None, help="stream|big: loam_lanes_score against S loam_map_score calls in that map")
    ap.add_argument("--localize", default=None,
                    help="stream|big: loam_lanes_localize against S loam_map_localize calls in that map")
    ap.add_argument("--commit", default=None,
                    help="stream|big: loam_lanes_map_commit of all lanes against S loam_mapping calls in that map")
    ap.add_argument("--k", default="256,64", help="--score / --localize: poses per lane, paired with --s by position")
    ap.add_argument("--feed", default="host", choices=("host", "device"),
                    help="device: steps fed from host and from device memory (lanes_push_device), alternating")
    ap.add_argument("--pairs", type=int, default=3, help="--feed device: alternating runs of each feed")
    ap.add_argument("--clouds", action="store_true", help="loam_lanes_clouds against S loam_lanes_registered calls")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.shared = a.shared or a.score or a.localize or a.commit
    K = 40 if a.occupancy else 23 if a.surround else 2 + 2 * (WARM + 11) + 1 if a.clouds else a.sweeps
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

    if a.occupancy:
        emit(run_occupancy(a.occupancy, streams, a.map_cap))
        return
    if a.clouds:
        for S in [int(v) for v in a.s.split(",") if v]:
            emit(run_clouds(S, streams, K, a.map_cap, pairs=a.pairs))
        return
    if a.shared:
        e = loam.Engine(loam.default_config(system_delay=1))
        for k in range(K):
            e.chain_sweep(streams[0][k], stamp=0.1 * k)
        M = e.map_export()
        e.close()
        M = dict(M, aft=np.zeros(6, np.float32), bef=np.zeros(6, np.float32))
        if a.shared == "big":
            M = shared_big_map(M)
        # (a lane in the stream map sees all of it: the smallest power of two that holds the map)
        total = int(M["corner"].shape[0] + M["surf"].shape[0])
        F = a.from_cap or (65536 if a.shared == "big" else 1 << int(np.ceil(np.log2(max(total, 1024)))))
        if a.score:
            for S, k in zip([int(v) for v in a.s.split(",") if v], [int(v) for v in a.k.split(",") if v]):
                emit(run_score(S, k, streams, a.score, M, F))
            return
        if a.commit:
            for S in [int(v) for v in a.s.split(",") if v]:
                # (the map grows with every commit and a lane gathers from all of it: room for it)
                emit(run_commit(S, streams, K, a.commit, M, max(F, 1 << 17), pairs=a.pairs, profile=S == a.profile_s))
            return
        if a.localize:
            for S, k in zip([int(v) for v in a.s.split(",") if v], [int(v) for v in a.k.split(",") if v]):
                emit(run_localize(S, k, streams, a.localize, M, F))
            return
        for S in [int(v) for v in a.s.split(",") if v]:
            emit(run_shared(S, streams, K, a.shared, M, F, profile=S == a.profile_s))
        return
    if a.surround:
        for S in [int(v) for v in a.s.split(",") if v]:
            emit(run_surround(S, streams, a.map_cap, a.yard_max))
        return
    if a.map_import:
        e = loam.Engine(loam.default_config(system_delay=1))
        for k in range(K):
            e.chain_sweep(streams[0][k], stamp=0.1 * k)
        stream_map = e.map_export()
        e.close()
        rng = np.random.default_rng(0)
        pts = rng.uniform(-100, 100, (a.map_import, 4)).astype(np.float32)
        synth = dict(corner=pts[:a.map_import // 2], surf=pts[a.map_import // 2:], center=(10, 5, 10))
        for S in [int(v) for v in a.s.split(",") if v]:
            for line in run_map_import(S, [("stream", stream_map), (f"synthetic{a.map_import}", synth)], a.map_cap,
                                       a.yard_max):
                emit(line)
        return
    if a.restart:
        k_lanes, every = [int(v) for v in a.restart.split(",")]
        for S in [int(v) for v in a.s.split(",") if v]:
            n = k_lanes or max(1, S // 4)
            line = run_restart(S, streams, K, a.map_cap, n, every, False)
            line.update(run_restart(S, streams, K, a.map_cap, n, every, True))
            emit(line)
        return
    if a.feed == "device":
        for S in [int(v) for v in a.s.split(",") if v]:
            emit(run_feed(S, streams, K, a.map_cap, pairs=a.pairs, profile=S == a.profile_s))
        return
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
