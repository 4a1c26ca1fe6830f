#!/usr/bin/env python3
"""Measurements of DESIGN.md §40 (loam_set_point_fields), one mode per process:

  point_fields_modes.py sort  MODE LIDAR P   k_sr_ring_sort ms/step (loam_get_kernel_times) of a P-problem batch
  point_fields_modes.py push  MODE           loam_lanes_push / loam_lanes_push_device call time at 64 lanes

MODE is model | ring | ring_time, LIDAR vlp16 | hdl64.  The three modes run on the same sweeps: 32
distinct problems repeated to P; the ring field is the model's own ring of each laser (from one
node call), the time field the point's firing position in the sweep.  Prints one JSON line."""
import ctypes
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

CFG = {"vlp16": dict(), "hdl64": dict(n_rings=64, ring_model=1, max_points=160000)}


def laser_rings(lidar, sweep):
    """the model's ring of each laser, from a node call on one sweep"""
    e = loam.Engine(loam.default_config(system_delay=0, **CFG[lidar]))
    e.scan_registration(sweep)
    rc, f = e.scan_registration(sweep)
    e.close()
    full = f["full"]
    ring_of_xyz = {r.tobytes(): int(i) for r, i in zip(np.ascontiguousarray(full[:, [2, 0, 1]]), full[:, 3])}
    n_lasers = int(sweep[:, 3].max()) + 1
    out = np.full(n_lasers, 65535, np.int64)
    for p in np.ascontiguousarray(sweep[::7]):
        r = ring_of_xyz.get(p[:3].tobytes())
        if r is not None:
            out[int(p[3])] = r
    return out


def clouds_of(mode, lidar, sweeps):
    if mode == "model":
        return [loam.CloudIn(s.ctypes.data, s.shape[0], 16) for s in sweeps], sweeps
    rings = laser_rings(lidar, sweeps[0])
    out, keep = [], []
    for s in sweeps:
        n = s.shape[0]
        tau = (np.arange(n) * (0.0999 / n)).astype(np.float32)
        ci, k = loam.records(s[:, :3], rings[s[:, 3].astype(np.int64)], tau)
        out.append(ci)
        keep.append(k)
    return out, keep


def set_mode(e, mode):
    if mode == "ring":
        e.set_point_fields(ring=(loam.FIELD_U16, 20))
    elif mode == "ring_time":
        e.set_point_fields(ring=(loam.FIELD_U16, 20), time=(loam.FIELD_F32, 24, 1.0, 0.0))


def sort(mode, lidar, P, steps=6, distinct=32):
    prevs, curs = sg.batch_problems(distinct, base_seed=7000, lidar=sg.HDL64 if lidar == "hdl64" else sg.VLP16)
    prevs = [np.ascontiguousarray(s) for s in prevs]
    curs = [np.ascontiguousarray(s) for s in curs]
    cp, keep1 = clouds_of(mode, lidar, prevs)
    cc, keep2 = clouds_of(mode, lidar, curs)
    e = loam.Engine(loam.default_config(**CFG[lidar]))
    set_mode(e, mode)
    bp, bc = [cp[i % distinct] for i in range(P)], [cc[i % distinct] for i in range(P)]
    e.batch_upload(bp, bc)
    e.batch_run()
    e.sync()
    e.set_profiling(True)
    for _ in range(steps):
        e.batch_run()
    e.sync()
    k = e.kernel_times()
    e.close()
    ms, launches = k["k_sr_ring_sort"]
    return {"what": "sort", "mode": mode, "lidar": lidar, "problems": P, "k_sr_ring_sort_ms_per_step": ms / max(launches, 1),
            "k_sr_features_ms_per_step": k["k_sr_features"][0] / max(k["k_sr_features"][1], 1)}


def push(mode, lanes=64, reps=8):
    sweeps = [np.ascontiguousarray(s) for s in sg.stream_sweeps(2, 1)]
    ci, keep = clouds_of(mode, "vlp16", sweeps)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    out = {"what": "push", "mode": mode, "lanes": lanes}
    for form in ("host", "device"):
        e = loam.Engine(loam.default_config(system_delay=0))
        set_mode(e, mode)
        e.lanes_open(lanes, 1 << 16)
        c = ci[1]
        dev = ctypes.c_void_p()
        if form == "device":
            nbytes = c.count * c.stride_bytes
            assert hip.hipMalloc(ctypes.byref(dev), nbytes) == 0
            assert hip.hipMemcpy(dev, c.data, nbytes, 1) == 0
        t = []
        for k in range(reps + 2):
            t0 = time.perf_counter()
            if form == "host":
                e.lanes_push([c] * lanes, stamp=0.1 * k)
            else:
                e.lanes_push_device([(dev.value, c.count, c.stride_bytes)] * lanes, stamp=0.1 * k)
            t.append(time.perf_counter() - t0)
            e.lanes_pull()
        e.lanes_close()
        e.close()
        if dev.value:
            hip.hipFree(dev)
        out[form + "_push_ms"] = float(np.median(t[2:]) * 1e3)   # (the first step is inside systemDelay, the second allocates)
    return out


if __name__ == "__main__":
    if sys.argv[1] == "sort":
        print(json.dumps(sort(sys.argv[2], sys.argv[3], int(sys.argv[4]))))
    else:
        print(json.dumps(push(sys.argv[2])))
