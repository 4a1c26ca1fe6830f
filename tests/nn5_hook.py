"""ctypes prototypes of the diagnostic 5-NN hook (loam_velodyne-1_amd/csrc/dev_hooks.h:
loam_dev_nn5_create / run / destroy).  Test infrastructure: the package does not bind these."""
import ctypes

import numpy as np

BATCH, STREAM = 0, 1
OVERFLOW, PLAIN = 1, 2       # flags
MAX_MAP, MAX_QUERIES = 16384, 4096
NONE = 0x7fffffff            # the index of an empty place
NAMES = ("loam_dev_nn5_create", "loam_dev_nn5_run", "loam_dev_nn5_destroy")


class Nn5Job(ctypes.Structure):
    _fields_ = [("map", ctypes.c_void_p), ("n_map", ctypes.c_int32),
                ("queries", ctypes.c_void_p), ("n_queries", ctypes.c_int32),
                ("seeds", ctypes.c_void_p), ("distinct", ctypes.c_void_p), ("form", ctypes.c_int32)]


def bind(lib):
    lib.loam_dev_nn5_create.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.loam_dev_nn5_run.argtypes = [ctypes.c_void_p, ctypes.POINTER(Nn5Job)] + [ctypes.c_void_p] * 6
    lib.loam_dev_nn5_destroy.argtypes = [ctypes.c_void_p]
    for n in NAMES:
        getattr(lib, n).restype = ctypes.c_int
    return lib


class Result:
    """flat / plain: (idx int32 [nq][5], dist uint32 [nq][5]); flags [nq]; overflow, plain_count"""

    def __init__(self, flat, plain, flags, counts):
        self.flat, self.plain, self.flags = flat, plain, flags
        self.overflow, self.plain_count = int(counts[0]), int(counts[1])


class Handle:
    def __init__(self, lib, device=0):
        self.lib = bind(lib)
        self.h = ctypes.c_void_p()
        rc = self.lib.loam_dev_nn5_create(device, ctypes.byref(self.h))
        if rc != 0:
            raise RuntimeError(f"loam_dev_nn5_create: {rc}")

    def close(self):
        if self.h:
            self.lib.loam_dev_nn5_destroy(self.h)
            self.h = None

    def run(self, map_xyz, queries_xyz, form, seeds=None, distinct=None):
        def pts4(a):
            a = np.asarray(a, np.float32)
            out = np.zeros((len(a), 4), np.float32)
            out[:, :3] = a[:, :3]
            return out
        m, q = pts4(map_xyz), pts4(queries_xyz)
        nq = len(q)
        j = Nn5Job()
        j.map, j.n_map, j.queries, j.n_queries, j.form = m.ctypes.data, len(m), q.ctypes.data, nq, form
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, np.int32)
            assert seeds.shape == (nq, 5)
            j.seeds = seeds.ctypes.data
        if distinct is not None:
            distinct = np.ascontiguousarray(distinct, np.int32)
            assert distinct.shape == (nq,)
            j.distinct = distinct.ctypes.data
        fi, pi = np.zeros((nq, 5), np.int32), np.zeros((nq, 5), np.int32)
        fd, pd = np.zeros((nq, 5), np.uint32), np.zeros((nq, 5), np.uint32)
        flags, counts = np.zeros(nq, np.int32), np.zeros(2, np.int32)
        rc = self.lib.loam_dev_nn5_run(self.h, ctypes.byref(j), fi.ctypes.data, fd.ctypes.data, pi.ctypes.data,
                                       pd.ctypes.data, flags.ctypes.data, counts.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"loam_dev_nn5_run: {rc}")
        return Result((fi, fd), (pi, pd), flags, counts)
