"""loam_dev_od_nn_* (csrc/dev_hooks.h) at the library boundary, without a GPU: the three symbols
are exported (and are no part of the public C-ABI), and _run refuses sizes out of range, a seed
outside the cloud and null pointers with LOAM_E_INVAL."""
import ctypes

import numpy as np

import od_nn_hook


def test_symbols_exported(loam):
    lib = loam.lib()
    for n in od_nn_hook.NAMES:
        assert hasattr(lib, n), n
        assert n not in loam.EXPORTS


def test_create_refuses_null_and_has_no_cpu_path(loam):
    lib = od_nn_hook.bind(loam.lib())
    assert lib.loam_dev_od_nn_create(0, None) == loam.LOAM_E_INVAL
    assert lib.loam_dev_od_nn_destroy(None) == loam.LOAM_E_INVAL
    h = ctypes.c_void_p()
    rc = lib.loam_dev_od_nn_create(0, ctypes.byref(h))
    if rc == 0:  # a GPU is present
        assert h and lib.loam_dev_od_nn_destroy(h) == 0
    else:
        assert rc == loam.LOAM_E_HIP and not h


def _job(n_cloud, n_queries, seeds=None, cloud=True, queries=True):
    c = np.zeros((max(n_cloud, 1), 4), np.float32)
    q = np.zeros((max(n_queries, 1), 4), np.float32)
    j = od_nn_hook.OdNnJob()
    j.cloud = c.ctypes.data if cloud else None
    j.queries = q.ctypes.data if queries else None
    j.n_cloud, j.n_queries = n_cloud, n_queries
    keep = [c, q]
    if seeds is not None:
        s = np.ascontiguousarray(seeds, np.int32)
        j.seeds = s.ctypes.data
        keep.append(s)
    return j, keep


def test_run_rejects_bad_arguments(loam):
    """(the argument checks come before the handle is used: a handle that is never dereferenced
    stands in for one where no GPU is present)"""
    lib = od_nn_hook.bind(loam.lib())
    out =[np.zeros(od_nn_hook.MAX_QUERIES, np.uint64) for _ in range(3)] + [np.zeros(od_nn_hook.MAX_QUERIES, np.int32)]
    ptrs = [o.ctypes.data for o in out]
    h = ctypes.c_void_p()
    real = lib.loam_dev_od_nn_create(0, ctypes.byref(h)) == 0
    if not real:
        dummy = np.zeros(64, np.uint64)
        h = ctypes.c_void_p(dummy.ctypes.data)
    INVAL = loam.LOAM_E_INVAL
    try:
        bad = [_job(0, 4), _job(od_nn_hook.MAX_CLOUD + 1, 4), _job(4, 0), _job(4, od_nn_hook.MAX_QUERIES + 1),
               _job(4, 2, seeds=[0, 4]), _job(4, 2, seeds=[-2, 0]), _job(4, 2, cloud=False), _job(4, 2, queries=False)]
        for j, keep in bad:
            assert lib.loam_dev_od_nn_run(h, ctypes.byref(j), *ptrs) == INVAL
        j, keep = _job(4, 2, seeds=[-1, 3])
        assert lib.loam_dev_od_nn_run(None, ctypes.byref(j), *ptrs) == INVAL
        assert lib.loam_dev_od_nn_run(h, None, *ptrs) == INVAL
        assert lib.loam_dev_od_nn_run(h, ctypes.byref(j), None, ptrs[1], ptrs[2], ptrs[3]) == INVAL
        assert lib.loam_dev_od_nn_run(h, ctypes.byref(j), ptrs[0], None, ptrs[2], ptrs[3]) == INVAL
        assert lib.loam_dev_od_nn_run(h, ctypes.byref(j), ptrs[0], ptrs[1], ptrs[2], None) == INVAL
    finally:
        if real:
            lib.loam_dev_od_nn_destroy(h)
