"""loam_dev_od_assoc_* (csrc/dev_hooks.h) at the library boundary, without a GPU: the three symbols
are exported (and are no part of the public C-ABI), and _run refuses null pointers, sizes, tuning
values, rings, query intensities and seeds out of range with LOAM_E_INVAL before it touches the
handle."""
import ctypes

import numpy as np

import od_assoc_hook as hook


def test_symbols_exported(loam):
    lib = loam.lib()
    for n in hook.NAMES:
        assert hasattr(lib, n), n
        assert n not in loam.EXPORTS


def test_create_refuses_null_and_has_no_cpu_path(loam):
    lib = hook.bind(loam.lib())
    assert lib.loam_dev_od_assoc_create(0, None) == loam.LOAM_E_INVAL
    assert lib.loam_dev_od_assoc_destroy(None) == loam.LOAM_E_INVAL
    h = ctypes.c_void_p()
    rc = lib.loam_dev_od_assoc_create(0, ctypes.byref(h))
    if rc == 0:  # a GPU is present
        assert h and lib.loam_dev_od_assoc_destroy(h) == 0
    else:
        assert rc == loam.LOAM_E_HIP and not h


def _problem(n=4, nq=2, ring=5.25, qw=0.0, **kw):
    c = np.zeros((max(n, 1), 4), np.float32)
    c[:, 3] = ring
    q = np.zeros((max(nq, 1), 4), np.float32)
    q[:, 3] = qw
    d = dict(corner_last=c[:n] if n else c[:0], surf_last=c, corner_q=q[:nq] if nq else q[:0], surf_q=q)
    d.update(kw)
    return d


def test_run_rejects_bad_arguments(loam):
    """(the argument checks come before the handle is used: a handle that is never dereferenced
    stands in for one where no GPU is present)"""
    lib = hook.bind(loam.lib())
    ind = np.zeros((hook.MAX_P, 3, 16), np.int32)
    mono = np.zeros((hook.MAX_P, 2), np.int32)
    rs = np.zeros((hook.MAX_P, 2, hook.RING_TAB), np.int32)
    cnt = np.zeros((hook.MAX_P, 2), np.int32)
    ptrs = [a.ctypes.data for a in (ind, mono, rs, cnt)]
    h = ctypes.c_void_p()
    real = lib.loam_dev_od_assoc_create(0, ctypes.byref(h)) == 0
    if not real:
        dummy = np.zeros(4096, np.uint64)
        h = ctypes.c_void_p(dummy.ctypes.data)
    INVAL = loam.LOAM_E_INVAL
    big = np.zeros((hook.MAX_CLOUD + 1, 4), np.float32)
    bigq = np.zeros((hook.MAX_QUERIES + 1, 4), np.float32)
    seeds = lambda *rows: np.array(rows, np.int32)
    bad = [
        ([_problem()] * (hook.MAX_P + 1), {}),                       # P out of range
        ([_problem(corner_last=np.zeros((0, 4), np.float32))], {}),  # an empty cloud
        ([_problem(surf_last=big)], {}),
        ([_problem(corner_q=bigq)], {}),
        ([_problem(corner_q=np.zeros((0, 4), np.float32), surf_q=np.zeros((0, 4), np.float32))], {}),  # no query
        ([_problem(ring=64.0)], {}), ([_problem(ring=-1.0)], {}), ([_problem(ring=float("nan"))], {}),
        ([_problem(qw=0.5)], {}), ([_problem(qw=-1.0)], {}),         # a query intensity with a fraction
        ([_problem(corner_seeds=seeds([0, 0, 4], [0, 0, 0]))], {}),  # a seed outside the cloud
        ([_problem(surf_seeds=seeds([0, -2, 0], [0, 0, 0]))], {}),
        ([_problem()], dict(od_win_mono=4)), ([_problem()], dict(od_win_mono_min=0)),
        ([_problem()], dict(launch=dict(od_sel_min=0, od_nn_lane=0, od_nn_lane_min=1))),
        ([_problem()], dict(launch=dict(od_sel_min=1, od_nn_lane=3, od_nn_lane_min=1))),
        ([_problem()], dict(launch=dict(od_sel_min=1, od_nn_lane=2, od_nn_lane_min=0))),
        ([_problem()], dict(grid=-1)), ([_problem()], dict(grid=hook.MAX_GRID + 1)),
        ([_problem()], dict(count=2)), ([_problem()], dict(hash_form=3)), ([_problem()], dict(hash_form=-1)),
    ]
    try:
        for problems, kw in bad:
            j, keep = hook.make_job(problems, **kw)
            assert lib.loam_dev_od_assoc_run(h, ctypes.byref(j), *ptrs) == INVAL, (kw, problems[0].keys())
        j, keep = hook.make_job([_problem()])
        j.P = 0
        assert lib.loam_dev_od_assoc_run(h, ctypes.byref(j), *ptrs) == INVAL
        j, keep = hook.make_job([_problem()])
        j.prob = None
        assert lib.loam_dev_od_assoc_run(h, ctypes.byref(j), *ptrs) == INVAL
        for field in ("corner_last", "surf_last", "corner_q", "surf_q"):
            j, keep = hook.make_job([_problem()])
            setattr(j.prob[0], field, None)
            assert lib.loam_dev_od_assoc_run(h, ctypes.byref(j), *ptrs) == INVAL, field
        j, keep = hook.make_job([_problem(corner_seeds=seeds([-1, 3, 0], [0, 0, -1]))])
        assert lib.loam_dev_od_assoc_run(None, ctypes.byref(j), *ptrs) == INVAL
        assert lib.loam_dev_od_assoc_run(h, None, *ptrs) == INVAL
        for k in range(4):
            p = list(ptrs)
            p[k] = None
            assert lib.loam_dev_od_assoc_run(h, ctypes.byref(j), *p) == INVAL
    finally:
        if real:
            lib.loam_dev_od_assoc_destroy(h)
