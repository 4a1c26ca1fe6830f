"""loam_dev_sr_ring_of (csrc/dev_hooks.h) at the library boundary, without a GPU: the symbol is
exported (and is no part of the public C-ABI), bad arguments give LOAM_E_INVAL before any device
call, and without a GPU a valid call gives LOAM_E_HIP (no CPU path).  Also the numpy restatement of
ring_id the GPU tests derive their boundaries from: 32 boundaries at the half-integer degrees for
VLP-16, 65 for the 64-ring linear model."""
import numpy as np

import sr_ring_hook as rh


def test_symbol_exported(loam):
    assert hasattr(loam.lib(), rh.NAME)
    assert rh.NAME not in loam.EXPORTS


def _call(f, model, pts, n, outs, **over):
    m = dict(model, **over)
    return f(0, m["n_rings"], m["ring_model"], m["ring_lo_deg"], m["ring_hi_deg"], pts, n, *outs)


def test_rejects_bad_arguments(loam):
    f = rh.bind(loam.lib())
    pts = np.ones((4, 4), np.float32)
    outs = [np.zeros(4, np.int32) for _ in range(3)]
    ptrs = [o.ctypes.data for o in outs]
    INVAL = loam.LOAM_E_INVAL
    assert _call(f, rh.VLP16, None, 4, ptrs) == INVAL
    assert _call(f, rh.VLP16, pts.ctypes.data, 0, ptrs) == INVAL
    assert _call(f, rh.VLP16, pts.ctypes.data, rh.MAX_N + 1, ptrs) == INVAL
    for k in range(3):
        assert _call(f, rh.VLP16, pts.ctypes.data, 4, ptrs[:k] + [None] + ptrs[k + 1:]) == INVAL
    assert _call(f, rh.VLP16, pts.ctypes.data, 4, ptrs, n_rings=1) == INVAL
    assert _call(f, rh.VLP16, pts.ctypes.data, 4, ptrs, n_rings=65) == INVAL
    assert _call(f, rh.VLP16, pts.ctypes.data, 4, ptrs, ring_model=2) == INVAL
    rc = _call(f, rh.VLP16, pts.ctypes.data, 4, ptrs)
    assert rc in (0, loam.LOAM_E_HIP)


def test_boundaries_of_the_restated_ring_id():
    b = rh.true_boundaries(rh.VLP16)
    assert len(b) == 32 and np.allclose(b, np.arange(-15.5, 15.6, 1.0), atol=2e-6)
    assert list(rh.ring_id(rh.VLP16, np.float32([-15.2, -0.6, -0.4, 0.4, 0.6, 15.4, 15.6, -15.6]))) == \
        [0, 14, 15, 15, 1, 15, 16, -1]
    b = rh.true_boundaries(rh.HDL64)
    step = 26.8 / 63
    assert len(b) == 65 and np.allclose(b[1:], -24.8 + (np.arange(64) + 0.5) * step, atol=1e-5)
    assert abs(b[0] - (-24.8 - 1.5 * step)) < 1e-5      # (int) truncates towards zero: ring 0 reaches 1.5 steps down
    assert len(rh.all_boundaries(rh.HDL64)) == 66       # ... and the stated lo - 0.5 step is no boundary
