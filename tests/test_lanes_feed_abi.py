"""loam_lanes_push_device at the C-ABI boundary, without a GPU: the symbol exists and
is listed, the header's declaration and flag values agree with the ctypes binding, null arguments are
LOAM_E_INVAL, the wrapper refuses a bad sweep object or a missing stream before it calls the library,
the diagnostic hook is exported (and no part of the public C-ABI), and the planning arithmetic
(lanes_feed_plan.hpp lanes_feed_plan) holds in a stand-alone program under AddressSanitizer / UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_lanes_score_abi import _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "loam_lanes_push_device"
HOOK = "loam_dev_lanes_gather"
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


class _Dev:
    """an object with __cuda_array_interface__ and nothing else (what a torch tensor on the GPU exposes)"""

    def __init__(self, shape, typestr="<f4", strides=None, ptr=0x7f0000001000):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3,
                                         "strides": strides}


def test_symbol_exported(loam):
    assert hasattr(loam.lib(), NAME)
    assert NAME in loam.EXPORTS
    for name in ("lanes_push_device", "lanes_step_device"):
        assert callable(getattr(loam.Engine, name)), name
    assert hasattr(loam.lib(), HOOK)
    assert HOOK not in loam.EXPORTS  # (csrc/dev_hooks.h, as the other hooks)


def test_header_matches_ctypes(loam):
    P = ctypes.POINTER
    mirror = {"loam_ctx *": ctypes.c_void_p, "const double *": P(ctypes.c_double), "const loam_cloud_in *": P(loam.CloudIn),
              "void *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32}
    params = _params(NAME)
    assert params == ["loam_ctx *", "const double *", "const loam_cloud_in *", "void *", "uint32_t"]
    assert list(getattr(loam.lib(), NAME).argtypes) == [mirror[t] for t in params]
    header = open(os.path.join(ROOT, "include", "loam", "loam.h")).read()
    flags = {k: int(v) for k, v in re.findall(r"#define (LOAM_FEED_[A-Z]+)\s+(\d+)", header)}
    assert flags == {"LOAM_FEED_WAIT": loam.FEED_WAIT, "LOAM_FEED_RELEASE": loam.FEED_RELEASE} == \
        {"LOAM_FEED_WAIT": 1, "LOAM_FEED_RELEASE": 2}
    assert ctypes.sizeof(loam.CloudIn) == 16


def test_null_arguments_are_invalid(loam):
    L = loam.lib()
    t = (ctypes.c_double * 1)(0.0)
    a = (loam.CloudIn * 1)()
    assert L.loam_lanes_push_device(None, t, a, None, 0) == loam.LOAM_E_INVAL
    assert L.loam_last_error()
    assert L.loam_lanes_push_device(None, None, a, None, 0) == loam.LOAM_E_INVAL
    assert L.loam_lanes_push_device(None, t, None, None, 3) == loam.LOAM_E_INVAL


def test_hook_refuses_bad_arguments_and_has_no_cpu_path(loam):
    f = getattr(loam.lib(), HOOK)
    f.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    a = (loam.CloudIn * 2)()
    out, n = np.zeros((2, 8, 4), np.uint32), np.zeros(2, np.int32)
    INVAL = loam.LOAM_E_INVAL
    assert f(0, 2, 8, None, out.ctypes.data, n.ctypes.data) == INVAL
    assert f(0, 2, 8, a, None, n.ctypes.data) == INVAL
    assert f(0, 2, 8, a, out.ctypes.data, None) == INVAL
    assert f(0, 0, 8, a, out.ctypes.data, n.ctypes.data) == INVAL
    assert f(0, loam.LANES_MAX + 1, 8, a, out.ctypes.data, n.ctypes.data) == INVAL
    assert f(0, 2, 0, a, out.ctypes.data, n.ctypes.data) == INVAL
    assert f(0, 2, (1 << 22) + 1, a, out.ctypes.data, n.ctypes.data) == INVAL
    # two empty lanes: nothing to read; without a GPU there is no CPU path
    assert f(0, 2, 8, a, out.ctypes.data, n.ctypes.data) in (0, loam.LOAM_E_HIP)


def _eng(loam):
    """an Engine of two lanes without a context (no `h`): the wrapper must refuse before it reaches the library"""
    e = object.__new__(loam.Engine)
    e.n_lanes = 2
    return e


@pytest.mark.parametrize("bad", [
    _Dev((100, 4), "<f8"),              # dtype
    _Dev((100, 4), "<i4"),
    _Dev((400,)),                       # rank
    _Dev((10, 10, 4)),
    _Dev((100, 2)),                     # fewer than 3 columns
    _Dev((100, 4), strides=(4, 400)),   # column stride (a transposed view)
    _Dev((100, 4), strides=(32, 8)),    # every second column
    _Dev((100, 4), strides=(-16, 4)),   # a reversed view
    np.zeros((100, 4), np.float32),     # host memory: no __cuda_array_interface__
    None,
])
def test_wrapper_refuses_a_bad_sweep_object(loam, bad):
    good = _Dev((100, 4))
    with pytest.raises(ValueError):
        loam.Engine.lanes_push_device(_eng(loam), [good, bad])
    with pytest.raises(ValueError):
        loam.Engine.lanes_step_device(_eng(loam), [bad, good])


def test_wrapper_refuses_a_wrong_lane_count_and_a_missing_stream(loam):
    good = _Dev((100, 4))
    with pytest.raises(ValueError):
        loam.Engine.lanes_push_device(_eng(loam), [good])
    with pytest.raises(ValueError):
        loam.Engine.lanes_push_device(_eng(loam), [good, good], stamp=[0.0, 0.1, 0.2])
    for kw in ({"wait": True}, {"release": True}, {"wait": True, "release": True}):
        with pytest.raises(ValueError):
            loam.Engine.lanes_push_device(_eng(loam), [good, good], **kw)
        with pytest.raises(ValueError):
            loam.Engine.lanes_step_device(_eng(loam), [good, good], **kw)


def test_wrapper_reads_the_array_interface(loam):
    c = loam._cloud_in_device(_Dev((100, 4)))
    assert (c.data, c.count, c.stride_bytes) == (0x7f0000001000, 100, 16)
    c = loam._cloud_in_device(_Dev((50, 3), strides=(32, 4), ptr=0x7f0000001004))  # the xyz columns of 32-byte records
    assert (c.data, c.count, c.stride_bytes) == (0x7f0000001004, 50, 32)
    c = loam._cloud_in_device((0x7f0000002000, 7, 20))
    assert (c.data, c.count, c.stride_bytes) == (0x7f0000002000, 7, 20)
    c = loam._cloud_in_device((0, 0, 16))  # a retiring lane
    assert (c.data, c.count) == (None, 0)
    ready = loam.CloudIn(0x10, 1, 12)
    assert loam._cloud_in_device(ready) is ready


@pytest.mark.skipif(not os.path.exists(CLANG) and shutil.which("g++") is None, reason="no host C++ compiler")
def test_plan_arithmetic_under_sanitizers(tmp_path):
    """lanes_feed_plan.hpp lanes_feed_plan in a stand-alone program under AddressSanitizer / UBSan
    (tests/lanes_feed_plan_check.cpp), compiled as plain C++ (the header needs no HIP): no range wraps,
    nothing is written past S entries or on a refusal"""
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("g++")
    exe = str(tmp_path / "lanes_feed_plan_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "lanes_feed_plan_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    cases, wrong, accepted = map(int, r.stdout.split())
    assert cases > 300000 and wrong == 0 and accepted > 100000 and cases - accepted > 30000
