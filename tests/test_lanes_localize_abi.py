"""loam_lanes_localize at the C-ABI boundary, without a GPU: the symbol exists and is
listed, the header's declaration agrees with the ctypes argument types, a null context is
LOAM_E_INVAL with `out` untouched, the wrappers refuse a bad shape before they call the library, and
the planning arithmetic (loc_plan.hpp lanes_localize_plan) holds in a stand-alone program under
AddressSanitizer / UBSan."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_lanes_score_abi import _Never, _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "loam_lanes_localize"
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_symbol_exported(loam):
    assert hasattr(loam.lib(), NAME)
    assert NAME in loam.EXPORTS
    for name in ("lanes_localize", "lanes_relocalize"):
        assert callable(getattr(loam.Engine, name)), name


def test_header_matches_ctypes(loam):
    P = ctypes.POINTER
    mirror = {"loam_ctx *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "const uint32_t *": P(ctypes.c_uint32),
              "const loam_pose6 *": P(loam.Pose6), "loam_localize_result *": P(loam.LocalizeResult)}
    params = _params(NAME)
    assert params == ["loam_ctx *", "uint32_t", "const uint32_t *", "uint32_t", "const loam_pose6 *", "const loam_pose6 *",
                      "loam_localize_result *"]
    assert list(getattr(loam.lib(), NAME).argtypes) == [mirror[t] for t in params]
    assert ctypes.sizeof(loam.LocalizeResult) == 60 and loam._LOC_DTYPE.itemsize == 60


def test_null_context_is_invalid(loam):
    L = loam.lib()
    lane = (ctypes.c_uint32 * 1)(0)
    pose = (loam.Pose6 * 2)()
    out = (loam.LocalizeResult * 2)()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    before = bytes(out)
    assert L.loam_lanes_localize(None, 1, lane, 2, pose, pose, out) == loam.LOAM_E_INVAL
    assert L.loam_last_error()
    assert L.loam_lanes_localize(None, 1, lane, 2, pose, None, out) == loam.LOAM_E_INVAL
    assert bytes(out) == before


@pytest.mark.parametrize("lanes, shape", [([0, 1], (3, 5, 6)), ([0, 1], (2, 5, 5)), ([0, 1], (6,)), ([0], (2, 2, 2, 6)),
                                          ([0, 1, 2], (5, 7)), ([0, 1], (1, 5, 6)), ([0, 1], (2, 0, 6))])
def test_wrapper_refuses_a_bad_shape(loam, lanes, shape):
    with pytest.raises(ValueError):
        loam.Engine.lanes_localize(_Never(), lanes, np.zeros(shape, np.float32))
    with pytest.raises(ValueError):  # a good aft, the bad shape in bef
        loam.Engine.lanes_localize(_Never(), lanes, np.zeros((len(lanes), 5, 6), np.float32), np.zeros(shape, np.float32))
    with pytest.raises(ValueError):
        loam.Engine.lanes_relocalize(_Never(), lanes, np.zeros(shape, np.float32), np.zeros((4, 6), np.float32), refine=2)


def test_wrapper_refuses_aft_and_bef_of_different_k(loam):
    with pytest.raises(ValueError):
        loam.Engine.lanes_localize(_Never(), [0, 1], np.zeros((2, 3, 6), np.float32), np.zeros((2, 4, 6), np.float32))
    with pytest.raises(ValueError):
        loam.Engine.lanes_localize(_Never(), [0, 1], np.zeros((2, 3, 6), np.float32), np.zeros((4, 6), np.float32))


def test_relocalize_refuses_a_bad_refine(loam):
    poses, od_sum = np.zeros((2, 3, 6), np.float32), np.zeros((4, 6), np.float32)
    for bad in (-1, loam.LOCALIZE_MAX // 2 + 1, loam.LOCALIZE_MAX + 1):
        with pytest.raises(ValueError):
            loam.Engine.lanes_relocalize(_Never(), [0, 1], poses, od_sum, refine=bad)
    with pytest.raises(ValueError):
        loam.Engine.lanes_relocalize(_Never(), [0, 1], poses, np.zeros((3, 6), np.float32), refine=1)


@pytest.mark.skipif(not os.path.exists(CLANG) and shutil.which("g++") is None, reason="no host C++ compiler")
def test_plan_arithmetic_under_sanitizers(tmp_path):
    """loc_plan.hpp lanes_localize_plan in a stand-alone program under AddressSanitizer / UBSan
    (tests/lanes_localize_plan_check.cpp), compiled as plain C++ (the header needs no HIP): no product
    overflows, nothing is written past n entries or on a refusal"""
    cxx = CLANG if os.path.exists(CLANG) else shutil.which("g++")
    exe = str(tmp_path / "lanes_localize_plan_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(ROOT, "tests", "lanes_localize_plan_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    cases, wrong, accepted = map(int, r.stdout.split())
    assert cases > 300000 and wrong == 0 and accepted > 100000
