"""loam_lanes_score at the C-ABI boundary, without a GPU: the symbol exists and is
listed, the header's declaration agrees with the ctypes argument types, a null context is
LOAM_E_INVAL with `out` untouched, the wrappers refuse a bad shape before they call the library, and
the launch arithmetic (score.hpp lanes_score_plan) holds in a stand-alone program under
AddressSanitizer / UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "loam_lanes_score"


def _params(name):
    """the C parameter types of `int name(...)` in the header, comments and names dropped"""
    header = open(os.path.join(ROOT, "include", "loam", "loam.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
    assert m, name
    out = []
    for prm in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        prm = " ".join(prm.split())
        ptr = re.fullmatch(r"(.*\*)\s*\w+", prm)
        out.append(ptr.group(1).strip() if ptr else prm.rsplit(" ", 1)[0])
    return [re.sub(r"\s*\*", " *", t) for t in out]


def test_symbol_exported(loam):
    assert hasattr(loam.lib(), NAME)
    assert NAME in loam.EXPORTS
    for name in ("lanes_score", "lanes_relocalize"):
        assert callable(getattr(loam.Engine, name)), name


def test_header_matches_ctypes(loam):
    P = ctypes.POINTER
    mirror = {"loam_ctx *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float,
              "const uint32_t *": P(ctypes.c_uint32), "const loam_pose6 *": P(loam.Pose6),
              "loam_score_result *": P(loam.ScoreResult)}
    params = _params(NAME)
    assert params == ["loam_ctx *", "uint32_t", "const uint32_t *", "float", "uint32_t", "const loam_pose6 *",
                      "loam_score_result *"]
    assert list(getattr(loam.lib(), NAME).argtypes) == [mirror[t] for t in params]
    assert ctypes.sizeof(loam.ScoreResult) == 32


def test_null_context_is_invalid(loam):
    L = loam.lib()
    lane = (ctypes.c_uint32 * 1)(0)
    pose = (loam.Pose6 * 2)()
    out = (loam.ScoreResult * 2)()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    before = bytes(out)
    assert L.loam_lanes_score(None, 1, lane, 1.0, 2, pose, out) == loam.LOAM_E_INVAL
    assert L.loam_last_error()
    assert bytes(out) == before


class _Never:
    """stands where the Engine's context handle is: the wrappers must raise before they use it"""
    n_lanes = 4

    @property
    def h(self):
        raise AssertionError("the library was called")

    def lanes_set_pose(self, *a, **k):
        raise AssertionError("lanes_set_pose was called")


@pytest.mark.parametrize("lanes, shape", [([0, 1], (3, 5, 6)), ([0, 1], (2, 5, 5)), ([0, 1], (6,)), ([0], (2, 2, 2, 6)),
                                          ([0, 1, 2], (5, 7)), ([0, 1], (1, 5, 6))])
def test_wrapper_refuses_a_bad_shape(loam, lanes, shape):
    with pytest.raises(ValueError):
        loam.Engine.lanes_score(_Never(), lanes, np.zeros(shape, np.float32))
    with pytest.raises(ValueError):
        loam.Engine.lanes_relocalize(_Never(), lanes, np.zeros(shape, np.float32), np.zeros((4, 6), np.float32))


def test_relocalize_refuses_a_bad_od_sum(loam):
    for bad in (np.zeros((3, 6), np.float32), np.zeros(6, np.float32), np.zeros((4, 5), np.float32)):
        with pytest.raises(ValueError):
            loam.Engine.lanes_relocalize(_Never(), [0, 1], np.zeros((2, 3, 6), np.float32), bad)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_plan_arithmetic_under_sanitizers(tmp_path):
    """score.hpp lanes_score_plan in a stand-alone program under AddressSanitizer / UBSan
    (tests/lanes_score_plan_check.cpp): no product overflows, nothing is written past n entries"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "lanes_score_plan_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fsanitize=address,undefined", "-o", exe, os.path.join(ROOT, "tests", "lanes_score_plan_check.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    cases, wrong = map(int, r.stdout.split())
    assert cases > 200000 and wrong == 0
