"""loam_lanes_map_import at the C-ABI boundary, without a GPU: the symbol exists and is listed, the
header's declaration agrees with the ctypes argument types, a null context, lane list or map is
refused without touching `dropped`, and the lane list's host-side check (lanes.hpp
lanes_list_check) reads its arrays inside their bounds (tests/lanes_list_check.cpp, a stand-alone
host program built with AddressSanitizer and UBSan)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "loam_lanes_map_import"


def _params(name):
    """the C parameter types of `int name(...)` in the header, comments and names dropped"""
    h = open(os.path.join(ROOT, "include", "loam", "loam.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", h, flags=re.S)
    assert m, name
    out = []
    for prm in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        prm = " ".join(prm.split())
        arr = re.fullmatch(r"(.*\S)\s+\w+\[\d*\]", prm)  # `uint64_t dropped[2]` is a pointer parameter
        ptr = re.fullmatch(r"(.*\*)\s*\w+", prm)
        out.append(arr.group(1) + " *" if arr else ptr.group(1).strip() if ptr else prm.rsplit(" ", 1)[0])
    return [re.sub(r"\s*\*", " *", t) for t in out]


def test_symbol_exported(loam):
    assert hasattr(loam.lib(), NAME)
    assert NAME in loam.EXPORTS


def test_header_matches_ctypes(loam):
    P = ctypes.POINTER
    mirror = {"loam_ctx *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "const uint32_t *": P(ctypes.c_uint32),
              "const loam_map *": P(loam.Map), "const loam_pose6 *": P(loam.Pose6), "uint64_t *": P(ctypes.c_uint64)}
    params = _params(NAME)
    assert params == ["loam_ctx *", "uint32_t", "const uint32_t *", "const loam_map *", "const loam_pose6 *",
                      "uint64_t *"]
    assert list(getattr(loam.lib(), NAME).argtypes) == [mirror[t] for t in params]


def test_null_arguments_are_invalid(loam):
    f = getattr(loam.lib(), NAME)
    m = loam.Map()
    lane = (ctypes.c_uint32 * 1)(0)
    fake = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(8)))  # never dereferenced
    for ctx, lanes, mp in ((None, lane, ctypes.byref(m)), (fake, None, ctypes.byref(m)), (fake, lane, None)):
        dropped = (ctypes.c_uint64 * 2)(77, 78)
        assert f(ctx, 1, lanes, mp, None, dropped) == loam.LOAM_E_INVAL
        assert loam.lib().loam_last_error()
        assert (dropped[0], dropped[1]) == (77, 78)


def test_engine_has_the_method(loam):
    assert callable(loam.Engine.lanes_map_import)


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_lane_list_check_stays_in_bounds(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "lanes_list_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fsanitize=address,undefined", "-o", exe, os.path.join(ROOT, "tests", "lanes_list_check.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lists, wrong = map(int, r.stdout.split())
    assert lists > 10000 and wrong == 0
