"""Shared lanes (loam_lanes_open_shared, loam_lanes_set_pose, loam_lanes_localize_info) at the C-ABI
boundary, without a GPU: the symbols exist and are listed, LOAM_LOC_NONE is in the header and in the
package, the header's declarations agree with the ctypes argument types, and a null context is
LOAM_E_INVAL for each of the three."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("loam_lanes_open_shared", "loam_lanes_set_pose", "loam_lanes_localize_info")


def _header():
    return open(os.path.join(ROOT, "include", "loam", "loam.h")).read()


def _params(name):
    """the C parameter types of `int name(...)` in the header, comments and names dropped"""
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", _header(), flags=re.S)
    assert m, name
    out = []
    for prm in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        prm = " ".join(prm.split())
        ptr = re.fullmatch(r"(.*\*)\s*\w+", prm)
        out.append(ptr.group(1).strip() if ptr else prm.rsplit(" ", 1)[0])
    return [re.sub(r"\s*\*", " *", t) for t in out]


def test_symbols_exported(loam):
    for name in NAMES:
        assert hasattr(loam.lib(), name), name
        assert name in loam.EXPORTS, name


def test_loc_none(loam):
    # (defined behind loam_map_localize's own statuses, which tests/test_localize_abi.py lists in full)
    m = re.search(r"#define\s+LOAM_LOC_NONE\s+\(LOAM_LOC_OFFGRID \+ (\d+)\)", _header())
    assert m and loam.LOC_OFFGRID + int(m.group(1)) == loam.LOC_NONE == 3
    assert loam.LOC_NONE not in (loam.LOC_SOLVED, loam.LOC_NO_LM, loam.LOC_OFFGRID)


def test_header_matches_ctypes(loam):
    P = ctypes.POINTER
    mirror = {"loam_ctx *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "const uint32_t *": P(ctypes.c_uint32),
              "const loam_pose6 *": P(loam.Pose6), "loam_localize_result *": P(loam.LocalizeResult)}
    want = {"loam_lanes_open_shared": ["loam_ctx *", "uint32_t", "uint32_t"],
            "loam_lanes_set_pose": ["loam_ctx *", "uint32_t", "const uint32_t *", "const loam_pose6 *", "const loam_pose6 *"],
            "loam_lanes_localize_info": ["loam_ctx *", "loam_localize_result *"]}
    for name in NAMES:
        params = _params(name)
        assert params == want[name], name
        assert list(getattr(loam.lib(), name).argtypes) == [mirror[t] for t in params], name


def test_null_context_is_invalid(loam):
    L = loam.lib()
    lane = (ctypes.c_uint32 * 1)(0)
    pose = (loam.Pose6 * 1)()
    out = (loam.LocalizeResult * 1)()
    before = bytes(out)
    assert L.loam_lanes_open_shared(None, 1, 4096) == loam.LOAM_E_INVAL
    assert L.loam_last_error()
    assert L.loam_lanes_set_pose(None, 1, lane, pose, None) == loam.LOAM_E_INVAL
    assert L.loam_last_error()
    assert L.loam_lanes_localize_info(None, out) == loam.LOAM_E_INVAL
    assert L.loam_last_error()
    assert bytes(out) == before


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_capacity_arithmetic_under_sanitizers(tmp_path):
    """lanes.hpp lanes_shared_check in a stand-alone program under AddressSanitizer / UBSan
    (tests/lanes_shared_check.cpp): no product of the arguments overflows"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "lanes_shared_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fsanitize=address,undefined", "-o", exe, os.path.join(ROOT, "tests", "lanes_shared_check.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cases, wrong = map(int, r.stdout.split())
    assert cases > 100000 and wrong == 0


def test_engine_has_the_methods(loam):
    for name in ("lanes_open_shared", "lanes_set_pose", "lanes_localize_info"):
        assert callable(getattr(loam.Engine, name)), name
