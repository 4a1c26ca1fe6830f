"""loam_lanes_clouds / loam_lanes_clouds_device at the C-ABI boundary, without a GPU:
both symbols are exported and listed, the diagnostic hook is present, the header's prototypes and
loam_lanes_clouds_out agree with the ctypes argument types and Structure (nine loam_batch_cloud of 32
bytes), null arguments are LOAM_E_INVAL and write nothing, Engine has the methods, and
the host-only chunk planner (csrc/lanes_clouds_plan.hpp) passes its edges in a stand-alone program
under AddressSanitizer / UBSan (nothing loaded into Python is sanitized)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("loam_lanes_clouds", "loam_lanes_clouds_device")
HOOK = "loam_dev_lanes_pack"
CLOUDS = ("full", "sharp", "less_sharp", "flat", "less_flat", "corner_last", "surf_last", "full_end", "registered")


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


def test_symbols_exported_and_hook_present(loam):
    for name in NAMES:
        assert hasattr(loam.lib(), name) and name in loam.EXPORTS
    assert hasattr(loam.lib(), HOOK) and HOOK not in loam.EXPORTS
    hooks = open(os.path.join(ROOT, "loam_velodyne-1_amd", "csrc", "dev_hooks.h")).read()
    assert re.search(r"\bint\s+" + HOOK + r"\s*\(", hooks)
    assert re.search(r"#define\s+LOAM_DEV_LANES_PACK_TILE\s+1024\b", hooks)


def test_header_matches_ctypes(loam):
    P = ctypes.POINTER
    mirror = {"loam_ctx *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "const uint32_t *": P(ctypes.c_uint32),
              "loam_lanes_clouds_out *": P(loam.LanesCloudsOut), "void *": ctypes.c_void_p}
    host = _params(NAMES[0])
    assert host == ["loam_ctx *", "uint32_t", "const uint32_t *", "loam_lanes_clouds_out *"]
    assert _params(NAMES[1]) == host + ["void *"]
    for name in NAMES:
        assert list(getattr(loam.lib(), name).argtypes) == [mirror[t] for t in _params(name)]


def test_struct_layout(loam):
    h = _header()
    assert re.search(r"#define\s+LOAM_LANE_CLOUDS\s+9\b", h)
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*loam_lanes_clouds_out\s*;", h)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        f = re.fullmatch(r"loam_batch_cloud (.*)", decl)
        assert f, decl
        names += [n.strip() for n in f.group(1).split(",")]
    assert tuple(names) == CLOUDS == loam.LANE_CLOUDS
    assert [n for n, _ in loam.LanesCloudsOut._fields_] == names
    assert all(t is loam.BatchCloud for _, t in loam.LanesCloudsOut._fields_)
    assert ctypes.sizeof(loam.BatchCloud) == 32 and ctypes.sizeof(loam.LanesCloudsOut) == 9 * 32
    assert [getattr(loam.LanesCloudsOut, n).offset for n in names] == [32 * i for i in range(9)]


def test_null_arguments_are_invalid(loam):
    """(lanes that are not open need a context, so a GPU: tests/test_gpu_lanes_clouds.py test_protocol)"""
    L = loam.lib()
    lane = (ctypes.c_uint32 * 1)(0)
    out = loam.LanesCloudsOut()
    ctypes.memset(ctypes.byref(out), 0xa5, ctypes.sizeof(out))
    before = bytes(out)
    assert L.loam_lanes_clouds(None, 1, lane, ctypes.byref(out)) == loam.LOAM_E_INVAL
    assert L.loam_last_error()
    assert L.loam_lanes_clouds(None, 1, None, None) == loam.LOAM_E_INVAL
    assert L.loam_lanes_clouds_device(None, 1, lane, ctypes.byref(out), None) == loam.LOAM_E_INVAL
    assert L.loam_lanes_clouds_device(None, 1, None, None, None) == loam.LOAM_E_INVAL
    assert bytes(out) == before
    hook = getattr(L, HOOK)
    hook.argtypes = [ctypes.c_int, ctypes.c_int32] + [ctypes.c_void_p] * 4 + [ctypes.c_int32] + [ctypes.c_void_p] * 2 + \
        [ctypes.c_uint64, ctypes.c_void_p]
    assert hook(0, 1, None, None, None, None, 1, None, None, 0, None) == loam.LOAM_E_INVAL


def test_engine_has_the_methods(loam):
    assert callable(getattr(loam.Engine, "lanes_clouds"))
    assert callable(getattr(loam.Engine, "lanes_clouds_device"))
    assert callable(getattr(loam.Engine, "lanes_registered"))  # stays


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_chunk_planner_under_sanitizers(tmp_path):
    """csrc/lanes_clouds_plan.hpp in a stand-alone program under AddressSanitizer / UBSan
    (tests/lanes_clouds_plan_check.cpp): staging sizes 1, 7 and 64 points, empty lanes, a lane of exactly
    the staging and one point more (refused), 100 000 random tables against a restatement"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "lanes_clouds_plan_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fsanitize=address,undefined", "-o", exe, os.path.join(ROOT, "tests", "lanes_clouds_plan_check.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    cases, wrong = map(int, r.stdout.split())
    assert cases > 100000 and wrong == 0
