"""loam_lanes_map_commit at the C-ABI boundary, without a GPU: the symbol is exported
and listed, the diagnostic hook is present, the header's prototype and loam_commit_result agree with
the ctypes argument types and Structure, a null context is LOAM_E_INVAL and writes nothing, Engine has
the method, and the host-only check of the lane list (lanes.hpp lanes_commit_check) passes its edges
in a stand-alone program under AddressSanitizer / UBSan (nothing loaded into Python is sanitized)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "loam_lanes_map_commit"
HOOK = "loam_dev_lanes_commit_input"


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


def test_symbol_exported_and_hook_present(loam):
    assert hasattr(loam.lib(), NAME) and NAME in loam.EXPORTS
    assert hasattr(loam.lib(), HOOK) and HOOK not in loam.EXPORTS
    hooks = open(os.path.join(ROOT, "loam_velodyne-1_amd", "csrc", "dev_hooks.h")).read()
    assert re.search(r"\bint\s+" + HOOK + r"\s*\(", hooks)


def test_header_matches_ctypes(loam):
    P = ctypes.POINTER
    mirror = {"loam_ctx *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "const uint32_t *": P(ctypes.c_uint32),
              "loam_commit_result *": P(loam.CommitResult)}
    params = _params(NAME)
    assert params == ["loam_ctx *", "uint32_t", "const uint32_t *", "loam_commit_result *"]
    assert list(getattr(loam.lib(), NAME).argtypes) == [mirror[t] for t in params]


def test_struct_layout(loam):
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*loam_commit_result\s*;", _header())
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        f = re.fullmatch(r"(uint64_t|uint32_t) (\w+)(?:\[(\d+)\])?", decl)
        assert f, decl
        fields.append((f.group(2), f.group(1), int(f.group(3)) if f.group(3) else 0))
    base = {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}
    want = [(n, base[t] * k if k else base[t]) for n, t, k in fields]
    assert [n for n, _ in loam.CommitResult._fields_] == [n for n, _ in want]
    for (n, got), (_, exp) in zip(loam.CommitResult._fields_, want):
        if hasattr(exp, "_length_"):
            assert (got._type_, got._length_) == (exp._type_, exp._length_), n
        else:
            assert got is exp, n
    # natural alignment: three uint64_t pairs, the uint32_t, padding to 8
    assert ctypes.sizeof(loam.CommitResult) == 56
    assert [getattr(loam.CommitResult, n).offset for n, _ in want] == [0, 16, 32, 48]


def test_null_arguments_are_invalid(loam):
    L = loam.lib()
    lane = (ctypes.c_uint32 * 1)(0)
    out = loam.CommitResult()
    ctypes.memset(ctypes.byref(out), 0xa5, ctypes.sizeof(out))
    before = bytes(out)
    assert L.loam_lanes_map_commit(None, 1, lane, ctypes.byref(out)) == loam.LOAM_E_INVAL
    assert L.loam_last_error()
    assert L.loam_lanes_map_commit(None, 1, None, None) == loam.LOAM_E_INVAL
    assert bytes(out) == before
    hook = getattr(L, HOOK)
    hook.argtypes = [ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 5
    assert hook(None, 0, None, None, None, None, None) == loam.LOAM_E_INVAL


def test_engine_has_the_method(loam):
    assert callable(getattr(loam.Engine, "lanes_map_commit"))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                    reason="hipcc not available")
def test_list_check_under_sanitizers(tmp_path):
    """lanes.hpp lanes_commit_check in a stand-alone program under AddressSanitizer / UBSan
    (tests/lanes_commit_check.cpp): no read beyond the list or the S-entry state arrays, every rule
    and their order against a plain restatement"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "lanes_commit_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    "-fsanitize=address,undefined", "-o", exe, os.path.join(ROOT, "tests", "lanes_commit_check.cpp")],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    cases, wrong = map(int, r.stdout.split())
    assert cases > 200000 and wrong == 0
