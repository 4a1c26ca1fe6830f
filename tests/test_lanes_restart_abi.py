"""loam_lanes_restart at the C-ABI boundary, without a GPU: the symbol exists and is listed, the
header's declaration agrees with the ctypes argument types, and a null context or a null
wait_steps is refused without touching the output."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params(name):
    """the C parameter types of `int name(...)` in the header, comments and names dropped"""
    h = open(os.path.join(ROOT, "include", "loam", "loam.h")).read()
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", h, flags=re.S)
    assert m, name
    out = []
    for prm in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        prm = " ".join(prm.split())
        ptr = re.fullmatch(r"(.*\*)\s*\w+", prm)
        out.append(ptr.group(1).strip() if ptr else prm.rsplit(" ", 1)[0])
    return [re.sub(r"\s*\*", " *", t) for t in out]


def test_symbol_exported(loam):
    assert hasattr(loam.lib(), "loam_lanes_restart")
    assert "loam_lanes_restart" in loam.EXPORTS


def test_header_matches_ctypes(loam):
    mirror = {"loam_ctx *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "uint32_t *": ctypes.POINTER(ctypes.c_uint32)}
    params = _params("loam_lanes_restart")
    assert params == ["loam_ctx *", "uint32_t", "uint32_t *"]
    assert list(loam.lib().loam_lanes_restart.argtypes) == [mirror[t] for t in params]


def test_null_arguments_are_invalid(loam):
    L = loam.lib()
    w = ctypes.c_uint32(77)
    assert L.loam_lanes_restart(None, 0, ctypes.byref(w)) == loam.LOAM_E_INVAL
    assert L.loam_last_error()
    assert w.value == 77


def test_engine_has_the_method(loam):
    assert callable(loam.Engine.lanes_restart)
