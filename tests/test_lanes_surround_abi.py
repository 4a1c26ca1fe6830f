"""loam_lanes_surround at the C-ABI boundary, without a GPU: the symbol exists and is listed, the
header's declaration agrees with the ctypes argument types, loam_lanes_cloud's fields agree with
the ctypes mirror in name, order and offset, and a null context or a null out is refused without
touching the caller's struct."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _struct_fields(name):
    """[(C type, field name)] of `typedef struct { ... } name;` in the header"""
    m = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*" + name + r"\s*;", _header(), flags=re.S)
    assert m, name
    out = []
    for decl in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        f = re.fullmatch(r"(.*?)(\s*\*\s*|\s+)(\w+)", decl)
        assert f, decl
        out.append((f.group(1) + (" *" if "*" in f.group(2) else ""), f.group(3)))
    return out


def test_symbol_exported(loam):
    assert hasattr(loam.lib(), "loam_lanes_surround")
    assert "loam_lanes_surround" in loam.EXPORTS


def test_header_matches_ctypes(loam):
    mirror = {"loam_ctx *": ctypes.c_void_p, "loam_lanes_cloud *": ctypes.POINTER(loam.LanesCloud)}
    params = _params("loam_lanes_surround")
    assert params == ["loam_ctx *", "loam_lanes_cloud *"]
    assert list(loam.lib().loam_lanes_surround.argtypes) == [mirror[t] for t in params]


def test_struct_matches_ctypes(loam):
    fields = _struct_fields("loam_lanes_cloud")
    assert fields == [("loam_point *", "pts"), ("uint64_t", "capacity"), ("uint64_t", "count"),
                      ("uint32_t *", "offset"), ("int32_t *", "published")]
    size = {"loam_point *": ctypes.sizeof(ctypes.c_void_p), "uint32_t *": ctypes.sizeof(ctypes.c_void_p),
            "int32_t *": ctypes.sizeof(ctypes.c_void_p), "uint64_t": 8}
    assert [n for n, _ in loam.LanesCloud._fields_] == [n for _, n in fields]
    at = 0
    for t, n in fields:  # (every member is 8 bytes wide and 8-byte aligned: no padding)
        assert getattr(loam.LanesCloud, n).offset == at, n
        assert getattr(loam.LanesCloud, n).size == size[t], n
        at += size[t]
    assert ctypes.sizeof(loam.LanesCloud) == at == 40


def test_null_arguments_are_invalid(loam):
    L = loam.lib()
    off = (ctypes.c_uint32 * 3)(7, 8, 9)
    pub = (ctypes.c_int32 * 2)(5, 6)
    c = loam.LanesCloud(None, 11, 22, ctypes.addressof(off), ctypes.addressof(pub))
    before = bytes(c)
    assert L.loam_lanes_surround(None, ctypes.byref(c)) == loam.LOAM_E_INVAL
    assert L.loam_last_error()
    assert bytes(c) == before and list(off) == [7, 8, 9] and list(pub) == [5, 6]
    # a null out: refused before the context is looked at
    assert L.loam_lanes_surround(ctypes.c_void_p(1), None) == loam.LOAM_E_INVAL
    assert L.loam_last_error()


def test_engine_has_the_method(loam):
    assert callable(loam.Engine.lanes_surround)
