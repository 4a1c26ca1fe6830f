"""loam_lanes_imu / loam_lanes_push_stamped / loam_lanes_imu_trans at the C-ABI boundary, without a
GPU: the symbols exist and are listed, the header's declarations agree with the ctypes argument
types, and a null context is refused without touching the outputs."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("loam_lanes_imu", "loam_lanes_push_stamped", "loam_lanes_imu_trans")


def _header():
    return open(os.path.join(ROOT, "include", "loam", "loam.h")).read()


def _params(h, name):
    """the C parameter types of `int name(...)` in the header, comments and names dropped; an
    array parameter is the pointer it decays to"""
    m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", h, flags=re.S)
    assert m, name
    out = []
    for prm in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","):
        prm = " ".join(prm.split())
        arr = re.fullmatch(r"(.*?)\s*\w+\s*\[\d*\]", prm)
        if arr:
            out.append(arr.group(1).strip() + " *")
            continue
        ptr = re.fullmatch(r"(.*\*)\s*\w+", prm)
        out.append(ptr.group(1).strip() if ptr else prm.rsplit(" ", 1)[0])
    return [re.sub(r"\s*\*", " *", t) for t in out]


def test_symbols_exported(loam):
    for n in SYMBOLS:
        assert hasattr(loam.lib(), n), n
        assert n in loam.EXPORTS, n


def test_header_matches_ctypes(loam):
    P = ctypes.POINTER
    mirror = {"loam_ctx *": ctypes.c_void_p, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double,
              "const double *": P(ctypes.c_double), "const loam_cloud_in *": P(loam.CloudIn), "float *": P(ctypes.c_float)}
    h = _header()
    want = {"loam_lanes_imu": ["loam_ctx *", "uint32_t", "double", "const double *", "const double *"],
            "loam_lanes_push_stamped": ["loam_ctx *", "const double *", "const loam_cloud_in *"],
            "loam_lanes_imu_trans": ["loam_ctx *", "float *"]}
    for n in SYMBOLS:
        params = _params(h, n)
        assert params == want[n], (n, params)
        assert list(getattr(loam.lib(), n).argtypes) == [mirror[t] for t in params], n
    # loam_lanes_push keeps its signature
    assert _params(h, "loam_lanes_push") == ["loam_ctx *", "double", "const loam_cloud_in *"]
    assert list(loam.lib().loam_lanes_push.argtypes) == [ctypes.c_void_p, ctypes.c_double, P(loam.CloudIn)]


def test_null_context_is_invalid(loam):
    L = loam.lib()
    inval = loam.LOAM_E_INVAL
    q = (ctypes.c_double * 4)(0, 0, 0, 1)
    a = (ctypes.c_double * 3)(0, 0, 9.81)
    assert L.loam_lanes_imu(None, 0, 0.0, q, a) == inval
    assert L.loam_last_error()
    raw = (loam.CloudIn * 1)()
    t = (ctypes.c_double * 1)(0.0)
    assert L.loam_lanes_push_stamped(None, t, raw) == inval
    out = (ctypes.c_float * 24)(*([7.0] * 24))
    assert L.loam_lanes_imu_trans(None, out) == inval
    assert list(out) == [7.0] * 24


def test_engine_has_the_methods(loam):
    for n in ("lanes_imu", "lanes_imu_trans", "lanes_push", "lanes_step"):
        assert callable(getattr(loam.Engine, n)), n
