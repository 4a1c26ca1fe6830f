"""loam_lanes_* at the C-ABI boundary, without a GPU: the six symbols exist, are listed and refuse a
null context without touching their outputs, and the ctypes mirror of loam_lane_out has the layout
the header declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ("loam_lanes_open", "loam_lanes_push", "loam_lanes_pull", "loam_lanes_registered", "loam_lanes_map_export",
           "loam_lanes_close")
# C type -> (size, alignment) of a loam_lane_out member
C_SIZES = {"int32_t": (4, 4), "uint32_t": (4, 4), "loam_pose6": (24, 4)}


def _header():
    return open(os.path.join(ROOT, "include", "loam", "loam.h")).read()


def _lane_out_fields(h):
    """(C type, field) of every member of loam_lane_out in declaration order (`type a, b;` lines)"""
    end = h.index("} loam_lane_out;")
    body = h[h.rindex("typedef struct {", 0, end):end]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.fullmatch(r"(int32_t|uint32_t|loam_pose6)\s+([a-z_]+(?:\s*,\s*[a-z_]+)*)", decl)
        assert m, decl
        fields += [(m.group(1), n.strip()) for n in m.group(2).split(",")]
    return fields


def test_symbols_exported(loam):
    for n in SYMBOLS:
        assert hasattr(loam.lib(), n), n
        assert n in loam.EXPORTS, n


def test_lanes_max_matches_header(loam):
    assert int(re.search(r"#define LOAM_LANES_MAX (\d+)", _header()).group(1)) == loam.LANES_MAX == 1024


def test_lane_out_layout_matches_header(loam):
    fields = _lane_out_fields(_header())
    assert [n for _, n in fields] == ["status", "published", "mapped", "od_iters", "mp_iters", "od_sum", "aft", "bef",
                                      "n_registered"]
    assert [n for n, _ in loam.LaneOut._fields_] == [n for _, n in fields]
    mirror = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "loam_pose6": loam.Pose6}
    assert ctypes.sizeof(loam.Pose6) == 24
    off = 0
    for (t, n), (_, ct) in zip(fields, loam.LaneOut._fields_):
        assert ct is mirror[t], n
        size, align = C_SIZES[t]
        off = (off + align - 1) // align * align
        assert getattr(loam.LaneOut, n).offset == off, n
        off += size
    assert off == 96
    assert ctypes.sizeof(loam.LaneOut) == 96
    assert tuple(n for n, _ in loam.LaneOut._fields_) == loam.LANE_KEYS


def test_null_context_is_invalid(loam):
    L = loam.lib()
    inval = loam.LOAM_E_INVAL
    assert L.loam_lanes_open(None, 4, 1 << 17) == inval
    assert L.loam_last_error()
    raw = (loam.CloudIn * 1)()
    assert L.loam_lanes_push(None, 0.0, raw) == inval
    out = (loam.LaneOut * 2)()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    before = bytes(out)
    assert L.loam_lanes_pull(None, out) == inval
    assert bytes(out) == before
    cloud = loam.CloudOut(None, 77, 0)
    assert L.loam_lanes_registered(None, 0, ctypes.byref(cloud)) == inval
    assert (cloud.pts, cloud.count, cloud.capacity) == (None, 77, 0)
    m = loam.Map()
    ctypes.memset(ctypes.byref(m), 0x5A, ctypes.sizeof(m))
    before = bytes(m)
    assert L.loam_lanes_map_export(None, 0, ctypes.byref(m)) == inval
    assert bytes(m) == before
    assert L.loam_lanes_close(None) == inval
    assert L.loam_last_error()
