"""loam_map_export / loam_map_import at the C-ABI boundary, without a GPU: the symbols exist and
refuse a null context, the ctypes mirrors of loam_map_cloud / loam_map have the layout the header
declares, and save_map / load_map round-trip a map dict bit for bit."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"loam_point *": (ctypes.c_void_p, 8), "uint32_t *": (ctypes.c_void_p, 8), "uint64_t": (ctypes.c_uint64, 8),
           "int32_t": (ctypes.c_int32, 4)}


def _header():
    return open(os.path.join(ROOT, "include", "loam", "loam.h")).read()


def _struct_fields(h, name):
    """(C type, field, array length or None) of the one-member-per-line struct `name`"""
    end = h.index("} %s;" % name)
    body = h[h.rindex("typedef struct {", 0, end):end]
    fields = []
    for line in body.splitlines()[1:]:
        line = line.split("/*")[0].strip()
        m = re.match(r"(loam_point \*|uint32_t \*|uint64_t|int32_t|loam_map_cloud|loam_pose6)\s*([a-z_]+)(\[(\d+)\])?;", line)
        if m:
            fields.append((m.group(1), m.group(2), int(m.group(4)) if m.group(4) else None))
    return fields


def test_symbols_exported(loam):
    for n in ("loam_map_export", "loam_map_import"):
        assert hasattr(loam.lib(), n), n
        assert n in loam.EXPORTS


def test_null_context_is_invalid(loam):
    m = loam.Map()
    assert loam.lib().loam_map_export(None, ctypes.byref(m)) == loam.LOAM_E_INVAL
    assert loam.lib().loam_last_error()
    assert loam.lib().loam_map_import(None, ctypes.byref(m), None) == loam.LOAM_E_INVAL
    assert loam.lib().loam_last_error()


def test_map_cloud_layout_matches_header(loam):
    fields = _struct_fields(_header(), "loam_map_cloud")
    assert [n for _, n, _ in fields] == ["pts", "capacity", "count", "cube_offset"]
    assert [(n, C_TYPES[t][0]) for t, n, _ in fields] == list(loam.MapCloud._fields_)
    for i, (n, _) in enumerate(loam.MapCloud._fields_):  # natural alignment of four 8-byte members
        assert getattr(loam.MapCloud, n).offset == 8 * i, n
    assert ctypes.sizeof(loam.MapCloud) == 32
    assert re.search(r"#define LOAM_MAP_CUBES (\d+)", _header()).group(1) == str(loam.MAP_CUBES) == str(21 * 11 * 21)


def test_map_layout_matches_header(loam):
    fields = _struct_fields(_header(), "loam_map")
    assert [n for _, n, _ in fields] == ["corner", "surf", "center", "surround_phase", "aft", "bef"]
    assert [n for n, _ in loam.Map._fields_] == [n for _, n, _ in fields]
    off = 0
    for (t, n, arr), (_, ct) in zip(fields, loam.Map._fields_):
        if t == "loam_map_cloud":
            assert ct is loam.MapCloud
            size, align = 32, 8
        elif t == "loam_pose6":
            assert ct is loam.Pose6 and ctypes.sizeof(loam.Pose6) == 24
            size, align = 24, 4
        else:
            base, size = C_TYPES[t]
            align = size
            if arr:
                assert ct._type_ is base and ct._length_ == arr, n
                size *= arr
            else:
                assert ct is base, n
        off = (off + align - 1) // align * align
        assert getattr(loam.Map, n).offset == off, n
        off += size
    assert off == 128
    assert ctypes.sizeof(loam.Map) == 128
    assert (loam.Map.center.offset, loam.Map.surround_phase.offset, loam.Map.aft.offset, loam.Map.bef.offset) == \
        (64, 76, 80, 104)


def test_save_load_round_trip(loam, tmp_path):
    rng = np.random.default_rng(3)
    bits = rng.integers(0, 2 ** 32, (2, 500, 4), dtype=np.uint64).astype(np.uint32)  # any float bits, NaNs included
    m = {"corner": bits[0, :300].view(np.float32), "surf": bits[1].view(np.float32),
         "corner_offset": np.sort(rng.integers(0, 301, loam.MAP_CUBES + 1)).astype(np.uint32),
         "surf_offset": np.sort(rng.integers(0, 501, loam.MAP_CUBES + 1)).astype(np.uint32),
         "center": np.array([12, 4, -9], np.int32), "surround_phase": 3,
         "aft": rng.standard_normal(6).astype(np.float32), "bef": rng.standard_normal(6).astype(np.float32)}
    path = str(tmp_path / "map.npz")
    loam.save_map(path, m)
    r = loam.load_map(path)
    assert set(r) == set(m) == set(loam.MAP_KEYS)
    assert r["surround_phase"] == 3 and isinstance(r["surround_phase"], int)
    for k in loam.MAP_KEYS:
        if k == "surround_phase":
            continue
        assert r[k].dtype == m[k].dtype and r[k].shape == m[k].shape, k
        assert r[k].tobytes() == m[k].tobytes(), k
