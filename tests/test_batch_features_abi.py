"""loam_batch_features at the C-ABI boundary, without a GPU: the symbol exists and refuses a null
context, and the ctypes mirrors of loam_batch_cloud / loam_batch_clouds have the layout the header
declares."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"loam_point *": ctypes.c_void_p, "uint32_t *": ctypes.c_void_p, "uint64_t": ctypes.c_uint64}


def _header():
    return open(os.path.join(ROOT, "include", "loam", "loam.h")).read()


def _struct_fields(h, name):
    """(C type, field) of the one-member-per-line struct `name` as the header declares it"""
    end = h.index("} %s;" % name)
    body = h[h.rindex("typedef struct {", 0, end):end]
    fields = []
    for line in body.splitlines()[1:]:
        line = line.split("/*")[0].strip()
        m = re.match(r"(loam_point \*|uint32_t \*|uint64_t)\s*([a-z_]+);", line)
        if m:
            fields.append((m.group(1), m.group(2)))
    return fields


def test_null_context_is_invalid(loam):
    out = loam.BatchClouds()
    assert loam.lib().loam_batch_features(None, 0, 1, ctypes.byref(out)) == loam.LOAM_E_INVAL
    assert loam.lib().loam_last_error()


def test_batch_cloud_layout_matches_header(loam):
    fields = _struct_fields(_header(), "loam_batch_cloud")
    assert [n for _, n in fields] == ["pts", "capacity", "count", "offset"]
    assert [(n, C_TYPES[t]) for t, n in fields] == list(loam.BatchCloud._fields_)
    # natural alignment of four 8-byte members
    for i, (n, _) in enumerate(loam.BatchCloud._fields_):
        assert getattr(loam.BatchCloud, n).offset == 8 * i, n
    assert ctypes.sizeof(loam.BatchCloud) == 32


def test_batch_clouds_layout_matches_header(loam):
    h = _header()
    m = re.search(r"typedef struct \{ loam_batch_cloud ([a-z_, ]+); \} loam_batch_clouds;", h)
    assert m, "loam_batch_clouds declaration"
    names = [n.strip() for n in m.group(1).split(",")]
    assert names == [n for n, _ in loam.BatchClouds._fields_] == list(loam.BATCH_CLOUDS)
    assert all(t is loam.BatchCloud for _, t in loam.BatchClouds._fields_)
    for i, n in enumerate(names):
        assert getattr(loam.BatchClouds, n).offset == 32 * i, n
    assert ctypes.sizeof(loam.BatchClouds) == 32 * 5
    # the order of the node call's loam_features clouds
    assert names == [n for n, _ in loam.Features._fields_][:5]
