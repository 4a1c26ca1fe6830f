"""loam_map_localize at the C-ABI boundary, without a GPU: loam_localize_result as include/loam/loam.h
declares it is the ctypes mirror field for field, the LOAM_LOC_* / LOAM_LOCALIZE_MAX constants are
the Python ones, and the call refuses a null context."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"loam_pose6": None, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32}


def _header():
    return open(os.path.join(ROOT, "include", "loam", "loam.h")).read()


def _result_fields(h):
    """(C type, field) of loam_localize_result in declaration order (several names per line allowed)"""
    end = h.index("} loam_localize_result;")
    body = h[h.rindex("typedef struct {", 0, end):end]
    fields = []
    for line in body.splitlines()[1:]:
        line = line.split("/*")[0].strip()
        m = re.match(r"(loam_pose6|int32_t|uint32_t)\s+(.*);", line)
        if m:
            fields += [(m.group(1), n.strip()) for n in m.group(2).split(",")]
    return fields


def test_result_layout_matches_header(loam):
    fields = _result_fields(_header())
    assert [n for _, n in fields] == ["aft", "status", "iters", "degenerate_steps", "rows_last", "rows_sum",
                                      "stack_corner", "stack_surf", "map_corner", "map_surf"]
    py = list(loam.LocalizeResult._fields_)
    assert [n for n, _ in py] == [n for _, n in fields]
    off = 0
    for (t, n), (_, ct) in zip(fields, py):
        if t == "loam_pose6":
            assert ct is loam.Pose6 and ctypes.sizeof(loam.Pose6) == 24, n
            size = 24
        else:
            assert ct is C_TYPES[t], n
            size = 4
        assert getattr(loam.LocalizeResult, n).offset == off, n  # (every member is 4-byte aligned: no padding)
        off += size
    assert off == ctypes.sizeof(loam.LocalizeResult) == 60
    assert loam.LOCALIZE_KEYS == tuple(n for _, n in fields)


def test_constants_match_header(loam):
    h = _header()
    vals = {k: int(v) for k, v in re.findall(r"#define (LOAM_LOC_[A-Z_]+|LOAM_LOCALIZE_MAX)\s+(\d+)", h)}
    assert vals == {"LOAM_LOC_SOLVED": loam.LOC_SOLVED, "LOAM_LOC_NO_LM": loam.LOC_NO_LM,
                    "LOAM_LOC_OFFGRID": loam.LOC_OFFGRID, "LOAM_LOCALIZE_MAX": loam.LOCALIZE_MAX}
    assert (loam.LOC_SOLVED, loam.LOC_NO_LM, loam.LOC_OFFGRID, loam.LOCALIZE_MAX) == (0, 1, 2, 1024)


def test_symbol_exported_and_null_context_is_invalid(loam):
    assert hasattr(loam.lib(), "loam_map_localize") and "loam_map_localize" in loam.EXPORTS
    pose, cl = loam.Pose6(), loam.CloudOut(None, 0, 0)
    out = (loam.LocalizeResult * 1)()
    out[0].status = 77
    rc = loam.lib().loam_map_localize(None, ctypes.byref(pose), ctypes.byref(cl), ctypes.byref(cl), 1,
                                      ctypes.byref(pose), None, out)
    assert rc == loam.LOAM_E_INVAL and loam.lib().loam_last_error()
    assert out[0].status == 77
