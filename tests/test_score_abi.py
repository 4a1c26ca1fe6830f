"""loam_map_score at the C-ABI boundary, without a GPU: loam_score_result as include/loam/loam.h
declares it is the ctypes mirror field for field (32 bytes), LOAM_SCORE_MAX is the Python constant,
the symbol is exported and listed, and the call refuses a null context."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C_TYPES = {"uint32_t": (ctypes.c_uint32, 4), "double": (ctypes.c_double, 8)}


def _header():
    return open(os.path.join(ROOT, "include", "loam", "loam.h")).read()


def _result_fields(h):
    """(C type, field) of loam_score_result in declaration order (several names per line allowed)"""
    end = h.index("} loam_score_result;")
    body = h[h.rindex("typedef struct {", 0, end):end]
    fields = []
    for line in body.splitlines()[1:]:
        line = line.split("/*")[0].strip()
        m = re.match(r"(uint32_t|double)\s+(.*);", line)
        if m:
            fields += [(m.group(1), n.strip()) for n in m.group(2).split(",")]
    return fields


def test_result_layout_matches_header(loam):
    fields = _result_fields(_header())
    assert [n for _, n in fields] == ["corner_scored", "surf_scored", "corner_in", "surf_in", "corner_cost", "surf_cost"]
    py = list(loam.ScoreResult._fields_)
    assert [n for n, _ in py] == [n for _, n in fields]
    off = 0
    for (t, n), (_, ct) in zip(fields, py):
        assert ct is C_TYPES[t][0], n
        assert off % C_TYPES[t][1] == 0, n  # (naturally aligned as declared: no padding)
        assert getattr(loam.ScoreResult, n).offset == off, n
        off += C_TYPES[t][1]
    assert off == ctypes.sizeof(loam.ScoreResult) == 32
    assert [getattr(loam.ScoreResult, n).offset for n, _ in py] == [0, 4, 8, 12, 16, 24]
    assert loam.SCORE_KEYS == tuple(n for _, n in fields)


def test_constant_matches_header(loam):
    vals = re.findall(r"#define LOAM_SCORE_MAX\s+(\d+)", _header())
    assert [int(v) for v in vals] == [loam.SCORE_MAX] == [65536]


def test_symbol_exported_and_null_context_is_invalid(loam):
    assert hasattr(loam.lib(), "loam_map_score") and "loam_map_score" in loam.EXPORTS
    pose, cl = loam.Pose6(), loam.CloudOut(None, 0, 0)
    out = (loam.ScoreResult * 1)()
    out[0].corner_in = 77
    rc = loam.lib().loam_map_score(None, ctypes.byref(cl), ctypes.byref(cl), 1.0, 1, ctypes.byref(pose), out)
    assert rc == loam.LOAM_E_INVAL and loam.lib().loam_last_error()
    assert out[0].corner_in == 77


def test_score_order_key(loam):
    """most inliers, then least cost, then lowest index"""
    import numpy as np
    s = {"corner_in": np.array([1, 2, 2, 2, 0], np.uint32), "surf_in": np.array([5, 5, 5, 5, 9], np.uint32),
         "corner_cost": np.array([0.0, 1.0, 0.5, 0.5, 0.0]), "surf_cost": np.array([0.0, 1.0, 0.5, 0.5, 0.0])}
    assert loam.score_order(s).tolist() == [4, 2, 3, 1, 0]
    assert loam.score_order(s, index=[9, 8, 7, 6, 5]).tolist() == [4, 3, 2, 1, 0]
