"""Every refusal the lanes entry points and the map services make before a kernel runs: the return
code and the whole loam_last_error() text against the hand-written table of tests/refusal_cases.py
(DESIGN.md §37), with every output buffer left as it was.

  1. the lanes entry points in each of closed / idle / in flight / pulled, for lanes with their
     own maps and for shared lanes; the table twice over one context, so a refusal that moved the
     lanes' state shows in the second pass
  2. the argument refusals of loam_map_localize and loam_map_score

No step runs: with system_delay = 1 the first push is only counted (refusal_cases.py)."""
import ctypes

import numpy as np
import pytest

import refusal_cases as rc

pytestmark = pytest.mark.gpu

U32, F64 = ctypes.c_uint32, ctypes.c_double


def _fill(obj):
    """a ctypes object filled with 0xA5, as an output a refusal must not touch"""
    ctypes.memset(ctypes.addressof(obj), 0xA5, ctypes.sizeof(obj))
    return obj


def _create(loam):
    cfg = loam.default_config(**rc.CONFIG)
    h = ctypes.c_void_p()
    assert loam.lib().loam_create(ctypes.byref(h), ctypes.byref(cfg), 0) == 0, loam.lib().loam_last_error()
    return h


def _raws(loam):
    """S valid host sweeps (inside system_delay they are not looked at)"""
    pts = np.ones((4, 4), np.float32)
    return (loam.CloudIn * rc.S)(*[loam.CloudIn(pts.ctypes.data, 4, 16) for _ in range(rc.S)]), pts


def _lane_list(a):
    lanes = a.get("lanes")
    arr = (U32 * len(lanes))(*lanes) if lanes is not None else None
    return a.get("n", len(lanes) if lanes is not None else 0), arr


def _cloud_out(loam, a, name):
    """an input cloud of loam_map_localize / loam_map_score: `name`=count points, or count 1 and no storage"""
    if a.get(name + "_null"):
        return loam.CloudOut(None, 1, 1), None
    n = a.get(name, 4)
    pts = np.zeros((n, 4), np.float32)
    return loam.CloudOut(pts.ctypes.data, n, n), pts


def _call(loam, h, call, a):
    """(return code, the outputs to compare, what must stay alive) of one call built from the plain arguments"""
    L = loam.lib()
    f = getattr(L, call)
    P6, S = loam.Pose6, rc.S
    outs, keep = [], []

    def out(obj, fill=True):  # an output: filled with 0xA5 unless it carries pointers the call reads
        outs.append((_fill(obj) if fill else obj, bytes(obj)))
        return obj

    if call in ("loam_lanes_open", "loam_lanes_open_shared"):
        r = f(h, a["n"], a["cap"])
    elif call == "loam_lanes_close":
        r = f(h)
    elif call == "loam_lanes_set_pose":
        n, lane = _lane_list(a)
        r = f(h, n, lane, (P6 * 4)(), (P6 * 4)())
    elif call == "loam_lanes_localize_info":
        r = f(h, out((loam.LocalizeResult * S)()))
    elif call == "loam_lanes_map_commit":
        n, lane = _lane_list(a)
        r = f(h, n, lane, ctypes.byref(out(loam.CommitResult())))
    elif call == "loam_dev_lanes_commit_input":
        f.argtypes = [ctypes.c_void_p, U32] + [ctypes.c_void_p] * 5
        o = [out((ctypes.c_float * 16)()), out((ctypes.c_float * 16)()), out((U32 * 2)()), out((ctypes.c_int32 * 125)()),
             out(U32())]
        r = f(h, a["lane"], *[ctypes.addressof(b) for b in o])
    elif call == "loam_lanes_score":
        n, lane = _lane_list(a)
        r = f(h, n, lane, a["max_dist"], a["k"], (P6 * 16)(), out((loam.ScoreResult * 16)()))
    elif call == "loam_lanes_localize":
        n, lane = _lane_list(a)
        r = f(h, n, lane, a["k"], (P6 * 16)(), None, out((loam.LocalizeResult * 16)()))
    elif call == "loam_lanes_push":
        raw, pts = _raws(loam)
        keep.append(pts)
        r = f(h, a["stamp"], raw)
    elif call == "loam_lanes_push_stamped":
        raw, pts = _raws(loam)
        keep.append(pts)
        r = f(h, (F64 * S)(*a["stamps"]), raw)
    elif call == "loam_lanes_push_device":
        raw, pts = _raws(loam)  # (host memory: every row of the table is refused before the sweeps are looked at)
        keep.append(pts)
        r = f(h, (F64 * S)(*a["stamps"]), raw, None, a["flags"])
    elif call == "loam_lanes_imu":
        r = f(h, a["lane"], a["stamp"], (F64 * 4)(0, 0, 0, 1), (F64 * 3)(0, 0, 9.81))
    elif call == "loam_lanes_restart":
        r = f(h, a["lane"], ctypes.byref(out(U32())))
    elif call == "loam_lanes_imu_trans":
        r = f(h, out((ctypes.c_float * (12 * S))()))
    elif call == "loam_lanes_pull":
        r = f(h, out((loam.LaneOut * S)()))
    elif call == "loam_lanes_registered":
        pts = out((ctypes.c_float * 64)())
        r = f(h, a["lane"], ctypes.byref(out(loam.CloudOut(ctypes.addressof(pts), 0, 16), fill=False)))
    elif call in ("loam_lanes_clouds", "loam_lanes_clouds_device"):
        n, lane = _lane_list(a)
        o = out(loam.LanesCloudsOut(), fill=False)  # (no pts, no offset: nothing is asked for, nothing may be written)
        r = f(h, n, lane, ctypes.byref(o)) if call == "loam_lanes_clouds" else f(h, n, lane, ctypes.byref(o), None)
    elif call == "loam_lanes_map_export":
        r = f(h, a["lane"], ctypes.byref(out(loam.Map())))
    elif call == "loam_lanes_map_import":
        n, lane = _lane_list(a)
        m = loam.Map()
        m.center[:] = a.get("center", (10, 5, 10))
        m.surround_phase = a.get("surround_phase", 4)
        if a.get("null_pts"):
            m.surf.count = 1
        r = f(h, n, lane, ctypes.byref(m), None, out((ctypes.c_uint64 * 2)()))
    elif call == "loam_lanes_surround":
        o = out(loam.LanesCloud(), fill=False)  # (an accepted call with no lane due writes count = 0 and nothing else)
        r = f(h, ctypes.byref(o))
    elif call == "loam_map_localize":
        c, kc = _cloud_out(loam, a, "corner")
        s, ks = _cloud_out(loam, a, "surf")
        keep += [kc, ks]
        r = f(h, ctypes.byref(P6()), ctypes.byref(c), ctypes.byref(s), a["n"], (P6 * 4)(), None,
              out((loam.LocalizeResult * 4)()))
    elif call == "loam_map_score":
        c, kc = _cloud_out(loam, a, "corner")
        s, ks = _cloud_out(loam, a, "surf")
        keep += [kc, ks]
        r = f(h, ctypes.byref(c), ctypes.byref(s), a.get("max_dist", 1.0), a["n"], (P6 * 4)(), out((loam.ScoreResult * 4)()))
    else:
        raise AssertionError(call)
    return r, outs, keep


def _check(loam, h, call, a, code, msg, where):
    r, outs, _keep = _call(loam, h, call, a)
    text = loam.lib().loam_last_error().decode()
    at = f"{where} {call} {a}"
    assert r == code, (at, r, text)
    if msg is None:
        return
    assert text == msg, (at, text, msg)
    for o, before in outs:
        assert bytes(o) == before, (at, "a refusal wrote into an output", type(o).__name__)


@pytest.mark.parametrize("state", rc.STATES)
@pytest.mark.parametrize("kind", rc.KINDS)
def test_lanes_refusals(loam, kind, state):
    L = loam.lib()
    h = _create(loam)
    try:
        if state != rc.CLOSED:
            opened = L.loam_lanes_open if kind == "own" else L.loam_lanes_open_shared
            assert opened(h, rc.S, rc.LANE_CAP) == 0, L.loam_last_error()
        if state in (rc.IN_FLIGHT, rc.PULLED):
            raw, _pts = _raws(loam)
            assert L.loam_lanes_push(h, 0.0, raw) == 0, L.loam_last_error()
        if state == rc.PULLED:
            out = (loam.LaneOut * rc.S)()
            assert L.loam_lanes_pull(h, out) == 0, L.loam_last_error()
            assert [o.status for o in out] == [loam.LOAM_E_NOT_READY] * rc.S  # (inside system_delay: nothing ran)
        cases = rc.expand(kind, state)
        assert len(cases) > 60
        for rep in range(2):
            for call, a, code, msg in cases:
                _check(loam, h, call, a, code, msg, f"{kind}/{state}/pass {rep}")
    finally:
        L.loam_destroy(h)


def test_map_refusals(loam):
    L = loam.lib()
    h = _create(loam)
    try:
        for call, a, msg in rc.MAP_ROWS:
            _check(loam, h, call, a, rc.INVAL, msg, "map")
    finally:
        L.loam_destroy(h)
