"""The whole cube map against the oracle's after every mapping frame.

Engine.map_export() and Oracle.map_export() hold all 4851 cubes of both kinds in store order, so a
wrong map update shows wherever it lands, not only within two cubes of the sensor.  Both sides get
the identical mapping frames of tests/map_cases.py (whose preconditions tests/test_map_cases.py
checks on the oracle alone), and everything is compared bit for bit, as uint32 words: every float of
every point of both clouds (intensity too: behind TransformToEnd it is the ring number), both offset
tables, center, aft and bef; then the registered cloud, /laser_cloud_surround when published,
mp_grid_shifts and mp_iters.

  streaming   Engine.mapping, every case, under the default tuning, vg_merge = 0 and every vg_split
  deferred    the raw sweeps of wide and below through chain_sweep (stream_defer at its default)
              against the oracle's whole pipeline, the map exported after every call
  lanes       three lanes (wide, wide_out, an unmodified stream) against three oracles
  commit      one shared lane's wide sweep committed (k_cm_rank's one-wave ranking) against the
              host restatement of tests/test_gpu_lanes_commit.py
  second run  wide on a second engine of the process
"""
import numpy as np
import pytest

import map_cases as mc
from test_gpu_lanes_commit import _engine, _hook, _points_same, _restate, _result_same, _to_map_step
from test_gpu_map import _bits, _check_offsets, cube_keys
from vg_cases import oracle_vg

pytestmark = pytest.mark.gpu

KINDS = ("corner", "surf")
TUNINGS = {"default": {}, "vg_merge=0": dict(vg_merge=0), "vg_split=0": dict(vg_split=0), "vg_split=1": dict(vg_split=1),
           "vg_split=2": dict(vg_split=2), "vg_split=3": dict(vg_split=3)}
LANE_CAP = 1 << 17


def _same(a, b, msg):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=msg)


def _map_same(g, o, msg):
    """an engine's export against the oracle's, every word; a difference is told by cube first"""
    _check_offsets(g)
    np.testing.assert_array_equal(g["center"], o["center"], err_msg=f"{msg} center")
    for kind in KINDS:
        go, oo = g[kind + "_offset"].astype(np.int64), o[kind + "_offset"].astype(np.int64)
        bad = np.flatnonzero(np.diff(go) != np.diff(oo))
        assert bad.size == 0, f"{msg}: {bad.size} {kind} cubes differ in size, first {bad[:8]}: {np.diff(go)[bad[:8]]} vs {np.diff(oo)[bad[:8]]}"
        np.testing.assert_array_equal(g[kind + "_offset"], o[kind + "_offset"], err_msg=f"{msg} {kind}_offset")
        assert g[kind].shape == o[kind].shape, (msg, kind)
        rows = np.flatnonzero((_bits(g[kind]) != _bits(o[kind])).any(axis=1))
        if rows.size:
            cubes = np.unique(np.searchsorted(oo, rows, side="right") - 1)
            raise AssertionError(f"{msg}: {rows.size} {kind} points in {cubes.size} cubes differ, first cubes {cubes[:8]}, "
                                 f"first point {rows[0]}: {g[kind][rows[0]]} vs {o[kind][rows[0]]}")
    _same(g["aft"], o["aft"], f"{msg} aft")
    _same(g["bef"], o["bef"], f"{msg} bef")
    assert g["surround_phase"] == o["surround_phase"], msg


def _frame_same(g, o, msg):
    """a mapping frame's record (map_cases.map_frame) of an engine against the oracle's"""
    _same(g["aft"], o["aft"], f"{msg} aft")
    _same(g["bef"], o["bef"], f"{msg} bef")
    assert (g["mp_shifts"], g["mp_iters"]) == (o["mp_shifts"], o["mp_iters"]), (msg, "mp_grid_shifts, mp_iters")
    _same(g["registered"], o["registered"], f"{msg} registered")
    assert (g["surround"] is None) == (o["surround"] is None), f"{msg} surround published"
    if o["surround"] is not None:
        _same(g["surround"], o["surround"], f"{msg} surround")
    _map_same(g["map"], o["map"], msg)


def _stream(loam, frames, **tuning):
    e = loam.Engine(loam.default_config(**mc.CFG))
    e.set_tuning(**tuning)
    out = [mc.map_frame(e, f) for f in frames]
    e.close()
    return out


@pytest.mark.parametrize("tuning", list(TUNINGS))
@pytest.mark.parametrize("name", mc.CASES)
def test_streaming(loam, oc, sg, name, tuning):
    frames, want = mc.frames(name, oc, sg), mc.oracle_run(name, oc, sg)
    e = loam.Engine(loam.default_config(**mc.CFG))
    if tuning == "default":
        assert (e.get_tuning("vg_merge"), e.get_tuning("vg_split")) == (1, 1)
    e.set_tuning(**TUNINGS[tuning])
    for m, (f, o) in enumerate(zip(frames, want)):
        _frame_same(mc.map_frame(e, f), o, f"{name} [{tuning}] frame {m}")
    e.close()


def test_second_run(loam, oc, sg):
    frames, want = mc.frames("wide", oc, sg), mc.oracle_run("wide", oc, sg)
    first, second = _stream(loam, frames), _stream(loam, frames)
    for m, (a, b, o) in enumerate(zip(first, second, want)):
        _frame_same(b, o, f"wide, second engine, frame {m}")
        _frame_same(b, a, f"wide, second engine against the first, frame {m}")


@pytest.mark.parametrize("name", ("wide", "below"))
def test_deferred_update(loam, oc, sg, name):
    want = mc.oracle_pipeline(name, oc, sg)
    e = loam.Engine(loam.default_config(**mc.CFG))
    assert e.get_tuning("stream_defer") == 1
    last, mapped = None, 0
    for k, sw in enumerate(mc.raw_sweeps(sg, name)):
        rc, pub, od, aft, bef, reg = e.chain_sweep(sw, stamp=0.1 * k, registered=True)
        o, msg = want[k], f"{name} chain_sweep {k}"
        assert (aft is not None) == (o is not None), msg
        g = {"map": e.map_export()}  # (after every call: the export waits for the deferred update)
        if o is None:
            if last is None:
                assert g["map"]["corner"].shape[0] == 0 and g["map"]["surf"].shape[0] == 0, msg
            else:
                _map_same(g["map"], last["map"], msg + " (no mapping frame)")
            continue
        s = e.stats()
        g.update(aft=aft, bef=bef, registered=reg, surround=e.mapping_surround(), mp_shifts=s["mp_grid_shifts"],
                 mp_iters=s["mp_iters"])
        _frame_same(g, o, msg)
        last, mapped = o, mapped + 1
    e.close()
    assert mapped >= 3


def test_lanes(loam, oc, sg):
    names = ("wide", "wide_out", "plain")
    want = [mc.oracle_pipeline(n, oc, sg) for n in names]
    feeds = [mc.raw_sweeps(sg, n) for n in names]
    steps = [k for k in range(mc.N_SWEEPS) if want[0][k] is not None]
    assert len(steps) >= 3 and all([k for k in range(mc.N_SWEEPS) if w[k] is not None] == steps for w in want)
    export_at = (steps[1], mc.N_SWEEPS - 1)  # one middle step (a mapping step) and the last one
    e = loam.Engine(loam.default_config(**mc.CFG))
    e.lanes_open(len(names), LANE_CAP)
    last = [None] * len(names)
    for k in range(mc.N_SWEEPS):
        out = e.lanes_step([f[k] for f in feeds], stamp=0.1 * k)
        sur = e.lanes_surround() if k in steps else None
        for l, n in enumerate(names):
            o, msg = want[l][k], f"lane {l} ({n}) step {k}"
            assert out["mapped"][l] == (1 if o is not None else 0), msg
            if o is not None:
                assert out["status"][l] == 0, msg
                _same(out["aft"][l], o["aft"], msg + " aft")
                _same(out["bef"][l], o["bef"], msg + " bef")
                assert out["mp_iters"][l] == o["mp_iters"], msg
                _same(e.lanes_registered(l), o["registered"], msg + " registered")
                assert (sur[l] is None) == (o["surround"] is None), msg
                if o["surround"] is not None:
                    _same(sur[l], o["surround"], msg + " surround")
                last[l] = o
            if k in export_at:
                _map_same(e.lanes_map_export(l), last[l]["map"], msg)
    e.lanes_close()
    e.close()
    assert mc.keys_of(last[0]) > mc.K_DENSE and mc.keys_of(last[1]) > mc.K_DENSE and sum(last[1]["map"]["dropped"]) > 0
    assert mc.keys_of(last[2]) < 100


def test_commit(loam, oc, sg):
    """the map: the oracle's after two wide frames (every far cube of the sweep already holds points);
    the lane: one shared lane over wide's raw sweeps, committed behind its first mapping step"""
    vg = oracle_vg(oc)
    prior = mc.oracle_run("wide", oc, sg)[1]["map"]
    raws = mc.raw_sweeps(sg, "wide")
    e = _engine(loam, 1, prior)
    outs, regs = [], []
    _to_map_step(e, lambda k: [raws[k]], range(1), outs, regs)
    assert outs[-1]["status"][0] == 0 and outs[-1]["mapped"][0] == 1
    before = e.map_export()
    _map_same(before, prior, "the imported map")
    inp = _hook(loam, e, 0)
    keys = [cube_keys(inp[kind], before["center"]) for kind in KINDS]
    nkeys = sum(np.unique(q[q >= 0]).size for q in keys)
    grown = sum(int((np.diff(before[kind + "_offset"].astype(np.int64))[np.unique(q[q >= 0])] > 0).sum())
                for kind, q in zip(KINDS, keys))
    print(f"commit: {inp['corner'].shape[0]} + {inp['surf'].shape[0]} stack points, {nkeys} keys, {grown} into non-empty cubes")
    assert nkeys > mc.K_DENSE and grown > 100
    res = e.lanes_map_commit([0])
    after = e.map_export()
    e.close()
    re = _restate(before, [inp], vg)
    _points_same(after, re, "commit([0]) of a wide sweep")
    _result_same(res, re, "commit([0]) of a wide sweep")
    for f in ("aft", "bef"):
        _same(after[f], before[f], f"the context's {f}")
