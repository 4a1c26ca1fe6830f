"""loam_lanes_push_device: a lanes step whose sweeps are already in device memory.

The specification is one sentence: the step is the one loam_lanes_push_stamped enqueues for the same
bytes in host memory.  So every comparison is bit for bit (uint32 views) against a second context fed
through lanes_push with the same records.

  1. the gather kernel through the hook loam_dev_lanes_gather against a numpy restatement of pack()
  2. device push == host push (S = 3, strides 16 / 32 / 12): pulls, registered clouds, exports
  3. device and host pushes alternating == the all-host run
  4. ordering against a producer stream (WAIT | RELEASE, buffers refilled without a host
     synchronisation; flags = 0 behind an explicit synchronisation)
  5. per-lane failures and call-level refusals
  6. a lane with /imu/data and a restarted lane, per-lane stamps
  7. shared lanes in an imported map, lanes_localize_info included
  8. S = 65

Streams: synthgen.stream_sweeps(10, seed), system_delay = 1, skip_frame_num = 1: step 0 is inside the
delay, step 1 the odometry's init frame, then mapping and pose-only steps alternate."""
import ctypes

import numpy as np
import pytest

import hipmem
import lanes_imu_cases as lc

pytestmark = pytest.mark.gpu

MAP_CAP = 1 << 17
HOOK = "loam_dev_lanes_gather"
SENTINEL = 0x7fc5a5a5  # LOAM_DEV_VG_SENTINEL
STRIDES = (16, 32, 12)


def _u32(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _same(a, b, msg):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    np.testing.assert_array_equal(_u32(a), _u32(b), err_msg=msg)


@pytest.fixture(scope="module")
def hip(loam):
    h = hipmem.Hip(loam)
    yield h
    h.release()


@pytest.fixture(scope="module")
def sweeps(sg):
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = sg.stream_sweeps(10, seed)
        return cache[seed]
    return get


def _records(sw, stride):
    """the sweep as records of `stride` bytes: x, y, z, then the sweep's fourth column and zeros"""
    a = np.zeros((sw.shape[0], stride // 4), np.float32)
    k = min(a.shape[1], sw.shape[1])
    a[:, :k] = sw[:, :k]
    return a


@pytest.fixture(scope="module")
def three(sweeps):
    """S = 3: two streams and a decimated copy of the first, as records of 16 / 32 / 12 bytes; [lane][step]"""
    seqs = [sweeps(1), sweeps(2), [s[::2] for s in sweeps(1)]]
    return [[_records(s, stride) for s in seq] for seq, stride in zip(seqs, STRIDES)]


def _dev(hip, rec):
    """the records uploaded into a fresh device buffer: the (ptr, count, stride) the device push takes"""
    return (hip.upload(rec), rec.shape[0], rec.shape[1] * 4)


def _engine(loam, S, **cfg):
    e = loam.Engine(loam.default_config(**dict(dict(system_delay=1, skip_frame_num=1), **cfg)))
    e.lanes_open(S, MAP_CAP)
    return e


def _pulled(e, lanes, imu=False, shared=False):
    """the step in flight, pulled: the pull's dict, the registered clouds of the lanes that mapped"""
    o = e.lanes_pull()
    rec = {"out": o, "reg": {l: e.lanes_registered(l) for l in lanes if o["mapped"][l] and o["status"][l] == 0}}
    if imu:
        rec["imu"] = e.lanes_imu_trans()
    if shared:
        rec["info"] = e.lanes_localize_info()
    return rec


def _run(e, n, push, lanes, export=True, **kw):
    recs = []
    for k in range(n):
        push(e, k)
        recs.append(_pulled(e, lanes, **kw))
    maps = {l: e.lanes_map_export(l) for l in lanes if export and recs[-1]["out"]["status"][l] == 0}
    return recs, maps


def _runs_eq(a, b, lanes, msg, lanes_b=None):
    """run a's lanes == run b's lanes_b, step by step and in the exported maps"""
    (ra, ma), (rb, mb) = a, b
    lanes_b = lanes if lanes_b is None else lanes_b
    assert len(ra) == len(rb)
    for k, (x, y) in enumerate(zip(ra, rb)):
        for la, lb in zip(lanes, lanes_b):
            for key in x["out"]:
                _same(x["out"][key][la], y["out"][key][lb], f"{msg} step {k} lane {la} {key}")
            assert (la in x["reg"]) == (lb in y["reg"]), (msg, k, la)
            if la in x["reg"]:
                _same(x["reg"][la], y["reg"][lb], f"{msg} step {k} lane {la} registered")
            if "imu" in x:
                _same(x["imu"][la], y["imu"][lb], f"{msg} step {k} lane {la} imu_trans")
            if "info" in x:
                assert x["info"][la].tobytes() == y["info"][lb].tobytes(), (msg, k, la)
    for la, lb in zip(lanes, lanes_b):
        assert (la in ma) == (lb in mb), (msg, la)
        if la in ma:
            for key in ("corner", "surf", "aft", "bef", "corner_offset", "surf_offset", "center"):
                _same(ma[la][key], mb[lb][key], f"{msg} map lane {la} {key}")
            assert ma[la]["surround_phase"] == mb[lb]["surround_phase"], (msg, la)


N3 = 7


@pytest.fixture(scope="module")
def host3(loam, three):
    """the yardstick: S = 3 over N3 steps through lanes_push"""
    e = _engine(loam, 3)
    out = _run(e, N3, lambda e, k: e.lanes_push([three[l][k] for l in range(3)], stamp=0.1 * k), range(3))
    e.close()
    kinds = [(int(r["out"]["published"][0]), int(r["out"]["mapped"][0])) for r in out[0]]
    # the delay step, the init frame, then mapping and pose-only steps
    assert kinds[0] == (0, 0) and kinds[1][1] == 0 and [m for _, m in kinds[2:]] == [1, 0, 1, 0, 1]
    assert all(len(out[0][2]["reg"][l]) > 1000 for l in range(3))
    return out


@pytest.fixture(scope="module")
def dev3(hip, three):
    """three's records in device memory, one buffer per (lane, step)"""
    return [[_dev(hip, three[l][k]) for k in range(N3)] for l in range(3)]


# ---------------------------------------------------------------- 1. the kernel through the hook
def _hook(loam):
    f = getattr(loam.lib(), HOOK)
    f.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    f.restype = ctypes.c_int
    return f


COUNTS = (0, 1, 255, 256, 257, 4097, 4999, 5000)


@pytest.mark.parametrize("stride, offset", [(12, 0), (12, 4), (16, 0), (16, 4), (16, 8), (20, 8), (20, 12), (32, 0),
                                            (32, 12)])
def test_gather_kernel_against_pack(loam, hip, stride, offset):
    S, cap = 8, 5000
    rng = np.random.default_rng(stride * 16 + offset)
    # one arena; lane s's records begin `offset` bytes behind a 16-aligned base
    sizes = [(offset + n * stride + 15) // 16 * 16 + 16 for n in COUNTS]
    bases = np.concatenate([[0], np.cumsum(sizes)])
    words = rng.integers(0, 1 << 32, int(bases[-1]) // 4, dtype=np.uint64).astype(np.uint32)
    # NaN payloads and infinities at known places besides the random ones
    words[::7] = np.uint32(0x7fc00001) + (np.arange(len(words[::7]), dtype=np.uint32) & np.uint32(0xffff))
    words[3::11] = 0x7f800000
    words[5::13] = 0xff800000
    words[6::17] = 0xffc12345
    arena = hip.upload(words)
    assert arena % 16 == 0
    raw = (loam.CloudIn * S)()
    for s, n in enumerate(COUNTS):
        raw[s] = loam.CloudIn(arena + int(bases[s]) + offset, n, stride)
    out = np.zeros((S, cap, 4), np.uint32)
    out_n = np.full(S, -2, np.int32)
    assert _hook(loam)(0, S, cap, raw, out.ctypes.data, out_n.ctypes.data) == 0, loam.lib().loam_last_error()
    np.testing.assert_array_equal(out_n, COUNTS)
    for s, n in enumerate(COUNTS):
        first = (int(bases[s]) + offset) // 4 + np.arange(n) * (stride // 4)
        want = np.zeros((n, 4), np.uint32)
        for c in range(4 if stride == 16 else 3):  # pack(): a 16-byte record is copied whole, else w = 0.0f
            want[:, c] = words[first + c]
        np.testing.assert_array_equal(out[s, :n], want, err_msg=f"lane {s}")
        assert (out[s, n:] == SENTINEL).all(), f"lane {s}: words beyond n"


def test_gather_hook_refuses_what_the_push_refuses(loam, hip):
    f = _hook(loam)
    buf = hip.malloc(4096)
    pinned, _ = hip.host_malloc(4096)
    out, out_n = np.zeros((2, 64, 4), np.uint32), np.zeros(2, np.int32)

    def call(a, b):
        raw = (loam.CloudIn * 2)(loam.CloudIn(*a), loam.CloudIn(*b))
        return f(0, 2, 64, raw, out.ctypes.data, out_n.ctypes.data)
    good = (buf, 64, 16)
    end = buf + 4096
    assert call(good, (end - (63 * 32 + 12), 64, 32)) == 0  # ends exactly at the allocation's end
    assert call(good, (end - (63 * 32 + 12) + 4, 64, 32)) == loam.LOAM_E_INVAL
    assert b"lane 1" in loam.lib().loam_last_error()
    assert call((end - 12, 1, 12), good) == 0
    assert call((end - 8, 1, 12), good) == loam.LOAM_E_INVAL
    assert b"lane 0" in loam.lib().loam_last_error()
    assert call((end - 16, 1, 16), good) == 0               # a 16-byte record is read whole
    assert call((end - 12, 1, 16), good) == loam.LOAM_E_INVAL
    assert call(good, (pinned, 64, 16)) == loam.LOAM_E_INVAL  # pinned host memory is not device memory
    # what fails a lane alone is no refusal: the lane gathers nothing
    assert call(good, (buf + 2, 8, 16)) == 0 and list(out_n) == [64, 0]
    assert call((None, 8, 16), (buf, 8, 8)) == 0 and list(out_n) == [0, 0]
    assert call((buf, 65, 16), (buf, 0, 16)) == 0 and list(out_n) == [0, 0]


# ---------------------------------------------------------------- 2. / 3. equality with the host push
def test_device_push_equals_host_push(loam, three, host3, dev3):
    e = _engine(loam, 3)
    got = _run(e, N3, lambda e, k: e.lanes_push_device([dev3[l][k] for l in range(3)], stamp=0.1 * k), range(3))
    e.close()
    _runs_eq(got, host3, range(3), "device push")


def test_alternating_pushes_equal_the_host_run(loam, three, host3, dev3):
    for first in (0, 1):  # (either kind on the init frame and on the mapping frames)
        def push(e, k):
            if (k + first) % 2:
                e.lanes_push([three[l][k] for l in range(3)], stamp=0.1 * k)
            else:
                e.lanes_push_device([dev3[l][k] for l in range(3)], stamp=[0.1 * k] * 3)
        e = _engine(loam, 3)
        got = _run(e, N3, push, range(3))
        e.close()
        _runs_eq(got, host3, range(3), f"alternating, first {first}")


# ---------------------------------------------------------------- 4. ordering
N_ORDER = 6


def test_ordering_against_a_producer_stream(loam, hip, three, host3):
    prod = hip.stream()
    nbytes = [[three[l][k].nbytes for k in range(N_ORDER)] for l in range(3)]
    bufs = [hip.malloc(max(nbytes[l])) for l in range(3)]
    # every step's records in pinned memory (the copies read them asynchronously)
    pinned = []
    for l in range(3):
        row = []
        for k in range(N_ORDER):
            p, view = hip.host_malloc(nbytes[l][k])
            view[:nbytes[l][k]] = three[l][k].view(np.uint8).reshape(-1)
            row.append(p)
        pinned.append(row)

    def refill(k):
        for l in range(3):
            hip.put_async(bufs[l], pinned[l][k], nbytes[l][k], prod)

    def raws(k):
        return [(bufs[l], three[l][k].shape[0], three[l][k].shape[1] * 4) for l in range(3)]
    want = (host3[0][:N_ORDER], {})

    # WAIT | RELEASE: the next step's refill is enqueued right behind the push, before the pull; nothing
    # but the events keeps it from overwriting the sweeps the gather reads
    e = _engine(loam, 3)
    recs = []
    refill(0)
    for k in range(N_ORDER):
        e.lanes_push_device(raws(k), stamp=0.1 * k, stream=prod, wait=True, release=True)
        if k + 1 < N_ORDER:
            refill(k + 1)
        recs.append(_pulled(e, range(3)))
    hip.sync(prod)
    e.close()
    _runs_eq((recs, {}), want, range(3), "WAIT | RELEASE")

    # flags = 0: the caller synchronises the producer before each push and refills after the pull
    e = _engine(loam, 3)
    recs = []
    for k in range(N_ORDER):
        refill(k)
        hip.sync(prod)
        e.lanes_push_device(raws(k), stamp=0.1 * k)
        recs.append(_pulled(e, range(3)))
    e.close()
    _runs_eq((recs, {}), want, range(3), "flags 0")


# ---------------------------------------------------------------- 5. failures
N_FAIL, K_FAIL = 5, 2
GARBAGE = 0x00dead00beef0000  # non-null, aligned, no memory: only ever given to a lane that has failed


def _bad_sweep(kind, good, cap):
    ptr, n, stride = good
    return {"retire": (0, 0, stride), "capacity": (ptr, cap + 1, stride), "null": (0, n, stride),
            "stride8": (ptr, n, 8), "plus2": (ptr + 2, n, stride)}[kind]


@pytest.mark.parametrize("kind", ["retire", "capacity", "null", "stride8", "plus2"])
def test_a_lane_fails_alone_with_the_host_pushs_code(loam, three, host3, dev3, kind):
    cap = int(loam.default_config().max_points)

    def push_dev(e, k):
        raws = [dev3[l][k] for l in range(3)]
        if k == K_FAIL:
            raws[1] = _bad_sweep(kind, raws[1], cap)
        elif k > K_FAIL:  # failed: its sweep is not looked at, the pointer is never read
            raws[1] = (GARBAGE, 1000, 16)
        e.lanes_push_device(raws, stamp=0.1 * k)

    def push_host(e, k):
        raws = [three[l][k] for l in range(3)]
        if k == K_FAIL:
            ptr, n, stride = _bad_sweep("null" if kind == "plus2" else kind, (raws[1].ctypes.data, raws[1].shape[0], 32), cap)
            raws[1] = loam.CloudIn(ptr or None, n, stride)
        e.lanes_push(raws, stamp=0.1 * k)
    e = _engine(loam, 3)
    got = _run(e, N_FAIL, push_dev, range(3))
    e.close()
    e = _engine(loam, 3)
    want = _run(e, N_FAIL, push_host, range(3))
    e.close()
    code = loam.LOAM_E_CAPACITY if kind == "capacity" else loam.LOAM_E_INVAL
    for k in range(N_FAIL):
        expect = code if k >= K_FAIL else loam.LOAM_E_NOT_READY if k == 0 else 0  # (step 0 is inside system_delay)
        assert got[0][k]["out"]["status"][1] == want[0][k]["out"]["status"][1] == expect, (kind, k)
    _runs_eq(got, want, range(3), f"{kind}: against the host push")
    # the other lanes equal their own runs (the export is of a later step there)
    _runs_eq((got[0], {}), (host3[0][:N_FAIL], {}), [0, 2], f"{kind}: the other lanes")


def test_call_level_refusals_change_nothing(loam, hip, three, host3, dev3):
    pinned, _ = hip.host_malloc(three[1][0].nbytes)
    INVAL = loam.LOAM_E_INVAL
    closed = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    closed.n_lanes = 3
    with pytest.raises(loam.LoamError) as ei:
        closed.lanes_push_device([dev3[l][0] for l in range(3)])
    assert ei.value.code == INVAL and "not open" in str(ei.value)
    closed.close()

    def refused(e, raws, stamp, flags=0, match=None):
        a = (loam.CloudIn * 3)(*[loam._cloud_in_device(r) for r in raws])
        t = (ctypes.c_double * 3)(*stamp)
        assert loam.lib().loam_lanes_push_device(e.h, t, a, None, flags) == INVAL
        if match:
            assert match in loam.lib().loam_last_error().decode()

    def push(e, k):
        raws = [dev3[l][k] for l in range(3)]
        t = [0.1 * k] * 3
        refused(e, raws, [t[0], float("nan"), t[2]], match="not finite")
        refused(e, raws, [t[0], t[1], float("inf")], match="not finite")
        refused(e, raws, t, flags=4, match="flag")
        refused(e, raws, t, flags=7, match="flag")
        if k >= 1:  # (inside system_delay no sweep is looked at)
            refused(e, [raws[0], (pinned, raws[1][1], raws[1][2]), raws[2]], t, match="lane 1")
            past = (raws[2][0] + 16, raws[2][1], raws[2][2])  # the last record leaves the allocation
            refused(e, [raws[0], raws[1], past], t, match="lane 2")
        e.lanes_push_device(raws, stamp=t)
        refused(e, raws, t, match="in flight")
    e = _engine(loam, 3)
    got = _run(e, N3, push, range(3))
    e.close()
    _runs_eq(got, host3, range(3), "refusals in between")


# ---------------------------------------------------------------- 6. IMU and restart
def test_imu_lane_and_restarted_lane(loam, sg, hip, sweeps):
    n, k_restart = 8, 4
    a = lc.Feed(sweeps(1)[:n], 0.0)
    a.sched = lc.schedule(sg.imu_stream(-0.5, lc.PERIOD * n + 0.1, seed=1), 0.0, n)
    b = lc.Feed(sweeps(2)[:n], 100.0)
    feeds = [a, b]
    dev = [[_dev(hip, np.ascontiguousarray(f.sweeps[k], np.float32)) for k in range(n)] for f in feeds]

    def run(device):
        e = _engine(loam, 2)
        waits = [0]

        def push(e, k):
            for msg in a.sched[k]:
                e.lanes_imu(0, *msg)
            if k == k_restart:
                waits[0] = e.lanes_restart(1)
            stamps = [f.stamps[k] for f in feeds]
            if not device:
                e.lanes_push([f.sweeps[k] for f in feeds], stamp=stamps)
                return
            raws = [dev[l][k] for l in range(2)]
            if k_restart <= k < k_restart + waits[0]:  # a waiting lane's sweep is not looked at
                raws[1] = (GARBAGE, 1000, 16)
            e.lanes_push_device(raws, stamp=stamps)
        out = _run(e, n, push, range(2), imu=True)
        e.close()
        return out
    got, want = run(True), run(False)
    assert np.abs(want[0][-1]["imu"][0]).max() > 0 and not want[0][-1]["imu"][1].any()
    assert want[0][k_restart]["out"]["status"][1] in (0, loam.LOAM_E_NOT_READY)
    assert any(r["out"]["mapped"][1] for r in want[0][k_restart + 1:])  # the restarted lane maps again
    _runs_eq(got, want, range(2), "imu + restart")


# ---------------------------------------------------------------- 7. shared lanes
def test_shared_lanes(loam, hip, sweeps):
    src = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
    for k, sw in enumerate(sweeps(1)):
        src.chain_sweep(sw, stamp=0.1 * k)
    m = src.map_export()
    src.close()
    assert m["corner"].shape[0] > 1000 and m["surf"].shape[0] > 1000
    n = 4
    recs = [[_records(sweeps(s)[k], stride) for k in range(n)] for s, stride in ((1, 32), (2, 16))]
    dev = [[_dev(hip, r) for r in row] for row in recs]

    def run(device):
        e = loam.Engine(loam.default_config(system_delay=1, skip_frame_num=1))
        assert e.map_import(**{k: m[k] for k in ("corner", "surf", "center", "surround_phase", "aft", "bef")}) == (0, 0)
        e.lanes_open_shared(2, 1 << 17)

        def push(e, k):
            if device:
                e.lanes_push_device([dev[l][k] for l in range(2)], stamp=0.1 * k)
            else:
                e.lanes_push([recs[l][k] for l in range(2)], stamp=0.1 * k)
        out = _run(e, n, push, range(2), export=False, shared=True)
        e.close()
        return out
    got, want = run(True), run(False)
    assert any(r["out"]["mapped"].all() for r in want[0])
    _runs_eq(got, want, range(2), "shared lanes")


# ---------------------------------------------------------------- 8. S = 65
def test_65_lanes(loam, hip, three, dev3):
    S, n = 65, 3  # the delay step, the init frame, one mapping step
    src = [l % 3 for l in range(S)]

    def run(device):
        e = _engine(loam, S)

        def push(e, k):
            if device:  # (lanes of one stream read the same device buffer)
                e.lanes_push_device([dev3[s][k] for s in src], stamp=0.1 * k)
            else:
                e.lanes_push([three[s][k] for s in src], stamp=0.1 * k)
        out = _run(e, n, push, (0, 31, 64))
        e.close()
        return out
    got, want = run(True), run(False)
    assert all(want[0][2]["out"]["mapped"][l] == 1 for l in (0, 31, 64))
    _runs_eq(got, want, (0, 31, 64), "S = 65")
