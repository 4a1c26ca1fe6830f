"""Inputs of tests/test_point_fields.py and tests/test_gpu_point_fields.py (loam_set_point_fields,
DESIGN.md §40): records with a ring and a time field in any layout, serialized PointCloud2
messages, and the numpy statement of what the engine does with them.  Built without a GPU."""
import struct

import numpy as np

U8, U16, U32, F32, F64 = 1, 2, 3, 4, 5          # LOAM_FIELD_*
_NP = {U8: np.uint8, U16: np.uint16, U32: np.uint32, F32: np.float32, F64: np.float64}
SIZE = {U8: 1, U16: 2, U32: 4, F32: 4, F64: 8}
TILE = 2048                                      # points of a ring-sort tile


class Layout:
    """where a record keeps its fields: ring = (type, offset), time = None or (type, offset), stride"""

    def __init__(self, ring, time, stride):
        self.ring, self.time, self.stride = ring, time, stride

    def end(self):
        e = self.ring[1] + SIZE[self.ring[0]]
        return max(e, self.time[1] + SIZE[self.time[0]]) if self.time else e


VELODYNE = Layout((U16, 20), (F32, 24), 32)      # PointXYZIRT


def records(layout, xyz, ring_values, time_values=None, lead=0, fill=0xA5):
    """the sweep as bytes: `lead` bytes of padding, then one record per point; every byte no field
    owns is `fill` (so a leak of the caller's bytes into the engine would show).  Returns the uint8
    array (keep it alive) and the address of the first record."""
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    buf = np.full(lead + max(n, 1) * layout.stride + 8, fill, np.uint8)
    rec = buf[lead:lead + n * layout.stride].reshape(n, layout.stride)
    rec[:, 0:12] = xyz.view(np.uint8).reshape(n, 12)
    t, o = layout.ring
    rec[:, o:o + SIZE[t]] = np.ascontiguousarray(ring_values).astype(_NP[t]).reshape(n, 1).view(np.uint8)
    if layout.time is not None:
        t, o = layout.time
        rec[:, o:o + SIZE[t]] = np.ascontiguousarray(time_values).astype(_NP[t]).reshape(n, 1).view(np.uint8)
    return buf, buf.ctypes.data + lead


def cloud_in(loam, layout, xyz, ring_values, time_values=None, lead=0):
    buf, ptr = records(layout, xyz, ring_values, time_values, lead)
    return loam.CloudIn(ptr, int(np.asarray(xyz).reshape(-1, 3).shape[0]), layout.stride), buf


def fields(loam, layout, scale=1.0, bias=0.0, ring_map=None):
    time = None if layout.time is None else (layout.time[0], layout.time[1], scale, bias)
    return loam.PointFields.of(layout.ring, time, ring_map)


# ---------------------------------------------------------------- the numpy statement
def tau_of(t, scale, bias):
    """(float)((double)t * scale + bias): the product and the sum rounded to double, then to float"""
    prod = np.asarray(t).astype(np.float64) * np.float64(scale)
    return (prod + np.float64(bias)).astype(np.float32)


def ring_of(values, n_rings, ring_map=None):
    v = np.asarray(values).astype(np.int64)
    if ring_map is None:
        return np.where(v < n_rings, v, -1)
    m = np.asarray(ring_map, np.int64)
    return np.where(v < len(m), m[np.minimum(v, len(m) - 1)], -1)


def kept(xyz, r, tau=None):
    ok = np.all(np.isfinite(np.asarray(xyz, np.float32).reshape(-1, 3)), axis=1) & (r >= 0)
    if tau is not None:
        with np.errstate(invalid="ignore"):
            ok &= (tau >= np.float32(0)) & (tau <= np.float32(0.5))
    return ok


def expected_full(xyz, r, tau):
    """the ring-and-time mode's full cloud: the kept points stably sorted by ring, (y, z, x) and
    float32(r) + tau"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    k = np.flatnonzero(kept(xyz, r, tau))
    k = k[np.argsort(r[k], kind="stable")]
    out = np.empty((len(k), 4), np.float32)
    out[:, 0], out[:, 1], out[:, 2] = xyz[k, 1], xyz[k, 2], xyz[k, 0]
    out[:, 3] = r[k].astype(np.float32) + tau[k]
    return out


def xyz_keys(xyz):
    """one bytes key per point from the bit patterns of its three coordinates"""
    a = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    return [row.tobytes() for row in a]


def rings_from_full(raw_xyz, full, absent=65535):
    """each input point's ring and intensity, recovered from a full cloud by coordinate bits
    (full = (y, z, x, intensity)); absent points get `absent` and intensity 0"""
    table = {k: i for i, k in enumerate(xyz_keys(full[:, [2, 0, 1]]))}
    assert len(table) == full.shape[0], "coordinates repeat in the full cloud"
    idx = np.array([table.get(k, -1) for k in xyz_keys(raw_xyz)], np.int64)
    inten = np.where(idx >= 0, full[np.maximum(idx, 0), 3], np.float32(0)).astype(np.float32)
    ring = np.where(idx >= 0, inten.astype(np.int64), absent)
    return ring, inten


# ---------------------------------------------------------------- sweeps
def with_nans_and_high_points(sweep, k=64):
    """the sweep with k NaN points and k points at 30 .. 60 degrees elevation spread through it,
    one of the high points first and one last (they keep their azimuth, so the sweep's ends do too)"""
    s = np.array(sweep, np.float32, copy=True)
    n = s.shape[0]
    pos = np.unique(np.linspace(0, n - 1, 2 * k).astype(np.int64))
    assert len(pos) == 2 * k and pos[0] == 0 and pos[-1] == n - 1
    mid = pos[1:-1]
    nan = np.concatenate([mid[0::2], mid[1:2]])                   # k of them
    high = np.setdiff1d(pos, nan)                                 # k too, the first and the last point among them
    assert len(nan) == k and len(high) == k and high[0] == 0 and high[-1] == n - 1
    elev = np.radians(np.linspace(30.0, 60.0, len(high)))
    s[high, 2] = (np.hypot(s[high, 0].astype(np.float64), s[high, 1].astype(np.float64)) * np.tan(elev)).astype(np.float32)
    s[nan, :3] = np.nan
    return s, high, nan


# ---------------------------------------------------------------- PointCloud2 (ROS1 wire format)
PF_UINT8, PF_UINT16, PF_UINT32, PF_FLOAT32, PF_FLOAT64 = 2, 4, 6, 7, 8


def _string(s):
    b = s.encode()
    return struct.pack("<I", len(b)) + b


def pointcloud2(field_list, point_step, data, stamp=1.5):
    """a serialized sensor_msgs/PointCloud2: field_list = [(name, offset, datatype)], data = the
    records' bytes"""
    n = len(data) // point_step
    sec = int(stamp)
    out = struct.pack("<III", 0, sec, int(round((stamp - sec) * 1e9))) + _string("velodyne")
    out += struct.pack("<II", 1, n) + struct.pack("<I", len(field_list))
    for name, off, dt in field_list:
        out += _string(name) + struct.pack("<IBI", off, dt, 1)
    out += struct.pack("<BII", 0, point_step, point_step * n) + struct.pack("<I", len(data)) + bytes(data)
    return out + struct.pack("<B", 1)


XYZ = [("x", 0, PF_FLOAT32), ("y", 4, PF_FLOAT32), ("z", 8, PF_FLOAT32)]
PC2_VELODYNE = XYZ + [("intensity", 16, PF_FLOAT32), ("ring", 20, PF_UINT16), ("time", 24, PF_FLOAT32)]
PC2_OUSTER = XYZ + [("intensity", 16, PF_FLOAT32), ("t", 20, PF_UINT32), ("reflectivity", 24, PF_UINT16),
                    ("ring", 26, PF_UINT8), ("ambient", 28, PF_UINT16), ("range", 32, PF_UINT32)]
PC2_NO_RING = XYZ + [("intensity", 12, PF_FLOAT32)]
