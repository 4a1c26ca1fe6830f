"""Device memory, pinned memory and streams for the GPU tests of the device feed, through ctypes on the
HIP runtime libloam_hip.so itself is linked against (loaded after loam.lib(), so both share one
runtime).  Test infrastructure: no torch."""
import ctypes

import numpy as np

H2D, D2H = 1, 2  # hipMemcpyHostToDevice, hipMemcpyDeviceToHost


class Hip:
    def __init__(self, loam):
        loam.lib()
        L = self.L = ctypes.CDLL("libamdhip64.so")
        vp, sz, P = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER
        L.hipMalloc.argtypes = [P(vp), sz]
        L.hipFree.argtypes = [vp]
        L.hipMemcpy.argtypes = [vp, vp, sz, ctypes.c_int]
        L.hipMemcpyAsync.argtypes = [vp, vp, sz, ctypes.c_int, vp]
        L.hipStreamCreate.argtypes = [P(vp)]
        L.hipStreamDestroy.argtypes = [vp]
        L.hipStreamSynchronize.argtypes = [vp]
        L.hipHostMalloc.argtypes = [P(vp), sz, ctypes.c_uint]
        L.hipHostFree.argtypes = [vp]
        self._dev, self._host, self._streams = [], [], []

    @staticmethod
    def _ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: HIP error {rc}")

    def malloc(self, nbytes):
        p = ctypes.c_void_p()
        self._ok(self.L.hipMalloc(ctypes.byref(p), max(int(nbytes), 16)), "hipMalloc")
        self._dev.append(p.value)
        return p.value

    def host_malloc(self, nbytes):
        """pinned host memory: (pointer, uint8 view of it)"""
        p = ctypes.c_void_p()
        n = max(int(nbytes), 16)
        self._ok(self.L.hipHostMalloc(ctypes.byref(p), n, 0), "hipHostMalloc")
        self._host.append(p.value)
        return p.value, np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(p.value))

    def stream(self):
        s = ctypes.c_void_p()
        self._ok(self.L.hipStreamCreate(ctypes.byref(s)), "hipStreamCreate")
        self._streams.append(s.value)
        return s.value

    def sync(self, stream):
        self._ok(self.L.hipStreamSynchronize(stream), "hipStreamSynchronize")

    def put(self, dst, arr):
        """a host array's bytes to device memory (synchronous)"""
        a = np.ascontiguousarray(arr)
        if a.nbytes:
            self._ok(self.L.hipMemcpy(dst, a.ctypes.data, a.nbytes, H2D), "hipMemcpy")

    def put_async(self, dst, src_ptr, nbytes, stream):
        if nbytes:
            self._ok(self.L.hipMemcpyAsync(dst, src_ptr, int(nbytes), H2D, stream), "hipMemcpyAsync")

    def get(self, src, nbytes):
        out = np.zeros(int(nbytes), np.uint8)
        if nbytes:
            self._ok(self.L.hipMemcpy(out.ctypes.data, src, int(nbytes), D2H), "hipMemcpy")
        return out

    def upload(self, arr):
        """a fresh device buffer holding the array's bytes"""
        a = np.ascontiguousarray(arr)
        p = self.malloc(a.nbytes)
        self.put(p, a)
        return p

    def release(self):
        """frees everything handed out (the caller has synchronised whatever used it)"""
        for s in self._streams:
            self.L.hipStreamSynchronize(s)
            self.L.hipStreamDestroy(s)
        for p in self._dev:
            self.L.hipFree(p)
        for p in self._host:
            self.L.hipHostFree(p)
        self._dev, self._host, self._streams = [], [], []
