"""Progressive (SOF2) JPEG files entropy-decoded on the GPU (csrc/jpeg_progressive_decode.hip; the entry points of
include/imageflow_hip_jpeg_progressive.h): the host front end prepares a file -- scans, streams, dependency levels -- and one
batch call decodes any mix of prepared files into the coefficient planes of the pixel stage, which never leave HBM.
`MethodNotImplemented` from prepare, or a nonzero status word, means: ask the host reader (ifhip_jpeg_read_coefficients_host)."""
import ctypes as C

import numpy as np
import torch

from .. import _native

NO_SUCH_CODE, PAST_SE, REFINE_SIZE, OUT_OF_BITS, BOUNDS = 1, 2, 4, 8, 16


def _bind():
    L = _native.lib()
    if getattr(L, "_jpeg_progressive_bound", False):
        return L
    L.ifhip_jpeg_progressive_prepare.argtypes = [C.POINTER(C.c_void_p), C.c_char_p, C.c_size_t]
    L.ifhip_jpeg_progressive_prepared_info.argtypes = [C.c_void_p] + [C.c_void_p] * 11
    L.ifhip_jpeg_progressive_prepared_destroy.argtypes = [C.c_void_p]
    L.ifhip_jpeg_progressive_prepared_destroy.restype = None
    L.ifhip_jpeg_progressive_decode_batch_device.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                             C.c_void_p, C.c_void_p]
    L.ifhip_jpeg_progressive_decode.argtypes = [C.c_char_p, C.c_size_t] + [C.c_void_p] * 5
    L._jpeg_progressive_bound = True
    return L


class PreparedProgressive:
    """ifhip_jpeg_progressive_prepared: one file behind the host front end.  Raises (MethodNotImplemented) for a file the device
    path does not take."""

    def __init__(self, data: bytes):
        L = _bind()
        self._h = C.c_void_p()
        data = bytes(data)
        _native.check(L.ifhip_jpeg_progressive_prepare(C.byref(self._h), data, len(data)))
        w, h, n = C.c_uint32(), C.c_uint32(), C.c_int()
        hs, vs = np.zeros(3, np.uint8), np.zeros(3, np.uint8)
        bw, bh = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
        qt = np.zeros((3, 64), np.uint16)
        ns, nt, nl = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _native.check(L.ifhip_jpeg_progressive_prepared_info(self._h, C.addressof(w), C.addressof(h), C.addressof(n), hs.ctypes.data,
                                                             vs.ctypes.data, bw.ctypes.data, bh.ctypes.data, qt.ctypes.data,
                                                             C.addressof(ns), C.addressof(nt), C.addressof(nl)))
        self.width, self.height, self.ncomp = w.value, h.value, n.value
        self.h_samp, self.v_samp = [int(v) for v in hs[:self.ncomp]], [int(v) for v in vs[:self.ncomp]]
        self.blocks_w, self.blocks_h = [int(v) for v in bw], [int(v) for v in bh]
        self.qt = qt
        self.n_scans, self.n_streams, self.n_levels = ns.value, nt.value, nl.value

    @property
    def handle(self):
        return self._h

    def plane_shape(self, c):
        return (self.blocks_h[c], self.blocks_w[c], 64)

    def close(self):
        if self._h:
            _bind().ifhip_jpeg_progressive_prepared_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def decode_batch_device(prepared, coef=None, status=None, device="cuda:0"):
    """prepared: PreparedProgressive objects of any mix of geometries -> (coef, status): coef[i] the list of file i's int16 cuda
    planes [bh_c, bw_c, 64], status an int32 cuda tensor of the files' status words.  Asynchronous on the current stream."""
    L = _bind()
    dev = torch.device(device)
    n = len(prepared)
    if coef is None:
        coef = [[torch.empty(p.plane_shape(c), dtype=torch.int16, device=dev) for c in range(p.ncomp)] for p in prepared]
    if status is None:
        status = torch.empty(n, dtype=torch.int32, device=dev)
    handles = (C.c_void_p * n)(*[p.handle.value for p in prepared])
    ptrs = [(C.c_void_p * n)(*[(coef[i][c].data_ptr() if c < prepared[i].ncomp else None) for i in range(n)]) for c in range(3)]
    sizes = (C.c_size_t * (3 * n))(*[(coef[i][c].numel() * 2 if c < prepared[i].ncomp else 0) for i in range(n) for c in range(3)])
    stream = torch.cuda.current_stream(dev).cuda_stream
    with torch.cuda.device(dev):
        _native.check(L.ifhip_jpeg_progressive_decode_batch_device(handles, n, ptrs[0], ptrs[1], ptrs[2], sizes, status.data_ptr(),
                                                                   C.c_void_p(stream)))
    return coef, status


def decode_host(data: bytes):
    """ifhip_jpeg_progressive_decode: one file, host buffers -> (planes [int16 arrays], qt uint16 [3][64], status word)"""
    L = _bind()
    p = PreparedProgressive(data)
    try:
        planes = [np.zeros(p.plane_shape(c), np.int16) for c in range(p.ncomp)]
    finally:
        p.close()
    ptr = [planes[c].ctypes.data if c < len(planes) else None for c in range(3)]
    qt = np.zeros((3, 64), np.uint16)
    word = C.c_uint32()
    data = bytes(data)
    _native.check(L.ifhip_jpeg_progressive_decode(data, len(data), ptr[0], ptr[1], ptr[2], qt.ctypes.data, C.addressof(word)))
    return planes, qt, word.value
