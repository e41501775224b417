"""tests/webp_indexed_emulate.cpp built with g++ and bound with ctypes: the CPU emulation of the device WebP coder with its
stage flags, for the tests that check its files (tests/test_webp_indexed_coder.py) and for the GPU tests that compare the
device's bytes with them."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import webp_emulation as PLAIN

HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = {}
COLOR_INDEXING = 1
STATS = PLAIN.STATS + ("indexed", "colours", "width_bits", "packed_width", "plain_bytes", "indexed_bytes")


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="webp_indexed_emulate_")
        so = os.path.join(d, "libwebp_indexed_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", os.path.join(HERE, "webp_indexed_emulate.cpp"), "-o", so], check=True)
        lib = C.CDLL(so)
        lib.webp_ix_index_width_bits.argtypes = [C.c_uint32]
        lib.webp_ix_index_width_bits.restype = C.c_uint32
        lib.webp_ix_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                       C.c_void_p]
        _EMU["lib"] = lib
    return _EMU["lib"]


def encode(bgra, alpha_meaningful=True, flags=COLOR_INDEXING, cap=None):
    """(the emulated file, the emulation's counters) of a BGRA frame [h, w, 4]; with a cap that is too small: (None, needed)"""
    lib = emulator()
    src = np.ascontiguousarray(bgra, np.uint8)
    h, w = src.shape[:2]
    room = PLAIN.max_file_bytes(w, h) if cap is None else cap
    out, n, stats = np.zeros(max(room, 1), np.uint8), C.c_size_t(0), np.zeros(len(STATS), np.uint32)
    rc = lib.webp_ix_encode(src.ctypes.data, w, h, src.strides[0], 1 if alpha_meaningful else 0, flags, out.ctypes.data, room, C.byref(n), stats.ctypes.data)
    if rc == 2:
        return None, n.value
    assert rc == 0, rc
    st = dict(zip(STATS, (int(v) for v in stats)))
    assert st["inconsistencies"] == 0, "the parse must tile every segment and the layout's sizes must be the writer's"
    return out[:n.value].tobytes(), st
