"""tests/webp_emulate.cpp built with g++ and bound with ctypes: the CPU emulation of the device WebP coder, for the tests
that check its files (tests/test_webp_device_coder.py) and for the GPU tests that compare the device's bytes with them."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = {}
STATS = ("inconsistencies", "matches_left", "matches_row", "groups", "segments", "fixed_codes", "payload_bits", "tokens", "matches_4096",
         "pixel_bits", "second_segment_bit", "head_bits", "constant_bands", "literal_bands")


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="webp_emulate_")
        so = os.path.join(d, "libwebp_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", os.path.join(HERE, "webp_emulate.cpp"), "-o", so], check=True)
        lib = C.CDLL(so)
        lib.webp_emu_max_file_bytes.argtypes = [C.c_uint32, C.c_uint32]
        lib.webp_emu_max_file_bytes.restype = C.c_uint64
        lib.webp_emu_shape.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        lib.webp_emu_predict.argtypes = [C.c_uint32] * 5
        lib.webp_emu_predict.restype = C.c_uint32
        lib.webp_emu_prefix.argtypes = [C.c_uint32, C.c_void_p]
        lib.webp_emu_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
        _EMU["lib"] = lib
    return _EMU["lib"]


def max_file_bytes(w, h):
    return int(emulator().webp_emu_max_file_bytes(w, h))


def shape(w, h):
    g = np.zeros(8, np.uint32)
    emulator().webp_emu_shape(w, h, g.ctypes.data)
    return dict(zip(("w", "h", "tiles_x", "tiles_y", "ent_x", "n_bands", "segs_per_band", "n_segs"), (int(v) for v in g)))


def encode(bgra, alpha_meaningful=True, cap=None):
    """(the emulated file, the emulation's counters) of a BGRA frame [h, w, 4]; with a cap that is too small: (None, needed)"""
    lib = emulator()
    src = np.ascontiguousarray(bgra, np.uint8)
    h, w = src.shape[:2]
    room = max_file_bytes(w, h) if cap is None else cap
    out, n, stats = np.zeros(max(room, 1), np.uint8), C.c_size_t(0), np.zeros(len(STATS), np.uint32)
    rc = lib.webp_emu_encode(src.ctypes.data, w, h, src.strides[0], 1 if alpha_meaningful else 0, out.ctypes.data, room, C.byref(n), stats.ctypes.data)
    if rc == 2:
        return None, n.value
    assert rc == 0, rc
    st = dict(zip(STATS, (int(v) for v in stats)))
    assert st["inconsistencies"] == 0, "the parse must tile every segment and the layout's sizes must be the writer's"
    return out[:n.value].tobytes(), st
