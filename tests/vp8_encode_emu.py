"""The CPU emulation of the device lossy WebP coder (tests/vp8_encode_emulate.cpp over csrc/vp8_encode_core.hpp) for the tests:
built once with g++, called through ctypes; the frames and qualities the CPU and the GPU tests share; Pillow's side."""
import ctypes as C
import io
import os
import subprocess
import tempfile

import numpy as np

from tests import webp_frames as F

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "vp8_encode_emulate.cpp")
QUALITIES = (0, 50, 85, 100)
_EMU = {}


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="vp8_encode_emulate_")
        so = os.path.join(d, "libvp8_encode_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-function", SRC, "-o", so], check=True)
        lib = C.CDLL(so)
        lib.vp8e_emu_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                        C.c_void_p, C.c_void_p]
        lib.vp8e_emu_max_file_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
        lib.vp8e_emu_max_file_bytes.restype = C.c_uint64
        lib.vp8e_emu_quality_to_index.argtypes = [C.c_float]
        lib.vp8e_emu_quality_to_index.restype = C.c_uint32
        lib.vp8e_emu_filter_level.argtypes = [C.c_uint32]
        lib.vp8e_emu_filter_level.restype = C.c_uint32
        lib.vp8e_emu_cost.argtypes = [C.c_uint32]
        lib.vp8e_emu_cost.restype = C.c_uint32
        lib.vp8e_emu_bool.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]
        lib.vp8e_emu_bool.restype = C.c_uint32
        _EMU["lib"] = lib
    return _EMU["lib"]


STATS = ("errors", "index", "updates", "skipped", "alpha", "partitions", "filter_level", "dc", "tm", "v", "h", "first_bytes", "skip_prob", "max_level")


def encode(bgra, quality, alpha_meaningful=True, filter_num=-1, cap=None):
    """BGRA [h, w, 4] -> (file bytes, expected BGRA [h, w, 4], stats dict); (None, None, stats) when the file does not fit cap"""
    src = np.ascontiguousarray(bgra, np.uint8)
    h, w = src.shape[:2]
    L = emulator()
    if cap is None:
        cap = int(L.vp8e_emu_max_file_bytes(w, h, 1 if alpha_meaningful else 0))
    out, expect, stats, n = np.zeros(cap, np.uint8), np.zeros((h, w, 4), np.uint8), np.zeros(16, np.uint32), C.c_size_t(0)
    rc = L.vp8e_emu_encode(src.ctypes.data, w, h, w * 4, 1 if alpha_meaningful else 0, float(quality), filter_num, out.ctypes.data, cap, C.byref(n),
                           expect.ctypes.data, stats.ctypes.data)
    st = dict(zip(STATS, (int(v) for v in stats)), length=int(n.value))
    assert rc in (0, 2), rc
    if rc:
        return None, None, st
    return out[:n.value].tobytes(), expect, st


def bool_bytes(bits, probs):
    """(bit, probability) pairs through the core's bool coder"""
    b, p = np.asarray(bits, np.uint8), np.asarray(probs, np.uint8)
    out = np.zeros(len(b) + 16, np.uint8)
    n = emulator().vp8e_emu_bool(b.ctypes.data, p.ctypes.data, len(b), out.ctypes.data, out.size)
    return out[:n].tobytes()


def checkers(w, h, period):
    """black and white squares: every clamp and the level limit"""
    y, x = np.mgrid[0:h, 0:w]
    f = np.empty((h, w, 4), np.uint8)
    f[...] = (((x // period + y // period) & 1) * 255)[..., None]
    f[..., 3] = 255
    return f


def small_frames():
    """name -> (BGRA, alpha_meaningful): one macroblock, ragged edges, one macroblock row, all eight partitions, alpha"""
    return {
        "1x1": (F.photo(1, 1), False),
        "15x17": (F.photo(15, 17), False),
        "16x16": (F.photo(16, 16), False),
        "17x33": (F.photo(17, 33), False),
        "48x32": (F.photo(48, 32), False),
        "16x144": (F.photo(16, 144), False),
        "alpha_90x61": (F.photo(90, 61, alpha=True), True),
        "opaque_alpha_40x24": (F.photo(40, 24), True),
        "flat_40x40": (F.one_colour(40, 40), False),
        "noise_33x31": (F.noise(33, 31), False),
        "checkers16_64x48": (checkers(64, 48, 16), False),
        "checkers4_40x36": (checkers(40, 36, 4), False),
    }


def photo_frame():
    return F.photo(800, 450)


def pillow_bgra(data):
    """libwebp's decode of a file -> (BGRA [h, w, 4], Pillow's mode)"""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    mode = im.mode
    rgba = np.asarray(im.convert("RGBA"))
    return np.ascontiguousarray(rgba[..., [2, 1, 0, 3]]), mode


def pillow_lossy(bgra, quality, method):
    """libwebp's own lossy file of the frame's colour -> (bytes, decoded BGRA)"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(bgra[..., [2, 1, 0]]), "RGB").save(buf, "WEBP", quality=quality, method=method)
    return buf.getvalue(), pillow_bgra(buf.getvalue())[0]


def psnr(a, b):
    """over B, G, R"""
    d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
    return 10.0 * np.log10(255.0 ** 2 / max(float(np.mean(d * d)), 1e-12))
