"""The CPU emulation of the device lossy WebP coder with stage flags (tests/vp8_encode_intra4_emulate.cpp over
csrc/vp8_encode_core.hpp: IFHIP_VP8_ENC_INTRA4, the sixteen 4x4 luma modes) for the tests: built once with g++, called through
ctypes; the frames the CPU and the GPU tests share beside those of tests/vp8_encode_emu.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from tests import vp8_encode_emu as E
from tests import webp_frames as F

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "vp8_encode_intra4_emulate.cpp")
INTRA4 = 1                              # include/imageflow_hip_webp_lossy_enc.h IFHIP_VP8_ENC_INTRA4
NAIVE_Y2 = 1 << 8                       # the emulation's test-only switch: Y2 contexts from the neighbour's own bit 24
QUALITIES = E.QUALITIES
_EMU = {}


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="vp8_encode_intra4_emulate_")
        so = os.path.join(d, "libvp8_encode_intra4_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unused-function", SRC, "-o", so], check=True)
        lib = C.CDLL(so)
        lib.vp8e4_emu_encode.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                         C.c_void_p, C.c_void_p, C.c_void_p]
        lib.vp8e4_emu_max_file_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32]
        lib.vp8e4_emu_max_file_bytes.restype = C.c_uint64
        lib.vp8e4_emu_mode_bytes.argtypes = [C.c_uint32]
        lib.vp8e4_emu_mode_bytes.restype = C.c_uint32
        lib.vp8e4_emu_dearest_leaf.restype = C.c_uint32
        _EMU["lib"] = lib
    return _EMU["lib"]


STATS = E.STATS + ("n_i4", "borders")


def max_file_bytes(w, h, alpha_meaningful, flags=INTRA4):
    return int(emulator().vp8e4_emu_max_file_bytes(w, h, 1 if alpha_meaningful else 0, flags))


def encode(bgra, quality, alpha_meaningful=True, flags=INTRA4, cap=None, penalty=-1):
    """BGRA [h, w, 4] -> (file bytes, expected BGRA [h, w, 4], stats dict with `modes` [mbh, mbw]: 0..3, or 4 for B_PRED);
    (None, None, stats) when the file does not fit cap.  penalty: a member of kVp8eIntra4Penalty's family to measure (-1: the coder's)"""
    src = np.ascontiguousarray(bgra, np.uint8)
    h, w = src.shape[:2]
    L = emulator()
    if cap is None:
        cap = max_file_bytes(w, h, alpha_meaningful, flags & INTRA4)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    out, expect, stats, n = np.zeros(cap, np.uint8), np.zeros((h, w, 4), np.uint8), np.zeros(16, np.uint32), C.c_size_t(0)
    modes = np.zeros((mbh, mbw), np.uint8)
    rc = L.vp8e4_emu_encode(src.ctypes.data, w, h, w * 4, 1 if alpha_meaningful else 0, float(quality), flags, penalty, out.ctypes.data, cap, C.byref(n), expect.ctypes.data,
                            stats.ctypes.data, modes.ctypes.data)
    st = dict(zip(STATS, (int(v) for v in stats)), length=int(n.value), modes=modes, n_mbs=mbw * mbh)
    st["row_borders"], st["column_borders"] = st["borders"] & 0xFFFF, st["borders"] >> 16
    assert rc in (0, 2), rc
    if rc:
        return None, None, st
    return out[:n.value].tobytes(), expect, st


def mix(mbw, mbh, textured, seed):
    """Macroblocks of texture where textured(mbx, mby), one flat colour per macroblock elsewhere.  The texture is diagonal
    stripes three pixels wide under a little noise: no whole-macroblock mode predicts it, the diagonal 4x4 modes do, at every
    quality -- plain noise, which nothing predicts, goes to 16x16 at the low qualities and would not give both kinds there.
    The flat macroblocks differ in colour, so each has a Y2 block with a level: the contexts a B_PRED macroblock must hand on."""
    h, w = 16 * mbh, 16 * mbw
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(seed)
    f = np.empty((h, w, 4), np.uint8)
    f[..., :3] = ((((x + y) // 3) % 2) * 150 + 40 + rng.integers(0, 24, (h, w)))[..., None]
    f[..., 3] = 255
    for my in range(mbh):
        for mx in range(mbw):
            if not textured(mx, my):
                f[16 * my:16 * my + 16, 16 * mx:16 * mx + 16, :3] = (30 + 37 * mx % 200, 200 - 41 * my, 60 + 23 * (mx + 2 * my))
    return f


def mix_frames():
    """name -> (BGRA, alpha_meaningful): B_PRED and 16x16 macroblocks adjacent in both directions.  mix_64x48: a checkerboard,
    texture where mbx + mby is odd.  mix_cols_80x32: flat, textured, flat, textured, textured along a row, the second row
    shifted by one -- a B_PRED macroblock between two 16x16 ones in both rows (the left Y2 chain) and the kinds adjacent
    vertically as well; the checkerboard's three rows have the same for the chain from above."""
    return {
        "mix_64x48": (mix(4, 3, lambda x, y: (x + y) & 1, 71), False),
        "mix_cols_80x32": (mix(5, 2, lambda x, y: (x - y) % 5 not in (0, 2), 72), False),
    }


def frames():
    out = dict(E.small_frames())
    out.update(mix_frames())
    return out
