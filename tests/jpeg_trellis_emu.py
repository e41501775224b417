"""tests/jpeg_trellis_emulate.cpp built with g++ and wrapped: the CPU emulation that defines the mozjpeg preset's trellis
stage (csrc/jpeg_trellis_core.hpp).  Shared by the CPU tests and the GPU tests; a frame's planes are computed once."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
S420, S444 = ([2, 1, 1], [2, 1, 1]), ([1, 1, 1], [1, 1, 1])
LAMBDA_ONE = 256                        # csrc/jpeg_trellis_core.hpp kTrLambdaOne
_EMU = {}


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="jpeg_trellis_emulate_")
        so = os.path.join(d, "libjpeg_trellis_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas",
                        os.path.join(HERE, "jpeg_trellis_emulate.cpp"), "-o", so], check=True)
        lib = C.CDLL(so)
        lib.jpeg_trellis_emulate.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 8
        lib.jpeg_trellis_search_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p]
        lib.jpeg_trellis_search_block.restype = None
        lib.jpeg_trellis_block_cost.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        lib.jpeg_trellis_block_cost.restype = C.c_int64
        lib.jpeg_trellis_rate_table.argtypes = [C.c_void_p, C.c_void_p]
        lib.jpeg_trellis_rate_table.restype = None
        _EMU["lib"] = lib
    return _EMU["lib"]


def emulate(bgra, qt, sampling=S420, lambda_scale=LAMBDA_ONE):
    """bgra: uint8 [h][w][4]; qt: uint16 [3][64].  Returns dict(coef, raw: 3 int16 planes [bh][bw][64] each, len: uint8 [2][256],
    guards: the two overflow-guard counters)."""
    h, w = bgra.shape[:2]
    hs, vs = sampling
    bw, bh = O.jpeg_block_geometry(w, h, hs, vs)
    src = np.ascontiguousarray(bgra, np.uint8)
    q = np.ascontiguousarray(qt, np.uint16)
    coef = [np.zeros((bh[c], bw[c], 64), np.int16) for c in range(3)]
    raw = [np.zeros((bh[c], bw[c], 64), np.int16) for c in range(3)]
    lens, guards = np.zeros((2, 256), np.uint8), np.zeros(2, np.int64)
    h8, v8 = np.array(hs, np.uint8), np.array(vs, np.uint8)
    rc = emulator().jpeg_trellis_emulate(src.ctypes.data, w, h, w * 4, h8.ctypes.data, v8.ctypes.data, q.ctypes.data, int(lambda_scale),
                                         *[p.ctypes.data for p in coef], *[p.ctypes.data for p in raw], lens.ctypes.data, guards.ctypes.data)
    assert rc == 0
    return {"coef": coef, "raw": raw, "len": lens, "guards": (int(guards[0]), int(guards[1])), "bw": bw, "bh": bh}


def search_block(raw, Q, lens, lambda_scale=LAMBDA_ONE):
    """One block (natural order int16 [64]) -> (levels int16 [64], cost, guards)."""
    raw, Q, lens = np.ascontiguousarray(raw, np.int16), np.ascontiguousarray(Q, np.uint16), np.ascontiguousarray(lens, np.uint8)
    level, cost, guards = np.zeros(64, np.int16), C.c_int64(0), np.zeros(2, np.int64)
    emulator().jpeg_trellis_search_block(raw.ctypes.data, Q.ctypes.data, lens.ctypes.data, int(lambda_scale), level.ctypes.data, C.byref(cost),
                                         guards.ctypes.data)
    return level, cost.value, (int(guards[0]), int(guards[1]))


def block_cost(raw, Q, level, lens, lambda_scale=LAMBDA_ONE):
    raw, Q, lens = np.ascontiguousarray(raw, np.int16), np.ascontiguousarray(Q, np.uint16), np.ascontiguousarray(lens, np.uint8)
    level = np.ascontiguousarray(level, np.int16)
    return int(emulator().jpeg_trellis_block_cost(raw.ctypes.data, Q.ctypes.data, level.ctypes.data, lens.ctypes.data, int(lambda_scale)))


def rate_table(hist):
    hist, lens = np.ascontiguousarray(hist, np.uint32), np.zeros(256, np.uint8)
    emulator().jpeg_trellis_rate_table(hist.ctypes.data, lens.ctypes.data)
    return lens


def real_blocks(w, h, sampling):
    """per component (real block columns, real block rows): the rest of a plane are dummy blocks"""
    hs, vs = sampling
    hmax, vmax = max(hs), max(vs)
    ceil = lambda a, b: -(-a // b)
    return [(ceil(ceil(w * hs[c], hmax), 8), ceil(ceil(h * vs[c], vmax), 8)) for c in range(3)]


def quality_tables(quality):
    from imageflow_amd.codecs.mozjpeg import quant_tables_for_quality
    return quant_tables_for_quality(quality)


FRAMES = ("photo", "noise", "flat")


@functools.lru_cache(maxsize=None)
def frame(kind, w, h):
    from tests import webp_frames as F
    f = {"photo": F.photo, "noise": F.noise, "flat": F.flat}[kind](w, h)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def reference(kind, w, h, quality, sampling_name="420", lambda_scale=LAMBDA_ONE):
    """The emulation's result for one of the named frames: computed once, shared, left unchanged."""
    r = emulate(frame(kind, w, h), quality_tables(quality), S420 if sampling_name == "420" else S444, lambda_scale)
    for p in r["coef"] + r["raw"]:
        p.setflags(write=False)
    return r
