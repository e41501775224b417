"""The device PNG coder's algorithm without a device (csrc/png_encode_core.hpp: filters and their choice, the match
search, symbol tables, length-limited code construction, the dynamic header, bit placement, checksum combination -- what the
gfx950 kernels of csrc/png_encode.hip are built from).  tests/png_emulate.cpp runs the passes lane by lane on the CPU;
zlib.decompress must accept every stream and return the bytes that went in.  The GPU tests
(tests/test_gpu_png_encode.py) check the kernels' files the same way."""
import ctypes as C
import io
import os
import subprocess
import tempfile
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import png_oracle as P

HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = {}
CHUNK = 32768


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="png_emulate_")
        so = os.path.join(d, "libpng_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", os.path.join(HERE, "png_emulate.cpp"), "-o", so], check=True)
        lib = C.CDLL(so)
        lib.png_emu_filter.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.png_emu_deflate.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p]
        lib.png_emu_file.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        for name in ("png_emu_crc32", "png_emu_adler32"):
            getattr(lib, name).argtypes = [C.c_void_p, C.c_uint32]
            getattr(lib, name).restype = C.c_uint32
        for name in ("png_emu_crc_combine", "png_emu_adler_combine"):
            getattr(lib, name).argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
            getattr(lib, name).restype = C.c_uint32
        lib.png_emu_symbols.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
        _EMU["lib"] = lib
    return _EMU["lib"]


def deflate(stream, bpp=3, pitch=1 + 3 * 100, level=6):
    """The emulated zlib stream of `stream` and the emulation's counters."""
    lib = emulator()
    src = np.frombuffer(bytes(stream), np.uint8)
    cap = len(src) + 5 * (len(src) // CHUNK + 1) + 64
    out, n, stats = np.zeros(cap, np.uint8), C.c_size_t(0), np.zeros(10, np.uint32)
    rc = lib.png_emu_deflate(src.ctypes.data, src.size, bpp, pitch, level, out.ctypes.data, cap, C.byref(n), stats.ctypes.data)
    assert rc == 0, rc
    assert stats[0] == 0, "the parse must tile every chunk and the plan's size must be the writer's"
    z = out[:n.value].tobytes()
    assert int(stats[6]) == zlib.crc32(z), "CRC-32 combined from the slices"
    return z, dict(fixed_distance=int(stats[1]), hashed=int(stats[2]), stored=int(stats[3]), fixed=int(stats[4]), dynamic=int(stats[5]),
                   tokens=int(stats[7]), len3=int(stats[8]), len258=int(stats[9]))


def stored_bound(n):
    chunks = -(-n // CHUNK)
    return n + 5 * -(-n // 65535) + 6 + 5 * chunks


def filtered(pixels):
    lib = emulator()
    h, w, bpp = pixels.shape
    bgra = np.full((h, w, 4), 255, np.uint8)
    bgra[..., 0], bgra[..., 1], bgra[..., 2] = pixels[..., 2], pixels[..., 1], pixels[..., 0]
    if bpp == 4:
        bgra[..., 3] = pixels[..., 3]
    out = np.zeros(h * (1 + w * bpp), np.uint8)
    lib.png_emu_filter(bgra.ctypes.data, w, h, 4 * w, bpp, out.ctypes.data)
    return out.tobytes()


def photo_stream(w=800, h=120):
    return P.filter_image(P.photo_frame(w, h))[1], 1 + 3 * w


STREAMS = {
    "zeros": lambda: (bytes(100000), 301),
    "one_byte": lambda: (b"\x5a" * 70001, 301),
    "noise": lambda: (np.random.default_rng(1).integers(0, 256, 90000, dtype=np.uint8).tobytes(), 301),
    "photo": photo_stream,
    "tiny": lambda: (b"\x01", 4),
    "exact_chunk": lambda: (np.random.default_rng(2).integers(0, 4, CHUNK, dtype=np.uint8).tobytes(), 301),
    "chunk_plus_one": lambda: (np.random.default_rng(3).integers(0, 4, CHUNK + 1, dtype=np.uint8).tobytes(), 301),
    "skewed": lambda: ((np.random.default_rng(4).geometric(0.02, 120000) % 256).astype(np.uint8).tobytes(), 301),
}


@pytest.mark.parametrize("name", sorted(STREAMS))
@pytest.mark.parametrize("level", [6, 0])
def test_zlib_inflates_every_emulated_stream(name, level):
    stream, pitch = STREAMS[name]()
    z, st = deflate(stream, 3, pitch, level)
    assert zlib.decompress(z) == stream
    assert len(z) <= stored_bound(len(stream))
    if level == 0:
        assert P.stored_only(z) and st["fixed"] == st["dynamic"] == 0


def test_runs_are_found_by_the_fixed_distances():
    stream = bytes(1 << 20)
    z, st = deflate(stream)
    assert zlib.decompress(z) == stream
    assert len(z) <= len(stream) // 100
    assert st["fixed_distance"] > 0 and st["stored"] == 0


def test_noise_falls_back_to_stored_blocks():
    stream = np.random.default_rng(5).integers(0, 256, 3 * CHUNK, dtype=np.uint8).tobytes()
    z, st = deflate(stream)
    assert st["stored"] == 3 and zlib.decompress(z) == stream


def test_a_chunk_with_a_single_distance_and_one_with_none():
    # one distinct distance: a period of 7 bytes that none of the fixed candidates (1, 3, 298, 301, 304) divides into... 7 is
    # found through the hash table only; every match then has distance 7 -> the one-bit distance code
    period = bytes([3, 1, 4, 1, 5, 9, 2])
    stream = period * 3000
    z, st = deflate(stream, 3, 301)
    assert zlib.decompress(z) == stream and st["stored"] == 0
    # no match at all: every 3-byte window differs (a de Bruijn-like counter), literals only -> a distance set nobody uses
    vals = np.arange(20000, dtype=np.uint32)
    stream = np.stack([vals & 63, 64 + ((vals >> 6) & 63), 128 + ((vals >> 12) & 63)], 1).astype(np.uint8).tobytes()
    z, st = deflate(stream, 3, 100003)
    assert zlib.decompress(z) == stream
    assert st["fixed_distance"] == st["hashed"] == 0 and st["dynamic"] > 0


def test_lengths_3_and_258():
    rng = np.random.default_rng(6)
    parts = []
    for i in range(400):
        parts.append(rng.integers(0, 256, 40, dtype=np.uint8).tobytes())
        parts.append(bytes([(i * 7) & 255]) * 4)                      # a literal and a 3-byte match at distance 1
        parts.append(rng.integers(0, 256, 9, dtype=np.uint8).tobytes())
        parts.append(bytes([i & 255]) * 300)                          # a run: 258 and a rest
    stream = b"".join(parts)
    z, st = deflate(stream, 3, 301)
    assert zlib.decompress(z) == stream
    assert st["len3"] >= 300 and st["len258"] >= 300
    lib = emulator()
    out = np.zeros(6, np.uint32)
    for length, dist, want in ((3, 1, (257, 0, 0, 0, 0, 0)), (258, 32768, (285, 0, 0, 29, 13, 8191)), (257, 5, (284, 5, 30, 4, 1, 0)),
                               (11, 4, (265, 1, 0, 3, 0, 0)), (130, 24577, (280, 4, 15, 29, 13, 0))):
        lib.png_emu_symbols(length, dist, out.ctypes.data)
        assert tuple(int(v) for v in out) == want, (length, dist)


@pytest.mark.parametrize("shape", [(1, 1, 3), (1, 300, 4), (300, 1, 3), (23, 37, 4), (120, 800, 3), (64, 64, 4)])
def test_emulated_filter_choice_equals_the_oracles(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    h, w, bpp = shape
    px = P.photo_frame(w, h, 3) if bpp == 3 else np.dstack([P.photo_frame(w, h, 4), rng.integers(0, 256, (h, w), dtype=np.uint8)])
    px[: h // 3] = 77                                                 # a flat band: ties between filters
    types, stream = P.filter_image(px)
    assert filtered(px) == stream
    z, _ = deflate(stream, bpp, 1 + w * bpp)
    assert zlib.decompress(z) == stream


def test_a_framed_file_opens_in_pillow():
    lib = emulator()
    px = P.product_frame(96)
    stream = filtered(px)
    z, _ = deflate(stream, 4, 1 + 4 * 96)
    out = np.zeros(len(z) + 256, np.uint8)
    n = lib.png_emu_file(np.frombuffer(z, np.uint8).ctypes.data, len(z), 96, 96, 6, out.ctypes.data)
    data = out[:n].tobytes()
    d = P.decode(data)
    P.check_ancillary(d["chunks"])
    assert np.array_equal(d["pixels"], px)
    im = Image.open(io.BytesIO(data))
    assert im.format == "PNG" and im.mode == "RGBA" and im.size == (96, 96)
    assert np.array_equal(np.asarray(im), px)


def test_checksum_combination_on_random_splits():
    lib = emulator()
    rng = np.random.default_rng(8)
    for _ in range(60):
        n = int(rng.integers(0, 5000))
        data = rng.integers(0, 256, n, dtype=np.uint8)
        cut = int(rng.integers(0, n + 1))
        a, b = data[:cut].copy(), data[cut:].copy()
        assert lib.png_emu_crc32(data.ctypes.data, n) == zlib.crc32(data.tobytes())
        assert lib.png_emu_crc_combine(zlib.crc32(a.tobytes()), zlib.crc32(b.tobytes()), b.size) == zlib.crc32(data.tobytes())
        assert lib.png_emu_adler32(data.ctypes.data, n) == zlib.adler32(data.tobytes())
        assert lib.png_emu_adler_combine(zlib.adler32(a.tobytes()), zlib.adler32(b.tobytes()), b.size) == zlib.adler32(data.tobytes())
    # a long second piece: the shift by square and multiply
    a, blen = b"head", 3_000_000_000
    assert lib.png_emu_crc_combine(zlib.crc32(a), zlib.crc32(bytes(1000)), 1000) == zlib.crc32(a + bytes(1000))
    big = bytes(1 << 20)
    c, ad = zlib.crc32(a), zlib.adler32(a)
    for _ in range(3):
        c, ad = zlib.crc32(big, c), zlib.adler32(big, ad)
    assert lib.png_emu_crc_combine(zlib.crc32(a), zlib.crc32(big * 3), 3 << 20) == c
    assert lib.png_emu_adler_combine(zlib.adler32(a), zlib.adler32(big * 3), 3 << 20) == ad
    assert blen > 1 << 31


def test_photo_and_product_streams_meet_the_level_1_reference():
    """The size condition of the GPU test, on the emulation: not larger than zlib level 1 with Z_FILTERED on the oracle's
    own filtered stream (the frames are smaller here to keep the CPU run short)."""
    for px in (P.photo_frame(800, 200), P.product_frame(400)):
        stream = P.filter_image(px)[1]
        z, st = deflate(stream, px.shape[2], 1 + px.shape[1] * px.shape[2])
        r1 = P.reference_size(stream, 1)
        print(px.shape, "S", len(z), "R1", r1, "R6", P.reference_size(stream, 6), st)
        assert zlib.decompress(z) == stream
        assert len(z) <= r1
