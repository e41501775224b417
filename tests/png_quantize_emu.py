"""The CPU emulation of the device palette coder for the tests: tests/png_quantize_emulate.cpp (with tests/png_emulate.cpp for
the zlib stream) built with g++ once per session, a wrapper around its one entry, the frames the tests share and the parts
of a palette file."""
import ctypes as C
import os
import struct
import subprocess
import tempfile
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = {}
QUALITY_TOO_LOW, FILE_OVERFLOW = 2, 1
DISTANCE_UNIT = 6 * 65025 * 65025


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="png_quantize_emulate_")
        so = os.path.join(d, "libpng_quantize_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", os.path.join(HERE, "png_quantize_emulate.cpp"),
                        os.path.join(HERE, "png_emulate.cpp"), "-o", so], check=True)
        lib = C.CDLL(so)
        lib.pq_emu_quantize.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_int, C.c_int,
                                        C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.pq_emu_quality_bound.argtypes = [C.c_uint32]
        lib.pq_emu_quality_bound.restype = C.c_uint64
        lib.pq_emu_distance.argtypes = [C.c_uint32, C.c_uint32]
        lib.pq_emu_distance.restype = C.c_uint64
        _EMU["lib"] = lib
    return _EMU["lib"]


def bgra_rows(rgba, stride=None):
    """uint8 [h, w, 4] RGBA -> BGRA rows [h, stride] (padding 0xA5)."""
    h, w, _ = rgba.shape
    stride = stride or 4 * w
    out = np.full((h, stride), 0xA5, np.uint8)
    out[:, :4 * w].reshape(h, w, 4)[...] = rgba[..., [2, 1, 0, 3]]
    return out


def quantize(rgba, alpha=True, quality=None, minimum_quality=None, speed=None, max_colors=256, dither=True, zlib_level=6, file=True, stride=None):
    """The emulation on one RGBA frame.  Returns a dict: palette [count, 4] RGBA in file order, indices [h, w], n_trans,
    level, entries, mse (before dithering, 1.0 = black against white), status, file (bytes or None)."""
    L = emulator()
    h, w, _ = rgba.shape
    rows = bgra_rows(rgba, stride)
    cap = h * (w + 1) + 5 * (h * (w + 1) // 32768 + 1) + 2048
    out = np.zeros(cap, np.uint8)
    ln, st = C.c_size_t(0), C.c_uint32(0)
    pal, idx, info, err = np.zeros(1028, np.uint8), np.zeros((h, w), np.uint8), np.zeros(4, np.uint32), np.zeros(2, np.uint64)
    opt = lambda v: -1 if v is None else int(v)  # noqa: E731
    rc = L.pq_emu_quantize(rows.ctypes.data, w, h, rows.shape[1], 1 if alpha else 0, opt(quality), opt(minimum_quality), opt(speed), max_colors,
                           1 if dither else 0, zlib_level, out.ctypes.data if file else None, cap, C.byref(ln), C.byref(st), pal.ctypes.data,
                           idx.ctypes.data, info.ctypes.data, err.ctypes.data)
    assert rc == 0, rc
    count = int(pal[1024:].view(np.uint32)[0])
    return {"palette": pal[:1024].reshape(256, 4)[:count].copy(), "indices": idx, "entries": int(info[0]), "level": int(info[1]),
            "n_trans": int(info[2]), "mse": int(err[0]) / (int(err[1]) * DISTANCE_UNIT), "status": int(st.value),
            "file": out[:ln.value].tobytes() if ln.value else None}


def normalized(rgba, alpha=True):
    """The frame as the quantiser sees it: alpha 255 where it is not meaningful, every pixel of alpha 0 as 00 00 00 00."""
    out = rgba.copy()
    if not alpha:
        out[..., 3] = 255
    out[out[..., 3] == 0] = 0
    return out


def chunks(data):
    """[(type, payload)] of a PNG file; every CRC is verified."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, at = [], 8
    while at < len(data):
        n, kind = struct.unpack(">I4s", data[at:at + 8])
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + body), kind
        out.append((kind, body))
        at += 12 + n
    assert at == len(data) and out[-1][0] == b"IEND"
    return out


def check_palette_file(data, w, h, palette, indices):
    """A palette PNG as lode.rs:162-195 frames it, holding `palette` [count, 4] and `indices` [h, w]."""
    from PIL import Image
    import io
    ch = chunks(data)
    kinds = [k for k, _ in ch]
    n_trans = int((palette[:, 3] < 255).sum())
    assert kinds == ([b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND"] if n_trans else [b"IHDR", b"PLTE", b"IDAT", b"IEND"]), kinds
    d = dict(ch)
    assert struct.unpack(">IIBBBBB", d[b"IHDR"]) == (w, h, 8, 3, 0, 0, 0)
    assert d[b"PLTE"] == palette[:, :3].tobytes()
    if n_trans:
        assert (palette[:n_trans, 3] < 255).all() and (palette[n_trans:, 3] == 255).all(), "non-opaque entries come first"
        assert d[b"tRNS"] == palette[:n_trans, 3].tobytes()
    stream = np.frombuffer(zlib.decompress(d[b"IDAT"]), np.uint8)
    assert stream.size == h * (1 + w)
    stream = stream.reshape(h, 1 + w)
    assert (stream[:, 0] == 0).all(), "filter type 0 on every row"
    assert np.array_equal(stream[:, 1:], indices)
    im = Image.open(io.BytesIO(data))
    assert im.format == "PNG" and im.mode == "P" and im.size == (w, h)
    assert np.array_equal(np.asarray(im), indices)
    assert np.array_equal(np.asarray(im.convert("RGBA")), palette[indices])
    return d


def colour_frame(w, h, n_colors, seed=1, alpha=False):
    """A frame of exactly n_colors distinct RGBA values (w * h >= n_colors), each used at least once; with alpha, a third
    of the values are semi-transparent (alpha 1..254)."""
    rng = np.random.default_rng(seed)
    cols = set()
    while len(cols) < n_colors:
        c = tuple(int(v) for v in rng.integers(0, 256, 3))
        a = int(rng.integers(1, 255)) if alpha and len(cols) % 3 == 0 else 255
        cols.add(c + (a,))
    cols = np.array(sorted(cols), np.uint8)
    idx = np.concatenate([np.arange(n_colors), rng.integers(0, n_colors, w * h - n_colors)])
    rng.shuffle(idx)
    return cols[idx].reshape(h, w, 4)


def photo_rgba(w, h, seed=7, alpha=False):
    """png_oracle.photo_frame as RGBA; with alpha, a diagonal alpha ramp with a fully transparent corner."""
    from tests import png_oracle
    rgb = png_oracle.photo_frame(w, h, seed)
    a = np.full((h, w), 255, np.uint8)
    if alpha:
        y, x = np.mgrid[0:h, 0:w]
        a = np.clip((x + y) * 300 // max(1, w + h - 2) - 20, 0, 255).astype(np.uint8)
    return np.dstack([rgb, a])
