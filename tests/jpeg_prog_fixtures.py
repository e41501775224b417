"""What the tests of the device progressive JPEG decoder share: the files (the corpus of tests/jpeg_prog_gen.py, Pillow's
progressive files, this library's own progressive writer's), the host reader as the yardstick, and the CPU emulation
(tests/jpeg_progressive_emulate.cpp, built once per process with g++)."""
import ctypes as C
import functools
import io
import os
import subprocess
import tempfile

import numpy as np

from imageflow_amd import _native
from tests import jpeg_prog_gen as G

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "jpeg_progressive_emulate.cpp")
METHOD_NOT_IMPLEMENTED = 2          # IFHIP_METHOD_NOT_IMPLEMENTED


def _lib():
    L = _native.lib()
    L.ifhip_jpeg_frame_info.argtypes = [C.c_char_p, C.c_size_t] + [C.c_void_p] * 9
    L.ifhip_jpeg_read_coefficients_host.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def host_read(data):
    """ifhip_jpeg_read_coefficients_host into planes of exactly the frame's size -> (rc, planes or None, qt)"""
    L = _lib()
    data = bytes(data)
    n = C.c_int()
    bw, bh = np.zeros(3, np.uint32), np.zeros(3, np.uint32)
    rc = L.ifhip_jpeg_frame_info(data, len(data), None, None, C.addressof(n), None, None, bw.ctypes.data, bh.ctypes.data, None, None)
    if rc:
        return rc, None, None
    planes = [np.full((int(bh[c]), int(bw[c]), 64), 0x1111, np.int16) for c in range(n.value)]
    ptr = [planes[c].ctypes.data if c < n.value else None for c in range(3)]
    qt = np.zeros((3, 64), np.uint16)
    rc = L.ifhip_jpeg_read_coefficients_host(data, len(data), ptr[0], ptr[1], ptr[2], qt.ctypes.data)
    return rc, (planes if rc == 0 else None), qt


@functools.lru_cache(maxsize=None)
def emulator():
    d = tempfile.mkdtemp(prefix="jpeg_progressive_emulate_")
    so = os.path.join(d, "libjpeg_progressive_emulate.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", so], check=True)
    lib = C.CDLL(so)
    lib.prog_emu_prepare.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.prog_emu_decode_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
    return lib


def emu_prepare(data):
    """-> (rc, dict of the prepared file's facts or None)"""
    info, qt = np.zeros(14, np.uint32), np.zeros((3, 64), np.uint16)
    data = bytes(data)
    rc = emulator().prog_emu_prepare(data, len(data), info.ctypes.data, qt.ctypes.data)
    if rc:
        return rc, None
    v = [int(x) for x in info]
    return 0, dict(width=v[0], height=v[1], ncomp=v[2], bw=v[3:6], bh=v[6:9], scans=v[9], streams=v[10], levels=v[11],
                   max_stream_bits=v[12], stage_words=v[13], qt=qt)


def emulate_batch(files):
    """the files through ONE emulated batch -> [(rc of prepare, status word, planes)]; planes sized exactly, pre-filled"""
    files = [bytes(f) for f in files]
    n = len(files)
    facts = [emu_prepare(f) for f in files]
    planes = [[np.full((p["bh"][c], p["bw"][c], 64), 0x5A5A, np.int16) for c in range(p["ncomp"])] if rc == 0 else [] for rc, p in facts]
    ptrs = (C.c_void_p * (3 * n))(*[(planes[i][c].ctypes.data if c < len(planes[i]) else None) for i in range(n) for c in range(3)])
    sizes = (C.c_size_t * (3 * n))(*[(planes[i][c].nbytes if c < len(planes[i]) else 0) for i in range(n) for c in range(3)])
    fp, fl = (C.c_char_p * n)(*files), (C.c_size_t * n)(*[len(f) for f in files])
    rcs, words = (C.c_int * n)(), (C.c_uint32 * n)()
    assert emulator().prog_emu_decode_batch(fp, fl, n, ptrs, sizes, rcs, words) == 0
    assert [rcs[i] for i in range(n)] == [rc for rc, _ in facts]
    return [(rcs[i], words[i], planes[i]) for i in range(n)]


def image(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    return np.clip(np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], -1) +
                   (35 * np.sin(x / 2.5) * np.cos(y / 4.0))[..., None] + rng.integers(-25, 26, (h, w, 3)), 0, 255).astype(np.uint8)


def save(img, **kw):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", **kw)
    return b.getvalue()


PILLOW_SIZES = [(1, 1), (8, 8), (17, 9), (100, 75), (321, 203)]          # tests/test_jpeg_progressive.py's
PILLOW_SAMPLINGS = ["4:4:4", "4:2:2", "4:2:0"]


@functools.lru_cache(maxsize=None)
def pillow_files():
    """name -> progressive file: every size x sampling with and without restart markers, qualities 30 and 90 in turn, one gray"""
    out, k = {}, 0
    for (w, h) in PILLOW_SIZES:
        for sub in PILLOW_SAMPLINGS:
            for rst in (0, (1 if w < 300 else 7) + k % 3):        # (Pillow's output buffer does not hold the largest file with a marker per block)
                q = (30, 90)[k % 2]
                k += 1
                kw = dict(restart_marker_blocks=rst) if rst else {}
                out["pillow_%dx%d_%s_q%d_rst%d" % (w, h, sub.replace(":", ""), q, rst)] = save(image(w, h, 3 * w + q), quality=q, subsampling=sub, progressive=True, **kw)
    out["pillow_gray_150x90"] = save(image(150, 90, 5)[..., 0], quality=75, progressive=True)
    for name, data in out.items():
        assert b"\xff\xc2" in data, name
    return out


@functools.lru_cache(maxsize=None)
def writer_files():
    """name -> file of this library's progressive writer (ifhip_jpeg_write, flags 2 and 3) from the planes of a baseline file"""
    from oracle import oracle as O
    L = _native.lib()
    L.ifhip_jpeg_write.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                                       C.c_size_t, C.POINTER(C.c_size_t)]
    out = {}
    for (w, h), sub in (((97, 61), "4:2:0"), ((64, 48), "4:4:4"), ((200, 33), "4:2:2")):
        j = O.jpeg_read_coefficients(save(image(w, h, w), quality=85, subsampling=sub, optimize=False))
        bw, bh = np.array(j["bw"][:3], np.uint32), np.array(j["bh"][:3], np.uint32)
        hs, vs = np.array(j["hs"][:3], np.uint8), np.array(j["vs"][:3], np.uint8)
        coef = [np.ascontiguousarray(j["coef"][c]) for c in range(3)]
        for flags in (2, 3):
            buf, n = np.zeros(1 << 20, np.uint8), C.c_size_t()
            _native.check(L.ifhip_jpeg_write(coef[0].ctypes.data, coef[1].ctypes.data, coef[2].ctypes.data, bw.ctypes.data, bh.ctypes.data, 3,
                                             hs.ctypes.data, vs.ctypes.data, w, h, 85, flags, buf.ctypes.data, buf.size, C.byref(n)))
            out["writer_%dx%d_%s_flags%d" % (w, h, sub.replace(":", ""), flags)] = buf[:n.value].tobytes()
    return out


@functools.lru_cache(maxsize=None)
def accepted_files():
    """every file the device path must decode: name -> bytes"""
    out = {name: G.entry(name)[0] for name in G.names()}
    out.update(pillow_files())
    out.update(writer_files())
    return out


DAMAGE_PER_FILE = 4


@functools.lru_cache(maxsize=None)
def damaged_files():
    """corpus files (the 1024 x 1024 one left out: its scans are a few symbols) with seeded flips and cuts inside their scans"""
    return {"%s_damage%d" % (name, k): G.damaged(name, k) for name in G.names(big=False) for k in range(DAMAGE_PER_FILE)}


@functools.lru_cache(maxsize=None)
def host_planes(name):
    """the host reader's answer for an accepted or damaged file, computed once: (rc, planes, qt)"""
    files = accepted_files()
    return host_read(files[name] if name in files else damaged_files()[name])
