"""The lossy WebP decoder's algorithm without a device: the host stage (csrc/vp8_read.cpp: frame header, bool decoder, modes,
coefficient tokens, the ALPH header) and csrc/vp8_decode_core.hpp (dequantisation, inverse WHT and DCT, the intra predictors
with libwebp's borders, both loop filters, the fancy upsampler, YUV -> BGRA, the alpha un-filters) -- what the gfx950 kernels
of csrc/vp8_decode.hip are built from.  tests/vp8_decode_emulate.cpp runs them on the CPU in the kernels' schedules; libwebp
1.6.0 through Pillow is the yardstick, bit for bit: every good file, every flipped and cut file with Pillow's verdict either
way, and every damaged file -- refused by Pillow -- with its status word.  The same cases run a second time through a
stand-alone program built with ASan + UBSan, where an access outside the given bounds ends the program."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tests import webp_lossy_fixtures as X

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "vp8_decode_emulate.cpp")
_EMU = {}
GOOD = sorted(X.good_files())
VERDICT = sorted(X.verdict_files())
BAD = sorted(X.damaged_files())


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="vp8_decode_emulate_")
        so = os.path.join(d, "libvp8_decode_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", so], check=True)
        lib = C.CDLL(so)
        lib.vp8_emu_decode.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        lib.vp8_emu_decode.restype = C.c_uint32
        _EMU["lib"] = lib
    return _EMU["lib"]


def emulate(data, cap=1 << 20):
    """a file -> (status, BGRA [h, w, 4] or None)"""
    vp8, alph, _, _ = X.parts(data)
    a = np.frombuffer(vp8, np.uint8).copy()
    b = np.frombuffer(alph, np.uint8).copy() if alph is not None else None
    out, dims = np.zeros(cap, np.uint32), np.zeros(2, np.uint32)
    st = emulator().vp8_emu_decode(a.ctypes.data, a.size, b.ctypes.data if b is not None and b.size else (a.ctypes.data if b is not None else None),
                                   b.size if b is not None else 0, out.ctypes.data, cap, dims[0:].ctypes.data, dims[1:].ctypes.data)
    if st:
        return st, None
    w, h = int(dims[0]), int(dims[1])
    return 0, out[:w * h].view(np.uint8).reshape(h, w, 4)


def checksum(bgra):
    s = 0
    for v in np.ascontiguousarray(bgra).view(np.uint32).ravel():
        s = ((s * 0x01000193) & 0xFFFFFFFF) ^ int(v)
    return s


def test_the_fixtures_hold_what_they_are_there_for():
    good = X.good_files()
    assert X.parts(good["size_56x40"])[1] is None and X.parts(good["rgba_56x40"])[1] is not None
    for name in ("rgba_aq100", "rgba_aq40", "rgba_exact", "rgba_56x40"):
        assert X.expected_bgra(name)[..., 3].min() < 255, name
    assert X.expected_bgra("size_150x130").shape == (130, 150, 4)
    verdicts = X.verdict_files()
    assert sum(want is not None for n, (_, want) in verdicts.items() if n.startswith("flip")) >= 12
    assert verdicts["cut_01"][1] is not None and verdicts["cut_12"][1] is None          # the last bits of a partition may be missing, its bytes not
    assert any(want is None for n, (_, want) in verdicts.items() if n.startswith("flip"))


@pytest.mark.parametrize("name", GOOD)
def test_emulation_decodes_what_libwebp_decodes(name):
    want = X.expected_bgra(name)
    st, got = emulate(X.good_files()[name])
    assert st == X.OK, name
    assert got.shape == want.shape and np.array_equal(got, want), name


@pytest.mark.parametrize("name", VERDICT)
def test_emulation_follows_libwebp_on_flipped_and_cut_files(name):
    data, want = X.verdict_files()[name]
    st, got = emulate(data)
    if want is None:
        assert st in (X.END_OF_MODES, X.END_OF_TOKENS, X.PARTITIONS), (name, st)
    else:
        assert st == X.OK and got.shape == want.shape and np.array_equal(got, want), name


@pytest.mark.parametrize("name", BAD)
def test_emulation_gives_every_damaged_file_its_status(name):
    data, status, _ = X.damaged_files()[name]
    assert X.pillow_refuses(data), name
    assert emulate(data)[0] == status, name


def test_every_case_again_under_asan_and_ubsan():
    """the stand-alone program: its own main, no sanitizer in this process"""
    d = tempfile.mkdtemp(prefix="vp8_decode_sanitize_")
    exe, cases = os.path.join(d, "vp8_decode_emulate"), os.path.join(d, "cases.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DVP8_DEC_EMU_MAIN", SRC, "-o", exe], check=True)
    want = []
    with open(cases, "wb") as f:
        def put(data, bgra, status):
            vp8, alph, _, _ = X.parts(data)
            f.write(struct.pack("<II", len(vp8), 0xFFFFFFFF if alph is None else len(alph)) + vp8 + (alph or b""))
            want.append("0 %d %d %d" % (bgra.shape[1], bgra.shape[0], checksum(bgra)) if bgra is not None else "%s 0 0 0" % status)
        for name in GOOD:
            put(X.good_files()[name], X.expected_bgra(name), 0)
        for name in VERDICT:
            data, bgra = X.verdict_files()[name]
            put(data, bgra, "*")
        for name in BAD:
            data, status, _ = X.damaged_files()[name]
            put(data, None, status)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    got = r.stdout.split("\n")[:-1]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if w.startswith("*"):
            assert g.split()[0] != "0" and g.split()[1:] == ["0", "0", "0"], (g, w)
        else:
            assert g == w
