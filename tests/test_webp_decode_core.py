"""The device WebP decoder's algorithm without a device (csrc/webp_decode_core.hpp: the bit reader, the prefix codes with
libwebp's refusals, the token loop with the distance map, the colour cache and meta groups, the inverse transforms -- what
the host prepare and the gfx950 kernels of csrc/webp_decode.hip are built from).  tests/webp_decode_emulate.cpp runs them on
the CPU with the kernels' schedules; libwebp through Pillow is the yardstick for every good file (tests/vp8l_reader.py
supplies the alpha bytes of files Pillow opens as RGB), and every damaged file -- refused by Pillow -- must give its status.
The same cases run a second time through a stand-alone program built with ASan + UBSan, where an access outside the given
bounds ends the program."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tests import webp_decode_fixtures as X

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "webp_decode_emulate.cpp")
_EMU = {}
GOOD = sorted(X.good_files())
BAD = sorted(n for n, (_, status) in X.damaged_files().items() if status != X.CONTAINER)


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="webp_decode_emulate_")
        so = os.path.join(d, "libwebp_decode_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", so], check=True)
        lib = C.CDLL(so)
        lib.webp_dec_emu_decode.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.webp_dec_emu_decode.restype = C.c_uint32
        _EMU["lib"] = lib
    return _EMU["lib"]


def emulate(payload, cap=1 << 20):
    """-> (status, BGRA [h, w, 4] or None, has_alpha)"""
    src = np.frombuffer(bytes(payload) + b"\0", np.uint8).copy()
    out, dims = np.zeros(cap, np.uint32), np.zeros(3, np.uint32)
    st = emulator().webp_dec_emu_decode(src.ctypes.data, len(payload), out.ctypes.data, cap, dims[0:].ctypes.data, dims[1:].ctypes.data, dims[2:].ctypes.data)
    if st:
        return st, None, None
    w, h = int(dims[0]), int(dims[1])
    return 0, out[:w * h].view(np.uint8).reshape(h, w, 4), int(dims[2])


def checksum(bgra):
    s = 0
    for v in np.ascontiguousarray(bgra).view(np.uint32).ravel():
        s = ((s * 0x01000193) & 0xFFFFFFFF) ^ int(v)
    return s


def test_the_fixtures_hold_the_features_they_are_there_for():
    info = {n: X.expected_bgra(n)[1] for n in GOOD if not n.startswith(("own_", "gen_"))}
    i = info["photo_q70_m4"]
    assert i["transforms"] == ["predictor", "cross_color"] and i["tile_bits"] == [3, 3]
    i = info["photo_q100_m6"]
    assert i["tile_bits"] == [2, 2] and i["groups"] == 3 and i["color_cache_bits"] == 0      # (this frame: three meta groups, no cache -- photo_cache has one)
    i = info["photo_q0_m0"]
    assert i["transforms"] == ["subtract_green", "predictor"] and i["tile_bits"][1] == 6
    assert info["rgba_exact"]["alpha_is_used"] == 1 and len(np.unique(X.expected_bgra("rgba_exact")[0][..., 3])) > 100
    for colours, bits in ((2, 3), (4, 2), (16, 1), (200, 0)):
        i = info["indexed_%d" % colours]
        assert i["transforms"] == ["color_indexing"] and i["tile_bits"] == [bits] and i["matches"], colours
    # (the graphic is bundled 8 pixels a dword, 12 dwords a row: 191 dwords are 16 rows, 648 are the pattern's 54 rows)
    assert max(length for _, length, _ in info["graphic"]["matches"]) == 191 and max(d for _, _, d in info["graphic"]["matches"]) == 648
    assert info["photo_cache"]["color_cache_bits"] == 1 and info["photo_cache"]["groups"] == 2 and info["photo_cache"]["tile_bits"] == [2, 2]
    assert all(k.startswith("simple") for k in info["1x1"]["code_kinds"])
    assert X.expected_bgra("photo_q70_m4")[0].shape == (130, 150, 4)              # the predictor crosses two band boundaries


@pytest.mark.parametrize("name", GOOD)
def test_emulation_decodes_what_libwebp_decodes(name):
    want, info = X.expected_bgra(name)
    st, got, alpha = emulate(X.payload_of(X.good_files()[name]))
    assert st == X.OK
    assert got.shape == want.shape and np.array_equal(got, want), (name, info["transforms"])
    assert alpha == info["alpha_is_used"]


@pytest.mark.parametrize("name", BAD)
def test_emulation_gives_every_damaged_file_its_status(name):
    data, status = X.damaged_files()[name]
    assert X.pillow_refuses(data), name
    assert emulate(X.payload_of(data))[0] == status, name


def test_every_case_again_under_asan_and_ubsan():
    """the stand-alone program: its own main, no sanitizer in this process"""
    d = tempfile.mkdtemp(prefix="webp_decode_sanitize_")
    exe, cases = os.path.join(d, "webp_decode_emulate"), os.path.join(d, "cases.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DWEBP_DEC_EMU_MAIN", SRC, "-o", exe], check=True)
    want = []
    with open(cases, "wb") as f:
        for name in GOOD:
            p = X.payload_of(X.good_files()[name])
            f.write(struct.pack("<I", len(p)) + p)
            bgra = X.expected_bgra(name)[0]
            want.append("0 %d %d %d" % (bgra.shape[1], bgra.shape[0], checksum(bgra)))
        for name in BAD:
            data, status = X.damaged_files()[name]
            p = X.payload_of(data)
            f.write(struct.pack("<I", len(p)) + p)
            want.append("%d 0 0 0" % status)
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split("\n")[:-1] == want
