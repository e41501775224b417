"""The device GIF decoder's algorithm without a device (csrc/gif_read.cpp: the container walk; csrc/gif_decode_core.hpp: the
closed-form code positions, the scan for clear codes, a segment's lengths by pointer jumping, its indices along the prefix
chains, the segments' places, the frame replay -- what the gfx950 kernels of csrc/gif_decode.hip are built from).
tests/gif_decode_emulate.cpp runs them on the CPU in the kernels' order over a block of exactly the device's sizes; the
oracle (tests/gif_oracle.py, pinned to Pillow by tests/test_gif_oracle.py) is the yardstick for every screen, Pillow itself
for the indices of every file it reads (tests/test_gif_gen.py), and every damaged file must give its status word.  The same
cases run a second time through a stand-alone program built with ASan + UBSan."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from tests import gif_fixtures as X
from tests import gif_oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "gif_decode_emulate.cpp")
_EMU = {}
GOOD = sorted(X.good_files())
BAD = sorted(X.damaged_files())


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="gif_decode_emulate_")
        so = os.path.join(d, "libgif_decode_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", SRC, "-o", so], check=True)
        lib = C.CDLL(so)
        lib.gif_dec_emu_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
        lib.gif_dec_emu_decode.restype = C.c_uint32
        _EMU["lib"] = lib
    return _EMU["lib"]


def emulate(data, target=0, grid_x=3, cap=1 << 20):
    """-> (status, BGRA [h, w, 4] or None, frames the walk saw)"""
    src = np.frombuffer(bytes(data) + b"\0", np.uint8).copy()
    out, dims = np.full(cap, 0x5A, np.uint8), np.zeros(3, np.uint32)
    st = emulator().gif_dec_emu_decode(src.ctypes.data, len(data), target, out.ctypes.data, cap, dims[0:].ctypes.data, dims[1:].ctypes.data, dims[2:].ctypes.data, grid_x)
    if st:
        assert (out == 0x5A).all(), "a damaged file's frame must stay untouched"
        return st, None, int(dims[2])
    w, h = int(dims[0]), int(dims[1])
    return 0, out[:4 * w * h].reshape(h, w, 4), int(dims[2])


def checksum(bgra):
    s = 0
    for v in np.ascontiguousarray(bgra).view(np.uint32).ravel():
        s = ((s * 0x01000193) & 0xFFFFFFFF) ^ int(v)
    return s


@pytest.mark.parametrize("name", GOOD)
def test_emulation_gives_the_oracles_screen(name):
    data, target = X.good_files()[name]
    st, got, _ = emulate(data, target)
    assert st == O.OK, name
    want = X.expected(name)
    assert got.shape == want.shape and np.array_equal(got, want), name


def test_the_grid_width_changes_nothing():
    for name in ("clear_at_64", "mixed_segments", "deferred_m8_long_tail"):
        data, target = X.good_files()[name]
        for grid_x in (1, 2, 1024):
            assert np.array_equal(emulate(data, target, grid_x)[1], X.expected(name)), (name, grid_x)


@pytest.mark.parametrize("name", BAD)
def test_emulation_gives_every_damaged_file_its_status(name):
    data, target, status = X.damaged_files()[name]
    assert O.decode(data, target)[0] == status, name
    st, _, seen = emulate(data, target)
    assert st == status, name
    if status == O.NO_SUCH_FRAME:
        assert seen == O.parse(data, target)["frames_seen"]


def test_the_references_crash_repro_files_decode_or_report_a_status_word():
    """the six 34-40 byte files of the reference's tests/crash_repro/: emulation and oracle agree on which, and on the screen"""
    files = X.golden_files()
    assert len(files) == 6 and all(34 <= len(d) <= 40 for d in files.values())
    decoded = 0
    for name, data in files.items():
        so, want, _ = O.decode(data)
        se, got, _ = emulate(data)
        assert se == so, (name, se, so)
        if not so:
            decoded += 1
            assert np.array_equal(got, want), name
    assert decoded >= 1


def test_the_core_header_closed_forms():
    """bit_offset(k) = the sum of the widths of codes 0 .. k - 1, for every minimum code size, through a tiny program"""
    d = tempfile.mkdtemp(prefix="gif_closed_form_")
    src, exe = os.path.join(d, "t.cpp"), os.path.join(d, "t")
    with open(src, "w") as f:
        f.write('#include "%s"\n#include <cstdio>\nnamespace ifhip { int fail(int s, const char*, ...) { return s; } }\n'
                'int main() { for (unsigned m = 1; m <= 8; ++m) { unsigned long long sum = 0; for (unsigned k = 0; k < 9000; ++k) {'
                ' if (ifhip::gif_bit_offset(m, k) != sum) { std::printf("bad %%u %%u\\n", m, k); return 1; } sum += ifhip::gif_width_at(m, k); } }'
                ' for (unsigned h = 1; h < 40; ++h) { unsigned seen[40] = {}; for (unsigned y = 0; y < h; ++y) { unsigned r = ifhip::gif_interlace_source_row(y, h); if (r >= h || seen[r]++) return 2; } }'
                ' std::printf("ok\\n"); return 0; }\n' % os.path.join(HERE, "..", "imageflow_amd", "csrc", "gif_decode_core.hpp"))
    subprocess.run(["g++", "-O1", "-std=c++17", src, "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True).stdout == "ok\n"
    from tests import gif_gen as G
    for m in range(1, 9):
        for k in (0, 1, 2, 3, 254, 255, 256, 3837, 3838, 3839, 5000):
            assert G.width_at(m, k) == O_width(m, k)


def O_width(m, k):
    clear, w = 1 << m, m + 1
    while w < 12 and k >= (1 << w) - clear - 1:
        w += 1
    return w


def test_every_case_again_under_asan_and_ubsan():
    """the stand-alone program: its own main, no sanitizer in this process"""
    d = tempfile.mkdtemp(prefix="gif_decode_sanitize_")
    exe, cases = os.path.join(d, "gif_decode_emulate"), os.path.join(d, "cases.bin")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DGIF_DEC_EMU_MAIN", SRC, "-o", exe], check=True)
    want = []
    with open(cases, "wb") as f:
        for name in GOOD:
            data, target = X.good_files()[name]
            f.write(struct.pack("<II", len(data), target) + data)
            bgra = X.expected(name)
            want.append("0 %d %d %d" % (bgra.shape[1], bgra.shape[0], checksum(bgra)))
        for name in BAD:
            data, target, status = X.damaged_files()[name]
            f.write(struct.pack("<II", len(data), target) + data)
            want.append("%d 0 0 0" % status)
        for name, data in X.golden_files().items():
            f.write(struct.pack("<II", len(data), 0) + data)
            so, bgra, _ = O.decode(data)
            want.append("%d 0 0 0" % so if so else "0 %d %d %d" % (bgra.shape[1], bgra.shape[0], checksum(bgra)))
    r = subprocess.run([exe, cases], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.split("\n")[:-1] == want
