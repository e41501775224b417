"""tests/color_link_emulate.cpp built with g++ and bound with ctypes: the CPU emulation of the colour link kernel and the links it
runs on (csrc/color_link.cpp), next to tests/color_profile_emulation.py."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "imageflow_amd", "csrc")
_EMU = {}
PLANNED, NOT_CONVERTIBLE, MALFORMED = 0, 1, 2
GRAY, RGB = 1, 2
GRID = 33


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="color_link_emulate_")
        so = os.path.join(d, "libcolor_link_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-ffp-contract=off", os.path.join(HERE, "color_link_emulate.cpp"), "-o", so], check=True)
        lib = C.CDLL(so)
        lib.cl_emu_link_from_icc.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        lib.cl_emu_transform.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p]
        _EMU["lib"] = lib
    return _EMU["lib"]


class Link:
    """kind GRAY: table = uint8 [256]; kind RGB: nodes = uint16 [33, 33, 33, 3], indexed [r][g][b]."""

    def __init__(self, kind, table, nodes):
        self.kind, self.table, self.nodes = kind, table, nodes


def link_from_icc(icc, frame_is_gray=False):
    """-> (status, Link or None, the reason text)"""
    icc = bytes(icc)
    kind, why = C.c_int(0), C.create_string_buffer(200)
    table, nodes = np.zeros(256, np.uint8), np.zeros((GRID, GRID, GRID, 3), np.uint16)
    status = emulator().cl_emu_link_from_icc(icc, len(icc), int(frame_is_gray), C.byref(kind), table.ctypes.data, nodes.ctypes.data, why, 200)
    return status, (Link(kind.value, table, nodes) if status == PLANNED else None), why.value.decode()


def transform(rows, w, link):
    """A copy of uint8 rows [h][stride] with the first w BGRA pixels of each row sent through the link."""
    out = np.array(rows, np.uint8, order="C")
    assert out.ndim == 2 and out.shape[1] >= 4 * w
    emulator().cl_emu_transform(out.ctypes.data, w, out.shape[0], out.strides[0], link.kind, link.table.ctypes.data, link.nodes.ctypes.data)
    return out


def transform_rgb(rgb, link):
    """uint8 [n, 3] R, G, B -> uint8 [n, 3] through the link (a grey link reads column 2's twin: pass grey in all three)."""
    rgb = np.asarray(rgb, np.uint8)
    rows = np.zeros((1, 4 * len(rgb)), np.uint8)
    rows[0, 0::4], rows[0, 1::4], rows[0, 2::4], rows[0, 3::4] = rgb[:, 2], rgb[:, 1], rgb[:, 0], 255
    out = transform(rows, len(rgb), link)
    return np.stack([out[0, 2::4], out[0, 1::4], out[0, 0::4]], axis=1)
