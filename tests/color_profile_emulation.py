"""tests/color_profile_emulate.cpp built with g++ and bound with ctypes: the CPU emulation of the colour conversion kernel, the
plans it runs on, and a small ICC writer for the profiles tests/test_jpeg_headers.py::make_icc does not reach."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "imageflow_amd", "csrc")
_EMU = {}
PLANNED, NOT_CONVERTIBLE, MALFORMED = 0, 1, 2
PLAN_FLOATS = 3 * 256 + 9                      # ifhip_color_plan: float linear[3][256], float matrix[9]

ADOBE_XYZ = ((0.6097, 0.3111, 0.0195), (0.2053, 0.6257, 0.0609), (0.1492, 0.0632, 0.7448))
SRGB_CHRM = (0.3127, 0.3290, 0.64, 0.33, 0.30, 0.60, 0.15, 0.06)        # white, red, green, blue as x, y


def emulator():
    if "lib" not in _EMU:
        d = tempfile.mkdtemp(prefix="color_profile_emulate_")
        so = os.path.join(d, "libcolor_profile_emulate.so")
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-ffp-contract=off", os.path.join(HERE, "color_profile_emulate.cpp"), "-o", so], check=True)
        lib = C.CDLL(so)
        lib.cp_emu_plan_from_icc.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_size_t]
        lib.cp_emu_plan_from_gamma_primaries.argtypes = [C.c_double, C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
        lib.cp_emu_status_text.argtypes = [C.c_int]
        lib.cp_emu_status_text.restype = C.c_char_p
        lib.cp_emu_l2s.argtypes = [C.c_void_p]
        lib.cp_emu_transform.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p]
        _EMU["lib"] = lib
    return _EMU["lib"]


def plan_from_icc(icc):
    """-> (status, plan as float32 [777]: the three tables R, G, B, then the row-major matrix; the reason text)"""
    plan, why = np.zeros(PLAN_FLOATS, np.float32), C.create_string_buffer(160)
    status = emulator().cp_emu_plan_from_icc(bytes(icc), len(icc), plan.ctypes.data, why, 160)
    return status, plan, why.value.decode()


def plan_from_gamma_primaries(gamma, xy):
    plan, why = np.zeros(PLAN_FLOATS, np.float32), C.create_string_buffer(160)
    v = np.asarray(xy, np.float64)
    assert v.shape == (8,)
    status = emulator().cp_emu_plan_from_gamma_primaries(float(gamma), v.ctypes.data, plan.ctypes.data, why, 160)
    return status, plan, why.value.decode()


def tables(plan):
    return plan[:768].reshape(3, 256)


def matrix(plan):
    return plan[768:].reshape(3, 3)


def l2s():
    t = np.zeros(16384, np.uint8)
    emulator().cp_emu_l2s(t.ctypes.data)
    return t


def transform(rows, w, plan):
    """A copy of uint8 rows [h][stride] with the first w BGRA pixels of each row converted."""
    out = np.array(rows, np.uint8, order="C")
    assert out.ndim == 2 and out.shape[1] >= 4 * w
    plan = np.ascontiguousarray(plan, np.float32)
    emulator().cp_emu_transform(out.ctypes.data, w, out.shape[0], out.strides[0], plan.ctypes.data)
    return out


# ---- a small ICC writer ------------------------------------------------------------------------------------------------
def s15(v):
    return struct.pack(">i", int(round(v * 65536)))


def curve(spec):
    """("para", function type, [g, a, b, ...]) | ("curv", [u16, ...]) | ("gamma", u8.8 as a float) | ("raw", bytes)"""
    kind = spec[0]
    if kind == "para":
        return b"para" + b"\0" * 4 + struct.pack(">HH", spec[1], 0) + b"".join(s15(v) for v in spec[2])
    if kind == "curv":
        return b"curv" + b"\0" * 4 + struct.pack(">I", len(spec[1])) + b"".join(struct.pack(">H", v) for v in spec[1])
    if kind == "gamma":
        return b"curv" + b"\0" * 4 + struct.pack(">I", 1) + struct.pack(">H", int(round(spec[1] * 256))) + b"\0\0"
    if kind == "raw":
        return spec[1]
    raise ValueError(kind)


def icc_profile(xyz, trcs, space=b"RGB ", pcs=b"XYZ ", extra=(), version=4, drop=()):
    """A matrix/TRC profile with one tone curve element per channel: xyz = the colourants of R, G and B (each X, Y, Z), trcs =
    three curve() specs, extra = further (signature, element bytes) tags, drop = signatures to leave out."""
    tags = [(sig, b"XYZ " + b"\0" * 4 + b"".join(s15(v) for v in c)) for sig, c in zip((b"rXYZ", b"gXYZ", b"bXYZ"), xyz)]
    tags += [(sig, curve(t)) for sig, t in zip((b"rTRC", b"gTRC", b"bTRC"), trcs)]
    tags = [t for t in tags if t[0] not in drop] + list(extra)
    table_end = 128 + 4 + 12 * len(tags)
    table, body = struct.pack(">I", len(tags)), b""
    for sig, e in tags:
        table += sig + struct.pack(">II", table_end + len(body), len(e))
        body += e + b"\0" * (-len(e) % 4)
    size = table_end + len(body)
    header = struct.pack(">I", size) + b"test" + bytes([version, 0x30 if version == 4 else 0x10, 0, 0]) + b"mntr" + space + pcs + b"\0" * 12 + b"acsp" + b"\0" * (128 - 40)
    return header + table + body


def a2b0_only_profile():
    """An RGB profile whose only way to the connection space is a LUT: an (empty-bodied) mAB element under A2B0."""
    return icc_profile((), (), extra=[(b"A2B0", b"mAB " + b"\0" * 28)])


# ---- the f64 statement the plans are checked against -----------------------------------------------------------------
def curve_f64(spec, x):
    x = np.asarray(x, np.float64)
    kind = spec[0]
    if kind == "curv":
        t = np.asarray(spec[1], np.float64) / 65535.0
        if len(t) == 0:
            y = x
        else:
            y = np.interp(x, np.arange(len(t)) / (len(t) - 1), t)
    elif kind == "gamma":
        y = x ** (int(round(spec[1] * 256)) / 256)
    elif kind == "para":
        p = [int(round(v * 65536)) / 65536 for v in spec[2]] + [0.0] * 7
        g, a, b, c, d, e, f = p[:7]
        with np.errstate(invalid="ignore", divide="ignore"):
            base = a * x + b
            powp = np.where(base > 0, np.abs(base) ** g, 0.0)
            if spec[1] == 0:
                y = x ** g
            elif spec[1] == 1:
                y = np.where(x >= -b / a, powp, 0.0) if a != 0 else np.zeros_like(x)
            elif spec[1] == 2:
                y = np.where(x >= -b / a, powp + c, c) if a != 0 else np.zeros_like(x)
            elif spec[1] == 3:
                y = np.where(x >= d, powp, c * x)
            else:
                y = np.where(x >= d, powp + e, c * x + f)
    else:
        raise ValueError(kind)
    return np.clip(np.nan_to_num(y, nan=0.0), 0.0, 1.0)


def matrix_f64(xyz):
    """inv(lcms2's sRGB colourants, s15.16) x the source's colourants as the profile stores them (s15.16)"""
    src = np.round(np.array(xyz, np.float64).T * 65536) / 65536
    return np.linalg.inv(lcms_srgb_f64()) @ src


def lcms_srgb_f64():
    """The colourants of lcms2's built-in sRGB profile (D65 = 0.3127, 0.3290 and the BT.709 primaries through
    cmsCreateRGBProfile), rows X, Y, Z and columns R, G, B, rounded to s15.16 as its tags hold them."""
    return np.round(bradford_adapted_f64(SRGB_CHRM) * 65536) / 65536


def bradford_adapted_f64(xy):
    """The RGB -> XYZ matrix of the primaries xy[2:8] scaled to the white xy[0:2], adapted to D50 with Bradford."""
    wx, wy = xy[0], xy[1]
    prim = np.array([[xy[2], xy[4], xy[6]], [xy[3], xy[5], xy[7]], [1 - xy[2] - xy[3], 1 - xy[4] - xy[5], 1 - xy[6] - xy[7]]], np.float64)
    white = np.array([wx / wy, 1.0, (1 - wx - wy) / wy])
    m = prim * np.linalg.solve(prim, white)[None, :]
    cone = np.array([[0.8951, 0.2664, -0.1614], [-0.7502, 1.7135, 0.0367], [0.0389, -0.0685, 1.0296]])
    d50 = np.array([0.9642, 1.0, 0.8249])
    return np.linalg.inv(cone) @ np.diag((cone @ d50) / (cone @ white)) @ cone @ m


def ulps(a, b):
    """The distance of two float32 arrays in units of the last place of the larger magnitude."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    scale = np.maximum(np.spacing(np.maximum(np.abs(a), np.abs(b))), np.float32(1e-45))
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / scale
