"""Mirror of codecs/cms.rs (transform_to_srgb) with codecs/source_profile.rs, pinned to the reference's lcms2 back end
(codecs/lcms2_transform.rs): a source's colour profile as a plan (csrc/color_profile.cpp) and the conversion of device-resident
Bitmaps to sRGB in place (csrc/color_profile.hip, ifhip_color_transform_batch_device).

Converted by a plan: RGB matrix/TRC ICC profiles (v2 / v4, XYZ connection space) and PNG gAMA + cHRM.  Converted by a link
(ColorLink below; csrc/color_link.cpp, csrc/color_link.hip): GRAY profiles with a tone curve on grey frames, and RGB profiles
that carry A2B0 (lut8 / lut16 with an XYZ connection space, lutAToB with XYZ or Lab).  Not converted (a FlowError that names
the case): CMYK, grey LUTs, lut8 / lut16 with a Lab connection space, D2B0; PNG cICP is not read at all."""
import ctypes as C

import numpy as np
import torch

from .. import _native
from ..errors import ErrorKind, FlowError
from ..graphics.bitmaps import Bitmap

_u32 = C.c_uint32
PLANNED, NOT_CONVERTIBLE, MALFORMED = 0, 1, 2     # include/imageflow_hip.h ifhip_color_plan_status


class ColorPlan(C.Structure):
    """ifhip_color_plan: linear light per byte value for R, G and B, and the row-major matrix source linear RGB -> sRGB linear RGB."""
    _fields_ = [("linear", (C.c_float * 256) * 3), ("matrix", C.c_float * 9)]

    def tables(self):
        return np.ctypeslib.as_array(self.linear).copy()

    def matrix3(self):
        return np.ctypeslib.as_array(self.matrix).reshape(3, 3).copy()


def _bind():
    L = _native.lib()
    if getattr(L, "_color_profile_bound", False):
        return L
    L.ifhip_color_plan_from_icc.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(ColorPlan)]
    L.ifhip_color_plan_from_gamma_primaries.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(ColorPlan)]
    L.ifhip_color_plan_status_text.argtypes = [C.c_int]
    L.ifhip_color_plan_status_text.restype = C.c_char_p
    L.ifhip_color_transform_batch_device.argtypes = [C.c_void_p, C.c_size_t, _u32, _u32, _u32, _u32, C.POINTER(ColorPlan), C.c_void_p]
    L.ifhip_color_transform.argtypes = [C.c_void_p, _u32, _u32, _u32, C.POINTER(ColorPlan)]
    vp = C.c_void_p
    L.ifhip_color_link_from_icc.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.ifhip_color_link_free.argtypes = [vp]
    L.ifhip_color_link_free.restype = None
    L.ifhip_color_link_kind.argtypes = [vp]
    L.ifhip_color_link_copy_nodes.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.ifhip_color_link_transform.argtypes = [vp, _u32, _u32, _u32, vp]
    L.ifhip_color_link_transform_batch_device.argtypes = [vp, C.c_size_t, _u32, _u32, _u32, _u32, vp, vp]
    L._color_profile_bound = True
    return L


def _last_error():
    m = _bind().ifhip_last_error_message()
    return m.decode("utf-8", "replace") if m else ""


def status_text(status):
    return _bind().ifhip_color_plan_status_text(status).decode()


def try_plan_from_icc(icc):
    """-> (status, plan or None, the message that names the case)"""
    plan = ColorPlan()
    icc = bytes(icc)
    status = _bind().ifhip_color_plan_from_icc(icc, len(icc), C.byref(plan))
    return status, (plan if status == PLANNED else None), ("" if status == PLANNED else _last_error())


def try_plan_from_gamma_primaries(gamma, xy):
    """SourceProfile::GammaPrimaries: gamma as gAMA states it (0.45455 for 2.2), xy = white, red, green, blue as x, y pairs."""
    plan = ColorPlan()
    v = (C.c_double * 8)(*[float(t) for t in xy])
    status = _bind().ifhip_color_plan_from_gamma_primaries(float(gamma), v, C.byref(plan))
    return status, (plan if status == PLANNED else None), ("" if status == PLANNED else _last_error())


def _or_raise(status, plan, message):
    if status == PLANNED:
        return plan
    raise FlowError(ErrorKind.MethodNotImplemented if status == NOT_CONVERTIBLE else ErrorKind.InvalidArgument, message)


def plan_from_icc(icc):
    return _or_raise(*try_plan_from_icc(icc))


def plan_from_gamma_primaries(gamma, xy):
    return _or_raise(*try_plan_from_gamma_primaries(gamma, xy))


def transform_to_srgb(b: Bitmap, plan: ColorPlan):
    """Queue the conversion of every frame of the batch on the current stream, in place; alpha bytes keep their values."""
    with torch.cuda.device(b.data.device):
        st = C.c_void_p(torch.cuda.current_stream(b.data.device).cuda_stream)
        _native.check(_bind().ifhip_color_transform_batch_device(b.data.data_ptr(), b.image_bytes, b.n, b.w, b.h, b.stride, C.byref(plan), st))


def transform_to_srgb_host(rows, w, plan: ColorPlan):
    """Host-buffer drop-in (numpy): uint8 rows [h, stride], converted in place through the device."""
    assert rows.dtype == np.uint8 and rows.ndim == 2 and rows.flags.c_contiguous
    _native.check(_bind().ifhip_color_transform(rows.ctypes.data, w, rows.shape[0], rows.shape[1], C.byref(plan)))
    return rows


# ---- colour links: GRAY and LUT-based profiles (include/imageflow_hip_color_link.h) ------------------------------------------
LINK_GRAY, LINK_RGB, LINK_GRID = 1, 2, 33


class ColorLink:
    """ifhip_color_link: a grey table (256 bytes) or an RGB device link (33^3 nodes) built from a profile's bytes; its device copy
    is made by the first conversion that needs it.  close() (or the collector) frees it after a wait for the device."""

    def __init__(self, handle):
        self.p = handle

    @property
    def kind(self):
        return _bind().ifhip_color_link_kind(self.p)

    def nodes(self):
        """uint8 [256] for a grey table; uint16 [33, 33, 33, 3] indexed [r][g][b] -> (R, G, B) for an RGB link"""
        gray = self.kind == LINK_GRAY
        out = np.zeros(256, np.uint8) if gray else np.zeros((LINK_GRID,) * 3 + (3,), np.uint16)
        written = C.c_size_t(0)
        _native.check(_bind().ifhip_color_link_copy_nodes(self.p, out.ctypes.data, out.nbytes, C.byref(written)))
        assert written.value == out.nbytes
        return out

    def close(self):
        if self.p:
            _bind().ifhip_color_link_free(self.p)
            self.p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def try_link_from_icc(icc, frame_is_gray=False):
    """-> (status, ColorLink or None, the message that names the case)"""
    icc = bytes(icc)
    handle = C.c_void_p()
    status = _bind().ifhip_color_link_from_icc(icc, len(icc), 1 if frame_is_gray else 0, C.byref(handle))
    return status, (ColorLink(handle) if status == PLANNED else None), ("" if status == PLANNED else _last_error())


def link_from_icc(icc, frame_is_gray=False):
    return _or_raise(*try_link_from_icc(icc, frame_is_gray))


def link_to_srgb(b: Bitmap, link: ColorLink):
    """Queue the conversion of every frame of the batch through the link on the current stream, in place; alpha bytes keep their
    values; a grey table reads the B byte."""
    with torch.cuda.device(b.data.device):
        st = C.c_void_p(torch.cuda.current_stream(b.data.device).cuda_stream)
        _native.check(_bind().ifhip_color_link_transform_batch_device(b.data.data_ptr(), b.image_bytes, b.n, b.w, b.h, b.stride, link.p, st))


def link_to_srgb_host(rows, w, link: ColorLink):
    """Host-buffer drop-in (numpy): uint8 rows [h, stride], converted in place through the device."""
    assert rows.dtype == np.uint8 and rows.ndim == 2 and rows.flags.c_contiguous
    _native.check(_bind().ifhip_color_link_transform(rows.ctypes.data, w, rows.shape[0], rows.shape[1], link.p))
    return rows
