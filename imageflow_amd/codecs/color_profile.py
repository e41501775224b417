"""Mirror of codecs/cms.rs (transform_to_srgb) with codecs/source_profile.rs, pinned to the reference's lcms2 back end
(codecs/lcms2_transform.rs): a source's colour profile as a plan (csrc/color_profile.cpp) and the conversion of device-resident
Bitmaps to sRGB in place (csrc/color_profile.hip, ifhip_color_transform_batch_device).

Converted: RGB matrix/TRC ICC profiles (v2 / v4, XYZ connection space) and PNG gAMA + cHRM.  Not converted (a FlowError that
names the case): GRAY and CMYK spaces, a Lab connection space, LUT-based profiles; PNG cICP is not read at all."""
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
