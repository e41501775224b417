"""Mirror of graphics/rounded_corners.rs::flow_bitmap_bgra_clear_around_rounded_corners (:187-346) on device-resident
Bitmaps, run by csrc/round_corners.hip (ifhip_round_corners_batch_device): every frame of the batch in place."""
import ctypes as C

import torch

from .. import _native
from .bitmaps import Bitmap

_u32 = C.c_uint32
# RoundCornersMode (imageflow_types/src/lib.rs:1254-1268) -> ifhip_round_corners_mode
MODES = {"percentage": 0, "pixels": 1, "circle": 2, "percentage_custom": 3, "pixels_custom": 4}


def _bind():
    L = _native.lib()
    if getattr(L, "_round_corners_bound", False):
        return L
    L.ifhip_round_corners_batch_device.argtypes = [C.c_void_p, C.c_size_t, _u32, _u32, _u32, _u32, C.c_int,
                                                   C.POINTER(C.c_float), _u32, C.c_void_p]
    L.ifhip_round_corners.argtypes = [C.c_void_p, _u32, _u32, _u32, C.c_int, C.POINTER(C.c_float), _u32]
    L._round_corners_bound = True
    return L


def clear_around_rounded_corners(b: Bitmap, mode, radii, matte):
    """Queue the clear on the current stream.  mode: a MODES key; radii: one value (percentage, pixels) or four in the
    JSON order top_left, top_right, bottom_right, bottom_left; matte: Color32 0xAARRGGBB."""
    r = list(radii) if hasattr(radii, "__len__") else [radii]
    r = (r * 4)[:4] if len(r) == 1 else r
    arr = (C.c_float * 4)(*[float(v) for v in r])
    with torch.cuda.device(b.data.device):
        st = C.c_void_p(torch.cuda.current_stream(b.data.device).cuda_stream)
        _native.check(_bind().ifhip_round_corners_batch_device(b.data.data_ptr(), b.image_bytes, b.n, b.w, b.h, b.stride,
                                                               MODES[mode], arr, matte & 0xFFFFFFFF, st))
