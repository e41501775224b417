"""Mirror of graphics/whitespace.rs::detect_content (:284-334) on device-resident Bitmaps: the reference's sequential
windowed search for the content rectangle, run by csrc/whitespace.hip (ifhip_detect_content_batch_device)."""
import ctypes as C

import torch

from .. import _native
from .bitmaps import Bitmap

_u32 = C.c_uint32


def _bind():
    L = _native.lib()
    if getattr(L, "_whitespace_bound", False):
        return L
    L.ifhip_detect_content_batch_device.argtypes = [C.c_void_p, C.c_size_t, _u32, _u32, _u32, _u32, C.c_int, _u32, C.c_void_p, C.c_void_p]
    L.ifhip_detect_content.argtypes = [C.c_void_p, _u32, _u32, _u32, C.c_int, _u32, C.POINTER(_u32)]
    L._whitespace_bound = True
    return L


def detect_content_into(b: Bitmap, threshold, rects: torch.Tensor):
    """Queue the detection on the current stream; rects: int32 [n, 4] (x1, y1, x2, y2 as u32 bits) on b's device."""
    if rects.dtype != torch.int32 or not rects.is_contiguous() or rects.numel() < 4 * b.n or rects.device != b.data.device:
        raise ValueError("rects must be a contiguous int32 tensor of n*4 entries on the bitmap's device")
    with torch.cuda.device(b.data.device):
        st = C.c_void_p(torch.cuda.current_stream(b.data.device).cuda_stream)
        _native.check(_bind().ifhip_detect_content_batch_device(b.data.data_ptr(), b.image_bytes, b.n, b.w, b.h, b.stride,
                                                                int(b.alpha_meaningful), threshold & 0xFFFFFFFF, rects.data_ptr(), st))


def detect_content(b: Bitmap, threshold):
    """detect_content for every frame of the batch -> list of (x1, y1, x2, y2).  Frames below 3 px on a side, and frames
    without any edge above the threshold, give the whole frame (:288-290, :326-333)."""
    rects = torch.empty((b.n, 4), dtype=torch.int32, device=b.data.device)
    detect_content_into(b, threshold, rects)
    return [tuple(int(v) & 0xFFFFFFFF for v in r) for r in rects.cpu().tolist()]
