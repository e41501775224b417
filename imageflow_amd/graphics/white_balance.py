"""Mirror of flow/nodes/white_balance.rs (:13-93) with graphics/histogram.rs on device-resident Bitmaps, run by
csrc/white_balance.hip (ifhip_white_balance_batch_device): every frame of the batch in place, each by its own histograms."""
import ctypes as C

import numpy as np
import torch

from .. import _native
from .bitmaps import Bitmap

_u32 = C.c_uint32
DEFAULT_THRESHOLD = np.float32(0.006)       # :77, an f32 literal


def _bind():
    L = _native.lib()
    if getattr(L, "_white_balance_bound", False):
        return L
    L.ifhip_white_balance_batch_device.argtypes = [C.c_void_p, C.c_size_t, _u32, _u32, _u32, _u32, C.c_float, C.c_void_p,
                                                   C.c_void_p]
    L.ifhip_white_balance.argtypes = [C.c_void_p, _u32, _u32, _u32, C.c_float, C.c_void_p]
    L._white_balance_bound = True
    return L


def white_balance_srgb(b: Bitmap, threshold=None, histograms: torch.Tensor = None):
    """Queue the node's work on the current stream.  threshold: Option<f32> (None = 0.006).  histograms (optional):
    a contiguous int64 tensor of n*768 entries on b's device that receives each frame's R, G, B counts ([n][3][256])."""
    if histograms is not None and (histograms.dtype != torch.int64 or not histograms.is_contiguous()
                                   or histograms.numel() < 768 * b.n or histograms.device != b.data.device):
        raise ValueError("histograms must be a contiguous int64 tensor of n*768 entries on the bitmap's device")
    t = DEFAULT_THRESHOLD if threshold is None else np.float32(threshold)
    with torch.cuda.device(b.data.device):
        st = C.c_void_p(torch.cuda.current_stream(b.data.device).cuda_stream)
        _native.check(_bind().ifhip_white_balance_batch_device(b.data.data_ptr(), b.image_bytes, b.n, b.w, b.h, b.stride,
                                                               float(t), histograms.data_ptr() if histograms is not None else None, st))
