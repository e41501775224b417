"""Host mirror of WebPDecoder (imageflow_core/src/codecs/webp.rs:20-248) on the device WebP decoder of libimageflow_hip.so
(csrc/webp_read.cpp, csrc/webp_decode.hip): lossless WebP files -> 8-bit BGRA frames in HBM -- the VP8L token loop and the
inverse transforms on the GPU.  For tests and tools; the job path is `decode` with a WebP io_id (csrc/shim_decode.cpp)."""
import ctypes as C

import numpy as np

from .. import _native
from ..errors import ErrorKind, FlowError
from ._file_decoder import decode_batch, decode_host

# include/imageflow_hip.h IFHIP_WEBP_DEC_*
STATUS = {0: "ok", 1: "truncated", 2: "code_lengths", 3: "bad_code", 4: "distance", 5: "copy_end", 6: "cache_symbol", 7: "transform",
          8: "too_little", 9: "container"}
COLOR_NONE, COLOR_SRGB, COLOR_OTHER = 0, 1, 2


class WebpFileInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "has_alpha", "lossless", "animated")] + [("color_kind", C.c_int32)]


def _bind():
    L = _native.lib()
    if getattr(L, "_webp_dec_bound", False):
        return L
    L.ifhip_webp_info.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(WebpFileInfo)]
    L.ifhip_webp_decode_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ifhip_webp_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_size_t, C.POINTER(C.c_uint32)]
    L._webp_dec_bound = True
    return L


def webp_info(data):
    """WebPGetFeatures: the container's facts (webp.rs:130-160).  Host only."""
    L = _bind()
    buf = np.frombuffer(bytes(data), np.uint8)
    info = WebpFileInfo()
    _native.check(L.ifhip_webp_info(buf.ctypes.data, buf.size, C.byref(info)))
    out = {n: int(getattr(info, n)) for n, _ in WebpFileInfo._fields_}
    for k in ("has_alpha", "lossless", "animated"):
        out[k] = bool(out[k])
    out.update(preferred_mime_type="image/webp", preferred_extension="webp", image_width=out["width"], image_height=out["height"],
               frame_decodes_into="bgra_32" if out["has_alpha"] else "bgr_32")
    return out


def decode_webp_batch(files, device="cuda:0", frames=None, fill=None):
    """files: n lossless WebP files (bytes) of any size and transforms, decoded in one batch (the token loop and at most four
    transform steps).  Returns (frames, status): frames[i] a Bitmap of one frame (None where the container did not parse or
    holds no lossless image), status[i] the file's status word.  frames: Bitmaps to decode into (their strides are
    honoured); fill: a byte the new frames are filled with first."""
    L = _bind()
    return decode_batch(L.ifhip_webp_info, L.ifhip_webp_decode_batch_device, WebpFileInfo, lambda info: bool(info.lossless), lambda info: bool(info.has_alpha),
                        files, device, frames, fill)


def decode_webp(data, device="cuda:0"):
    """WebPDecoder::read_frame: one file -> a Bitmap (alpha_meaningful = has_alpha).  A damaged stream raises ImageMalformed-style."""
    frames, status = decode_webp_batch([data], device)
    if status[0]:
        raise FlowError(ErrorKind.InvalidArgument, f"ImageMalformed: libwebp decoding error: {STATUS.get(status[0], status[0])}")
    return frames[0]


def decode_webp_host(data, stride=None, out=None):
    """Host-buffer drop-in (numpy): the file -> BGRA rows [h, stride] uint8."""
    L = _bind()
    return decode_host(L.ifhip_webp_info, L.ifhip_webp_decode, WebpFileInfo, data, stride, out)
