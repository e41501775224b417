"""Host mirror of WebPDecoder (imageflow_core/src/codecs/webp.rs:162-248) on the device lossy WebP decoder of
libimageflow_hip.so (csrc/vp8_read.cpp, csrc/vp8_decode.hip): still lossy WebP files (`VP8 `, with or without `ALPH`) -> 8-bit
BGRA frames in HBM -- bool-decoding on the host, dequantisation, inverse transforms, intra prediction, loop filter, alpha plane
and conversion on the GPU.  For tests and tools; the job path is `decode` with a WebP io_id once
Context.set_webp_lossy_decoder(True) is told (csrc/shim_decode.cpp)."""
import ctypes as C

from .. import _native
from ..errors import ErrorKind, FlowError
from ._file_decoder import decode_batch, decode_host
from .webp_decoder import WebpFileInfo, webp_info  # noqa: F401  (the container's facts are the lossless reader's call)

# include/imageflow_hip.h IFHIP_VP8_DEC_*
STATUS = {0: "ok", 1: "container", 2: "not_lossy", 3: "frame_header", 4: "partitions", 5: "end_of_modes", 6: "end_of_tokens",
          7: "alpha_header", 8: "alpha_stream"}


def _bind():
    L = _native.lib()
    if getattr(L, "_webp_lossy_dec_bound", False):
        return L
    L.ifhip_webp_info.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(WebpFileInfo)]
    L.ifhip_webp_lossy_decode_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ifhip_webp_lossy_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_size_t, C.POINTER(C.c_uint32)]
    L._webp_lossy_dec_bound = True
    return L


def decode_webp_lossy_batch(files, device="cuda:0", frames=None, fill=None):
    """files: n still lossy WebP files (bytes) of any size, decoded in one batch.  Returns (frames, status): frames[i] a Bitmap
    of one frame (None where the container did not parse, or the file is lossless or animated), status[i] the file's status
    word.  frames: Bitmaps to decode into (their strides are honoured); fill: a byte the new frames are filled with first."""
    L = _bind()
    return decode_batch(L.ifhip_webp_info, L.ifhip_webp_lossy_decode_batch_device, WebpFileInfo, lambda info: not info.lossless and not info.animated,
                        lambda info: bool(info.has_alpha), files, device, frames, fill)


def decode_webp_lossy(data, device="cuda:0"):
    """WebPDecoder::read_frame: one file -> a Bitmap (alpha_meaningful = has_alpha).  A damaged stream raises ImageMalformed-style."""
    frames, status = decode_webp_lossy_batch([data], device)
    if status[0]:
        raise FlowError(ErrorKind.InvalidArgument, f"ImageMalformed: libwebp decoding error: {STATUS.get(status[0], status[0])}")
    return frames[0]


def decode_webp_lossy_host(data, stride=None, out=None):
    """Host-buffer drop-in (numpy): the file -> BGRA rows [h, stride] uint8."""
    L = _bind()
    return decode_host(L.ifhip_webp_info, L.ifhip_webp_lossy_decode, WebpFileInfo, data, stride, out)
