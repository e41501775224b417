"""Host mirror of GifDecoder (imageflow_core/src/codecs/gif/mod.rs:21-309) on the device GIF decoder of libimageflow_hip.so
(csrc/gif_read.cpp, csrc/gif_decode.hip): GIF files -> the logical screen after the selected frame as 8-bit BGRA in HBM --
segment-parallel LZW and the frame replay (dispose, blit) on the GPU.  For tests and tools; the job path is `decode` with a
GIF io_id and the decoder command {"select_frame": N} (csrc/shim_decode.cpp)."""
import ctypes as C

import numpy as np

from .. import _native
from ..errors import ErrorKind, FlowError
from ._file_decoder import decode_batch, decode_frames, decode_host

# include/imageflow_hip.h IFHIP_GIF_DEC_*
STATUS = {0: "ok", 1: "too_little", 2: "bad_code", 3: "container", 4: "min_code_size", 5: "no_palette", 6: "frame_too_large", 7: "no_such_frame"}


class GifFileInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "has_global_palette", "background_index")]


def _bind():
    L = _native.lib()
    if getattr(L, "_gif_dec_bound", False):
        return L
    L.ifhip_gif_info.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(GifFileInfo)]
    L.ifhip_gif_decode_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ifhip_gif_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_size_t, C.POINTER(C.c_uint32)]
    L.ifhip_gif_frame_count.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_uint32]
    L.ifhip_gif_decode_frames_device.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
    L._gif_dec_bound = True
    return L


def gif_info(data):
    """GifDecoder::create + get_unscaled_image_info (mod.rs:45-101,181-194): the header's facts; no frame has been read.  Host only."""
    L = _bind()
    buf = np.frombuffer(bytes(data), np.uint8)
    info = GifFileInfo()
    _native.check(L.ifhip_gif_info(buf.ctypes.data, buf.size, C.byref(info)))
    out = {n: int(getattr(info, n)) for n, _ in GifFileInfo._fields_}
    out["has_global_palette"] = bool(out["has_global_palette"])
    out.update(preferred_mime_type="image/gif", preferred_extension="gif", image_width=out["width"], image_height=out["height"],
               frame_decodes_into="bgra_32", lossless=False, multiple_frames=False)
    return out


def decode_gif_batch(files, frame_index=None, device="cuda:0", frames=None, fill=None):
    """files: n GIF files (bytes) of any size, decoded and composed in one batch of five launches.  frame_index: the frame of
    each file to hand on (None: frame 0 of each).  Returns (frames, status): frames[i] a Bitmap of the logical screen (None
    where the header did not parse or describes no pixels), status[i] the file's status word.  frames: Bitmaps to decode into
    (their strides are honoured); fill: a byte the new frames are filled with first."""
    L = _bind()
    want = (C.c_uint32 * len(files))(*[int(v) for v in frame_index]) if frame_index is not None else None
    return decode_batch(L.ifhip_gif_info, L.ifhip_gif_decode_batch_device, GifFileInfo, lambda info: bool(info.width and info.height), lambda info: True,
                        files, device, frames, fill, lead=(want,))


def decode_gif(data, frame_index=0, device="cuda:0"):
    """GifDecoder::read_frame with SelectFrame(frame_index): one file -> a Bitmap.  A damaged file raises."""
    frames, status = decode_gif_batch([data], [frame_index], device)
    if status[0]:
        raise FlowError(ErrorKind.InvalidArgument, f"ImageMalformed: GIF decoding error: {STATUS.get(status[0], status[0])}")
    return frames[0]


def gif_frame_count(data):
    """GifDecoder::has_more_frames until it says no: (frames, delays in hundredths of a second, user-input flags).  Host only;
    a file the walk refuses raises."""
    L = _bind()
    buf = np.frombuffer(bytes(data), np.uint8)
    n = C.c_uint32(0)
    _native.check(L.ifhip_gif_frame_count(buf.ctypes.data, buf.size, C.byref(n), None, None, 0))
    delays, flags = (C.c_uint32 * max(n.value, 1))(), (C.c_uint32 * max(n.value, 1))()
    _native.check(L.ifhip_gif_frame_count(buf.ctypes.data, buf.size, C.byref(n), delays, flags, n.value))
    return n.value, list(delays)[:n.value], [bool(f) for f in list(flags)[:n.value]]


def decode_gif_frames(data, device="cuda:0", stride=None, fill=None, with_status=False):
    """Every composed screen of one file in one pass (ifhip_gif_decode_frames_device): -> (screens, delays): screens a Bitmap
    whose frame k is the logical screen behind frame k's blit -- what decode_gif(data, k) gives --, delays in hundredths of a
    second.  A damaged frame anywhere raises (with_status: -> (screens, delays, status word) instead, the block untouched)."""
    L = _bind()
    screens, status, delays, _ = decode_frames(L.ifhip_gif_info, L.ifhip_gif_frame_count, L.ifhip_gif_decode_frames_device, GifFileInfo, data, device, stride, fill)
    if with_status:
        return screens, delays, status
    if status:
        raise FlowError(ErrorKind.InvalidArgument, f"ImageMalformed: GIF decoding error: {STATUS.get(status, status)}")
    return screens, delays


def decode_gif_host(data, frame_index=0, stride=None, out=None):
    """Host-buffer drop-in (numpy): the file -> BGRA rows [h, stride] uint8."""
    L = _bind()
    return decode_host(L.ifhip_gif_info, L.ifhip_gif_decode, GifFileInfo, data, stride, out, lead=(frame_index,))
